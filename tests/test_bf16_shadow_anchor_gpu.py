"""The bf16 shadow registry (csrc/api.hip, csrc/common.h) against entries that outlived their tensors.  A bf16 recurrence registers bf16
copies of h and da by address; a host that hands those addresses to a tensor library afterwards leaves the entries live over memory that now
holds something else.  vd_gemm_tn_acc(flags = VD_FLAG_BF16) takes shadows only for the contraction the producers leave behind -- A from the
registered base of h, B up to the registered end of da -- so fp32 operands that merely lie inside two stale ranges are contracted from
their own rows.  Without the anchors the contractions below multiply the recurrence's old bf16 bytes (relative error of order 1).

Bound: both operands rounded to bf16, fp32 accumulation, against the fp32 operands' fp64 product: the bf16 pass's error, a few 1e-3
(tests/test_ops_gpu.py test_bf16_contraction_of_fp32_rows); 1e-2 here, as its producer-shadow test."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T, N, H, V = 3, 4096, 128, 40


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from visdial_amd import ops as o
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# (A offset in rows of M floats, B offset in rows of Nc floats, from the start of the h / gates buffers): A at the registered base with B at
# the start of da's range; A inside h's range with B ending at da's registered end; both inside
@pytest.mark.parametrize("a_off, b_end", [(0, False), (512, True), (512, False)], ids=['A-at-base', 'B-at-end', 'inside'])
def test_operands_inside_stale_shadow_ranges_are_contracted_from_their_own_rows(ops, a_off, b_end):
    rng = np.random.RandomState(3)
    Wh = dev((rng.randn(H, 4 * H) / np.sqrt(H)).astype(np.float32))
    tab = dev(rng.randn(V + 1, 4 * H).astype(np.float32) * 0.5)
    tok = dev(rng.randint(0, V + 1, size=(T, N)).astype(np.int32))
    dh_last = dev(rng.randn(N, H).astype(np.float32))
    hbuf = torch.empty(T * N * H, device="cuda")
    gbuf = torch.empty(T * N * 4 * H, device="cuda")
    c, dc = torch.empty(T, N, H, device="cuda"), torch.empty(N, H, device="cuda")
    ops.lstm_forward(tab, Wh, gbuf.view(T, N, 4 * H), hbuf.view(T, N, H), c, T, N, H, 0, 4 * H, tok_gather=tok, flags=ops.FLAG_BF16)
    ops.lstm_backward(Wh, gbuf.view(T, N, 4 * H), c, dc, T, N, H, dh_last=dh_last, flags=ops.FLAG_BF16)   # both ranges registered
    torch.cuda.synchronize()
    # the tensor library writes other data over the two ranges: the registry does not see it
    g = torch.Generator(device='cuda').manual_seed(11)
    hbuf.copy_(torch.tanh(torch.randn(hbuf.numel(), device='cuda', generator=g)))
    gbuf.copy_(torch.randn(gbuf.numel(), device='cuda', generator=g) * 0.01)
    M, Nc, K = 256, 512, 2048
    a = hbuf[a_off * M: (a_off + K) * M].view(K, M)
    b0 = gbuf.numel() - K * Nc if b_end else 1024 * Nc
    b = gbuf[b0: b0 + K * Nc].view(K, Nc)
    c0 = torch.randn(M, Nc, device='cuda', generator=g) * 0.1
    out = c0.clone()
    ops.gemm_tn_acc(a, b, out, M=M, N=Nc, K=K, flags=ops.FLAG_BF16)
    torch.cuda.synchronize()
    ref = c0.double() + a.double().t() @ b.double()
    err = float((out.double() - ref).norm() / ref.norm())
    print('A at row %d, B %s: rel-L2 against the fp32 operands\' fp64 product %.3g' % (a_off, 'at the end' if b_end else 'inside', err))
    assert err < 1e-2, err
