"""The exact-split step kernel (csrc/split_core.h gemm_split_kernel) at the edges of what its 16x16x32 form brought in: the 32-k macro
step and its 16-k half step, the register-direct A operand, the 32-row waves of the 128-row workgroup, and the 2 x 2 quad of 16 x 16
accumulators handed to the epilogues as a 32 x 32 tile (gemm_core.h quad_to_tile).

References are fp64 numpy.  Bounds: rel-L2 < 1e-5 (tests/gemm_cases.py REL_L2, what tests/test_attention_ops_gpu.py holds the split image
products to) and the 1e-5 / 2e-5 of tests/test_ops_gpu.py's split9 recurrence.  The one-hot cases are exact: every output element is a
single product of two small integers.

How the kernel is reached.  Only two families of entry points launch it, and both have a row threshold (csrc/paths.h):
  * the image products vd_img_common_forward_p / vd_img_tr_backward_p with VD_FLAG_SPLIT9 from rows >= 128 (vd_img_split_ok); they pass
    dense operands (lda = K), so the poison sits BEHIND the operand: the A tensor ends a NaN-filled buffer, and a read past
    A + M * lda that reaches an accumulator shows up as NaN; the outputs lie in front of guard rows;
  * the option recurrence from rows >= 2048 (VD_THROUGHPUT_ROWS).
Rows below a threshold (1, 31, 33; 1, 129, 200) run too: they take the fall-back of the same entry point and must meet the same bound."""
import functools

import numpy as np
import pytest
import torch

import attention_ref as ar
import gemm_cases as gc
import test_ops_gpu as tog
from test_attention_ops_gpu import internal, ops, ptr, stream  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

D = np.float64
BOUND = gc.REL_L2
WAVE_ROWS, WG_ROWS = 32, 128             # split_core.h SplitCfg: a wave's rows, a workgroup's rows


def behind_nan(a):
    """`a` on the device as the LAST rows of a buffer whose remaining 4096 floats are NaN"""
    a = np.ascontiguousarray(a, np.float32)
    buf = torch.full((a.size + 4096,), float('nan'), device='cuda')
    buf[:a.size] = torch.from_numpy(a.reshape(-1)).cuda()
    return buf, buf[:a.size].view(*a.shape)


@functools.lru_cache(maxsize=None)
def product_case(rows, K, N):
    """operands of one [rows x K] x [K x N] product and what both epilogues make of it, fp64.  Shared: read only."""
    rng = np.random.RandomState(rows * 7919 + K * 131 + N)
    x = np.tanh(rng.randn(rows, K)).astype(np.float32)                       # the A operand: fp32 rows
    W = (rng.randn(N, K) / np.sqrt(K)).astype(np.float32)                    # forward: Wc [Kc x H] = Bt [N x K]
    bc = (rng.randn(N) * 0.1).astype(np.float32)
    qc = (rng.randn(rows, N) * 0.5).astype(np.float32)                       # R = 1, S2 = 1: one query row per image row
    iqc = np.tanh(x.astype(D) @ W.astype(D).T + bc.astype(D) + qc.astype(D))
    return x, W, bc, qc, iqc


# rows: below the threshold (fall-back) | the threshold = one full workgroup | one row, one wave - 1, one wave + 1 into the second workgroup |
# 191, 193, 200 (inside the second workgroup's waves 1 to 3) | three workgroups
ROWS = [1, 31, 33, WG_ROWS, WG_ROWS + 1, WG_ROWS + WAVE_ROWS - 1, WG_ROWS + WAVE_ROWS + 1, 191, 193, 200, 2 * WG_ROWS + 1]
# K: half step only | one full step | full + half | two full + half | the longest (16 steps)
KS = [16, 32, 48, 80, 512]


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("rows", ROWS)
def test_forward_product_rows_and_k_tail(ops, internal, rows, K):
    """vd_img_common_forward_p (EpiImgCommon): iqc = tanh(x W^T + bc + qc) on N = 144 columns (a ragged second column tile)"""
    N = 144
    x, W, bc, qc, ref = product_case(rows, K, N)
    rep = ar.Report('split9 forward rows %d K %d:' % (rows, K))
    xbuf, xd = behind_nan(x)
    Wd, bcd, qcd = tog.dev(W), tog.dev(bc), tog.dev(qc)
    out = ar.Guarded((rows, N))
    # evaluation form: `pre` is the dropped tensor itself, B = rows images of S2 = 1 region, R = 1, no masks, scale 1
    internal.common_forward(ptr(xd), None, ptr(xd), ptr(Wd), ptr(bcd), ptr(qcd), None, ptr(out.t), rows, 1, 1, K, N, 1.0, ops.FLAG_SPLIT9,
                            stream())
    torch.cuda.synchronize()
    e = rep.close('iqc', out, ref, BOUND, ar.tile_slices(rows, N) + [('last wave', (slice((rows - 1) // WAVE_ROWS * WAVE_ROWS, rows),))])
    print('rows %d K %d: rel-L2 %.3e' % (rows, K, e if e is not None else float('nan')))
    rep.guard('iqc', out)
    rep.ok()
    assert bool(torch.isnan(xbuf[x.size:]).all())


@pytest.mark.parametrize("K", [16, 48, 80])
@pytest.mark.parametrize("rows", [128, WG_ROWS + 1, 200])
def test_backward_product_atomic_epilogue(ops, internal, rows, K):
    """vd_img_tr_backward_p (EpiImgTrBwd): dpre += dz Wc + p * datt, R = 1, accumulated onto a non-zero dpre; N = H = 48 (one ragged tile)"""
    H = 48
    rng = np.random.RandomState(rows * 31 + K)
    dz = rng.randn(rows, K).astype(np.float32)
    Wc = (rng.randn(K, H) / np.sqrt(K)).astype(np.float32)
    p = rng.rand(rows).astype(np.float32)
    datt = rng.randn(rows, H).astype(np.float32)
    dpre0 = (rng.randn(rows, H) * 0.5).astype(np.float32)
    ref = dpre0.astype(D) + dz.astype(D) @ Wc.astype(D) + p.astype(D)[:, None] * datt.astype(D)
    rep = ar.Report('split9 tr_backward rows %d K %d:' % (rows, K))
    dzbuf, dzd = behind_nan(dz)
    Wd, pd, dd = tog.dev(Wc), tog.dev(p), tog.dev(datt)
    out = ar.Guarded((rows, H), init=dpre0)
    internal.tr_backward(ptr(dzd), ptr(Wd), ptr(pd), ptr(dd), None, ptr(out.t), rows, 1, 1, H, K, 1.0, ops.FLAG_SPLIT9, stream())
    torch.cuda.synchronize()
    rep.close('dpre', out, ref, BOUND, ar.tile_slices(rows, H))
    rep.guard('dpre', out)
    rep.ok()


@pytest.mark.parametrize("hot", [0, 9, 17, 30, 47])
def test_accumulator_quad_to_rows_one_hot(ops, internal, hot):
    """every row of A is (r + 1) at k = hot, every column of B is (1024 + c) / 1024 at k = hot: out[r, c] = (r + 1) (1024 + c) / 1024, exact
    in fp32 and in the split (integers below 2^24 over a power of two), and different for every (r, c) -- a swapped row, column, 16 x 16
    quad member or wave shows as a wrong VALUE at a known place.  K = 48: `hot` walks both k halves of the full step and the half step."""
    rows, K, H = 2 * WG_ROWS + 7, 48, 272
    dz = np.zeros((rows, K), np.float32)
    dz[:, hot] = np.arange(1, rows + 1, dtype=np.float32)
    Wc = np.zeros((K, H), np.float32)
    Wc[hot, :] = (1024 + np.arange(H, dtype=np.float32)) / np.float32(1024)
    ref = np.outer(np.arange(1, rows + 1, dtype=D), (1024 + np.arange(H, dtype=D)) / 1024)
    assert np.array_equal(ref.astype(np.float32).astype(D), ref)
    out = ar.Guarded((rows, H), init=np.zeros((rows, H), np.float32))
    dzd, Wd = tog.dev(dz), tog.dev(Wc)
    pd, dd = torch.zeros(rows, device='cuda'), torch.zeros(rows, H, device='cuda')
    internal.tr_backward(ptr(dzd), ptr(Wd), ptr(pd), ptr(dd), None, ptr(out.t), rows, 1, 1, H, K, 1.0, ops.FLAG_SPLIT9, stream())
    torch.cuda.synchronize()
    got = out.t.cpu().numpy().astype(D)
    bad = np.argwhere(got != ref)
    assert bad.size == 0, 'hot k %d: %d wrong elements, first (row, col) %s: got %r want %r' % (
        hot, len(bad), tuple(bad[0]), got[tuple(bad[0])], ref[tuple(bad[0])])
    assert not out.written_guard_rows()


# small row counts (below VD_THROUGHPUT_ROWS: the latency-shape kernels answer for the same flag) and rows that reach the split step kernels:
# one row into the seventeenth workgroup, one wave + 1 into it, an exact multiple of 128
LSTM_ROWS = [1, 129, 200, 2049, 2048 + 33, 2176]


@pytest.mark.parametrize("table", [True, False], ids=['table', 'dense'])
@pytest.mark.parametrize("H", [32, 96])
@pytest.mark.parametrize("N", LSTM_ROWS)
def test_lstm_step_forward_backward(ops, N, H, table):
    """K = H forward (32: one full step; 96: three) and 4H backward (128, 384) against the fp64 LSTM, bounds of test_ops_gpu.py"""
    tog._lstm_forward_backward(ops, 3, N, H, False, table, flags=ops.FLAG_SPLIT9)


@pytest.mark.parametrize("N,H", [(2048 + 33, 96), (2049, 32)])
def test_lstm_step_masked(ops, N, H):
    tog._lstm_forward_backward(ops, 3, N, H, True, True, flags=ops.FLAG_SPLIT9)
