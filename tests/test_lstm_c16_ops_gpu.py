"""Operator parity of the compact-bf16 recurrence (csrc/lstm.hip vd_lstm_forward_c16 / vd_lstm_backward_c16: the option recurrence of a
bf16 pass) beside tests/test_ops_gpu.py::test_bf16_compact_state_saturated_gates, which keeps the saturated gates: moderate pre-activations
here, and what that test leaves out -- h16 compared, a ragged 128-row tile (N = 2088), T = 1 (only the K = 0 launches, h_last from step 0)
and H = 256.  Against the fp64 recurrence on the bf16-rounded table rows and weights (Wx = I, b = 0) within the config's bounds, 1e-2
forward and 2e-2 backward, on the whole tensor and on the last row tile alone (rows 2048..2087 where N = 2088); guards unchanged."""
import numpy as np
import pytest
import torch

from oracle import visdial_oracle as vo

pytestmark = pytest.mark.gpu

TILE = 128                       # rows per tile of CfgF9 / CfgB11 and their bf16 twins
GUARD = 64
V = 50
CASES = [(1, 2088, 128), (3, 2088, 128), (2, 2048, 256)]


@pytest.fixture(scope="module")
def entries():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from visdial_amd import _lib
    return _lib.internal('vd_lstm_forward_c16'), _lib.internal('vd_lstm_backward_c16')


def guarded(n, dtype):
    """a flat device buffer of n elements (NaN) in front of GUARD marked ones"""
    b = torch.full((n + GUARD,), float('nan'), device='cuda', dtype=dtype)
    b[n:] = -7168.0              # exact in bf16
    return b


def rel_l2(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


@pytest.mark.parametrize('T,N,H', CASES)
def test_c16_parity(entries, T, N, H):
    fwd, bwd = entries
    rng = np.random.RandomState(T + N + H)
    f32 = lambda *s: rng.randn(*s).astype(np.float32)
    Wh = (f32(H, 4 * H) / np.sqrt(H) * 0.5).astype(np.float32)
    tab = f32(V + 1, 4 * H) * np.float32(0.5)
    tok = rng.randint(1, V + 1, size=(T, N)).astype(np.int32)
    dh_last = f32(N, H)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    tab16, Wh16 = dev(tab).to(torch.bfloat16), dev(Wh).to(torch.bfloat16)
    Whd, tokd, dhd = dev(Wh), dev(tok), dev(dh_last)
    bf, fl = torch.bfloat16, torch.float32
    gates16, h16 = guarded(T * N * 4 * H, bf), guarded(T * N * H, bf)
    h_last, c, dc = guarded(N * H, fl), guarded(T * N * H, fl), guarded(N * H, fl)
    guards = lambda: [b[-GUARD:].clone() for b in (gates16, h16, h_last, c, dc)]
    g0 = guards()
    stream = torch.cuda.current_stream().cuda_stream
    fwd(tab16.data_ptr(), 4 * H, tokd.data_ptr(), Whd.data_ptr(), gates16.data_ptr(), h16.data_ptr(), h_last.data_ptr(), c.data_ptr(), T, N, H, stream)
    torch.cuda.synchronize()
    host = lambda b, *shape: b[:-GUARD].float().cpu().numpy().reshape(shape)
    got = dict(h16=host(h16, T, N, H), c=host(c, T, N, H), h_last=host(h_last, 1, N, H))
    assert all(torch.equal(a, b) for a, b in zip(g0, guards())), 'forward wrote behind a buffer'
    assert torch.isnan(dc[:-GUARD]).all(), 'forward wrote dc_work'

    # fp64 recurrence on the operands the kernel multiplies: bf16 table rows, bf16 weights (h is rounded to bf16 between steps: inside the bound)
    xw = tab16.float().cpu().numpy().astype(np.float64)[tok]
    W = np.concatenate([np.eye(4 * H), Wh16.float().cpu().numpy().astype(np.float64)], 0)
    h_ref, c_ref, g_ref = vo.lstm_forward(xw, W, np.zeros(4 * H))
    assert np.abs(xw).max() < 4 and (np.abs(g_ref[:, :, :3 * H] - 0.5) < 0.49).mean() > 0.9        # moderate: the gates are not saturated
    ref = dict(h16=h_ref, c=c_ref, h_last=h_ref[-1:])
    last = slice(TILE * ((N - 1) // TILE), N)

    def check(name, a, r, tol):
        e_all, e_tile = rel_l2(a, r), rel_l2(a[:, last], r[:, last])
        print('C16 T=%d N=%d H=%d %-7s whole %.3e last tile (rows %d..%d) %.3e bound %.0e' % (T, N, H, name, e_all, last.start, N - 1, e_tile, tol))
        assert np.isfinite(a).all(), name
        return [] if e_all < tol and e_tile < tol else ['%s: whole %.3e, last tile %.3e, bound %.0e' % (name, e_all, e_tile, tol)]

    bad = []
    for name in ('h16', 'c', 'h_last'):
        bad += check(name, got[name], ref[name], 1e-2)

    bwd(Whd.data_ptr(), gates16.data_ptr(), c.data_ptr(), dhd.data_ptr(), dc.data_ptr(), T, N, H, stream)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(g0, guards())), 'backward wrote behind a buffer'
    assert np.array_equal(host(c, T, N, H), got['c']) and np.array_equal(host(h16, T, N, H), got['h16']), 'backward wrote its inputs'
    _, _, _, _, dc0_ref, da_ref = vo.lstm_backward(xw, W, g_ref, h_ref, c_ref, dh_last=dh_last.astype(np.float64), return_da=True)
    bad += check('dc_work', host(dc, 1, N, H), dc0_ref[None], 2e-2)
    bad += check('da', host(gates16, T, N, 4 * H), da_ref, 2e-2)
    assert not bad, bad
