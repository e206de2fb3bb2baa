"""The pin of tests/attention_ref.py, on the CPU: every hand-written backward of the helper (and vo.mn_attention_backward) against
torch.autograd in float64 on the same forward written in torch -- max-abs difference relative to the tensor's max-abs <= 1e-10 -- and the
comparison routine of the GPU tests against a perturbed reference, a written guard row and the clean case."""
import numpy as np
import pytest
import torch

import attention_ref as ar
from oracle import visdial_oracle as vo

TOL = 1e-10


def maxrel(got, ref):
    got, ref = ar.to_np(got), ar.to_np(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def leaf(a):
    return torch.tensor(np.asarray(a, np.float64), requires_grad=True)


# (B, R, S2, H, Kc): B != R; one case per dropout setting
@pytest.mark.parametrize("use_drop", [False, True])
@pytest.mark.parametrize("B,R,S2,H,Kc", [(2, 3, 7, 12, 8), (3, 1, 5, 4, 4)])
def test_image_attention_backward_is_autograd(B, R, S2, H, Kc, use_drop):
    rng = np.random.RandomState(B * 100 + R * 10 + S2 + use_drop)
    N = B * R
    pre = np.tanh(rng.randn(B * S2, H))
    m1 = (rng.rand(N * S2, H) > 0.5).astype(np.uint8) if use_drop else None
    m2 = (rng.rand(N * S2, Kc) > 0.5).astype(np.uint8) if use_drop else None
    Wc, bc = rng.randn(Kc, H) * 0.3, rng.randn(Kc) * 0.1
    qc, wa, ba, u0 = rng.randn(N, Kc) * 0.5, rng.randn(Kc) * 0.3, rng.randn(1), rng.randn(N, H)
    datt = rng.randn(N, H)
    sc = 2.0 if use_drop else 1.0
    fwd = ar.img_forward(pre, m1, m2, Wc, bc, qc, wa, ba, u0, B, R, S2, sc)
    bwd = ar.img_backward(fwd, datt, m1, m2, Wc, wa, B, R, S2, sc)

    tpre, tWc, tqc, twa, tba = leaf(pre), leaf(Wc), leaf(qc), leaf(wa), leaf(ba)
    idx = torch.arange(N).div(R, rounding_mode='floor')[:, None] * S2 + torch.arange(S2)[None, :]        # the gather by n // R
    x = tpre[idx.reshape(-1)]
    if use_drop:
        x = x * torch.tensor(m1, dtype=torch.float64) * sc
    z = x @ tWc.T + torch.tensor(bc) + tqc.repeat_interleave(S2, 0)
    z.retain_grad()
    y = torch.tanh(z)
    if use_drop:
        y = y * torch.tensor(m2, dtype=torch.float64) * sc
    score = (y @ twa + tba[0]).reshape(N, S2)
    p = torch.softmax(score, 1)
    u1 = torch.einsum('ns,nsh->nh', p, x.reshape(N, S2, H)) + torch.tensor(u0)
    assert maxrel(fwd['img_tr'], x) <= TOL and maxrel(fwd['iqc'], y) <= TOL and maxrel(fwd['p'], p) <= TOL and maxrel(fwd['u1'], u1) <= TOL
    (u1 * torch.tensor(datt)).sum().backward()
    assert maxrel(bwd['dz'], z.grad) <= TOL
    assert maxrel(bwd['dwa'], twa.grad) <= TOL
    assert maxrel(bwd['dqc'], tqc.grad) <= TOL
    assert maxrel(bwd['dpre'], tpre.grad) <= TOL
    assert maxrel(bwd['dWc'], tWc.grad) <= TOL
    # dba cancels to zero in exact arithmetic (a softmax ignores a shift): held to the sum of the magnitudes it is made of
    assert abs(bwd['dba'] - float(tba.grad[0])) <= TOL * np.abs(bwd['dscore']).sum()
    assert abs(bwd['dba']) <= 1e-12 * np.abs(bwd['dscore']).sum()


@pytest.mark.parametrize("B,R,H", [(1, 1, 4), (3, 10, 36), (2, 16, 8)])
def test_hrea_attention_backward_is_autograd(B, R, H):
    rng = np.random.RandomState(B + R + H)
    sq, sh, h, datt = rng.randn(B, R), rng.randn(B, R), rng.randn(B, R, H), rng.randn(B, R, H)
    if R > 1:
        sh[0, 1] = -sq[0, R - 1]                                       # an exact zero on a visible pair -> ReplaceZero(-inf)
    P, att = ar.hrea_forward(sq, sh, h)
    if R > 1:
        assert P[0, R - 1, 1] == 0.0
    assert np.all(P[:, 0, 0] == 1.0) and np.isfinite(att).all()
    dsq, dsh, dh, dA = ar.hrea_backward(P, h, datt)
    tsq, tsh, th = leaf(sq), leaf(sh), leaf(h)
    A = tsq[:, :, None] + tsh[:, None, :]
    A = torch.where(torch.triu(torch.ones(R, R, dtype=torch.bool), 1)[None], torch.zeros((), dtype=torch.float64), A)
    A = torch.where(A == 0, torch.full((), -np.inf, dtype=torch.float64), A)
    tP = torch.softmax(A, -1)
    tatt = torch.einsum('bij,bjk->bik', tP, th)
    assert maxrel(P, tP) <= TOL and maxrel(att, tatt) <= TOL
    (tatt * torch.tensor(datt)).sum().backward()
    assert maxrel(dh, th.grad) <= TOL
    if R > 1:
        assert dA[0, R - 1, 1] == 0.0                                  # nothing flows through the replaced score
        assert maxrel(dsh, tsh.grad) <= TOL
    else:                                                              # (a softmax over one score has no gradient at all)
        assert np.abs(dsh).max() == 0.0 and float(tsh.grad.abs().max()) == 0.0
    # dsq[i] is the sum of row i of dA, zero in exact arithmetic (sq[i] shifts the whole softmax row): against the magnitudes it sums
    scale = np.abs(dA).sum(2)
    assert np.all(np.abs(dsq - tsq.grad.numpy()) <= TOL * scale) and np.all(np.abs(dsq) <= 1e-12 * scale)


@pytest.mark.parametrize("N,H", [(1, 4), (5, 36)])
def test_rowdot_backward_is_autograd(N, H):
    rng = np.random.RandomState(N + H)
    x, w, b, dout = rng.randn(N, H), rng.randn(H), rng.randn(1), rng.randn(N)
    tx, tw, tb = leaf(x), leaf(w), leaf(b)
    out = tx @ tw + tb[0]
    assert maxrel(ar.rowdot_forward(x, w, b), out) <= TOL
    (out * torch.tensor(dout)).sum().backward()
    dw, db, dx = ar.rowdot_backward(x, w, dout)
    assert maxrel(dw, tw.grad) <= TOL and maxrel(dx, tx.grad) <= TOL and abs(db - float(tb.grad[0])) <= TOL * np.abs(dout).max()


@pytest.mark.parametrize("B,R,H", [(1, 1, 4), (3, 10, 36)])
def test_mn_attention_backward_is_autograd_under_a_non_causal_mask(B, R, H):
    rng = np.random.RandomState(B + R + H + 1)
    q, h, dhatt = rng.randn(B, R, H) * 0.3, rng.randn(B, R, H) * 0.3, rng.randn(B, R, H)
    mask = (rng.rand(B, R, R) < 0.4).astype(np.uint8)
    mask[np.arange(B)[:, None], np.arange(R)[None, :], rng.randint(0, R, size=(B, R))] = 0         # every row keeps a visible fact
    assert R == 1 or not np.array_equal(mask, vo.causal_mask(B, R))
    p, hatt = vo.mn_attention_forward(q, h, mask)
    assert np.all(p[mask != 0] == 0.0)
    dq, dh = vo.mn_attention_backward(q, h, p, dhatt)
    tq, th = leaf(q), leaf(h)
    s = torch.einsum('bik,bjk->bij', tq, th)
    s = torch.where(torch.tensor(mask != 0), torch.full((), -9999999.0, dtype=torch.float64), s)
    tp = torch.softmax(s, -1)
    thatt = torch.einsum('bij,bjk->bik', tp, th)
    assert maxrel(p, tp) <= TOL and maxrel(hatt, thatt) <= TOL
    (thatt * torch.tensor(dhatt)).sum().backward()
    assert maxrel(dh, th.grad) <= TOL
    if R > 1:
        assert maxrel(dq, tq.grad) <= TOL
    else:
        assert np.abs(dq).max() <= 1e-25 and float(tq.grad.abs().max()) <= 1e-25


# ------------------------------------------------------------------------------------------------------------ the comparison routine
def _case():
    rng = np.random.RandomState(0)
    rows, cols = 294, 144                                              # ragged in both directions: 38 rows, 16 columns in the last tiles
    ref = rng.randn(rows, cols)
    out = ar.Guarded((rows, cols), device='cpu', init=ref)
    return rows, cols, ref, out


def _run(ref, out, rows, cols):
    rep = ar.Report('case', log=lambda s: None)
    rep.close('x', out, ref, 1e-5, ar.tile_slices(rows, cols) + [ar.row_block('round N - 1', 5, 49)])
    rep.guard('x', out)
    return rep


def test_compare_passes_the_clean_case():
    rows, cols, ref, out = _case()
    rep = _run(ref, out, rows, cols)
    rep.ok()
    assert set(k[1] for k in rep.errors) == {'whole', 'last row tile', 'last column tile', 'round N - 1'}
    assert max(rep.errors.values()) < 1e-7                             # the fp32 rounding of the stored copy


def test_compare_reports_one_perturbed_element_of_the_last_ragged_tile():
    """a relative 1e-3 in ONE element (of 1.5 x the rms) of the 38 x 16 corner: 1.5e-3 / sqrt(294 * 144) = 7e-6 of the whole tensor's norm
    -- the whole-tensor figure alone would pass it -- and 2e-5 of either ragged tile's"""
    rows, cols, ref, out = _case()
    corner = np.abs(ref[256:, 128:])
    i, j = np.unravel_index(np.abs(corner - 1.5).argmin(), corner.shape)
    bad = ref.copy()
    bad[256 + i, 128 + j] *= 1 + 1e-3
    rep = _run(bad, out, rows, cols)
    assert rep.errors[('x', 'whole')] < 1e-5
    assert len(rep.failures) == 3 and 'last row tile' in rep.failures[0] and 'last column tile' in rep.failures[1]      # + the last round's rows
    with pytest.raises(AssertionError, match='last row tile'):
        rep.ok()


def test_compare_reports_a_written_guard_row():
    rows, cols, ref, out = _case()
    out.buf[rows * cols + 3 * cols + 5] = 0.0                          # guard row 3
    rep = _run(ref, out, rows, cols)
    assert len(rep.failures) == 1 and 'guard rows written' in rep.failures[0] and 'row 3' in rep.failures[0]
    with pytest.raises(AssertionError, match='guard'):
        rep.ok()


def test_compare_reports_an_unwritten_output_a_nan_and_a_bit_difference():
    rows, cols, ref, _ = _case()
    out = ar.Guarded((rows, cols), device='cpu')                       # never written: SENTINEL everywhere
    assert len(_run(ref, out, rows, cols).failures) == 4
    out = ar.Guarded((rows, cols), device='cpu', init=ref)
    out.t[0, 0] = float('nan')
    assert any('whole' in f for f in _run(ref, out, rows, cols).failures)
    rep = ar.Report(log=lambda s: None)
    rep.exact('x', np.float32([1.0, 2.0]), np.float32([1.0, np.nextafter(np.float32(2.0), np.float32(3.0))]))
    assert len(rep.failures) == 1
    rep = ar.Report(log=lambda s: None)
    rep.scalar('dba', 1.0 + 2e-5, 1.0, 1e-5)
    rep.scalar('dba', 1.0 + 5e-6, 1.0, 1e-5)
    assert len(rep.failures) == 1
