"""tests/lstm2_cases.py proves itself without a GPU: the checker passes the float32 emulation of a correct call on every case and fails every
mutant on the case that names it; the fp64 reference equals a torch float64 restatement with autograd gradients; the table's counts and
tokens keep the contract of include/visdial_hip.h."""
import warnings

import numpy as np
import pytest
import torch

import lstm2_cases as lc

IDS = [c.id for c in lc.CASES]


def test_table_holds_the_required_cases():
    want = {'one-row': (32, [(1, 1, None)]), 'short-ragged': (32, [(2, 33, None)]), 'odd-H-mixed': (96, [(3, 40, None), (1, 70, None)]),
            'live-two': (64, [(7, 70, [0, 0, 5, 32, 33, 64, 70]), (4, 70, [1, 1, 70, 70])]), 'never-live': (128, [(3, 130, [0, 31, 97])]),
            'wide': (512, [(2, 40, [8, 40])]), 'mixed-nact': (64, [(3, 64, [10, 40, 64]), (5, 33, None)])}
    for sid, (H, stacks) in want.items():
        assert lc.SHAPES[sid][1:] == (H, stacks), sid
        assert {'%s-fp32' % sid, '%s-bf16' % sid} <= set(IDS)
    ns = {N for _, _, st in lc.SHAPES.values() for _, N, _ in st}
    assert {1, 33} <= ns and any(N % 32 == 0 for N in ns)


@pytest.mark.parametrize('sid', list(lc.SHAPES))
def test_counts_and_tokens_keep_the_contract(sid):
    for s in lc.operands(sid):
        T, N, tok = s.T, s.N, s.tok
        assert tok.shape == (T, N) and tok.min() >= 0 and tok.max() <= lc.V
        assert (tok[T - 1] == 0).any() or N == 1, 'a row that ends in a zero token'
        if s.nact is None:
            ln = (tok != 0).sum(0)                               # right-aligned, no zero inside a row
            assert all((tok[T - ln[n]:, n] != 0).all() and (tok[:T - ln[n], n] == 0).all() for n in range(N))
            assert ln.max() == T
            continue
        na = s.nact
        assert na.dtype == np.int32 and na.shape == (T,)
        assert (na >= 0).all() and (na <= N).all() and (np.diff(na) >= 0).all()
        for t in range(T):
            assert (tok[t, na[t]:] == 0).all(), 'a dead row holds a token'
            first = slice(na[t - 1] if t else 0, na[t])              # rows whose span starts here: the claim is tight
            assert (tok[t, first] != 0).all()
        ln = lc.lengths_of(T, N, na)
        assert (np.diff(ln) <= 0).all(), 'rows in order of descending length'
        span = np.arange(T)[:, None] >= (T - ln)[None, :]
        assert ((tok == 0) & span).any(), 'zeros inside the live span'
        assert ((tok[T - 1] == 0) & (ln > 0)).any(), 'a live row that ends in a zero token'
        # the caller's contract on the buffers
        for name in lc.FWD_OUT:
            a = lc.view(s, name, s.fwd0[name])
            for t in range(T):
                assert not a[t, na[t]:s.never].any() and np.isnan(a[t, s.never:]).all() and np.isfinite(a[t, :na[t]]).all()
        for name, flat in list(s.fwd0.items()) + list(s.bwd0.items()):
            assert (flat[-lc.GUARD:] == lc.MARK).all()
            a = lc.view(s, name, flat)
            assert np.isnan(a[:, s.never:]).all() and np.isfinite(a[:, :s.never]).all()


@pytest.mark.parametrize('cid', IDS)
def test_checker_passes_the_correct_emulation(cid):
    c = lc.case(cid)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for direction in ('fwd', 'bwd'):
            rep = lc.assert_ok(c, direction, lc.emulate(c, direction))
            # a float32 evaluation of the recurrences stays at or below 3.5e-7 on every slice, whatever the case's bound
            assert max(w[1] for w in rep.worst.values()) <= 3.5e-7


def test_mutant_table_covers_the_listed_mistakes():
    assert {'ragged_last_row', 'round_up_rows', 'stale_mask', 'no_b2', 'dc_first_ignored', 'dc_first_always', 'k0_reads_h0', 'dh1_from_next',
            'wh2_of_stack0', 'h_pow2_colmap', 'guard_overwrite'} <= set(lc.MUTANTS)


@pytest.mark.parametrize('mutant', list(lc.MUTANTS))
def test_checker_fails_every_mutant_on_its_case(mutant):
    c = lc.case(lc.MUTANTS[mutant])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        reps = [lc.check(c, direction, lc.emulate(c, direction, mutant)) for direction in ('fwd', 'bwd')]
    assert not all(r.ok for r in reps), 'no check of %s notices %s' % (c.id, mutant)


def test_h_pow2_colmap_is_visible_only_at_h_96():
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for c in lc.CASES:
            if c.arith == 'fp32' and c.H & (c.H - 1) == 0:
                assert lc.check(c, 'fwd', lc.emulate(c, 'fwd', 'h_pow2_colmap')).ok


def test_checker_notices_single_faults():
    """one wrong element in the last live row of one step; a dead row written; a NaN in a live row"""
    c = lc.case('live-two-fp32')
    s = lc.operands(c.shape)[0]
    for name, t, row, val in (('h2', 4, 32, None), ('c1', 3, 40, 1e-3), ('gates2', 6, 3, np.nan)):
        got = lc.emulate(c, 'fwd')
        a = lc.view(s, name, got[0][name])
        a[t, row, 5] = a[t, row, 5] * np.float32(1.01) + np.float32(1e-3) if val is None else val
        rep = lc.check(c, 'fwd', got)
        assert not rep.ok and any(name in f for f in rep.failures), (name, rep.failures)
    # the whole-tensor rel-L2 alone would let the first one pass: 1 % on one row of 33 live ones among 7 steps
    got = lc.emulate(c, 'fwd')
    a = lc.view(s, 'h2', got[0]['h2'])
    a[4, 32] *= np.float32(1 + 2e-5)
    rep = lc.check(c, 'fwd', got)
    assert [f for f in rep.failures if 'h2' in f] and not any('whole' in f for f in rep.failures)


def torch_two_layer(s):
    """two masked LSTM layers in torch float64; gradients by autograd.  Layer 2 reads a detached copy of h1, so that dL/dh1 through layer 2's
    input alone (dh1_seq) is a leaf gradient; layer 1 is then driven by it"""
    dd = torch.float64
    T, N, H = s.T, s.N, s.H
    tt = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    keep = tt(s.tok != 0)[:, :, None]

    def layer(x, W, b):
        Dx = x.shape[-1]
        c0 = torch.zeros(N, H, dtype=dd, requires_grad=True)
        h, c, pre, hs, cs, gs = torch.zeros(N, H, dtype=dd), c0, [], [], [], []
        for t in range(T):
            e = torch.zeros(N, 4 * H, dtype=dd, requires_grad=True)           # da[t] = the gradient of a zero added to the pre-activation
            a = b + x[t] @ W[:Dx] + h @ W[Dx:] + e
            i, f, o, g = torch.sigmoid(a[:, :H]), torch.sigmoid(a[:, H:2 * H]), torch.sigmoid(a[:, 2 * H:3 * H]), torch.tanh(a[:, 3 * H:])
            c = (f * c + i * g) * keep[t]
            h = o * torch.tanh(c) * keep[t]
            pre.append(e); hs.append(h); cs.append(c); gs.append(torch.cat([i, f, o, g], 1) * keep[t])
        return c0, pre, torch.stack(hs), torch.stack(cs), torch.stack(gs)

    c01, pre1, h1, c1, g1 = layer(tt(s.x), tt(s.W1), tt(s.b1))
    h1_in = h1.detach().requires_grad_()
    c02, pre2, h2, c2, g2 = layer(h1_in, tt(s.W2), tt(s.b2))
    (h2[T - 1] * tt(s.dlast)).sum().backward()
    h1.backward(h1_in.grad)
    fwd = dict(gates1=g1, h1=h1, c1=c1, gates2=g2, h2=h2, c2=c2)
    bwd = dict(gates1=torch.stack([a.grad for a in pre1]), gates2=torch.stack([a.grad for a in pre2]), dh1_seq=h1_in.grad, dc1=c01.grad, dc2=c02.grad)
    return {k: v.detach().numpy() for k, v in fwd.items()}, {k: v.numpy() for k, v in bwd.items()}


@pytest.mark.parametrize('sid,si', [('odd-H-mixed', 0), ('mixed-nact', 0)])
def test_reference_equals_torch_autograd(sid, si):
    """pins the composition of the two oracle calls and the dh1_seq, dc1, dc2 references.  The backward reference starts from the forward
    state rounded to fp32 (2^-24 relative), torch from its own fp64 state: 1e-6.  With counts (mixed-nact), dc of a row that is pad before
    step t0 is dL/dc0 of its own sequence, which autograd cannot see behind the mask: those rows are compared through a second torch run on
    a stack cut to the steps from t0 on."""
    s = lc.operands(sid)[si]
    fwd, bwd = torch_two_layer(s)
    for k in lc.FWD_OUT:
        assert lc.rel_l2(fwd[k], s.ref_fwd[k]) < 1e-12, k
    for k in ('gates1', 'gates2', 'dh1_seq'):
        assert lc.rel_l2(bwd[k], s.ref_bwd[k]) < 1e-6, k
    t0s = s.T - (lc.lengths_of(s.T, s.N, s.nact) if s.nact is not None else np.full(s.N, s.T))
    at0 = t0s == 0
    assert at0.any()
    for k in ('dc1', 'dc2'):
        assert lc.rel_l2(bwd[k][at0], s.ref_bwd[k][at0]) < 1e-6, k
    for t0 in sorted(set(t0s[:s.never]) - {0}):
        q = t0s == t0
        cut = lc.Stack()
        cut.T, cut.N, cut.H = s.T - t0, int(q.sum()), s.H
        cut.tok, cut.x, cut.dlast, cut.W1, cut.b1, cut.W2, cut.b2 = s.tok[t0:, q], s.x[t0:, q], s.dlast[q], s.W1, s.b1, s.W2, s.b2
        _, b2 = torch_two_layer(cut)
        for k in ('dc1', 'dc2'):
            assert np.abs(s.ref_bwd[k][q]).max() > 0
            assert lc.rel_l2(b2[k], s.ref_bwd[k][q]) < 1e-6, (k, t0)
