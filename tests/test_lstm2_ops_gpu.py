"""Operator parity of the two-layer skewed wavefront (csrc/lstm.hip vd_lstm2_forward[_flags] / vd_lstm2_backward[_flags]) on the cases of
tests/lstm2_cases.py: every output of both directions against fp64 on the whole tensor, on each step's live rows and on each step's last
live row tile; dead rows and guards untouched; live-row counts against no counts bit for bit; the bf16 switch; the argument checks.
fp32 goes through ops.lstm2_forward / lstm2_backward (the C ABI names), bf16 through ops.lstm2_pass(.., FLAG_BF16).  Measured figures:
profiles/lstm2_ops_parity.txt."""
import numpy as np
import pytest
import torch

import lstm2_cases as lc

pytestmark = pytest.mark.gpu

IDS = [c.id for c in lc.CASES]
COUNTED = [c.id for c in lc.CASES if any(nact is not None for _, _, nact in c.stacks)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from visdial_amd import ops as o
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_RUNS = {}


def run(ops, c, direction, counts=True):
    """one call on fresh copies of the case's buffers; what it left behind, per stack {name -> flat float32 array with its guard}.  Shared
    among the tests of this file"""
    key = (c.id, direction, counts)
    if key in _RUNS:
        return _RUNS[key]
    descs = []
    for s in lc.operands(c.shape):
        d = dict(T=s.T, N=s.N, Wh1=dev(s.Wh1), Wx2=dev(s.Wx2), Wh2=dev(s.Wh2), nact=s.nact if counts else None)
        if direction == 'fwd':
            d.update(tok_mask=dev(s.tok), b2=dev(s.b2))
        d.update({k: dev(v) for k, v in (s.fwd0 if direction == 'fwd' else s.bwd0).items()})
        descs.append(d)
    if c.arith == 'bf16':
        ops.lstm2_pass(descs, c.H, ops.FLAG_BF16, backward=direction == 'bwd')
    elif direction == 'fwd':
        ops.lstm2_forward(descs, c.H)
    else:
        ops.lstm2_backward(descs, c.H)
    torch.cuda.synchronize()
    names = lc.FWD_OUT if direction == 'fwd' else lc.BWD_OUT + lc.BWD_IN
    _RUNS[key] = [{k: d[k].cpu().numpy() for k in names} for d in descs]
    return _RUNS[key]


@pytest.mark.parametrize('cid', IDS)
def test_parity(ops, cid):
    """forward, then backward (on the fp64 forward state rounded to fp32), through the checker of tests/lstm2_cases.py"""
    c = lc.case(cid)
    reps = {}
    for direction in ('fwd', 'bwd'):
        got = run(ops, c, direction)
        reps[direction] = rep = lc.check(c, direction, got)
        for (si, name), (_, e, b, label) in sorted(rep.worst.items()):
            print('PARITY %-18s %s stack %d %-8s worst slice %-9s rel-L2 %.3e bound %.0e' % (c.id, direction, si, name, label, e, b))
        if direction == 'bwd':                                   # the inputs of the backward call are inputs: not a bit of them changes
            for s, g in zip(lc.operands(c.shape), got):
                for k in lc.BWD_IN:
                    assert g[k].tobytes() == s.bwd0[k].tobytes(), k
    assert all(r.ok for r in reps.values()), '\n'.join((reps['fwd'].failures + reps['bwd'].failures)[:12])


@pytest.mark.parametrize('cid', COUNTED)
def test_counts_against_no_counts(ops, cid):
    """the same operands with nact = NULL: the same tok_mask, the same zero-filled buffers.  The tile config is fixed per entry, the row
    tiles start at row 0 and the rows of a tile are independent, so every live row of every output is bit-identical between the two runs.
    dc1 / dc2 are compared on the rows that are live from step 0 on: without counts a row that is pad before step t0 is carried through its
    masked steps, where the zero forget gate clears its dc (dL/dc0 = 0), while with counts it stops at what flows into step t0
    (include/visdial_hip.h)."""
    c = lc.case(cid)
    for direction, names in (('fwd', lc.FWD_OUT), ('bwd', lc.BWD_OUT)):
        with_counts, without = run(ops, c, direction), run(ops, c, direction, counts=False)
        for si, s in enumerate(lc.operands(c.shape)):
            for name in names:
                a, b = lc.view(s, name, with_counts[si][name]), lc.view(s, name, without[si][name])
                live = s.live[:1] if name in ('dc1', 'dc2') else s.live
                same = all(a[t, :n].tobytes() == b[t, :n].tobytes() for t, n in enumerate(live))
                print('COUNTS %-18s %s stack %d %-8s live rows %s' % (c.id, direction, si, name, 'bit-identical' if same else 'DIFFER'))
                assert same, (direction, si, name)
                assert with_counts[si][name][-lc.GUARD:].tobytes() == without[si][name][-lc.GUARD:].tobytes()


def whole_err(s, got, ref, name):
    return lc.rel_l2(lc.view(s, name, got[name])[:, :s.never], ref[name][:, :s.never])


@pytest.mark.parametrize('sid', list(lc.SHAPES))
def test_bf16_switch(ops, sid):
    """vd_lstm2_forward_p takes the fp32 tick config under VD_FLAG_BF16 when H % 64 != 0: bit-identical to flags = 0 there, measurably
    different from fp32 (rel-L2 of h2 against fp64 above 1e-5) at H = 64, 128, 512.  The backward takes the bf16 config at every H."""
    c32, c16 = lc.case(sid + '-fp32'), lc.case(sid + '-bf16')
    H = c32.H
    f32, f16 = run(ops, c32, 'fwd'), run(ops, c16, 'fwd')
    b32, b16 = run(ops, c32, 'bwd'), run(ops, c16, 'bwd')
    for si, s in enumerate(lc.operands(sid)):
        if H % 64:
            for name in lc.FWD_OUT:
                assert f32[si][name].tobytes() == f16[si][name].tobytes(), name
        else:
            e32, e16 = whole_err(s, f32[si], s.ref_fwd, 'h2'), whole_err(s, f16[si], s.ref_fwd, 'h2')
            print('SWITCH %-12s fwd stack %d h2 fp32 %.3e bf16 %.3e' % (sid, si, e32, e16))
            assert e16 > 1e-5 and e32 < 1e-5
        e32, e16 = whole_err(s, b32[si], s.ref_bwd, 'dh1_seq'), whole_err(s, b16[si], s.ref_bwd, 'dh1_seq')
        print('SWITCH %-12s bwd stack %d dh1_seq fp32 %.3e bf16 %.3e' % (sid, si, e32, e16))
        assert b32[si]['dh1_seq'].tobytes() != b16[si]['dh1_seq'].tobytes()
        assert e16 > 2e-5 and e32 < 2e-5


def test_backward_refuses_decreasing_counts(ops):
    """nact = [5, 3] at N = 8: every count is in range, so the call is safe on a build without the check too; the backward is meaningful
    for non-decreasing counts only (dc is initialised at the last step, for its rows).  Refused with a message that names the field, and
    nothing is written.  (No test passes a count outside [0, N]: without the check such a call would write out of bounds.)"""
    from visdial_amd import _lib
    T, N, H = 2, 8, 32
    rng = np.random.RandomState(5)
    host = dict(Wh1=rng.randn(H, 4 * H), Wx2=rng.randn(H, 4 * H), Wh2=rng.randn(H, 4 * H), gates1=rng.rand(T, N, 4 * H), gates2=rng.rand(T, N, 4 * H),
                c1=rng.randn(T, N, H), c2=rng.randn(T, N, H), dh_last2=rng.randn(N, H), dh1_seq=np.full((T, N, H), lc.FILL),
                dc1=np.full((N, H), lc.FILL), dc2=np.full((N, H), lc.FILL))
    host = {k: lc.buf(v) for k, v in host.items()}
    nact = np.array([5, 3], np.int32)
    for call in (lambda d: ops.lstm2_backward(d, H), lambda d: ops.lstm2_pass(d, H, ops.FLAG_BF16, backward=True)):
        d = dict(T=T, N=N, nact=nact, **{k: dev(v) for k, v in host.items()})
        with pytest.raises(_lib.VisdialHipError, match='nact'):
            call([d])
        torch.cuda.synchronize()
        for k, v in host.items():
            assert d[k].cpu().numpy().tobytes() == v.tobytes(), k
