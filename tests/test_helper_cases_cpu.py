"""tests/helper_cases.py checked without a GPU: the references are pinned (mix32 on hand-computed vectors and against the C text, the fp64
heads, log-softmax and sums against torch in float64, the integer restatements against their definitions), the tables cover what they
promise, every checker passes a float32 numpy emulation of a correct call on every case, and fails each of a set of subtly wrong emulations
wherever the mutant applies.  A mutant may be exempt on at most two cases, each with its reason (EXEMPT)."""
import os
import re

import numpy as np
import pytest
import torch

import helper_cases as hc
import train_knobs_ref as kr
from oracle import visdial_oracle as vo

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'visdial_amd', 'csrc')
IDS = lambda table: [c.id for c in table]
T64 = lambda a: torch.from_numpy(np.array(a, np.float64))


# ------------------------------------------------------------------------------------------------------------ tripwire on the C text
def _code(path):
    src = open(os.path.join(CSRC, path)).read()
    src = re.sub(r'/\*.*?\*/', ' ', src, flags=re.S)
    return ' '.join(re.sub(r'//[^\n]*', ' ', src).split())


RECORDED = {
    'elementwise.hip': [
        (1, '__device__ __forceinline__ uint32_t mix32(uint64_t x) { x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; '
            'x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33; return (uint32_t)x; }'),
        (1, 'const uint32_t thr = (uint32_t)(p * 16777216.0f);'),
        (1, 'const uint32_t h = mix32(seed * 0x9E3779B97F4A7C15ULL + (uint64_t)(i4 + k));'),
        (1, 'm[k] = ((h >> 8) >= thr) ? 1 : 0;'),
        (2, 'const int jj = min(j + u, cnt - 1);'),
        (2, 'segment_rowsum_kernel<256'),
        (1, 'const int c2 = c + blockDim.x * 4;'),
        (1, 'hipLaunchKernelGGL(tok_scan_kernel, dim3(1), dim3(1024), 0, s, count, V, offset, cursor);'),
        (1, 'hipLaunchKernelGGL(zero_inactive_rows_kernel, dim3(64, T), dim3(256),'),
        (1, 'hipLaunchKernelGGL(zero_inactive_multi_kernel, dim3(128, T), dim3(256),'),
        (1, 'if (b == i && i + 1 < z.n && q >= (z.ncols[i] >> 2)) { q -= z.ncols[i] >> 2; b = i + 1; }'),
        (1, 'if (v != 0.f) unsafeAtomicAdd(demb + (long)tok[r] * E + e, v);'),
    ],
    'loss.hip': [
        (1, '#define MAX_OPT 128'),
        (1, 'for (long c = V + tid; c < ld; c += 256) row[c] = 0.f;'),
        (1, 'if (tok_in[r] == 0 || target[r] <= 0) {'),
        (2, 'r += (sc[j] > s) || (sc[j] == s && j < o);'),
        (1, 'for (int k = lane * 4; k < H; k += 256) {'),
        (3, 'for (int k = tid * 4; k < H; k += 1024)'),
    ],
}


def test_kernel_text_reads_as_recorded():
    """what helper_cases.py restates (mix32, the threshold, the strides and grids its shapes are chosen around), as whitespace-normalised
    text with the number of places it stands in"""
    for path, items in RECORDED.items():
        src = _code(path)
        for count, text in items:
            assert src.count(text) == count, (
                "%s no longer holds %d x `%s`: restate it in tests/helper_cases.py, re-derive the shapes of the case tables around it, then "
                "record the new text here" % (path, count, text))


# ------------------------------------------------------------------------------------------------------------ the integer references
def test_mix32_on_hand_computed_vectors():
    """computed with unbounded Python integers reduced mod 2^64 after each product"""
    vectors = {0x0: 0x0, 0x1: 0x34c2cb2c, 0x2: 0x650683e7, 0x9e3779b97f4a7c15: 0xa4ab2eea, 0xa768c027950a1d3f: 0xff9af39f,
               0xffffffffffffffff: 0x4b825f21}
    for x, want in vectors.items():
        assert int(hc.mix32(np.uint64(x))[0]) == want, hex(x)
    M = 2 ** 64 - 1

    def plain(x):
        x ^= x >> 33
        x = (x * 0xff51afd7ed558ccd) & M
        x ^= x >> 33
        x = (x * 0xc4ceb9fe1a85ec53) & M
        return (x ^ (x >> 33)) & 0xffffffff
    assert (1234 * 0x9E3779B97F4A7C15 + 5) & M == 0xa768c027950a1d3f
    for seed in hc.SEEDS:
        got = hc.dropout_hash24(9, seed)
        assert got.tolist() == [plain((seed * 0x9E3779B97F4A7C15 + i) & M) >> 8 for i in range(9)], seed


def test_dropout_reference():
    assert int(hc.dropout_threshold(0.0)) == 0 and int(hc.dropout_threshold(0.5)) == 2 ** 23 and int(hc.dropout_threshold(hc.P_MAX)) == 2 ** 24 - 1
    assert int(hc.dropout_threshold(0.2)) == int(np.float32(0.2) * np.float32(2 ** 24)) == 3355443
    assert set(c.p['n'] for c in hc.DROPOUT) == {1, 3, 4, 5, 1023, 1024, 1025, 2049}
    assert set(c.p['seed'] for c in hc.DROPOUT) == set(hc.SEEDS) and set(c.p['p'] for c in hc.DROPOUT) >= {0.0, 0.2, 0.5, hc.P_MAX}
    for c in hc.DROPOUT:
        want = hc.dropout_layout(c).specs[0].exact
        n = c.p['n']
        assert set(np.unique(want[:n]).tolist()) <= {0, 1} and (want[n:] == hc.BMARK).all() and want.size == n + hc.GUARD
        if c.p['p'] == 0.0:
            assert (want[:n] == 1).all()                                                    # p = 0 is all ones
        if c.p['p'] == hc.P_MAX:
            assert want[:n].sum() <= 1
    big = hc.dropout_bits(200000, 1234, 0.2)
    assert abs(big.mean() - 0.8) < 5e-3
    on = [c for c in hc.DROPOUT if c.id == 'drop-n5-on-threshold'][0]
    assert int(hc.dropout_hash24(5, 1234)[2]) == int(hc.dropout_threshold(on.p['p'])) and 0 < on.p['p'] < 1
    assert hc.dropout_bits(5, 1234, on.p['p'])[2] == 1 and hc.dropout_bits(5, 1234, on.p['p'], strict=True)[2] == 0


def test_token_sort_and_ranks_references():
    assert set(c.p['V'] for c in hc.TOKEN_SORT) == {1, 2, 57, 1023, 1024, 1025, 11323} and len(hc.TOKEN_SORT) >= 14
    assert set(c.p['n'] for c in hc.TOKEN_SORT) == {0, 1, 63, 64, 65, 255, 256, 257, 5000}
    assert set(c.p['dist'] for c in hc.TOKEN_SORT) >= {'one', 'distinct', 'half', 'last'}
    for c in hc.TOKEN_SORT:
        lay = hc.token_sort_layout(c)
        V, n, tok = c.p['V'], c.p['n'], lay.tokens
        off = lay.specs[0].exact
        assert off[0] == 0 and off[V] == n and all(off[v + 1] - off[v] == int((tok == v).sum()) for v in range(0, V, max(1, V // 50)))
        assert tok.size == n and (n == 0 or (0 <= tok.min() and tok.max() < V))
        if c.p['dist'] == 'distinct':
            assert len(set(tok.tolist())) == n
        if c.p['dist'] == 'half':
            assert n < 100 or 0.3 < (tok == 0).mean() < 0.7
    assert set(c.p['O'] for c in hc.RANKS) == {1, 2, 127, 128}
    for c in hc.RANKS:
        lay = hc.ranks_layout(c)
        want = lay.specs[0].exact[:lay.s.size].reshape(lay.s.shape)
        assert np.array_equal(want, vo.compute_ranks(lay.s))                                # the oracle's stable descending sort
        assert all(sorted(r.tolist()) == list(range(1, c.p['O'] + 1)) for r in want)
        assert (want[0] == np.arange(1, c.p['O'] + 1)).all() and (want[3] == np.arange(1, c.p['O'] + 1)).all()     # equal; +0 == -0
        if c.p['O'] >= 127:
            assert np.isinf(lay.s[4]).any() and np.signbit(lay.s[3]).any() and not np.signbit(lay.s[3]).all()


# ------------------------------------------------------------------------------------------------------------ the fp64 references
def _ref(spec):
    return spec.ref[:-hc.GUARD]


@pytest.mark.parametrize("case", hc.LOGSOFTMAX, ids=IDS(hc.LOGSOFTMAX))
def test_log_softmax_reference_is_torch_in_float64(case):
    lay = hc.logsoftmax_layout(case)
    V, rows, ld = case.p['V'], case.p['rows'], case.p['V'] + case.p['pad']
    assert np.abs(lay.x).max() <= 80
    want = torch.log_softmax(T64(lay.x), 1).numpy()
    if V == 1:
        assert (hc.bits(lay.specs[0].exact[:rows * ld].reshape(rows, ld)[:, 0]) == 0).all()
        return
    ref = _ref(lay.specs[0]).reshape(rows, ld)[:, :V]
    assert np.isfinite(ref).all() and float(np.abs(ref - want).max()) <= 1e-12 * max(1.0, float(np.abs(want).max()))
    assert np.isnan(lay.specs[0].out0[:rows * ld].reshape(rows, ld)[:, V:]).all()
    if case.p['hot'] in ('first', 'last'):
        col = 0 if case.p['hot'] == 'first' else V - 1
        assert (lay.x[:2, col] == 80).all() and (np.delete(lay.x[:2], col, 1) == -80).all()


@pytest.mark.parametrize("eps,wg", hc.NLL_VARIANTS)
@pytest.mark.parametrize("case", hc.NLL, ids=IDS(hc.NLL))
def test_nll_reference_is_torch_in_float64(case, eps, wg):
    lay = hc.nll_layout(case, eps, wg)
    V, ld, rows = case.p['V'], case.p['V'] + case.p['pad'], hc.NLL_ROWS
    live = lay.live
    assert live.tolist() == [True, True, False, False, True, True] and lay.target[0] == 1 and lay.target[1] == V
    assert lay.tok_in[2] == 0 and lay.target[2] > 0 and lay.tok_in[3] != 0 and lay.target[3] == 0
    x = T64(lay.x[live]).requires_grad_()
    loss = torch.nn.functional.cross_entropy(x, torch.from_numpy((lay.target[live] - 1).astype(np.int64)), reduction='none', label_smoothing=eps)
    loss.sum().backward()
    ref = _ref(lay.specs[0])
    assert float(np.abs(ref[live] - loss.detach().numpy()).max()) <= 1e-12 * max(1.0, float(loss.detach().max()))
    buf = lay.specs[1].out0[:rows * ld].reshape(rows, ld)
    assert np.isnan(buf[:, V:]).all() and np.isnan(buf[~live]).all() and np.abs(buf[live, :V]).max() <= 80
    if wg:
        g = _ref(lay.specs[1]).reshape(rows, ld)
        assert float(np.abs(g[live, :V] - x.grad.numpy()).max()) <= 1e-12 and (g[~live] == 0).all() and (g[:, V:] == 0).all()
        assert (hc.bits(lay.specs[1].exact[:rows * ld].reshape(rows, ld)[:, V:]) == 0).all()


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("case", hc.SCORE, ids=IDS(hc.SCORE))
def test_score_reference_is_torch_in_float64(case, eps):
    lay = hc.score_layout(case, eps)
    O, H, N = case.p['O'], case.p['H'], case.p['N']
    optH, enc = T64(lay.optH).requires_grad_(), T64(lay.enc).requires_grad_()
    s = torch.einsum('noh,nh->no', optH, enc)
    loss = torch.nn.functional.cross_entropy(s, torch.from_numpy(lay.gt.astype(np.int64)), reduction='none', label_smoothing=eps)
    (loss.sum() * lay.gscale).backward()
    tol = lambda t: 1e-12 * max(1.0, float(t.detach().abs().max()))
    assert float(np.abs(_ref(lay.specs[0]) - s.detach().numpy().reshape(-1)).max()) <= tol(s) and float(s.detach().abs().max()) <= 80
    if case.p['mode'] != 'scores':
        assert float(np.abs(_ref(lay.specs[1]) - loss.detach().numpy()).max()) <= tol(loss)
    if case.p['mode'] == 'train':
        assert float(np.abs(_ref(lay.specs[2]) - optH.grad.numpy().reshape(-1)).max()) <= tol(optH.grad)
        assert float(np.abs(_ref(lay.specs[3]) - enc.grad.numpy().reshape(-1)).max()) <= tol(enc.grad)
    if eps == 0.0 and case.p['mode'] != 'scores':                                           # and the oracle's head
        _, _, rows_ref = vo.cross_entropy(s.detach().numpy(), lay.gt)
        assert float(np.abs(_ref(lay.specs[1]) - rows_ref).max()) <= tol(loss)
    if case.p['hot']:
        assert set(np.unique(s.detach().numpy()).tolist()) == {-80.0, 80.0}
    assert (N == 1 and lay.gt[0] in (0, O - 1)) or (lay.gt[0] == 0 and lay.gt[1] == O - 1)


def test_score_table_covers_what_it_promises():
    S = hc.SCORE
    assert len(S) >= 12 and set(c.p['O'] for c in S) == {1, 2, 63, 64, 65, 100, 128} and set(c.p['N'] for c in S) == {1, 3}
    assert set(c.p['H'] for c in S) == {4, 252, 256, 260, 1020, 1024, 1028} and set(c.p['mode'] for c in S) == {'train', 'scores', 'loss'}
    assert sum(c.p['hot'] for c in S) == 1 and max(c.p['O'] for c in S) == hc.MAX_OPT
    one = [int(hc.score_layout(c, 0.0).gt[0]) == 0 for c in S if c.p['N'] == 1 and c.p['O'] > 1]
    assert True in one and False in one                                                     # N = 1: gt at 0 and at O - 1 in turn
    vs = set(c.p['V'] for c in hc.NLL)
    assert vs == set(hc.V_SET) == set(c.p['V'] for c in hc.LOGSOFTMAX)
    assert set(c.p['pad'] for c in hc.NLL) == {0, 3, 300} and set(c.p['pad'] for c in hc.LOGSOFTMAX) == {0, 2}
    assert set(c.p['rows'] for c in hc.LOGSOFTMAX) == {1, 3}
    assert sorted(str(c.p['hot']) for c in hc.NLL if c.p['hot']) == ['first', 'flat80', 'last']


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("case", hc.SEGSUM, ids=IDS(hc.SEGSUM))
def test_segment_sum_reference_is_torch_in_float64(case, bf16):
    lay = hc.segsum_layout(case, bf16)
    n, ncol, ldx, ldo, V = (case.p[k] for k in ('n', 'ncol', 'ldx', 'ldo', 'V'))
    s = lay.specs[0]
    out0 = s.out0[:V * ldo].reshape(V, ldo)
    want = T64(out0[:, :ncol]).index_add(0, torch.from_numpy(lay.tokens.astype(np.int64)), T64(lay.x)).numpy()
    ref = _ref(s).reshape(V, ldo)
    have = np.isin(np.arange(V), lay.tokens)
    assert float(np.abs(ref[have, :ncol] - want[have]).max()) <= 1e-12 * max(1.0, float(np.abs(want).max()))
    assert np.array_equal(s.bounded[:V * ldo].reshape(V, ldo), np.outer(have, np.arange(ldo) < ncol))
    assert (out0[:, ncol:] == hc.MARK).all() and (out0[:, :ncol] != 0).all()
    assert sorted(lay.perm.tolist()) == list(range(n)) and (np.diff(lay.tokens[lay.perm]) >= 0).all()
    X = lay.inp['X'][:n * ldx].reshape(n, ldx)
    if bf16:
        assert X.dtype == np.uint16 and (X[:, ncol:] == hc.NAN16).all() and np.array_equal(hc._bf16_values(X[:, :ncol]), lay.x)
        assert np.isnan(hc._bf16_values(np.array([hc.NAN16]))).all()
    else:
        assert np.isnan(X[:, ncol:]).all() and np.array_equal(X[:, :ncol], lay.x)


def test_sum_tables_cover_what_they_promise():
    S = hc.SEGSUM
    assert len(S) >= 12 and set(c.p['n'] for c in S) == {1, 3, 4, 5, 255, 256, 257, 600}
    assert set(c.p['ncol'] for c in S) == {4, 1020, 1024, 1028, 2048, 2052, 3072}
    assert any(c.p['ldx'] > c.p['ncol'] for c in S) and any(c.p['ldo'] > c.p['ncol'] for c in S)
    span = hc.segsum_layout([c for c in S if c.p['dist'] == 'span3'][0], False)
    run = np.flatnonzero(span.tokens[span.perm] == 0)
    assert run[0] == 0 and run[-1] >= 2 * hc.CHUNK                                         # the pad token's run reaches the third chunk
    each = hc.segsum_layout([c for c in S if c.p['dist'] == 'each' and c.p['n'] == 255][0], False)
    assert (np.diff(each.tokens[each.perm]) > 0).all()                                      # a token change at every row
    assert max(hc.segsum_layout(c, False).inp['X'].nbytes for c in S) < 3.2e6
    assert set(c.p['E'] for c in hc.GATHER) == {4, 300, 512, 2048} and set(c.p['rows'] for c in hc.GATHER) == {1, 7, 213}
    assert any(c.p['rows'] > c.p['V'] + 1 for c in hc.GATHER) and set(c.p['mask'] for c in hc.GATHER) == {True, False}
    assert any(c.p['rows'] * c.p['E'] // 4 % 256 for c in hc.GATHER)
    for c in hc.GATHER:
        tok = hc.gather_layout(c).inp['tok'][:c.p['rows']]
        assert tok[0] == 0 and tok[-1] == c.p['V'] or c.p['rows'] == 1
    assert set(c.p['E'] for c in hc.SCATTER) == {1, 3, 300} and set(c.p['dist'] for c in hc.SCATTER) >= {'one', 'distinct'}
    assert set(c.p['T'] for c in hc.MASKTIME) == {1, 3} and set(c.p['N'] for c in hc.MASKTIME) == {1, 5, 257} and set(c.p['D'] for c in hc.MASKTIME) == {1, 3, 300}
    Z = hc.ZERO_ROWS
    assert set(c.p['T'] for c in Z) == {1, 4} and set(c.p['N'] for c in Z) == {1, 7, 300} and set(c.p['ncols'] for c in Z) == {4, 128, 2048}
    assert any(c.p['ld'] > c.p['ncols'] and c.p['tstride'] > c.p['N'] * c.p['ld'] for c in Z)
    assert any(c.p['N'] == 300 and c.p['ncols'] == 2048 and (300 - c.p['nact'][0]) * 512 > 2 * 64 * 256 for c in Z)
    assert all(c.p['tstride'] >= c.p['N'] * c.p['ld'] and c.p['tstride'] % 4 == 0 and c.p['ld'] % 4 == 0 for c in Z)
    for tab in (Z, hc.ZERO_MULTI):
        nact = [(a, c.p['N']) for c in tab for a in c.p['nact']]
        assert any(a == 0 for a, N in nact) and any(a == N for a, N in nact) and any(0 < a < N for a, N in nact)
    assert set(len(c.p['widths']) for c in hc.ZERO_MULTI) == {1, 2, 6}
    assert (16, 4, 4, 4, 4, 16) in [c.p['widths'] for c in hc.ZERO_MULTI] and (4, 8, 2048, 4, 512, 12) in [c.p['widths'] for c in hc.ZERO_MULTI]
    assert set((c.p['op'].split('-')[0], c.p['n']) for c in hc.POINTWISE) == set((o, n) for o in ('dropout_apply', 'tanh_backward', 'axpby') for n in (1, 255, 256, 257))


@pytest.mark.parametrize("case", hc.SCATTER, ids=IDS(hc.SCATTER))
def test_scatter_reference_is_the_oracle(case):
    lay = hc.scatter_layout(case)
    E, rows, V = case.p['E'], case.p['rows'], case.p['V']
    s = lay.specs[0]
    ref = s.out0[:(V + 1) * E].astype(np.float64).reshape(V + 1, E)
    dx = lay.inp['dx'][:rows * E].astype(np.float64).reshape(rows, E)
    if 'mask' in lay.inp:
        dx = dx * lay.inp['mask'][:rows * E].reshape(rows, E) * 2.0
    vo.lookup_backward(ref, lay.tokens, dx)
    own = s.bounded[:(V + 1) * E].reshape(V + 1, E)
    assert float(np.abs(_ref(s).reshape(V + 1, E) - ref)[own].max()) <= 1e-12 * max(1.0, float(np.abs(ref).max()))
    assert not own[np.setdiff1d(np.arange(V + 1), lay.tokens)].any()                         # a token row without a member is not owned
    assert (dx[0] == 0).all() and (rows == 1 or np.signbit(lay.inp['dx'][E:2 * E]).all())
    if case.p['dist'] == 'one':
        assert len(set(lay.tokens.tolist())) == 1
    if case.p['dist'] == 'distinct':
        assert len(set(lay.tokens.tolist())) == min(rows, V + 1)


@pytest.mark.parametrize("case", hc.MASKTIME, ids=IDS(hc.MASKTIME))
def test_mask_time_reference_is_torch(case):
    lay = hc.masktime_layout(case)
    T, N, D = (case.p[k] for k in 'TND')
    tok = torch.from_numpy(np.array(lay.inp['tok'][:T * N]).reshape(T, N))
    feat = T64(lay.inp['feat'][:N * D].reshape(N, D)).requires_grad_()
    out = feat[None] * (tok != 0)[:, :, None]
    dout = T64(lay.inp['dout'][:T * N * D].reshape(T, N, D))
    out.backward(dout)
    assert np.array_equal(lay.specs[0].exact[:T * N * D], out.detach().numpy().astype(np.float32).reshape(-1))
    assert float(np.abs(_ref(lay.specs[1]) - feat.grad.numpy().reshape(-1)).max()) <= 1e-12 * 10
    assert (np.array(lay.inp['dout'][:T * N * D]).reshape(T, N, D)[tok.numpy() == 0] == np.float32(1e30)).all()
    if N >= 5:
        assert (tok[:, 0] == 0).all() and (tok[:, 1] != 0).all()


# ------------------------------------------------------------------------------------------------------------ checkers: pass and fail
def _guard_damage(lay, good):
    """the first and the last guard element of every output, and the element in front of the guard where it is a mark"""
    for s in lay.specs:
        for idx in (s.out0.size - hc.GUARD, s.out0.size - 1):
            bad = dict(good)
            bad[s.name] = good[s.name].copy()
            bad[s.name][idx] = 0
            assert not hc.check(lay, bad).ok, (lay.case.id, s.name, idx)


def _run_family(table, layout, emulate, mutants, applies=None, exempt=None, args=(), need=1):
    """every case: the checker passes the emulation and catches guard damage; every mutant: caught wherever it applies (`applies`, or
    for a bit-for-bit family wherever the mutant's outputs differ from the right ones), except on the cases of `exempt`"""
    exempt = exempt or {}
    caught = dict((m, 0) for m in mutants)
    for c in table:
        lay = layout(c, *args)
        good = emulate(lay)
        v = hc.check(lay, good)
        assert v.ok and v.ratio <= 0.5, (c.id, args, v)
        _guard_damage(lay, good)
        for m in mutants:
            hit = applies(c, m) if applies else None               # None: wherever the mutant's outputs differ from the right ones
            if hit is False:
                continue
            bad = emulate(lay, m)
            if hit is None and not hc.differs(bad, good):
                continue
            vb = hc.check(lay, bad)
            if c.id in exempt.get(m, {}):
                assert vb.ok, (c.id, 'is exempt from `%s` but the checker catches it: drop the exemption' % m)
                continue
            assert not vb.ok, (m, c.id, args)
            caught[m] += 1
    for m in mutants:
        assert len(exempt.get(m, {})) <= 2 and caught[m] >= need, (m, caught[m], args)
    return caught


# mutant -> the cases it does not move past the bound, each with its reason.  No more than two per mutant and family.
EXEMPT_LSE = {'lse without the max subtraction': {
    'lsm-V65-pad2-r3-first': 'e^80 = 5.5e34 is finite in fp32 and holds all the mass: the plain sum is as accurate as the shifted one',
    'lsm-V257-pad2-r3-last': 'the same with the maximum in the last column; the flat +80 row of V = 11322 overflows and is caught'}}
EXEMPT_NLL = {'lse without the max subtraction': {
    'nll-V65-pad3-first': 'e^80 is finite in fp32: the plain sum is as accurate as the shifted one',
    'nll-V257-pad3-last': 'the same; the flat +80 rows of V = 11322 overflow and are caught'}}
EXEMPT_SCORE = {'lse without the max subtraction': {
    'score-O128-H4-N3-train-pm80': 'at most 128 options: 128 e^80 = 7.1e36 cannot overflow fp32 at |score| <= 80, so the head has no case '
                                   'that shows this mutant; the gen head and log_softmax_rows do (V = 11322)'},
    'last option dropped from the lse': {
        'score-O128-H4-N3-train-pm80': 'option O - 1 scores -80 beside two of +80: it adds e^-160 to the sum, below the rounding of fp64'}}


def test_dropout_checker():
    _run_family(hc.DROPOUT, hc.dropout_layout, hc.emulate_dropout, ['tail writes 4 bytes at n - 1', 'threshold compared with >'])


def test_pointwise_checker():
    _run_family(hc.POINTWISE, hc.pointwise_layout, hc.emulate_pointwise, ['one element too many'], need=len(hc.POINTWISE))


def test_gather_checker():
    _run_family(hc.GATHER, hc.gather_layout, hc.emulate_gather, ['last quad dropped'], need=len(hc.GATHER))


def test_scatter_checker():
    _run_family(hc.SCATTER, hc.scatter_layout, hc.emulate_scatter, ['token off by one', 'mask ignored'],
                applies=lambda c, m: c.p['mask'] if m == 'mask ignored' else True, need=3)


def test_mask_time_checker():
    _run_family(hc.MASKTIME, hc.masktime_layout, hc.emulate_masktime, ['mask ignored'], need=4)


def test_zero_rows_checker():
    _run_family(hc.ZERO_ROWS, hc.zero_rows_layout, hc.emulate_zero_rows, list(hc.ZERO_MUTANTS), need=4)


def test_zero_multi_checker():
    _run_family(hc.ZERO_MULTI, hc.zero_multi_layout, hc.emulate_zero_multi,
                ['one row too many', 'one row too few', 'buffer boundary off by one quad'], need=4)
    # the kernel-order emulation and the plain statement of the contract agree on every case
    for c in hc.ZERO_MULTI:
        lay = hc.zero_multi_layout(c)
        assert not hc.differs(hc.emulate_zero_multi(lay), lay.good())
    n1 = [c for c in hc.ZERO_MULTI if len(c.p['widths']) == 1]
    assert all(not hc.differs(hc.emulate_zero_multi(hc.zero_multi_layout(c), 'buffer boundary off by one quad'), hc.zero_multi_layout(c).good())
               for c in n1)                                                                  # (one buffer has no boundary)


def test_token_sort_checker():
    _run_family(hc.TOKEN_SORT, hc.token_sort_layout, hc.emulate_token_sort, ['offset[V] missing', 'inclusive scan', 'sorted by row'],
                applies=lambda c, m: bool((np.diff(hc.token_sort_layout(c).tokens) < 0).any()) if m == 'sorted by row' else None, need=8)
    c = [c for c in hc.TOKEN_SORT if c.p['n'] == 0][0]                                       # n = 0 leaves perm untouched
    lay = hc.token_sort_layout(c)
    bad = hc.emulate_token_sort(lay)
    bad['perm'][0] = 0
    assert not hc.check(lay, bad).ok
    c = [c for c in hc.TOKEN_SORT if c.p['n'] == 257][0]                                     # a row listed twice is no permutation
    lay = hc.token_sort_layout(c)
    bad = hc.emulate_token_sort(lay)
    bad['perm'][5] = bad['perm'][6]
    assert not hc.check(lay, bad).ok
    bad = hc.emulate_token_sort(lay)
    bad['work'][2 * c.p['V']] = 0                                                            # the scratch is guarded behind 2 V
    assert not hc.check(lay, bad).ok


@pytest.mark.parametrize("bf16", [False, True])
def test_segment_sum_checker(bf16):
    muts = ['clamp adds its duplicate row', 'second bf16 column group dropped', 'run flushed to the next token', 'out overwritten']
    _run_family(hc.SEGSUM, hc.segsum_layout, hc.emulate_segsum, [m for m in muts if bf16 or 'bf16' not in m],
                applies=lambda c, m: hc.segsum_mutant_applies(c, bf16, m), args=(bf16,), need=5)


def test_log_softmax_checker():
    _run_family(hc.LOGSOFTMAX, hc.logsoftmax_layout, hc.emulate_logsoftmax, ['lse without the max subtraction', 'last column dropped'],
                applies=lambda c, m: c.p['hot'] is not None if 'lse' in m else c.p['V'] > 1, exempt=EXEMPT_LSE)
    for c in hc.LOGSOFTMAX:                                                                 # V = 1: exactly +0, not -0
        if c.p['V'] == 1:
            lay = hc.logsoftmax_layout(c)
            bad = hc.emulate_logsoftmax(lay)
            bad['x'][0] = -0.0
            assert not hc.check(lay, bad).ok


@pytest.mark.parametrize("eps,wg", hc.NLL_VARIANTS)
def test_nll_checker(eps, wg):
    muts = ['lse without the max subtraction', 'target off by one', 'a masked row contributing', 'pad columns left alone',
            'pad columns beyond 256 left alone', 'logits written with write_grad = 0']
    muts = [m for m in muts if any(hc.nll_mutant_applies(c, eps, wg, m) for c in hc.NLL)]
    assert ('pad columns beyond 256 left alone' in muts) == bool(wg)
    _run_family(hc.NLL, hc.nll_layout, hc.emulate_nll, muts, applies=lambda c, m: hc.nll_mutant_applies(c, eps, wg, m), exempt=EXEMPT_NLL,
                args=(eps, wg))
    lay = hc.nll_layout(hc.NLL[2], eps, wg)                                                  # a masked row's loss: +0, not -0
    bad = hc.emulate_nll(lay)
    bad['loss'][2] = -0.0
    assert not hc.check(lay, bad).ok
    if wg:                                                                                  # a gradient row that does not sum to 0
        bad = hc.emulate_nll(lay)
        bad['logits'][:hc.NLL[2].p['V']] += np.float32(3e-5)
        assert any('row sums' in f for f in hc.check(lay, bad).failures)


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_score_checker(eps):
    muts = ['target off by one', 'gscale dropped', 'last option dropped from the lse', 'lse without the max subtraction']
    caught = _run_family(hc.SCORE, hc.score_layout, hc.emulate_score, muts, applies=hc.score_mutant_applies, exempt=EXEMPT_SCORE, args=(eps,), need=0)
    assert caught.pop('lse without the max subtraction') == 0 and min(caught.values()) >= 5, caught     # (EXEMPT_SCORE says why)
    lay = hc.score_layout([c for c in hc.SCORE if c.p['mode'] == 'scores'][0], eps)          # scores only: loss_rows untouched
    bad = hc.emulate_score(lay)
    bad['loss'][0] = 0.0
    assert not hc.check(lay, bad).ok


def test_ranks_checker():
    _run_family(hc.RANKS, hc.ranks_layout, hc.emulate_ranks, ['ties broken by higher index'], need=3)


def test_every_table_is_reached():
    """the tables this module walks are all of them"""
    assert list(hc.FAMILIES) == ['dropout_mask', 'pointwise', 'embed_gather', 'embed_scatter_acc', 'mask_time', 'zero_inactive_rows',
                                 'zero_inactive_multi', 'token_sort', 'segment_rowsum_acc', 'log_softmax_rows', 'logsoftmax_nll', 'score_ce', 'ranks']
    assert sum(len(t) for t in hc.FAMILIES.values()) == len(hc.case_list()) - len(hc.FAMILIES)
