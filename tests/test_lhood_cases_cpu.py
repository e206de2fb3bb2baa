"""tests/lhood_cases.py checked without a GPU: every head case reaches the kernel family it names under the restated dispatch, the table
covers what it promises, the C predicates still read as recorded here, the fp64 references are torch's, and the checkers pass a float32
numpy evaluation of every case and fail each of a set of subtly wrong ones wherever the mutant applies."""
import os
import re

import numpy as np
import pytest
import torch

import lhood_cases as lc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'visdial_amd', 'csrc')
HEAD_IDS = [c.id for c in lc.HEAD]
OPS = ('nll', 'lse')


# ------------------------------------------------------------------------------------------------------------ family reached, coverage
@pytest.mark.parametrize("case", lc.HEAD, ids=HEAD_IDS)
def test_head_case_reaches_the_family_it_names(case):
    assert case.path == case.family, (case.id, case.path)
    assert case.rows > int(lc.head_values(case.values).act.max()) + 1


def test_dispatch_at_the_thresholds():
    fam = lambda H, V, ldh=None, ldw=None, ha=0, wa=0: lc.head_family(1000, ldh or H, V, ldw or H, H, ha, wa)
    assert fam(64, 128) == 'mfma' and fam(48, 128) == 'rows' and fam(64, 127) == 'rows' and fam(72, 300) == 'rows'
    assert fam(64, 128, ldh=65) == 'rows' and fam(64, 128, ldw=66) == 'rows' and fam(64, 128, ldh=68, ldw=72) == 'mfma'
    assert fam(64, 128, ha=4) == 'rows' and fam(64, 128, wa=8) == 'rows' and fam(64, 128, ha=16, wa=32) == 'mfma'
    assert fam(12288, 2) == 'rows' and fam(12292, 2) == 'refused' and fam(12292, 128) == 'refused' and fam(12304, 128) == 'mfma'
    assert fam(64, 128, ldh=60) == 'refused' and fam(64, 128, ldw=63) == 'refused'
    assert lc.head_family(2 ** 24, 64, 128, 64, 64) == 'rows'                                # 2^24 rows x 256 bytes = 2^32
    assert [lc.prefix_fits(T, r) for T, r in ((1, 1), (255, 600), (256, 4), (0, 4), (5, 0))] == [True, True, False, False, False]
    assert all(lc.prefix_fits(c.T, c.rows) for c in lc.ORDER)


def test_table_covers_what_it_promises():
    H = lc.HEAD
    assert set(c.family for c in H) == {'mfma', 'rows'}                                     # both families, and every case runs as nll AND lse
    mf = [(c.H, c.V, c.n_act, c.ldh - c.H, c.ldw - c.H, c.bias) for c in H if c.family == 'mfma' and not c.hot and not c.h_off]
    assert set(mf) == {(64, 128, 128, 0, 0, True), (64, 129, 129, 0, 0, True), (80, 255, 1, 4, 8, True), (512, 384, 127, 0, 0, False),
                       (512, 1290, 300, 4, 4, True), (1040, 640, 257, 0, 0, True)}
    assert sorted(c.hot for c in H if c.hot) == ['first', 'last'] and all((c.H, c.V, c.n_act) == (512, 1290, 300) for c in H if c.hot)
    assert [(c.h_off % 4, c.h_off > 0, c.rows > 2 * c.n_act + 5) for c in H if c.family == 'mfma' and c.h_off] == [(0, True, True)]
    rows = [(c.H, c.V) for c in H if c.family == 'rows']
    assert rows == [(1, 1), (32, 7), (32, 63), (32, 257), (72, 300), (512, 127), (512, 1290), (512, 1290), (12288, 2)]
    assert lc.HEAD_BY_NAME['rows-512x1290-ldh-odd'].ldh == 513 and lc.HEAD_BY_NAME['rows-512x1290-misaligned'].h_off == 1
    assert lc.HEAD_BY_NAME['rows-12288x2'].H == lc.ROW_LDS_FLOATS
    assert set(c.values for c in H if c.name in lc.SHARED) == {'mfma-512x1290-n300'}
    # k-tiles of 16: 4 (3 DMA stages + 1), 5, 32, 65
    assert sorted(set(c.H // 16 for c in H if c.family == 'mfma')) == [4, 5, 32, 65]
    assert set(c.n_act for c in H) >= {1, 127, 128, 129}
    for c in H:
        v = lc.head_values(c.values)
        cols = set((v.target[v.act] - 1).tolist())
        assert (v.target[np.setdiff1d(np.arange(c.rows), v.act)] == 0).all()
        assert v.target[v.act].min() >= 1 and v.target[v.act].max() <= c.V
        if c.n_act == 1:
            assert cols == {c.tgt0}
            continue
        assert {0, c.V - 1} <= cols, c.id
        if c.n_act >= 5:
            assert {col for col in (127, 128) if col < c.V} <= cols, c.id
        if c.n_act >= 128:                                                                  # every (wave, lane-half, register) slot of EpiLhood::pick
            assert len(set(col % 128 for col in cols)) == min(128, c.V), c.id
        if v.twins:
            i0, i1, i2 = v.twins
            assert len({i0, i1, i2}) == 3 and v.target[v.act[i0]] == v.target[v.act[i1]] == v.target[v.act[i2]]
            assert np.array_equal(v.h[v.act[i0]], v.h[v.act[i1]]) and np.array_equal(v.h[v.act[i0]], v.h[v.act[i2]])
            if c.n_act > 256:                                                               # first tile, another lane of a middle tile, the last tile
                assert i0 < 128 <= i1 < c.n_act // 128 * 128 <= i2 and i0 % 32 != i1 % 32
    one = sorted(c.tgt0 for c in H if c.n_act == 1)
    assert one == [0, 254]                                                                  # one live row: column 0 and column V - 1 in turn
    # the +-80 cases: the spread, and where the maximum of every row lies
    for c in H:
        if c.hot:
            x = lc.logits64(lc.head_layout(c))
            col = lc.head_values(c.values).hot_col
            assert x.min() < -60 and np.delete(x, col, 1).max() > 60 and (x.argmax(1) == col).all()
            assert col // 128 == (0 if c.hot == 'first' else (c.V - 1) // 128) and 4 <= col % 32 < 8
    E = lc.EDGE
    assert set(c.H for c in E) >= {4, 252, 256, 260, 1028} and set(c.rows for c in E) == {1, 5, 1037} and set(c.T for c in E) == {0, 1, 9}
    assert any(c.ldo > c.C for c in E) and set(c.bias for c in E) == {True, False} and any(c.ldh > c.H and c.ldw > c.H for c in E)
    assert any(lc.edge_layout(c).empty is not None and lc.edge_layout(c).twin is not None for c in E)
    assert [(T, r) for T, r, _ in lc.ORDER_SHAPES] == [(1, 1), (21, 255), (21, 256), (21, 257), (255, 600), (20, 700)]
    assert any(lc.order_reference(lc.order_layout(c))['info'][0] == 1 for c in lc.ORDER if c.profile == 'holed')
    assert [n for n, _ in lc.LIVE] == [1, 1, 1023, 1024, 1025, 257 * 1024 + 3] and lc.cdiv(lc.LIVE[-1][0], lc.LIVE_BLOCK) > 256
    S = lc.SUM
    assert set(c.rows for c in S) == {1, 255, 257} and all(c.rows % c.C == 0 for c in S) and any(c.ldo > c.C for c in S) and any(c.empty for c in S)


# ------------------------------------------------------------------------------------------------------------ tripwire on the C text
def _code(path):
    src = open(os.path.join(CSRC, path)).read()
    src = re.sub(r'/\*.*?\*/', ' ', src, flags=re.S)
    return ' '.join(re.sub(r'//[^\n]*', ' ', src).split())


RECORDED = {
    'paths.h': [
        (1, 'static inline bool vd_lhood_fused_fits(long rows, long ldh, long V, long ldw, int H) { return H >= 64 && H % 16 == 0 && V >= 128 && '
            'ldh % 4 == 0 && ldw % 4 == 0 && rows * ldh * 4 < (1L << 32) && V * ldw * 4 < (1L << 32); }'),
        (1, 'static inline bool vd_lhood_prefix_fits(int T, long rows) { return T >= 1 && T < 256 && rows >= 1; }'),
    ],
    'lhood.hip': [
        (1, 'using LhoodCfg = GemmCfg<4, 1, 4, 16, 0, 3, 49152>;'),
        (1, 'constexpr int ORDER_ROWS = 256;'),
        (2, 'if (vd_lhood_fused_fits(rows, ldh, V, ldw, H) && ((uintptr_t)h & 15) == 0 && ((uintptr_t)W & 15) == 0) {'),
        (2, 'n_act >= 0 && n_act < (1L << 31) && rows >= 0 && V >= 1 && H >= 1 && ldh >= H && ldw >= H,'),
        (2, 'if (n_act == 0) return VD_OK;'),
        (2, 'VD_CHECK_ARG((size_t)H * 4 <= 48 * 1024,'),
        (1, 'C >= 1 && vd_lhood_prefix_fits(T, rows) && (long)T * rows < (1L << 31), "lhood order: bad args T=%d rows=%ld", T, (long)rows);'),
        (1, 'return rows + blocks * (T + 1) + blocks;'),
        (1, 'const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);'),
        (1, 'for (int k = lane * 4; k < K; k += 256) {'),
        (1, 'for (int b = tid; b < (int)blockIdx.x; b += 256) before += counts[b];'),
        (1, 'const int blocks = vd_cdiv(n, 1024);'),
    ],
}


def test_dispatch_predicates_read_as_recorded():
    """the predicates and constants lhood_cases.py restates, as whitespace-normalised text with the number of places they stand in"""
    for path, items in RECORDED.items():
        src = _code(path)
        for count, text in items:
            assert src.count(text) == count, (
                "%s no longer holds %d x `%s`: restate the dispatch in tests/lhood_cases.py (fused_fits, head_family, prefix_fits and the "
                "constants above them), re-derive the families of the case table, then record the new text here" % (path, count, text))


# ------------------------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("case", lc.HEAD, ids=HEAD_IDS)
def test_head_reference_is_torch_in_float64(case):
    lay = lc.head_layout(case)
    v = lay.v
    x = torch.from_numpy(v.h[v.act]).double() @ torch.from_numpy(np.array(v.W)).double().T
    if case.bias:
        x = x + torch.from_numpy(np.array(v.b)).double()
    tcol = torch.from_numpy((v.target[v.act] - 1).astype(np.int64))
    lse = torch.logsumexp(x, 1).numpy()
    nll = -torch.log_softmax(x, 1).gather(1, tcol[:, None])[:, 0].numpy()
    for op, t in (('lse', lse), ('nll', nll)):
        ref = lc.head_reference(lay, op)
        assert ref.shape == (case.n_act,) and np.isfinite(ref).all()
        assert float(np.abs(ref - t).max()) <= 1e-12 * max(1.0, float(np.abs(t).max())), (case.id, op)
    # everything the contract says is never read is NaN
    hv, wv = lay.hview(lay.hbuf), lay.wview(lay.wbuf)
    dead = np.setdiff1d(np.arange(case.rows), v.act)
    assert np.isnan(hv[dead]).all() and np.isnan(hv[:, case.H:]).all() and np.isnan(wv[:, case.H:]).all()
    assert np.isnan(lay.hbuf[:case.h_off]).all() and np.isnan(lay.hbuf[-lc.TAIL:]).all() and np.isnan(lay.wbuf[-lc.TAIL:]).all()
    assert np.isfinite(hv[v.act, :case.H]).all() and np.isfinite(wv[:, :case.H]).all()
    assert lay.bbuf is None or np.isnan(lay.bbuf[case.V:]).all()


@pytest.mark.parametrize("case", [c for c in lc.EDGE if c.T], ids=[c.id for c in lc.EDGE if c.T])
def test_edge_reference_is_torch_in_float64(case):
    lay = lc.edge_layout(case)
    ref, mag = lc.edge_reference(lay)
    h, W = torch.from_numpy(np.array(lay.h)).double(), torch.from_numpy(np.array(lay.W)).double()
    logits = h @ W.T                                                                        # [h rows x V]
    if case.bias:
        logits = logits + torch.from_numpy(lay.bbuf[:case.V]).double()
    want = np.zeros(case.rows)
    for r in range(min(case.rows, 40)):
        for t in range(case.T):
            if lay.etgt[t, r] > 0:
                nd = lay.enode[t, r]
                want[r] += float(logits[lay.node_row[nd], lay.etgt[t, r] - 1]) - float(lay.lse[nd])
    n = min(case.rows, 40)
    assert np.isfinite(ref).all() and float(np.abs(ref[:n] - want[:n]).max()) <= 1e-12 * max(1.0, float(mag.max()))
    assert (mag >= np.abs(ref) - 1e-9).all()


# ------------------------------------------------------------------------------------------------------------ the checkers
def _wrong(v, what):
    assert not v.ok, what
    return v


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("case", lc.HEAD, ids=HEAD_IDS)
def test_head_checker_passes_float32_and_catches_damage(case, op):
    lay = lc.head_layout(case)
    good = lc.emulate_head(lay, op)
    v = lc.check_head(lay, op, good)
    assert v.ok and v.ratio < 0.5, (case.id, op, v)
    for idx, val in ((case.n_act, 0.0), (good.size - 1, 0.0), (case.n_act - 1, np.nan)):   # the first and the last guard element; a NaN
        bad = good.copy()
        bad[idx] = val
        _wrong(lc.check_head(lay, op, bad), (case.id, op, idx))
    if lay.v.twins:                                                                         # one ulp between the repeated rows
        bad = good.copy()
        bad[lay.v.twins[2]] = np.nextafter(bad[lay.v.twins[2]], np.float32(np.inf))
        assert any('repeated rows differ' in f for f in _wrong(lc.check_head(lay, op, bad), (case.id, op)).failures)
    if case.V == 1 and op == 'nll':
        bad = good.copy()
        bad[0] = -0.0
        _wrong(lc.check_head(lay, op, bad), 'negative zero')


# (mutant, op) -> the cases the mutant does not move past the bound, each with its reason.  No more than two per mutant.
EXEMPT = {
    ('last tile dropped', 'lse'): {
        'mfma-512x1290-n300-max-first': 'the row maximum of 160 in column 5 holds all the mass: the last tile adds exp(-80) to the sum',
    },
    ('bias dropped', 'nll'): {
        'rows-1x1': 'one vocabulary entry: the bias cancels in lse - logit',
    },
}


@pytest.mark.parametrize("mutant", lc.MUTANTS_HEAD)
@pytest.mark.parametrize("op", OPS)
def test_head_checker_fails_the_mutant(mutant, op):
    exempt = EXEMPT.get((mutant, op), {})
    assert len(exempt) <= 2
    if mutant == 'target off by one' and op == 'lse':
        assert not any(lc.head_mutant_applies(c, op, mutant) for c in lc.HEAD)
        return                                                 # (vd_lhood_lse_p takes no target)
    ran = 0
    for case in lc.HEAD:
        if not lc.head_mutant_applies(case, op, mutant):
            continue
        lay = lc.head_layout(case)
        v = lc.check_head(lay, op, lc.emulate_head(lay, op, mutant))
        if case.name in exempt:
            assert v.ok, (case.id, 'is exempt from `%s` but the checker catches it: drop the exemption' % mutant)
            continue
        assert not v.ok, (mutant, op, case.id)
        ran += 1
    fams = set(c.family for c in lc.HEAD if lc.head_mutant_applies(c, op, mutant) and c.name not in exempt)
    assert ran >= 5 and ('mfma' in fams), (mutant, op, ran)


@pytest.mark.parametrize("case", lc.EDGE, ids=[c.id for c in lc.EDGE])
def test_edge_checker_passes_float32_and_fails_the_wrong_node(case):
    lay = lc.edge_layout(case)
    ref, mag = lc.edge_reference(lay)
    good = lc.emulate_edge(lay)
    v = lc.check_edge(lay, good, ref, mag)
    assert v.ok, (case.id, v.failures)
    idx = lay.out_index()
    for i in (lc.O_OFF - 1, int(idx[-1]) + 1, good.size - 1) + ((int(idx[case.C - 1]) + 1,) if case.ldo > case.C else ()):
        bad = good.copy()
        bad[i] = 0.0
        assert any('guard' in f for f in _wrong(lc.check_edge(lay, bad, ref, mag), (case.id, i)).failures)
    if case.T == 0:
        assert (good[idx].view(np.uint32) == 0).all()
        bad = good.copy()
        bad[idx[0]] = -0.0
        _wrong(lc.check_edge(lay, bad, ref, mag), 'negative zero at T = 0')
        return                                                 # (no edge: the wrong-node mutant does not apply)
    assert 0 < v.ratio <= 1.0
    _wrong(lc.check_edge(lay, lc.emulate_edge(lay, lse_shift=1), ref, mag), (case.id, 'lse of the wrong node'))
    if lay.empty is not None:
        bad = good.copy()
        bad[idx[lay.empty]] = -0.0
        _wrong(lc.check_edge(lay, bad, ref, mag), 'negative zero')
        bad = good.copy()
        bad[idx[lay.twin[1]]] = np.nextafter(bad[idx[lay.twin[1]]], np.float32(np.inf))
        assert any('tie' in f for f in _wrong(lc.check_edge(lay, bad, ref, mag), 'tie').failures)


@pytest.mark.parametrize("case", lc.ORDER, ids=[lc.order_id(c) for c in lc.ORDER])
def test_order_checker_passes_the_stable_sort_and_fails_an_unstable_one(case):
    lay = lc.order_layout(case)
    ref = lc.order_reference(lay)
    L = ref['length'][ref['perm']]
    assert (np.diff(L) <= 0).all() and sorted(ref['perm'].tolist()) == list(range(case.rows))
    assert all((np.diff(ref['perm'][L == k]) > 0).all() for k in np.unique(L))             # rows of one length keep their order
    assert ref['info'][1:].tolist() == [int((ref['length'] > t).sum()) for t in range(case.T)]
    # the plain definition, by python's stable sort
    assert ref['perm'].tolist() == sorted(range(case.rows), key=lambda r: -int(ref['length'][r]))
    good = lc.emulate_order(lay)
    assert lc.check_order(lay, good).ok
    for k in good:
        bad = dict(good)
        bad[k] = good[k].copy()
        bad[k][-lc.GUARD] = 0
        _wrong(lc.check_order(lay, bad), (k, 'guard'))
    if case.rows == 1:
        return                                                 # (one row: no two equal lengths, the mutant does not apply)
    _wrong(lc.check_order(lay, lc.emulate_order(lay, unstable=True)), (lc.order_id(case), 'unstable order'))


def test_live_reference_and_checker():
    for n, kind in lc.LIVE[:5]:
        tok, tgt, act0 = lc.live_inputs(n, kind)
        ref = lc.live_reference(tok, tgt)
        assert ref.tolist() == [i for i in range(n) if tok[i] != 0 and tgt[i] > 0]
        act = act0.copy()
        act[:ref.size] = ref
        assert lc.check_live(tok, tgt, act0, ref.size, act).ok
        assert not lc.check_live(tok, tgt, act0, ref.size + 1, act).ok
        bad = act.copy()
        bad[ref.size] = 0                                       # act[count] written
        assert not lc.check_live(tok, tgt, act0, ref.size, bad).ok
        if n > 1000:
            assert 0 < ref.size < n and (tok == 0).any() and (tgt == 0).any() and (tgt < 0).any() and ((tok != 0) & (tgt <= 0)).any()


@pytest.mark.parametrize("case", lc.SUM, ids=[lc.sum_id(c) for c in lc.SUM])
def test_sum_checker_passes_the_contract_and_fails_the_inverse_permutation(case):
    lay = lc.sum_layout(case)
    good = lc.emulate_sum(lay)
    assert lc.check_sum(lay, good).ok
    idx = lay.out_index(np.arange(case.rows))
    # the same by a plain loop over candidates
    for r in range(0, case.rows, 7):
        s = np.float32(0)
        for t in range(case.T):
            hit = np.flatnonzero(lay.act == t * case.rows + r)
            if hit.size:
                s = np.float32(s + lay.nll[hit[0]])
        cand = r if lay.perm is None else int(lay.perm[r])
        assert good[idx[cand]].view(np.uint32) == np.float32(np.float32(0) - s).view(np.uint32)
    if case.empty or case.T == 0:
        assert (good[idx].view(np.uint32) == 0).all()                                       # all +0
    bad = good.copy()
    bad[idx[-1] + 1] = 0.0
    _wrong(lc.check_sum(lay, bad), 'guard')
    if lay.perm is None or case.rows == 1 or case.empty or case.T == 0:
        return                                                 # (no permutation, one row, or all scores +0: the mutant does not apply)
    _wrong(lc.check_sum(lay, lc.emulate_sum(lay, inverse=True)), (lc.sum_id(case), 'perm applied as its inverse'))
