"""tests/gemm_cases.py checked without a GPU: every case reaches the kernel family (and the K-range lengths) it names under the restated
dispatch, the table covers what it promises, the restated C predicates still read as recorded here, the fp64 reference is torch's, and
the checker passes a correct float32 product and fails each of a set of subtly wrong ones."""
import os
import re

import numpy as np
import pytest
import torch

import gemm_cases as gc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'visdial_amd', 'csrc')
IDS = [c.id for c in gc.CASES]


# ------------------------------------------------------------------------------------------------------------ family reached, coverage
@pytest.mark.parametrize("case", gc.CASES, ids=IDS)
def test_case_reaches_the_family_it_names(case):
    p = case.path
    assert p.family == case.family, (case.id, p)
    if case.ktiles is not None:
        assert p.ktiles == case.ktiles, (case.id, p.ktiles)
    if p.ktiles is not None:                                   # the LDS-DMA pipelines move whole 16-row tiles
        assert all(r % 16 == 0 and r > 0 for r in p.krows[:len(p.ktiles)])


def test_named_k_ranges_are_the_ones_the_issue_derives():
    assert gc.path_nt(1025, 770, 1040, 1048, 1044, accumulate=2).krows == (528, 512)
    assert gc.path_nt(1025, 770, 1040, 1048, 1044, accumulate=1).family == 'glds'               # only atomic accumulation splits K
    assert gc.path_tn(128, 256, 1040, 136, 260).krows == (528, 512)
    assert gc.path_tn(130, 300, 2500, 140, 304).krows == (848, 848, 804)
    assert gc.path_tn(128, 128, 65552, 136, 132).krows[-2:] == (1024, 16) and len(gc.path_tn(128, 128, 65552, 136, 132).krows) == 65
    assert gc.path_tn(128, 128, 65568, 136, 132).krows[-1] == 32
    assert gc.path_tn(128, 128, 1029, 136, 132).krows == (1024, 5)
    assert gc.path_tn(256, 128, 8197, 264, 132, gc.FLAG_SPLIT9).krows == (8192, 5)
    # the shapes of tests/test_ops_gpu.py::test_gemm_nt, as its comment now says
    fam = lambda M, N, K: gc.path_nt(M, N, K, K, K, 0, True, 0)
    assert [fam(*s).family for s in [(200, 512, 512), (260, 300, 300), (33, 40, 4), (1, 512, 2048), (1500, 300, 64), (1025, 44, 80)]] == ['small'] * 6
    assert fam(3920, 512, 512) == gc.Path('glds', (32,), (512,)) and fam(11323, 300, 2048).ktiles == (128,)
    assert fam(5000, 2048, 300).family == 'staged'


def test_table_covers_what_it_promises():
    C = gc.CASES
    assert gc.REQUIRED <= set((c.entry, c.family) for c in C)
    assert all(c.lda > c.wa and c.ldb > c.wb and c.ldc > c.N for c in C)                      # ld > width everywhere
    assert all(c.lda % 4 == 0 and c.ldb % 4 == 0 and gc.OFF % 4 == 0 and gc.OFF > 0 for c in C)   # 16-byte aligned views at a column offset
    assert any(c.entry == 'nt' and c.N % 4 for c in C)
    for r in (1, 2, 3):                                        # each ragged K of NN on rows padded exactly and more than exactly
        assert any(c.entry == 'nn' and c.K % 4 == r and c.lda == gc.ceil4(c.K) for c in C), r
        assert any(c.entry == 'nn' and c.K % 4 == r and c.lda > gc.ceil4(c.K) for c in C), r
        assert any(c.entry == 'nn' and c.K % 4 == r and c.family == 'staged' for c in C), r
    assert any(c.entry == 'tn' and c.M % 4 and c.N % 4 and c.lda == gc.ceil4(c.M) and c.ldb == gc.ceil4(c.N) for c in C)
    assert any(c.entry == 'tn' and c.M % 4 and c.lda > gc.ceil4(c.M) for c in C)
    assert any(c.entry == 'rows' and c.M % 4 and c.N % 4 for c in C)
    assert set(c.ktiles for c in C if c.entry == 'nt' and c.family == 'glds') == {(4,), (5,), (6,)}
    assert set(c.ktiles[-1] for c in C if c.entry == 'tn' and c.family == 'kmajor' and len(c.ktiles) > 2) == {1, 2}
    for fam in ('small', 'staged', 'glds'):                    # the whole epilogue grid on one shape per family
        full = set((c.bias, c.act, c.accumulate) for c in C if c.entry == 'nt' and c.family == fam)
        assert full >= set((b, t, a) for b in (0, 1) for t in (0, 1) for a in (0, 1)) | {(0, 0, 2)}, fam
    for fam in ('small', 'staged'):
        assert set((c.bias, c.accumulate) for c in C if c.entry == 'nn' and c.family == fam) == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(c.K == 0 for c in C if c.entry == 'nt') and any(c.K == 0 for c in C if c.entry == 'nn') and any(c.K == 0 for c in C if c.entry == 'tn')
    assert sorted(set((c.row_tile, c.M) for c in C if c.entry == 'live')) == sorted(gc.LIVE_SHAPES)
    assert [gc.cdiv(M, t) for t, M in gc.LIVE_SHAPES] == [1, 8, 9, 2, 9]
    assert gc.live_prefixes(270, 32) == [0, 1, 32, 33, 270] and gc.live_prefixes(20, 32) == [0, 1, 20]
    assert max(c.rows_a * c.lda + c.rows_b * c.ldb for c in C) * 4 < 80e6                     # the largest case moves about 70 MB


# ------------------------------------------------------------------------------------------------------------ tripwire on the C text
NAMES = r'(?:splits|kchunk|max_splits|K1|kmaj|tiles|grid)'


def _code(path):
    src = open(os.path.join(CSRC, path)).read()
    src = re.sub(r'/\*.*?\*/', ' ', src, flags=re.S)
    return re.sub(r'//[^\n]*', ' ', src)


def _body(src, head):
    """the brace-matched body of the function whose definition matches `head`"""
    m = re.search(head, src)
    assert m, head
    i = src.index('{', src.index(')', m.end()))
    depth, j = 0, i
    while True:
        depth += {'{': 1, '}': -1}.get(src[j], 0)
        j += 1
        if depth == 0:
            return src[i + 1:j - 1]


def _closing(s, i):
    depth = 0
    while True:
        depth += {'(': 1, ')': -1}.get(s[i], 0)
        i += 1
        if depth == 0:
            return i


def _predicates(body, returns=False):
    """in source order: the condition of every `if`, every statement that assigns one of the dispatch variables (and every `return`
    of a one-line predicate), whitespace-normalised"""
    found = [(m.start(), 'if ' + body[m.end() - 1:_closing(body, m.end() - 1)]) for m in re.finditer(r'\bif\s*(?:constexpr\s*)?\(', body)]
    found += [(m.start(1), m.group(1)) for m in re.finditer(r'(?:(?<=[;{})])|(?<=\belse))\s*((?:const |static )?(?:int |long |bool )?%s\s*=[^=;][^;]*;)' % NAMES, body)]
    if returns:
        found += [(m.start(), m.group(0)) for m in re.finditer(r'\breturn\b[^;]*;', body)]
    return [' '.join(t.split()) for _, t in sorted(found)]


def dispatch_text():
    ops, core, paths = _code('gemm_ops.hip'), _code('gemm_core.h'), _code('paths.h')
    return {
        'use_small': _predicates(_body(ops, r'static inline bool use_small\('), True),
        'vd_tn_kmajor_fits': _predicates(_body(paths, r'static inline bool vd_tn_kmajor_fits\('), True),
        'vd_tn_split_tiles': _predicates(_body(paths, r'static inline bool vd_tn_split_tiles\('), True),
        'vd_gemm_nt': _predicates(_body(ops, r'\bint vd_gemm_nt\(')),
        'vd_gemm_nn': _predicates(_body(ops, r'\bint vd_gemm_nn\(')),
        'vd_gemm_nn_live_p': _predicates(_body(ops, r'\bint vd_gemm_nn_live_p\(')),
        'vd_gemm_tn_acc': _predicates(_body(ops, r'\bint vd_gemm_tn_acc\(')),
        'vd_gemm_tn_rows_acc': _predicates(_body(ops, r'\bint vd_gemm_tn_rows_acc\(')),
        'launch_gemm_glds': _predicates(_body(core, r'static int launch_gemm_glds\(')),
        'launch_gemm': _predicates(_body(core, r'static int launch_gemm\(')),
    }


RECORDED = {
    'use_small': [
        'return (long)vd_cdiv(M, CfgBig::BM) * vd_cdiv(N, CfgBig::BN) < 48;',
    ],
    'vd_tn_kmajor_fits': [
        'return M % 128 == 0 && N % 128 == 0 && K >= 1024;',
    ],
    'vd_tn_split_tiles': [
        'return M % VD_SPLIT_TN_BM == 0 && N % VD_SPLIT_TN_BN == 0;',
    ],
    'vd_gemm_nt': [
        'if (int rc = check_align(A, lda, "vd_gemm_nt A"))',
        'if (int rc = check_align(W, ldw, "vd_gemm_nt W"))',
        'if (use_small(M, N))',
        'if (M >= 1024 && K >= 64 && K % 16 == 0 && (long)M * lda * 4 < (1L << 32) && (long)N * ldw * 4 < (1L << 32))',
        'int splits = 1;',
        'const long tiles = (long)vd_cdiv(M, 128) * vd_cdiv(N, 128);',
        'if (accumulate == 2 && !bias && act == VD_ACT_NONE && tiles < 512 && K >= 1024)',
        'splits = (int)vd_cdiv(768, tiles);',
        'if (splits > K / 512)',
        'splits = K / 512;',
    ],
    'vd_gemm_nn': [
        'if (int rc = check_align(A, lda, "vd_gemm_nn A"))',
        'if (int rc = check_align(B, ldb, "vd_gemm_nn B"))',
        'if (use_small(M, N))',
    ],
    'vd_gemm_nn_live_p': [
        'if (int rc = check_align(A, lda, "vd_gemm_nn (live rows) A"))',
        'if (int rc = check_align(B, ldb, "vd_gemm_nn (live rows) B"))',
        'if (row_tile == CfgSmall::BM)',
    ],
    'vd_gemm_tn_acc': [
        'if (int rc = check_align(A, lda, "vd_gemm_tn_acc A"))',
        'if (int rc = check_align(B, ldb, "vd_gemm_tn_acc B"))',
        'if (K == 0)',
        'const long tiles = (long)vd_cdiv(M, CfgBig::BM) * vd_cdiv(N, CfgBig::BN);',
        'if ((flags & VD_FLAG_SPLIT9) && !(flags & VD_FLAG_BF16) && vd_tn_split_tiles(M, N) && K >= 8192 && 16L * lda * 4 < (1L << 31) && 16L * ldb * 4 < (1L << 31))',
        'const int K1 = K & ~15;',
        'if (int rc = launch_gemm_split_tn<9>(M, N, K1, A, lda, B, ldb, C, ldc, (hipStream_t)stream))',
        'if (K1 == K)',
        'const bool kmaj = !(flags & VD_FLAG_BF16) && vd_tn_kmajor_fits(M, N, K);',
        'if (kmaj && K % 16 != 0)',
        'const int K1 = K & ~15;',
        'if (int rc = vd_gemm_tn_acc(A, lda, B, ldb, C, ldc, M, N, K1, flags, stream))',
        'long splits = vd_cdiv(768, tiles);',
        'const long max_splits = vd_cdiv(K, 1024);',
        'if (splits > max_splits)',
        'splits = max_splits;',
        'if (splits < 1)',
        'splits = 1;',
        'if (flags & VD_FLAG_BF16)',
        'if (M % 128 == 0 && N % 128 == 0 && K >= 32 && lda == M && ldb == N && (long)32 * N * 2 + 256 < (1L << 31))',
        'if (a16 && b16)',
        'const int K1 = K & ~31;',
        'if (int rc = launch_gemm_bf16_tn_tr(a16, b16, C, ldc, M, N, K1, (hipStream_t)stream))',
        'if (K1 == K)',
        'if (vd_tn_split_tiles(M, N) && K >= 1024 && lda % 4 == 0 && ldb % 4 == 0 && 16L * lda * 4 < (1L << 31) && 16L * ldb * 4 < (1L << 31))',
        'const int K1 = K & ~15;',
        'if (int rc = launch_gemm_split_tn<1>(M, N, K1, A, lda, B, ldb, C, ldc, (hipStream_t)stream))',
        'if (K1 == K)',
        'if (kmaj)',
    ],
    'vd_gemm_tn_rows_acc': [
        'if (int rc = check_align(A, lda, "vd_gemm_tn_rows_acc A"))',
        'if (int rc = check_align(B, ldb, "vd_gemm_tn_rows_acc B"))',
        'if (K == 0)',
        'const long tiles = (long)vd_cdiv(M, Cfg::BM) * vd_cdiv(N, Cfg::BN);',
        'long splits = vd_cdiv(768, tiles);',
        'const long max_splits = vd_cdiv(K, 1024);',
        'if (splits > max_splits)',
        'splits = max_splits;',
        'if (splits < 1)',
        'splits = 1;',
    ],
    'launch_gemm_glds': [
        'if (M <= 0 || N <= 0)',
        'if (KMAJ)',
        'int kchunk = vd_cdiv(vd_cdiv(K, splits), 16) * 16;',
        'if (kchunk < 16)',
        'kchunk = 16;',
        'splits = vd_cdiv(K, kchunk);',
        'if (!attr_set)',
        'int grid = tiles_m * tiles_n * splits;',
        'if (EpiDeadOf<Epi>::value)',
        'grid = (tiles_m + 7) / 8 * 8 * tiles_n;',
    ],
    'launch_gemm': [
        'if (M <= 0 || N <= 0)',
        'if (splits < 1)',
        'splits = 1;',
        'int kchunk = K > 0 ? vd_cdiv(vd_cdiv(K, splits), Cfg::BK) * Cfg::BK : Cfg::BK;',
        'if (K > 0)',
        'splits = vd_cdiv(K, kchunk);',
        'splits = 1;',
        'if (!attr_set)',
        'int grid = tiles_m * tiles_n * splits;',
        'if (EpiDeadOf<Epi>::value)',
        'grid = (tiles_m + 7) / 8 * 8 * tiles_n;',
    ],
}


def test_dispatch_predicates_read_as_recorded():
    """the predicates gemm_cases.py restates -- use_small, the `if` chains and split arithmetic of the entry points, launch_gemm_glds's and
    launch_gemm's kchunk lines, the two shape predicates of paths.h -- as whitespace-normalised text"""
    now = dispatch_text()
    for name in RECORDED:
        assert now[name] == RECORDED[name], (
            "the dispatch of %s changed: restate it in tests/gemm_cases.py (path_* and the comments that quote the C lines), re-derive the "
            "case table's families and K ranges, correct the comment above test_gemm_nt in tests/test_ops_gpu.py if its shapes moved, then "
            "record the new text here.  Now:\n%s" % (name, '\n'.join(now[name])))
    assert set(now) == set(RECORDED)


# ------------------------------------------------------------------------------------------------------------ the reference and the checker
CPU_FLOPS = 2e9                                                # cases below this run in well under a second here
SMALL = [c for c in gc.CASES if c.flops <= CPU_FLOPS]
assert set((c.entry, c.family) for c in SMALL) == gc.REQUIRED   # only the two 65 000-row contractions are left out


@pytest.mark.parametrize("case", SMALL, ids=[c.id for c in SMALL])
def test_reference_is_torch_matmul_in_float64(case):
    lay = gc.layout(case)
    ref, mag = gc.reference(lay)
    a, b = lay.valid()
    t = torch.matmul(torch.from_numpy(np.ascontiguousarray(a)).double(), torch.from_numpy(np.ascontiguousarray(b)).double())
    if case.bias:
        t = t + torch.from_numpy(lay.bias[:case.N]).double()
    if case.act:
        t = torch.tanh(t)
    if case.accumulate:
        t = t + torch.from_numpy(np.ascontiguousarray(lay.c0())).double()
    assert ref.shape == (case.M, case.N) and np.isfinite(ref).all() and np.isfinite(mag).all()
    scale = max(1.0, float(np.abs(mag).max())) if mag.size else 1.0
    assert ref.size == 0 or float(np.abs(ref - t.numpy()).max()) <= 1e-13 * scale


def _wrong(lay, ref, mag, buf, why):
    v = gc.check(lay, buf, ref, mag)
    assert not v.ok, (lay.case.id, why)
    return v


@pytest.mark.parametrize("case", SMALL, ids=[c.id for c in SMALL])
def test_checker_passes_a_float32_product_and_fails_the_mutants(case):
    c, lay = case, gc.layout(case)
    ref, mag = gc.reference(lay)
    good = gc.emulate(lay)
    v = gc.check(lay, good, ref, mag)
    assert v.ok, (c.id, v.failures)
    if c.exact and c.K > 0:
        assert 0 < v.bound_ratio <= 1.0
    a, b = lay.valid()
    if c.M == 0 or c.N == 0:
        return
    # one guard element overwritten: a pad column of the last row, the row behind the last, the trailing guard
    for idx in (gc.OFF + (c.M - 1) * c.ldc + c.N, gc.OFF + c.M * c.ldc, good.size - 1):
        bad = good.copy()
        bad[idx] = 0.0
        assert any('guard' in f for f in _wrong(lay, ref, mag, bad, 'guard').failures)
    # a NaN in the result
    bad = good.copy()
    lay.result(bad)[c.M - 1, c.N - 1] = np.nan
    _wrong(lay, ref, mag, bad, 'nan')
    if c.bias:                                                 # bias added twice
        _wrong(lay, ref, mag, gc.emulate(lay, bias_times=2), 'bias twice')
    if c.K == 0:
        return
    if c.exact:
        # one k term dropped in one output element (the last one: the ragged corner), the largest term of its dot product
        i, j = c.M - 1, c.N - 1
        terms = a[i, :].astype(np.float64) * b[:, j].astype(np.float64)
        bad = good.copy()
        lay.result(bad)[i, j] = np.float32(lay.result(good)[i, j] - terms[np.argmax(np.abs(terms))])
        assert any('elementwise' in f for f in _wrong(lay, ref, mag, bad, 'dropped term').failures)
    if c.entry in ('nn', 'live') and c.K % 4:
        # the finite pad column [K, ceil4(K)) of A multiplied by a B row that is not zero
        pad = gc.view(lay.A, c.rows_a, c.lda)[:, c.K:c.K + 1]
        _wrong(lay, ref, mag, gc.emulate(lay, extra=pad * b[:1, :]), 'pad column used')
    if c.rows_a > 1 and c.entry != 'rows':
        # the operand read with ld = width: rows run into each other and into what the stride skips
        packed = lay.A[gc.OFF:gc.OFF + c.rows_a * c.wa].reshape(c.rows_a, c.wa)
        with np.errstate(all='ignore'):
            _wrong(lay, ref, mag, gc.emulate(lay, A=packed if c.entry in ('nt', 'nn', 'live') else packed.T), 'ld = width')
    if c.entry == 'rows':
        # A walked with B's index list
        A = gc.view(lay.A, c.rows_a, c.lda)[:, :c.wa]
        _wrong(lay, ref, mag, gc.emulate(lay, A=A[lay.rb].T), 'index lists swapped')
    if c.M == c.N and c.M > 1 and c.flags == 0:
        # A and B swapped on a square case: the transposed product
        _wrong(lay, ref, mag, gc.emulate(lay, A=b.T, B=a.T), 'operands swapped')


def test_a_square_case_exists_for_the_swap_mutant():
    assert any(c.M == c.N and c.M > 1 and c.flags == 0 for c in SMALL)


def test_bf16_bound_is_the_projects_and_holds_for_rounded_operands():
    """FLAG_BF16 is held to rel-L2 1e-2: operands rounded to bf16 (unit roundoff 2^-9) pass, operands with an exponent bit flipped do not"""
    case = [c for c in gc.CASES if c.flags & gc.FLAG_BF16][0]
    lay = gc.layout(case)
    a, b = lay.valid()
    rnd = lambda x: torch.from_numpy(np.ascontiguousarray(x)).bfloat16().float().numpy()
    assert case.rel_bound == 1e-2 and not case.exact
    assert gc.check(lay, gc.emulate(lay, A=rnd(a), B=rnd(b))).ok
    assert not gc.check(lay, gc.emulate(lay, A=rnd(a) * 2, B=rnd(b))).ok
