"""Case table, fp64 reference and checker for the GEMM entry points of csrc/gemm_ops.hip (no GPU needed).

  * `path_*`: the dispatch of vd_gemm_nt / vd_gemm_nn / vd_gemm_nn_live_p / vd_gemm_tn_acc / vd_gemm_tn_rows_acc RESTATED -- which kernel
    family a call runs and how long its K ranges are -- the same arrangement as ops.lstm_fwd_row_tile.  tests/test_gemm_cases_cpu.py holds
    the text of the C predicates it restates (a change there fails that test until this file and the table follow).
  * `CASES`: every case names the family it is meant to reach (and, where that is the point, the K-range lengths in 16-row tiles).
  * `Layout`: the operands of a case as the runtime passes them -- views at a column offset into wider buffers, a leading dimension larger
    than the width, NaN in everything the contract says is never used, a large finite mark in the pad columns it requires to be finite, the
    output in front of marked columns, rows and a trailing guard.
  * `reference` (fp64 numpy on the valid sub-blocks, pinned to torch.matmul by the CPU test) and `check` (pass / fail of a result).

Bounds.  rel-L2 < 1e-5 against fp64 is what tests/test_ops_gpu.py holds these entry points to (1e-2 under FLAG_BF16).  The elementwise
bound  |got - ref| <= (K + 4) * 2^-24 * (|A|.|B| + |bias| + |C0|)  is the forward error of a length-K fp32 dot product in ANY summation
order (every partial sum is a rounded sum of roundings of the terms: at most K roundings on the path of a term, unit roundoff 2^-24),
plus the bias add, the accumulation into C0, and the final store: it covers split-K and float atomics.  It applies to the exact-fp32 paths
without tanh; not to split9 / bf16.  It is derived, not measured."""
import collections
import functools

import numpy as np

FLAG_BF16, FLAG_SPLIT9 = 1, 2            # include/visdial_hip.h VD_FLAG_BF16 / VD_FLAG_SPLIT9
BM = BN = 128                            # gemm_ops.hip CfgBig (and the LDS-DMA configuration)
SMALL_TILE = 32                          # gemm_ops.hip CfgSmall::BM
U = 2.0 ** -24                           # fp32 unit roundoff
REL_L2, REL_L2_BF16 = 1e-5, 1e-2
OFF = 4                                  # column offset of every operand and of C inside its buffer, floats
TAIL = 64                                # trailing elements behind every buffer (NaN behind operands, MARK behind C)
PAD = np.float32(3e18)                   # pad columns the contract requires to be finite
MARK = np.float32(-7.25e3)               # what C's buffer holds wherever a call must not write

Path = collections.namedtuple('Path', 'family ktiles krows')     # ktiles: K-range lengths in 16-row tiles (LDS-DMA pipelines), krows: in rows


def cdiv(a, b):
    return (a + b - 1) // b


def ceil4(x):
    return cdiv(x, 4) * 4


# ------------------------------------------------------------------------------------------------------------ the restated dispatch
def use_small(M, N):
    # gemm_ops.hip use_small: (long)vd_cdiv(M, CfgBig::BM) * vd_cdiv(N, CfgBig::BN) < 48
    return cdiv(M, BM) * cdiv(N, BN) < 48


def _ranges(K, kchunk):
    return tuple(min(K, s + kchunk) - s for s in range(0, K, kchunk))


def glds_ranges(K, splits):
    # gemm_core.h launch_gemm_glds: kchunk = vd_cdiv(vd_cdiv(K, splits), 16) * 16; if (kchunk < 16) kchunk = 16; splits = vd_cdiv(K, kchunk);
    # kernel: ks = split * kchunk, ke = min(K, ks + kchunk), nk = (ke - ks) / 16
    kchunk = max(16, cdiv(cdiv(K, splits), 16) * 16)
    return _ranges(K, kchunk)


def staged_ranges(K, splits, BK=16):
    # gemm_core.h launch_gemm: kchunk = K > 0 ? vd_cdiv(vd_cdiv(K, splits), Cfg::BK) * Cfg::BK : Cfg::BK; splits = vd_cdiv(K, kchunk) (1 at K = 0)
    if K == 0:
        return (0,)
    return _ranges(K, cdiv(cdiv(K, max(1, splits)), BK) * BK)


def _tiles16(krows):
    return tuple(r // 16 for r in krows)


def path_nt(M, N, K, lda, ldw, accumulate=0, bias=False, act=0):
    """vd_gemm_nt: small | staged | glds | glds-splitk"""
    if use_small(M, N):                                                    # if (use_small(M, N)) launch_gemm<CfgSmall>
        return Path('small', None, staged_ranges(K, 1, 128))
    # if (M >= 1024 && K >= 64 && K % 16 == 0 && (long)M * lda * 4 < (1L << 32) && (long)N * ldw * 4 < (1L << 32))
    if M >= 1024 and K >= 64 and K % 16 == 0 and M * lda * 4 < 2 ** 32 and N * ldw * 4 < 2 ** 32:
        splits = 1
        tiles = cdiv(M, 128) * cdiv(N, 128)
        # if (accumulate == 2 && !bias && act == VD_ACT_NONE && tiles < 512 && K >= 1024) { splits = vd_cdiv(768, tiles);
        #   if (splits > K / 512) splits = K / 512; }
        if accumulate == 2 and not bias and act == 0 and tiles < 512 and K >= 1024:
            splits = min(cdiv(768, tiles), K // 512)
        kr = glds_ranges(K, splits)
        return Path('glds-splitk' if len(kr) > 1 else 'glds', _tiles16(kr), kr)
    return Path('staged', None, staged_ranges(K, 1))                        # launch_gemm<CfgBig>


def path_nn(M, N, K):
    """vd_gemm_nn: small | staged"""
    if use_small(M, N):                                                    # if (use_small(M, N)) launch_gemm<CfgSmall>
        return Path('small', None, staged_ranges(K, 1, 128))
    return Path('staged', None, staged_ranges(K, 1))                        # launch_gemm<CfgBig>


def path_nn_live(M, N, K, row_tile):
    """vd_gemm_nn_live_p: the caller names the row tile -- if (row_tile == CfgSmall::BM) CfgSmall, else CfgBig"""
    assert row_tile in (SMALL_TILE, BM)
    return Path('small' if row_tile == SMALL_TILE else 'staged', None, staged_ranges(K, 1, 128 if row_tile == SMALL_TILE else 16))


def tn_kmajor_fits(M, N, K):
    # paths.h vd_tn_kmajor_fits: M % 128 == 0 && N % 128 == 0 && K >= 1024
    return M % 128 == 0 and N % 128 == 0 and K >= 1024


def tn_split_tiles(M, N):
    # paths.h vd_tn_split_tiles: M % VD_SPLIT_TN_BM (256) == 0 && N % VD_SPLIT_TN_BN (128) == 0
    return M % 256 == 0 and N % 128 == 0


def _tn_splits(M, N, K):
    # long splits = vd_cdiv(768, tiles); max_splits = vd_cdiv(K, 1024); if (splits > max_splits) splits = max_splits; if (splits < 1) splits = 1;
    tiles = cdiv(M, BM) * cdiv(N, BN)
    return max(1, min(cdiv(768, tiles), cdiv(K, 1024)))


def path_tn(M, N, K, lda, ldb, flags=0, shadows=False):
    """vd_gemm_tn_acc: noop (K == 0) | staged | kmajor | kmajor+tail | split9 | split9+tail | bf16-staged (| bf16-split1 | bf16-tr, the
    two bf16 contractions of 128 / 256-row tiles: tests/test_ops_gpu.py)"""
    if K == 0:                                                             # if (K == 0) return VD_OK;
        return Path('noop', None, ())
    # if ((flags & VD_FLAG_SPLIT9) && !(flags & VD_FLAG_BF16) && vd_tn_split_tiles(M, N) && K >= 8192 && 16L * lda * 4 < (1L << 31) &&
    #     16L * ldb * 4 < (1L << 31)): K1 = K & ~15 rows through launch_gemm_split_tn<9>, the rest through the staged kernel
    if flags & FLAG_SPLIT9 and not flags & FLAG_BF16 and tn_split_tiles(M, N) and K >= 8192 and 16 * lda * 4 < 2 ** 31 and 16 * ldb * 4 < 2 ** 31:
        return Path('split9' if K % 16 == 0 else 'split9+tail', None, (K & ~15,) + ((K & 15,) if K & 15 else ()))
    kmaj = not flags & FLAG_BF16 and tn_kmajor_fits(M, N, K)                # const bool kmaj = !(flags & VD_FLAG_BF16) && vd_tn_kmajor_fits(M, N, K);
    if kmaj and K % 16 != 0:                                               # if (kmaj && K % 16 != 0): K1 = K & ~15 by recursion, then the tail
        head = path_tn(M, N, K & ~15, lda, ldb, flags)
        assert head.family == 'kmajor'
        return Path('kmajor+tail', head.ktiles, head.krows + (K & 15,))
    splits = _tn_splits(M, N, K)
    if flags & FLAG_BF16:                                                  # if (flags & VD_FLAG_BF16)
        # if (M % 128 == 0 && N % 128 == 0 && K >= 32 && lda == M && ldb == N && ...) and both shadows registered
        if M % 128 == 0 and N % 128 == 0 and K >= 32 and lda == M and ldb == N and shadows:
            return Path('bf16-tr', None, None)
        # if (vd_tn_split_tiles(M, N) && K >= 1024 && lda % 4 == 0 && ldb % 4 == 0 && 16L * lda * 4 < (1L << 31) && 16L * ldb * 4 < (1L << 31))
        if tn_split_tiles(M, N) and K >= 1024 and lda % 4 == 0 and ldb % 4 == 0 and 16 * lda * 4 < 2 ** 31 and 16 * ldb * 4 < 2 ** 31:
            return Path('bf16-split1', None, None)
        return Path('bf16-staged', None, staged_ranges(K, splits, 32))      # launch_gemm<GemmCfg<4, 1, 4, 32, 0, 3, 0, 1>>(.., splits, ..)
    if kmaj:                                                               # if (kmaj) launch_gemm_glds<.., true>(M, N, K, splits, ..)
        kr = glds_ranges(K, splits)
        return Path('kmajor', _tiles16(kr), kr)
    return Path('staged', None, staged_ranges(K, splits))                   # launch_gemm<GemmCfg<4, 1, 4, 16, 0, 4, 41984>>(.., splits, ..)


def path_tn_rows(M, N, K):
    """vd_gemm_tn_rows_acc: always the register-staged kernel over the index lists, with vd_gemm_tn_acc's split rule"""
    if K == 0:
        return Path('noop', None, ())
    return Path('staged', None, staged_ranges(K, _tn_splits(M, N, K)))


# ------------------------------------------------------------------------------------------------------------ the case table
class Case(object):
    """entry: nt | nn | live | tn | rows.  K is the contraction length (the number of index pairs for `rows`, whose operands have R rows).
    lda / ldb / ldc default to the smallest multiple of 4 above the width plus a margin that differs between the operands."""

    def __init__(self, entry, M, N, K, family, ktiles=None, lda=None, ldb=None, bias=False, act=0, accumulate=0, flags=0, R=None,
                 row_tile=None):
        self.entry, self.M, self.N, self.K, self.family, self.ktiles = entry, M, N, K, family, ktiles
        self.bias, self.act, self.accumulate, self.flags, self.R, self.row_tile = bool(bias), act, accumulate, flags, R, row_tile
        wa = M if entry in ('tn', 'rows') else K              # width of a row of A / of B
        wb = K if entry == 'nt' else N
        self.wa, self.wb = wa, wb
        self.lda = ceil4(wa) + 8 if lda is None else lda
        self.ldb = ceil4(wb) + 4 if ldb is None else ldb
        self.ldc = ceil4(N) + 12
        if entry in ('tn', 'rows'):
            self.accumulate = 2                                # C += with float atomics
        self.rows_a = {'nt': M, 'nn': M, 'live': M, 'tn': K, 'rows': R}[entry]
        self.rows_b = {'nt': N, 'nn': K, 'live': K, 'tn': K, 'rows': R}[entry]

    @property
    def id(self):
        s = '%s-%s-%dx%dx%d' % (self.entry, self.family, self.M, self.N, self.K)
        s += '-lda%d-ldb%d' % (self.lda, self.ldb)
        if self.entry in ('nt', 'nn'):
            s += '-b%d-t%d-acc%d' % (self.bias, self.act, self.accumulate)
        if self.flags:
            s += '-f%d' % self.flags
        if self.R is not None:
            s += '-R%d' % self.R
        if self.row_tile is not None:
            s += '-tile%d' % self.row_tile
        return s

    @property
    def path(self):
        c = self
        if c.entry == 'nt':
            return path_nt(c.M, c.N, c.K, c.lda, c.ldb, c.accumulate, c.bias, c.act)
        if c.entry == 'nn':
            return path_nn(c.M, c.N, c.K)
        if c.entry == 'live':
            return path_nn_live(c.M, c.N, c.K, c.row_tile)
        if c.entry == 'tn':
            return path_tn(c.M, c.N, c.K, c.lda, c.ldb, c.flags)
        return path_tn_rows(c.M, c.N, c.K)

    @property
    def exact(self):
        """the elementwise bound applies: exact fp32 products, no tanh"""
        return not self.flags and not self.act

    @property
    def rel_bound(self):
        return REL_L2_BF16 if self.flags & FLAG_BF16 else REL_L2

    @property
    def flops(self):
        return 2 * self.M * self.N * self.K

    @property
    def atomic(self):
        return self.accumulate == 2


def _epilogues():
    """bias x act x accumulate 0 / 1, and accumulate = 2 the way the runtime calls it (no bias, no activation)"""
    return [dict(bias=b, act=t, accumulate=a) for b in (1, 0) for t in (0, 1) for a in (0, 1)] + [dict(bias=0, act=0, accumulate=2)]


def _nt_cases():
    plain = dict(bias=1, act=0, accumulate=0)
    out = []
    # small: CfgSmall has BK = 128 with a 4-way intra-block split: K below one wave's slice, one tile, one tile + 4, three tiles
    out += [Case('nt', 1, 1, 4, 'small', **plain)]
    out += [Case('nt', 33, 30, 8, 'small', **e) for e in _epilogues()]
    out += [Case('nt', 130, 258, K, 'small', **plain) for K in (36, 128, 132, 300)]
    out += [Case('nt', 5, 8, 0, 'small', **e) for e in (plain, dict(bias=1, act=1, accumulate=0), dict(bias=0, act=0, accumulate=1))]
    # staged (CfgBig): M < 1024; K < 64; K % 16 != 0
    out += [Case('nt', 900, 898, 20, 'staged', **e) for e in _epilogues()]
    out += [Case('nt', 1025, 770, 60, 'staged', **plain), Case('nt', 1025, 770, 68, 'staged', **plain)]
    # glds: 9 x 7 tiles, a one-row last row tile, a two-column last column tile, N % 4 == 2; 4 / 5 / 6 K tiles against 3 A and 2 B buffers
    out += [Case('nt', 1025, 770, 64, 'glds', (4,), **plain), Case('nt', 1025, 770, 96, 'glds', (6,), **plain)]
    out += [Case('nt', 1025, 770, 80, 'glds', (5,), **e) for e in _epilogues()]
    out += [Case('nt', 1025, 770, 1040, 'glds-splitk', (33, 32), bias=0, act=0, accumulate=2)]
    return out


def _nn_cases():
    grid = [dict(bias=b, accumulate=a) for b in (1, 0) for a in (0, 1)]
    plain = grid[0]
    out = []
    out += [Case('nn', 7, 8, 5, 'small', lda=lda, **e) for lda in (8, 16) for e in grid]            # K % 4 == 1
    out += [Case('nn', 7, 8, K, 'small', lda=lda, **plain) for K in (6, 7) for lda in (8, 16)]      # K % 4 == 2, 3
    out += [Case('nn', 51, 2048, 13, 'small', lda=16, **plain), Case('nn', 51, 2048, 12, 'small', **plain)]
    out += [Case('nn', 5, 8, 0, 'small', **e) for e in (plain, dict(bias=0, accumulate=1))]
    out += [Case('nn', 900, 1024, 18, 'staged', lda=lda, **e) for lda, es in ((20, grid), (28, [plain])) for e in es]
    out += [Case('nn', 900, 1024, 130, 'staged', lda=132, **plain), Case('nn', 900, 1024, 19, 'staged', lda=20, **plain),
            Case('nn', 900, 1024, 17, 'staged', lda=24, **plain)]
    return out


LIVE_SHAPES = [(32, 20), (32, 256), (32, 270), (128, 130), (128, 1100)]       # (row tile, M): 1, 8, 9 small tiles; 2, 9 big tiles


def live_prefixes(M, tile):
    return sorted(set(min(L, M) for L in (0, 1, tile, tile + 1, M)))


def _live_cases():
    return [Case('live', M, 128, K, 'small' if tile == 32 else 'staged', bias=1, row_tile=tile) for tile, M in LIVE_SHAPES for K in (12, 30)]


def _tn_cases():
    return [
        Case('tn', 10, 6, 37, 'staged', lda=12, ldb=8),                     # M % 4 == 2, N % 4 == 2 on rows padded to ceil4
        Case('tn', 130, 300, 2500, 'staged'),                               # three K ranges, the last ragged (848 + 848 + 804)
        Case('tn', 10, 6, 0, 'noop', lda=12, ldb=8),
        Case('tn', 128, 128, 1024, 'kmajor', (64,)),
        Case('tn', 128, 256, 1040, 'kmajor', (33, 32)),
        Case('tn', 128, 128, 65552, 'kmajor', (64,) * 64 + (1,)),           # the last range one K tile
        Case('tn', 128, 128, 65568, 'kmajor', (64,) * 64 + (2,)),           # two
        Case('tn', 128, 128, 1029, 'kmajor+tail', (64,)),
        Case('tn', 256, 128, 8192, 'split9', flags=FLAG_SPLIT9),
        Case('tn', 256, 128, 8197, 'split9+tail', flags=FLAG_SPLIT9),
        Case('tn', 10, 6, 37, 'bf16-staged', lda=12, ldb=8, flags=FLAG_BF16),
    ]


def _rows_cases():
    return [Case('rows', 10, 6, 77, 'staged', lda=12, ldb=8, R=50), Case('rows', 130, 300, 2500, 'staged', R=400)]


CASES = _nt_cases() + _nn_cases() + _live_cases() + _tn_cases() + _rows_cases()
assert len(set(c.id for c in CASES)) == len(CASES)

# every (entry point, family) pair the table must reach
REQUIRED = {('nt', 'small'), ('nt', 'staged'), ('nt', 'glds'), ('nt', 'glds-splitk'), ('nn', 'small'), ('nn', 'staged'), ('live', 'small'),
            ('live', 'staged'), ('tn', 'staged'), ('tn', 'kmajor'), ('tn', 'kmajor+tail'), ('tn', 'split9'), ('tn', 'split9+tail'),
            ('tn', 'bf16-staged'), ('tn', 'noop'), ('rows', 'staged')}


def cases_of(entry):
    return [c for c in CASES if c.entry == entry]


# ------------------------------------------------------------------------------------------------------------ operands as the runtime passes them
def _operand(rng, rows, width, ld, scale, finite_to):
    """flat buffer [OFF | rows x ld | TAIL] of NaN; row r holds `width` random values at OFF + r * ld, then PAD up to `finite_to`"""
    flat = np.full(OFF + rows * ld + TAIL, np.nan, np.float32)
    v = flat[OFF:OFF + rows * ld].reshape(rows, ld)
    v[:, :width] = rng.randn(rows, width).astype(np.float32) * np.float32(scale)
    v[:, width:finite_to] = PAD
    return flat


def view(flat, rows, ld):
    return flat[OFF:OFF + rows * ld].reshape(rows, ld)


class Layout(object):
    """a case's buffers (numpy float32, flat): A, B, bias (or None), C0; index lists for `rows`; the valid sub-blocks a, b [.. x ..]"""

    def __init__(self, c):
        rng = np.random.RandomState(len(c.id) * 7919 + c.M * 31 + c.N * 17 + c.K + c.lda)
        self.case = c
        # what may be read beyond the width: NN's A up to ceil4(K) (finite), TN's operands up to ceil4(M) / ceil4(N) (finite); nothing else
        fa = ceil4(c.wa) if c.entry in ('nn', 'live', 'tn', 'rows') else c.wa
        fb = ceil4(c.wb) if c.entry in ('tn', 'rows') else c.wb
        self.A = _operand(rng, c.rows_a, c.wa, c.lda, 1.0, fa)
        self.B = _operand(rng, c.rows_b, c.wb, c.ldb, 0.1, fb)
        self.bias = None
        if c.bias:
            self.bias = np.full(c.N + TAIL, np.nan, np.float32)
            self.bias[:c.N] = rng.randn(c.N).astype(np.float32)
        self.ra = self.rb = None
        if c.entry == 'rows':                                  # ordered and repeated indices, different lists for the two operands
            self.ra = np.sort(rng.choice(c.R, size=c.K, replace=c.K > c.R)).astype(np.int32)
            self.rb = np.maximum(self.ra - rng.randint(0, 3, size=c.K), 0).astype(np.int32)
        self.c_rows = c.M + 2                                  # two marked rows behind the last
        self.C0 = np.full(OFF + self.c_rows * c.ldc + TAIL, MARK, np.float32)
        if c.accumulate:
            view(self.C0, self.c_rows, c.ldc)[:c.M, :c.N] = rng.randn(c.M, c.N).astype(np.float32)

    def valid(self, A=None, B=None):
        """(a, b) with the product a @ b: the valid sub-blocks of (A, B), float32"""
        c = self.case
        a = view(self.A if A is None else A, c.rows_a, c.lda)[:, :c.wa]
        b = view(self.B if B is None else B, c.rows_b, c.ldb)[:, :c.wb]
        if c.entry == 'nt':
            return a, b.T
        if c.entry in ('nn', 'live'):
            return a, b
        if c.entry == 'rows':
            return a[self.ra].T, b[self.rb]
        return a.T, b

    def c0(self):
        c = self.case
        return view(self.C0, self.c_rows, c.ldc)[:c.M, :c.N]

    def result(self, Cflat):
        c = self.case
        return view(np.asarray(Cflat), self.c_rows, c.ldc)[:c.M, :c.N]

    def with_result(self, block):
        """C0's buffer with `block` [M x N] stored in the output's place"""
        out = self.C0.copy()
        self.result(out)[...] = block
        return out


@functools.lru_cache(maxsize=2)
def layout(case):
    return Layout(case)


# ------------------------------------------------------------------------------------------------------------ reference and checker
def reference(lay):
    """(ref, mag) in fp64 on the valid sub-blocks: ref = act(a @ b + bias) (+ C0), mag = |a| @ |b| + |bias| + |C0|"""
    c = lay.case
    a, b = lay.valid()
    a, b = a.astype(np.float64), b.astype(np.float64)
    ref = a @ b
    mag = np.abs(a) @ np.abs(b)
    if c.bias:
        ref = ref + lay.bias[:c.N].astype(np.float64)
        mag = mag + np.abs(lay.bias[:c.N].astype(np.float64))
    if c.act:
        ref = np.tanh(ref)
    if c.accumulate:
        ref = ref + lay.c0().astype(np.float64)
        mag = mag + np.abs(lay.c0().astype(np.float64))
    return ref, mag


Verdict = collections.namedtuple('Verdict', 'ok failures rel_l2 bound_ratio')


def guards_intact(lay, Cflat):
    """everything of C's buffer outside C[:M, :N] came back bit for bit"""
    c = lay.case
    before, after = lay.C0.copy(), np.array(Cflat, np.float32, copy=True)
    lay.result(before)[...] = 0
    view(after, lay.c_rows, c.ldc)[:c.M, :c.N] = 0
    bad = np.nonzero(before.view(np.uint32) != after.view(np.uint32))[0]
    return bad


def check(lay, Cflat, ref=None, mag=None, rows=None):
    """pass / fail of the buffer `Cflat` a call left behind.  `rows`: restrict the numeric bounds to these output rows (live-prefix calls)"""
    c = lay.case
    if ref is None:
        ref, mag = reference(lay)
    got = lay.result(Cflat).astype(np.float64)
    sel = slice(None) if rows is None else rows
    g, r, m = got[sel], ref[sel], mag[sel]
    fails = []
    rel, ratio = 0.0, 0.0
    if g.size:
        if not np.isfinite(g).all():
            fails.append('%d non-finite results' % int((~np.isfinite(g)).sum()))
        nr = float(np.linalg.norm(r))
        d = np.where(np.isfinite(g), g - r, np.inf)
        rel = float(np.linalg.norm(d)) / nr if nr > 0 else (0.0 if not np.any(d) else np.inf)
        if not rel < c.rel_bound:
            fails.append('rel-L2 %.3g >= %.0e' % (rel, c.rel_bound))
        if c.exact:
            bound = (c.K + 4) * U * m
            with np.errstate(divide='ignore', invalid='ignore'):
                q = np.where(bound > 0, np.abs(d) / bound, np.where(d == 0, 0.0, np.inf))
            ratio = float(q.max())
            if not ratio <= 1.0:
                i = np.unravel_index(int(np.argmax(q)), q.shape)
                fails.append('elementwise bound exceeded %.3g x at %s (%d elements)' % (ratio, i, int((q > 1.0).sum())))
    bad = guards_intact(lay, Cflat)
    if bad.size:
        fails.append('%d guard elements written, first at flat index %d' % (bad.size, int(bad[0])))
    return Verdict(not fails, fails, rel, ratio)


# ------------------------------------------------------------------------------------------------------------ a numpy fp32 model of a call (CPU tests)
def emulate(lay, A=None, B=None, extra=None, bias_times=1):
    """what a correct kernel leaves in C's buffer, computed with numpy in float32 on the valid sub-blocks; `A` / `B` replace the valid
    blocks (mutants), `extra` [M x N] is added to the product before the epilogue"""
    c = lay.case
    a, b = lay.valid()
    a = a if A is None else A
    b = b if B is None else B
    v = a.astype(np.float32) @ b.astype(np.float32)
    if extra is not None:
        v = v + extra.astype(np.float32)
    if c.bias:
        for _ in range(bias_times):
            v = v + lay.bias[:c.N]
    if c.act:
        v = np.tanh(v)
    if c.accumulate:
        v = v + lay.c0()
    return lay.with_result(v.astype(np.float32))
