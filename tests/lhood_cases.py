"""Case table, fp64 references and checkers for the entry points of csrc/lhood.hip (no GPU needed): the arrangement of tests/gemm_cases.py.

  * `fused_fits`, `head_family`, `prefix_fits`: the dispatch of vd_lhood_nll / vd_lhood_lse_p and the predicate of vd_lhood_order_p
    RESTATED.  tests/test_lhood_cases_cpu.py holds the text of the C predicates (a change there fails that test until this file follows).
  * `HEAD`, `EDGE`, `ORDER`, `LIVE`, `SUM`: the case tables.  A head case runs through vd_lhood_nll AND vd_lhood_lse_p and names the kernel
    family (`mfma` | `rows`) it is meant to reach.
  * `*Layout`: the operands of a case as the runtime may pass them -- h [rows x ldh] and W [V x ldw] inside larger buffers, NaN in every
    row of h that is not listed, in the pad columns [H, ld), and behind h, W, bias and lse; target 0 on unlisted rows; every output in
    front of GUARD marked elements and between marked columns where ldo > C.
  * `*_reference` (fp64 numpy; pinned to torch by the CPU test), `check_*` (pass / fail of what a call left behind) and `emulate_*` (a
    numpy float32 model of a correct call, with the mutants of the CPU test).

Bounds.  nll and lse: the project's own bound for a candidate log-likelihood term, 1e-4 * max(1, |ref|.max()) (tests/test_lhood_gpu.py
`bound`), on the worst element of the whole output and of each named slice (the slice against its own reference).  Integers and
vd_lhood_sum: bit for bit.  The edge sum, per candidate:

    |got - ref| <= (K + T + 4) * 2^-24 * sum_t ( |h| . |W[tgt - 1]| + |bias[tgt - 1]| + |lse[nd]| ).

Derivation (u = 2^-24, first order in u).  A term is fl(fl(d + b) - l) with d a length-K fp32 dot product.  In ANY summation order (lane
partials of fmas, then a butterfly) every product passes through at most K rounded operations on its way to d, so |d - d_exact| <=
K u |h|.|W|.  The bias add and the subtraction of lse each round once, relative to a value of magnitude at most m_t = |h|.|W| + |b| + |l|:
2 u m_t.  The running sum over the candidate's at most T terms rounds at most T times, each relative to a partial sum of magnitude at most
sum_t m_t: T u sum_t m_t.  Together (K + 2 + T) u sum_t m_t; the remaining 2 u cover the second-order terms ((1 + u)^n - 1 <= 1.0001 n u for
the n <= 1100 of this table).  It is derived, not measured.  No tolerance here is taken from the code under test."""
import collections
import functools
import math

import numpy as np

U = 2.0 ** -24                           # fp32 unit roundoff
TILE = 128                               # lhood.hip LhoodCfg::BM = BN: vocabulary entries / live rows per tile
GUARD = 128                              # marked elements behind every output
TAIL = 64                                # NaN elements behind h, W, bias, lse
W_OFF = 4                                # offset of W inside its buffer, floats (16-byte aligned)
MARK = np.float32(-7.25e3)               # float outputs wherever a call must not write
IMARK = np.int32(-77)                    # integer outputs wherever a call must not write
ROW_LDS_FLOATS = 48 * 1024 // 4          # lhood.hip: (size_t)H * 4 <= 48 * 1024, the h row of the row kernels in LDS
ORDER_ROWS = 256                         # lhood.hip ORDER_ROWS: rows per block of the counting sort
LIVE_BLOCK = 1024                        # lhood.hip: rows per block of vd_lhood_live_rows


def cdiv(a, b):
    return (a + b - 1) // b


def bound(ref):
    """tests/test_lhood_gpu.py `bound`"""
    return 1e-4 * max(1.0, float(np.abs(ref).max())) if np.size(ref) else 1e-4


# ------------------------------------------------------------------------------------------------------------ the restated dispatch
def fused_fits(rows, ldh, V, ldw, H):
    # paths.h vd_lhood_fused_fits:
    # H >= 64 && H % 16 == 0 && V >= 128 && ldh % 4 == 0 && ldw % 4 == 0 && rows * ldh * 4 < (1L << 32) && V * ldw * 4 < (1L << 32)
    return H >= 64 and H % 16 == 0 and V >= 128 and ldh % 4 == 0 and ldw % 4 == 0 and rows * ldh * 4 < 2 ** 32 and V * ldw * 4 < 2 ** 32


def head_family(rows, ldh, V, ldw, H, h_addr=0, w_addr=0):
    """vd_lhood_nll / vd_lhood_lse_p at n_act > 0: 'mfma' | 'rows' | 'refused'.  h_addr / w_addr: the byte addresses of h and W (device
    allocations are aligned far beyond 16 bytes: the byte offset inside the buffer decides)
      if (vd_lhood_fused_fits(rows, ldh, V, ldw, H) && ((uintptr_t)h & 15) == 0 && ((uintptr_t)W & 15) == 0) -> the MFMA kernel
      VD_CHECK_ARG((size_t)H * 4 <= 48 * 1024, ".. too large for the row kernel") -> the row kernel"""
    if not (rows >= 0 and V >= 1 and H >= 1 and ldh >= H and ldw >= H):
        return 'refused'
    if fused_fits(rows, ldh, V, ldw, H) and h_addr & 15 == 0 and w_addr & 15 == 0:
        return 'mfma'
    return 'rows' if H * 4 <= 48 * 1024 else 'refused'


def prefix_fits(T, rows):
    # paths.h vd_lhood_prefix_fits: T >= 1 && T < 256 && rows >= 1
    return T >= 1 and T < 256 and rows >= 1


# ------------------------------------------------------------------------------------------------------------ head cases (nll, lse)
class HeadCase(object):
    """vd_lhood_nll and vd_lhood_lse_p on one set of operands.  `hot`: None, or 'first' / 'last' -- logits spread over +-80 with every
    row's maximum in column 5 (first tile) / column V - 3 (the last, ragged tile).  `h_off`: offset of h inside its buffer, floats.
    `values`: the name of the case whose VALUES (h rows, W, bias, act, targets) this one shares under another layout.  `tgt0`: the
    target column of a one-row case."""

    def __init__(self, name, family, H, V, n_act, pad_h=0, pad_w=0, bias=True, hot=None, h_off=0, more_rows=0, values=None, tgt0=0,
                 why=''):
        self.name, self.family, self.H, self.V, self.n_act = name, family, H, V, n_act
        self.ldh, self.ldw, self.bias, self.hot, self.h_off, self.values, self.tgt0, self.why = H + pad_h, H + pad_w, bool(bias), hot, h_off, values or name, tgt0, why
        self.rows = 2 * n_act + 5 + more_rows

    @property
    def id(self):
        return self.name

    @property
    def path(self):
        return head_family(self.rows, self.ldh, self.V, self.ldw, self.H, 4 * self.h_off, 4 * W_OFF)


HEAD = [
    # ---- family mfma: (H, V, n_act, ldh - H, ldw - H, bias)
    HeadCase('mfma-64x128-n128', 'mfma', 64, 128, 128, why='every minimum at once'),
    HeadCase('mfma-64x129-n129', 'mfma', 64, 129, 129, why='one-entry ragged vocabulary tile (bias +3 on column V - 1), one-row ragged row tile'),
    HeadCase('mfma-80x255-n1-first', 'mfma', 80, 255, 1, 4, 8, tgt0=0, why='5 k-tiles, one live row, strided operands; target column 0'),
    HeadCase('mfma-80x255-n1-last', 'mfma', 80, 255, 1, 4, 8, tgt0=254, why='the same with the target in column V - 1'),
    HeadCase('mfma-512x384-n127-nobias', 'mfma', 512, 384, 127, bias=False, why='no ragged tile, NULL bias'),
    HeadCase('mfma-512x1290-n300', 'mfma', 512, 1290, 300, 4, 4, why='10 full tiles + 10 entries; 2 full row tiles + 44 rows'),
    HeadCase('mfma-1040x640-n257', 'mfma', 1040, 640, 257, why='65 k-tiles'),
    HeadCase('mfma-512x1290-n300-max-first', 'mfma', 512, 1290, 300, 4, 4, hot='first', why='logits +-80, row maximum in the first tile'),
    HeadCase('mfma-512x1290-n300-max-last', 'mfma', 512, 1290, 300, 4, 4, hot='last', why='logits +-80, row maximum in the ragged last tile'),
    HeadCase('mfma-64x130-n140-offset', 'mfma', 64, 130, 140, 4, 0, h_off=8, more_rows=300, why='h at a 16-byte-aligned offset, rows > max(act) + 1'),
    # ---- family rows: (H, V)
    HeadCase('rows-1x1', 'rows', 1, 1, 3, why='the result must be exactly +0'),
    HeadCase('rows-32x7', 'rows', 32, 7, 5, 3, 5),
    HeadCase('rows-32x63', 'rows', 32, 63, 5, why='waves 1-3 have no vocabulary entry'),
    HeadCase('rows-32x257', 'rows', 32, 257, 140, 1, 2),
    HeadCase('rows-72x300', 'rows', 72, 300, 140, 4, 4, why='H % 16 != 0'),
    HeadCase('rows-512x127', 'rows', 512, 127, 5, 4, 4, why='V < 128'),
    HeadCase('rows-512x1290-ldh-odd', 'rows', 512, 1290, 300, 1, 4, values='mfma-512x1290-n300', why='ldh = H + 1'),
    HeadCase('rows-512x1290-misaligned', 'rows', 512, 1290, 300, 4, 4, h_off=1, values='mfma-512x1290-n300', why='h one float off alignment'),
    HeadCase('rows-12288x2', 'rows', 12288, 2, 5, why='the 48 KB limit of the row kernel\'s LDS'),
]
assert len(set(c.name for c in HEAD)) == len(HEAD)
HEAD_BY_NAME = dict((c.name, c) for c in HEAD)
SHARED = ('mfma-512x1290-n300', 'rows-512x1290-ldh-odd', 'rows-512x1290-misaligned')     # one set of values through both families


def _target_columns(V, n, twins, tgt0):
    """(s, columns): 0-based target columns (i * s mod V), i < n, for the smallest s > 1 coprime to V (1 where there is none) such that,
    once the twins share a column and the columns 0, V - 1, 127, 128 that the walk misses have replaced entries it can spare, the list
    holds those columns and, where n >= TILE, every residue mod TILE"""
    if n == 1:
        return 1, np.array([tgt0], np.int64)
    want = [col for col in (0, V - 1, TILE - 1, TILE) if 0 <= col < V]
    for s in [s for s in range(2, V + 2) if math.gcd(s, V) == 1] + [1]:
        tcol = (np.arange(n, dtype=np.int64) * s) % V
        if twins:
            tcol[list(twins[1:])] = tcol[twins[0]]
        for col in want + (list(range(min(TILE, V))) if n >= TILE else []):
            if col in tcol or (col not in want and col in tcol % TILE):
                continue
            for i in range(n):                                 # an entry that is no twin, holds no wanted column and whose residue stands elsewhere too
                spare = n < TILE or (tcol % TILE == tcol[i] % TILE).sum() > 1
                if (not twins or i not in twins) and tcol[i] not in want and spare:
                    tcol[i] = col
                    break
        if set(want) <= set(tcol.tolist()) and (n < TILE or len(set((tcol % TILE).tolist())) == min(TILE, V)):
            return s, tcol
    raise AssertionError('no target walk for V = %d, n_act = %d' % (V, n))


HeadValues = collections.namedtuple('HeadValues', 'h W b act target twins stride hot_col')


@functools.lru_cache(maxsize=None)
def head_values(name):
    """the VALUES of a head case: h [rows x H] (all rows random here; the layout keeps the listed ones), W [V x H], b [V] or None, act
    (ascending), target [rows] (0 off the list), the three twin positions (or None), the target stride"""
    c = HEAD_BY_NAME[name]
    H, V, n = c.H, c.V, c.n_act
    rng = np.random.RandomState(H * 7919 + V * 31 + n * 17 + (0 if c.hot is None else 1 + len(c.hot)))
    scale = 20.0 if c.hot else 1.0
    h = rng.standard_normal((c.rows, H)).astype(np.float32)
    W = (rng.standard_normal((V, H)) * (scale / np.sqrt(H))).astype(np.float32)
    b = (rng.standard_normal(V) * 0.3).astype(np.float32) if c.bias else None
    if c.bias and V == 129:
        b[V - 1] = 3.0                                         # the one entry of the ragged tile carries mass
    hot_col = None
    if c.hot:                                                  # h[:, 0] = 1 and W[:, 0] = 160 in one column only: that column is every row's maximum
        hot_col = 5 if c.hot == 'first' else V - 3
        h[:, 0] = 1.0
        W[:, 0] = 0.0
        W[hot_col, 0] = 160.0
    act = np.sort(rng.choice(c.rows - 1, size=n, replace=False)).astype(np.int32)      # (row act[i] + 1 always exists)
    twins = None
    if 3 <= n < TILE or n >= TILE + 2:                         # first tile; another lane of a middle tile; the (ragged) last tile.  (Not where
        twins = (7 if n > 16 else 0, 200 if n > 2 * TILE else n // 2, n - 1)  # two shared targets would leave fewer than 128 distinct ones.)
    s, tcol = _target_columns(V, n, twins, c.tgt0)
    if twins:
        h[act[list(twins[1:])]] = h[act[twins[0]]]
    target = np.zeros(c.rows, np.int32)
    target[act] = tcol + 1
    for a in (h, W, act, target) + ((b,) if b is not None else ()):
        a.setflags(write=False)
    return HeadValues(h, W, b, act, target, twins, s, hot_col)


class HeadLayout(object):
    """flat float32 buffers hbuf = [h_off | rows x ldh | TAIL], wbuf = [W_OFF | V x ldw | TAIL], bbuf = [V | TAIL] or None, all NaN outside
    the values; act, target int32; out0 = [n_act | GUARD] of MARK"""

    def __init__(self, c):
        self.case, self.v = c, head_values(c.values)
        v = self.v
        self.hbuf = np.full(c.h_off + c.rows * c.ldh + TAIL, np.nan, np.float32)
        self.hview(self.hbuf)[v.act, :c.H] = v.h[v.act]
        self.wbuf = np.full(W_OFF + c.V * c.ldw + TAIL, np.nan, np.float32)
        self.wview(self.wbuf)[:, :c.H] = v.W
        self.bbuf = None
        if c.bias:
            self.bbuf = np.full(c.V + TAIL, np.nan, np.float32)
            self.bbuf[:c.V] = v.b
        self.act, self.target = v.act, v.target
        self.out0 = np.full(c.n_act + GUARD, MARK, np.float32)

    def hview(self, buf):
        c = self.case
        return buf[c.h_off:c.h_off + c.rows * c.ldh].reshape(c.rows, c.ldh)

    def wview(self, buf):
        c = self.case
        return buf[W_OFF:W_OFF + c.V * c.ldw].reshape(c.V, c.ldw)

    def slices(self, op):
        """named index sets of the output: the ragged last row tile, the rows whose target lies in the ragged vocabulary tile, the twins"""
        c, n = self.case, self.case.n_act
        out = []
        if n % TILE and n > TILE:
            out.append(('last ragged row tile', np.arange(n // TILE * TILE, n)))
        if op == 'nll' and c.V % TILE and c.V > TILE:
            idx = np.flatnonzero(self.target[self.act] - 1 >= c.V // TILE * TILE)
            if idx.size:
                out.append(('targets in the ragged vocabulary tile', idx))
        if self.v.twins:
            out.append(('repeated rows', np.array(self.v.twins)))
        return out


@functools.lru_cache(maxsize=4)
def head_layout(case):
    return HeadLayout(case)


def logits64(lay):
    c, v = lay.case, lay.v
    x = v.h[v.act].astype(np.float64) @ v.W.astype(np.float64).T
    return x + v.b.astype(np.float64) if c.bias else x


@functools.lru_cache(maxsize=None)
def _head_reference(values, bias):
    lay = head_layout([c for c in HEAD if c.values == values and c.bias == bias][0])
    x = logits64(lay)
    mx = x.max(1)
    lse = mx + np.log(np.exp(x - mx[:, None]).sum(1))
    nll = lse - x[np.arange(len(lay.act)), lay.target[lay.act] - 1]
    lse.setflags(write=False)
    nll.setflags(write=False)
    return {'lse': lse, 'nll': nll}


def head_reference(lay, op):
    """fp64: lse[i] = logsumexp_v(h[act[i]] . W[v] + bias[v]); nll[i] = lse[i] - logit of column target[act[i]] - 1.  Computed once per set
    of values and shared: read only"""
    return _head_reference(lay.case.values, lay.case.bias)[op]


Verdict = collections.namedtuple('Verdict', 'ok failures err ratio')


def _guard_failures(before, after, keep, what):
    """`after` equals `before` bit for bit outside the index set `keep`"""
    a, b = np.array(before, copy=True), np.array(after, copy=True)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    ai, bi = a.view(np.uint32).reshape(-1), b.view(np.uint32).reshape(-1)
    mask = np.ones(ai.size, bool)
    mask[keep] = False
    bad = np.flatnonzero((ai != bi) & mask)
    return ['%s: %d guard elements written, first at flat index %d' % (what, bad.size, int(bad[0]))] if bad.size else []


def check_head(lay, op, out):
    """pass / fail of the buffer [n_act | GUARD] a call of `op` ('nll' | 'lse') left behind"""
    c, n = lay.case, lay.case.n_act
    out = np.asarray(out, np.float32)
    ref = head_reference(lay, op)
    got = out[:n].astype(np.float64)
    fails = []
    if not np.isfinite(got).all():
        fails.append('%d non-finite results' % int((~np.isfinite(got)).sum()))
    d = np.where(np.isfinite(got), np.abs(got - ref), np.inf)
    err, ratio = float(d.max()), float(d.max()) / bound(ref)
    if not err < bound(ref):
        fails.append('worst |err| %.3e >= %.3e at %d' % (err, bound(ref), int(np.argmax(d))))
    for name, idx in lay.slices(op):
        e, bd = float(d[idx].max()), bound(ref[idx])
        ratio = max(ratio, e / bd)
        if not e < bd:
            fails.append('%s: worst |err| %.3e >= %.3e' % (name, e, bd))
    if lay.v.twins:
        t = out[list(lay.v.twins)].view(np.uint32)
        if not (t[0] == t[1] == t[2]):
            fails.append('the repeated rows differ: %s' % out[list(lay.v.twins)])
    if op == 'nll' and c.V == 1 and (out[:n].view(np.uint32) != 0).any():
        fails.append('V = 1: nll is not exactly +0: %s' % out[:n])
    fails += _guard_failures(lay.out0, out, np.arange(n), op)
    return Verdict(not fails, fails, err, ratio)


MUTANTS_HEAD = ('last tile dropped', 'bias dropped', 'target off by one', 'W at ld = H', 'h row + 1', 'partial state dropped')


def head_mutant_applies(c, op, mutant):
    if mutant == 'last tile dropped':
        return c.V > TILE                                      # (of one tile nothing would be left)
    if mutant == 'bias dropped':
        return c.bias
    if mutant == 'target off by one':
        return op == 'nll' and c.V > 1
    if mutant == 'W at ld = H':
        return c.ldw > c.H
    if mutant == 'partial state dropped':
        return c.V >= 8
    return True


def emulate_head(lay, op, mutant=None):
    """what a correct call leaves in [n_act | GUARD], computed with numpy in float32; `mutant`: one of MUTANTS_HEAD"""
    c, v, n = lay.case, lay.v, lay.case.n_act
    rows = lay.act.astype(np.int64) + (1 if mutant == 'h row + 1' else 0)
    h = lay.hview(lay.hbuf)[rows, :c.H]
    W = lay.wview(lay.wbuf)[:, :c.H]
    if mutant == 'W at ld = H':
        W = lay.wbuf[W_OFF:W_OFF + c.V * c.H].reshape(c.V, c.H)
    with np.errstate(all='ignore'):
        x = h @ W.T
        if c.bias and mutant != 'bias dropped':
            x = x + lay.bbuf[:c.V]
        tcol = lay.target[lay.act] - 1
        if mutant == 'target off by one':
            tcol = (tcol + 1) % c.V
        pick = x[np.arange(n), tcol]
        keep = np.ones(c.V, bool)
        if mutant == 'last tile dropped':
            keep[(c.V - 1) // TILE * TILE:] = False
            pick = np.where(keep[tcol], pick, np.float32(0))   # the kernel's pick stays 0 until the target's tile is seen
        if mutant == 'partial state dropped':
            keep[(np.arange(c.V) % 32 >= 4) & (np.arange(c.V) % 32 < 8)] = False
        xs = x[:, keep]
        mx = xs.max(1)
        lse = (mx + np.log(np.exp(xs - mx[:, None]).sum(1, dtype=np.float32))).astype(np.float32)
        res = lse if op == 'lse' else ((lse - pick).astype(np.float32) if c.V > 1 or mutant else np.zeros(n, np.float32))
    if v.twins and mutant != 'h row + 1':                     # (BLAS is not position independent; the kernels' contract is)
        res[list(v.twins[1:])] = res[v.twins[0]]
    out = lay.out0.copy()
    out[:n] = res
    return out


# ------------------------------------------------------------------------------------------------------------ the edge sum
class EdgeCase(object):
    """vd_lhood_edge_sum_p: `rows` candidates of T steps over a tree of `nodes` nodes, C candidates per score row of width ldo"""

    def __init__(self, H, rows, T, C, bias=True, pad_h=0, pad_w=0, pad_o=3, why=''):
        self.H, self.rows, self.T, self.C, self.bias, self.why = H, rows, T, C, bool(bias), why
        assert rows % C == 0 and pad_h % 4 == 0 and pad_w % 4 == 0 and H % 4 == 0
        self.ldh, self.ldw, self.ldo, self.V = H + pad_h, H + pad_w, C + pad_o, 50
        self.nodes = max(2, min(40, rows * T))

    @property
    def id(self):
        return 'edge-H%d-rows%d-T%d-C%d-b%d-ldh%d-ldw%d-ldo%d' % (self.H, self.rows, self.T, self.C, self.bias, self.ldh, self.ldw, self.ldo)


EDGE = [
    EdgeCase(4, 5, 9, 5, why='one lane only'),
    EdgeCase(252, 5, 9, 5, why='below the 256-float stride'),
    EdgeCase(256, 5, 9, 5, pad_h=4, pad_w=8, why='at the stride; ldh, ldw > H'),
    EdgeCase(260, 5, 9, 5, bias=False, why='above the stride: a second trip of one lane; NULL bias'),
    EdgeCase(1028, 5, 9, 5, pad_h=8, pad_w=4, why='a fifth trip of one lane'),
    EdgeCase(256, 1, 1, 1, pad_o=0, why='one candidate, one step, ldo = C'),
    EdgeCase(256, 1037, 9, 17, pad_h=4, pad_w=4, pad_o=5, why='260 workgroups, the last with one wave at work; ldo > C'),
    EdgeCase(260, 1037, 1, 61, bias=False, why='T = 1'),
    EdgeCase(256, 5, 0, 5, why='T = 0: every candidate +0, no operand is read'),
    EdgeCase(252, 1037, 0, 17, bias=False, why='T = 0'),
]
O_OFF = 2                                # column offset of the scores inside their rows' buffer (the runtime's o0)


class EdgeLayout(object):
    def __init__(self, c):
        self.case = c
        rng = np.random.RandomState(c.H * 131 + c.rows * 17 + c.T * 7 + c.C)
        hrows = 2 * c.nodes + 3
        self.node_row = np.sort(rng.choice(hrows, size=c.nodes, replace=False)).astype(np.int32)
        rng.shuffle(self.node_row)                                       # node ids are not in row order
        self.hbuf = np.full(hrows * c.ldh + TAIL, np.nan, np.float32)
        hv = self.hbuf[:hrows * c.ldh].reshape(hrows, c.ldh)
        hv[self.node_row, :c.H] = rng.standard_normal((c.nodes, c.H)).astype(np.float32)
        self.wbuf = np.full(W_OFF + c.V * c.ldw + TAIL, np.nan, np.float32)
        wv = self.wbuf[W_OFF:W_OFF + c.V * c.ldw].reshape(c.V, c.ldw)
        wv[:, :c.H] = (rng.standard_normal((c.V, c.H)) / np.sqrt(c.H)).astype(np.float32)
        self.h, self.W = hv[:, :c.H], wv[:, :c.H]
        self.bbuf = None
        if c.bias:
            self.bbuf = np.full(c.V + TAIL, np.nan, np.float32)
            self.bbuf[:c.V] = (rng.standard_normal(c.V) * 0.3).astype(np.float32)
        self.lse = np.full(c.nodes + TAIL, np.nan, np.float32)
        self.lse[:c.nodes] = (4.0 + rng.standard_normal(c.nodes)).astype(np.float32)
        # edges: left-aligned runs of random length, one row of them with a hole (tgt <= 0 is skipped wherever it stands)
        lens = rng.randint(0, c.T + 1, size=c.rows)
        self.etgt = (rng.randint(1, c.V + 1, size=(c.T, c.rows)) * (np.arange(c.T)[:, None] < lens[None, :])).astype(np.int32)
        self.enode = (rng.randint(0, c.nodes, size=(c.T, c.rows)) * (self.etgt > 0)).astype(np.int32)
        self.empty = self.twin = None
        if c.rows >= 5 and c.T:
            self.etgt[:, 1] = 0                                          # a candidate with no edge
            self.enode[:, 1] = 0
            self.etgt[c.T // 2, 2] = 0                                   # a hole
            self.etgt[:, c.rows - 1] = self.etgt[:, 0]                   # two identical candidates, in different workgroups where rows allows
            self.enode[:, c.rows - 1] = self.enode[:, 0]
            if c.T > 1:
                self.etgt[0, 0] = self.etgt[0, c.rows - 1] = 1
                self.etgt[1, 0] = self.etgt[1, c.rows - 1] = c.V         # W rows 0 and V - 1
            self.empty, self.twin = 1, (0, c.rows - 1)
        self.out_rows = c.rows // c.C
        self.out0 = np.full(O_OFF + self.out_rows * c.ldo + GUARD, MARK, np.float32)

    def out_index(self):
        c = self.case
        r = np.arange(c.rows)
        return O_OFF + (r // c.C) * c.ldo + r % c.C


@functools.lru_cache(maxsize=2)
def edge_layout(case):
    return EdgeLayout(case)


def edge_reference(lay, lse_shift=0):
    """(ref, mag) [rows] in fp64: sum_t (W[tgt - 1] . h[node_row[nd]] + bias[tgt - 1] - lse[nd]) and the sum of the magnitudes.
    `lse_shift`: the mutant that takes an edge's lse from node nd + shift"""
    c = lay.case
    ref, mag = np.zeros(c.rows), np.zeros(c.rows)
    h, W = lay.h.astype(np.float64), lay.W.astype(np.float64)
    for t in range(c.T):
        on = lay.etgt[t] > 0
        tg, nd = lay.etgt[t][on] - 1, lay.enode[t][on]
        hr, wr = h[lay.node_row[nd]], W[tg]
        b = lay.bbuf[:c.V].astype(np.float64)[tg] if c.bias else 0.0
        l = lay.lse[:c.nodes].astype(np.float64)[(nd + lse_shift) % c.nodes]
        ref[on] += (hr * wr).sum(1) + b - l
        mag[on] += (np.abs(hr) * np.abs(wr)).sum(1) + np.abs(b) + np.abs(l)
    return ref, mag


def check_edge(lay, out, ref=None, mag=None):
    c = lay.case
    out = np.asarray(out, np.float32)
    if ref is None:
        ref, mag = edge_reference(lay)
    idx = lay.out_index()
    got = out[idx].astype(np.float64)
    fails = []
    if not np.isfinite(got).all():
        fails.append('%d non-finite results' % int((~np.isfinite(got)).sum()))
    d = np.where(np.isfinite(got), np.abs(got - ref), np.inf)
    bd = (c.H + c.T + 4) * U * mag
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(bd > 0, d / bd, np.where(d == 0, 0.0, np.inf))
    ratio = float(q.max())
    if not ratio <= 1.0:
        fails.append('elementwise bound exceeded %.3g x at candidate %d (%d candidates)' % (ratio, int(np.argmax(q)), int((q > 1).sum())))
    zero = np.flatnonzero(mag == 0)                            # no edge: +0.0 with the sign bit clear
    if (out[idx[zero]].view(np.uint32) != 0).any():
        fails.append('a candidate without an edge is not +0.0')
    if lay.twin is not None and out[idx[lay.twin[0]]].view(np.uint32) != out[idx[lay.twin[1]]].view(np.uint32):
        fails.append('two identical candidates do not tie')
    fails += _guard_failures(lay.out0, out, idx, 'out')
    return Verdict(not fails, fails, float(d.max()), ratio)


def emulate_edge(lay, lse_shift=0):
    """float32 numpy model: a float32 dot product, + bias, - lse, added in step order"""
    c = lay.case
    acc = np.zeros(c.rows, np.float32)
    for t in range(c.T):
        on = lay.etgt[t] > 0
        tg, nd = lay.etgt[t][on] - 1, lay.enode[t][on]
        d = (lay.h[lay.node_row[nd]] * lay.W[tg]).sum(1, dtype=np.float32)
        if c.bias:
            d = d + lay.bbuf[:c.V][tg]
        acc[on] = acc[on] + (d - lay.lse[:c.nodes][(nd + lse_shift) % c.nodes])
    out = lay.out0.copy()
    out[lay.out_index()] = acc
    return out


# ------------------------------------------------------------------------------------------------------------ the length order
ORDER_SHAPES = [(1, 1, 1), (21, 255, 5), (21, 256, 4), (21, 257, 1), (255, 600, 100), (20, 700, 7)]      # (T, rows, C)
PROFILES = ('equal', 'empty', 'one long', 'staircase', 'holed')
OrderCase = collections.namedtuple('OrderCase', 'T rows C profile')
ORDER = [OrderCase(T, rows, C, p) for T, rows, C in ORDER_SHAPES for p in PROFILES]


def order_id(c):
    return 'order-T%d-rows%d-%s' % (c.T, c.rows, c.profile.replace(' ', '-'))


class OrderLayout(object):
    def __init__(self, c):
        self.case = c
        T, rows = c.T, c.rows
        rng = np.random.RandomState(T * 1009 + rows * 13 + len(c.profile))
        r = np.arange(rows)
        lens = {'equal': np.full(rows, max(1, T // 2)), 'empty': np.zeros(rows, np.int64),
                'one long': np.where(r == (rows * 2) // 3, T, 0), 'staircase': r % (T + 1),
                'holed': rng.randint(0, T + 1, size=rows)}[c.profile]
        tok = rng.randint(1, 1000, size=(T, rows)) * (np.arange(T)[:, None] < lens[None, :])
        if c.profile == 'holed':                               # a token behind the first pad in every third row that has room for one
            for q in r[::3]:
                if lens[q] + 1 < T:
                    tok[rng.randint(lens[q] + 1, T), q] = 5
        self.tok = tok.astype(np.int32)
        self.tgt = rng.randint(0, 1000, size=(T, rows)).astype(np.int32)
        self.out0 = {'perm': np.full(rows + GUARD, IMARK, np.int32), 'rep': np.full(rows + GUARD, IMARK, np.int32),
                     'tok_s': np.full(T * rows + GUARD, IMARK, np.int32), 'tgt_s': np.full(T * rows + GUARD, IMARK, np.int32),
                     'info': np.full(1 + T + GUARD, IMARK, np.int32)}

    def work_ints(self):
        # lhood.hip vd_lhood_order_work_ints: rows + blocks * (T + 1) + blocks
        blocks = cdiv(self.case.rows, ORDER_ROWS)
        return self.case.rows + blocks * (self.case.T + 1) + blocks


@functools.lru_cache(maxsize=2)
def order_layout(case):
    return OrderLayout(case)


def order_reference(lay):
    """perm = the STABLE argsort by descending count of leading non-pad steps, rep = perm // C, info = [holed, nact[0 .. T)] with nact[t] =
    rows longer than t, tok_s / tgt_s [t][p] = tok / tgt [t][perm[p]]"""
    c = lay.case
    nz = lay.tok != 0
    run = np.logical_and.accumulate(nz, axis=0)
    length = run.sum(0)
    perm = np.argsort(-length, kind='stable').astype(np.int32)
    info = np.concatenate([[int((nz & ~run).any())], [(length > t).sum() for t in range(c.T)]]).astype(np.int32)
    return {'perm': perm, 'rep': (perm // c.C).astype(np.int32), 'tok_s': lay.tok[:, perm].reshape(-1), 'tgt_s': lay.tgt[:, perm].reshape(-1),
            'info': info, 'length': length}


def check_order(lay, outs):
    """outs: name -> the buffer [.. | GUARD] the call left behind; everything bit for bit"""
    ref = order_reference(lay)
    fails = []
    for k in ('perm', 'rep', 'tok_s', 'tgt_s', 'info'):
        got, n = np.asarray(outs[k], np.int32), ref[k].size
        if not np.array_equal(got[:n], ref[k]):
            fails.append('%s differs at %d of %d places, first at %d' % (k, int((got[:n] != ref[k]).sum()), n, int(np.flatnonzero(got[:n] != ref[k])[0])))
        fails += _guard_failures(lay.out0[k], got, np.arange(n), k)
    return Verdict(not fails, fails, 0.0, 0.0)


def emulate_order(lay, unstable=False):
    """`unstable`: the first two neighbours of equal length change places, everything gathered through that order"""
    c, ref = lay.case, order_reference(lay)
    perm = ref['perm'].copy()
    if unstable:
        L = ref['length'][perm]
        i = int(np.flatnonzero(L[1:] == L[:-1])[0])
        perm[[i, i + 1]] = perm[[i + 1, i]]
    vals = {'perm': perm, 'rep': (perm // c.C).astype(np.int32), 'tok_s': lay.tok[:, perm].reshape(-1), 'tgt_s': lay.tgt[:, perm].reshape(-1),
            'info': ref['info']}
    outs = {}
    for k, v in vals.items():
        outs[k] = lay.out0[k].copy()
        outs[k][:v.size] = v
    return outs


# ------------------------------------------------------------------------------------------------------------ the live-row list
LIVE = [(1, 'live'), (1, 'dead'), (1023, 'mixed'), (1024, 'mixed'), (1025, 'mixed'), (257 * 1024 + 3, 'mixed')]   # the last: 258 blocks,
#                                                          the 256-strided `before` loop of lhood_live_write_kernel takes its second trip


def live_inputs(n, kind):
    """tok_in, target [n] with pad inputs AND pad targets mixed in (a row is live where tok_in != 0 and target > 0); act0 = [n | GUARD]"""
    rng = np.random.RandomState(n % 100003 + len(kind))
    tok = (rng.randint(1, 50, size=n) * (rng.rand(n) < 0.7)).astype(np.int32)
    tgt = (rng.randint(1, 50, size=n) * (rng.rand(n) < 0.7)).astype(np.int32)
    if kind == 'live':
        tok[:], tgt[:] = 3, 4
    elif kind == 'dead':
        tok[:], tgt[:] = 3, 0
    else:
        tgt[::37] = -1                                         # a negative target is a pad too
        tok[n - 1], tgt[n - 1] = 9, 9                          # the last row is live: the last thread that writes
    return tok, tgt, np.full(n + GUARD, IMARK, np.int32)


def live_reference(tok, tgt):
    return np.flatnonzero((tok != 0) & (tgt > 0)).astype(np.int32)


def check_live(tok, tgt, act0, count, act):
    ref = live_reference(tok, tgt)
    fails = []
    if count != ref.size:
        fails.append('count %d, expected %d' % (count, ref.size))
    elif not np.array_equal(np.asarray(act)[:ref.size], ref):
        fails.append('act[:count] differs')
    fails += _guard_failures(act0, np.asarray(act, np.int32), np.arange(ref.size), 'act')
    return Verdict(not fails, fails, 0.0, 0.0)


# ------------------------------------------------------------------------------------------------------------ the sum with perm
SumCase = collections.namedtuple('SumCase', 'rows C T ldo perm empty')
SUM = [SumCase(1, 1, 9, 4, True, False), SumCase(255, 5, 9, 9, True, False), SumCase(255, 51, 9, 60, True, False),
       SumCase(257, 257, 9, 300, True, False), SumCase(257, 1, 9, 4, True, False), SumCase(257, 257, 9, 257, False, False),
       SumCase(255, 5, 9, 9, True, True), SumCase(257, 1, 0, 4, True, False)]


def sum_id(c):
    return 'sum-rows%d-C%d-T%d-ldo%d-%s%s' % (c.rows, c.C, c.T, c.ldo, 'perm' if c.perm else 'noperm', '-nolive' if c.empty else '')


class SumLayout(object):
    """act: an ascending subset of the T x rows rows (none under `empty`, where nll = act = NULL), nll [n_act | TAIL of NaN], perm a random
    permutation; out0 = [O_OFF | rows / C x ldo | GUARD] of MARK"""

    def __init__(self, c):
        self.case = c
        rng = np.random.RandomState(c.rows * 31 + c.C * 7 + c.T + c.ldo)
        n = c.T * c.rows
        live = np.zeros(n, bool) if c.empty else rng.rand(n) < 0.6
        if n and not c.empty:
            live[[0, n - 1]] = True
            if c.rows > 3:
                live[np.arange(c.T) * c.rows + 3] = False      # a candidate without a live row
        self.act = np.flatnonzero(live).astype(np.int32)
        self.nll = np.full(self.act.size + TAIL, np.nan, np.float32)
        self.nll[:self.act.size] = rng.standard_normal(self.act.size).astype(np.float32) * 3
        self.perm = rng.permutation(c.rows).astype(np.int32) if c.perm else None
        self.out0 = np.full(O_OFF + (c.rows // c.C) * c.ldo + GUARD, MARK, np.float32)

    def out_index(self, cand):
        c = self.case
        return O_OFF + (cand // c.C) * c.ldo + cand % c.C


@functools.lru_cache(maxsize=2)
def sum_layout(case):
    return SumLayout(case)


def emulate_sum(lay, inverse=False):
    """fp32, step order, negated as 0 - sum, scattered through perm: the contract, bit for bit.  `inverse`: perm applied as its inverse"""
    c = lay.case
    full = np.zeros(c.T * c.rows, np.float32)
    full[lay.act] = lay.nll[:lay.act.size]
    acc = np.zeros(c.rows, np.float32)
    for t in range(c.T):
        acc = acc + full[t * c.rows:(t + 1) * c.rows]
    cand = np.arange(c.rows) if lay.perm is None else lay.perm.astype(np.int64)
    if inverse:
        cand = np.argsort(cand)
    out = lay.out0.copy()
    out[lay.out_index(cand)] = np.float32(0) - acc
    return out


def check_sum(lay, out):
    c = lay.case
    want, out = emulate_sum(lay), np.asarray(out, np.float32)
    fails = []
    idx = lay.out_index(np.arange(c.rows))
    if not np.array_equal(out[idx].view(np.uint32), want[idx].view(np.uint32)):
        fails.append('%d scores differ in bits' % int((out[idx].view(np.uint32) != want[idx].view(np.uint32)).sum()))
    fails += _guard_failures(lay.out0, out, idx, 'out')
    return Verdict(not fails, fails, 0.0, 0.0)
