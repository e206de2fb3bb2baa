"""Case tables, layouts, references, checkers and float32 emulations for the entry points of csrc/elementwise.hip and csrc/loss.hip (no GPU
needed): the arrangement of tests/gemm_cases.py and tests/lhood_cases.py.

  * One table per family (DROPOUT, POINTWISE, GATHER, SCATTER, MASKTIME, ZERO_ROWS, ZERO_MULTI, TOKEN_SORT, SEGSUM, LOGSOFTMAX, NLL, SCORE,
    RANKS); every case carries a `why` and the smallest shape that reaches its path.
  * `*_layout(case)`: the operands as the runtime may pass them -- inputs inside larger buffers with NaN (floats) or BIGTOK (ints) behind
    them and in every pad column [ncol, ld); every output filled with a mark (MARK, IMARK, BMARK) in front of GUARD marked elements -- and
    the list of `Spec`s, one per output buffer: which elements must hold given bits and which are held to a bound against fp64.
  * `check(layout, outputs)`: pass / fail of what a call left behind.  Everything the operation does not own -- guards, pad columns, rows
    that are not listed, token rows without a member, the live rows [0, nact[t]) of the zeroing kernels -- must come back bit for bit.
  * `emulate_*(layout, mutant)`: a numpy float32 model of a correct call, and of the subtly wrong ones of tests/test_helper_cases_cpu.py.

References: fp64 numpy for floats (pinned to torch by the CPU test); exact restatements for the rest -- the dropout bit is `mix32` (the
64-bit finaliser of elementwise.hip) in wrapping uint64 arithmetic with thr = uint32(float32(p) * 2^24); `offset` is the exclusive scan of
bincount; a rank is 1 + #{j : s_j > s_o or (s_j == s_o and j < o)}.  oracle/visdial_oracle.py (lookup_backward, cross_entropy,
compute_ranks) and tests/train_knobs_ref.py state the heads.

Bounds, u = 2^-24, first order in u; none is taken from the code under test.
  * Bit for bit: dropout_mask, dropout_apply (one rounded product), embed_gather, mask_time_forward, both zeroing kernels, token_sort
    (offset; perm a permutation grouped by token, the order inside a token free), ranks, every "must not write" region, masked rows of the
    gen head (loss exactly +0, gradient exactly zero), the logits after write_grad = 0.
  * Sums of m addends in any order (embed_scatter_acc, segment_rowsum_acc and _bf16, mask_time_backward), per element:
        |got - ref| <= (m + 4) u (|out0| + sum |addend|).
    Derivation: however the m addends and out0 are grouped (register partial sums, then float atomics), every addition rounds once,
    relative to a partial sum of magnitude at most S = |out0| + sum |addend|, and there are at most m of them: m u S.  The masked scale of
    the scatter (x * 2) is exact; the remaining 4 u cover a rounded scale and the second-order terms ((1 + u)^m - 1 <= 1.0001 m u for the
    m <= 600 of these tables).  An element with no addend is not touched: bit for bit.  The bf16 form sums the bf16 inputs exactly widened to
    fp32, the reference sums the same values in fp64: the same bound.
  * Score dot products: (H + 4) u |optH| . |enc| per score -- every product passes through at most H rounded operations (fma or not).
  * tanh_backward, axpby: 4 u x the sum of the magnitudes of the terms: dx = dy - dy t t has three roundings without contraction, relative
    to at most |dy| + |dy t t|; c = alpha a + beta b likewise.
  * Everything behind an expf / logf (lse, log-softmax, losses): the project's own bound 1e-4 * max(1, |ref|.max()) (tests/test_lhood_gpu.py
    `bound`), on the worst element of the whole output and of each named slice (the slice against its own reference).
  * Gradients of the two heads: rel-L2 1e-5, the bound tests/test_ops_gpu.py holds them to; the row sums of the gen head's gradient, whose
    exact value is 0, within 1e-4 (the bound above at |ref| = 0).

|logit| <= 80 everywhere, so every reference is finite.  e^80 = 5.5e34 is finite in fp32: one column of +80 cannot show a missing max
subtraction, a flat row of 11322 columns of +80 does (the plain sum of exp, 6.3e38, overflows) -- the `flat80` cases."""
import collections
import functools

import numpy as np

U = 2.0 ** -24
GUARD = 128                              # marked elements behind every output
TAIL = 64                                # NaN / BIGTOK elements behind every input
MARK = np.float32(-7.25e3)
IMARK = np.int32(-77)
BMARK = np.uint8(0x5A)
BIGTOK = np.int32(0x3fffffff)            # behind every integer input: as a row or token index it would leave every buffer
NAN16 = np.uint16(0x7fc0)                # bf16 NaN
F32, F64, I32, U8 = np.float32, np.float64, np.int32, np.uint8
MAX_OPT = 128                            # loss.hip
CHUNK = 256                              # elementwise.hip segment_rowsum_kernel<256>: sorted rows per workgroup
Verdict = collections.namedtuple('Verdict', 'ok failures err ratio')
Case = collections.namedtuple('Case', 'id why p')      # p: a dict of the family's parameters


def case(id, why, **p):
    return Case(id, why, p)


def cached(fn):
    """one layout per (case, arguments): built once, shared by the tests that need it, read only"""
    store = {}

    @functools.wraps(fn)
    def wrapper(c, *args):
        key = (c.id,) + args
        if key not in store:
            store[key] = fn(c, *args)
        return store[key]
    return wrapper


def bound(ref):
    """tests/test_lhood_gpu.py `bound`"""
    return 1e-4 * max(1.0, float(np.abs(ref).max())) if np.size(ref) else 1e-4


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def fin(vals, dtype=F32, tail=TAIL):
    """an input: the values, flat, in front of `tail` elements that must never be read"""
    vals = np.ascontiguousarray(vals, dtype).reshape(-1)
    fill = {F32: np.nan, I32: BIGTOK, U8: BMARK, np.uint16: NAN16}[dtype]
    out = np.concatenate([vals, np.full(tail, fill, dtype)])
    out.setflags(write=False)
    return out


def marked(n, dtype=F32):
    return np.full(n + GUARD, {F32: MARK, I32: IMARK, U8: BMARK}[dtype], dtype)


def strided(vals, ld, fill=np.nan, dtype=F32):
    """[rows x ncol] values as [rows x ld] with `fill` in the pad columns"""
    vals = np.asarray(vals, dtype)
    out = np.full((vals.shape[0], ld), fill, dtype)
    out[:, :vals.shape[1]] = vals
    return out


class Spec(object):
    """what a call must leave in one output buffer.  `exact`: the whole buffer as it must read wherever `bounded` is False (bit for bit;
    default out0).  `bounded`: the elements held against `ref` (fp64, whole buffer) by `rule`: 'elem' (|err| <= bnd per element; where
    bnd = 0 the value must equal the reference), 'proj' (1e-4 max(1, |ref|.max()) over all of them and over each of `slices`), 'rel'
    (rel-L2 1e-5 over all of them), 'perm' (token_sort's perm: `ref` = (tok, n))."""

    def __init__(self, name, out0, exact=None, bounded=None, ref=None, rule=None, bnd=None, slices=()):
        self.name, self.out0, self.exact = name, out0, out0 if exact is None else exact
        self.bounded, self.ref, self.rule, self.bnd, self.slices = bounded, ref, rule, bnd, slices
        assert self.exact.shape == out0.shape and self.exact.dtype == out0.dtype
        for a in (self.out0, self.exact):
            a.setflags(write=False)


def check_spec(s, got):
    got = np.asarray(got)
    if got.shape != s.out0.shape or got.dtype != s.out0.dtype:
        return ['%s: shape / type' % s.name], np.inf, np.inf
    f, err, ratio = [], 0.0, 0.0
    own = s.bounded if s.bounded is not None else np.zeros(got.shape, bool)
    bad = np.flatnonzero((bits(got) != bits(s.exact)) & ~own)
    if bad.size:
        f.append('%s: %d elements that must come back bit for bit differ, the first at %d (%r, must be %r)'
                 % (s.name, bad.size, bad[0], got[bad[0]], s.exact[bad[0]]))
    if not own.any():
        return f, err, ratio
    idx = np.flatnonzero(own)
    if s.rule == 'scratch':                                        # any content
        return f, err, ratio
    if s.rule == 'perm':
        tok, n = s.ref
        p = got[idx]
        if sorted(p.tolist()) != list(range(n)):
            f.append('%s: not a permutation of the rows' % s.name)
        elif (np.diff(tok[p]) < 0).any():
            f.append('%s: rows not grouped by ascending token' % s.name)
        return f, err, (2.0 if f else 0.0)
    g, r = got[idx].astype(F64), s.ref[idx]
    if not np.isfinite(g).all():
        return f + ['%s: not finite' % s.name], np.inf, np.inf
    e = np.abs(g - r)
    err = float(e.max())
    if s.rule == 'elem':
        b = s.bnd[idx]
        ratio = float((e[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0
        if (e[b == 0] != 0).any() or (bits(got[idx][b == 0]) != bits(r[b == 0].astype(F32))).any():
            f.append('%s: an element with no rounding differs from its reference' % s.name)
            ratio = max(ratio, 2.0)
    elif s.rule == 'proj':
        ratio = err / bound(r)
        for name, sl in s.slices:
            rs = float(np.abs(got[sl].astype(F64) - s.ref[sl]).max()) / bound(s.ref[sl])
            if rs > 1.0:
                f.append('%s: slice `%s` at %.3f of its bound' % (s.name, name, rs))
            ratio = max(ratio, rs)
    elif s.rule == 'rel':
        ratio = float(np.linalg.norm(g - r) / max(np.linalg.norm(r), 1e-30)) / 1e-5
    if ratio > 1.0:
        f.append('%s: worst error / bound %.3f (worst |err| %.3e)' % (s.name, ratio, err))
    return f, err, ratio


def check(lay, outs, only=None):
    """`only`: the names of the outputs to judge (an entry point that shares its layout with another), default all"""
    f, err, ratio = [], 0.0, 0.0
    for s in lay.specs:
        if only is not None and s.name not in only:
            continue
        fs, e, r = check_spec(s, outs[s.name])
        f, err, ratio = f + fs, max(err, e), max(ratio, r)
    for name, fn in getattr(lay, 'extra', ()):                     # whole-call properties (gradient row sums)
        e, r = fn(outs)
        if r > 1.0:
            f.append('%s at %.3f of its bound' % (name, r))
        ratio = max(ratio, r)
    return Verdict(not f, f, err, ratio)


class Layout(object):
    def __init__(self, case, inp, specs, **kw):
        self.case, self.inp, self.specs = case, inp, specs
        self.__dict__.update(kw)

    def out0(self):
        return dict((s.name, s.out0.copy()) for s in self.specs)

    def good(self):
        """every output as its spec's `exact` (the whole answer of a bit-for-bit family)"""
        return dict((s.name, s.exact.copy()) for s in self.specs)


def differs(a, b):
    return any((bits(a[k]) != bits(b[k])).any() for k in a)


# ------------------------------------------------------------------------------------------------------------ dropout_mask
def mix32(x):
    """elementwise.hip mix32 on a uint64 array, wrapping"""
    x = np.array(x, np.uint64, ndmin=1)
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xff51afd7ed558ccd)
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xc4ceb9fe1a85ec53)
    x ^= x >> np.uint64(33)
    return (x & np.uint64(0xffffffff)).astype(np.uint32)


def dropout_hash24(n, seed, first=0):
    base = np.uint64((seed * 0x9E3779B97F4A7C15) % 2 ** 64)
    return mix32(base + np.arange(first, first + n, dtype=np.uint64)) >> np.uint32(8)


def dropout_threshold(p):
    return np.uint32(np.float32(p) * np.float32(16777216.0))


def dropout_bits(n, seed, p, strict=False):
    h, thr = dropout_hash24(n, seed), dropout_threshold(p)
    return ((h > thr) if strict else (h >= thr)).astype(U8)


P_MAX = 1.0 - 2.0 ** -24
SEEDS = (0, 1234, 2 ** 63 + 5)
DROPOUT = [case('drop-n%d-p%d-s%d' % (n, ip, (i + ip) % 3), why, n=n, p=p, seed=SEEDS[(i + ip) % 3])
           for i, (n, why) in enumerate([(1, 'one byte: the tail loop only'), (3, 'tail of 3'), (4, 'one packed store, no tail'),
                                         (5, 'a packed store and a tail of 1'), (1023, 'the last thread of a block in the tail loop'),
                                         (1024, 'one full block of packed stores'), (1025, 'a second block for one byte'),
                                         (2049, 'three blocks')])
           for ip, p in enumerate((0.0, 0.2, 0.5, P_MAX))]
# the threshold met exactly: p = (the 24 hash bits of element 2) / 2^24, so element 2 is kept by >= and dropped by >
_h2 = int(dropout_hash24(1, 1234, first=2)[0])
DROPOUT.append(case('drop-n5-on-threshold', 'element 2 hashes to the threshold itself: kept', n=5, p=_h2 / 2.0 ** 24, seed=1234))


@cached
def dropout_layout(c):
    n = c.p['n']
    out0 = marked(n, U8)
    want = out0.copy()
    want[:n] = dropout_bits(n, c.p['seed'], c.p['p'])
    return Layout(c, {}, [Spec('mask', out0, want)])


def emulate_dropout(lay, mutant=None):
    """the kernel's walk: thread i4 / 4 computes four bits, stores them packed where i4 + 3 < n, else byte by byte"""
    n, seed, p = (lay.case.p[k] for k in ('n', 'seed', 'p'))
    m = dropout_bits(n + 3, seed, p, strict=(mutant == 'threshold compared with >'))
    out = lay.specs[0].out0.copy()
    full = n // 4 * 4
    out[:full] = m[:full]
    if mutant == 'tail writes 4 bytes at n - 1':
        if n % 4:
            out[n - 1:n + 3] = m[n - 1:n + 3]
    else:
        out[full:n] = m[full:n]
    return {'mask': out}


# ------------------------------------------------------------------------------------------------------------ pointwise glue
POINTWISE = [case('%s-n%d' % (op, n), why + '; ' + w2, op=op, n=n)
             for op, why in (('dropout_apply', 'y = mask ? x * 1.25 : +0, NaN under dropped elements'), ('tanh_backward', 'dx = dy (1 - y^2)'),
                             ('axpby', 'c = 0.5 a - 2 b'), ('axpby-bnull', 'b = NULL, beta = NaN ignored'),
                             ('axpby-inplace', 'c aliases a, b = NULL, alpha = -1 (how retrieve_* negates the NLL)'))
             for n, w2 in ((1, 'one thread'), (255, 'one short of a block'), (256, 'one block'), (257, 'a second block for one element'))]


@cached
def pointwise_layout(c):
    op, n = c.p['op'], c.p['n']
    rng = np.random.RandomState(n + len(op))
    a, b = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
    own = np.zeros(n + GUARD, bool)
    own[:n] = True
    out0 = marked(n)
    ref, bnd = np.zeros(n + GUARD), np.zeros(n + GUARD)
    if op == 'dropout_apply':
        m = (rng.rand(n) > 0.4).astype(U8)
        m[0] = 0
        x = a.copy()
        x[m == 0] = np.nan
        want = out0.copy()
        want[:n] = np.where(m != 0, x * np.float32(1.25), np.float32(0))
        return Layout(c, {'x': fin(x), 'mask': fin(m, U8)}, [Spec('y', out0, want)], scale=1.25)
    if op == 'tanh_backward':
        t = np.tanh(b).astype(F32)
        dy, t64 = a.astype(F64), t.astype(F64)
        ref[:n], bnd[:n] = dy * (1 - t64 * t64), 4 * U * (np.abs(dy) + np.abs(dy) * t64 * t64)
        return Layout(c, {'dy': fin(a), 'y': fin(t)}, [Spec('dx', out0, bounded=own, ref=ref, rule='elem', bnd=bnd)])
    if op == 'axpby':
        ref[:n], bnd[:n] = 0.5 * a.astype(F64) - 2.0 * b, 4 * U * (0.5 * np.abs(a) + 2.0 * np.abs(b))
        return Layout(c, {'a': fin(a), 'b': fin(b)}, [Spec('c', out0, bounded=own, ref=ref, rule='elem', bnd=bnd)], alpha=0.5, beta=-2.0)
    if op == 'axpby-bnull':
        want = out0.copy()
        want[:n] = np.float32(0.5) * a                          # alpha a + 0: one rounded product
        return Layout(c, {'a': fin(a)}, [Spec('c', out0, want)], alpha=0.5, beta=np.nan)
    out0[:n] = a                                                  # in place: the output buffer IS a
    want = out0.copy()
    want[:n] = -a
    return Layout(c, {}, [Spec('c', out0, want)], alpha=-1.0, beta=np.nan)


def emulate_pointwise(lay, mutant=None):
    c, n = lay.case, lay.case.p['n']
    s = lay.specs[0]
    out = s.out0.copy()
    i = lay.inp
    hi = n + 1 if mutant == 'one element too many' else n         # (the inputs have TAIL elements behind them)
    if c.p['op'] == 'dropout_apply':
        with np.errstate(invalid='ignore'):
            out[:hi] = np.where(i['mask'][:hi] != 0, i['x'][:hi] * np.float32(lay.scale), np.float32(0))
    elif c.p['op'] == 'tanh_backward':
        t = i['y'][:hi]
        out[:hi] = i['dy'][:hi] * (np.float32(1) - t * t)
    elif c.p['op'] == 'axpby':
        out[:hi] = np.float32(lay.alpha) * i['a'][:hi] + np.float32(lay.beta) * i['b'][:hi]
    elif c.p['op'] == 'axpby-bnull':
        out[:hi] = np.float32(lay.alpha) * i['a'][:hi] + np.float32(0)
    else:
        out[:hi] = np.float32(lay.alpha) * out[:hi] + np.float32(0)
    return {s.name: out}


# ------------------------------------------------------------------------------------------------------------ embed_gather
GATHER = [case('gather-E%d-r%d-V%d-%s' % (E, rows, V, 'mask' if mask else 'nomask'), why, E=E, rows=rows, V=V, mask=mask)
          for E, rows, V, mask, why in [
              (4, 1, 3, False, 'one float4, one thread'),
              (4, 7, 3, True, 'more output rows (7) than table rows (4): the row-permutation use; repeated tokens'),
              (300, 7, 5, True, '525 float4s: a partial third workgroup; E = 300'),
              (300, 213, 40, False, '15975 float4s: the last workgroup holds 103'),
              (512, 213, 9, True, '27264 float4s: the last workgroup holds 128; every token many times'),
              (2048, 7, 3, False, '14 full workgroups, no partial one'),
              (2048, 1, 2, True, 'one row of 512 float4s with the mask')]]


@cached
def gather_layout(c):
    E, rows, V = c.p['E'], c.p['rows'], c.p['V']
    rng = np.random.RandomState(E + rows)
    emb = rng.standard_normal((V + 1, E)).astype(F32)              # row 0 is NOT zero here: token 0 must read table row 0
    tok = rng.randint(0, V + 1, size=rows).astype(I32)
    tok[0], tok[-1] = 0, V
    if rows > 2:
        tok[1] = tok[2] = V // 2
    out0 = marked(rows * E)
    want = out0.copy()
    inp = {'emb': fin(emb), 'tok': fin(tok, I32)}
    if c.p['mask']:
        m = (rng.rand(rows, E) > 0.5).astype(U8) * rng.randint(1, 256, size=(rows, E)).astype(U8)     # any non-zero byte keeps
        want[:rows * E] = np.where(m != 0, emb[tok] * np.float32(2), np.float32(0)).reshape(-1)
        inp['mask'] = fin(m, U8)
    else:
        want[:rows * E] = emb[tok].reshape(-1)                     # scale is ignored without a mask
    return Layout(c, inp, [Spec('out', out0, want)], scale=2.0)


def emulate_gather(lay, mutant=None):
    """thread idx of rows * E / 4 takes row idx / e4, quad idx % e4"""
    E, rows = lay.case.p['E'], lay.case.p['rows']
    e4 = E // 4
    total = rows * e4 - (1 if mutant == 'last quad dropped' else 0)
    idx = np.arange(total)
    r, q = idx // e4, idx % e4
    cols = (q[:, None] * 4 + np.arange(4)[None, :])
    tok = lay.inp['tok'][:rows]
    emb = lay.inp['emb'][:-TAIL].reshape(-1, E)
    v = emb[tok[r][:, None], cols]
    if 'mask' in lay.inp:
        m = lay.inp['mask'][:rows * E].reshape(rows, E)[r[:, None], cols]
        v = np.where(m != 0, v * np.float32(lay.scale), np.float32(0))
    out = lay.specs[0].out0.copy()
    out[(r[:, None] * E + cols).reshape(-1)] = v.reshape(-1)
    return {'out': out}


# ------------------------------------------------------------------------------------------------------------ embed_scatter_acc
SCATTER = [case('scatter-E%d-r%d-V%d-%s-%s' % (E, rows, V, dist, 'mask' if mask else 'nomask'), why, E=E, rows=rows, V=V, dist=dist, mask=mask)
           for E, rows, V, dist, mask, why in [
               (1, 5, 3, 'one', False, 'E = 1; every row the same token: 5 atomics on one float'),
               (3, 7, 9, 'distinct', True, 'E % 4 != 0 (the host accepts it); every row its own token; mask with scale 2'),
               (3, 300, 5, 'one', True, '300 addends on each of 3 floats, 900 elements: a partial fourth workgroup'),
               (300, 213, 40, 'random', True, 'E = 300, tokens repeat, rows without a member stay'),
               (300, 40, 7, 'one', False, 'all rows on token 0'),
               (300, 41, 40, 'distinct', False, 'every row its own token, token V included')]]


@cached
def scatter_layout(c):
    E, rows, V, dist = c.p['E'], c.p['rows'], c.p['V'], c.p['dist']
    rng = np.random.RandomState(E * 7 + rows)
    tok = {'one': np.zeros(rows, I32) + (0 if E == 300 else 2), 'distinct': np.arange(rows, dtype=I32) % (V + 1),
           'random': rng.randint(0, V + 1, size=rows).astype(I32)}[dist]
    dx = rng.standard_normal((rows, E)).astype(F32)
    dx[0] = 0.0                                                   # a row of exact +0 and one of -0: skipped, the element keeps its bits
    if rows > 1:
        dx[1] = -0.0
    demb0 = rng.standard_normal((V + 1, E)).astype(F32)
    demb0[tok[0], 0] = -0.0
    inp = {'tok': fin(tok, I32), 'dx': fin(dx)}
    add = dx.astype(F64)
    if c.p['mask']:
        m = (rng.rand(rows, E) > 0.5).astype(U8)
        inp['mask'] = fin(m, U8)
        add = add * m * 2.0
    n = (V + 1) * E
    out0 = marked(n)
    out0[:n] = demb0.reshape(-1)
    ref, mag, cnt = demb0.astype(F64), np.abs(demb0).astype(F64), np.zeros((V + 1, E))
    np.add.at(ref, tok, add)
    np.add.at(mag, tok, np.abs(add))
    np.add.at(cnt, tok, (add != 0).astype(F64))
    own = np.zeros(n + GUARD, bool)
    own[:n] = (cnt > 0).reshape(-1)
    full = lambda a: np.concatenate([a.reshape(-1), np.zeros(GUARD)])
    return Layout(c, inp, [Spec('demb', out0, bounded=own, ref=full(ref), rule='elem', bnd=full((cnt + 4) * U * mag))], scale=2.0, tokens=tok)


def emulate_scatter(lay, mutant=None):
    E, rows, V = lay.case.p['E'], lay.case.p['rows'], lay.case.p['V']
    out = lay.specs[0].out0.copy()
    d = out[:(V + 1) * E].reshape(V + 1, E)
    dx = lay.inp['dx'][:rows * E].reshape(rows, E)
    tok = lay.inp['tok'][:rows] + (1 if mutant == 'token off by one' else 0)
    m = lay.inp['mask'][:rows * E].reshape(rows, E) if 'mask' in lay.inp and mutant != 'mask ignored' else None
    for r in range(rows):
        v = dx[r] if m is None else np.where(m[r] != 0, dx[r] * np.float32(lay.scale), np.float32(0))
        nz = v != 0
        d[tok[r] % (V + 1)][nz] = (d[tok[r] % (V + 1)] + v)[nz]
    return {'demb': out}


# ------------------------------------------------------------------------------------------------------------ mask_time
MASKTIME = [case('masktime-T%d-N%d-D%d' % (T, N, D), why, T=T, N=N, D=D)
            for T, N, D, why in [(1, 1, 1, 'one element'), (3, 5, 3, 'D = 3; column 0 all pad, column 1 no pad'),
                                 (3, 257, 1, 'D = 1: the row index is the element index; a second workgroup for one element'),
                                 (1, 257, 300, 'T = 1, 77100 elements'), (3, 5, 300, 'D = 300'), (3, 1, 3, 'N = 1')]]


@cached
def masktime_layout(c):
    T, N, D = c.p['T'], c.p['N'], c.p['D']
    rng = np.random.RandomState(T * 100 + N + D)
    tok = (rng.rand(T, N) > 0.4).astype(I32) * rng.randint(1, 50, size=(T, N)).astype(I32)
    if N >= 5:
        tok[:, 0], tok[:, 1] = 0, 7
    else:
        tok[0, 0] = 3
    feat = rng.standard_normal((N, D)).astype(F32)
    dout = rng.standard_normal((T, N, D)).astype(F32)
    dout[tok == 0] = 1e30                                          # must not reach dfeat
    live = (tok != 0)
    fwd0 = marked(T * N * D)
    fwant = fwd0.copy()
    fwant[:T * N * D] = np.where(live[:, :, None], feat[None], np.float32(0)).reshape(-1)
    n = N * D
    add = np.where(live[:, :, None], dout.astype(F64), 0.0)
    cnt = np.broadcast_to(live.sum(0)[:, None], (N, D))
    full = lambda a: np.concatenate([np.asarray(a, F64).reshape(-1), np.zeros(GUARD)])
    own = np.zeros(n + GUARD, bool)
    own[:n] = True
    bnd = np.where(cnt > 0, (cnt + 4) * U * np.abs(add).sum(0), 0.0)
    return Layout(c, {'feat': fin(feat), 'tok': fin(tok, I32), 'dout': fin(dout)},
                  [Spec('out', fwd0, fwant), Spec('dfeat', marked(n), bounded=own, ref=full(add.sum(0)), rule='elem', bnd=full(bnd))])


def emulate_masktime(lay, mutant=None):
    T, N, D = (lay.case.p[k] for k in 'TND')
    tok = lay.inp['tok'][:T * N].reshape(T, N)
    live = np.ones((T, N), bool) if mutant == 'mask ignored' else tok != 0
    feat, dout = lay.inp['feat'][:N * D].reshape(N, D), lay.inp['dout'][:T * N * D].reshape(T, N, D)
    o = lay.out0()
    o['out'][:T * N * D] = np.where(live[:, :, None], feat[None], np.float32(0)).reshape(-1)
    s = np.zeros((N, D), F32)
    for t in range(T):
        s = np.where(live[t][:, None], s + dout[t], s)
    o['dfeat'][:N * D] = s.reshape(-1)
    return o


# ------------------------------------------------------------------------------------------------------------ the zeroing kernels
ZERO_ROWS = [case('zrows-T%d-N%d-c%d-ld%d-ts%d' % (T, N, nc, ld, ts), why, T=T, N=N, ncols=nc, ld=ld, tstride=ts, nact=nact)
             for T, N, nc, ld, ts, nact, why in [
                 (1, 1, 4, 4, 4, (0,), 'one quad'),
                 (1, 1, 4, 8, 16, (1,), 'nact = N: nothing to zero'),
                 (4, 7, 128, 132, 7 * 132 + 8, (0, 7, 3, 6), 'ld > ncols and tstride > N ld; nact 0, N and between'),
                 (4, 7, 4, 4, 28, (6, 0, 7, 1), 'dense, one quad per row'),
                 (4, 300, 128, 128, 300 * 128, (0, 300, 299, 1), 'N = 300: 9568 quads in slice 0'),
                 (1, 300, 2048, 2052, 300 * 2052 + 4, (17,), '144896 quads on 16384 threads: nine grid-stride trips')]]


def _zero_expected(buf, T, N, ncols, ld, tstride, nact, drow=0, dquad=0):
    out = buf.copy()
    for t in range(T):
        first = max(0, min(N, nact[t] + drow))
        rows = np.arange(first, N)
        cols = np.arange(ncols + 4 * dquad)
        out[(t * tstride + rows[:, None] * ld + cols[None, :]).reshape(-1)] = 0.0
    return out


@cached
def zero_rows_layout(c):
    T, N, ld, ts = (c.p[k] for k in ('T', 'N', 'ld', 'tstride'))
    rng = np.random.RandomState(T + N + ld)
    n = T * ts
    out0 = marked(n)
    out0[:n] = rng.standard_normal(n).astype(F32) + np.float32(3)   # live state: no element is zero beforehand
    nact = np.array(c.p['nact'], I32)
    return Layout(c, {'nact': fin(nact, I32)}, [Spec('buf', out0, _zero_expected(out0, T, N, c.p['ncols'], ld, ts, nact))])


ZERO_MUTANTS = {'one row too many': (-1, 0), 'one row too few': (1, 0), 'one quad too many': (0, 1), 'one quad too few': (0, -1)}


def emulate_zero_rows(lay, mutant=None):
    p = lay.case.p
    drow, dquad = ZERO_MUTANTS.get(mutant, (0, 0))
    return {'buf': _zero_expected(lay.specs[0].out0, p['T'], p['N'], p['ncols'], p['ld'], p['tstride'], lay.inp['nact'], drow, dquad)}


ZERO_MULTI = [case('zmulti-n%d-T%d-N%d-%s' % (len(w), T, N, 'x'.join(map(str, w))), why, T=T, N=N, widths=w, nact=nact)
              for w, T, N, nact, why in [
                  ((4,), 1, 1, (0,), 'one buffer, one quad'),
                  ((128,), 4, 7, (0, 7, 3, 6), 'one buffer: the boundary search never steps'),
                  ((4, 8), 4, 7, (6, 0, 7, 1), 'two buffers'),
                  ((16, 4, 4, 4, 4, 16), 4, 7, (0, 7, 3, 6), 'the encoder stack at H = 4: gates1, h1, c1, h2, c2, gates2'),
                  ((4, 8, 2048, 4, 512, 12), 4, 7, (2, 7, 0, 5), 'six unequal widths, one-quad buffers between wide ones'),
                  ((4, 8, 2048, 4, 512, 12), 1, 300, (17,), '183101 quads on 32768 threads: six grid-stride trips')]]


@cached
def zero_multi_layout(c):
    T, N, w = c.p['T'], c.p['N'], c.p['widths']
    rng = np.random.RandomState(T + N + sum(w))
    nact = np.array(c.p['nact'], I32)
    specs = []
    for i, nc in enumerate(w):
        out0 = marked(T * N * nc)
        out0[:T * N * nc] = rng.standard_normal(T * N * nc).astype(F32) + np.float32(3)
        specs.append(Spec('buf%d' % i, out0, _zero_expected(out0, T, N, nc, nc, N * nc, nact)))
    return Layout(c, {'nact': fin(nact, I32)}, specs)


def emulate_zero_multi(lay, mutant=None):
    """the kernel's walk: quad idx of (N - first) * per_row -> row idx / per_row, then the unrolled search for the buffer"""
    p = lay.case.p
    T, N, w = p['T'], p['N'], p['widths']
    drow, _ = ZERO_MUTANTS.get(mutant, (0, 0)) if mutant in ('one row too many', 'one row too few') else (0, 0)
    per_row = sum(x // 4 for x in w)
    outs = lay.out0()
    for t in range(T):
        first = max(0, min(N, int(lay.inp['nact'][t]) + drow))
        idx = np.arange((N - first) * per_row)
        r, q = idx // per_row, idx % per_row
        b = np.zeros_like(q)
        for i in range(5):
            lim = w[i] // 4 if i < len(w) else 0
            step = (b == i) & (i + 1 < len(w)) & ((q > lim) if mutant == 'buffer boundary off by one quad' else (q >= lim))
            q = np.where(step, q - lim, q)
            b = np.where(step, i + 1, b)
        for i in range(len(w)):
            sel = b == i
            base = ((t * N + first + r[sel]) * w[i] + q[sel] * 4)
            o = outs['buf%d' % i]
            at = (base[:, None] + np.arange(4)[None, :]).reshape(-1)
            o[at[at < o.size]] = 0.0
    return outs


# ------------------------------------------------------------------------------------------------------------ token_sort
TOKEN_SORT = [case('sort-V%d-n%d-%s' % (V, n, dist), why, V=V, n=n, dist=dist)
              for V, n, dist, why in [
                  (1, 0, 'one', 'V = 1, n = 0: offset = [0, 0], perm untouched'), (1, 1, 'one', 'one row'),
                  (1, 63, 'one', 'one token in every lane of a short wave'), (2, 64, 'half', 'a full wave, two tokens'),
                  (2, 65, 'last', 'a second wave for one row; only token V - 1'), (57, 0, 'one', 'n = 0 with V > 1'),
                  (57, 255, 'half', 'one short of a block; half pad'), (57, 5000, 'half', 'the shape of test_ops_gpu.py'),
                  (1023, 63, 'distinct', 'V one below the scan\'s threads; every lane its own token'),
                  (1023, 256, 'distinct', 'one block of distinct tokens'), (1024, 257, 'distinct', 'V at the scan\'s threads; a second block'),
                  (1024, 65, 'random', 'random tokens'), (1025, 64, 'one', 'V above the scan\'s threads (per = 2); one token in every lane'),
                  (1025, 256, 'last', 'only token 1024: the scan\'s last element'), (11323, 1, 'last', 'the full vocabulary, one row'),
                  (11323, 257, 'half', 'per = 12'), (11323, 5000, 'distinct', '5000 distinct tokens')]]


@cached
def token_sort_layout(c):
    V, n, dist = c.p['V'], c.p['n'], c.p['dist']
    rng = np.random.RandomState(V + n)
    if dist == 'one':
        tok = np.full(n, min(7, V - 1), I32)
    elif dist == 'last':
        tok = np.full(n, V - 1, I32)
    elif dist == 'distinct':
        tok = rng.permutation(V)[:n].astype(I32)
    else:
        tok = rng.randint(0, V, size=n).astype(I32)
        if dist == 'half':
            tok[rng.rand(n) < 0.5] = 0
    off0 = marked(V + 1, I32)
    want = off0.copy()
    want[:V + 1] = np.concatenate([[0], np.cumsum(np.bincount(tok, minlength=V))])
    own = np.zeros(n + GUARD, bool)
    own[:n] = True
    work_own = np.zeros(2 * V + GUARD, bool)
    work_own[:2 * V] = True                                        # scratch: any content, nothing behind 2 V
    tok.setflags(write=False)
    return Layout(c, {'tok': fin(tok, I32)},
                  [Spec('offset', off0, want), Spec('perm', marked(n, I32), bounded=own, ref=(tok, n), rule='perm'),
                   Spec('work', marked(2 * V, I32), bounded=work_own, ref=(np.zeros(0, I32), 2 * V), rule='scratch')], tokens=tok)


def emulate_token_sort(lay, mutant=None):
    V, n = lay.case.p['V'], lay.case.p['n']
    tok = lay.tokens
    o = lay.out0()
    count = np.bincount(tok, minlength=V)
    scan = np.concatenate([[0], np.cumsum(count)])
    if mutant == 'inclusive scan':
        scan = np.concatenate([np.cumsum(count), [n]])
    o['offset'][:V + 1] = scan
    if mutant == 'offset[V] missing':
        o['offset'][V] = IMARK
    rev = np.arange(n)[::-1]                                       # rows of one token in descending order: any order inside a token is right
    o['perm'][:n] = np.arange(n) if mutant == 'sorted by row' else rev[np.argsort(tok[rev], kind='stable')]
    o['work'][:V], o['work'][V:2 * V] = count, scan[1:]
    return o


# ------------------------------------------------------------------------------------------------------------ segment_rowsum_acc
SEGSUM = [case('segsum-n%d-c%d-ldx%d-ldo%d-%s' % (n, nc, nc + px, nc + po, dist), why, n=n, ncol=nc, ldx=nc + px, ldo=nc + po, V=V, dist=dist)
          for n, nc, px, po, V, dist, why in [
              (1, 4, 0, 0, 3, 'each', 'one row, one quad: cnt = 1, three clamped prefetches'),
              (3, 1020, 4, 0, 5, 'each', 'cnt % 4 = 3; one thread short of the 1024-column trip; ldx > ncol'),
              (4, 1024, 0, 4, 5, 'each', 'cnt % 4 = 0; exactly one trip (bf16: no second group); ldo > ncol'),
              (5, 1028, 4, 4, 4, 'runs', 'a second trip of thread 0 (bf16: the second group holds one quad)'),
              (5, 3072, 0, 0, 3, 'runs', 'three fp32 trips; bf16: a second trip whose second group is empty'),
              (3, 2052, 0, 0, 4, 'one', 'bf16: both groups full and a second trip of thread 0'),
              (255, 4, 4, 4, 300, 'each', 'one short of a chunk; a token change at every row'),
              (256, 1024, 0, 0, 7, 'runs', 'one full chunk'),
              (256, 2048, 4, 0, 9, 'half', 'two fp32 trips; bf16: both column groups full'),
              (257, 2048, 0, 4, 6, 'one', 'a second chunk of one row; one token through both chunks'),
              (257, 2052, 4, 4, 9, 'runs', 'chunk of one row, ragged third trip'),
              (600, 4, 0, 4, 600, 'each', 'three chunks, the last of 88 rows; every row its own token'),
              (600, 1028, 4, 0, 40, 'span3', 'the pad token\'s run of 560 rows spans all three chunks')]]


def _bf16_bits(x):
    return (bits(np.asarray(x, F32)) >> np.uint32(16)).astype(np.uint16)


def _bf16_values(b):
    return (b.astype(np.uint32) << np.uint32(16)).view(F32)


@cached
def segsum_layout(c, bf16):
    n, ncol, ldx, ldo, V, dist = (c.p[k] for k in ('n', 'ncol', 'ldx', 'ldo', 'V', 'dist'))
    rng = np.random.RandomState(n * 31 + ncol + (1 if bf16 else 0))
    if dist == 'each':
        tok = rng.permutation(V)[:n].astype(I32)
    elif dist == 'one':
        tok = np.full(n, 2, I32)
    else:
        tok = rng.randint(0, V, size=n).astype(I32)
        if dist in ('half', 'span3'):
            tok[rng.rand(n) < (0.5 if dist == 'half' else 1.0)] = 0
        if dist == 'span3':
            tok[rng.choice(n, 40, replace=False)] = rng.randint(1, V, size=40)
    perm = np.argsort(tok, kind='stable').astype(I32)
    x = rng.standard_normal((n, ncol)).astype(F32)
    if bf16:
        xb = _bf16_bits(x)
        x = _bf16_values(xb)
        xin = fin(strided(xb, ldx, NAN16, np.uint16), np.uint16)
    else:
        xin = fin(strided(x, ldx))
    o = strided(rng.standard_normal((V, ncol)).astype(F32), ldo, MARK)
    out0 = marked(V * ldo)
    out0[:V * ldo] = o.reshape(-1)
    ref, mag, cnt = o.astype(F64), np.abs(o).astype(F64), np.zeros((V, ldo))
    np.add.at(ref[:, :ncol], tok, x.astype(F64))
    np.add.at(mag[:, :ncol], tok, np.abs(x).astype(F64))
    np.add.at(cnt[:, :ncol], tok, 1.0)
    own = np.zeros(V * ldo + GUARD, bool)
    own[:V * ldo] = (cnt > 0).reshape(-1)
    full = lambda a: np.concatenate([a.reshape(-1), np.zeros(GUARD)])
    for a in (tok, perm, x):
        a.setflags(write=False)
    return Layout(c, {'X': xin, 'tok': fin(tok, I32), 'perm': fin(perm, I32)},
                  [Spec('out', out0, bounded=own, ref=full(ref), rule='elem', bnd=full((cnt + 4) * U * mag))], bf16=bf16, x=x, tokens=tok, perm=perm)


def segsum_mutant_applies(c, bf16, mutant):
    n, ncol, dist = c.p['n'], c.p['ncol'], c.p['dist']
    if mutant == 'clamp adds its duplicate row':
        return any(min(CHUNK, n - p0) % 4 for p0 in range(0, n, CHUNK))
    if mutant == 'second bf16 column group dropped':
        return bf16 and ncol > 1024
    if mutant == 'run flushed to the next token':
        return dist not in ('one',) and n > 1
    return True


def emulate_segsum(lay, mutant=None):
    """the kernel's order: each chunk of 256 sorted rows keeps the running sum of the current token and adds it to `out` when the token
    changes and at the end of the chunk"""
    p = lay.case.p
    n, ncol, ldo, V = p['n'], p['ncol'], p['ldo'], p['V']
    out = lay.specs[0].out0.copy()
    o = out[:V * ldo].reshape(V, ldo)
    x, tok, perm = lay.x, lay.tokens, lay.perm
    if mutant == 'second bf16 column group dropped':
        x = np.where((np.arange(ncol) % 2048 >= 1024)[None, :], np.float32(0), x)
    for p0 in range(0, n, CHUNK):
        rows = perm[p0:p0 + CHUNK]
        cur, acc = tok[rows[0]], np.zeros(ncol, F32)
        for r in rows:
            if tok[r] != cur:
                dst = tok[r] if mutant == 'run flushed to the next token' else cur
                o[dst, :ncol] = o[dst, :ncol] + acc
                cur, acc = tok[r], np.zeros(ncol, F32)
            acc = acc + x[r]
        if mutant == 'clamp adds its duplicate row':
            for _ in range((4 - len(rows) % 4) % 4):
                acc = acc + x[rows[-1]]
        if mutant == 'out overwritten':
            o[cur, :ncol] = acc
        else:
            o[cur, :ncol] = o[cur, :ncol] + acc
    return {'out': out}


# ------------------------------------------------------------------------------------------------------------ the heads: shared pieces
def lse64(x):
    x = np.asarray(x, F64)
    mx = x.max(-1, keepdims=True)
    return (mx + np.log(np.exp(x - mx).sum(-1, keepdims=True)))[..., 0]


def lse32(x, no_max=False):
    """fp32: max, sum of expf, logf; no_max: the mutant that leaves the max subtraction out"""
    x = np.asarray(x, F32)
    with np.errstate(over='ignore'):
        if no_max:
            return np.log(np.exp(x).sum(-1, dtype=F32))
        mx = x.max(-1, keepdims=True)
        return (mx + np.log(np.exp(x - mx).sum(-1, dtype=F32, keepdims=True)))[..., 0]


def head_rows(rng, rows, V, hot):
    """logits [rows x V], |x| <= 80.  hot: rows 0 and 1 hold +80 in column 0 ('first') / V - 1 ('last') against -80 elsewhere, or +80 in
    every column ('flat80')"""
    x = np.clip(rng.standard_normal((rows, V)) * 3.0, -80, 80).astype(F32)
    k = min(2, rows)
    if hot == 'flat80':
        x[:k] = 80.0
    elif hot:
        x[:k] = -80.0
        x[:k, 0 if hot == 'first' else V - 1] = 80.0
    return x


V_SET = (1, 2, 63, 64, 65, 255, 256, 257, 11322)
V_WHY = {1: 'one column: exactly +0', 2: 'two columns', 63: 'one short of a wave', 64: 'one wave', 65: 'one wave and a column',
         255: 'one short of the block', 256: 'one column per thread', 257: 'a second trip of thread 0', 11322: 'the vocabulary: 45 trips'}
HOT = [(65, 'first', 'row maximum +80 in column 0 against -80'), (257, 'last', 'row maximum +80 in column V - 1 against -80'),
       (11322, 'flat80', '+80 in every column: the plain sum of exp overflows fp32')]

# ------------------------------------------------------------------------------------------------------------ log_softmax_rows
LOGSOFTMAX = [case('lsm-V%d-pad%d-r%d' % (V, pad, rows), V_WHY[V], V=V, pad=pad, rows=rows, hot=None)
              for i, V in enumerate(V_SET) for pad, rows in (((0, 1), (2, 3)) if i % 2 == 0 else ((2, 1), (0, 3)))] + \
             [case('lsm-V%d-pad2-r3-%s' % (V, hot), why, V=V, pad=2, rows=3, hot=hot) for V, hot, why in HOT]


@cached
def logsoftmax_layout(c):
    V, pad, rows, hot = (c.p[k] for k in ('V', 'pad', 'rows', 'hot'))
    ld = V + pad
    x = head_rows(np.random.RandomState(V * 3 + pad + rows), rows, V, hot)
    out0 = marked(rows * ld)
    out0[:rows * ld] = strided(x, ld).reshape(-1)
    ref = np.zeros(rows * ld + GUARD)
    r2 = ref[:rows * ld].reshape(rows, ld)
    r2[:, :V] = x.astype(F64) - lse64(x)[:, None]
    if V == 1:                                                    # x - (x + log 1): exactly +0
        want = out0.copy()
        want.reshape(-1)[:rows * ld].reshape(rows, ld)[:, :V] = 0.0
        return Layout(c, {}, [Spec('x', out0, want)], x=x)
    own = np.zeros(rows * ld + GUARD, bool)
    own[:rows * ld].reshape(rows, ld)[:, :V] = True
    at = lambda r, col: np.asarray(r) * ld + np.asarray(col)
    slices = [('row maxima', at(np.arange(rows), x.argmax(1))), ('column 0', at(np.arange(rows), 0)), ('column V - 1', at(np.arange(rows), V - 1))]
    return Layout(c, {}, [Spec('x', out0, bounded=own, ref=ref, rule='proj', slices=slices)], x=x)


def emulate_logsoftmax(lay, mutant=None):
    V, pad, rows = (lay.case.p[k] for k in ('V', 'pad', 'rows'))
    ld = V + pad
    out = lay.specs[0].out0.copy()
    o = out[:rows * ld].reshape(rows, ld)
    n = V - 1 if mutant == 'last column dropped' else V
    with np.errstate(invalid='ignore'):
        o[:, :n] = lay.x[:, :n] - lse32(lay.x[:, :n], no_max=(mutant == 'lse without the max subtraction'))[:, None]
    return {'x': out}


# ------------------------------------------------------------------------------------------------------------ logsoftmax_nll
NLL_ROWS = 6                                                       # target column 0, column V - 1, pad input, pad target, two more
NLL = [case('nll-V%d-pad%d' % (V, pad), V_WHY[V], V=V, pad=pad, hot=None) for i, V in enumerate(V_SET) for pad in ((0, 3)[i % 2],)] + \
      [case('nll-V65-pad300', 'ld - V = 300: more pad columns than the 256 threads of a row (they were left as they were)', V=65, pad=300, hot=None),
       case('nll-V256-pad3', 'one column per thread and three pad columns', V=256, pad=3, hot=None)] + \
      [case('nll-V%d-pad3-%s' % (V, hot), why, V=V, pad=3, hot=hot) for V, hot, why in HOT]
NLL_VARIANTS = [(eps, wg) for eps in (0.0, 0.1) for wg in (0, 1)]


@cached
def nll_layout(c, eps, wg):
    import train_knobs_ref as kr
    V, pad, hot = c.p['V'], c.p['pad'], c.p['hot']
    rows, ld = NLL_ROWS, V + pad
    rng = np.random.RandomState(V * 5 + pad)
    x = head_rows(rng, rows, V, hot)
    tok_in = np.array([5, 9, 0, 4, 1, 2], I32)
    target = np.array([1, V, min(2, V), 0, rng.randint(1, V + 1), rng.randint(1, V + 1)], I32)
    live = (tok_in != 0) & (target > 0)
    x[~live] = np.nan                                             # a masked row is never read
    buf = strided(x, ld)
    with np.errstate(invalid='ignore'):
        loss, grad = kr.logsoftmax_nll(buf, V, tok_in, target, eps)
    n = rows * ld
    loss0 = marked(rows)
    lwant = loss0.copy()
    lwant[:rows][~live] = 0.0
    lown = np.zeros(rows + GUARD, bool)
    lown[:rows] = live
    specs = [Spec('loss', loss0, lwant, bounded=lown, ref=np.concatenate([loss, np.zeros(GUARD)]), rule='proj',
                  slices=[('target in column 0', np.array([0])), ('target in column V - 1', np.array([1]))])]
    out0 = marked(n)
    out0[:n] = buf.reshape(-1)
    extra = ()
    if wg:
        want = out0.copy()
        w2 = want[:n].reshape(rows, ld)
        w2[~live] = 0.0
        w2[:, V:] = 0.0
        own = np.zeros(n + GUARD, bool)
        own[:n].reshape(rows, ld)[live, :V] = True
        specs.append(Spec('logits', out0, want, bounded=own, ref=np.concatenate([grad.reshape(-1), np.zeros(GUARD)]), rule='rel'))

        def rowsums(outs):                                         # the exact sum of a gradient row is 0: within bound(0) = 1e-4
            g = outs['logits'][:n].reshape(rows, ld)[live, :V].astype(F64)
            worst = float(np.abs(g.sum(1)).max()) if np.isfinite(g).all() else np.inf
            return worst, worst / bound(np.zeros(1))
        extra = (('gradient row sums', rowsums),)
    else:
        specs.append(Spec('logits', out0))                         # write_grad = 0: untouched bit for bit
    return Layout(c, {'tok_in': fin(tok_in, I32), 'target': fin(target, I32)}, specs, extra=extra, x=x, live=live, eps=eps, wg=wg,
                  tok_in=tok_in, target=target)


def nll_mutant_applies(c, eps, wg, mutant):
    if mutant == 'pad columns left alone':
        return wg == 1 and c.p['pad'] > 0
    if mutant == 'pad columns beyond 256 left alone':
        return wg == 1 and c.p['pad'] > 256
    if mutant == 'lse without the max subtraction':
        return c.p['hot'] is not None
    if mutant == 'target off by one':
        return c.p['V'] > 1
    if mutant == 'logits written with write_grad = 0':
        return wg == 0
    return True


def emulate_nll(lay, mutant=None):
    V, pad = lay.case.p['V'], lay.case.p['pad']
    rows, ld, eps = NLL_ROWS, V + pad, np.float32(lay.eps)
    o = lay.out0()
    g = o['logits'][:rows * ld].reshape(rows, ld)
    wg = lay.wg or mutant == 'logits written with write_grad = 0'
    if wg and mutant != 'pad columns left alone':
        g[:, V:V + (256 if mutant == 'pad columns beyond 256 left alone' else pad)] = 0.0
    for r in range(rows):
        masked_row = lay.target[r] <= 0 or (lay.tok_in[r] == 0 and mutant != 'a masked row contributing')
        if masked_row:
            o['loss'][r] = 0.0
            if wg:
                g[r, :V] = 0.0
            continue
        x = lay.x[r]
        lse = lse32(x, no_max=(mutant == 'lse without the max subtraction'))
        tgt = (lay.target[r] - (0 if mutant == 'target off by one' else 1)) % V
        hot = (np.arange(V) == tgt).astype(F32)
        with np.errstate(invalid='ignore', over='ignore'):
            loss = lse - x[tgt]
            grad = np.exp(x - lse) - hot
            if lay.eps:
                loss = loss + eps * (x[tgt] - x.sum(dtype=F32) * (np.float32(1) / np.float32(V)))
                grad = grad + eps * (hot - np.float32(1) / np.float32(V))
        o['loss'][r] = loss
        if wg:
            g[r, :V] = grad
    return o


# ------------------------------------------------------------------------------------------------------------ score_ce
SCORE = [case('score-O%d-H%d-N%d-%s' % (O, H, N, mode + ('-pm80' if hot else '')), why, O=O, H=H, N=N, mode=mode, hot=hot)
         for O, H, N, mode, hot, why in [
             (1, 4, 1, 'train', False, 'one option, one lane: loss exactly +0, zero gradients'),
             (2, 252, 3, 'train', False, 'lane 63 idle; waves 2 and 3 without an option'),
             (63, 256, 3, 'train', False, 'one short of the lse wave; H at the 256-float lane stride'),
             (64, 260, 1, 'train', False, 'one option per lane; a second trip of lane 0'),
             (65, 1020, 3, 'train', False, 'a second lse trip of lane 0; thread 255 idle in the gradient loop'),
             (100, 1024, 3, 'train', False, 'the model\'s 100 options; H at the 1024-float thread stride'),
             (128, 1028, 3, 'train', False, 'MAX_OPT; a second gradient trip of thread 0'),
             (63, 1024, 1, 'train', False, 'N = 1 at the thread stride'),
             (128, 4, 3, 'train', True, 'scores of exactly +-80: the lse matters'),
             (65, 256, 3, 'scores', False, 'gt = NULL: scores only, loss_rows untouched'),
             (100, 260, 1, 'scores', False, 'scores only, N = 1'),
             (64, 1028, 3, 'loss', False, 'loss without gradients'),
             (2, 4, 1, 'loss', False, 'loss without gradients at the smallest shape')]]


@cached
def score_layout(c, eps):
    import train_knobs_ref as kr
    O, H, N, mode, hot = (c.p[k] for k in ('O', 'H', 'N', 'mode', 'hot'))
    rng = np.random.RandomState(O * 13 + H + N)
    optH = (rng.standard_normal((N, O, H)) * 0.2).astype(F32)
    enc = (rng.standard_normal((N, H)) * 0.2).astype(F32)
    gt = np.array([0, O - 1, min(3, O - 1)], I32)[:N] if N > 1 else np.array([(O - 1) * (H // 4 % 2)], I32)
    if hot:
        enc[:] = 0.0
        enc[:, 0] = 1.0
        optH[:, :, 0] = -80.0
        optH[:, [3, O - 2], 0] = 80.0
    gscale = float(np.float32(1.0 / N))
    ref = kr.score_ce(optH, enc, gt, eps, gscale)
    full = lambda a: np.concatenate([np.asarray(a, F64).reshape(-1), np.zeros(GUARD)])
    own = lambda n: np.concatenate([np.ones(n, bool), np.zeros(GUARD, bool)])
    sb = (H + 4) * U * np.einsum('noh,nh->no', np.abs(optH).astype(F64), np.abs(enc).astype(F64))
    specs = [Spec('scores', marked(N * O), bounded=own(N * O), ref=full(ref['scores']), rule='elem', bnd=full(sb))]
    if mode == 'scores':
        specs.append(Spec('loss', marked(N)))
    else:
        specs.append(Spec('loss', marked(N), bounded=own(N), ref=full(ref['loss_rows']), rule='proj',
                          slices=[('round %d' % i, np.array([i])) for i in range(N)]))
    if mode == 'train':
        specs += [Spec('dOptH', marked(N * O * H), bounded=own(N * O * H), ref=full(ref['dOptH']), rule='rel'),
                  Spec('dEnc', marked(N * H), bounded=own(N * H), ref=full(ref['dEnc']), rule='rel')]
    else:
        specs += [Spec('dOptH', marked(4)), Spec('dEnc', marked(4))]                       # not passed: NULL
    return Layout(c, {'optH': fin(optH), 'enc': fin(enc), 'gt': fin(gt, I32)}, specs, optH=optH, enc=enc, gt=gt, gscale=gscale, eps=eps)


def score_mutant_applies(c, mutant):
    if mutant == 'target off by one':
        return c.p['O'] > 1 and c.p['mode'] != 'scores'
    if mutant == 'gscale dropped':
        return c.p['N'] > 1 and c.p['mode'] == 'train' and c.p['O'] > 1
    if mutant == 'lse without the max subtraction':
        return c.p['hot']
    if mutant == 'last option dropped from the lse':
        return c.p['O'] > 1 and c.p['mode'] != 'scores'
    return True


def emulate_score(lay, mutant=None):
    O, H, N, mode = (lay.case.p[k] for k in ('O', 'H', 'N', 'mode'))
    o = lay.out0()
    optH, enc = lay.optH, lay.enc
    sc = (optH * enc[:, None, :]).sum(-1, dtype=F32)
    o['scores'][:N * O] = sc.reshape(-1)
    if mode == 'scores':
        return o
    gt = (lay.gt + (1 if mutant == 'target off by one' else 0)) % O
    eps, gscale = np.float32(lay.eps), np.float32(1.0 if mutant == 'gscale dropped' else lay.gscale)
    lse = lse32(sc[:, :O - 1] if mutant == 'last option dropped from the lse' else sc, no_max=(mutant == 'lse without the max subtraction'))
    hot = (np.arange(O)[None, :] == gt[:, None]).astype(F32)
    sg = sc[np.arange(N), gt]
    loss = lse - sg
    ds = np.exp(sc - lse[:, None]) - hot
    if lay.eps:
        invO = np.float32(1) / np.float32(O)
        loss = loss + eps * (sg - sc.sum(1, dtype=F32) * invO)
        ds = ds + eps * (hot - invO)
    ds = ds * gscale
    o['loss'][:N] = loss
    if mode == 'train':
        o['dOptH'][:N * O * H] = (ds[:, :, None] * enc[:, None, :]).reshape(-1)
        o['dEnc'][:N * H] = (ds[:, :, None] * optH).sum(1, dtype=F32).reshape(-1)
    return o


# ------------------------------------------------------------------------------------------------------------ ranks
RANK_KINDS = ('equal', 'distinct', 'pairs', 'zeros', 'inf')
RANKS = [case('ranks-O%d' % O, why, O=O) for O, why in [(1, 'one option: rank 1'), (2, 'two options'), (127, 'one thread idle'), (128, 'MAX_OPT')]]


def ranks_rule(s):
    """1 + #{j : s_j > s_o or (s_j == s_o and j < o)} per row"""
    s = np.asarray(s)
    j, o = np.arange(s.shape[1])[None, :, None], np.arange(s.shape[1])[None, None, :]
    sj, so = s[:, :, None], s[:, None, :]
    return (1 + ((sj > so) | ((sj == so) & (j < o))).sum(1)).astype(I32)


@cached
def ranks_layout(c):
    O = c.p['O']
    rng = np.random.RandomState(O)
    s = np.zeros((len(RANK_KINDS), O), F32)
    s[0] = 0.25                                                   # all equal: index order
    s[1] = rng.permutation(O).astype(F32) - O / 2                 # all distinct
    s[2] = (rng.permutation(O) // 2).astype(F32)                  # tie pairs
    s[3] = np.where(np.arange(O) % 2 == 0, np.float32(0.0), np.float32(-0.0))[rng.permutation(O)]     # +0 == -0: index order
    s[4] = rng.choice(np.array([np.inf, -np.inf, 1.0, -1.0], F32), size=O)
    out0 = marked(s.size, I32)
    want = out0.copy()
    want[:s.size] = ranks_rule(s).reshape(-1)
    return Layout(c, {'scores': fin(s)}, [Spec('ranks', out0, want)], N=len(RANK_KINDS), s=s)


def emulate_ranks(lay, mutant=None):
    s = lay.s
    o = lay.out0()
    if mutant == 'ties broken by higher index':
        r = ranks_rule(s[:, ::-1])[:, ::-1]
    else:                                                          # the descending stable sort position
        r = np.empty(s.shape, I32)
        for n in range(s.shape[0]):
            r[n, sorted(range(s.shape[1]), key=lambda j: -s[n, j])] = np.arange(1, s.shape[1] + 1)
    o['ranks'][:s.size] = r.reshape(-1)
    return o


FAMILIES = collections.OrderedDict([
    ('dropout_mask', DROPOUT), ('pointwise', POINTWISE), ('embed_gather', GATHER), ('embed_scatter_acc', SCATTER), ('mask_time', MASKTIME),
    ('zero_inactive_rows', ZERO_ROWS), ('zero_inactive_multi', ZERO_MULTI), ('token_sort', TOKEN_SORT), ('segment_rowsum_acc', SEGSUM),
    ('log_softmax_rows', LOGSOFTMAX), ('logsoftmax_nll', NLL), ('score_ce', SCORE), ('ranks', RANKS)])
for _name, _table in FAMILIES.items():
    assert len(set(c.id for c in _table)) == len(_table), _name
    assert all(c.why for c in _table), _name


def case_list():
    """the case list of profiles/helper_ops_parity.txt"""
    lines = []
    for name, table in FAMILIES.items():
        lines.append('%s (%d cases)' % (name, len(table)))
        lines += ['    %-44s %s' % (c.id, c.why) for c in table]
    return lines
