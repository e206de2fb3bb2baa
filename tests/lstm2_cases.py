"""Case table, fp64 reference, checker and float32 emulation for the two-layer skewed wavefront of csrc/lstm.hip (vd_lstm2_forward[_flags] /
vd_lstm2_backward[_flags]); no GPU needed: the arrangement of tests/gemm_cases.py and tests/lhood_cases.py.

  * `SHAPES` / `CASES`: a case is an H, an arithmetic (`fp32` | `bf16`) and one or two stacks (T, N, nact or None).
  * `operands(shape_id)`: tokens, weights, the buffers of a forward and of a backward call as the runtime passes them, and the fp64
    reference of both (oracle.visdial_oracle.lstm_forward / lstm_backward on the two layers; pinned to torch autograd by the CPU test).
      - with `nact` the rows are in order of descending length and row n is pad before step T - len[n] (runtime.hip upload_tokens); inside
        its span a row holds zeros at some interior and trailing steps, which tok_mask must still mask; gates1 has its dead rows zeroed and
        h1, c1, gates2, h2, c2 (forward), dh1_seq, dc1, dc2 (backward) are zero-filled (include/visdial_hip.h);
      - without `nact` the rows are right-aligned with lengths 0..T and every output buffer starts from FILL, since every row is written;
      - rows that are live at NO step (>= max_t nact[t]) hold NaN in every buffer, input or output: a correct call neither reads nor
        writes them;
      - every buffer is followed by GUARD elements of MARK;
      - backward operands are the fp64 forward state rounded to fp32 and the backward reference starts from those rounded values, so the
        backward arithmetic alone is measured (tests/test_lstm_dispatch_gpu.py).
  * `check(case, direction, got)`: pass / fail of what a call left behind.  Every output against the reference on the whole tensor, on each
    step's live rows and on each step's LAST LIVE ROW TILE alone (rows 32 * ((n - 1) // 32) .. n - 1), rel-L2 against the slice's own
    reference norm; a slice whose reference is all zero must come back exactly zero.  With nact, rows >= nact[t] of every written buffer
    hold what was put there (zero bit for bit, NaN where never live).  Guards unchanged, no NaN in a live element.  dc1 / dc2 are checked
    on the rows of the last step: a row that is pad before step t0 keeps the dc that flows into step t0 (dL/dc0 of its own sequence).
  * `emulate(case, direction, mutant)`: a numpy float32 model of a correct call on those buffers, and one mutant per mistake the kernels
    could make; `MUTANTS` names the case that catches each (tests/test_lstm2_cases_cpu.py).

Bounds: the project's own, those of tests/test_ops_gpu.py::test_lstm2_wavefront_matches_oracle -- fp32 1e-5 forward, 2e-5 backward; bf16
(both operands of every product rounded to bf16, fp32 accumulate and state) 1e-2 forward, 2e-2 backward.  The float32 emulation of this
file stays at or below 3.5e-7 on every slice of every case, single rows included, so the fp32 bounds leave about 30x over a correct fp32
evaluation.  No bound here is taken from the code under test."""
import collections
import functools

import numpy as np

from oracle import visdial_oracle as vo

TILE = 32                                # rows per tile of the tick configs (CfgFwdSmallC, CfgBwdSmallD and their bf16 twins)
GUARD = 64                               # marked elements behind every buffer
MARK = np.float32(-7.25e3)
FILL = np.float32(0.75)                  # what an output buffer holds before a call that writes every row of it
D, V = 20, 30                            # input width and vocabulary of the layer-1 projection

BOUNDS = {('fp32', 'fwd'): 1e-5, ('fp32', 'bwd'): 2e-5, ('bf16', 'fwd'): 1e-2, ('bf16', 'bwd'): 2e-2}

FWD_OUT = ('gates1', 'h1', 'c1', 'gates2', 'h2', 'c2')
BWD_OUT = ('gates1', 'gates2', 'dh1_seq', 'dc1', 'dc2')
BWD_IN = ('c1', 'c2', 'dh_last2')

# id, H, stacks (T, N, nact)
SHAPES = collections.OrderedDict((s[0], s) for s in [
    ('one-row', 32, [(1, 1, None)]),                                          # only K = 0 cell tiles and one K = H projection; one column tile
    ('short-ragged', 32, [(2, 33, None)]),                                    # T < 3: L1 finishes before L2 starts; 32 + 1 rows
    ('odd-H-mixed', 96, [(3, 40, None), (1, 70, None)]),                      # H no power of two; one stack ends while the other runs
    ('live-two', 64, [(7, 70, [0, 0, 5, 32, 33, 64, 70]), (4, 70, [1, 1, 70, 70])]),   # no live row; counts at, over, far from a tile; nact = N
    ('never-live', 128, [(3, 130, [0, 31, 97])]),                             # rows 97..129 live at no step; a tick with no problem at all
    ('wide', 512, [(2, 40, [8, 40])]),                                        # the model's width: 16 forward column tiles
    ('wide-dead', 512, [(2, 40, [8, 33])]),                                   # the same width with rows that are never live (NaN) in a ragged tile
    ('mixed-nact', 64, [(3, 64, [10, 40, 64]), (5, 33, None)]),               # counts beside no counts in the same launches
    ('tile-rows', 32, [(3, 64, None)]),                                       # N a multiple of 32 without counts
])

Case = collections.namedtuple('Case', 'id shape H arith stacks')
CASES = [Case('%s-%s' % (sid, arith), sid, H, arith, stacks) for sid, H, stacks in SHAPES.values() for arith in ('fp32', 'bf16')]


def case(cid):
    return next(c for c in CASES if c.id == cid)


def buf(a):
    """a flat float32 copy of `a` in front of GUARD marked elements"""
    a = np.asarray(a, np.float32).reshape(-1)
    return np.concatenate([a, np.full(GUARD, MARK, np.float32)])


def lengths_of(T, N, nact):
    """row n is live from step T - len[n] on: the lengths that `nact` (non-decreasing) claims"""
    ln = np.zeros(N, np.int64)
    for t in range(T - 1, -1, -1):
        ln[:nact[t]] = T - t
    return ln


def make_tokens(rng, T, N, nact):
    tok = rng.randint(1, V + 1, size=(T, N)).astype(np.int32)
    if nact is None:
        ln = rng.randint(0, T + 1, size=N)
        ln[0] = T                                  # one full row; one empty row, which ends in a zero token (h[T-1] = 0)
        if N > 1:
            ln[1] = 0
        for n in range(N):
            tok[:T - ln[n], n] = 0
        return tok
    ln = lengths_of(T, N, nact)
    for n in range(N):
        tok[:T - ln[n], n] = 0
    # zeros inside the claimed span (upload_tokens: masked per token there): never at the row's first claimed step, so the counts stay tight
    for n in range(N):
        if ln[n] >= 3 and (n % 4 == 1 or n == nact[-1] - 1):
            tok[T - ln[n] + 1 + rng.randint(0, ln[n] - 2), n] = 0      # interior
        if ln[n] >= 2 and (n % 4 == 0):
            tok[T - 1, n] = 0                                          # trailing: h[T-1] = 0 for this row
    return tok


class Stack(object):
    """one stack of a shape: operands, initial buffers of both calls and their fp64 references"""


@functools.lru_cache(maxsize=None)
def operands(shape_id):
    _, H, stacks = SHAPES[shape_id]
    rng = np.random.RandomState(sum(map(ord, shape_id)))
    out = []
    d = np.float64
    for T, N, nact in stacks:
        s = Stack()
        s.T, s.N, s.H = T, N, H
        s.nact = None if nact is None else np.ascontiguousarray(nact, dtype=np.int32)
        s.live = np.full(T, N, np.int64) if nact is None else np.asarray(nact, np.int64)
        s.never = N if nact is None else int(max(nact))               # rows >= never are live at no step
        s.tok = make_tokens(rng, T, N, nact)
        f32 = lambda *shape: rng.randn(*shape).astype(np.float32)
        emb = f32(V + 1, D); emb[0] = 0
        W1 = (f32(D + H, 4 * H) / np.sqrt(D + H)).astype(np.float32); b1 = f32(4 * H) * np.float32(0.1)
        W2 = (f32(2 * H, 4 * H) / np.sqrt(2 * H)).astype(np.float32); b2 = f32(4 * H) * np.float32(0.1)
        s.Wh1, s.Wx2, s.b2, s.Wh2 = (np.ascontiguousarray(a) for a in (W1[D:], W2[:H], b2, W2[H:]))
        s.W1, s.b1, s.W2 = W1, b1, W2
        s.x = emb[s.tok]
        s.dlast = f32(N, H)
        # fp64 reference, composed as tests/test_ops_gpu.py::test_lstm2_wavefront_matches_oracle composes it
        h1, c1, g1 = vo.lstm_forward(s.x.astype(d), W1.astype(d), b1.astype(d), s.tok)
        h2, c2, g2 = vo.lstm_forward(h1, W2.astype(d), b2.astype(d), s.tok)
        s.ref_fwd = dict(gates1=g1, h1=h1, c1=c1, gates2=g2, h2=h2, c2=c2)
        r = lambda a: a.astype(np.float32).astype(d)                   # the backward starts from the ROUNDED forward state
        dx2, _, _, _, dc2, da2 = vo.lstm_backward(r(h1), W2.astype(d), r(g2), r(h2), r(c2), dh_last=s.dlast.astype(d), return_da=True)
        _, _, _, _, dc1, da1 = vo.lstm_backward(s.x.astype(d), W1.astype(d), r(g1), r(h1), r(c1), dh_seq=dx2, return_da=True)
        if nact is not None:
            # a row that is pad before step t0 is not touched there: its dc stops at what flows INTO step t0, which is dL/dc0 of the row's own
            # sequence [t0, T) (its state before t0 is zero).  The oracle on that sequence, for the rows of each t0 > 0
            t0s = T - lengths_of(T, N, nact)
            for t0 in sorted(set(t0s[:s.never]) - {0}):
                q = np.where(t0s == t0)[0]
                cut = lambda a: r(a)[t0:, q]
                dc2[q] = vo.lstm_backward(cut(h1), W2.astype(d), cut(g2), cut(h2), cut(c2), dh_last=s.dlast.astype(d)[q])[4]
                dc1[q] = vo.lstm_backward(s.x.astype(d)[t0:, q], W1.astype(d), cut(g1), cut(h1), cut(c1), dh_seq=dx2[t0:, q])[4]
        s.ref_bwd = dict(gates1=da1, gates2=da2, dh1_seq=dx2, dc1=dc1, dc2=dc2)

        dead = np.arange(N)[None, :] >= s.live[:, None]                # [T, N]

        def prep(a, zero_dead):
            """the initial contents of a buffer: a copy with dead rows zeroed (if asked) and never-live rows NaN"""
            a = np.array(a, np.float32)
            if zero_dead:
                a[dead] = 0
            a[..., s.never:, :] = np.nan
            return buf(a)

        xw = (s.x.reshape(T * N, D).astype(d) @ W1[:D].astype(d) + b1).astype(np.float32).reshape(T, N, 4 * H)
        blank = lambda *shape: np.full(shape, 0 if nact is not None else FILL, np.float32)
        s.fwd0 = dict(gates1=prep(xw, nact is not None), h1=prep(blank(T, N, H), False), c1=prep(blank(T, N, H), False),
                      gates2=prep(blank(T, N, 4 * H), False), h2=prep(blank(T, N, H), False), c2=prep(blank(T, N, H), False))
        s.bwd0 = dict(gates1=prep(g1, False), gates2=prep(g2, False), c1=prep(c1, False), c2=prep(c2, False), dh_last2=prep(s.dlast, False),
                      dh1_seq=prep(blank(T, N, H), False), dc1=prep(blank(N, H), False), dc2=prep(blank(N, H), False))
        out.append(s)
    return tuple(out)


def width(name, H):
    return 4 * H if name.startswith('gates') else H


def view(s, name, flat):
    """the [T x N x C] view ([1 x N x C] for dc1, dc2, dh_last2) of a flat buffer, without its guard"""
    C = width(name, s.H)
    T = 1 if name in ('dc1', 'dc2', 'dh_last2') else s.T
    return flat[:T * s.N * C].reshape(T, s.N, C)


def live_of(s, name):
    """live rows per step of a buffer; dc1 / dc2 are written for the rows of the last step"""
    return s.live[-1:] if name in ('dc1', 'dc2', 'dh_last2') else s.live


# ------------------------------------------------------------------------------------------------------------ the checker
def rel_l2(got, ref):
    """rel-L2 of a slice against its own reference norm; an all-zero reference asks for exact zeros (inf otherwise)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    nr = float(np.linalg.norm(ref))
    if nr == 0.0:
        return 0.0 if not np.any(got != 0) else float('inf')
    e = float(np.linalg.norm(got - ref)) / nr
    return e if e == e else float('inf')


def slices(s, name):
    """(label, step, row0, row1) of every checked slice of an output: whole, each step's live rows, each step's last live row tile"""
    lv = live_of(s, name)
    out = [('whole', None, 0, s.never)]
    for t, n in enumerate(lv):
        n = int(n)
        if n > 0:
            out.append(('t%d live' % t, t, 0, n))
            out.append(('t%d tile' % t, t, TILE * ((n - 1) // TILE), n))
    return out


Report = collections.namedtuple('Report', 'ok failures worst')


def check(c, direction, got):
    """`got`: per stack, {buffer name -> flat float32 array, guard included} as a forward ('fwd') or backward ('bwd') call left them.
    Returns Report(ok, failures, worst): worst[(stack, name)] = (largest slice error / its bound, error, bound, slice label)."""
    stacks = operands(c.shape)
    names = FWD_OUT if direction == 'fwd' else BWD_OUT
    init = 'fwd0' if direction == 'fwd' else 'bwd0'
    fails, worst = [], {}
    for si, (s, g) in enumerate(zip(stacks, got)):
        ref = s.ref_fwd if direction == 'fwd' else s.ref_bwd
        for name in names:
            flat, flat0 = np.asarray(g[name]), getattr(s, init)[name]
            tag = '%s %s stack %d %s' % (c.id, direction, si, name)
            if flat.dtype != np.float32 or flat.shape != flat0.shape:
                fails.append('%s: buffer of %s %s, expected float32 %s' % (tag, flat.dtype, flat.shape, flat0.shape))
                continue
            if not np.array_equal(flat[-GUARD:], flat0[-GUARD:]):
                fails.append('%s: guard overwritten' % tag)
            a, a0 = view(s, name, flat), view(s, name, flat0)
            rf = np.asarray(ref[name]).reshape(a.shape)
            lv = live_of(s, name)
            for t, n in enumerate(lv):
                n = int(n)
                if np.isnan(a[t, :n]).any():
                    fails.append('%s: NaN in a live row of step %d' % (tag, t))
                if s.nact is not None and a[t, n:].tobytes() != a0[t, n:].tobytes():      # bit for bit; NaN rows keep their NaN
                    fails.append('%s: step %d wrote rows >= nact = %d' % (tag, t, n))
            for label, t, r0, r1 in slices(s, name):
                e = rel_l2(a[:, r0:r1] if t is None else a[t, r0:r1], rf[:, r0:r1] if t is None else rf[t, r0:r1])
                b = BOUNDS[c.arith, direction]
                if not e < b:
                    fails.append('%s: %s rel-L2 %.3e, bound %.1e' % (tag, label, e, b))
                if (si, name) not in worst or e / b > worst[si, name][0]:
                    worst[si, name] = (e / b, e, b, label)
    return Report(not fails, fails, worst)


def assert_ok(c, direction, got):
    rep = check(c, direction, got)
    assert rep.ok, '\n'.join(rep.failures[:12])
    return rep


# ------------------------------------------------------------------------------------------------------------ float32 emulation, mutants
# mutant -> the case that catches it (tests/test_lstm2_cases_cpu.py holds every one of them to that)
MUTANTS = collections.OrderedDict([
    ('ragged_last_row', 'short-ragged-fp32'),      # the last row of a ragged tile is not stored
    ('round_up_rows', 'never-live-fp32'),          # rows up to the next multiple of 32 beyond nact[t] are written
    ('stale_mask', 'live-two-fp32'),               # the mask of step t - 1 is used at step t
    ('no_b2', 'one-row-fp32'),                     # b2 is dropped from the layer-2 projection
    ('dc_first_ignored', 'one-row-fp32'),          # dc_first is ignored at the last step: dc_next is read from the buffer
    ('dc_first_always', 'short-ragged-fp32'),      # dc_first is applied at every step
    ('k0_reads_h0', 'one-row-fp32'),               # the K = 0 tick reads h[0] as a previous state
    ('dh1_from_next', 'short-ragged-fp32'),        # dh1_seq[t] is taken from da2[t + 1]
    ('wh2_of_stack0', 'mixed-nact-fp32'),          # layer 2 of the second stack reads the first stack's Wh2
    ('h_pow2_colmap', 'odd-H-mixed-fp32'),         # the g * H + jb * 32 + jj column map with H rounded up to a power of two
    ('guard_overwrite', 'one-row-fp32'),           # one element behind a buffer is written
    ('skip_masked_store', 'live-two-fp32'),        # a masked row inside the live span is skipped instead of zeroed
])


def sigmoid32(x):
    return (np.float32(1) / (np.float32(1) + np.exp(-x))).astype(np.float32)


def stored_rows(n, N, mutant, counted):
    """the rows a tick stores for a live count n"""
    if mutant == 'ragged_last_row' and n % TILE:
        return n - 1
    if mutant == 'round_up_rows' and counted:
        return min(N, -(-n // TILE) * TILE)
    return n


def colmap(W, H, mutant):
    """SrcKSel: column vc of a gate tile reads weight column g * H + j"""
    if mutant != 'h_pow2_colmap':
        return W
    Hp = 1 << (H - 1).bit_length()
    c = np.arange(4 * H)
    return W[:, ((c // Hp) * H + c % Hp) % (4 * H)]


def emulate(c, direction, mutant=None):
    """what a correct call (or the mutant) leaves behind, in float32 numpy, on copies of the case's initial buffers"""
    stacks = operands(c.shape)
    got = []
    for si, s in enumerate(stacks):
        T, N, H = s.T, s.N, s.H
        counted = s.nact is not None
        Wh2 = stacks[0].Wh2 if (mutant == 'wh2_of_stack0' and si == 1) else s.Wh2
        if direction == 'fwd':
            g = {k: v.copy() for k, v in s.fwd0.items()}
            A = {k: view(s, k, g[k]) for k in g}                       # views: writes land in the flat buffers
            for layer in (1, 2):
                gates, h, cc = A['gates%d' % layer], A['h%d' % layer], A['c%d' % layer]
                Wh = colmap(s.Wh1 if layer == 1 else Wh2, H, mutant)
                for t in range(T):
                    if s.live[t] <= 0:
                        continue
                    n = stored_rows(int(s.live[t]), N, mutant, counted)
                    if layer == 2:                                     # the layer-2 input projection of step t
                        p = A['h1'][t, :n] @ s.Wx2
                        gates[t, :n] = p if mutant == 'no_b2' else p + s.b2
                    a = gates[t, :n].copy()
                    if t:
                        a += h[t - 1, :n] @ Wh
                    elif mutant == 'k0_reads_h0':
                        a += h[0, :n] @ Wh
                    i, f, o = sigmoid32(a[:, :H]), sigmoid32(a[:, H:2 * H]), sigmoid32(a[:, 2 * H:3 * H])
                    gg = np.tanh(a[:, 3 * H:])
                    cn = i * gg + (f * cc[t - 1, :n] if t else 0)
                    hn = o * np.tanh(cn)
                    keep = (s.tok[t - 1 if (mutant == 'stale_mask' and t) else t, :n] != 0)
                    new = [np.where(keep[:, None], v, np.float32(0)) for v in (np.concatenate([i, f, o, gg], 1), hn, cn)]
                    rows = keep if mutant == 'skip_masked_store' else slice(None)
                    for dst, val in zip((gates, h, cc), new):
                        dst[t, :n][rows] = val[rows]
            if mutant == 'guard_overwrite':
                g['h2'][T * N * H] = 0
        else:
            g = {k: v.copy() for k, v in s.bwd0.items()}
            A = {k: view(s, k, g[k]) for k in g}
            for layer in (2, 1):
                gates, cc, dc = A['gates%d' % layer], A['c%d' % layer], A['dc%d' % layer][0]
                Wh = s.Wh1 if layer == 1 else Wh2
                for t in range(T - 1, -1, -1):
                    if s.live[t] <= 0:
                        continue
                    n = stored_rows(int(s.live[t]), N, mutant, counted)
                    last = t == T - 1
                    dh = np.zeros((n, H), np.float32)
                    if not last:
                        dh += gates[t + 1, :n] @ Wh.T
                    if layer == 2 and last:
                        dh += A['dh_last2'][0, :n]
                    if layer == 1:
                        dh += A['dh1_seq'][t, :n]
                    i, f, o, gg = (gates[t, :n, k * H:(k + 1) * H].copy() for k in range(4))
                    tc = np.tanh(cc[t, :n])
                    first = (last and mutant != 'dc_first_ignored') or mutant == 'dc_first_always'
                    dcn = dh * o * (1 - tc * tc) + (0 if first else dc[:n])
                    cp = cc[t - 1, :n] if t else np.zeros((n, H), np.float32)
                    gates[t, :n] = np.concatenate([dcn * gg * i * (1 - i), dcn * cp * f * (1 - f), dh * tc * o * (1 - o), dcn * i * (1 - gg * gg)], 1)
                    dc[:n] = dcn * f
                    if layer == 2:                                     # dh1[t] = da2[t] * Wx2^T
                        src = gates[t + 1, :n] if (mutant == 'dh1_from_next' and not last) else gates[t, :n]
                        A['dh1_seq'][t, :n] = src @ s.Wx2.T
            if mutant == 'guard_overwrite':
                g['dc2'][N * H] = 0
        got.append(g)
    return got
