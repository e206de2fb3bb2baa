"""Operator parity for the training knobs (internal entry points, csrc/rt_core.h, bound by visdial_amd._lib.internal) against
the fp64 restatement tests/train_knobs_ref.py (pinned to torch on the CPU by tests/test_train_knobs_cpu.py):

  1. the smoothed discriminative head (csrc/loss.hip LS1) at one option, two options, the ops suite's shape and the most options a round
     holds: loss rows, dOptH and dEnc; one option gives the plain kernel's bits;
  2. the smoothed generative head (LS2) at one word, a ragged small vocabulary and the full one with its two alignment columns: live rows,
     a pad-input row, a pad-target row and an empty row, the pad columns, and the forward-only form;
  3. the global norm, its scale and the clipped / decayed update (csrc/elementwise.hip GC1-GC3, WD1) at every tail of the float4 path, one
     and many workgroups and more than one trip of the grid-stride loop, with the norm below, equal to and above c and with an inf in
     the gradient; two calls give the same bits.

Bounds: rel-L2 < 1e-5 against fp64 for every output of a head -- what test_ops_gpu.py holds the plain heads to; the added arithmetic is
one more reduction of the same length.  The update: w < 1e-6 and m, v < 5e-5 as test_clamp_adam; the norm within 1e-5 relative of fp64
(a thread adds at most a few dozen squares serially in front of a tree of <= 20 levels); the written-back gradient < 1.5e-5, because it
carries the scale c / norm -- the norm's bound -- and two fp32 products.  A reference that is exactly zero (one class: loss and gradient
vanish) is matched exactly.  Every output lies in front of guard elements that must stay untouched."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import train_knobs_ref as tk

pytestmark = pytest.mark.gpu

BOUND = 1e-5
D = np.float64
GUARD = 64
MARK = 7.25


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from visdial_amd import ops as o
    return o


@pytest.fixture(scope="module")
def internal(ops):
    from visdial_amd import _lib
    return types.SimpleNamespace(
        score_ce=_lib.internal('vd_score_ce_p'), logsoftmax_nll=_lib.internal('vd_logsoftmax_nll_p'),
        clip_scale=_lib.internal('vd_grad_clip_scale_p'), clip_decay_adam=_lib.internal('vd_clip_decay_adam_p'),
        work_floats=int(_lib.internal('vd_clip_work_floats', C.c_int64)()))


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def f32(rng, *shape):
    return rng.randn(*shape).astype(np.float32)


def guarded(a):
    """`a` on the device in front of GUARD marked elements: (the whole buffer, the view of a)"""
    a = np.ascontiguousarray(a)
    buf = torch.full((a.size + GUARD,), MARK, dtype=torch.from_numpy(a).dtype, device='cuda')
    buf[:a.size] = torch.from_numpy(a.reshape(-1)).cuda()
    return buf, buf[:a.size].view(*a.shape)


def guard_ok(buf):
    return bool((buf[-GUARD:] == MARK).all().item())


def err(got, ref):
    """rel-L2 against fp64; an exactly zero reference is matched exactly"""
    got, ref = np.asarray(got.cpu().numpy() if torch.is_tensor(got) else got, D), np.asarray(ref, D)
    nr = np.linalg.norm(ref)
    if nr == 0.0:
        return 0.0 if not got.any() else np.inf
    return float(np.linalg.norm(got - ref) / nr)


# ------------------------------------------------------------------------------------------------------------ 1. disc head
@pytest.mark.parametrize("N, O, H", [(1, 1, 4), (3, 2, 4), (23, 100, 512), (2, 128, 512)])
@pytest.mark.parametrize("eps", [0.1, 0.6])
def test_smoothed_score_ce(ops, internal, N, O, H, eps):
    rng = np.random.RandomState(N * 1009 + O * 31 + H)
    sc = np.float32(0.2 if H >= 64 else 1.0)
    optH, enc = f32(rng, N, O, H) * sc, f32(rng, N, H) * sc
    gt = rng.randint(0, O, size=N).astype(np.int32)
    gscale = 1.0 / N
    ref = tk.score_ce(optH, enc, gt, eps, gscale)
    d_optH, d_enc, d_gt = (torch.from_numpy(a).cuda() for a in (optH, enc, gt))

    def run(smooth):
        out = types.SimpleNamespace()
        for k, shape in (('scores', (N, O)), ('loss_rows', (N,)), ('dOptH', (N, O, H)), ('dEnc', (N, H))):
            b, v = guarded(np.zeros(shape, np.float32))
            setattr(out, k + '_buf', b)
            setattr(out, k, v)
        internal.score_ce(ptr(d_optH), ptr(d_enc), ptr(d_gt), ptr(out.scores), ptr(out.loss_rows), ptr(out.dOptH), ptr(out.dEnc), N, O, H,
                          gscale, smooth, stream())
        torch.cuda.synchronize()
        assert all(guard_ok(getattr(out, k + '_buf')) for k in ('scores', 'loss_rows', 'dOptH', 'dEnc'))
        return out
    got = run(eps)
    figures = {k: err(getattr(got, k), ref[k]) for k in ('scores', 'loss_rows', 'dOptH', 'dEnc')}
    print('score_ce (%d, %d, %d) eps %g: %s' % (N, O, H, eps, figures))
    assert all(v < BOUND for v in figures.values()), figures
    plain = run(0.0)                                                              # smooth = 0 is vd_score_ce itself
    want = types.SimpleNamespace(**{k: torch.zeros_like(getattr(plain, k)) for k in ('scores', 'loss_rows', 'dOptH', 'dEnc')})
    ops.score_ce(d_optH, d_enc, want.scores, N, O, H, gt=d_gt, loss_rows=want.loss_rows, dOptH=want.dOptH, dEnc=want.dEnc, gscale=gscale)
    for k in ('scores', 'loss_rows', 'dOptH', 'dEnc'):
        assert torch.equal(getattr(plain, k), getattr(want, k)), k
        if O == 1:                                                                # one class: the smoothed target is the one-hot one
            assert torch.equal(getattr(got, k), getattr(want, k)), k
    if O > 1:                                                                     # ... and with more it is not
        assert not torch.equal(got.dEnc, want.dEnc) and not torch.equal(got.loss_rows, want.loss_rows)
    # forward-only keeps its form: loss rows without gradients
    rows = torch.zeros(N, device='cuda')
    internal.score_ce(ptr(d_optH), ptr(d_enc), ptr(d_gt), ptr(torch.zeros(N, O, device='cuda')), ptr(rows), None, None, N, O, H, gscale, eps,
                      stream())
    assert torch.equal(rows, got.loss_rows)


# ------------------------------------------------------------------------------------------------------------ 2. gen head
@pytest.mark.parametrize("V, ld", [(1, 4), (5, 8), (11322, 11324)])
@pytest.mark.parametrize("eps", [0.1, 0.6])
def test_smoothed_logsoftmax_nll(ops, internal, V, ld, eps):
    rng = np.random.RandomState(V + ld)
    rows = 9
    x = f32(rng, rows, ld) * np.float32(2.0)
    x[:, V:] = MARK                                                               # the alignment columns hold anything before the call
    tok_in = rng.randint(1, V + 1, size=rows).astype(np.int32)
    target = rng.randint(1, V + 1, size=rows).astype(np.int32)
    target[0], target[rows - 1] = 1, V                                            # the first and the last valid column
    tok_in[2] = 0                                                                 # a pad-input row
    target[4] = 0                                                                 # a pad-target row
    tok_in[6] = target[6] = 0                                                     # an empty row
    loss_ref, grad_ref = tk.logsoftmax_nll(x, V, tok_in, target, eps)
    d_in, d_tg = torch.from_numpy(tok_in).cuda(), torch.from_numpy(target).cuda()

    def run(write_grad, smooth):
        lbuf, logits = guarded(x)
        rbuf, loss = guarded(np.zeros(rows, np.float32))
        internal.logsoftmax_nll(ptr(logits), ld, rows, V, ptr(d_in), ptr(d_tg), ptr(loss), write_grad, smooth, stream())
        torch.cuda.synchronize()
        assert guard_ok(lbuf) and guard_ok(rbuf)
        return logits, loss
    grad, loss = run(1, eps)
    figures = dict(loss_rows=err(loss, loss_ref), grad=err(grad, grad_ref))
    print('logsoftmax_nll (%d, %d) eps %g: %s' % (V, ld, eps, figures))
    assert all(v < BOUND for v in figures.values()), figures
    g = grad.cpu().numpy()
    assert not g[[2, 4, 6]].any() and not loss.cpu().numpy()[[2, 4, 6]].any()     # masked rows stay exactly zero
    assert not g[:, V:].any()                                                     # the pad columns stay 0
    live = [r for r in range(rows) if r not in (2, 4, 6)]
    if V > 1:
        assert np.abs(g[live, :V].sum(1)).max() < 1e-5                            # softmax - t sums to 0 over the valid columns
    kept, loss_fwd = run(0, eps)                                                  # forward-only: the same loss, the logits untouched
    assert torch.equal(loss_fwd, loss) and np.array_equal(kept.cpu().numpy(), x)
    # smooth = 0 is vd_logsoftmax_nll itself
    plain, loss_plain = run(1, 0.0)
    want = torch.from_numpy(x).cuda()
    want_loss = torch.zeros(rows, device='cuda')
    ops.logsoftmax_nll(want, V, d_in, d_tg, want_loss, write_grad=True)
    assert torch.equal(plain, want) and torch.equal(loss_plain, want_loss)
    if V == 1:
        assert torch.equal(grad, want) and torch.equal(loss, want_loss)           # one class: the plain head's bits


# ------------------------------------------------------------------------------------------------------------ 3. norm + update
SIZES = [1, 3, 4, 1023, 4097, 2 ** 20 + 3, 3 * 2 ** 20 + 5]      # tails 1 / 3 / 0, one and several workgroups, 1024 of them, several trips
GSCALE, STEP, DECAY = 0.5, 1e-3 * np.sqrt(1 - 0.999) / (1 - 0.9), 1e-3 * 0.1


def update_case(n, kind):
    rng = np.random.RandomState(n % 100003 + len(kind))
    w, m, v = f32(rng, n), f32(rng, n) * np.float32(0.1), (rng.rand(n) * 0.1).astype(np.float32)
    if kind == 'equal':      # || 0.5 g || = 2 exactly in any order of summation: four elements of 2 (or one of 4)
        g = np.zeros(n, np.float32)
        g[:4] = 2.0 if n >= 4 else 0.0
        if n < 4:
            g[n - 1] = 4.0
        return w, g, m, v, 2.0
    g = f32(rng, n) * np.float32(4.0)
    norm = tk.grad_norm(g, GSCALE)
    if kind == 'inf':
        g[n // 2] = np.inf
    return w, g, m, v, {'below': 2.0 * norm, 'above': norm / 3.0, 'inf': 1.0}[kind]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ['below', 'equal', 'above', 'inf'])
def test_norm_scale_and_update(ops, internal, n, kind):
    w, g, m, v, c = update_case(n, kind)
    c = float(np.float32(c))
    ref = tk.clip_decay_adam(w, g, m, v, GSCALE, STEP, c=c, decay=DECAY)

    def run():
        bufs = [guarded(a) for a in (w, g, m, v)]
        wbuf, work = guarded(np.zeros(internal.work_floats, np.float32))
        internal.clip_scale(ptr(bufs[1][1]), n, GSCALE, c, ptr(work), stream())
        internal.clip_decay_adam(*[ptr(b[1]) for b in bufs], n, GSCALE, 5.0, 0.9, 0.999, 1e-8, STEP, ptr(work), DECAY, stream())
        torch.cuda.synchronize()
        assert all(guard_ok(b[0]) for b in bufs) and guard_ok(wbuf)
        return [b[1] for b in bufs] + [work[:2].clone()]
    got = run()
    scale, norm = (float(x) for x in got[4].cpu().numpy())
    if kind == 'inf':
        assert norm == np.inf and scale == 1.0 and all(bool(torch.isfinite(t).all().item()) for t in got[:4])
    else:
        assert abs(norm - ref[4]) < BOUND * ref[4], (norm, ref[4])
    if kind == 'equal':
        assert (norm, scale) == (2.0, 1.0)                                        # GC1: the scale applies above c only
    elif kind == 'below':
        assert scale == 1.0
    elif kind == 'above':
        assert abs(scale - ref[5]) < BOUND * ref[5] and scale < 0.5
    figures = dict(w=err(got[0], ref[0]), g=err(got[1], ref[1]), m=err(got[2], ref[2]), v=err(got[3], ref[3]))
    print('update n = %d, %s: norm %.9g (fp64 %.9g), scale %.9g, %s' % (n, kind, norm, ref[4], scale, figures))
    assert figures['w'] < 1e-6 and figures['g'] < 1.5e-5 and figures['m'] < 5e-5 and figures['v'] < 5e-5, figures
    again = run()
    for a, b in zip(got, again):                                                  # GC3: a fixed order
        assert torch.equal(a, b)


@pytest.mark.parametrize("n", [3, 4097])
def test_update_without_a_scale_and_without_the_knobs(ops, internal, n):
    w, g, m, v, _ = update_case(n, 'below')
    bufs = [guarded(a)[1] for a in (w, g, m, v)]
    internal.clip_decay_adam(*[ptr(b) for b in bufs], n, GSCALE, 5.0, 0.9, 0.999, 1e-8, STEP, None, DECAY, stream())   # decay alone
    ref = tk.clip_decay_adam(w, g, m, v, GSCALE, STEP, decay=DECAY)
    assert err(bufs[0], ref[0]) < 1e-6 and err(bufs[1], ref[1]) < 1e-6 and err(bufs[2], ref[2]) < 5e-5 and err(bufs[3], ref[3]) < 5e-5
    plain_ref = tk.clip_decay_adam(w, g, m, v, GSCALE, STEP)
    assert err(bufs[0], plain_ref[0]) > 1e-5                                      # ... and the decay is there
    # a scale of 1 and no decay: vd_clamp_adam's bits
    a = [guarded(x)[1] for x in (w, g, m, v)]
    b = [guarded(x)[1] for x in (w, g, m, v)]
    internal.clip_decay_adam(*[ptr(t) for t in a], n, GSCALE, 5.0, 0.9, 0.999, 1e-8, STEP, None, 0.0, stream())
    ops.clamp_adam(b[0], b[1], b[2], b[3], STEP, gscale=GSCALE)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
