"""fp64 numpy restatement of the training knobs of the model-level runtime: label smoothing (csrc/loss.hip LS1-LS2), the global-norm clip
and decoupled weight decay (csrc/elementwise.hip GC1-GC2, WD1).  Written from the rules, not from the kernels: the targets are formed as
(1 - eps) onehot + eps / K and contracted directly.  tests/test_train_knobs_cpu.py pins it against torch on the CPU; the GPU tests compare
the kernels with it."""
import numpy as np

D = np.float64


def smooth_targets(idx, K, eps):
    """t [n x K] = (1 - eps) onehot(idx) + eps / K   (LS1 / LS2; idx 0-based)"""
    idx = np.asarray(idx).reshape(-1)
    t = np.full((idx.size, K), eps / K, D)
    t[np.arange(idx.size), idx] += 1.0 - eps
    return t


def lse(x):
    x = np.asarray(x, D)
    mx = x.max(-1, keepdims=True)
    return (mx + np.log(np.exp(x - mx).sum(-1, keepdims=True)))[..., 0]


def smoothed_ce(scores, idx, eps):
    """rows of scores [n x K], class idx [n] (0-based) -> loss rows [n] = lse - sum_k t_k s_k and d loss / d scores = softmax - t"""
    s = np.asarray(scores, D)
    t = smooth_targets(idx, s.shape[1], eps)
    l = lse(s)
    return l - (t * s).sum(1), np.exp(s - l[:, None]) - t


def score_ce(optH, enc, gt, eps, gscale):
    """LS1 around the disc head: optH [N x O x H], enc [N x H], gt [N] 0-based -> scores, loss rows, dOptH, dEnc (ds = (softmax - t) gscale)"""
    optH, enc = np.asarray(optH, D), np.asarray(enc, D)
    scores = np.einsum('noh,nh->no', optH, enc)
    loss, ds = smoothed_ce(scores, gt, eps)
    ds = ds * gscale
    return dict(scores=scores, loss_rows=loss, dOptH=ds[:, :, None] * enc[:, None, :], dEnc=np.einsum('no,noh->nh', ds, optH))


def logsoftmax_nll(logits, V, tok_in, target, eps):
    """LS2: logits [rows x ld] with V valid columns, decoder input tok_in [rows], 1-based target [rows] -> loss rows and the matrix the
    kernel leaves in place of the logits: softmax - t on the rows that contribute, zeros on masked rows and on the pad columns"""
    x = np.asarray(logits, D)
    tok_in, target = np.asarray(tok_in).reshape(-1), np.asarray(target).reshape(-1)
    loss, grad = np.zeros(x.shape[0], D), np.zeros_like(x)
    live = (tok_in != 0) & (target > 0)
    if live.any():
        loss[live], grad[live, :V] = smoothed_ce(x[live, :V], target[live] - 1, eps)
    return loss, grad


def grad_norm(g, gscale):
    """GC1: || gscale g ||_2 over the whole flat gradient"""
    with np.errstate(over='ignore', invalid='ignore'):
        return float(np.sqrt(((np.asarray(g, D) * gscale) ** 2).sum()))


def clip_scale(norm, c):
    """GC1: c / norm if c > 0 and the norm is finite and > c, otherwise 1"""
    return c / norm if c > 0 and np.isfinite(norm) and norm > c else 1.0


def clip_decay_adam(w, g, m, v, gscale, step, c=0.0, decay=0.0, clip=5.0, b1=0.9, b2=0.999, eps=1e-8):
    """GC2 + WD1: g <- clamp(gscale scale g, +-clip); Adam's moments; w <- w - step m / (sqrt(v) + eps) - decay w_old (decay = lr lambda).
    Returns w, g, m, v, the norm and the scale."""
    w, g, m, v = (np.asarray(a, D) for a in (w, g, m, v))
    norm = grad_norm(g, gscale)
    scale = clip_scale(norm, c)
    with np.errstate(over='ignore', invalid='ignore'):
        gg = np.clip(g * (gscale * scale), -clip, clip)
        m2 = b1 * m + (1 - b1) * gg
        v2 = b2 * v + (1 - b2) * gg * gg
        w2 = w - step * m2 / (np.sqrt(v2) + eps) - decay * w
    return w2, gg, m2, v2, norm, scale
