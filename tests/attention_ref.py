"""numpy fp64 restatements of the operators of csrc/attention.hip, and the comparison routine of tests/test_attention_ops_gpu.py.

Everything here is plain numpy in float64 on the values the device is given (fp32 inputs are cast, never re-rounded).  The backwards are
written out by hand, as the kernels are; tests/test_attention_ref_cpu.py holds each of them to torch.autograd in float64 on the same
forward, so a GPU test that disagrees with this module points at the kernel.

Image attention (encoders/mn-att-ques-im-hist.lua:68-104), for N = B * R question rounds over B images of S2 regions:
    img_tr[(n, s), :] = dropout1(pre[(n // R, s), :])                          gather by n // R, mask1 * scale
    iqc[(n, s), :]    = dropout2(tanh(img_tr[(n, s), :] Wc^T + bc + qc[n, :]))  mask2 * scale
    p[n, :]           = softmax_s(iqc[(n, s), :] . wa + ba)
    u1[n, :]          = u0[n, :] + sum_s p[n, s] img_tr[(n, s), :]
"""
import numpy as np

F64 = np.float64


def _f64(a):
    return None if a is None else np.asarray(a, F64)


# ------------------------------------------------------------------------------------------------------------------ image attention
def img_gather_drop(pre, mask1, B, R, S2, scale):
    """[N*S2 x H]: row (n, s) is row (n // R, s) of pre [B*S2 x H], times mask1 * scale where a mask is given"""
    n = np.arange(B * R)
    rows = ((n // R)[:, None] * S2 + np.arange(S2)[None, :]).reshape(-1)
    x = _f64(pre)[rows]
    if mask1 is not None:
        x = x * _f64(mask1) * scale
    return x


def img_forward(pre, mask1, mask2, Wc, bc, qc, wa, ba, u0, B, R, S2, scale):
    """-> dict(img_tr [N*S2 x H], t = the tanh before dropout 2 [N*S2 x Kc], iqc [N*S2 x Kc], p [N x S2], u1 [N x H])"""
    N = B * R
    img_tr = img_gather_drop(pre, mask1, B, R, S2, scale)
    t = np.tanh(img_tr @ _f64(Wc).T + _f64(bc) + np.repeat(_f64(qc), S2, 0))
    iqc = t * _f64(mask2) * scale if mask2 is not None else t
    score = (iqc @ _f64(wa) + _f64(ba)[0]).reshape(N, S2)
    e = np.exp(score - score.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)
    H = img_tr.shape[1]
    u1 = np.einsum('ns,nsh->nh', p, img_tr.reshape(N, S2, H)) + _f64(u0)
    return dict(img_tr=img_tr, t=t, iqc=iqc, p=p, u1=u1)


def img_backward(fwd, datt, mask1, mask2, Wc, wa, B, R, S2, scale):
    """from datt = dLoss / du1 [N x H] -> dict(dscore [N x S2], dwa [Kc], dba (scalar), dz [N*S2 x Kc] (what the device writes over
    iqc: the gradient before the tanh), dqc [N x Kc], dpre [B*S2 x H] (summed over the R rounds of an image), dWc [Kc x H])"""
    N = B * R
    img_tr, t, iqc, p = fwd['img_tr'], fwd['t'], fwd['iqc'], fwd['p']
    H, Kc = img_tr.shape[1], iqc.shape[1]
    datt, wa, Wc = _f64(datt), _f64(wa), _f64(Wc)
    dp = np.einsum('nh,nsh->ns', datt, img_tr.reshape(N, S2, H))
    dscore = p * (dp - (p * dp).sum(1, keepdims=True))
    dwa = np.einsum('ns,nsk->k', dscore, iqc.reshape(N, S2, Kc))
    diqc = dscore[:, :, None] * wa[None, None, :]
    dz = (diqc * (_f64(mask2).reshape(N, S2, Kc) * scale if mask2 is not None else 1.0)) * (1 - t.reshape(N, S2, Kc) ** 2)
    dqc = dz.sum(1)
    dz = dz.reshape(N * S2, Kc)
    dimg = p[:, :, None] * datt[:, None, :] + (dz @ Wc).reshape(N, S2, H)
    if mask1 is not None:
        dimg = dimg * _f64(mask1).reshape(N, S2, H) * scale
    dpre = dimg.reshape(B, R, S2, H).sum(1).reshape(B * S2, H)
    return dict(dscore=dscore, dwa=dwa, dba=dscore.sum(), dz=dz, dqc=dqc, dpre=dpre, dWc=dz.T @ img_tr)


# ------------------------------------------------------------------------------------------------------------------ hrea attention
def hrea_forward(sq, sh, h):
    """encoders/hrea-ques-im-hist.lua:83-131.  sq, sh [B x R], h [B x R x H]: A[i, j] = sq[i] + sh[j]; MaskFuture (j > i -> 0);
    ReplaceZero (every exact 0 -> -inf); softmax over j; att[i] = sum_j P[i, j] h[j].  -> P [B x R x R], att [B x R x H]"""
    sq, sh, h = _f64(sq), _f64(sh), _f64(h)
    R = sq.shape[1]
    A = sq[:, :, None] + sh[:, None, :]
    A = np.where(np.triu(np.ones((R, R), bool), 1)[None], 0.0, A)
    A = np.where(A == 0, -np.inf, A)
    A = A - A.max(-1, keepdims=True)
    e = np.exp(A)
    P = e / e.sum(-1, keepdims=True)
    return P, np.einsum('bij,bjk->bik', P, h)


def hrea_backward(P, h, datt):
    """-> dsq [B x R], dsh [B x R], dh [B x R x H] (through the weighted sum alone: sh's own Linear is the caller's) and dA [B x R x R],
    the gradient of the scores.  A replaced score has P = 0 exactly, so nothing flows through it.  dsq is a row sum of dA, which cancels
    to zero in exact arithmetic (sq[i] shifts a whole softmax row): hold it to the sum of |dA| over the row, not to its own size."""
    P, h, datt = _f64(P), _f64(h), _f64(datt)
    dP = np.einsum('bik,bjk->bij', datt, h)
    dA = P * (dP - (P * dP).sum(-1, keepdims=True))
    return dA.sum(2), dA.sum(1), np.einsum('bij,bik->bjk', P, datt), dA


# ------------------------------------------------------------------------------------------------------------------ nn.Linear(H, 1)
def rowdot_forward(x, w, b):
    return _f64(x) @ _f64(w) + _f64(b)[0]


def rowdot_backward(x, w, dout):
    """-> dw [H], db (scalar), dx [N x H]"""
    x, w, dout = _f64(x), _f64(w), _f64(dout)
    return x.T @ dout, dout.sum(), dout[:, None] * w[None, :]


# ------------------------------------------------------------------------------------------------------------------ comparison
SENTINEL = 123456.0
GUARD_ROWS = 128
TILE = 128


def to_np(a):
    if hasattr(a, 'detach'):
        a = a.detach().cpu().numpy()
    return np.asarray(a, F64)


def rel_l2(got, ref):
    got, ref = to_np(got), to_np(ref)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30))


def tile_slices(rows, cols=None):
    """the rows of the last (ragged) 128-row tile and the columns of the last (ragged) 128-column tile of a [rows x cols] tensor"""
    out = [('last row tile', (slice((rows - 1) // TILE * TILE, rows),))]
    if cols is not None:
        out.append(('last column tile', (slice(None), slice((cols - 1) // TILE * TILE, cols))))
    return out


def row_block(label, i, n):
    """rows [i * n, (i + 1) * n): the S2 rows of a round, or of an image"""
    return (label, (slice(i * n, (i + 1) * n),))


class Guarded:
    """An output of `shape` with GUARD_ROWS rows of SENTINEL behind it (a 1-D tensor counts as one row).  The output itself starts as
    SENTINEL (a written output) or as `init` (an accumulated one).  `.t` is the contiguous view the kernel is given."""

    def __init__(self, shape, device='cuda', init=None):
        import torch
        shape = tuple(int(s) for s in shape)
        n = int(np.prod(shape))
        rowlen = int(np.prod(shape[1:])) if len(shape) > 1 else n
        self.buf = torch.full((n + GUARD_ROWS * rowlen,), SENTINEL, dtype=torch.float32, device=device)
        self.t = self.buf[:n].view(shape)
        self.guard = self.buf[n:].view(GUARD_ROWS, rowlen)
        if init is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(init, dtype=np.float32)).to(device))

    def written_guard_rows(self):
        bad = (self.guard != SENTINEL).any(1).nonzero().reshape(-1)
        return [int(i) for i in bad.cpu()]


class Report:
    """Collects what misses its bound.  `close` holds got to ref in rel-L2 over the whole tensor and over every named slice, with ONE
    bound; `guard` requires the guard rows of a Guarded output unchanged.  Every figure is printed; `ok()` raises with all failures."""

    def __init__(self, what='', log=print):
        self.what, self.log, self.failures, self.errors = what, log, [], {}

    def close(self, name, got, ref, bound=1e-5, slices=()):
        got = got.t if isinstance(got, Guarded) else got
        g, r = to_np(got), to_np(ref)
        assert g.shape == r.shape, (name, g.shape, r.shape)
        for label, idx in [('whole', (slice(None),))] + list(slices):
            e = rel_l2(g[idx], r[idx])
            self.errors[(name, label)] = e
            self.log('%s %-6s %-18s rel-L2 %.3e' % (self.what, name, label, e))
            if not e < bound:                                   # (a NaN misses the bound too)
                self.failures.append('%s %s [%s]: rel-L2 %.3e >= %.1e' % (self.what, name, label, e, bound))
        return self.errors[(name, 'whole')]

    def within(self, name, got, ref, bound):
        """|got - ref| <= bound, element by element (bound: a number or an array): for a sum that cancels in exact arithmetic, whose error
        scales with the magnitudes summed, not with the result"""
        e = np.abs(to_np(got).reshape(-1) - to_np(ref).reshape(-1))
        b = np.broadcast_to(np.asarray(bound, F64).reshape(-1), e.shape)
        worst = int(np.argmax(e - b))
        self.errors[(name, 'abs')] = float(e.max())
        self.log('%s %-6s max |got - ref| %.3e (bound there %.3e)' % (self.what, name, e[worst], b[worst]))
        if not np.all(e <= b):
            self.failures.append('%s %s: |got - ref| %.3e > %.3e at element %d' % (self.what, name, e[worst], b[worst], worst))

    def scalar(self, name, got, ref, bound):
        self.within(name, np.asarray([float(got)]), np.asarray([float(ref)]), bound)

    def exact(self, name, got, ref):
        g, r = to_np(got), to_np(ref)
        assert g.shape == r.shape, (name, g.shape, r.shape)
        n = int((g != r).sum())
        if n:
            self.failures.append('%s %s: %d elements differ (bit-for-bit expected)' % (self.what, name, n))

    def guard(self, name, out):
        rows = out.written_guard_rows()
        if rows:
            self.failures.append('%s %s: guard rows written (first: row %d behind the output, %d rows)' % (self.what, name, rows[0], len(rows)))

    def ok(self):
        assert not self.failures, '\n'.join(self.failures)
