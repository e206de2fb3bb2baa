"""numpy fp64 restatement of the image attention over a region count per image: rules IR1 - IR6 at the top of csrc/attention.hip.

Same tensors and names as tests/attention_ref.py (img_forward / img_backward), plus cnt [B]: the number of live regions of every image.
    IR1  region s of image b is live iff s < cnt[b], 1 <= cnt[b] <= S2; round n reads cnt[n // R]
    IR2  max, sum and softmax of the scores run over the live regions only; p[n, s] = +0.0 exactly for s >= cnt; a hidden row of iqc
         is never read (so it may hold anything, NaN included)
    IR3  the weighted sum and dp run over s < cnt: hidden rows of pre / mask1 are never read by them
    IR4  dscore and dz are exact zeros for every hidden region; dqc, dwa, dba add live regions only; the dense products (dz Wc, dz^T img_tr),
         the bias column sum and the projection's backward are unchanged: a hidden row contributes 0 * finite
    IR5  so the hidden rows of the features must be finite where a dense product reads them
    IR6  with cnt = S2 everywhere this is attention_ref.img_forward / img_backward
tests/test_region_ref_cpu.py holds every function here to torch.autograd in float64 on a softmax over masked_fill(-inf)."""
import numpy as np

from attention_ref import F64, _f64, img_gather_drop


def live_mask(cnt, B, R, S2):
    """[N x S2] bool: region s of round n is live (IR1)"""
    cnt = np.asarray(cnt).astype(np.int64).reshape(-1)
    assert cnt.shape == (B,) and cnt.min() >= 1 and cnt.max() <= S2, (cnt, B, S2)
    return np.arange(S2)[None, :] < np.repeat(cnt, R)[:, None]


def region_attend(iqc, img_tr, wa, ba, u0, live):
    """the attention head alone, from a given iqc [N*S2 x Kc] and img_tr [N*S2 x H] whose hidden rows are never read (IR2, IR3):
    -> p [N x S2], u1 [N x H]"""
    N, S2 = live.shape
    iqc, img_tr = _f64(iqc), _f64(img_tr)
    Kc, H = iqc.shape[1], img_tr.shape[1]
    iq = np.where(live[:, :, None], iqc.reshape(N, S2, Kc), 0.0)
    x = np.where(live[:, :, None], img_tr.reshape(N, S2, H), 0.0)
    score = np.where(live, iq @ _f64(wa) + _f64(ba)[0], -np.inf)
    e = np.where(live, np.exp(score - score.max(1, keepdims=True)), 0.0)
    p = e / e.sum(1, keepdims=True)
    return p, np.einsum('ns,nsh->nh', p, x) + _f64(u0)


def region_forward(pre, mask1, mask2, Wc, bc, qc, wa, ba, u0, cnt, B, R, S2, scale):
    """-> dict(img_tr, t, iqc, p, u1, live): attention_ref.img_forward with the softmax and the weighted sum over the live regions.  The dense
    product runs over every row (IR5): t / iqc of a hidden row are whatever the features there give."""
    live = live_mask(cnt, B, R, S2)
    img_tr = img_gather_drop(pre, mask1, B, R, S2, scale)
    t = np.tanh(img_tr @ _f64(Wc).T + _f64(bc) + np.repeat(_f64(qc), S2, 0))
    iqc = t * _f64(mask2) * scale if mask2 is not None else t
    p, u1 = region_attend(iqc, img_tr, wa, ba, u0, live)
    return dict(img_tr=img_tr, t=t, iqc=iqc, p=p, u1=u1, live=live)


def region_head_backward(iqc, img_tr, p, datt, mask2, wa, live, scale):
    """the backward of the head alone (the two masked kernels), hidden rows of iqc / img_tr never read:
    -> dict(dscore [N x S2], dwa [Kc], dba, dz [N*S2 x Kc], dqc [N x Kc]).  dz = dscore * wa * mask2 * scale * (1 - t^2) with
    t = iqc / scale where dropout 2 kept the element (a dropped element has dz = 0 whatever t was)."""
    N, S2 = live.shape
    iqc, img_tr, datt, wa = _f64(iqc), _f64(img_tr), _f64(datt), _f64(wa)
    Kc, H = iqc.shape[1], img_tr.shape[1]
    iq = np.where(live[:, :, None], iqc.reshape(N, S2, Kc), 0.0)
    x = np.where(live[:, :, None], img_tr.reshape(N, S2, H), 0.0)
    dp = np.einsum('nh,nsh->ns', datt, x)
    dscore = np.where(live, p * (dp - (p * dp).sum(1, keepdims=True)), 0.0)
    dwa = np.einsum('ns,nsk->k', dscore, iq)
    if mask2 is not None:
        m2 = _f64(mask2).reshape(N, S2, Kc)
        t = iq / scale
        dz = dscore[:, :, None] * wa[None, None, :] * m2 * scale * (1 - t ** 2)
    else:
        dz = dscore[:, :, None] * wa[None, None, :] * (1 - iq ** 2)
    dz = np.where(live[:, :, None], dz, 0.0)
    return dict(dscore=dscore, dwa=dwa, dba=dscore.sum(), dz=dz.reshape(N * S2, Kc), dqc=dz.sum(1))


def region_backward(fwd, datt, mask1, mask2, Wc, wa, B, R, S2, scale):
    """from datt = dLoss / du1 [N x H] -> dict(dscore, dwa, dba, dz, dqc, dpre [B*S2 x H], dWc [Kc x H]) as attention_ref.img_backward.
    The two dense products and the epilogue of dpre are the unmasked ones (IR4): hidden rows of dz and p are zero, the features finite."""
    N = B * R
    live, img_tr, p = fwd['live'], fwd['img_tr'], fwd['p']
    H = img_tr.shape[1]
    out = region_head_backward(fwd['iqc'], img_tr, p, datt, mask2, wa, live, scale)
    dimg = p[:, :, None] * _f64(datt)[:, None, :] + (out['dz'] @ _f64(Wc)).reshape(N, S2, H)
    if mask1 is not None:
        dimg = dimg * _f64(mask1).reshape(N, S2, H) * scale
    out['dpre'] = dimg.reshape(B, R, S2, H).sum(1).reshape(B * S2, H)
    out['dWc'] = out['dz'].T @ img_tr
    return out
