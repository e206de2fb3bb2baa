"""tests/region_ref.py (IR1 - IR6 of csrc/attention.hip in fp64) against torch.autograd in float64: the autograd model is a softmax over
masked_fill(-inf), forward and every gradient; with full counts region_ref is attention_ref.img_forward / img_backward."""
import numpy as np
import pytest
import torch

import attention_ref as ar
import region_ref as rr

CASES = [  # B, R, S2, H, Kc, counts, dropout masks
    (3, 1, 5, 4, 4, (1, 3, 5), False),
    (3, 1, 5, 4, 4, (1, 3, 5), True),
    (4, 2, 9, 8, 12, (1, 4, 9, 2), True),
    (2, 3, 16, 12, 8, (16, 7), False),
]


def make(B, R, S2, H, Kc, drop, seed=0):
    rng = np.random.RandomState(seed)
    N = B * R
    d = dict(pre=rng.randn(B * S2, H), Wc=rng.randn(Kc, H) * 0.3, bc=rng.randn(Kc) * 0.1, qc=rng.randn(N, Kc) * 0.5, wa=rng.randn(Kc),
             ba=rng.randn(1), u0=rng.randn(N, H), datt=rng.randn(N, H))
    d['mask1'] = (rng.rand(N * S2, H) < 0.5).astype(np.float64) if drop else None
    d['mask2'] = (rng.rand(N * S2, Kc) < 0.5).astype(np.float64) if drop else None
    d['scale'] = 2.0 if drop else 1.0
    return d


def autograd(d, cnt, B, R, S2):
    """the same forward in torch float64, the mask as masked_fill(-inf) on the scores -> (p, u1, grads of sum(u1 * datt))"""
    T = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)
    pre, Wc, bc, qc, wa, ba, u0 = (T(d[k]) for k in ('pre', 'Wc', 'bc', 'qc', 'wa', 'ba', 'u0'))
    N, H = B * R, pre.shape[1]
    rows = torch.tensor(((np.arange(N) // R)[:, None] * S2 + np.arange(S2)[None, :]).reshape(-1))
    x = pre[rows]
    if d['mask1'] is not None:
        x = x * torch.tensor(d['mask1']) * d['scale']
    z = x @ Wc.T + bc + qc.repeat_interleave(S2, 0)
    z.retain_grad()
    iqc = torch.tanh(z)
    if d['mask2'] is not None:
        iqc = iqc * torch.tensor(d['mask2']) * d['scale']
    score = (iqc @ wa + ba[0]).reshape(N, S2)
    score.retain_grad()
    hidden = torch.tensor(~rr.live_mask(cnt, B, R, S2))
    p = torch.softmax(score.masked_fill(hidden, float('-inf')), 1)
    u1 = u0 + torch.einsum('ns,nsh->nh', p, x.reshape(N, S2, H))
    (u1 * torch.tensor(d['datt'])).sum().backward()
    g = dict(dscore=score.grad, dz=z.grad, dqc=qc.grad, dwa=wa.grad, dba=ba.grad[0], dpre=pre.grad, dWc=Wc.grad)
    return p.detach().numpy(), u1.detach().numpy(), {k: v.detach().numpy() for k, v in g.items()}


@pytest.mark.parametrize('B,R,S2,H,Kc,cnt,drop', CASES)
def test_region_ref_equals_autograd_over_masked_fill(B, R, S2, H, Kc, cnt, drop):
    d = make(B, R, S2, H, Kc, drop)
    fwd = rr.region_forward(d['pre'], d['mask1'], d['mask2'], d['Wc'], d['bc'], d['qc'], d['wa'], d['ba'], d['u0'], cnt, B, R, S2, d['scale'])
    bwd = rr.region_backward(fwd, d['datt'], d['mask1'], d['mask2'], d['Wc'], d['wa'], B, R, S2, d['scale'])
    p, u1, g = autograd(d, cnt, B, R, S2)
    np.testing.assert_allclose(fwd['p'], p, rtol=0, atol=1e-14)
    np.testing.assert_allclose(fwd['u1'], u1, rtol=1e-13, atol=1e-13)
    for k, v in g.items():
        np.testing.assert_allclose(np.asarray(bwd[k]).reshape(np.shape(v)), v, rtol=1e-11, atol=1e-12, err_msg=k)
    # IR2 / IR4: exact zeros on every hidden region, in the reference and in autograd alike
    hid = ~fwd['live']
    assert hid.any() and (fwd['p'][hid] == 0).all() and not np.signbit(fwd['p'][hid]).any() and (p[hid] == 0).all()
    assert (bwd['dscore'][hid] == 0).all() and (bwd['dz'].reshape(B * R, S2, Kc)[hid] == 0).all()
    assert (g['dscore'][hid] == 0).all() and (g['dz'].reshape(B * R, S2, Kc)[hid] == 0).all()
    np.testing.assert_allclose(fwd['p'].sum(1), 1.0, rtol=0, atol=1e-14)


@pytest.mark.parametrize('B,R,S2,H,Kc,cnt,drop', CASES)
def test_hidden_rows_are_never_read_by_the_head(B, R, S2, H, Kc, cnt, drop):
    """IR2 / IR3: NaN in the hidden rows of iqc and of the image tensor changes nothing and comes back nowhere"""
    d = make(B, R, S2, H, Kc, drop, seed=1)
    fwd = rr.region_forward(d['pre'], d['mask1'], d['mask2'], d['Wc'], d['bc'], d['qc'], d['wa'], d['ba'], d['u0'], cnt, B, R, S2, d['scale'])
    live = fwd['live']
    want = rr.region_head_backward(fwd['iqc'], fwd['img_tr'], fwd['p'], d['datt'], d['mask2'], d['wa'], live, d['scale'])
    iqc, x = fwd['iqc'].copy(), fwd['img_tr'].copy()
    iqc[~live.reshape(-1)] = np.nan
    x[~live.reshape(-1)] = np.nan
    p, u1 = rr.region_attend(iqc, x, d['wa'], d['ba'], d['u0'], live)
    got = rr.region_head_backward(iqc, x, p, d['datt'], d['mask2'], d['wa'], live, d['scale'])
    assert (p == fwd['p']).all() and (u1 == fwd['u1']).all()
    for k in want:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k


@pytest.mark.parametrize('drop', [False, True])
def test_full_counts_are_the_unmasked_reference(drop):
    """IR6"""
    B, R, S2, H, Kc = 3, 2, 9, 8, 12
    d = make(B, R, S2, H, Kc, drop, seed=2)
    cnt = np.full(B, S2)
    a = ar.img_forward(d['pre'], d['mask1'], d['mask2'], d['Wc'], d['bc'], d['qc'], d['wa'], d['ba'], d['u0'], B, R, S2, d['scale'])
    f = rr.region_forward(d['pre'], d['mask1'], d['mask2'], d['Wc'], d['bc'], d['qc'], d['wa'], d['ba'], d['u0'], cnt, B, R, S2, d['scale'])
    for k in ('img_tr', 't', 'iqc', 'p', 'u1'):
        np.testing.assert_allclose(f[k], a[k], rtol=1e-14, atol=1e-15, err_msg=k)
    ab = ar.img_backward(a, d['datt'], d['mask1'], d['mask2'], d['Wc'], d['wa'], B, R, S2, d['scale'])
    fb = rr.region_backward(f, d['datt'], d['mask1'], d['mask2'], d['Wc'], d['wa'], B, R, S2, d['scale'])
    for k in ab:
        np.testing.assert_allclose(fb[k], ab[k], rtol=1e-12, atol=1e-13, err_msg=k)


def test_counts_outside_one_to_s2_are_refused():
    for bad in ((0, 2), (3, 10), (2,)):
        with pytest.raises(AssertionError):
            rr.live_mask(bad, 2, 1, 9)
