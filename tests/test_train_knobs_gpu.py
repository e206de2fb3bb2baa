"""The training knobs through the model-level runtime (NativeModel; lf-ques-im-hist, dropout 0, a tiny synthetic configuration).  The
unchanged path is the reference:

  * linearity: cross-entropy is linear in its target, so the smoothed gradient of every tensor -- and the loss -- is
    (1 - eps) G(y) + (eps / K) sum_k G(all targets = k), the G's taken from 1 + K plain steps on the same batch (K = O for disc with
    answer_ind replaced, K = V for gen with answer_out replaced at its non-pad positions); rel-L2 1e-4 per tensor, the project's
    cross-host parity bound.  A library that ignores the variable fails it;
  * clip: dW, m and v after `update` are those of a plain model updated with gscale c / norm, the norm taken on the host in fp64 from the
    read-back gradient (m and v, not only w: Adam's first step is scale-invariant in w);
  * decay: w is the plain update's w minus lr lambda w_old;
  * only_forward = 1, retrieval scores and ranks are bit-identical with eps on and off; with every knob off `update` gives vd_clamp_adam's
    bits; three trainIterations with every knob on run and the loss is finite."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import grad_mismatches, small_params
from test_model_gpu import rel
from visdial_amd.dataloader import SyntheticDataloader
from visdial_amd.opts import derive

pytestmark = pytest.mark.gpu

EPS = 0.2


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def tiny(decoder, **kw):
    return derive(small_params(encoder='lf-ques-im-hist', decoder=decoder, dropout=0.0, vocabSize=23, numOptions=5, imgNorm=1, **kw))


def native(p, weights=None):
    from visdial_amd.native import NativeModel
    m = NativeModel(p, init_seed=5)
    if weights is not None:
        m.set_parameters_dict(weights)
    return m


def step(model, batch):
    """(loss, gradient dict) of one forwardBackward"""
    loss = model.forwardBackward(batch)
    return loss, {k: v.astype(np.float64) for k, v in model.get_gradients_dict().items()}


@pytest.mark.parametrize("decoder", ['disc', 'gen'])
def test_smoothed_gradient_is_the_linear_combination_of_plain_ones(gpu, decoder):
    p = tiny(decoder)
    batch = SyntheticDataloader(p, seed=11).getTrainBatch(p)
    plain = native(p)
    W = plain.get_parameters_dict()
    loss_y, g_y = step(plain, batch)
    if decoder == 'disc':
        K = p['numOptions']
        swapped = [dict(batch, answer_ind=np.full_like(batch['answer_ind'], k + 1)) for k in range(K)]
    else:
        K = p['vocabSize']
        swapped = [dict(batch, answer_out=np.where(batch['answer_out'] > 0, k + 1, 0).astype(batch['answer_out'].dtype)) for k in range(K)]
    loss_u, g_u = 0.0, {k: np.zeros_like(v) for k, v in g_y.items()}
    for b in swapped:
        l, g = step(plain, b)
        loss_u += l / K
        for k in g:
            g_u[k] += g[k] / K
    plain.close()
    smooth = native(dict(p, labelSmoothing=EPS), W)
    loss_s, g_s = step(smooth, batch)
    smooth.close()
    want = {k: (1 - EPS) * g_y[k] + EPS * g_u[k] for k in g_y}
    want_loss = (1 - EPS) * loss_y + EPS * loss_u
    print('%s: loss %.7f, combination %.7f, plain %.7f' % (decoder, loss_s, want_loss, loss_y))
    assert abs(loss_s - want_loss) < 1e-4 * abs(want_loss)
    bad = grad_mismatches(g_s, want)
    assert not bad, bad
    assert grad_mismatches(g_s, g_y), "the smoothed gradient is the plain one"


def moments(model):
    return {which: model._get(i) for i, which in enumerate(('w', 'dW', 'm', 'v'))}


def flat_norm(g):
    return float(np.sqrt(sum((v.astype(np.float64) ** 2).sum() for v in g.values())))


def updated(p, W, batch, gscale=1.0):
    """W, dW, m, v after one forwardBackward + update of a fresh model on weights W"""
    model = native(p, W)
    model.forwardBackward(batch)
    model.update(gscale=gscale)
    out = moments(model)
    model.close()
    return out


def same_update(got, want, names):
    for k in names:
        figures = {which: rel(got[which][k], want[which][k]) for which in ('w', 'dW', 'm', 'v')}
        assert figures['w'] < 1e-6 and figures['dW'] < 1.5e-5 and figures['m'] < 5e-5 and figures['v'] < 5e-5, (k, figures)


@pytest.mark.parametrize("decoder", ['disc', 'gen'])
def test_clip_is_a_plain_update_with_a_smaller_gscale(gpu, decoder):
    p = tiny(decoder)
    batch = SyntheticDataloader(p, seed=12).getTrainBatch(p)
    plain = native(p)
    W = plain.get_parameters_dict()
    plain.forwardBackward(batch)
    norm = flat_norm(plain.get_gradients_dict())                                  # gscale = 1
    plain.close()
    c = norm / 3
    want = updated(p, W, batch, gscale=c / norm)
    same_update(updated(dict(p, gradClipNorm=c), W, batch), want, W)
    unclipped = updated(p, W, batch)
    same_update(updated(dict(p, gradClipNorm=2 * norm), W, batch), unclipped, W)  # a norm below c: the plain update
    assert any(rel(unclipped['m'][k], want['m'][k]) > 0.5 for k in W)             # ... which is another one


def test_decay_takes_lr_lambda_w_off_the_plain_update(gpu):
    p = tiny('disc')
    lam = 5.0
    batch = SyntheticDataloader(p, seed=13).getTrainBatch(p)
    plain = native(p)
    W = plain.get_parameters_dict()
    plain.forwardBackward(batch)
    plain.update()
    want = moments(plain)
    plain.close()
    decayed = native(dict(p, weightDecay=lam), W)
    decayed.forwardBackward(batch)
    decayed.update()
    got = moments(decayed)
    lr_after = decayed.optims['learningRate']
    decayed.close()
    assert lr_after == pytest.approx(p['learningRate'] * p['lrDecayRate'], rel=1e-6)          # (the params are fp32 in vd_model_params)
    for k in W:
        w_old = W[k].astype(np.float64)
        if k == 'embed':
            w_old[0] = 0.0                                                        # the pad row is zeroed in front of every step
        assert rel(got['w'][k], want['w'][k].astype(np.float64) - p['learningRate'] * lam * w_old) < 1e-6, k
        if np.abs(w_old).max() > 0:                                               # lr before the step's decay, on every tensor
            assert rel(got['w'][k], want['w'][k]) > 1e-3, k
        for which in ('dW', 'm', 'v'):
            assert rel(got[which][k], want[which][k]) < 5e-5 or np.abs(got[which][k] - want[which][k]).max() < 1e-7, (k, which)


@pytest.mark.parametrize("decoder", ['disc', 'gen'])
def test_forward_only_and_retrieval_do_not_see_the_smoothing(gpu, decoder):
    p = tiny(decoder)
    dl = SyntheticDataloader(p, seed=14, num_threads=4)
    train = dl.getTrainBatch(p)
    val, _ = dl.getTestBatch(1, p, 'val')
    plain = native(p)
    smooth = native(dict(p, labelSmoothing=EPS, gradClipNorm=1.0, weightDecay=0.1), plain.get_parameters_dict())
    out = []
    for m in (plain, smooth):
        m.training(False)
        fwd = m.forwardBackward(train, onlyForward=True)
        ranks_gt = np.asarray(m.retrieveBatch(val, useGt=True))
        N, O = ranks_gt.size, p['numOptions']
        out.append((np.float32(fwd), ranks_gt, m.scores(N, O), np.asarray(m.retrieveBatch(val, useGt=False))))
        m.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_every_knob_off_is_vd_clamp_adam(gpu):
    """c = lambda = 0 written out: the flat W, dW, m, v after `update` carry the bits vd_clamp_adam leaves on copies of what stood there"""
    from visdial_amd import _lib, ops
    from visdial_amd.native import _DevArray
    p = tiny('disc')
    model = native(dict(p, labelSmoothing=0.0, gradClipNorm=0.0, weightDecay=0.0))
    batch = SyntheticDataloader(p, seed=15).getTrainBatch(p)
    ptrs = [C.c_void_p() for _ in range(4)]
    _lib.call("vd_model_flat_pointers", model.h, *[C.byref(x) for x in ptrs])
    n = int(_lib.load().vd_model_flat_size(model.h))
    flat = [torch.as_tensor(_DevArray(x.value, n), device='cuda') for x in ptrs]
    for t in range(1, 3):
        model.forwardBackward(batch)
        model.synchronize()
        copies = [x.clone() for x in flat]
        lr = model.optims['learningRate']
        model.update()
        model.synchronize()
        ops.clamp_adam(*copies, np.float32(lr * np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t)))
        torch.cuda.synchronize()
        for a, b in zip(flat, copies):
            assert torch.equal(a, b)
    model.close()


@pytest.mark.parametrize("decoder", ['disc', 'gen'])
def test_three_iterations_with_every_knob_on(gpu, decoder):
    p = tiny(decoder, labelSmoothing=0.1, gradClipNorm=0.5, weightDecay=0.01)
    model = native(p)
    dl = SyntheticDataloader(p, seed=16)
    losses = [model.trainIteration(dl) for _ in range(3)]
    assert np.isfinite(losses).all() and np.isfinite(model.runningLoss)
    assert all(np.isfinite(v).all() for v in model.get_parameters_dict().values())
    model.close()
