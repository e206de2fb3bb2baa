"""The image attention over a region count per image through the model-level runtime: vd_model_set_tensor '@img_regions'
(csrc/runtime.hip; rules IR1 - IR6 of csrc/attention.hip), NativeModel.upload / attach_img_regions, and train.py / evaluate.py -imgRegions.

The oracle knows square grids only, and needs nothing else: a dialog whose image holds k^2 live regions IS that dialog on a k x k grid of
its first k^2 regions.  So the reference of a batch of 3 dialogs with counts (1, 4, 9) is vo.forward_backward per dialog with
imgSpatialSize = 1, 2, 3, composed the way tests/test_native_gpu.py composes halves: mean over dialogs for `disc`, sum for `gen`.
Sizes: conftest.small_params with imgSpatialSize = 3 and R = 10: N * S2 = 270 rows, which puts the image products on the exact split
under lstmPrecision = split9 (paths.h vd_img_split_ok: >= 128 rows).  Bounds are the project's: |dloss| < 1e-4, conftest.grad_mismatches
(rel-L2 1e-4), scores rel-L2 1e-4."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, grad_mismatches, small_params
from oracle import visdial_oracle as vo
from test_model_gpu import rel
from visdial_amd.dataloader import SyntheticDataloader, dropout_mask_shapes
from visdial_amd.opts import derive

pytestmark = pytest.mark.gpu

COUNTS = (1, 4, 9)
S, R = 3, 10
TOL = 1e-4


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def setting(enc, dec, prec='fp32', seed=5):
    """(params, batch of 3 dialogs with img_regions = COUNTS and zeros in the hidden rows, the same batch with finite garbage there)"""
    p = derive(small_params(encoder=enc, decoder=dec, imgSpatialSize=S, maxQuesCount=R, batchSize=3, lstmPrecision=prec, gpuid=0))
    batch = SyntheticDataloader(p, seed=seed).getTrainBatch(p)
    C = p['imgFeatureSize']
    cnt = np.asarray(COUNTS, np.int32)
    hidden = np.arange(S * S)[None, :] >= cnt[:, None]
    f = np.array(batch['img_feat'], np.float32).reshape(3, S * S, C)
    garbage = f.copy()
    garbage[hidden] = 3.0 * np.random.RandomState(seed + 1).randn(int(hidden.sum()), C).astype(np.float32)
    f[hidden] = 0.0
    zero = dict(batch, img_feat=f.reshape(3, S, S, C), img_regions=cnt)
    return p, zero, dict(zero, img_feat=garbage.reshape(3, S, S, C))


def dialog(batch, i, k=None):
    """dialog i alone; k: its image as a k x k grid of its first k^2 regions, without the counts"""
    B, Rr = batch['ques_fwd'].shape[:2]
    out = {key: np.array(v[i:i + 1] if v.shape[0] == B else v[i * Rr:(i + 1) * Rr]) for key, v in batch.items()}
    if k is not None:
        C = out['img_feat'].shape[-1]
        out['img_feat'] = np.ascontiguousarray(out['img_feat'].reshape(1, -1, C)[:, :k * k].reshape(1, k, k, C))
        out.pop('img_regions')
    return out


def oracle(p, P, batch):
    """loss, scores (disc) and gradients of the batch from one oracle run per dialog on its own grid"""
    outs = [vo.forward_backward(p['encoder'], p['decoder'], P, dict(p, imgSpatialSize=int(round(np.sqrt(c))), batchSize=1),
                                dialog(batch, i, int(round(np.sqrt(c)))), None) for i, c in enumerate(COUNTS)]
    w = 1.0 / len(outs) if p['decoder'] == 'disc' else 1.0
    grads = {k: w * sum(np.asarray(o['grads'][k], np.float64) for o in outs) for k in outs[0]['grads']}
    scores = np.concatenate([o['scores'] for o in outs]) if p['decoder'] == 'disc' else None
    return w * sum(o['loss'] for o in outs), scores, grads


def native(p, seed=3):
    from visdial_amd.native import NativeModel
    m = NativeModel(p, init_seed=seed)
    m.training(False)
    return m


def step(m, p, batch, only_forward=False):
    loss = m.forwardBackward(batch, onlyForward=only_forward)
    N = batch['ques_fwd'].shape[0] * batch['ques_fwd'].shape[1]
    scores = m.scores(N, p['numOptions']) if p['decoder'] == 'disc' else None
    return loss, scores, (None if only_forward else m.get_gradients_dict())


# ------------------------------------------------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("prec", ['fp32', 'split9'])
@pytest.mark.parametrize("dec", ['disc', 'gen'])
@pytest.mark.parametrize("enc", ['mn-att-ques-im-hist', 'lf-att-ques-im-hist'])
def test_mixed_counts_equal_the_oracle_on_each_dialogs_own_grid(gpu, enc, dec, prec):
    p, zero, garbage = setting(enc, dec, prec)
    m = native(p)
    P = {k: v.astype(np.float64) for k, v in m.get_parameters_dict().items()}
    ref_loss, ref_scores, ref_grads = oracle(p, P, zero)
    loss, scores, g = step(m, p, zero)
    print('%s %s %s: loss %.6f (oracle %.6f)' % (enc, dec, prec, loss, ref_loss))
    if scores is not None:
        print('scores rel-L2 %.3e' % rel(scores, ref_scores))
    bad = grad_mismatches(g, ref_grads)
    print('gradient mismatches: %s' % (bad,))
    assert abs(loss - ref_loss) < TOL, (loss, ref_loss)
    assert scores is None or rel(scores, ref_scores) < TOL
    assert not bad, bad
    # finite garbage in the hidden rows of the features: the forward never reads them through the head, the backward adds 0 * finite
    f_loss, f_scores, _ = step(m, p, zero, only_forward=True)
    g_loss, g_scores, _ = step(m, p, garbage, only_forward=True)
    assert np.float32(f_loss).tobytes() == np.float32(g_loss).tobytes(), (f_loss, g_loss)
    assert scores is None or np.array_equal(f_scores.view(np.uint32), g_scores.view(np.uint32))
    loss2, _, g2 = step(m, p, garbage)
    bad = grad_mismatches(g2, ref_grads)
    print('with garbage in the hidden rows: loss %.6f, gradient mismatches: %s' % (loss2, bad))
    assert abs(loss2 - ref_loss) < TOL and not bad, bad
    m.close()


# ------------------------------------------------------------------------------------------------------------ 2. full counts, training mode
@pytest.mark.parametrize("prec", ['fp32', 'split9'])
@pytest.mark.parametrize("enc,dec", [('mn-att-ques-im-hist', 'disc'), ('lf-att-ques-im-hist', 'gen')])
def test_full_counts_in_training_mode_are_the_step_without_the_attachment(gpu, enc, dec, prec):
    """IR6 through the runtime: pinned dropout masks, counts = 9 everywhere"""
    p, zero, garbage = setting(enc, dec, prec)
    rng = np.random.RandomState(11)
    masks = {k: (rng.rand(*shp) > 0.5).astype(np.uint8) for k, shp in dropout_mask_shapes(p, zero).items()}
    m = native(p)
    m.training(True)
    m.set_dropout_masks(masks)
    plain = {k: v for k, v in garbage.items() if k != 'img_regions'}
    a_loss, a_scores, a_g = step(m, p, plain)
    b_loss, b_scores, b_g = step(m, p, dict(plain, img_regions=np.full(3, S * S, np.int32)))
    assert np.float32(a_loss).tobytes() == np.float32(b_loss).tobytes(), (a_loss, b_loss)
    assert a_scores is None or np.array_equal(a_scores.view(np.uint32), b_scores.view(np.uint32))
    bad = grad_mismatches(b_g, {k: np.asarray(v, np.float64) for k, v in a_g.items()})
    print('%s %s %s: loss %.6f, gradient mismatches against the step without counts: %s' % (enc, dec, prec, a_loss, bad))
    assert not bad, bad
    m.close()


# ------------------------------------------------------------------------------------------------------------ 3. the attachment's lifetime
def test_a_later_upload_into_the_slot_without_counts_runs_unmasked(gpu):
    p, zero, garbage = setting('mn-att-ques-im-hist', 'disc')
    m = native(p)
    P = {k: v.astype(np.float64) for k, v in m.get_parameters_dict().items()}
    plain = {k: v for k, v in garbage.items() if k != 'img_regions'}
    ref = vo.forward_backward(p['encoder'], p['decoder'], P, p, plain, None)                # every row of the 3 x 3 grid, garbage included
    masked, masked_scores, _ = step(m, p, garbage)                                           # slot 0, with counts
    other, _, _ = step(m, p, SyntheticDataloader(p, seed=9).getTrainBatch(p))               # slot 1
    loss, scores, g = step(m, p, plain)                                                      # slot 0 again, no counts
    print('masked %.6f, unmasked on the same rows %.6f (oracle %.6f)' % (masked, loss, ref['loss']))
    assert abs(loss - ref['loss']) < TOL and rel(scores, ref['scores']) < TOL and not grad_mismatches(g, ref['grads'])
    assert rel(masked_scores, scores) > TOL                                                  # the garbage rows do change the function
    # and twice in a row, without a step in between (the same slot)
    m.upload(garbage)
    loss2, _, _ = step(m, p, plain)
    assert np.float32(loss2).tobytes() == np.float32(loss).tobytes()
    # an attachment replaces the one before it on the same upload
    m.upload(plain)
    m.attach_img_regions([9, 9, 9])
    m.attach_img_regions(COUNTS)
    loss3 = m.forwardBackward(None, onlyForward=True)
    assert np.float32(loss3).tobytes() == np.float32(step(m, p, garbage, only_forward=True)[0]).tobytes()
    m.close()


# ------------------------------------------------------------------------------------------------------------ 4. rollout
def test_round_rollout_over_mixed_counts_gives_the_full_rollouts_ranks(gpu):
    """retrieve_rollout_batch on a disc model: the passes of -rolloutEncoder round (forward_round: R = 1, cnt[row]) against those of `full`"""
    import test_eval_rollout_gpu as D
    p, dl, batch = D.setting('mn-att-ques-im-hist', 'synthetic')                             # 4 dialogs, 2 x 2 regions
    cnt = np.asarray([1, 4, 2, 3], np.int32)
    f = np.array(batch['img_feat'], np.float32).reshape(4, 4, -1)
    f[np.arange(4)[None, :] >= cnt[:, None]] = 0.0
    batch = dict(batch, img_feat=f.reshape(batch['img_feat'].shape), img_regions=cnt)
    full = D.native(p, retrieveRollout=1, rolloutEncoder='full')
    rnd = D.native(p, retrieveRollout=1, rolloutEncoder='round')
    plain = D.native(p)
    a, b = D.device_rollout(full, batch, [(0, 4)]), D.device_rollout(rnd, batch, [(0, 4)])
    D.same(b, a, batch['options'], 'mn-att-ques-im-hist, mixed counts, round against full')
    # the counts are read: without them the same rows rank differently somewhere, or at least score differently
    c = D.device_rollout(full, {k: v for k, v in batch.items() if k != 'img_regions'}, [(0, 4)])
    assert rel(c[1], a[1]) > D.TOL
    # and the history is the picks' (the host loop of a model without the variables generates the same one)
    host = D.host_loop(plain, batch, [(0, 4)])
    assert np.array_equal(host[2], D.rollout_picked_history(batch, D.picks_of(b[0])))
    for m in (full, rnd, plain):
        m.close()


# ------------------------------------------------------------------------------------------------------------ 5. the scripts
def test_train_and_evaluate_with_img_regions_on_the_fixture(gpu, tmp_path):
    pre = os.path.join(ROOT, 'tests', 'golden', 'prepro')
    data = ['-inputQues', os.path.join(pre, 'visdial_data.h5'), '-inputJson', os.path.join(pre, 'visdial_params.json'),
            '-inputImg', os.path.join(ROOT, 'tests', 'golden', 'regions', 'data_regions.npz'), '-imgRegions', '9', '-host', 'native']
    save = str(tmp_path / "ckpt") + "/"
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '-encoder', 'mn-att-ques-im-hist', '-decoder', 'disc',
                        '-imgFeatureSize', '8', '-rnnHiddenSize', '32', '-embedSize', '16', '-commonEmbeddingSize', '32', '-batchSize', '2',
                        '-savePath', save, '-saveIter', '1000', '--maxIters', '2', '-saveFormat', 'pt'] + data,
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert 'using synthetic' not in r.stdout and '-imgRegions 9: imgSpatialSize = 3' in r.stdout
    saved = torch.load(save + 'model_final.pt', weights_only=True)
    assert saved['modelParams']['imgRegions'] == 9 and saved['modelParams']['imgSpatialSize'] == 3 and saved['modelParams']['imgNorm'] == 0
    ranks = str(tmp_path / 'ranks.json')
    e = subprocess.run([sys.executable, os.path.join(ROOT, 'evaluate.py'), '-loadPath', save + 'model_final.pt', '-batchSize', '3',
                        '-split', 'val', '-saveRanks', '1', '-saveRankPath', ranks] + data,
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert e.returncode == 0, e.stdout[-2000:] + e.stderr[-2000:]
    assert 'r@1:' in e.stdout and 'meanRR:' in e.stdout and '-imgRegions 9: imgSpatialSize = 3' in e.stdout
    rec = json.load(open(ranks))
    assert len(rec) == 40 and rec[0]['image_id'] == 2001 and all(1 <= x['ranks'] <= 100 for x in rec)


# ------------------------------------------------------------------------------------------------------------ 6. refusals
def test_the_library_refuses_by_its_words(gpu):
    from visdial_amd import _lib
    p, zero, _ = setting('mn-att-ques-im-hist', 'disc')
    m = native(p)
    with pytest.raises(_lib.VisdialHipError, match="'@img_regions' attaches to the batch uploaded last, and no batch has been uploaded"):
        m.attach_img_regions(COUNTS)
    m.upload({k: v for k, v in zero.items() if k != 'img_regions'})
    with pytest.raises(_lib.VisdialHipError, match=r"'@img_regions' holds one count per image, B = 3 values for this batch, got 2"):
        m.attach_img_regions([1, 2])
    for bad in ([1, 2.5, 3], [0, 1, 1], [1, 1, 10], [1, float('nan'), 2], [-1, 1, 1]):
        with pytest.raises(_lib.VisdialHipError, match=r"a region count is an integer in 1 \.\. S2 = 9"):
            m.attach_img_regions(bad)
    with pytest.raises(_lib.VisdialHipError) as e:
        a = np.zeros(3, np.float32)
        _lib.call("vd_model_set_tensor", m.h, b"@img_region", a.ctypes.data, a.size)
    assert "unknown batch attachment '@img_region' (the library knows '@dense_relevance' and '@dense_relevance_live')" in str(e.value)
    assert "'@img_regions'" in str(e.value)
    m.attach_img_regions(COUNTS)                                  # the refusals left the upload usable
    assert np.isfinite(m.forwardBackward(None, onlyForward=True))
    m.close()
    q = derive(small_params(encoder='mn-ques-im-hist', decoder='disc', maxQuesCount=R, batchSize=3, gpuid=0))
    n = native(q)
    n.upload(SyntheticDataloader(q, seed=1).getTrainBatch(q))
    with pytest.raises(_lib.VisdialHipError, match="encoder 'mn-ques-im-hist' has no image attention"):
        n.attach_img_regions(COUNTS)
    n.close()
