"""Dense-annotation fine-tuning and NDCG through the model-level runtime (NativeModel): the batch attachment '@dense_relevance', the dense
head score_ce_dense_kernel, '@ndcg' / ndcg_kernel and VD_DENSE_MIX (csrc/loss.hip DT1-DT5), against visdial_amd/dense.py (fp64) and against
the PLAIN head, which the oracle tests already hold:

  1 loss from scores: after a dense step vd_model_loss is dense_ce of vd_model_scores' own scores, |diff| < 1e-4 (the bound
    tests/test_model_gpu.py holds vd_model_loss to against the oracle; an fp32 log-sum-exp over <= 128 terms);
  2 identity: rel = onehot(gt) on every row -- and no annotated row with mu = 1 -- give the plain step's loss and every gradient tensor
    of the plain step, rel-L2 < 1e-4 per tensor (conftest.grad_mismatches, the project's parity bound);
  3 linearity: G(t1 / 2 + t2 / 2) = G(t1) / 2 + G(t2) / 2 for two one-hot matrices, dropout masks pinned, the same bound: with 2 this pins
    the dense gradient to the plain head;
  4 weights: with mu = 0 another answer_ind in the rounds without an annotation changes no bit of the loss or the scores and moves no
    gradient tensor beyond REPEAT (below), while with mu = 0.5 the same change moves them by more than 1e-3; mu = 0.5 is check 1's loss;
  5 '@ndcg' is dense.ndcg_rows of the returned scores to 1e-12 (the call passes the kernel's doubles through bit for bit, in 2 N floats),
    rows with exactly tied scores (repeated candidates), k = 0, k = 1, k = O and rows without an annotation among them;
  6 the refusals, by their words;  7 a model that never attaches anything repeats its loss, scores and ranks bit for bit and its gradients
  within REPEAT;  8 evaluate.py -denseAnnotations.

REPEAT: gradients are not compared bit for bit, because the plain step itself does not repeat its gradient bits: the shared embedding, the
bias column sums, att.W and opt.W are accumulated with float atomics, whose order differs from run to run.  Measured on the MI355X over four
runs of one plain step of these settings, nothing attached: loss, scores and ranks identical; embed, ques1.b, ques2.b, hist1.b, img_common.b,
att.W, opt.W and opt.b differ by rel-L2 1.8e-9 .. 7.3e-7, every other tensor repeats.  Two orders of a sum of K fp32 terms differ by about
sqrt(K) 2^-24 relative; the longest sum here is opt.b's, K = N O To = 6 x 128 x 5 = 3 840 terms, which gives 3.7e-6.  REPEAT = 1e-5 is
about three times that and a tenth of the parity bound; a round that leaked into the gradient would move it by the order of 1 / N.

Sizes: B = 2, R = 3 (N = 6 rounds), H = 64, O in {5, 64, 65, 100, 128}: one partial wave, the wave boundary on either side, the workload's
size and MAX_OPT; 3 x 3 image maps.  Two cases repeat candidates inside a round, so the de-duplicating upload (d_optH_full) runs."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import grad_mismatches, small_params
from visdial_amd import dense
from visdial_amd.dataloader import SyntheticDataloader, dropout_mask_shapes
from visdial_amd.opts import derive

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENSE = os.path.join(ROOT, 'tests', 'golden', 'dense')
# (encoder, O, lstmPrecision, candidates repeat inside a round)
CASES = [('mn-att-ques-im-hist', 5, 'fp32', False), ('lf-ques', 64, 'split9', False), ('mn-att-ques-im-hist', 65, 'split9', True),
         ('lf-ques', 100, 'fp32', True), ('mn-att-ques-im-hist', 128, 'split9', False)]
IDS = ['%s-O%d-%s%s' % (e, o, prec, '-repeats' if dup else '') for e, o, prec, dup in CASES]
REPEAT = 1e-5                   # rel-L2 between two runs of the same step (the docstring has the reasoning)
EXACT_ZERO = ('att.b',)         # feeds a softmax over the regions: its exact gradient is 0, so a relative bound against an fp32 reference is undefined
WORST = {}                      # check -> the worst figure seen (printed by the last test: profiles/dense_finetune.txt quotes them)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def setting(enc, O, prec='split9', dup=False, decoder='disc', **kw):
    p = derive(small_params(encoder=enc, decoder=decoder, rnnHiddenSize=64, maxQuesCount=3, batchSize=2, numOptions=O, lstmPrecision=prec, **kw))
    dl = SyntheticDataloader(p, seed=17 + O)
    batch = dl.getTrainBatch(p)
    if dup and decoder == 'disc':         # every odd candidate repeats the one before it: half the rows are distinct, their scores tie exactly
        batch['options'] = np.array(batch['options'])
        batch['options'][:, 1::2] = batch['options'][:, 0:O - 1:2]
    masks = {k: (np.random.RandomState(5).rand(*s) > 0.5).astype(np.uint8) for k, s in dropout_mask_shapes(p, batch).items()}
    return p, batch, masks


def native(p, weights=None, masks=None):
    from visdial_amd.native import NativeModel
    m = NativeModel(p, init_seed=5)
    if weights is not None:
        m.set_parameters_dict(weights)
    if masks:
        m.set_dropout_masks(masks)
    return m


def step(model, batch, rel=None):
    """(loss, float64 gradient dict, scores) of one training step, `rel` attached behind the upload"""
    model.upload(batch)
    if rel is not None:
        model.attach_dense_relevance(rel)
    loss = model.forwardBackward()
    N = batch['ques_fwd'].shape[0] * batch['ques_fwd'].shape[1]
    return loss, {k: v.astype(np.float64) for k, v in model.get_gradients_dict().items()}, model.scores(N, batch['options'].shape[1])


def onehot(idx, O):
    t = np.zeros((len(idx), O), np.float32)
    t[np.arange(len(idx)), idx] = 1.0
    return t


def mixed_rel(O, seed=3):
    """six rows: sparse with ties | not annotated | k = O | k = 1 | k = 0 | sparse"""
    rng = np.random.RandomState(seed)
    rel = np.zeros((6, O), np.float32)
    for r in (0, 5):
        k = max(2, O // 3)
        rel[r, rng.choice(O, size=k, replace=False)] = rng.randint(1, 4, size=k) / 5.0
    rel[1] = -1.0
    rel[2] = rng.randint(1, 6, size=O) / 5.0
    rel[3, rng.randint(O)] = 0.8
    return rel


def note(check, value):
    WORST[check] = max(WORST.get(check, 0.0), float(value))


def worst_rel(g, ref):
    out = 0.0
    for k in ref:
        nb = float(np.linalg.norm(ref[k]))
        if nb >= 1e-12 and k not in EXACT_ZERO:
            out = max(out, float(np.linalg.norm(g[k] - ref[k])) / nb)
    return out


# ------------------------------------------------------------------------------------------------------------ 1, 4b: loss from scores
@pytest.mark.parametrize("enc, O, prec, dup", CASES, ids=IDS)
@pytest.mark.parametrize("mix", [0.0, 0.5])
def test_the_loss_is_dense_ce_of_the_steps_own_scores(gpu, enc, O, prec, dup, mix):
    p, batch, masks = setting(enc, O, prec, dup)
    model = native(dict(p, denseMix=mix), masks=masks)
    rel = mixed_rel(O)
    loss, g, scores = step(model, batch, rel)
    rows, total = model.option_rows()
    model.close()
    assert rows < total or not dup                                                  # the de-duplicating upload ran where candidates repeat
    want, _ = dense.dense_ce(scores, rel, batch['answer_ind'] - 1, mix)
    print('O = %d, mu = %g: vd_model_loss %.7f, dense_ce of the scores %.7f' % (O, mix, loss, want))
    note('1 |loss - dense_ce(scores)|', abs(loss - want))
    assert abs(loss - want) < 1e-4
    assert all(np.isfinite(v).all() for v in g.values())


# ------------------------------------------------------------------------------------------------------------ 2: identity
@pytest.mark.parametrize("enc, O, prec, dup", CASES, ids=IDS)
def test_onehot_relevance_and_mix_one_are_the_plain_step(gpu, enc, O, prec, dup):
    p, batch, masks = setting(enc, O, prec, dup)
    plain = native(p, masks=masks)
    W = plain.get_parameters_dict()
    loss0, g0, s0 = step(plain, batch)
    plain.close()
    gt = batch['answer_ind'] - 1
    for name, params, rel in (('rel = onehot(gt)', p, onehot(gt, O)), ('no annotated row, mu = 1', dict(p, denseMix=1.0), np.full((6, O), -1.0))):
        model = native(params, W, masks)
        loss, g, s = step(model, batch, rel)
        model.close()
        figure = worst_rel(g, g0)
        print('%s: loss %.7f (plain %.7f), worst gradient rel-L2 %.3g' % (name, loss, loss0, figure))
        note('2 identity, gradient rel-L2', figure)
        assert np.array_equal(s, s0)
        assert abs(loss - loss0) < 1e-4
        bad = grad_mismatches(g, g0, zero=EXACT_ZERO)
        assert not bad, (name, bad)


# ------------------------------------------------------------------------------------------------------------ 3: linearity
@pytest.mark.parametrize("enc, O, prec, dup", CASES, ids=IDS)
def test_the_gradient_is_affine_in_the_target(gpu, enc, O, prec, dup):
    p, batch, masks = setting(enc, O, prec, dup)
    assert masks                                                                    # dropout is on and its noise is pinned
    model = native(p, masks=masks)
    gt = batch['answer_ind'] - 1
    other = (gt + 1 + np.random.RandomState(9).randint(0, O - 1, size=gt.size)) % O    # another candidate in every round
    t1, t2 = onehot(gt, O), onehot(other, O)
    l1, g1, _ = step(model, batch, t1)
    l2, g2, _ = step(model, batch, t2)
    lm, gm, _ = step(model, batch, 0.5 * t1 + 0.5 * t2)
    model.close()
    want = {k: 0.5 * g1[k] + 0.5 * g2[k] for k in g1}
    figure = worst_rel(gm, want)
    print('O = %d: losses %.6f %.6f, mixed %.6f; worst rel-L2 of G(t1 / 2 + t2 / 2) against G(t1) / 2 + G(t2) / 2: %.3g' % (O, l1, l2, lm, figure))
    note('3 linearity, gradient rel-L2', figure)
    assert abs(lm - 0.5 * (l1 + l2)) < 1e-4
    bad = grad_mismatches(gm, want, zero=EXACT_ZERO)
    assert not bad, bad
    assert grad_mismatches(g2, g1, zero=EXACT_ZERO), "another target gave the same gradient"


# ------------------------------------------------------------------------------------------------------------ 4a: weights
@pytest.mark.parametrize("enc, O, prec, dup", [CASES[0], CASES[3]], ids=[IDS[0], IDS[3]])
def test_rounds_of_weight_zero_leave_no_trace(gpu, enc, O, prec, dup):
    p, batch, masks = setting(enc, O, prec, dup)
    rel = mixed_rel(O)
    rel[4] = -1.0                                                                   # rows 1 and 4 carry no annotation
    model = native(p, masks=masks)                                                  # mu = 0 (unset)
    loss, g, scores = step(model, batch, rel)
    moved = np.array(batch['answer_ind'])
    moved[[1, 4]] = (moved[[1, 4]] + 1) % O + 1                                     # two further: another candidate also where pairs repeat
    loss2, g2, scores2 = step(model, dict(batch, answer_ind=moved), rel)
    model.close()
    figure = worst_rel(g2, g)
    print('O = %d, mu = 0: worst gradient rel-L2 after another answer_ind in the rounds without an annotation: %.3g' % (O, figure))
    note('4 weight 0, gradient rel-L2', figure)
    assert loss == loss2 and np.array_equal(scores, scores2)
    assert not grad_mismatches(g2, g, tol=REPEAT, zero=EXACT_ZERO)
    half = native(dict(p, denseMix=0.5), masks=masks)                               # the same change where those rounds do train
    la, ga, _ = step(half, batch, rel)
    lb, gb, _ = step(half, dict(batch, answer_ind=moved), rel)
    half.close()
    assert la != lb and worst_rel(gb, ga) > 1e-3
    # ... and a round of weight 0 (not annotated, or annotated without a relevant candidate) is not in the loss at all
    keep = [0, 2, 3, 5]
    want, _ = dense.dense_ce(scores[keep], rel[keep], (moved - 1)[keep], 0.0)
    assert abs(loss - want) < 1e-4


# ------------------------------------------------------------------------------------------------------------ 5: NDCG
@pytest.mark.parametrize("enc, O, prec, dup", CASES, ids=IDS)
def test_ndcg_is_the_fp64_restatement_on_the_returned_scores(gpu, enc, O, prec, dup):
    p, batch, masks = setting(enc, O, prec, dup)
    model = native(p)
    model.training(False)
    rel = mixed_rel(O, seed=O)
    ranks = model.retrieveBatch(batch, useGt=False)
    scores = model.scores(6, O)
    if dup:
        assert (scores[:, 1::2] == scores[:, 0:O - 1:2]).all()                      # exactly tied scores: the tie rule decides
    got = model._ndcg_of_batch(batch, rel)                                          # attached after the retrieval: the scores are the batch's
    want = dense.ndcg_rows(scores, rel)
    print('O = %d: ndcg %s' % (O, np.array2string(got, precision=6)))
    note('5 |ndcg - ndcg_rows|', np.abs(got - want).max())
    assert got.dtype == np.float64 and np.abs(got - want).max() <= 1e-12
    assert got[1] == -2.0 and got[4] == -1.0 and 0.0 < got[2] <= 1.0 and 0.0 <= got[3] <= 1.0
    # the ranks the kernel ranks by are vd_model_ranks': a row's NDCG is 1 when its relevance is ordered as its scores are
    order = np.zeros((6, O), np.float32)
    order[np.arange(6)[:, None], np.argsort(ranks, axis=1)] = np.arange(O, 0, -1, dtype=np.float32)[None, :]
    assert np.array_equal(model._ndcg_of_batch(batch, order), np.ones(6))
    # a training step with the matrix attached before it ranks the same scores
    model.training(True)
    model.set_dropout_masks(masks)
    _, _, s = step(model, batch, rel)
    assert np.abs(model.ndcg_rows() - dense.ndcg_rows(s, rel)).max() <= 1e-12
    model.close()


def test_ndcg_of_a_generative_model_and_its_refusal_to_train_on_the_matrix(gpu):
    p, batch, _ = setting('lf-ques', 5, 'fp32', decoder='gen')
    dl = SyntheticDataloader(p, seed=4)
    test_batch, _ = dl.getTestBatch(1, dict(p, batchSize=2), 'val')
    model = native(p)
    model.training(False)
    model.retrieveBatch(test_batch, useGt=False)
    rel = mixed_rel(5)
    got = model._ndcg_of_batch(test_batch, rel)
    assert np.abs(got - dense.ndcg_rows(model.scores(6, 5), rel)).max() <= 1e-12
    model.training(True)
    model.upload(batch)
    model.attach_dense_relevance(rel)
    with pytest.raises(RuntimeError) as e:
        model.forwardBackward()
    assert "the batch carries '@dense_relevance'" in str(e.value) and "this model's decoder is 'gen'" in str(e.value)
    assert np.isfinite(model.forwardBackward(batch))                                # the next upload dropped the matrix
    model.close()


# ------------------------------------------------------------------------------------------------------------ 6: refusals
def test_refusals_keep_their_words(gpu):
    from visdial_amd._lib import VisdialHipError
    p, batch, masks = setting('lf-ques', 5, 'fp32')
    rel = mixed_rel(5)
    model = native(p)

    def refused(call, *words):
        with pytest.raises(VisdialHipError) as e:
            call()
        for w in words:
            assert w in str(e.value), str(e.value)
    refused(lambda: model.attach_dense_relevance(rel), "vd_model_set_tensor: '@dense_relevance' attaches to the batch uploaded last, and no batch "
            "has been uploaded")
    model.upload(batch)
    refused(lambda: model.attach_dense_relevance(rel[:5]), "'@dense_relevance' holds N x O = 6 x 5 = 30 values for this batch, got 25")
    bad = np.array(rel)
    bad[1, 2] = 0.5
    refused(lambda: model.attach_dense_relevance(bad), "'@dense_relevance' row 1 mixes -1 (4 entries) with relevances")
    bad = np.array(rel)
    bad[0, 3] = np.nan
    refused(lambda: model.attach_dense_relevance(bad), "'@dense_relevance' row 0, candidate 3 = nan: a relevance is finite and >= 0")
    bad = np.array(rel)
    bad[2, 0] = -0.5
    refused(lambda: model.attach_dense_relevance(bad), "'@dense_relevance' row 2, candidate 0 = -0.5: a relevance is finite and >= 0")
    refused(lambda: model.ndcg_rows(), "vd_model_get_tensor: '@ndcg'")              # nothing has been scored yet
    model.forwardBackward(onlyForward=True)
    refused(lambda: model.ndcg_rows(), "vd_model_get_tensor: '@ndcg' needs the relevance matrix of the current batch", "'@dense_relevance'")
    zero = np.zeros((6, 5), np.float32)
    zero[[0, 3]] = -1.0                                                             # mu = 0: W = 0
    model.attach_dense_relevance(zero)
    refused(lambda: model.forwardBackward(), "'@dense_relevance' gives every round the weight 0 (W = 0, VD_DENSE_MIX = 0)")
    assert np.isfinite(model.forwardBackward(onlyForward=True))                     # only_forward = 1 ignores the matrix (DT5)
    model.close()


def test_refusals_of_unknown_attachments_smoothing_and_the_mix(gpu):
    import ctypes as C
    from visdial_amd._lib import VisdialHipError, call
    p, batch, masks = setting('lf-ques', 5, 'fp32')
    rel = mixed_rel(5)
    model = native(p)
    buf = np.zeros(4, np.float32)
    for fn, args in (("vd_model_set_tensor", (b"@relevance", buf.ctypes.data, 4)), ("vd_model_get_tensor", (b"@dcg", 0, buf.ctypes.data, 4))):
        with pytest.raises(VisdialHipError) as e:
            call(fn, model.h, *args)
        assert "unknown batch attachment '%s'" % args[0].decode() in str(e.value)
    model.close()
    smooth = native(dict(p, labelSmoothing=0.1))
    smooth.upload(batch)
    smooth.attach_dense_relevance(rel)
    with pytest.raises(VisdialHipError) as e:
        smooth.forwardBackward()
    assert "the batch carries '@dense_relevance' and this model was created with VD_LABEL_SMOOTHING = 0.1" in str(e.value)
    smooth.close()
    for value in (2, -0.1, 'nan', 'x', ''):
        with pytest.raises(VisdialHipError) as e:
            native(dict(p, denseMix=value))
        assert "vd_model_create: VD_DENSE_MIX = '%s' must be a finite real in [0, 1]" % value in str(e.value)
    assert 'VD_DENSE_MIX' not in os.environ


# ------------------------------------------------------------------------------------------------------------ 7: unchanged paths
def test_a_model_without_an_attachment_repeats_itself(gpu):
    p, batch, masks = setting('mn-att-ques-im-hist', 100, 'split9')
    out = []
    for _ in range(2):
        model = native(p, masks=masks)
        loss, g, s = step(model, batch)
        model.training(False)
        out.append((loss, g, s, model.retrieveBatch(batch, useGt=False)))
        model.close()
    (l1, g1, s1, r1), (l2, g2, s2, r2) = out
    assert l1 == l2 and np.array_equal(s1, s2) and np.array_equal(r1, r2)
    figure = worst_rel(g2, g1)
    print('two runs of one plain step: worst gradient rel-L2 %.3g' % figure)
    note('7 plain step twice, gradient rel-L2', figure)
    assert not grad_mismatches(g2, g1, tol=REPEAT, zero=EXACT_ZERO)


# ------------------------------------------------------------------------------------------------------------ 8: evaluate.py
def test_evaluate_py_prints_the_same_ndcg_on_both_hosts_and_nothing_without_the_flag(gpu, tmp_path, capsys):
    import evaluate
    from test_eval_rollout_gpu import native as seeded, setting as prepro
    from test_rollout_cpu import PRE
    p, dl, batch = prepro('mn-ques-im-hist')
    model = seeded(p)
    ckpt = str(tmp_path / 'disc.pt')
    torch.save({'modelW': model.wrapperW.clone().cpu(),
                'modelParams': {k: v for k, v in p.items() if isinstance(v, (int, float, str, bool))}}, ckpt)
    model.close()
    data = ['-inputQues', os.path.join(PRE, 'visdial_data.h5'), '-inputImg', os.path.join(PRE, 'data_img.h5'),
            '-inputJson', os.path.join(PRE, 'visdial_params.json')]
    ann = os.path.join(DENSE, 'val_dense_annotations.json')
    records, lines = {}, {}
    for host, flag in (('native', 1), ('python', 1), ('native', 0), ('native', 2)):
        out = str(tmp_path / ('%s%d.json' % (host, flag)))
        evaluate.main(['-loadPath', ckpt, '-batchSize', '3', '-split', 'val', '-host', host, '-saveRanks', '1', '-saveRankPath', out] + data +
                      (['-denseAnnotations', ann] if flag else []) + (['-optionCache', '1'] if flag == 2 else []))
        records[host, flag] = json.load(open(out))
        lines[host, flag] = capsys.readouterr().out.splitlines()
    told = {k: [l for l in v if l.startswith('NDCG')] for k, v in lines.items()}
    assert told['native', 0] == [] and not any('ndcg' in r for r in records['native', 0])
    strip = lambda recs: [{k: v for k, v in r.items() if k != 'ndcg'} for r in recs]
    assert strip(records['native', 1]) == records['native', 0]                      # the flag adds, it changes nothing
    metrics = lambda ls: [l for l in ls if l.startswith('\t')]
    assert metrics(lines['native', 1]) == metrics(lines['native', 0]) and len(metrics(lines['native', 0])) == 7
    for k in (('native', 1), ('python', 1), ('native', 2)):
        assert len(told[k]) == 1, lines[k]
        print(k, told[k][0])
    value = lambda l: float(l.split()[1])
    assert abs(value(told['native', 1][0]) - value(told['python', 1][0])) < 1e-6
    assert abs(value(told['native', 1][0]) - value(told['native', 2][0])) < 1e-6   # -optionCache: the same scores
    counts = lambda l: l.split('\t', 1)[1]
    assert counts(told['native', 1][0]) == counts(told['python', 1][0])
    assert counts(told['native', 1][0]).startswith('(4 annotated rounds in val, 1 of them without a relevant candidate left out; 1 annotations')
    with_ndcg = {(r['image_id'], r['round_id']): r['ndcg'] for r in records['native', 1] if 'ndcg' in r}
    assert sorted(with_ndcg) == [(2001, 3), (2002, 7), (2003, 1), (2004, 10)] and with_ndcg[2004, 10] == -1.0
    for r, q in zip(records['native', 1], records['python', 1]):
        assert ('ndcg' in r) == ('ndcg' in q) and abs(r.get('ndcg', 0) - q.get('ndcg', 0)) < 1e-6


def test_zz_print_the_worst_figures(gpu):
    for k in sorted(WORST):
        print('WORST %s: %.3g' % (k, WORST[k]))
