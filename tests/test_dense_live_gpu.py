"""A dense training step over the live rounds' candidate rows only, through the model-level runtime (NativeModel): the batch attachment
'@dense_relevance_live', dense_live_tokens_kernel and score_ce_dense_live_kernel (csrc/loss.hip DL1-DL5), against the all-rows dense step
('@dense_relevance'), which tests/test_dense_gpu.py holds to the fp64 restatement and to the plain head.  Sizes, cases and helpers are that
file's: B = 2, R = 3 (N = 6 rounds), H = 64, O in {5, 64, 65, 100, 128}, two cases with repeated candidates (the de-duplicating upload, whose
row index the compaction resolves); mixed_rel at mu = 0 leaves rounds 0, 2, 3, 5 live.

  1 a live step against the all-rows step of the same weights and pinned dropout masks: |loss difference| < 1e-4, every gradient tensor
    within conftest.grad_mismatches' default bound (rel-L2 1e-4), the live rounds' scores within 1e-4 max(1, |s|) (the tie tolerance of
    unexplained_rank_flips);  2 option_rows() is (4 O, 6 O) after the live step and the upload's own counts after the all-rows one;
  3 the other rounds' score rows are exactly 0, the loss is dense.dense_ce of the live rows' scores to 1e-4, and another answer_ind in the
    rounds that are not live changes no bit of loss or scores and moves no gradient beyond REPEAT (that file's run-to-run bound);
  4 every round live (onehot(gt) on all rows; no annotation with mu = 1): loss and scores of '@dense_relevance' bit for bit, gradients within
    REPEAT, the upload's row count;  5 live, all, live on ONE upload: each step is its kind's step;  6 retrieval after a live attachment is
    the plain retrieval bit for bit, '@ndcg' after a live training step is dense.ndcg_rows on the live rounds to 1e-12, -1 for k = 0 and -2
    without an annotation;  7 live sets of one round (the first, the last) and one live round per dialog;  8 the refusals by their words;
  9 train.py -denseRows live on the prepro fixture.

Measured on the MI355X over these cases (the worst figures, printed by the last test; profiles/dense_live.txt quotes them)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import grad_mismatches
from test_dense_gpu import CASES, EXACT_ZERO, IDS, REPEAT, mixed_rel, native, onehot, setting, worst_rel
from visdial_amd import dense

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIVE = [0, 2, 3, 5]             # the rounds of weight > 0 of mixed_rel at mu = 0
WORST = {}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def attach_and_step(model, batch, rel, live):
    """(loss, float64 gradient dict, scores, option_rows) of one training step on the upload in the slot"""
    model.attach_dense_relevance(rel, live=live)
    loss = model.forwardBackward()
    N, O = batch['ques_fwd'].shape[0] * batch['ques_fwd'].shape[1], batch['options'].shape[1]
    return loss, {k: v.astype(np.float64) for k, v in model.get_gradients_dict().items()}, model.scores(N, O), model.option_rows()


def step(model, batch, rel, live):
    model.upload(batch)
    return attach_and_step(model, batch, rel, live)


def note(check, value):
    WORST[check] = max(WORST.get(check, 0.0), float(value))


def assert_live_is_all(got, ref, live, tag):
    """check 1's three bounds and check 3's zero rows on a (live step, all-rows step) pair"""
    (l1, g1, s1, _), (l0, g0, s0, _) = got, ref
    figure, ds = worst_rel(g1, g0), float((np.abs(s1[live] - s0[live]) / np.maximum(1.0, np.abs(s0[live]))).max())
    print('%s: loss %.7f (all rows %.7f), worst gradient rel-L2 %.3g, worst live score difference / max(1, |s|) %.3g' % (tag, l1, l0, figure, ds))
    note('1 |loss difference|', abs(l1 - l0))
    note('1 gradient rel-L2', figure)
    note('1 live score difference / max(1, |s|)', ds)
    assert abs(l1 - l0) < 1e-4
    bad = grad_mismatches(g1, g0, zero=EXACT_ZERO)
    assert not bad, (tag, bad)
    assert ds < 1e-4
    other = np.setdiff1d(np.arange(s1.shape[0]), live)
    assert (s1[other] == 0).all() and not (s0[other] == 0).all()


# ------------------------------------------------------------------------------------------------------------ 1, 2, 3
@pytest.mark.parametrize("enc, O, prec, dup", CASES, ids=IDS)
def test_a_live_step_is_the_all_rows_step_over_fewer_rows(gpu, enc, O, prec, dup):
    p, batch, masks = setting(enc, O, prec, dup)
    rel = mixed_rel(O)
    assert dense.live_rounds(rel, 0.0).tolist() == LIVE
    model = native(p, masks=masks)
    ref = step(model, batch, rel, False)
    got = step(model, batch, rel, True)
    model.close()
    assert_live_is_all(got, ref, LIVE, 'O = %d' % O)
    assert got[3] == (4 * O, 6 * O)                                                 # 2: fails without the feature
    # ... and the upload's own counts after the all-rows one: the distinct rows (random candidates repeat by chance too), of 6 O
    assert ref[3][1] == 6 * O and ref[3][0] <= 6 * O and (ref[3][0] < 6 * O or not dup)
    want, _ = dense.dense_ce(got[2][LIVE], rel[LIVE], (batch['answer_ind'] - 1)[LIVE], 0.0)
    note('3 |loss - dense_ce(live scores)|', abs(got[0] - want))
    assert abs(got[0] - want) < 1e-4
    assert all(np.isfinite(v).all() for v in got[1].values())


@pytest.mark.parametrize("enc, O, prec, dup", [CASES[0], CASES[3]], ids=[IDS[0], IDS[3]])
def test_rounds_that_are_not_live_leave_no_trace(gpu, enc, O, prec, dup):
    p, batch, masks = setting(enc, O, prec, dup)
    rel = mixed_rel(O)
    model = native(p, masks=masks)
    loss, g, scores, _ = step(model, batch, rel, True)
    moved = np.array(batch['answer_ind'])
    moved[[1, 4]] = (moved[[1, 4]] + 1) % O + 1
    loss2, g2, scores2, rows = step(model, dict(batch, answer_ind=moved), rel, True)
    model.close()
    figure = worst_rel(g2, g)
    print('O = %d: worst gradient rel-L2 after another answer_ind in the rounds that are not live: %.3g' % (O, figure))
    note('3 another answer_ind, gradient rel-L2', figure)
    assert loss == loss2 and scores.tobytes() == scores2.tobytes() and rows == (4 * O, 6 * O)
    assert not grad_mismatches(g2, g, tol=REPEAT, zero=EXACT_ZERO)


# ------------------------------------------------------------------------------------------------------------ 4: every round live
@pytest.mark.parametrize("enc, O, prec, dup", [CASES[1], CASES[2]], ids=[IDS[1], IDS[2]])
def test_every_round_live_is_the_all_rows_attachment(gpu, enc, O, prec, dup):
    p, batch, masks = setting(enc, O, prec, dup)
    gt = batch['answer_ind'] - 1
    for name, params, rel in (('rel = onehot(gt)', p, onehot(gt, O)), ('no annotated row, mu = 1', dict(p, denseMix=1.0), np.full((6, O), -1.0))):
        model = native(params, masks=masks)
        l0, g0, s0, r0 = step(model, batch, rel, False)
        l1, g1, s1, r1 = step(model, batch, rel, True)
        model.close()
        figure = worst_rel(g1, g0)
        print('%s, O = %d: worst gradient rel-L2 %.3g, rows %s' % (name, O, figure, r1))
        note('4 every round live, gradient rel-L2', figure)
        assert l1 == l0 and s1.tobytes() == s0.tobytes() and r1 == r0 and r0[1] == 6 * O
        assert not grad_mismatches(g1, g0, tol=REPEAT, zero=EXACT_ZERO)


# ------------------------------------------------------------------------------------------------------------ 5: one upload
@pytest.mark.parametrize("enc, O, prec, dup", [CASES[2], CASES[4]], ids=[IDS[2], IDS[4]])
def test_live_all_live_on_one_upload(gpu, enc, O, prec, dup):
    p, batch, masks = setting(enc, O, prec, dup)
    rel = mixed_rel(O)
    model = native(p, masks=masks)
    first = {False: step(model, batch, rel, False), True: step(model, batch, rel, True)}
    model.upload(batch)
    for live in (True, False, True):
        loss, g, s, rows = attach_and_step(model, batch, rel, live)
        l0, g0, s0, r0 = first[live]
        note('5 one upload, gradient rel-L2', worst_rel(g, g0))
        assert loss == l0 and s.tobytes() == s0.tobytes() and rows == r0, live
        assert not grad_mismatches(g, g0, tol=REPEAT, zero=EXACT_ZERO), live
    # another live set on the same upload: the attachment replaces the one before it
    rel2 = np.array(rel)
    rel2[[0, 2]] = -1.0
    ref = step(model, batch, rel2, False)
    model.upload(batch)
    attach_and_step(model, batch, rel, True)
    got = attach_and_step(model, batch, rel2, True)
    model.close()
    assert got[3] == (2 * O, 6 * O)
    assert_live_is_all(got, ref, [3, 5], 'O = %d, live {3, 5} behind {0, 2, 3, 5}' % O)


# ------------------------------------------------------------------------------------------------------------ 6: retrieval and NDCG
@pytest.mark.parametrize("enc, O, prec, dup", [CASES[2], CASES[3]], ids=[IDS[2], IDS[3]])
def test_retrieval_and_ndcg_see_all_rounds(gpu, enc, O, prec, dup):
    p, batch, masks = setting(enc, O, prec, dup)
    rel = mixed_rel(O)
    model = native(p, masks=masks)
    model.training(False)
    ranks0 = model.retrieveBatch(batch, useGt=False)
    s0 = model.scores(6, O)
    model.upload(batch)
    model.attach_dense_relevance(rel, live=True)
    ranks1 = model._retrieved_ranks(False)
    s1 = model.scores(6, O)
    assert s1.tobytes() == s0.tobytes() and np.array_equal(ranks0, ranks1) and not (s1 == 0).all(1).any()
    assert model.option_rows()[1] == 6 * O and model.option_rows()[0] != 4 * O
    assert np.abs(model.ndcg_rows() - dense.ndcg_rows(s0, rel)).max() <= 1e-12        # of every round: the retrieval scored them all
    f0 = model.forwardBackward(onlyForward=True)                                    # only_forward = 1 ignores the live set too
    assert np.isfinite(f0) and not (model.scores(6, O) == 0).all(1).any()
    model.training(True)
    _, _, s, rows = step(model, batch, rel, True)
    got = model.ndcg_rows()
    model.close()
    want = dense.ndcg_rows(s, rel)
    note('6 |ndcg - ndcg_rows| after a live step', np.abs(got[LIVE] - want[LIVE]).max())
    assert rows == (4 * O, 6 * O) and np.abs(got[LIVE] - want[LIVE]).max() <= 1e-12 and (got[LIVE] >= 0).all()
    assert got[4] == -1.0 and got[1] == -2.0


# ------------------------------------------------------------------------------------------------------------ 7: live sets
@pytest.mark.parametrize("live", [[0], [5], [1, 5], [2, 3]], ids=['first', 'last', 'one-per-dialog-1-5', 'one-per-dialog-2-3'])
@pytest.mark.parametrize("enc, O, prec, dup", [CASES[2], CASES[3]], ids=[IDS[2], IDS[3]])
def test_live_sets(gpu, enc, O, prec, dup, live):
    p, batch, masks = setting(enc, O, prec, dup)
    full = mixed_rel(O)
    rel = np.full((6, O), -1.0, np.float32)                                         # one annotated round per dialog is the real data's pattern
    for n, src in zip(live, (0, 5)):
        rel[n] = full[src]
    assert dense.live_rounds(rel, 0.0).tolist() == live
    model = native(p, masks=masks)
    ref = step(model, batch, rel, False)
    got = step(model, batch, rel, True)
    model.close()
    assert got[3] == (len(live) * O, 6 * O)
    assert_live_is_all(got, ref, live, 'O = %d, live %s' % (O, live))


# ------------------------------------------------------------------------------------------------------------ 8: refusals
def test_refusals_by_their_words(gpu):
    from visdial_amd._lib import VisdialHipError
    p, batch, masks = setting('lf-ques', 5, 'fp32')
    rel = mixed_rel(5)

    def refused(call, *words):
        with pytest.raises(VisdialHipError) as e:
            call()
        for w in words:
            assert w in str(e.value), str(e.value)
    model = native(p)
    refused(lambda: model.attach_dense_relevance(rel, live=True), "vd_model_set_tensor: '@dense_relevance_live' attaches to the batch uploaded "
            "last, and no batch has been uploaded")
    model.upload(batch)
    refused(lambda: model.attach_dense_relevance(rel[:5], live=True), "'@dense_relevance_live' holds N x O = 6 x 5 = 30 values for this batch, got 25")
    bad = np.array(rel)
    bad[1, 2] = 0.5
    refused(lambda: model.attach_dense_relevance(bad, live=True), "'@dense_relevance_live' row 1 mixes -1 (4 entries) with relevances")
    bad = np.array(rel)
    bad[0, 3] = np.nan
    refused(lambda: model.attach_dense_relevance(bad, live=True), "'@dense_relevance_live' row 0, candidate 3 = nan: a relevance is finite and >= 0")
    zero = np.zeros((6, 5), np.float32)
    zero[[0, 3]] = -1.0                                                             # mu = 0: W = 0, no live round
    model.attach_dense_relevance(zero, live=True)
    refused(lambda: model.forwardBackward(), "gives every round the weight 0 (W = 0, VD_DENSE_MIX = 0)")
    assert np.isfinite(model.forwardBackward(onlyForward=True))
    from visdial_amd._lib import call
    buf = np.zeros(4, np.float32)
    refused(lambda: call("vd_model_set_tensor", model.h, b"@dense_relevance_all", buf.ctypes.data, 4),
            "unknown batch attachment '@dense_relevance_all' (the library knows '@dense_relevance' and '@dense_relevance_live')")
    model.close()
    half = native(dict(p, lstmPrecision='bf16'))
    half.upload(batch)
    refused(lambda: half.attach_dense_relevance(rel, live=True), "'@dense_relevance_live'", "this model was created with lstmBf16 = 1")
    half.attach_dense_relevance(rel)                                                # the all-rows form is what it was
    assert np.isfinite(half.forwardBackward())
    half.close()
    smooth = native(dict(p, labelSmoothing=0.1))
    smooth.upload(batch)
    smooth.attach_dense_relevance(rel, live=True)
    refused(lambda: smooth.forwardBackward(), "the batch carries '@dense_relevance' and this model was created with VD_LABEL_SMOOTHING = 0.1")
    smooth.close()


def test_a_generative_model_takes_the_live_name_for_ndcg_and_refuses_to_train_on_it(gpu):
    p, batch, _ = setting('lf-ques', 5, 'fp32', decoder='gen')
    model = native(p)
    model.upload(batch)
    model.attach_dense_relevance(mixed_rel(5), live=True)
    with pytest.raises(RuntimeError) as e:
        model.forwardBackward()
    assert "the batch carries '@dense_relevance'" in str(e.value) and "this model's decoder is 'gen'" in str(e.value)
    assert np.isfinite(model.forwardBackward(batch))
    model.close()


# ------------------------------------------------------------------------------------------------------------ 9: train.py
def test_train_py_dense_rows_live_end_to_end(gpu, tmp_path, monkeypatch, capsys):
    import train
    from test_rollout_cpu import PRE
    from visdial_amd.native import NativeModel
    losses = {}
    plain_iteration = NativeModel.trainIteration
    out = {}
    for rows in ('all', 'live'):
        losses[rows] = []
        monkeypatch.setattr(NativeModel, 'trainIteration', lambda self, dl, rows=rows: losses[rows].append(plain_iteration(self, dl)))
        monkeypatch.setattr(sys, 'argv', [
            'train.py', '-host', 'native', '-encoder', 'lf-ques-im-hist', '-decoder', 'disc', '-imgFeatureSize', '16', '-rnnHiddenSize', '32',
            '-embedSize', '16', '-batchSize', '2', '-savePath', str(tmp_path / rows) + '/', '-numEpochs', '100', '-saveIter', '1000',
            '--maxIters', '2', '-saveFormat', 'pt', '-denseAnnotations', os.path.join(ROOT, 'tests', 'golden', 'dense', 'train_dense_sample.json'),
            '-denseRows', rows, '-inputQues', os.path.join(PRE, 'visdial_data.h5'), '-inputImg', os.path.join(PRE, 'data_img.h5'),
            '-inputJson', os.path.join(PRE, 'visdial_params.json')])
        train.main()
        out[rows] = capsys.readouterr().out
        saved = torch.load(str(tmp_path / rows / 'model_final.pt'), weights_only=True)
        assert saved['modelParams']['denseRows'] == rows
    line = [l for l in out['live'].splitlines() if l.startswith('-denseRows live: the last step ran')]
    assert len(line) == 1 and '-denseRows' not in out['all'].split('Training..')[1]
    executed, total = int(line[0].split()[6]), int(line[0].split()[8])
    print(line[0], '| first-iteration loss: all %.7f, live %.7f' % (losses['all'][0], losses['live'][0]))
    assert 0 < executed < total == 2 * 10 * 100 and executed % 100 == 0
    assert len(losses['all']) == len(losses['live']) == 2 and abs(losses['all'][0] - losses['live'][0]) < 1e-4


def test_zz_print_the_worst_figures(gpu):
    for k in sorted(WORST):
        print('WORST %s: %.3g' % (k, WORST[k]))
