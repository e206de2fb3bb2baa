"""Rollout on the device (VD_BEAM_ROLLOUT = 1; csrc/beam.hip R1-R6): vd_model_beam_search answering every round on a history of the model's
own earlier answers, against the per-dialog host loop (split_eval.rollout_dialog: one upload and one encode per round), against the
PLAIN search of a model created without the variable on the history the rollout generated (the fixed point: it holds R5 and the
full-width layout of the history rows), at the edges of R2 / R3, and with the switch off.

The committed prepro fixture: 4 `val` dialogs (3 `test` dialogs, rounds missing), R = 10, V = 51, Th = 14, hidden 32, embedding 16, chunks
of 3 + 1 dialogs; the attention encoder (the graph encoders' length-sorted history) on the synthetic loader at the same sizes.  Scores
are held to the 1e-5 of the batched-beam test (test_beam_search_gpu.py)."""
import numpy as np
import pytest
import torch

from test_rollout_cpu import prepro_loader
from visdial_amd.opts import default_params, derive
from visdial_amd.split_eval import beam_search_round, rollout_history_row

pytestmark = pytest.mark.gpu

KEYS = ('ques_fwd', 'hist', 'img_feat')
ENCODERS = ['lf-ques-im-hist', 'hre-ques-im-hist', 'mn-att-ques-im-hist']
TOL = 1e-5


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def native(p, **kw):
    from visdial_amd.native import NativeModel
    m = NativeModel(dict(p, **kw), init_seed=1234)
    m.training(False)
    return m


def setting(enc, split='val'):
    """(params, batch of every dialog with the history at its untrimmed width, <START>, <END>)"""
    if 'att' in enc:
        from visdial_amd.dataloader import SyntheticDataloader
        p = derive(default_params(encoder=enc, decoder='gen', vocabSize=51, embedSize=16, rnnHiddenSize=32, imgFeatureSize=16,
                                  imgSpatialSize=2, commonEmbeddingSize=32, numLayers=2, maxQuesCount=10, maxQuesLen=8, maxAnsLen=6,
                                  maxHistoryLenPerRound=14, batchSize=4, gpuid=0))
        dl = SyntheticDataloader(p, seed=3)
        batch = dl.getTrainBatch(p)
        assert batch['hist'].shape == (4, 10, 14) and batch['ques_fwd'].shape[2] <= 14
        return p, {k: np.ascontiguousarray(batch[k]) for k in KEYS}, dl.startToken, dl.endToken
    p, dl = prepro_loader((split,), enc)
    n = dl.numThreads[split]
    from visdial_amd.split_eval import SplitEval
    host = SplitEval()
    host.params = p
    batch = host.rollout_batch(dl, np.arange(1, n + 1), split)
    assert 'hist' not in batch or batch['hist'].shape == (n, 10, 14)
    return p, {k: batch[k] for k in KEYS if k in batch}, dl.word2ind['<START>'], dl.word2ind['<END>']


def chunk(batch, lo, hi):
    return {k: np.array(v[lo:hi]) for k, v in batch.items()}              # copies: the host loop rewrites its batch's history


def host_rollout(model, batch, k, L, START, END, limits=(0, 0, 0.0)):
    """the per-dialog loop: (tokens [N x L], scores [N], the history it generated [B x R x Th])"""
    B = batch['ques_fwd'].shape[0]
    toks, scores, hist = [], [], np.array(batch['hist'])

    def search(r):
        model._gen_begin(np.full(k, r, np.int32))
        return beam_search_round(model._gen_step, model._gen_select, k, L, START, END, 1, 0.5, *limits)
    for i in range(B):
        one = chunk(batch, i, i + 1)
        for found in model.rollout_dialog(one, search, END):
            toks.append(np.asarray(found[0][0]))
            scores.append(found[0][1])
        hist[i] = one['hist'][0]
    return np.array(toks), np.array(scores), hist


def device_rollout(model, batch, k, L, START, END, chunks):
    toks, scores = [], []
    for lo, hi in chunks:
        model._gen_encode(chunk(batch, lo, hi))
        t, s = model._gen_beam(k, L, START, END)
        toks.append(t)
        scores.append(s)
    return np.concatenate(toks), np.concatenate(scores)


def rebuilt_history(batch, toks, END):
    """every history row from the answers by R2 / R3, on the host"""
    B, R, Th = batch['hist'].shape
    hist = np.array(batch['hist'])
    for i in range(B):
        for r in range(1, R):
            hist[i, r] = rollout_history_row(batch['ques_fwd'][i, r - 1], toks[i * R + r - 1], Th, END)
    return hist


def same(got, want, what):
    print('%s: %d rows, tokens equal: %s, max |score difference| %.3g' % (what, len(want[1]), np.array_equal(got[0], want[0]),
                                                                           np.abs(got[1] - want[1]).max()))
    assert np.array_equal(got[0], want[0]), what
    assert np.abs(got[1] - want[1]).max() < TOL, what


_CACHE = {}


def rollouts(enc):
    """k = 3, L = 6 on `val`: the host loop on a model created WITHOUT the variable and the device rollout in chunks of 3 + 1, computed
    once per encoder and shared by the tests below"""
    if enc not in _CACHE:
        p, batch, START, END = setting(enc)
        plain, roll = native(p), native(p, beamRollout=1)
        host = host_rollout(plain, batch, 3, 6, START, END)
        dev = device_rollout(roll, batch, 3, 6, START, END, [(0, 3), (3, 4)])
        roll.close()
        _CACHE[enc] = (p, batch, START, END, plain, host, dev)
    return _CACHE[enc]


@pytest.mark.parametrize("enc", ENCODERS)
def test_device_rollout_equals_the_host_loop(gpu, enc):
    p, batch, START, END, plain, host, dev = rollouts(enc)
    assert dev[0].shape == (40, 6) and dev[1].shape == (40,)
    same(dev, host, enc)
    # R6 and R2 agree: the history the host loop generated is the answers' rows
    assert np.array_equal(host[2], rebuilt_history(batch, dev[0], END))


@pytest.mark.parametrize("enc", ENCODERS)
def test_the_plain_search_on_the_generated_history_returns_the_rollout(gpu, enc):
    """the fixed point: an ordinary batch at the trimmed width, a model without the variable, every round at once"""
    p, batch, START, END, plain, host, dev = rollouts(enc)
    hist = rebuilt_history(batch, dev[0], END)
    changed = int((hist != batch['hist']).any(2).sum())
    print('%s: %d of %d history rows differ from the ground truth' % (enc, changed, hist.shape[0] * hist.shape[1]))
    assert changed >= 1
    width = int((hist != 0).sum(2).max())                             # rows are right-aligned: what getIndexData would keep
    assert not hist[:, :, :hist.shape[2] - width].any()
    fixed = dict(batch, hist=np.ascontiguousarray(hist[:, :, hist.shape[2] - width:]))
    plain._gen_encode(fixed)
    same(plain._gen_beam(3, 6, START, END), dev, enc)


@pytest.mark.parametrize("case", ['nothing finishes', 'answers are cut', 'missing rounds'])
def test_the_edges_of_the_rule_on_the_device(gpu, case):
    enc = 'lf-ques-im-hist'
    k, L, limits, split, chunks = {'nothing finishes': (3, 3, (0, 0, 0.0), 'val', [(0, 3), (3, 4)]),
                                   'answers are cut': (3, 10, (8, 0, 0.0), 'val', [(0, 3), (3, 4)]),
                                   'missing rounds': (3, 6, (0, 0, 0.0), 'test', [(0, 2), (2, 3)])}[case]
    p, batch, START, END = setting(enc, split)
    knobs = dict(beamMinLen=limits[0]) if limits[0] else {}
    plain, roll = native(p, **knobs), native(p, beamRollout=1, **knobs)
    host = host_rollout(plain, batch, k, L, START, END, limits)
    dev = device_rollout(roll, batch, k, L, START, END, chunks)
    same(dev, host, case)
    R, Th = batch['hist'].shape[1:]
    lq = (batch['ques_fwd'] != 0).sum(2).reshape(-1)
    words = np.array([len(rollout_history_row([], t, L, END).nonzero()[0]) for t in dev[0]])
    if case == 'nothing finishes':                                     # slot 0 is appended without <END>: both its words
        open_ = ~(dev[0] == END).any(1)
        print('%d of %d answers did not finish' % (open_.sum(), len(open_)))
        assert open_.sum() >= len(open_) // 2 and (words[open_] == L - 1).all()
    elif case == 'answers are cut':                                    # some answer is longer than the columns its question leaves
        assert (words >= 8).all() and (words > Th - lq).any()
    else:                                                              # the test split's missing rounds: lq = 0, a row of answer words alone
        print('%d question rows with lq = 0, %d all-zero history rows' % ((lq == 0).sum(), (~host[2].any(2)).sum()))
        assert (lq == 0).sum() >= 10
    assert np.array_equal(host[2], rebuilt_history(batch, dev[0], END))
    plain.close()
    roll.close()


def test_generate_answers_writes_the_per_dialog_records(gpu):
    """generateAnswers(beamBatch = 3, rollout = 1) on the native host = beamBatch = 0, rollout = 1; the knob is the model's"""
    p, dl = prepro_loader(('val',), 'lf-ques-im-hist')
    limits = dict(beamMinLen=2, beamNoRepeat=2, beamLengthPenalty=0.5)
    plain, roll = native(p, **limits), native(p, beamRollout=1, **limits)
    cfg = dict(beamSize=3, beamLen=6, maxThreads=4, rollout=1, **limits)
    ref = plain.generateAnswers(dl, 'val', cfg)
    assert roll.generateAnswers(dl, 'val', dict(cfg, beamBatch=3)) == ref
    assert ref != plain.generateAnswers(dl, 'val', dict(cfg, rollout=0))
    with pytest.raises(ValueError, match='beamRollout'):
        plain.generateAnswers(dl, 'val', dict(cfg, beamBatch=3))
    with pytest.raises(ValueError, match='beamRollout'):
        roll.generateAnswers(dl, 'val', dict(cfg, beamBatch=3, rollout=0))
    plain.close()
    roll.close()


def test_off_is_off(gpu):
    from visdial_amd import _lib
    from visdial_amd.native import NativeModel
    p, batch, START, END, plain, host, dev = rollouts('lf-ques-im-hist')
    # unset and 0: the plain search of every round on the uploaded history, as the per-dialog search on it finds them
    plain._gen_encode(batch)
    unset = plain._gen_beam(3, 6, START, END)
    zero = native(p, beamRollout=0)
    zero._gen_encode(batch)
    off = zero._gen_beam(3, 6, START, END)
    assert np.array_equal(off[0], unset[0]) and np.array_equal(off[1], unset[1])
    assert not np.array_equal(unset[0], dev[0])
    for i in range(2):
        plain._gen_encode(chunk(batch, i, i + 1))
        for r in range(10):
            plain._gen_begin(np.full(3, r, np.int32))
            t, s = beam_search_round(plain._gen_step, plain._gen_select, 3, 6, START, END)[0]
            assert np.array_equal(unset[0][i * 10 + r], t) and abs(unset[1][i * 10 + r] - s) < TOL
    zero.close()
    # an encoder without a history: the variable is accepted and the search is the plain one, bit for bit
    q, nohist, _, _ = setting('lf-ques-im')
    assert 'hist' not in nohist
    a, b = native(q), native(q, beamRollout=1)
    a._gen_encode(nohist)
    b._gen_encode(nohist)
    ta, tb = a._gen_beam(3, 6, START, END), b._gen_beam(3, 6, START, END)
    assert np.array_equal(ta[0], tb[0]) and np.array_equal(ta[1], tb[1])
    a.close()
    # what a rollout model refuses, by name
    with pytest.raises(_lib.VisdialHipError, match='VD_BEAM_ROLLOUT'):
        b._gen_sample(4, START, END, 1.0, np.full((4, 40), 0.5))
    b.close()
    with pytest.raises(_lib.VisdialHipError, match='VD_BEAM_ROLLOUT'):
        NativeModel(dict(p, beamRollout=1, beamGroups=2))
    with pytest.raises(_lib.VisdialHipError, match='VD_BEAM_ROLLOUT'):
        NativeModel(dict(p, beamRollout=2))
    NativeModel(dict(p, decoder='disc', numOptions=4, beamRollout=7)).close()     # ignored for disc
    narrow = native(p, beamRollout=1)
    with pytest.raises(_lib.VisdialHipError, match='VD_BEAM_ROLLOUT'):              # a history row has to hold a question
        narrow.upload(dict(batch, hist=np.ascontiguousarray(batch['hist'][:, :, -4:])))
    narrow.close()
