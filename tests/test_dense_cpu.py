"""Dense annotations without a device: visdial_amd/dense.py (the fp64 restatement of csrc/loss.hip DT1-DT4) against a hand case, the
oracle's rank rule and torch.autograd; the annotation reader and its refusals on the committed fixture (tests/golden/dense, written by
tests/golden/make_dense_fixture.py); the loader's dense batches; the flags of train.py / evaluate.py; the refusal of the operator-level
host; DENSE_SWITCHES behind the two frozen tables, what the library sees for a params and what it refuses (vd_model_create parses its
switches before it touches a device); the frozen header."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

from oracle import visdial_oracle as vo
from test_beam_cpu import _tiny_val
from test_rollout_cpu import prepro_loader
from visdial_amd import dense

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENSE = os.path.join(ROOT, 'tests', 'golden', 'dense')
VAL, TRAIN = os.path.join(DENSE, 'val_dense_annotations.json'), os.path.join(DENSE, 'train_dense_sample.json')


# ------------------------------------------------------------------------------------------------------------ DT2
def test_ndcg_hand_case():
    s = np.array([[0.1, 0.9, 0.5, 0.3]], np.float32)
    rel = np.array([[1, 0, 0.5, 0]])
    # k = 2; by score: candidate 1 (rel 0) then candidate 2 (rel 0.5): DCG = 0 / log2 2 + 0.5 / log2 3; ideal: 1 / log2 2 + 0.5 / log2 3
    dcg, idcg = 0.5 / np.log2(3), 1 + 0.5 / np.log2(3)
    assert int((rel > 0).sum()) == 2
    np.testing.assert_allclose(dense.ndcg_rows(s, rel), [dcg / idcg], rtol=1e-15)
    assert dense.ndcg_rows(rel.astype(np.float32), rel)[0] == 1.0                   # ranked as the relevance ranks: exactly 1


def test_tie_rule_is_the_rank_computation_and_the_sentinels():
    rng = np.random.RandomState(0)
    s = rng.randint(0, 4, size=(7, 12)).astype(np.float32)                          # many exactly tied scores
    assert np.array_equal(dense._ranks(s), vo.compute_ranks(s))                     # utils.computeRanks: ties to the lower index
    rel = rng.randint(0, 3, size=(7, 12)) / 2.0                                     # tied relevances too
    rel[2], rel[5] = 0.0, -1.0
    got = dense.ndcg_rows(s, rel)
    assert got[2] == dense.NO_RELEVANT == -1.0 and got[5] == dense.NOT_ANNOTATED == -2.0
    for n in (0, 1, 3, 4, 6):                                                       # an independent statement: sort, then cut at k
        k = int((rel[n] > 0).sum())
        by_score = sorted(range(12), key=lambda o: (-s[n, o], o))[:k]
        ideal = sorted(range(12), key=lambda o: (-rel[n, o], o))[:k]
        dcg = sum(rel[n, o] / np.log2(2 + i) for i, o in enumerate(by_score))
        idcg = sum(rel[n, o] / np.log2(2 + i) for i, o in enumerate(ideal))
        assert abs(got[n] - dcg / idcg) < 1e-14
    # swapping two candidates of equal score changes which one is ranked first: the lower index
    s2, r2 = np.array([[1.0, 1.0]], np.float32), np.array([[0.0, 1.0]])
    assert dense.ndcg_rows(s2, r2)[0] == 0.0 and dense.ndcg_rows(s2, r2[:, ::-1])[0] == 1.0
    assert dense.ndcg_mean(got) == (float(got[got >= 0].mean()), 6, 1)
    for bad, word in ((np.array([[0.5, -1.0]]), 'row 0'), (np.array([[0.0, 1.0], [np.nan, 0.0]]), 'row 1'), (np.array([[-0.5, -0.5]]), 'row 0')):
        with pytest.raises(ValueError, match='relevance %s is neither annotated' % word):
            dense.ndcg_rows(np.zeros(bad.shape, np.float32), bad)


# ------------------------------------------------------------------------------------------------------------ DT3, DT4
def _torch_soft_ce(s, t, w):
    x = torch.tensor(s, dtype=torch.float64, requires_grad=True)
    rows = -(torch.tensor(t) * torch.log_softmax(x, 1)).sum(1)
    loss = (torch.tensor(w) * rows).sum() / float(w.sum())
    loss.backward()
    return float(loss.detach()), x.grad.numpy()


@pytest.mark.parametrize("O", [1, 5, 100])
@pytest.mark.parametrize("mix", [0.0, 0.5, 1.0])
def test_dense_ce_is_a_weighted_soft_target_cross_entropy_under_autograd(O, mix):
    rng = np.random.RandomState(O + int(10 * mix))
    N = 8
    s = rng.randn(N, O) * 3
    gt = rng.randint(0, O, N)
    rel = rng.randint(0, 4, size=(N, O)) / 3.0
    rel[0, 0] = 1.0                                                                 # at least one round trains
    rel[1], rel[2], rel[5] = -1.0, 0.0, -1.0
    t, w = dense.dense_targets(rel, gt, mix)
    assert w[2] == 0.0 and w[1] == w[5] == mix and w[0] == 1.0
    np.testing.assert_allclose(t[w > 0].sum(1), 1.0, rtol=1e-14)
    loss, ds = dense.dense_ce(s, rel, gt, mix)
    want, grad = _torch_soft_ce(s, t, w)
    np.testing.assert_allclose(loss, want, rtol=1e-12)
    np.testing.assert_allclose(ds, grad, rtol=1e-12, atol=1e-15)
    assert not ds[2].any() and (mix > 0 or not ds[[1, 5]].any())


def test_dense_ce_is_the_plain_cross_entropy_where_it_should_be():
    rng = np.random.RandomState(4)
    N, O = 6, 9
    s, gt = rng.randn(N, O) * 2, rng.randint(0, O, N)
    x = torch.tensor(s, requires_grad=True)
    plain = torch.nn.functional.cross_entropy(x, torch.tensor(gt))                  # mean over the rounds
    plain.backward()
    onehot = np.zeros((N, O))
    onehot[np.arange(N), gt] = 1.0
    for rel, mix in ((onehot, 0.0), (onehot * 0.4, 0.3), (np.full((N, O), -1.0), 1.0)):
        loss, ds = dense.dense_ce(s, rel, gt, mix)
        np.testing.assert_allclose(loss, float(plain.detach()), rtol=1e-12)
        np.testing.assert_allclose(ds, x.grad.numpy(), rtol=1e-12, atol=1e-15)
    with pytest.raises(ValueError, match='dense batch with W = 0'):
        dense.dense_ce(s, np.full((N, O), -1.0), gt, 0.0)
    with pytest.raises(ValueError, match=r'mix = 2 must be a finite real in \[0, 1\]'):
        dense.dense_ce(s, onehot, gt, 2)


# ------------------------------------------------------------------------------------------------------------ the reader and the fixture
def test_the_fixture_is_what_its_script_writes_and_holds_the_cases(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    import make_dense_fixture as mk
    mk.HERE = str(tmp_path)
    mk.main()
    for name in ('val_dense_annotations.json', 'train_dense_sample.json'):
        assert open(os.path.join(str(tmp_path), 'dense', name)).read() == open(os.path.join(DENSE, name)).read()
    val, train = dense.load_dense_annotations(VAL), dense.load_dense_annotations(TRAIN)     # "gt_relevance" and "relevance"
    assert 'gt_relevance' in json.load(open(VAL))[0] and 'relevance' in json.load(open(TRAIN))[0]
    assert sorted(val) == [(2001, 3), (2002, 7), (2003, 1), (2004, 10), (9999, 4)]
    assert sorted(train) == [(1001, 2), (1002, 5), (1004, 9)]
    k = {key: int((v > 0).sum()) for key, v in val.items()}
    assert k[2002, 7] == 100 and k[2003, 1] == 1 and k[2004, 10] == 0                # k = O, k = 1, k = 0
    assert len(np.unique(val[2001, 3])) < k[2001, 3]                                 # ties in relevance
    assert all(v.shape == (100,) and v.min() >= 0 and v.max() <= 1 for v in list(val.values()) + list(train.values()))
    p, dl = prepro_loader(('val',))
    rel = dense.relevance_matrix(dl.unique_img_val, val, dl.maxQuesCount, dl.numOptions)
    assert rel.shape == (40, 100) and rel.dtype == np.float32
    annotated = dense.annotated_rows(rel)
    assert list(np.nonzero(annotated)[0]) == [2, 16, 20, 39]                         # (dialog, round - 1): one annotated round per dialog
    assert np.array_equal(rel[16], val[2002, 7].astype(np.float32)) and (rel[~annotated] == -1).all()
    p, dl = prepro_loader(('train',))
    rel = dense.relevance_matrix(dl.unique_img_train, train, dl.maxQuesCount, dl.numOptions)
    assert list(np.nonzero(dense.annotated_rows(rel))[0]) == [1, 14, 38]             # dialogs 1003 and 1005 carry none
    with pytest.raises(ValueError, match='image_id 2003, round_id 1 has a wrong length: 100 relevances for 7 candidates'):
        dense.relevance_matrix([2003], val, 10, 7)


def test_the_reader_refuses_by_name(tmp_path):
    path = str(tmp_path / 'a.json')

    def refused(entries, words):
        json.dump(entries, open(path, 'w'))
        with pytest.raises(ValueError) as e:
            dense.load_dense_annotations(path)
        assert words in str(e.value) and path in str(e.value)
    ok = dict(image_id=1, round_id=2, gt_relevance=[0.0, 1.0])
    refused([ok, dict(ok, gt_relevance=[0.5, 0.5])], 'entry 1 is a duplicate annotation of image_id 1, round_id 2')
    refused([ok, dict(image_id=2, round_id=2, relevance=[0.0, 1.0, 0.5])],
            'entry 1 (image_id 2, round_id 2) has a wrong length: 3 relevances, the entries before it 2')
    refused([dict(image_id=1, round_id=2)], 'entry 0 needs image_id, round_id and gt_relevance (or relevance)')
    refused([dict(ok, gt_relevance=[0.0, -1.0])], 'entry 0 (image_id 1, round_id 2): a relevance is finite and >= 0')
    refused(dict(a=1), 'dense annotations are a JSON list')
    json.dump([ok, dict(image_id=1, round_id=3, relevance=[1, 0])], open(path, 'w'))
    assert sorted(dense.load_dense_annotations(path)) == [(1, 2), (1, 3)]


# ------------------------------------------------------------------------------------------------------------ the loader
def test_dense_train_batches_draw_annotated_dialogs_only_and_train_batches_stay():
    train = dense.load_dense_annotations(TRAIN)
    p, dl = prepro_loader(('train',))
    p = dict(p, decoder='disc', batchSize=4)
    seen = set()
    for _ in range(8):
        b = dl.getDenseTrainBatch(p, train)
        seen |= set(int(i) for i in b['image_id'])
        assert b['dense_relevance'].shape == (40, 100) and b['options'].shape[:2] == (40, 100) and b['answer_ind'].shape == (40,)
        annotated = dense.annotated_rows(b['dense_relevance']).reshape(4, 10)
        assert (annotated.sum(1) == 1).all()                                        # one annotated round per dialog
        for i, iid in enumerate(b['image_id']):
            r = [rr for (ii, rr) in train if ii == iid][0]
            assert annotated[i, r - 1] and np.array_equal(b['dense_relevance'][i * 10 + r - 1], train[int(iid), r].astype(np.float32))
    assert seen == {1001, 1002, 1004}                                               # with replacement, never 1003 or 1005
    with pytest.raises(ValueError, match='no dialog of the train split is annotated'):
        dl.getDenseTrainBatch(p, dense.load_dense_annotations(VAL))
    # getTrainBatch of a seeded loader: what the same draws from numpy's stream select, and no new key
    _, fresh = prepro_loader(('train',))
    inds = np.random.RandomState(1234).randint(1, 6, size=4)
    b = fresh.getTrainBatch(p)
    want = fresh.getIndexData(inds, p, 'train')
    assert set(b) == set(want) | {'options'} and 'image_id' not in b and 'dense_relevance' not in b
    for k in want:
        assert np.array_equal(b[k].reshape(want[k].shape), want[k]), k
    # the synthetic loader's dense batches: the ids of annotated images, its own batch otherwise
    from visdial_amd.dataloader import SyntheticDataloader
    from visdial_amd.opts import default_params
    sp = default_params(decoder='disc', encoder='lf-ques', vocabSize=30, batchSize=3, numOptions=100)
    syn = SyntheticDataloader(sp, seed=2, num_threads=5)
    b = syn.getDenseTrainBatch(sp, {(2, 4): np.ones(100), (5, 1): np.zeros(100), (77, 1): np.ones(100)})
    assert set(int(i) for i in b['image_id']) <= {2, 5} and b['dense_relevance'].shape == (30, 100)
    a, c = SyntheticDataloader(sp, seed=2, num_threads=5).getTrainBatch(sp), SyntheticDataloader(sp, seed=2, num_threads=5).getTrainBatch(sp)
    assert all(np.array_equal(a[k], c[k]) for k in a) and 'image_id' not in a


# ------------------------------------------------------------------------------------------------------------ flags
@pytest.mark.parametrize("argv, words", [
    (['-denseAnnotations', 'a.json'], "-denseAnnotations with -decoder gen: the dense target trains the option scores of decoder 'disc'"),
    (['-denseAnnotations', 'a.json', '-decoder', 'disc', '-labelSmoothing', '0.1'],
     '-denseAnnotations with -labelSmoothing 0.1: a dense target is not smoothed'),
    (['-denseMix', '2'], '-denseMix 2.0 must be a finite real in [0, 1]'),
    (['-denseMix', '-0.5'], '-denseMix -0.5 must be a finite real in [0, 1]'),
    (['-denseMix', 'nan'], '-denseMix nan must be a finite real in [0, 1]'),
    (['-denseMix', 'x'], "argument -denseMix/--denseMix: invalid float value: 'x'")])
def test_train_flags_refuse_by_name(capsys, argv, words):
    from visdial_amd import opts
    with pytest.raises(SystemExit):
        opts.parse(argv)
    assert words in capsys.readouterr().err


def test_train_flags_reach_the_params_and_a_resumed_run_takes_them_from_the_command_line():
    from visdial_amd import opts
    o = opts.parse([])
    assert (o['denseAnnotations'], o['denseMix']) == ('', 0.0)
    o = opts.parse(['-denseAnnotations', TRAIN, '-denseMix', '0.25', '-decoder', 'disc', '-host', 'native'])
    assert (o['denseAnnotations'], o['denseMix']) == (TRAIN, 0.25)
    assert not {k for k, _, _ in opts.OPTIONS} & {'denseAnnotations', 'denseMix'}   # OPTIONS mirrors opts.lua
    opts.parse(['-denseAnnotations', TRAIN, '-loadPath', 'x.t7'])                   # the decoder is the checkpoint's: train.py checks again
    with pytest.raises(ValueError, match='-denseAnnotations with -decoder gen'):
        opts.check_dense(dict(denseAnnotations=TRAIN, decoder='gen'))
    src = open(os.path.join(ROOT, 'train.py')).read()
    kept = re.search(r"for k in \('numEpochs'.*?\):", src, re.S).group(0)
    assert "'denseAnnotations'" in kept and "'denseMix'" in kept


def test_the_operator_level_host_refuses_dense_training_by_name(monkeypatch):
    from visdial_amd.model import refuse_dense_training
    refuse_dense_training({}), refuse_dense_training(dict(denseAnnotations='')), refuse_dense_training(dict(denseAnnotations=None))
    with pytest.raises(ValueError) as e:
        refuse_dense_training(dict(denseAnnotations='a.json'))
    assert "denseAnnotations = 'a.json'" in str(e.value) and '-host native' in str(e.value)
    import train
    monkeypatch.setattr(sys, 'argv', ['train.py', '-denseAnnotations', 'a.json', '-decoder', 'disc'])    # -host python is the default
    with pytest.raises(SystemExit) as e:
        train.main()
    assert "denseAnnotations = 'a.json'" in str(e.value) and '-host native' in str(e.value)


def test_evaluate_flag_defaults_to_unset_and_a_bad_file_is_refused_by_name(tmp_path):
    import evaluate
    assert evaluate.parse_args(['-loadPath', 'x']).denseAnnotations == ''
    assert evaluate.parse_args(['-loadPath', 'x', '-denseAnnotations', VAL, '-optionCache', '1', '-rollout', '0']).denseAnnotations == VAL
    from visdial_amd.split_eval import SplitEval
    assert SplitEval.denseAnnotations is None and SplitEval.ndcgRows is None


# ------------------------------------------------------------------------------------------------------------ the switch
class Stop(Exception):
    pass


def test_the_dense_row_chains_behind_the_two_frozen_tables():
    from visdial_amd import native
    assert len(native.SWITCHES) == 13 and len(native.TRAIN_SWITCHES) == 3
    assert tuple(r[:2] for r in native.DENSE_SWITCHES) == (('denseMix', 'VD_DENSE_MIX'),)
    assert all(len(r) == len(native.SWITCHES[0]) and r[5] is None for r in native.DENSE_SWITCHES)
    assert native.ALL_SWITCHES == native.SWITCHES + native.TRAIN_SWITCHES + native.DENSE_SWITCHES


@pytest.mark.parametrize("before", [None, 'before'], ids=['unset', 'preset'])
def test_what_the_library_sees_and_the_environment_comes_back(monkeypatch, before):
    from visdial_amd import native
    params = _tiny_val()[0]
    monkeypatch.delenv('VD_DENSE_MIX', raising=False)
    if before:
        monkeypatch.setenv('VD_DENSE_MIX', before)
    seen = []

    def fake_call(name, *args):
        assert name == 'vd_model_create'
        seen.append(os.environ.get('VD_DENSE_MIX'))
        raise Stop()
    monkeypatch.setattr(native, 'call', fake_call)
    for p, want in ((dict(params), None), (dict(params, denseMix=0.5), '0.5'), (dict(params, denseMix=0), '0'), (dict(params, denseMix=None), None),
                    (dict(params, decoder='disc', denseMix=1.0), '1.0'), (dict(params, denseMix='x'), 'x')):      # Python validates nothing
        with pytest.raises(Stop):
            native.NativeModel(p)
        assert seen[-1] == want and os.environ.get('VD_DENSE_MIX') == before


@pytest.mark.parametrize("decoder", ['gen', 'disc'])
@pytest.mark.parametrize("value", [2, -0.1, 1.0000001, float('nan'), float('inf'), 'x', ''])
def test_the_library_refuses_the_mix_by_name(decoder, value):
    from visdial_amd import _lib
    from visdial_amd.native import NativeModel
    with pytest.raises(_lib.VisdialHipError) as e:
        NativeModel(dict(_tiny_val()[0], decoder=decoder, denseMix=value))
    assert ("vd_model_create: VD_DENSE_MIX = '%s' must be a finite real in [0, 1] (0 = rounds without an annotation do not train)" % value) in str(e.value)
    assert 'VD_DENSE_MIX' not in os.environ


def test_what_passes_the_switch():
    """without a device the create fails at its first allocation, not naming the variable; on a device it succeeds"""
    from visdial_amd import _lib
    from visdial_amd.native import NativeModel
    for value in (0, 1, 0.5, '1e-1', '0.0'):
        try:
            NativeModel(dict(_tiny_val()[0], decoder='disc', denseMix=value)).close()
        except _lib.VisdialHipError as e:
            assert 'VD_DENSE_MIX' not in str(e), str(e)


# ------------------------------------------------------------------------------------------------------------ frozen surfaces
def test_the_header_still_declares_101_names_and_documents_the_additions():
    from visdial_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'visdial_hip.h')).read()
    names = set(re.findall(r'\b(vd_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', header, flags=re.S)))
    assert len(names) == 101 and names == set(_lib.PROTOTYPES)
    assert re.search(r'^#define\s+VD_ABI_VERSION\s+2\s*$', header, re.M) and _lib.ABI_VERSION == 2
    read = lambda *parts: open(os.path.join(ROOT, *parts)).read()
    for word in ('@dense_relevance', '@ndcg', 'VD_DENSE_MIX'):
        for text in (header, read('INTEGRATION.md'), read('README.md'), read('DESIGN.md')):
            assert word in text, word
    loss = read('visdial_amd', 'csrc', 'loss.hip')
    for word in ('DT1', 'DT2', 'DT3', 'DT4', 'DT5', 'score_ce_dense_kernel', 'ndcg_kernel', 'score_ce_kernel', 'score_ce_smooth_kernel'):
        assert word in loss
    assert 'VD_DENSE_MIX' in read('visdial_amd', 'csrc', 'rt_switches.h')
