"""Rollout (generate.py -rollout 1; csrc/beam.hip R1-R6): every round is answered on a history of the model's OWN answers to the rounds
before it.  Here, without a device: the rule (split_eval.rollout_history_row) rebuilds the dataloader's history from the ground-truth
answers bit for bit, the per-dialog host loop drives a host exactly as R1-R6 say, and the argument rules and documents are in place."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from visdial_amd import split_eval, utils
from visdial_amd.opts import default_params, derive
from visdial_amd.split_eval import SplitEval, beam_search_round, rollout_history_row

PRE = os.path.join(ROOT, 'tests', 'golden', 'prepro')


def prepro_loader(splits=('val', 'test'), enc='lf-ques-im-hist'):
    """the committed prepro fixture as generate.py loads it (concatHistory = False, maxHistoryLen = 60)"""
    from visdial_amd.dataloader import Dataloader
    p = derive(default_params(encoder=enc, decoder='gen', embedSize=16, rnnHiddenSize=32, numLayers=2, imgFeatureSize=16, gpuid=0,
                              inputQues=os.path.join(PRE, 'visdial_data.h5'), inputImg=os.path.join(PRE, 'data_img.h5'),
                              inputJson=os.path.join(PRE, 'visdial_params.json')))
    dl = Dataloader(seed=1234).initialize(dict(p, concatHistory=False, maxHistoryLen=60), list(splits))
    for k in ('vocabSize', 'maxQuesCount', 'maxQuesLen', 'maxAnsLen'):
        p[k] = getattr(dl, k)
    return p, dl


@pytest.fixture(scope="module")
def loader():
    return prepro_loader()


# ------------------------------------------------------------------------------------------------------------ 1. the rule
@pytest.mark.parametrize("split,rows,zero_rows", [('val', 36, 0), ('test', 27, 10)])
def test_ground_truth_answers_rebuild_the_dataloaders_history(loader, split, rows, zero_rows):
    """R2 / R3 fed the ground-truth `ans_in` rows (<START>, the words, zeros) give data[split]['hist'] rows 1 .. R-1 exactly"""
    p, dl = loader
    d = dl.data[split]
    END = dl.word2ind['<END>']
    n, R, Th = d['hist'].shape
    assert Th == dl.maxQuesLen + dl.maxAnsLen == 14
    seen = zeros = 0
    for i in range(n):
        for r in range(1, R):
            got = rollout_history_row(d['ques_fwd'][i, r - 1], d['ans_in'][i, r - 1], Th, END)
            assert got.shape == (Th,) and np.array_equal(got, d['hist'][i, r]), (split, i, r, got, d['hist'][i, r])
            seen += 1
            zeros += int(not got.any())
    assert (seen, zeros) == (rows, zero_rows)


def test_the_rule_on_hand_made_rows():
    END, Th = 9, 6
    row = lambda *t: np.array(t)
    # lq = 0: only the answer's words; with no words either, all zeros
    assert rollout_history_row(row(0, 0, 0), row(1, 4, 5, END, 0), Th, END).tolist() == [0, 0, 0, 0, 4, 5]
    assert rollout_history_row(row(0, 0, 0), row(1, END, 0, 0, 0), Th, END).tolist() == [0] * 6
    # no <END>: every entry behind <START> is a word
    assert rollout_history_row(row(0, 2, 3), row(1, 4, 5, 6), Th, END).tolist() == [0, 2, 3, 4, 5, 6]
    # an empty answer (<END> at once, or nothing behind <START>)
    assert rollout_history_row(row(0, 2, 3), row(1, END, 7, 7), Th, END).tolist() == [0, 0, 0, 0, 2, 3]
    assert rollout_history_row(row(2, 3), row(1), Th, END).tolist() == [0, 0, 0, 0, 2, 3]
    # longer than Th - lq: the answer is cut, the question stays whole
    assert rollout_history_row(row(2, 3, 4, 5), row(1, 6, 7, 8, 6, END), Th, END).tolist() == [2, 3, 4, 5, 6, 7]
    assert rollout_history_row(row(2, 3, 4, 5, 6, 7), row(1, 8, END), Th, END).tolist() == [2, 3, 4, 5, 6, 7]
    # an interior 0 stops the answer; an interior 0 of the question is skipped (its non-zero tokens, in order)
    assert rollout_history_row(row(0, 2, 3), row(1, 4, 0, 5, END), Th, END).tolist() == [0, 0, 0, 2, 3, 4]
    assert rollout_history_row(row(2, 0, 3), row(1, 4, END), Th, END).tolist() == [0, 0, 0, 2, 3, 4]
    # <START> itself is never a word, whatever its id
    assert rollout_history_row(row(2), row(END, 4, END), Th, END).tolist() == [0, 0, 0, 0, 2, 4]
    with pytest.raises(ValueError, match='rollout'):
        rollout_history_row(row(2, 3, 4, 5, 6, 7, 8), row(1, END), Th, END)


# ------------------------------------------------------------------------------------------------------------ 2. the host loop
def stub_logp(hist_row, tokens, V):
    """[k x V] log-probabilities that depend on the history row and on each slot's token only (an all-zero row for token 0)"""
    out = np.zeros((len(tokens), V), np.float32)
    for i, t in enumerate(tokens):
        if int(t) == 0:
            continue
        seed = (int(np.dot(np.asarray(hist_row, np.int64), np.arange(1, len(hist_row) + 1) ** 2)) * 131 + int(t) * 7919) % (2 ** 31)
        x = np.random.RandomState(seed).standard_normal(V)
        out[i] = (x - np.log(np.exp(x).sum())).astype(np.float32)
    return out


class StubHost(SplitEval):
    """a host whose decoder step is `stub_logp` of the history row of the round begun, as last given to `_gen_encode`"""

    def __init__(self, p):
        self.params = p
        self.encoded = []                                   # a copy of every batch's history

    def _set_training(self, on):
        pass

    def _gen_encode(self, batch):
        self.hist = np.array(batch['hist'])
        self.encoded.append(self.hist)

    def _gen_begin(self, rounds):
        self.round = int(np.asarray(rounds)[0])

    def _gen_step(self, tokens):
        return stub_logp(self.hist[0, self.round], tokens, int(self.params['vocabSize']))

    def _gen_select(self, src, n_keep):
        pass

    def _gen_beam(self, *a):
        raise AssertionError('the device search is not reached')


def test_the_host_loop_encodes_once_per_round_on_its_own_answers(loader):
    p, dl = loader
    START, END, V = dl.word2ind['<START>'], dl.word2ind['<END>'], dl.vocabSize
    k, L, n = 3, 6, 3
    host = StubHost(p)
    out = host.generateAnswers(dl, 'val', dict(beamSize=k, beamLen=L, maxThreads=n, rollout=1, beamBatch=0))
    d = dl.data['val']
    R, Th = d['hist'].shape[1:]
    assert len(out) == n and len(host.encoded) == n * R              # one encode per round and dialog
    differs = 0
    for i in range(n):
        passes = host.encoded[i * R:(i + 1) * R]
        want = np.array(d['hist'][i])                                # R1: the caption row; rows >= 1 are rewritten below
        for r in range(R):
            assert passes[r].shape == (1, R, Th)                      # the UNTRIMMED width
            assert np.array_equal(passes[r][0, :r + 1], want[:r + 1]), (i, r)
            found = beam_search_round(lambda t: stub_logp(want[r], t, V), lambda s, m: None, k, L, START, END)
            assert out[i]['dialog'][r]['answer'] == utils.idToWords(found[0][0], dl.ind2word)
            assert out[i]['dialog'][r]['question'] == utils.idToWords(d['ques_fwd'][i, r], dl.ind2word)
            if r + 1 < R:
                want[r + 1] = rollout_history_row(d['ques_fwd'][i, r], found[0][0], Th, END)
        differs += int((want != d['hist'][i]).any(1).sum())
    assert differs > 0                                               # the generated history is not the ground truth's
    # rollout = 0: the calls it makes today -- one encode per dialog, the trimmed ground-truth history
    host = StubHost(p)
    plain = host.generateAnswers(dl, 'val', dict(beamSize=k, beamLen=L, maxThreads=n))
    assert len(host.encoded) == n and plain != out
    for i in range(n):
        assert np.array_equal(host.encoded[i], dl.getIndexData(np.array([i + 1]), p, 'val')['hist'])
    host = StubHost(p)
    assert host.generateAnswers(dl, 'val', dict(beamSize=k, beamLen=L, maxThreads=n, rollout=0)) == plain and len(host.encoded) == n
    # the constraints combine with it
    host = StubHost(p)
    limited = host.generateAnswers(dl, 'val', dict(beamSize=k, beamLen=L, maxThreads=1, rollout=1, beamMinLen=3, beamNoRepeat=2,
                                                    beamLengthPenalty=1.0))
    assert len(host.encoded) == R and all(len(e['answer'].split()) >= 3 for e in limited[0]['dialog'])


def test_an_encoder_without_a_history_generates_as_before():
    p, dl = prepro_loader(('val',), 'lf-ques')
    calls = []

    class NoHist(StubHost):
        def _gen_encode(self, batch):
            assert 'hist' not in batch
            calls.append(1)

        def _gen_step(self, tokens):
            return stub_logp(np.full(3, self.round), tokens, int(self.params['vocabSize']))
    a = NoHist(p).generateAnswers(dl, 'val', dict(beamSize=2, beamLen=4, maxThreads=2, rollout=1))
    assert len(calls) == 2
    assert a == NoHist(p).generateAnswers(dl, 'val', dict(beamSize=2, beamLen=4, maxThreads=2))


# ------------------------------------------------------------------------------------------------------------ 3. argument rules
def test_generate_py_takes_the_flag_and_refuses_what_cannot_roll_out():
    import generate
    a = generate.parse_args(['-loadPath', 'x'])
    assert a['rollout'] == 0
    a = generate.parse_args(['-loadPath', 'x', '-rollout', '1', '-minLen', '2', '-noRepeatNgram', '2', '-lengthPenalty', '0.5', '-beamBatch', '4'])
    assert a['rollout'] == 1 and a['minLen'] == 2 and a['beamBatch'] == 4
    with pytest.raises(ValueError, match='-rollout'):
        generate.parse_args(['-loadPath', 'x', '-rollout', '1', '-sampleWords', '1'])
    with pytest.raises(ValueError, match='-rollout'):
        generate.parse_args(['-loadPath', 'x', '-rollout', '1', '-beamSize', '6', '-beamGroups', '2'])
    with pytest.raises(SystemExit):
        generate.parse_args(['-loadPath', 'x', '-rollout', '2'])


def test_generate_answers_refuses_what_cannot_roll_out(loader):
    from visdial_amd.model import Model
    from visdial_amd.native import NativeModel
    p, dl = loader
    host = StubHost(p)
    with pytest.raises(ValueError, match='rollout'):
        host.generateAnswers(dl, 'val', dict(rollout=1, sampleWords=1))
    with pytest.raises(ValueError, match='rollout'):
        host.generateAnswers(dl, 'val', dict(rollout=1, beamSize=4, beamGroups=2))
    with pytest.raises(ValueError, match='rollout'):
        host.generateAnswers(dl, 'val', dict(rollout=2))
    # the operator-level host has no device rollout and says where it is
    assert Model._beam_rollout is SplitEval._beam_rollout and NativeModel._beam_rollout is not SplitEval._beam_rollout
    with pytest.raises(ValueError, match='-host native'):
        host.generateAnswers(dl, 'val', dict(rollout=1, beamBatch=2))
    assert not host.encoded
    SplitEval()._beam_rollout(0)


def test_the_c_surface_is_where_it_was_and_the_variable_is_documented():
    from visdial_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'visdial_hip.h')).read()
    assert re.search(r'^#define\s+VD_ABI_VERSION\s+2\s*$', header, re.M) and _lib.ABI_VERSION == 2
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    names = set(re.findall(r'\b(vd_[a-z0-9_]+)\s*\(', code))
    assert len(names) == 101 and names == set(_lib.PROTOTYPES)
    assert 'vd_beam_rollout_append_p' not in header                  # internal to the library
    read = lambda *parts: open(os.path.join(ROOT, *parts)).read()
    for text in (header, read('visdial_amd', 'csrc', 'rt_switches.h'), read('INTEGRATION.md'), read('README.md')):
        assert 'VD_BEAM_ROLLOUT' in text
    beam = read('visdial_amd', 'csrc', 'beam.hip')
    assert 'beam_rollout_append_kernel' in beam and 'vd_beam_rollout_append_p' in read('visdial_amd', 'csrc', 'rt_core.h')
    for rule in ('R1.', 'R2.', 'R3.', 'R4.', 'R5.', 'R6.'):
        assert re.search(r'^//\s+' + re.escape(rule), beam, re.M), rule
        assert re.search(r'^#\s+' + re.escape(rule), read('visdial_amd', 'split_eval.py'), re.M), rule
    assert 'VD_BEAM' not in read('lua', 'visdial_ffi.lua')            # the Lua host is out of scope
    assert split_eval.rollout_history_row.__doc__
