"""Ranking on a rollout (evaluate.py -rollout 1; csrc/beam.hip E1-E5): the candidates of round r are ranked on a history of the model's OWN
answers to the rounds before it.  Here, without a device: the rule (split_eval.rollout_candidate_row + rollout_history_row) fed the
ground-truth candidates rebuilds the dataloader's history bit for bit, the pick and the words on hand-made rows, the host loop driven by
a stub host exactly as E1-E5 say, every refusal of evaluate.py by its flag, and the C surface and documents in place."""
import argparse
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_rollout_cpu import prepro_loader
from visdial_amd import split_eval
from visdial_amd.split_eval import SplitEval, rollout_candidate_row, rollout_history_row, rollout_pick, rollout_picked_history


@pytest.fixture(scope="module")
def loader():
    return prepro_loader(('val',), 'mn-ques-im-hist')


# ------------------------------------------------------------------------------------------------------------ 1. the rule
def test_ground_truth_candidates_rebuild_the_dataloaders_history(loader):
    """E3 + E4 fed opt_list[opt[i, r-1, ans_ind - 1] - 1] give data['val']['hist'] rows 1 .. 9 exactly: 36 of 36"""
    p, dl = loader
    d = dl.data['val']
    n, R, Th = d['hist'].shape
    assert (n, R, Th) == (4, 10, 14) and d['opt_list'].shape[1] == 6 and not dl.concatHistory
    seen = 0
    for i in range(n):
        for r in range(1, R):
            cand = d['opt_list'][d['opt'][i, r - 1, d['ans_ind'][i, r - 1] - 1] - 1]
            got = rollout_history_row(d['ques_fwd'][i, r - 1], rollout_candidate_row(cand), Th, 0)
            assert np.array_equal(got, d['hist'][i, r]), (i, r, got, d['hist'][i, r])
            seen += 1
    assert seen == 36
    # the facts the rule leans on: duplicate candidates inside a round are common, and the list has an empty answer
    opts = d['opt_list'][d['opt'] - 1]                                   # [4 x 10 x 100 x 6]
    dup = sum(100 - len(np.unique(opts[i, r], axis=0)) for i in range(n) for r in range(R))
    assert dup == 105 and (~d['opt_list'].any(1)).sum() == 1
    # ... and the same through the batch-level helper, which evaluate.py counts the differing rows with
    batch = dict(ques_fwd=d['ques_fwd'], hist=d['hist'], options=opts.reshape(40, 100, 6))
    assert np.array_equal(rollout_picked_history(batch, d['ans_ind'].reshape(-1) - 1), d['hist'])


def test_pick_and_candidate_row_on_hand_made_rows():
    # E2: rank 1, wherever it stands; the ranks of equal scores went to the lower index when they were computed
    assert rollout_pick([3, 1, 2]) == 1 and rollout_pick(np.array([1, 2, 3, 4])) == 0
    from oracle import visdial_oracle as vo
    tie = vo.compute_ranks(np.array([[0.5, 2.0, 2.0, -1.0, 2.0]]))
    assert tie.tolist() == [[4, 1, 2, 5, 3]] and rollout_pick(tie[0]) == 1
    assert rollout_pick(vo.compute_ranks(np.zeros((1, 100)))[0]) == 0
    for bad in ([2, 3, 4], [1, 1, 2]):
        with pytest.raises(ValueError, match='rank 1'):
            rollout_pick(bad)
    # E3: the words, in the shape rollout_history_row takes with endToken = 0
    Th = 6
    hist = lambda q, o: rollout_history_row(np.array(q), rollout_candidate_row(np.array(o)), Th, 0).tolist()
    assert rollout_candidate_row([4, 5, 0, 0]).tolist() == [0, 4, 5, 0]
    assert hist([0, 2, 3], [4, 5, 0, 0]) == [0, 0, 2, 3, 4, 5]
    assert rollout_candidate_row([0, 0, 0]).tolist() == [0, 0] and hist([0, 2, 3], [0, 0, 0]) == [0, 0, 0, 0, 2, 3]      # an empty row
    assert hist([0, 0, 0], [0, 0, 0]) == [0] * 6                                                                            # lq = 0 and no words
    assert rollout_candidate_row([4, 5, 6, 7]).tolist() == [0, 4, 5, 6, 7, 0] and hist([2], [4, 5, 6, 7]) == [0, 2, 4, 5, 6, 7]   # full width
    assert hist([2, 3, 8], [4, 5, 6, 7]) == [2, 3, 8, 4, 5, 6]                                                              # the answer is cut
    assert rollout_candidate_row([4, 0, 5, 6]).tolist() == [0, 4, 0] and hist([2], [4, 0, 5, 6]) == [0, 0, 0, 0, 2, 4]      # an interior 0 stops
    assert hist([2], [9, 9, 0]) == [0, 0, 0, 2, 9, 9]                                                                       # no token is an <END>


# ------------------------------------------------------------------------------------------------------------ 2. the host loop
class StubHost(SplitEval):
    """a host whose score of candidate o of round n depends on the round's history row and the candidate's tokens only"""

    def __init__(self, p):
        self.params = dict(p)
        self.seen = []                                      # a copy of every retrieved batch's history
        self.asked = []                                     # params useGt at every retrieval

    def _set_training(self, on):
        pass

    @staticmethod
    def scores(hist_row, options):
        key = int(np.dot(np.asarray(hist_row, np.int64), np.arange(1, len(hist_row) + 1) ** 2))
        tok = np.asarray(options, np.int64) @ (np.arange(1, options.shape[1] + 1) ** 3)
        return np.sin(0.37 * key + 1.3 * tok)               # equal tokens -> equal scores

    def retrieveBatch(self, batch):
        from oracle import visdial_oracle as vo
        self.seen.append(np.array(batch['hist']))
        self.asked.append(bool(self.params['useGt']))
        B, R = batch['hist'].shape[:2]
        s = np.stack([self.scores(batch['hist'][n // R, n % R], batch['options'][n]) for n in range(B * R)])
        return vo.compute_ranks(s, np.asarray(batch['answer_ind']).reshape(-1) - 1 if self.params['useGt'] else None)


def val_batch(host, dl, n=2):
    batch, nxt = host._test_batch(dl, 1, 'val', 1)
    return batch


def test_the_host_loop_retrieves_once_per_round_on_its_own_picks(loader):
    from oracle import visdial_oracle as vo
    p, dl = loader
    host = StubHost(dict(p, decoder='disc', batchSize=2, useGt=True))
    batch = val_batch(host, dl)
    truth = batch.pop('hist_gt')
    B, R, Th = batch['hist'].shape
    assert (B, R, Th) == (2, 10, 14) and np.array_equal(truth, dl.data['val']['hist'][:2])      # the UNTRIMMED width
    ranks = host.retrieve_rollout_batch(batch)
    assert len(host.seen) == R and ranks.shape == (B * R, 100) and host.params['useGt'] is True and not any(host.asked)
    want = np.array(truth)
    for r in range(R):
        # call r saw rows 0 .. r as E1 / E4 build them; only row r + 1 changes before call r + 1
        assert np.array_equal(host.seen[r][:, :r + 1], want[:, :r + 1]), r
        if r > 0:
            assert np.array_equal(host.seen[r][:, r + 1:], host.seen[r - 1][:, r + 1:]) and np.array_equal(host.seen[r][:, :r], host.seen[r - 1][:, :r])
        for i in range(B):
            n = i * R + r
            mine = vo.compute_ranks(StubHost.scores(want[i, r], batch['options'][n])[None])[0]
            assert np.array_equal(ranks[n], mine), (i, r)                                     # round r's ranks are pass r's
            if r + 1 < R:
                cand = batch['options'][n, rollout_pick(mine)]
                want[i, r + 1] = rollout_history_row(batch['ques_fwd'][i, r], rollout_candidate_row(cand), Th, 0)
    assert np.array_equal(batch['hist'], want) and (want != truth).any(2).sum() >= 1            # R6: the batch holds the generated rows
    assert np.array_equal(host.rollout_history(dict(batch, hist=truth), ranks), want)
    # a batch without a history is ranked once
    host = StubHost(dict(p, decoder='disc', useGt=False))
    calls = []
    host.retrieveBatch = lambda b: calls.append(1) or np.tile(np.arange(1, 101), (20, 1))
    nohist = {k: v for k, v in batch.items() if k != 'hist'}
    assert host.retrieve_rollout_batch(nohist).shape == (20, 100) and len(calls) == 1


def test_retrieve_and_predict_take_the_flag(loader):
    p, dl = loader
    plain = StubHost(dict(p, decoder='disc', batchSize=3))
    m0, rec0 = plain.retrieve(dl, 'val')
    assert len(plain.seen) == 2 and plain.seen[0].shape[2] <= 14 and plain.rolloutRows == (0, 0)       # as ever: one call per batch
    host = StubHost(dict(p, decoder='disc', batchSize=3, rollout=1))
    m1, rec1 = host.retrieve(dl, 'val')
    assert len(host.seen) == 20 and all(h.shape[2] == 14 for h in host.seen)
    differ, rows = host.rolloutRows
    assert rows == 40 and 1 <= differ <= 36
    assert [(r['image_id'], r['round_id']) for r in rec1] == [(r['image_id'], r['round_id']) for r in rec0] and len(rec1) == 40
    assert all(isinstance(r['ranks'], float) and 1 <= r['ranks'] <= 100 for r in rec1) and rec1 != rec0
    # round 0 sees the caption either way: its ground-truth rank does not move
    assert [r['ranks'] for r in rec1 if r['round_id'] == 1] == [r['ranks'] for r in rec0 if r['round_id'] == 1]
    allr = host.predict(dl, 'val')
    assert len(allr) == 40 and sorted(allr[5]['ranks']) == list(range(1, 101))
    gt = dl.data['val']['ans_ind'].reshape(-1)
    assert [r['ranks'][g - 1] for r, g in zip(allr, gt)] == [r['ranks'] for r in rec1]
    # refusals of the hosts themselves
    for bad, word in ((dict(rollout=2), 'rollout'), (dict(rollout=1, optionCache=1), 'optionCache'),
                      (dict(rollout=1, useHistory=True, concatHistory=True), 'concatHistory')):
        with pytest.raises(ValueError, match=word):
            StubHost(dict(p, decoder='disc', batchSize=3, **bad)).retrieve(dl, 'val')
    gen = StubHost(dict(p, decoder='gen', batchSize=3, rollout=1))
    with pytest.raises(ValueError, match='-host native'):
        gen.retrieve(dl, 'val')
    assert not gen.seen


# ------------------------------------------------------------------------------------------------------------ 3. argument rules
def test_evaluate_py_takes_the_flag_and_names_what_it_refuses():
    import evaluate
    a = evaluate.parse_args(['-loadPath', 'x'])
    assert a.rollout == 0 and a.beamSize == 5 and a.beamLen == 20 and (a.minLen, a.noRepeatNgram, a.lengthPenalty) == (0, 0, 0.0)
    a = evaluate.parse_args(['-loadPath', 'x', '-rollout', '1', '-beamSize', '3', '-beamLen', '6', '-minLen', '2', '-noRepeatNgram', '2',
                             '-lengthPenalty', '0.5'])
    assert a.rollout == 1 and (a.beamSize, a.beamLen, a.minLen, a.noRepeatNgram, a.lengthPenalty) == (3, 6, 2, 2, 0.5)
    with pytest.raises(SystemExit):
        evaluate.parse_args(['-loadPath', 'x', '-rollout', '2'])
    disc = dict(encoder='mn-att-ques-im-hist', decoder='disc', useHistory=True, concatHistory=False)
    args = lambda **kw: argparse.Namespace(**dict(dict(rollout=1, optionCache=0, perplexity=0, host='native'), **kw))
    evaluate.check_rollout(args(), disc)
    evaluate.check_rollout(args(host='python'), disc)
    evaluate.check_rollout(args(), dict(disc, decoder='gen'))
    evaluate.check_rollout(args(rollout=0, optionCache=1, perplexity=1, host='python'), dict(disc, decoder='gen', concatHistory=True))
    for bad, p, flag in ((args(optionCache=1), disc, '-optionCache'), (args(perplexity=1), disc, '-perplexity'),
                         (args(), dict(disc, encoder='lf-ques-im-hist', concatHistory=True), 'lf-ques-im-hist'),
                         (args(host='python'), dict(disc, decoder='gen'), '-host native')):
        with pytest.raises(SystemExit) as e:
            evaluate.check_rollout(bad, p)
        assert '-rollout 1' in str(e.value) and flag in str(e.value), e.value
    with pytest.raises(SystemExit, match='concatHistory'):
        evaluate.check_rollout(args(), dict(disc, encoder='lf-ques-hist', concatHistory=True))
    evaluate.check_rollout(args(), dict(disc, encoder='lf-ques-im', useHistory=False, concatHistory=True))      # no history: nothing to roll out


def test_the_c_surface_is_where_it_was_and_the_variable_is_documented():
    from visdial_amd import _lib
    read = lambda *parts: open(os.path.join(ROOT, *parts)).read()
    header = read('include', 'visdial_hip.h')
    assert re.search(r'^#define\s+VD_ABI_VERSION\s+2\s*$', header, re.M) and _lib.ABI_VERSION == 2
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    names = set(re.findall(r'\b(vd_[a-z0-9_]+)\s*\(', code))
    assert len(names) == 101 and names == set(_lib.PROTOTYPES)
    assert 'vd_disc_rollout_pick_p' not in header                     # internal to the library
    for text in (header, read('visdial_amd', 'csrc', 'rt_switches.h'), read('INTEGRATION.md'), read('README.md'), read('visdial_amd', 'native.py')):
        assert 'VD_RETRIEVE_ROLLOUT' in text
    beam = read('visdial_amd', 'csrc', 'beam.hip')
    assert 'disc_rollout_pick_kernel' in beam and 'vd_disc_rollout_pick_p' in read('visdial_amd', 'csrc', 'rt_core.h')
    assert beam.count('rollout_write_row(') == 3                      # one write-out body, called by both kernels
    for rule in ('E1.', 'E2.', 'E3.', 'E4.', 'E5.'):
        assert re.search(r'^//\s+' + re.escape(rule), beam, re.M), rule
        assert re.search(r'^#\s+' + re.escape(rule), read('visdial_amd', 'split_eval.py'), re.M), rule
    assert beam.index('//  R6.') < beam.index('//  E1.')
    assert 'VD_RETRIEVE' not in read('lua', 'visdial_ffi.lua')        # the Lua host needs no code
    assert '-rollout' in read('README.md') and 'rollout' in read('DESIGN.md')
    for fn in (split_eval.rollout_candidate_row, split_eval.rollout_pick, SplitEval.retrieve_rollout_batch):
        assert fn.__doc__
