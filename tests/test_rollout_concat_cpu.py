"""Rollouts on a CONCATENATED history (evaluate.py -rollout 1 -rolloutHistory concat; csrc/beam.hip CH1-CH6), for the encoders whose history
row is the running concatenation of the dialog.  Here, without a device: the rule (split_eval.rollout_concat_row) fed the ground-truth answers
rebuilds the loader's concatenated history bit for bit (W = 140, longest row 120: nothing is cut), its edges on hand-made rows, the prefix
property CH6 in fp64 with the numpy oracle's LSTM, the host loop driven by a stub host, the argument rules of evaluate.py, the thirteenth
creation-time switch through NativeModel, and the C surface and documents in place."""
import argparse
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_beam_cpu import _tiny_val
from test_eval_rollout_cpu import StubHost
from test_rollout_cpu import PRE
from visdial_amd import split_eval
from visdial_amd.opts import default_params, derive
from visdial_amd.split_eval import (SplitEval, rollout_candidate_row, rollout_concat_len, rollout_concat_new, rollout_concat_row,
                                    rollout_pick, rollout_picked_history)


@pytest.fixture(scope="module")
def loader():
    """the committed prepro fixture as evaluate.py loads it for an lf encoder: concatHistory, W = min(R * (Tq + Ta), 300) = 140"""
    from visdial_amd.dataloader import Dataloader
    p = derive(default_params(encoder='lf-ques-im-hist', decoder='disc', embedSize=16, rnnHiddenSize=32, numLayers=2, imgFeatureSize=16, gpuid=0,
                              inputQues=os.path.join(PRE, 'visdial_data.h5'), inputImg=os.path.join(PRE, 'data_img.h5'),
                              inputJson=os.path.join(PRE, 'visdial_params.json')))
    assert p['useHistory'] and p['concatHistory']
    dl = Dataloader(seed=1234).initialize(p, ['val', 'test'])
    for k in ('vocabSize', 'maxQuesCount', 'maxQuesLen', 'maxAnsLen', 'numOptions'):
        p[k] = getattr(dl, k)
    return p, dl


# ------------------------------------------------------------------------------------------------------------ 1. the rule
@pytest.mark.parametrize("split,rows,end_only", [('val', 36, 0), ('test', 27, 10)])
def test_ground_truth_answers_rebuild_the_loaders_concatenated_history(loader, split, rows, end_only):
    """CH1 - CH4 fed the ground-truth `ans_in` rows (<START>, the words, zeros) give data[split]['hist'] rows 1 .. R-1 exactly"""
    p, dl = loader
    d = dl.data[split]
    END = dl.word2ind['<END>']
    n, R, W = d['hist'].shape
    assert W == 140 and d['hist_len'].max() <= 120
    seen = alone = 0
    for i in range(n):
        for r in range(1, R):
            cut = []
            got = rollout_concat_row(d['hist'][i, r - 1], d['ques_fwd'][i, r - 1], d['ans_in'][i, r - 1], END, END, cut)
            assert got.shape == (W,) and np.array_equal(got, d['hist'][i, r]), (split, i, r)
            assert cut == [False] and rollout_concat_len(got) == d['hist_len'][i, r]
            seen += 1
            alone += int(rollout_concat_new(d['ques_fwd'][i, r - 1], d['ans_in'][i, r - 1], END, END) == [END])
    assert (seen, alone) == (rows, end_only)                  # the test split's missing rounds: their rows gain only <END>


def test_ground_truth_candidates_rebuild_it_through_the_batch_helper(loader):
    p, dl = loader
    d = dl.data['val']
    END = dl.word2ind['<END>']
    opts = d['opt_list'][d['opt'] - 1]
    batch = dict(ques_fwd=d['ques_fwd'], hist=d['hist'], options=opts.reshape(40, 100, -1))
    cut = []
    assert np.array_equal(rollout_picked_history(batch, d['ans_ind'].reshape(-1) - 1, True, END, cut), d['hist'])
    assert len(cut) == 36 and not any(cut)
    assert not np.array_equal(rollout_picked_history(batch, d['ans_ind'].reshape(-1) - 1), d['hist'])       # E4 is another rule


def test_the_rule_on_hand_made_rows():
    END = 9
    row = lambda *t: np.array(t)

    def nxt(prev, q, a, answerEnd=END):
        cut = []
        out = rollout_concat_row(row(*prev), row(*q), row(*a), END, answerEnd, cut)
        return out.tolist(), cut[0]
    # an all-zero row 0: lenH = 0, the new tokens alone
    assert nxt([0] * 8, [0, 2, 3], [1, 4, 5, END]) == ([0, 0, 0, END, 2, 3, 4, 5], False)
    # lq = 0: <END> and the words; no words either: <END> alone (the missing rounds of the test split)
    assert nxt([0, 0, 0, 0, 0, 0, 6, 7], [0, 0, 0], [1, 4, END]) == ([0, 0, 0, 0, 6, 7, END, 4], False)
    assert nxt([0, 0, 0, 0, 0, 0, 6, 7], [0, 0, 0], [1, END, 0]) == ([0, 0, 0, 0, 0, 6, 7, END], False)
    # an empty answer (<END> at once; nothing behind <START>; a candidate row without words)
    assert nxt([0, 0, 0, 0, 0, 0, 6, 7], [0, 2, 3], [1, END, 4]) == ([0, 0, 0, 6, 7, END, 2, 3], False)
    assert nxt([0, 0, 0, 0, 0, 0, 6, 7], [2, 3], [1]) == ([0, 0, 0, 6, 7, END, 2, 3], False)
    assert nxt([0, 0, 0, 0, 0, 0, 6, 7], [2, 3], rollout_candidate_row([0, 0, 0]), 0) == ([0, 0, 0, 6, 7, END, 2, 3], False)
    # an exact fit
    assert nxt([0, 0, 0, 0, 0, 0, 6, 7], [2, 3], [1, 4, 5, 8, END]) == ([6, 7, END, 2, 3, 4, 5, 8], False)
    # room for <END> only
    assert nxt([0, 1, 2, 3, 4, 5, 6, 7], [2, 3], [1, 4, END]) == ([1, 2, 3, 4, 5, 6, 7, END], True)
    # a cut inside the words; a cut inside the question
    assert nxt([0, 0, 0, 0, 5, 5, 6, 7], [2, 3], [1, 4, 8, END]) == ([5, 5, 6, 7, END, 2, 3, 4], True)
    assert nxt([0, 0, 5, 5, 5, 5, 6, 7], [2, 3], [1, 4, 8, END]) == ([5, 5, 5, 5, 6, 7, END, 2], True)
    # a full row repeats itself -- unless there is nothing to add, which cannot be: <END> always is
    assert nxt([1, 2, 3, 4, 5, 5, 6, 7], [2, 3], [1, 4, END]) == ([1, 2, 3, 4, 5, 5, 6, 7], True)
    assert nxt([1, 2, 3, 4, 5, 5, 6, 7], [0, 0], [1, END]) == ([1, 2, 3, 4, 5, 5, 6, 7], True)
    # a 0 inside the row's tokens: CH2 counts from the FIRST non-zero column and keeps it
    assert rollout_concat_len([0, 0, 6, 0, 7]) == 3 and rollout_concat_len([0] * 5) == 0 and rollout_concat_len([3, 0, 0]) == 3
    assert nxt([0, 0, 0, 0, 0, 6, 0, 7], [2], [1, 4, END]) == ([0, 0, 6, 0, 7, END, 2, 4], False)
    # an interior 0 of the question is skipped, an interior 0 of the answer stops it; <START> is never a word, whatever its id
    assert nxt([0, 0, 0, 0, 0, 0, 0, 7], [2, 0, 3], [END, 4, 0, 5]) == ([0, 0, 0, 7, END, 2, 3, 4], False)
    # a picked candidate: no token is an <END> there (answerEnd = 0)
    assert nxt([0, 0, 0, 0, 0, 0, 0, 7], [2], rollout_candidate_row([END, 4, 0]), 0) == ([0, 0, 0, 7, END, 2, END, 4], False)
    # every row is a prefix extension of the one before (what CH6 rests on), through a cut and a repeat
    h = row(0, 0, 0, 0, 0, 0, 6, 7)
    for q, a in (([2, 3], [1, 4, END]), ([5], [1, 4, 4, 4, END]), ([5], [1, END])):
        n = rollout_concat_new(q, a, END, END)
        g = rollout_concat_row(h, q, a, END, END)
        lh, lg = rollout_concat_len(h), rollout_concat_len(g)
        assert g[8 - lg:].tolist() == h[8 - lh:].tolist() + n[:lg - lh] and lg - lh == min(len(n), 8 - lh)
        h = g
    assert rollout_concat_len(h) == 8


# ------------------------------------------------------------------------------------------------------------ 2. CH6 in fp64
def test_the_prefix_property_in_fp64_with_the_oracles_lstm():
    """the state of a two-layer maskZero stack after row r + 1 = its state after row r continued over the kept new tokens, for both layers --
    through an ordinary append, a cut row and a repeated row"""
    from oracle import visdial_oracle as vo
    rng = np.random.RandomState(5)
    D, H, V, W, END = 6, 8, 12, 10, 11
    emb = rng.randn(V + 1, D)
    emb[0] = 0
    W1, b1 = rng.randn(D + H, 4 * H) / 3, 0.1 * rng.randn(4 * H)
    W2, b2 = rng.randn(2 * H, 4 * H) / 3, 0.1 * rng.randn(4 * H)

    def stack(tokens, state=None):
        """the two layers over a token list (no pad: a pad in front leaves the zero state as it is), from `state` = ((h1, c1), (h2, c2))"""
        tok = np.asarray(tokens, np.int64).reshape(-1, 1)
        (h1, c1), (h2, c2) = state or ((None, None), (None, None))
        if tok.size == 0:
            return state
        hs1, cs1, _ = vo.lstm_forward(emb[tok], W1, b1, None, h1, c1)
        hs2, cs2, _ = vo.lstm_forward(hs1, W2, b2, None, h2, c2)
        return (hs1[-1], cs1[-1]), (hs2[-1], cs2[-1])

    def full_row(rowv):
        """the same stack over the right-aligned row with maskZero, as the encoders run it"""
        tok = np.asarray(rowv, np.int64).reshape(-1, 1)
        hs1, cs1, _ = vo.lstm_forward(emb[tok], W1, b1, tok)
        hs2, cs2, _ = vo.lstm_forward(hs1, W2, b2, tok)
        return (hs1[-1], cs1[-1]), (hs2[-1], cs2[-1])
    h = np.array([0, 0, 0, 0, 0, 0, 0, 3, 4, 5])
    carry = full_row(h)
    kinds = []
    for q, a in (([2, 6], [1, 7, END]), ([8, 9], [1, 2, 3, END]), ([4], [1, 5, END])):     # append, cut (room for 3 of 5), repeat (full)
        new = rollout_concat_new(q, a, END, END)
        g = rollout_concat_row(h, q, a, END, END)
        kept = new[:rollout_concat_len(g) - rollout_concat_len(h)]
        kinds.append((len(kept), len(new)))
        carry = stack(kept, carry)
        whole = full_row(g)
        for layer in range(2):
            for k in range(2):
                assert np.abs(carry[layer][k] - whole[layer][k]).max() < 1e-13, (kinds, layer, k)
        h = g
    assert kinds == [(4, 4), (3, 5), (0, 3)]


# ------------------------------------------------------------------------------------------------------------ 3. the host loop
def test_the_host_loop_concatenates_its_own_picks(loader):
    from oracle import visdial_oracle as vo
    p, dl = loader
    END = dl.word2ind['<END>']
    host = StubHost(dict(p, decoder='disc', batchSize=2, useGt=True, rollout=1, rolloutHistory='concat', rolloutConcatEnd=END))
    assert host._rollout() == 1 and host._concat_end() == END
    batch, _ = host._test_batch(dl, 1, 'val', 1)
    truth = batch.pop('hist_gt')
    B, R, W = batch['hist'].shape
    assert (B, R, W) == (2, 10, 140)
    ranks = host.retrieve_rollout_batch(batch)
    assert len(host.seen) == R and all(s.shape == (B, R, W) for s in host.seen) and ranks.shape == (B * R, 100)
    want = np.array(truth)
    for r in range(R):
        assert np.array_equal(host.seen[r][:, :r + 1], want[:, :r + 1]), r
        for i in range(B):
            n = i * R + r
            mine = vo.compute_ranks(StubHost.scores(want[i, r], batch['options'][n])[None])[0]
            assert np.array_equal(ranks[n], mine)
            if r + 1 < R:
                cand = rollout_candidate_row(batch['options'][n, rollout_pick(mine)])
                want[i, r + 1] = rollout_concat_row(want[i, r], batch['ques_fwd'][i, r], cand, END, 0)
    assert np.array_equal(batch['hist'], want) and (want != truth).any(2).sum() >= 1
    cut = []
    assert np.array_equal(host.rollout_history(dict(batch, hist=truth), ranks, cut), want) and cut == [False] * 18
    # retrieve(): the tally of differing and cut rows; at W = 40 rows are cut
    host = StubHost(dict(p, decoder='disc', batchSize=3, rollout=1, rolloutHistory='concat', rolloutConcatEnd=END))
    host.retrieve(dl, 'val')
    assert len(host.seen) == 20 and host.rolloutRows[1] == 40 and 1 <= host.rolloutRows[0] <= 36 and host.rolloutCut == 0
    # without the key the refusal stands; with it a per-round model and a missing <END> are refused by name
    for bad, word in ((dict(), 'concatHistory'), (dict(rolloutHistory='row'), 'concatHistory'),
                      (dict(rolloutHistory='concat'), 'rolloutConcatEnd'), (dict(rolloutHistory='concat', rolloutConcatEnd=99), 'rolloutConcatEnd'),
                      (dict(rolloutHistory='concat', rolloutConcatEnd=END, concatHistory=False, encoder='mn-ques-im-hist'), 'one row per round')):
        with pytest.raises(ValueError, match=word):
            StubHost(dict(p, decoder='disc', batchSize=3, rollout=1, **bad)).retrieve(dl, 'val')
    nohist = StubHost(dict(p, decoder='disc', rollout=1, rolloutHistory='concat', useHistory=False))       # ignored without a history
    assert nohist._rollout() == 1 and nohist._concat_end() == 0


def test_the_cut_is_counted(loader):
    p, dl = loader
    END = dl.word2ind['<END>']
    host = StubHost(dict(p, decoder='disc', batchSize=4, useGt=False, rollout=1, rolloutHistory='concat', rolloutConcatEnd=END))
    batch, _ = host._test_batch(dl, 1, 'val', 1)
    batch.pop('hist_gt')
    batch['hist'] = np.ascontiguousarray(batch['hist'][:, :, -40:])
    ranks = host.retrieve_rollout_batch(batch)
    cut = []
    hist = host.rollout_history(batch, ranks, cut)
    assert np.array_equal(hist, batch['hist']) and sum(cut) >= 20 and ((hist[:, -1] != 0).sum(1) == 40).all()
    assert any(np.array_equal(hist[i, 9], hist[i, 8]) for i in range(4))                                   # a full row repeats itself


def test_rollout_dialog_takes_the_rule():
    class Host(SplitEval):
        def __init__(self):
            self.seen = []

        def _gen_encode(self, batch):
            self.seen.append(np.array(batch['hist'][0]))
    END = 9
    batch = dict(ques_fwd=np.array([[[0, 2, 3], [0, 0, 4], [5, 6, 7]]]), hist=np.array([[[0] * 7 + [8], [7] * 8, [7] * 8]]))
    answers = [np.array([1, 4, END, 0]), np.array([1, 5, 5, 5]), np.array([1, END, 0, 0])]
    host = Host()
    found = host.rollout_dialog(batch, lambda r: [(answers[r], -1.0)], END, concat=True)
    assert len(found) == 3 and len(host.seen) == 3
    assert batch['hist'][0].tolist() == [[0, 0, 0, 0, 0, 0, 0, 8], [0, 0, 0, 8, END, 2, 3, 4], [8, END, 2, 3, 4, END, 4, 5]]
    assert host.seen[1][1].tolist() == [0, 0, 0, 8, END, 2, 3, 4] and host.seen[1][2].tolist() == [7] * 8   # R5: rows > r as they were


# ------------------------------------------------------------------------------------------------------------ 4. argument rules
def test_evaluate_py_takes_the_flag_and_names_what_it_refuses():
    import evaluate
    a = evaluate.parse_args(['-loadPath', 'x'])
    assert a.rolloutHistory == 'row'
    a = evaluate.parse_args(['-loadPath', 'x', '-rollout', '1', '-rolloutHistory', 'concat'])
    assert a.rolloutHistory == 'concat' and a.rollout == 1
    for bad in (['-rolloutHistory', 'concat'], ['-rollout', '1', '-rolloutHistory', 'rows']):
        with pytest.raises(SystemExit):
            evaluate.parse_args(['-loadPath', 'x'] + bad)
    lf = dict(encoder='lf-ques-im-hist', decoder='disc', useHistory=True, concatHistory=True)
    mn = dict(encoder='mn-att-ques-im-hist', decoder='disc', useHistory=True, concatHistory=False)
    args = lambda **kw: argparse.Namespace(**dict(dict(rollout=1, optionCache=0, perplexity=0, host='native', rolloutHistory='concat',
                                                       rolloutEncoder='full'), **kw))
    for host in ('native', 'python'):
        evaluate.check_rollout(args(host=host), lf)
    evaluate.check_rollout(args(), dict(lf, decoder='gen'))
    evaluate.check_rollout(args(), dict(lf, encoder='lf-ques-im', useHistory=False))           # no history: ignored, like the other rollout flags
    evaluate.check_rollout(args(rolloutHistory='row'), mn)
    evaluate.check_rollout(argparse.Namespace(rollout=1, optionCache=0, perplexity=0, host='native'), mn)   # a Namespace without the attribute
    with pytest.raises(SystemExit) as e:                                                        # `row` with a concatHistory model, as ever
        evaluate.check_rollout(args(rolloutHistory='row'), lf)
    assert all(w in str(e.value) for w in ('-rollout 1', 'lf-ques-im-hist', 'concatHistory', '-rolloutHistory concat'))
    with pytest.raises(SystemExit) as e:
        evaluate.check_rollout(argparse.Namespace(rollout=1, optionCache=0, perplexity=0, host='native'), lf)
    assert 'concatHistory' in str(e.value) and '-rolloutHistory concat' in str(e.value)
    with pytest.raises(SystemExit) as e:                                                        # `concat` with a per-round model, by name
        evaluate.check_rollout(args(), mn)
    assert '-rolloutHistory concat' in str(e.value) and 'mn-att-ques-im-hist' in str(e.value)
    with pytest.raises(SystemExit, match='-host native'):
        evaluate.check_rollout(args(host='python'), dict(lf, decoder='gen'))
    evaluate.check_rollout(args(rolloutEncoder='round'), lf)                                    # the round pass continues from a carried state


# ------------------------------------------------------------------------------------------------------------ 5. the switch
class Stop(Exception):
    pass


def test_the_thirteenth_switch_reaches_the_library_and_the_environment_comes_back(monkeypatch):
    from visdial_amd import native
    params = _tiny_val()[0]
    assert len(native.SWITCHES) == 13 and native.SWITCHES[-1][:2] == ('rolloutConcatEnd', 'VD_ROLLOUT_CONCAT_END')
    seen = []

    def fake_call(name, *args):
        assert name == 'vd_model_create'
        seen.append(os.environ.get('VD_ROLLOUT_CONCAT_END'))
        raise Stop()
    monkeypatch.setattr(native, 'call', fake_call)
    for before in (None, 'before'):
        if before is None:
            monkeypatch.delenv('VD_ROLLOUT_CONCAT_END', raising=False)
        else:
            monkeypatch.setenv('VD_ROLLOUT_CONCAT_END', before)
        for p, want in ((dict(params), None), (dict(params, rolloutConcatEnd=51), '51'), (dict(params, rolloutConcatEnd=None), None),
                        (dict(params, rolloutConcatEnd=0), '0'), (dict(params, rolloutConcatEnd='x'), 'x')):       # Python validates nothing
            with pytest.raises(Stop):
                native.NativeModel(p)
            assert seen[-1] == want and os.environ.get('VD_ROLLOUT_CONCAT_END') == before


REFUSALS = [(dec, dict(rolloutConcatEnd=v), "vd_model_create: VD_ROLLOUT_CONCAT_END = '%s' must be an integer >= 0: the <END> token id (0 = off)" % v)
            for dec in ('gen', 'disc') for v in (-1, 'x', '', '5x', 2 ** 40)]
REFUSALS += [('disc', dict(retrieveRollout=1, rolloutConcatEnd=10 ** 6), 'vd_model_create: VD_ROLLOUT_CONCAT_END = 1000000 is no token id: vocabSize is'),
             ('gen', dict(beamRollout=1, rolloutConcatEnd=10 ** 6), 'vd_model_create: VD_ROLLOUT_CONCAT_END = 1000000 is no token id: vocabSize is'),
             ('disc', dict(retrieveRollout=1, rolloutConcatEnd=3, encoder='mn-ques-im-hist'),
              "vd_model_create: VD_ROLLOUT_CONCAT_END = 3 with encoder 'mn-ques-im-hist': its history is one row per round")]


@pytest.mark.parametrize("decoder, knobs, fragment", REFUSALS, ids=['%s-%s' % (d, '-'.join('%s=%s' % kv for kv in k.items())) for d, k, _ in REFUSALS])
def test_refusals_of_the_switch(decoder, knobs, fragment):
    from visdial_amd import _lib
    from visdial_amd.native import NativeModel
    params = dict(_tiny_val()[0], encoder='lf-ques-im-hist')
    before = os.environ.get('VD_ROLLOUT_CONCAT_END')
    with pytest.raises(_lib.VisdialHipError) as e:
        NativeModel(dict(params, decoder=decoder, **knobs))
    assert fragment in str(e.value)
    assert os.environ.get('VD_ROLLOUT_CONCAT_END') == before


def test_where_the_switch_is_ignored():
    """without a device the create fails at its first allocation, not naming the variable; on a device it succeeds"""
    from visdial_amd import _lib
    from visdial_amd.native import NativeModel
    params = dict(_tiny_val()[0], encoder='lf-ques-im-hist')
    for knobs in (dict(decoder='disc', rolloutConcatEnd=10 ** 6),                                        # nothing rolls out
                  dict(decoder='gen', rolloutConcatEnd=10 ** 6, rolloutEncoder='round'),
                  dict(decoder='disc', retrieveRollout=1, rolloutConcatEnd=10 ** 6, encoder='lf-ques-im'),   # no history
                  dict(decoder='disc', retrieveRollout=1, rolloutConcatEnd=3, rolloutEncoder='round'),   # with the round pass
                  dict(decoder='disc', retrieveRollout=1, rolloutConcatEnd=int(params['vocabSize']))):
        try:
            NativeModel(dict(params, **knobs)).close()
        except _lib.VisdialHipError as e:
            assert 'VD_ROLLOUT_CONCAT_END' not in str(e), str(e)


# ------------------------------------------------------------------------------------------------------------ 6. surface and documents
def test_the_c_surface_is_where_it_was_and_the_rule_is_written_down():
    from visdial_amd import _lib, ops
    read = lambda *parts: open(os.path.join(ROOT, *parts)).read()
    header = read('include', 'visdial_hip.h')
    assert re.search(r'^#define\s+VD_ABI_VERSION\s+2\s*$', header, re.M) and _lib.ABI_VERSION == 2
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    names = set(re.findall(r'\b(vd_[a-z0-9_]+)\s*\(', code))
    assert len(names) == 101 and names == set(_lib.PROTOTYPES)
    assert re.search(r'^#define\s+VD_FLAG_HOLD\s+128\s*$', header, re.M) and ops.FLAG_HOLD == 128
    assert 'static const int VD_FLAG_HOLD = 128;' in read('lua', 'visdial_ffi.lua')
    for text in (header, read('visdial_amd', 'csrc', 'rt_switches.h'), read('INTEGRATION.md'), read('README.md'), read('visdial_amd', 'native.py'),
                 read('DESIGN.md')):
        assert 'VD_ROLLOUT_CONCAT_END' in text
    beam = read('visdial_amd', 'csrc', 'beam.hip')
    assert beam.count('rollout_write_row(') == 3 and beam.count('rollout_concat_row(') == 3
    for rule in ('CH1.', 'CH2.', 'CH3.', 'CH4.', 'CH5.', 'CH6.'):
        assert re.search(r'^//\s+' + re.escape(rule), beam, re.M), rule
        assert re.search(r'^#\s+' + re.escape(rule), read('visdial_amd', 'split_eval.py'), re.M), rule
    assert beam.index('//  R6.') < beam.index('//  E1.') < beam.index('//  E5.') < beam.index('//  CH1.') < beam.index('#include "common.h"')
    assert '-rolloutHistory' in read('README.md') and 'EpiLstmFwdHold' in read('visdial_amd', 'csrc', 'lstm.hip')
    assert 'history_round_concat' in read('visdial_amd', 'csrc', 'rt_encoders.h') and 'rnd.carry.' in read('visdial_amd', 'csrc', 'rt_encoders.h')
    for fn in (split_eval.rollout_concat_row, split_eval.rollout_concat_new, split_eval.rollout_concat_len):
        assert fn.__doc__
