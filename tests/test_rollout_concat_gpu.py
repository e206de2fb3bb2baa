"""Rollouts on a CONCATENATED history on the device (VD_ROLLOUT_CONCAT_END; csrc/beam.hip CH1-CH6) and VD_FLAG_HOLD of vd_lstm_forward.

1. VD_FLAG_HOLD through ops.lstm_forward: against an fp64 restatement at the bound test_ops_gpu.test_lstm_forward_backward holds the plain
   call to (rel-L2 1e-5 on h and c); a row without a live step returns (h0, c0) bit for bit; the plain maskZero call over [prefix ; new
   tokens] against the plain call on the prefix followed by HOLD on the new window (CH6 on the device); the refusals.  N = 5 and 33 run the
   distributed split-K epilogue, N = 2049 the register-staged generic kernel (a HOLD pass never takes the LDS-DMA pipeline).
   Measured on the device: rel-L2 against fp64 2.8e-8 - 4.7e-8 (h), 2.5e-8 - 3.7e-8 (c) over the five shapes; the continuation against
   the one full-width call: bit-identical final state (test_hold_continues_the_plain_recurrence).
2. The device rollout of decoder disc (VD_RETRIEVE_ROLLOUT = 1 with the <END> id set) against the host loop
   (split_eval.retrieve_rollout_batch with params rolloutHistory = 'concat') on a model created without either variable, by the method of
   test_eval_rollout_gpu.py: ranks and generated history exact, scores rel-L2 < 1e-4, the host loop's smallest gap between a round's best
   score and the best differently-worded candidate printed and held to >= 100 x 1e-4 x rms(scores).  lf-ques-im-hist and lf-ques-hist on
   the prepro `val` fixture (4 dialogs in chunks of 3 + 1, R = 10, O = 100, To = 6, W = 140, V = 51, H = 32, E = 16), lf-att-ques-im-hist on
   the synthetic loader at the sizes of test_eval_rollout_gpu.setting (its concatenated width: 203); the cut: the prepro batch with the
   history sliced to its last 40 columns (rows cut and repeat from about round 3).  Weights: oracle.init_params(seed), the seed found per
   case on the CPU from the numpy oracle's fp64 scores (GAPS below).  Smallest gaps there, in units of 1e-4 x rms(scores):
   lf-ques-im-hist seed 1: 143; lf-ques-hist seed 1: 330; lf-att-ques-im-hist seed 3: 572; the cut (lf-ques-im-hist, W = 40) seed 7: 236.
3. The fixed point: ONE plain retrieval of a model created without the switch on the generated history returns the rollout.
4. Decoder gen: VD_BEAM_ROLLOUT = 1 with the <END> id set, k = 3, beamLen = 6, against rollout_dialog with the concat rule; another end_token is
   refused; evaluate.py -rollout 1 -rolloutHistory concat end to end on a gen and on a disc checkpoint.
5. The switch unset: a model created without the variable computes what it computed, and a concat model is still refused without the flag.

Every disc case runs VD_ROLLOUT_ENCODER = full and = round (rt_encoders.h history_round_concat: the history stack continued from a carried
state over the window of new tokens through VD_FLAG_HOLD); `round` is held to the host loop like `full` and to `full` itself (same ranks
and history, scores at 1e-4), and whether the two are bit-identical is printed: the full pass runs the wavefront's tick kernels, the
continuation the step kernels, so they need not be.
On the device the host loop's fp32 gaps came out as the oracle's (143, 330, 572, 236), `full` was bit-identical to the host loop in all four
cases (rel-L2 0) and to the plain retrieval on the generated history; `round` had the same ranks and history and scores at rel-L2 1.1e-7 -
1.3e-7 of `full` (not bit-identical); the cut case cut 28 of its 36 generated rows; the gen answers of `full`, `round` and the host loop
were equal."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import visdial_oracle as vo
from test_eval_rollout_gpu import (CHUNKS, KEYS, TOL, chunk, device_rollout, host_loop, native, picks_of, plain_retrieval, rms, same,
                                   smallest_gap, trimmed)
from test_model_gpu import rel
from test_rollout_cpu import PRE
from visdial_amd.opts import default_params, derive
from visdial_amd.split_eval import SplitEval, beam_search_round, rollout_concat_row, rollout_picked_history

pytestmark = pytest.mark.gpu

SEEDS = {('lf-ques-im-hist', 'prepro'): 1, ('lf-ques-hist', 'prepro'): 1, ('lf-att-ques-im-hist', 'synthetic'): 3,
         ('lf-ques-im-hist', 'cut'): 7}
CASES = sorted(SEEDS)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------------------ 1. VD_FLAG_HOLD
def hold_ref(xp, Wh, mask, h0, c0):
    """fp64: xp [T x N x 4H] = the input projection, gates i, f, o, g; a row with mask 0 at a step keeps its state"""
    T, N, H4 = xp.shape
    H = H4 // 4
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    h, c = np.array(h0, np.float64), np.array(c0, np.float64)
    hs, cs = [], []
    for t in range(T):
        a = xp[t].astype(np.float64) + h @ Wh.astype(np.float64)
        i, f, o, g = sig(a[:, :H]), sig(a[:, H:2 * H]), sig(a[:, 2 * H:3 * H]), np.tanh(a[:, 3 * H:])
        cn = f * c + i * g
        hn = o * np.tanh(cn)
        live = (mask[t] != 0)[:, None]
        h, c = np.where(live, hn, h), np.where(live, cn, c)
        hs.append(h)
        cs.append(c)
    return np.stack(hs), np.stack(cs)


def hold_inputs(T, N, H, seed):
    rng = np.random.RandomState(seed)
    lens = rng.randint(0, T + 1, size=N)
    lens[:3] = (0, T, 1)                                                 # no live step, every step, the last alone
    mask = (np.arange(T)[:, None] >= T - lens[None, :]).astype(np.int32)  # right-aligned
    xp = rng.randn(T, N, 4 * H).astype(np.float32)
    Wh = (rng.randn(H, 4 * H) / np.sqrt(H)).astype(np.float32)
    h0, c0 = (0.5 * rng.randn(N, H)).astype(np.float32), rng.randn(N, H).astype(np.float32)
    return lens, mask, xp, Wh, h0, c0


def run_lstm(ops, xp, Wh, mask, h0, c0, flags):
    T, N, H4 = xp.shape
    H = H4 // 4
    h = torch.full((T, N, H), 7.0, device="cuda")
    c = torch.full((T, N, H), 7.0, device="cuda")
    gates = None if flags else torch.empty(T, N, 4 * H, device="cuda")
    ops.lstm_forward(dev(xp), dev(Wh), gates, h, c, T, N, H, N * 4 * H, 4 * H, tok_mask=dev(mask), h0=None if h0 is None else dev(h0),
                     c0=None if c0 is None else dev(c0), flags=flags)
    torch.cuda.synchronize()
    return h.cpu().numpy(), c.cpu().numpy()


@pytest.mark.parametrize("N,H", [(5, 32), (33, 32), (5, 64), (33, 64), (2049, 32)])
def test_hold_matches_its_fp64_restatement(gpu, N, H):
    from visdial_amd import ops
    T = 6
    lens, mask, xp, Wh, h0, c0 = hold_inputs(T, N, H, 100 * N + H)
    h, c = run_lstm(ops, xp, Wh, mask, h0, c0, ops.FLAG_HOLD)
    h_ref, c_ref = hold_ref(xp, Wh, mask, h0, c0)
    eh, ec = rel(h, h_ref), rel(c, c_ref)
    print('N = %d H = %d: rel-L2 h %.3g c %.3g' % (N, H, eh, ec))
    assert eh < 1e-5 and ec < 1e-5                                       # test_ops_gpu.test_lstm_forward_backward's bound
    assert rel(h[-1, N - 1], h_ref[-1, N - 1]) < 1e-5                    # the last (ragged) row
    dead = lens == 0
    assert dead.any() and np.array_equal(h[-1, dead], h0[dead]) and np.array_equal(c[-1, dead], c0[dead])   # bit for bit
    for t in range(T):                                                   # and a held row holds (h0, c0) until its first token
        held = mask[:t + 1].sum(0) == 0
        assert np.array_equal(h[t, held], h0[held]) and np.array_equal(c[t, held], c0[held])


@pytest.mark.parametrize("N,H", [(5, 32), (33, 64)])
def test_hold_continues_the_plain_recurrence(gpu, N, H):
    """CH6 on the device: plain maskZero over [prefix ; window] = plain over the prefix, then HOLD over the window from the carried state.
    Measured on the MI355X for both shapes: max |dh| = max |dc| = 0, the final state is bit-identical (the same step kernel, the same
    per-row K order, and the held rows write what they read).  Only the tolerance is asserted."""
    from visdial_amd import ops
    rng = np.random.RandomState(N + H)
    Tp, Tw = 7, 6
    lp, lw = rng.randint(1, Tp + 1, size=N), rng.randint(0, Tw + 1, size=N)
    lw[:2] = (0, Tw)
    Wh = (rng.randn(H, 4 * H) / np.sqrt(H)).astype(np.float32)
    T = Tp + Tw
    full = np.zeros((T, N, 4 * H), np.float32)
    fmask = np.zeros((T, N), np.int32)
    pre, pmask = np.zeros((Tp, N, 4 * H), np.float32), np.zeros((Tp, N), np.int32)
    win, wmask = np.zeros((Tw, N, 4 * H), np.float32), np.zeros((Tw, N), np.int32)
    for n in range(N):                                                   # every layout right-aligned, as the history is
        x = rng.randn(lp[n] + lw[n], 4 * H).astype(np.float32)
        full[T - len(x):, n], fmask[T - len(x):, n] = x, 1
        pre[Tp - lp[n]:, n], pmask[Tp - lp[n]:, n] = x[:lp[n]], 1
        if lw[n]:
            win[Tw - lw[n]:, n], wmask[Tw - lw[n]:, n] = x[lp[n]:], 1
    hf, cf = run_lstm(ops, full, Wh, fmask, None, None, 0)
    hp, cp = run_lstm(ops, pre, Wh, pmask, None, None, 0)
    hw, cw = run_lstm(ops, win, Wh, wmask, hp[-1], cp[-1], ops.FLAG_HOLD)
    dh, dc = np.abs(hw[-1] - hf[-1]).max(), np.abs(cw[-1] - cf[-1]).max()
    print('N = %d H = %d: continuation against the full call, final state: max |dh| %.3g max |dc| %.3g, bit-identical: %s'
          % (N, H, dh, dc, bool(dh == 0 and dc == 0)))
    assert rel(hw[-1], hf[-1]) < 1e-5 and rel(cw[-1], cf[-1]) < 1e-5


def test_hold_refusals(gpu):
    from visdial_amd import _lib, ops
    lens, mask, xp, Wh, h0, c0 = hold_inputs(3, 5, 32, 1)
    h, c, g = torch.empty(3, 5, 32, device="cuda"), torch.empty(3, 5, 32, device="cuda"), torch.empty(3, 5, 128, device="cuda")
    go = lambda flags, gates=None, m=mask: ops.lstm_forward(dev(xp), dev(Wh), gates, h, c, 3, 5, 32, 5 * 128, 128,
                                                           tok_mask=None if m is None else dev(m), h0=dev(h0), c0=dev(c0), flags=flags)
    for other in (ops.FLAG_BF16, ops.FLAG_SPLIT9, ops.FLAG_SPLIT6, ops.FLAG_SPLIT3, ops.FLAG_LIVE_PREFIX, ops.FLAG_STATE_ONLY):
        with pytest.raises(_lib.VisdialHipError, match='VD_FLAG_HOLD'):
            go(ops.FLAG_HOLD | other)
    with pytest.raises(_lib.VisdialHipError, match='VD_FLAG_(HOLD|TREE)'):
        ops.lstm_forward(dev(xp), dev(Wh), None, h, c, 3, 5, 32, 5 * 128, 128, tok_mask=dev(np.concatenate([mask, mask])), h0=dev(h0),
                         c0=dev(c0), flags=ops.FLAG_HOLD | ops.FLAG_TREE)
    with pytest.raises(_lib.VisdialHipError, match='VD_FLAG_HOLD.*gates must be NULL'):
        go(ops.FLAG_HOLD, g)
    with pytest.raises(_lib.VisdialHipError, match='VD_FLAG_HOLD needs tok_mask'):
        go(ops.FLAG_HOLD, None, None)
    go(ops.FLAG_HOLD)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ 2. the device rollout, disc
def concat_loader(enc, splits=('val',)):
    """the committed prepro fixture as evaluate.py loads it for an lf encoder (concatHistory: W = 140)"""
    from visdial_amd.dataloader import Dataloader
    p = derive(default_params(encoder=enc, decoder='disc', embedSize=16, rnnHiddenSize=32, numLayers=2, imgFeatureSize=16, gpuid=0,
                              inputQues=os.path.join(PRE, 'visdial_data.h5'), inputImg=os.path.join(PRE, 'data_img.h5'),
                              inputJson=os.path.join(PRE, 'visdial_params.json')))
    assert p['concatHistory']
    dl = Dataloader(seed=1234).initialize(p, list(splits))
    for k in ('vocabSize', 'maxQuesCount', 'maxQuesLen', 'maxAnsLen', 'numOptions'):
        p[k] = getattr(dl, k)
    return p, dl


def setting(enc, source, decoder='disc'):
    """(params, the batch of every `val` dialog with the concatenated history at its untrimmed width, <START>, <END>)"""
    if source == 'synthetic':
        from visdial_amd.dataloader import SyntheticDataloader
        p = derive(default_params(encoder=enc, decoder=decoder, vocabSize=51, embedSize=16, rnnHiddenSize=32, imgFeatureSize=16, imgSpatialSize=2,
                                  commonEmbeddingSize=32, numLayers=2, maxQuesCount=10, maxQuesLen=8, maxAnsLen=6, maxHistoryLenPerRound=14,
                                  batchSize=4, gpuid=0))
        dl = SyntheticDataloader(p, seed=3)
        batch = dl.getTrainBatch(dict(p, decoder='disc'))
        assert batch['hist'].shape[:2] == (4, 10) and batch['hist'].shape[2] > 140 and batch['options'].shape == (40, 100, 6)
        return p, {k: np.ascontiguousarray(batch[k]) for k in KEYS}, dl.startToken, dl.endToken
    p, dl = concat_loader(enc)
    p = dict(p, decoder=decoder, batchSize=dl.numThreads['val'])
    host = SplitEval()
    host.params = p
    batch, _ = host._test_batch(dl, 1, 'val', 1)
    batch.pop('hist_gt', None)
    assert batch['hist'].shape == (4, 10, 140)
    if source == 'cut':                                                   # row 0 (the caption, <= 14 tokens) fits; the later rows do not
        assert (batch['hist'][:, 0] != 0).sum(1).max() <= 14
        batch['hist'] = np.ascontiguousarray(batch['hist'][:, :, -40:])
    return p, batch, dl.word2ind['<START>'], dl.word2ind['<END>']


def weights(p, seed):
    return {k: np.asarray(v, np.float32) for k, v in vo.init_params(p['encoder'], p['decoder'], p, seed=seed).items()}


_CACHE = {}


def rollouts(case):
    """the host loop on a model created WITHOUT the variables and the device rollout in chunks of 3 + 1, once per case"""
    if case not in _CACHE:
        p, batch, START, END = setting(*case)
        concat = dict(rolloutHistory='concat', rolloutConcatEnd=END)
        plain = native(p, SEEDS[case])
        plain.params.update(concat)                                       # the host loop's rule; the model itself was created without it
        host = host_loop(plain, batch, CHUNKS)
        devr = {}
        for which in ('full', 'round'):
            roll = native(p, SEEDS[case], retrieveRollout=1, rolloutEncoder=which, **concat)
            devr[which] = device_rollout(roll, batch, CHUNKS)
            roll.close()
        _CACHE[case] = (p, batch, END, plain, host, devr['full'], devr['round'])
    return _CACHE[case]


@pytest.mark.parametrize("case", CASES, ids=['%s-%s' % c for c in CASES])
def test_device_rollout_equals_the_host_loop(gpu, case):
    p, batch, END, plain, host, devr, rnd = rollouts(case)
    W = batch['hist'].shape[2]
    assert host[3] == [10, 10] and devr[0].shape == (40, 100) and host[2].shape == (4, 10, W)
    same(devr, host, batch['options'], '%s (%s), W = %d' % (case + (W,)))
    print('scores bit-identical to the host loop\'s: %s' % np.array_equal(devr[1], host[1]))
    # VD_ROLLOUT_ENCODER = round: the later passes continue the history stack from the carried state over the new tokens alone (CH6)
    same(rnd, host, batch['options'], '%s (%s), W = %d, round against the host loop' % (case + (W,)))
    print('round against full: ranks equal: %s, score rel-L2 %.3g, bit-identical: %s'
          % (np.array_equal(rnd[0], devr[0]), rel(rnd[1], devr[1]), np.array_equal(rnd[1], devr[1])))
    assert np.array_equal(rnd[0], devr[0]) and rel(rnd[1], devr[1]) < TOL
    cut = []
    hist = rollout_picked_history(batch, picks_of(devr[0]), True, END, cut)
    assert np.array_equal(host[2], hist)                                  # the history the host loop generated is the device's picks' rows
    lens = (hist != 0).sum(2)
    print('%d of 36 generated rows cut; longest row %d of %d' % (sum(cut), lens.max(), W))
    if case[1] == 'cut':
        assert sum(cut) >= 20 and (lens[:, -1] == W).all() and any(np.array_equal(hist[i, 9], hist[i, 8]) for i in range(4))
    elif case[1] == 'prepro':
        assert sum(cut) == 0
    for i in range(4):                                                    # CH4: every row extends the one before
        for r in range(9):
            n = int(lens[i, r])
            k = int((hist[i, r + 1] != 0).sum()) - n
            assert k >= 0 and (n == 0 or np.array_equal(hist[i, r + 1, W - n - k:W - k], hist[i, r, W - n:]))


@pytest.mark.parametrize("case", CASES, ids=['%s-%s' % c for c in CASES])
def test_one_plain_retrieval_on_the_generated_history_returns_the_rollout(gpu, case):
    """the fixed point: an ordinary batch, a model created without the switch, every round at once"""
    p, batch, END, plain, host, devr, rnd = rollouts(case)
    hist = rollout_picked_history(batch, picks_of(devr[0]), True, END)
    changed = int((hist != batch['hist']).any(2).sum())
    ranks, scores = plain_retrieval(plain, dict(batch, hist=trimmed(hist)), CHUNKS)
    print('%s (%s): %d of 40 history rows differ from the uploaded ones; score rel-L2 %.3g' % (case + (changed, rel(scores, devr[1]))))
    assert changed >= 1
    assert np.array_equal(ranks, devr[0]) and rel(scores, devr[1]) < TOL


def test_the_switch_is_checked_and_the_round_pass_names_what_it_cannot_do(gpu):
    from visdial_amd import _lib
    from visdial_amd.native import NativeModel
    p, batch, END, plain, host, devr, rnd = rollouts(CASES[1])
    deep = native(dict(p, numLayers=3), 1, retrieveRollout=1, rolloutConcatEnd=END, rolloutHistory='concat', rolloutEncoder='round')
    with pytest.raises(_lib.VisdialHipError, match='continues a two-layer history stack; this model has numLayers = 3'):   # no silent fall-back
        deep.retrieve_rollout_batch(chunk(batch, 0, 3))
    deep.close()
    with pytest.raises(_lib.VisdialHipError, match='VD_ROLLOUT_CONCAT_END = 52 is no token id'):
        NativeModel(dict(p, retrieveRollout=1, rolloutConcatEnd=52))
    with pytest.raises(_lib.VisdialHipError, match="VD_ROLLOUT_CONCAT_END = 51 with encoder 'mn-ques-im-hist'"):
        NativeModel(dict(p, encoder='mn-ques-im-hist', retrieveRollout=1, rolloutConcatEnd=51))
    NativeModel(dict(p, rolloutConcatEnd=52)).close()                     # nothing rolls out: ignored
    NativeModel(dict(p, encoder='lf-ques-im', retrieveRollout=1, rolloutConcatEnd=52)).close()   # no history: ignored


def test_the_switch_unset_is_the_parent(gpu):
    p, batch, END, plain, host, devr, rnd = rollouts(CASES[1])
    keep = dict(plain.params)
    try:
        for k in ('rolloutHistory', 'rolloutConcatEnd'):
            plain.params.pop(k)
        a = plain.retrieveBatch(chunk(batch, 0, 3), useGt=False)
        sa = plain.scores(30, 100)
        b = plain.retrieveBatch(chunk(batch, 0, 3), useGt=False)
        assert np.array_equal(a, b) and np.array_equal(sa, plain.scores(30, 100))     # bit for bit
        P = {k: v.astype(np.float64) for k, v in weights(p, SEEDS[CASES[1]]).items()}
        assert rel(sa, vo.retrieve(p['encoder'], 'disc', P, p, chunk(batch, 0, 3))) < TOL
        plain.params['rollout'] = 1                                       # a concat model is still refused without the flag
        with pytest.raises(ValueError, match='concatHistory'):
            plain._rollout()
        unset = native(p, SEEDS[CASES[1]], retrieveRollout=1)             # the device rollout without the <END> id: not this rule's rows
        with pytest.raises(ValueError, match='rolloutConcatEnd'):
            unset.params.update(rolloutHistory='concat', rolloutConcatEnd=END)
            unset.retrieve_rollout_batch(chunk(batch, 0, 3))
        unset.close()
    finally:
        plain.params.clear()
        plain.params.update(keep)


# ------------------------------------------------------------------------------------------------------------ 4. decoder gen
def test_gen_rollout_equals_the_host_loop(gpu):
    from visdial_amd import _lib
    p, batch, START, END = setting('lf-ques-im-hist', 'prepro', decoder='gen')
    k, L = 3, 6
    plain = native(p, 1)
    roll = native(p, 1, beamRollout=1, rolloutConcatEnd=END, rolloutHistory='concat',
                  rolloutBeam=dict(beamSize=k, beamLen=L, startToken=START, endToken=END))
    gen_keys = ('ques_fwd', 'hist', 'img_feat')
    toks, hist = [], np.array(batch['hist'])

    def search(r):
        plain._gen_begin(np.full(k, r, np.int32))
        return beam_search_round(plain._gen_step, plain._gen_select, k, L, START, END)
    for i in range(4):
        one = {key: np.array(batch[key][i:i + 1]) for key in gen_keys}
        toks += [np.asarray(found[0][0]) for found in plain.rollout_dialog(one, search, END, concat=True)]
        hist[i] = one['hist'][0]
    toks = np.array(toks)
    def device(model):
        out = []
        for lo, hi in CHUNKS:
            model._gen_encode({key: np.array(batch[key][lo:hi]) for key in gen_keys})
            out.append(model._gen_beam(k, L, START, END)[0])
        return np.concatenate(out)
    got = device(roll)
    rnd = native(p, 1, beamRollout=1, rolloutConcatEnd=END, rolloutHistory='concat', rolloutEncoder='round')
    print('round answers equal full\'s: %s' % np.array_equal(device(rnd), got))
    assert np.array_equal(device(rnd), got)
    rnd.close()
    print('answers equal: %s; %d of 40 history rows differ from the ground truth\'s' % (np.array_equal(got, toks),
                                                                                      (hist != batch['hist']).any(2).sum()))
    assert np.array_equal(got, toks)
    for i in range(4):                                                    # the host loop's history is CH1 - CH4 of the device's answers
        for r in range(9):
            assert np.array_equal(hist[i, r + 1], rollout_concat_row(hist[i, r], batch['ques_fwd'][i, r], got[i * 10 + r], END, END))
    # the composition: the candidates ranked on that history = a plain model's retrieval on it
    ranks = np.asarray(roll.retrieve_rollout_batch(batch))
    scores = roll.scores(40, 100)
    assert np.array_equal(roll.rollout_history(batch, ranks), hist)
    want = plain.retrieveBatch(dict(batch, hist=trimmed(hist)), useGt=False)
    print('score rel-L2 %.3g' % rel(scores, plain.scores(40, 100)))
    assert np.array_equal(ranks, want) and rel(scores, plain.scores(40, 100)) < TOL
    roll._gen_encode({key: np.array(batch[key][:3]) for key in gen_keys})
    with pytest.raises(_lib.VisdialHipError, match='end_token = %d.*VD_ROLLOUT_CONCAT_END = %d' % (END - 1, END)):
        roll._gen_beam(k, L, START, END - 1)
    roll.close()
    plain.close()


@pytest.mark.parametrize("decoder", ['disc', 'gen'])
def test_evaluate_py_runs_end_to_end_on_both_hosts(gpu, tmp_path, capsys, decoder):
    import evaluate
    p, batch, START, END = setting('lf-ques-im-hist', 'prepro', decoder=decoder)
    model = native(p, 1)
    ckpt = str(tmp_path / 'model.pt')
    torch.save({'modelW': model.wrapperW.clone().cpu(),
                'modelParams': {k: v for k, v in p.items() if isinstance(v, (int, float, str, bool))}}, ckpt)
    model.close()
    data = ['-inputQues', os.path.join(PRE, 'visdial_data.h5'), '-inputImg', os.path.join(PRE, 'data_img.h5'),
            '-inputJson', os.path.join(PRE, 'visdial_params.json')]
    common = ['-loadPath', ckpt, '-batchSize', '3', '-split', 'val', '-rollout', '1', '-saveRanks', '1', '-beamSize', '3', '-beamLen', '6']
    with pytest.raises(SystemExit, match='-rolloutHistory concat lifts the refusal'):
        evaluate.main(common + ['-host', 'native', '-saveRankPath', str(tmp_path / 'no.json')] + data)
    capsys.readouterr()
    records, lines = {}, {}
    for host in ('native', 'round') if decoder == 'gen' else ('native', 'round', 'python'):   # (a gen rollout is the device's: -host native)
        out = str(tmp_path / ('%s.json' % host))
        how = ['-host', 'native', '-rolloutEncoder', 'round'] if host == 'round' else ['-host', host]
        evaluate.main(common + how + ['-rolloutHistory', 'concat', '-saveRankPath', out] + data)
        records[host] = json.load(open(out))
        lines[host] = capsys.readouterr().out.splitlines()
        told = [l for l in lines[host] if l.startswith('rollout')]
        print(told)
        assert len(records[host]) == 40 and len(told) == 2 and told[1].startswith('rolloutHistory concat: 0 generated history rows were cut')
        assert 1 <= int(told[0].split()[1]) <= 36 and int(told[0].split()[3]) == 40
    assert records['round'] == records['native']
    if decoder == 'disc':
        assert records['native'] == records['python']
        assert [l for l in lines['native'] if l.startswith(('\t', 'rollout'))] == [l for l in lines['python'] if l.startswith(('\t', 'rollout'))]
    else:
        with pytest.raises(SystemExit, match='-host native'):
            evaluate.main(common + ['-host', 'python', '-rolloutHistory', 'concat', '-saveRankPath', str(tmp_path / 'no.json')] + data)


# The search behind SEEDS, on the CPU (import this module and call GAPS()): the numpy oracle as the host of the host loop.
class OracleHost(SplitEval):
    def __init__(self, p, seed, END):
        self.params = dict(p, rolloutHistory='concat', rolloutConcatEnd=END)
        self.P = vo.init_params(p['encoder'], p['decoder'], p, seed=seed)
        self.passes = []

    def retrieveBatch(self, batch):
        s = vo.retrieve(self.params['encoder'], 'disc', self.P, self.params, batch)
        self.passes.append(s)
        return vo.compute_ranks(s)


def GAPS(seeds=range(1, 5), cases=CASES):
    """per seed and case: the smallest gap of the oracle's host loop in units of TOL x rms(scores); a seed serves where it is >= 100"""
    for case in cases:
        p, batch, START, END = setting(*case)
        for seed in seeds:
            host = OracleHost(p, seed, END)
            host.retrieve_rollout_batch(chunk(batch, 0, 4))
            scores = np.empty((40, 100))
            for r in range(10):
                scores[r::10] = host.passes[r][r::10]
            print('%s (%s) seed %d: %.0f' % (case + (seed, smallest_gap(scores, batch['options']) / (TOL * rms(scores)))), flush=True)
