"""Ranking on a rollout on the device (VD_RETRIEVE_ROLLOUT = 1; csrc/beam.hip E1-E5): vd_model_retrieve ranking every round on a history of the
model's own picks, against the host loop (split_eval.retrieve_rollout_batch: one upload and one retrieval per round) on a model created
WITHOUT the variable, against ONE plain retrieval of such a model on the history rebuilt from the picks (the fixed point: it holds E5 and
the full-width layout), at the edges of E2 - E4, with the switch off, composed with the beam-search rollout for decoder gen, and through
evaluate.py -rollout 1 on both hosts.

Sizes: the committed prepro fixture's 4 `val` dialogs (3 `test` dialogs, rounds missing), R = 10, O = 100, To = 6, Th = 14, V = 51, hidden 32,
embedding 16, in chunks of 3 + 1 dialogs (the upload de-duplicates there: 120 distinct answers); the attention encoder on the synthetic
loader at the same sizes (no repeats: the plain path).

The synthetic loader's answers DO repeat at V = 51 (its one-word answers: 3 295 distinct rows of 4 000, so those chunks de-duplicate too);
the plain upload path -- the pick reads the candidate's own row -- runs in a fourth case, the same sizes at V = 1001.

Scores are held to rel-L2 < 1e-4, the tolerance of the cross-host disc retrieval tests (test_native_gpu.py, test_model_gpu.py).  The picks are
compared exactly, which is only fair if rounding does not decide them: every case prints the smallest gap in the host loop between a
round's best score and the best score of a candidate with DIFFERENT tokens and asserts that it is >= 100 x that tolerance.  The tolerance
is relative to the L2 norm of the scores, i.e. it allows a root-mean-square deviation of 1e-4 x rms(scores) per score, so the gap is
held to 100 x 1e-4 x rms(scores) (at initialisation the scores are small, rms 0.02 - 0.15: no seed reaches an absolute 1e-2).  The weights are
oracle.init_params(seed), the seed chosen per setting on the CPU from the numpy oracle's fp64 scores of the same rollouts.  Smallest gaps
there, in units of 1e-4 x rms(scores): hre-ques-im-hist seed 6: 799; mn-ques-im-hist seed 11: 392; mn-att-ques-im-hist seed 10: 347 (V = 51), 279
(V = 1001); the edges (mn-ques-im-hist, seed 11): identical candidates 405, empty candidates 407, Th = Tq 1608, test split 1740.
On the device the host loop's fp32 gaps came out the same (799, 392, 347, 279; 405, 407, 1608, 1740), and in every case the device
rollout's scores were bit-identical to the host loop's and to the plain retrieval's on the rebuilt history (rel-L2 0); 36 of the 40
history rows (all 36 generated ones) differed from the ground truth's.
GAPS below has the search."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import visdial_oracle as vo
from test_model_gpu import rel
from test_rollout_cpu import prepro_loader
from visdial_amd.opts import default_params, derive
from visdial_amd.split_eval import SplitEval, rollout_candidate_row, rollout_history_row, rollout_pick, rollout_picked_history

pytestmark = pytest.mark.gpu

TOL = 1e-4                     # rel-L2 of scores, as the cross-host disc retrieval tests hold
MIN_GAP = 100 * TOL
# the weights of a case are oracle.init_params(seed): seeds found on the CPU by GAPS() below
SEEDS = {'hre-ques-im-hist': 6, 'mn-ques-im-hist': 11, 'mn-att-ques-im-hist': 10, 'gen': 1}
CASES = [('hre-ques-im-hist', 'prepro'), ('mn-ques-im-hist', 'prepro'), ('mn-att-ques-im-hist', 'synthetic'),
         ('mn-att-ques-im-hist', 'synthetic-wide')]
KEYS = ('ques_fwd', 'hist', 'img_feat', 'options', 'answer_ind')


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def setting(enc, source='prepro', split='val', decoder='disc'):
    """(params, dataloader, the batch of every dialog of the split with the history at its untrimmed width)"""
    if source.startswith('synthetic'):
        from visdial_amd.dataloader import SyntheticDataloader
        p = derive(default_params(encoder=enc, decoder=decoder, vocabSize=1001 if source == 'synthetic-wide' else 51, embedSize=16, rnnHiddenSize=32, imgFeatureSize=16,
                                  imgSpatialSize=2, commonEmbeddingSize=32, numLayers=2, maxQuesCount=10, maxQuesLen=8, maxAnsLen=6,
                                  maxHistoryLenPerRound=14, batchSize=4, gpuid=0))
        dl = SyntheticDataloader(p, seed=3)
        batch = dl.getTrainBatch(p)
        assert batch['hist'].shape == (4, 10, 14) and batch['options'].shape == (40, 100, 6)
        return p, dl, {k: np.ascontiguousarray(batch[k]) for k in KEYS}
    p, dl = prepro_loader((split,), enc)
    p = dict(p, decoder=decoder, numOptions=dl.numOptions, batchSize=dl.numThreads[split])
    host = SplitEval()
    host.params = p
    batch, _ = host._test_batch(dl, 1, split, 1)
    batch.pop('hist_gt', None)
    assert 'hist' not in batch or batch['hist'].shape[1:] == (10, 14)
    return p, dl, batch


def weights(p, seed=None):
    seed = seed or SEEDS.get('gen' if p['decoder'] == 'gen' else p['encoder'], 1)       # (1: nothing is picked exactly there)
    return {k: np.asarray(v, np.float32) for k, v in vo.init_params(p['encoder'], p['decoder'], p, seed=seed).items()}


def native(p, seed=None, **kw):
    from visdial_amd.native import NativeModel
    m = NativeModel(dict(p, **kw))
    m.set_parameters_dict(weights(p, seed))
    m.training(False)
    return m


def chunk(batch, lo, hi):
    """dialogs [lo, hi) of a batch, as copies (the host loop rewrites its batch's history)"""
    B, R = batch['ques_fwd'].shape[:2]                                     # a field is per dialog [B ...] or per round [B * R ...]
    return {k: np.array(v[lo:hi] if v.shape[0] == B else v[lo * R:hi * R]) for k, v in batch.items() if k != 'num_rounds'}


def host_loop(model, batch, chunks):
    """split_eval.retrieve_rollout_batch on a model without the variable, chunk by chunk: (all ranks [N x O], round r's scores from pass r
    [N x O], the history it generated, the number of retrievals it made per chunk).  The chunks are the device rollout's: a batch of
    another size may run other kernels, and the ranks of two candidates that lie within rounding of each other would follow."""
    R = batch['ques_fwd'].shape[1]
    ranks, scores, hist, calls = [], [], [], []
    for lo, hi in chunks:
        work = chunk(batch, lo, hi)
        N, O = work['options'].shape[:2]
        passes = []
        orig = model.retrieveBatch

        def spy(b, useGt=None):
            out = orig(b, useGt)
            passes.append(model.scores(N, O))
            return out
        model.retrieveBatch = spy
        try:
            ranks.append(np.asarray(SplitEval.retrieve_rollout_batch(model, work)))
        finally:
            del model.retrieveBatch
        sc = np.empty((N, O), np.float32)
        for r in range(len(passes)):
            sc[r::R] = passes[r][r::R]
        scores.append(sc)
        hist.append(work['hist'])
        calls.append(len(passes))
    return np.concatenate(ranks), np.concatenate(scores), np.concatenate(hist), calls


def plain_retrieval(model, batch, chunks):
    """(all ranks, scores) of ordinary retrievals, in the same chunks"""
    ranks, scores = [], []
    for lo, hi in chunks:
        part = chunk(batch, lo, hi)
        ranks.append(np.asarray(model.retrieveBatch(part, useGt=False)))
        scores.append(model.scores(*part['options'].shape[:2]))
    return np.concatenate(ranks), np.concatenate(scores)


def device_rollout(model, batch, chunks):
    """(all ranks, scores, per chunk (rows the option LSTM ran, candidates))"""
    ranks, scores, rows = [], [], []
    for lo, hi in chunks:
        part = chunk(batch, lo, hi)
        before = np.array(part['hist'])
        ranks.append(np.asarray(model.retrieve_rollout_batch(part)))
        assert np.array_equal(part['hist'], before)                       # one upload: the host's batch is not what is rewritten
        scores.append(model.scores(*part['options'].shape[:2]))
        rows.append(model.option_rows())
    return np.concatenate(ranks), np.concatenate(scores), rows


def smallest_gap(scores, options):
    """over the rounds: the best score minus the best score of a candidate whose tokens differ from the best candidate's"""
    gap = np.inf
    for s, opts in zip(scores, options):
        best = int(np.argmax(s))
        other = (opts != opts[best]).any(1)
        if other.any():
            gap = min(gap, float(s[best] - s[other].max()))
    return gap


def picks_of(ranks):
    return np.array([rollout_pick(row) for row in ranks])


def trimmed(hist):
    """a right-aligned history at the width getIndexData would keep"""
    width = max(1, int((hist != 0).sum(2).max()))
    assert not hist[:, :, :hist.shape[2] - width].any()
    return np.ascontiguousarray(hist[:, :, hist.shape[2] - width:])


def rms(x):
    return float(np.sqrt(np.mean(np.square(np.asarray(x, np.float64)))))


def same(dev, host, options, what):
    gap = smallest_gap(host[1], options)
    print('%s: %d rounds, smallest gap to a different answer %.4g = %.0f x TOL x rms(scores) (rms %.4g), ranks equal: %s, score rel-L2 %.3g, '
          'max |difference| %.3g' % (what, len(host[0]), gap, gap / (TOL * rms(host[1])), rms(host[1]), np.array_equal(dev[0], host[0]),
                                     rel(dev[1], host[1]), np.abs(dev[1] - host[1]).max()))
    assert gap >= MIN_GAP * rms(host[1]), what
    assert np.array_equal(picks_of(dev[0]), picks_of(host[0])), what
    assert np.array_equal(dev[0], host[0]), what
    assert rel(dev[1], host[1]) < TOL, what


_CACHE = {}
CHUNKS = [(0, 3), (3, 4)]


def rollouts(case):
    """the host loop on a model created WITHOUT the variable and the device rollout in chunks of 3 + 1, once per case"""
    if case not in _CACHE:
        p, dl, batch = setting(*case)
        plain, roll = native(p), native(p, retrieveRollout=1)
        host = host_loop(plain, batch, CHUNKS)
        dev = device_rollout(roll, batch, CHUNKS)
        roll.forwardBackward(None, onlyForward=True)                      # the slot of the last chunk once more, no upload
        dev += (roll.scores(10, 100),)
        _CACHE[case] = (p, batch, plain, roll, host, dev)
    return _CACHE[case]


@pytest.mark.parametrize("case", CASES)
def test_device_rollout_equals_the_host_loop(gpu, case):
    p, batch, plain, roll, host, dev = rollouts(case)
    assert host[3] == [10, 10] and dev[0].shape == (40, 100) and dev[1].shape == (40, 100)
    same(dev, host, batch['options'], '%s (%s)' % case)
    # which upload path the chunks took: the fixture's answers repeat (de-duplicated: opt_uid), and so do the synthetic loader's at V = 51
    # (its one-word answers); at V = 1001 they do not, and the pick reads the candidate's own row
    print('option rows run / candidates per chunk: %s' % (dev[2],))
    assert all(ex == tot for ex, tot in dev[2]) if case[1] == 'synthetic-wide' else all(ex < 0.95 * tot for ex, tot in dev[2])
    # the history the host loop generated is the picks' rows (E4), and it is the device's too: the slot still holds it, so a forward
    # pass on the slot of the last chunk (no upload) scores it as an ordinary batch
    assert np.array_equal(host[2], rollout_picked_history(batch, picks_of(dev[0])))
    assert rel(dev[3], dev[1][30:]) < TOL and np.array_equal(vo.compute_ranks(dev[3]), dev[0][30:])


@pytest.mark.parametrize("case", CASES)
def test_one_plain_retrieval_on_the_generated_history_returns_the_rollout(gpu, case):
    """the fixed point: an ordinary batch at the trimmed width, a model without the variable, every round at once"""
    p, batch, plain, roll, host, dev = rollouts(case)
    hist = rollout_picked_history(batch, picks_of(dev[0]))
    changed = int((hist != batch['hist']).any(2).sum())
    print('%s (%s): %d of %d history rows differ from the ground truth\'s' % (case + (changed, hist.shape[0] * hist.shape[1])))
    assert changed >= 1
    ranks, scores = plain_retrieval(plain, dict(batch, hist=trimmed(hist)), CHUNKS)
    print('score rel-L2 %.3g' % rel(scores, dev[1]))
    assert np.array_equal(ranks, dev[0]) and rel(scores, dev[1]) < TOL
    # and the ground-truth ranks a retrieve() would report are those of the all ranks
    gt = plain.retrieveBatch(chunk(dict(batch, hist=trimmed(hist)), 0, 3), useGt=True)
    assert np.array_equal(gt, dev[0][np.arange(30), batch['answer_ind'][:30] - 1])


EDGES = {'identical candidates': 11, 'empty candidates': 11, 'Th = Tq': 11, 'test split': 11}      # edge -> seed (GAPS)
EDGE_ROUNDS = (2, 13, 27)


def edge_setting(edge):
    enc = 'mn-ques-im-hist'
    p, dl, batch = setting(enc, split='test' if edge == 'test split' else 'val')
    if edge == 'identical candidates':                                  # E2: every score of the round is equal -> pick 0
        for n in EDGE_ROUNDS:
            batch['options'][n] = batch['options'][n, 7]
    elif edge == 'empty candidates':                                    # E3: no words -> the next row is the question alone
        for n in EDGE_ROUNDS:
            batch['options'][n] = 0
    elif edge == 'Th = Tq':                                             # E4: the answer is what is cut
        batch['hist'] = np.ascontiguousarray(batch['hist'][:, :, -batch['ques_fwd'].shape[2]:])
        assert batch['hist'].shape[2] == batch['ques_fwd'].shape[2] == 8
    else:
        assert 'answer_ind' not in batch and batch['ques_fwd'].shape[0] == 3
    return p, batch, EDGES[edge]


@pytest.mark.parametrize("edge", sorted(EDGES))
def test_the_edges_of_the_rule_on_the_device(gpu, edge):
    p, batch, seed = edge_setting(edge)
    R = 10
    B = batch['ques_fwd'].shape[0]
    plain, roll = native(p, seed), native(p, seed, retrieveRollout=1)
    chunks = [(0, B - 1), (B - 1, B)]
    host = host_loop(plain, batch, chunks)
    dev = device_rollout(roll, batch, chunks)
    same(dev, host, batch['options'], edge)
    hist = rollout_picked_history(batch, picks_of(dev[0]))
    assert np.array_equal(host[2], hist)
    lq = (batch['ques_fwd'] != 0).sum(2).reshape(-1)
    la = np.array([len(rollout_candidate_row(batch['options'][n, k])) - 2 for n, k in enumerate(picks_of(dev[0]))])
    Th = batch['hist'].shape[2]
    if edge == 'identical candidates':
        for n in EDGE_ROUNDS:
            assert np.array_equal(dev[0][n], np.arange(1, 101)) and np.array_equal(dev[1][n], np.full(100, dev[1][n, 0]))
    elif edge == 'empty candidates':
        for n in EDGE_ROUNDS:
            assert np.array_equal(hist[n // R, n % R + 1], rollout_history_row(batch['ques_fwd'][n // R, n % R], [0], Th, 0))
            assert (hist[n // R, n % R + 1] != 0).sum() == lq[n]
    elif edge == 'Th = Tq':
        cut = la > Th - lq
        print('%d of %d picked answers are cut' % (cut.sum(), len(cut)))
        assert cut.sum() >= 10 and ((hist != 0).sum(2) <= Th).all()
    else:                                                               # rounds missing: lq = 0; all 100 candidates are one answer
        zero = int((~hist.any(2)).sum())
        print('%d question rows with lq = 0, %d all-zero history rows' % ((lq == 0).sum(), zero))
        assert (lq == 0).sum() >= 10
        assert zero == sum(int(lq[n] == 0 and la[n] == 0) for n in range(B * R) if n % R != R - 1)
    # the slot holds exactly that history: ONE plain retrieval on it returns the rollout
    ranks, scores = plain_retrieval(plain, dict(batch, hist=trimmed(hist)), chunks)
    assert np.array_equal(ranks, dev[0]) and rel(scores, dev[1]) < TOL
    plain.close()
    roll.close()


def test_off_is_off(gpu):
    from visdial_amd import _lib
    from visdial_amd.native import NativeModel
    case = CASES[1]
    p, batch, plain, roll, host, dev = rollouts(case)
    # unset and 0: the retrieval on the uploaded history, as the oracle computes it; the slot's history stays as uploaded
    ranks = plain.retrieveBatch(batch, useGt=False)
    unset = plain.scores(40, 100)
    P = {k: v.astype(np.float64) for k, v in weights(p).items()}
    assert rel(unset, vo.retrieve(p['encoder'], 'disc', P, p, batch)) < TOL
    assert np.array_equal(ranks, vo.compute_ranks(unset)) and not np.array_equal(ranks, dev[0])
    loss = plain.forwardBackward(None, onlyForward=True)               # the same slot, no upload
    assert np.array_equal(plain.scores(40, 100), unset) and np.isfinite(loss)
    zero = native(p, retrieveRollout=0)
    assert np.array_equal(zero.retrieveBatch(batch, useGt=False), ranks) and np.array_equal(zero.scores(40, 100), unset)
    assert np.array_equal(zero.retrieve_rollout_batch(chunk(batch, 0, 3)), host[0][:30])     # the host loop, on this host too
    zero.close()
    # vd_model_forward_backward of a rollout model is the plain step on the uploaded history (rows >= 1 at full width: exact)
    l0, l1 = plain.forwardBackward(batch, onlyForward=True), roll.forwardBackward(batch, onlyForward=True)
    assert abs(l0 - l1) < 1e-5 and rel(roll.scores(40, 100), unset) < TOL
    # an encoder without a history: the variable is accepted and nothing depends on an answer
    q, _, nohist = setting('lf-ques-im')
    assert 'hist' not in nohist
    a, b = native(q), native(q, retrieveRollout=1)
    assert np.array_equal(a.retrieveBatch(nohist, useGt=False), b.retrieve_rollout_batch(nohist))
    assert np.array_equal(a.scores(40, 100), b.scores(40, 100))
    a.close()
    b.close()
    # what is refused, by name
    roll.training(True)
    with pytest.raises(_lib.VisdialHipError, match='VD_RETRIEVE_ROLLOUT'):
        roll.retrieveBatch(batch, useGt=False)
    roll.training(False)
    with pytest.raises(_lib.VisdialHipError, match='VD_RETRIEVE_ROLLOUT'):
        NativeModel(dict(p, retrieveRollout=2))
    with pytest.raises(_lib.VisdialHipError, match='VD_OPTION_CACHE'):
        NativeModel(dict(p, retrieveRollout=1, optionCache=1))
    NativeModel(dict(p, decoder='gen', retrieveRollout=7)).close()    # ignored for gen
    with pytest.raises(_lib.VisdialHipError, match='VD_RETRIEVE_ROLLOUT'):   # a history row has to hold a question
        roll.upload(dict(batch, hist=np.ascontiguousarray(batch['hist'][:, :, -4:])))


@pytest.mark.parametrize("fused", [0, 1])
def test_gen_composition_equals_a_plain_retrieval_on_the_generated_history(gpu, fused):
    """encode + beam search (k = 3, L = 6, beamRollout = 1) + retrieve on ONE slot = a plain model's retrieve on the history rebuilt from
    the answers the search returned"""
    p, dl, batch = setting('hre-ques-im-hist', decoder='gen')
    START, END = dl.word2ind['<START>'], dl.word2ind['<END>']
    p = dict(p, fusedLhood=fused)
    roll = native(p, beamRollout=1, rolloutBeam=dict(beamSize=3, beamLen=6, startToken=START, endToken=END))
    plain = native(p)
    ranks = np.asarray(roll.retrieve_rollout_batch(batch))
    scores = roll.scores(40, 100)
    tokens = roll._rollout_answers[0]
    assert tokens.shape == (40, 6) and (tokens[:, 0] == START).all()
    hist = roll.rollout_history(batch, ranks)
    for i in range(4):
        for r in range(9):
            assert np.array_equal(hist[i, r + 1], rollout_history_row(batch['ques_fwd'][i, r], tokens[i * 10 + r], 14, END))
    changed = int((hist != batch['hist']).any(2).sum())
    print('fusedLhood %d: %d of 40 history rows differ from the ground truth\'s' % (fused, changed))
    assert changed >= 1
    want = plain.retrieveBatch(dict(batch, hist=trimmed(hist)), useGt=False)
    print('score rel-L2 %.3g' % rel(scores, plain.scores(40, 100)))
    assert np.array_equal(ranks, want) and rel(scores, plain.scores(40, 100)) < TOL
    assert not np.array_equal(ranks, plain.retrieveBatch(batch, useGt=False))      # and it is not the ground-truth history's ranking
    roll.close()
    plain.close()


def test_evaluate_py_writes_the_same_records_on_both_hosts(gpu, tmp_path, capsys):
    import evaluate
    from test_rollout_cpu import PRE
    p, dl, batch = setting('mn-ques-im-hist')
    model = native(p)
    ckpt = str(tmp_path / 'disc.pt')
    torch.save({'modelW': model.wrapperW.clone().cpu(),
                'modelParams': {k: v for k, v in p.items() if isinstance(v, (int, float, str, bool))}}, ckpt)
    model.close()
    data = ['-inputQues', os.path.join(PRE, 'visdial_data.h5'), '-inputImg', os.path.join(PRE, 'data_img.h5'),
            '-inputJson', os.path.join(PRE, 'visdial_params.json')]
    records, lines = {}, {}
    for host, rollout in (('native', 1), ('python', 1), ('native', 0)):
        out = str(tmp_path / ('%s%d.json' % (host, rollout)))
        evaluate.main(['-loadPath', ckpt, '-batchSize', '3', '-split', 'val', '-host', host, '-rollout', str(rollout), '-saveRanks', '1',
                       '-saveRankPath', out] + data)
        records[host, rollout] = json.load(open(out))
        lines[host, rollout] = capsys.readouterr().out.splitlines()
    assert len(records['native', 1]) == 40 and records['native', 1] == records['python', 1]
    assert records['native', 1] != records['native', 0]
    metrics = lambda ls: [l for l in ls if l.startswith('\t')]
    assert len(metrics(lines['native', 1])) == 7 and metrics(lines['native', 1]) == metrics(lines['python', 1])
    told = [l for l in lines['native', 1] if l.startswith('rollout:')]
    assert told == [l for l in lines['python', 1] if l.startswith('rollout:')] and len(told) == 1
    differ, rows = int(told[0].split()[1]), int(told[0].split()[3])
    assert rows == 40 and 1 <= differ <= 36
    assert not [l for l in lines['native', 0] if l.startswith('rollout:')]


# The search behind SEED, on the CPU (import this module and call GAPS()): the numpy oracle as the host of the host loop.
class OracleHost(SplitEval):
    def __init__(self, p, seed):
        self.params = dict(p)
        self.P = vo.init_params(p['encoder'], p['decoder'], p, seed=seed)
        self.passes = []

    def retrieveBatch(self, batch):
        s = vo.retrieve(self.params['encoder'], 'disc', self.P, self.params, batch)
        self.passes.append(s)
        return vo.compute_ranks(s)


def GAPS(seeds=range(1, 9)):
    """per seed and setting: the smallest gap of the oracle's host loop in units of TOL x rms(scores); a seed serves where it is >= 100"""
    settings = [('%s (%s)' % c, ) + setting(*c)[::2] for c in CASES] + [(e, ) + edge_setting(e)[:2] for e in sorted(EDGES)]
    for seed in seeds:
        row = []
        for name, p, batch in settings:
            B = batch['ques_fwd'].shape[0]
            host = OracleHost(p, seed)
            host.retrieve_rollout_batch(chunk(batch, 0, B))
            scores = np.empty((B * 10, 100))
            for r in range(10):
                scores[r::10] = host.passes[r][r::10]
            row.append('%s %.0f' % (name, smallest_gap(scores, batch['options']) / (TOL * rms(scores))))
        print('seed %d: %s' % (seed, '  '.join(row)), flush=True)
