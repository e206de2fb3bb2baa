"""Top-k / nucleus truncation inside the batched device sampler (a NativeModel created with params topK / topP = VD_SAMPLE_TOPK /
VD_SAMPLE_TOPP around vd_model_create; csrc/sample.hip T1-T4) against the host rule split_eval.truncated_weights: pinned logits
(vocabulary projection weight 0, bias = a crafted vector, so every row of every step has exactly those logits), the unchanged path
with the knobs off, determinism, the sampled distribution, the per-dialog loops of both hosts, the refusals and generate.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_sample_gpu import check_records, host_draw, nucleus_margin, replay_margins
from visdial_amd.opts import default_params, derive
from visdial_amd.split_eval import truncated_weights

pytestmark = pytest.mark.gpu
PRE = os.path.join(ROOT, 'tests', 'golden', 'prepro')
TOL = 1e-6                                                     # the margin of tests/test_sample_gpu.py


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


class Dialogs(object):
    """synthetic dialogs behind the getIndexData / word2ind / ind2word surface generateAnswers reads"""

    def __init__(self, p, n, V):
        q = dict(p, batchSize=n)
        from visdial_amd.dataloader import SyntheticDataloader
        self.b = SyntheticDataloader(q, seed=5).getTrainBatch(q)
        self.numThreads = {'val': n}
        self.word2ind = {'<START>': V - 1, '<END>': V}
        self.ind2word = {i: '<START>' if i == V - 1 else '<END>' if i == V else 'w%d' % i for i in range(1, V + 1)}

    def getIndexData(self, inds, params, dtype):
        ix = np.asarray(inds, np.int64) - 1
        return {k: np.ascontiguousarray(self.b[k][ix]) for k in ('ques_fwd', 'hist', 'img_feat') if k in self.b}


def tiny(V, n=2):
    p = derive(default_params(encoder='lf-ques', decoder='gen', vocabSize=V, embedSize=12, rnnHiddenSize=32, numLayers=2, maxQuesCount=10,
                              maxQuesLen=6, maxAnsLen=6, maxHistoryLenPerRound=12, batchSize=n, gpuid=0))
    return p, Dialogs(p, n, V)


def native(p, **knobs):
    from visdial_amd.native import NativeModel
    m = NativeModel(dict(p, **knobs), init_seed=1234)
    m._set_training(False)
    return m


def set_tensor(m, name, a):
    from visdial_amd import _lib
    a = np.ascontiguousarray(a, dtype=np.float32)
    _lib.call("vd_model_set_tensor", m.h, name.encode(), a.ctypes.data, a.size)


# ------------------------------------------------------------------------------------------------------------ pinned logits
def crafted_logits(V):
    """runs of equal logits at the head (2 x 4.0, 3 x 3.0, 6 x 2.0, 9 x 1.0, 20 x 0.0: the top-k and nucleus boundaries of CASES fall
    inside them) and a tail of distinct values below, all at shuffled columns"""
    rng = np.random.RandomState(V)
    head = np.repeat([4.0, 3.0, 2.0, 1.0, 0.0], [2, 3, 6, 9, 20])
    x = np.concatenate([head, rng.uniform(-8.0, -0.5, size=V - head.size)]).astype(np.float32)
    return x[rng.permutation(V)]


def pinned(V, k, p):
    pr, dl = tiny(V)
    m = native(pr, topK=k, topP=p)
    shapes = {n: (r, c) for n, _, r, c in m.tensors}
    set_tensor(m, 'vocab.W', np.zeros(shapes['vocab.W']))
    set_tensor(m, 'vocab.b', crafted_logits(V))
    batch = dl.getIndexData(np.arange(1, 3), pr, 'val')
    m._gen_encode(batch)
    N = batch['ques_fwd'].shape[0] * batch['ques_fwd'].shape[1]
    m._gen_begin(np.arange(N, dtype=np.int32))
    logp = m._gen_step(np.full(N, V - 1, np.int64))              # the device's own fp32 log-probabilities of the pinned logits
    assert all(np.array_equal(logp[0], row) for row in logp)
    m._gen_encode(batch)
    return m, logp[0], N


def uniforms(rng, L, N):
    u = rng.random_sample((L, N))
    u[0, :4] = [0.0, 2.0 ** -53, 1 - 2.0 ** -53, 0.5]
    u[-1, -2:] = [0.0, 1 - 2.0 ** -53]
    return u


#        V   k    p    T
CASES = [(40, 4, 1.0, 1.0),       # k inside the run of 3.0
         (40, 8, 1.0, 0.7),       # ... of 2.0
         (40, 0, 0.5, 1.0),       # the nucleus ends inside the run of 3.0
         (40, 8, 0.9, 1.0),       # ... of 2.0, p taken of the top-8 mass
         (40, 39, 0.999, 1.0),
         (300, 4, 1.0, 1.0),
         (300, 0, 0.5, 1.0),      # inside the run of 3.0
         (300, 8, 0.9, 1.0),
         (300, 6, 0.95, 0.7),     # T < 1 sharpens the weights the nucleus sums; ends between two runs
         (300, 290, 0.97, 1.0),   # both boundaries in the tail, chunks of two columns
         (11322, 40, 0.9, 1.0)]


@pytest.mark.parametrize("V, k, p, T", CASES)
def test_pinned_logits_every_token_lies_in_the_kept_set(gpu, V, k, p, T):
    m, logp, N = pinned(V, k, p)
    margin = nucleus_margin(logp, T, k, p)
    assert margin >= TOL, margin                                # the boundary is nowhere near rounding: no exception needed
    keep = truncated_weights(logp, T, k, p) > 0
    order = np.argsort(-logp, kind='stable')
    n_keep = int(keep.sum())
    assert 1 <= n_keep < V and np.array_equal(np.sort(order[:n_keep]), np.nonzero(keep)[0])
    if V <= 300 and (k, p) not in ((39, 0.999), (290, 0.97), (6, 0.95)):
        assert logp[order[n_keep - 1]] == logp[order[n_keep]]   # the boundary splits a run of equal log-probabilities
    L = 12
    toks, ll = m._gen_sample(L, V - 1, V, T, uniforms(np.random.RandomState(k + V), L, N))
    assert toks.shape == (N, L + 1) and (toks[:, 0] == V - 1).all()
    drawn = toks[:, 1:] - 1
    assert (drawn >= 0).all() and keep[drawn].all(), sorted(set(drawn[~keep[drawn]].tolist()))
    assert len(set(drawn.reshape(-1).tolist())) > 1 or n_keep == 1
    # the log-likelihood adds the UNtruncated log-probability of every token through the first <END>
    for r in range(N):
        e = np.nonzero(toks[r, 1:] == V)[0]
        upto = e[0] + 1 if e.size else L
        want = float(np.sum(logp[drawn[r, :upto]].astype(np.float64)))
        assert abs(ll[r] - want) <= 1e-12 * max(1.0, abs(want))
    m.close()


@pytest.mark.parametrize("V", [40, 300, 11322])
@pytest.mark.parametrize("k, p", [(1, 1.0), (0, 1e-6), (1, 1e-6)])
def test_pinned_logits_one_survivor_is_the_arg_max(gpu, V, k, p):
    m, logp, N = pinned(V, k, p)
    best = int(np.argsort(-logp, kind='stable')[0])
    assert (logp == logp[best]).sum() == 2 and best == np.nonzero(logp == logp[best])[0][0]      # a tie: the lowest index
    L = 5
    for T in (1.0, 0.5):
        toks, ll = m._gen_sample(L, V - 1, V, T, uniforms(np.random.RandomState(V), L, N))
        assert (toks[:, 1:] == best + 1).all(), (T, sorted(set(toks[:, 1:].reshape(-1).tolist())))
    m.close()


def test_distribution_of_the_truncated_draws(gpu):
    V, k, p, T, L = 40, 8, 0.9, 1.0, 100
    m, logp, N = pinned(V, k, p)
    w = truncated_weights(logp, T, k, p)
    q = w / w.sum()
    assert (q > 0).sum() == 6
    rng = np.random.RandomState(99)
    counts = np.zeros(V, np.int64)
    for _ in range(10):                                         # 10 batches x 20 rows x 100 steps = 20 000 draws
        toks, _ = m._gen_sample(L, V - 1, V, T, rng.random_sample((L, N)))
        counts += np.bincount(toks[:, 1:].reshape(-1) - 1, minlength=V)
    n = int(counts.sum())
    assert n == 10 * N * L == 20000
    sd = np.sqrt(n * q * (1 - q))                               # binomial; 5 standard deviations
    print("counts", counts[q > 0], "expected", n * q[q > 0], "5 sd", 5 * sd[q > 0])
    assert (counts[q == 0] == 0).all()
    assert (np.abs(counts - n * q)[q > 0] <= 5 * sd[q > 0]).all()
    m.close()


# ------------------------------------------------------------------------------------------------------------ off means off, determinism
def test_knobs_off_and_k_at_least_v_are_the_untruncated_sampler(gpu, monkeypatch):
    monkeypatch.delenv('VD_SAMPLE_TOPK', raising=False)
    monkeypatch.delenv('VD_SAMPLE_TOPP', raising=False)
    V, L = 60, 8
    p, dl = tiny(V)
    batch = dl.getIndexData(np.arange(1, 3), p, 'val')
    u = uniforms(np.random.RandomState(4), L, 20)
    out = []
    for knobs in (dict(), dict(topK=0, topP=1.0), dict(topK=V), dict(topK=V + 5, topP=1)):
        m = native(p, **knobs)                                  # same init_seed: the same weights
        m._gen_encode(batch)
        out.append(m._gen_sample(L, V - 1, V, 0.9, u))
        m.close()
    assert len(set(out[0][0][:, 1:].reshape(-1).tolist())) > 5
    for toks, ll in out[1:]:
        assert np.array_equal(toks, out[0][0]) and np.array_equal(ll, out[0][1])
    m = native(p, topK=5)                                       # (and a knob that is on changes the draws)
    m._gen_encode(batch)
    assert not np.array_equal(m._gen_sample(L, V - 1, V, 0.9, u)[0], out[0][0])
    m.close()


@pytest.mark.parametrize("V, k, p", [(60, 7, 0.8), (11322, 40, 0.9), (300, 0, 0.6)])
def test_two_calls_give_the_same_arrays(gpu, V, k, p):
    pr, dl = tiny(V)
    m = native(pr, topK=k, topP=p)
    batch = dl.getIndexData(np.arange(1, 3), pr, 'val')
    u = uniforms(np.random.RandomState(8), 10, 20)
    got = []
    for _ in range(2):
        m._gen_encode(batch)
        got.append(m._gen_sample(10, V - 1, V, 1.1, u))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    assert (got[0][0][:, 1:] >= 1).all()
    m.close()


# ------------------------------------------------------------------------------------------------------------ the per-dialog loops
@pytest.fixture(scope="module")
def fixture_model(gpu):
    """the committed prepro fixture (4 val dialogs x 10 rounds) as generate.py loads it, and a randomly initialised lf-ques + gen
    model over it created with topK = 5, topP = 0.9"""
    from visdial_amd.dataloader import Dataloader
    p = derive(default_params(encoder='lf-ques', decoder='gen', embedSize=16, rnnHiddenSize=32, numLayers=2, gpuid=0,
                              inputQues=os.path.join(PRE, 'visdial_data.h5'), inputImg=os.path.join(PRE, 'data_img.h5'),
                              inputJson=os.path.join(PRE, 'visdial_params.json')))
    dl = Dataloader(seed=1234).initialize(dict(p, concatHistory=False, maxHistoryLen=60), ['val'])
    for k in ('vocabSize', 'maxQuesCount', 'maxQuesLen', 'maxAnsLen'):
        p[k] = getattr(dl, k)
    nat = native(p, topK=5, topP=0.9)
    yield p, dl, nat
    nat.close()


SEED = 7


def test_batched_truncated_sampling_equals_the_per_dialog_loops(fixture_model):
    """seed 7 (SEED).  The share of the 4 x 10 rounds whose host replay alone has a margin below TOL is computed, printed and held to
    <= 2 % here; with 320 draws over 51 words and TOL = 1e-6 the expected count is about 320 * 6 * 2e-6 = 0.004 rounds, i.e. a share
    of 0 % for practically every seed (not yet confirmed on a device), so equal records are the expected outcome."""
    from visdial_amd.model import Model
    p, dl, nat = fixture_model
    cfg = dict(sampleWords=1, beamLen=8, maxThreads=4, temperature=0.9, seed=SEED, topK=5, topP=0.9)
    ref = nat.generateAnswers(dl, 'val', cfg)
    assert ref != nat.generateAnswers(dl, 'val', dict(cfg, topK=0, topP=1.0))        # the per-dialog path needs no matching model
    margins = replay_margins(nat, dl, p, cfg, np.random.RandomState(SEED).random_sample)
    rounds = len(margins)
    near = sum(min(v) < TOL for v in margins.values())
    print("seed %d: %d of %d rounds have a margin below %g in the host replay" % (SEED, near, rounds, TOL))
    assert rounds == 40 and near <= 0.02 * rounds
    for sb in (1, 3):
        explained = check_records(nat.generateAnswers(dl, 'val', dict(cfg, sampleBatch=sb)), ref, margins, TOL, sb)
        assert explained <= 0.02 * rounds, (sb, explained)
    # the operator-level host: its per-dialog loop truncates; its device sampler does not and says where to go
    py = Model(p)
    py.set_parameters_dict(nat.get_parameters_dict())
    assert check_records(py.generateAnswers(dl, 'val', cfg), ref, margins, TOL, 'python') <= 0.02 * rounds
    with pytest.raises(ValueError, match='-host native'):
        py.generateAnswers(dl, 'val', dict(cfg, sampleBatch=2))
    assert len(py.generateAnswers(dl, 'val', dict(cfg, sampleBatch=2, topK=0, topP=1.0))) == 4     # untruncated: as before


def test_generate_py_top_k_top_p_writes_the_per_dialog_results(fixture_model, tmp_path):
    """generate.py -host native -sampleWords 1 -sampleBatch 2 -topK 5 -topP 0.9 in a fresh process against -sampleBatch 0"""
    p, dl, nat = fixture_model
    plain = {k: v for k, v in p.items() if isinstance(v, (int, float, str, bool))}
    ckpt = str(tmp_path / 'model.pt')
    torch.save({'modelW': nat.wrapperW.float().cpu(), 'modelParams': plain, 'optims': {'learningRate': 1e-3}}, ckpt)
    data = ['-inputQues', p['inputQues'], '-inputImg', p['inputImg'], '-inputJson', p['inputJson']]
    res = {}
    for sb in ('0', '2'):
        out = str(tmp_path / ('gen_' + sb))
        g = subprocess.run([sys.executable, os.path.join(ROOT, 'generate.py'), '-loadPath', ckpt, '-maxThreads', '4', '-beamLen', '8',
                            '-host', 'native', '-sampleWords', '1', '-sampleBatch', sb, '-topK', '5', '-topP', '0.9', '-resultPath', out]
                           + data, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert g.returncode == 0, g.stdout[-2000:] + g.stderr[-2000:]
        res[sb] = json.load(open(os.path.join(out, 'results.json')))
        assert res[sb]['opts']['topK'] == 5 and res[sb]['opts']['topP'] == 0.9 and res[sb]['opts']['sampleBatch'] == int(sb)
    cfg = dict(beamLen=8, maxThreads=4, temperature=1.0, topK=5, topP=0.9)
    margins = replay_margins(nat, dl, p, cfg, np.random.RandomState(1234).random_sample)           # generate.py's default -seed
    assert len(res['0']['data']) == 4
    assert check_records(res['2']['data'], res['0']['data'], margins, TOL, 'generate.py') <= 0.02 * len(margins)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_create_refuses_bad_values_and_disc_ignores_them(gpu):
    from visdial_amd import _lib
    from visdial_amd.native import NativeModel
    p, dl = tiny(30)
    for knobs, name in ((dict(topK=-1), 'VD_SAMPLE_TOPK'), (dict(topK='abc'), 'VD_SAMPLE_TOPK'), (dict(topK='5x'), 'VD_SAMPLE_TOPK'),
                        (dict(topP=0), 'VD_SAMPLE_TOPP'), (dict(topP=1.5), 'VD_SAMPLE_TOPP'), (dict(topP=float('nan')), 'VD_SAMPLE_TOPP'),
                        (dict(topP='p'), 'VD_SAMPLE_TOPP'), (dict(topP=-0.5), 'VD_SAMPLE_TOPP')):
        m = None
        with pytest.raises(_lib.VisdialHipError, match=name) as e:
            m = NativeModel(dict(p, **knobs))
        assert m is None and str(list(knobs.values())[0]) in str(e.value)      # the value is named; no model is left behind
        assert 'VD_SAMPLE_TOPK' not in os.environ and 'VD_SAMPLE_TOPP' not in os.environ
    d = dict(p, decoder='disc', numOptions=4)
    for knobs in (dict(topK=5, topP=0.5), dict(topK=-1, topP='abc')):          # decoder disc has no sampling: ignored
        m = NativeModel(dict(d, **knobs))
        assert (m._knobs['topK'], m._knobs['topP']) == (0, 1.0)
        m.close()
    # the batched path of a model created without the knob cannot truncate
    m = native(p)
    with pytest.raises(ValueError, match='created with topK = 0'):
        m.generateAnswers(dl, 'val', dict(sampleWords=1, sampleBatch=2, topK=5, beamLen=4))
    assert len(m.generateAnswers(dl, 'val', dict(sampleWords=1, sampleBatch=0, topK=5, beamLen=4))) == 2
    m.close()
    m = native(p, topK=5)
    with pytest.raises(ValueError, match='created with topK = 5'):
        m.generateAnswers(dl, 'val', dict(sampleWords=1, sampleBatch=2, topK=5, topP=0.5, beamLen=4))
    assert len(m.generateAnswers(dl, 'val', dict(sampleWords=1, sampleBatch=2, topK=5, beamLen=4))) == 2
    m.close()
