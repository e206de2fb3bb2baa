"""Batched sampling (generateAnswers with sampleWords = 1 and sampleBatch > 0: every round of a chunk of dialogs sampled together
on the device) against a numpy restatement of the host's draw (RandomState.choice), the per-dialog host loop (sampleBatch = 0)
and the fp64 oracle's teacher-forced log-likelihood of the sampled answers.  A token may differ only where its uniform lies
within rounding of a CDF boundary; every such mismatch is checked against the margin of the per-dialog path's fp64 weights."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import visdial_oracle as vo
from test_beam_search_gpu import tiny
from visdial_amd.opts import default_params, derive
from visdial_amd.split_eval import truncated_weights

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def dev(a, dtype):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device='cuda')


# ---------------------------------------------------------------------------------------------------------------- the kernel
def nucleus_margin(logp, T, k, p):
    """the fp64 distance of the nucleus target to the nearest prefix sum of the host rule, relative to the target (inf without a nucleus)"""
    if p >= 1.0:
        return np.inf
    order = np.argsort(-logp, kind='stable')
    n = min(k, logp.size) if k > 0 else logp.size
    cum = np.cumsum(np.exp(logp[order[:n]].astype(np.float64) / T))
    target = p * cum[-1]
    return float(np.abs(cum - target).min() / target)


def host_draw(logp, u, T, k=0, p=1.0):
    """split_eval.py's per-dialog draw: exp(logp / T) -- with top-k `k` / nucleus `p` on, split_eval.truncated_weights -- normalised,
    RandomState.choice(V, p) = cdf.searchsorted(u, 'right') with cdf = cumsum(p) / cdf[-1].  Returns (index, margin): the smaller of
    the fp64 distance of u to the nearest CDF boundary and the relative distance of the nucleus target to the nearest prefix sum."""
    if k == 0 and p == 1.0:
        pr = np.exp(logp.astype(np.float64) / T)             # stated here, not taken from the code under test
    else:
        pr = truncated_weights(logp, T, k, p)
    pr = pr / pr.sum()
    cdf = np.cumsum(pr)
    cdf /= cdf[-1]
    return int(cdf.searchsorted(u, side='right')), min(float(np.abs(cdf - u).min()), nucleus_margin(logp, T, k, p))


@pytest.mark.parametrize("V", [5, 256, 257, 11322])
@pytest.mark.parametrize("T", [0.3, 1.0, 2.5])
def test_sample_draw_is_the_host_draw(gpu, V, T):
    from visdial_amd import ops
    rng = np.random.RandomState(V + int(T * 10))
    rows, L, START, END = 40, 3, 1, 2
    Vp = (V + 3) // 4 * 4
    x = np.full((rows, Vp), 1e4, np.float32)                    # pad columns hold garbage that must be ignored
    x[:, :V] = rng.standard_normal((rows, V)).astype(np.float32) * rng.choice([0.5, 3.0, 12.0], size=(rows, 1)).astype(np.float32)
    tok = rng.randint(1, V + 1, size=rows).astype(np.int32)
    tok[3::7] = 0                                               # MaskZero(LogSoftMax): all-zero rows
    u = rng.random_sample(rows)
    u[:6] = [0.0, 2.0 ** -53, 1e-12, 1 - 2.0 ** -53, 1 - 1e-12, 0.5]
    u[20:23] = [0.0, 1 - 2.0 ** -53, 1 - 1e-15]
    hist = torch.empty(rows, L + 1, dtype=torch.int32, device='cuda')
    tk = torch.empty(1, rows, dtype=torch.int32, device='cuda')
    loglik = torch.empty(rows, dtype=torch.float64, device='cuda')
    status = torch.full((1,), 5, dtype=torch.int32, device='cuda')
    ops.sample_init(L, START, hist, tk, loglik, status)
    assert status.item() == 0 and (hist[:, 0] == START).all() and (hist[:, 1:] == 0).all() and (tk == START).all()
    step = 2
    hist[:, 1] = 9                                              # an earlier column without <END>
    hist[5, 1] = END                                            # row 5 has ended: its log-likelihood stays
    tk.copy_(dev(tok[None], torch.int32))
    lg = dev(x, torch.float32)
    ops.sample_draw(lg, V, tk, dev(u, torch.float64), T, step, L, END, hist, loglik, status)
    ref = dev(x, torch.float32)
    ops.log_softmax_rows(ref, V)                                # the kernel the log-probabilities must equal bit for bit
    lp = ref.cpu().numpy()[:, :V]
    lp[tok == 0] = 0.0
    assert np.array_equal(lg.cpu().numpy(), x)                  # logits are not written
    assert status.item() == 0
    h, t, ll = hist.cpu().numpy(), tk.cpu().numpy()[0], loglik.cpu().numpy()
    assert np.array_equal(h[:, step], t) and (h[:, step + 1:] == 0).all()
    mismatches = 0
    for r in range(rows):
        c, margin = host_draw(lp[r], u[r], T)
        if t[r] != c + 1:
            mismatches += 1
            assert margin < 1e-12, (r, t[r], c + 1, margin)
        assert 1 <= t[r] <= V
        expect = 0.0 if r == 5 else float(lp[r, t[r] - 1])     # bit-identical to vd_log_softmax_rows at the drawn index
        assert ll[r] == expect, (r, ll[r], expect)
    assert mismatches <= 1


def test_sample_draw_flags_an_all_underflow_row(gpu):
    from visdial_amd import ops
    rows, V, L = 3, 11322, 1
    x = np.zeros((rows, V), np.float32)                        # uniform rows: every logp = -log V = -9.33
    x[1, 0] = 50.0                                             # row 1 has one likely word: exp(0 / T) = 1 survives
    hist = torch.empty(rows, L + 1, dtype=torch.int32, device='cuda')
    tk = torch.empty(1, rows, dtype=torch.int32, device='cuda')
    loglik = torch.empty(rows, dtype=torch.float64, device='cuda')
    status = torch.empty(1, dtype=torch.int32, device='cuda')
    ops.sample_init(L, 1, hist, tk, loglik, status)
    ops.sample_draw(dev(x, torch.float32), V, tk, dev(np.full(rows, 0.5), torch.float64), 0.01, 1, L, 2, hist, loglik, status)
    assert status.item() == 1
    h = hist.cpu().numpy()
    assert h[0, 1] == 0 and h[2, 1] == 0 and h[1, 1] == 1      # nothing drawn where everything underflowed
    assert loglik.cpu().numpy()[0] == 0.0


# ---------------------------------------------------------------------------------------------------------------- model level
def replay_margins(model, dl, p, cfg, uniform):
    """the per-dialog sampling loop of split_eval.py (with cfg's topK / topP, if any) replayed through `_gen_step` with the uniforms
    `uniform()` hands out in the loop's order: {(dialog index, round): [margin of host_draw, per step]}"""
    START = dl.word2ind['<START>']
    L, T, k, pp = cfg['beamLen'], cfg.get('temperature', 1.0), cfg.get('topK', 0), cfg.get('topP', 1.0)
    model._set_training(False)
    out = {}
    for conv in range(cfg['maxThreads']):
        batch = dl.getIndexData(np.array([conv + 1]), p, 'val')
        R = batch['ques_fwd'].shape[1]
        model._gen_encode(batch)
        model._gen_begin(np.arange(R, dtype=np.int32))
        tok = np.full(R, START, np.int64)
        for _ in range(L):
            logp = model._gen_step(tok)
            model._gen_select(np.arange(R, dtype=np.int32), R)
            for i in range(R):
                c, margin = host_draw(logp[i], uniform(), T, k, pp)
                out.setdefault((conv, i), []).append(margin)
                tok[i] = c + 1
    model._set_training(True)
    return out


def check_records(got, ref, margins, tol, what):
    """equal records, or every differing round has a margin below `tol` at or before its first differing word; returns how many differ"""
    assert len(got) == len(ref) and [d['image_id'] for d in got] == [d['image_id'] for d in ref], what
    explained = 0
    for conv, (a, b) in enumerate(zip(got, ref)):
        for it, (x, y) in enumerate(zip(a['dialog'], b['dialog'])):
            assert x['question'] == y['question'], (what, conv, it)
            if x['answer'] == y['answer']:
                continue
            wa, wb = x['answer'].split(), y['answer'].split()
            k = next((i for i, (s, t) in enumerate(zip(wa, wb)) if s != t), min(len(wa), len(wb)))
            m = min(margins[conv, it][:k + 1])
            assert m < tol, (what, conv, it, m, x['answer'], y['answer'])
            explained += 1
    return explained


@pytest.mark.parametrize("enc", ['lf-ques-im-hist', 'mn-ques-hist', 'hre-ques-im-hist'])
def test_batched_sampling_equals_the_per_dialog_loop_and_the_oracle(gpu, enc):
    from visdial_amd.model import Model
    from visdial_amd.native import NativeModel
    p, dl = tiny(enc)
    nat = NativeModel(p, init_seed=1234)
    py = Model(p)
    py.set_parameters_dict(nat.get_parameters_dict())
    base = dict(sampleWords=1, beamLen=6, maxThreads=3, temperature=0.8, seed=7)
    ref = nat.generateAnswers(dl, 'val', base)
    rs = np.random.RandomState(7)
    margins = replay_margins(nat, dl, p, base, rs.random_sample)
    for model, name in ((nat, 'native'), (py, 'python')):
        for sb in (0, 1, 2, 3):
            check_records(model.generateAnswers(dl, 'val', dict(base, sampleBatch=sb)), ref, margins, 1e-6, (name, sb))
    # all three dialogs in one device call: the returned log-likelihoods against the fp64 oracle's teacher-forced ones
    P = {k: v.astype(np.float64) for k, v in nat.get_parameters_dict().items()}
    P['embed'][0] = 0
    START, END = dl.word2ind['<START>'], dl.word2ind['<END>']
    batch = dl.getIndexData(np.arange(1, 4), p, 'val')
    B, R = batch['ques_fwd'].shape[:2]
    L, T = 6, 0.8
    u = np.random.RandomState(3).random_sample((L, B * R))
    enc_out, st = vo.encoder_forward(enc, P, p, batch, None)
    for model in (nat, py):
        model._set_training(False)
        model._gen_encode(batch)
        toks, ll = model._gen_sample(L, START, END, T, u)
        assert toks.shape == (B * R, L + 1) and (toks[:, 0] == START).all() and (toks[:, 1:] >= 1).all()
        oin, oout = toks[:, :L].copy(), toks[:, 1:].copy()
        for r in range(B * R):                                  # the answer ends at its first <END> (which counts)
            e = np.nonzero(oout[r] == END)[0]
            if e.size:
                oout[r, e[0] + 1:] = 0
        b2 = dict(option_in=oin.reshape(B, R, 1, L), option_out=oout.reshape(B, R, 1, L))
        lh = vo.gen_retrieve_scores(P, p, b2, enc_out, st)[:, 0]
        assert np.all(np.abs(ll - lh) <= 1e-4 * np.abs(lh)), np.abs(ll - lh).max()
        model._set_training(True)
    nat.close()


def test_lua_batched_sampling_equals_the_lua_per_dialog_loop(gpu):
    from lua_host import LuaHost, first
    from luavm import to_lua, to_py
    from visdial_amd.native import NativeModel
    p, dl = tiny('lf-ques-im-hist')
    host = LuaHost(p)                                           # same initial parameters as NativeModel(p, init_seed=1234)
    m = host.model()
    D = host.dataloader(dl)
    D.fields['word2ind'] = to_lua(host.vm, dict(dl.word2ind))
    D.fields['ind2word'] = to_lua(host.vm, {int(k): v for k, v in dl.ind2word.items()})
    D.fields['numThreads'] = to_lua(host.vm, {'val': 3})
    base = dict(sampleWords=1, beamLen=6, maxThreads=3, temperature=1.3)
    res = {}
    for sb in (0, 2, 3):
        host.vm.torch.f_manualSeed(21)                          # torch.manualSeed(21) before each run
        res[sb] = to_py(first(host.invoke(m, 'generateAnswers', D, 'val', to_lua(host.vm, dict(base, sampleBatch=sb)))))
    nat = NativeModel(p, init_seed=1234)                        # the fp64-weight margins of the same draws
    margins = replay_margins(nat, dl, p, base, np.random.RandomState(21).random_sample)
    nat.close()
    for sb in (2, 3):                                           # the Lua loop normalises fp32 weights: 1e-6
        check_records(res[sb], res[0], margins, 1e-6, sb)
    host.close()


def test_model_sample_argument_errors(gpu):
    from visdial_amd import _lib
    from visdial_amd.native import NativeModel
    p, dl = tiny('lf-ques-im-hist')
    nat = NativeModel(p, init_seed=1234)
    toks, ll = np.zeros((9, 7), np.int32), np.zeros(9)
    u = np.full((6, 9), 0.5)

    def sample(L=6, T=1.0, uu=u):
        _lib.call("vd_model_sample", nat.h, L, 1, 2, T, uu.ctypes.data, toks.ctypes.data, ll.ctypes.data)
    with pytest.raises(_lib.VisdialHipError, match='vd_model_encode'):
        sample()
    nat._set_training(False)
    nat._gen_encode(dl.getIndexData(np.arange(1, 4), p, 'val'))
    assert nat._N == 9
    with pytest.raises(_lib.VisdialHipError, match='beam_len'):
        sample(L=0)
    for T in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(_lib.VisdialHipError, match='temperature'):
            sample(T=T)
    for bad in (1.0, -1e-300, float('nan')):
        v = u.copy()
        v[3, 4] = bad
        with pytest.raises(_lib.VisdialHipError, match=r'outside \[0, 1\)'):
            sample(uu=v)
    with pytest.raises(_lib.VisdialHipError, match='underflowed at temperature 1e-05'):
        sample(T=1e-5)
    sample()                                                    # the model is still usable
    assert (toks[:, 0] == 1).all() and (toks[:, 1:] >= 1).all()
    nat.close()


def test_batched_sampling_needs_the_generative_decoder(gpu):
    from visdial_amd import _lib
    from visdial_amd.native import NativeModel
    p, dl = tiny('lf-ques-im-hist')
    p['decoder'] = 'disc'
    p['numOptions'] = 4
    nat = NativeModel(p)
    toks, ll, u = np.zeros((6, 7), np.int32), np.zeros(6), np.full((6, 6), 0.5)
    with pytest.raises(_lib.VisdialHipError, match='generative decoder'):
        _lib.call("vd_model_sample", nat.h, 6, 1, 2, 1.0, u.ctypes.data, toks.ctypes.data, ll.ctypes.data)
    nat.close()


def test_generate_py_sample_batch_writes_the_same_results(gpu, tmp_path):
    """generate.py -sampleWords 1 -sampleBatch 2 (both hosts) writes the `data` of -sampleBatch 0"""
    from test_dataloader_cpu import raw_dataset
    rng = np.random.RandomState(5)
    n, R = 5, 3
    info, raw, img = raw_dataset(rng, n=n, R=R, MQ=6, MA=5, V=30, O=5, nopt=40, F=8)
    for k in list(raw):
        raw[k.replace('_train', '_val')] = raw[k]
    img['images_val'] = img['images_train']
    info['unique_img_val'] = ['VisualDialog_val2018_%012d.jpg' % (1000 + i) for i in range(n)]
    np.savez(str(tmp_path / 'visdial_data.npz'), **raw)
    np.savez(str(tmp_path / 'data_img.npz'), **img)
    json.dump(info, open(str(tmp_path / 'visdial_params.json'), 'w'))
    data = ['-inputQues', str(tmp_path / 'visdial_data.h5'), '-inputImg', str(tmp_path / 'data_img.h5'),
            '-inputJson', str(tmp_path / 'visdial_params.json')]
    save = str(tmp_path / "ckpt") + "/"
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '-encoder', 'lf-ques-im-hist', '-decoder', 'gen',
                        '-imgFeatureSize', '8', '-rnnHiddenSize', '32', '-embedSize', '16', '-batchSize', '2', '-savePath', save,
                        '-numEpochs', '100', '-saveIter', '1000', '--maxIters', '30', '-saveFormat', 'pt'] + data,
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = {}
    for host in ('native', 'python'):
        for sb in ('0', '2'):
            out = str(tmp_path / ('gen_%s_%s' % (host, sb)))
            g = subprocess.run([sys.executable, os.path.join(ROOT, 'generate.py'), '-loadPath', save + 'model_final.pt', '-maxThreads',
                                str(n), '-beamLen', '8', '-sampleWords', '1', '-temperature', '0.9', '-sampleBatch', sb, '-host', host,
                                '-resultPath', out] + data, capture_output=True, text=True, timeout=600, cwd=ROOT)
            assert g.returncode == 0, g.stdout[-2000:] + g.stderr[-2000:]
            res[host, sb] = json.load(open(os.path.join(out, 'results.json')))
            assert res[host, sb]['opts']['sampleBatch'] == int(sb) and res[host, sb]['opts']['seed'] == 1234
    for host in ('native', 'python'):
        assert len(res[host, '0']['data']) == n
        assert res[host, '2']['data'] == res[host, '0']['data'], host


# ---------------------------------------------------------------------------------------------------------------- full size
class Dialogs(object):
    """synthetic dialogs behind the getIndexData / word2ind / ind2word surface generateAnswers reads (scripts/mb_generate.py)"""

    def __init__(self, p, n, V):
        q = dict(p, batchSize=n)
        from visdial_amd.dataloader import SyntheticDataloader
        self.b = SyntheticDataloader(q, seed=5).getTrainBatch(q)
        self.numThreads = {'val': n}
        self.word2ind = {'<START>': V - 1, '<END>': V}
        self.ind2word = {i: '<START>' if i == V - 1 else '<END>' if i == V else 'w%d' % i for i in range(1, V + 1)}

    def getIndexData(self, inds, params, dtype):
        ix = np.asarray(inds, np.int64) - 1
        return {k: np.ascontiguousarray(self.b[k][ix]) for k in ('ques_fwd', 'hist', 'img_feat')}


def test_full_size_batched_sampling_equals_the_per_dialog_loop(gpu):
    from visdial_amd.native import NativeModel
    V, R, D = 11322, 10, 20
    p = derive(default_params(encoder='lf-ques-im-hist', decoder='gen', vocabSize=V, embedSize=300, rnnHiddenSize=512,
                              imgFeatureSize=4096, numLayers=2, maxQuesCount=R, maxQuesLen=20, maxAnsLen=20, maxHistoryLenPerRound=40,
                              batchSize=20, gpuid=0))
    dl = Dialogs(p, D, V)
    nat = NativeModel(p, init_seed=1)
    nat.training(False)
    cfg = dict(sampleWords=1, beamLen=20, maxThreads=D, temperature=1.0, seed=1234)
    ref = nat.generateAnswers(dl, 'val', cfg)
    got = nat.generateAnswers(dl, 'val', dict(cfg, sampleBatch=20))
    margins = replay_margins(nat, dl, p, cfg, np.random.RandomState(1234).random_sample)
    near = sum(m < 1e-6 for v in margins.values() for m in v)
    explained = check_records(got, ref, margins, 1e-6, 'full size')
    print("full size: %d draws, %d with u within 1e-6 of a CDF boundary, %d rounds differ (each explained)" % (
        sum(len(v) for v in margins.values()), near, explained))
    assert sum(a == b for a, b in zip(got, ref)) + explained >= D
    nat.close()
