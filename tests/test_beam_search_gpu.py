"""Batched beam search (generateAnswers with beamBatch > 0: every round of a chunk of dialogs searched together on the device) against
the per-dialog host-driven search (beamBatch = 0), the fp64 oracle's beam search (oracle/visdial_oracle.py:generate_beam) and, at
full size, an fp64 restatement of the bookkeeping that records how close every decision was."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import visdial_oracle as vo
from visdial_amd.opts import default_params, derive

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def tiny(enc):
    from test_dataloader_cpu import raw_dataset
    from visdial_amd.dataloader import Dataloader
    info, raw, img = raw_dataset(np.random.RandomState(2), n=3, R=3, MQ=5, MA=4, V=20, O=4, nopt=12, F=8)
    raw = {k.replace('_train', '_val'): v for k, v in raw.items()}
    img = {k.replace('_train', '_val'): v for k, v in img.items()}
    info['unique_img_val'] = info.pop('unique_img_train')
    p = derive(default_params(encoder=enc, decoder='gen', embedSize=12, rnnHiddenSize=32, imgFeatureSize=8, imgEmbedSize=8,
                              numLayers=2, batchSize=1, learningRate=1e-3, gpuid=0))
    dl = Dataloader(seed=1).from_arrays(info, raw, img, p, ['val'])
    for k in ('vocabSize', 'maxQuesCount', 'maxQuesLen', 'maxAnsLen'):
        p[k] = getattr(dl, k)
    return p, dl


@pytest.mark.parametrize("enc", ['lf-ques-im-hist', 'mn-ques-hist', 'hre-ques-im-hist'])
def test_batched_beam_search_equals_the_host_search_and_the_oracle(gpu, enc):
    from lua_host import LuaHost, first
    from luavm import to_lua, to_py
    from visdial_amd import utils
    from visdial_amd.model import Model
    from visdial_amd.native import NativeModel
    p, dl = tiny(enc)
    nat = NativeModel(p, init_seed=1234)
    py = Model(p)
    py.set_parameters_dict(nat.get_parameters_dict())
    base = dict(beamSize=3, beamLen=6, maxThreads=2)
    ref = nat.generateAnswers(dl, 'val', base)
    host = LuaHost(p)                      # same initial parameters as NativeModel(p, init_seed=1234)
    m = host.model()
    D = host.dataloader(dl)
    D.fields['word2ind'] = to_lua(host.vm, dict(dl.word2ind))
    D.fields['ind2word'] = to_lua(host.vm, {int(k): v for k, v in dl.ind2word.items()})
    D.fields['numThreads'] = to_lua(host.vm, {'val': 3})
    for bb in (2, 3):                      # 3 exceeds the two dialogs searched
        cfg = dict(base, beamBatch=bb)
        assert nat.generateAnswers(dl, 'val', cfg) == ref, bb
        assert py.generateAnswers(dl, 'val', cfg) == ref, bb
        out = to_py(first(host.invoke(m, 'generateAnswers', D, 'val', to_lua(host.vm, cfg))))
        assert [d['image_id'] for d in out] == [d['image_id'] for d in ref]
        for conv in range(2):
            for it in range(len(ref[conv]['dialog'])):
                assert out[conv]['dialog'][it]['answer'].split() == ref[conv]['dialog'][it]['answer'].split(), (bb, conv, it)
    # all three dialogs in one device search: tokens and scores against the oracle's per-round beam search
    P = {k: v.astype(np.float64) for k, v in nat.get_parameters_dict().items()}
    START, END = dl.word2ind['<START>'], dl.word2ind['<END>']
    batch = dl.getIndexData(np.arange(1, 4), p, 'val')
    R = batch['ques_fwd'].shape[1]
    for model in (nat, py):
        model._set_training(False)
        model._gen_encode(batch)
        toks, scores = model._gen_beam(3, 6, START, END)
        for conv in range(3):
            one = dl.getIndexData(np.array([conv + 1]), p, 'val')
            for it, (beam, score) in enumerate(vo.generate_beam(enc, P, p, one, 3, 6, START, END)):
                assert np.array_equal(toks[conv * R + it], np.asarray(beam)), (conv, it)
                assert abs(scores[conv * R + it] - score) < 1e-5, (conv, it, scores[conv * R + it], score)
                assert utils.idToWords(toks[conv * R + it], dl.ind2word) == utils.idToWords(beam, dl.ind2word)
    nat.close()
    host.close()


def test_batched_beam_search_needs_the_generative_decoder(gpu):
    from visdial_amd import _lib
    from visdial_amd.native import NativeModel
    p, dl = tiny('lf-ques-im-hist')
    p['decoder'] = 'disc'
    p['numOptions'] = 4
    nat = NativeModel(p)
    toks, scores = np.zeros((6, 6), np.int32), np.zeros(6)
    with pytest.raises(_lib.VisdialHipError, match='generative decoder'):
        _lib.call("vd_model_beam_search", nat.h, 3, 6, 1, 2, toks.ctypes.data, scores.ctypes.data)
    nat.close()


def test_generate_py_beam_batch_writes_the_same_results(gpu, tmp_path):
    """generate.py -beamBatch 2 (both hosts) writes the `data` of -beamBatch 0"""
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
        for bb in ('0', '2'):
            out = str(tmp_path / ('gen_%s_%s' % (host, bb)))
            g = subprocess.run([sys.executable, os.path.join(ROOT, 'generate.py'), '-loadPath', save + 'model_final.pt', '-maxThreads',
                                str(n), '-beamSize', '4', '-beamLen', '8', '-beamBatch', bb, '-host', host, '-resultPath', out] + data,
                               capture_output=True, text=True, timeout=600, cwd=ROOT)
            assert g.returncode == 0, g.stdout[-2000:] + g.stderr[-2000:]
            res[host, bb] = json.load(open(os.path.join(out, 'results.json')))
            assert res[host, bb]['opts']['beamBatch'] == int(bb)
    for host in ('native', 'python'):
        assert len(res[host, '0']['data']) == n
        assert res[host, '2']['data'] == res[host, '0']['data'], host


# ---------------------------------------------------------------------------------------------------------------- full size
def margin_beam(P, p, enc_out, qs, it, k, L, START, END):
    """generate_beam's round `it` (oracle/visdial_oracle.py) in fp64, returning (tokens, score, margin): the smallest gap of any
    decision the search took -- a top-k boundary that could matter (the boundary candidate reaches the keep threshold or is <END>),
    the keep boundary, and the best-finished choice.  Decisions between the children of one all-zero row are exact and are
    not counted."""
    H, Lyr = p['rnnHiddenSize'], p['numLayers']
    names = vo._layer_names('dec', p)
    hid = []
    for lv in range(Lyr):
        if qs is not None:
            h = enc_out[it] if lv == Lyr - 1 else qs[lv]['h'][-1][it]
            c = qs[lv]['c'][-1][it]
        else:
            h = enc_out[it] if lv == Lyr - 1 else np.zeros(H)
            c = np.zeros(H)
        hid.append((np.tile(h, (k, 1)), np.tile(c, (k, 1))))
    beams = np.zeros((L, k), np.int64)
    beams[0] = START
    scores = np.zeros(k)
    finish, margin = [], np.inf
    for step in range(1, L):
        explore = 1 if step == 1 else k
        tok = beams[step - 1:step]
        x = vo.lookup(P['embed'], tok)
        newh = []
        for lv in range(Lyr):
            h, c, _ = vo.lstm_forward(x, P[names[lv] + '.W'], P[names[lv] + '.b'], tok, hid[lv][0], hid[lv][1])
            newh.append((h[0], c[0]))
            x = h
        logits = x[0] @ P['vocab.W'].T + P['vocab.b']
        m = logits.max(-1, keepdims=True)
        logp = logits - (m + np.log(np.exp(logits - m).sum(-1, keepdims=True)))
        zero = tok[0] == 0
        logp[zero] = 0.0
        cands, bounds = [], []
        for w in range(explore):
            order = np.argsort(-logp[w], kind='stable')
            for cid in order[:k]:
                cb = beams[:, w].copy()
                cb[step] = cid + 1
                sc = scores[w] + logp[w, cid]
                (finish.append((sc, cb)) if cid + 1 == END else cands.append((sc, cb, w)))
            if not zero[w]:
                a, b = order[k - 1], order[k]
                bounds.append((logp[w, a] - logp[w, b], scores[w] + logp[w, a], a + 1 == END or b + 1 == END))
        cands.sort(key=lambda a: -a[0])
        thr = cands[min(k, len(cands)) - 1][0] if cands else -np.inf
        for gap, sc, is_end in bounds:
            if is_end or sc >= thr - 1e-3:
                margin = min(margin, gap)
        if len(cands) > k:
            a, b = cands[k - 1], cands[k]
            if not (a[2] == b[2] and zero[a[2]]):
                margin = min(margin, a[0] - b[0])
        for i, (sc, cb, w) in enumerate(cands[:k]):
            beams[:, i] = cb
            scores[i] = sc
            for lv in range(Lyr):
                hid[lv][0][i] = newh[lv][0][w]
                hid[lv][1][i] = newh[lv][1][w]
    finish.sort(key=lambda a: -a[0])
    if len(finish) > 1:
        margin = min(margin, finish[0][0] - finish[1][0])
    if finish:
        return finish[0][1], finish[0][0], margin
    if len(cands) > 1:
        margin = min(margin, scores[0] - scores[1])
    return beams[:, 0], scores[0], margin


def full_size_fixture():
    """H = 512, V = 11 322, 2 layers, lf-ques-im-hist + gen, 4 dialogs x 10 rounds, the library-default initialisation (seed 7)
    with the vocabulary projection scaled by 60 so that the random model has the peaked next-word distributions of a trained
    one: near-uniform rows put some top-k boundary of almost every round within 1e-3 (35 of 40 rounds qualify here)"""
    from types import SimpleNamespace
    from visdial_amd.dataloader import SyntheticDataloader
    from visdial_amd.params import init_host
    p = derive(default_params(encoder='lf-ques-im-hist', decoder='gen', vocabSize=11322, embedSize=300, rnnHiddenSize=512,
                              imgFeatureSize=512, numLayers=2, maxQuesCount=10, maxQuesLen=12, maxAnsLen=10, maxHistoryLenPerRound=24,
                              batchSize=4, gpuid=0))
    batch = SyntheticDataloader(p, seed=3).getTrainBatch(p)
    P = init_host(SimpleNamespace(entries=vo.param_spec(p['encoder'], p['decoder'], p)), p['rnnHiddenSize'], 7)
    P['vocab.W'] = P['vocab.W'] * np.float32(60.0)
    return p, batch, P


def test_full_size_batched_beam_search_matches_the_fp64_bookkeeping(gpu):
    from visdial_amd.native import NativeModel
    p, batch, P32 = full_size_fixture()
    nat = NativeModel(p)
    nat.set_parameters_dict(P32)
    nat.training(False)
    k, L, START, END = 5, 20, 1, 2
    nat._gen_encode(batch)
    toks, scores = nat._gen_beam(k, L, START, END)
    P = {n: v.astype(np.float64) for n, v in nat.get_parameters_dict().items()}
    P['embed'][0] = 0
    enc_out, st = vo.encoder_forward(p['encoder'], P, p, {kk: batch[kk] for kk in ('ques_fwd', 'hist', 'img_feat')}, None)
    qs = st.get('qs') if isinstance(st.get('qs'), list) else None
    N = batch['ques_fwd'].shape[0] * batch['ques_fwd'].shape[1]
    assert toks.shape == (N, L) and N >= 40
    qualified, bad = 0, []
    for it in range(N):
        beam, score, margin = margin_beam(P, p, enc_out, qs, it, k, L, START, END)
        if margin < 1e-3:
            continue
        qualified += 1
        if not (np.array_equal(toks[it], beam) and abs(scores[it] - score) < 1e-4):
            bad.append((it, margin, toks[it].tolist(), beam.tolist(), scores[it], score))
    assert not bad, bad[:3]
    assert qualified >= 0.8 * N, (qualified, N)
    nat.close()
