"""Batched sampling (params.sampleBatch > 0 with sampleWords = 1) without a device: the Lua host on the dry library makes ONE
vd_model_sample per chunk of dialogs (no per-step vd_model_decode_*), both hosts' argument rules, and the shared host loop of
split_eval.py over numpy stand-ins for the device steps -- the uniform order and the chunking give the per-dialog records."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from conftest import ROOT
from lua_host import first
from luavm import LuaError, to_lua, to_py
from test_beam_cpu import _lua, _tiny_val

BEAM_REFUSAL = 'beamBatch > 0 is batched beam search; sampling (sampleWords = 1) runs on the host: use beamBatch = 0'


def test_lua_generate_answers_batched_sampling_is_one_device_call_per_chunk():
    p, dl = _tiny_val()
    host, m, D = _lua(p, dl)
    n0 = len(host.dry.calls)
    cfg = dict(sampleWords=1, sampleBatch=2, beamLen=6, maxThreads=3, temperature=0.7)
    out = to_py(first(host.invoke(m, 'generateAnswers', D, 'val', to_lua(host.vm, cfg))))
    names = [c[0] for c in host.dry.calls[n0:]]
    assert names.count('vd_model_sample') == 2                 # dialogs [1, 2] and [3]
    assert names.count('vd_model_encode') == 2
    assert not any(n.startswith('vd_model_decode_') for n in names)
    calls = [c for c in host.dry.calls[n0:] if c[0] == 'vd_model_sample']
    assert [tuple(c[1][1:5]) for c in calls] == [(6, dl.word2ind['<START>'], dl.word2ind['<END>'], 0.7)] * 2
    assert len(out) == 3 and [len(d['dialog']) for d in out] == [3, 3, 3]
    ids = list(dl.unique_img_val)
    assert [d['image_id'] for d in out] == ids[:3]
    from visdial_amd import utils
    for conv in (1, 3):
        batch = dl.getIndexData(np.array([conv]), p, 'val')
        assert [r['question'] for r in out[conv - 1]['dialog']] == [utils.idToWords(batch['ques_fwd'][0, it], dl.ind2word)
                                                                     for it in range(3)]
    host.close()


def test_lua_refuses_sample_batch_without_sampling():
    p, dl = _tiny_val()
    host, m, D = _lua(p, dl)
    with pytest.raises(LuaError, match='sampleBatch'):
        host.invoke(m, 'generateAnswers', D, 'val', to_lua(host.vm, dict(sampleBatch=2, maxThreads=1)))
    with pytest.raises(LuaError, match='beamBatch > 0 is batched beam search'):    # unchanged, also next to sampleBatch
        host.invoke(m, 'generateAnswers', D, 'val', to_lua(host.vm, dict(sampleWords=1, beamBatch=2, sampleBatch=2, maxThreads=1)))
    host.close()


class Host(object):
    """numpy stand-ins for the device steps of split_eval.SplitEval.generateAnswers.  A row's log-probabilities are a fixed
    function of (its question, steps taken, input token); `_gen_sample` restates csrc/sample.hip's per-row rule in fp64."""
    V = None                                                   # the dataloader's vocabulary size

    def _set_training(self, on):
        pass

    def _gen_encode(self, batch):
        q = batch['ques_fwd'].astype(np.int64)                # (a batch pads its questions to its own longest one)
        self.keys = [zlib.crc32(q[b, r][q[b, r] != 0].tobytes()) + 7 * r for b in range(q.shape[0]) for r in range(q.shape[1])]

    def _logp(self, key, t, tok):
        rs = np.random.RandomState((key * 31 + t * 1009 + int(tok)) % (2 ** 32))
        x = (rs.standard_normal(self.V) * 2).astype(np.float32)
        m = x.max()
        return (x - (m + np.log(np.exp(x - m).sum()))).astype(np.float32)

    def _gen_begin(self, rounds):
        self.rows, self.t = [self.keys[r] for r in rounds], 0

    def _gen_step(self, tokens):
        out = np.stack([self._logp(k, self.t, tok) for k, tok in zip(self.rows, tokens)])
        self.t += 1
        return out

    def _gen_select(self, src, n_keep):
        assert list(src) == list(range(n_keep)) == list(range(len(self.rows)))   # sampling passes the identity

    def _gen_sample(self, beamLen, startToken, endToken, temperature, uniforms):
        self.sample_calls.append(uniforms.shape)
        N = len(self.keys)
        assert uniforms.shape == (beamLen, N)
        hist = np.zeros((N, beamLen + 1), np.int32)
        hist[:, 0] = startToken
        loglik = np.zeros(N)
        for r in range(N):
            for s in range(1, beamLen + 1):
                lp = self._logp(self.keys[r], s - 1, hist[r, s - 1])
                w = np.exp(lp.astype(np.float64) / temperature)
                c = int(np.searchsorted(np.cumsum(w), uniforms[s - 1, r] * w.sum(), side='right'))
                c = min(c, int(np.nonzero(w > 0)[0][-1]))
                if endToken not in hist[r, 1:s]:
                    loglik[r] += float(lp[c])
                hist[r, s] = c + 1
        return hist, loglik


def _host(p):
    from visdial_amd.split_eval import SplitEval

    class H(Host, SplitEval):
        params = p
        V = p['vocabSize']
    h = H()
    h.sample_calls = []
    return h


def test_batched_sampling_host_loop_gives_the_per_dialog_records():
    p, dl = _tiny_val()
    dl.numThreads = {'val': 3}
    base = dict(sampleWords=1, beamLen=7, maxThreads=3, temperature=0.8, seed=11)
    h0 = _host(p)
    ref = h0.generateAnswers(dl, 'val', base)
    assert h0.sample_calls == []
    assert len(ref) == 3 and all(len(d['dialog']) == 3 for d in ref)
    assert len({d['dialog'][it]['answer'] for d in ref for it in range(3)}) > 1
    for sb, calls in ((1, 3), (2, 2), (3, 1)):
        h = _host(p)
        assert h.generateAnswers(dl, 'val', dict(base, sampleBatch=sb)) == ref, sb
        assert len(h.sample_calls) == calls, (sb, h.sample_calls)
    other = _host(p).generateAnswers(dl, 'val', dict(base, sampleBatch=2, seed=12))
    assert other != ref                                        # the seed reaches the batched draws


def test_python_hosts_refuse_sample_batch_without_sampling():
    p, dl = _tiny_val()
    with pytest.raises(ValueError, match='sampleBatch'):
        _host(p).generateAnswers(dl, 'val', dict(sampleBatch=2, maxThreads=1))
    with pytest.raises(ValueError, match='sampleBatch'):
        _host(p).generateAnswers(dl, 'val', dict(sampleWords=0, sampleBatch=1, maxThreads=1))
    with pytest.raises(ValueError) as e:                       # the beamBatch refusal, word for word
        _host(p).generateAnswers(dl, 'val', dict(sampleWords=1, beamBatch=2, sampleBatch=2, maxThreads=1))
    assert str(e.value) == BEAM_REFUSAL


def test_generate_py_lists_sample_batch_and_seed():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'generate.py'), '-h'], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert '-sampleBatch' in r.stdout and '-seed' in r.stdout
