"""Batched beam search (params.beamBatch > 0) through the Lua host on the dry library: lua/model.lua:generateAnswers drives the
whole search with ONE vd_model_beam_search per chunk of dialogs (no per-step vd_model_decode_step), and refuses beamBatch together
with sampling.  The Python hosts' refusal is checked here too (it needs no device)."""
import numpy as np
import pytest

from lua_host import LuaHost, first
from luavm import LuaError, to_lua, to_py
from visdial_amd.opts import default_params, derive


def _tiny_val():
    from test_dataloader_cpu import raw_dataset
    from visdial_amd.dataloader import Dataloader
    info, raw, img = raw_dataset(np.random.RandomState(2), n=3, R=3, MQ=5, MA=4, V=20, O=4, nopt=12, F=8)
    raw = {k.replace('_train', '_val'): v for k, v in raw.items()}
    img = {k.replace('_train', '_val'): v for k, v in img.items()}
    info['unique_img_val'] = info.pop('unique_img_train')
    p = derive(default_params(encoder='lf-ques-im-hist', decoder='gen', embedSize=12, rnnHiddenSize=32, imgFeatureSize=8, imgEmbedSize=8,
                              numLayers=2, batchSize=1, learningRate=1e-3, gpuid=0))
    dl = Dataloader(seed=1).from_arrays(info, raw, img, p, ['val'])
    for k in ('vocabSize', 'maxQuesCount', 'maxQuesLen', 'maxAnsLen'):
        p[k] = getattr(dl, k)
    return p, dl


def _lua(p, dl):
    host = LuaHost(p, dry=True)
    m = host.model()
    D = host.dataloader(dl)
    D.fields['word2ind'] = to_lua(host.vm, dict(dl.word2ind))
    D.fields['ind2word'] = to_lua(host.vm, {int(k): v for k, v in dl.ind2word.items()})
    D.fields['numThreads'] = to_lua(host.vm, {'val': 3})
    return host, m, D


def test_lua_generate_answers_batched_beam_search_is_one_device_call_per_chunk():
    p, dl = _tiny_val()
    host, m, D = _lua(p, dl)
    n0 = len(host.dry.calls)
    out = to_py(first(host.invoke(m, 'generateAnswers', D, 'val', to_lua(host.vm, dict(beamSize=3, beamLen=6, maxThreads=3, beamBatch=2)))))
    names = [c[0] for c in host.dry.calls[n0:]]
    assert names.count('vd_model_beam_search') == 2            # dialogs [1, 2] and [3]
    assert names.count('vd_model_encode') == 2
    assert not any(n.startswith('vd_model_decode_') for n in names)
    calls = [c for c in host.dry.calls[n0:] if c[0] == 'vd_model_beam_search']
    assert [tuple(c[1][1:5]) for c in calls] == [(3, 6, dl.word2ind['<START>'], dl.word2ind['<END>'])] * 2
    assert len(out) == 3 and [len(d['dialog']) for d in out] == [3, 3, 3]
    ids = list(dl.unique_img_val)
    assert [d['image_id'] for d in out] == ids[:3]
    from visdial_amd import utils
    batch = dl.getIndexData(np.array([3]), p, 'val')
    assert [r['question'] for r in out[2]['dialog']] == [utils.idToWords(batch['ques_fwd'][0, it], dl.ind2word) for it in range(3)]
    host.close()


def test_lua_batched_beam_search_refuses_sampling():
    p, dl = _tiny_val()
    host, m, D = _lua(p, dl)
    with pytest.raises(LuaError, match='beamBatch'):
        host.invoke(m, 'generateAnswers', D, 'val', to_lua(host.vm, dict(sampleWords=1, beamBatch=2, maxThreads=1)))
    host.close()


def test_python_hosts_refuse_batched_beam_search_with_sampling():
    from visdial_amd.split_eval import SplitEval

    class Host(SplitEval):                     # the refusal comes before any device call
        params = {'decoder': 'gen'}

    p, dl = _tiny_val()
    with pytest.raises(ValueError, match='beamBatch'):
        Host().generateAnswers(dl, 'val', dict(sampleWords=1, beamBatch=2, maxThreads=1))
