"""Detector regions without a device (csrc/attention.hip IR1 - IR6): both loaders (padding, zeroed rows, `img_regions` in train / val / test
batches; with M = 0 the synthetic loader's stream untouched), the -imgRegions flag of train.py / evaluate.py / generate.py with its
defaults and refusals, NativeModel's attachment call, the frozen surfaces, the rules at the top of attention.hip and the documents."""
import json
import os
import re
import sys

import numpy as np
import pytest

from conftest import small_params
from visdial_amd import opts
from visdial_amd.dataloader import Dataloader, SyntheticDataloader, pad_regions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRE = os.path.join(ROOT, 'tests', 'golden', 'prepro')
REGIONS = os.path.join(ROOT, 'tests', 'golden', 'regions', 'data_regions.npz')
QUES_NPZ = os.path.join(PRE, 'expected.npz')
M, C = 9, 8


# ------------------------------------------------------------------------------------------------------------ the fixture
def test_the_fixture_is_what_its_generator_writes():
    z = np.load(REGIONS)
    pre = np.load(QUES_NPZ)
    assert os.path.getsize(REGIONS) < 8 * 1024
    for split in ('train', 'val', 'test'):
        f, cnt = z['regions_' + split], z['num_regions_' + split]
        assert f.dtype == np.float32 and f.shape == (pre['img.images_' + split].shape[0], M, C)
        assert cnt.shape == (f.shape[0],) and cnt.min() == 1 and cnt.max() == M
        hidden = np.arange(M)[None, :] >= cnt[:, None]
        assert (f[hidden] == 1e3).all() and np.isfinite(f).all()                    # the loader has something to zero


# ------------------------------------------------------------------------------------------------------------ the real-data loader
def prepro_arrays():
    z = np.load(QUES_NPZ)
    return {k[len('data.'):]: z[k] for k in z.files if k.startswith('data.')}


def region_loader(subsets, img=None, **kw):
    p = opts.derive(opts.default_params(encoder='mn-att-ques-im-hist', decoder='disc', imgFeatureSize=C, imgRegions=M, host='native',
                                        inputImg=REGIONS, **kw))
    opts.apply_img_regions(p)
    info = json.load(open(os.path.join(PRE, 'visdial_params.json')))
    return p, Dataloader(seed=1).from_arrays(info, prepro_arrays(), np.load(REGIONS) if img is None else img, p, subsets)


def test_dataloader_pads_zeroes_and_carries_the_counts(capsys):
    p, dl = region_loader(['train', 'val', 'test'])
    assert p['imgSpatialSize'] == 3 and p['imgNorm'] == 0 and '-imgRegions 9: imgSpatialSize = 3' in capsys.readouterr().out
    z = np.load(REGIONS)
    batches = {'train': dl.getTrainBatch(dict(p, batchSize=4, numTrainThreads=dl.numThreads['train'])),
               'val': dl.getTestBatch(1, dict(p, batchSize=3), 'val')[0], 'test': dl.getTestBatch(2, dict(p, batchSize=2), 'test')[0]}
    for split, b in batches.items():
        B = b['ques_fwd'].shape[0]
        assert b['img_feat'].shape == (B, 3, 3, C) and b['img_feat'].dtype == np.float32
        assert b['img_regions'].shape == (B,) and b['img_regions'].dtype == np.int32
        f = b['img_feat'].reshape(B, 9, C)
        hidden = np.arange(9)[None, :] >= b['img_regions'][:, None]
        assert (f[hidden] == 0).all() and (f[~hidden] > 0).all()
    # rows and counts are the file's, picked through img_pos
    b = batches['val']
    pos = prepro_arrays()['img_pos_val'][:3].astype(int)
    assert np.array_equal(b['img_regions'], z['num_regions_val'][pos])
    for i, j in enumerate(pos):
        k = int(z['num_regions_val'][j])
        assert np.array_equal(b['img_feat'][i].reshape(9, C)[:k], z['regions_val'][j, :k])


def test_a_grid_wider_than_m_is_padded_with_zero_rows():
    f = np.arange(2 * 5 * 3, dtype=np.float32).reshape(2, 5, 3) + 1
    out = pad_regions(f, [5, 2], 9)
    assert out.shape == (2, 9, 3) and np.array_equal(out[0, :5], f[0]) and not out[0, 5:].any()
    assert np.array_equal(out[1, :2], f[1, :2]) and not out[1, 2:].any()
    p = opts.apply_img_regions(opts.derive(dict(encoder='lf-att-ques-im-hist', imgRegions=5, host='native')))
    assert p['imgSpatialSize'] == 3
    for m, s in ((1, 1), (4, 2), (5, 3), (9, 3), (10, 4), (36, 6), (100, 10), (101, 11)):
        assert opts.apply_img_regions(dict(encoder='mn-att-ques-im-hist', imgRegions=m, host='native'))['imgSpatialSize'] == s


def test_the_loader_refuses_by_name():
    z = dict(np.load(REGIONS))
    with pytest.raises(ValueError, match=r"-imgRegions 9: .* holds no dataset 'num_regions_val'"):
        region_loader(['val'], {k: v for k, v in z.items() if k != 'num_regions_val'})
    with pytest.raises(ValueError, match=r"-imgRegions 9: .* holds no dataset 'regions_train'"):
        region_loader(['train'], {'images_train': np.zeros((5, C, 3, 3), np.float32)})
    with pytest.raises(ValueError, match=r"'regions_val' of .* has the shape \(4, 8, 8\), its second dimension must be M = 9"):
        region_loader(['val'], dict(z, regions_val=z['regions_val'][:, :8]))
    for bad, word in ((0, '0'), (10, '10'), (2.5, '2.5')):
        cnt = z['num_regions_val'].astype(np.float64)
        cnt[1] = bad
        with pytest.raises(ValueError, match=r"'num_regions_val' of .* must hold one integer count in 1 \.\. 9 per image, found %s" % re.escape(word)):
            region_loader(['val'], dict(z, num_regions_val=cnt))
    with pytest.raises(ValueError, match=r"'num_regions_val' of .* found the shape \(3,\) for 4 images"):
        region_loader(['val'], dict(z, num_regions_val=z['num_regions_val'][:3]))


# ------------------------------------------------------------------------------------------------------------ the synthetic loader
@pytest.mark.parametrize("fast", [False, True])
def test_synthetic_loader_draws_counts_and_zeroes_the_hidden_rows(fast):
    p = opts.derive(small_params(imgSpatialSize=3, imgRegions=7, batchSize=6))
    dl = SyntheticDataloader(p, seed=5, fast=fast)
    seen = set()
    for b in (dl.getTrainBatch(p), dl.getTestBatch(1, p, 'val')[0], dl.getTestBatch(1, p, 'test')[0], dl.getTrainBatch(p)):
        cnt = b['img_regions']
        assert cnt.dtype == np.int32 and cnt.shape == (6,) and cnt.min() >= 1 and cnt.max() <= 7
        f = b['img_feat'].reshape(6, 9, -1)
        hidden = np.arange(9)[None, :] >= cnt[:, None]
        assert b['img_feat'].shape == (6, 3, 3, p['imgFeatureSize']) and (f[hidden] == 0).all() and (f[~hidden] != 0).all()
        seen.update(cnt.tolist())
    assert len(seen) > 3
    with pytest.raises(ValueError, match='imgRegions = 10 does not fit imgSpatialSize = 3'):
        SyntheticDataloader(dict(p, imgRegions=10), seed=5).getTrainBatch(p)


@pytest.mark.parametrize("enc,dec", [('mn-att-ques-im-hist', 'disc'), ('lf-att-ques-im-hist', 'gen'), ('lf-ques-im-hist', 'disc')])
@pytest.mark.parametrize("fast", [False, True])
def test_with_m_zero_the_synthetic_stream_is_untouched(enc, dec, fast):
    """imgRegions = 0 / absent draws nothing extra; and with M > 0 everything except the image rows is still the same stream"""
    p = opts.derive(small_params(encoder=enc, decoder=dec, imgSpatialSize=3))
    ref, zero = SyntheticDataloader(p, seed=9, fast=fast), SyntheticDataloader(dict(p, imgRegions=0), seed=9, fast=fast)
    assert zero.region_rng is None
    reg = SyntheticDataloader(dict(p, imgRegions=9), seed=9, fast=fast) if 'att' in enc else None
    for _ in range(3):
        a, b = ref.getTrainBatch(p), zero.getTrainBatch(p)
        assert sorted(a) == sorted(b) and 'img_regions' not in b
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
        if reg is not None:
            c = reg.getTrainBatch(p)
            assert sorted(c) == sorted(list(a) + ['img_regions'])
            for k in a:
                if k != 'img_feat':
                    assert a[k].tobytes() == c[k].tobytes(), k
            live = np.arange(9)[None, :] < c['img_regions'][:, None]
            assert np.array_equal(c['img_feat'].reshape(-1, 9, 16)[live], a['img_feat'].reshape(-1, 9, 16)[live])


# ------------------------------------------------------------------------------------------------------------ -imgRegions
def test_the_flag_its_default_and_where_it_is_declared(capsys):
    assert opts.parse([])['imgRegions'] == 0
    assert 'imgRegions' not in {k for k, _, _ in opts.OPTIONS}                      # OPTIONS mirrors opts.lua
    src = open(os.path.join(ROOT, 'visdial_amd', 'opts.py')).read()
    assert src.index("'-denseRows'") < src.index("'-imgRegions'") < src.index('vars(ap.parse_args(argv))')
    plain = opts.parse(['-encoder', 'mn-att-ques-im-hist', '-host', 'native'])
    assert plain['imgRegions'] == 0 and plain['imgSpatialSize'] == 14 and 'imgRegions' not in capsys.readouterr().out
    o = opts.parse(['-encoder', 'mn-att-ques-im-hist', '-host', 'native', '-imgRegions', '100', '-imgFeatureSize', '2048'])
    assert o['imgRegions'] == 100 and o['imgSpatialSize'] == 10 and o['imgNorm'] == 0
    assert '-imgRegions 100: imgSpatialSize = 10' in capsys.readouterr().out
    assert opts.parse(['-encoder', 'lf-att-ques-im-hist', '-host', 'native', '--imgRegions', '36'])['imgSpatialSize'] == 6
    import train
    assert train._plain(dict(imgRegions=9))['imgRegions'] == 9                      # saved in modelParams
    kept = open(os.path.join(ROOT, 'train.py')).read()
    assert "'imgRegions'" in kept and 'apply_img_regions' in kept                   # on -loadPath it comes from the command line


@pytest.mark.parametrize("argv,words", [
    (['-imgRegions', '-1'], '-imgRegions -1 must be an integer >= 0'),
    (['-imgRegions', '-3', '-encoder', 'mn-att-ques-im-hist', '-host', 'native'], '-imgRegions -3 must be an integer >= 0'),
    (['-imgRegions', '9', '-encoder', 'mn-ques-im-hist', '-host', 'native'], '-imgRegions 9 with -encoder mn-ques-im-hist: a region count per image masks the image attention'),
    (['-imgRegions', '9', '-encoder', 'hrea-ques-im-hist', '-host', 'native'], '-imgRegions 9 with -encoder hrea-ques-im-hist'),
    (['-imgRegions', '9', '-host', 'native'], '-imgRegions 9 with -encoder lf-ques-hist'),
    (['-imgRegions', '9', '-encoder', 'mn-att-ques-im-hist'], 'use -host native'),
    (['-imgRegions', '9', '-encoder', 'lf-att-ques-im-hist', '-host', 'python'], '-imgRegions 9: the masked image attention runs in the model-level runtime only')])
def test_train_refuses_by_name_before_any_model_exists(argv, words, capsys):
    with pytest.raises(SystemExit):
        opts.parse(argv)
    assert words in capsys.readouterr().err


def test_evaluate_and_generate_take_the_flag_from_the_command_line(monkeypatch):
    import evaluate
    import generate
    assert evaluate.parse_args(['-loadPath', 'x']).imgRegions == 0 and evaluate.parse_args(['-loadPath', 'x', '-imgRegions', '9']).imgRegions == 9
    assert generate.parse_args(['-loadPath', 'x'])['imgRegions'] == 0 and generate.parse_args(['-loadPath', 'x', '-imgRegions', '36'])['imgRegions'] == 36
    with pytest.raises(SystemExit, match='-imgRegions -2 must be an integer >= 0'):
        evaluate.parse_args(['-loadPath', 'x', '-imgRegions', '-2'])
    with pytest.raises(ValueError, match='-imgRegions -2 must be an integer >= 0'):
        generate.parse_args(['-loadPath', 'x', '-imgRegions', '-2'])
    # the checkpoint's value is not what is used: the flag of this command line replaces it, and the refusals see the checkpoint's encoder
    for mod, exc in ((evaluate, SystemExit), (generate, ValueError)):
        for mp, host, words in ((dict(encoder='mn-ques-im-hist', decoder='disc', imgRegions=0), 'native', '-imgRegions 9 with -encoder mn-ques-im-hist'),
                                (dict(encoder='mn-att-ques-im-hist', decoder='gen', imgRegions=9), 'python', 'use -host native')):
            monkeypatch.setattr(mod, 'load_checkpoint', lambda path, mp=mp: {'modelParams': dict(mp)})
            monkeypatch.setattr(sys, 'argv', [mod.__name__ + '.py', '-loadPath', 'x', '-imgRegions', '9', '-host', host])
            with pytest.raises(exc, match=words):
                mod.main()


def test_train_on_a_checkpoint_takes_the_flag_from_the_command_line(monkeypatch, capsys, tmp_path):
    import train
    argv = ['train.py', '-loadPath', 'x', '-imgRegions', '9', '-host', 'native', '-inputJson', str(tmp_path / 'none.json')]
    monkeypatch.setattr(sys, 'argv', argv)
    monkeypatch.setattr(train, 'load_checkpoint', lambda path: {'modelParams': dict(encoder='mn-ques-im-hist', decoder='disc', imgNorm=1)})
    with pytest.raises(SystemExit, match='-imgRegions 9 with -encoder mn-ques-im-hist'):
        train.main()
    # the checkpoint's own imgRegions / imgSpatialSize are not what is used
    mp = dict(encoder='mn-att-ques-im-hist', decoder='disc', imgNorm=0, imgRegions=100, imgSpatialSize=10)
    monkeypatch.setattr(train, 'load_checkpoint', lambda path: {'modelParams': mp})
    with pytest.raises(SystemExit, match='-loadPath given but no dataset'):
        train.main()
    assert mp['imgRegions'] == 9 and mp['imgSpatialSize'] == 3 and '-imgRegions 9: imgSpatialSize = 3' in capsys.readouterr().out
    monkeypatch.setattr(sys, 'argv', argv[:3] + argv[5:])                            # without the flag: the grid of the checkpoint, no counts
    with pytest.raises(SystemExit, match='-loadPath given but no dataset'):
        train.main()
    assert mp['imgRegions'] == 0 and mp['imgSpatialSize'] == 3
    monkeypatch.setattr(sys, 'argv', argv[:5])                                       # -host python
    with pytest.raises(SystemExit, match='use -host native'):
        train.main()


def test_the_python_host_refuses_by_name():
    from visdial_amd.model import Model, refuse_img_regions
    refuse_img_regions({}), refuse_img_regions(dict(imgRegions=0)), refuse_img_regions(dict(imgRegions=None))
    with pytest.raises(ValueError) as e:
        Model(dict(small_params(), imgRegions=9))
    assert 'imgRegions = 9' in str(e.value) and '-host native' in str(e.value)


def test_native_model_attaches_under_the_name(monkeypatch):
    from visdial_amd import native
    seen = []
    monkeypatch.setattr(native, 'call', lambda name, *args: seen.append((name, args[1], args[3])))
    m = native.NativeModel.__new__(native.NativeModel)
    m.h = None
    m.attach_img_regions(np.asarray([1, 4, 9], np.int32))
    m.attach_img_regions([[2], [3]])
    assert seen == [('vd_model_set_tensor', b'@img_regions', 3), ('vd_model_set_tensor', b'@img_regions', 2)]
    src = open(os.path.join(ROOT, 'visdial_amd', 'native.py')).read()
    assert "batch.get('img_regions') is not None" in src and "'img_feat', 'img_regions'" in src   # upload, and the generation upload


# ------------------------------------------------------------------------------------------------------------ frozen surfaces
def test_the_frozen_surfaces_stay_frozen():
    from visdial_amd import _lib, native
    assert len(native.SWITCHES) == 13 and len(native.TRAIN_SWITCHES) == 3 and len(native.DENSE_SWITCHES) == 1
    assert native.ALL_SWITCHES == native.SWITCHES + native.TRAIN_SWITCHES + native.DENSE_SWITCHES
    assert not any('egion' in r[0] or 'REGION' in r[1] for r in native.ALL_SWITCHES)        # an attachment, not a switch
    header = open(os.path.join(ROOT, 'include', 'visdial_hip.h')).read()
    names = set(re.findall(r'\b(vd_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', header, flags=re.S)))
    assert len(names) == 101 and names == set(_lib.PROTOTYPES)
    assert re.search(r'^#define\s+VD_ABI_VERSION\s+2\s*$', header, re.M) and _lib.ABI_VERSION == 2
    read = lambda name: open(os.path.join(ROOT, 'visdial_amd', 'csrc', name)).read()
    assert 'REGION' not in read('rt_switches.h') and 'getenv' not in read('attention.hip')
    core = read('rt_core.h')
    for name in ('vd_img_att_forward_p', 'vd_img_att_backward_p'):
        assert re.search(r'^int %s\(' % name, core, re.M) and 'const int32_t* cnt' in core[core.index('int %s(' % name):][:600]
        assert name not in header
    att = read('attention.hip')
    ext = att[att.index('extern "C" {'):att.index('}  // extern "C"')]
    # the C-ABI entry points keep their signatures (the header above) and take no count: each is one call of its _p with a null cnt
    assert 'cnt' not in ext and ext.count('_p(') == 2 and 'hipLaunchKernelGGL(img_att_' not in ext
    for name in ('vd_img_att_forward', 'vd_img_att_backward'):
        assert re.search(r'return %s_p\([^;]*\bnullptr, \(hipStream_t\)stream\);' % name, ext)


def test_the_rules_stand_once_at_the_top_of_attention_hip_and_the_documents_name_the_attachment():
    read = lambda *parts: open(os.path.join(ROOT, *parts)).read()
    att = read('visdial_amd', 'csrc', 'attention.hip')
    top = att[:att.index('#include')]
    for i in range(1, 7):
        assert att.count('IR%d:' % i) == 1 and 'IR%d:' % i in top
    assert [top.index('IR%d:' % i) for i in range(1, 7)] == sorted(top.index('IR%d:' % i) for i in range(1, 7))
    # one kernel per stage under the name it always had, a nullable cnt its argument, launched from one place
    assert '_regions_kernel' not in att and 'template <bool MASKED>' not in att
    for k in ('score', 'wsum', 'dscore', 'dz'):
        decl = re.search(r'\nimg_att_%s_kernel\(([^)]*)\)' % k, att)
        assert decl and 'const int32_t* __restrict__ cnt' in decl.group(1) and 'int R' in decl.group(1)
        assert att.count('hipLaunchKernelGGL(img_att_%s_kernel,' % k) == 1
    ref = read('tests', 'region_ref.py')
    for i in range(1, 7):
        assert 'IR%d' % i in ref
    for text in (read('include', 'visdial_hip.h'), read('INTEGRATION.md'), read('README.md'), read('DESIGN.md')):
        assert '@img_regions' in text
    runtime = read('visdial_amd', 'csrc', 'runtime.hip')
    assert "(the library knows '@dense_relevance' and '@dense_relevance_live')" in runtime and "'@img_regions'" in runtime
    assert 'sl.regions = nullptr;' in runtime[runtime.index('sl.rel = nullptr;'):][:120]     # cleared where sl.rel is
    assert 'imgRegions' in read('README.md') and 'profiles/img_regions.txt' in read('README.md')
