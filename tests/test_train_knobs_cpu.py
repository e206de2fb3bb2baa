"""The training knobs without a device: tests/train_knobs_ref.py against independent implementations (torch on the CPU), what the library
sees for a params and what it refuses and with which words (vd_model_create parses its switches before it touches a device), the train.py
flags, the refusal of the operator-level host, and the frozen surfaces (thirteen SWITCHES rows, 101 declared entry points)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import train_knobs_ref as tk
from test_beam_cpu import _tiny_val

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = (('labelSmoothing', 'VD_LABEL_SMOOTHING'), ('gradClipNorm', 'VD_GRAD_CLIP_NORM'), ('weightDecay', 'VD_WEIGHT_DECAY'))
NAMES = tuple(v for _, v in KNOBS)
VAR = dict(KNOBS)


@pytest.fixture(scope='module')
def params():
    return _tiny_val()[0]


# ------------------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("K", [1, 2, 100, 5])                                   # O = 1, 2, 100 and V = 5
@pytest.mark.parametrize("eps", [0.0, 0.1, 0.6])
def test_smoothed_ce_is_torch_cross_entropy(K, eps):
    rng = np.random.RandomState(K * 7 + int(eps * 10))
    s = rng.randn(6, K) * 3
    idx = rng.randint(0, K, 6)
    x = torch.tensor(s, dtype=torch.float64, requires_grad=True)
    rows = torch.nn.functional.cross_entropy(x, torch.tensor(idx), label_smoothing=eps, reduction='none')
    rows.sum().backward()
    loss, grad = tk.smoothed_ce(s, idx, eps)
    np.testing.assert_allclose(loss, rows.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(grad, x.grad.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(tk.smooth_targets(idx, K, eps).sum(1), 1.0, rtol=1e-14)


def test_heads_follow_autograd_and_mask_their_rows():
    rng = np.random.RandomState(3)
    N, O, H, eps, gscale = 3, 4, 8, 0.2, 1.0 / 3
    optH, enc, gt = rng.randn(N, O, H), rng.randn(N, H), rng.randint(0, O, N)
    a, b = torch.tensor(optH, requires_grad=True), torch.tensor(enc, requires_grad=True)
    sc = torch.einsum('noh,nh->no', a, b)
    (torch.nn.functional.cross_entropy(sc, torch.tensor(gt), label_smoothing=eps, reduction='sum') * gscale).backward()
    r = tk.score_ce(optH, enc, gt, eps, gscale)
    np.testing.assert_allclose(r['dOptH'], a.grad.numpy(), rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(r['dEnc'], b.grad.numpy(), rtol=1e-11, atol=1e-13)
    # gen: V = 5 valid columns of ld = 8; row 1 has a pad input, row 2 a pad target, row 3 both
    V, ld = 5, 8
    x = rng.randn(5, ld)
    tok_in, target = np.array([4, 0, 3, 0, 1]), np.array([2, 3, 0, 0, 5])
    loss, grad = tk.logsoftmax_nll(x, V, tok_in, target, eps)
    t = torch.tensor(x[:, :V], requires_grad=True)
    rows = torch.nn.functional.cross_entropy(t[[0, 4]], torch.tensor([1, 4]), label_smoothing=eps, reduction='none')
    rows.sum().backward()
    np.testing.assert_allclose(loss[[0, 4]], rows.detach().numpy(), rtol=1e-12)
    np.testing.assert_allclose(grad[:, :V], t.grad.numpy(), rtol=1e-12, atol=1e-14)
    assert not loss[1:4].any() and not grad[1:4].any() and not grad[:, V:].any()


@pytest.mark.parametrize("c", [0.5, 3.0, 1e9])
def test_clip_is_torch_clip_grad_norm(c):
    rng = np.random.RandomState(5)
    parts = [rng.randn(7, 3), rng.randn(11), rng.randn(2, 2, 2)]
    ps = [torch.nn.Parameter(torch.zeros(a.shape, dtype=torch.float64)) for a in parts]
    for p, a in zip(ps, parts):
        p.grad = torch.tensor(a)
    total = float(torch.nn.utils.clip_grad_norm_(ps, c))
    flat = np.concatenate([a.reshape(-1) for a in parts])
    norm = tk.grad_norm(flat, 1.0)
    assert abs(norm - total) < 1e-12 * total
    # torch divides by norm + 1e-6: the same scale to 1e-6 relative; above c the rule leaves the gradient alone exactly
    np.testing.assert_allclose(flat * tk.clip_scale(norm, c), np.concatenate([p.grad.numpy().reshape(-1) for p in ps]), rtol=2e-6)
    assert tk.clip_scale(norm, c) == (1.0 if c > norm else c / norm)


def test_clip_rule_edges_and_the_update():
    assert tk.clip_scale(2.0, 2.0) == 1.0 and tk.clip_scale(2.0, 0.0) == 1.0 and tk.clip_scale(4.0, 2.0) == 0.5
    assert tk.clip_scale(float('inf'), 2.0) == 1.0 and tk.clip_scale(float('nan'), 2.0) == 1.0
    rng = np.random.RandomState(1)
    w, g, m, v = rng.randn(9), rng.randn(9) * 4, rng.randn(9) * 0.1, rng.rand(9) * 0.1
    plain = tk.clip_decay_adam(w, g, m, v, 0.5, 1e-3)
    norm = np.linalg.norm(0.5 * g)
    clipped = tk.clip_decay_adam(w, g, m, v, 0.5, 1e-3, c=norm / 4)
    scaled = tk.clip_decay_adam(w, g, m, v, 0.5 / 4, 1e-3)
    for a, b in zip(clipped[:4], scaled[:4]):                                     # GC2: a clip is a smaller gscale
        np.testing.assert_allclose(a, b, rtol=1e-14)
    assert clipped[4] == pytest.approx(norm) and clipped[5] == pytest.approx(0.25)
    decayed = tk.clip_decay_adam(w, g, m, v, 0.5, 1e-3, decay=1e-3 * 0.1)
    np.testing.assert_allclose(decayed[0], plain[0] - 1e-4 * w, rtol=1e-14)       # WD1
    for a, b in zip(decayed[1:4], plain[1:4]):
        assert np.array_equal(a, b)
    g[3] = np.inf                                                                 # a non-finite norm clips nothing and spreads no NaN
    out = tk.clip_decay_adam(w, g, m, v, 0.5, 1e-3, c=1.0)
    assert out[5] == 1.0 and all(np.isfinite(a).all() for a in out[:4]) and out[1][3] == 5.0


# ------------------------------------------------------------------------------------------------------------ what the library sees
class Stop(Exception):
    pass


@pytest.mark.parametrize("before", [{}, {k: 'before-%d' % i for i, k in enumerate(NAMES)}], ids=['unset', 'preset'])
def test_what_the_library_sees_and_the_environment_comes_back(monkeypatch, params, before):
    from visdial_amd import native
    for k in NAMES:
        monkeypatch.delenv(k, raising=False)
    for k, v in before.items():
        monkeypatch.setenv(k, v)
    seen = []

    def fake_call(name, *args):
        assert name == 'vd_model_create'
        seen.append({k: os.environ.get(k) for k in NAMES})
        raise Stop()
    monkeypatch.setattr(native, 'call', fake_call)
    unset = {k: None for k in NAMES}
    cases = ((dict(params), unset),
             (dict(params, labelSmoothing=0.1, gradClipNorm=2.5, weightDecay=0.01),
              dict(VD_LABEL_SMOOTHING='0.1', VD_GRAD_CLIP_NORM='2.5', VD_WEIGHT_DECAY='0.01')),
             (dict(params, labelSmoothing=0.0, gradClipNorm=0, weightDecay=None),                      # None is absent, 0 is written out
              dict(unset, VD_LABEL_SMOOTHING='0.0', VD_GRAD_CLIP_NORM='0')),
             (dict(params, decoder='disc', labelSmoothing=0.2), dict(unset, VD_LABEL_SMOOTHING='0.2')),   # both decoders
             (dict(params, labelSmoothing='x', gradClipNorm=float('nan'), weightDecay=''),             # Python validates nothing
              dict(VD_LABEL_SMOOTHING='x', VD_GRAD_CLIP_NORM='nan', VD_WEIGHT_DECAY='')))
    for p, want in cases:
        with pytest.raises(Stop):
            native.NativeModel(p)
        assert seen[-1] == want
        assert {k: os.environ.get(k) for k in NAMES} == {k: before.get(k) for k in NAMES}
    assert len(seen) == len(cases)


def test_the_rows_chain_behind_the_thirteen():
    from visdial_amd import native
    assert len(native.SWITCHES) == 13 and native.SWITCHES[-1][:2] == ('rolloutConcatEnd', 'VD_ROLLOUT_CONCAT_END')
    assert tuple(r[:2] for r in native.TRAIN_SWITCHES) == KNOBS
    assert all(len(r) == len(native.SWITCHES[0]) and r[5] is None for r in native.TRAIN_SWITCHES)


# ------------------------------------------------------------------------------------------------------------ refusals
REAL0 = "must be a finite real >= 0 (0 = off)"
REFUSALS = [(dec, key, v, tail)
            for dec in ('gen', 'disc')
            for key, values, tail in (('labelSmoothing', (-0.1, 1, 1.5, float('nan'), 'x', '', 0.99999999), "must be a real in [0, 1) (0 = off)"),
                                      ('gradClipNorm', (-1, float('nan'), float('inf'), 'x'), REAL0),
                                      ('weightDecay', (-1, float('nan'), float('inf'), 'x'), REAL0))
            for v in values]


@pytest.mark.parametrize("decoder, key, value, tail", REFUSALS, ids=['%s-%s=%s' % r[:3] for r in REFUSALS])
def test_refusals_keep_their_words(params, decoder, key, value, tail):
    from visdial_amd import _lib
    from visdial_amd.native import NativeModel
    before = {k: os.environ.get(k) for k in NAMES}
    with pytest.raises(_lib.VisdialHipError) as e:
        NativeModel(dict(params, decoder=decoder, **{key: value}))
    assert "vd_model_create: %s = '%s' %s" % (VAR[key], value, tail) in str(e.value)
    assert {k: os.environ.get(k) for k in NAMES} == before


def test_what_passes_the_switches(params):
    """without a device the create fails at its first allocation, naming none of the variables; on a device it succeeds"""
    from visdial_amd import _lib
    from visdial_amd.native import NativeModel
    for decoder in ('gen', 'disc'):
        for knobs in (dict(labelSmoothing=0, gradClipNorm=0, weightDecay=0), dict(labelSmoothing=0.999, gradClipNorm=1e30, weightDecay=1e-4),
                      dict(labelSmoothing='1e-1', gradClipNorm='5', weightDecay='0.0')):
            try:
                NativeModel(dict(params, decoder=decoder, **knobs)).close()
            except _lib.VisdialHipError as e:
                assert not [k for k in NAMES if k in str(e)], str(e)


# ------------------------------------------------------------------------------------------------------------ train.py
@pytest.mark.parametrize("flag, value, words", [
    ('-labelSmoothing', '-0.1', '-labelSmoothing -0.1 must be a real in [0, 1) (0 = off)'),
    ('-labelSmoothing', '1', '-labelSmoothing 1.0 must be a real in [0, 1) (0 = off)'),
    ('-labelSmoothing', 'nan', '-labelSmoothing nan must be a real in [0, 1) (0 = off)'),
    ('-labelSmoothing', '0.99999999', '-labelSmoothing 0.99999999 must be a real in [0, 1) (0 = off)'),   # 1.0f in fp32, as the library reads it
    ('-labelSmoothing', 'x', "argument -labelSmoothing/--labelSmoothing: invalid float value: 'x'"),
    ('-gradClipNorm', '-1', '-gradClipNorm -1.0 must be a finite real >= 0 (0 = off)'),
    ('-gradClipNorm', 'inf', '-gradClipNorm inf must be a finite real >= 0 (0 = off)'),
    ('-weightDecay', 'nan', '-weightDecay nan must be a finite real >= 0 (0 = off)'),
    ('-weightDecay', 'x', "argument -weightDecay/--weightDecay: invalid float value: 'x'")])
def test_train_flags_refuse_by_name(capsys, flag, value, words):
    from visdial_amd import opts
    with pytest.raises(SystemExit):
        opts.parse([flag + '=' + value])
    assert words in capsys.readouterr().err


def test_train_flags_reach_the_params_and_stay_out_of_the_reference_table():
    from visdial_amd import opts
    o = opts.parse([])
    assert (o['labelSmoothing'], o['gradClipNorm'], o['weightDecay']) == (0.0, 0.0, 0.0)
    o = opts.parse(['-labelSmoothing', '0.1', '-gradClipNorm', '10', '-weightDecay', '1e-4', '-host', 'native'])
    assert (o['labelSmoothing'], o['gradClipNorm'], o['weightDecay']) == (0.1, 10.0, 1e-4)
    assert not {k for k, _, _ in opts.OPTIONS} & set(VAR)                          # OPTIONS mirrors opts.lua
    src = open(os.path.join(ROOT, 'train.py')).read()
    kept = re.search(r"for k in \('numEpochs'.*?\):", src, re.S).group(0)          # on -loadPath they come from the command line
    assert all("'%s'" % k in kept for k in VAR)


@pytest.mark.parametrize("key", list(VAR))
def test_the_operator_level_host_refuses_a_knob_by_name(monkeypatch, capsys, key):
    from visdial_amd.model import refuse_training_knobs
    refuse_training_knobs({}), refuse_training_knobs({k: 0 for k in VAR}), refuse_training_knobs({k: None for k in VAR})
    for v in (0.1, 'x'):
        with pytest.raises(ValueError) as e:
            refuse_training_knobs({key: v})
        assert ('%s = %r' % (key, v)) in str(e.value) and '-host native' in str(e.value)
    # train.py -host python (the default): refused before a dataloader or a model exists
    import train
    monkeypatch.setattr(sys, 'argv', ['train.py', '-' + key, '0.25'])
    with pytest.raises(SystemExit) as e:
        train.main()
    assert ('%s = 0.25' % key) in str(e.value) and '-host native' in str(e.value)


# ------------------------------------------------------------------------------------------------------------ frozen surfaces
def test_the_header_still_declares_101_names_and_the_abi_version():
    from visdial_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'visdial_hip.h')).read()
    names = set(re.findall(r'\b(vd_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', header, flags=re.S)))
    assert len(names) == 101 and names == set(_lib.PROTOTYPES)
    assert re.search(r'^#define\s+VD_ABI_VERSION\s+2\s*$', header, re.M) and _lib.ABI_VERSION == 2
    for v in NAMES:
        assert v in header
