"""Top-k / nucleus truncation of answer sampling (params topK / topP, generate.py -topK / -topP) without a device: the host rule
`split_eval.truncated_weights` on crafted rows, the per-dialog loop over numpy stand-ins for the device steps, generate.py's argument
handling and NativeModel's handling of VD_SAMPLE_TOPK / VD_SAMPLE_TOPP around vd_model_create."""
import os

import numpy as np
import pytest

from test_beam_cpu import _tiny_val
from test_sample_cpu import _host
from visdial_amd.split_eval import truncated_weights

# twelve columns, probabilities that are exact ties as fp32 logs; order: 1 2 | 3 4 5 | 0 6 7 8 | 9 | 10 11
PROBS = np.array([0.05, 0.2, 0.2, 0.1, 0.1, 0.1, 0.05, 0.05, 0.05, 0.04, 0.03, 0.03])
ROW = np.log(PROBS).astype(np.float32)


def kept(w):
    return sorted(np.nonzero(w)[0].tolist())


def test_off_returns_the_weights_bit_for_bit():
    rng = np.random.RandomState(0)
    for T in (0.3, 1.0, 2.5):
        lp = (rng.standard_normal(300) * 3).astype(np.float32)
        lp[5] = -np.inf
        want = np.exp(lp.astype(np.float64) / T)                # split_eval.py's weights before this feature
        got = truncated_weights(lp, T, 0, 1.0)
        assert got.dtype == np.float64 and np.array_equal(got, want)
        assert np.array_equal(truncated_weights(lp, T), want)


@pytest.mark.parametrize("k, p, want", [
    (2, 1.0, [1, 2]),
    (1, 1.0, [1]),                                              # a tie for the first place: the lower index
    (4, 1.0, [1, 2, 3, 4]),                                     # a tie at the k-th place: the lower indices of 3 4 5
    (7, 1.0, [0, 1, 2, 3, 4, 5, 6]),                            # ... of 0 6 7 8
    (12, 1.0, list(range(12))),                                 # k = V
    (100, 1.0, list(range(12))),                                # k > V
    (0, 1e-6, [1]),                                             # p so small that one token survives
    (0, 0.55, [1, 2, 3, 4]),                                    # sums .2 .4 .5 .6: the boundary falls inside the run 3 4 5
    (0, 0.3999, [1, 2]),
    (0, 0.4001, [1, 2, 3]),
    (4, 0.9, [1, 2, 3, 4]),                                     # S_k = .6, target .54
    (5, 0.5, [1, 2]),                                           # S_k = .7, target .35: p is taken of the top-k mass
    (3, 0.999, [1, 2, 3]),
])
def test_crafted_rows(k, p, want):
    for T in ((1.0, 0.5) if p == 1.0 else (1.0,)):              # the nucleus sets are worked out for T = 1; top-k ignores T
        w = truncated_weights(ROW, T, k, p)
        full = np.exp(ROW.astype(np.float64) / T)
        assert kept(w) == want, (T, kept(w))
        assert np.array_equal(w[want], full[want])              # survivors keep their weight, bit for bit
    if k >= 12 and p == 1.0:
        assert np.array_equal(truncated_weights(ROW, 0.7, k, p), np.exp(ROW.astype(np.float64) / 0.7))


def test_rows_with_minus_infinity_and_underflow():
    with np.errstate(divide='ignore'):
        lp = np.log(np.array([0.5, 0, 0.25, 0, 0, 0.25, 0, 0, 0, 0, 0, 0])).astype(np.float32)     # -inf where the probability is 0
    assert kept(truncated_weights(lp, 1.0, 5, 1.0)) == [0, 2, 5]     # top-5 holds two -inf columns: weight 0, never drawn
    assert kept(truncated_weights(lp, 1.0, 2, 1.0)) == [0, 2]
    assert kept(truncated_weights(lp, 1.0, 0, 0.99)) == [0, 2, 5]
    assert kept(truncated_weights(lp, 1.0, 0, 0.7)) == [0, 2]
    assert kept(truncated_weights(lp, 1.0, 0, 0.45)) == [0]
    # w == 0 columns are never part of the nucleus: a target that rounding puts past the last positive weight stops there
    assert kept(truncated_weights(lp, 1.0, 0, 1.0 - 2.0 ** -53)) == [0, 2, 5]
    # every weight underflows (today's failure): nothing is kept, the draw fails as it does without truncation
    w = truncated_weights(np.arange(-1, -13, -1).astype(np.float32), 1e-3, 3, 0.5)
    assert w.shape == (12,) and w.sum() == 0.0


def test_bad_knobs_are_refused():
    for k, p in ((-1, 1.0), (0, 0.0), (0, -0.1), (0, 1.5), (0, float('nan'))):
        with pytest.raises(ValueError, match='topK'):
            truncated_weights(ROW, 1.0, k, p)


# ------------------------------------------------------------------------------------------------------------ the per-dialog loop
def test_per_dialog_loop_truncates_and_is_untouched_when_off():
    p, dl = _tiny_val()
    dl.numThreads = {'val': 3}
    base = dict(sampleWords=1, beamLen=7, maxThreads=3, temperature=0.8, seed=11)
    ref = _host(p).generateAnswers(dl, 'val', base)
    assert _host(p).generateAnswers(dl, 'val', dict(base, topK=0, topP=1.0)) == ref      # the same rng calls in the same order
    assert _host(p).generateAnswers(dl, 'val', dict(base, topK=10 ** 6)) == ref          # k >= V keeps every column
    greedy = _host(p).generateAnswers(dl, 'val', dict(base, topK=1))
    assert greedy == _host(p).generateAnswers(dl, 'val', dict(base, topK=1, seed=12))    # k = 1: the arg-max whatever the draws
    assert greedy == _host(p).generateAnswers(dl, 'val', dict(base, topP=1e-9))
    assert greedy != ref

    class Spy(object):
        """every sampled token lies in the kept set of the row it was drawn from"""

        def __init__(self, h, k, pp):
            self.h, self.k, self.pp, self.rows = h, k, pp, 0
            self.step, h._gen_step = h._gen_step, self._gen_step
            self.last = None

        def _gen_step(self, tokens):
            if self.last is not None:
                for i, t in enumerate(tokens):
                    assert truncated_weights(self.last[i], 0.8, self.k, self.pp)[int(t) - 1] > 0
                    self.rows += 1
            self.last = self.step(tokens)
            return self.last

        def _begin(self):
            self.last = None
    for k, pp in ((3, 1.0), (0, 0.6), (5, 0.7)):
        h = _host(p)
        spy = Spy(h, k, pp)
        begin = h._gen_begin
        h._gen_begin = lambda rounds, begin=begin, spy=spy: (spy._begin(), begin(rounds))[1]
        out = h.generateAnswers(dl, 'val', dict(base, topK=k, topP=pp))
        assert spy.rows == 3 * 3 * 6 and out != ref


def test_generate_answers_argument_rules():
    p, dl = _tiny_val()
    for cfg in (dict(topK=5), dict(topP=0.9), dict(sampleWords=0, topK=5, topP=0.9)):
        with pytest.raises(ValueError, match='need sampleWords = 1'):
            _host(p).generateAnswers(dl, 'val', dict(cfg, maxThreads=1))
    for cfg in (dict(topK=-1), dict(topP=0.0), dict(topP=1.5)):
        with pytest.raises(ValueError, match='topK'):
            _host(p).generateAnswers(dl, 'val', dict(cfg, sampleWords=1, maxThreads=1))
    # the batched path asks the host whether its device sampler truncates with these knobs, before any device work
    asked = []
    h = _host(p)
    h._sample_truncation = lambda k, pp: asked.append((k, pp))
    h._gen_sample = None
    with pytest.raises(TypeError):
        h.generateAnswers(dl, 'val', dict(sampleWords=1, sampleBatch=2, topK=4, topP=0.5, maxThreads=1))
    assert asked == [(4, 0.5)]


# ------------------------------------------------------------------------------------------------------------ generate.py
def test_generate_py_arguments():
    import generate
    a = generate.parse_args(['-loadPath', 'x.pt', '-sampleWords', '1', '-topK', '40', '-topP', '0.9'])
    assert a['topK'] == 40 and a['topP'] == 0.9 and a['sampleWords'] == 1          # `a` is the `opts` of the results file
    d = generate.parse_args(['-loadPath', 'x.pt'])
    assert d['topK'] == 0 and d['topP'] == 1.0
    for flags in (['-topK', '5'], ['-topP', '0.5'], ['-sampleWords', '0', '-topK', '5', '-topP', '0.9'], ['-beamBatch', '2', '-topK', '3']):
        with pytest.raises(ValueError, match='-sampleWords 1'):
            generate.parse_args(['-loadPath', 'x.pt'] + flags)
    for flags in (['-topK', '-1'], ['-topP', '0'], ['-topP', '1.5'], ['-topP', 'nan']):
        with pytest.raises(ValueError, match='-topK'):
            generate.parse_args(['-loadPath', 'x.pt', '-sampleWords', '1'] + flags)


# ------------------------------------------------------------------------------------------------------------ NativeModel
class Stop(Exception):
    pass


@pytest.mark.parametrize("before", [{}, {'VD_SAMPLE_TOPK': '7', 'VD_SAMPLE_TOPP': '0.25'}])
def test_native_model_sets_and_restores_the_variables(monkeypatch, before):
    from visdial_amd import native
    p, _ = _tiny_val()
    names = ('VD_SAMPLE_TOPK', 'VD_SAMPLE_TOPP')
    for k in names:
        monkeypatch.delenv(k, raising=False)
    for k, v in before.items():
        monkeypatch.setenv(k, v)
    seen = []

    def fake_call(name, *args):
        assert name == 'vd_model_create'
        seen.append({k: os.environ.get(k) for k in names})
        raise Stop()
    monkeypatch.setattr(native, 'call', fake_call)
    for params, want in ((dict(p, topK=40, topP=0.9), {'VD_SAMPLE_TOPK': '40', 'VD_SAMPLE_TOPP': '0.9'}),
                         (dict(p, topK=0, topP=1.0), {'VD_SAMPLE_TOPK': '0', 'VD_SAMPLE_TOPP': '1.0'}),
                         (dict(p, topK='abc'), {'VD_SAMPLE_TOPK': 'abc', 'VD_SAMPLE_TOPP': None}),     # the library refuses, not Python
                         (dict(p), {'VD_SAMPLE_TOPK': None, 'VD_SAMPLE_TOPP': None})):                 # no knob: created with both unset
        with pytest.raises(Stop):
            native.NativeModel(params)
        assert seen[-1] == want
        assert {k: os.environ.get(k) for k in names} == {k: before.get(k) for k in names}               # also after a failed create
    assert len(seen) == 4


def test_create_refuses_bad_values_before_any_device_call():
    """vd_model_create validates the two variables before it touches the device, so the refusals need none"""
    from visdial_amd import _lib
    from visdial_amd.native import NativeModel
    p, _ = _tiny_val()
    for knobs, name in ((dict(topK=-1), 'VD_SAMPLE_TOPK'), (dict(topK='abc'), 'VD_SAMPLE_TOPK'), (dict(topK='5x'), 'VD_SAMPLE_TOPK'),
                        (dict(topK=''), 'VD_SAMPLE_TOPK'), (dict(topK=2 ** 40), 'VD_SAMPLE_TOPK'), (dict(topP=0), 'VD_SAMPLE_TOPP'),
                        (dict(topP=1.5), 'VD_SAMPLE_TOPP'), (dict(topP=float('nan')), 'VD_SAMPLE_TOPP'), (dict(topP='p'), 'VD_SAMPLE_TOPP'),
                        (dict(topP=-0.5), 'VD_SAMPLE_TOPP'), (dict(topK=5, topP=float('inf')), 'VD_SAMPLE_TOPP')):
        with pytest.raises(_lib.VisdialHipError, match=name) as e:
            NativeModel(dict(p, **knobs))
        assert "'%s'" % list(knobs.values())[-1] in str(e.value)                # the value is named
    try:                                                                        # good values pass the check: without a device the
        NativeModel(dict(p, topK=5, topP=0.5)).close()                          # create fails later, at its first allocation
    except _lib.VisdialHipError as e:
        assert 'VD_SAMPLE' not in str(e)
