"""The twelve creation-time switches of vd_model_create (csrc/rt_switches.h) and the table NativeModel hands them over with
(visdial_amd/native.py SWITCHES): what the library sees for a params, what it refuses and with which words, and what it never reads.
vd_model_create parses the switches before it touches a device, so none of this needs one."""
import os

import pytest

from test_beam_cpu import _tiny_val

# (params key, variable): the params value goes through as str(value); optionCache and fusedLhood have their own rules (below)
KNOBS = (('optionCache', 'VD_OPTION_CACHE'), ('fusedLhood', 'VD_LHOOD_TREE'), ('topK', 'VD_SAMPLE_TOPK'), ('topP', 'VD_SAMPLE_TOPP'),
         ('beamGroups', 'VD_BEAM_GROUPS'), ('beamDiversity', 'VD_BEAM_DIVERSITY'), ('beamMinLen', 'VD_BEAM_MIN_LEN'),
         ('beamNoRepeat', 'VD_BEAM_NO_REPEAT'), ('beamLengthPenalty', 'VD_BEAM_LENGTH_PENALTY'), ('beamRollout', 'VD_BEAM_ROLLOUT'),
         ('retrieveRollout', 'VD_RETRIEVE_ROLLOUT'), ('rolloutEncoder', 'VD_ROLLOUT_ENCODER'))
NAMES = tuple(v for _, v in KNOBS)
VAR = dict(KNOBS)


@pytest.fixture(scope='module')
def params():
    return _tiny_val()[0]


class Stop(Exception):
    pass


# ------------------------------------------------------------------------------------------------------------ what the library sees
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
    unset = dict({k: None for k in NAMES}, VD_OPTION_CACHE='0', VD_LHOOD_TREE='0')
    every = dict(optionCache=3, fusedLhood=2, topK=40, topP=0.9, beamGroups=3, beamDiversity=0.25, beamMinLen=2, beamNoRepeat=3,
                 beamLengthPenalty=0.7, beamRollout=1, retrieveRollout=1, rolloutEncoder='round')
    want_every = {VAR[k]: str(v) for k, v in every.items()}
    want_every['VD_LHOOD_TREE'] = '1'
    cases = ((dict(params), unset),
             (dict(params, **every), want_every),
             (dict(params, fusedLhood=1), unset),
             (dict(params, optionCache=None), unset),
             (dict(params, optionCache=1, fusedLhood=0), dict(unset, VD_OPTION_CACHE='1')),
             (dict(params, **{k: None for k in every}), unset),                                       # None is absent
             (dict(params, topK='abc', beamGroups=0, topP=float('nan'), beamRollout='', rolloutEncoder='Round'),   # Python validates nothing
              dict(unset, VD_SAMPLE_TOPK='abc', VD_BEAM_GROUPS='0', VD_SAMPLE_TOPP='nan', VD_BEAM_ROLLOUT='', VD_ROLLOUT_ENCODER='Round')))
    for p, want in cases:
        with pytest.raises(Stop):
            native.NativeModel(p)
        assert seen[-1] == want
        assert {k: os.environ.get(k) for k in NAMES} == {k: before.get(k) for k in NAMES}              # also after a failed create
    assert len(seen) == len(cases)


# ------------------------------------------------------------------------------------------------------------ refusals
INT0 = "must be an integer >= 0 (0 = off)"
REFUSALS = []                                                                    # (decoder, knobs, fragments of the message)


def _values(decoders, key, values, tail):
    for dec in decoders:
        for v in values:
            REFUSALS.append((dec, {key: v}, ("vd_model_create: %s = '%s' %s" % (VAR[key], v, tail),)))


# always read
REFUSALS += [('gen', dict(optionCache=1), ("vd_model_create: VD_OPTION_CACHE caches the candidate encodings of decoder 'disc'; this model's "
                                           "decoder is 'gen'",)),
             ('disc', dict(optionCache=1, lstmPrecision='bf16'), ('vd_model_create: VD_OPTION_CACHE needs the state-only option recurrence',
                                                                  '(lstmBf16 = 1)')),
             ('disc', dict(optionCache=2 ** 30), ('vd_model_create: VD_OPTION_CACHE = 1073741824 rows is out of range',)),
             ('disc', dict(fusedLhood=2), ("vd_model_create: VD_LHOOD_TREE scores the candidates of decoder 'gen' over a prefix tree; this "
                                           "model's decoder is 'disc'",)),
             ('gen', dict(fusedLhood=2, lstmPrecision='bf16'), ('vd_model_create: VD_LHOOD_TREE runs the exact fp32 tree recurrence '
                                                                '(VD_FLAG_TREE)', '(lstmBf16 = 1)'))]
_values(('gen', 'disc'), 'rolloutEncoder', ('Round', '', 'rounds'), "must be 'full' or 'round' (unset = full)")
# decoder gen only
_values(('gen',), 'topK', (-1, 'abc', '5x', '', 2 ** 40), INT0)
_values(('gen',), 'topP', (0, 1.5, float('nan'), 'p', -0.5, float('inf')), "must be a real in (0, 1] (1 = off)")
_values(('gen',), 'beamGroups', (0, -1, 'x', '', 2 ** 40), "must be an integer >= 1 (1 = off)")
_values(('gen',), 'beamDiversity', (-0.1, float('nan'), float('inf'), 'x', 1e39), "must be a finite real >= 0")
_values(('gen',), 'beamMinLen', (-1, 'x', 2 ** 40), INT0)
_values(('gen',), 'beamNoRepeat', (-1, 'x', 2 ** 40), INT0)
_values(('gen',), 'beamLengthPenalty', (-1, float('nan'), float('inf'), 'x'), "must be a finite real >= 0 (0 = off)")
_values(('gen',), 'beamRollout', (2, '', 'yes', '10'), "must be 1 or 0 (0 = off)")
REFUSALS.append(('gen', dict(beamRollout=1, beamGroups=2), ('vd_model_create: VD_BEAM_ROLLOUT = 1 with VD_BEAM_GROUPS = 2: a rollout feeds ONE '
                                                            'answer per round back',)))
# decoder disc only
_values(('disc',), 'retrieveRollout', (2, ''), "must be 1 or 0 (0 = off)")
REFUSALS.append(('disc', dict(retrieveRollout=1, optionCache=1), ('vd_model_create: VD_RETRIEVE_ROLLOUT = 1 with VD_OPTION_CACHE: a cached '
                                                                  'batch carries only the candidate rows the cache did not hold',)))


@pytest.mark.parametrize("decoder, knobs, fragments", REFUSALS,
                         ids=['%s-%s' % (d, '-'.join('%s=%s' % kv for kv in k.items())) for d, k, _ in REFUSALS])
def test_refusals_keep_their_words(params, decoder, knobs, fragments):
    from visdial_amd import _lib
    from visdial_amd.native import NativeModel
    before = {k: os.environ.get(k) for k in NAMES}
    with pytest.raises(_lib.VisdialHipError) as e:
        NativeModel(dict(params, decoder=decoder, **knobs))
    for f in fragments:
        assert f in str(e.value)
    assert {k: os.environ.get(k) for k in NAMES} == before


# ------------------------------------------------------------------------------------------------------------ what is ignored
def _passes_the_switches(make):
    """without a device the create fails at its first allocation, naming none of the variables; on a device it succeeds"""
    from visdial_amd import _lib
    try:
        make().close()
    except _lib.VisdialHipError as e:
        assert not [k for k in NAMES if k in str(e)], str(e)


def test_what_is_not_read_and_what_is_tolerated(monkeypatch, params):
    from visdial_amd import _lib, native
    # the sampling and beam variables and VD_BEAM_ROLLOUT are not read for decoder disc, VD_RETRIEVE_ROLLOUT not for decoder gen
    for decoder, knobs in (('disc', dict(topK='abc')), ('disc', dict(beamGroups=0)), ('disc', dict(beamRollout=2)),
                           ('disc', dict(beamLengthPenalty='x')), ('gen', dict(retrieveRollout='x')),
                           ('disc', dict(topK='abc', topP='p', beamGroups=0, beamMinLen=-1, beamNoRepeat='x', beamLengthPenalty='x', beamRollout=2)),
                           ('gen', dict(topK=5, topP=0.5, beamGroups=2, beamDiversity=0.0, beamMinLen=1, beamNoRepeat=2, beamLengthPenalty=0.5,
                                        beamRollout=0, rolloutEncoder='round')),
                           ('disc', dict(retrieveRollout=1, rolloutEncoder='round'))):
        _passes_the_switches(lambda: native.NativeModel(dict(params, decoder=decoder, **knobs)))
    # params optionCache / fusedLhood go through int() in Python: text never reaches the library from NativeModel
    for knobs in (dict(optionCache='abc'), dict(fusedLhood='abc')):
        with pytest.raises(ValueError, match='invalid literal'):
            native.NativeModel(dict(params, **knobs))
    # the library itself reads the two through atol: text is 0, a leading number counts, nothing is refused for its form
    real = _lib.call

    def create_with(env):
        def call(name, *args):
            if name == 'vd_model_create':
                os.environ.update(env)                                           # (NativeModel puts its own values back afterwards)
            return real(name, *args)
        return call
    for decoder, env in (('gen', {'VD_OPTION_CACHE': 'abc'}), ('gen', {'VD_OPTION_CACHE': ''}), ('gen', {'VD_OPTION_CACHE': '-5'}),
                         ('disc', {'VD_LHOOD_TREE': 'abc'}), ('disc', {'VD_LHOOD_TREE': ''}), ('disc', {'VD_LHOOD_TREE': '-1'}),
                         ('disc', {'VD_OPTION_CACHE': '2x'}), ('gen', {'VD_LHOOD_TREE': '1x'})):
        monkeypatch.setattr(native, 'call', create_with(env))
        _passes_the_switches(lambda: native.NativeModel(dict(params, decoder=decoder)))
    for decoder, env, fragment in (('gen', {'VD_OPTION_CACHE': '2x'}, "VD_OPTION_CACHE caches the candidate encodings of decoder 'disc'"),
                                   ('disc', {'VD_OPTION_CACHE': '1073741824 rows'}, 'VD_OPTION_CACHE = 1073741824 rows is out of range'),
                                   ('disc', {'VD_LHOOD_TREE': '1x'}, "VD_LHOOD_TREE scores the candidates of decoder 'gen'")):
        monkeypatch.setattr(native, 'call', create_with(env))
        with pytest.raises(_lib.VisdialHipError) as e:
            native.NativeModel(dict(params, decoder=decoder))
        assert fragment in str(e.value)
