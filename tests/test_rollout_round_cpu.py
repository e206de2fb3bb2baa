"""Encoding a rollout one round at a time (VD_ROLLOUT_ENCODER = round; csrc/rt_encoders.h forward_round), without a device: the flag of both
scripts and what they refuse, the C surface, and the premise the round pass rests on -- every encoder with a history is causal over the
rounds, so the output of round r does not depend on history rows > r -- on the numpy oracle in fp64."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from oracle import visdial_oracle as vo
from test_rollout_cpu import prepro_loader

HISTORY_ENCODERS = ['lf-ques-hist', 'lf-ques-im-hist', 'lf-att-ques-im-hist', 'hre-ques-hist', 'hre-ques-im-hist', 'hrea-ques-im-hist',
                    'mn-ques-hist', 'mn-ques-im-hist', 'mn-att-ques-im-hist']


def gen_setting(enc, split='val'):
    """test_rollout_gpu.setting for every encoder with a history.  The synthetic loader concatenates the history of any lf-* encoder, while
    generate.py's history is per round for all of them: lf-att-ques-im-hist takes mn-att-ques-im-hist's batch (the same shapes)."""
    from test_rollout_gpu import setting
    if enc == 'lf-att-ques-im-hist':
        p, batch, START, END = setting('mn-att-ques-im-hist', split)
        return dict(p, encoder=enc), batch, START, END
    return setting(enc, split)


# ------------------------------------------------------------------------------------------------------------ 1. the flag
def test_generate_py_takes_the_flag_and_names_what_it_refuses():
    import generate
    a = generate.parse_args(['-loadPath', 'x'])
    assert a['rolloutEncoder'] == 'full'                               # `a` is the `opts` of results.json
    on = ['-loadPath', 'x', '-rollout', '1', '-beamBatch', '4', '-host', 'native']
    assert generate.parse_args(on + ['-rolloutEncoder', 'round'])['rolloutEncoder'] == 'round'
    assert generate.parse_args(on + ['-rolloutEncoder', 'full'])['rolloutEncoder'] == 'full'
    assert generate.parse_args(['-loadPath', 'x', '-rolloutEncoder', 'full'])['rolloutEncoder'] == 'full'
    for args, needs in ((['-loadPath', 'x', '-beamBatch', '4', '-host', 'native'], '-rollout 1'),
                        (['-loadPath', 'x', '-rollout', '1', '-beamBatch', '4', '-host', 'python'], '-host python'),
                        (['-loadPath', 'x', '-rollout', '1', '-beamBatch', '0', '-host', 'native'], '-beamBatch')):
        with pytest.raises(ValueError) as e:
            generate.parse_args(args + ['-rolloutEncoder', 'round'])
        assert '-rolloutEncoder round' in str(e.value) and needs in str(e.value), e.value
    with pytest.raises(SystemExit):
        generate.parse_args(on + ['-rolloutEncoder', 'bogus'])


def test_evaluate_py_takes_the_flag_and_names_what_it_refuses():
    import evaluate
    assert evaluate.parse_args(['-loadPath', 'x']).rolloutEncoder == 'full'
    on = ['-loadPath', 'x', '-rollout', '1', '-host', 'native']
    assert evaluate.parse_args(on + ['-rolloutEncoder', 'round']).rolloutEncoder == 'round'
    assert evaluate.parse_args(['-loadPath', 'x', '-rolloutEncoder', 'full']).rolloutEncoder == 'full'
    for args, needs in ((['-loadPath', 'x', '-host', 'native'], '-rollout 1'),
                        (['-loadPath', 'x', '-rollout', '1', '-host', 'python'], '-host python')):
        with pytest.raises(SystemExit) as e:
            evaluate.parse_args(args + ['-rolloutEncoder', 'round'])
        assert '-rolloutEncoder round' in str(e.value) and needs in str(e.value), e.value
    with pytest.raises(SystemExit):
        evaluate.parse_args(on + ['-rolloutEncoder', 'bogus'])


def test_the_operator_level_host_points_to_the_native_one():
    from visdial_amd.model import Model
    p, _ = prepro_loader(('val',), 'lf-ques-im-hist')
    with pytest.raises(ValueError, match='-host native'):             # refused before anything touches a device
        Model(dict(p, rolloutEncoder='round'))


# ------------------------------------------------------------------------------------------------------------ 2. the C surface
def test_the_c_surface_is_where_it_was_and_the_variable_is_documented():
    from visdial_amd import _lib
    read = lambda *parts: open(os.path.join(ROOT, *parts)).read()
    header = read('include', 'visdial_hip.h')
    assert re.search(r'^#define\s+VD_ABI_VERSION\s+2\s*$', header, re.M) and _lib.ABI_VERSION == 2
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    names = set(re.findall(r'\b(vd_[a-z0-9_]+)\s*\(', code))
    assert len(names) == 101 and names == set(_lib.PROTOTYPES)
    for internal in ('vd_mn_attention_round_p', 'vd_hrea_attention_round_p', 'vd_round_embed_p', 'vd_rows_cat_p'):
        assert internal not in header and internal in read('visdial_amd', 'csrc', 'rt_core.h')
    for text in (header, read('visdial_amd', 'csrc', 'rt_switches.h'), read('INTEGRATION.md'), read('README.md'), read('visdial_amd', 'native.py')):
        assert 'VD_ROLLOUT_ENCODER' in text
    att = read('visdial_amd', 'csrc', 'attention.hip')
    assert 'mn_att_round_kernel' in att and 'hrea_att_round_kernel' in att
    assert 'forward_round' in read('DESIGN.md') and '-rolloutEncoder' in read('README.md')
    assert 'VD_ROLLOUT_ENCODER' not in read('lua', 'visdial_ffi.lua')  # the Lua host needs no code


# ------------------------------------------------------------------------------------------------------------ 3. the premise
@pytest.mark.parametrize("enc", HISTORY_ENCODERS)
def test_every_history_encoder_is_causal_over_the_rounds(enc):
    """fp64 oracle at the sizes of the device tests (gen_setting: the prepro fixture's 4 val dialogs, the synthetic loader for the
    attention encoders; R = 10, Th = 14, hidden 32, embedding 16, V = 51): replacing history rows > r by other tokens leaves the encoder
    output of rounds <= r exactly as it was, for every r"""
    p, batch, _, _ = gen_setting(enc)
    P = vo.init_params(enc, 'gen', p, seed=3)
    B, R, Th = batch['hist'].shape
    assert (B, R, Th) == (4, 10, 14)
    base, _ = vo.encoder_forward(enc, P, p, batch, None)
    base = base.reshape(B, R, -1)
    rng = np.random.RandomState(7)
    moved = 0
    for r in range(R - 1):
        hist = np.array(batch['hist'])
        hist[:, r + 1:] = rng.randint(1, p['vocabSize'] + 1, size=hist[:, r + 1:].shape)
        out, _ = vo.encoder_forward(enc, P, p, dict(batch, hist=hist), None)
        out = out.reshape(B, R, -1)
        assert np.array_equal(out[:, :r + 1], base[:, :r + 1]), (enc, r)
        moved += int((out[:, r + 1:] != base[:, r + 1:]).any())
    assert moved == R - 1                                              # and the later rounds do read what was replaced
