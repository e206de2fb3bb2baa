"""The live rounds of a dense step without a device (csrc/loss.hip DL1-DL5): dense.live_rounds against a hand-written table,
dense.live_option_tokens against a plain loop, the -denseRows flag of train.py with its defaults and refusals, the frozen switch tables
and header, and the places that document '@dense_relevance_live'."""
import os
import re
import sys

import numpy as np
import pytest

from visdial_amd import dense

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(ROOT, 'tests', 'golden', 'dense', 'train_dense_sample.json')


# ------------------------------------------------------------------------------------------------------------ DL1
def table():
    """six rounds: annotated | not annotated | annotated | k = 0 | not annotated | annotated with one relevant candidate"""
    rel = np.zeros((6, 4), np.float32)
    rel[0] = [0.5, 0.0, 1.0, 0.0]
    rel[1] = -1.0
    rel[2] = [0.2, 0.2, 0.2, 0.2]
    rel[4] = -1.0
    rel[5] = [0.0, 0.0, 0.0, 0.4]
    return rel


def test_live_rounds_against_a_hand_written_table():
    rel = table()
    assert dense.live_rounds(rel, 0.0).tolist() == [0, 2, 5]                        # mu = 0: the annotated rounds with a relevant candidate
    assert dense.live_rounds(rel, 0.5).tolist() == [0, 1, 2, 4, 5]                  # mu > 0: the rounds without an annotation too; never k = 0
    assert dense.live_rounds(rel, 1.0).tolist() == [0, 1, 2, 4, 5]
    assert dense.live_rounds(rel[[0, 2, 5]], 0.0).tolist() == [0, 1, 2]             # all live
    assert dense.live_rounds(rel[[1, 4]], 0.25).tolist() == [0, 1]                  # all live through the mix
    assert dense.live_rounds(rel[[1, 3, 4, 5]], 0.0).tolist() == [3]                # one live
    assert dense.live_rounds(rel[[1, 3, 4]], 0.0).tolist() == []                    # W = 0: the step refuses it
    assert dense.live_rounds(rel, 0.0).dtype == np.int64
    # the live rounds are the rounds of weight > 0 of DT3, whatever the ground truth
    for mix in (0.0, 0.5):
        _, w = dense.dense_targets(rel, [0, 1, 2, 3, 0, 1], mix)
        assert dense.live_rounds(rel, mix).tolist() == np.nonzero(w > 0)[0].tolist()
    bad = table()
    bad[1, 2] = 0.5
    with pytest.raises(ValueError, match='relevance row 1 is neither annotated'):
        dense.live_rounds(bad, 0.0)
    with pytest.raises(ValueError, match='must be a finite real in'):
        dense.live_rounds(rel, 2.0)


# ------------------------------------------------------------------------------------------------------------ DL3: the compaction
@pytest.mark.parametrize("with_uid", [False, True], ids=['own-rows', 'uid'])
@pytest.mark.parametrize("live", [[0], [5], [0, 2, 3, 5], [1, 4]], ids=str)
def test_live_option_tokens_against_a_plain_loop(with_uid, live):
    rng = np.random.RandomState(len(live) + 7 * with_uid)
    N, O, To = 6, 5, 3
    if with_uid:
        rows = 11                                                                   # distinct rows of the upload
        uid = rng.randint(0, rows, size=N * O).astype(np.int32)
    else:
        rows, uid = N * O, None
    tok = rng.randint(0, 50, size=(To, rows)).astype(np.int32)
    got = dense.live_option_tokens(tok, uid, live, O)
    want = np.zeros((To, len(live) * O), np.int32)
    for t in range(To):
        for s, n in enumerate(live):
            for o in range(O):
                c = n * O + o
                want[t, s * O + o] = tok[t, uid[c] if with_uid else c]
    assert got.dtype == np.int32 and got.shape == want.shape and got.flags['C_CONTIGUOUS'] and np.array_equal(got, want)


def test_live_option_tokens_of_every_round_is_the_upload():
    tok = np.arange(24, dtype=np.int32).reshape(2, 12)
    assert np.array_equal(dense.live_option_tokens(tok, None, range(4), 3), tok)
    assert dense.live_option_tokens(tok, None, [], 3).shape == (2, 0)


# ------------------------------------------------------------------------------------------------------------ -denseRows
def test_dense_rows_parses_defaults_to_all_and_stays_out_of_the_reference_flags():
    from visdial_amd import opts
    assert opts.parse([])['denseRows'] == 'all'
    dense_run = ['-denseAnnotations', TRAIN, '-decoder', 'disc', '-host', 'native']
    assert opts.parse(dense_run)['denseRows'] == 'all'
    o = opts.parse(dense_run + ['-denseRows', 'live'])
    assert o['denseRows'] == 'live' and o['denseAnnotations'] == TRAIN
    assert opts.parse(dense_run + ['--denseRows', 'all'])['denseRows'] == 'all'
    assert 'denseRows' not in {k for k, _, _ in opts.OPTIONS}                       # OPTIONS mirrors opts.lua
    opts.check_dense_rows({}), opts.check_dense_rows(dict(denseRows='all', lstmPrecision='bf16')), opts.check_dense_rows(dict(denseRows=None))
    opts.check_dense_rows(dict(denseRows='live', denseAnnotations=TRAIN, lstmPrecision='split9'))
    src = open(os.path.join(ROOT, 'train.py')).read()
    kept = re.search(r"for k in \('numEpochs'.*?\):", src, re.S).group(0)           # a resumed run takes it from the command line
    assert "'denseRows'" in kept and 'check_dense_rows' in src and 'option_rows' in src
    import train
    assert train._plain(dict(denseRows='live'))['denseRows'] == 'live'              # saved in modelParams


@pytest.mark.parametrize("argv, words", [
    (['-denseRows', 'live'], '-denseRows live without -denseAnnotations'),
    (['-denseRows', 'live', '-decoder', 'disc', '-host', 'native'], '-denseRows live without -denseAnnotations'),
    (['-denseRows', 'live', '-denseAnnotations', TRAIN, '-decoder', 'disc', '-host', 'native', '-lstmPrecision', 'bf16'],
     '-denseRows live with -lstmPrecision bf16'),
    (['-denseRows', 'some'], "argument -denseRows/--denseRows: invalid choice: 'some'")])
def test_dense_rows_refusals_by_name(capsys, argv, words):
    from visdial_amd import opts
    with pytest.raises(SystemExit):
        opts.parse(argv)
    assert words in capsys.readouterr().err


def test_the_operator_level_host_refuses_live_rows_by_name(monkeypatch):
    from visdial_amd.model import refuse_dense_training
    refuse_dense_training(dict(denseRows='all')), refuse_dense_training(dict(denseRows=None)), refuse_dense_training({})
    with pytest.raises(ValueError) as e:
        refuse_dense_training(dict(denseAnnotations='a.json', denseRows='live'))
    assert "denseRows = 'live'" in str(e.value) and '-host native' in str(e.value)
    import train
    monkeypatch.setattr(sys, 'argv', ['train.py', '-denseAnnotations', TRAIN, '-decoder', 'disc', '-denseRows', 'live'])   # -host python
    with pytest.raises(SystemExit) as e:
        train.main()
    assert "denseRows = 'live'" in str(e.value) and '-host native' in str(e.value)
    with pytest.raises(ValueError, match="-denseRows 'rows' must be 'all' or 'live'"):
        from visdial_amd import opts
        opts.check_dense_rows(dict(denseRows='rows'))


def test_native_attaches_under_the_live_name_only_when_asked(monkeypatch):
    from visdial_amd import native
    seen = []
    monkeypatch.setattr(native, 'call', lambda name, *args: seen.append((name, args[1])))
    m = native.NativeModel.__new__(native.NativeModel)
    m.h = None
    rel = np.zeros((2, 3), np.float32)
    m.attach_dense_relevance(rel)
    m.attach_dense_relevance(rel, live=False)
    m.attach_dense_relevance(rel, live=True)
    assert seen == [('vd_model_set_tensor', b'@dense_relevance'), ('vd_model_set_tensor', b'@dense_relevance'),
                    ('vd_model_set_tensor', b'@dense_relevance_live')]


# ------------------------------------------------------------------------------------------------------------ frozen surfaces
def test_the_frozen_tables_and_the_101_header_names_still_hold():
    from visdial_amd import _lib, native
    assert len(native.SWITCHES) == 13 and len(native.TRAIN_SWITCHES) == 3
    assert tuple(r[:2] for r in native.DENSE_SWITCHES) == (('denseMix', 'VD_DENSE_MIX'),)
    assert native.ALL_SWITCHES == native.SWITCHES + native.TRAIN_SWITCHES + native.DENSE_SWITCHES
    assert not any('denseRows' in r[:2] or 'ROWS' in r[1] for r in native.ALL_SWITCHES)   # the live form is an attachment, not a switch
    header = open(os.path.join(ROOT, 'include', 'visdial_hip.h')).read()
    names = set(re.findall(r'\b(vd_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', header, flags=re.S)))
    assert len(names) == 101 and names == set(_lib.PROTOTYPES)
    assert re.search(r'^#define\s+VD_ABI_VERSION\s+2\s*$', header, re.M) and _lib.ABI_VERSION == 2


def test_the_documents_name_the_attachment_and_loss_hip_the_rules():
    read = lambda *parts: open(os.path.join(ROOT, *parts)).read()
    for text in (read('include', 'visdial_hip.h'), read('INTEGRATION.md'), read('README.md'), read('DESIGN.md')):
        assert '@dense_relevance_live' in text
    loss = read('visdial_amd', 'csrc', 'loss.hip')
    for word in ('DL1', 'DL2', 'DL3', 'DL4', 'DL5', 'dense_live_tokens_kernel', 'score_ce_dense_live_kernel', 'score_ce_dense_kernel',
                 'score_ce_kernel', 'score_ce_smooth_kernel'):
        assert word in loss
    assert loss.index('DT5') < loss.index('DL1') < loss.index('#include')            # stated once, behind DT5 at the top
    runtime = read('visdial_amd', 'csrc', 'runtime.hip')
    assert "the library knows '@dense_relevance' and '@dense_relevance_live'" in runtime
    assert 'VD_DENSE_ROWS' not in runtime + read('visdial_amd', 'csrc', 'rt_switches.h')   # no environment variable
