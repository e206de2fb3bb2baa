"""Generative retrieval over a prefix tree of the candidates' tokens (params fusedLhood = 2, VD_FLAG_TREE, VD_LHOOD_TREE) without a
device: the flag bit in the header, csrc/common.h, the operator-level host and the generated Lua binding, with the C symbol set where
it was (101 entry points, ABI version 2); a numpy prefix tree -- the reference for node counts and level widths the GPU tests hold
vd_model_option_rows to -- over the committed prepro fixture and over the edge cases (a duplicate, an empty candidate, a strict prefix
of another); and the refusals of evaluate.py -fusedLhood 2 before any device call."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from visdial_amd import h5lite, ops

PRE = os.path.join(ROOT, 'tests', 'golden', 'prepro')
QUES, IMG, INFO = (os.path.join(PRE, n) for n in ('visdial_data.h5', 'data_img.h5', 'visdial_params.json'))
needs_hdf5 = pytest.mark.skipif(not h5lite.available(), reason="libhdf5 not loadable on this machine")


# ------------------------------------------------------------------------------------------------------------------ the reference tree
def prefix_tree(option_in, option_out):
    """option_in / option_out [rounds x O x T] -> the forest a dictionary builds, one candidate and one step at a time: level t holds a
    node per distinct (parent node, token) among the candidates still running at step t (depth-0 parents: the round).  Returns
    (level widths, edges): edges[r] = [(level, node in level, target), ...] of candidate r, where option_in and option_out are both
    non-zero."""
    R, O, T = option_in.shape
    cur = [r // O for r in range(R * O)]                        # depth-0 parent: the candidate's round
    alive = [True] * (R * O)
    widths, edges = [], [[] for _ in range(R * O)]
    for t in range(T):                                          # level-major, candidates in order: first occurrence numbers a node
        level = {}
        for r in range(R * O):
            tok = int(option_in[r // O, r % O, t])
            if not alive[r] or tok == 0:
                alive[r] = False                                # ended: a token behind a pad starts no node
                continue
            cur[r] = level.setdefault((cur[r], tok), len(level))
            if option_out[r // O, r % O, t] != 0:
                edges[r].append((t, cur[r], int(option_out[r // O, r % O, t])))
        if not level:
            break
        widths.append(len(level))
    return widths, edges


def rows_run(widths, G):
    N = max(widths)
    return sum(min(N, -(-w // G) * G) for w in widths)


def candidates(words, T, V):
    """left-aligned candidates of one round: option_in = <START> w.. 0.., option_out = w.. <END> 0.. (none for an empty candidate)"""
    oin = np.zeros((1, len(words), T), np.int32)
    oout = np.zeros((1, len(words), T), np.int32)
    for o, w in enumerate(words):
        oin[0, o, 0] = V - 1
        oin[0, o, 1:1 + len(w)] = w
        if w:
            oout[0, o, :len(w)] = w
            oout[0, o, len(w)] = V
    return oin, oout


def test_tree_of_a_duplicate_an_empty_candidate_and_a_strict_prefix():
    from visdial_amd import prefix_tree as pt
    V, T = 30, 6
    words = [[5, 6, 7], [], [5, 6], [5, 6, 7], [5, 9], [8]]       # 0 and 3 duplicates, 1 empty, 2 a strict prefix of 0, 4 shares one token
    oin, oout = candidates(words, T, V)
    widths, edges = prefix_tree(oin, oout)
    # <START> | 5, 8 | 5 6, 5 9 | 5 6 7
    assert widths == [1, 2, 2, 1]
    assert pt.level_widths(oin[None]) == widths and pt.well_formed(oin)
    assert edges[0] == edges[3] and len(edges[0]) == 4             # the duplicates walk the same nodes with the same targets
    assert edges[1] == []                                          # the empty candidate has no edge: it scores 0
    assert [e[:2] for e in edges[2]] == [e[:2] for e in edges[0][:3]]       # the prefix walks the first nodes of the longer one ...
    assert edges[2][2][2] == V and edges[0][2][2] == 7             # ... and leaves it by another target (<END> against the next word)
    assert sum(widths) == 6 and int((oin != 0).sum()) == 17
    st = pt.stats(oin[None])
    assert (st['nodes'], st['live'], st['executed']) == (6, 17, rows_run(widths, 32))
    # a second round with the same candidates shares nothing with the first: the roots differ
    two = np.concatenate([oin, oin], 0)
    assert pt.level_widths(two[None]) == [2 * w for w in widths]
    # a token behind a pad: no tree (the runtime takes the length-ordered path)
    holed = oin.copy()
    holed[0, 0, 2] = 0
    assert not pt.well_formed(holed)


def test_rows_run_formula():
    from visdial_amd import prefix_tree as pt
    assert pt.rows_run([3, 40, 203, 97, 31]) == 32 + 64 + 203 + 128 + 32          # N = 203 < 2048: 32-row tiles, capped at N
    assert pt.rows_run([200, 2300, 4200, 1500, 129]) == 256 + 2304 + 4200 + 1536 + 256   # 128-row tiles
    assert pt.rows_run([]) == 0
    assert ops.lstm_fwd_row_tile(203) == 32 and ops.lstm_fwd_row_tile(4200) == 128


@needs_hdf5
def test_tree_of_the_committed_val_batch():
    """the committed prepro fixture, split val, a gen batch of 3 dialogs: 10 606 distinct prefixes for 15 480 live (candidate, step)
    rows -- the dictionary tree and the vectorised one of the package agree on every level"""
    from visdial_amd import prefix_tree as pt
    from visdial_amd.dataloader import Dataloader
    from visdial_amd.opts import default_params, derive
    opt = derive(default_params(encoder='lf-ques-im-hist', decoder='gen', batchSize=3, inputQues=QUES, inputImg=IMG, inputJson=INFO))
    dl = Dataloader(seed=1).initialize(opt, ['val'])
    batch, _ = dl.getTestBatch(1, opt, 'val')
    oin, oout = np.asarray(batch['option_in']), np.asarray(batch['option_out'])
    B, R, O, T = oin.shape
    assert B == 3 and pt.well_formed(oin)
    widths, edges = prefix_tree(oin.reshape(B * R, O, T), oout.reshape(B * R, O, T))
    live = int((oin != 0).sum())
    print('val batch of 3 dialogs: %d nodes for %d live rows (%.2f), level widths %s' % (sum(widths), live, sum(widths) / live, widths))
    assert (sum(widths), live) == (10606, 15480)
    assert pt.level_widths(oin) == widths
    assert widths[0] == B * R                                      # every candidate of a round starts with <START>: one node per round
    assert sum(len(e) for e in edges) == int(((oin != 0) & (oout != 0)).sum())


# ------------------------------------------------------------------------------------------------------------------ the surface
def test_flag_value_everywhere_and_the_symbol_set_where_it_was():
    header = open(os.path.join(ROOT, 'include', 'visdial_hip.h')).read()
    common = open(os.path.join(ROOT, 'visdial_amd', 'csrc', 'common.h')).read()
    lua = open(os.path.join(ROOT, 'lua', 'visdial_ffi.lua')).read()
    assert re.search(r'^#define\s+VD_FLAG_TREE\s+64\s*$', header, re.M)
    assert re.search(r'^#define\s+VD_FLAG_TREE\s+64\s*$', common, re.M)
    assert 'static const int VD_FLAG_TREE = 64;' in lua
    assert ops.FLAG_TREE == 64
    others = ops.FLAG_BF16 | ops.FLAG_SPLIT9 | ops.FLAG_SPLIT6 | ops.FLAG_SPLIT3 | ops.FLAG_LIVE_PREFIX | ops.FLAG_STATE_ONLY
    assert ops.FLAG_TREE & others == 0
    assert re.search(r'^#define\s+VD_ABI_VERSION\s+2\s*$', header, re.M)
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    names = set(re.findall(r'\b(vd_[a-z0-9_]+)\s*\(', code))
    assert len(names) == 101
    assert names == set(re.findall(r"^\s+'(vd_[a-z0-9_]+)',$", lua, re.M))
    # the new functions of the library are internal: not in the header, not extern "C"
    for name in ('vd_lhood_lse_p', 'vd_lhood_edge_sum_p'):
        assert name not in names
    # the switch is an environment variable read at create, documented where VD_OPTION_CACHE is
    assert 'VD_LHOOD_TREE' in header and 'VD_LHOOD_TREE' in open(os.path.join(ROOT, 'visdial_amd', 'csrc', 'rt_switches.h')).read()


def test_ops_lstm_forward_checks_the_two_plane_mask_before_the_library_call():
    class T2(object):
        def numel(self):
            return 7
    with pytest.raises(ValueError, match=r"FLAG_TREE takes a two-plane tok_mask"):
        ops.lstm_forward(None, None, None, None, None, 2, 3, 32, 0, 128, tok_mask=T2(), flags=ops.FLAG_TREE)


# ------------------------------------------------------------------------------------------------------------------ the hosts
def checkpoint(tmp_path, decoder):
    import torch
    from visdial_amd.opts import default_params
    mp = {k: v for k, v in default_params(encoder='lf-ques', decoder=decoder).items() if isinstance(v, (int, float, str, bool))}
    path = str(tmp_path / ('%s.pt' % decoder))
    torch.save({'modelW': torch.zeros(4), 'modelParams': mp, 'optims': {'learningRate': 1e-3}}, path)
    return path


def run_evaluate(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'evaluate.py')] + list(args), capture_output=True, text=True, timeout=300, cwd=ROOT)


def test_evaluate_py_refuses_the_tree_for_disc_and_for_the_python_host_before_any_device_call(tmp_path):
    r = run_evaluate('-h')
    assert r.returncode == 0 and re.search(r'fusedLhood \{0,1,2\}', r.stdout), r.stdout[-2000:]
    r = run_evaluate('-loadPath', checkpoint(tmp_path, 'disc'), '-fusedLhood', '2', '-host', 'native')
    assert r.returncode != 0 and '-fusedLhood 2' in r.stderr and 'generative' in r.stderr, r.stderr[-2000:]
    gen = checkpoint(tmp_path, 'gen')
    for host in (['-host', 'python'], []):                           # python is the default host
        r = run_evaluate('-loadPath', gen, '-fusedLhood', '2', *host)
        assert r.returncode != 0 and '-fusedLhood 2' in r.stderr and '-host native' in r.stderr, r.stderr[-2000:]
        assert 'Traceback' not in r.stderr and 'Evaluating' not in r.stdout


def test_operator_level_host_names_the_mode_and_the_native_host():
    from visdial_amd.model import Model
    with pytest.raises(ValueError, match=r"fusedLhood = 2.*-host native"):
        Model({'encoder': 'lf-ques', 'decoder': 'gen', 'fusedLhood': 2})
