"""The length order of generative retrieval's candidates (VD_FLAG_LIVE_PREFIX, csrc/lhood.hip lhood_order_*) without a device: a numpy
statement of the order, of the per-step prefix counts and of the "hole" that forbids the promise, checked against
oracle.visdial_oracle.compute_lhood; and the header / csrc/common.h / operator-level host agree on the flag bit and the row-group
macro while the C symbol set stays the parent's 101."""
import os
import re

import numpy as np

from conftest import ROOT


def lengths(option_in):
    """[T x rows] time-major -> (length = number of leading non-pad steps, holed = a token behind the first pad) per row"""
    tok = option_in != 0
    lens = np.cumprod(tok, axis=0).sum(0)
    return lens, tok.sum(0) != lens


def length_order(option_in):
    """descending length, ties by row index; nact[t] = rows longer than t.  What lhood_order_* computes on the device."""
    lens, holed = lengths(option_in)
    perm = np.argsort(-lens, kind='stable')
    nact = (lens[None, :] > np.arange(option_in.shape[0])[:, None]).sum(1)
    return perm, nact, bool(holed.any())


def rows_run(nact, rows, G):
    """(step, candidate) rows inside a row group of height G that holds a live row, per step"""
    return np.minimum(rows, -(-nact // G) * G)


def candidates(rs, T, lens, V):
    rows = len(lens)
    oin = np.zeros((T, rows), np.int64)
    oout = np.zeros((T, rows), np.int64)
    for r, L in enumerate(lens):
        w = rs.randint(1, V - 1, size=L)
        oin[0, r] = V - 1
        oin[1:1 + L, r] = w
        if L:
            oout[:L, r] = w
            oout[L, r] = V
    return oin, oout


def test_order_prefix_counts_and_round_trip_against_compute_lhood():
    from oracle import visdial_oracle as vo
    rs = np.random.RandomState(4)
    T, V = 9, 23
    lens = np.array([3, 0, 8, 1, 3, 0, 8, 5, 2, 3, 7, 1, 4])    # empties, full-length ones, ties
    oin, oout = candidates(rs, T, lens, V)
    rows = len(lens)
    perm, nact, holed = length_order(oin)
    assert not holed
    # ties keep their row order; the order is a permutation
    assert sorted(perm.tolist()) == list(range(rows))
    ls = (lens + 1)[perm]                                       # option_in carries <START>: its length is the answer's + 1
    assert all(ls[i] > ls[i + 1] or (ls[i] == ls[i + 1] and perm[i] < perm[i + 1]) for i in range(rows - 1))
    # in that order the live rows of every step are a prefix, and the prefixes are nested
    sin = oin[:, perm]
    for t in range(T):
        assert (sin[t, :nact[t]] != 0).all() and (sin[t, nact[t]:] == 0).all()
    assert all(nact[t] >= nact[t + 1] for t in range(T - 1)) and nact[0] == rows
    # the rows outside the prefixes are exactly the rows with option_in == 0
    outside = np.arange(rows)[None, :] >= nact[:, None]
    np.testing.assert_array_equal(outside, sin == 0)
    # a row group of any height G that is skipped holds only pad rows, and every live row lies in one that runs
    for G in (1, 4, 32, 128):
        run = rows_run(nact, rows, G)
        assert (run >= nact).all() and (run <= rows).all() and ((run % G == 0) | (run == rows)).all()
        assert int((sin != 0).sum()) <= int(run.sum()) <= T * rows
    # candidates permuted into that order and back give compute_lhood's scores
    x = rs.standard_normal((T, rows, V))
    logp = x - np.log(np.exp(x).sum(-1, keepdims=True))
    ref = vo.compute_lhood(oout, logp)
    # (contiguous like the originals: numpy picks the summation order of .sum(0) by memory layout, and the comparison is exact)
    sorted_scores = vo.compute_lhood(np.ascontiguousarray(oout[:, perm]), np.ascontiguousarray(logp[:, perm]))
    back = np.empty_like(sorted_scores)
    back[perm] = sorted_scores
    np.testing.assert_array_equal(back, ref)
    assert (ref[lens == 0] == 0.0).all()


def test_a_candidate_with_a_hole_is_recognised():
    rs = np.random.RandomState(5)
    oin, _ = candidates(rs, 7, np.array([2, 4, 0, 6]), 17)
    assert not length_order(oin)[2]
    holed = oin.copy()
    holed[1, 1] = 0                                             # <START> 0 w2 w3 w4: a pad followed by a token
    lens, h = lengths(holed)
    assert h.tolist() == [False, True, False, False] and lens[1] == 1
    assert length_order(holed)[2]
    tail = oin.copy()
    tail[6, 2] = 5                                              # a token far behind the run
    assert length_order(tail)[2]
    allpad = np.zeros((7, 3), np.int64)                         # no token at all: length 0, no hole, nothing to run
    perm, nact, h = length_order(allpad)
    assert not h and nact.tolist() == [0] * 7 and perm.tolist() == [0, 1, 2]


def test_header_common_h_and_ops_agree_on_the_flag_and_the_symbol_set_is_the_parents():
    from visdial_amd import _lib, ops
    header = open(os.path.join(ROOT, 'include', 'visdial_hip.h')).read()
    common = open(os.path.join(ROOT, 'visdial_amd', 'csrc', 'common.h')).read()

    def defines(text):
        return {k: int(v) for k, v in re.findall(r'^#define\s+(VD_[A-Z0-9_]+)\s+(\d+)\s*(?:/[/*].*)?$', text, flags=re.M)}
    h, c = defines(header), defines(common)
    flag, G = h['VD_FLAG_LIVE_PREFIX'], h['VD_LIVE_PREFIX_ROWS']
    others = [h[k] for k in ('VD_FLAG_BF16', 'VD_FLAG_SPLIT9', 'VD_FLAG_SPLIT6', 'VD_FLAG_SPLIT3')]
    assert flag > 0 and flag & (flag - 1) == 0 and all(flag & o == 0 for o in others)          # one bit, used by no other flag
    assert 0 < G <= 256 and G % 32 == 0 and G % 128 == 0                                         # a multiple of both step row tiles
    assert c['VD_FLAG_LIVE_PREFIX'] == flag and c['VD_LIVE_PREFIX_ROWS'] == G
    assert (ops.FLAG_LIVE_PREFIX, ops.LIVE_PREFIX_ROWS) == (flag, G)
    # the operator-level host's statement of the step kernels' row tile is csrc/paths.h's
    paths = open(os.path.join(ROOT, 'visdial_amd', 'csrc', 'paths.h')).read()
    big, small = map(int, re.search(r'VD_LSTM_FWD_TILE_BIG = (\d+), VD_LSTM_FWD_TILE_SMALL = (\d+)', paths).groups())
    thr = int(re.search(r'VD_THROUGHPUT_ROWS = (\d+)', paths).group(1))
    assert [ops.lstm_fwd_row_tile(n) for n in (1, thr - 1, thr, 10 * thr)] == [small, small, big, big] and G % big == 0 and G % small == 0
    text = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(re.findall(r'\b(vd_[a-z0-9_]+)\s*\(', text))
    assert len(declared) == 101 and declared == set(_lib.PROTOTYPES) and '#define VD_ABI_VERSION 2' in header
    ffi = open(os.path.join(ROOT, 'lua', 'visdial_ffi.lua')).read()
    assert set(re.findall(r"^\s*'(vd_[a-z0-9_]+)',", ffi, flags=re.M)) == declared
