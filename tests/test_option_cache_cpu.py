"""Answer-encoding cache of disc evaluation, the parts that need no GPU:
  * the host index (visdial_amd/option_cache.py) over the real batches the product `Dataloader` builds from tests/golden/prepro:
    misses = distinct (row, To) keys counted independently here, a second pass has none, a flush starts over, a small capacity
    never hands out a slot beyond it and still resolves every row;
  * To is part of the key;
  * the surface: `evaluate.py -optionCache`, VD_FLAG_STATE_ONLY = 32 in the header, csrc/common.h, ops.py and the generated Lua binding,
    with the symbol set and the ABI version where they were;
  * the arithmetic contract of the state-only recurrence restated in numpy: a two-slot ping-pong over the steps ends on the oracle's
    option encoding at t = To - 1."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from visdial_amd import h5lite, ops
from visdial_amd.dataloader import Dataloader
from visdial_amd.option_cache import DEFAULT_ROWS, OptionIndex
from visdial_amd.opts import default_params, derive

PRE = os.path.join(ROOT, 'tests', 'golden', 'prepro')
QUES, IMG, INFO = (os.path.join(PRE, n) for n in ('visdial_data.h5', 'data_img.h5', 'visdial_params.json'))
needs_hdf5 = pytest.mark.skipif(not h5lite.available(), reason="libhdf5 not loadable on this machine")


def split_batches(split):
    """the candidate rows [N*O x To] of every batch of 2 dialogs of a split, through the real Dataloader"""
    opt = derive(default_params(encoder='lf-ques-im-hist', decoder='disc', batchSize=2, inputQues=QUES, inputImg=IMG, inputJson=INFO))
    dl = Dataloader(seed=1).initialize(opt, [split])
    out, start, n = [], 1, dl.numThreads[split]
    while start <= n:
        b, start = dl.getTestBatch(start, opt, split)
        o = np.asarray(b['options'])
        out.append(np.ascontiguousarray(o.reshape(-1, o.shape[-1]), dtype=np.int32))
    return out


def one_pass(index, batches, seen):
    """resolve + commit every batch; checks every row against `seen` (key -> slot, kept by the test); returns the misses per batch"""
    misses = []
    for rows in batches:
        base = index.count
        slots, miss = index.resolve(rows)
        assert slots.shape == (rows.shape[0],) and slots.dtype == np.int32 and miss.dtype == np.int32
        assert slots.max() < index.capacity
        new = {}
        for r, s in zip(rows, slots):
            k = (r.tobytes(), rows.shape[1])
            if k in seen:
                assert s == seen[k]                                   # a committed entry keeps its slot
            else:                                                     # a miss: every copy in the batch names the same miss row
                i = new.setdefault(k, len(new))
                assert s == (base + i if base + i < index.capacity else -(1 + i))
                np.testing.assert_array_equal(miss[i], r)
        assert miss.shape == (len(new), rows.shape[1])
        # every row resolves to a row of a table whose tail [base, base + misses) holds this batch's misses
        g = OptionIndex.gather_rows(slots, base)
        assert g.min() >= 0 and g.max() < base + max(len(new), 1) and (g[slots >= 0] == slots[slots >= 0]).all()
        stored = index.commit()
        assert stored == min(len(new), index.capacity - base) and index.count == base + stored
        for k, i in new.items():
            if base + i < index.capacity:
                seen[k] = base + i
        misses.append(len(new))
    return misses


@needs_hdf5
@pytest.mark.parametrize("split", ["val", "test"])
def test_index_over_the_real_batches_of_a_split(split):
    batches = split_batches(split)
    assert len(batches) >= 2
    distinct = {(r.tobytes(), rows.shape[1]) for rows in batches for r in rows}        # counted independently of the index
    total = sum(rows.shape[0] for rows in batches)
    assert len(distinct) < total                                                       # the split repeats its answers
    index, seen = OptionIndex(), {}
    assert index.capacity == DEFAULT_ROWS
    first = one_pass(index, batches, seen)
    assert sum(first) == len(distinct) == index.count
    assert one_pass(index, batches, seen) == [0] * len(batches)                        # warm: nothing left to encode
    index.flush()
    assert index.count == 0
    assert one_pass(index, batches, {}) == first                                       # after a flush the counts repeat
    print("%s: %d candidate rows, %d distinct, misses per batch %s" % (split, total, len(distinct), first))


@needs_hdf5
@pytest.mark.parametrize("split", ["val", "test"])
def test_a_full_table_inserts_nothing_more_and_still_resolves_every_row(split):
    batches = split_batches(split)
    distinct = {r.tobytes() for rows in batches for r in rows}
    assert len(distinct) > 64
    index, seen = OptionIndex(64), {}
    first = one_pass(index, batches, seen)                                             # (asserts slots < 64 and the -(1 + i) form)
    assert index.count == 64 and sum(first) >= len(distinct)
    second = one_pass(index, batches, seen)
    assert index.count == 64 and sum(second) > 0                                       # what did not fit is encoded per batch again
    assert sum(second) < sum(rows.shape[0] for rows in batches)                        # ... and what fitted is not


def test_to_is_part_of_the_key():
    rows = np.array([[5, 6, 0, 0], [7, 0, 0, 0], [5, 6, 0, 0]], np.int32)
    index = OptionIndex(16)
    slots, miss = index.resolve(rows)
    assert slots.tolist() == [0, 1, 0] and miss.tolist() == [[5, 6, 0, 0], [7, 0, 0, 0]]
    assert index.commit() == 2
    assert index.resolve(rows)[1].shape[0] == 0
    # the same tokens behind one more trailing pad: the pad advances the state (no maskZero), so nothing cached applies
    longer = np.concatenate([rows, np.zeros((3, 1), np.int32)], 1)
    slots, miss = index.resolve(longer)
    assert miss.shape == (2, 5) and slots.tolist() == [0, 1, 0] and index.count == 0
    index.commit()
    assert index.count == 2 and index.resolve(rows)[1].shape[0] == 2


def test_resolve_without_commit_leaves_no_entry():
    a = np.array([[1, 2], [3, 4]], np.int32)
    b = np.array([[3, 4], [9, 9]], np.int32)
    index = OptionIndex(16)
    index.resolve(a)                       # uploaded, then replaced: never stepped
    slots, miss = index.resolve(b)
    assert index.count == 0 and slots.tolist() == [0, 1] and miss.tolist() == b.tolist()
    index.commit()
    assert index.commit() == 0             # nothing pending twice
    slots, miss = index.resolve(a)
    assert slots.tolist() == [2, 0] and miss.tolist() == [[1, 2]]
    with pytest.raises(ValueError):
        OptionIndex(0)


def test_evaluate_lists_the_flag():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'evaluate.py'), '-h'], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and '-optionCache' in r.stdout


def test_flag_value_everywhere_and_the_symbol_set_where_it_was():
    header = open(os.path.join(ROOT, 'include', 'visdial_hip.h')).read()
    common = open(os.path.join(ROOT, 'visdial_amd', 'csrc', 'common.h')).read()
    lua = open(os.path.join(ROOT, 'lua', 'visdial_ffi.lua')).read()
    assert re.search(r'^#define\s+VD_FLAG_STATE_ONLY\s+32\s*$', header, re.M)
    assert re.search(r'^#define\s+VD_FLAG_STATE_ONLY\s+32\s*$', common, re.M)
    assert 'static const int VD_FLAG_STATE_ONLY = 32;' in lua
    assert ops.FLAG_STATE_ONLY == 32
    assert ops.FLAG_STATE_ONLY & (ops.FLAG_BF16 | ops.FLAG_SPLIT9 | ops.FLAG_SPLIT6 | ops.FLAG_SPLIT3 | ops.FLAG_LIVE_PREFIX) == 0
    assert re.search(r'^#define\s+VD_ABI_VERSION\s+2\s*$', header, re.M)
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    names = set(re.findall(r'\b(vd_[a-z0-9_]+)\s*\(', code))
    assert len(names) == 101
    assert names == set(re.findall(r"^\s+'(vd_[a-z0-9_]+)',$", lua, re.M))


def test_two_slot_recurrence_ends_on_the_oracles_option_encoding():
    """VD_FLAG_STATE_ONLY's contract in numpy: step t reads slot (t - 1) & 1 (zeros at t = 0), writes slot t & 1, keeps no gate; the
    state in slot (To - 1) & 1 is decoders/disc.lua's encoding -- trailing pads included, for an even and an odd To"""
    from oracle import visdial_oracle as vo
    rng = np.random.RandomState(7)
    V, E, H, N, O = 23, 8, 16, 3, 5
    P = {'embed': rng.randn(V + 1, E), 'opt.W': rng.randn(E + H, 4 * H) * 0.3, 'opt.b': rng.randn(4 * H) * 0.1}
    P['embed'][0] = 0
    for To in (6, 7):
        options = rng.randint(1, V + 1, (N, O, To))
        options[np.arange(To)[None, None, :] >= rng.randint(1, To + 1, (N, O, 1))] = 0    # left-aligned, trailing pads
        _, st = vo.disc_decoder_forward(P, None, options, np.zeros((N, H)))
        tok = options.reshape(N * O, To).T
        table = P['embed'] @ P['opt.W'][:E] + P['opt.b']                                   # Emb * Wx + b, gathered by token id
        h, c = np.zeros((2, N * O, H)), np.zeros((2, N * O, H))
        for t in range(To):
            hp = h[(t - 1) & 1] if t else np.zeros((N * O, H))
            cp = c[(t - 1) & 1] if t else np.zeros((N * O, H))
            a = table[tok[t]] + hp @ P['opt.W'][E:]
            i, f, o, g = vo.sigmoid(a[:, :H]), vo.sigmoid(a[:, H:2 * H]), vo.sigmoid(a[:, 2 * H:3 * H]), np.tanh(a[:, 3 * H:])
            c[t & 1] = f * cp + i * g
            h[t & 1] = o * np.tanh(c[t & 1])
        np.testing.assert_allclose(h[(To - 1) & 1], st['h'][To - 1], rtol=0, atol=1e-12)
        np.testing.assert_allclose(c[(To - 1) & 1], st['c'][To - 1], rtol=0, atol=1e-12)
        np.testing.assert_allclose(h[(To - 1) & 1].reshape(N, O, H), st['optH'], rtol=0, atol=1e-12)
        # the pads matter: stopping at the last token is another state
        assert np.abs(st['h'][To - 1] - st['h'][0]).max() > 1e-3
