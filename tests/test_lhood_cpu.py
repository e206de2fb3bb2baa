"""The live-row log-likelihood head of generative retrieval (params.fusedLhood, csrc/lhood.hip) without a device: the Lua host on
the dry library makes ONE vd_model_retrieve_lhood per batch and no vd_model_retrieve (and the calls it always made without the flag),
a disc model with the flag is refused by every host before a device call, the header / ctypes table / generated ffi / built library
agree on the new symbols, evaluate.py lists the flag, and the numpy statement of "live row" names exactly the rows over which
utils.computeLhood (oracle.visdial_oracle.compute_lhood) sums."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, small_params
from lua_host import LuaHost, first
from luavm import LuaError, to_py
from visdial_amd.dataloader import SyntheticDataloader
from visdial_amd.opts import derive

NEW = ('vd_lhood_live_rows', 'vd_lhood_nll', 'vd_lhood_sum', 'vd_model_retrieve_lhood')


def live_rows(option_in, option_out):
    """[T x rows] time-major tokens -> the linear indices t * rows + r that count, step-major then row: the decoder input is not a
    pad and there is a target.  What vd_lhood_live_rows writes."""
    return np.flatnonzero((option_in.reshape(-1) != 0) & (option_out.reshape(-1) > 0))


def _gen_batch(p):
    dl = SyntheticDataloader(p, seed=13)
    batch = dl.getTrainBatch(p)
    dl.add_gen_options(batch, batch['ques_fwd'].shape[0])
    return batch


def test_lua_retrieve_batch_with_fused_lhood_is_one_lhood_call():
    p = derive(small_params(encoder='lf-ques-im-hist', decoder='gen'))
    batch = _gen_batch(p)
    host = LuaHost(p, dry=True)
    m = host.model()
    host.invoke(m, 'setMode', False)
    host.get(m, 'params').set('useGt', True)
    n0 = len(host.dry.calls)
    r0 = to_py(first(host.invoke(m, 'retrieveBatch', host.batch(batch))))
    base = [c[0] for c in host.dry.calls[n0:]]
    assert base.count('vd_model_retrieve') == 1 and 'vd_model_retrieve_lhood' not in base
    host.get(m, 'params').set('fusedLhood', 1)
    n1 = len(host.dry.calls)
    r1 = to_py(first(host.invoke(m, 'retrieveBatch', host.batch(batch))))
    fused = [c[0] for c in host.dry.calls[n1:]]
    assert fused.count('vd_model_retrieve_lhood') == 1 and 'vd_model_retrieve' not in fused
    # nothing else changes: the same calls in the same order around the one that was swapped
    assert [n for n in fused if n != 'vd_model_retrieve_lhood'] == [n for n in base if n != 'vd_model_retrieve']
    assert r1.shape == r0.shape == (batch['ques_fwd'].shape[0], p['maxQuesCount']) and r1.dtype == np.float64
    host.get(m, 'params').set('fusedLhood', 0)                 # 0 = the calls it makes today
    n2 = len(host.dry.calls)
    host.invoke(m, 'retrieveBatch', host.batch(batch))
    assert [c[0] for c in host.dry.calls[n2:]] == base
    host.close()


def test_lua_refuses_fused_lhood_with_a_disc_model():
    p = derive(small_params(encoder='lf-ques', decoder='disc'))
    batch = SyntheticDataloader(p, seed=13).getTrainBatch(p)
    host = LuaHost(p, dry=True)
    m = host.model()
    host.get(m, 'params').set('fusedLhood', 1)
    n0 = len(host.dry.calls)
    with pytest.raises(LuaError, match='fusedLhood.*only for generative model'):
        host.invoke(m, 'retrieveBatch', host.batch(batch))
    assert not any(c[0].startswith('vd_model_retrieve') for c in host.dry.calls[n0:])
    host.close()


def test_python_operator_host_refuses_fused_lhood_with_a_disc_model():
    from visdial_amd.model import Model

    class Host(Model):                         # the refusal comes before any device call
        def __init__(self):
            self.params = {'decoder': 'disc', 'fusedLhood': 1}

    with pytest.raises(ValueError, match="fusedLhood.*only for the generative decoder.*'disc'"):
        Host().retrieveBatch({})


def test_header_ctypes_table_ffi_and_library_agree_on_the_new_symbols():
    from visdial_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'visdial_hip.h')).read()
    ffi = open(os.path.join(ROOT, 'lua', 'visdial_ffi.lua')).read()
    text = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert '#define VD_ABI_VERSION 2' in header and _lib.ABI_VERSION == 2       # functions were only added
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(['make', '-C', os.path.join(ROOT, 'visdial_amd', 'csrc'), '-j8'])
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        decl = re.search(r'\bint\s+%s\s*\(([^;]*?)\)\s*;' % name, text, flags=re.S)
        assert decl, name
        nargs = len([a for a in decl.group(1).split(',') if a.strip()])
        assert len(_lib.PROTOTYPES[name]) == nargs, name                        # one ctypes type per declared argument
        assert re.search(r'\bint\s+%s\s*\(' % name, ffi), name                   # the cdef
        assert "'%s'" % name in ffi, name                                        # and the symbol list the binding checks
        assert hasattr(lib, name), name
    declared = set(re.findall(r'\b(vd_[a-z0-9_]+)\s*\(', text))
    assert len(declared) == 101 and '101 entry points' in header


def test_evaluate_py_lists_fused_lhood():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'evaluate.py'), '-h'], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert '-fusedLhood' in r.stdout


def test_live_rows_are_the_rows_compute_lhood_sums():
    """an empty candidate (option_in = <START>, 0.., option_out = 0..), a full-length one and a length-1 one: the live rows are
    exactly the (step, candidate) pairs utils.computeLhood adds, and summing the picked log-probabilities over them per candidate
    IS its result; the empty candidate has no live row and scores exactly 0"""
    from oracle import visdial_oracle as vo
    T, V, START, END = 6, 11, 10, 11
    words = [[], [3, 1, 4, 1, 5], [9]]                        # lengths 0, T - 1 (full), 1
    oin = np.zeros((T, 3), np.int64)
    oout = np.zeros((T, 3), np.int64)
    for r, w in enumerate(words):
        oin[0, r] = START
        oin[1:1 + len(w), r] = w
        if w:                                                  # processOptions writes no <END> for length 0
            oout[:len(w), r] = w
            oout[len(w), r] = END
    act = live_rows(oin, oout)
    want = [t * 3 + r for t in range(T) for r, w in enumerate(words) if w and t <= len(w)]
    assert act.tolist() == want and sorted(want) == want       # step-major, then row = ascending
    assert not any(a % 3 == 0 for a in act)                    # the empty candidate has no live row
    rs = np.random.RandomState(0)
    x = rs.standard_normal((T, 3, V))
    logp = x - np.log(np.exp(x).sum(-1, keepdims=True))
    ref = vo.compute_lhood(oout, logp)                         # sums over oout != 0
    assert set(act.tolist()) == set(np.flatnonzero(oout.reshape(-1) != 0).tolist())
    mine = np.zeros(3)
    for a in act:                                              # in step order per candidate
        t, r = divmod(int(a), 3)
        mine[r] += logp[t, r, oout[t, r] - 1]
    np.testing.assert_array_equal(mine, ref)
    assert ref[0] == 0.0 and mine[0] == 0.0
    # a row with a target but a pad INPUT is masked by MaskZero (gen.lua:23-24): not live either
    oin2 = oin.copy()
    oin2[2, 1] = 0
    assert (2 * 3 + 1) not in live_rows(oin2, oout).tolist()
