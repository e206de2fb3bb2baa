"""The entry points of csrc/lhood.hip as operators over the case tables of tests/lhood_cases.py: vd_lhood_nll and vd_lhood_live_rows through
the C ABI, vd_lhood_lse_p / vd_lhood_edge_sum_p / vd_lhood_order_p / vd_lhood_order_work_ints / vd_lhood_sum_p (internal: declarations in
csrc/rt_core.h) through visdial_amd._lib.internal, which binds them from the symbols the built library exports.  Both kernel families of the head (the fused MFMA kernel and the
one-workgroup-per-row kernel) at their smallest shapes, ragged tiles, strided and offset operands, NULL bias, every target slot, logits
spread over +-80; the edge sum around its 256-float stride; the length order up to T = 255 on every length profile; the live-row list past
256 counting blocks; the sum scattered through a permutation; the refusals and no-ops.

Every operand holds NaN wherever the contract says it is never read; every output lies in front of 128 marked guard elements that must
come back bit for bit.  Bounds (lhood_cases.py): nll / lse within 1e-4 * max(1, |ref|.max()) of fp64 over the whole output and each named
slice; the edge sum within (K + T + 4) 2^-24 x the magnitudes it adds; integers and vd_lhood_sum_p bit for bit.  Every input is legal for its
entry point.  Each test prints its worst error over its bound; the worst figures per family are printed when the module has run
(profiles/lhood_ops_parity.txt: VD_LHOOD_PARITY_OUT=<file> writes them)."""
import ctypes as C
import functools
import os
import re
import types

import numpy as np
import pytest
import torch

import lhood_cases as lc

pytestmark = pytest.mark.gpu

WORST = {}                                                     # (entry point, family) -> [cases, worst ratio to the bound, worst |err|]
DIFF = {}                                                      # op -> worst |mfma - rows| on the shared operands
REQUIRED = {('vd_lhood_nll', 'mfma'), ('vd_lhood_nll', 'rows'), ('vd_lhood_lse_p', 'mfma'), ('vd_lhood_lse_p', 'rows'),
            ('vd_lhood_edge_sum_p', '-'), ('vd_lhood_order_p', '-'), ('vd_lhood_live_rows', '-'), ('vd_lhood_sum_p', '-')}
HEAD_ENTRY = {'nll': 'vd_lhood_nll', 'lse': 'vd_lhood_lse_p'}


@pytest.fixture(scope="module")
def lib():
    """the C ABI entry points through _lib.call and the five internal ones through _lib.internal"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from visdial_amd import _lib
    return types.SimpleNamespace(
        nll=functools.partial(_lib.call, 'vd_lhood_nll'), live_rows=functools.partial(_lib.call, 'vd_lhood_live_rows'),
        lse=_lib.internal('vd_lhood_lse_p'), edge_sum=_lib.internal('vd_lhood_edge_sum_p'), order=_lib.internal('vd_lhood_order_p'),
        order_work_ints=_lib.internal('vd_lhood_order_work_ints', C.c_int64), sum=_lib.internal('vd_lhood_sum_p'),
        Error=_lib.VisdialHipError)


@pytest.fixture(scope="module", autouse=True)
def parity_record():
    yield
    if set(WORST) != REQUIRED or set(DIFF) != {'nll', 'lse'}:  # a partial run measures a part: the record keeps the last whole one
        return
    lines = ["lhood.hip entry points against fp64 (tests/test_lhood_ops_gpu.py over tests/lhood_cases.py), worst case per entry point and kernel family.",
             "ratio = worst error / bound: nll, lse 1e-4 max(1, |ref|.max()) over the output and each named slice; edge sum (K + T + 4) 2^-24 x",
             "magnitudes, per candidate; order, live rows, sum: bit for bit (ratio 0 = equal).  |err| = worst |fp32 result - fp64|.",
             "%-22s %-6s %5s %12s %12s" % ("entry point", "family", "cases", "ratio", "|err|")]
    for (entry, fam), (n, ratio, err) in sorted(WORST.items()):
        lines.append("%-22s %-6s %5d %12.5f %12.3e" % (entry, fam, n, ratio, err))
    lines.append("mfma against rows on the operands of %s (printed, not asserted): worst |nll difference| %.3e, worst |lse difference| %.3e"
                 % (lc.SHARED[0], DIFF['nll'], DIFF['lse']))
    print('\n' + '\n'.join(lines))
    if os.environ.get('VD_LHOOD_PARITY_OUT'):                  # how profiles/lhood_ops_parity.txt was written
        with open(os.environ['VD_LHOOD_PARITY_OUT'], 'w') as f:
            f.write('\n'.join(lines) + '\n')


def note(entry, family, name, v):
    w = WORST.setdefault((entry, family), [0, 0.0, 0.0])
    w[0] += 1
    w[1], w[2] = max(w[1], v.ratio), max(w[2], v.err)
    print("%s %s: worst error / bound %.5f (worst |err| %.3e)" % (entry, name, v.ratio, v.err))


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()             # (a copy: the tables' arrays are read only)


def ptr(t, off=0):
    return None if t is None else t.data_ptr() + 4 * off


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ nll and lse
class HeadDevice(object):
    def __init__(self, lay):
        self.lay = lay
        self.h, self.W, self.b, self.act, self.target = dev(lay.hbuf), dev(lay.wbuf), dev(lay.bbuf), dev(lay.act), dev(lay.target)
        assert self.h.data_ptr() % 16 == 0 and self.W.data_ptr() % 16 == 0     # the offsets inside the buffers decide the family

    def run(self, lib, op):
        c = self.lay.case
        out = dev(self.lay.out0)
        if op == 'nll':
            lib.nll(ptr(self.h, c.h_off), c.ldh, c.rows, ptr(self.act), c.n_act, ptr(self.target), ptr(self.W, lc.W_OFF), c.ldw, ptr(self.b),
                    c.V, c.H, ptr(out), stream())
        else:
            lib.lse(ptr(self.h, c.h_off), c.ldh, c.rows, ptr(self.act), c.n_act, ptr(self.W, lc.W_OFF), c.ldw, ptr(self.b), c.V, c.H, ptr(out),
                    stream())
        return host(out)


@pytest.mark.parametrize("op", ['nll', 'lse'])
@pytest.mark.parametrize("case", lc.HEAD, ids=[c.id for c in lc.HEAD])
def test_lhood_head_cases(lib, case, op):
    """against fp64 over the whole output and every named slice, finite, the repeated rows in identical bits (position independence), the
    guard intact, and the same bits from a second run of the whole case"""
    lay = lc.head_layout(case)
    d = HeadDevice(lay)
    got = d.run(lib, op)
    v = lc.check_head(lay, op, got)
    note(HEAD_ENTRY[op], case.family, case.id, v)
    assert v.ok, (case.id, op, v.failures)
    assert np.array_equal(d.run(lib, op).view(np.uint32), got.view(np.uint32)), (case.id, op, 'a second run gave other bits')


@pytest.mark.parametrize("op", ['nll', 'lse'])
def test_lhood_head_families_on_the_same_operands(lib, op):
    """the fused MFMA kernel and the row kernel (reached by ldh = H + 1 and by a base pointer one float off alignment) on one set of values:
    each is held to fp64 by test_lhood_head_cases; their mutual difference is printed, not asserted"""
    outs = {}
    for name in lc.SHARED:
        case = lc.HEAD_BY_NAME[name]
        lay = lc.head_layout(case)
        outs[name] = HeadDevice(lay).run(lib, op)[:case.n_act].astype(np.float64)
        assert np.isfinite(outs[name]).all()
    ref = lc.head_reference(lc.head_layout(lc.HEAD_BY_NAME[lc.SHARED[0]]), op)
    DIFF[op] = max(float(np.abs(outs[lc.SHARED[0]] - outs[n]).max()) for n in lc.SHARED[1:])
    print("%s: worst |mfma - rows| %.3e; worst |mfma - fp64| %.3e, worst |rows - fp64| %.3e"
          % (HEAD_ENTRY[op], DIFF[op], float(np.abs(outs[lc.SHARED[0]] - ref).max()), max(float(np.abs(outs[n] - ref).max()) for n in lc.SHARED[1:])))
    assert np.array_equal(outs[lc.SHARED[1]], outs[lc.SHARED[2]])                            # the row kernel: the same bits under both layouts


# ------------------------------------------------------------------------------------------------------------ the edge sum
@pytest.mark.parametrize("case", lc.EDGE, ids=[c.id for c in lc.EDGE])
def test_lhood_edge_sum_cases(lib, case):
    lay = lc.edge_layout(case)
    c = case
    bufs = [dev(a) for a in (lay.hbuf, lay.node_row, lay.lse, lay.enode, lay.etgt, lay.wbuf, lay.bbuf)]
    if c.T == 0:
        bufs = [None] * 7                                      # T = 0 reads no operand: null pointers are accepted
    h, node_row, lse, enode, etgt, W, b = bufs

    def run():
        out = dev(lay.out0)
        lib.edge_sum(ptr(h), c.ldh, ptr(node_row), ptr(lse), ptr(enode), ptr(etgt), c.T, c.rows, c.C, ptr(W, lc.W_OFF) if W is not None else None,
                     c.ldw, ptr(b), c.H, ptr(out, lc.O_OFF), c.ldo, stream())
        return host(out)
    got = run()
    v = lc.check_edge(lay, got)
    note('vd_lhood_edge_sum_p', '-', case.id, v)
    assert v.ok, (case.id, v.failures)
    assert np.array_equal(run().view(np.uint32), got.view(np.uint32)), (case.id, 'a second run gave other bits')


# ------------------------------------------------------------------------------------------------------------ the length order
@pytest.mark.parametrize("case", lc.ORDER, ids=[lc.order_id(c) for c in lc.ORDER])
def test_lhood_order_cases(lib, case):
    lay = lc.order_layout(case)
    c = case
    work_ints = int(lib.order_work_ints(c.T, c.rows))
    assert work_ints == lay.work_ints()
    tok, tgt = dev(lay.tok.reshape(-1)), dev(lay.tgt.reshape(-1))
    work0 = np.full(work_ints + lc.GUARD, lc.IMARK, np.int32)
    o = {k: dev(a) for k, a in lay.out0.items()}
    work = dev(work0)
    lib.order(ptr(tok), ptr(tgt), c.T, c.rows, c.C, ptr(o['perm']), ptr(o['rep']), ptr(o['tok_s']), ptr(o['tgt_s']), ptr(work), ptr(o['info']),
              stream())
    v = lc.check_order(lay, {k: host(t) for k, t in o.items()})
    note('vd_lhood_order_p', '-', lc.order_id(case), v)
    assert v.ok, (lc.order_id(case), v.failures)
    assert (host(work)[work_ints:] == lc.IMARK).all(), 'written behind the scratch of vd_lhood_order_work_ints'


# ------------------------------------------------------------------------------------------------------------ the live-row list
@pytest.mark.parametrize("n,kind", lc.LIVE, ids=['live-n%d-%s' % nk for nk in lc.LIVE])
def test_lhood_live_rows_cases(lib, n, kind):
    tok, tgt, act0 = lc.live_inputs(n, kind)
    blocks = lc.cdiv(n, lc.LIVE_BLOCK)
    act, work, dtok, dtgt = dev(act0), dev(np.full(blocks + 1 + lc.GUARD, lc.IMARK, np.int32)), dev(tok), dev(tgt)
    count = C.c_int32(-5)
    lib.live_rows(ptr(dtok), ptr(dtgt), n, ptr(act), ptr(work), C.addressof(count), stream())
    v = lc.check_live(tok, tgt, act0, int(count.value), host(act))
    note('vd_lhood_live_rows', '-', 'n = %d (%s)' % (n, kind), v)
    assert v.ok, (n, kind, v.failures)
    assert (host(work)[blocks + 1:] == lc.IMARK).all(), 'written behind the scratch'


# ------------------------------------------------------------------------------------------------------------ the sum with perm
@pytest.mark.parametrize("case", lc.SUM, ids=[lc.sum_id(c) for c in lc.SUM])
def test_lhood_sum_perm_cases(lib, case):
    lay = lc.sum_layout(case)
    c = case
    nll, act, perm, out = dev(lay.nll), dev(lay.act), dev(lay.perm), dev(lay.out0)
    if c.empty:
        nll = act = None                                       # n_act = 0 with nll = act = NULL: every candidate +0
    lib.sum(ptr(nll), ptr(act), lay.act.size, c.T, c.rows, c.C, ptr(perm), ptr(out, lc.O_OFF), c.ldo, stream())
    v = lc.check_sum(lay, host(out))
    note('vd_lhood_sum_p', '-', lc.sum_id(case), v)
    assert v.ok, (lc.sum_id(case), v.failures)


# ------------------------------------------------------------------------------------------------------------ refusals and no-ops
def test_lhood_refusals_and_noops(lib):
    """no kernel is launched in any of these; what a refused or empty call was given comes back bit for bit"""
    rng = np.random.RandomState(2)
    f = dev(rng.randn(4096).astype(np.float32))
    ints = dev(np.arange(64, dtype=np.int32) % 2 + 1)
    out0 = np.full(256, lc.MARK, np.float32)
    out = dev(out0)
    s = stream()

    def nll(h=ptr(f), ldh=64, rows=8, act=ptr(ints), n_act=2, tgt=ptr(ints), W=ptr(f, 1024), ldw=64, V=4, H=64, o=ptr(out)):
        return lib.nll(h, ldh, rows, act, n_act, tgt, W, ldw, None, V, H, o, s)

    def lse(h=ptr(f), ldh=64, rows=8, act=ptr(ints), n_act=2, W=ptr(f, 1024), ldw=64, V=4, H=64, o=ptr(out)):
        return lib.lse(h, ldh, rows, act, n_act, W, ldw, None, V, H, o, s)

    def refused(call, words):
        with pytest.raises(lib.Error, match=re.escape(words)):
            call()
        assert np.array_equal(host(out).view(np.uint32), out0.view(np.uint32)), 'a refused call wrote'
    # n_act = 0 with null pointers: returns 0, writes nothing
    assert nll(h=None, act=None, n_act=0, tgt=None, W=None, o=None) == 0 and lse(h=None, act=None, n_act=0, W=None, o=None) == 0
    assert nll(n_act=0) == 0 and lse(n_act=0) == 0
    assert np.array_equal(host(out).view(np.uint32), out0.view(np.uint32))
    # H beyond the row kernel's LDS on a shape the fused kernel does not take
    refused(lambda: nll(ldh=12292, ldw=12292, V=2, H=12292), "vd_lhood_nll: H = 12292 too large for the row kernel")
    refused(lambda: lse(ldh=12292, ldw=12292, V=2, H=12292), "lhood lse: H = 12292 too large for the row kernel")
    refused(lambda: nll(ldh=60), "vd_lhood_nll: bad args")
    refused(lambda: nll(ldw=63), "vd_lhood_nll: bad args")
    refused(lambda: lse(ldh=60), "lhood lse: bad args")
    refused(lambda: nll(h=None), "vd_lhood_nll: null pointer")
    refused(lambda: lse(o=None), "lhood lse: null pointer")
    # T = 256: one key more than the counting sort's block holds
    refused(lambda: lib.order(ptr(ints), ptr(ints), 256, 4, 1, ptr(out), ptr(out), ptr(out), ptr(out), ptr(out), ptr(out), s),
            "lhood order: bad args T=256 rows=4")
    refused(lambda: lib.order(ptr(ints), ptr(ints), 0, 4, 1, ptr(out), ptr(out), ptr(out), ptr(out), ptr(out), ptr(out), s),
            "lhood order: bad args T=0 rows=4")
    refused(lambda: lib.edge_sum(ptr(f), 6, ptr(ints), ptr(f), ptr(ints), ptr(ints), 1, 2, 1, ptr(f), 8, None, 4, ptr(out), 1, s), "lhood edge sum: bad args")
    refused(lambda: lib.edge_sum(ptr(f), 8, ptr(ints), ptr(f), ptr(ints), ptr(ints), 1, 2, 2, ptr(f), 8, None, 4, ptr(out), 1, s), "lhood edge sum: bad args")
    refused(lambda: lib.sum(None, None, 3, 1, 4, 1, None, ptr(out), 1, s), "vd_lhood_sum: null pointer")
    # no candidate: nothing to do
    assert lib.edge_sum(None, 8, None, None, None, None, 3, 0, 1, None, 8, None, 4, ptr(out), 1, s) == 0
    assert lib.sum(None, None, 0, 3, 0, 1, None, ptr(out), 1, s) == 0
    count = C.c_int32(-5)
    assert lib.live_rows(ptr(ints), ptr(ints), 0, ptr(out), ptr(out), C.addressof(count), s) == 0 and count.value == 0
    assert np.array_equal(host(out).view(np.uint32), out0.view(np.uint32))


def test_lhood_parity_figures_are_complete():
    """the last test of the module: the worst figures per entry point and family of everything that ran, each within its bound; after a
    whole run, every family with all its cases"""
    for key, (n, ratio, err) in sorted(WORST.items()):
        print("%-22s %-6s %5d cases, worst error / bound %.5f, worst |err| %.3e" % (key + (n, ratio, err)))
        assert n > 0 and ratio <= 1.0
    if set(WORST) != REQUIRED:
        return                                                 # (a partial run: the figures above cover what ran)
    assert WORST[('vd_lhood_nll', 'mfma')][0] == sum(c.family == 'mfma' for c in lc.HEAD)
    assert WORST[('vd_lhood_lse_p', 'rows')][0] == sum(c.family == 'rows' for c in lc.HEAD)
