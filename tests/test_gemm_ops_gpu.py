"""The GEMM entry points of csrc/gemm_ops.hip -- vd_gemm_nt, vd_gemm_nn, vd_gemm_tn_acc, vd_gemm_tn_rows_acc through visdial_amd.ops, the
internal vd_gemm_nn_live_p through visdial_amd._lib.internal -- over the case table of tests/gemm_cases.py: every kernel family of the dispatch, at the
strides the runtime passes (views at a column offset, leading dimension > width), ragged widths on padded rows, every epilogue mode, short
K loops of the LDS-DMA pipelines, against fp64.

Every operand holds NaN wherever the contract says it is never used and a large finite mark in the pad columns that must only be finite;
the output lies in front of marked columns, rows and a trailing guard that must come back bit for bit.  Bounds (gemm_cases.py): rel-L2 <
1e-5 (1e-2 under FLAG_BF16) and, on the exact-fp32 paths without tanh, |got - ref| <= (K + 4) 2^-24 (|A|.|B| + |bias| + |C0|) per element.
The worst figures per family are printed when the whole module has run (profiles/gemm_ops_parity.txt: VD_GEMM_PARITY_OUT=<file> writes them)."""
import os
import re

import numpy as np
import pytest
import torch

import gemm_cases as gc

pytestmark = pytest.mark.gpu

WORST = {}                                                     # (entry, family) -> [cases, worst rel-L2, worst ratio to the elementwise bound]
ENTRY_NAME = {'nt': 'vd_gemm_nt', 'nn': 'vd_gemm_nn', 'live': 'vd_gemm_nn_live_p', 'tn': 'vd_gemm_tn_acc', 'rows': 'vd_gemm_tn_rows_acc'}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from visdial_amd import ops as o
    return o


@pytest.fixture(scope="module")
def live_p(ops):
    from visdial_amd import _lib
    return _lib.internal('vd_gemm_nn_live_p')


@pytest.fixture(scope="module", autouse=True)
def parity_record():
    yield
    if set(WORST) != gc.REQUIRED:                              # a partial run measures a part: the record keeps the last whole one
        return
    lines = ["GEMM entry points against fp64 (tests/test_gemm_ops_gpu.py over tests/gemm_cases.py), worst case per kernel family.",
             "rel-L2 bound 1e-5 (1e-2 bf16); ratio = max |got - ref| / ((K + 4) 2^-24 (|A|.|B| + |bias| + |C0|)), bound 1, exact fp32 without tanh only.",
             "%-22s %-12s %5s %12s %12s" % ("entry point", "family", "cases", "rel-L2", "ratio")]
    for (entry, fam), (n, rel, ratio) in sorted(WORST.items()):
        lines.append("%-22s %-12s %5d %12.3e %12s" % (ENTRY_NAME[entry], fam, n, rel, "%.4f" % ratio if ratio is not None else "n/a"))
    print('\n' + '\n'.join(lines))
    if os.environ.get('VD_GEMM_PARITY_OUT'):                   # how profiles/gemm_ops_parity.txt was written
        with open(os.environ['VD_GEMM_PARITY_OUT'], 'w') as f:
            f.write('\n'.join(lines) + '\n')


def note(case, v):
    w = WORST.setdefault((case.entry, case.family), [0, 0.0, None])
    w[0] += 1
    w[1] = max(w[1], v.rel_l2)
    if case.exact:
        w[2] = max(w[2] or 0.0, v.bound_ratio)
    print("%s: rel-L2 %.3e, ratio to the elementwise bound %s" % (case.id, v.rel_l2, "%.4f" % v.bound_ratio if case.exact else "n/a"))


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return None if a is None else torch.from_numpy(a).cuda()


def bits(t):
    return t.view(torch.int32)


class Device(object):
    """a layout's buffers on the device; a fresh C per call"""

    def __init__(self, lay):
        self.lay = lay
        self.A, self.B, self.bias, self.ra, self.rb = dev(lay.A), dev(lay.B), dev(lay.bias), dev(lay.ra), dev(lay.rb)
        self.C0 = dev(lay.C0)

    def run(self, ops, live_p=None, mask=None):
        c = self.lay.case
        Cbuf = self.C0.clone()
        a, b, out = self.A[gc.OFF:], self.B[gc.OFF:], Cbuf[gc.OFF:]
        if c.entry == 'nt':
            ops.gemm_nt(a, b, out, bias=self.bias, act=c.act, accumulate=c.accumulate, M=c.M, N=c.N, K=c.K, lda=c.lda, ldw=c.ldb, ldc=c.ldc)
        elif c.entry == 'nn':
            ops.gemm_nn(a, b, out, bias=self.bias, accumulate=c.accumulate, M=c.M, N=c.N, K=c.K, lda=c.lda, ldb=c.ldb, ldc=c.ldc)
        elif c.entry == 'live':
            live_p(a.data_ptr(), c.lda, b.data_ptr(), c.ldb, self.bias.data_ptr(), out.data_ptr(), c.ldc, c.M, c.N, c.K, mask.data_ptr(),
                   c.row_tile, stream())
        elif c.entry == 'tn':
            ops.gemm_tn_acc(a, b, out, M=c.M, N=c.N, K=c.K, lda=c.lda, ldb=c.ldb, ldc=c.ldc, flags=c.flags)
        else:
            ops.gemm_tn_rows_acc(a, self.ra, b, self.rb, out, M=c.M, N=c.N, lda=c.lda, ldb=c.ldb, ldc=c.ldc)
        torch.cuda.synchronize()
        return Cbuf


def run_case(ops, case):
    lay = gc.layout(case)
    d = Device(lay)
    got = d.run(ops)
    v = gc.check(lay, got.cpu().numpy())
    note(case, v)
    assert v.ok, (case.id, v.failures)
    if not case.atomic:                                        # one owner per element, a fixed K order: the same bits on a second call
        assert torch.equal(bits(d.run(ops)), bits(got)), case.id
    return v


def ids(entry):
    return [c.id for c in gc.cases_of(entry)]


@pytest.mark.parametrize("case", gc.cases_of('nt'), ids=ids('nt'))
def test_gemm_nt_cases(ops, case):
    run_case(ops, case)


@pytest.mark.parametrize("case", gc.cases_of('nn'), ids=ids('nn'))
def test_gemm_nn_cases(ops, case):
    run_case(ops, case)


@pytest.mark.parametrize("case", gc.cases_of('tn'), ids=ids('tn'))
def test_gemm_tn_acc_cases(ops, case):
    run_case(ops, case)


@pytest.mark.parametrize("case", gc.cases_of('rows'), ids=ids('rows'))
def test_gemm_tn_rows_acc_cases(ops, case):
    run_case(ops, case)


@pytest.mark.parametrize("case", gc.cases_of('live'), ids=ids('live'))
def test_gemm_nn_live_prefix_cases(ops, live_p, case):
    """rows of the tiles whose first row is live meet the bounds (and are vd_gemm_nn's bits where it runs the same tile family); rows of
    dead tiles and the guards keep their mark; an empty prefix writes nothing"""
    c, lay = case, gc.layout(case)
    d = Device(lay)
    ref, mag = gc.reference(lay)
    same_family = gc.path_nn(c.M, c.N, c.K).family == c.family
    if same_family:
        whole = d.C0.clone()
        ops.gemm_nn(d.A[gc.OFF:], d.B[gc.OFF:], whole[gc.OFF:], bias=d.bias, M=c.M, N=c.N, K=c.K, lda=c.lda, ldb=c.ldb, ldc=c.ldc)
        torch.cuda.synchronize()
        assert gc.check(lay, whole.cpu().numpy(), ref, mag).ok
    worst = gc.Verdict(True, [], 0.0, 0.0)
    for L in gc.live_prefixes(c.M, c.row_tile):
        mask = torch.zeros(c.M + gc.TAIL, dtype=torch.int32, device='cuda')
        mask[:L] = 1
        mask[c.M:] = 1                                         # behind the last row: a tile predicate read there would call dead tiles live
        got = d.run(ops, live_p, mask)
        live_rows = min(c.M, gc.cdiv(L, c.row_tile) * c.row_tile)
        if L == 0:
            assert torch.equal(bits(got), bits(d.C0)), (c.id, 'an empty prefix wrote')
            continue
        host = got.cpu().numpy()
        v = gc.check(lay, host, ref, mag, rows=slice(0, live_rows))
        assert v.ok, (c.id, L, v.failures)
        dead = lay.result(host)[live_rows:]
        assert (dead.view(np.uint32) == gc.MARK.view(np.uint32)).all(), (c.id, L, 'rows of dead tiles written')
        if same_family:
            assert torch.equal(bits(got)[:gc.OFF + live_rows * c.ldc], bits(whole)[:gc.OFF + live_rows * c.ldc]), (c.id, L)
        worst = gc.Verdict(True, [], max(worst.rel_l2, v.rel_l2), max(worst.bound_ratio, v.bound_ratio))
    note(c, worst)


# ------------------------------------------------------------------------------------------------------------ refusals
def refused(call, words, out):
    from visdial_amd._lib import VisdialHipError
    before = out.clone()
    with pytest.raises(VisdialHipError, match=re.escape(words)):
        call()
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(before)), 'a refused call wrote C'


@pytest.fixture()
def bufs(ops):
    rng = np.random.RandomState(5)
    return [torch.from_numpy(rng.randn(4096).astype(np.float32)).cuda() for _ in range(3)]


ALIGN = "pointer must be 16-byte aligned and leading dimension a multiple of 4"


def test_gemm_nt_refusals(ops, bufs):
    a, w, c = bufs
    nt = lambda A=a, W=w, K=8, lda=12, ldw=12: ops.gemm_nt(A, W, c, M=8, N=8, K=K, lda=lda, ldw=ldw, ldc=12)
    nt()                                                       # (the accepted form of the calls below)
    refused(lambda: nt(lda=13), "vd_gemm_nt A: " + ALIGN + " (ld=13)", c)
    refused(lambda: nt(ldw=14), "vd_gemm_nt W: " + ALIGN + " (ld=14)", c)
    refused(lambda: nt(A=a[1:]), "vd_gemm_nt A: " + ALIGN, c)
    refused(lambda: nt(W=w[2:]), "vd_gemm_nt W: " + ALIGN, c)
    refused(lambda: nt(K=6), "vd_gemm_nt: bad args M=8 N=8 K=6", c)


def test_gemm_nn_refusals(ops, bufs):
    a, b, c = bufs
    nn = lambda A=a, B=b, N=8, K=8, lda=12, ldb=12: ops.gemm_nn(A, B, c, M=8, N=N, K=K, lda=lda, ldb=ldb, ldc=12)
    nn()
    nn(K=5, lda=8)                                             # a ragged K on rows padded to ceil4(K) is taken
    refused(lambda: nn(lda=10), "vd_gemm_nn A: " + ALIGN + " (ld=10)", c)
    refused(lambda: nn(ldb=9), "vd_gemm_nn B: " + ALIGN + " (ld=9)", c)
    refused(lambda: nn(A=a[3:]), "vd_gemm_nn A: " + ALIGN, c)
    refused(lambda: nn(B=b[1:]), "vd_gemm_nn B: " + ALIGN, c)
    refused(lambda: nn(N=6), "vd_gemm_nn: bad args M=8 N=6 K=8", c)
    refused(lambda: nn(K=5, lda=4), "vd_gemm_nn: bad args M=8 N=8 K=5", c)


def test_gemm_tn_refusals(ops, bufs):
    a, b, c = bufs
    idx = torch.arange(8, dtype=torch.int32, device='cuda')
    tn = lambda A=a, B=b, M=8, N=8, lda=12, ldb=12: ops.gemm_tn_acc(A, B, c, M=M, N=N, K=8, lda=lda, ldb=ldb, ldc=12)
    rows = lambda A=a, B=b, M=8, N=8, lda=12, ldb=12: ops.gemm_tn_rows_acc(A, idx, B, idx, c, M=M, N=N, lda=lda, ldb=ldb, ldc=12)
    for fn, name in ((tn, "vd_gemm_tn_acc"), (rows, "vd_gemm_tn_rows_acc")):
        fn()
        fn(M=10, N=6)                                          # ragged M, N on rows padded to ceil4
        refused(lambda: fn(lda=13), name + " A: " + ALIGN + " (ld=13)", c)
        refused(lambda: fn(ldb=18), name + " B: " + ALIGN + " (ld=18)", c)
        refused(lambda: fn(A=a[1:]), name + " A: " + ALIGN, c)
        refused(lambda: fn(B=b[2:]), name + " B: " + ALIGN, c)
        refused(lambda: fn(M=10, lda=8), name + ": bad args M=10 N=8 K=8", c)
        refused(lambda: fn(N=6, ldb=4), name + ": bad args M=8 N=6 K=8", c)


def test_gemm_nn_live_prefix_refusals(ops, live_p, bufs):
    a, b, c = bufs
    mask = torch.ones(64, dtype=torch.int32, device='cuda')
    bias = torch.zeros(8, device='cuda')
    call = lambda A=a, lda=12, N=8, K=8, tile=32: live_p(A.data_ptr(), lda, b.data_ptr(), 12, bias.data_ptr(), c.data_ptr(), 12, 8, N, K,
                                                         mask.data_ptr(), tile, stream())
    call()
    torch.cuda.synchronize()
    for tile in (0, 16, 64, 256):
        refused(lambda: call(tile=tile), "vd_gemm_nn (live rows): bad args M=8 N=8 K=8 row tile %d" % tile, c)
    refused(lambda: call(N=6), "vd_gemm_nn (live rows): bad args M=8 N=6 K=8 row tile 32", c)
    refused(lambda: call(K=5, lda=4), "vd_gemm_nn (live rows): bad args M=8 N=8 K=5 row tile 32", c)
    refused(lambda: call(lda=14), "vd_gemm_nn (live rows) A: " + ALIGN + " (ld=14)", c)
    refused(lambda: call(A=a[1:]), "vd_gemm_nn (live rows) A: " + ALIGN, c)
