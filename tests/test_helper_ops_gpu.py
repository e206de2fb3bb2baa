"""The entry points of csrc/elementwise.hip and csrc/loss.hip as operators over the case tables of tests/helper_cases.py: the C ABI through
visdial_amd._lib.call, vd_zero_inactive_multi / vd_segment_rowsum_acc_bf16 / vd_score_ce_p / vd_logsoftmax_nll_p (internal: declarations in
csrc/common.h and csrc/rt_core.h) through visdial_amd._lib.internal, which binds them from the symbols the built library exports.

Every input lies inside a larger buffer with NaN or a large token id behind it and in its pad columns; every output starts as marks in
front of 128 marked guard elements, and everything the operation does not own must come back bit for bit.  Bounds: helper_cases.py.  Each
test prints its worst error over its bound; the worst figures per entry point are printed when the module has run
(profiles/helper_ops_parity.txt: VD_HELPER_PARITY_OUT=<file> writes them after a whole run).

tests/golden/helper_nll_parent.json holds, for every gen-head case with ld - V <= 3, the SHA-256 of the loss rows and of the logits buffer
that the build BEFORE the pad-column loop of logsoftmax_nll_body left behind (written by this module run against that build with
VD_HELPER_PARENT_OUT=<file>); test_logsoftmax_nll_cases asserts the same bits."""
import ctypes as C
import functools
import hashlib
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import helper_cases as hc

pytestmark = pytest.mark.gpu

WORST = {}                                                     # entry point -> [cases, worst ratio to the bound, worst |err|]
PARENT = {}                                                    # gen-head case -> hashes of this run (ld - V <= 3)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'helper_nll_parent.json')
EXPECTED = {'vd_dropout_mask': len(hc.DROPOUT), 'vd_dropout_apply': 4, 'vd_tanh_backward': 4, 'vd_axpby': 12, 'vd_embed_gather': len(hc.GATHER),
            'vd_embed_scatter_acc': len(hc.SCATTER), 'vd_mask_time_forward': len(hc.MASKTIME), 'vd_mask_time_backward': len(hc.MASKTIME),
            'vd_zero_inactive_rows': len(hc.ZERO_ROWS), 'vd_zero_inactive_multi': len(hc.ZERO_MULTI), 'vd_token_sort': len(hc.TOKEN_SORT),
            'vd_segment_rowsum_acc': len(hc.SEGSUM), 'vd_segment_rowsum_acc_bf16': len(hc.SEGSUM), 'vd_log_softmax_rows': len(hc.LOGSOFTMAX),
            'vd_logsoftmax_nll': 2 * len(hc.NLL), 'vd_logsoftmax_nll_p': 2 * len(hc.NLL),
            'vd_score_ce': len(hc.SCORE), 'vd_score_ce_p': sum(c.p['mode'] != 'scores' for c in hc.SCORE), 'vd_ranks': len(hc.RANKS)}


class VdZeroSet(C.Structure):                                  # csrc/common.h
    _fields_ = [('buf', C.c_void_p * 6), ('ncols', C.c_int * 6), ('n', C.c_int), ('quads_per_row', C.c_long)]


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from visdial_amd import _lib
    public = ('dropout_mask', 'dropout_apply', 'tanh_backward', 'axpby', 'embed_gather', 'embed_scatter_acc', 'mask_time_forward',
              'mask_time_backward', 'zero_inactive_rows', 'token_sort', 'segment_rowsum_acc', 'log_softmax_rows', 'logsoftmax_nll', 'score_ce',
              'ranks')
    internal = ('zero_inactive_multi', 'segment_rowsum_acc_bf16', 'score_ce_p', 'logsoftmax_nll_p')
    return types.SimpleNamespace(Error=_lib.VisdialHipError, **dict((n, _lib.internal('vd_' + n)) for n in internal),
                                 **dict((n, functools.partial(_lib.call, 'vd_' + n)) for n in public))


@pytest.fixture(scope="module", autouse=True)
def parity_record():
    yield
    if os.environ.get('VD_HELPER_PARENT_OUT') and PARENT:      # how tests/golden/helper_nll_parent.json was written (on the build before)
        with open(os.environ['VD_HELPER_PARENT_OUT'], 'w') as f:
            json.dump(PARENT, f, indent=0, sort_keys=True)
    if dict((k, v[0]) for k, v in WORST.items()) != EXPECTED:  # a partial run measures a part: the record keeps the last whole one
        return
    lines = ["elementwise.hip and loss.hip entry points against fp64 and exact restatements (tests/test_helper_ops_gpu.py over tests/helper_cases.py),",
             "worst case per entry point.  ratio = worst error / bound (helper_cases.py): sums (m + 4) 2^-24 x magnitudes per element; scores",
             "(H + 4) 2^-24 |optH|.|enc|; tanh_backward, axpby 4 x 2^-24 x magnitudes; lse, log-softmax, losses 1e-4 max(1, |ref|.max()) over the output",
             "and each named slice; head gradients rel-L2 1e-5; everything else bit for bit (ratio 0 = equal).  |err| = worst |fp32 result - fp64|.",
             "%-28s %5s %12s %12s" % ("entry point", "cases", "ratio", "|err|")]
    for entry, (n, ratio, err) in sorted(WORST.items()):
        lines.append("%-28s %5d %12.5f %12.3e" % (entry, n, ratio, err))
    lines.append("gen head against the build before the pad-column loop (tests/golden/helper_nll_parent.json): %d runs with ld - V <= 3, loss rows and "
                 "logits buffer bit-identical in every one" % len(PARENT))
    lines += ['', 'Cases (tests/helper_cases.py); segment_rowsum_acc runs as fp32 and bf16, logsoftmax_nll as eps 0 / 0.1 x write_grad 0 / 1, score_ce as',
              'vd_score_ce and vd_score_ce_p at eps = 0.1.'] + hc.case_list()
    print('\n' + '\n'.join(lines[:len(WORST) + 6]))
    if os.environ.get('VD_HELPER_PARITY_OUT'):                 # how profiles/helper_ops_parity.txt was written
        with open(os.environ['VD_HELPER_PARITY_OUT'], 'w') as f:
            f.write('\n'.join(lines) + '\n')


def note(entry, name, v):
    w = WORST.setdefault(entry, [0, 0.0, 0.0])
    w[0] += 1
    w[1], w[2] = max(w[1], v.ratio), max(w[2], v.err)
    print("%s %s: worst error / bound %.5f (worst |err| %.3e)" % (entry, name, v.ratio, v.err))


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    if a is None:
        return None
    a = np.array(a)                                            # (a copy: the tables' arrays are read only)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def ptr(t, off_bytes=0):
    return None if t is None else t.data_ptr() + off_bytes


def host(t):
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    return a


def judge(entry, lay, outs, only=None):
    v = hc.check(lay, outs, only)
    note(entry, lay.case.id, v)
    assert v.ok, (entry, lay.case.id, v.failures)


IDS = lambda table: [c.id for c in table]


# ------------------------------------------------------------------------------------------------------------ dropout and glue
@pytest.mark.parametrize("case", hc.DROPOUT, ids=IDS(hc.DROPOUT))
def test_dropout_mask_cases(lib, case):
    lay = hc.dropout_layout(case)
    m = dev(lay.specs[0].out0)
    lib.dropout_mask(ptr(m), case.p['n'], case.p['seed'], case.p['p'], stream())
    judge('vd_dropout_mask', lay, {'mask': host(m)})


@pytest.mark.parametrize("case", hc.POINTWISE, ids=IDS(hc.POINTWISE))
def test_pointwise_cases(lib, case):
    lay = hc.pointwise_layout(case)
    op, n = case.p['op'], case.p['n']
    i = dict((k, dev(v)) for k, v in lay.inp.items())
    s = lay.specs[0]
    out = dev(s.out0)
    if op == 'dropout_apply':
        lib.dropout_apply(ptr(i['x']), ptr(i['mask']), ptr(out), n, lay.scale, stream())
    elif op == 'tanh_backward':
        lib.tanh_backward(ptr(i['dy']), ptr(i['y']), ptr(out), n, stream())
    elif op == 'axpby':
        lib.axpby(ptr(i['a']), ptr(i['b']), ptr(out), n, lay.alpha, lay.beta, stream())
    elif op == 'axpby-bnull':
        lib.axpby(ptr(i['a']), None, ptr(out), n, lay.alpha, lay.beta, stream())
    else:
        lib.axpby(ptr(out), None, ptr(out), n, lay.alpha, lay.beta, stream())
    judge('vd_axpby' if op.startswith('axpby') else 'vd_' + op, lay, {s.name: host(out)})


# ------------------------------------------------------------------------------------------------------------ the embedding
@pytest.mark.parametrize("case", hc.GATHER, ids=IDS(hc.GATHER))
def test_embed_gather_cases(lib, case):
    lay = hc.gather_layout(case)
    i = dict((k, dev(v)) for k, v in lay.inp.items())
    out = dev(lay.specs[0].out0)
    lib.embed_gather(ptr(i['emb']), ptr(i['tok']), ptr(i.get('mask')), ptr(out), case.p['rows'], case.p['E'], lay.scale, stream())
    judge('vd_embed_gather', lay, {'out': host(out)})


@pytest.mark.parametrize("case", hc.SCATTER, ids=IDS(hc.SCATTER))
def test_embed_scatter_acc_cases(lib, case):
    lay = hc.scatter_layout(case)
    i = dict((k, dev(v)) for k, v in lay.inp.items())
    out = dev(lay.specs[0].out0)
    lib.embed_scatter_acc(ptr(out), ptr(i['tok']), ptr(i.get('mask')), ptr(i['dx']), case.p['rows'], case.p['E'], lay.scale, stream())
    judge('vd_embed_scatter_acc', lay, {'demb': host(out)})


@pytest.mark.parametrize("case", hc.MASKTIME, ids=IDS(hc.MASKTIME))
def test_mask_time_cases(lib, case):
    lay = hc.masktime_layout(case)
    T, N, D = (case.p[k] for k in 'TND')
    i = dict((k, dev(v)) for k, v in lay.inp.items())
    o = dict((k, dev(v)) for k, v in lay.out0().items())
    lib.mask_time_forward(ptr(i['feat']), ptr(i['tok']), ptr(o['out']), T, N, D, stream())
    lib.mask_time_backward(ptr(i['dout']), ptr(i['tok']), ptr(o['dfeat']), T, N, D, stream())
    outs = dict((k, host(v)) for k, v in o.items())
    judge('vd_mask_time_forward', lay, outs, ('out',))
    judge('vd_mask_time_backward', lay, outs, ('dfeat',))


# ------------------------------------------------------------------------------------------------------------ the zeroing kernels
@pytest.mark.parametrize("case", hc.ZERO_ROWS, ids=IDS(hc.ZERO_ROWS))
def test_zero_inactive_rows_cases(lib, case):
    """through the C entry point: ops.zero_inactive_rows only passes contiguous buffers"""
    lay = hc.zero_rows_layout(case)
    p = case.p
    nact, buf = dev(lay.inp['nact']), dev(lay.specs[0].out0)
    lib.zero_inactive_rows(ptr(buf), p['tstride'], p['ld'], p['ncols'], ptr(nact), p['T'], p['N'], stream())
    judge('vd_zero_inactive_rows', lay, {'buf': host(buf)})


@pytest.mark.parametrize("case", hc.ZERO_MULTI, ids=IDS(hc.ZERO_MULTI))
def test_zero_inactive_multi_cases(lib, case):
    lay = hc.zero_multi_layout(case)
    p = case.p
    nact = dev(lay.inp['nact'])
    bufs = [dev(s.out0) for s in lay.specs]
    z = VdZeroSet()
    z.n, z.quads_per_row = len(bufs), -1                       # (the launcher fills quads_per_row in)
    for k, b in enumerate(bufs):
        z.buf[k], z.ncols[k] = ptr(b), p['widths'][k]
    lib.zero_inactive_multi(C.byref(z), ptr(nact), p['T'], p['N'], stream())
    judge('vd_zero_inactive_multi', lay, dict(('buf%d' % k, host(b)) for k, b in enumerate(bufs)))


# ------------------------------------------------------------------------------------------------------------ token sort, segmented row sum
@pytest.mark.parametrize("case", hc.TOKEN_SORT, ids=IDS(hc.TOKEN_SORT))
def test_token_sort_cases(lib, case):
    lay = hc.token_sort_layout(case)
    tok = dev(lay.inp['tok'])
    o = dict((k, dev(v)) for k, v in lay.out0().items())
    lib.token_sort(ptr(tok), case.p['n'], case.p['V'], ptr(o['offset']), ptr(o['work']), ptr(o['perm']), stream())
    judge('vd_token_sort', lay, dict((k, host(v)) for k, v in o.items()))


@pytest.mark.parametrize("bf16", [False, True], ids=['fp32', 'bf16'])
@pytest.mark.parametrize("case", hc.SEGSUM, ids=IDS(hc.SEGSUM))
def test_segment_rowsum_acc_cases(lib, case, bf16):
    lay = hc.segsum_layout(case, bf16)
    p = case.p
    i = dict((k, dev(v)) for k, v in lay.inp.items())
    out = dev(lay.specs[0].out0)
    call = lib.segment_rowsum_acc_bf16 if bf16 else lib.segment_rowsum_acc
    call(ptr(i['X']), p['ldx'], ptr(i['tok']), ptr(i['perm']), p['n'], p['ncol'], ptr(out), p['ldo'], stream())
    judge('vd_segment_rowsum_acc_bf16' if bf16 else 'vd_segment_rowsum_acc', lay, {'out': host(out)})


# ------------------------------------------------------------------------------------------------------------ the heads
@pytest.mark.parametrize("case", hc.LOGSOFTMAX, ids=IDS(hc.LOGSOFTMAX))
def test_log_softmax_rows_cases(lib, case):
    lay = hc.logsoftmax_layout(case)
    x = dev(lay.specs[0].out0)
    lib.log_softmax_rows(ptr(x), case.p['V'] + case.p['pad'], case.p['rows'], case.p['V'], stream())
    judge('vd_log_softmax_rows', lay, {'x': host(x)})


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.mark.parametrize("eps,wg", hc.NLL_VARIANTS, ids=['eps%g-wg%d' % v for v in hc.NLL_VARIANTS])
@pytest.mark.parametrize("case", hc.NLL, ids=IDS(hc.NLL))
def test_logsoftmax_nll_cases(lib, case, eps, wg):
    lay = hc.nll_layout(case, eps, wg)
    V, ld = case.p['V'], case.p['V'] + case.p['pad']
    i = dict((k, dev(v)) for k, v in lay.inp.items())
    o = dict((k, dev(v)) for k, v in lay.out0().items())
    if eps:
        lib.logsoftmax_nll_p(ptr(o['logits']), ld, hc.NLL_ROWS, V, ptr(i['tok_in']), ptr(i['target']), ptr(o['loss']), wg, eps, stream())
    else:
        lib.logsoftmax_nll(ptr(o['logits']), ld, hc.NLL_ROWS, V, ptr(i['tok_in']), ptr(i['target']), ptr(o['loss']), wg, stream())
    outs = dict((k, host(v)) for k, v in o.items())
    if case.p['pad'] <= 3:
        key = '%s|eps%g|wg%d' % (case.id, eps, wg)
        PARENT[key] = [sha(outs['loss']), sha(outs['logits'])]
        if not os.environ.get('VD_HELPER_PARENT_OUT'):
            assert PARENT[key] == json.load(open(GOLDEN))[key], (key, 'loss or gradient differ in bits from the build before the pad-column loop')
    judge('vd_logsoftmax_nll_p' if eps else 'vd_logsoftmax_nll', lay, outs)


SCORE_RUNS = [(c, eps) for c in hc.SCORE for eps in (0.0, 0.1) if not (eps and c.p['mode'] == 'scores')]     # (the smoothed head needs gt: test_refusals)


@pytest.mark.parametrize("case,eps", SCORE_RUNS, ids=['%s-%s' % (c.id, 'eps0.1' if e else 'plain') for c, e in SCORE_RUNS])
def test_score_ce_cases(lib, case, eps):
    lay = hc.score_layout(case, eps)
    O, H, N, mode = (case.p[k] for k in ('O', 'H', 'N', 'mode'))
    i = dict((k, dev(v)) for k, v in lay.inp.items())
    o = dict((k, dev(v)) for k, v in lay.out0().items())
    gt = None if mode == 'scores' else ptr(i['gt'])
    dO, dE = (ptr(o['dOptH']), ptr(o['dEnc'])) if mode == 'train' else (None, None)
    if eps:
        lib.score_ce_p(ptr(i['optH']), ptr(i['enc']), gt, ptr(o['scores']), ptr(o['loss']), dO, dE, N, O, H, lay.gscale, eps, stream())
    else:
        lib.score_ce(ptr(i['optH']), ptr(i['enc']), gt, ptr(o['scores']), ptr(o['loss']), dO, dE, N, O, H, lay.gscale, stream())
    judge('vd_score_ce_p' if eps else 'vd_score_ce', lay, dict((k, host(v)) for k, v in o.items()))


@pytest.mark.parametrize("case", hc.RANKS, ids=IDS(hc.RANKS))
def test_ranks_cases(lib, case):
    lay = hc.ranks_layout(case)
    s, out = dev(lay.inp['scores']), dev(lay.specs[0].out0)
    lib.ranks(ptr(s), ptr(out), lay.N, case.p['O'], stream())
    judge('vd_ranks', lay, {'ranks': host(out)})


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals(lib):
    """every call here is refused by the host before any launch; what a refused call was given comes back bit for bit"""
    f = dev(np.random.RandomState(2).randn(4096).astype(np.float32))
    ints = dev(np.zeros(64, np.int32))
    out0 = np.full(4096, hc.MARK, np.float32)
    out = dev(out0)
    assert f.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    s, F, I, O = stream(), ptr(f), ptr(ints), ptr(out)
    align = "pointer must be 16-byte aligned and leading dimension a multiple of 4"

    def refused(call, words):
        with pytest.raises(lib.Error, match=re.escape(words)):
            call()
        assert np.array_equal(host(out).view(np.uint32), out0.view(np.uint32)), 'a refused call wrote'

    def score(optH=F, enc=F, gt=I, sc=O, loss=O, dO=O + 1024, dE=O + 2048, N=1, Opt=2, H=4):
        return lambda: lib.score_ce(optH, enc, gt, sc, loss, dO, dE, N, Opt, H, 1.0, s)

    def score_p(optH=F, enc=F, gt=I, dO=O + 1024, dE=O + 2048):
        return lambda: lib.score_ce_p(optH, enc, gt, O, O, dO, dE, 1, 2, 4, 1.0, 0.1, s)
    refused(score(Opt=129), "vd_score_ce: bad args (O=129 must be <= 128)")
    refused(score(H=6), "vd_score_ce: bad args")
    for kw in (dict(optH=F + 4), dict(enc=F + 8), dict(dO=O + 4), dict(dE=O + 12)):
        refused(score(**kw), "vd_score_ce: " + align)
        refused(score_p(**kw), "vd_score_ce_p: " + align)
    refused(score_p(gt=None), "vd_score_ce_p: bad args")
    refused(lambda: lib.embed_gather(F, I, None, O, 2, 6, 1.0, s), "vd_embed_gather: bad args (E=6)")
    refused(lambda: lib.embed_gather(F + 4, I, None, O, 2, 4, 1.0, s), "vd_embed_gather: " + align)
    refused(lambda: lib.embed_gather(F, I, None, O + 8, 2, 4, 1.0, s), "vd_embed_gather: " + align)
    refused(lambda: lib.embed_gather(F, I, I + 1, O, 2, 4, 1.0, s), "vd_embed_gather: the mask is read four bytes at a time")
    refused(lambda: lib.zero_inactive_rows(O, 16, 8, 6, I, 1, 2, s), "vd_zero_inactive_rows: bad args")
    refused(lambda: lib.zero_inactive_rows(O, 18, 8, 4, I, 1, 2, s), "vd_zero_inactive_rows: " + align)
    refused(lambda: lib.zero_inactive_rows(O + 4, 16, 8, 4, I, 1, 2, s), "vd_zero_inactive_rows: " + align)
    refused(lambda: lib.segment_rowsum_acc(F + 4, 4, I, I, 2, 4, O, 4, s), "vd_segment_rowsum_acc: " + align)
    refused(lambda: lib.segment_rowsum_acc(F, 6, I, I, 2, 4, O, 4, s), "vd_segment_rowsum_acc: bad args")
    refused(lambda: lib.segment_rowsum_acc_bf16(F, 4, I, I, 2, 0, O, 4, s), "vd_segment_rowsum_acc_bf16: bad args")
    refused(lambda: lib.segment_rowsum_acc_bf16(F + 4, 4, I, I, 2, 4, O, 4, s), "vd_segment_rowsum_acc_bf16: the rows are read four bf16 at a time")
    refused(lambda: lib.dropout_mask(O + 1, 4, 0, 0.5, s), "vd_dropout_mask: bad args")
    refused(lambda: lib.dropout_mask(O, 4, 0, 1.0, s), "vd_dropout_mask: bad args")


def test_helper_parity_figures_are_complete():
    """the last test of the module: the worst figures per entry point of everything that ran, each within its bound; after a whole run,
    every entry point with all its cases"""
    for entry, (n, ratio, err) in sorted(WORST.items()):
        print("%-28s %5d cases, worst error / bound %.5f, worst |err| %.3e" % (entry, n, ratio, err))
        assert n > 0 and ratio <= 1.0
    if set(WORST) == set(EXPECTED):
        assert dict((k, v[0]) for k, v in WORST.items()) == EXPECTED
