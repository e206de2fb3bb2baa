"""Operator parity for the image attention over a region count per image (csrc/attention.hip IR1 - IR6) against the fp64 restatement of
tests/region_ref.py (pinned to torch.autograd on the CPU by tests/test_region_ref_cpu.py).  The two internal entry points
vd_img_att_forward_p / vd_img_att_backward_p (declarations in csrc/rt_core.h) are bound by visdial_amd._lib.internal, as
tests/test_attention_ops_gpu.py binds the split products.

  1. the chain vd_img_common_forward -> vd_img_att_forward_p -> vd_img_att_backward_p -> vd_img_tr_backward -> vd_img_common_wgrad, each
     step fed the device's own earlier outputs, with finite garbage in the hidden rows of the features (the dense products read them);
  2. the four masked kernels alone with NaN in the hidden rows of iqc and pre: nothing comes back NaN, hidden p / dscore / dz are exact 0;
  3. full counts against the null-cnt call: p, u1, dscore, dz, dqc bit for bit (IR6), dwa / dba within the bound (atomics).

Shapes (B, R, S2, H, Kc): (7, 2, 49, 192, 144) with counts on either side of the 8 region groups of wsum / dz and of the 16 waves of
score / dscore, one region and a full image; (3, 1, 5, 4, 4): R = 1, the form of a round pass; (2, 2, 196, 320, 272): the real S2.
Bounds (tests/test_attention_ops_gpu.py's own): rel-L2 < 1e-5 per output and per named slice; dba, a sum that cancels in exact arithmetic,
to 1e-5 x the magnitudes it sums; 128 guard rows behind every output untouched."""
import functools
import types

import numpy as np
import pytest
import torch

import attention_ref as ar
import region_ref as rr

pytestmark = pytest.mark.gpu

BOUND = 1e-5
D = np.float64

CASES = [((7, 2, 49, 192, 144), (1, 8, 9, 16, 17, 48, 49)),
         ((3, 1, 5, 4, 4), (1, 3, 5)),
         ((2, 2, 196, 320, 272), (196, 100))]
IDS = ['S2=49', 'S2=5,R=1', 'S2=196']


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from visdial_amd import ops as o
    return o


@pytest.fixture(scope="module")
def head(ops):
    from visdial_amd import _lib
    return types.SimpleNamespace(forward=_lib.internal('vd_img_att_forward_p'), backward=_lib.internal('vd_img_att_backward_p'))


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def f32(rng, *shape):
    return rng.randn(*shape).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(shape, cnt, use_drop):
    """operands of one case and its fp64 forward / backward over the live regions.  The hidden rows of pre hold finite garbage (five times
    the live rows' range).  Shared between tests: read only."""
    B, R, S2, H, Kc = shape
    rng = np.random.RandomState(B * 1000003 + R * 10007 + S2 * 101 + H * 7 + Kc + int(use_drop))
    N = B * R
    c = types.SimpleNamespace(B=B, R=R, S2=S2, H=H, Kc=Kc, N=N, sc=2.0 if use_drop else 1.0, cnt=np.asarray(cnt, np.int32))
    c.live = rr.live_mask(cnt, B, R, S2)                                            # [N x S2]
    c.live_img = rr.live_mask(cnt, B, 1, S2).reshape(-1)                            # [B*S2]
    c.pre = np.tanh(f32(rng, B * S2, H))
    c.pre[~c.live_img] = 5.0 * f32(rng, int((~c.live_img).sum()), H)
    c.m1 = (rng.rand(N * S2, H) > 0.5).astype(np.uint8) if use_drop else None
    c.m2 = (rng.rand(N * S2, Kc) > 0.5).astype(np.uint8) if use_drop else None
    c.Wc, c.bc = f32(rng, Kc, H) / np.float32(np.sqrt(H)), f32(rng, Kc) * np.float32(0.1)
    c.qc = f32(rng, N, Kc) * np.float32(0.5)
    c.wa, c.ba = f32(rng, Kc) * np.float32(2.0 / np.sqrt(Kc)), f32(rng, 1)
    c.u0, c.datt = f32(rng, N, H), f32(rng, N, H)
    c.fwd = rr.region_forward(c.pre, c.m1, c.m2, c.Wc, c.bc, c.qc, c.wa, c.ba, c.u0, cnt, B, R, S2, c.sc)
    c.bwd = rr.region_backward(c.fwd, c.datt, c.m1, c.m2, c.Wc, c.wa, B, R, S2, c.sc)
    acc = lambda ref: (rng.randn(*np.shape(ref)) * 0.5 * max(float(np.sqrt((np.asarray(ref, D) ** 2).mean())), 1e-3)).astype(np.float32)
    c.dwa0, c.dpre0, c.dWc0 = acc(c.bwd['dwa']), acc(c.bwd['dpre']), acc(c.bwd['dWc'])
    c.name = '%s counts %s %s' % (shape, tuple(cnt), 'drop' if use_drop else 'no drop')
    return c


def upload(c, **over):
    d = {k: getattr(c, k) for k in ('pre', 'm1', 'm2', 'Wc', 'bc', 'qc', 'wa', 'ba', 'u0', 'datt', 'cnt')}
    d.update(over)
    return types.SimpleNamespace(**{k: dev(v) for k, v in d.items()})


def rows_slices(c, cols):
    return ar.tile_slices(c.N * c.S2, cols) + [ar.row_block('round N - 1', c.N - 1, c.S2), ar.row_block('round 0', 0, c.S2)]


def round_slices(c, cols):
    return ar.tile_slices(c.N, cols)[1:] + [ar.row_block('round N - 1', c.N - 1, 1), ar.row_block('round 0', 0, 1)]


def vec_slices(n):
    return [('last column tile', (slice((n - 1) // ar.TILE * ar.TILE, n),))]


def hidden_exact_zero(rep, name, got, hidden):
    """IR2 / IR4: every hidden element is an exact zero (of either sign for the gradients; +0.0 for p is checked by the caller)"""
    g = got.detach().cpu().numpy().reshape(hidden.shape[0], hidden.shape[1], -1)[hidden]
    n = int((g != 0).sum()) + int(np.isnan(g).sum())
    if n:
        rep.failures.append('%s %s: %d hidden elements are not exact zeros' % (rep.what, name, n))


def no_nan(rep, name, got):
    n = int(torch.isnan(got).sum().item())
    if n:
        rep.failures.append('%s %s: %d NaN' % (rep.what, name, n))


# ------------------------------------------------------------------------------------------------------------ 1. the chain
@pytest.mark.parametrize("use_drop", [False, True], ids=['nodrop', 'drop'])
@pytest.mark.parametrize("shape,cnt", CASES, ids=IDS)
def test_region_attention_chain(ops, head, shape, cnt, use_drop):
    c = case(shape, cnt, use_drop)
    d = upload(c)
    B, R, S2, H, Kc, N, sc = c.B, c.R, c.S2, c.H, c.Kc, c.N, c.sc
    hid = ~c.live
    assert hid.any()
    rep = ar.Report('regions chain %s:' % c.name)
    iqc = ar.Guarded((N * S2, Kc))
    ops.img_common_forward(d.pre, d.m1, d.Wc, d.bc, d.qc, d.m2, iqc.t, N, R, S2, H, Kc, sc)
    rep.close('iqc', iqc, c.fwd['iqc'], BOUND, rows_slices(c, Kc))                  # every row: the dense product is unmasked (IR5)
    p, u1 = ar.Guarded((N, S2)), ar.Guarded((N, H))
    head.forward(ptr(iqc.t), ptr(d.wa), ptr(d.ba), ptr(d.pre), ptr(d.m1), ptr(d.u0), ptr(p.t), ptr(u1.t), N, R, S2, H, Kc, sc, ptr(d.cnt),
                 stream())
    rep.close('p', p, c.fwd['p'], BOUND, [ar.row_block('round N - 1', N - 1, 1), ar.row_block('round 0', 0, 1)])
    rep.close('u1', u1, c.fwd['u1'], BOUND, round_slices(c, H))
    hidden_exact_zero(rep, 'p', p.t, hid)
    pn = p.t.cpu().numpy()
    assert not np.signbit(pn[hid]).any(), 'p of a hidden region is +0.0'
    rep.guard('iqc', iqc)

    dwa, dba = ar.Guarded((Kc,), init=c.dwa0), ar.Guarded((1,), init=[0.25])
    dqc, work = ar.Guarded((N, Kc)), ar.Guarded((N, S2))
    head.backward(ptr(iqc.t), ptr(d.wa), ptr(d.pre), ptr(d.m1), ptr(d.m2), ptr(p.t), ptr(d.datt), ptr(dwa.t), ptr(dba.t), ptr(dqc.t),
                  ptr(work.t), N, R, S2, H, Kc, sc, ptr(d.cnt), stream())
    rep.close('dz', iqc, c.bwd['dz'], BOUND, rows_slices(c, Kc))
    rep.close('dscore', work, c.bwd['dscore'], BOUND, [ar.row_block('round N - 1', N - 1, 1), ar.row_block('round 0', 0, 1)])
    hidden_exact_zero(rep, 'dz', iqc.t, hid)
    hidden_exact_zero(rep, 'dscore', work.t, hid)
    rep.close('dwa', dwa, c.dwa0.astype(D) + c.bwd['dwa'], BOUND, vec_slices(Kc))
    rep.scalar('dba', dba.t.item(), 0.25 + c.bwd['dba'], BOUND * np.abs(c.bwd['dscore']).sum())
    rep.close('dqc', dqc, c.bwd['dqc'], BOUND, round_slices(c, Kc))
    dpre = ar.Guarded((B * S2, H), init=c.dpre0)
    ops.img_tr_backward(iqc.t, d.Wc, p.t, d.datt, d.m1, dpre.t, N, R, S2, H, Kc, sc)
    rep.close('dpre', dpre, c.dpre0.astype(D) + c.bwd['dpre'], BOUND,
              ar.tile_slices(B * S2, H) + [ar.row_block('image B - 1', B - 1, S2), ar.row_block('image 0', 0, S2)])
    # a hidden row of an image receives 0 * finite: its accumulator keeps its initial value bit for bit
    got = dpre.t.cpu().numpy()
    assert np.array_equal(got[~c.live_img], c.dpre0[~c.live_img]), 'dpre of a hidden row moved'
    dWc = ar.Guarded((Kc, H), init=c.dWc0)
    ops.img_common_wgrad(iqc.t, d.pre, d.m1, dWc.t, N, R, S2, H, Kc, sc)
    rep.close('dWc', dWc, c.dWc0.astype(D) + c.bwd['dWc'], BOUND, ar.tile_slices(Kc, H))
    for name, out in (('iqc/dz', iqc), ('p', p), ('u1', u1), ('dwa', dwa), ('dba', dba), ('dqc', dqc), ('work', work), ('dpre', dpre),
                      ('dWc', dWc)):
        rep.guard(name, out)
    rep.ok()


# ------------------------------------------------------------------------------------------------------------ 2. hidden rows are never read
@pytest.mark.parametrize("use_drop", [False, True], ids=['nodrop', 'drop'])
@pytest.mark.parametrize("shape,cnt", CASES, ids=IDS)
def test_masked_kernels_never_read_a_hidden_row(head, shape, cnt, use_drop):
    """the four masked kernels alone, on the reference's own iqc: NaN in every hidden row of iqc and of pre"""
    c = case(shape, cnt, use_drop)
    B, R, S2, H, Kc, N, sc = c.B, c.R, c.S2, c.H, c.Kc, c.N, c.sc
    hid = ~c.live
    pre = c.pre.copy()
    pre[~c.live_img] = np.nan
    iqc_in = c.fwd['iqc'].astype(np.float32)
    iqc_in[hid.reshape(-1)] = np.nan
    d = upload(c, pre=pre)
    # what the head gives from this (fp32-rounded) iqc: the reference on the same values
    live_iqc = np.where(c.live.reshape(-1)[:, None], iqc_in, 0.0)
    pr, u1r = rr.region_attend(live_iqc, c.fwd['img_tr'], c.wa, c.ba, c.u0, c.live)
    ref = rr.region_head_backward(live_iqc, c.fwd['img_tr'], pr, c.datt, c.m2, c.wa, c.live, sc)
    rep = ar.Report('regions NaN %s:' % c.name)
    iqc = ar.Guarded((N * S2, Kc), init=iqc_in)
    p, u1 = ar.Guarded((N, S2)), ar.Guarded((N, H))
    head.forward(ptr(iqc.t), ptr(d.wa), ptr(d.ba), ptr(d.pre), ptr(d.m1), ptr(d.u0), ptr(p.t), ptr(u1.t), N, R, S2, H, Kc, sc, ptr(d.cnt),
                 stream())
    rep.close('p', p, pr, BOUND)
    rep.close('u1', u1, u1r, BOUND, round_slices(c, H))
    hidden_exact_zero(rep, 'p', p.t, hid)
    dwa, dba = ar.Guarded((Kc,), init=c.dwa0), ar.Guarded((1,), init=[0.25])
    dqc, work = ar.Guarded((N, Kc)), ar.Guarded((N, S2))
    head.backward(ptr(iqc.t), ptr(d.wa), ptr(d.pre), ptr(d.m1), ptr(d.m2), ptr(p.t), ptr(d.datt), ptr(dwa.t), ptr(dba.t), ptr(dqc.t),
                  ptr(work.t), N, R, S2, H, Kc, sc, ptr(d.cnt), stream())
    for name, out in (('p', p), ('u1', u1), ('dz', iqc), ('dscore', work), ('dqc', dqc), ('dwa', dwa), ('dba', dba)):
        no_nan(rep, name, out.t)
        rep.guard(name, out)
    hidden_exact_zero(rep, 'dz', iqc.t, hid)
    hidden_exact_zero(rep, 'dscore', work.t, hid)
    rep.close('dz', iqc, ref['dz'], BOUND, rows_slices(c, Kc))
    rep.close('dscore', work, ref['dscore'], BOUND)
    rep.close('dqc', dqc, ref['dqc'], BOUND, round_slices(c, Kc))
    rep.close('dwa', dwa, c.dwa0.astype(D) + ref['dwa'], BOUND, vec_slices(Kc))
    rep.scalar('dba', dba.t.item(), 0.25 + ref['dba'], BOUND * np.abs(ref['dscore']).sum())
    rep.ok()


# ------------------------------------------------------------------------------------------------------------ 3. IR6
@pytest.mark.parametrize("use_drop", [False, True], ids=['nodrop', 'drop'])
@pytest.mark.parametrize("shape,cnt", CASES, ids=IDS)
def test_full_counts_are_the_unmasked_kernels_bit_for_bit(ops, head, shape, cnt, use_drop):
    c = case(shape, cnt, use_drop)
    B, R, S2, H, Kc, N, sc = c.B, c.R, c.S2, c.H, c.Kc, c.N, c.sc
    d = upload(c, cnt=np.full(B, S2, np.int32))
    rep = ar.Report('regions full counts %s:' % c.name)
    iqc0 = torch.empty(N * S2, Kc, device='cuda')
    ops.img_common_forward(d.pre, d.m1, d.Wc, d.bc, d.qc, d.m2, iqc0, N, R, S2, H, Kc, sc)
    outs = {}
    for key, cp in (('null', None), ('full', ptr(d.cnt))):
        iqc = ar.Guarded((N * S2, Kc), init=iqc0.cpu().numpy())
        p, u1 = ar.Guarded((N, S2)), ar.Guarded((N, H))
        head.forward(ptr(iqc.t), ptr(d.wa), ptr(d.ba), ptr(d.pre), ptr(d.m1), ptr(d.u0), ptr(p.t), ptr(u1.t), N, R, S2, H, Kc, sc, cp, stream())
        dwa, dba = ar.Guarded((Kc,), init=c.dwa0), ar.Guarded((1,), init=[0.25])
        dqc, work = ar.Guarded((N, Kc)), ar.Guarded((N, S2))
        head.backward(ptr(iqc.t), ptr(d.wa), ptr(d.pre), ptr(d.m1), ptr(d.m2), ptr(p.t), ptr(d.datt), ptr(dwa.t), ptr(dba.t), ptr(dqc.t),
                      ptr(work.t), N, R, S2, H, Kc, sc, cp, stream())
        outs[key] = dict(p=p, u1=u1, dscore=work, dz=iqc, dqc=dqc, dwa=dwa, dba=dba)
        for name, out in outs[key].items():
            rep.guard(key + ' ' + name, out)
    for name in ('p', 'u1', 'dscore', 'dz', 'dqc'):
        a, b = outs['null'][name].t.cpu().numpy(), outs['full'][name].t.cpu().numpy()
        if not np.array_equal(a.view(np.uint32), b.view(np.uint32)):
            rep.failures.append('%s %s: %d elements differ from the null-cnt call (bit for bit expected)'
                                % (rep.what, name, int((a.view(np.uint32) != b.view(np.uint32)).sum())))
    assert not torch.isnan(outs['full']['dz'].t).any()
    dscore_abs = float(outs['null']['dscore'].t.abs().sum().item())
    rep.close('dwa', outs['full']['dwa'], outs['null']['dwa'].t, BOUND, vec_slices(Kc))
    rep.scalar('dba', outs['full']['dba'].t.item(), outs['null']['dba'].t.item(), BOUND * dscore_abs)
    rep.ok()


def test_the_entry_points_refuse_bad_arguments(head):
    from visdial_amd import _lib
    x = torch.zeros(64, device='cuda')
    cnt = torch.ones(1, dtype=torch.int32, device='cuda')
    with pytest.raises(_lib.VisdialHipError, match='vd_img_att_forward_p: bad args'):
        head.forward(ptr(x), ptr(x), ptr(x), ptr(x), None, ptr(x), ptr(x), ptr(x), 1, 0, 4, 4, 4, 1.0, ptr(cnt), stream())       # R = 0
    with pytest.raises(_lib.VisdialHipError, match='vd_img_att_backward_p: bad args'):
        head.backward(ptr(x), ptr(x), ptr(x), None, None, ptr(x), ptr(x), ptr(x), ptr(x), ptr(x), ptr(x), 1, 1, 4, 4, 6, 1.0, ptr(cnt),
                      stream())                                                                                                   # Kc % 4
    # the C ABI is the same body with a null cnt: R = 0 is refused under the name that was called, before any kernel divides by it
    with pytest.raises(_lib.VisdialHipError, match='vd_img_att_forward: bad args'):
        _lib.call('vd_img_att_forward', ptr(x), ptr(x), ptr(x), ptr(x), None, ptr(x), ptr(x), ptr(x), 1, 0, 4, 4, 4, 1.0, stream())
    with pytest.raises(_lib.VisdialHipError, match='vd_img_att_backward: bad args'):
        _lib.call('vd_img_att_backward', ptr(x), ptr(x), ptr(x), None, None, ptr(x), ptr(x), ptr(x), ptr(x), ptr(x), ptr(x), 1, 0, 4, 4, 4, 1.0,
                  stream())
