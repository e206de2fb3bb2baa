"""Operator parity for csrc/attention.hip against the fp64 restatements of tests/attention_ref.py (pinned to torch.autograd on the CPU by
tests/test_attention_ref_cpu.py):

  1. the five fp32 image-attention entry points as a chain, at the shapes that reach the second column tile of img_att_wsum_kernel /
     img_att_dz_kernel, the second trip of the 256-strided loops of img_att_score_kernel / img_att_dscore_kernel, S2 = 196, the smallest
     legal widths and eight column tiles;
  2. the dense products of a split9 pass operator by operator -- vd_img_drop_gather, vd_img_common_forward_p, vd_img_tr_backward_p,
     vd_img_common_wgrad_p (internal: bound by visdial_amd._lib.internal, declarations in csrc/rt_core.h) -- on ragged
     row / column tiles, the XCD grid map, the 128-row threshold, ragged transposes, the evaluation form, the tail contraction and
     every fall-back of the weight gradient; each against fp64 AND against the fp32 entry point on the same inputs;
  3. vd_hrea_attention_*, vd_rowdot_*, vd_mn_attention_* and the LDS guards of the latter.

Bounds (the project's: test_ops_gpu.py, test_lstm_forward_backward_split9): rel-L2 < 1e-5 against fp64 for every output of an fp32 entry
point AND of a split product, over the whole tensor and over each named slice (last ragged 128-row tile, last ragged 128-column tile,
rows of round N - 1, rows of image B - 1 for dpre); gathers and integer results bit for bit.  A sum that cancels to zero in exact arithmetic
(dba = sum of dscore; dsq[i] = sum_j dA[i, j]) is held to 1e-5 x the sum of the magnitudes it adds up, which is what its fp32 rounding
error scales with; no other output is.  Every written or accumulated output lies in front of 128
guard rows that must stay untouched.  The split-versus-fp32 error ratio is printed, not asserted."""
import functools
import types

import numpy as np
import pytest
import torch

import attention_ref as ar
from oracle import visdial_oracle as vo

pytestmark = pytest.mark.gpu

BOUND = 1e-5
D = np.float64


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from visdial_amd import ops as o
    return o


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def f32(rng, *shape):
    return rng.randn(*shape).astype(np.float32)


def acc_init(rng, ref):
    """non-zero initial values of an accumulated output, half the rms of what is added: an error of the sum cannot hide behind them"""
    ref = np.asarray(ref, D)
    return (rng.randn(*ref.shape) * 0.5 * max(float(np.sqrt((ref ** 2).mean())), 1e-3)).astype(np.float32)


def ptr(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def internal(ops):
    """the four internal entry points of a split9 pass (csrc/rt_core.h), bound by visdial_amd._lib.internal"""
    from visdial_amd import _lib
    return types.SimpleNamespace(
        drop_gather=_lib.internal('vd_img_drop_gather'), common_forward=_lib.internal('vd_img_common_forward_p'),
        tr_backward=_lib.internal('vd_img_tr_backward_p'), common_wgrad=_lib.internal('vd_img_common_wgrad_p'))


def split_ok(rows, H, Kc):
    """csrc/paths.h vd_img_split_ok at these sizes"""
    return rows >= 128 and H % 16 == 0 and Kc % 16 == 0


# ------------------------------------------------------------------------------------------------------------ inputs + fp64, once per case
@functools.lru_cache(maxsize=None)
def img_case(B, R, S2, H, Kc, use_drop):
    """asymmetric random operands of one image-attention case and its fp64 forward / backward.  Shared between tests: read only."""
    rng = np.random.RandomState(B * 1000003 + R * 10007 + S2 * 101 + H * 7 + Kc + int(use_drop))
    N = B * R
    c = types.SimpleNamespace(B=B, R=R, S2=S2, H=H, Kc=Kc, N=N, sc=2.0 if use_drop else 1.0)
    c.pre = np.tanh(f32(rng, B * S2, H))
    c.m1 = (rng.rand(N * S2, H) > 0.5).astype(np.uint8) if use_drop else None
    c.m2 = (rng.rand(N * S2, Kc) > 0.5).astype(np.uint8) if use_drop else None
    c.Wc, c.bc = f32(rng, Kc, H) / np.float32(np.sqrt(H)), f32(rng, Kc) * np.float32(0.1)
    c.qc = f32(rng, N, Kc) * np.float32(0.5)
    c.wa, c.ba = f32(rng, Kc) * np.float32(2.0 / np.sqrt(Kc)), f32(rng, 1)
    c.u0, c.datt = f32(rng, N, H), f32(rng, N, H)
    c.fwd = ar.img_forward(c.pre, c.m1, c.m2, c.Wc, c.bc, c.qc, c.wa, c.ba, c.u0, B, R, S2, c.sc)
    c.bwd = ar.img_backward(c.fwd, c.datt, c.m1, c.m2, c.Wc, c.wa, B, R, S2, c.sc)
    c.xdrop = c.fwd['img_tr'].astype(np.float32)                      # exact: pre * {0, 1, 2}
    assert np.array_equal(c.xdrop.astype(D), c.fwd['img_tr'])
    c.dwa0, c.dpre0, c.dWc0 = acc_init(rng, c.bwd['dwa']), acc_init(rng, c.bwd['dpre']), acc_init(rng, c.bwd['dWc'])
    c.name = '(%d, %d, %d, %d, %d) %s' % (B, R, S2, H, Kc, 'drop' if use_drop else 'no drop')
    return c


def upload(c):
    return types.SimpleNamespace(**{k: dev(getattr(c, k)) for k in ('pre', 'm1', 'm2', 'Wc', 'bc', 'qc', 'wa', 'ba', 'u0', 'datt')})


def rows_slices(c, cols):
    """of a [N*S2 x cols] tensor: the ragged last row tile, the ragged last column tile, the rows of round N - 1"""
    return ar.tile_slices(c.N * c.S2, cols) + [ar.row_block('round N - 1', c.N - 1, c.S2)]


def round_slices(c, cols):
    """of a [N x cols] tensor: the ragged last column tile, the row of round N - 1"""
    return ar.tile_slices(c.N, cols)[1:] + [ar.row_block('round N - 1', c.N - 1, 1)]


def vec_slices(n):
    return [('last column tile', (slice((n - 1) // ar.TILE * ar.TILE, n),))]


def dpre_slices(c):
    return ar.tile_slices(c.B * c.S2, c.H) + [ar.row_block('image B - 1', c.B - 1, c.S2)]


# ------------------------------------------------------------------------------------------------------------ 1. the fp32 chain
IMG_CASES = [(2, 3, 49, 192, 144),      # second, half-empty column tile of wsum and dz; ragged row tile (294 rows)
             (1, 2, 196, 320, 272),     # second trip of both 256-strided loops on a partial wave; the real S2
             (3, 1, 5, 4, 4),           # smallest legal widths, S2 below the wave count
             (2, 3, 50, 64, 1024)]      # eight column tiles


@pytest.mark.parametrize("use_drop", [False, True])
@pytest.mark.parametrize("B,R,S2,H,Kc", IMG_CASES)
def test_image_attention_fp32_chain(ops, B, R, S2, H, Kc, use_drop):
    """vd_img_common_forward -> vd_img_att_forward -> vd_img_att_backward -> vd_img_tr_backward -> vd_img_common_wgrad, each fed the
    device's own earlier outputs as in a step"""
    c = img_case(B, R, S2, H, Kc, use_drop)
    d = upload(c)
    N, sc = c.N, c.sc
    rep = ar.Report('fp32 chain %s:' % c.name)
    iqc = ar.Guarded((N * S2, Kc))
    ops.img_common_forward(d.pre, d.m1, d.Wc, d.bc, d.qc, d.m2, iqc.t, N, R, S2, H, Kc, sc)
    rep.close('iqc', iqc, c.fwd['iqc'], BOUND, rows_slices(c, Kc))
    p, u1 = ar.Guarded((N, S2)), ar.Guarded((N, H))
    ops.img_att_forward(iqc.t, d.wa, d.ba, d.pre, d.m1, d.u0, p.t, u1.t, N, R, S2, H, Kc, sc)
    rep.close('p', p, c.fwd['p'], BOUND, [ar.row_block('round N - 1', N - 1, 1)])
    rep.close('u1', u1, c.fwd['u1'], BOUND, round_slices(c, H))
    rep.guard('iqc', iqc)

    dwa, dba = ar.Guarded((Kc,), init=c.dwa0), ar.Guarded((1,), init=[0.25])
    dqc, work = ar.Guarded((N, Kc)), ar.Guarded((N, S2))
    ops.img_att_backward(iqc.t, d.wa, d.pre, d.m1, d.m2, p.t, d.datt, dwa.t, dba.t, dqc.t, work.t, N, R, S2, H, Kc, sc)
    rep.close('dz', iqc, c.bwd['dz'], BOUND, rows_slices(c, Kc))
    rep.close('dscore', work, c.bwd['dscore'], BOUND, [ar.row_block('round N - 1', N - 1, 1)])
    rep.close('dwa', dwa, c.dwa0.astype(D) + c.bwd['dwa'], BOUND, vec_slices(Kc))
    rep.scalar('dba', dba.t.item(), 0.25 + c.bwd['dba'], BOUND * np.abs(c.bwd['dscore']).sum())
    rep.close('dqc', dqc, c.bwd['dqc'], BOUND, round_slices(c, Kc))
    dpre = ar.Guarded((B * S2, H), init=c.dpre0)
    ops.img_tr_backward(iqc.t, d.Wc, p.t, d.datt, d.m1, dpre.t, N, R, S2, H, Kc, sc)
    rep.close('dpre', dpre, c.dpre0.astype(D) + c.bwd['dpre'], BOUND, dpre_slices(c))
    dWc = ar.Guarded((Kc, H), init=c.dWc0)
    ops.img_common_wgrad(iqc.t, d.pre, d.m1, dWc.t, N, R, S2, H, Kc, sc)
    rep.close('dWc', dWc, c.dWc0.astype(D) + c.bwd['dWc'], BOUND, ar.tile_slices(Kc, H))
    for name, out in (('iqc/dz', iqc), ('p', p), ('u1', u1), ('dwa', dwa), ('dba', dba), ('dqc', dqc), ('work', work), ('dpre', dpre),
                      ('dWc', dWc)):
        rep.guard(name, out)
    rep.ok()


# ------------------------------------------------------------------------------------------------------------ 2. the split products
GATHER_SHAPE, GATHER_H = (2, 3, 49), [4, 192]


def gather_inputs(H, use_mask):
    B, R, S2 = GATHER_SHAPE
    rng = np.random.RandomState(H + int(use_mask))
    pre = f32(rng, B * S2, H)
    return pre, (rng.rand(B * R * S2, H) > 0.5).astype(np.uint8) if use_mask else None


@pytest.mark.parametrize("use_mask", [False, True])
@pytest.mark.parametrize("H", GATHER_H)
def test_img_drop_gather_is_the_gather_bit_for_bit(ops, internal, H, use_mask):
    B, R, S2 = GATHER_SHAPE
    N = B * R
    pre, m1 = gather_inputs(H, use_mask)
    rows = ((np.arange(N) // R)[:, None] * S2 + np.arange(S2)[None, :]).reshape(-1)
    want = pre[rows]
    if use_mask:
        want = np.where(m1 != 0, want * np.float32(2.0), np.float32(0.0))
    assert np.array_equal(want.astype(D), ar.img_gather_drop(pre, m1, B, R, S2, 2.0))      # the helper's gather says the same
    out = ar.Guarded((N * S2, H))
    pre_d, m1_d = dev(pre), dev(m1)                       # (named: a temporary would be freed, and its block reused, before the launch)
    internal.drop_gather(ptr(pre_d), ptr(m1_d), ptr(out.t), N, R, S2, H, 2.0, stream())
    rep = ar.Report('drop_gather H = %d mask = %s:' % (H, use_mask))
    rep.exact('xdrop', out.t, want)
    assert want.dtype == np.float32 and np.array_equal(out.t.cpu().numpy().view(np.uint32), want.view(np.uint32))     # the bits themselves
    rep.guard('xdrop', out)
    rep.ok()


SPLIT_CASES = [(2, 3, 49, 192, 144),    # ragged row tile (294 rows) and ragged column tile in both products
               (1, 2, 196, 320, 272),
               (2, 3, 50, 64, 1024),    # forward: 8 column tiles -> the XCD grid map, 3 row tiles over 4 row groups
               (2, 4, 16, 48, 80),      # exactly 128 rows; H, Kc multiples of 16 but not of 32: ragged transposes in both directions
               (1, 1, 127, 48, 80),     # 127 rows: below the threshold
               (2, 3, 49, 36, 20)]      # H % 16 != 0


def ratio_line(what, name, e9, e32):
    print('RATIO %s %s: fp32 %.3e split9 %.3e split9/fp32 %.2f' % (what, name, e32, e9, e9 / max(e32, 1e-30)))


@pytest.mark.parametrize("use_drop", [False, True])
@pytest.mark.parametrize("B,R,S2,H,Kc", SPLIT_CASES)
def test_split9_forward_and_tr_backward(ops, internal, B, R, S2, H, Kc, use_drop):
    """vd_img_common_forward_p and vd_img_tr_backward_p with VD_FLAG_SPLIT9, each on the fp64 reference's own inputs (rounded to fp32:
    6e-8, far inside the bound), beside the fp32 entry point on the same inputs"""
    c = img_case(B, R, S2, H, Kc, use_drop)
    d = upload(c)
    N, sc = c.N, c.sc
    ok = split_ok(N * S2, H, Kc)
    what = 'split9 %s%s:' % (c.name, '' if ok else ' (falls back)')
    rep = ar.Report(what)
    xdrop = dev(c.xdrop)
    iqc32, iqc9 = ar.Guarded((N * S2, Kc)), ar.Guarded((N * S2, Kc))
    ops.img_common_forward(d.pre, d.m1, d.Wc, d.bc, d.qc, d.m2, iqc32.t, N, R, S2, H, Kc, sc)
    internal.common_forward(ptr(d.pre), ptr(d.m1), ptr(xdrop), ptr(d.Wc), ptr(d.bc), ptr(d.qc), ptr(d.m2), ptr(iqc9.t), N, R, S2, H, Kc, sc,
                            ops.FLAG_SPLIT9, stream())
    e32 = rep.close('iqc fp32', iqc32, c.fwd['iqc'], BOUND, rows_slices(c, Kc))
    e9 = rep.close('iqc split9', iqc9, c.fwd['iqc'], BOUND, rows_slices(c, Kc))
    ratio_line(what, 'iqc', e9, e32)
    if not ok:
        rep.exact('iqc (the same deterministic kernel)', iqc9.t, iqc32.t)
    else:
        assert not torch.equal(iqc9.t, iqc32.t)          # the split kernel ran: another summation order cannot give 4e4 equal roundings
    dz, p = dev(c.bwd['dz'].astype(np.float32)), dev(c.fwd['p'].astype(np.float32))
    dpre32, dpre9 = ar.Guarded((B * S2, H), init=c.dpre0), ar.Guarded((B * S2, H), init=c.dpre0)
    ops.img_tr_backward(dz, d.Wc, p, d.datt, d.m1, dpre32.t, N, R, S2, H, Kc, sc)
    internal.tr_backward(ptr(dz), ptr(d.Wc), ptr(p), ptr(d.datt), ptr(d.m1), ptr(dpre9.t), N, R, S2, H, Kc, sc, ops.FLAG_SPLIT9, stream())
    ref = c.dpre0.astype(D) + c.bwd['dpre']
    e32 = rep.close('dpre fp32', dpre32, ref, BOUND, dpre_slices(c))
    e9 = rep.close('dpre split9', dpre9, ref, BOUND, dpre_slices(c))
    ratio_line(what, 'dpre', e9, e32)
    # Which path dpre took cannot be read off its bits in general: EpiImgTrBwd accumulates the R rounds of an image with float atomics, in
    # either kernel, so two runs of ONE kernel may differ in the last bit.  With R = 1 every element receives one addition: there the
    # fall-back must repeat the fp32 entry point exactly.
    if not ok and R == 1:
        rep.exact('dpre (the same kernel, one addition per element)', dpre9.t, dpre32.t)
    for name, out in (('iqc fp32', iqc32), ('iqc split9', iqc9), ('dpre fp32', dpre32), ('dpre split9', dpre9)):
        rep.guard(name, out)
    rep.ok()


def test_split9_forward_in_the_evaluation_form(ops, internal):
    """csrc/rt_encoders.h forward_round: `pre` itself is the dropped image tensor, R = 1, no masks, scale 1"""
    B, R, S2, H, Kc = 6, 1, 49, 192, 144
    c = img_case(B, R, S2, H, Kc, False)
    d = upload(c)
    what = 'split9 evaluation form %s:' % c.name
    rep = ar.Report(what)
    iqc32, iqc9 = ar.Guarded((B * S2, Kc)), ar.Guarded((B * S2, Kc))
    ops.img_common_forward(d.pre, None, d.Wc, d.bc, d.qc, None, iqc32.t, B, 1, S2, H, Kc, 1.0)
    internal.common_forward(ptr(d.pre), None, ptr(d.pre), ptr(d.Wc), ptr(d.bc), ptr(d.qc), None, ptr(iqc9.t), B, 1, S2, H, Kc, 1.0,
                            ops.FLAG_SPLIT9, stream())
    e32 = rep.close('iqc fp32', iqc32, c.fwd['iqc'], BOUND, rows_slices(c, Kc))
    e9 = rep.close('iqc split9', iqc9, c.fwd['iqc'], BOUND, rows_slices(c, Kc))
    ratio_line(what, 'iqc', e9, e32)
    assert not torch.equal(iqc9.t, iqc32.t)              # the split kernel ran (no quiet fall-back, `pre` arrived as xdrop)
    rep.guard('iqc fp32', iqc32)
    rep.guard('iqc split9', iqc9)
    rep.ok()


WGRAD_CASES = [  # what, (B, R, S2), H, Kc, xdrop given, takes the split contraction
    ('K = 1029: tail of 5 rows', (7, 3, 49), 128, 256, True, True),
    ('K = 1024: the threshold, no tail', (8, 4, 32), 128, 256, True, True),
    ('K = 1077: 67 steps, ragged last K range, empty workgroups, tail of 5', (1, 3, 359), 128, 256, True, True),
    ('K = 1023: below the threshold', (31, 1, 33), 128, 256, True, False),
    ('K = 1029, 2 x 2 tiles', (7, 3, 49), 256, 512, True, True),
    ('K = 1029, tiles do not fit', (7, 3, 49), 192, 256, True, False),
    ('K = 1029, null xdrop', (7, 3, 49), 128, 256, False, False)]


@pytest.mark.parametrize("what,shape,H,Kc,with_xdrop,split", WGRAD_CASES, ids=[w[0].split(':')[0] for w in WGRAD_CASES])
def test_split9_weight_gradient(ops, internal, what, shape, H, Kc, with_xdrop, split):
    """vd_img_common_wgrad_p with VD_FLAG_SPLIT9: dWc += dz^T img_tr, accumulated onto a non-zero dWc"""
    B, R, S2 = shape
    N, K = B * R, B * R * S2
    rng = np.random.RandomState(K + H + Kc + int(with_xdrop))
    pre = np.tanh(f32(rng, B * S2, H))
    m1 = (rng.rand(K, H) > 0.5).astype(np.uint8)
    dz = f32(rng, K, Kc) * np.float32(0.1)
    img_tr = ar.img_gather_drop(pre, m1, B, R, S2, 2.0)
    inc = dz.astype(D).T @ img_tr
    dWc0 = acc_init(rng, inc)
    ref = dWc0.astype(D) + inc
    pre_d, m1_d, dz_d = dev(pre), dev(m1), dev(dz)
    xdrop = dev(img_tr.astype(np.float32)) if with_xdrop else None
    dWc32, dWc9 = ar.Guarded((Kc, H), init=dWc0), ar.Guarded((Kc, H), init=dWc0)
    ops.img_common_wgrad(dz_d, pre_d, m1_d, dWc32.t, N, R, S2, H, Kc, 2.0)
    internal.common_wgrad(ptr(dz_d), ptr(pre_d), ptr(m1_d), ptr(xdrop), ptr(dWc9.t), N, R, S2, H, Kc, 2.0, ops.FLAG_SPLIT9, stream())
    what = 'split9 wgrad Kc = %d H = %d %s:' % (Kc, H, what)
    rep = ar.Report(what)
    e32 = rep.close('dWc fp32', dWc32, ref, BOUND, ar.tile_slices(Kc, H))
    e9 = rep.close('dWc split9', dWc9, ref, BOUND, ar.tile_slices(Kc, H))
    ratio_line(what, 'dWc', e9, e32)
    # The split contraction ran where it should.  That a fall-back (K < 1024, tiles that do not fit, null xdrop) took the fp32 kernel is NOT
    # checked by bits: that kernel splits K over workgroups and adds the partial sums with float atomics, so it need not repeat itself.
    assert not split or not torch.equal(dWc9.t, dWc32.t)
    rep.guard('dWc fp32', dWc32)
    rep.guard('dWc split9', dWc9)
    rep.ok()


# ------------------------------------------------------------------------------------------------------------ 3. hrea, rowdot, mn
HREA_CASES = [(1, 1, 4), (3, 10, 36), (2, 16, 512), (5, 10, 512)]
MN_CASES = [(1, 1, 4), (3, 10, 36), (7, 10, 512)]


def hrea_inputs(B, R, H):
    rng = np.random.RandomState(B * 100 + R * 10 + H)
    sq, sh, h, datt = f32(rng, B, R), f32(rng, B, R), f32(rng, B, R, H) * np.float32(0.5), f32(rng, B, R, H)
    if R > 1:
        sh[0, 1] = -sq[0, R - 1]                 # dialog 0, round R - 1, fact 1 (visible): an exact zero -> ReplaceZero(-inf)
        assert sq[0, R - 1] + sh[0, 1] == 0.0
    return sq, sh, h, datt


@pytest.mark.parametrize("B,R,H", HREA_CASES)
def test_hrea_attention(ops, B, R, H):
    N = B * R
    sq, sh, h, datt = hrea_inputs(B, R, H)
    P_ref, att_ref = ar.hrea_forward(sq, sh, h)
    dsq_ref, dsh_ref, dh_ref, dA = ar.hrea_backward(P_ref, h, datt)
    rep = ar.Report('hrea (%d, %d, %d):' % (B, R, H))
    P, att = ar.Guarded((N, R)), ar.Guarded((N, H))
    h_d = dev(h)
    ops.hrea_attention_forward(dev(sq), dev(sh), h_d, P.t, att.t, B, R, H)
    rep.close('P', P, P_ref.reshape(N, R), BOUND, [ar.row_block('dialog B - 1', B - 1, R)])
    rep.close('att', att, att_ref.reshape(N, H), BOUND, ar.tile_slices(N, H)[1:] + [ar.row_block('dialog B - 1', B - 1, R)])
    Pn = P.t.cpu().numpy().reshape(B, R, R)
    assert np.all(Pn[:, 0, 0] == 1.0)
    assert np.all(Pn[np.broadcast_to(np.triu(np.ones((R, R), bool), 1), (B, R, R))] == 0.0)           # the future gets exactly zero
    assert torch.isfinite(P.t).all() and torch.isfinite(att.t).all()
    if R > 1:
        assert Pn[0, R - 1, 1] == 0.0 and P_ref[0, R - 1, 1] == 0.0
    dsq, dsh, dh = ar.Guarded((N,)), ar.Guarded((N,)), ar.Guarded((N, H))
    ops.hrea_attention_backward(h_d, P.t, dev(datt), dsq.t, dsh.t, dh.t, B, R, H)
    assert torch.isfinite(dsq.t).all() and torch.isfinite(dsh.t).all() and torch.isfinite(dh.t).all()
    rep.within('dsq', dsq.t, dsq_ref, BOUND * np.abs(dA).sum(2).reshape(-1))                          # a sum that cancels (see the header)
    assert not (dsq.t == ar.SENTINEL).any() and not (dsh.t == ar.SENTINEL).any()                      # written, every element
    rep.close('dsh', dsh, dsh_ref.reshape(N), BOUND)
    rep.close('dh', dh, dh_ref.reshape(N, H), BOUND, ar.tile_slices(N, H)[1:] + [ar.row_block('dialog B - 1', B - 1, R)])
    assert R == 1 or dA[0, R - 1, 1] == 0.0      # the reference the three were held to passes nothing through the replaced score
    for name, out in (('P', P), ('att', att), ('dsq', dsq), ('dsh', dsh), ('dh', dh)):
        rep.guard(name, out)
    rep.ok()


@pytest.mark.parametrize("N,H", [(1, 4), (5, 36), (203, 772), (40, 512)])
def test_rowdot(ops, N, H):
    """H = 772: four blocks of the backward grid, the last one ragged"""
    rng = np.random.RandomState(N + H)
    x, w, b = f32(rng, N, H), f32(rng, H) * np.float32(0.3), f32(rng, 1)
    dout = f32(rng, N) + np.float32(1.5)            # a non-zero mean: db = db0 + sum(dout) is well conditioned, and held like every output
    rep = ar.Report('rowdot (%d, %d):' % (N, H))
    out = ar.Guarded((N,))
    x_d, w_d = dev(x), dev(w)
    ops.rowdot_forward(x_d, w_d, dev(b), out.t, N, H)
    rep.close('out', out, ar.rowdot_forward(x, w, b), BOUND)
    dw_ref, db_ref, dx_ref = ar.rowdot_backward(x, w, dout)
    dw0, db0 = acc_init(rng, dw_ref), np.float32([0.75])
    dw, db, dx = ar.Guarded((H,), init=dw0), ar.Guarded((1,), init=db0), ar.Guarded((N, H))
    ops.rowdot_backward(x_d, w_d, dev(dout), dw.t, db.t, dx.t, N, H)
    rep.close('dw', dw, dw0.astype(D) + dw_ref, BOUND, [('last block of 256', (slice((H - 1) // 256 * 256, H),))])
    assert 0.75 + np.abs(dout.astype(D)).sum() <= 2 * abs(0.75 + db_ref)                              # (no cancellation in these data)
    rep.scalar('db', db.t.item(), 0.75 + db_ref, BOUND * abs(0.75 + db_ref))
    rep.close('dx', dx, dx_ref, BOUND, ar.tile_slices(N, H) + [('last block of 256', (slice(None), slice((H - 1) // 256 * 256, H)))])
    for name, o in (('out', out), ('dw', dw), ('db', db), ('dx', dx)):
        rep.guard(name, o)
    rep.ok()


def random_mask(rng, B, R):
    """1 = hidden; every row keeps at least one visible fact"""
    mask = (rng.rand(B, R, R) < 0.4).astype(np.uint8)
    mask[np.arange(B)[:, None], np.arange(R)[None, :], rng.randint(0, R, size=(B, R))] = 0
    return mask


def mn_inputs(B, R, H):
    rng = np.random.RandomState(B * 100 + R * 10 + H)
    return f32(rng, B, R, H) * np.float32(0.2), f32(rng, B, R, H) * np.float32(0.2), f32(rng, B, R, H)


def mn_mask(B, R, H, mask_kind):
    return vo.causal_mask(B, R) if mask_kind == 'causal' else random_mask(np.random.RandomState(R + H), B, R)


def run_mn(ops, B, R, H, mask, what, backward=True):
    N = B * R
    q, h, dhatt = mn_inputs(B, R, H)
    p_ref, hatt_ref = vo.mn_attention_forward(q.astype(D), h.astype(D), mask)
    rep = ar.Report('mn (%d, %d, %d) %s:' % (B, R, H, what))
    last = [ar.row_block('dialog B - 1', B - 1, R)]
    P, hatt = ar.Guarded((N, R)), ar.Guarded((N, H))
    q_d, h_d = dev(q), dev(h)
    ops.mn_attention_forward(q_d, h_d, dev(mask), P.t, hatt.t, B, R, H)
    rep.close('P', P, p_ref.reshape(N, R), BOUND, last)
    rep.close('hAtt', hatt, hatt_ref.reshape(N, H), BOUND, ar.tile_slices(N, H)[1:] + last)
    assert np.all(P.t.cpu().numpy().reshape(B, R, R)[mask != 0] == 0.0)                               # hidden facts get exactly zero
    outs = [('P', P), ('hAtt', hatt)]
    if backward:
        dq_ref, dh_ref = vo.mn_attention_backward(q.astype(D), h.astype(D), p_ref, dhatt.astype(D))
        dQ, dH = ar.Guarded((N, H)), ar.Guarded((N, H))
        ops.mn_attention_backward(q_d, h_d, P.t, dev(dhatt), dQ.t, dH.t, B, R, H)
        rep.close('dQ', dQ, dq_ref.reshape(N, H), BOUND, ar.tile_slices(N, H)[1:] + last)
        rep.close('dHm', dH, dh_ref.reshape(N, H), BOUND, ar.tile_slices(N, H)[1:] + last)
        outs += [('dQ', dQ), ('dHm', dH)]
    for name, out in outs:
        rep.guard(name, out)
    rep.ok()


@pytest.mark.parametrize("mask_kind", ['causal', 'random'])
@pytest.mark.parametrize("B,R,H", MN_CASES)
def test_mn_attention(ops, B, R, H, mask_kind):
    run_mn(ops, B, R, H, mn_mask(B, R, H, mask_kind), mask_kind)


def test_mn_attention_lds_guards(ops):
    """The workgroup's LDS is the dynamic staging (2 R H floats forward, 3 R H backward) PLUS the kernels' static score tiles (1 KB
    forward, 2 KB backward); both guards count both against 64 KB.  R = 16: the largest accepted H runs and matches fp64, the next
    H % 4 == 0 is refused by name before anything is launched.  (The headline's (10, 512) is a case of test_mn_attention.)"""
    from visdial_amd import _lib
    R, B = 16, 2
    tile = R * R * 4
    assert 3 * R * 328 * 4 + 2 * tile <= 65536 < 3 * R * 332 * 4 + 2 * tile
    assert 2 * R * 504 * 4 + tile <= 65536 < 2 * R * 508 * 4 + tile
    rng = np.random.RandomState(16)
    run_mn(ops, B, R, 328, vo.causal_mask(B, R), 'largest backward shape')
    run_mn(ops, B, R, 504, random_mask(rng, B, R), 'largest forward shape', backward=False)

    def call(fwd, R, H):
        n = B * R * H
        t = [torch.zeros(n, device='cuda') for _ in range(6)]
        if fwd:
            ops.mn_attention_forward(t[0], t[1], torch.zeros(B * R * R, dtype=torch.uint8, device='cuda'), torch.zeros(B * R * R, device='cuda'),
                                     t[2], B, R, H)
        else:
            ops.mn_attention_backward(t[0], t[1], torch.zeros(B * R * R, device='cuda'), t[2], t[3], t[4], B, R, H)
    # These two shapes passed the guards as they were (staging alone <= 64 KB).  They are refused before anything is launched; should a
    # guard ever regress, the call would launch a workgroup of more than 64 KB of LDS, on buffers of the full size.
    with pytest.raises(_lib.VisdialHipError, match='LDS staging'):
        call(True, 16, 508)
    with pytest.raises(_lib.VisdialHipError, match='LDS staging'):
        call(False, 16, 332)
    for fwd in (True, False):
        with pytest.raises(_lib.VisdialHipError):
            call(fwd, 17, 36)
        with pytest.raises(_lib.VisdialHipError):
            call(fwd, 10, 6)
    torch.cuda.synchronize()
