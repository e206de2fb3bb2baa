"""The two kernels of a live dense step (csrc/loss.hip DL3) as operators, entered through the internal vd_dense_live_tokens_p and
vd_score_ce_dense_live_p, bound by visdial_amd._lib.internal (declarations in csrc/rt_core.h):

  dense_live_tokens_kernel     bit for bit against dense.live_option_tokens: To in {1, 5}, O in {5, 64, 65, 128} (a partial wave, the wave
                               boundary on either side, MAX_OPT), N = 6 rounds, the live sets {0}, {5}, {0, 2, 3, 5}, {1, 4}, with and
                               without the row index of a de-duplicated upload; guard ints on both sides of the output come back untouched.
  score_ce_dense_live_kernel   against an fp64 restatement built from dense.dense_ce: H in {32, 64, 512} (one float4 per lane of a part of a
                               wave, of a quarter of the block, two passes of the k loop), the same O and live sets.  optH holds exactly
                               n_live * O rows with NaN guard rows behind it (a round that is not live must read none of it), every output
                               is prefilled with NaN: the rows of scores, loss_rows and dEnc of the other rounds must come back exactly 0,
                               dOptH's guard rows untouched.  Bounds, those of tests/test_dense_gpu.py check 1 and conftest.grad_mismatches:
                               1e-4 absolute on the loss rows, rel-L2 1e-4 per tensor on scores, dOptH and dEnc.
                               With every round live and the same operands it reproduces vd_score_ce_dense_p bit for bit."""
import types

import numpy as np
import pytest
import torch

from visdial_amd import dense

pytestmark = pytest.mark.gpu

N = 6
LIVE_SETS = ([0], [5], [0, 2, 3, 5], [1, 4])
OS = (5, 64, 65, 128)
GUARD = 128
MIX = 0.5
WORST = {}


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from visdial_amd import _lib
    return types.SimpleNamespace(
        tokens=_lib.internal('vd_dense_live_tokens_p'), head=_lib.internal('vd_score_ce_dense_live_p'),
        dense=_lib.internal('vd_score_ce_dense_p'), Error=_lib.VisdialHipError)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------------------ the compaction
@pytest.mark.parametrize("with_uid", [False, True], ids=['own-rows', 'uid'])
@pytest.mark.parametrize("O", OS)
@pytest.mark.parametrize("To", [1, 5])
def test_live_tokens_are_the_numpy_compaction_bit_for_bit(lib, To, O, with_uid):
    rng = np.random.RandomState(100 * To + O + with_uid)
    if with_uid:
        rows = max(2, (N * O) // 2 + 1)                                             # distinct rows of a de-duplicated upload
        uid = rng.randint(0, rows, size=N * O).astype(np.int32)
    else:
        rows, uid = N * O, None
    tok = rng.randint(0, 1000, size=(To, rows)).astype(np.int32)
    d_tok, d_uid = dev(tok), None if uid is None else dev(uid)
    for live in LIVE_SETS:
        want = dense.live_option_tokens(tok, uid, live, O)
        n = want.size
        out = torch.full((GUARD + n + GUARD,), -7, dtype=torch.int32, device='cuda')
        d_live = dev(np.asarray(live, np.int32))
        lib.tokens(d_tok.data_ptr(), rows, To, None if d_uid is None else d_uid.data_ptr(), d_live.data_ptr(), len(live), O,
                   out.data_ptr() + 4 * GUARD, stream())
        got = host(out)
        assert np.array_equal(got[GUARD:GUARD + n].reshape(To, len(live) * O), want), live
        assert (got[:GUARD] == -7).all() and (got[GUARD + n:] == -7).all(), live
    # no live round: nothing is launched, nothing is written
    out = torch.full((GUARD,), -7, dtype=torch.int32, device='cuda')
    lib.tokens(d_tok.data_ptr(), rows, To, None, d_live.data_ptr(), 0, O, out.data_ptr(), stream())
    assert (host(out) == -7).all()
    with pytest.raises(lib.Error, match='vd_dense_live_tokens_p: bad args'):
        lib.tokens(None, rows, To, None, d_live.data_ptr(), 1, O, out.data_ptr(), stream())


# ------------------------------------------------------------------------------------------------------------ the live head
def relevance(live, O, rng):
    """rounds of `live` carry a weight under MIX: annotated with relevant candidates and not annotated in turn; the others are k = 0"""
    rel = np.zeros((N, O), np.float32)
    for j, n in enumerate(live):
        if j % 2 == 1:
            rel[n] = -1.0
        else:
            k = max(1, O // 3)
            rel[n, rng.choice(O, size=k, replace=False)] = rng.randint(1, 6, size=k) / 5.0
    return rel


def reference(optH, enc, gt, rel, live, O):
    """fp64: scores, loss_rows, dOptH (compact) and dEnc of the live rounds from dense.dense_ce"""
    optH, enc = optH.astype(np.float64), enc.astype(np.float64)
    H = enc.shape[1]
    scores, loss_rows, dEnc = np.zeros((N, O)), np.zeros(N), np.zeros((N, H))
    for slot, n in enumerate(live):
        scores[n] = optH[slot * O:(slot + 1) * O] @ enc[n]
    _, w = dense.dense_targets(rel, gt, MIX)
    assert np.nonzero(w > 0)[0].tolist() == list(live)
    _, ds = dense.dense_ce(scores[live], rel[live], gt[live], MIX)                  # W over the live rounds is W over the batch
    dOptH = np.zeros((len(live) * O, H))
    for slot, n in enumerate(live):
        row, _ = dense.dense_ce(scores[n:n + 1], rel[n:n + 1], gt[n:n + 1], MIX)    # one round alone: its own loss
        loss_rows[n] = w[n] * row
        dOptH[slot * O:(slot + 1) * O] = ds[slot][:, None] * enc[n][None, :]
        dEnc[n] = ds[slot] @ optH[slot * O:(slot + 1) * O]
    return scores, loss_rows, dOptH, dEnc, float(w.sum())


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("O", OS)
@pytest.mark.parametrize("H", [32, 64, 512])
def test_live_head_against_fp64_and_zero_rows_for_the_other_rounds(lib, H, O):
    rng = np.random.RandomState(H + O)
    enc = (rng.randn(N, H) / np.sqrt(H)).astype(np.float32) * 3.0
    gt = rng.randint(0, O, size=N).astype(np.int32)
    d_enc, d_gt = dev(enc), dev(gt)
    for live in LIVE_SETS:
        nl = len(live)
        rel = relevance(live, O, rng)
        optH = rng.randn(nl * O, H).astype(np.float32)
        slot = np.full(N, -1, np.int32)
        slot[live] = np.arange(nl)
        want_s, want_l, want_do, want_de, W = reference(optH, enc, gt, rel, live, O)
        d_optH = dev(np.concatenate([optH, np.full((GUARD, H), np.nan, np.float32)]))
        d_rel, d_slot = dev(rel), dev(slot)
        nan = lambda *shape: torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')
        scores, loss_rows, dOptH, dEnc = nan(N, O), nan(N), nan(nl * O + GUARD, H), nan(N, H)
        lib.head(d_optH.data_ptr(), d_enc.data_ptr(), d_gt.data_ptr(), d_rel.data_ptr(), d_slot.data_ptr(), scores.data_ptr(),
                 loss_rows.data_ptr(), dOptH.data_ptr(), dEnc.data_ptr(), N, O, H, 1.0 / W, MIX, stream())
        s, l, do, de = host(scores), host(loss_rows), host(dOptH), host(dEnc)
        other = np.setdiff1d(np.arange(N), live)
        for name, a in (('scores', s), ('loss_rows', l), ('dEnc', de)):             # exactly 0 (either sign bit would do; +0 is what is written)
            assert (a[other] == 0).all() and not np.isnan(a).any(), (name, live)
        assert np.isnan(do[nl * O:]).all() and not np.isnan(do[:nl * O]).any(), live   # the guard rows behind the compact gradient
        figs = (np.abs(l - want_l).max(), rel_l2(s[live], want_s[live]), rel_l2(do[:nl * O], want_do), rel_l2(de[live], want_de[live]))
        print('H = %d, O = %d, live %s: |loss_rows| %.3g, rel-L2 scores %.3g, dOptH %.3g, dEnc %.3g' % ((H, O, live) + figs))
        for k, v in zip(('loss rows', 'scores', 'dOptH', 'dEnc'), figs):
            WORST[k] = max(WORST.get(k, 0.0), float(v))
        assert figs[0] < 1e-4 and max(figs[1:]) < 1e-4, (live, figs)
        # forward only of the same head: scores and loss rows, no gradient buffer touched
        scores2, loss2 = nan(N, O), nan(N)
        lib.head(d_optH.data_ptr(), d_enc.data_ptr(), d_gt.data_ptr(), d_rel.data_ptr(), d_slot.data_ptr(), scores2.data_ptr(),
                 loss2.data_ptr(), None, None, N, O, H, 1.0 / W, MIX, stream())
        assert host(scores2).tobytes() == s.tobytes() and host(loss2).tobytes() == l.tobytes()


@pytest.mark.parametrize("O", OS)
@pytest.mark.parametrize("H", [32, 64, 512])
def test_every_round_live_is_the_dense_head_bit_for_bit(lib, H, O):
    rng = np.random.RandomState(7 * H + O)
    enc = (rng.randn(N, H) / np.sqrt(H)).astype(np.float32) * 3.0
    gt = rng.randint(0, O, size=N).astype(np.int32)
    optH = rng.randn(N * O, H).astype(np.float32)
    rel = relevance([0, 1, 2, 3, 5], O, rng)                                        # round 4: k = 0, the body's own weight-0 branch
    out = []
    operands = [dev(optH), dev(enc), dev(gt), dev(rel)]
    for live_form in (False, True):
        nan = lambda *shape: torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')
        scores, loss_rows, dOptH, dEnc = nan(N, O), nan(N), nan(N * O, H), nan(N, H)
        args = [t.data_ptr() for t in operands]
        keep = dev(np.arange(N, dtype=np.int32))
        if live_form:
            args.append(keep.data_ptr())
        (lib.head if live_form else lib.dense)(*(args + [scores.data_ptr(), loss_rows.data_ptr(), dOptH.data_ptr(), dEnc.data_ptr(), N, O, H,
                                                         1.0 / 4.5, MIX, stream()]))
        out.append([host(t) for t in (scores, loss_rows, dOptH, dEnc)])
    for name, a, b in zip(('scores', 'loss_rows', 'dOptH', 'dEnc'), *out):
        assert not np.isnan(a).any() and a.tobytes() == b.tobytes(), name
    assert (out[1][2][4 * O:5 * O] == 0).all() and out[1][1][4] == 0                # the k = 0 round: zero gradient, loss 0, scores written
    assert np.abs(out[1][0][4]).max() > 0


def test_refusals_and_the_worst_figures(lib):
    z = torch.zeros(64, dtype=torch.float32, device='cuda')
    p = z.data_ptr()
    with pytest.raises(lib.Error, match='vd_score_ce_dense_live_p: bad args'):
        lib.head(p, p, p, p, None, p, p, None, None, 1, 4, 4, 1.0, 0.0, stream())
    with pytest.raises(lib.Error, match='vd_score_ce_dense_live_p: dOptH and dEnc go together'):
        lib.head(p, p, p, p, p, p, p, p, None, 1, 4, 4, 1.0, 0.0, stream())
    with pytest.raises(lib.Error, match='vd_score_ce_dense_live_p: the mix 2 is not in'):
        lib.head(p, p, p, p, p, p, p, None, None, 1, 4, 4, 1.0, 2.0, stream())
    for k in sorted(WORST):
        print('WORST live head, %s: %.3g' % (k, WORST[k]))
