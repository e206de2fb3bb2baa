"""The batched beam-search kernels (csrc/beam.hip: vd_beam_topk / init / advance / select_rows / finish) against a numpy
restatement of the per-dialog bookkeeping of SplitEval.generateAnswers (split_eval.py; model.lua:466-573), bit for bit: top-k
indices and values, the per-slot source, the history buffer, the fp64 scores and the best finished candidate after every step."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def dev(a, dtype):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device='cuda')


# ---------------------------------------------------------------------------------------------------------------- top-k
def topk_case(rng, rows, V, k, ties):
    """logits [rows x Vp] (pad columns hold garbage that must be ignored) and tokens with some 0 (all-zero rows)"""
    Vp = (V + 3) // 4 * 4
    x = np.full((rows, Vp), 1e4, np.float32)
    if ties:      # few distinct values: exact ties at many indices, across the k boundary
        x[:, :V] = rng.choice(np.array([0.25, -1.5, 0.75, 2.0], np.float32), size=(rows, V))
        x[0, :V] = 0.5                                         # a row of one value: the k lowest indices
        x[1, :V] = -2.0
        x[1, V - k - 2:] = 3.0                                 # the k + 2 highest values tie at the END of the row
    else:
        x[:, :V] = rng.standard_normal((rows, V)).astype(np.float32) * 3
    tok = rng.randint(1, 50, size=rows).astype(np.int32)
    tok[2::5] = 0
    return x, tok


@pytest.mark.parametrize("V", [7, 37, 130, 1001, 11322])
@pytest.mark.parametrize("k", [1, 5, 32])
@pytest.mark.parametrize("ties", [False, True])
def test_topk_is_the_stable_argsort_of_log_softmax_rows(gpu, V, k, ties):
    from visdial_amd import ops
    if k > V:
        pytest.skip("k > V is refused")
    rng = np.random.RandomState(V * 7 + k + ties)
    rows = 12
    x, tok = topk_case(rng, rows, V, k, ties)
    lg = dev(x, torch.float32)
    ti, tv = torch.full((rows, k), -7, dtype=torch.int32, device='cuda'), torch.full((rows, k), 9.0, device='cuda')
    ops.beam_topk(lg, V, dev(tok, torch.int32), k, ti, tv)
    ref = dev(x, torch.float32)
    ops.log_softmax_rows(ref, V)                               # the kernel the values must equal bit for bit
    lp = ref.cpu().numpy()[:, :V]
    assert np.array_equal(lg.cpu().numpy(), x)                 # logits are not written
    ti, tv = ti.cpu().numpy(), tv.cpu().numpy()
    for r in range(rows):
        if tok[r] == 0:
            exp_i, exp_v = np.arange(k), np.zeros(k, np.float32)
        else:
            exp_i = np.argsort(-lp[r], kind='stable')[:k]      # value descending, index ascending
            exp_v = lp[r, exp_i]
        assert np.array_equal(ti[r], exp_i), (r, ti[r], exp_i)
        assert np.array_equal(tv[r].view(np.int32), exp_v.astype(np.float32).view(np.int32)), r


def test_topk_refuses_k_above_its_bound(gpu):
    from visdial_amd import _lib, ops
    lg = torch.zeros(2, 40, device='cuda')
    ti, tv = torch.empty(2, 33, dtype=torch.int32, device='cuda'), torch.empty(2, 33, device='cuda')
    with pytest.raises(_lib.VisdialHipError, match='k = 33'):
        ops.beam_topk(lg, 40, torch.ones(2, dtype=torch.int32, device='cuda'), 33, ti, tv)


# ---------------------------------------------------------------------------------------------------------------- advance
def ref_advance(top_idx, top_val, k, step, L, END, scores, hist, best):
    """one step of the per-dialog beam search of SplitEval.generateAnswers for every group: returns (scores, hist, src, next_tok)
    and updates best in place.  best[g] = None or (score, length, column)."""
    G = scores.shape[0]
    explore = 1 if step == 1 else k
    scores, hist = scores.copy(), hist.copy()
    old_hist = hist.copy()
    old_scores = scores.copy()
    src = np.full((G, k), -1, np.int32)
    for g in range(G):
        cands, finish = [], []
        for w in range(explore):
            for q in range(k):
                t = int(top_idx[g * k + w, q]) + 1
                sc = old_scores[g, w] + float(top_val[g * k + w, q])
                cb = old_hist[g, w].copy()
                cb[step] = t
                (finish if t == END else cands).append((sc, cb, w))
        cands.sort(key=lambda a: -a[0])
        for i, (sc, cb, w) in enumerate(cands[:k]):
            hist[g, i], scores[g, i], src[g, i] = cb, sc, w
        finish.sort(key=lambda a: -a[0])
        if finish and (best[g] is None or finish[0][0] > best[g][0]):
            best[g] = (finish[0][0], step + 1, finish[0][1])
    return scores, hist, src, hist[:, :, step].copy()


def ref_finish(hist, scores, best):
    toks = np.stack([b[2] if b is not None else hist[g, 0] for g, b in enumerate(best)])
    return toks, np.array([b[0] if b is not None else scores[g, 0] for g, b in enumerate(best)])


def synthetic_topk(rng, G, k, V, END, step, plan):
    """top-k rows as the kernel would produce them (distinct indices, values descending), shaped by `plan[g]`:
    'end1' -> <END> among slot 0's candidates at step 1 (n_keep < k); 'allend' -> k = 1 and <END> first (n_keep = 0 at step 1);
    'ties' -> values from a coarse set (equal fp64 scores across slots); 'never' -> <END> never proposed"""
    idx = np.zeros((G * k, k), np.int32)
    val = np.zeros((G * k, k), np.float32)
    for g in range(G):
        for w in range(k):
            r = g * k + w
            pool = np.array([c for c in range(V) if not (plan[g] == 'never' and c == END - 1)])
            idx[r] = rng.choice(pool, size=k, replace=False)
            if plan[g] == 'ties':
                val[r] = -np.sort(rng.choice(np.array([0.5, 1.0, 1.5], np.float32), size=k))
            else:
                val[r] = -np.sort(rng.exponential(1.0, size=k)).astype(np.float32)
            if plan[g] == 'end1' and step == 1 and w == 0:
                idx[r, min(1, k - 1)] = END - 1
                idx[r, 0] = (END if END < V else END - 2)        # distinct from END - 1
            if plan[g] == 'allend' and step == 1 and w == 0:
                idx[r, 0] = END - 1
            if plan[g] == 'endlate' and step >= 2 and rng.rand() < 0.3:
                q = rng.randint(k)
                if END - 1 not in idx[r]:
                    idx[r, q] = END - 1
    return idx, val


@pytest.mark.parametrize("k,plan", [(5, ['end1', 'ties', 'never', 'endlate', 'endlate']),
                                    (1, ['allend', 'never', 'endlate']),
                                    (3, ['end1', 'ties', 'ties', 'endlate']),
                                    (32, ['endlate', 'ties'])])
def test_advance_init_select_finish_match_the_host_bookkeeping(gpu, k, plan):
    from visdial_amd import ops
    rng = np.random.RandomState(k)
    G, L, V, START, END = len(plan), 7, 60, 3, 5
    i32, f64 = dict(dtype=torch.int32, device='cuda'), dict(dtype=torch.float64, device='cuda')
    n = G * k
    hist = [torch.full((n, L), -9, **i32), torch.full((n, L), -9, **i32)]
    tok, src = torch.full((n,), -9, **i32), torch.full((n,), -9, **i32)
    scores, best_score = torch.full((n,), 7.0, **f64), torch.full((G,), 7.0, **f64)
    best_len, best_hist = torch.full((G,), 9, **i32), torch.zeros(G, L, **i32)
    ops.beam_init(G, k, L, START, hist[0], tok, scores, best_score, best_len)
    r_hist = np.zeros((G, k, L), np.int64)
    r_hist[:, :, 0] = START
    r_scores = np.zeros((G, k))
    best = [None] * G
    assert np.array_equal(hist[0].cpu().numpy().reshape(G, k, L), r_hist)
    assert (tok.cpu().numpy() == START).all() and (scores.cpu().numpy() == 0).all() and (best_len.cpu().numpy() == 0).all()
    H = 6
    state = torch.randn(n, H, device='cuda')
    cur = 0
    for step in range(1, L):
        idx, val = synthetic_topk(rng, G, k, V, END, step, plan)
        ops.beam_advance(dev(idx, torch.int32), dev(val, torch.float32), G, k, step, L, END, scores, hist[cur], hist[cur ^ 1], src,
                         tok, best_score, best_len, best_hist)
        r_scores, r_hist, r_src, r_tok = ref_advance(idx, val, k, step, L, END, r_scores, r_hist, best)
        cur ^= 1
        assert np.array_equal(src.cpu().numpy().reshape(G, k), r_src), step
        assert np.array_equal(hist[cur].cpu().numpy().reshape(G, k, L), r_hist), step
        assert np.array_equal(tok.cpu().numpy().reshape(G, k), r_tok), step
        assert np.array_equal(scores.cpu().numpy().reshape(G, k), r_scores), step        # fp64, bit for bit
        bl = best_len.cpu().numpy()
        for g in range(G):
            if best[g] is None:
                assert bl[g] == 0
            else:
                assert bl[g] == best[g][1] and best_score[g].item() == best[g][0]
                assert np.array_equal(best_hist[g].cpu().numpy(), best[g][2])
        # the state select: a kept slot copies the stepped row of its source, the others keep their own
        stepped = torch.randn(n, H, device='cuda')
        before = state.clone()
        ops.beam_select_rows(state, stepped, src, k)
        s_, b_, st_, sr = state.cpu().numpy(), before.cpu().numpy(), stepped.cpu().numpy(), src.cpu().numpy()
        for r in range(n):
            exp = st_[(r // k) * k + sr[r]] if sr[r] >= 0 else b_[r]
            assert np.array_equal(s_[r], exp), (step, r)
    if plan[0] in ('end1', 'allend'):
        assert best[0] is not None                                     # <END> was proposed at step 1
    if 'never' in plan:
        assert best[plan.index('never')] is None                       # falls back to column 0
    out_tok, out_sc = torch.empty(G, L, **i32), torch.empty(G, **f64)
    ops.beam_finish(G, k, L, hist[cur], scores, best_score, best_len, best_hist, out_tok, out_sc)
    e_tok, e_sc = ref_finish(r_hist, r_scores, best)
    assert np.array_equal(out_tok.cpu().numpy(), e_tok) and np.array_equal(out_sc.cpu().numpy(), e_sc)


def test_advance_with_nothing_to_keep_at_step_one(gpu):
    """k = 1 and slot 0's only candidate is <END>: n_keep = 0, the slot keeps <START> + 0 and its pre-step state (src -1)"""
    from visdial_amd import ops
    i32, f64 = dict(dtype=torch.int32, device='cuda'), dict(dtype=torch.float64, device='cuda')
    L, END = 4, 2
    hist = [torch.empty(1, L, **i32), torch.empty(1, L, **i32)]
    tok, src, scores = torch.empty(1, **i32), torch.empty(1, **i32), torch.empty(1, **f64)
    bs, bl, bh = torch.empty(1, **f64), torch.empty(1, **i32), torch.empty(1, L, **i32)
    ops.beam_init(1, 1, L, 1, hist[0], tok, scores, bs, bl)
    ops.beam_advance(dev([[END - 1]], torch.int32), dev([[-0.25]], torch.float32), 1, 1, 1, L, END, scores, hist[0], hist[1], src, tok,
                     bs, bl, bh)
    assert src.item() == -1 and tok.item() == 0 and scores.item() == 0.0
    assert hist[1].cpu().numpy().tolist() == [[1, 0, 0, 0]]
    assert bl.item() == 2 and bs.item() == -0.25 and bh.cpu().numpy().tolist() == [[1, END, 0, 0]]
