"""Generative retrieval over a prefix tree of the candidates' tokens, on the GPU: VD_FLAG_TREE of vd_lstm_forward (a level-by-level
recurrence over a forest: every row continues the state of a PARENT row of the step before).

Operator level.
* Identity parents: h and c equal VD_FLAG_LIVE_PREFIX's bit for bit on the live prefix (same step kernels, same tiles, same K order),
  rows at or beyond ceil(n_t / VD_LIVE_PREFIX_ROWS) * VD_LIVE_PREFIX_ROWS keep a sentinel.  Both kernel families, dense and table mode,
  with and without h0.
* Real forests against oracle.visdial_oracle.lstm_forward in fp64 run over every node's root-to-node path: relerr(h), relerr(c) below
  1e-5, the bound tests/test_ops_gpu.py holds vd_lstm_forward to.  Each forest has a parent with many children, a childless node, a
  level wider than the one before and a ragged last tile; two nodes with the same parent and token get identical bits wherever their
  row tiles run the K loop in the same order (the K-tile rotation of the ungathered kernels is kept, which the identity case pins: a
  row's bits depend on its row tile's rotation, as they do under VD_FLAG_LIVE_PREFIX).  The fp64 reference of a forest is computed
  once and shared by the dense and the table case.
* Every refused combination is an argument error that names the flag."""
import numpy as np
import pytest
import torch

from oracle import visdial_oracle as vo
from test_lhood_gpu import dev
from test_lhood_prefix_gpu import in_private_pool, private_pool, run_lstm  # noqa: F401 (the pool fixtures act by being here)
from test_ops_gpu import relerr

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


# ------------------------------------------------------------------------------------------------------------------ the operator
IDENTITY_CASES = [
    # name, H, N, nodes per step
    ('small kernels, ragged tiles', 64, 203, [203, 97, 96, 31, 1]),
    ('LDS-DMA kernels, 4200 rows to under a tile', 512, 4200, [4200, 3000, 1500, 700, 300, 129, 60, 17]),
]


@pytest.mark.parametrize("mode", ['dense', 'table'])
@pytest.mark.parametrize("with_h0", [True, False])
@pytest.mark.parametrize("name,H,N,widths", IDENTITY_CASES)
def test_tree_with_identity_parents_equals_live_prefix(gpu, name, H, N, widths, with_h0, mode):
    from visdial_amd import ops
    G = ops.LIVE_PREFIX_ROWS
    rs = np.random.RandomState(11)
    T, V = len(widths), 50
    tok = np.zeros((2, T, N), np.int32)
    for t, n in enumerate(widths):
        tok[0, t, :n] = rs.randint(1, V + 1, size=n)
    tok[1] = np.arange(N)[None, :]                                # every row continues itself
    tok[1][tok[0] == 0] = 2 ** 30                                 # parent entries of rows without a node are never used as rows
    Wh = dev(rs.standard_normal((H, 4 * H)) / np.sqrt(H), torch.float32)
    h0 = dev(rs.standard_normal((N, H)) * 0.5, torch.float32) if with_h0 else None
    c0 = dev(rs.standard_normal((N, H)) * 0.5, torch.float32) if with_h0 else None
    table = xproj = None
    if mode == 'table':
        table = dev(rs.standard_normal((V + 1, 4 * H)), torch.float32)
    else:
        xproj = torch.randn((T, N, 4 * H), device='cuda', generator=torch.Generator(device='cuda').manual_seed(5))
    tk = dev(tok, torch.int32)
    live = run_lstm(tk[0].contiguous(), xproj, table, Wh, h0, c0, T, N, H, ops.FLAG_LIVE_PREFIX)[1:]
    tree = run_lstm(tk, xproj, table, Wh, h0, c0, T, N, H, ops.FLAG_TREE, gates=False)[1:]
    for what, a, b in zip(('h', 'c'), live, tree):
        for t, n in enumerate(widths):
            assert not (a[t, :n] == SENTINEL).any(), (what, t)
            assert np.array_equal(a[t, :n].view(np.uint32), b[t, :n].view(np.uint32)), (what, t)
            end = min(N, -(-n // G) * G)
            assert (b[t, end:] == SENTINEL).all(), (what, t, 'a skipped row group was written')
            mid = b[t, n:end]
            assert ((mid == 0) | (mid == SENTINEL)).all(), (what, t)


def make_forest(seed, R, widths, V):
    """tokens and parents [T x N] of a forest with the given level widths over R roots: node 0 .. 9 of every level hang off parent 0 (a
    parent with many children), the last node of a level has no child, nodes 1 and 2 share parent AND token"""
    rs = np.random.RandomState(seed)
    T, N = len(widths), max(widths)
    tok = np.zeros((T, N), np.int32)
    par = np.full((T, N), 2 ** 30, np.int32)
    for t, n in enumerate(widths):
        prev = R if t == 0 else widths[t - 1]
        tok[t, :n] = rs.randint(1, V + 1, size=n)
        par[t, :n] = rs.randint(0, max(1, prev - 1), size=n)       # never the last node of the level before
        if t and n > 12:
            par[t, :10] = 0
            tok[t, 2] = tok[t, 1]
            par[t, 2] = par[t, 1]
    return tok, par


def forest_reference(tok, par, widths, emb, Wx, b, Wh, h0, c0):
    """h and c of every node in fp64: the oracle's lstm_forward over the node's root-to-node path, one call per level"""
    W = np.concatenate([Wx, Wh], 0).astype(np.float64)
    ref_h, ref_c = [], []
    for d, n in enumerate(widths):
        idx = np.arange(n)
        x = np.zeros((d + 1, n, emb.shape[1]))
        for t in range(d, -1, -1):
            x[t] = emb[tok[t, idx]]
            idx = par[t, idx]
        h_all, c_all, _ = vo.lstm_forward(x, W, b.astype(np.float64), None, h0[idx].astype(np.float64), c0[idx].astype(np.float64))
        ref_h.append(h_all[-1])
        ref_c.append(c_all[-1])
    return ref_h, ref_c


FORESTS = {
    'small kernels': (64, 3, [3, 40, 203, 97, 31]),
    'LDS-DMA kernels': (512, 200, [200, 2300, 4200, 1500, 129]),
}
_forest_cache = {}


def forest_case(name):
    if name not in _forest_cache:
        H, R, widths = FORESTS[name]
        V, D = 50, 8
        rs = np.random.RandomState(17)
        tok, par = make_forest(23, R, widths, V)
        emb = rs.standard_normal((V + 1, D)).astype(np.float32)
        Wx = (rs.standard_normal((D, 4 * H)) / np.sqrt(D)).astype(np.float32)
        b = (rs.standard_normal(4 * H) * 0.1).astype(np.float32)
        Wh = (rs.standard_normal((H, 4 * H)) / np.sqrt(H)).astype(np.float32)
        h0 = (rs.standard_normal((R, H)) * 0.5).astype(np.float32)
        c0 = (rs.standard_normal((R, H)) * 0.5).astype(np.float32)
        table = (emb.astype(np.float64) @ Wx + b).astype(np.float32)             # the device multiplies these fp32 rows
        ref = forest_reference(tok, par, widths, emb.astype(np.float64), Wx, b, Wh, h0, c0)
        _forest_cache[name] = dict(H=H, R=R, widths=widths, tok=tok, par=par, table=table, Wh=Wh, h0=h0, c0=c0, ref=ref)
    return _forest_cache[name]


@pytest.mark.parametrize("mode", ['dense', 'table'])
@pytest.mark.parametrize("name", list(FORESTS))
def test_tree_forest_matches_fp64_oracle_over_every_path(gpu, name, mode):
    from visdial_amd import ops
    case = forest_case(name)
    H, widths, tok, par = case['H'], case['widths'], case['tok'], case['par']
    T, N = tok.shape
    assert any(widths[t] > widths[t - 1] for t in range(1, T)) and widths[-1] % ops.lstm_fwd_row_tile(N) != 0
    for t in range(1, T):
        kids = np.bincount(par[t, :widths[t]], minlength=widths[t - 1])
        assert kids.max() >= 10 and kids.min() == 0               # a parent with many children, a childless node
    Wh, h0, c0 = (dev(case[k], torch.float32) for k in ('Wh', 'h0', 'c0'))
    table = dev(case['table'], torch.float32)
    mask = dev(np.stack([tok, par]), torch.int32)
    if mode == 'table':
        _, h, c = run_lstm(mask, None, table, Wh, h0, c0, T, N, H, ops.FLAG_TREE, gates=False)
    else:
        xproj = table[dev(tok, torch.int64)].contiguous()         # [T x N x 4H]
        _, h, c = run_lstm(mask, xproj, None, Wh, h0, c0, T, N, H, ops.FLAG_TREE, gates=False)
    for t, n in enumerate(widths):
        eh, ec = relerr(h[t, :n], case['ref'][0][t]), relerr(c[t, :n], case['ref'][1][t])
        print('%s %s level %d (%d nodes): relerr h %.2e c %.2e' % (name, mode, t, n, eh, ec))
        assert eh < 1e-5 and ec < 1e-5, (t, eh, ec)
        # the same parent and the same token: the same bits.  The step kernels keep the K order of the ungathered kernels (the identity
        # test above pins it), and that order is rotated per row tile: tile m starts its K loop at K tile (5 m + 3 n) mod (H / BK).  So
        # the bits are a function of (parent, token, 5 m mod (H / BK)) -- asserted for every such group of the level, the planted pair
        # (rows 1 and 2) among them
        tile = ops.lstm_fwd_row_tile(N)
        nk = H // (32 if tile == 32 else 16)                        # BK of the latency / the throughput step kernels
        rot = (np.arange(n) // tile * 5) % nk
        key = (par[t, :n].astype(np.int64) * 64 + tok[t, :n]) * nk + rot
        _, first, inv = np.unique(key, return_index=True, return_inverse=True)
        assert len(first) < n or n <= 12                          # (make_forest plants a pair on every level of more than 12 nodes)
        for a in (h, c):
            assert np.array_equal(a[t, :n].view(np.uint32), a[t, first[inv]].view(np.uint32)), t


def test_tree_is_refused_with_other_arithmetic_gates_state_only_and_without_a_mask(gpu):
    from visdial_amd import ops
    from visdial_amd._lib import VisdialHipError
    T, N, H = 2, 64, 32
    mask = torch.ones((2, T, N), dtype=torch.int32, device='cuda')
    mask[1] = 0
    x = torch.zeros((T, N, 4 * H), device='cuda')
    Wh = torch.zeros((H, 4 * H), device='cuda')
    g, h, c = torch.zeros((T, N, 4 * H), device='cuda'), torch.zeros((T, N, H), device='cuda'), torch.zeros((T, N, H), device='cuda')
    for other in (ops.FLAG_BF16, ops.FLAG_SPLIT9, ops.FLAG_SPLIT6, ops.FLAG_SPLIT3):
        with pytest.raises(VisdialHipError, match=r"VD_FLAG_TREE.*VD_FLAG_BF16 / VD_FLAG_SPLIT"):
            ops.lstm_forward(x, Wh, None, h, c, T, N, H, N * 4 * H, 4 * H, tok_mask=mask, flags=ops.FLAG_TREE | other)
    with pytest.raises(VisdialHipError, match=r"VD_FLAG_TREE.*VD_FLAG_STATE_ONLY"):
        ops.lstm_forward(x, Wh, None, h, c, T, N, H, N * 4 * H, 4 * H, tok_mask=mask, flags=ops.FLAG_TREE | ops.FLAG_STATE_ONLY)
    with pytest.raises(VisdialHipError, match=r"VD_FLAG_TREE.*gates must be NULL"):
        ops.lstm_forward(x, Wh, g, h, c, T, N, H, N * 4 * H, 4 * H, tok_mask=mask, flags=ops.FLAG_TREE)
    with pytest.raises(VisdialHipError, match=r"VD_FLAG_TREE needs tok_mask"):
        ops.lstm_forward(x, Wh, None, h, c, T, N, H, N * 4 * H, 4 * H, flags=ops.FLAG_TREE)
    with pytest.raises(ValueError, match=r"FLAG_TREE takes a two-plane tok_mask"):
        ops.lstm_forward(x, Wh, None, h, c, T, N, H, N * 4 * H, 4 * H, tok_mask=mask[0].contiguous(), flags=ops.FLAG_TREE)
    ops.lstm_forward(x, Wh, None, h, c, T, N, H, N * 4 * H, 4 * H, tok_mask=mask, flags=ops.FLAG_TREE)   # and the plain call is accepted
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ model level
# The tree path behind vd_model_retrieve_lhood (params fusedLhood = 2 -> VD_LHOOD_TREE at vd_model_create), through NativeModel and the
# Lua host.  The tree, the node list and the edges are built inside the library; what the tests see of them is the scores (which
# candidate walks which nodes) and vd_model_option_rows (the level widths, exactly, against the dictionary tree of
# tests/test_lhood_tree_cpu.py).
def set_candidate(batch, r, words, vocab):
    """candidate r (flat round x option index) = <START> words.. / words.. <END>"""
    T = batch['option_in'].shape[-1]
    fin, fout = batch['option_in'].reshape(-1, T), batch['option_out'].reshape(-1, T)
    assert len(words) <= T - 1
    fin[r], fout[r] = 0, 0
    fin[r, 0] = vocab - 1
    fin[r, 1:1 + len(words)] = words
    if len(words):
        fout[r, :len(words)] = words
        fout[r, len(words)] = vocab


def words_of(batch, r):
    T = batch['option_in'].shape[-1]
    row = batch['option_in'].reshape(-1, T)[r, 1:]
    return [int(w) for w in row[row != 0]]


def plant_shared_beginnings(batch, p, rng):
    """planted lengths, then per round: options 2..7 share their first two tokens, option 10 is a strict prefix of option 9; round 1's
    option 8 is a copy of its option 3; candidate 1 is empty (oracle_case), one candidate has the full length"""
    from test_lhood_prefix_gpu import plant_lengths
    B, R, O, T = batch['option_in'].shape
    N, V = B * R, p['vocabSize']
    lens = rng.randint(1, T - 1, size=N * O)
    lens[1] = 0
    plant_lengths(batch, lens, V, rng)
    batch['option_in'] = np.ascontiguousarray(batch['option_in'])
    batch['option_out'] = np.ascontiguousarray(batch['option_out'])
    for n in range(N):
        head = [int(w) for w in rng.randint(1, V - 1, size=2)]
        for o in range(2, 8):
            set_candidate(batch, n * O + o, head + [10 + o] + words_of(batch, n * O + o)[3:], V)      # a third token of its own: no accidental copies
        long = words_of(batch, n * O + 9)
        if len(long) < 2:
            long = long + [3, 4]
            set_candidate(batch, n * O + 9, long, V)
        set_candidate(batch, n * O + 10, long[:len(long) - 1], V)
    set_candidate(batch, 2 * O, [int(w) for w in rng.randint(1, V - 1, size=T - 1)], V)      # a full-length one
    dup = (O + 3, O + 8)
    set_candidate(batch, dup[1], words_of(batch, dup[0]), V)
    set_candidate(batch, 1, [], V)
    return dup


def tree_rows(batch):
    """(executed, total, nodes, live) of a batch that is one chunk, from the dictionary tree"""
    from test_lhood_tree_cpu import prefix_tree, rows_run
    from visdial_amd import ops
    B, R, O, T = batch['option_in'].shape
    widths, _ = prefix_tree(batch['option_in'].reshape(B * R, O, T), batch['option_out'].reshape(B * R, O, T))
    return rows_run(widths, ops.lstm_fwd_row_tile(max(widths))), T * B * R * O, sum(widths), int((batch['option_in'] != 0).sum())


@pytest.mark.parametrize("enc", ['lf-ques', 'lf-ques-im-hist', 'mn-att-ques-im-hist', 'hre-ques-im-hist', 'hrea-ques-im-hist'])
def test_tree_retrieval_matches_oracle_on_the_native_and_the_lua_host(gpu, enc):
    import ctypes as C
    import os
    from lua_host import LuaHost, first
    from luavm import to_py
    from test_lhood_gpu import bound, oracle_case
    from visdial_amd import _lib, t7
    from visdial_amd.native import NativeModel
    p, batch = oracle_case(enc)
    B, R, O, T = batch['option_in'].shape
    N = B * R
    dup = plant_shared_beginnings(batch, p, np.random.RandomState(3))
    gt = batch['answer_ind'].reshape(-1) - 1
    plain = NativeModel(dict(p, fusedLhood=1), init_seed=3)       # the same model without the switch: the length-ordered path
    plain.training(False)
    plain.retrieveBatch(batch, useGt=True)
    rows_ordered = plain.option_rows()
    plain.close()
    nat = NativeModel(dict(p, fusedLhood=2), init_seed=3)
    nat.training(False)
    Pf = nat.get_parameters_dict()
    ref = vo.retrieve(enc, 'gen', {k: v.astype(np.float64) for k, v in Pf.items()}, p, batch).reshape(-1)

    def check(who, scores, gt_ranks, all_ranks):
        err = float(np.abs(scores - ref).max())
        print('%-26s %-8s worst |score - oracle| %.3e (bound %.3e)' % (enc, who, err, bound(ref)))
        assert np.isfinite(scores).all() and err < bound(ref), (who, err)
        assert scores[1] == 0.0 and not np.signbit(scores[1]), who
        assert scores[dup[0]].view(np.uint32) == scores[dup[1]].view(np.uint32), who          # the same nodes: ties exactly ...
        all_ranks = np.asarray(all_ranks).reshape(N, O)
        assert all_ranks[1, 8] == all_ranks[1, 3] + 1, who                                    # ... and ranks by index
        np.testing.assert_array_equal(np.asarray(gt_ranks).reshape(-1), vo.compute_ranks(scores.reshape(N, O), gt), err_msg=who)
        np.testing.assert_array_equal(all_ranks, vo.compute_ranks(scores.reshape(N, O)), err_msg=who)

    g = nat.retrieveBatch(batch, useGt=True)
    executed, total = nat.option_rows()
    want_exec, want_total, nodes, live = tree_rows(batch)
    print('%s: %d nodes for %d live rows; executed %d of %d (length-ordered path: %d)' % (enc, nodes, live, executed, total, rows_ordered[0]))
    assert (executed, total) == (want_exec, want_total)
    assert rows_ordered[1] == total and executed < rows_ordered[0]
    s_nat = nat.scores(N, O)
    check('native', s_nat.reshape(-1), g, nat.retrieveBatch(batch, useGt=False))
    assert np.array_equal(s_nat.view(np.uint32), nat.scores(N, O).view(np.uint32))            # the same call twice
    before = os.environ.get('VD_LHOOD_TREE')
    os.environ['VD_LHOOD_TREE'] = '1'                             # the Lua host: the variable selects the mode when the model is created
    try:
        host = LuaHost(p)
        m = host.model()
    finally:
        if before is None:
            del os.environ['VD_LHOOD_TREE']
        else:
            os.environ['VD_LHOOD_TREE'] = before
    host.invoke(m, 'setFlatParameters', host.tensor(t7.named_to_flat(Pf, nat._entries(), enc), 'Float'))
    host.invoke(m, 'setMode', False)
    host.get(m, 'params').set('fusedLhood', 2)
    host.get(m, 'params').set('useGt', True)
    g = to_py(first(host.invoke(m, 'retrieveBatch', host.batch(batch))))
    s_lua = np.empty((N, O), np.float32)
    _lib.call('vd_model_scores', C.c_void_p(host.get(m, 'h').val), s_lua.ctypes.data, s_lua.size)
    ex_lua, tot_lua = C.c_int64(), C.c_int64()
    _lib.call('vd_model_option_rows', C.c_void_p(host.get(m, 'h').val), C.byref(ex_lua), C.byref(tot_lua))
    assert (ex_lua.value, tot_lua.value) == (want_exec, want_total)
    host.get(m, 'params').set('useGt', False)
    check('lua', s_lua.reshape(-1), g, to_py(first(host.invoke(m, 'retrieveBatch', host.batch(batch)))))
    assert np.array_equal(s_lua.view(np.uint32), s_nat.view(np.uint32))                       # one library, one path: the same bits
    nat.close()
    host.close()


def pooled_candidates(batch, p, rng, pool=300, mean_len=3.0):
    """every candidate drawn from a pool of `pool` answers (lengths 1 + Poisson(mean_len - 1), capped) with probability ~ 1 / (rank + 1):
    beginnings repeat inside a round, as answers such as "yes" / "yes it is" do"""
    B, R, O, T = batch['option_in'].shape
    V = p['vocabSize']
    answers = [[int(w) for w in rng.randint(1, V - 1, size=min(T - 1, 1 + rng.poisson(mean_len - 1)))] for _ in range(pool)]
    for k in range(1, pool, 3):                                   # every third answer continues the one before it
        answers[k] = (answers[k - 1] + answers[k])[:T - 1]
    w = 1.0 / (1.0 + np.arange(pool))
    pick = rng.choice(pool, size=B * R * O, p=w / w.sum())
    batch['option_in'] = np.zeros((B, R, O, T), np.int32)
    batch['option_out'] = np.zeros((B, R, O, T), np.int32)
    for r, k in enumerate(pick):
        set_candidate(batch, r, answers[k], V)


def tree_dense_ordered(p, batch, with_ordered=True):
    """the same batch through a model created with the switch (tree, then its dense head) and a fresh one without it (length-ordered
    head, dense head) -> dict of scores, ranks and counters"""
    from visdial_amd.native import NativeModel
    B, R, O, _ = batch['option_in'].shape
    out = {}
    nat = NativeModel(dict(p, fusedLhood=2), init_seed=1)
    nat.training(False)
    out['tree_ranks'] = np.asarray(nat.retrieveBatch(batch, useGt=False)).reshape(B * R, O)
    out['tree'], out['tree_rows'] = nat.scores(B * R, O).copy(), nat.option_rows()
    nat.retrieveBatch(batch, useGt=False)
    assert np.array_equal(out['tree'].view(np.uint32), nat.scores(B * R, O).view(np.uint32))     # the same call twice: bit-identical
    nat.params['fusedLhood'] = 0                                  # vd_model_retrieve of the same model: unaffected by the switch
    nat.retrieveBatch(batch, useGt=False)
    out['dense_of_tree_model'] = nat.scores(B * R, O).copy()
    nat.close()
    if with_ordered:
        fresh = NativeModel(dict(p, fusedLhood=1), init_seed=1)
        fresh.training(False)
        fresh.retrieveBatch(batch, useGt=False)
        out['ordered'], out['ordered_rows'] = fresh.scores(B * R, O).copy(), fresh.option_rows()
        fresh.params['fusedLhood'] = 0
        fresh.retrieveBatch(batch, useGt=False)
        out['dense'] = fresh.scores(B * R, O).copy()
        fresh.close()
    return out


def test_mid_size_pooled_candidates_tree_against_dense(gpu):
    """H 64, V 200, 20 x 10 x 100 candidates from a pool: one chunk whose widest level has more than 2 048 nodes (the LDS-DMA step kernel
    and the MFMA head)"""
    from test_lhood_gpu import bound, order_violations
    from test_lhood_prefix_gpu import mid_params
    from visdial_amd.dataloader import SyntheticDataloader
    p = mid_params()
    batch, _ = SyntheticDataloader(p, seed=7, num_threads=20).getTestBatch(1, p, 'val')
    pooled_candidates(batch, p, np.random.RandomState(21))
    want_exec, want_total, nodes, live = tree_rows(batch)
    r = tree_dense_ordered(p, batch)
    dense, tree = r['dense'], r['tree']
    assert np.array_equal(dense.view(np.uint32), r['dense_of_tree_model'].view(np.uint32))
    tol = bound(dense)
    diff = float(np.abs(dense.astype(np.float64) - tree).max())
    flipped, bad = order_violations(dense, tree, tol)
    print('mid size, pooled: %d nodes for %d live rows (%.3f); executed %d of %d (length-ordered: %d); worst |dense - tree| %.3e (allowed '
          '%.3e); option pairs in another order %d (unexplained %d)' % (nodes, live, nodes / live, r['tree_rows'][0], r['tree_rows'][1],
                                                                        r['ordered_rows'][0], diff, tol, flipped, len(bad)))
    assert np.isfinite(tree).all() and diff <= tol, (diff, tol)
    assert not bad, bad[:10]
    np.testing.assert_array_equal(r['tree_ranks'], vo.compute_ranks(tree))
    assert r['tree_rows'] == (want_exec, want_total)
    assert r['tree_rows'][0] < r['ordered_rows'][0]


def test_a_holed_candidate_takes_the_length_ordered_path_unchanged(gpu):
    from test_lhood_prefix_gpu import mid_params, plant_lengths
    from visdial_amd.dataloader import SyntheticDataloader
    p = mid_params(batchSize=3, maxQuesCount=5, numOptions=13, maxAnsLen=9)
    rng = np.random.RandomState(8)
    batch, _ = SyntheticDataloader(p, seed=7, num_threads=4).getTestBatch(1, p, 'val')
    B, R, O, T = batch['option_in'].shape
    lens = rng.randint(1, 10, size=B * R * O)
    plant_lengths(batch, lens, p['vocabSize'], rng)
    batch['option_in'].reshape(-1, T)[int(np.flatnonzero(lens >= 4)[0]), 2] = 0         # <START> w1 0 w3 ..: a token behind a pad
    r = tree_dense_ordered(p, batch)
    assert np.array_equal(r['tree'].view(np.uint32), r['ordered'].view(np.uint32))
    assert r['tree_rows'] == r['ordered_rows'] == (T * B * R * O, T * B * R * O)         # the order kernels' fallback: every row


def test_full_size_tree_against_dense(gpu):
    """H 512, V 11 322, 20 x 10 x 100, T 21, candidates from a pool, once: as test_full_size_length_ordered_against_dense"""
    from test_lhood_gpu import bound, full_size_params, order_violations
    from visdial_amd.dataloader import SyntheticDataloader
    p = full_size_params()
    batch, _ = SyntheticDataloader(p, seed=7, num_threads=20).getTestBatch(1, p, 'val')
    pooled_candidates(batch, p, np.random.RandomState(77), pool=2000)
    for e in (1, 4242, 19999):
        set_candidate(batch, e, [], p['vocabSize'])
    want_exec, want_total, nodes, live = tree_rows(batch)
    r = tree_dense_ordered(p, batch, with_ordered=False)
    dense, tree = r['dense_of_tree_model'], r['tree']
    tol = bound(dense)
    diff = float(np.abs(dense.astype(np.float64) - tree).max())
    flipped, bad = order_violations(dense, tree, tol)
    print('full size, pooled: %d nodes for %d live rows (%.3f); executed %d of %d = %.3f; worst |dense - tree| %.3e (allowed %.3e); option '
          'pairs in another order %d (unexplained %d)' % (nodes, live, nodes / live, r['tree_rows'][0], r['tree_rows'][1],
                                                          r['tree_rows'][0] / r['tree_rows'][1], diff, tol, flipped, len(bad)))
    assert np.isfinite(tree).all() and diff <= tol, (diff, tol)
    assert not bad, bad[:10]
    assert (tree.reshape(-1)[[1, 4242, 19999]] == 0.0).all()
    np.testing.assert_array_equal(r['tree_ranks'], vo.compute_ranks(tree))
    assert r['tree_rows'] == (want_exec, want_total) and want_total == 21 * 200 * 100


def test_the_switch_is_refused_for_disc_and_for_the_bf16_recurrence(gpu):
    import os
    from conftest import small_params
    from visdial_amd._lib import VisdialHipError
    from visdial_amd.native import NativeModel
    from visdial_amd.opts import derive
    before = os.environ.get('VD_LHOOD_TREE')
    with pytest.raises(VisdialHipError, match=r"VD_LHOOD_TREE.*decoder 'gen'.*'disc'"):
        NativeModel(derive(small_params(encoder='lf-ques', decoder='disc', fusedLhood=2)))
    with pytest.raises(VisdialHipError, match=r"VD_LHOOD_TREE.*lstmBf16 = 1"):
        NativeModel(derive(small_params(encoder='lf-ques', decoder='gen', fusedLhood=2, lstmPrecision='bf16')))
    assert os.environ.get('VD_LHOOD_TREE') == before
