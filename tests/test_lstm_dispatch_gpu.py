"""The corners of the recurrence step dispatch (csrc/lstm.hip: lstm_step_fwd / lstm_step_bwd hold each ladder once, for every epilogue).

H = 32; N = 40 takes the 32-row latency kernels with a ragged last tile, N = 2 088 the throughput kernels with a ragged 128-row tile.
Forward: T = 1 (with h0 at N = 2 088: a throughput shape on the generic kernel with K > 0) and T = 3 (without h0: K = 0 first, then the
pipeline), with and without h0 / c0, dense projection and token table, for flags 0, STATE_ONLY, LIVE_PREFIX, TREE with identity parents,
and SPLIT9 (alone and with STATE_ONLY) where the split runs.  Backward: one or two incoming operands at the last step, with and without
dc_last, fp32 / SPLIT9 / BF16.

Every bound is one the project already holds at other shapes: flags 0 and SPLIT9 against the fp64 restatement with the bounds of
test_ops_gpu.test_lstm_forward_backward (1e-5 forward, 2e-5 backward), BF16 with the gradient bound of
test_model_gpu.test_bf16_option_lstm_step (2e-2), and STATE_ONLY / LIVE_PREFIX / TREE bit for bit against the call they restate
(test_option_cache_gpu, test_lhood_prefix_gpu, test_lhood_tree_gpu)."""
import functools

import numpy as np
import pytest
import torch

from oracle import visdial_oracle as vo

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0
H, D, V = 32, 20, 30
# live rows per step: tokens are left-aligned and the rows lie in order of descending length, so the live rows of a step are a prefix.
# (40, 3): a ragged second tile, then a step with no live row; (2088, 1): dead row groups at the only step; (2088, 3): down to under a tile
NACT = {(40, 1): [40], (40, 3): [40, 33, 0], (2088, 1): [1500], (2088, 3): [2088, 1000, 100]}
SHAPES = [(N, T) for N in (40, 2088) for T in (1, 3)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from visdial_amd import ops as o
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def relerr(got, ref):
    got = got.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(got) else np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30))


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@functools.lru_cache(maxsize=None)
def inputs(N, T, masked=True):
    """seeded inputs of one shape and their fp64 forward state, with and without h0 / c0: computed once, read by every test"""
    rng = np.random.RandomState(7 * N + T)
    f32 = lambda *s: rng.randn(*s).astype(np.float32)
    emb = f32(V + 1, D)
    emb[0] = 0
    tok = rng.randint(1, V + 1, size=(T, N)).astype(np.int32)
    if masked:
        for t, n in enumerate(NACT[N, T]):
            tok[t, n:] = 0
    W = (f32(D + H, 4 * H) / np.sqrt(D + H)).astype(np.float32)
    b = f32(4 * H) * 0.1
    h0, c0 = f32(N, H) * 0.5, f32(N, H) * 0.5
    x = emb[tok]
    W64, b64 = W.astype(np.float64), b.astype(np.float64)
    ref = {w: vo.lstm_forward(x.astype(np.float64), W64, b64, tok if masked else None, h0.astype(np.float64) if w else None,
                              c0.astype(np.float64) if w else None) for w in (False, True)}
    tab = (emb.astype(np.float64) @ W64[:D] + b64).astype(np.float32)
    xp = (x.reshape(T * N, D).astype(np.float64) @ W64[:D] + b64).astype(np.float32)
    return dict(tok=tok, x=x, W=W, h0=h0, c0=c0, tab=tab, xp=xp, ref=ref)


def forward(ops, N, T, with_h0, mode, flags):
    """one vd_lstm_forward call on the shape's inputs, every output pre-filled with the sentinel -> (gates or None, h, c) as numpy"""
    I = inputs(N, T)
    state_only, tree = bool(flags & ops.FLAG_STATE_ONLY), bool(flags & ops.FLAG_TREE)
    gates = None if state_only or tree else torch.full((T, N, 4 * H), SENTINEL, device="cuda")
    h = torch.full((2 if state_only else T, N, H), SENTINEL, device="cuda")
    c = torch.full((2 if state_only else T, N, H), SENTINEL, device="cuda")
    tok = dev(I['tok'])
    mask = tok
    if tree:   # plane 1: every row continues itself; the entries of rows without a node are never used as rows
        par = np.broadcast_to(np.arange(N, dtype=np.int32), (T, N)).copy()
        par[I['tok'] == 0] = 2 ** 30
        mask = dev(np.stack([I['tok'], par]))
    kw = dict(tok_mask=mask, h0=dev(I['h0']) if with_h0 else None, c0=dev(I['c0']) if with_h0 else None, flags=flags)
    if mode == 'table':
        ops.lstm_forward(dev(I['tab']), dev(I['W'][D:]), gates, h, c, T, N, H, 0, 4 * H, tok_gather=tok, **kw)
    else:
        ops.lstm_forward(dev(I['xp']), dev(I['W'][D:]), gates, h, c, T, N, H, N * 4 * H, 4 * H, **kw)
    torch.cuda.synchronize()
    return (None if gates is None else gates.cpu().numpy()), h.cpu().numpy(), c.cpu().numpy()


@functools.lru_cache(maxsize=None)
def saving_call(ops, N, T, with_h0, mode, flags=0):
    """the plain call (gates saved, every row computed) that the other modes restate: run once per case"""
    return forward(ops, N, T, with_h0, mode, flags)


def FWD_SPLIT(test):
    """h0 / c0 absent or present x dense projection or token table"""
    return pytest.mark.parametrize("mode", ['dense', 'table'])(pytest.mark.parametrize("with_h0", [False, True])(test))


def FWD(test):
    return FWD_SPLIT(pytest.mark.parametrize("N,T", SHAPES)(test))


def check_against_fp64(N, T, with_h0, out):
    h_ref, c_ref, g_ref = inputs(N, T)['ref'][with_h0]
    gates, h, c = out
    errs = relerr(h, h_ref), relerr(c, c_ref), relerr(gates, g_ref)
    print("rel-L2 vs fp64 (h, c, gates):", errs)
    assert not (h == SENTINEL).any() and not (c == SENTINEL).any() and not (gates == SENTINEL).any()
    assert errs[0] < 1e-5 and errs[1] < 1e-5 and errs[2] < 1e-5


@FWD
def test_forward_fp32_matches_fp64(ops, N, T, with_h0, mode):
    check_against_fp64(N, T, with_h0, saving_call(ops, N, T, with_h0, mode))


@FWD_SPLIT
def test_forward_split9_matches_fp64(ops, with_h0, mode):
    check_against_fp64(2088, 3, with_h0, saving_call(ops, 2088, 3, with_h0, mode, ops.FLAG_SPLIT9))


def check_state_only(ops, N, T, with_h0, mode, flags):
    _, h, c = saving_call(ops, N, T, with_h0, mode, flags)
    _, h2, c2 = forward(ops, N, T, with_h0, mode, flags | ops.FLAG_STATE_ONLY)
    last = (T - 1) & 1
    assert same_bits(h2[last], h[T - 1]) and same_bits(c2[last], c[T - 1])
    assert float(np.abs(h[T - 1]).max()) > 0.05 or NACT[N, T][-1] == 0


@FWD
def test_forward_state_only_ends_in_the_saving_calls_state(ops, N, T, with_h0, mode):
    check_state_only(ops, N, T, with_h0, mode, 0)


@FWD_SPLIT
def test_forward_state_only_split9_ends_in_the_saving_calls_state(ops, with_h0, mode):
    check_state_only(ops, 2088, 3, with_h0, mode, ops.FLAG_SPLIT9)


@FWD
def test_forward_live_prefix_equals_the_plain_call_on_live_tiles(ops, N, T, with_h0, mode):
    full = saving_call(ops, N, T, with_h0, mode)
    live = forward(ops, N, T, with_h0, mode, ops.FLAG_LIVE_PREFIX)
    G, tile = ops.LIVE_PREFIX_ROWS, ops.lstm_fwd_row_tile(N)
    dead_rows = 0
    for what, a, b in zip(('gates', 'h', 'c'), full, live):
        for t, n in enumerate(NACT[N, T]):
            run = min(N, -(-n // tile) * tile)                 # a tile whose first row is live runs whole: its pad rows are stored as zeros
            assert same_bits(a[t, :run], b[t, :run]), (what, t)
            end = min(N, -(-n // G) * G)
            assert (b[t, end:] == SENTINEL).all(), (what, t, 'a dead row group was written')
            assert ((b[t, run:end] == 0) | (b[t, run:end] == SENTINEL)).all(), (what, t)
            dead_rows += N - end
    assert dead_rows > 0 or (N, T) == (40, 1)


@FWD
def test_forward_tree_with_identity_parents_equals_live_prefix(ops, N, T, with_h0, mode):
    live = forward(ops, N, T, with_h0, mode, ops.FLAG_LIVE_PREFIX)
    tree = forward(ops, N, T, with_h0, mode, ops.FLAG_TREE)
    G = ops.LIVE_PREFIX_ROWS
    for what, a, b in zip(('h', 'c'), live[1:], tree[1:]):
        for t, n in enumerate(NACT[N, T]):
            assert not (a[t, :n] == SENTINEL).any(), (what, t)
            assert same_bits(a[t, :n], b[t, :n]), (what, t)
            end = min(N, -(-n // G) * G)
            assert (b[t, end:] == SENTINEL).all(), (what, t, 'a dead row group was written')
            assert ((b[t, n:end] == 0) | (b[t, n:end] == SENTINEL)).all(), (what, t)


# ------------------------------------------------------------------------------------------------------------------ backward
@functools.lru_cache(maxsize=None)
def backward_reference(N, T, two, with_dc):
    """fp64 backward from the exact forward state of the unmasked inputs (no h0): every row live, so that the second operand matters"""
    I = inputs(N, T, masked=False)
    h_ref, c_ref, g_ref = I['ref'][False]
    rng = np.random.RandomState(N + T)
    dh_seq, dh_last, dc_last = (rng.randn(*s).astype(np.float32) for s in ((T, N, H), (N, H), (N, H)))
    dh_last = dh_last if two else None
    dc_last = dc_last if with_dc else None
    f64 = lambda a: None if a is None else a.astype(np.float64)
    _, dW, _, dh0, dc0, da = vo.lstm_backward(I['x'].astype(np.float64), I['W'].astype(np.float64), g_ref, h_ref, c_ref, dh_seq=f64(dh_seq),
                                              dh_last=f64(dh_last), dc_last=f64(dc_last), return_da=True)
    return dict(dh_seq=dh_seq, dh_last=dh_last, dc_last=dc_last, dWh=dW[D:], dh0=dh0, dc0=dc0, da=da)


def backward_cases():
    for N, T in SHAPES:
        for two in (False, True):
            for with_dc in (False, True):
                for arith in ('fp32', 'split9') + (('bf16',) if N == 2088 else ()):
                    yield pytest.param(N, T, two, with_dc, arith, id="N%d-T%d-%s-%s-%s" % (N, T, 'dh_seq+dh_last' if two else 'dh_seq',
                                                                                          'dc_last' if with_dc else 'no_dc_last', arith))


@pytest.mark.parametrize("N,T,two,with_dc,arith", backward_cases())
def test_backward_matches_fp64(ops, N, T, two, with_dc, arith):
    I, R = inputs(N, T, masked=False), backward_reference(N, T, two, with_dc)
    h_ref, c_ref, g_ref = I['ref'][False]
    # the exact forward state, so that the backward arithmetic alone is measured (as test_split_error_table feeds it)
    gates, c, h = dev(g_ref.astype(np.float32)), dev(c_ref.astype(np.float32)), dev(h_ref.astype(np.float32))
    dc_work, dh0 = torch.full((N, H), SENTINEL, device="cuda"), torch.full((N, H), SENTINEL, device="cuda")
    opt = lambda a: None if a is None else dev(a)
    kw = dict(dh_seq=dev(R['dh_seq']), dh_last=opt(R['dh_last']), dc_last=opt(R['dc_last']), dh0=dh0, flags=ops.PRECISION_FLAGS[arith])
    dWh0 = np.random.RandomState(3).randn(H, 4 * H).astype(np.float32)
    dWh = dev(dWh0)
    if arith != 'bf16':   # (the bf16 contraction reads the shadows a bf16 FORWARD pass registers for h: not this file's subject)
        kw.update(h_seq=h, dWh=dWh)
    ops.lstm_backward(dev(I['W'][D:]), gates, c, dc_work, T, N, H, **kw)
    torch.cuda.synchronize()
    errs = dict(da=relerr(gates, R['da']), dc0=relerr(dc_work, R['dc0']), dh0=relerr(dh0, R['dh0']), dWh=relerr(dWh, dWh0 + R['dWh']))
    print("rel-L2 vs fp64:", errs)
    # fp32 and the exact split: the bound of test_lstm_forward_backward(_split9); bf16 operands: the gradient bound of test_bf16_option_lstm_step
    bound = 2e-2 if arith == 'bf16' else 2e-5
    if arith == 'bf16':
        del errs['dWh']
    assert all(e < bound for e in errs.values()), errs
