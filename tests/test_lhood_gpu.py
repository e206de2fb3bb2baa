"""The live-row log-likelihood head of generative retrieval on the GPU (csrc/lhood.hip, vd_model_retrieve_lhood, params.fusedLhood):
the operator against numpy fp64 at H = 512, V = 11 322, determinism, the three hosts against the fp64 oracle on the cases of
test_native_gen_retrieval_matches_oracle, dense against fused at full size on both length profiles, and evaluate.py -fusedLhood.

The bound is the project's own for a candidate log-likelihood, 1e-4 * max(1, |ref|.max()) (test_native_gen_retrieval_matches_oracle).
Each path is held to it against the oracle, so two paths may differ by at most twice that, and an option pair may change order between
them only where the dense scores are closer than twice that."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, small_params
from oracle import visdial_oracle as vo
from visdial_amd.dataloader import SyntheticDataloader
from visdial_amd.opts import default_params, derive

pytestmark = pytest.mark.gpu
H, V = 512, 11322


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def dev(a, dtype):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device='cuda')


def bound(ref):
    return 1e-4 * max(1.0, float(np.abs(ref).max())) if np.size(ref) else 1e-4


# ------------------------------------------------------------------------------------------------------------------ the operator
def nll_fp64(h, act, target, W, b):
    x = h[act].astype(np.float64) @ W.astype(np.float64).T + b.astype(np.float64)
    mx = x.max(1)
    lse = mx + np.log(np.exp(x - mx[:, None]).sum(1))
    return lse - x[np.arange(len(act)), target[act] - 1]


def op_case(seed, rows, n_act, scale=1.0):
    """h [rows x H], n_act live rows picked out of it (ascending), targets that include column 0 and column V - 1"""
    rng = np.random.RandomState(seed)
    h = rng.standard_normal((rows, H)).astype(np.float32)
    W = (rng.standard_normal((V, H)) * (scale / np.sqrt(H))).astype(np.float32)
    b = (rng.standard_normal(V) * 0.1).astype(np.float32)
    act = np.sort(rng.choice(rows, size=n_act, replace=False)).astype(np.int32)
    target = rng.randint(1, V + 1, size=rows).astype(np.int32)
    if n_act >= 2:
        target[act[0]], target[act[-1]] = 1, V
    return h, W, b, act, target


def run_nll(h, W, b, act, target):
    from visdial_amd import ops
    nll = torch.full((max(len(act), 1),), float('nan'), device='cuda')
    ops.lhood_nll(dev(h, torch.float32), dev(act, torch.int32) if len(act) else torch.zeros(1, dtype=torch.int32, device='cuda'), len(act),
                  dev(target, torch.int32), dev(W, torch.float32), dev(b, torch.float32), nll)
    torch.cuda.synchronize()
    return nll.cpu().numpy()


@pytest.mark.parametrize("name,rows,n_act,scale", [('base', 20000, 8192, 1.0), ('logits span +-80', 20000, 8192, 20.0),
                                                   ('ragged row tile', 3000, 1037, 1.0), ('no live row', 64, 0, 1.0)])
def test_lhood_nll_matches_fp64(gpu, name, rows, n_act, scale):
    h, W, b, act, target = op_case(3, rows, n_act, scale)
    out = run_nll(h, W, b, act, target)
    if n_act == 0:
        assert np.isnan(out).all()                              # returned at once: nothing written
        return
    ref = nll_fp64(h, act, target, W, b)
    if scale > 1:
        x = h[act[:256]].astype(np.float64) @ W.astype(np.float64).T
        assert x.max() > 60 and x.min() < -60, (x.min(), x.max())
    err = float(np.abs(out[:n_act] - ref).max())
    print('vd_lhood_nll %-18s n_act %5d: worst |err| %.3e  (bound %.3e, |ref| max %.3f)' % (name, n_act, err, bound(ref), np.abs(ref).max()))
    assert np.isfinite(out[:n_act]).all()
    assert err < bound(ref), (err, bound(ref))


def test_lhood_nll_is_deterministic_and_position_independent(gpu):
    h, W, b, act, target = op_case(5, 6000, 2500)
    # the rows act[7] (tile 0), act[200] (tile 1, another lane) and act[2499] (the ragged last tile) become copies of one row
    for i in (200, 2499):
        h[act[i]] = h[act[7]]
        target[act[i]] = target[act[7]]
    a, b2 = run_nll(h, W, b, act, target), run_nll(h, W, b, act, target)
    assert np.array_equal(a.view(np.uint32), b2.view(np.uint32))
    assert a[7].view(np.uint32) == a[200].view(np.uint32) == a[2499].view(np.uint32)
    assert np.abs(a[:2500] - nll_fp64(h, act, target, W, b)).max() < 1e-4 * max(1.0, np.abs(a).max())


def test_lhood_live_rows_and_sum(gpu):
    """the two companions against numpy: the live-row list of a [T x rows] batch with an empty candidate, and the per-candidate sum
    in step order, negated, written at a column offset of a wider score matrix"""
    from visdial_amd import ops
    rng = np.random.RandomState(9)
    T, rows, Cc = 21, 2600, 13                                  # 2600 = 200 rounds x 13 options: 54 600 rows, 54 counting blocks
    lens = rng.randint(0, T, size=rows)
    lens[5] = 0
    oin = np.zeros((T, rows), np.int32)
    oout = np.zeros((T, rows), np.int32)
    for r in range(rows):
        L = int(lens[r])
        oin[0, r] = 99
        oin[1:1 + L, r] = rng.randint(1, 90, size=L)
        if L:
            oout[:L, r] = oin[1:1 + L, r]
            oout[L, r] = 100
    want = np.flatnonzero((oin.reshape(-1) != 0) & (oout.reshape(-1) > 0)).astype(np.int32)
    n = T * rows
    act = torch.full((n,), -1, dtype=torch.int32, device='cuda')
    work = torch.zeros(((n + 1023) // 1024 + 1,), dtype=torch.int32, device='cuda')
    cnt = ops.lhood_live_rows(dev(oin.reshape(-1), torch.int32), dev(oout.reshape(-1), torch.int32), act, work)
    assert cnt == len(want)
    np.testing.assert_array_equal(act[:cnt].cpu().numpy(), want)
    nll = rng.standard_normal(cnt).astype(np.float32)
    O = 20
    out = torch.full((rows // Cc, O), 7.0, device='cuda')
    ops.lhood_sum(dev(nll, torch.float32), act, cnt, T, rows, Cc, out, O, dst_off=3)
    ref = np.full((rows // Cc, O), 7.0, np.float32)
    full = np.zeros(n, np.float32)
    full[want] = nll
    acc = np.zeros(rows, np.float32)
    for t in range(T):                                          # fp32, step order
        acc = acc + full[t * rows:(t + 1) * rows]
    ref[:, 3:3 + Cc] = -acc.reshape(-1, Cc)
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got, ref)
    assert got[0, 3 + 5] == 0.0                                 # the empty candidate


# ------------------------------------------------------------------------------------------------- the three hosts against the oracle
def oracle_case(enc):
    kw = dict(imgNorm=1, dropout=0.5, numOptions=12, batchSize=2)
    if 'att' in enc:
        kw.update(imgFeatureSize=32, imgSpatialSize=3)
    p = derive(small_params(encoder=enc, decoder='gen', **kw))
    batch, _ = SyntheticDataloader(p, seed=31, num_threads=4).getTestBatch(1, p, 'val')
    batch['option_in'][0, 0, 1, 1:] = 0           # an EMPTY candidate scores log-likelihood 0
    batch['option_out'][0, 0, 1, :] = 0
    if batch['answer_ind'][0] == 2:
        batch['answer_ind'][0] = 1
    return p, batch


@pytest.mark.parametrize("enc", ['lf-ques', 'lf-ques-im-hist', 'mn-att-ques-im-hist', 'hre-ques-im-hist', 'hrea-ques-im-hist'])
def test_fused_lhood_retrieval_matches_oracle_on_every_host(gpu, enc):
    """test_native_gen_retrieval_matches_oracle with fusedLhood = 1 through the native host, the operator-level host and the Lua host
    on the real library: scores within the oracle bound, GT ranks and all ranks = compute_ranks of the device scores"""
    from lua_host import LuaHost, first
    from luavm import to_py
    from visdial_amd import _lib, t7
    from visdial_amd.model import Model
    from visdial_amd.native import NativeModel
    p, batch = oracle_case(enc)
    p['fusedLhood'] = 1
    N, O = batch['option_in'].shape[0] * batch['option_in'].shape[1], batch['option_in'].shape[2]
    gt = batch['answer_ind'].reshape(-1) - 1
    nat = NativeModel(dict(p), init_seed=3)
    nat.training(False)
    Pf = nat.get_parameters_dict()
    ref = vo.retrieve(enc, 'gen', {k: v.astype(np.float64) for k, v in Pf.items()}, p, batch).reshape(-1)

    def check(who, scores, gt_ranks, all_ranks):
        err = float(np.abs(scores - ref).max())
        print('%-26s %-8s worst |score - oracle| %.3e (bound %.3e)' % (enc, who, err, bound(ref)))
        assert np.isfinite(scores).all() and err < bound(ref), (who, err)
        assert scores[1] == 0.0, who                            # the planted empty candidate (round 0, option 1), exactly
        np.testing.assert_array_equal(np.asarray(gt_ranks).reshape(-1), vo.compute_ranks(scores.reshape(N, O), gt), err_msg=who)
        np.testing.assert_array_equal(np.asarray(all_ranks).reshape(N, O), vo.compute_ranks(scores.reshape(N, O)), err_msg=who)

    g = nat.retrieveBatch(batch, useGt=True)
    s_nat = nat.scores(N, O)
    check('native', s_nat.reshape(-1), g, nat.retrieveBatch(batch, useGt=False))
    # the operator-level host on the same parameters
    py = Model(dict(p))
    py.set_parameters_dict(Pf)
    py.wrapper.evaluate()
    py.params['useGt'] = True
    g = np.asarray(py.retrieveBatch(batch))
    s_py = py.scores.cpu().numpy().copy()
    py.params['useGt'] = False
    check('python', s_py.reshape(-1), g, np.asarray(py.retrieveBatch(batch)))
    # the Lua host on the real library
    host = LuaHost(p)
    m = host.model()
    host.invoke(m, 'setFlatParameters', host.tensor(t7.named_to_flat(Pf, nat._entries(), enc), 'Float'))
    host.invoke(m, 'setMode', False)
    host.get(m, 'params').set('fusedLhood', 1)
    host.get(m, 'params').set('useGt', True)
    g = to_py(first(host.invoke(m, 'retrieveBatch', host.batch(batch))))
    s_lua = np.empty((N, O), np.float32)
    _lib.call('vd_model_scores', C.c_void_p(host.get(m, 'h').val), s_lua.ctypes.data, s_lua.size)
    host.get(m, 'params').set('useGt', False)
    check('lua', s_lua.reshape(-1), g, to_py(first(host.invoke(m, 'retrieveBatch', host.batch(batch)))))
    nat.close()
    host.close()


def test_disc_model_is_refused_by_the_library(gpu):
    from visdial_amd._lib import VisdialHipError
    from visdial_amd.native import NativeModel
    p = derive(small_params(encoder='lf-ques', decoder='disc', fusedLhood=1))
    batch = SyntheticDataloader(p, seed=13).getTrainBatch(p)
    nat = NativeModel(p)
    with pytest.raises(VisdialHipError, match="vd_model_retrieve_lhood.*'disc'"):
        nat.retrieveBatch(batch, useGt=True)
    nat.close()


# ------------------------------------------------------------------------------------------------------------------------ full size
def full_size_params():
    return derive(default_params(encoder='lf-ques-im-hist', decoder='gen', vocabSize=V, embedSize=300, rnnHiddenSize=H,
                                 imgFeatureSize=4096, numLayers=2, maxQuesCount=10, maxQuesLen=20, maxAnsLen=20,
                                 maxHistoryLenPerRound=40, numOptions=100, batchSize=20, gpuid=0))


def set_option_lengths(batch, lens, p, rng):
    """replace the candidates of a gen retrieval batch by ones of the given lengths [N * O] (0 = an empty candidate), T = 21"""
    B, R, O = batch['option_in'].shape[:3]
    T = int(p['maxAnsLen']) + 1
    oin = np.zeros((B * R * O, T), np.int32)
    oout = np.zeros((B * R * O, T), np.int32)
    tok = rng.randint(1, V - 1, size=(B * R * O, T - 1)).astype(np.int32)
    pos = np.arange(T - 1)[None, :]
    body = tok * (pos < lens[:, None])
    oin[:, 0] = V - 1                                           # <START>
    oin[:, 1:] = body
    oout[:, :T - 1] = body
    oout[np.arange(len(lens)), lens] = np.where(lens > 0, V, 0)  # <END>; none for an empty candidate (processOptions)
    batch['option_in'], batch['option_out'] = oin.reshape(B, R, O, T), oout.reshape(B, R, O, T)


def profile_lengths(profile, n, rng):
    if profile == 'uniform':                                    # the synthetic loader's own: uniform 1..20
        return rng.randint(1, 21, size=n)
    return np.minimum(20, 1 + rng.poisson(2.0, size=n))          # mean 3, capped at 20: stands in for VisDial's answer lengths


def order_violations(dense, fused, tol):
    """option pairs whose order differs between the two paths (ties by lower index), and those of them whose DENSE scores are
    further apart than tol"""
    idx = np.arange(dense.shape[1])
    before = lambda s: (s[:, None] > s[None, :]) | ((s[:, None] == s[None, :]) & (idx[:, None] < idx[None, :]))
    flipped, bad = 0, []
    for r in range(dense.shape[0]):
        a, b = np.nonzero(np.triu(before(dense[r]) != before(fused[r]), 1))
        flipped += a.size
        gap = np.abs(dense[r, a].astype(np.float64) - dense[r, b])
        bad += [(r, int(a[k]), int(b[k]), float(gap[k])) for k in np.nonzero(gap > tol)[0]]
    return flipped, bad


@pytest.mark.parametrize("profile", ['uniform', 'short'])
def test_full_size_fused_against_dense(gpu, profile):
    """20 dialogs x 10 rounds x 100 options, T 21, V 11 322, H 512 through the native host, dense and fused on the same model and batch"""
    from visdial_amd.native import NativeModel
    p = full_size_params()
    rng = np.random.RandomState(77)
    batch, _ = SyntheticDataloader(p, seed=7, num_threads=20).getTestBatch(1, p, 'val')
    lens = profile_lengths(profile, 20 * 10 * 100, rng)
    empty = [1, 4242, 19999]
    lens[empty] = 0
    set_option_lengths(batch, lens, p, rng)
    dup = (37 * 100 + 3, 37 * 100 + 58)                         # round 37: option 58 is a copy of option 3
    for k in ('option_in', 'option_out'):
        flat = batch[k].reshape(-1, batch[k].shape[-1])
        flat[dup[1]] = flat[dup[0]]
    nat = NativeModel(dict(p), init_seed=1)
    nat.training(False)
    N, O = 200, 100
    nat.retrieveBatch(batch, useGt=False)
    dense = nat.scores(N, O).copy()
    nat.params['fusedLhood'] = 1
    all_fused = np.asarray(nat.retrieveBatch(batch, useGt=False)).reshape(N, O)
    fused = nat.scores(N, O).copy()
    nat.retrieveBatch(batch, useGt=False)
    assert np.array_equal(fused.view(np.uint32), nat.scores(N, O).view(np.uint32))     # the same call twice: bit-identical
    nat.close()
    tol = 2 * bound(dense)
    diff = float(np.abs(dense.astype(np.float64) - fused).max())
    flipped, bad = order_violations(dense, fused, tol)
    live = float(((batch['option_in'] != 0) & (batch['option_out'] > 0)).mean())
    print('full size, %s lengths: live rows %.3f, worst |dense - fused| %.3e (allowed %.3e), option pairs in another order %d (unexplained %d)'
          % (profile, live, diff, tol, flipped, len(bad)))
    assert np.isfinite(fused).all() and diff <= tol, (diff, tol)
    assert not bad, bad[:10]
    for e in empty:                                             # exactly 0 on both paths
        assert dense.reshape(-1)[e] == 0.0 and fused.reshape(-1)[e] == 0.0
    # the planted duplicate ties exactly and ranks by index
    assert fused.reshape(-1)[dup[0]].view(np.uint32) == fused.reshape(-1)[dup[1]].view(np.uint32)
    assert all_fused[37, 58] == all_fused[37, 3] + 1
    np.testing.assert_array_equal(all_fused, vo.compute_ranks(fused))


# ------------------------------------------------------------------------------------------------------------------------------ CLI
def test_evaluate_fused_lhood_cli(gpu, tmp_path):
    """evaluate.py -fusedLhood 1 on a gen checkpoint of a short train.py run, both hosts: the metrics and rank records of
    -fusedLhood 0, up to ground-truth ranks moved by a near tie of the dense scores"""
    save = str(tmp_path / "ckpt") + "/"
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '-encoder', 'lf-ques-im-hist', '-decoder', 'gen', '-imgFeatureSize', '64',
                        '-rnnHiddenSize', '64', '-embedSize', '32', '-batchSize', '4', '--vocabSize', '200', '--numTrainThreads', '40',
                        '-host', 'native', '-savePath', save, '-numEpochs', '10', '-saveIter', '10', '--maxIters', '100'],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = {}
    for host in ('native', 'python'):
        for flag in (0, 1):
            path = str(tmp_path / ('ranks_%s_%d.json' % (host, flag)))
            e = subprocess.run([sys.executable, os.path.join(ROOT, 'evaluate.py'), '-loadPath', save + 'model_final.t7', '-batchSize', '4',
                                '--numThreads', '8', '-saveRanks', '1', '-saveRankPath', path, '-host', host, '-fusedLhood', str(flag)],
                               capture_output=True, text=True, timeout=600, cwd=ROOT)
            assert e.returncode == 0, e.stdout[-2000:] + e.stderr[-2000:]
            assert 'r@1:' in e.stdout and 'meanRR:' in e.stdout
            metrics = [l for l in e.stdout.splitlines() if l.startswith('\t')]           # utils.processRanks' lines
            out[host, flag] = (metrics, json.load(open(path)))
    for host in ('native', 'python'):
        (m0, r0), (m1, r1) = out[host, 0], out[host, 1]
        assert len(r0) == len(r1) and [(a['image_id'], a['round_id']) for a in r0] == [(a['image_id'], a['round_id']) for a in r1]
        moved = [(a, b) for a, b in zip(r0, r1) if a['ranks'] != b['ranks']]
        if not moved:
            assert m0 == m1, (m0, m1)
            continue
        # a ground-truth rank moved: only a near tie of the dense scores explains it
        from visdial_amd.checkpoint import load_checkpoint, restore_weights
        from visdial_amd.native import NativeModel
        saved = load_checkpoint(save + 'model_final.t7')
        p = derive(saved['modelParams'])
        p.update(gpuid=0, batchSize=4, useGt=True)
        dl = SyntheticDataloader(p, seed=4321, num_threads=8)
        nat = NativeModel(p)
        restore_weights(nat, saved, None)
        nat.training(False)
        R, O, start, bad = p['maxQuesCount'], p['numOptions'], 1, 0
        while start <= 8:
            batch, nxt = dl.getTestBatch(start, p, 'val')
            nat.retrieveBatch(batch, useGt=True)
            dense = nat.scores((nxt - start) * R, O).copy()
            nat.params['fusedLhood'] = 1
            nat.retrieveBatch(batch, useGt=True)
            fused = nat.scores((nxt - start) * R, O).copy()
            nat.params['fusedLhood'] = 0
            bad += len(order_violations(dense, fused, 2 * bound(dense))[1])
            start = nxt
        nat.close()
        assert bad == 0, (host, moved[:3])


def test_evaluate_refuses_fused_lhood_for_a_disc_checkpoint(gpu, tmp_path):
    save = str(tmp_path / "ckpt") + "/"
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '-encoder', 'lf-ques', '-decoder', 'disc', '-rnnHiddenSize', '64',
                        '-embedSize', '32', '-batchSize', '4', '--vocabSize', '100', '--numTrainThreads', '8', '-host', 'native',
                        '-savePath', save, '-numEpochs', '1', '-saveIter', '10', '--maxIters', '2'],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    e = subprocess.run([sys.executable, os.path.join(ROOT, 'evaluate.py'), '-loadPath', save + 'model_final.t7', '-fusedLhood', '1'],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert e.returncode != 0 and 'only for a generative model' in (e.stdout + e.stderr)
