"""The model-level C ABI (csrc/runtime.hip, the calls a LuaJIT model.lua proxy makes -- INTEGRATION.md) against the
CPU oracle and against the Python host that composes the operator-level entry points: same step, same numbers."""
import numpy as np
import pytest
import torch

from conftest import grad_mismatches, small_params, unexplained_rank_flips
from oracle import visdial_oracle as vo
from test_model_gpu import ALL_ENC, CASES, WIDE, fuse_masks, make_masks, rel
from visdial_amd.dataloader import SyntheticDataloader
from visdial_amd.opts import derive

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.mark.parametrize("case", ['tiny', 'odd', 'hops3', 'mid'])
@pytest.mark.parametrize("train_mode", [False, True])
def test_native_step_matches_oracle(gpu, case, train_mode):
    from visdial_amd.native import NativeModel
    p = derive(small_params(**CASES[case]))
    batch = SyntheticDataloader(p, seed=11).getTrainBatch(p)
    model = NativeModel(p, init_seed=5)
    masks = None
    if train_mode:
        masks = make_masks(p, batch, np.random.RandomState(5))
        model.set_dropout_masks(masks)
    else:
        model.training(False)
    P0 = {k: v.astype(np.float64) for k, v in model.get_parameters_dict().items()}
    assert set(P0) == {e[0] for e in vo.param_spec(p['encoder'], p['decoder'], p)}
    loss = model.forwardBackward(batch)
    drop = {k: v.astype(np.float64) for k, v in masks.items()} if masks else None
    ref = vo.forward_backward(p['encoder'], p['decoder'], P0, p, batch, drop)
    assert abs(loss - ref['loss']) < 1e-4
    g = model.get_gradients_dict()
    bad = grad_mismatches(g, ref['grads'])
    assert not bad, bad
    N, O = batch['options'].shape[0], batch['options'].shape[1]
    assert rel(model.scores(N, O), ref['scores']) < 1e-4
    model.update()
    after = model.get_parameters_dict()
    for k in P0:
        w2, _ = vo.clamp_adam(P0[k].reshape(-1), g[k].astype(np.float64).reshape(-1), {}, p['learningRate'])
        assert np.abs(after[k].reshape(-1) - w2).max() < 1e-6, k
    model.close()


def test_native_equals_python_host(gpu):
    """same parameters, same batch, same pinned dropout masks: the two hosts launch the same kernels"""
    from visdial_amd.model import Model
    from visdial_amd.native import NativeModel
    p = derive(small_params(**CASES['odd']))
    batch = SyntheticDataloader(p, seed=3).getTrainBatch(p)
    masks = make_masks(p, batch, np.random.RandomState(1))
    py = Model(p)
    py.set_dropout_masks(masks)
    nat = NativeModel(p)
    nat.set_parameters_dict(py.get_parameters_dict())
    nat.set_dropout_masks(masks)
    py.wrapper.zeroGradParameters()
    l1 = py.forwardBackward(batch)
    l2 = nat.forwardBackward(batch)
    assert abs(l1 - l2) < 1e-6
    g1, g2 = py.get_gradients_dict(), nat.get_gradients_dict()
    for k in g1:
        assert rel(g2[k], g1[k]) < 2e-6 or np.abs(g2[k] - g1[k]).max() < 1e-7, k     # float atomics: order-dependent sums
    nat.close()


def test_native_training_loop_and_ranks(gpu):
    from visdial_amd.native import NativeModel
    p = derive(small_params(**CASES['tiny']))
    dl = SyntheticDataloader(p, seed=9)
    fixed = dl.getTrainBatch(p)
    dl.getTrainBatch = lambda params, **kw: fixed        # overfit one batch: the loss must fall
    model = NativeModel(p)
    losses = [model.trainIteration(dl) for _ in range(60)]
    assert np.isfinite(losses).all() and losses[-1] < 0.5 * losses[0]
    model.training(False)
    ranks = model.retrieveBatch(fixed, useGt=True)
    P = {k: v.astype(np.float64) for k, v in model.get_parameters_dict().items()}
    ref = vo.retrieve(p['encoder'], p['decoder'], P, p, fixed)
    N, O = fixed['options'].shape[0], fixed['options'].shape[1]
    dev = model.scores(N, O)
    assert rel(dev, ref) < 1e-4
    np.testing.assert_array_equal(ranks, vo.compute_ranks(dev, fixed['answer_ind'].reshape(-1) - 1))
    allr = model.retrieveBatch(fixed, useGt=False)
    assert np.all(np.sort(allr, 1) == np.arange(1, O + 1)[None, :])
    model.close()


def test_native_refuses_unknown_plugins(gpu):
    from visdial_amd import _lib
    from visdial_amd.native import NativeModel
    with pytest.raises(_lib.VisdialHipError):
        NativeModel(derive(small_params(encoder='lf-ques', decoder='gen')) | {'encoder': 'lf-quesX'})
    with pytest.raises(_lib.VisdialHipError):
        NativeModel(derive(small_params(encoder='lf-ques', decoder='gen')) | {'decoder': 'ctc'})


def test_native_refuses_unknown_precision(gpu):
    """vd_model_params.lstmBf16 takes 0, 1, 3, 6 or 9; any other value is an argument error, not a quiet fp32 pass"""
    import ctypes as C
    from visdial_amd import _lib
    mp = _lib.ModelParams(vocabSize=60, embedSize=20, rnnHiddenSize=64, maxQuesCount=5, numOptions=9, lstmBf16=5)
    h = C.c_void_p()
    with pytest.raises(_lib.VisdialHipError, match='lstmBf16'):
        _lib.call("vd_model_create", C.byref(mp), b'lf-ques', b'disc', C.byref(h))
    assert not h.value


def pair_matches_oracle(p, pinned):
    """one step of p's encoder x decoder pair through the MODEL-LEVEL ABI (what lua/model.lua calls): loss, every gradient tensor,
    forward-only mode, one Adam step -- against the fp64 oracle.  pinned: training mode with pinned dropout masks (evaluate mode for a
    pair without a dropout site), else evaluate mode."""
    from visdial_amd.native import NativeModel
    enc, dec = p['encoder'], p['decoder']
    batch = SyntheticDataloader(p, seed=21).getTrainBatch(p)
    model = NativeModel(p, init_seed=17)
    assert [t[0] for t in model.tensors] == [e[0] for e in vo.param_spec(enc, dec, p)]
    masks = fuse_masks(p, batch, np.random.RandomState(8)) if pinned else None
    if masks is not None:
        model.set_dropout_masks(masks)
    else:
        model.training(False)
    P0 = {k: v.astype(np.float64) for k, v in model.get_parameters_dict().items()}
    loss = model.forwardBackward(batch)
    drop = {k: v.astype(np.float64) for k, v in masks.items()} if masks else None
    ref = vo.forward_backward(enc, dec, P0, p, batch, drop)
    assert abs(loss - ref['loss']) < 1e-4 * max(1.0, abs(ref['loss']))
    g = model.get_gradients_dict()
    bad = grad_mismatches(g, ref['grads'])
    assert not bad, bad
    # forward-only (Model:evaluate path, model.lua:128): same loss, gradients untouched
    loss2 = model.forwardBackward(batch, onlyForward=True)
    assert abs(loss2 - loss) < 1e-5 * max(1.0, abs(loss))
    g2 = model.get_gradients_dict()
    assert all(np.array_equal(g[k], g2[k]) for k in g)
    model.update()
    after = model.get_parameters_dict()
    for k in P0:
        w2, _ = vo.clamp_adam(P0[k].reshape(-1), g[k].astype(np.float64).reshape(-1), {}, p['learningRate'])
        assert np.abs(after[k].reshape(-1) - w2).max() < 1e-6, k
    model.close()
    return P0


@pytest.mark.parametrize("enc,dec", [(e, d) for e in ALL_ENC for d in ('disc', 'gen')
                                     if (e, d) != ('mn-att-ques-im-hist', 'disc')])     # that pair: tests above
@pytest.mark.parametrize("case", ['tiny', 'mid'])
def test_native_all_pairs_match_oracle(gpu, enc, dec, case):
    """every encoder x decoder plug-in pair.  tiny: training mode with pinned dropout masks; mid: evaluate mode at H = 512 / 100
    options."""
    kw = dict(WIDE[case])
    if 'att' in enc:
        kw.update(imgFeatureSize=32 if case == 'tiny' else 512, imgSpatialSize=3 if case == 'tiny' else 7)
    pair_matches_oracle(derive(small_params(encoder=enc, decoder=dec, **kw)), pinned=case == 'tiny')


@pytest.mark.parametrize("dec", ['disc', 'gen'])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("enc", ['lf-ques-hist', 'lf-ques-im-hist', 'hre-ques-im-hist', 'hrea-ques-im-hist'])
def test_native_history_branch_at_other_depths_matches_oracle(gpu, enc, L, dec):
    """numLayers = 1 and 3, where the history branch of the Sequential encoders leaves the two-layer wavefront for one recurrence per
    layer (csrc/rt_encoders.h HistoryBranch): the 'tiny' case of test_native_all_pairs_match_oracle at those depths"""
    P0 = pair_matches_oracle(derive(small_params(encoder=enc, decoder=dec, numLayers=L, **WIDE['tiny'])), pinned=True)
    assert sum(k.startswith('hist') and k.endswith('.W') for k in P0) == L


@pytest.mark.parametrize("enc", ['lf-ques', 'lf-ques-im-hist', 'mn-att-ques-im-hist', 'hre-ques-im-hist', 'hrea-ques-im-hist'])
def test_native_gen_retrieval_matches_oracle(gpu, enc):
    """gen-decoder candidate ranking (model.lua:392-420, utils.computeLhood) through vd_model_retrieve / vd_model_ranks"""
    from visdial_amd.native import NativeModel
    kw = dict(imgNorm=1, dropout=0.5, numOptions=12, batchSize=2)
    if 'att' in enc:
        kw.update(imgFeatureSize=32, imgSpatialSize=3)
    p = derive(small_params(encoder=enc, decoder='gen', **kw))
    batch, _ = SyntheticDataloader(p, seed=31, num_threads=4).getTestBatch(1, p, 'val')
    batch['option_in'][0, 0, 1, 1:] = 0           # an EMPTY candidate scores log-likelihood 0
    batch['option_out'][0, 0, 1, :] = 0
    if batch['answer_ind'][0] == 2:
        batch['answer_ind'][0] = 1
    model = NativeModel(p, init_seed=3)
    model.training(False)
    gt_ranks = model.retrieveBatch(batch, useGt=True)
    N, O = batch['option_in'].shape[0] * batch['option_in'].shape[1], batch['option_in'].shape[2]
    dev = model.scores(N, O)
    assert np.isfinite(dev).all()
    P = {k: v.astype(np.float64) for k, v in model.get_parameters_dict().items()}
    ref = vo.retrieve(enc, 'gen', P, p, batch)
    assert np.abs(dev - ref).max() < 1e-4 * max(1.0, np.abs(ref).max())
    np.testing.assert_array_equal(gt_ranks, vo.compute_ranks(dev, batch['answer_ind'].reshape(-1) - 1))
    allr = model.retrieveBatch(batch, useGt=False)
    np.testing.assert_array_equal(allr, vo.compute_ranks(dev))
    model.close()


@pytest.mark.parametrize("enc,dec", [('lf-ques-im-hist', 'gen'), ('hre-ques-im-hist', 'disc'), ('mn-ques-im-hist', 'gen')])
def test_native_pairs_train(gpu, enc, dec):
    """pipelined trainIteration (upload of the next batch overlapped) on a fixed batch: the loss must fall"""
    from visdial_amd.native import NativeModel
    p = derive(small_params(encoder=enc, decoder=dec, **WIDE['tiny']))
    dl = SyntheticDataloader(p, seed=9)
    fixed = dl.getTrainBatch(p)
    dl.getTrainBatch = lambda params, **kw: fixed
    model = NativeModel(p)
    losses = [model.trainIteration(dl) for _ in range(60)]
    assert np.isfinite(losses).all() and losses[-1] < 0.7 * losses[0], (losses[0], losses[-1])
    model.close()


def test_native_full_size_step_matches_cpp_restatement(gpu):
    """The bench's own path at the bench's own size: BASELINE.json configs[3] (20 dialogs x 10 rounds x 100 options,
    14x14x512, V = 11322, H = 512), dropout on with pinned masks, through the MODEL-LEVEL ABI, against
    oracle/cpu_step.cpp (fp32 on the host cores).  Bounds as in test_full_size_step_matches_cpp_restatement."""
    from oracle import cpu_step
    from visdial_amd.native import NativeModel
    from visdial_amd.opts import default_params
    p = default_params(encoder='mn-att-ques-im-hist', decoder='disc', imgFeatureSize=512, imgSpatialSize=14,
                       batchSize=20, vocabSize=11322, gpuid=0, maxHistoryLenPerRound=40)
    batch = SyntheticDataloader(p, seed=4321, fast=True).getTrainBatch(p)
    model = NativeModel(p, init_seed=99)
    masks = make_masks(p, batch, np.random.RandomState(6))
    model.set_dropout_masks(masks)
    P0 = model.get_parameters_dict()
    loss = model.forwardBackward(batch)
    g = model.get_gradients_dict()
    N, O = batch['options'].shape[0], batch['options'].shape[1]
    scores = model.scores(N, O)
    cs = cpu_step.CpuStep(p, vo.param_spec(p['encoder'], p['decoder'], p), P0)
    ref_loss, ref_scores = cs.step(batch, masks, want_scores=True)
    G = cs.named(cs.G)
    assert abs(loss - ref_loss) < 1e-4, (loss, ref_loss)
    assert rel(scores, ref_scores) < 1e-4
    bad = grad_mismatches(g, G, tol=5e-4, zero=('att.b',))   # two fp32 computations of different summation order;
    # 'att.b' shifts every logit of a softmax: its exact gradient is 0 and both sides hold fp32 rounding noise
    assert not bad, bad
    gt = batch['answer_ind'].reshape(-1) - 1
    flipped, unexplained = unexplained_rank_flips(scores, ref_scores)     # both fp32: only near ties may differ
    assert not unexplained, unexplained[:10]
    assert (vo.compute_ranks(scores, gt) != vo.compute_ranks(ref_scores, gt)).sum() <= flipped
    # one Adam step on both sides, then the parameters
    model.update()
    cs.step(batch, masks, update=True, lr=p['learningRate'])
    W1, W2 = model.get_parameters_dict(), cs.named(cs.W)
    settled = {k: np.abs(G[k]) > 1e-6 for k in G}          # Adam's first step is ~lr*sign(g): skip entries at the noise floor
    for k in W1:
        d = np.abs(W1[k].reshape(-1) - W2[k].reshape(-1))[settled[k].reshape(-1)]
        assert d.size == 0 or d.max() < 2e-6, (k, float(d.max()))
    model.close()


@pytest.mark.parametrize("train_mode", [False, True])
def test_native_ragged_empty_and_max_length_inputs(gpu, train_mode):
    """edge cases of the batch contract through the model-level ABI (its own host-side length sort and uploads):
    pad-only questions / history rounds / options, a dialog of empty questions, full-length rows, ties, collisions"""
    from test_model_gpu import _make_ragged
    from visdial_amd.native import NativeModel
    p = derive(small_params(**CASES['odd']))
    batch = _make_ragged(SyntheticDataloader(p, seed=23).getTrainBatch(p), p, np.random.RandomState(3))
    model = NativeModel(p, init_seed=8)
    masks = None
    if train_mode:
        masks = make_masks(p, batch, np.random.RandomState(9))
        model.set_dropout_masks(masks)
    else:
        model.training(False)
    P0 = {k: v.astype(np.float64) for k, v in model.get_parameters_dict().items()}
    loss = model.forwardBackward(batch)
    drop = {k: v.astype(np.float64) for k, v in masks.items()} if masks else None
    ref = vo.forward_backward(p['encoder'], p['decoder'], P0, p, batch, drop)
    assert np.isfinite(loss) and abs(loss - ref['loss']) < 1e-4
    g = model.get_gradients_dict()
    bad = grad_mismatches(g, ref['grads'])
    assert not bad, bad
    N, O = batch['options'].shape[0], batch['options'].shape[1]
    dev = model.scores(N, O)
    assert rel(dev, ref['scores']) < 1e-4
    ranks = model.retrieveBatch(batch, useGt=False) if not train_mode else None
    if ranks is not None:        # ties (identical options) resolve like utils.computeRanks: lower index first
        np.testing.assert_array_equal(ranks, vo.compute_ranks(model.scores(N, O)))
    model.close()


@pytest.mark.parametrize("config", ['1', '2', '2-split9', '4-bf16'])
def test_native_full_size_other_configs_are_additive_over_dialogs(gpu, config):
    """BASELINE.json configs[1] (lf-ques-im-hist + gen, fc7 4096-d features, batch 20, concatenated history up to 300
    steps), configs[2] (hre-ques-im-hist + disc, batch 20 x 10 rounds x 100 options) and configs[4] (mn-att-ques-im-hist + disc on 7x7x2048
    features with the bf16 pass) at their FULL sizes through the model-level ABI -- in the arithmetic x host x size `bench.py` times them:
    '2-split9' = configs[2] with its option recurrence on the exact split (bench.py config_params(2)), '4-bf16' = configs[4] with the COMPACT
    bf16 state of the native runtime (vd_lstm_forward_c16 / _backward_c16 at 20 000 option rows).  The oracle is too slow there, so the step
    is checked through the size-independent property data parallelism relies on: dialogs are independent, hence loss and every gradient of
    the 20-dialog batch equal the sum (gen: summed NLL) / the mean (disc: mean cross-entropy) over its two 10-dialog halves.  For the bf16
    pass the identity holds to ~1e-3 only: the 10 000-row and 20 000-row recurrences can differ in the last bit of an fp32 state, which can
    flip the bf16 rounding of an operand (tests/test_model_gpu.py::test_full_size_step_is_additive_over_dialogs)."""
    from visdial_amd.native import NativeModel
    from visdial_amd.opts import default_params
    cfg = int(config[0])
    kw = {1: dict(encoder='lf-ques-im-hist', decoder='gen', imgFeatureSize=4096),
          2: dict(encoder='hre-ques-im-hist', decoder='disc', imgFeatureSize=4096),
          4: dict(encoder='mn-att-ques-im-hist', decoder='disc', imgFeatureSize=2048, imgSpatialSize=7)}[cfg]
    kw['lstmPrecision'] = config.split('-')[1] if '-' in config else 'fp32'        # ('2' pins the fp32-MFMA recurrence: split9 is the library default)
    p = default_params(batchSize=20, vocabSize=11322, gpuid=0, maxHistoryLenPerRound=40, **kw)
    full = SyntheticDataloader(p, seed=77, fast=True).getTrainBatch(p)
    if cfg == 1:
        assert full["hist"].shape[2] >= 150           # the concatenated-history recurrence really is long

    def part(lo, hi):
        out = {}
        for k, v in full.items():
            rows = v.shape[0] // 20                   # leading dim is dialogs (B) or rounds (B*R)
            out[k] = v[lo * rows:hi * rows]
        return out
    model = NativeModel(p, init_seed=3)
    model.training(False)                             # no dropout noise: the three runs must see the same function
    names = [t[0] for t in model.tensors]
    out = []
    for lo, hi in ((0, 20), (0, 10), (10, 20)):
        loss = model.forwardBackward(part(lo, hi))
        g = model.get_gradients_dict()
        out.append((loss, np.concatenate([g[k].reshape(-1) for k in names]).astype(np.float64)))
        if p['decoder'] == 'disc':
            assert model.option_rows()[0] == (hi - lo) * p['maxQuesCount'] * p['numOptions']     # every option row ran (no accidental dedup)
    (lf, gf), (l1, g1), (l2, g2) = out
    w = 1.0 if cfg == 1 else 0.5
    tol_l, tol_g = (2e-4, 2e-3) if config == '4-bf16' else (2e-5, 1e-4)
    assert np.isfinite(lf) and abs(lf - w * (l1 + l2)) < tol_l * max(1.0, abs(lf)), (lf, l1, l2)
    gm = w * (g1 + g2)
    err = float(np.linalg.norm(gf - gm) / np.linalg.norm(gm))
    print("full-size additivity %s: dloss %.2e, gradient rel-L2 %.2e" % (config, abs(lf - w * (l1 + l2)), err))
    assert err < tol_g, err
    model.close()


def test_native_configs0_lf_ques_gen_at_batch_8_matches_oracle(gpu):
    """BASELINE.json configs[0] AS WRITTEN -- `-encoder lf-ques -decoder gen`, batch 8, the reference's default sizes (H = 512, E = 300,
    two LSTM layers, V = 11 322; train.lua:22-24, opts.lua) -- on the HIP path (there is deliberately no CPU product path) against the
    fp64 oracle: loss (summed NLL over answer tokens) and every gradient tensor within 1e-4; then three trainIteration steps follow
    the oracle's clamp + Adam."""
    from visdial_amd.native import NativeModel
    from visdial_amd.opts import default_params
    p = derive(default_params(encoder='lf-ques', decoder='gen', batchSize=8, vocabSize=11322, gpuid=0))
    batch = SyntheticDataloader(p, seed=8, fast=True).getTrainBatch(p)
    assert batch['ques_fwd'].shape[0] == 8 and 'img_feat' not in batch
    model = NativeModel(p, init_seed=4)
    model.training(False)
    P0 = {k: v.astype(np.float64) for k, v in model.get_parameters_dict().items()}
    loss = model.forwardBackward(batch)
    ref = vo.forward_backward('lf-ques', 'gen', P0, p, batch, None)
    assert abs(loss - ref['loss']) < 1e-4 * max(1.0, abs(ref['loss'])), (loss, ref['loss'])
    g = model.get_gradients_dict()
    bad = grad_mismatches(g, ref['grads'])
    assert not bad, bad
    model.update()
    after = model.get_parameters_dict()
    for k in P0:
        w2, _ = vo.clamp_adam(P0[k].reshape(-1), g[k].astype(np.float64).reshape(-1), {}, p['learningRate'])
        assert np.abs(after[k].reshape(-1) - w2).max() < 1e-6, k
    model.close()


@pytest.mark.parametrize("enc,dec", [('lf-ques-im-hist', 'gen'), ('mn-att-ques-im-hist', 'disc')])
def test_native_evaluate_equals_python_host(gpu, enc, dec):
    """Model:evaluate (model.lua:109-139) over a split through the model-level ABI = the operator-level host's, same
    parameters, same batches (two loaders with the same seed)"""
    from visdial_amd.model import Model
    from visdial_amd.native import NativeModel
    kw = dict(WIDE['tiny'])
    if 'att' in enc:
        kw.update(imgFeatureSize=32, imgSpatialSize=3)
    p = derive(small_params(encoder=enc, decoder=dec, **kw))
    py = Model(p)
    nat = NativeModel(p)
    nat.set_parameters_dict(py.get_parameters_dict())
    l1, ppl1 = py.evaluate(SyntheticDataloader(p, seed=5, num_threads=5), 'val')
    l2, ppl2 = nat.evaluate(SyntheticDataloader(p, seed=5, num_threads=5), 'val')
    assert np.isfinite(l1) and abs(l1 - l2) < 1e-5 * max(1.0, abs(l1)) and abs(ppl1 - ppl2) < 1e-4 * max(1.0, ppl1)
    nat.close()


@pytest.mark.parametrize("enc", ['lf-ques-im-hist', 'mn-ques-hist', 'hre-ques-im-hist'])
def test_native_beam_search_matches_oracle(gpu, enc):
    """Model:generateAnswers (model.lua:432-613) through vd_model_encode / decode_begin / decode_step / decode_select on a
    tiny real-format dataset: beam-search token sequences equal the fp64 oracle's and the operator-level host's;
    sampling with the same seed gives the same sentences as the operator-level host."""
    from test_dataloader_cpu import raw_dataset
    from visdial_amd import utils
    from visdial_amd.dataloader import Dataloader
    from visdial_amd.model import Model
    from visdial_amd.native import NativeModel
    from visdial_amd.opts import default_params
    rng = np.random.RandomState(2)
    info, raw, img = raw_dataset(rng, n=3, R=3, MQ=5, MA=4, V=20, O=4, nopt=12, F=8)
    raw = {k.replace('_train', '_val'): v for k, v in raw.items()}
    img = {k.replace('_train', '_val'): v for k, v in img.items()}
    info['unique_img_val'] = info.pop('unique_img_train')
    p = derive(default_params(encoder=enc, decoder='gen', embedSize=12, rnnHiddenSize=32, imgFeatureSize=8, imgEmbedSize=8,
                              numLayers=2, batchSize=1, learningRate=1e-3, gpuid=0))
    dl = Dataloader(seed=1).from_arrays(info, raw, img, p, ['val'])
    for k in ('vocabSize', 'maxQuesCount', 'maxQuesLen', 'maxAnsLen'):
        p[k] = getattr(dl, k)
    nat = NativeModel(p, init_seed=4)
    py = Model(p)
    py.set_parameters_dict(nat.get_parameters_dict())
    cfg = dict(beamSize=3, beamLen=6, maxThreads=2)
    out = nat.generateAnswers(dl, 'val', cfg)
    assert out == py.generateAnswers(dl, 'val', cfg)
    P = {k: v.astype(np.float64) for k, v in nat.get_parameters_dict().items()}
    START, END = dl.word2ind['<START>'], dl.word2ind['<END>']
    for conv in (1, 2):
        batch = dl.getIndexData(np.array([conv]), p, 'val')
        ref = vo.generate_beam(enc, P, p, batch, 3, 6, START, END)
        for it, (beam, score) in enumerate(ref):
            assert out[conv - 1]['dialog'][it]['answer'] == utils.idToWords(beam, dl.ind2word), (conv, it)
    smp = dict(sampleWords=1, temperature=0.7, beamLen=5, maxThreads=2, seed=7)
    a, b = nat.generateAnswers(dl, 'val', smp), py.generateAnswers(dl, 'val', smp)
    assert a == b and all(x['answer'].startswith(' <START>') for x in a[0]['dialog'])
    nat.close()


@pytest.mark.parametrize("enc,dec", [('lf-ques-im-hist', 'gen'), ('mn-att-ques-im-hist', 'disc')])
def test_running_loss_is_the_same_through_both_hosts(gpu, enc, dec):
    """model.lua:73-93: the loss EMA is fed curLoss / numTokens for gen (the criterion SUMS over tokens) and curLoss for
    disc.  Same parameters, same dataloader stream, dropout off: the two hosts must log the same `[Loss:...]`."""
    from visdial_amd.model import Model
    from visdial_amd.native import NativeModel
    p = derive(small_params(encoder=enc, decoder=dec, **CASES['tiny']))
    py, nat = Model(dict(p)), NativeModel(dict(p))
    nat.set_parameters_dict(py.get_parameters_dict())
    py.wrapper.evaluate()
    nat.training(False)
    d1, d2 = SyntheticDataloader(p, seed=21), SyntheticDataloader(p, seed=21)
    cur = []
    for _ in range(3):
        a, b = py.trainIteration(d1), nat.trainIteration(d2)
        assert abs(a - b) < 1e-4 * max(1.0, abs(a)), (a, b)          # curLoss itself (gen: the un-normalised sum)
        cur.append(a)
    assert py.runningLoss > 0 and abs(py.runningLoss - nat.runningLoss) < 1e-5 * max(1.0, py.runningLoss)
    if dec == 'gen':      # the EMA is per token: far below the summed NLL the criterion returns
        assert nat.runningLoss < 0.2 * min(cur)
    nat.close()


def test_retrieve_between_training_steps_does_not_train_on_the_eval_batch(gpu):
    """trainIteration prefetches the next training batch into the library's second slot; evaluate / retrieve / predict
    between two steps replace it.  The next trainIteration must notice and fetch a training batch again (lua/model.lua:
    havePrefetched = false on those paths) -- same parameters as the Python host after the same interleaving."""
    from visdial_amd.model import Model
    from visdial_amd.native import NativeModel
    p = derive(small_params(**CASES['tiny']))
    py, nat = Model(dict(p)), NativeModel(dict(p))
    nat.set_parameters_dict(py.get_parameters_dict())
    py.wrapper.evaluate()
    nat.training(False)
    d1, d2 = SyntheticDataloader(p, seed=5), SyntheticDataloader(p, seed=5)
    val = SyntheticDataloader(p, seed=77).getTrainBatch(p)
    for it in range(4):
        a, b = py.trainIteration(d1), nat.trainIteration(d2)
        assert abs(a - b) < 1e-4, (it, a, b)
        if it % 2 == 0:
            py.params['useGt'] = True
            r1, r2 = py.retrieveBatch(val), nat.retrieveBatch(val, useGt=True)
            r1 = r1.cpu().numpy() if hasattr(r1, 'cpu') else np.asarray(r1)
            np.testing.assert_array_equal(r1.reshape(-1), np.asarray(r2).reshape(-1))
    w1, w2 = py.get_parameters_dict(), nat.get_parameters_dict()
    for k in w1:
        if k == 'att.b':        # true gradient 0 (softmax shift invariance): both hosts feed fp32 rounding noise through Adam's normalisation
            continue
        assert np.abs(w1[k] - w2[k]).max() < 2e-5, k
    nat.close()


@pytest.mark.parametrize("host", ['native', 'python'])
def test_duplicate_options_are_encoded_once_and_exactly(gpu, host):
    """decoders/disc.lua:4-15: an option's encoding depends on its tokens only, and on real VisDial the 100 candidates of
    a round repeat across the rounds of a batch.  Both hosts encode every DISTINCT candidate row once (forward gather,
    backward scatter-add of the copies' gradients).  The oracle encodes all N*O rows: loss, scores, every gradient and the
    post-Adam parameters must still match (duplicates share one forward value; their gradients add)."""
    p = derive(small_params(**CASES['odd']))
    batch = SyntheticDataloader(p, seed=17).getTrainBatch(p)
    B, R = batch['ques_fwd'].shape[:2]
    O = batch['options'].shape[1]
    opts = batch['options'].reshape(B, R, O, -1).copy()
    opts[:, 1:] = opts[:, :1]                        # every round of a dialog offers the same candidates
    opts[:, :, O - 1] = opts[:, :, 0]                # ... and one candidate appears twice inside a round
    batch['options'] = opts.reshape(B * R, O, -1)
    total = B * R * O
    distinct = len({r.tobytes() for r in batch['options'].reshape(total, -1)})
    assert distinct <= 0.5 * total
    if host == 'native':
        from visdial_amd.native import NativeModel
        model = NativeModel(p, init_seed=5)
        model.training(False)
    else:
        from visdial_amd.model import Model
        model = Model(p)
        model.wrapper.evaluate()
        model.wrapper.zeroGradParameters()
    P0 = {k: v.astype(np.float64) for k, v in model.get_parameters_dict().items()}
    loss = model.forwardBackward(batch)
    if host == 'native':
        assert model.option_rows() == (distinct, total)
        scores = model.scores(B * R, O)
    else:
        assert model.decoder.NO == distinct
        scores = model.decoder.output.cpu().numpy()
    ref = vo.forward_backward(p['encoder'], p['decoder'], P0, p, batch, None)
    assert abs(loss - ref['loss']) < 1e-4
    assert rel(scores, ref['scores']) < 1e-4
    # identical candidates get identical scores, bit for bit
    s3 = scores.reshape(B * R, O)
    np.testing.assert_array_equal(s3[:, O - 1], s3[:, 0])
    bad = grad_mismatches(model.get_gradients_dict(), ref['grads'])
    assert not bad, bad
    if host == 'native':
        model.close()


def test_native_split9_throughput_shape_matches_oracle(gpu):
    """The headline's arithmetic through the model-level runtime at a shape that takes every split9 kernel but is small enough for the fp64
    oracle: 3 000 option rows (>= 2 048: the LDS-DMA step kernels on the exact 3 x bf16 split of both operands), H = 256 and K = 19 x 3 000 rows
    = 16 x 3 562 + 8 for the weight-gradient contraction (gemm_split_tn_kernel<9> + the ragged tail on the fp32 MFMA); the image attention's
    three dense products on the split too (csrc/attention.hip vd_img_*_p: 30 rounds x 36 regions = 1 080 rows = 16 x 67 + 8, K = Kc = H = 256).
    fp32-grade: loss, scores and every gradient within the fp32 tolerance of the other native tests, the recurrent weight gradient to 2e-6."""
    from visdial_amd.native import NativeModel
    kw = dict(vocabSize=300, embedSize=64, rnnHiddenSize=256, imgFeatureSize=64, imgSpatialSize=6, commonEmbeddingSize=256, maxQuesCount=10,
              batchSize=3, numOptions=100, maxQuesLen=8, maxAnsLen=20, maxHistoryLenPerRound=12)
    p = derive(small_params(lstmPrecision='split9', **kw))
    batch = SyntheticDataloader(p, seed=43).getTrainBatch(p)
    model = NativeModel(p, init_seed=6)
    model.training(False)
    P0 = {k: v.astype(np.float64) for k, v in model.get_parameters_dict().items()}
    loss = model.forwardBackward(batch)
    g = model.get_gradients_dict()
    N, O = batch['options'].shape[0], batch['options'].shape[1]
    assert model.option_rows() == (N * O, N * O) and N * O >= 2048
    scores = model.scores(N, O)
    ref = vo.forward_backward(p['encoder'], p['decoder'], P0, p, batch, None)
    assert abs(loss - ref['loss']) < 1e-4 and rel(scores, ref['scores']) < 1e-4
    bad = grad_mismatches(g, ref['grads'])
    assert not bad, bad
    print("split9 at 3 000 rows: dloss %.2e, opt.W gradient rel-L2 %.2e" % (abs(loss - ref['loss']), rel(g['opt.W'], ref['grads']['opt.W'])))
    assert rel(g['opt.W'], ref['grads']['opt.W']) < 2e-6      # the recurrent weight gradient is fp32-grade, not merely inside 1e-4
    model.close()


@pytest.mark.parametrize("size", ['h128', 'h512', 'h128-rows9000'])
def test_native_bf16_compact_state_within_the_stated_bound(gpu, size):
    """BASELINE.json configs[4] through the model-level runtime: bf16 operands AND compact bf16 state in the option recurrence (saved
    gates / da, projection-table rows and h as bf16, c and the last state fp32 -- csrc/common.h `vd_lstm_forward_c16`).  The config's own
    stated bound (tests/test_model_gpu.py::test_bf16_option_lstm_step): |loss diff| < 1e-3, score rel-L2 < 1e-2, gradient rel-L2 < 2e-2
    per tensor, >= 90 % of the ground-truth ranks identical to the fp64 oracle's."""
    from visdial_amd.native import NativeModel
    kw = dict(vocabSize=300, embedSize=64, rnnHiddenSize=128, imgFeatureSize=2048, imgSpatialSize=7,
              commonEmbeddingSize=128, maxQuesCount=10, batchSize=3, numOptions=100, maxQuesLen=10, maxAnsLen=20)
    if size == 'h512':
        kw.update(embedSize=300, rnnHiddenSize=512, commonEmbeddingSize=512, maxQuesLen=20, maxHistoryLenPerRound=40)
    if size == 'h128-rows9000':
        kw.update(batchSize=9)                                   # 9 000 option rows (71 row tiles of 128: several rounds of workgroups, ragged last tile)
    p = derive(small_params(lstmPrecision='bf16', **kw))         # N * O = 3000 rows (9000): the throughput kernels run
    batch = SyntheticDataloader(p, seed=41).getTrainBatch(p)
    model = NativeModel(p, init_seed=2)
    model.training(False)
    P0 = {k: v.astype(np.float64) for k, v in model.get_parameters_dict().items()}
    loss = model.forwardBackward(batch)
    g = model.get_gradients_dict()
    N, O = batch['options'].shape[0], batch['options'].shape[1]
    scores = model.scores(N, O)
    ref = vo.forward_backward(p['encoder'], p['decoder'], P0, p, batch, None)
    errs = {k: rel(g[k], ref['grads'][k]) for k in ref['grads'] if np.abs(ref['grads'][k]).max() > 1e-6}
    agree = (vo.compute_ranks(scores, batch['answer_ind'] - 1) == vo.compute_ranks(ref['scores'], batch['answer_ind'] - 1)).mean()
    print("bf16 compact state (dloss, score rel, max grad rel, rank agreement):", abs(loss - ref['loss']), rel(scores, ref['scores']),
          max(errs.items(), key=lambda kv: kv[1]), agree)
    assert abs(loss - ref['loss']) < 1e-3 and rel(scores, ref['scores']) < 1e-2 and max(errs.values()) < 2e-2 and agree >= 0.9
    assert rel(scores, ref['scores']) > 1e-5          # the switch really changes the arithmetic
    model.close()
