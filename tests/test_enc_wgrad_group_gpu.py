"""The encoder LSTMs' weight gradients through the grouped live-row launch (csrc/gemm_core.h gemm_block_glds_live, rt_core.h wgrad_flush)
against the fp64 oracle: one step of forward + backward through NativeModel, dropout off, `grad.<lstm>.W` and `.b` of every encoder LSTM.

Which products take the new launch is decided by paths.h vd_wgrad_group_fits: the LSTM runs on a LENGTH-SORTED sequence set (the text stacks
of the nngraph encoders, the two-layer history branch of the Sequential ones), M and N of C [M x N] are multiples of the 128 x 128 tile, and
the pass is not bf16.  At H = 128, E = 64 that is both layers' dWh [128 x 512] and the layer-2 dWx [128 x 512] of each sorted stack (six
products in one launch for mn-att-ques-im-hist, three for the history branch of lf-ques-im-hist); the layer-1 dWx (M = E = 64), the bias
sums, H = 96 and lstmPrecision = 'bf16' keep the old kernels, and so do the unsorted question layers of lf-ques-im-hist.  The disc step
flushes the launch behind its option recurrence, the gen step at the end of the encoder backward: both placements run here.

Shape: batch 4 x 10 rounds = N = 40 rows per step (N % 16 = 8: a step with more than 32 live rows ends in a SHORT k-step of 8 rows), history
24 wide, questions 12 wide.  Batch 'full' holds rows of length 1 and of full length; batch 'short' holds no full-length row, so its leading
steps have no live row at all.

Bound per tensor: TWICE the deviation of the parent commit's library from the same oracle on the same inputs, the largest of 10 repetitions
(a step's figure moves from run to run with the order of its float atomics), measured once on an MI355X with the parent library loaded
through VD_LIB_PATH: PARENT_DEV below, printed by running this file as a script.  (tests/test_side_lane_gpu.py states its bounds the same way.)
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

# case: (encoder, decoder, rnnHiddenSize, lstmPrecision, batch)
CASES = {
    'mn-att-disc/full': ('mn-att-ques-im-hist', 'disc', 128, 'split9', 'full'),
    'mn-att-disc/short': ('mn-att-ques-im-hist', 'disc', 128, 'split9', 'short'),
    'lf-gen/full': ('lf-ques-im-hist', 'gen', 128, 'split9', 'full'),
    'lf-gen/short': ('lf-ques-im-hist', 'gen', 128, 'split9', 'short'),
    'mn-att-disc/H96': ('mn-att-ques-im-hist', 'disc', 96, 'split9', 'full'),        # ineligible: old path
    'mn-att-disc/bf16': ('mn-att-ques-im-hist', 'disc', 128, 'bf16', 'full'),      # ineligible: old path
}
LSTMS = ('hist1', 'hist2', 'ques1', 'ques2')
TH, TQ = 24, 12

# relative L2 deviation of the PARENT library's gradients from the fp64 oracle, largest of 10 repetitions (see the module docstring)
PARENT_DEV = {
    'mn-att-disc/full': {'hist1.W': 5.392e-07, 'hist1.b': 2.683e-07, 'hist2.W': 5.061e-07, 'hist2.b': 2.450e-07, 'ques1.W': 4.375e-07,
                         'ques1.b': 2.891e-07, 'ques2.W': 4.399e-07, 'ques2.b': 2.468e-07},
    'mn-att-disc/short': {'hist1.W': 4.545e-07, 'hist1.b': 2.694e-07, 'hist2.W': 4.671e-07, 'hist2.b': 2.744e-07, 'ques1.W': 4.023e-07,
                          'ques1.b': 3.503e-07, 'ques2.W': 3.886e-07, 'ques2.b': 2.582e-07},
    'lf-gen/full': {'hist1.W': 5.384e-07, 'hist1.b': 1.705e-07, 'hist2.W': 5.066e-07, 'hist2.b': 1.766e-07, 'ques1.W': 3.810e-07,
                    'ques1.b': 1.463e-07, 'ques2.W': 3.561e-07, 'ques2.b': 1.431e-07},
    'lf-gen/short': {'hist1.W': 4.837e-07, 'hist1.b': 1.957e-07, 'hist2.W': 4.866e-07, 'hist2.b': 2.050e-07, 'ques1.W': 3.493e-07,
                     'ques1.b': 1.379e-07, 'ques2.W': 3.145e-07, 'ques2.b': 1.414e-07},
    'mn-att-disc/H96': {'hist1.W': 5.653e-07, 'hist1.b': 3.548e-07, 'hist2.W': 5.044e-07, 'hist2.b': 3.179e-07, 'ques1.W': 4.378e-07,
                        'ques1.b': 3.823e-07, 'ques2.W': 4.247e-07, 'ques2.b': 2.965e-07},
    'mn-att-disc/bf16': {'hist1.W': 2.602e-03, 'hist1.b': 2.198e-03, 'hist2.W': 1.942e-03, 'hist2.b': 8.848e-04, 'ques1.W': 2.379e-03,
                         'ques1.b': 2.553e-03, 'ques2.W': 1.437e-03, 'ques2.b': 9.017e-04},
}


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def case_params(case):
    from visdial_amd.opts import default_params
    enc, dec, H, prec, _ = CASES[case]
    return default_params(encoder=enc, decoder=dec, vocabSize=200, embedSize=64, rnnHiddenSize=H, commonEmbeddingSize=H, imgFeatureSize=32,
                          imgSpatialSize=3 if 'att' in enc else 1, imgEmbedSize=64, maxQuesCount=10, maxQuesLen=TQ, maxAnsLen=6,
                          maxHistoryLenPerRound=TH, maxHistoryLen=TH, numOptions=5, batchSize=4, seed=3, lstmPrecision=prec)


def right_aligned(lengths, width, V, rng):
    rows = np.zeros((len(lengths), width), np.int32)
    for r, n in enumerate(lengths):
        rows[r, width - n:] = rng.randint(1, V + 1, size=n)
    return rows


def case_batch(case, p):
    """a synthetic batch whose question and history rows get hand-set lengths, at the full widths TQ / TH"""
    from visdial_amd.dataloader import SyntheticDataloader
    kind = CASES[case][4]
    batch = SyntheticDataloader(p, seed=17).getTrainBatch(p)
    B, R = batch['ques_fwd'].shape[:2]
    N, V = B * R, p['vocabSize']
    assert N == 40 and N % 16 != 0
    rng = np.random.RandomState(41)
    if kind == 'full':      # lengths 1 and full width among the rows, every length class of a k-step boundary in between
        hl = np.array([1, TH, 1, TH, 2, 15, 16, 17, TH - 1] + list(rng.randint(1, TH + 1, size=N - 9)))
        ql = np.array([TQ, 1, TQ, 1, 2, TQ - 1] + list(rng.randint(1, TQ + 1, size=N - 6)))
    else:                   # no row of full length: steps [0, width - longest) have no live row
        hl = np.array([1, 17, 17, 2] + list(rng.randint(1, 18, size=N - 4)))
        ql = np.array([8, 1, 8] + list(rng.randint(1, 9, size=N - 3)))
    batch['hist'] = right_aligned(rng.permutation(hl), TH, V, rng).reshape(B, R, TH)
    batch['ques_fwd'] = right_aligned(rng.permutation(ql), TQ, V, rng).reshape(B, R, TQ)
    return batch


_shared = {}


def setup(case):
    """(params, batch, initial parameters, oracle gradients): computed once per case, shared, never modified"""
    if case not in _shared:
        from oracle import visdial_oracle as vo
        from visdial_amd.native import NativeModel
        p = case_params(case)
        batch = case_batch(case, p)
        model = NativeModel(dict(p), init_seed=5)
        P0 = model.get_parameters_dict()
        model.close()
        ref = vo.forward_backward(p['encoder'], p['decoder'], {k: v.astype(np.float64) for k, v in P0.items()}, p, batch, None)
        _shared[case] = (p, batch, P0, ref)
    return _shared[case]


def deviations(case, repetitions=1):
    """{tensor: largest relative L2 deviation from the oracle over `repetitions` steps on the same inputs}"""
    from visdial_amd.native import NativeModel
    p, batch, P0, ref = setup(case)
    model = NativeModel(dict(p), init_seed=5)
    model.set_parameters_dict(P0)
    model.training(False)
    out = {}
    for _ in range(repetitions):
        loss = model.forwardBackward(batch)
        assert np.isfinite(loss)
        g = model.get_gradients_dict()
        for name in LSTMS:
            for k in (name + '.W', name + '.b'):
                a, b = np.asarray(g[k], np.float64), np.asarray(ref['grads'][k], np.float64)
                assert float(np.linalg.norm(b)) > 0, k
                out[k] = max(out.get(k, 0.0), float(np.linalg.norm(a - b)) / float(np.linalg.norm(b)))
    model.close()
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_encoder_lstm_gradients_match_oracle_like_the_parent(gpu, case):
    dev = deviations(case)
    bound = PARENT_DEV[case]
    for k, v in dev.items():
        print("%-18s %-8s %.3e (bound %.3e)" % (case, k, v, 2 * bound[k]))
    assert sorted(dev) == sorted(bound), "tensors compared differ from the ones measured on the parent"
    bad = [(k, v, 2 * bound[k]) for k, v in dev.items() if not v <= 2 * bound[k]]
    assert not bad, bad


if __name__ == '__main__':      # the table: VD_LIB_PATH=<parent library> python tests/test_enc_wgrad_group_gpu.py
    print("PARENT_DEV = {")
    for case in CASES:
        dev = deviations(case, repetitions=10)
        print("    %r: {%s}," % (case, ', '.join("%r: %.3e" % kv for kv in sorted(dev.items()))))
    print("}")
