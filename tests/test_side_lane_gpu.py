"""The native runtime's two lanes (csrc/runtime.hip: s_main + ONE side stream for the encoder chains, image prefetch / history branch,
table-gradient chain and batch uploads): what can go wrong is a lost ordering edge between main and the side lane, slot reuse when the
host runs ahead, and teardown.  A lost edge only shows when kernels outlast their enqueue, so the shapes are just large enough for the
option recurrence to take the throughput kernels: 3 dialogs x 10 rounds x 100 options = 3 000 rows (paths.h VD_THROUGHPUT_ROWS = 2 048),
H = 128, To = 8, a 4 x 4 x 64 image map, pinned seeds.

Every comparison is "the same steps, scheduled differently": the two sides differ only in the order of float atomics (the shared embedding
gradient has concurrent writers, the attention's weight gradients are summed atomically), which Adam carries into the parameters.  Figures
are relative L2 differences per tensor (|a - b| / |b| for a loss).  The bound per tensor is TWICE the deviation the same comparison showed
on the library of the parent commit (four side streams), measured on an MI355X under GPU_MAX_HW_QUEUES=4 as the largest of 25
repetitions, PARENT_DEV below; `att.b` / `att2.b` ... are left out like bench.py's DUMP_SKIP does (their exact gradient is 0, what a step
computes for them is rounding noise).  A tensor the parent reproduced exactly must be reproduced exactly.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
SKIP = re.compile(r'att\d*\.b')            # bench.py DUMP_SKIP
CASES = {'mn-att-disc': ('mn-att-ques-im-hist', 'disc'),     # image prefetch, table-gradient chain
         'hre-disc': ('hre-ques-im-hist', 'disc'),           # history branch
         'lf-gen': ('lf-ques-im-hist', 'gen')}               # history branch off the main stream

# measured on the parent commit's library (see the module docstring): {comparison: {figure: largest deviation of 25 repetitions}}
PARENT_DEV = {
    'mn-att-disc': {'att.W': 3.16e-08, 'embed': 4.94e-09, 'hist1.W': 1.90e-08, 'hist1.b': 1.06e-08, 'hist2.W': 1.95e-08, 'hist2.b': 5.37e-09,
                    'img_common.W': 2.62e-08, 'img_common.b': 2.58e-08, 'img_proj.W': 3.22e-08, 'img_proj.b': 1.85e-08, 'loss0': 0.0, 'loss1': 1.02e-07,
                    'loss2': 1.02e-07, 'mn1.W': 2.09e-08, 'mn1.b': 2.52e-08, 'mn2.W': 2.30e-08, 'mn2.b': 2.53e-08, 'opt.W': 3.06e-08,
                    'opt.b': 5.83e-09, 'out.W': 2.11e-08, 'out.b': 2.23e-08, 'ques1.W': 1.81e-08, 'ques1.b': 1.29e-08, 'ques2.W': 1.86e-08,
                    'ques2.b': 5.35e-09, 'ques_common.W': 2.49e-08, 'ques_common.b': 2.79e-08},
    'hre-disc': {'dialog.W': 2.17e-08, 'dialog.b': 1.04e-09, 'embed': 5.07e-09, 'hist1.W': 1.69e-08, 'hist1.b': 5.31e-09, 'hist2.W': 1.75e-08,
                 'hist2.b': 7.48e-09, 'img_embed.W': 1.58e-08, 'img_embed.b': 2.32e-08, 'loss0': 0.0, 'loss1': 0.0, 'loss2': 0.0,
                 'opt.W': 2.44e-08, 'opt.b': 7.75e-09, 'ques1.W': 1.78e-08, 'ques1.b': 1.18e-08, 'ques2.W': 1.77e-08, 'ques2.b': 3.02e-09},
    'lf-gen': {'dec1.W': 1.30e-08, 'dec1.b': 5.28e-09, 'dec2.W': 1.51e-08, 'dec2.b': 5.28e-09, 'embed': 4.01e-09, 'fuse.W': 2.25e-08,
               'fuse.b': 2.78e-08, 'hist1.W': 1.89e-08, 'hist1.b': 1.18e-08, 'hist2.W': 1.87e-08, 'hist2.b': 1.06e-08, 'loss0': 0.0,
               'loss1': 0.0, 'loss2': 0.0, 'ques1.W': 1.46e-08, 'ques1.b': 1.06e-08, 'ques2.W': 1.45e-08, 'ques2.b': 1.05e-08,
               'vocab.W': 1.64e-08, 'vocab.b': 1.30e-08},
    'run-ahead': {'att.W': 3.87e-08, 'embed': 5.36e-09, 'hist1.W': 2.30e-08, 'hist1.b': 1.18e-08, 'hist2.W': 2.37e-08, 'hist2.b': 5.42e-09,
                  'img_common.W': 3.76e-08, 'img_common.b': 4.07e-08, 'img_proj.W': 2.44e-08, 'img_proj.b': 2.50e-08, 'loss0': 0.0, 'mn1.W': 2.63e-08,
                  'mn1.b': 3.93e-08, 'mn2.W': 2.72e-08, 'mn2.b': 2.86e-08, 'opt.W': 3.72e-08, 'opt.b': 1.94e-08, 'out.W': 2.14e-08,
                  'out.b': 2.17e-08, 'ques1.W': 2.20e-08, 'ques1.b': 1.53e-08, 'ques2.W': 2.32e-08, 'ques2.b': 1.83e-08, 'ques_common.W': 3.18e-08,
                  'ques_common.b': 4.75e-08},
}


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def case_params(case, streams):
    from visdial_amd.opts import default_params
    enc, dec = CASES[case]
    att = 'att' in enc
    return default_params(encoder=enc, decoder=dec, vocabSize=1000, embedSize=64, rnnHiddenSize=128, commonEmbeddingSize=128,
                          imgFeatureSize=64, imgSpatialSize=4 if att else 1, imgEmbedSize=64, maxQuesCount=10, maxQuesLen=12, maxAnsLen=8,
                          maxHistoryLenPerRound=16, maxHistoryLen=12, numOptions=100, batchSize=3, useStreams=int(streams), seed=77,
                          lstmPrecision='split9')


def figures(model, losses):
    out = {'loss%d' % i: np.array([v], np.float64) for i, v in enumerate(losses)}
    out.update({k: v for k, v in model.get_parameters_dict().items() if not SKIP.fullmatch(k)})
    return out


def train_iterations(case, streams, steps=3):
    """`steps` pipelined trainIterations (the loop bench.py times) -> {loss<i>, <parameter>: array}"""
    from visdial_amd.dataloader import SyntheticDataloader
    from visdial_amd.native import NativeModel
    p = case_params(case, streams)
    model = NativeModel(dict(p), init_seed=5)
    dl = SyntheticDataloader(p, seed=21, fast=True)
    losses = [model.trainIteration(dl) for _ in range(steps)]
    model.synchronize()
    out = figures(model, losses)
    model.close()
    return out


def low_level_steps(read_every_loss, steps=4):
    """`steps` x (vd_model_forward_backward, update, upload of the next batch) through the low-level calls on the first case, the loss read
    after every step or only after the last one (the host then runs ahead of the device as far as the two batch slots let it)"""
    from visdial_amd.dataloader import SyntheticDataloader
    from visdial_amd.native import NativeModel, call
    p = case_params('mn-att-disc', 1)
    model = NativeModel(dict(p), init_seed=5)
    dl = SyntheticDataloader(p, seed=33, fast=True)
    batches = [dl.getTrainBatch(p) for _ in range(steps + 1)]
    model.upload(batches[0])
    losses = []
    for i in range(steps):
        call("vd_model_forward_backward", model.h, 0)
        model.update()
        model.upload(batches[i + 1])
        if read_every_loss or i == steps - 1:
            losses.append(model.loss())
    model.synchronize()
    out = figures(model, losses[-1:])
    model.close()
    return out


def deviations(got, ref):
    """{figure: relative L2 difference}"""
    out = {}
    for k in sorted(ref):
        a, b = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64)
        out[k] = float(np.linalg.norm(a - b)) / max(float(np.linalg.norm(b)), 1e-30)
    return out


def check(comparison, got, ref):
    dev = deviations(got, ref)
    bound = PARENT_DEV[comparison]
    for k, v in dev.items():
        print("%-14s %-18s %.3e (bound %.3e)" % (comparison, k, v, 2 * bound[k]))
    assert sorted(dev) == sorted(bound), "figures compared differ from the ones measured on the parent"
    bad = [(k, v, 2 * bound[k]) for k, v in dev.items() if not v <= 2 * bound[k]]
    assert not bad, bad


_serial = {}


def serial_reference(case):
    """the whole step on the main stream (useStreams = 0): computed once per case, shared, never modified"""
    if case not in _serial:
        _serial[case] = train_iterations(case, 0)
    return _serial[case]


@pytest.mark.parametrize("case", list(CASES))
def test_overlapped_equals_serial(gpu, case):
    check(case, train_iterations(case, 1), serial_reference(case))


def test_run_ahead_equals_step_by_step(gpu):
    """slot reuse: four steps enqueued without reading a loss == the same four steps with the loss read after each"""
    check('run-ahead', low_level_steps(False), low_level_steps(True))


def test_same_result_at_any_queue_count(gpu, tmp_path):
    """the first case in fresh processes under GPU_MAX_HW_QUEUES = 1, 4 and unset: each equals the serial reference"""
    ref = serial_reference('mn-att-disc')
    for queues in ('1', '4', None):
        env = dict(os.environ)
        env.pop('GPU_MAX_HW_QUEUES', None)
        if queues is not None:
            env['GPU_MAX_HW_QUEUES'] = queues
        out = str(tmp_path / ('q%s.npz' % queues))
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, timeout=120).returncode
        except subprocess.TimeoutExpired:
            pytest.fail("GPU_MAX_HW_QUEUES=%s: the child did not finish in 120 s; nothing more was started" % queues)
        if rc < 0:
            pytest.fail("GPU_MAX_HW_QUEUES=%s: the child died by signal %d; nothing more was started" % (queues, -rc))
        assert rc == 0, "GPU_MAX_HW_QUEUES=%s: the child exited with %d" % (queues, rc)
        with np.load(out) as z:
            check('mn-att-disc', {k: z[k] for k in z.files}, ref)


@pytest.mark.parametrize("streams", [0, 1])
def test_create_step_destroy_three_times(gpu, streams):
    """teardown and vd_model_synchronize walk the stream list: every call returns VD_OK (visdial_amd._lib.call raises otherwise)"""
    from visdial_amd import _lib
    from visdial_amd.dataloader import SyntheticDataloader
    from visdial_amd.native import NativeModel
    p = case_params('mn-att-disc', streams)
    batch = SyntheticDataloader(p, seed=9, fast=True).getTrainBatch(p)
    for _ in range(3):
        model = NativeModel(dict(p), init_seed=5)
        loss = model.forwardBackward(batch)
        model.update()
        _lib.call("vd_model_synchronize", model.h)
        assert np.isfinite(loss)
        model.close()
        assert model.h is None


if __name__ == '__main__':      # the child of test_same_result_at_any_queue_count
    np.savez(sys.argv[1], **train_iterations('mn-att-disc', 1))
