"""The image attention over a region count per image (vd_model_set_tensor '@img_regions'; csrc/attention.hip IR1-IR6) at the size of VisDial
v1.0 detector features through the native host: mn-att-ques-im-hist + disc, 20 dialogs x 10 rounds x 100 options (N = 200 rounds), M = 100
regions per image at most (S = 10, S2 = 100), C = 2048, H = K = 512, split9, random weights, one synthetic batch uploaded once per path.

  --mode step (default): the training step (vd_model_forward_backward(m, 0) + vd_model_loss; no update) on
      plain      no attachment: the four head kernels with a null cnt
      full       '@img_regions' with every count = 100: the same kernels with counts, over every region
      mixed      counts uniform in 10 .. 100 (fixed seed; the hidden rows of the features zero): the same kernels over 55 % of the rows
    alternated in one process after warm-up; per path the median step time over --repeats windows of --inner steps with min / max.
    --paths plain runs the first alone (a library that does not know the attachment -- the parent commit's, through VD_LIB_PATH);
    --tag NAME marks the process's lines for an A/B of two libraries, processes alternated by the caller.
  --mode trace: --inner steps of every path after a warm-up, nothing timed: run it under `rocprofv3 --kernel-trace --stats` for the times of
      img_att_{score,wsum,dscore,dz}_kernel with and without counts (one kernel each: the paths are told apart by their order in the
      trace; a library from before the fold shows the counted launches under _regions names), and for the share of the three dense image products
      (EpiImgCommon, EpiImgTrBwd, the TN weight gradient) in the step.

    python scripts/mb_regions.py [--mode step|trace] [--repeats 15] [--inner 5] [--paths all|plain,full,mixed] [--tag NAME]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from visdial_amd.dataloader import SyntheticDataloader, pad_regions  # noqa: E402
from visdial_amd.native import NativeModel  # noqa: E402
from visdial_amd.opts import default_params, derive  # noqa: E402

ap = argparse.ArgumentParser(description='the masked image attention at 20 x 10 x 100, M = 100, C = 2048')
ap.add_argument('--mode', choices=('step', 'trace'), default='step')
ap.add_argument('--repeats', type=int, default=15)
ap.add_argument('--inner', type=int, default=5, help='steps per timed window')
ap.add_argument('--paths', default='all', help="'all' or a comma-separated list of plain, full, mixed")
ap.add_argument('--tag', default='')
opt = ap.parse_args()

B, R, O, To, M, S, C = 20, 10, 100, 20, 100, 10, 2048


def params():
    return derive(default_params(encoder='mn-att-ques-im-hist', decoder='disc', vocabSize=11322, imgFeatureSize=C, imgSpatialSize=S,
                                 maxHistoryLenPerRound=40, batchSize=B, numOptions=O, maxQuesCount=R, maxAnsLen=To, lstmPrecision='split9',
                                 gpuid=0))


def counts(path):
    if path == 'plain':
        return None
    return np.full(B, M, np.int32) if path == 'full' else np.random.RandomState(3).randint(10, M + 1, size=B).astype(np.int32)


def make(path, batch):
    m = NativeModel(params())
    cnt = counts(path)
    if path == 'mixed':                                             # what a loader hands over: zeros behind the count (IR5)
        batch = dict(batch, img_feat=pad_regions(batch['img_feat'].reshape(B, S * S, C), cnt, S * S).reshape(B, S, S, C))
    m.upload(batch)
    if cnt is not None:
        m.attach_img_regions(cnt)
    return m


def window(m, steps):
    m.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        m.forwardBackward(deferLoss=True)
    m.loss()
    m.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    p = params()
    batch = SyntheticDataloader(p, seed=7, fast=True).getTrainBatch(p)
    tag = opt.tag and opt.tag + ' '
    paths = tuple(opt.paths.split(',')) if opt.paths != 'all' else ('plain', 'full', 'mixed')
    assert set(paths) <= {'plain', 'full', 'mixed'}, paths
    models = {k: make(k, batch) for k in paths}
    for m in models.values():
        window(m, 3)                                                # warm-up: code objects, workspaces
    if opt.mode == 'trace':
        for k in paths:
            window(models[k], opt.inner)
        return
    ms = {k: [] for k in paths}
    for _ in range(opt.repeats):
        for k in paths:                                             # alternated
            ms[k].append(window(models[k], opt.inner))
    for k in paths:
        a, cnt = np.asarray(ms[k]), counts(k)
        live = 'all %d' % (B * S * S) if cnt is None else '%d of %d' % (int(cnt.sum()), B * S * S)
        print('%s%-6s step %.3f ms (min %.3f, max %.3f; %d windows of %d steps)  loss %.5f  live region rows %s'
              % (tag, k, np.median(a), a.min(), a.max(), a.size, opt.inner, models[k].loss(), live), flush=True)


if __name__ == '__main__':
    main()
