"""Dense-annotation fine-tuning at the headline size through the native host (model-level ABI): mn-att-ques-im-hist + disc, 20 dialogs x
10 rounds x 100 options (N = 200 rounds), H = 512, To = 20, split9, random weights, one synthetic batch uploaded once per path.

  --mode step (default): the training step (vd_model_forward_backward(m, 0) + vd_model_loss; no update, the weights stand still) on
      plain      no attachment: score_ce_kernel
      mix1       '@dense_relevance' with no annotated row, mu = 1: score_ce_dense_kernel computing the plain head's target
      finetune   one annotated round per dialog, mu = 0: B of N rounds carry a gradient, the option-LSTM backward still runs all N * O rows
      live       the same matrix as '@dense_relevance_live' (loss.hip DL1-DL5): the option recurrence, its backward, the table-gradient row
                 sum and dWh run the B * O candidate rows of the annotated rounds
    alternated in one process after warm-up; per path the median step time over --repeats with min / max and the median family_ms
    (option LSTM forward, backward, dWh).  --paths plain runs the first alone (a library that does not know the attachment -- the parent
    commit's, through VD_LIB_PATH), --paths plain,finetune those two (a library that does not know the live name);
    --tag NAME marks the process's lines for an A/B of two libraries, processes alternated by the caller.
  --mode ndcg: vd_model_get_tensor '@ndcg' per call on the scores of one retrieval (kernel + the 1.6 KB read-back + synchronise), host clock.
  --mode trace: a few steps of every path and a few '@ndcg' calls, nothing timed: run it under `rocprofv3 --kernel-trace --stats` for the
      per-kernel times of score_ce_kernel, score_ce_dense_kernel and ndcg_kernel and the dispatch counts.
  --mode agree: one live step against one all-rows fine-tuning step of the same weights and pinned dropout masks at this size: |loss
      difference|, the worst gradient rel-L2 over the tensors, the worst score difference over max(1, |s|) on the live rounds, the rows executed.

    python scripts/mb_dense.py [--mode step|ndcg|trace|agree] [--repeats 15] [--paths all|plain,finetune,...] [--tag NAME]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from visdial_amd.dataloader import SyntheticDataloader  # noqa: E402
from visdial_amd.native import NativeModel  # noqa: E402
from visdial_amd.opts import default_params, derive  # noqa: E402

ap = argparse.ArgumentParser(description='the dense training head and the NDCG kernel at the headline size')
ap.add_argument('--mode', choices=('step', 'ndcg', 'trace', 'agree'), default='step')
ap.add_argument('--repeats', type=int, default=15)
ap.add_argument('--inner', type=int, default=5, help='steps per timed window')
ap.add_argument('--paths', default='all', help="'all' or a comma-separated list of plain, mix1, finetune, live")
ap.add_argument('--tag', default='')
opt = ap.parse_args()

B, R, O, To, H = 20, 10, 100, 20, 512
N = B * R


def params(**kw):
    return derive(default_params(encoder='mn-att-ques-im-hist', decoder='disc', vocabSize=11322, imgFeatureSize=512, imgSpatialSize=14,
                                 maxHistoryLenPerRound=40, batchSize=B, numOptions=O, maxQuesCount=R, maxAnsLen=To, lstmPrecision='split9',
                                 gpuid=0, **kw))


def relevance(kind):
    rel = np.full((N, O), -1.0, np.float32)
    if kind in ('finetune', 'live'):                                 # one annotated round per dialog, ~10 relevant candidates each
        rng = np.random.RandomState(3)
        for i in range(B):
            row = np.zeros(O, np.float32)
            row[rng.choice(O, size=10, replace=False)] = rng.randint(1, 6, size=10) / 5.0
            rel[i * R + rng.randint(R)] = row
    return rel


def make(path, batch):
    m = NativeModel(params(denseMix=1.0 if path == 'mix1' else None))
    m.upload(batch)
    if path != 'plain':
        m.attach_dense_relevance(relevance(path), **({'live': True} if path == 'live' else {}))
    return m


def agree(batch):
    """the live step against the all-rows step: same weights (one model, no update), dropout noise pinned"""
    from visdial_amd import dense
    from visdial_amd.dataloader import dropout_mask_shapes
    masks = {k: (np.random.RandomState(5).rand(*s) > 0.5).astype(np.uint8) for k, s in dropout_mask_shapes(params(), batch).items()}
    m = NativeModel(params())
    m.set_dropout_masks(masks)
    rel, out = relevance('finetune'), {}
    for kind in ('finetune', 'live'):
        m.upload(batch)
        m.attach_dense_relevance(rel, **({'live': True} if kind == 'live' else {}))
        loss = m.forwardBackward()
        out[kind] = (loss, {k: v.astype(np.float64) for k, v in m.get_gradients_dict().items()}, m.scores(N, O), m.option_rows())
    (l0, g0, s0, r0), (l1, g1, s1, r1) = out['finetune'], out['live']
    live = dense.live_rounds(rel, 0.0)
    worst, name = max((float(np.linalg.norm(g1[k] - g0[k]) / np.linalg.norm(g0[k])), k) for k in g0 if np.linalg.norm(g0[k]) >= 1e-12 and k != 'att.b')
    ds = float((np.abs(s1[live] - s0[live]) / np.maximum(1.0, np.abs(s0[live]))).max())
    dead = np.setdiff1d(np.arange(N), live)
    print('agree: all-rows loss %.7f rows %s | live loss %.7f rows %s | |loss difference| %.3g | worst gradient rel-L2 %.3g (%s) | worst live '
          'score difference / max(1, |s|) %.3g | other rounds\' score rows all zero: %s'
          % (l0, r0, l1, r1, abs(l1 - l0), worst, name, ds, bool((s1[dead] == 0).all())), flush=True)
    m.close()


def window(m, steps):
    m.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        m.forwardBackward(deferLoss=True)
    m.loss()
    m.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3, m.family_ms()


def main():
    p = params()
    batch = SyntheticDataloader(p, seed=7, fast=True).getTrainBatch(p)
    tag = opt.tag and opt.tag + ' '
    paths = tuple(opt.paths.split(',')) if opt.paths != 'all' else ('plain', 'mix1', 'finetune', 'live')
    assert set(paths) <= {'plain', 'mix1', 'finetune', 'live'}, paths
    if opt.mode == 'agree':
        return agree(batch)
    if opt.mode == 'step':
        models = {k: make(k, batch) for k in paths}
        for m in models.values():
            window(m, 3)                                     # warm-up: code objects, workspaces
        ms = {k: [] for k in paths}
        fam = {k: [] for k in paths}
        for _ in range(opt.repeats):
            for k in paths:                                  # alternated
                t, f = window(models[k], opt.inner)
                ms[k].append(t)
                fam[k].append(f)
        for k in paths:
            a, f = np.asarray(ms[k]), np.median(np.asarray(fam[k]), axis=0)
            print('%s%-9s step %.3f ms (min %.3f, max %.3f; %d windows of %d steps)  family_ms fwd %.2f bwd %.2f dWh %.2f  loss %.5f  rows %d of %d'
                  % ((tag, k, np.median(a), a.min(), a.max(), a.size, opt.inner, f[0], f[1], f[2], models[k].loss()) + models[k].option_rows()),
                  flush=True)
        return
    m = make('finetune', batch)
    m.training(False)
    m.retrieveBatch(batch, useGt=False)
    m.attach_dense_relevance(relevance('finetune'))
    if opt.mode == 'ndcg':
        for _ in range(20):
            m.ndcg_rows()
        t = []
        for _ in range(opt.repeats):
            t0 = time.perf_counter()
            for _ in range(100):
                m.ndcg_rows()
            t.append((time.perf_counter() - t0) / 100 * 1e6)
        t = np.asarray(t)
        print("%s'@ndcg' per call (kernel + read-back + synchronise): %.1f us (min %.1f, max %.1f); %d annotated rounds of %d"
              % (tag, np.median(t), t.min(), t.max(), int((m.ndcg_rows() != -2).sum()), N), flush=True)
        return
    for _ in range(10):                                      # --mode trace
        m.ndcg_rows()
    m.training(True)
    for k in paths:
        mm = make(k, batch)
        window(mm, 6)
        mm.close()


if __name__ == '__main__':
    main()
