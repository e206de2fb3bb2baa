"""Generative retrieval at full size through the native host (model-level ABI): the dense head (vd_model_retrieve: vd_gemm_nt of
ALL T x N*O rows into a logits buffer + vd_logsoftmax_nll + a sum over time) against the live-row head (vd_model_retrieve_lhood,
params fusedLhood = 1: csrc/lhood.hip).  lf-ques-im-hist + gen, H = 512, V = 11 322, 2 layers, 20 dialogs x 10 rounds x 100
options, T = 21, random weights.  Two candidate-length profiles, per profile: live rows / total rows, the executed GEMM FLOPs of both
heads (from shapes), batches/s of both heads alternated in one process after warm-up with the spread over the repeats, the worst
|score difference| and the number of rounds whose ground-truth rank differs.
    python scripts/mb_retrieval.py [--repeats 7] [--only fused --profile uniform|short]   (--only fused: that head alone, for a trace)
A/B of two libraries (VD_LIB_PATH selects one): --tag NAME marks the process's lines, every profile also prints option_rows() of the
last fused call (the rows the candidate recurrence ran), and --save-scores PATH.npz keeps the fused scores per profile so that two
libraries' scores can be compared afterwards."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from visdial_amd.dataloader import SyntheticDataloader  # noqa: E402
from visdial_amd.native import NativeModel  # noqa: E402
from visdial_amd.opts import default_params, derive  # noqa: E402

ap = argparse.ArgumentParser(description='dense vs live-row log-likelihood head of generative retrieval at full size')
ap.add_argument('--repeats', type=int, default=7)
ap.add_argument('--only', choices=('fused',), help='the live-row head alone, for a kernel trace')
ap.add_argument('--profile', choices=('uniform', 'short'), help='one length profile only')
ap.add_argument('--tag', default='', help='printed in front of the per-head lines (A/B of two libraries)')
ap.add_argument('--save-scores', default='', help='write the fused scores of every profile to this .npz')
opt = ap.parse_args()
V, H, R, O, B, L = 11322, 512, 10, 100, 20, 20
T = L + 1

p = derive(default_params(encoder='lf-ques-im-hist', decoder='gen', vocabSize=V, embedSize=300, rnnHiddenSize=H, imgFeatureSize=4096,
                          numLayers=2, maxQuesCount=R, maxQuesLen=20, maxAnsLen=L, maxHistoryLenPerRound=40, numOptions=O, batchSize=B,
                          gpuid=0))


def lengths(profile, n, rng):
    if profile == 'uniform':                         # SyntheticDataloader.add_gen_options: uniform 1..20
        return rng.randint(1, L + 1, size=n)
    return np.minimum(L, 1 + rng.poisson(2.0, size=n))   # mean 3, capped at 20


def with_lengths(batch, lens, rng):
    n = len(lens)
    tok = rng.randint(1, V - 1, size=(n, L)).astype(np.int32) * (np.arange(L)[None, :] < lens[:, None])
    oin = np.zeros((n, T), np.int32)
    oout = np.zeros((n, T), np.int32)
    oin[:, 0] = V - 1                                # <START>
    oin[:, 1:] = tok
    oout[:, :L] = tok
    oout[np.arange(n), lens] = V                     # <END>
    return dict(batch, option_in=oin.reshape(B, R, O, T), option_out=oout.reshape(B, R, O, T))


nat = NativeModel(p, init_seed=1)
nat.training(False)
base, _ = SyntheticDataloader(p, seed=7, num_threads=B).getTestBatch(1, p, 'val')
N = B * R
print("lf-ques-im-hist + gen, H %d, V %d, %d layers, %d dialogs x %d rounds x %d options, T %d, native host, random weights"
      % (H, V, p['numLayers'], B, R, O, T))
print("('short' stands in for the real answer-length distribution -- the dataset paper gives a mean of about 3 words --, which is not on "
      "this machine)", flush=True)


def run(fused, batch):
    nat.params['fusedLhood'] = int(fused)
    t0 = time.perf_counter()
    gt = np.asarray(nat.retrieveBatch(batch, useGt=True)).reshape(-1)       # upload + retrieve + ranks: one evaluate.py batch
    return time.perf_counter() - t0, gt


saved = {}
for profile in ([opt.profile] if opt.profile else ['uniform', 'short']):
    rng = np.random.RandomState(77)
    lens = lengths(profile, N * O, rng)
    batch = with_lengths(base, lens, rng)
    live = int(((batch['option_in'] != 0) & (batch['option_out'] > 0)).sum())
    total = T * N * O
    print("\n%s lengths (mean %.2f): live rows %d / %d = %.3f" % (profile, lens.mean(), live, total, live / total))
    print("  vocabulary GEMM executed: dense %.3f TFLOP, live-row %.3f TFLOP" % (2.0 * total * V * H / 1e12, 2.0 * live * V * H / 1e12))
    heads = (1,) if opt.only else (0, 1)
    for f in heads:                                  # warm-up: workspaces, code objects
        run(f, batch)
        run(f, batch)
    if 1 in heads:
        ex, tot = nat.option_rows()
        print("  %soption_rows after the fused head: executed %d of %d = %.3f" % (opt.tag and opt.tag + ' ', ex, tot, ex / max(tot, 1)))
    times = {f: [] for f in heads}
    res = {}
    for _ in range(opt.repeats):                     # alternated
        for f in heads:
            dt, gt = run(f, batch)
            times[f].append(dt)
            res[f] = (gt, nat.scores(N, O).copy())
    for f in heads:
        t = np.asarray(times[f])
        print("  %s%-8s %7.2f ms per batch (median of %d; min %.2f, max %.2f) = %6.2f batches/s" % (
            opt.tag and opt.tag + ' ', 'fused' if f else 'dense', np.median(t) * 1e3, len(t), t.min() * 1e3, t.max() * 1e3, 1.0 / np.median(t)), flush=True)
    if opt.save_scores:
        saved[profile] = res[1][1]
    if not opt.only:
        d, f = res[0], res[1]
        print("  speed-up %.2fx; worst |dense - fused| score %.3e (|score| max %.1f); rounds whose ground-truth rank differs: %d of %d"
              % (np.median(times[0]) / np.median(times[1]), np.abs(d[1].astype(np.float64) - f[1]).max(), np.abs(d[1]).max(),
                 int((d[0] != f[0]).sum()), N))
if opt.save_scores:
    np.savez(opt.save_scores, **saved)
nat.close()
