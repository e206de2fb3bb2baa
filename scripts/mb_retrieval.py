"""Generative retrieval at full size through the native host (model-level ABI): the dense head (vd_model_retrieve: vd_gemm_nt of
ALL T x N*O rows into a logits buffer + vd_logsoftmax_nll + a sum over time) against the live-row head (vd_model_retrieve_lhood,
params fusedLhood = 1: csrc/lhood.hip).  lf-ques-im-hist + gen, H = 512, V = 11 322, 2 layers, 20 dialogs x 10 rounds x 100
options, T = 21, random weights.  Two candidate-length profiles, per profile: live rows / total rows, the executed GEMM FLOPs of both
heads (from shapes), batches/s of both heads alternated in one process after warm-up with the spread over the repeats, the worst
|score difference| and the number of rounds whose ground-truth rank differs.
    python scripts/mb_retrieval.py [--repeats 7] [--only fused --profile uniform|short]   (--only fused: that head alone, for a trace)
A/B of two libraries (VD_LIB_PATH selects one): --tag NAME marks the process's lines, every profile also prints option_rows() of the
last fused call (the rows the candidate recurrence ran), and --save-scores PATH.npz keeps the fused scores per profile so that two
libraries' scores can be compared afterwards.

Third leg (--tree): the same batches through a second model created with params fusedLhood = 2 (VD_LHOOD_TREE: the candidates over a
prefix tree of their tokens), alternated with the other heads; per profile nodes / live rows, the rows the tree recurrence ran, and
the host time of the upload with and without the tree build.  A library that does not know the switch (the parent commit's through
VD_LIB_PATH) is run without --tree.  --profile pooled: every candidate drawn from a pool of --gen-pool answers (lengths 1 +
Poisson(2) capped at 20, every third answer continuing the one before it) with probability ~ 1 / (rank + 1), so that beginnings repeat
inside a round; nobody has measured how often they do on the real VisDial splits.

--mode disc: discriminative evaluation with and without the answer-encoding cache (params optionCache) at full
size: mn-att-ques-im-hist + disc, 20 dialogs x 10 rounds x 100 options, To = 20, split9.  The synthetic loader has no repeats, so the
candidates of --batches batches are drawn from a pool of --pool distinct answers.  Per case batches/s over one pass of those batches
(upload + retrieve + ranks per batch, as evaluate.py runs it), median over --repeats with min / max: uncached; cached and cold (first
pass after a flush); cached and warm (second pass), with the rows the recurrence ran and the device memory the process holds after
each case.  --cases uncached runs the first alone (the parent commit's library through VD_LIB_PATH knows no cache), --cases cached the other two
(for a kernel trace).
--mode disc --rollout 1: ranking on a rollout (evaluate.py -rollout 1; csrc/beam.hip E1-E5) at the same full size, the synthetic loader's
own candidates: per batch (upload + retrieve + ranks, as evaluate.py runs it) the plain retrieval on the ground-truth history (a model
created without VD_RETRIEVE_ROLLOUT), the device rollout (one upload + one vd_model_retrieve on a model created with it) and the host loop
(R uploads + retrievals, --host-batches of the batches), alternated.  The device rollout's time over the plain retrieval's is what the
R - 1 further encoder passes, scorings and picks cost: the option recurrence runs once in both.  --cases plain runs the first alone (the
parent commit's library through VD_LIB_PATH knows no rollout), --cases device the second (for a kernel trace).  --rolloutHistory concat: the
same paths for lf-ques-im-hist + disc on its concatenated history (W = 300; CH1-CH6, VD_ROLLOUT_CONCAT_END).  --rolloutEncoder round creates
the device rollout's model with VD_ROLLOUT_ENCODER = round (passes 1 .. R - 1 encode the round they rank alone); both adds that model as a
fourth path `round` beside `device`, alternated with it.
--mode step: the option recurrence alone (vd_lstm_forward, table mode, 20 000 x 512, 20 steps), saving against VD_FLAG_STATE_ONLY,
alternated, device time by events."""
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
ap.add_argument('--only', choices=('fused', 'tree'), help='one head alone, for a kernel trace')
ap.add_argument('--profile', choices=('uniform', 'short', 'pooled'), help='one length profile only')
ap.add_argument('--tree', action='store_true', help='--mode gen: also the prefix-tree head (params fusedLhood = 2)')
ap.add_argument('--gen-pool', type=int, default=2000, help='--profile pooled: answers the candidates are drawn from')
ap.add_argument('--tag', default='', help='printed in front of the per-head lines (A/B of two libraries)')
ap.add_argument('--save-scores', default='', help='write the fused scores of every profile to this .npz')
ap.add_argument('--mode', choices=('gen', 'disc', 'step'), default='gen')
ap.add_argument('--pool', type=int, default=2000, help='--mode disc: distinct answers the candidates are drawn from')
ap.add_argument('--batches', type=int, default=6, help='--mode disc: batches per pass')
ap.add_argument('--cases', choices=('all', 'uncached', 'cached', 'plain', 'device'), default='all', help='--mode disc')
ap.add_argument('--rollout', type=int, choices=(0, 1), default=0, help='--mode disc: ranking on a rollout, three paths (see above)')
ap.add_argument('--rolloutEncoder', choices=('full', 'round', 'both'), default='full',
                help='--mode disc --rollout 1: the encoder of the device rollout\'s later passes; both = the two as separate paths')
ap.add_argument('--rolloutHistory', choices=('row', 'concat'), default='row',
                help='--mode disc --rollout 1: concat = lf-ques-im-hist + disc on its concatenated history (W = 300), the models created with '
                     'VD_ROLLOUT_CONCAT_END (csrc/beam.hip CH1-CH6); row = mn-att-ques-im-hist on per-round rows, as ever')
ap.add_argument('--host-batches', type=int, default=2, help='--mode disc --rollout 1: batches the host loop ranks per pass')
opt = ap.parse_args()


def held_mb():
    """device memory in use on the card, MB (the library allocates with hipMalloc, outside the tensor library's pool)"""
    import torch
    free, total = torch.cuda.mem_get_info()
    return (total - free) / 1e6


def disc_mode():
    B, R, O, To, H = 20, 10, 100, 20, 512
    p = derive(default_params(encoder='mn-att-ques-im-hist', decoder='disc', vocabSize=11322, imgFeatureSize=512, imgSpatialSize=14,
                              maxHistoryLenPerRound=40, batchSize=B, numOptions=O, maxQuesCount=R, maxAnsLen=To, lstmPrecision='split9',
                              gpuid=0))
    tag = opt.tag and opt.tag + ' '
    rng = np.random.RandomState(5)
    lens = rng.randint(1, To + 1, size=opt.pool)
    pool = (rng.randint(1, p['vocabSize'], size=(opt.pool, To)) * (np.arange(To)[None, :] < lens[:, None])).astype(np.int32)
    pool = np.unique(pool, axis=0)
    dl = SyntheticDataloader(p, seed=7, num_threads=B * opt.batches)
    batches, start = [], 1
    for _ in range(opt.batches):
        b, start = dl.getTestBatch(start, p, 'val')
        b['options'] = pool[rng.randint(0, pool.shape[0], size=B * R * O)].reshape(B * R, O, To)
        batches.append(b)
    distinct = len({r.tobytes() for b in batches for r in b['options'].reshape(-1, To)})
    print("%smn-att-ques-im-hist + disc, H %d, %d dialogs x %d rounds x %d options, To %d, split9, native host, random weights; pool of %d "
          "distinct answers, %d batches per pass = %d candidate rows, %d distinct" % (tag, H, B, R, O, To, pool.shape[0], opt.batches,
                                                                                  opt.batches * B * R * O, distinct), flush=True)
    base_mb = held_mb()

    def one_pass(nat):
        rows, t0 = 0, time.perf_counter()
        for b in batches:
            nat.retrieveBatch(b, useGt=True)
            rows += nat.option_rows()[0]
        return (time.perf_counter() - t0) / len(batches), rows

    def report(name, ts, rows, mb):
        t = np.asarray(ts)
        print("  %s%-14s %7.2f ms per batch (median of %d; min %.2f, max %.2f) = %6.2f batches/s; rows the recurrence ran per pass %d; "
              "device memory held %.0f MB" % (tag, name, np.median(t) * 1e3, len(t), t.min() * 1e3, t.max() * 1e3, 1.0 / np.median(t), rows,
                                             mb), flush=True)
    scores = {}
    for cached in {'uncached': (0,), 'cached': (1,), 'all': (0, 1)}[opt.cases]:
        nat = NativeModel(dict(p, optionCache=cached), init_seed=1)
        nat.training(False)
        one_pass(nat)                                   # warm-up: workspaces, code objects
        one_pass(nat)
        cold, warm, rows_c, rows_w = [], [], 0, 0
        for _ in range(opt.repeats):
            if cached:
                nat.training(True)                      # flush
                nat.training(False)
            t, rows_c = one_pass(nat)
            cold.append(t)
            t, rows_w = one_pass(nat)
            warm.append(t)
        scores[cached] = nat.scores(B * R, O).copy()
        mb = held_mb() - base_mb
        if cached:
            report('cached cold', cold, rows_c, mb)
            report('cached warm', warm, rows_w, mb)
        else:
            report('uncached', cold + warm, rows_c, mb)
        nat.close()
    if len(scores) == 2:
        print("  worst |cached - uncached| score of the last batch %.3e (|score| max %.2f)"
              % (np.abs(scores[0].astype(np.float64) - scores[1]).max(), np.abs(scores[0]).max()))


def disc_rollout_mode():
    from visdial_amd.split_eval import SplitEval
    B, R, O, To, H = 20, 10, 100, 20, 512
    concat = opt.rolloutHistory == 'concat'
    if concat:
        p = derive(default_params(encoder='lf-ques-im-hist', decoder='disc', vocabSize=11322, imgFeatureSize=4096, batchSize=B, numOptions=O,
                                  maxQuesCount=R, maxAnsLen=To, lstmPrecision='split9', gpuid=0))
    else:
        p = derive(default_params(encoder='mn-att-ques-im-hist', decoder='disc', vocabSize=11322, imgFeatureSize=512, imgSpatialSize=14,
                                  maxHistoryLenPerRound=40, batchSize=B, numOptions=O, maxQuesCount=R, maxAnsLen=To, lstmPrecision='split9',
                                  gpuid=0))
    tag = opt.tag and opt.tag + ' '
    dl = SyntheticDataloader(p, seed=7, num_threads=B * opt.batches)
    rule = dict(rolloutHistory='concat', rolloutConcatEnd=dl.endToken) if concat else {}
    batches, start = [], 1
    for _ in range(opt.batches):
        b, start = dl.getTestBatch(start, p, 'val')
        batches.append(b)
    print("%s%s + disc, H %d, %d dialogs x %d rounds x %d options, To %d, Th %d, Tq %d, split9, native host, random weights, "
          "%d batches per pass" % (tag, p['encoder'], H, B, R, O, To, batches[0]['hist'].shape[2], batches[0]['ques_fwd'].shape[2], opt.batches), flush=True)
    want = {'all': ('plain', 'device', 'host'), 'plain': ('plain',), 'device': ('device',)}[opt.cases]
    if opt.rolloutEncoder == 'both' and 'device' in want:
        want = want + ('round',)
    plain = roll = rnd = None
    if 'plain' in want or 'host' in want:
        plain = NativeModel(dict(p), init_seed=1)
        plain.training(False)
        plain.params.update(rule)                       # the host loop's rule; the model itself is created without the variable
    if 'device' in want:
        roll = NativeModel(dict(p, retrieveRollout=1, rolloutEncoder='round' if opt.rolloutEncoder == 'round' else 'full', **rule), init_seed=1)
        roll.training(False)
    if 'round' in want:
        rnd = NativeModel(dict(p, retrieveRollout=1, rolloutEncoder='round', **rule), init_seed=1)
        rnd.training(False)

    def one_pass(case):
        bs = batches[:opt.host_batches] if case == 'host' else batches
        out, t0 = None, time.perf_counter()
        for b in bs:
            if case == 'plain':
                out = plain.retrieveBatch(b, useGt=False)
            elif case == 'device':
                out = roll.retrieve_rollout_batch(b)
            elif case == 'round':
                out = rnd.retrieve_rollout_batch(b)
            else:
                out = SplitEval.retrieve_rollout_batch(plain, dict(b, hist=np.array(b['hist'])))
        return (time.perf_counter() - t0) / len(bs), out
    cases = want
    for c in cases:                                     # warm-up: workspaces, code objects
        one_pass(c)
        one_pass(c)
    times, last = {c: [] for c in cases}, {}
    for _ in range(opt.repeats):                        # alternated
        for c in cases:
            t, last[c] = one_pass(c)
            times[c].append(t)
    for c in cases:
        t = np.asarray(times[c])
        print("  %s%-12s %8.2f ms per batch (median of %d; min %.2f, max %.2f) = %7.2f batches/s" % (
            tag, c, np.median(t) * 1e3, len(t), t.min() * 1e3, t.max() * 1e3, 1.0 / np.median(t)), flush=True)
    if 'device' in last and 'host' in last:
        same = np.array_equal(roll.retrieve_rollout_batch(batches[opt.host_batches - 1]), last['host'])
        print("  device rollout and host loop return the same ranks for batch %d: %s" % (opt.host_batches - 1, same))
    if 'device' in last and 'round' in last:
        d, q = np.median(times['device']), np.median(times['round'])
        print("  round against full: %.2fx (%.2f ms per batch less); the same ranks for the last batch: %s"
              % (d / q, (d - q) * 1e3, np.array_equal(last['device'], last['round'])))
    if 'device' in times and 'plain' in times:
        d, q = np.median(times['device']), np.median(times['plain'])
        print("  the R - 1 further encoder passes, scorings and picks: %.2f ms per batch = %.0f %% of the device rollout's batch"
              % ((d - q) * 1e3, 100.0 * (d - q) / d))
    if 'device' in last and 'plain' in last:
        first = lambda r: np.asarray(r).reshape(B * R, O).argmin(1)
        print("  rounds of the last batch whose rank-1 candidate differs between the rollout and the ground-truth history: %d of %d"
              % (int((first(last['device']) != first(last['plain'])).sum()), B * R))
    for m in (plain, roll, rnd):
        if m is not None:
            m.close()


def step_mode():
    import torch
    from visdial_amd import ops
    N, H, T, Vt = 20000, 512, 20, 11323
    g = torch.Generator(device='cuda').manual_seed(1)
    table = torch.randn(Vt, 4 * H, device='cuda', generator=g) * 0.5
    Wh = torch.randn(H, 4 * H, device='cuda', generator=g) / H ** 0.5
    tok = torch.randint(1, Vt, (T, N), device='cuda', dtype=torch.int32, generator=g)
    gates, h, c = (torch.empty(T, N, k * H, device='cuda') for k in (4, 1, 1))
    h2, c2 = torch.empty(2, N, H, device='cuda'), torch.empty(2, N, H, device='cuda')
    for name, flags in (('split9', ops.FLAG_SPLIT9), ('fp32', 0)):
        def run(state):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            if state:
                ops.lstm_forward(table, Wh, None, h2, c2, T, N, H, 0, 4 * H, tok_gather=tok, flags=flags | ops.FLAG_STATE_ONLY)
            else:
                ops.lstm_forward(table, Wh, gates, h, c, T, N, H, 0, 4 * H, tok_gather=tok, flags=flags)
            b.record()
            b.synchronize()
            return a.elapsed_time(b)
        for st in (0, 1, 0, 1):
            run(st)
        ts = {0: [], 1: []}
        for _ in range(opt.repeats):
            for st in (0, 1):
                ts[st].append(run(st))
        same = bool((h2[(T - 1) & 1] == h[T - 1]).all()) and bool((c2[(T - 1) & 1] == c[T - 1]).all())
        for st in (0, 1):
            t = np.asarray(ts[st])
            print("  %s%s %-10s %d x %d, %d steps: %7.3f ms per pass (median of %d; min %.3f, max %.3f) = %.3f ms per step"
                  % (opt.tag and opt.tag + ' ', name, 'state-only' if st else 'saving', N, H, T, np.median(t), len(t), t.min(), t.max(),
                     np.median(t) / T), flush=True)
        print("  %s: final h and c bit-identical: %s" % (name, same))


if opt.mode == 'disc':
    disc_rollout_mode() if opt.rollout else disc_mode()
    sys.exit(0)
if opt.mode == 'step':
    step_mode()
    sys.exit(0)
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


def pooled(batch, rng):
    """candidates drawn from a pool with a heavy tail (see the module docstring)"""
    answers = [[int(w) for w in rng.randint(1, V - 1, size=min(L, 1 + rng.poisson(2.0)))] for _ in range(opt.gen_pool)]
    for k in range(1, opt.gen_pool, 3):
        answers[k] = (answers[k - 1] + answers[k])[:L]
    w = 1.0 / (1.0 + np.arange(opt.gen_pool))
    pick = rng.choice(opt.gen_pool, size=B * R * O, p=w / w.sum())
    oin = np.zeros((B * R * O, T), np.int32)
    oout = np.zeros((B * R * O, T), np.int32)
    oin[:, 0] = V - 1
    for r, k in enumerate(pick):
        a = answers[k]
        oin[r, 1:1 + len(a)] = a
        oout[r, :len(a)] = a
        oout[r, len(a)] = V
    lens = np.array([len(answers[k]) for k in pick])
    return dict(batch, option_in=oin.reshape(B, R, O, T), option_out=oout.reshape(B, R, O, T)), lens


use_tree = opt.tree or opt.only == 'tree'
nat = NativeModel(p, init_seed=1)
nat.training(False)
nat_tree = None
if use_tree:
    nat_tree = NativeModel(dict(p, fusedLhood=2), init_seed=1)       # the same weights (same seed), created with VD_LHOOD_TREE
    nat_tree.training(False)
base, _ = SyntheticDataloader(p, seed=7, num_threads=B).getTestBatch(1, p, 'val')
N = B * R
print("lf-ques-im-hist + gen, H %d, V %d, %d layers, %d dialogs x %d rounds x %d options, T %d, native host, random weights"
      % (H, V, p['numLayers'], B, R, O, T))
print("('short' stands in for the real answer-length distribution -- the dataset paper gives a mean of about 3 words --, which is not on "
      "this machine)", flush=True)


def run(fused, batch):
    model = nat_tree if fused == 2 else nat
    model.params['fusedLhood'] = int(fused)
    t0 = time.perf_counter()
    gt = np.asarray(model.retrieveBatch(batch, useGt=True)).reshape(-1)     # upload + retrieve + ranks: one evaluate.py batch
    return time.perf_counter() - t0, gt


def upload_ms(model, batch, n=5):
    ts = []
    for _ in range(n):
        model.synchronize()
        t0 = time.perf_counter()
        model.upload(batch)
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


saved = {}
NAMES = {0: 'dense', 1: 'fused', 2: 'tree'}
for profile in ([opt.profile] if opt.profile else ['uniform', 'short', 'pooled']):
    rng = np.random.RandomState(77)
    if profile == 'pooled':
        batch, lens = pooled(base, rng)
    else:
        lens = lengths(profile, N * O, rng)
        batch = with_lengths(base, lens, rng)
    live = int(((batch['option_in'] != 0) & (batch['option_out'] > 0)).sum())
    total = T * N * O
    print("\n%s lengths (mean %.2f): live rows %d / %d = %.3f" % (profile, lens.mean(), live, total, live / total))
    print("  vocabulary GEMM executed: dense %.3f TFLOP, live-row %.3f TFLOP" % (2.0 * total * V * H / 1e12, 2.0 * live * V * H / 1e12))
    heads = ({'fused': (1,), 'tree': (2,)}[opt.only] if opt.only else (0, 1)) + ((2,) if opt.tree and opt.only != 'tree' else ())
    for f in heads:                                  # warm-up: workspaces, code objects
        run(f, batch)
        run(f, batch)
    if 1 in heads:
        run(1, batch)
        ex, tot = nat.option_rows()
        print("  %soption_rows after the fused head: executed %d of %d = %.3f" % (opt.tag and opt.tag + ' ', ex, tot, ex / max(tot, 1)))
    if 2 in heads:
        from visdial_amd import prefix_tree
        st = prefix_tree.stats(batch['option_in'])
        ex, tot = nat_tree.option_rows()
        print("  %stree: %d nodes for %d rows with a token = %.3f; option_rows executed %d of %d = %.3f; widest level %d"
              % (opt.tag and opt.tag + ' ', st['nodes'], st['live'], st['nodes'] / max(st['live'], 1), ex, tot, ex / max(tot, 1),
                 max(st['widths'])))
        print("  %shost time of one upload: %.2f ms with the tree build, %.2f ms without" % (opt.tag and opt.tag + ' ',
                                                                                           upload_ms(nat_tree, batch), upload_ms(nat, batch)))
    times = {f: [] for f in heads}
    res = {}
    for _ in range(opt.repeats):                     # alternated
        for f in heads:
            dt, gt = run(f, batch)
            times[f].append(dt)
            res[f] = (gt, (nat_tree if f == 2 else nat).scores(N, O).copy())
    for f in heads:
        t = np.asarray(times[f])
        print("  %s%-8s %7.2f ms per batch (median of %d; min %.2f, max %.2f) = %6.2f batches/s" % (
            opt.tag and opt.tag + ' ', NAMES[f], np.median(t) * 1e3, len(t), t.min() * 1e3, t.max() * 1e3, 1.0 / np.median(t)), flush=True)
    if opt.save_scores and 1 in res:
        saved[profile] = res[1][1]
    if 2 in res and 0 in res:
        d, f = res[0], res[2]
        print("  tree: speed-up over dense %.2fx, over fused %.2fx; worst |dense - tree| score %.3e; rounds whose ground-truth rank differs: %d of %d"
              % (np.median(times[0]) / np.median(times[2]), np.median(times[1]) / np.median(times[2]),
                 np.abs(d[1].astype(np.float64) - f[1]).max(), int((d[0] != f[0]).sum()), N))
    if not opt.only:
        d, f = res[0], res[1]
        print("  speed-up %.2fx; worst |dense - fused| score %.3e (|score| max %.1f); rounds whose ground-truth rank differs: %d of %d"
              % (np.median(times[0]) / np.median(times[1]), np.abs(d[1].astype(np.float64) - f[1]).max(), np.abs(d[1]).max(),
                 int((d[0] != f[0]).sum()), N))
if opt.save_scores:
    np.savez(opt.save_scores, **saved)
nat.close()
if nat_tree is not None:
    nat_tree.close()
