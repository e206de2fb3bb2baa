"""Answer generation at full size through the native host (model-level ABI): the per-dialog host loop (beamBatch / sampleBatch 0:
vd_model_decode_step + a V-wide host sort or draw per explored row) against the batched device path (beamBatch / sampleBatch 20:
vd_model_beam_search / vd_model_sample over every round of 20 dialogs, the host's uniforms uploaded once).  lf-ques-im-hist + gen,
H = 512, V = 11 322, 2 layers, length 20, random weights; beam 5, or sampling at temperature 1.  Prints dialogs/s per path and how
many dialogs have identical records.
    python scripts/mb_generate.py --mode beam|sample [dialogs] [--only batched]   (--only batched: the device path alone, for a trace)
    --mode sample --topK k --topP p: top-k / nucleus truncation on both paths (the model is created with the knobs: the device sampler
    takes them at vd_model_create)
    --mode beam --beamSize k --beamGroups G --beamDiversity l: diverse beam search on both paths (the model is created with the knobs);
    also prints the share of rounds whose G answers are not all the same.  --vocabScale s multiplies the vocabulary projection of the
    random model (60 = the peaked rows of test_beam_search_gpu.full_size_fixture; near-uniform rows otherwise)
    --mode beam --minLen m --noRepeatNgram n --lengthPenalty a: the beam constraints (csrc/beam.hip C1-C6) on both paths (the model is
    created with the knobs)
    --mode beam --rollout 1: every round answered on a history of the model's own earlier answers (csrc/beam.hip R1-R6): the per-dialog
    loop (one encode per round) against the device rollout (the model is created with the knob).  The history is then generate.py's:
    one row of question + answer per round, maxQuesLen + maxAnsLen = 40 wide, the caption in row 0"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from visdial_amd.dataloader import SyntheticDataloader  # noqa: E402
from visdial_amd.native import NativeModel  # noqa: E402
from visdial_amd.opts import default_params, derive  # noqa: E402

ap = argparse.ArgumentParser(description='batched vs per-dialog answer generation at full size')
ap.add_argument('dialogs', nargs='?', type=int, default=20)
ap.add_argument('--mode', choices=('beam', 'sample'), required=True)
ap.add_argument('--only', choices=('batched',), help='the device path alone, for a kernel trace')
ap.add_argument('--topK', type=int, default=0, help='--mode sample: sample among the k most likely words (0 = off)')
ap.add_argument('--topP', type=float, default=1.0, help='--mode sample: nucleus truncation (1 = off)')
ap.add_argument('--beamSize', type=int, default=5, help='--mode beam: slots per round')
ap.add_argument('--beamGroups', type=int, default=1, help='--mode beam: diverse beam search in that many groups (1 = off)')
ap.add_argument('--beamDiversity', type=float, default=0.5, help='--mode beam with --beamGroups > 1: the penalty per earlier choice')
ap.add_argument('--minLen', type=int, default=0, help='--mode beam: no answer of fewer than that many words (0 = off)')
ap.add_argument('--noRepeatNgram', type=int, default=0, help='--mode beam: no n-gram of that many words twice in a hypothesis (0 = off)')
ap.add_argument('--lengthPenalty', type=float, default=0.0, help='--mode beam: finished hypotheses compete on score / length^that (0 = off)')
ap.add_argument('--rollout', type=int, default=0, choices=(0, 1), help='--mode beam: answer on the generated history (0 = off)')
ap.add_argument('--rolloutEncoder', default='full', choices=('full', 'round'),
                help='--rollout 1: round = passes 1 .. R - 1 encode the round they answer alone (VD_ROLLOUT_ENCODER)')
ap.add_argument('--vocabScale', type=float, default=1.0, help='multiply vocab.W of the random model (peaked rows)')
opt = ap.parse_args()
MODE_KNOBS = opt.topK != 0 or opt.topP != 1.0
if MODE_KNOBS and opt.mode != 'sample':
    ap.error('--topK / --topP truncate sampling: use --mode sample')
GROUPS = opt.beamGroups
if (GROUPS != 1 or opt.beamSize != 5) and opt.mode != 'beam':
    ap.error('--beamSize / --beamGroups belong to beam search: use --mode beam')
LIMITS = {} if (opt.minLen, opt.noRepeatNgram, opt.lengthPenalty) == (0, 0, 0.0) else dict(
    beamMinLen=opt.minLen, beamNoRepeat=opt.noRepeatNgram, beamLengthPenalty=opt.lengthPenalty)
if LIMITS and opt.mode != 'beam':
    ap.error('--minLen / --noRepeatNgram / --lengthPenalty belong to beam search: use --mode beam')
if opt.rollout and (opt.mode != 'beam' or GROUPS != 1):
    ap.error('--rollout 1 belongs to beam search without groups: use --mode beam --beamGroups 1')
if opt.rolloutEncoder == 'round' and not opt.rollout:
    ap.error('--rolloutEncoder round belongs to a rollout: use --rollout 1')
MODE, D, ONLY_BATCHED = opt.mode, opt.dialogs, opt.only == 'batched'
V, R = 11322, 10


class Dialogs(object):
    """D synthetic dialogs behind the getIndexData / word2ind / ind2word surface generateAnswers reads"""

    def __init__(self, p, n):
        q = dict(p, batchSize=n)
        self.b = SyntheticDataloader(q, seed=5).getTrainBatch(q)
        if opt.rollout:          # generate.py's history (concatHistory = False): caption, then question + ground-truth answer per round
            from visdial_amd.split_eval import rollout_history_row
            Th = int(p['maxQuesLen']) + int(p['maxAnsLen'])
            hist = np.zeros((n, R, Th), np.int32)
            hist[:, 0] = self.b['hist'][:, 0, -Th:]
            for i in range(n):
                for r in range(1, R):
                    hist[i, r] = rollout_history_row(self.b['ques_fwd'][i, r - 1], self.b['answer_in'][i, r - 1], Th, V)
            self.b['hist'] = hist
        self.data = {'val': {'hist': self.b['hist']}}
        self.numThreads = {'val': n}
        self.word2ind = {'<START>': V - 1, '<END>': V}
        self.ind2word = {i: '<START>' if i == V - 1 else '<END>' if i == V else 'w%d' % i for i in range(1, V + 1)}

    def getIndexData(self, inds, params, dtype):
        ix = np.asarray(inds, np.int64) - 1
        return {k: np.ascontiguousarray(self.b[k][ix]) for k in ('ques_fwd', 'hist', 'img_feat')}


p = derive(default_params(encoder='lf-ques-im-hist', decoder='gen', vocabSize=V, embedSize=300, rnnHiddenSize=512, imgFeatureSize=4096,
                          numLayers=2, maxQuesCount=R, maxQuesLen=20, maxAnsLen=20, maxHistoryLenPerRound=40, batchSize=20, gpuid=0))
dl = Dialogs(p, D)
knobs = dict(topK=opt.topK, topP=opt.topP) if MODE_KNOBS else {}
if GROUPS != 1:
    knobs.update(beamGroups=GROUPS, beamDiversity=opt.beamDiversity)
knobs.update(LIMITS)
if opt.rollout:
    knobs.update(beamRollout=1, rolloutEncoder=opt.rolloutEncoder)
nat = NativeModel(dict(p, **knobs), init_seed=1)
nat.training(False)
if opt.vocabScale != 1.0:
    P = nat.get_parameters_dict()
    P['vocab.W'] = P['vocab.W'] * np.float32(opt.vocabScale)
    nat.set_parameters_dict(P)
if MODE == 'beam':
    key, cfg = 'beamBatch', dict(beamSize=opt.beamSize, beamLen=20, maxThreads=D)
    what = 'beam %d' % cfg['beamSize']
    if GROUPS != 1:
        cfg.update(beamGroups=GROUPS, beamDiversity=opt.beamDiversity)
        what += ' in %d groups (diversity %g)' % (GROUPS, opt.beamDiversity)
    if LIMITS:
        cfg.update(LIMITS)
        what += ' (minLen %d, noRepeatNgram %d, lengthPenalty %g)' % (opt.minLen, opt.noRepeatNgram, opt.lengthPenalty)
    if opt.rollout:
        cfg.update(rollout=1)
        what += ', rollout (encoder: %s)' % opt.rolloutEncoder
else:
    key, cfg = 'sampleBatch', dict(sampleWords=1, beamLen=20, temperature=1.0, maxThreads=D, seed=1234, topK=opt.topK, topP=opt.topP)
    what = 'sampling' + (' (topK %d, topP %g)' % (opt.topK, opt.topP) if MODE_KNOBS else '')
print("lf-ques-im-hist + gen, H %d, V %d, %d layers, %s, length %d%s, %d dialogs x %d rounds" % (
    p['rnnHiddenSize'], V, p['numLayers'], what, cfg['beamLen'],
    ', temperature %g' % cfg['temperature'] if MODE == 'sample' else '', D, R), flush=True)
nat.generateAnswers(dl, 'val', dict(cfg, maxThreads=min(D, 20), **{key: 20}))          # warm-up: workspaces, code objects
res = {}
for b in ((20,) if ONLY_BATCHED else (0, 20)):
    reps = 1 if b == 0 else 5
    t0 = time.perf_counter()
    for _ in range(reps):
        out = nat.generateAnswers(dl, 'val', dict(cfg, **{key: b}))
    dt = (time.perf_counter() - t0) / reps
    res[b] = out
    print("%s %2d: %8.3f s for %d dialogs = %9.2f dialogs/s  (%.2f ms per dialog)" % (key, b, dt, D, D / dt, dt / D * 1e3), flush=True)
    res[b, 't'] = dt
if not ONLY_BATCHED:
    same = sum(a == b for a, b in zip(res[0], res[20]))
    print("speed-up %.1fx; dialogs with identical records: %d of %d" % (res[0, 't'] / res[20, 't'], same, D))
if GROUPS > 1:
    rounds = [e['answers'] for d in out for e in d['dialog']]
    print("rounds whose %d answers are not all the same: %d of %d; distinct answers per round on average: %.2f" % (
        GROUPS, sum(len(set(a)) > 1 for a in rounds), len(rounds), float(np.mean([len(set(a)) for a in rounds]))))
nat.close()
