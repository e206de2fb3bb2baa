"""Answer generation by temperature sampling at full size through the native host (model-level ABI): per dialog with host draws
(sampleBatch 0: vd_model_decode_step + a V-wide host draw per round and step) against the batched device path (sampleBatch 20:
vd_model_sample over every round of 20 dialogs, the host's uniforms uploaded once).  lf-ques-im-hist + gen, H = 512,
V = 11 322, 2 layers, length 20, temperature 1, random weights.  Prints dialogs/s per path and how many dialogs have
identical records.
    python scripts/mb_sample.py [dialogs] [--only batched]      (--only batched: the device path alone, for a kernel trace)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from visdial_amd.dataloader import SyntheticDataloader  # noqa: E402
from visdial_amd.native import NativeModel  # noqa: E402
from visdial_amd.opts import default_params, derive  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith('--')]
ONLY_BATCHED = '--only' in sys.argv and sys.argv[sys.argv.index('--only') + 1] == 'batched'
D = int(args[0]) if args and args[0] != 'batched' else 20
V, R = 11322, 10


class Dialogs(object):
    """D synthetic dialogs behind the getIndexData / word2ind / ind2word surface generateAnswers reads"""

    def __init__(self, p, n):
        q = dict(p, batchSize=n)
        self.b = SyntheticDataloader(q, seed=5).getTrainBatch(q)
        self.numThreads = {'val': n}
        self.word2ind = {'<START>': V - 1, '<END>': V}
        self.ind2word = {i: '<START>' if i == V - 1 else '<END>' if i == V else 'w%d' % i for i in range(1, V + 1)}

    def getIndexData(self, inds, params, dtype):
        ix = np.asarray(inds, np.int64) - 1
        return {k: np.ascontiguousarray(self.b[k][ix]) for k in ('ques_fwd', 'hist', 'img_feat')}


p = derive(default_params(encoder='lf-ques-im-hist', decoder='gen', vocabSize=V, embedSize=300, rnnHiddenSize=512, imgFeatureSize=4096,
                          numLayers=2, maxQuesCount=R, maxQuesLen=20, maxAnsLen=20, maxHistoryLenPerRound=40, batchSize=20, gpuid=0))
dl = Dialogs(p, D)
nat = NativeModel(p, init_seed=1)
nat.training(False)
cfg = dict(sampleWords=1, beamLen=20, temperature=1.0, maxThreads=D, seed=1234)
print("lf-ques-im-hist + gen, H %d, V %d, %d layers, sampling, length %d, temperature %g, %d dialogs x %d rounds" % (
    p['rnnHiddenSize'], V, p['numLayers'], cfg['beamLen'], cfg['temperature'], D, R), flush=True)
nat.generateAnswers(dl, 'val', dict(cfg, sampleBatch=20, maxThreads=min(D, 20)))          # warm-up: workspaces, code objects
res = {}
for sb in ((20,) if ONLY_BATCHED else (0, 20)):
    reps = 1 if sb == 0 else 5
    t0 = time.perf_counter()
    for _ in range(reps):
        out = nat.generateAnswers(dl, 'val', dict(cfg, sampleBatch=sb))
    dt = (time.perf_counter() - t0) / reps
    res[sb] = out
    print("sampleBatch %2d: %8.3f s for %d dialogs = %9.2f dialogs/s  (%.2f ms per dialog)" % (sb, dt, D, D / dt, dt / D * 1e3), flush=True)
    res[sb, 't'] = dt
if not ONLY_BATCHED:
    same = sum(a == b for a, b in zip(res[0], res[20]))
    print("speed-up %.1fx; dialogs with identical records: %d of %d" % (res[0, 't'] / res[20, 't'], same, D))
nat.close()
