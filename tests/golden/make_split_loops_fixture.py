"""Writes tests/golden/split_loops.json: what the split-level loops of visdial_amd/split_eval.py (SplitEval.evaluate / retrieve / predict /
generateAnswers) return, print, tally and ask of their host, over a numpy stand-in host with no device and no library.  The file was
recorded once, before the loops were folded, and is NOT regenerated from later code: tests/test_split_loops_cpu.py replays `run_cases()`
and compares everything exactly, the ordered list of host calls included -- equal call lists mean no device work was added or dropped.

The stand-in: a decoder whose log-probability row is a fixed function of (the round's question and history rows 0 .. r, the token prefix),
a `retrieveBatch` whose score is a fixed function of (the round's history or question row, the candidate's tokens), and a loader that
serves one fixed draw of `SyntheticDataloader` in sequential batches (trimmed, as the real loader trims) and by dialog index.
Shapes: 3 dialogs, R = 3, O = 5, vocabulary 12, beamSize 4, beamLen 5, batchSize 2 -- the last batch is ragged.

    python tests/golden/make_split_loops_fixture.py
"""
import contextlib
import io
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from visdial_amd.dataloader import SyntheticDataloader                                   # noqa: E402
from visdial_amd.split_eval import SplitEval, beam_search_round, truncated_weights         # noqa: E402

V, R, O, N_DIALOGS = 12, 3, 5, 3
START, END = V - 1, V
BEAM = dict(beamSize=4, beamLen=5)
CREATED = dict(_beam_grouping=(1, 0.5), _beam_constraints=(0, 0, 0.0), _beam_rollout=(0,), _sample_truncation=(0, 1.0))     # a device's defaults
ENCODERS = dict(row=dict(encoder='hre-ques-hist', useHistory=True, concatHistory=False),
                concat=dict(encoder='lf-ques-hist', useHistory=True, concatHistory=True),
                nohist=dict(encoder='lf-ques-im', useHistory=False, concatHistory=True))


def params(kind, decoder, **more):
    p = dict(decoder=decoder, vocabSize=V, maxQuesCount=R, numOptions=O, batchSize=2, maxQuesLen=4, maxAnsLen=3, maxHistoryLenPerRound=8,
             maxHistoryLen=4, imgFeatureSize=4)
    p.update(ENCODERS[kind])
    p.update(more)
    return p


def trimmed(a):
    """a right-aligned token array without the leading columns that are zero in every row (at least one column stays)"""
    live = np.flatnonzero(a.reshape(-1, a.shape[-1]).any(0))
    return np.ascontiguousarray(a[..., min(int(live[0]) if live.size else a.shape[-1] - 1, a.shape[-1] - 1):])


class Loader(SyntheticDataloader):
    """one fixed draw of N_DIALOGS dialogs, served as `getTestBatch` / `getIndexData` serve a split; dialog 2 has two rounds only"""

    def __init__(self, p, seed=7):
        SyntheticDataloader.__init__(self, p, seed=seed, num_threads=N_DIALOGS)
        self.full = self.getTrainBatch(p, batch_size=N_DIALOGS)
        if p['decoder'] == 'gen':
            self.add_gen_options(self.full, N_DIALOGS)
        if 'hist' in self.full:
            self.data = {s: {'hist': self.full['hist']} for s in ('val', 'test')}
        for s in ('val', 'test'):
            setattr(self, 'unique_img_' + s, [11, 12, 13])
            setattr(self, s + '_num_rounds', np.array([3, 2, 3]))
        self.ind2word = {i: '<START>' if i == START else '<END>' if i == END else 'w%d' % i for i in range(1, V + 1)}
        self.word2ind = {w: i for i, w in self.ind2word.items()}

    def _dialogs(self, idx):
        f, n = self.full, N_DIALOGS
        out = {}
        for k, a in f.items():
            if k in ('options', 'answer_ind'):                   # one row per round
                a = a.reshape((n, R) + a.shape[1:])[idx]
                out[k] = np.ascontiguousarray(a.reshape((-1,) + a.shape[2:]))
            else:
                out[k] = trimmed(a[idx]) if k in ('ques_fwd', 'hist') else np.ascontiguousarray(a[idx])
        return out

    def getTestBatch(self, start_id, p, dtype='val'):
        nxt = min(start_id + int(p['batchSize']), self.numThreads[dtype] + 1)
        return self._dialogs(np.arange(start_id - 1, nxt - 1)), nxt

    def getIndexData(self, convIds, p, dtype='val'):
        return self._dialogs(np.asarray(convIds, np.int64) - 1)


def shape_of(a):
    if isinstance(a, dict):
        return sorted([k, list(np.shape(v))] for k, v in a.items())
    if isinstance(a, np.ndarray):
        return list(a.shape)
    return a.item() if isinstance(a, np.generic) else a


def nonzero(row):
    row = np.asarray(row, np.int64).reshape(-1)
    return row[row != 0].tobytes()


def logp_row(key, prefix):
    """log_softmax of logits drawn from (key, prefix), <END> made likely; odd keys quantise the logits, so their rows have ties"""
    rs = np.random.RandomState(zlib.crc32(repr((key, prefix)).encode()))
    x = 2.0 * rs.randn(V)
    x[END - 1] += 1.5
    if key % 2:
        x = np.round(x * 2.0) / 2.0
    m = x.max()
    return (x - (m + np.log(np.exp(x - m).sum()))).astype(np.float32)


class Host(SplitEval):
    """the stand-in host; `calls` is the ordered list of the host methods the loops called, with the shapes of their arguments.
    device: the knobs this host's device search / sampler was "created with" (None: the refusals of SplitEval itself)"""

    def __init__(self, p, device=None):
        self.params, self.device, self.calls = dict(p), device, []

    def _log(self, name, *args):
        self.calls.append([name] + [shape_of(a) for a in args])

    def _set_training(self, on):
        pass

    # ------------------------------------------------------------------ the table-driven decoder
    def _gen_encode(self, batch):
        self._log('_gen_encode', batch)
        q = batch['ques_fwd']
        self.keys = [zlib.crc32(nonzero(q[b, r]) + b'|' + b'|'.join(nonzero(h) for h in batch['hist'][b, :r + 1]) if 'hist' in batch
                                else nonzero(q[b, r]) + b'|%d' % r) for b in range(q.shape[0]) for r in range(q.shape[1])]

    def _begin(self, rounds):
        self.cur = [(self.keys[int(r)], ()) for r in rounds]

    def _step(self, tokens):
        assert len(tokens) == len(self.cur)
        self.stepped = [(k, ('reset',)) if int(t) == 0 else (k, pre + (int(t),)) for (k, pre), t in zip(self.cur, tokens)]
        return np.stack([np.zeros(V, np.float32) if int(t) == 0 else logp_row(*s) for s, t in zip(self.stepped, tokens)])

    def _select(self, src, n_keep):
        for i, s in enumerate([self.stepped[int(j)] for j in src[:n_keep]]):
            self.cur[i] = s

    def _gen_begin(self, rounds):
        self._log('_gen_begin', np.asarray(rounds))
        self._begin(rounds)

    def _gen_step(self, tokens):
        self._log('_gen_step', np.asarray(tokens))
        return self._step(tokens)

    def _gen_select(self, src, n_keep):
        self._log('_gen_select', np.asarray(src), n_keep)
        self._select(src, n_keep)

    def _asked(self, name, *knobs):
        self._log(name, *knobs)
        if self.device is None:
            return getattr(SplitEval, name)(self, *knobs)
        if name != '_beam_grouping' or knobs[0] > 1 or self._made(name)[0] > 1:     # (one group: the diversity is not looked at)
            if tuple(knobs) != self._made(name):
                raise ValueError('stand-in: %s%r, created with %r' % (name, tuple(knobs), self._made(name)))

    def _made(self, name):
        return tuple(self.device.get(name, CREATED[name]))

    def _beam_grouping(self, groups, diversity):
        self._asked('_beam_grouping', groups, diversity)

    def _beam_constraints(self, minLen, noRepeat, lengthPenalty):
        self._asked('_beam_constraints', minLen, noRepeat, lengthPenalty)

    def _beam_rollout(self, rollout):
        self._asked('_beam_rollout', rollout)

    def _sample_truncation(self, topK, topP):
        self._log('_sample_truncation', topK, topP)
        if self.device is None or (topK, topP) != self._made('_sample_truncation'):
            raise ValueError('stand-in: _sample_truncation%r' % ((topK, topP),))

    def _gen_beam(self, beamSize, beamLen, startToken, endToken):
        """every round of the last `_gen_encode` batch, in the layout of NativeModel._gen_beam"""
        self._log('_gen_beam', beamSize, beamLen, startToken, endToken)
        G, lam = self._made('_beam_grouping')
        toks, scores = [], []
        for n in range(len(self.keys)):
            self._begin(np.full(beamSize, n))
            found = beam_search_round(self._step, self._select, beamSize, beamLen, startToken, endToken, G, lam,
                                      *self._made('_beam_constraints'))
            toks.append([np.asarray(t, np.int32) for t, _ in found])
            scores.append([s for _, s in found])
        toks, scores = np.asarray(toks), np.asarray(scores)
        return (toks, scores) if G > 1 else (toks[:, 0], scores[:, 0])

    def _gen_sample(self, beamLen, startToken, endToken, temperature, uniforms):
        self._log('_gen_sample', beamLen, startToken, endToken, temperature, uniforms)
        topK, topP = self._made('_sample_truncation')
        N = len(self.keys)
        assert uniforms.shape == (beamLen, N)
        out = np.zeros((N, beamLen + 1), np.int32)
        out[:, 0] = startToken
        loglik = np.zeros(N)
        for r in range(N):
            for s in range(1, beamLen + 1):
                lp = logp_row(self.keys[r], tuple(int(t) for t in out[r, :s]))
                w = truncated_weights(lp, temperature, topK, topP)
                c = min(int(np.searchsorted(np.cumsum(w), uniforms[s - 1, r] * w.sum(), side='right')), int(np.nonzero(w > 0)[0][-1]))
                loglik[r] += float(lp[c])
                out[r, s] = c + 1
        return out, loglik

    # ------------------------------------------------------------------ retrieval and loss
    def retrieveBatch(self, batch):
        self._log('retrieveBatch', batch, bool(self.params['useGt']))
        B, R_ = batch['ques_fwd'].shape[:2]
        N = B * R_
        cands = np.asarray(batch['options'] if 'options' in batch else batch['option_in'], np.int64).reshape(N, O, -1)
        rows = np.asarray(batch['hist'] if 'hist' in batch else batch['ques_fwd'], np.int64).reshape(N, -1)
        rows = [r[r != 0] for r in rows]                             # (a batch's width is its own)
        key = np.array([int(np.dot(r, np.arange(1, r.size + 1) ** 2)) for r in rows])
        tok = cands @ (np.arange(1, cands.shape[2] + 1) ** 3)
        self.scores = np.sin(0.37 * key[:, None] + 1.3 * tok).astype(np.float32)      # equal tokens -> equal scores
        self.last = (len(set(map(bytes, cands.reshape(N * O, -1)))), N * O)
        order = np.argsort(-self.scores, axis=1, kind='stable')
        ranks = np.empty((N, O), np.int32)
        np.put_along_axis(ranks, order, np.arange(1, O + 1, dtype=np.int32)[None, :], axis=1)
        if self.params['useGt']:
            return ranks[np.arange(N), np.asarray(batch['answer_ind']).reshape(-1) - 1]
        return ranks

    def option_rows(self):
        return self.last

    def forwardBackward(self, batch, onlyForward=False):
        self._log('forwardBackward', batch, onlyForward)
        return float(int(np.asarray(batch['ques_fwd'], np.int64).sum()) % 97) / 8.0


def dense_annotations():
    rel = lambda *v: np.array(v, np.float64)
    return {(11, 2): rel(0.4, 0.0, 1.0, 0.4, 0.2),              # ties
            (12, 1): rel(0.0, 0.0, 0.0, 0.0, 0.0),              # no relevant candidate
            (12, 3): rel(0.2, 0.2, 0.2, 0.2, 0.2),              # a round dialog 12 does not have
            (13, 3): rel(0.0, 0.6, 0.0, 0.0, 0.0),              # k = 1, in the ragged batch
            (99, 1): rel(1.0, 0.0, 0.0, 0.0, 0.0)}              # an image outside the split


def plain(v):
    """JSON's view of a value"""
    if isinstance(v, dict):
        return {str(k): plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    if isinstance(v, np.ndarray):
        return v.tolist()
    return v.item() if isinstance(v, np.generic) else v


def run(method, p, args=(), device=None, dense=False, loader=None, dtype='val'):
    dl = loader(p) if loader else Loader(p)
    host = Host(p, device)
    if dense:
        host.denseAnnotations = dense_annotations()
    out = io.StringIO()
    rec = {}
    try:
        with contextlib.redirect_stdout(out):
            rec['result'] = getattr(host, method)(dl, dtype, *args)
    except (ValueError, SystemExit) as e:
        rec['error'] = [type(e).__name__, str(e)]
    rec.update(stdout=out.getvalue(), optionCacheRows=host.optionCacheRows, lhoodTreeStats=host.lhoodTreeStats, rolloutRows=host.rolloutRows,
               rolloutCut=host.rolloutCut, ndcgRows=host.ndcgRows, ndcg=getattr(host, 'ndcg', None), calls=host.calls)
    return plain(rec)


def run_cases():
    cases = {}
    concat = dict(rollout=1, rolloutHistory='concat', rolloutConcatEnd=END)
    for method in ('retrieve', 'predict'):
        cases[method + ' plain'] = run(method, params('row', 'disc'))
        cases[method + ' rollout'] = run(method, params('row', 'disc', rollout=1))
        cases[method + ' rollout concat'] = run(method, params('concat', 'disc', **concat))
        cases[method + ' dense'] = run(method, params('row', 'disc'), dense=True)
        cases[method + ' rollout dense'] = run(method, params('row', 'disc', rollout=1), dense=True)
        cases[method + ' no history'] = run(method, params('nohist', 'disc'))
        cases[method + ' rollout no history'] = run(method, params('nohist', 'disc', **concat))
        cases[method + ' optionCache'] = run(method, params('row', 'disc', optionCache=1))
        cases[method + ' gen lhood tree'] = run(method, params('row', 'gen', fusedLhood=2))
        cases[method + ' gen lhood tree optionCache dense'] = run(method, params('concat', 'gen', fusedLhood=2, optionCache=1), dense=True)
    cases['predict test dense'] = run('predict', params('row', 'disc'), dense=True, dtype='test')
    cases['retrieve rollout, a loader without data'] = run('retrieve', params('row', 'disc', rollout=1),
                                                           loader=lambda p: SyntheticDataloader(p, seed=5, num_threads=N_DIALOGS))
    cases['evaluate disc'] = run('evaluate', params('row', 'disc'))
    cases['evaluate gen'] = run('evaluate', params('row', 'gen'))
    for name, bad in (('rollout 2 + optionCache', dict(rollout=2, optionCache=1)),
                      ('optionCache + concatHistory', dict(rollout=1, optionCache=1)),
                      ('concatHistory', dict(rollout=1)),
                      ('concat without <END>', dict(rollout=1, rolloutHistory='concat')),
                      ('concat on a per-round encoder', dict(rollout=1, rolloutHistory='concat', concatHistory=False))):
        cases['retrieve refuses: ' + name] = run('retrieve', params('concat', 'disc', **bad))
    cases['retrieve refuses: gen rollout on this host'] = run('retrieve', params('row', 'gen', rollout=1))

    def gen(kind='row', device=None, **knobs):
        return run('generateAnswers', params(kind, 'gen'), (dict(BEAM, **knobs),), device)
    limits = dict(beamMinLen=2, beamNoRepeat=2, beamLengthPenalty=0.7)
    for kind in ('row', 'concat', 'nohist'):
        cases['generate %s beamBatch 0' % kind] = gen(kind)
        cases['generate %s rollout' % kind] = gen(kind, rollout=1)
    cases['generate beamBatch 2'] = gen(device={}, beamBatch=2)
    cases['generate maxThreads 2 seed'] = gen(maxThreads=2, seed=5)
    cases['generate beamGroups 2'] = gen(beamGroups=2)
    cases['generate beamGroups 2 diversity penalty'] = gen(beamGroups=2, beamDiversity=1.5, beamLengthPenalty=0.7)
    cases['generate beamGroups 2 beamBatch 2'] = gen(device=dict(_beam_grouping=(2, 0.5)), beamGroups=2, beamBatch=2)
    cases['generate beamGroups 2 beamBatch 2 penalty'] = gen(
        device=dict(_beam_grouping=(2, 0.5), _beam_constraints=(0, 0, 0.7)), beamGroups=2, beamBatch=2, beamLengthPenalty=0.7)
    cases['generate constraints'] = gen(**limits)
    cases['generate constraints beamBatch 2'] = gen(device=dict(_beam_constraints=(2, 2, 0.7)), beamBatch=2, **limits)
    cases['generate rollout constraints'] = gen(rollout=1, **limits)
    cases['generate rollout beamBatch 2'] = gen(device=dict(_beam_rollout=(1,)), rollout=1, beamBatch=2)
    cases['generate sampleWords'] = gen(sampleWords=1, temperature=0.8, seed=11)
    cases['generate sampleWords topK topP'] = gen(sampleWords=1, temperature=0.8, seed=11, topK=5, topP=0.7)
    cases['generate sampleWords sampleBatch 2'] = gen(device={}, sampleWords=1, temperature=0.8, seed=11, sampleBatch=2)
    cases['generate sampleWords sampleBatch 2 topK topP'] = gen(device=dict(_sample_truncation=(5, 0.7)), sampleWords=1, temperature=0.8,
                                                                 seed=11, sampleBatch=2, topK=5, topP=0.7)
    # parameters that break two rules get the message of the earlier check; one pair per adjacent pair of checks that can be broken
    # together (sampling against a rule that needs beam search cannot)
    cases['generate refuses: disc'] = run('generateAnswers', params('row', 'disc'), (dict(BEAM, beamBatch=2, sampleWords=1),))
    for name, bad in (('beamBatch with sampling + bad topK', dict(beamBatch=2, sampleWords=1, topK=-1)),
                      ('sampleBatch without sampling + topK', dict(sampleBatch=2, topK=3)),
                      ('topK without sampling + bad topK', dict(topK=-1)),
                      ('bad topP + truncation the sampler lacks', dict(sampleWords=1, topP=2.0, sampleBatch=2)),
                      ('truncation the sampler lacks + bad groups', dict(sampleWords=1, topK=3, sampleBatch=2, beamGroups=3)),
                      ('bad groups + groups with sampling', dict(beamGroups=3, sampleWords=1)),
                      ('bad diversity + groups with sampling', dict(beamGroups=2, beamDiversity=-1.0, sampleWords=1)),
                      ('groups with sampling + bad minLen', dict(beamGroups=2, sampleWords=1, beamMinLen=-1)),
                      ('bad minLen + constraints with sampling', dict(beamMinLen=9, sampleWords=1)),
                      ('vocabulary too small + constraints with sampling', dict(beamSize=8, beamLen=6, beamNoRepeat=2, sampleWords=1)),
                      ('constraints with sampling + rollout 2', dict(beamMinLen=1, sampleWords=1, rollout=2)),
                      ('rollout 2 + rollout with sampling', dict(rollout=2, sampleWords=1)),
                      ('rollout 2 + groups', dict(rollout=2, beamGroups=2)),
                      ('rollout with sampling', dict(rollout=1, sampleWords=1)),
                      ('rollout with groups + device groups', dict(rollout=1, beamGroups=2, beamBatch=2)),
                      ('device groups + device constraints', dict(beamBatch=2, beamGroups=2, beamMinLen=1)),
                      ('device constraints + device rollout', dict(beamBatch=2, beamMinLen=1, rollout=1)),
                      ('device rollout', dict(beamBatch=2, rollout=1))):
        cases['generate refuses: ' + name] = gen(**bad)
    return cases


def main():
    with open(os.path.join(HERE, 'split_loops.json'), 'w') as f:
        json.dump(run_cases(), f, sort_keys=True, separators=(',', ':'))
        f.write('\n')


if __name__ == '__main__':
    main()
