"""Diverse beam search (params beamGroups = G > 1, beamDiversity = lambda; the rule is D1-D7 at the top of csrc/beam.hip) without a
device: split_eval.beam_search_round driven by a table-driven fake decoder -- a deterministic log-probability row per token prefix
-- against an independent brute-force restatement, the properties that follow from the rule, the containment fact the device search
rests on, every refusal, and the frozen C surface."""
import os
import re
import zlib

import numpy as np
import pytest

from conftest import ROOT
from visdial_amd import split_eval
from visdial_amd.split_eval import SplitEval, beam_search_round, pick_answer

V, L, START, END = 40, 8, 1, 2
GRID = [(4, 2, 0.5), (6, 3, 0.5), (6, 6, 1e4), (12, 3, 0.3), (32, 8, 0.5), (32, 2, 0.5)]
SEEDS = range(6)


class TableDecoder(object):
    """A decoder whose state is the token prefix since the last reset.  A token-0 step returns an all-zero row and resets the state
    whatever it was (maskZero); any other step returns log_softmax of logits drawn from a generator seeded by (seed, prefix), <END>
    made likely enough that groups run short of unfinished candidates.  Odd seeds quantise the logits, so rows have ties."""

    def __init__(self, seed, vocab=V):
        self.seed, self.vocab, self.rows, self.zero_rows = seed, vocab, {}, 0

    def advance(self, state, tok):
        if tok == 0:
            return np.zeros(self.vocab, np.float32), ('reset',)
        state = state + (int(tok),)
        if state not in self.rows:
            rs = np.random.RandomState(zlib.crc32(repr((self.seed, state)).encode()))
            x = 2.0 * rs.randn(self.vocab)
            x[END - 1] += 2.5
            if self.seed % 2:
                x = np.round(x * 2.0) / 2.0
            m = x.max()
            self.rows[state] = (x - (m + np.log(np.exp(x - m).sum()))).astype(np.float32)
        return self.rows[state], state

    # the host's device steps: _gen_begin / _gen_step / _gen_select
    def begin(self, k):
        self.cur = [()] * k

    def step(self, tokens):
        assert len(tokens) == len(self.cur)
        out = [self.advance(s, t) for s, t in zip(self.cur, tokens)]
        self.zero_rows += sum(1 for t in tokens if t == 0)
        self.stepped = [s for _, s in out]
        return np.stack([r for r, _ in out])

    def select(self, src, n_keep):
        cur = list(self.cur)
        for i in range(n_keep):
            cur[i] = self.stepped[src[i]]
        self.cur = cur


def search(seed, k, G, lam, vocab=V):
    dec = TableDecoder(seed, vocab)
    dec.begin(k)
    out = beam_search_round(dec.step, dec.select, k, L, START, END, G, lam)
    return [(np.asarray(t).tolist(), s) for t, s in out], dec


def brute_force(seed, k, G, lam):
    """D1-D7 restated with plain lists: the whole row is penalised, every order is a full sort by (value descending, position
    ascending), every slot carries its own decoder state and an untouched slot keeps its PRE-step one."""
    dec = TableDecoder(seed)
    kp = k // G
    cols, sc, st = [[START] + [0] * (L - 1) for _ in range(k)], [0.0] * k, [()] * k
    fin = [[] for _ in range(G)]
    for s in range(1, L):
        stepped = [dec.advance(st[i], cols[i][s - 1]) for i in range(k)]
        count = [0] * V
        ncols, nsc, nst = list(cols), list(sc), list(st)
        for g in range(G):
            cands = []
            for w in range(g * kp, g * kp + (1 if s == 1 else kp)):
                row = stepped[w][0]
                a = [np.float32(row[v]) - np.float32(lam) * np.float32(count[v]) for v in range(V)]
                for v in sorted(range(V), key=lambda v: (-a[v], v))[:kp]:
                    col = list(cols[w])
                    col[s] = v + 1
                    score, key = sc[w] + float(row[v]), sc[w] + float(a[v])
                    if v + 1 == END:
                        fin[g].append((score, col))
                    else:
                        cands.append((key, score, col, w))
            order = sorted(range(len(cands)), key=lambda i: (-cands[i][0], i))
            for i, c in enumerate(order[:kp]):
                _, score, col, w = cands[c]
                ncols[g * kp + i], nsc[g * kp + i], nst[g * kp + i] = col, score, stepped[w][1]
                count[col[s] - 1] += 1
        cols, sc, st = ncols, nsc, nst
    out = []
    for g in range(G):
        best = None
        for score, col in fin[g]:
            if best is None or score > best[1]:
                best = (col, score)
        out.append(best if best is not None else (cols[g * kp], sc[g * kp]))
    return out


def todays_loop(dec, beamSize, beamLen, startToken, endToken):
    """the per-dialog search of one round as generateAnswers had it before the search became a function"""
    beams = np.zeros((beamLen, beamSize), np.int64)
    beams[0] = startToken
    scores = np.zeros(beamSize)
    finish = []
    for step in range(1, beamLen):
        exploreSize = 1 if step == 1 else beamSize
        logp = dec.step(beams[step - 1])
        cands = []
        for wordId in range(exploreSize):
            top = np.argsort(-logp[wordId], kind='stable')[:beamSize]
            for cid in top:
                cb = beams[:, wordId].copy()
                cb[step] = cid + 1
                sc = scores[wordId] + float(logp[wordId, cid])
                if cid + 1 == endToken:
                    finish.append(dict(beam=cb, length=step + 1, score=sc))
                else:
                    cands.append(dict(score=sc, beam=cb, src=wordId))
        cands.sort(key=lambda a: -a['score'])
        keep = cands[:beamSize]
        if keep:
            dec.select(np.array([c['src'] for c in keep], np.int32), len(keep))
        for i, c in enumerate(keep):
            beams[:, i] = c['beam']
            scores[i] = c['score']
    finish.sort(key=lambda a: -a['score'])
    return (finish[0]['beam'], finish[0]['score']) if finish else (beams[:, 0], scores[0])


@pytest.mark.parametrize("k,G,lam", GRID)
def test_the_search_function_equals_the_brute_force_restatement(k, G, lam):
    zero_rows = 0
    for seed in SEEDS:
        got, dec = search(seed, k, G, lam)
        assert len(got) == G
        assert got == brute_force(seed, k, G, lam), seed              # tokens and fp64 scores, exactly
        zero_rows += dec.zero_rows
    assert zero_rows > 0                                              # some slot ran dry: all-zero rows were searched and penalised


def test_the_inputs_hold_all_zero_rows_and_ties():
    for k, G, lam in GRID:
        assert sum(search(seed, k, G, lam)[1].zero_rows for seed in SEEDS) > 0, (k, G)
    _, dec = search(1, 6, 3, 0.5)
    assert any(len(np.unique(r)) < V for r in dec.rows.values())


@pytest.mark.parametrize("k,G", [(k, G) for k, G, _ in GRID])
def test_without_a_penalty_every_group_is_the_plain_search_of_its_slots(k, G):
    for seed in SEEDS:
        plain, _ = search(seed, k // G, 1, 0.5)
        grouped, _ = search(seed, k, G, 0.0)
        assert grouped == plain * G, seed                             # bit for bit


def test_one_slot_groups_under_a_large_penalty_hold_different_words():
    several = 0
    for seed in range(20):
        got, _ = search(seed, 6, 6, 1e4)
        words = []
        for tokens, _ in got:
            body = tokens[1:tokens.index(END)] if END in tokens else tokens[1:]
            words.append({p: t for p, t in enumerate(body) if t != 0})
        for p in range(L):
            at_p = [w[p] for w in words if p in w]
            assert len(at_p) == len(set(at_p)), (seed, p, got)
        several += len({tuple(t) for t, _ in got}) > 1
    assert several > 0


class RecordingDecoder(TableDecoder):
    """a TableDecoder that keeps the (src, n_keep) of every select call"""

    def begin(self, k):
        TableDecoder.begin(self, k)
        self.selects = []

    def select(self, src, n_keep):
        self.selects.append((np.asarray(src).tolist(), n_keep))
        TableDecoder.select(self, src, n_keep)


def test_one_group_is_todays_loop():
    for seed in SEEDS:
        for k in (1, 3, 5):
            dec = RecordingDecoder(seed)
            dec.begin(k)
            beam, score = todays_loop(dec, k, L, START, END)
            got, _ = search(seed, k, 1, 0.5)
            assert got == [(beam.tolist(), score)], (seed, k)
            dec2 = RecordingDecoder(seed)
            dec2.begin(k)
            (t3, s3), = beam_search_round(dec2.step, dec2.select, k, L, START, END)      # the knobs default to off
            assert (np.asarray(t3).tolist(), s3) == got[0]
            assert dec2.selects == dec.selects and dec.selects, (seed, k)                # the kept prefix, and only when there is one
    assert any(n_keep < k for _, n_keep in dec.selects)                                  # an <END> among step 1's k candidates keeps k - 1


def test_pick_answer_is_d7():
    fin, open_ = [START, 5, END, 0], [START, 5, 6, 7]
    assert pick_answer([(open_, -0.1), (fin, -3.0), (fin[:1] + [9, END, 0], -2.0)], END) == ([START, 9, END, 0], -2.0)
    assert pick_answer([(fin, -2.0), (open_, -1.0), ([START, 9, END, 0], -2.0)], END) == (fin, -2.0)      # ties to the lower group
    assert pick_answer([(open_, -5.0), ([START, 8, 8, 8], -1.0)], END) == (open_, -5.0)                   # nothing finished: group 0


def test_the_top_of_a_penalised_row_lies_within_the_unpenalised_top_k():
    """what lets the device search reuse one top-k at the full k: re-ranking the unpenalised row's top k by the penalised values
    gives the penalised row's top k', ties and all-zero rows included"""
    rs = np.random.RandomState(11)
    for trial in range(3000):
        k, G, lam = GRID[trial % len(GRID)]
        kp = k // G
        kind = trial % 3
        if kind == 0:
            row = rs.randn(V).astype(np.float32)
        elif kind == 1:
            row = (np.round(rs.randn(V) * 2.0) / 2.0).astype(np.float32)        # ties
        else:
            row = np.zeros(V, np.float32)                                        # a slot whose token is 0
        order = np.argsort(-row, kind='stable')
        count = np.zeros(V, np.int64)
        # the words of the earlier groups' (G - 1) k' slots: likely ones, repeats allowed, never <END>
        for v in rs.choice(order[:k], size=rs.randint(0, (G - 1) * kp + 1)):
            count[v] += v + 1 != END
        a = row - np.float32(lam) * count.astype(np.float32)
        full = np.argsort(-a, kind='stable')[:kp]
        top = order[:k]
        rerank = top[np.lexsort((top, -a[top]))][:kp]                            # value descending, index ascending
        assert np.array_equal(full, rerank), (trial, k, G)


# ---------------------------------------------------------------------------------------------------------------- generateAnswers
class TableHost(SplitEval):
    """generateAnswers over the table decoder: no device"""

    def __init__(self, vocab):
        self.params, self.vocab = {'decoder': 'gen'}, vocab

    def _set_training(self, flag):
        pass

    def _gen_encode(self, batch):
        self.batch = batch
        self.conv = self._conv(0)

    def _conv(self, i):
        return int(np.asarray(self.batch['ques_fwd'][i]).sum()) + 7 * int(np.asarray(self.batch['hist'][i]).sum())

    def _gen_begin(self, rounds):
        self.dec = TableDecoder(1000 * self.conv + int(rounds[0]), self.vocab)
        self.dec.begin(len(rounds))

    def _gen_step(self, tokens):
        return self.dec.step(tokens)

    def _gen_select(self, src, n_keep):
        self.dec.select(src, n_keep)

    # a "device" search of every round of the chunk, in the layout of NativeModel._gen_beam
    grouping = (1, 0.5)

    def _beam_grouping(self, groups, diversity):
        assert (groups, diversity) == self.grouping

    def _gen_beam(self, beamSize, beamLen, startToken, endToken):
        G, lam = self.grouping
        toks, scores = [], []
        for i in range(len(self.batch['ques_fwd'])):
            self.conv = self._conv(i)
            for it in range(self.batch['ques_fwd'].shape[1]):
                self._gen_begin(np.full(beamSize, it, np.int32))
                found = beam_search_round(self._gen_step, self._gen_select, beamSize, beamLen, startToken, endToken, G, lam)
                toks.append([np.asarray(t, np.int32) for t, _ in found])
                scores.append([s for _, s in found])
        toks, scores = np.asarray(toks), np.asarray(scores)
        return (toks, scores) if G > 1 else (toks[:, 0], scores[:, 0])


def _tiny_val():
    from test_beam_cpu import _tiny_val as tiny
    return tiny()


def test_generate_answers_adds_the_groups_answers_and_leaves_one_group_as_it_was():
    p, dl = _tiny_val()
    host = TableHost(p['vocabSize'])
    base = dict(beamSize=6, beamLen=6, maxThreads=2)
    plain = host.generateAnswers(dl, 'val', base)
    assert host.generateAnswers(dl, 'val', dict(base, beamGroups=1, beamDiversity=0.7)) == plain
    assert all(set(e) == {'question', 'answer'} for d in plain for e in d['dialog'])
    out = host.generateAnswers(dl, 'val', dict(base, beamGroups=3))
    assert out == host.generateAnswers(dl, 'val', dict(base, beamGroups=3, beamDiversity=0.5))            # the default
    assert [d['image_id'] for d in out] == [d['image_id'] for d in plain]
    differ = 0
    for d, d0 in zip(out, plain):
        for e, e0 in zip(d['dialog'], d0['dialog']):
            assert e['question'] == e0['question'] and len(e['answers']) == 3 and e['answer'] in e['answers']
            differ += len(set(e['answers'])) > 1
    assert differ > 0
    # the chunked path (beamBatch > 0) over a host whose search returns [N x G x beamLen] / [N x G] writes the same records
    host.grouping = (3, 0.5)
    for bb in (1, 2, 3):
        assert host.generateAnswers(dl, 'val', dict(base, beamGroups=3, beamBatch=bb)) == out, bb
    host.grouping = (1, 0.5)
    assert host.generateAnswers(dl, 'val', dict(base, beamBatch=2)) == plain


def test_every_refusal_comes_before_any_device_work():
    class Host(SplitEval):
        params = {'decoder': 'gen'}

    for bad, what in ((dict(beamGroups=0), 'beamGroups'), (dict(beamGroups=-2), 'beamGroups'), (dict(beamGroups=4), 'beamGroups'),
                      (dict(beamGroups=3, beamDiversity=-0.5), 'beamDiversity'),
                      (dict(beamGroups=3, beamDiversity=float('inf')), 'beamDiversity'),
                      (dict(beamGroups=3, beamDiversity=float('nan')), 'beamDiversity'),
                      (dict(beamGroups=3, sampleWords=1), 'beamGroups'),
                      (dict(beamGroups=3, beamBatch=2), '-host native')):
        with pytest.raises(ValueError, match=what):
            Host().generateAnswers(None, 'val', dict(dict(beamSize=6, maxThreads=1), **bad))
    with pytest.raises(ValueError, match='beamGroups'):
        beam_search_round(None, None, 6, L, START, END, 4, 0.5)
    with pytest.raises(ValueError, match='beamDiversity'):
        beam_search_round(None, None, 6, L, START, END, 3, -1.0)


def test_generate_py_takes_the_flags_and_refuses_what_the_library_would():
    import generate
    a = generate.parse_args(['-loadPath', 'x', '-beamSize', '6', '-beamGroups', '3', '-beamDiversity', '0.25'])
    assert a['beamGroups'] == 3 and a['beamDiversity'] == 0.25
    a = generate.parse_args(['-loadPath', 'x'])
    assert a['beamGroups'] == 1 and a['beamDiversity'] == 0.5
    for bad in (['-beamGroups', '0'], ['-beamSize', '6', '-beamGroups', '4'], ['-beamSize', '6', '-beamGroups', '3', '-beamDiversity', '-1'],
                ['-beamSize', '6', '-beamGroups', '3', '-sampleWords', '1']):
        with pytest.raises(ValueError):
            generate.parse_args(['-loadPath', 'x'] + bad)


def test_the_c_surface_is_where_it_was():
    from visdial_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'visdial_hip.h')).read()
    lua = open(os.path.join(ROOT, 'lua', 'visdial_ffi.lua')).read()
    assert re.search(r'^#define\s+VD_ABI_VERSION\s+2\s*$', header, re.M) and _lib.ABI_VERSION == 2
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    names = set(re.findall(r'\b(vd_[a-z0-9_]+)\s*\(', code))
    assert len(names) == 101 and '101 entry points' in header
    assert names == set(_lib.PROTOTYPES) == set(re.findall(r"^\s+'(vd_[a-z0-9_]+)',$", lua, re.M))
    assert 'vd_beam_advance_grouped_p' not in names                  # internal to the library: not in the header, not extern "C"
    runtime = open(os.path.join(ROOT, 'visdial_amd', 'csrc', 'rt_switches.h')).read()
    for var in ('VD_BEAM_GROUPS', 'VD_BEAM_DIVERSITY'):
        assert var in header and var in runtime
    assert 'VD_BEAM' not in lua                                      # the Lua host is out of scope
    assert split_eval.beam_search_round.__doc__ and 'D1-D7' in open(os.path.join(ROOT, 'visdial_amd', 'csrc', 'beam.hip')).read()
