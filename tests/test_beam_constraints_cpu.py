"""The beam constraints (params beamMinLen / beamNoRepeat / beamLengthPenalty; the rule is C1-C6 at the top of csrc/beam.hip) without a
device: split_eval.beam_banned on hand-written columns, beam_search_round over a table-driven decoder -- a fixed [V x V] table of
log-softmax rows indexed by the last token -- with each property first shown to FAIL without its knob, the length penalty against an
independent pass over the finished set, every refusal, and the frozen C surface."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT
from visdial_amd import split_eval
from visdial_amd.split_eval import SplitEval, beam_banned, beam_search_round, pick_answer

S, E = 41, 42                  # <START>, <END> of the hand-written columns


# ------------------------------------------------------------------------------------------------------------------ C1-C3
def test_minimum_length_bans_end_up_to_step_m():
    col = [S, 5, 6, 7, 0, 0]
    assert beam_banned(col, 3, 3, 0, E) == [E]                    # s = m: a candidate ending here would have m - 1 words
    assert beam_banned(col, 4, 3, 0, E) == []                     # s = m + 1
    assert beam_banned(col, 1, 3, 0, E) == [E]
    assert beam_banned(col, 3, 0, 0, E) == [] and beam_banned(col, 1, 0, 0, E) == []
    assert beam_banned(np.array(col), 3, 3, 1, E) == [5, 6, E]    # both knobs; a numpy column


def test_no_repeat_ngram_bans_what_followed_the_last_words_before():
    col = [S, 5, 6, 5, 0, 0, 0]
    assert beam_banned(col, 4, 0, 1, E) == [5, 6]                 # n = 1: every word of the column
    assert beam_banned(col, 4, 0, 2, E) == [6]                    # p = (5): 5 was followed by 6
    assert beam_banned(col, 3, 0, 2, E) == []                     # p = (6): never seen before
    col = [S, 5, 6, 7, 5, 6, 0]
    assert beam_banned(col, 6, 0, 3, E) == [7]                    # p = (5 6): followed by 7
    assert beam_banned(col, 6, 0, 2, E) == [7]                    # p = (6): followed by 7
    assert beam_banned(col, 5, 0, 3, E) == []                     # p = (7 5)
    assert beam_banned([S, 5, 6, 5, 7, 5, 0], 6, 0, 2, E) == [6, 7]   # two earlier occurrences of p
    # an overlapping repeat: a a a
    assert beam_banned([S, 5, 5, 0, 0, 0], 3, 0, 2, E) == [5]     # p = (5), the window at word 1 is (5) and 5 followed it
    assert beam_banned([S, 5, 5, 5, 0, 0], 4, 0, 3, E) == [5]     # p = (5 5), the window at word 1 overlaps p
    assert beam_banned([S, 5, 5, 0, 0, 0], 3, 0, 3, E) == []      # s = n: only p itself, nothing earlier


def test_zeros_short_columns_and_start():
    # a window or a followed word that is 0 (a slot never filled) is ignored
    assert beam_banned([S, 5, 0, 5, 0, 0], 4, 0, 2, E) == []      # 5 was followed by 0
    assert beam_banned([S, 5, 6, 0, 0, 0], 4, 0, 2, E) == []      # p = (0)
    assert beam_banned([S, 0, 5, 0, 5, 0], 5, 0, 3, E) == []      # p = (0 5), the window (0 5) holds a 0
    assert beam_banned([S, 5, 0, 6, 0, 0], 4, 0, 1, E) == [5, 6]  # n = 1: the words that are there
    # s < n: nothing yet
    assert beam_banned([S, 5, 0, 0, 0, 0], 2, 0, 3, E) == []
    assert beam_banned([S, 0, 0, 0, 0, 0], 1, 0, 2, E) == [] and beam_banned([S, 0, 0, 0, 0, 0], 1, 0, 1, E) == []
    # <START> is never a word: position 0 opens no window and is not banned, even where the model emitted the same id as a word
    assert beam_banned([S, 7, S, 0, 0, 0], 3, 0, 2, E) == []      # p = (S); position 0 followed by 7 does not count
    assert beam_banned([S, 7, 0, 0, 0, 0], 2, 0, 1, E) == [7]
    assert beam_banned([S, S, 7, 0, 0, 0], 3, 0, 2, E) == []
    assert beam_banned([S, S, 7, S, 0, 0], 4, 0, 2, E) == [7]     # ... but the word at position 1 does


# ------------------------------------------------------------------------------------------------------------------ the table
V, K, L, END = 16, 3, 7, 16
SEED = 3
STARTS = range(1, END)


def table(seed=SEED):
    """log-softmax rows of the next word given the last one: peaked, so that greedy continuations loop, <END> likely enough to end
    answers early"""
    rs = np.random.RandomState(seed)
    x = 2.5 * rs.randn(V, V)
    x[:, END - 1] += 2.0
    m = x.max(1, keepdims=True)
    return (x - (m + np.log(np.exp(x - m).sum(1, keepdims=True)))).astype(np.float32)


def step_fn(tab):
    return lambda tokens: np.stack([tab[t - 1] if t != 0 else np.zeros(V, np.float32) for t in tokens])


def search(start, G=1, **kw):
    out = beam_search_round(step_fn(table()), lambda src, n_keep: None, K * G, L, start, END, G, 0.5, **kw)
    return [(np.asarray(t).tolist(), s) for t, s in out]


def words(tokens):
    body = tokens[1:tokens.index(END)] if END in tokens else tokens[1:]
    return [w for w in body if w != 0]


def repeats(ws, n):
    grams = [tuple(ws[i:i + n]) for i in range(len(ws) - n + 1)]
    return len(grams) != len(set(grams))


@pytest.mark.parametrize("G", [1, 3])
def test_explicit_off_values_are_the_defaults(G):
    for start in STARTS:
        assert search(start, G, minLen=0, noRepeat=0, lengthPenalty=0.0) == search(start, G)


@pytest.mark.parametrize("G", [1, 3])
def test_minimum_length(G):
    m = 3
    plain = [a for start in STARTS for a in search(start, G)]
    assert any(END in t and len(words(t)) < m for t, _ in plain)               # the plain search does return shorter answers
    got = [a for start in STARTS for a in search(start, G, minLen=m)]
    assert any(END in t for t, _ in got)
    assert all(len(words(t)) >= m for t, _ in got if END in t)
    assert all(len(words(t)) <= L - 2 for t, _ in search(1, G, minLen=L - 2) if END in t)


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_no_repeat_ngram(G, n):
    # pushed past the short answers the plain search repeats n-grams; with the knob no returned column does
    pushed = [a for start in STARTS for a in search(start, G, minLen=L - 2)]
    assert any(repeats(words(t), n) for t, _ in pushed)
    got = [a for start in STARTS for a in search(start, G, minLen=L - 2, noRepeat=n)]
    assert not any(repeats(words(t), n) for t, _ in got)
    if n > 1:
        assert any(repeats(words(t), n - 1) for t, _ in got)                   # and it bans no more than it says


def test_a_ban_changes_no_other_value():
    """C4 / C5: the score of a constrained answer is the sum of the table's own entries along it"""
    tab = table()
    for start in STARTS:
        for toks, score in search(start, minLen=3, noRepeat=2):
            if END in toks and 0 not in toks[:toks.index(END)]:
                t = toks[:toks.index(END) + 1]
                assert score == sum(float(tab[a - 1, b - 1]) for a, b in zip(t[:-1], t[1:]))


# ------------------------------------------------------------------------------------------------------------------ C6
def finished_set(tab, k, start):
    """the finished candidates of the plain search (rules 1-4 of csrc/beam.hip) in insertion order, as (step, score, column), with
    plain lists and full sorts; the length penalty changes nothing of this"""
    cols, sc, fin = [[start] + [0] * (L - 1) for _ in range(k)], [0.0] * k, []
    for s in range(1, L):
        cands = []
        for w in range(1 if s == 1 else k):
            last = cols[w][s - 1]
            row = tab[last - 1] if last != 0 else np.zeros(V, np.float32)
            for v in sorted(range(V), key=lambda v: (-row[v], v))[:k]:
                col = list(cols[w])
                col[s] = v + 1
                score = sc[w] + float(row[v])
                (fin if v + 1 == END else cands).append((s, score, col))
        order = sorted(range(len(cands)), key=lambda i: (-cands[i][1], i))[:k]
        for i, c in enumerate(order):
            cols[i], sc[i] = cands[c][2], cands[c][1]
    return fin


def c6_choice(fin, alpha):
    """C6 by the letter: per step the highest score, ties to the earliest; across steps x replaces y iff
    x.score * lp[y.len] > y.score * lp[x.len]"""
    lp = [float(s) ** alpha for s in range(L)]
    best = None
    for s in range(1, L):
        here = [c for c in fin if c[0] == s]
        if not here:
            continue
        x = here[0]
        for c in here[1:]:
            if c[1] > x[1]:
                x = c
        if best is None or x[1] * lp[best[0]] > best[1] * lp[x[0]]:
            best = x
    return best


@pytest.mark.parametrize("alpha", [0.7, 1.0, 2.0])
def test_length_penalty_picks_what_c6_picks_among_the_finished_set(alpha):
    tab, changed = table(), 0
    for start in STARTS:
        fin = finished_set(tab, K, start)
        assert fin
        plain = search(start)[0]
        top = max(fin, key=lambda c: c[1])
        assert plain == (top[2], top[1])                                        # the plain search: the highest score
        want = c6_choice(fin, alpha)
        assert search(start, lengthPenalty=alpha)[0] == (want[2], want[1])
        # the comparison without a division is the one on score / length^alpha: exact arithmetic picks the same candidate
        lp = [float(s) ** alpha for s in range(L)]
        exact = max(fin, key=lambda c: Fraction(c[1]) / Fraction(lp[c[0]]))
        assert exact[1:] == want[1:]
        changed += want[2] != plain[0]
        if want[2] != plain[0]:
            assert len(words(want[2])) > len(words(plain[0]))                   # a penalty only ever prefers a longer answer
    assert changed > 0                                                          # without the knob the choice is another one


def test_pick_answer_takes_the_penalty():
    a = ([S, 5, E, 0, 0, 0], -2.0)            # length 2
    b = ([S, 5, 6, 7, E, 0], -3.0)            # length 4
    c = ([S, 5, 6, 7, 8, 9], -0.5)            # unfinished: never the answer while another finished
    assert pick_answer([a, b, c], E) == a and pick_answer([b, a, c], E) == a
    assert pick_answer([a, b, c], E, 1.0) == b and pick_answer([c, b, a], E, 1.0) == b      # -3/4 > -2/2
    assert pick_answer([a, b], E, 0.5) == a                                                 # -3/2 < -2/sqrt(2)
    tie = ([S, 5, 6, 7, E, 0], -4.0)                                                        # -4/4 = -2/2: the lower group
    assert pick_answer([a, tie], E, 1.0) == a and pick_answer([tie, a], E, 1.0) == tie
    assert pick_answer([c, c], E, 1.0) == c


# ------------------------------------------------------------------------------------------------------------------ generateAnswers
def test_generate_answers_applies_the_constraints_on_both_paths():
    from test_diverse_beam_cpu import TableHost, _tiny_val
    p, dl = _tiny_val()

    class Host(TableHost):
        limits, asked = (0, 0, 0.0), []

        def _beam_constraints(self, minLen, noRepeat, lengthPenalty):
            self.asked.append((minLen, noRepeat, lengthPenalty))
            assert (minLen, noRepeat, lengthPenalty) == self.limits

        def _gen_beam(self, beamSize, beamLen, startToken, endToken):
            toks, scores = [], []
            for i in range(len(self.batch['ques_fwd'])):
                self.conv = self._conv(i)
                for it in range(self.batch['ques_fwd'].shape[1]):
                    self._gen_begin(np.full(beamSize, it, np.int32))
                    found = beam_search_round(self._gen_step, self._gen_select, beamSize, beamLen, startToken, endToken, 1, 0.5, *self.limits)
                    toks.append(np.asarray(found[0][0], np.int32))
                    scores.append(found[0][1])
            return np.asarray(toks), np.asarray(scores)

    host = Host(p['vocabSize'])
    host.params = dict(host.params, vocabSize=p['vocabSize'])
    base = dict(beamSize=3, beamLen=6, maxThreads=2)
    plain = host.generateAnswers(dl, 'val', base)
    assert host.generateAnswers(dl, 'val', dict(base, beamMinLen=0, beamNoRepeat=0, beamLengthPenalty=0.0)) == plain
    cfg = dict(base, beamMinLen=3, beamNoRepeat=1, beamLengthPenalty=1.0)
    out = host.generateAnswers(dl, 'val', cfg)
    assert out != plain and not host.asked                                     # the hook is the batched path's
    for d in out:
        for e in d['dialog']:
            ws = [w for w in e['answer'].split() if w not in ('<START>', '<END>')]
            assert len(ws) == len(set(ws)) and ('<END>' not in e['answer'] or len(ws) >= 3), e
    host.limits = (3, 1, 1.0)
    for bb in (1, 2, 3):
        assert host.generateAnswers(dl, 'val', dict(cfg, beamBatch=bb)) == out, bb
    assert host.asked == [(3, 1, 1.0)] * 3
    host.limits = (0, 0, 0.0)
    assert host.generateAnswers(dl, 'val', dict(base, beamBatch=2)) == plain


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_comes_before_any_device_work():
    class Host(SplitEval):
        params = {'decoder': 'gen', 'vocabSize': 30}

    base = dict(beamSize=5, beamLen=8, maxThreads=1)
    for bad, what in ((dict(beamMinLen=-1), 'beamMinLen'), (dict(beamMinLen=1.5), 'beamMinLen'), (dict(beamMinLen='2'), 'beamMinLen'),
                      (dict(beamMinLen=7), 'beamMinLen'),                       # > beamLen - 2
                      (dict(beamNoRepeat=-2), 'beamNoRepeat'), (dict(beamNoRepeat=0.5), 'beamNoRepeat'),
                      (dict(beamLengthPenalty=-1.0), 'beamLengthPenalty'), (dict(beamLengthPenalty=float('nan')), 'beamLengthPenalty'),
                      (dict(beamLengthPenalty=float('inf')), 'beamLengthPenalty'), (dict(beamLengthPenalty='1'), 'beamLengthPenalty'),
                      (dict(beamMinLen=2, sampleWords=1), 'sampleWords'), (dict(beamNoRepeat=2, sampleWords=1), 'sampleWords'),
                      (dict(beamLengthPenalty=1.0, sampleWords=1), 'sampleWords'),
                      (dict(beamMinLen=2, beamSize=20, beamLen=12), 'vocabSize'),       # 30 < 20 + 12 - 1
                      (dict(beamNoRepeat=2, beamSize=20, beamLen=12), 'vocabSize'),
                      (dict(beamMinLen=2, beamBatch=2), '-host native'), (dict(beamNoRepeat=1, beamBatch=2), '-host native'),
                      (dict(beamLengthPenalty=0.5, beamBatch=2), '-host native')):
        with pytest.raises(ValueError, match=what):
            Host().generateAnswers(None, 'val', dict(base, **bad))
    for kw, what in ((dict(minLen=-1), 'beamMinLen'), (dict(minLen=L - 1), 'beamMinLen'), (dict(noRepeat=-1), 'beamNoRepeat'),
                     (dict(lengthPenalty=-0.5), 'beamLengthPenalty'), (dict(lengthPenalty=float('nan')), 'beamLengthPenalty')):
        with pytest.raises(ValueError, match=what):
            beam_search_round(None, None, K, L, 1, END, **kw)
    with pytest.raises(ValueError, match='vocabSize'):                          # V = 16 < 12 + 7 - 1: a row could run out of words
        beam_search_round(step_fn(table()), lambda src, n_keep: None, 12, L, 1, END, minLen=2)
    beam_search_round(step_fn(table()), lambda src, n_keep: None, 12, L, 1, END, lengthPenalty=1.0)      # no ban: nothing to refuse


def test_the_operator_level_host_refuses_the_batched_search_and_names_the_native_host():
    from visdial_amd.model import Model
    with pytest.raises(ValueError, match='-host native'):
        Model._beam_constraints(None, 3, 0, 0.0)
    with pytest.raises(ValueError, match='-host native'):
        Model._beam_constraints(None, 0, 2, 0.0)
    with pytest.raises(ValueError, match='-host native'):
        Model._beam_constraints(None, 0, 0, 1.0)
    Model._beam_constraints(None, 0, 0, 0.0)


def test_generate_py_takes_the_flags_and_refuses_what_the_library_would():
    import generate
    a = generate.parse_args(['-loadPath', 'x', '-minLen', '3', '-noRepeatNgram', '2', '-lengthPenalty', '0.7'])
    assert (a['minLen'], a['noRepeatNgram'], a['lengthPenalty']) == (3, 2, 0.7)
    a = generate.parse_args(['-loadPath', 'x', '-beamSize', '6', '-beamGroups', '3', '-minLen', '1'])       # combines with groups
    assert (a['minLen'], a['beamGroups']) == (1, 3)
    a = generate.parse_args(['-loadPath', 'x'])
    assert (a['minLen'], a['noRepeatNgram'], a['lengthPenalty']) == (0, 0, 0.0)
    for bad in (['-minLen', '-1'], ['-noRepeatNgram', '-1'], ['-lengthPenalty', '-0.5'], ['-lengthPenalty', 'nan'],
                ['-lengthPenalty', 'inf'], ['-beamLen', '6', '-minLen', '5'], ['-minLen', '2', '-sampleWords', '1'],
                ['-noRepeatNgram', '2', '-sampleWords', '1'], ['-lengthPenalty', '1', '-sampleWords', '1']):
        with pytest.raises(ValueError):
            generate.parse_args(['-loadPath', 'x'] + bad)
    for bad in (['-minLen', '1.5'], ['-noRepeatNgram', 'x']):                  # argparse's own refusal of a non-integer
        with pytest.raises(SystemExit):
            generate.parse_args(['-loadPath', 'x'] + bad)


def test_the_c_surface_is_where_it_was_and_the_variables_are_documented():
    from visdial_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'visdial_hip.h')).read()
    assert re.search(r'^#define\s+VD_ABI_VERSION\s+2\s*$', header, re.M) and _lib.ABI_VERSION == 2
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    names = set(re.findall(r'\b(vd_[a-z0-9_]+)\s*\(', code))
    assert len(names) == 101 and '101 entry points' in header and names == set(_lib.PROTOTYPES)
    assert not {'vd_beam_topk_ban_p', 'vd_beam_advance_lp_p'} & names          # internal to the library
    runtime = open(os.path.join(ROOT, 'visdial_amd', 'csrc', 'rt_switches.h')).read()
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for var in ('VD_BEAM_MIN_LEN', 'VD_BEAM_NO_REPEAT', 'VD_BEAM_LENGTH_PENALTY'):
        assert var in header and var in runtime and var in integration
    assert 'VD_BEAM_LMAX' in header
    assert 'VD_BEAM' not in open(os.path.join(ROOT, 'lua', 'visdial_ffi.lua')).read()   # the Lua host is out of scope
    kernels = open(os.path.join(ROOT, 'visdial_amd', 'csrc', 'beam.hip')).read()
    assert all('//  C%d. ' % i in kernels for i in range(1, 7)) and 'C1-C6' in split_eval.beam_search_round.__doc__
