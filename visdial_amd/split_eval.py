"""Split-level loops of the reference's Model (model.lua:109-246, 432-613) shared by both hosts: Model:evaluate (validation loss /
perplexity), Model:retrieve (ground-truth ranks + R@k / MRR) and Model:predict (all 100 ranks per round) over the
sequential batches of `dataloader:getTestBatch`.  A host provides `params`, `_set_training(bool)`,
`forwardBackward(batch, onlyForward=True)` and `retrieveBatch(batch)` (ranks per `params['useGt']`); for
Model:generateAnswers the four device steps `_gen_encode(batch)`, `_gen_begin(rounds)`, `_gen_step(tokens) -> logp`,
`_gen_select(src, n_keep)` (= vd_model_encode / decode_begin / decode_step / decode_select of the model-level ABI), and for the
batched beam search (params beamBatch > 0) `_gen_beam(beamSize, beamLen, startToken, endToken) -> (tokens [N x beamLen], scores
[N])` over every round of the last `_gen_encode` batch (= vd_model_beam_search; the operator-level host composes the vd_beam_*
kernels), and for batched sampling (params sampleBatch > 0) `_gen_sample(beamLen, startToken, endToken, temperature, uniforms
[beamLen x N]) -> (tokens [N x (beamLen + 1)], log-likelihoods [N])` (= vd_model_sample; vd_sample_* for the operator-level host), with
`_sample_truncation(topK, topP)` raising unless that sampler truncates with exactly these knobs.  Diverse beam search (params
beamGroups = G > 1): `_beam_grouping(groups, diversity)` raises unless that `_gen_beam` searches in exactly these groups, and it then
returns every group's answer, (tokens [N x G x beamLen], scores [N x G]).  Beam constraints (params beamMinLen / beamNoRepeat /
beamLengthPenalty): `_beam_constraints(minLen, noRepeat, lengthPenalty)` raises unless that `_gen_beam` searches under exactly these.
Rollout (params rollout = 1): `_beam_rollout(rollout)` raises unless that `_gen_beam` feeds every round's answer into the next round's
history on the device, R1-R6 below.  Ranking on a rollout (params rollout = 1 of retrieve / predict; evaluate.py -rollout 1): E1-E5 below
and `retrieve_rollout_batch`, over the host's own `retrieveBatch`; a host with a device rollout overrides it."""
import collections
import math
import types

import numpy as np

from . import utils


def truncated_weights(logp, temperature, topK=0, topP=1.0):
    """The sampling weights of ONE row of fp32 log-probabilities under top-k / nucleus truncation: the rule the per-dialog loop below
    applies and the device sampler (csrc/sample.hip, T1-T4) is held to.
      1. w[c] = exp(float64(logp[c]) / temperature)
      2. candidate order: logp descending as fp32 values, equal values by ascending index
      3. topK > 0: the first min(topK, V) of that order stay
      4. topP < 1: S_k = the fp64 sum of w over what 3. kept; the shortest prefix of the order whose running sum is >= topP * S_k
         stays -- at least one column, and none with w == 0 unless there is nothing else (every weight underflowed: the draw fails
         as it does without truncation)
      5. every other column gets weight 0.
    topK = 0 with topP = 1 returns w of 1. untouched.  The weights are not normalised; the drawn token's log-likelihood is its
    UNtruncated logp."""
    topK, topP = int(topK), float(topP)
    if topK < 0 or not (0.0 < topP <= 1.0):
        raise ValueError('topK = %r must be an integer >= 0 (0 = off) and topP = %r a real in (0, 1] (1 = off)' % (topK, topP))
    lp = np.asarray(logp, np.float32).reshape(-1)
    w = np.exp(lp.astype(np.float64) / temperature)
    if topK == 0 and topP == 1.0:
        return w
    order = np.argsort(-lp, kind='stable')
    n = min(topK, w.size) if topK > 0 else w.size
    if topP < 1.0:
        cum = np.cumsum(w[order[:n]])
        reach = int(np.searchsorted(cum, topP * cum[-1], side='left')) + 1     # the first prefix whose sum is >= topP * S_k
        n = max(1, min(reach, n, int((w[order[:n]] > 0).sum())))
    out = np.zeros_like(w)
    out[order[:n]] = w[order[:n]]
    return out


def check_beam_groups(beamSize, groups, diversity):
    """the refusals of diverse beam search (csrc/beam.hip D1-D7): G >= 1 divides beamSize, lambda (unused at G = 1) is a finite real >= 0"""
    if groups < 1 or beamSize % groups != 0:
        raise ValueError('beamGroups = %d must be >= 1 and divide beamSize = %d' % (groups, beamSize))
    if groups > 1 and not (np.isfinite(np.float32(diversity)) and diversity >= 0.0):     # applied in fp32
        raise ValueError('beamDiversity = %r must be a finite real >= 0' % (diversity,))


def check_beam_constraints(beamSize, beamLen, minLen, noRepeat, lengthPenalty, vocabSize=None):
    """the refusals of the beam constraints (csrc/beam.hip C1-C6): minLen and noRepeat are integers >= 0, lengthPenalty a finite real
    >= 0 (0 = off each); minLen <= beamLen - 2, because <END> must be allowed at the last step; while a ban is on a row must keep
    beamSize unbanned words: vocabSize >= beamSize + beamLen - 1 (checked where the vocabulary is known)"""
    for name, v in (('beamMinLen', minLen), ('beamNoRepeat', noRepeat)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
            raise ValueError('%s = %r must be an integer >= 0 (0 = off)' % (name, v))
    if isinstance(lengthPenalty, (bool, str)) or not (np.isfinite(lengthPenalty) and lengthPenalty >= 0.0):
        raise ValueError('beamLengthPenalty = %r must be a finite real >= 0 (0 = off)' % (lengthPenalty,))
    if minLen > 0 and minLen > beamLen - 2:
        raise ValueError('beamMinLen = %d exceeds beamLen - 2 = %d: <END> must be allowed at the last step' % (minLen, beamLen - 2))
    if (minLen > 0 or noRepeat > 0) and vocabSize is not None and vocabSize < beamSize + beamLen - 1:
        raise ValueError('beamMinLen = %d / beamNoRepeat = %d need vocabSize = %d >= beamSize + beamLen - 1 = %d, so that a row never '
                         'runs out of unbanned words' % (minLen, noRepeat, vocabSize, beamSize + beamLen - 1))


def check_rollout(value):
    """params rollout as 0 / 1 (None = 0), for generateAnswers and for retrieve / predict"""
    rollout = int(value or 0)
    if rollout not in (0, 1):
        raise ValueError('rollout = %r must be 0 or 1' % (value,))
    return rollout


def beam_banned(column, step, minLen, noRepeat, endToken):
    """C1-C3 of csrc/beam.hip: the tokens (1-based ids, ascending) a slot with this column may not take at step `step`.  The words of
    the column are positions 1 .. step-1 (position 0, <START>, is not a word); an n-gram that holds a 0 is ignored.  minLen = m: <END>
    is banned at every step <= m.  noRepeat = n >= 1, once step >= n: with p the last n - 1 words, every word that followed an earlier
    occurrence of p is banned (n = 1: every word of the column)."""
    banned = set()
    if step <= minLen:
        banned.add(int(endToken))
    n = int(noRepeat)
    if n >= 1 and step >= n:
        g = [int(t) for t in column[:step]]                       # g[i] = word i for i >= 1
        p = g[step - n + 1:step]
        if 0 not in p:
            for i in range(1, step - n + 1):
                if g[i:i + n - 1] == p and g[i + n - 1] != 0:
                    banned.add(g[i + n - 1])
    return sorted(banned)


def length_penalty_table(beamLen, lengthPenalty):
    """C6: lp[s] = s^alpha for the lengths s < beamLen, in fp64 over libm's pow, as the library builds the table it uploads"""
    return [float(s) ** float(lengthPenalty) for s in range(beamLen)]


def beam_replaces(x_score, x_len, y_score, y_len, lp):
    """C6: a finished candidate x of another length replaces the incumbent y iff x.score / x.len^alpha > y.score / y.len^alpha, decided
    without a division: one fp64 product on either side"""
    return x_score * lp[y_len] > y_score * lp[x_len]


def best_finished(finish, lp):
    """C6 over a finished set in insertion order (dicts with `score` and `step`, the length): per step the best by score, ties to the
    earliest; across steps `beam_replaces` against the incumbent, ties staying with it.  None if nothing finished."""
    best = None
    for step in sorted(set(c['step'] for c in finish)):
        x = None
        for c in finish:
            if c['step'] == step and (x is None or c['score'] > x['score']):
                x = c
        if best is None or beam_replaces(x['score'], x['step'], best['score'], best['step'], lp):
            best = x
    return best


def pick_answer(answers, endToken, lengthPenalty=0.0):
    """D7: the round's answer among its groups' (tokens, score): the highest score of the groups that finished something (a finished
    answer holds <END>, a slot's column never does), ties to the lower group; group 0's if none finished.  lengthPenalty > 0 (C6): a
    later group's answer replaces the incumbent by `beam_replaces`, its length the position of <END>."""
    best = None
    lp = None
    for tokens, score in answers:
        toks = np.asarray(tokens).tolist()
        if endToken not in toks:
            continue
        if best is None:
            best = (tokens, score)
        elif lengthPenalty > 0.0:
            lp = lp or length_penalty_table(len(toks), lengthPenalty)
            if beam_replaces(score, toks.index(endToken), best[1], np.asarray(best[0]).tolist().index(endToken), lp):
                best = (tokens, score)
        elif score > best[1]:
            best = (tokens, score)
    return best if best is not None else answers[0]


# Rollout (csrc/beam.hip R1-R6; generate.py -rollout 1): round r is answered on a history that holds the model's OWN answers to the rounds
# before it.  Th = the width of the batch's history, lq = the number of non-zero tokens of a question row.
#   R1. round 0's history row is the batch's (the caption).
#   R2. for r >= 1, history row r = the non-zero tokens of question row r - 1, in order, then the first min(la, Th - lq) words of the answer
#       chosen for round r - 1, right-aligned in Th columns with zeros in front (lq = 0 and no words: all zeros).
#   R3. an answer's words are entries 1, 2, ... of its token row [beamLen] up to but excluding the first <END> or 0; entry 0 is <START>; an
#       answer that never finished gives all its beamLen - 1 words.
#   R4. the answer chosen for a round is what the search returns for it, under whatever constraints are in force (groups are refused).
#   R5. round r is answered from an encoder pass that holds rows 0 .. r as above; rows > r do not reach it (every encoder is causal).
#   R6. the batch's history rows >= 1 are ignored and overwritten: after the run the batch holds the generated rows.
def rollout_history_row(ques_row, answer_row, Th, endToken):
    """R2 / R3: the history row [Th] that follows a round with question row `ques_row` and answer token row `answer_row`"""
    q = [int(t) for t in np.asarray(ques_row).reshape(-1) if int(t) != 0]
    if len(q) > Th:
        raise ValueError('rollout: a question of %d tokens does not fit a history row of Th = %d' % (len(q), Th))
    words = []
    for t in np.asarray(answer_row).reshape(-1)[1:]:
        if int(t) == int(endToken) or int(t) == 0:
            break
        words.append(int(t))
    row = q + words[:Th - len(q)]
    out = np.zeros(Th, np.int64)
    if row:
        out[Th - len(row):] = row
    return out



# Rollout on a concatenated history (csrc/beam.hip CH1-CH6; evaluate.py -rollout 1 -rolloutHistory concat): the encoders whose history row is the
# running concatenation of the dialog (lf-ques-hist, lf-ques-im-hist, lf-att-ques-im-hist; dataloader.lua:243-255).  W = the width of the
# batch's history, END = the <END> token id.
#   CH1. row 0 is the batch's (R1).
#   CH2. lenH(r) = W - (the index of the first non-zero column of row r), 0 for an all-zero row; the last lenH columns of row r are its
#        tokens, carried over as they are (a 0 among them included).
#   CH3. the new tokens of round r are END, then the non-zero tokens of question row r in order, then the answer's words (R3 for a beam
#        answer, E2 / E3 for a picked candidate).  END is appended even when the question is empty and there are no words, as the loader does
#        for the missing rounds of the test split.
#   CH4. row r + 1 = row r's lenH tokens followed by the first min(n_new, W - lenH) new tokens, right-aligned in W columns with zeros in
#        front.  What does not fit is cut at the END of the new tokens: words first, then question tokens, then END; a full row repeats
#        itself.  (The reference's loader has no such case: it would index out of range.)  Every row is a prefix extension of the one before.
#   CH5. R5, R6 and E5 hold as written: an lf encoder reads only its own row.
#   CH6. prefix property: the history stack's state after row r + 1 is its state after row r continued over the kept new tokens.
def rollout_concat_new(ques_row, answer_row, endToken, answerEnd):
    """CH3: the new tokens of a round with question row `ques_row` and answer token row `answer_row` (entry 0 stands in <START>'s place, the
    words end at the first `answerEnd` or 0: answerEnd = END for a beam answer, 0 for a `rollout_candidate_row`)"""
    new = [int(endToken)] + [int(t) for t in np.asarray(ques_row).reshape(-1) if int(t) != 0]
    for t in np.asarray(answer_row).reshape(-1)[1:]:
        if int(t) == int(answerEnd) or int(t) == 0:
            break
        new.append(int(t))
    return new


def rollout_concat_len(row):
    """CH2: lenH of a history row [W]"""
    nz = np.flatnonzero(np.asarray(row).reshape(-1))
    return int(np.asarray(row).size - nz[0]) if nz.size else 0


def rollout_concat_row(prev_row, ques_row, answer_row, endToken, answerEnd, cut=None):
    """CH2 - CH4: the concatenated history row [W] that follows `prev_row` [W] after a round with question row `ques_row` and answer token
    row `answer_row`.  `cut` (a list): gains True if CH4 cut a new token, else False."""
    prev = np.asarray(prev_row).reshape(-1)
    W, lenH = prev.size, rollout_concat_len(prev_row)
    new = rollout_concat_new(ques_row, answer_row, endToken, answerEnd)
    keep = new[:W - lenH]
    if cut is not None:
        cut.append(len(keep) < len(new))
    row = [int(t) for t in prev[W - lenH:]] + keep
    out = np.zeros(W, np.int64)
    out[W - len(row):] = row
    return out


# Ranking on a rollout (csrc/beam.hip E1-E5; evaluate.py -rollout 1): the candidates of round r of a discriminative model are ranked on a
# history that holds the model's own picks for the rounds before it.  O = numOptions, To = the width of an `options` row.
#   E1. round 0's history row is the batch's (R1).
#   E2. the answer chosen for round r is the candidate that the rank computation (vd_ranks) gives rank 1 among the round's O scores: the
#       highest score, among equal scores the lowest index.
#   E3. a candidate's words are entries 0, 1, ... of its `options` row [To] up to but excluding the first 0: the rows are left-aligned and
#       hold neither <START> nor <END>; an all-zero row is an empty answer.
#   E4. history row r + 1 is R2 of question row r and those words (the question whole, the first min(la, Th - lq) words, right-aligned).
#   E5. R5 and R6 hold: round r is scored from a pass in which rows 0 .. r are final; the batch's rows >= 1 are ignored and overwritten.
#       The pass after the last append scores every round as its own pass did (rows <= r are final after pass r, the encoders are causal).
# For decoder gen the answer fed back is the beam search's (R4): an evaluation then describes the dialogs generate.py -rollout 1 writes.
def rollout_candidate_row(option_row):
    """E3: an `options` row [To] as the answer token row `rollout_history_row` takes, with endToken = 0: an entry in <START>'s place
    (which is never a word), then the words up to the first 0"""
    words = []
    for t in np.asarray(option_row).reshape(-1):
        if int(t) == 0:
            break
        words.append(int(t))
    return np.array([0] + words + [0], np.int64)


def rollout_pick(ranks_row):
    """E2: the 0-based index of the candidate with rank 1 in one round's ranks [O] (a permutation of 1 .. O: ties went to the lower index
    when the ranks were computed)"""
    first = np.flatnonzero(np.asarray(ranks_row).reshape(-1) == 1)
    if first.size != 1:
        raise ValueError('rollout: %d candidates of a round have rank 1; the ranks of a round are a permutation of 1 .. O' % first.size)
    return int(first[0])


def rollout_picked_history(batch, picks, concat=False, endToken=None, cut=None):
    """E1 / E4: the history [B x R x Th] of `batch` (ques_fwd [B x R x Tq], hist [B x R x Th], options [B * R x O x To]) when round r of
    every dialog was answered with candidate picks[dialog * R + r]: row 0 is the batch's, rows >= 1 are rebuilt.  concat: by CH1 - CH4 with
    <END> = endToken instead of E4 (`cut` as `rollout_concat_row`)"""
    answers = [rollout_candidate_row(batch['options'][n, int(pick)]) for n, pick in enumerate(picks)]
    return rollout_answered_history(batch, answers, 0, endToken if concat else 0, cut)


def rollout_next_row(prev_row, ques_row, answer_row, Th, answerEnd, concatEnd=0, cut=None):
    """the one step of every rollout: the history row [Th] that follows `prev_row` after a round with question row `ques_row` and answer
    token row `answer_row`, whose words end at the first `answerEnd` or 0 (<END> for a beam answer, 0 for a `rollout_candidate_row`).
    concatEnd = 0: R2 / E4, one row per round (`prev_row` is not read); concatEnd = the <END> id: CH2 - CH4, `cut` as `rollout_concat_row`"""
    if concatEnd:
        return rollout_concat_row(prev_row, ques_row, answer_row, concatEnd, answerEnd, cut)
    return rollout_history_row(ques_row, answer_row, Th, answerEnd)


def rollout_answered_history(batch, answers, answerEnd, concatEnd=0, cut=None):
    """the history [B x R x Th] of `batch` (ques_fwd [B x R x Tq], hist [B x R x Th]) when round r of every dialog was answered with the
    token row answers[dialog * R + r]: row 0 is the batch's, rows >= 1 are rebuilt by `rollout_next_row`"""
    B, R, Th = batch['hist'].shape
    hist = np.array(batch['hist'])
    for i in range(B):
        for r in range(R - 1):
            hist[i, r + 1] = rollout_next_row(hist[i, r], batch['ques_fwd'][i, r], answers[i * R + r], Th, answerEnd, concatEnd, cut)
    return hist


def beam_search_round(step_fn, select_fn, k, L, start, end, groups=1, diversity=0.5, minLen=0, noRepeat=0, lengthPenalty=0.0):
    """The beam search of ONE round on the host (model.lua:466-573): `step_fn(tokens [k]) -> logp [k x V]` is one decoder step of the k
    slots (a slot whose token is 0 gets an all-zero row), `select_fn(src, n_keep)` makes slot i < n_keep continue from the stepped
    state of slot src[i]; the slots start from the round's encoder state (`_gen_begin`).  Returns one (tokens [L], score) per group.
    groups = 1 is the reference's search (rules 1-4 of csrc/beam.hip); groups = G > 1 is diverse beam search with Hamming diversity
    `diversity`, D1-D7 there: group g owns slots g k' .. g k' + k' - 1 (k' = k / G), the groups of a step run in order, a group's row
    is penalised in fp32 by diversity * (the number of earlier groups' slots filled with that word at this step), the penalised
    values pick and order the candidates (the key), the unpenalised sum is the score that is carried and reported.
    minLen / noRepeat / lengthPenalty are the constraints C1-C6 there, each off at 0: a banned word (`beam_banned` of the slot's column)
    counts as -inf in the explored row, every other value and every score is untouched; with a length penalty the best finished
    candidate is `best_finished`'s instead of the highest-scoring one."""
    check_beam_groups(k, groups, diversity)
    check_beam_constraints(k, L, minLen, noRepeat, lengthPenalty)
    ban = minLen > 0 or noRepeat > 0
    lp = length_penalty_table(L, lengthPenalty) if lengthPenalty > 0.0 else None

    def unbanned(row, column, step):
        """C4: the explored row with its banned words at -inf"""
        if row.shape[0] < k + L - 1:
            raise ValueError('beamMinLen = %d / beamNoRepeat = %d need vocabSize = %d >= beamSize + beamLen - 1 = %d'
                             % (minLen, noRepeat, row.shape[0], k + L - 1))
        banned = beam_banned(column, step, minLen, noRepeat, end)
        if not banned:
            return row
        row = np.array(row, np.float32)
        row[np.asarray(banned) - 1] = -np.inf
        return row
    beamSize, beamLen, startToken, endToken = k, L, start, end
    beams = np.zeros((beamLen, beamSize), np.int64)
    beams[0] = startToken
    scores = np.zeros(beamSize)
    # groups = 1 is one group of k slots whose key IS the score: nothing is penalised, and `step_fn`'s rows are taken as they come
    kp, lam, penalise = beamSize // groups, np.float32(diversity), groups > 1
    finish = [[] for _ in range(groups)]
    for step in range(1, beamLen):
        exploreSize = 1 if step == 1 else kp                              # all beams are <START> at first (D3)
        logp = step_fn(beams[step - 1])
        if penalise:
            logp = np.asarray(logp, np.float32)
            count = np.zeros(logp.shape[1], np.int64)                     # D2: from zero at every step
        # An untouched slot (D6) names itself: `select_fn` fills a prefix of the slots, and the state such a slot holds is never
        # observed -- its next token is 0, and a token-0 step zeroes the state whatever it was (maskZero)
        src = np.arange(beamSize, dtype=np.int32)
        for g in range(groups):
            base = g * kp
            cands = []
            for w in range(base, base + exploreSize):
                a = logp[w]
                if penalise:
                    a = a - lam * count.astype(np.float32)                # D4: fp32, product and difference rounded separately
                if ban:
                    a = unbanned(np.asarray(a), beams[:, w], step)        # C4: a penalty leaves -inf where it is
                for cid in np.argsort(-a, kind='stable')[:kp]:            # torch.topk(..., true)
                    cb = beams[:, w].copy()
                    cb[step] = cid + 1                                    # vocabulary ids are 1-based
                    sc = scores[w] + float(logp[w, cid])                  # D5: the true log-likelihood
                    if cid + 1 == endToken:
                        finish[g].append(dict(beam=cb, score=sc, step=step))
                    else:
                        cands.append(dict(key=scores[w] + float(a[cid]) if penalise else sc, score=sc, beam=cb, src=w))
            cands.sort(key=lambda c: -c['key'])                           # D6 (stable; Lua's table.sort is not)
            keep = cands[:kp]
            for i, c in enumerate(keep):
                beams[:, base + i] = c['beam']
                scores[base + i] = c['score']
                src[base + i] = c['src']
                if penalise:
                    count[c['beam'][step] - 1] += 1
        if penalise:
            select_fn(src, beamSize)
        elif keep:                                                        # the reference's call: the kept prefix, if there is one
            select_fn(src[:len(keep)], len(keep))
    out = []
    for g in range(groups):                                               # D7
        if lp is not None and finish[g]:                                  # C6
            best = best_finished(finish[g], lp)
            out.append((best['beam'], best['score']))
            continue
        finish[g].sort(key=lambda c: -c['score'])
        # (the reference errors if none ended)
        out.append((finish[g][0]['beam'], finish[g][0]['score']) if finish[g] else (beams[:, g * kp], scores[g * kp]))
    return out


class SplitEval(object):
    optionCacheRows = (0, 0)     # params optionCache: (rows the option LSTM ran, candidate rows) summed over the last retrieve / predict
    # params fusedLhood = 2: nodes of the prefix trees, live (candidate, step) rows, rows the tree recurrence ran, (step, candidate) rows
    # of the batches, summed over the last retrieve / predict
    lhoodTreeStats = dict(nodes=0, live=0, executed=0, total=0)

    rolloutRows = (0, 0)         # params rollout: (history rows that differ from the ground truth's, history rows) of the last retrieve / predict
    rolloutCut = 0               # params rolloutHistory = 'concat': the generated history rows CH4 cut, of the last retrieve / predict

    # dense annotations ({(image_id, round_id): relevance}, dense.load_dense_annotations) a host was given: retrieve / predict then also
    # compute the NDCG of every annotated round from the final scores of its batch (csrc/loss.hip DT2) and leave it in `ndcgRows`
    # [dialogs x R] (-1: no relevant candidate, -2: not annotated); None = no NDCG, every printed number and record as ever
    denseAnnotations = None
    ndcgRows = None

    def _ndcg_of_batch(self, batch, rel):
        """NDCG [N] of the scores the last retrieval of `batch` left, on the host (dense.ndcg_rows); the native host overrides it with
        the device kernel"""
        from . import dense
        s = self.scores
        s = s.detach().cpu().numpy() if hasattr(s, 'detach') else np.asarray(s)
        return dense.ndcg_rows(s.reshape(rel.shape), rel)

    def _ndcg_report(self, dataloader, dtype, ranks, ndcg):
        """after the metrics: NDCG over the annotated rounds that have one, and the counts (none of it without denseAnnotations); `ndcg`:
        the NDCG rows of the batches of `_rank_split`, `ranks` what it returned"""
        self.ndcgRows = None
        if self.denseAnnotations is None:
            return
        from . import dense
        n, R = ranks.shape[:2]
        rows = np.concatenate(ndcg).reshape(n, R) if ndcg else np.full((n, R), dense.NOT_ANNOTATED)
        rounds = getattr(dataloader, dtype + '_num_rounds', None)
        if rounds is not None:                                     # rounds that do not exist carry no annotation
            rows[np.arange(R)[None, :] >= np.asarray(rounds).reshape(-1, 1)[:n]] = dense.NOT_ANNOTATED
        self.ndcgRows = rows
        mean, annotated, left_out = dense.ndcg_mean(rows)
        ids = set(int(i) for i in (getattr(dataloader, 'unique_img_' + dtype, None) or []))
        outside = sum(1 for (iid, _) in self.denseAnnotations if iid not in ids)
        print('NDCG: %.6f\t(%d annotated rounds in %s, %d of them without a relevant candidate left out; %d annotations of images outside '
              'the split)' % (mean, annotated, dtype, left_out, outside))
        self.ndcg = dict(ndcg=mean, annotated=annotated, left_out=left_out, outside=outside)

    def _rollout(self):
        """params rollout (0 / 1) of retrieve / predict, refusing what cannot be ranked on a rollout"""
        rollout = check_rollout(self.params.get('rollout'))
        if rollout and int(self.params.get('optionCache', 0) or 0):
            raise ValueError('rollout = 1 with optionCache: a cached batch carries only the candidates the cache did not hold, and the '
                             'rollout reads a picked candidate\'s tokens from the batch; combining the two is left for a follow-up')
        concat = self.params.get('rolloutHistory') == 'concat'
        if rollout and self.params.get('concatHistory') and self.params.get('useHistory') and not concat:
            raise ValueError("rollout = 1 with encoder '%s' (concatHistory): its history row is the running concatenation of the rounds, "
                             "and E4 describes the per-round row only; params rolloutHistory = 'concat' (with rolloutConcatEnd = the <END> "
                             "id) rolls out by the concatenation rule CH1-CH6" % self.params.get('encoder'))
        if rollout and concat and self.params.get('useHistory'):
            if not self.params.get('concatHistory'):
                raise ValueError("rollout = 1 with rolloutHistory = 'concat' and encoder '%s': its history is one row per round (E4), not the "
                                 "running concatenation" % self.params.get('encoder'))
            self._concat_end()
        return rollout

    def _concat_end(self):
        """the <END> id of CH3 if this host rolls out on a concatenated history (params rolloutHistory = 'concat'), else 0"""
        if self.params.get('rolloutHistory') != 'concat' or not (self.params.get('useHistory') and self.params.get('concatHistory')):
            return 0
        end = int(self.params.get('rolloutConcatEnd') or 0)
        if end < 1 or end > int(self.params.get('vocabSize', end)):
            raise ValueError("rolloutHistory = 'concat' needs params rolloutConcatEnd = the <END> token id in [1, vocabSize], got %r"
                             % (self.params.get('rolloutConcatEnd'),))
        return end

    def _all_ranks(self, batch):
        """the host's own retrieval of every candidate's rank, [N x O], whatever params useGt says"""
        keep = self.params.get('useGt')
        self.params['useGt'] = False
        try:
            ranks = np.asarray(self.retrieveBatch(batch))
        finally:
            self.params['useGt'] = keep
        return ranks.reshape(batch['ques_fwd'].shape[0] * batch['ques_fwd'].shape[1], -1)

    def retrieve_rollout_batch(self, batch):
        """E1-E5 on the host, the obviously-right path (like beamBatch = 0): R retrievals of the whole batch; before call r + 1 history row
        r + 1 of every dialog is rewritten IN `batch` from the rank-1 candidate of round r in call r (E2 - E4; params rolloutHistory =
        'concat': CH1 - CH4 with <END> = params rolloutConcatEnd); round r's ranks are those of call r.  `batch` carries `options` (decoder disc) and the history at its untrimmed width.  Returns all ranks [N x O]; a batch
        without a history is ranked once, as ever."""
        if 'hist' not in batch:
            return self._all_ranks(batch)
        if 'options' not in batch:
            raise ValueError("rollout = 1 on this host ranks the candidates of decoder 'disc'; for decoder 'gen' the rollout is the beam "
                             "search's and runs in the model-level runtime: use -host native (visdial_amd.native.NativeModel)")
        B, R, Th = batch['hist'].shape
        end = self._concat_end()                                           # CH1 - CH4 instead of E4
        out = None
        for r in range(R):
            ranks = self._all_ranks(batch)
            out = np.array(ranks) if out is None else out
            out[r::R] = ranks[r::R]
            if r + 1 < R:
                for i in range(B):
                    cand = rollout_candidate_row(batch['options'][i * R + r, rollout_pick(ranks[i * R + r])])
                    batch['hist'][i, r + 1] = rollout_next_row(batch['hist'][i, r], batch['ques_fwd'][i, r], cand, Th, 0, end)
        return out

    def _test_batch(self, dataloader, start, dtype, rollout):
        """`getTestBatch`; under a rollout with the history at its UNTRIMMED width (as `rollout_batch`) and a copy of the ground truth's"""
        batch, nxt = dataloader.getTestBatch(start, self.params, dtype)
        if rollout and 'hist' in batch:
            data = getattr(dataloader, 'data', None)
            if data is not None:
                batch['hist'] = np.ascontiguousarray(data[dtype]['hist'][start - 1:nxt - 1]).astype(np.int32)
            batch['hist'] = np.array(batch['hist'])
            batch['hist_gt'] = np.array(batch['hist'])
        return batch, nxt

    def _ranked(self, batch, tally, rollout, image_ids):
        """retrieveBatch + the tally (a Counter: `update` ADDS) of the answer-encoding cache (params optionCache; decoder disc) and of the
        prefix trees.  rollout: `retrieve_rollout_batch`, the ground-truth ranks taken from all ranks if params useGt, + the tally of the
        history rows that differ from the ground truth's.  Returns (ranks, the NDCG [N] of the batch's rounds or None); `image_ids`: the
        batch's dialogs"""
        if rollout:
            truth = batch.pop('hist_gt', None)
            ranks = np.asarray(self.retrieve_rollout_batch(batch))
            if truth is not None:
                cut = []
                hist = self.rollout_history(batch, ranks, cut)
                tally.update(differ=int((hist != truth).any(2).sum()), rows=hist.shape[0] * hist.shape[1], cut=int(sum(cut)))
        else:
            ranks = np.asarray(self.retrieveBatch(batch))
        if int(self.params.get('fusedLhood', 0) or 0) == 2:
            from . import prefix_tree
            st = prefix_tree.stats(batch['option_in'])
            ex, tot = self.option_rows()
            tally.update(nodes=st['nodes'], live=st['live'], executed=ex, total=tot)
        if int(self.params.get('optionCache', 0) or 0):
            ex, tot = self.option_rows()
            tally.update(cacheRan=ex, cacheRows=tot)
        ndcg = None
        if self.denseAnnotations is not None:                  # NDCG reads the final scores only: any decoder, head, cache or rollout
            from . import dense
            rel = dense.relevance_matrix(image_ids, self.denseAnnotations, batch['ques_fwd'].shape[1], int(self.params.get('numOptions', 100)))
            ndcg = np.asarray(self._ndcg_of_batch(batch, rel), np.float64)
        if rollout and self.params.get('useGt'):
            ranks = ranks[np.arange(ranks.shape[0]), np.asarray(batch['answer_ind']).reshape(-1) - 1]
        return ranks, ndcg

    def rollout_history(self, batch, ranks, cut=None):
        """the history [B x R x Th] a rollout of `batch` generated, given the all ranks [N x O] it returned: rebuilt from the picks (E4);
        `cut` (a list) gains one entry per rebuilt row of a concatenated history, as `rollout_concat_row`"""
        end = self._concat_end()
        return rollout_picked_history(batch, [rollout_pick(row) for row in ranks], bool(end), end, cut)

    def evaluate(self, dataloader, dtype):
        """model.lua:109-139: validation loss / perplexity over a split: the sum over batches of `forwardBackward(batch, true)` (gen:
        summed token NLL; disc: the batch's MEAN cross-entropy) divided by the number of non-pad target tokens -- for both decoders,
        as the reference does (dataloader.lua:398-421 puts answer_out into every batch).  Synthetic disc batches without answer_out:
        the mean cross-entropy over rounds.  Returns (loss, ppl)."""
        self._set_training(False)
        n = dataloader.numThreads[dtype]
        cur, count, start = 0.0, 0.0, 1
        while start <= n:
            batch, nxt = dataloader.getTestBatch(start, self.params, dtype)
            if 'answer_out' in batch:
                count += float((np.asarray(batch['answer_out']) > 0).sum())
                cur += self.forwardBackward(batch, onlyForward=True)
            else:
                rounds = float(np.asarray(batch['answer_ind']).size)
                count += rounds
                cur += self.forwardBackward(batch, onlyForward=True) * rounds
            start = nxt
        cur /= max(count, 1.0)
        print('\n%s\tLoss: %f\t Perplexity: %f\n' % (dtype, cur, math.exp(cur)))
        self._set_training(True)
        return cur, math.exp(cur)

    def _rank_records(self, dataloader, dtype, ranks, last_round_only):
        """{image_id, round_id, ranks} records as model.lua:174-184 / :222-241 builds them: real image ids, only the
        rounds that exist (num_rounds), and for the test split of predict() the last round only."""
        ids = getattr(dataloader, 'unique_img_' + dtype, None)
        rounds = getattr(dataloader, dtype + '_num_rounds', None)
        n, R = ranks.shape[0], ranks.shape[1]
        out = []
        for i in range(n):
            iid = ids[i] if ids is not None and i < len(ids) else i + 1
            nr = int(rounds[i]) if rounds is not None else R
            if last_round_only:
                out.append({'image_id': iid, 'round_id': nr, 'ranks': ranks[i, nr - 1].tolist()})
            else:
                for j in range(nr):
                    r = ranks[i, j]
                    out.append({'image_id': iid, 'round_id': j + 1, 'ranks': r.tolist() if np.ndim(r) else float(r)})
            if self.ndcgRows is not None:                            # the records of annotated rounds gain their NDCG (-1: none, DT2)
                for rec in out[-(1 if last_round_only else nr):] if nr else []:
                    v = float(self.ndcgRows[i, rec['round_id'] - 1])
                    if v != -2.0:
                        rec['ndcg'] = v
        return out

    def _rank_split(self, dataloader, dtype):
        """the batch walk of retrieve (params useGt: the ground truth's rank, [n x R]) and predict (every candidate's, [n x R x O]); leaves
        the tallies of the walk in optionCacheRows / lhoodTreeStats / rolloutRows / rolloutCut.  Returns (ranks, the NDCG rows of the
        batches for `_ndcg_report`)."""
        n = dataloader.numThreads[dtype]
        R = int(self.params['maxQuesCount'])
        O = int(self.params.get('numOptions', 100))
        ranks = np.full((n, R) if self.params['useGt'] else (n, R, O), O + 1.0)       # model.lua:153-154
        start, tally, ndcg, rollout = 1, collections.Counter(), [], self._rollout()
        image_ids = getattr(dataloader, 'unique_img_' + dtype, None) or list(range(1, n + 1))
        while start <= n:
            batch, nxt = self._test_batch(dataloader, start, dtype, rollout)
            got, rows = self._ranked(batch, tally, rollout, image_ids[start - 1:nxt - 1])
            ranks[start - 1:nxt - 1] = got.reshape((-1,) + ranks.shape[1:])
            ndcg += [] if rows is None else [rows]
            start = nxt
        self.optionCacheRows = (tally['cacheRan'], tally['cacheRows'])
        self.lhoodTreeStats = {key: tally[key] for key in ('nodes', 'live', 'executed', 'total')}
        self.rolloutRows = (tally['differ'], tally['rows'])
        self.rolloutCut = tally['cut']
        return ranks, ndcg

    def retrieve(self, dataloader, dtype):
        """model.lua:142-189: ground-truth ranks + metrics.  params rollout = 1: the same on a history of the model's own answers
        (`retrieve_rollout_batch`, E1-E5 above); `rolloutRows` then counts the history rows that differ.  Returns (metrics, records)."""
        self._set_training(False)
        self.params['useGt'] = True
        ranks, ndcg = self._rank_split(dataloader, dtype)
        print('\n%s - Retrieval:' % dtype)
        metrics = utils.processRanks(ranks)
        self._ndcg_report(dataloader, dtype, ranks, ndcg)
        self._set_training(True)
        return metrics, self._rank_records(dataloader, dtype, ranks, False)

    def predict(self, dataloader, dtype):
        """model.lua:192-246: all 100 ranks per round (val: every existing round; test: the last round only); params rollout as retrieve"""
        self._set_training(False)
        self.params['useGt'] = False
        ranks, ndcg = self._rank_split(dataloader, dtype)
        self._ndcg_report(dataloader, dtype, ranks, ndcg)
        self._set_training(True)
        return self._rank_records(dataloader, dtype, ranks, dtype == 'test')

    # ------------------------------------------------------------------ generation (model.lua:432-613)
    def _beam_grouping(self, groups, diversity):
        """raises unless this host's `_gen_beam` searches with exactly these diverse-beam knobs (the plain search here)"""
        if groups > 1:
            raise ValueError("beamBatch > 0 with beamGroups = %d: the grouped device search runs in the model-level runtime only: use "
                             "-host native (visdial_amd.native.NativeModel); this host searches in groups with beamBatch = 0" % groups)

    def _beam_constraints(self, minLen, noRepeat, lengthPenalty):
        """raises unless this host's `_gen_beam` searches under exactly these constraints (none here: the operator-level device search
        goes through the frozen vd_beam_* operators)"""
        if minLen > 0 or noRepeat > 0 or lengthPenalty > 0.0:
            raise ValueError("beamBatch > 0 with beamMinLen = %d / beamNoRepeat = %d / beamLengthPenalty = %g: the constrained device "
                             "search runs in the model-level runtime only: use -host native (visdial_amd.native.NativeModel); this "
                             "host applies the constraints with beamBatch = 0" % (minLen, noRepeat, lengthPenalty))

    def _beam_rollout(self, rollout):
        """raises unless this host's `_gen_beam` rolls out exactly so (never here: the operator-level device search has no entry point
        that rewrites the history between rounds)"""
        if rollout:
            raise ValueError("beamBatch > 0 with rollout = 1: the device rollout runs in the model-level runtime only: use -host native "
                             "(visdial_amd.native.NativeModel); this host rolls out with beamBatch = 0")

    def rollout_batch(self, dataloader, convIds, dtype):
        """`getIndexData` with the history at its UNTRIMMED width: getIndexData trims to the ground-truth lengths of the chunk, and a
        generated answer may be longer"""
        batch = dataloader.getIndexData(convIds, self.params, dtype)
        if 'hist' in batch:
            batch['hist'] = np.ascontiguousarray(dataloader.data[dtype]['hist'][np.asarray(convIds, np.int64) - 1]).astype(np.int32)
        return batch

    def rollout_dialog(self, batch, search, endToken, concat=False):
        """R1-R6 (concat: CH1-CH6, the row by `rollout_concat_row`) for the ONE dialog of `batch` on the host: `search(r)` is the beam search of round r from the state `_gen_begin` left,
        returning its groups' (tokens, score) (`beam_search_round`).  Round r >= 1 first gets its history row from round r - 1's answer
        (batch['hist'] is rewritten in place) and a new `_gen_encode`.  Returns search(r) per round."""
        R, Th = batch['ques_fwd'].shape[1], batch['hist'].shape[2]
        found = []
        for r in range(R):
            if r > 0:
                batch['hist'][0, r] = rollout_next_row(batch['hist'][0, r - 1], batch['ques_fwd'][0, r - 1], found[-1][0][0], Th, endToken,
                                                       endToken if concat else 0)
            self._gen_encode(batch)
            found.append(search(r))
        return found

    def generateAnswers(self, dataloader, dtype, params=None):
        """Beam search (default) or temperature sampling with the generative decoder, one dialog at a time,
        exactly as the reference drives it from the host: the decoder step (embedding, LSTM stack, vocabulary
        projection, log-softmax) runs on the device for all hypotheses at once, candidate bookkeeping is host
        control flow.  params beamBatch = B > 0: the beam search of dialogs [s, s+B) runs together on the device, every round of
        the chunk at once (one encode + one `_gen_beam` per chunk); same records.  params sampleBatch = B > 0 (with sampleWords = 1):
        the same for temperature sampling (one encode + one `_gen_sample` per chunk); the host still draws every uniform, in the
        per-dialog loop's order, so the records are the same up to draws within rounding of a CDF boundary.  params topK / topP (with
        sampleWords = 1): top-k / nucleus truncation of the sampled distribution, `truncated_weights` above; the batched path needs a
        host whose device sampler truncates (`_sample_truncation`).  params beamGroups = G > 1 (beam search only): diverse beam search,
        `beam_search_round` above, with Hamming diversity params beamDiversity (default 0.5): every dialog entry gains `answers`, the
        G groups' answers in group order, and `answer` is the best of them (`pick_answer`); with beamBatch > 0 it needs a host
        whose device search runs in groups (`_beam_grouping`).  params beamMinLen / beamNoRepeat / beamLengthPenalty (beam search only,
        each off at 0): no answer of fewer than beamMinLen words, no n-gram of beamNoRepeat words twice in a hypothesis, finished
        hypotheses compete on score / length^beamLengthPenalty (csrc/beam.hip C1-C6); with beamBatch > 0 they need a host whose device
        search applies them (`_beam_constraints`).  params rollout = 1 (beam search, beamGroups = 1): every round is answered on a history
        of the model's own answers to the rounds before it instead of the ground truth's (R1-R6 above, `rollout_dialog`): one encode per
        round and dialog with beamBatch = 0; with beamBatch > 0 it needs a host whose device search rolls out (`_beam_rollout`).  An encoder
        without a history generates as with rollout = 0.
        Returns [{image_id, dialog: [{question, answer}...]}]."""
        s = self._generation_settings(params or {})
        s.startToken, s.endToken = dataloader.word2ind['<START>'], dataloader.word2ind['<END>']
        s.numThreads = int(s.maxThreads or dataloader.numThreads[dtype])
        ind2word = dataloader.ind2word
        self._set_training(False)
        img_ids = getattr(dataloader, 'unique_img_' + dtype, None)

        def record(convId, questions, answers, groups=None):
            """{image_id, dialog: [{question, answer}...]}: one question row and one answer row per round; with `groups` (per round,
            the G groups' token rows) every entry also gets `answers`"""
            rec = {'image_id': img_ids[convId - 1] if img_ids else int(convId),
                   'dialog': [{'question': utils.idToWords(q, ind2word), 'answer': utils.idToWords(a, ind2word)}
                              for q, a in zip(questions, answers)]}
            for entry, rows in zip(rec['dialog'], [] if groups is None else groups):
                entry['answers'] = [utils.idToWords(a, ind2word) for a in rows]
            return rec
        answerTable = (self._generate_chunks if s.chunk > 0 else self._generate_dialogs)(dataloader, dtype, s, record)
        self._set_training(True)
        return answerTable

    def _generation_settings(self, params):
        """the settings of generateAnswers from its params, refusing what cannot be generated before any device work"""
        if self.params['decoder'] == 'disc':
            raise SystemExit('Sampling/beam search only for generative model')
        sampleWords = bool(params.get('sampleWords', 0) == 1)
        beamBatch = int(params.get('beamBatch', 0) or 0)
        if beamBatch > 0 and sampleWords:
            raise ValueError('beamBatch > 0 is batched beam search; sampling (sampleWords = 1) runs on the host: use beamBatch = 0')
        sampleBatch = int(params.get('sampleBatch', 0) or 0)
        if sampleBatch > 0 and not sampleWords:
            raise ValueError('sampleBatch > 0 is batched sampling: it needs sampleWords = 1')
        temperature = float(params.get('temperature', 1.0))
        topK, topP = int(params.get('topK', 0) or 0), float(params.get('topP', 1.0))
        truncate = topK != 0 or topP != 1.0
        if truncate and not sampleWords:
            raise ValueError('topK / topP truncate the sampled distribution: they need sampleWords = 1 (beam search does not truncate)')
        if truncate:
            truncated_weights(np.zeros(1, np.float32), temperature, topK, topP)       # refuses a bad knob before any device work
            if sampleBatch > 0:
                self._sample_truncation(topK, topP)
        beamSize, beamLen = int(params.get('beamSize', 5)), int(params.get('beamLen', 20))
        beamGroups = int(1 if params.get('beamGroups') is None else params['beamGroups'])
        beamDiversity = float(0.5 if params.get('beamDiversity') is None else params['beamDiversity'])
        if beamGroups != 1:
            check_beam_groups(beamSize, beamGroups, beamDiversity)
            if sampleWords:
                raise ValueError('beamGroups > 1 is diverse beam search: sampling (sampleWords = 1) has no groups')
        minLen, noRepeat, lengthPenalty = (0 if params.get(key) is None else params[key]
                                           for key in ('beamMinLen', 'beamNoRepeat', 'beamLengthPenalty'))
        if minLen != 0 or noRepeat != 0 or lengthPenalty != 0:
            check_beam_constraints(beamSize, beamLen, minLen, noRepeat, lengthPenalty, self.params.get('vocabSize'))
            if sampleWords:
                raise ValueError('beamMinLen / beamNoRepeat / beamLengthPenalty constrain beam search: sampling (sampleWords = 1) has none')
        minLen, noRepeat, lengthPenalty = int(minLen), int(noRepeat), float(lengthPenalty)
        rollout = check_rollout(params.get('rollout'))
        if rollout and sampleWords:
            raise ValueError('rollout = 1 feeds the beam search\'s answers back: with sampling (sampleWords = 1) one divergent draw would '
                             'cascade over the rounds')
        if rollout and beamGroups > 1:
            raise ValueError('rollout = 1 with beamGroups = %d: the choice among a round\'s groups is made on the host; a rollout over diverse '
                             'beam search is left for a follow-up' % beamGroups)
        if beamBatch > 0:
            self._beam_grouping(beamGroups, beamDiversity)
            self._beam_constraints(minLen, noRepeat, lengthPenalty)
            self._beam_rollout(rollout)
        return types.SimpleNamespace(
            sampleWords=sampleWords, chunk=sampleBatch if sampleWords else beamBatch, temperature=temperature, topK=topK, topP=topP,
            truncate=truncate, beamSize=beamSize, beamLen=beamLen, beamGroups=beamGroups, beamDiversity=beamDiversity, minLen=minLen,
            noRepeat=noRepeat, lengthPenalty=lengthPenalty, rollout=rollout, maxThreads=params.get('maxThreads'),
            seed=int(params.get('seed', 1234)))

    def _generate_chunks(self, dataloader, dtype, s, record):
        """generateAnswers, s.chunk dialogs at a time on the device: one `_gen_encode` + one `_gen_sample` / `_gen_beam` per chunk"""
        rng = np.random.RandomState(s.seed)
        answerTable = []
        for first in range(1, s.numThreads + 1, s.chunk):
            convIds = np.arange(first, min(first + s.chunk, s.numThreads + 1))
            batch = self.rollout_batch(dataloader, convIds, dtype) if s.rollout else dataloader.getIndexData(convIds, self.params, dtype)
            B, R = len(convIds), batch['ques_fwd'].shape[1]
            self._gen_encode(batch)
            grouped = None
            if s.sampleWords:
                u = rng.random_sample((B, s.beamLen, R))        # the per-dialog loop's draws: dialog, then step, then round
                tokens, _ = self._gen_sample(s.beamLen, s.startToken, s.endToken, s.temperature,
                                             u.transpose(1, 0, 2).reshape(s.beamLen, B * R))     # [step x row]
            else:
                tokens, scores = self._gen_beam(s.beamSize, s.beamLen, s.startToken, s.endToken)
                if s.beamGroups > 1:                            # tokens [N x G x beamLen], scores [N x G]
                    grouped = tokens
                    tokens = [pick_answer(list(zip(t, sc)), s.endToken, s.lengthPenalty)[0] for t, sc in zip(grouped, scores)]
            answerTable += [record(convId, batch['ques_fwd'][i], tokens[i * R:(i + 1) * R],        # row = dialog * R + round
                                   None if grouped is None else grouped[i * R:(i + 1) * R]) for i, convId in enumerate(convIds)]
        return answerTable

    def _generate_dialogs(self, dataloader, dtype, s, record):
        """generateAnswers one dialog at a time, as the reference drives it from the host"""
        rng = np.random.RandomState(s.seed)

        def search(it):
            """the beam search of round `it` of the dialog encoded last: its groups' (tokens, score)"""
            self._gen_begin(np.full(s.beamSize, it, np.int32))                    # hiddenBeams, model.lua:478-503
            return beam_search_round(self._gen_step, self._gen_select, s.beamSize, s.beamLen, s.startToken, s.endToken, s.beamGroups,
                                     s.beamDiversity, s.minLen, s.noRepeat, s.lengthPenalty)
        answerTable = []
        for convId in range(1, s.numThreads + 1):
            convIds = np.array([convId])
            batch = self.rollout_batch(dataloader, convIds, dtype) if s.rollout else dataloader.getIndexData(convIds, self.params, dtype)
            R = batch['ques_fwd'].shape[1]
            grouped = None
            if s.sampleWords:
                self._gen_encode(batch)                                           # forwardBackward(batch, true, true)
                self._gen_begin(np.arange(R, dtype=np.int32))
                answerIn = np.full(R, s.startToken, np.int64)
                answer = [answerIn[:, None].copy()]
                for timeStep in range(s.beamLen):
                    logp = self._gen_step(answerIn)
                    self._gen_select(np.arange(R, dtype=np.int32), R)
                    if s.truncate:
                        pr = np.stack([truncated_weights(logp[i], s.temperature, s.topK, s.topP) for i in range(R)])
                    else:
                        pr = np.exp(logp.astype(np.float64) / s.temperature)
                    pr /= pr.sum(1, keepdims=True)
                    answerIn = np.array([rng.choice(pr.shape[1], p=pr[i]) + 1 for i in range(R)], np.int64)
                    answer.append(answerIn[:, None])
                answers = np.concatenate(answer, 1)
            else:
                if s.rollout and 'hist' in batch:                                 # (beamGroups = 1: a rollout refuses groups)
                    found = self.rollout_dialog(batch, search, s.endToken)
                else:
                    self._gen_encode(batch)
                    found = [search(it) for it in range(R)]
                answers = [pick_answer(f, s.endToken, s.lengthPenalty)[0] if s.beamGroups > 1 else f[0][0] for f in found]
                if s.beamGroups > 1:
                    grouped = [[tokens for tokens, _ in f] for f in found]
            answerTable.append(record(convId, batch['ques_fwd'][0], answers, grouped))
        return answerTable
