"""Dense relevance annotations (VisDial v1.0): the rules DT1-DT4 at the top of csrc/loss.hip restated in fp64 numpy, and the reader of
the annotation files.  Both Python hosts and the tests use this restatement; the device kernels (score_ce_dense_kernel, ndcg_kernel) are
held to it.

A file is a JSON list of {"image_id", "round_id" (1-based), "gt_relevance" | "relevance": [O floats]} -- one annotated round per dialog,
a relevance in [0, 1] for each of its O candidates (the format of the public dataset's description: visdial_1.0_val_dense_annotations.json
says "gt_relevance", the train sample "relevance")."""
import json

import numpy as np

NO_RELEVANT = -1.0       # DT2: an annotated round without a relevant candidate (k = 0) has no NDCG
NOT_ANNOTATED = -2.0     # DT2: a round that carries no annotation


def load_dense_annotations(path):
    """{(image_id, round_id): float64 [O]} of the file at `path`; refuses by name an entry without a relevance list, a second entry for
    an (image, round), lists of different lengths, and a relevance that is not finite and >= 0"""
    with open(path) as f:
        entries = json.load(f)
    if not isinstance(entries, list):
        raise ValueError("%s: dense annotations are a JSON list of {image_id, round_id, gt_relevance | relevance} entries, got %s"
                         % (path, type(entries).__name__))
    out, O = {}, None
    for i, e in enumerate(entries):
        rel = e.get('gt_relevance', e.get('relevance')) if isinstance(e, dict) else None
        if rel is None or 'image_id' not in e or 'round_id' not in e:
            raise ValueError("%s: entry %d needs image_id, round_id and gt_relevance (or relevance)" % (path, i))
        key = (int(e['image_id']), int(e['round_id']))
        if key in out:
            raise ValueError("%s: entry %d is a duplicate annotation of image_id %d, round_id %d" % ((path, i) + key))
        rel = np.asarray(rel, np.float64).reshape(-1)
        O = rel.size if O is None else O
        if rel.size != O:
            raise ValueError("%s: entry %d (image_id %d, round_id %d) has a wrong length: %d relevances, the entries before it %d"
                             % ((path, i) + key + (rel.size, O)))
        if not (np.isfinite(rel).all() and (rel >= 0).all()):
            raise ValueError("%s: entry %d (image_id %d, round_id %d): a relevance is finite and >= 0" % ((path, i) + key))
        out[key] = rel
    return out


def relevance_matrix(image_ids, annotations, R, O):
    """DT1's matrix, float32 [len(image_ids) * R x O]: row (i, r) = the relevance of round r + 1 of image_ids[i], or all -1 where the
    annotations hold none.  An annotation of another length than O is refused by name."""
    rel = np.full((len(image_ids) * R, O), -1.0, np.float32)
    for i, iid in enumerate(image_ids):
        for r in range(R):
            a = annotations.get((int(iid), r + 1))
            if a is not None:
                if a.size != O:
                    raise ValueError("dense annotation of image_id %d, round_id %d has a wrong length: %d relevances for %d candidates"
                                     % (int(iid), r + 1, a.size, O))
                rel[i * R + r] = a
    return rel


def annotated_rows(rel):
    """DT1 checked on a matrix: bool [N], True = annotated; raises ValueError on a mixed row, a NaN or another negative value"""
    rel = np.asarray(rel, np.float64)
    none = (rel == -1).all(1)
    ok = np.isfinite(rel).all(1) & (rel >= 0).all(1)
    bad = ~(none | ok)
    if bad.any():
        raise ValueError("relevance row %d is neither annotated (every entry finite and >= 0) nor a full row of -1" % int(np.argmax(bad)))
    return ok


def _ranks(values):
    """1-based descending ranks of every row, among equal values the lower index first (ranks_kernel in csrc/loss.hip, utils.computeRanks)"""
    order = np.argsort(-values, axis=1, kind='stable')
    ranks = np.empty(order.shape, np.int64)
    np.put_along_axis(ranks, order, np.arange(1, values.shape[1] + 1)[None, :], axis=1)
    return ranks


def ndcg_rows(scores, rel):
    """DT2: float64 [N]; NO_RELEVANT (-1) for an annotated row with k = 0, NOT_ANNOTATED (-2) for a row of -1"""
    scores, rel = np.asarray(scores), np.asarray(rel, np.float64)
    annotated = annotated_rows(rel)
    out = np.full(rel.shape[0], NOT_ANNOTATED)
    srank, rrank = _ranks(scores), _ranks(rel)
    for n in np.nonzero(annotated)[0]:
        k = int((rel[n] > 0).sum())
        if k == 0:
            out[n] = NO_RELEVANT
            continue
        dcg = idcg = 0.0
        for o in range(rel.shape[1]):                                  # index order, as the kernel adds them
            if srank[n, o] <= k:
                dcg += rel[n, o] / np.log2(1.0 + srank[n, o])
            if rrank[n, o] <= k:
                idcg += rel[n, o] / np.log2(1.0 + rrank[n, o])
        out[n] = dcg / idcg
    return out


def ndcg_mean(rows):
    """(mean NDCG over the rows that have one, annotated rows, annotated rows with k = 0 left out of the mean)"""
    rows = np.asarray(rows, np.float64)
    have = rows >= 0
    return (float(rows[have].mean()) if have.any() else float('nan')), int((rows != NOT_ANNOTATED).sum()), int((rows == NO_RELEVANT).sum())


def dense_targets(rel, gt, mix):
    """DT3: (t float64 [N x O], w float64 [N]); gt = 0-based ground-truth option of every round"""
    rel = np.asarray(rel, np.float64)
    if not (0.0 <= float(mix) <= 1.0):
        raise ValueError("mix = %r must be a finite real in [0, 1]" % (mix,))
    annotated = annotated_rows(rel)
    N, O = rel.shape
    t = np.zeros((N, O))
    t[np.arange(N), np.asarray(gt).reshape(-1)] = 1.0
    w = np.full(N, float(mix))
    tot = rel.sum(1)
    live = annotated & (tot > 0)
    t[live] = rel[live] / tot[live, None]
    w[annotated] = 0.0
    w[live] = 1.0
    return t, w


def live_rounds(rel, mix):
    """DL1: the rounds whose DT3 weight is > 0 under `mix`, ascending (int64 [n_live]): annotated with a relevant candidate, or not annotated
    with mix > 0.  These are the rounds whose candidate rows a step on '@dense_relevance_live' executes."""
    rel = np.asarray(rel, np.float64)
    _, w = dense_targets(rel, np.zeros(rel.shape[0], np.int64), mix)
    return np.nonzero(w > 0)[0]


def live_option_tokens(tok_step_major, uid, live, O):
    """DL3's compaction: int32 [To x len(live) * O] from the uploaded step-major tokens [To x rows]; output row (slot, o) is the row of candidate
    (live[slot], o) -- uid[live[slot] * O + o] where the upload de-duplicated the candidates (uid [N * O]), else the candidate's own row"""
    tok = np.asarray(tok_step_major)
    cand = (np.asarray(live, np.int64)[:, None] * int(O) + np.arange(int(O))[None, :]).reshape(-1)
    src = cand if uid is None else np.asarray(uid, np.int64).reshape(-1)[cand]
    return np.ascontiguousarray(tok[:, src], dtype=np.int32).reshape(tok.shape[0], cand.size)


def dense_ce(scores, rel, gt, mix):
    """DT4: (loss, ds [N x O]) in fp64 -- loss = sum_n w_n (lse_n - sum_o t_o s_o) / W, ds = w_n (softmax - t) / W, W = sum_n w_n;
    a batch with W = 0 is refused by name"""
    s = np.asarray(scores, np.float64)
    t, w = dense_targets(rel, gt, mix)
    W = w.sum()
    if not W > 0:
        raise ValueError("dense batch with W = 0: no annotated round has a relevant candidate and rounds without an annotation weigh "
                         "mix = %r" % (mix,))
    mx = s.max(1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(s - mx).sum(1))
    rows = lse - (t * s).sum(1)
    soft = np.exp(s - lse[:, None])
    return float((w * rows).sum() / W), (w[:, None] * (soft - t)) / W
