"""Prefix tree of a retrieval batch's candidates, on the host (numpy): what the model-level runtime builds at upload time for
params fusedLhood = 2 (csrc/runtime.hip build_lhood_tree), restated for the figures the hosts print -- nodes per level, nodes against
live (candidate, step) rows, and the rows the tree recurrence runs.  One tree over all options of a batch (the runtime's single chunk)."""
import numpy as np


def well_formed(option_in):
    """every candidate is one left-aligned run of tokens (no token behind a pad)"""
    live = np.asarray(option_in).reshape(-1, np.shape(option_in)[-1]) != 0
    return bool((live[:, 1:] <= live[:, :-1]).all())


def level_widths(option_in):
    """option_in [B x R x O x T] -> nodes per level: level t holds one node per distinct (round, first t + 1 tokens) among the candidates
    with t + 1 or more tokens.  Trailing levels without a node are left out."""
    a = np.asarray(option_in)
    O, T = a.shape[-2], a.shape[-1]
    tok = a.reshape(-1, T).astype(np.int64)
    cur = np.arange(tok.shape[0], dtype=np.int64) // O              # depth-0 parents: the candidate's round
    alive = np.ones(tok.shape[0], bool)
    widths = []
    for t in range(T):
        alive &= tok[:, t] != 0
        if not alive.any():
            break
        _, inv = np.unique(cur[alive] * (1 << 32) + tok[alive, t], return_inverse=True)
        cur[alive] = inv.reshape(-1)
        widths.append(int(inv.max()) + 1)
    return widths


def rows_run(widths, tile=None):
    """(step, row) slots in a row tile the tree recurrence computes: sum_t min(N, ceil(n_t / G) * G), N = the widest level, G = the step
    kernel's row tile for N (ops.lstm_fwd_row_tile)"""
    if not widths:
        return 0
    N = max(widths)
    G = tile or (128 if N >= 2048 else 32)
    return int(sum(min(N, -(-n // G) * G) for n in widths))


def stats(option_in):
    w = level_widths(option_in)
    return dict(nodes=int(sum(w)), live=int((np.asarray(option_in) != 0).sum()), widths=w, executed=rows_run(w))
