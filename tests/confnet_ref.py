"""Numpy restatement of include/las_hip.h K10h (las_nbest_network): hypotheses merged one after the other into a word transition network
by the 0/1-cost table, the back-trace rule written literally, the overflow rule, and the bin masses as sequential sums in slot order
(np.float32, or float64 for the properties that want exact sums).  No imports from `las`; nbest_ref is imported for the cross-check of
the first merge against the plain edit distance."""
import numpy as np

import nbest_ref  # noqa: F401  (distance(): what merging a second hypothesis into the first must cost)

EPS = -1


def table(syms, b):
    """syms[i-1] = the set of symbols of bin i, b the tokens of the hypothesis -> D [B + 1, L + 1] int64, one numpy row at a time (the
    left move costs 1 whatever the row: the running minimum of nbest_ref.table_fast)"""
    B, L = len(syms), len(b)
    b = np.asarray(b, np.int64).reshape(L)
    D = np.zeros((B + 1, L + 1), np.int64)
    D[0, :] = np.arange(L + 1)
    cols = np.arange(L + 1)
    for i in range(1, B + 1):
        cup = 0 if EPS in syms[i - 1] else 1
        has = np.isin(b, np.fromiter(syms[i - 1], np.int64, len(syms[i - 1])))
        t = np.empty(L + 1, np.int64)
        t[0] = D[i - 1, 0] + cup
        t[1:] = np.minimum(D[i - 1, 1:] + cup, D[i - 1, :-1] + np.where(has, 0, 1))
        D[i] = np.minimum.accumulate(t - cols) + cols
    return D


def table_literal(syms, b):
    """the recurrence cell by cell, as the header writes it (small cases: checks table())"""
    B, L = len(syms), len(b)
    D = np.zeros((B + 1, L + 1), np.int64)
    for j in range(L + 1):
        D[0, j] = j
    for i in range(1, B + 1):
        cup = 0 if EPS in syms[i - 1] else 1
        D[i, 0] = D[i - 1, 0] + cup
        for j in range(1, L + 1):
            D[i, j] = min(D[i - 1, j] + cup, D[i, j - 1] + 1, D[i - 1, j - 1] + (0 if b[j - 1] in syms[i - 1] else 1))
    return D


def trace(D, syms, b):
    """-> the steps from (B, L) back to (0, 0): (rule, i, j) with rule 1 match, 2 new alternative, 3 EPS, 4 new bin behind bin i"""
    i, j = len(syms), len(b)
    steps = []
    while i > 0 or j > 0:
        cup = 0 if (i > 0 and EPS in syms[i - 1]) else 1
        if i > 0 and j > 0 and b[j - 1] in syms[i - 1] and D[i, j] == D[i - 1, j - 1]:
            steps.append((1, i, j))
            i, j = i - 1, j - 1
        elif i > 0 and j > 0 and D[i, j] == D[i - 1, j - 1] + 1:
            steps.append((2, i, j))
            i, j = i - 1, j - 1
        elif i > 0 and D[i, j] == D[i - 1, j] + cup:
            steps.append((3, i, j))
            i -= 1
        else:
            steps.append((4, i, j))
            j -= 1
    return steps


def network(hyps, w, max_bins, mode="f32"):
    """one utterance: hyps = the live hypotheses best first, w [>= len] their weights -> dict(cols [nh, B] int32 (rows of slots that
    were not merged hold EPS), merged [nh] int8, nbins, best [B] int32, post [B] float32 / float64, costs [nh] the table's corner of
    every merge (None where the network was empty))"""
    nh = len(hyps)
    fl = np.float32 if mode == "f32" else np.float64
    w = np.asarray(w, np.float32)
    rows = [None] * nh
    merged = np.zeros(nh, np.int8)
    costs = [None] * nh
    sizes = []                                                         # the bins in front of every slot's merge
    B = 0
    for k in range(nh):
        sizes.append(B)
        b = [max(int(t), 0) for t in hyps[k]]
        live = [q for q in range(k) if merged[q]]
        syms = [set(rows[q][i] for q in live) for i in range(B)]
        D = table(syms, b)
        costs[k] = int(D[B, len(b)]) if live else None
        steps = trace(D, syms, b)
        ins = sum(1 for s in steps if s[0] == 4)
        if B + ins > max_bins:
            continue
        new = {q: [] for q in live}
        mine = []
        for rule, i, j in reversed(steps):
            for q in live:
                new[q].append(EPS if rule == 4 else rows[q][i - 1])
            mine.append(EPS if rule == 3 else b[j - 1])
        for q in live:
            rows[q] = new[q]
        rows[k] = mine
        merged[k] = 1
        B += ins
        assert len(mine) == B
    cols = np.full((nh, B), EPS, np.int32)
    for k in range(nh):
        if merged[k]:
            cols[k] = rows[k]
    best = np.full(B, EPS, np.int32)
    post = np.zeros(B, fl)
    for i in range(B):
        order = []                                                     # the bin's symbols by their first contributing slot
        for k in range(nh):
            if merged[k] and cols[k, i] not in order:
                order.append(int(cols[k, i]))
        for c, s in enumerate(order):
            acc = fl(0)
            for k in range(nh):
                if merged[k] and cols[k, i] == s:
                    acc = fl(acc + fl(w[k]))
            if c == 0 or acc > post[i]:
                best[i], post[i] = s, acc
    return dict(cols=cols, merged=merged, nbins=B, best=best, post=post, costs=costs, sizes=sizes + [B])


def masses(cols, merged, w, i, mode="f64"):
    """{symbol: mass} of bin i, in order of the first contributing slot"""
    fl = np.float32 if mode == "f32" else np.float64
    out = {}
    for k in range(len(merged)):
        if merged[k]:
            s = int(cols[k][i])
            out[s] = fl(out.get(s, fl(0)) + fl(np.float32(w[k])))
    return out
