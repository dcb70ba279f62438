"""Float64 restatement of las_ctc_align (include/las_hip.h K10d): the max-plus extended-label recursion with a back-trace and
the contract's tie rule.  The device adds one fp64 value per frame, in frame order, and multiplies nothing, so this restatement -- the
same additions in the same order -- gives the same bits.

lp is class-major, [Vc, >= T] (one utterance of las_ctc_log_softmax's output), blank = class Vc - 1."""
import collections

import numpy as np

Alignment = collections.namedtuple("Alignment", "score states first last")     # states / first / last: int arrays, None when unalignable

NEG = -np.inf


def unalignable(L):
    return Alignment(NEG, None, np.full(L, -1, np.int64), np.full(L, -1, np.int64))


def align(lp, labels, T):
    """Best CTC alignment of `labels` to frames 0 .. T-1.  best(t, s) = lp + max(prev(s), prev(s-1), prev(s-2) if allowed); on equal
    values the smaller step wins; the final state is the larger of 2L and 2L-1, 2L on a tie."""
    lp = np.asarray(lp)
    Vc = lp.shape[0]
    labels = [int(c) for c in labels]
    L = len(labels)
    if any(c < 0 or c > Vc - 2 for c in labels):
        return unalignable(L)
    S = 2 * L + 1
    ext = np.full(S, Vc - 1, np.int64)
    ext[1::2] = labels
    em = lp[ext, :T].astype(np.float64)                         # [S, T]
    skip = np.zeros(S, bool)
    for s in range(3, S, 2):
        skip[s] = labels[s >> 1] != labels[(s >> 1) - 1]
    a = np.full(S, NEG)
    a[:2] = em[:2, 0]
    bp = np.zeros((T, S), np.int64)
    for t in range(1, T):
        m, k = a.copy(), np.zeros(S, np.int64)
        a1 = np.concatenate(([NEG], a[:-1]))
        a2 = np.where(skip, np.concatenate(([NEG, NEG], a[:-2]))[:S], NEG)
        c = a1 > m
        m[c], k[c] = a1[c], 1
        c = a2 > m
        m[c], k[c] = a2[c], 2
        a = m + em[:, t]
        bp[t] = k
    fin = S - 1
    if S >= 2 and a[S - 2] > a[S - 1]:
        fin = S - 2
    if a[fin] == NEG:
        return unalignable(L)
    states = np.zeros(T, np.int64)
    s = fin
    for t in range(T - 1, -1, -1):
        states[t] = s
        s -= bp[t, s]
    first, last = np.full(L, -1, np.int64), np.full(L, -1, np.int64)
    for t in range(T):
        if states[t] & 1:
            j = states[t] >> 1
            if first[j] < 0:
                first[j] = t
            last[j] = t
    return Alignment(float(a[fin]), states, first, last)


def check_path(lp, labels, T, frame_state):
    """frame_state[0:T] is a valid CTC alignment of `labels` (starts in state 0 or 1, moves by 0, 1 or 2 -- 2 only from a label to a
    different label -- ends in 2L or 2L-1) that collapses to them; -> its float64 score, summed in frame order."""
    lp = np.asarray(lp)
    Vc = lp.shape[0]
    labels = [int(c) for c in labels]
    L = len(labels)
    st = [int(s) for s in frame_state[:T]]
    assert len(st) == T and all(0 <= s <= 2 * L for s in st), st
    assert st[0] in (0, 1), st[0]
    assert st[-1] in (2 * L, 2 * L - 1), (st[-1], L)
    for p, s in zip(st[:-1], st[1:]):
        assert s - p in (0, 1, 2), (p, s)
        if s - p == 2:
            assert s & 1 and labels[s >> 1] != labels[(s >> 1) - 1], (p, s)
    classes = [labels[s >> 1] if s & 1 else Vc - 1 for s in st]
    collapsed = [c for i, c in enumerate(classes) if c != Vc - 1 and (i == 0 or st[i] != st[i - 1])]
    assert collapsed == labels, (collapsed, labels)
    score = np.float64(lp[classes[0], 0])
    for t in range(1, T):
        score = score + np.float64(lp[classes[t], t])
    return float(score)
