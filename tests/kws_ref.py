"""Float64 restatement of las_kws_search (include/las_hip.h K10j): the end series of the keyword recursion, the hits the
streaming rule keeps, the counts and `best`.  The device does one fp64 subtraction and one fp64 addition per state and frame, in frame
order, and multiplies nothing, so this restatement -- the same operations in the same order -- gives the same bits.

lp is class-major, [Vc, >= T] (one utterance of las_ctc_log_softmax's output), blank = class Vc - 1."""
import collections

import numpy as np

NEG = -np.inf
MAX_L = 32

Result = collections.namedtuple("Result", "end_score end_start hits kept total best")
# end_score f64 [Tp], end_start int64 [Tp] (-inf / -1 behind T and where the end state is not reached); hits: the kept list, in time order,
# [(start, end, score)]; kept = len(hits); total: hits closed; best = (score, start, end)


def searchable(labels, Vc, U=MAX_L):
    L = len(labels)
    return 1 <= L <= min(U, MAX_L) and all(0 <= int(c) <= Vc - 2 for c in labels)


def frame_max(lp, T):
    """m[t] = max_c lp[c, t] in the input's own float32"""
    return np.asarray(lp)[:, :T].max(axis=0)


def series(lp, labels, T):
    """-> (end_score [T] f64, end_start [T] int64): best(t, 2L - 2) and its start"""
    lp = np.asarray(lp)
    Vc = lp.shape[0]
    labels = [int(c) for c in labels]
    L = len(labels)
    S = 2 * L - 1
    ext = np.full(S, Vc - 1, np.int64)
    ext[0::2] = labels
    e = lp[ext, :T].astype(np.float64) - frame_max(lp, T).astype(np.float64)[None, :]        # [S, T], one subtraction each
    skip = np.zeros(S, bool)
    for s in range(2, S, 2):
        skip[s] = labels[s >> 1] != labels[(s >> 1) - 1]
    b, st = np.full(S, NEG), np.full(S, -1, np.int64)
    out_b, out_s = np.full(T, NEG), np.full(T, -1, np.int64)
    for t in range(T):
        cb, cs = b.copy(), st.copy()                                                           # 1. stay
        b1, s1 = np.concatenate(([NEG], b[:-1])), np.concatenate(([-1], st[:-1]))              # 2. s - 1
        c = b1 > cb
        cb[c], cs[c] = b1[c], s1[c]
        b2 = np.where(skip, np.concatenate(([NEG, NEG], b[:-2]))[:S], NEG)                     # 3. s - 2 where allowed
        s2 = np.concatenate(([-1, -1], st[:-2]))[:S]
        c = b2 > cb
        cb[c], cs[c] = b2[c], s2[c]
        if 0.0 > cb[0]:                                                                        # 4. the fresh start
            cb[0], cs[0] = 0.0, t
        b, st = cb + e[:, t], cs
        out_b[t], out_s[t] = b[S - 1], st[S - 1]
    return out_b, out_s


def hits_of(end_score, end_start, thr, H):
    """the streaming rule over an end series -> (kept list [(start, end, score)], total closed)"""
    thr = float(np.float64(np.float32(thr)))
    kept, total, cur = [], 0, None                      # cur = the open hit [score, start, end]

    def close(h):
        nonlocal total
        total += 1
        if len(kept) < H:
            kept.append((h[1], h[2], h[0]))
            return
        w = 0
        for k in range(1, H):
            if kept[k][2] < kept[w][2]:                 # the smallest score, the earliest among equals
                w = k
        if h[0] > kept[w][2]:
            del kept[w]
            kept.append((h[1], h[2], h[0]))

    for t in range(len(end_score)):
        sc, st = float(end_score[t]), int(end_start[t])
        if not np.isfinite(sc) or not sc >= thr:
            continue
        if cur is not None and st <= cur[2]:
            if sc >= cur[0]:
                cur = [sc, st, t]
        else:
            if cur is not None:
                close(cur)
            cur = [sc, st, t]
    if cur is not None:
        close(cur)
    return kept, total


def best_of(end_score, end_start):
    best = (NEG, -1, -1)
    for t in range(len(end_score)):
        sc = float(end_score[t])
        if np.isfinite(sc) and sc >= best[0]:           # equal values: the later end
            best = (sc, int(end_start[t]), t)
    return best


def search(lp, labels, T, thr, H, Tp=None, U=MAX_L):
    """one (utterance, phrase) of las_kws_search; T already clamped to [1, Tp]"""
    lp = np.asarray(lp)
    Tp = lp.shape[1] if Tp is None else Tp
    es, et = np.full(Tp, NEG), np.full(Tp, -1, np.int64)
    if not searchable(labels, lp.shape[0], U):
        return Result(es, et, [], 0, 0, (NEG, -1, -1))
    es[:T], et[:T] = series(lp, labels, T)
    kept, total = hits_of(es[:T], et[:T], thr, H)
    return Result(es, et, kept, len(kept), total, best_of(es[:T], et[:T]))
