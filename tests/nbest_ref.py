"""Numpy restatement of include/las_hip.h K10g (las_nbest_risk, las_nbest_confidence): the integer Levenshtein table, the back-trace
rule written literally, and risk / conf as sequential np.float32 loops (one product, one sum, in slot order).  No imports from `las`."""
import numpy as np


def table(a, b):
    """D [len(a) + 1, len(b) + 1] int64: D[i][j] = the unit-cost edit distance of a[:i] and b[:j]"""
    La, Lb = len(a), len(b)
    D = np.zeros((La + 1, Lb + 1), np.int64)
    D[:, 0] = np.arange(La + 1)
    D[0, :] = np.arange(Lb + 1)
    for i in range(1, La + 1):
        for j in range(1, Lb + 1):
            D[i, j] = min(D[i - 1, j] + 1, D[i, j - 1] + 1, D[i - 1, j - 1] + (0 if a[i - 1] == b[j - 1] else 1))
    return D


def table_fast(a, b):
    """the same table one numpy row at a time (for the long cases of the GPU tests): the in-row dependency D[i][j] = min(t[j],
    D[i][j-1] + 1) is a running minimum of t[k] - k"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    La, Lb = len(a), len(b)
    D = np.zeros((La + 1, Lb + 1), np.int64)
    D[0, :] = np.arange(Lb + 1)
    cols = np.arange(Lb + 1)
    for i in range(1, La + 1):
        t = np.empty(Lb + 1, np.int64)
        t[0] = i
        t[1:] = np.minimum(D[i - 1, 1:] + 1, D[i - 1, :-1] + (a[i - 1] != b))
        D[i] = np.minimum.accumulate(t - cols) + cols
    return D


def distance(a, b):
    return int(table_fast(a, b)[len(a), len(b)])


def backtrace(a, b, D=None):
    """-> match [len(a)] int8: 1 where a[i] was matched along the path the rule picks from (len(a), len(b))"""
    D = table_fast(a, b) if D is None else D
    i, j = len(a), len(b)
    match = np.zeros(len(a), np.int8)
    while i > 0 or j > 0:
        if i > 0 and j > 0 and a[i - 1] == b[j - 1] and D[i, j] == D[i - 1, j - 1]:
            match[i - 1] = 1
            i, j = i - 1, j - 1
        elif i > 0 and j > 0 and D[i, j] == D[i - 1, j - 1] + 1:
            i, j = i - 1, j - 1
        elif i > 0 and D[i, j] == D[i - 1, j] + 1:
            i -= 1
        else:
            j -= 1
    return match


def risk(token_lists, w):
    """one utterance: token_lists = the live hypotheses, w [>= len] float32 -> (dist [nh, nh] int32, risk [nh] float32, pick)"""
    nh = len(token_lists)
    w = np.asarray(w, np.float32)
    dist = np.zeros((nh, nh), np.int32)
    for i in range(nh):
        for j in range(i + 1, nh):
            dist[i, j] = dist[j, i] = distance(token_lists[i], token_lists[j])
    r = np.zeros(nh, np.float32)
    for i in range(nh):
        acc = np.float32(0)
        for k in range(nh):
            acc = np.float32(acc + np.float32(w[k] * np.float32(dist[i, k])))
        r[i] = acc
    pick = -1 if nh == 0 else 0
    for k in range(1, nh):
        if r[k] < r[pick] or (r[k] == r[pick] and w[k] > w[pick]):
            pick = k
    return dist, r, pick


def confidence(token_lists, w, pivot):
    """one utterance -> (match [nh, len(pivot)] int8, conf [len(pivot)] float32); None, None for a pivot outside the live slots"""
    nh = len(token_lists)
    if pivot < 0 or pivot >= nh:
        return None, None
    w = np.asarray(w, np.float32)
    a = token_lists[pivot]
    match = np.zeros((nh, len(a)), np.int8)
    for k in range(nh):
        match[k] = backtrace(a, token_lists[k])
    conf = np.zeros(len(a), np.float32)
    for i in range(len(a)):
        acc = np.float32(0)
        for k in range(nh):
            acc = np.float32(acc + np.float32(w[k] * np.float32(match[k, i])))
        conf[i] = acc
    return match, conf
