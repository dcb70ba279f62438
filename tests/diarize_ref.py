"""Float64 numpy restatement of las_bic_change / las_bic_cluster (include/las_hip.h K17), written from the contract's words: the
statistics by sums in frame order, the log-determinant by a Cholesky of plain loops (vectorised over a batch of matrices, no LAPACK
anywhere in a decision), the peak and tie rules as loops.  Also the synthetic two-voice recording of the diarization tests."""
import numpy as np

INF = float("inf")


# ---- statistics ------------------------------------------------------------------------------------------------------------------------
def stats(feat, mask, a, b, D):
    """(n, S1 [D], S2 [D, D]) of the masked frames of rows [a, b): fp32 widened to double, summed in frame order"""
    n, S1, S2 = 0.0, np.zeros(D), np.zeros((D, D))
    for t in range(a, b):
        if mask is None or mask[t]:
            x = feat[t, :D].astype(np.float64)
            n += 1.0
            S1 = S1 + x
            S2 = S2 + np.outer(x, x)
    return n, S1, S2


def window_stats(feat, mask, starts, w, D):
    """the statistics of the windows [s, s + w) for every s of starts at once (n [C], S1 [C, D], S2 [C, D, D]); frame order per window"""
    starts = np.asarray(starts, np.int64)
    C = len(starts)
    n, S1, S2 = np.zeros(C), np.zeros((C, D)), np.zeros((C, D, D))
    for f in range(w):
        x = feat[starts + f, :D].astype(np.float64)
        m = np.ones(C) if mask is None else (np.asarray(mask)[starts + f] != 0).astype(np.float64)
        x = np.where(m[:, None] != 0, x, 0.0)                             # (a masked-out frame adds exact zeros: the sums' bits are the skip's)
        n = n + m
        S1 = S1 + x
        S2 = S2 + x[:, :, None] * x[:, None, :]
    return n, S1, S2


def add(p, q):
    return p[0] + q[0], p[1] + q[1], p[2] + q[2]


def covariance(st, floor):
    n, S1, S2 = st
    n = np.asarray(n, np.float64)[..., None, None]
    S1 = np.asarray(S1)
    D = S1.shape[-1]
    with np.errstate(all="ignore"):
        return (S2 - S1[..., :, None] * S1[..., None, :] / n) / n + floor * np.eye(D)


def chol_logdet(A):
    """log det of symmetric positive definite matrices [..., D, D] by a right-looking Cholesky in plain loops"""
    A = np.array(A, np.float64, copy=True)
    D = A.shape[-1]
    out = np.zeros(A.shape[:-2])
    with np.errstate(all="ignore"):
        for k in range(D):
            p = A[..., k, k]
            out = out + np.log(p)
            s = np.sqrt(p)
            for i in range(k + 1, D):
                A[..., i, k] = A[..., i, k] / s
            for i in range(k + 1, D):
                for j in range(k + 1, i + 1):
                    A[..., i, j] = A[..., i, j] - A[..., i, k] * A[..., j, k]
    return out


def logdet(st, floor):
    return chol_logdet(covariance(st, floor))


def delta_bic(x, y, lam, floor, Lx=None, Ly=None):
    """x, y: statistics (scalars or batches).  dBIC = 1/2 [n L(x u y) - n1 L(x) - n2 L(y)] - lam 1/2 (D + D (D + 1) / 2) log n"""
    D = np.asarray(x[1]).shape[-1]
    Lx = logdet(x, floor) if Lx is None else Lx
    Ly = logdet(y, floor) if Ly is None else Ly
    u = add(x, y)
    n = np.asarray(u[0], np.float64)
    with np.errstate(all="ignore"):
        return 0.5 * (n * logdet(u, floor) - x[0] * Lx - y[0] * Ly) - lam * 0.5 * (D + D * (D + 1) / 2) * np.log(n)


# ---- the change curve -------------------------------------------------------------------------------------------------------------------
def candidates(length, w, hop):
    return 0 if length < 2 * w else (length - 2 * w) // hop + 1


def change_curve(feat, mask, off, length, D, w, hop, nmin, lam, floor):
    """v [C_s] of one sequence"""
    C = candidates(length, w, hop)
    if C == 0:
        return np.zeros(0)
    t = off + w + np.arange(C) * hop
    x, y = window_stats(feat, mask, t - w, w, D), window_stats(feat, mask, t, w, D)
    v = delta_bic(x, y, lam, floor)
    return np.where((x[0] < nmin) | (y[0] < nmin), -INF, v)


def peaks(v, R):
    out = np.zeros(len(v), np.uint8)
    for c in range(len(v)):
        ok = v[c] > 0
        for k in range(max(0, c - R), c):
            ok = ok and v[c] > v[k]
        for k in range(c + 1, min(len(v), c + R + 1)):
            ok = ok and v[c] >= v[k]
        out[c] = 1 if ok else 0
    return out


def peak_margin(v, R):
    """the least distance, relative to 1 + |value|, by which a decision of the peak rule on v holds: every candidate's sign test
    (candidates at -inf have none), every peak against each rival of its window, and every non-peak with v > 0 against the rival
    that beats it by most; a rival of exactly the candidate's value is a tie, which the index rule decides, and is left out"""
    m = INF
    flags = peaks(v, R)
    for c in range(len(v)):
        if not np.isfinite(v[c]):
            continue
        m = min(m, abs(v[c]) / (1 + abs(v[c])))
        if v[c] <= 0:
            continue
        rivals = [v[k] for k in range(max(0, c - R), min(len(v), c + R + 1)) if k != c and np.isfinite(v[k]) and v[k] != v[c]]
        if not rivals:
            continue
        if flags[c]:
            m = min(m, min(v[c] - r for r in rivals) / (1 + abs(v[c])))
        else:
            m = min(m, max(r - v[c] for r in rivals) / (1 + abs(v[c])))
    return m


# ---- the clustering ---------------------------------------------------------------------------------------------------------------------
class Clustering(object):
    pass


def _stack(sts):
    return np.array([u[0] for u in sts], np.float64), np.stack([u[1] for u in sts]), np.stack([u[2] for u in sts])


def cluster(units, K, lam, floor):
    """units: the statistics of one recording's units -> Clustering(label, n_clusters, dist [S, S] (upper triangle, nan elsewhere),
    merges [(i, j)], merge_val, stop_val: the least d the loop stopped on (None: it ran out of pairs), margin: the least distance,
    relative to 1 + |d|, by which a decision held -- the chosen pair against the runner-up (exact ties, which the index rule decides,
    left out) and, for K = 0, the chosen d against 0)"""
    S = len(units)
    st = [tuple(u) for u in units]
    L = [float(logdet(u, floor)) for u in st]
    d = np.full((S, S), np.nan)
    for i in range(S - 1):
        d[i, i + 1:] = delta_bic(st[i], _stack(st[i + 1:]), lam, floor, L[i], np.array(L[i + 1:]))
    out = Clustering()
    out.dist = d.copy()
    live, rep = [True] * S, list(range(S))
    out.merges, out.merge_val, out.stop_val, out.margin = [], [], None, INF
    while True:
        idx = [k for k in range(S) if live[k]]
        if len(idx) <= 1:
            break
        best, second = None, INF
        for a, i in enumerate(idx):
            for j in idx[a + 1:]:
                if best is None or d[i, j] < best[0]:                     # (i ascending, then j: the first of equal minima)
                    if best is not None:
                        second = min(second, best[0])
                    best = (d[i, j], i, j)
                else:
                    second = min(second, d[i, j])
        v, i, j = best
        stop = (K > 0 and len(idx) <= K) or (K == 0 and not v < 0)
        if K == 0:
            out.margin = min(out.margin, abs(v) / (1 + abs(v)))
        if stop:
            out.stop_val = v
            break
        if second != v and second < INF:
            out.margin = min(out.margin, (second - v) / (1 + abs(v)))
        out.merges.append((i, j))
        out.merge_val.append(v)
        st[i] = add(st[i], st[j])
        L[i] = float(logdet(st[i], floor))
        live[j] = False
        rep = [i if r == j else r for r in rep]
        others = [k for k in idx if k != i and k != j]
        if others:
            row = delta_bic(st[i], _stack([st[k] for k in others]), lam, floor, L[i], np.array([L[k] for k in others]))
            for k, x in zip(others, row):
                d[min(i, k), max(i, k)] = x
    reps = sorted(set(rep))
    out.label = [reps.index(r) for r in rep]
    out.n_clusters = len(reps)
    return out


def groups(label):
    return [[s for s, l in enumerate(label) if l == c] for c in range(max(label) + 1)]


# ---- host helpers of las.diarize restated ---------------------------------------------------------------------------------------------------
def split_at(run, flags, w, hop):
    """a run [a, b) in VAD frames and the peak flags of its b - a - 1 feature frames -> its sub-runs"""
    a, b = run
    cuts = [a + w + c * hop for c in np.flatnonzero(flags)]
    edges = [a] + cuts + [b]
    return list(zip(edges[:-1], edges[1:]))


# ---- the synthetic recording of the CLI test ----------------------------------------------------------------------------------------------
RATE = 16000


def two_voices():
    """A 3.0 s, B 2.5 s abutting, 0.6 s of zeros, A 2.0 s, 0.6 s of zeros, B 3.0 s: white noise (RandomState(5)) coloured by
    lfilter([1], [1, -a]), a = 0.95 for voice A and -0.7 for voice B, every burst scaled to 0.05 RMS; float32 at 16 kHz"""
    from scipy.signal import lfilter
    rng = np.random.RandomState(5)

    def voice(a, seconds):
        x = lfilter([1.0], [1.0, -a], rng.randn(int(seconds * RATE)))
        return 0.05 * x / np.sqrt(np.mean(x * x))

    z = np.zeros(int(0.6 * RATE))
    return np.concatenate([voice(0.95, 3.0), voice(-0.7, 2.5), z, voice(0.95, 2.0), z, voice(-0.7, 3.0)]).astype(np.float32)
