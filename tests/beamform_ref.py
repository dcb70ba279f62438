"""The three beamforming calls of include/las_hip.h K18 (las_gcc_phat, las_tdoa_track, las_delay_sum) restated in float64 numpy,
numpy.fft in double, and the generators of the inputs the tests use.  Nothing here touches a device."""
import numpy as np

MAX_CHANNELS, MAX_FFT, MAX_LAG = 16, 16384, 512      # include/las_hip.h LAS_BF_*
EPS = 1e-12


def windows(n, L):
    H = L // 2
    return 1 if n <= L else -(-(n - L) // H) + 1


def hann(L):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(L) + 0.5) / L)


def twiddle(NF):
    """[NF / 2 + 1, 2]: (cos, -sin)(2 pi k / NF), the table las_gcc_phat takes"""
    k = np.arange(NF // 2 + 1)
    return np.stack([np.cos(2.0 * np.pi * k / NF), -np.sin(2.0 * np.pi * k / NF)], axis=1)


def next_pow2(v):
    p = 1
    while p < v:
        p *= 2
    return p


def widen(x):
    """the samples as the kernels see them: int16 as float32(v) / float32(32767), fp32 as it is; then double"""
    x = np.asarray(x)
    if x.dtype == np.int16:
        return (x.astype(np.float32) / np.float32(32767.0)).astype(np.float64)
    return x.astype(np.float32).astype(np.float64)


def frames(x, L, w0, w1):
    """windows [w0, w1) of the rows of x [C, n] -> [C, w1 - w0, L], zeros at and behind n"""
    H = L // 2
    C, n = x.shape
    idx = (np.arange(w0, w1) * H)[:, None] + np.arange(L)[None, :]
    return np.where(idx < n, x[:, np.minimum(idx, n - 1)], 0.0)


def gcc_phat(x, ref, L, D, NF, block=64):
    """x [C, n] (int16 or float) -> r float64 [C, Wn, 2 D + 1], column D + tau = lag tau"""
    x = widen(x)
    C, n = x.shape
    Wn = windows(n, L)
    h = hann(L)
    r = np.empty((C, Wn, 2 * D + 1))
    for w0 in range(0, Wn, block):
        w1 = min(Wn, w0 + block)
        X = np.fft.rfft(frames(x, L, w0, w1) * h, NF, axis=-1)
        P = X * np.conj(X[ref])[None]
        G = P / np.maximum(np.abs(P), EPS)
        rr = np.fft.irfft(G, NF, axis=-1)
        r[:, w0:w1] = np.concatenate([rr[..., NF - D:], rr[..., :D + 1]], axis=-1)
    return r


def _best_predecessor(prev, gamma):
    """for every state s: (max_s' (prev[s'] - gamma |s - s'|), its s'); ties to the smaller |s - s'|, then the smaller s'"""
    S = len(prev)
    s = np.arange(S)
    dist = np.abs(s[:, None] - s[None, :])
    cand = prev[None, :] - gamma * dist.astype(np.float64)            # one rounded product, one rounded difference
    mx = cand.max(axis=1)
    key = np.where(cand == mx[:, None], dist * (2 * S) + s[None, :], np.iinfo(np.int64).max)
    return mx, key.argmin(axis=1)


def track_channel(r, gamma):
    """r [Wn, S] -> the lag index (0 .. S - 1) per window"""
    r = np.asarray(r, np.float32).astype(np.float64)
    Wn, S = r.shape
    D = (S - 1) // 2
    score = r[0].copy()
    bp = np.zeros((Wn, S), np.int64)
    for w in range(1, Wn):
        mx, bp[w] = _best_predecessor(score, gamma)
        score = r[w] + mx
    s = np.arange(S)
    key = np.where(score == score.max(), np.abs(s - D) * (2 * S) + s, np.iinfo(np.int64).max)
    path = np.empty(Wn, np.int64)
    path[-1] = key.argmin()
    for w in range(Wn - 1, 0, -1):
        path[w - 1] = bp[w, path[w]]
    return path


def weights(r, tau, ref):
    """r [C, Wn, S], tau [C, Wn] -> a float32 [C, Wn]"""
    r = np.asarray(r, np.float32).astype(np.float64)
    C, Wn, S = r.shape
    D = (S - 1) // 2
    q = np.maximum(0.0, np.take_along_axis(r, (np.asarray(tau) + D)[..., None], axis=2)[..., 0])
    q[ref] = 0.0
    q[ref] = q.max(axis=0)
    total = np.zeros(Wn)
    for c in range(C):                                                # the sum in channel order
        total = total + q[c]
    a = np.where(total > 0, q / np.where(total > 0, total, 1.0), 0.0)
    a[ref] = np.where(total > 0, a[ref], 1.0)
    return a.astype(np.float32)


def tdoa_track(r, ref, gamma):
    """r [C, Wn, 2 D + 1] (rounded to fp32 first, as the device holds it) -> (tau int32 [C, Wn], a float32 [C, Wn])"""
    C, Wn, S = r.shape
    D = (S - 1) // 2
    tau = np.zeros((C, Wn), np.int32)
    for c in range(C):
        if c != ref:
            tau[c] = track_channel(r[c], gamma) - D
    return tau, weights(r, tau, ref)


def raw_argmax(r):
    """the lag of the largest value per window, untracked: [..., Wn]"""
    D = (r.shape[-1] - 1) // 2
    return r.argmax(axis=-1) - D


def fade(n, L, Wn):
    """per sample (w0, w1, f): y = (1 - f) z_w0 + f z_w1"""
    H = L // 2
    t = np.arange(n)
    q = t - H
    w0 = np.where(q < 0, 0, q // H)
    f = np.where(q < 0, 0.0, (q - w0 * H) / float(H))
    last = w0 >= Wn - 1
    w0 = np.where(last, Wn - 1, w0)
    f = np.where(last, 0.0, f)
    return w0, np.minimum(w0 + 1, Wn - 1), f


def delay_sum(x, tau, a, L):
    """x [C, n], tau int [C, Wn], a [C, Wn] -> y float64 [n]"""
    x = widen(x)
    C, n = x.shape
    tau, a = np.asarray(tau, np.int64), np.asarray(a, np.float32).astype(np.float64)
    Wn = tau.shape[1]
    w0, w1, f = fade(n, L, Wn)
    t = np.arange(n)

    def z(w):
        acc = np.zeros(n)
        for c in range(C):
            i = t + tau[c, w]
            ok = (i >= 0) & (i < n)
            acc = acc + a[c, w] * np.where(ok, x[c, np.clip(i, 0, n - 1)], 0.0)
        return acc
    return (1.0 - f) * z(w0) + f * z(w1)


def enhance(x, ref, L, D, NF, gamma):
    """the three calls chained as las.beamform does: r is rounded to fp32 between the first two"""
    r = gcc_phat(x, ref, L, D, NF).astype(np.float32)
    tau, a = tdoa_track(r, ref, gamma)
    return delay_sum(x, tau, a, L), tau, a, r


# ---- generators ----------------------------------------------------------------------------------------------------------------------

def ar1(rng, n, pole):
    from scipy.signal import lfilter
    y = lfilter([1.0], [1.0, -pole], rng.randn(n))
    return y / np.sqrt(np.mean(y * y))


def array_recording(seconds=6.0, fs=16000, delays=((0, 7, -12, 3), (0, -5, 9, -20)), snr_db=0.0, pause=None, seed=0, level=0.05):
    """Two coloured-noise voices (AR(1), poles 0.9 and 0.5) one after the other, each half of the recording; channel c hears voice v
    delayed by delays[v][c] samples (x_c[t] = s_v[t - delay]) plus independent white noise at snr_db per channel.  pause = (t0, t1) in
    seconds silences the voices there (the noise stays).  -> (x float32 [C, n], clean float64 [n] = the sources as channel 0 would hear
    them without noise, voice int [n]: 0 / 1, -1 in the pause, delays)"""
    rng = np.random.RandomState(seed)
    n = int(seconds * fs)
    half = n // 2
    C = len(delays[0])
    pad = 64
    src = [ar1(rng, n + 2 * pad, 0.9) * level, ar1(rng, n + 2 * pad, 0.5) * level]
    voice = np.where(np.arange(n) < half, 0, 1)
    if pause is not None:
        voice[int(pause[0] * fs):int(pause[1] * fs)] = -1
    t = np.arange(n)
    x = np.zeros((C, n))
    clean = np.zeros(n)
    for v in (0, 1):
        on = voice == v
        for c in range(C):
            x[c] += np.where(on, src[v][pad + t - delays[v][c]], 0.0)
        clean += np.where(on, src[v][pad + t - delays[v][0]], 0.0)
    noise = level * 10.0 ** (-snr_db / 20.0)
    x += noise * rng.randn(C, n)
    return x.astype(np.float32), clean, voice, np.asarray(delays)


def active_windows(voice, L, v):
    """the windows that lie wholly inside voice v"""
    H = L // 2
    n = len(voice)
    return [w for w in range(windows(n, L)) if w * H + L <= n and (voice[w * H:w * H + L] == v).all()]


def snr_db(y, clean, on):
    """of the samples `on`, after the least-squares gain of clean in y"""
    y, c = np.asarray(y, np.float64)[on], clean[on]
    g = np.dot(y, c) / np.dot(c, c)
    return 10.0 * np.log10(np.dot(g * c, g * c) / np.dot(y - g * c, y - g * c))


def exact_tracker_input(C, Wn, D, seed, ties=True):
    """r float32 [C, Wn, 2 D + 1] in multiples of 2^-10 within [-1, 1], for gamma = 2^-7 (or any multiple of 2^-10 up to 1): every product,
    difference and sum of the recursion is then exact in double, and equal values -- ties -- occur and mean something.  With ties, a
    few rows are built to tie: a constant row (every predecessor reachable at the same value but for the penalty), two equal peaks
    at mirrored lags, and the last window with equal peaks at -3 and +3 and at lag -1 and +1 below them."""
    rng = np.random.RandomState(seed)
    S = 2 * D + 1
    r = rng.randint(-64, 65, size=(C, Wn, S)).astype(np.float64)
    for c in range(C):
        for w in range(Wn):
            r[c, w, rng.randint(S)] += 512                            # a peak that wanders
    if ties:
        for c in range(C):
            if Wn > 2:
                r[c, 1, :] = 16
            if Wn > 4:
                r[c, 3, :] = 0
                r[c, 3, max(0, D - min(D, 5))] = r[c, 3, min(S - 1, D + min(D, 5))] = 640
            r[c, -1, :] = 0
            e = min(D, 3)
            r[c, -1, D - e] = r[c, -1, D + e] = 700
            r[c, -1, D - 1] = r[c, -1, D + 1] = 600
    return (r / 1024.0).astype(np.float32)
