"""The four MVDR calls of include/las_hip.h K19 (las_mvdr_mask, las_mvdr_cov, las_mvdr_weights, las_mvdr_apply) and their
chain restated in float64 numpy, numpy.fft in double, written from the contract and not from the kernels; and the generator of the
recording the tests use.  Nothing here touches a device."""
import numpy as np

import beamform_ref as BR

MAX_CHANNELS, MAX_FFT, MIN_FFT = 16, 1024, 64         # include/las_hip.h LAS_BF_MAX_CHANNELS, LAS_MVDR_MAX_FFT
G_MIN = 1e-6

widen = BR.widen
twiddle = BR.twiddle


def frames(n, NF):
    """Tf = ceil(n / Hs) + 1"""
    Hs = NF // 2
    return -(-n // Hs) + 1


def blocks(Tf, Bf):
    return -(-Tf // Bf)


def window(NF):
    return np.sin(np.pi * (np.arange(NF) + 0.5) / NF)


def frame_samples(x, NF, t0, t1):
    """frames [t0, t1) of the rows of x [..., n] -> [..., t1 - t0, NF]: frame t covers [(t - 1) Hs, (t + 1) Hs), zeros outside [0, n)"""
    Hs = NF // 2
    n = x.shape[-1]
    idx = ((np.arange(t0, t1) - 1) * Hs)[:, None] + np.arange(NF)[None, :]
    return np.where((idx >= 0) & (idx < n), x[..., np.clip(idx, 0, n - 1)], 0.0)


def stft(x, NF):
    """x [C, n] (already widened) -> X complex128 [C, Tf, K]"""
    return np.fft.rfft(frame_samples(x, NF, 0, frames(x.shape[-1], NF)) * window(NF), axis=-1)


def seq_sum(a):
    """the terms added one after the other from 0, each sum rounded once (numpy's own sum adds pairwise)"""
    s = 0.0
    for v in np.asarray(a, np.float64).ravel():
        s = s + v
    return float(s)


def mask(x, ref, NF, ratio, floor, hang):
    """-> (m float32 [Tf], e float64 [Tf]) from channel ref alone"""
    fr = frame_samples(widen(np.asarray(x)[ref]), NF, 0, frames(np.asarray(x).shape[-1], NF))
    e = np.zeros(fr.shape[0])
    for i in range(NF):                               # ascending order from 0 (a sample outside [0, n) adds an exact 0)
        e = e + fr[:, i] * fr[:, i]
    thr = max(e.max() * ratio, floor)
    raw = (e >= thr) & (e > 0)
    Tf = len(e)
    m = np.array([raw[max(0, t - hang):t + hang + 1].any() for t in range(Tf)])
    return m.astype(np.float32), e


def counts_of(m, Bf):
    """[1 + Nb]: N0 (the blocks' noise sums added in block order), then M_b (ascending frame order)"""
    s = np.asarray(m, np.float32).astype(np.float64)
    q = 1.0 - s
    Tf = len(s)
    Nb = blocks(Tf, Bf)
    out = np.zeros(1 + Nb)
    out[1:] = [seq_sum(s[b * Bf:(b + 1) * Bf]) for b in range(Nb)]
    out[0] = seq_sum([seq_sum(q[b * Bf:(b + 1) * Bf]) for b in range(Nb)])
    return out


def _hermitian(P):
    """the upper triangle kept, the lower its conjugate, the diagonal real"""
    C = P.shape[-1]
    iu = np.triu(np.ones((C, C), bool), 1)
    up = np.where(iu, P, 0.0)
    d = np.zeros_like(P)
    i = np.arange(C)
    d[..., i, i] = P[..., i, i].real
    return up + np.conj(np.swapaxes(up, -1, -2)) + d


def cov(x, m, NF, Bf):
    """x [C, n], m [Tf] in [0, 1] -> (counts [1 + Nb], phi_n complex128 [K, C, C], phi_y [Nb, K, C, C]); every sum in float64"""
    X = stft(widen(x), NF)
    C, Tf, K = X.shape
    s = np.asarray(m, np.float32).astype(np.float64)
    q = 1.0 - s
    cnt = counts_of(m, Bf)
    Nb = len(cnt) - 1
    phi_n = np.zeros((K, C, C), complex)
    if cnt[0] != 0:
        phi_n = np.einsum("t,itk,jtk->kij", q, X, X.conj()) / cnt[0]
    phi_y = np.zeros((Nb, K, C, C), complex)
    for b in range(Nb):
        if cnt[1 + b] != 0:
            sl = slice(b * Bf, min(Tf, (b + 1) * Bf))
            phi_y[b] = np.einsum("t,itk,jtk->kij", s[sl], X[:, sl], X[:, sl].conj()) / cnt[1 + b]
    return cnt, _hermitian(phi_n), _hermitian(phi_y)


def solve_bin(phi_n_k, phi_y_bk, loading):
    """-> (G = A^-1 P, tn) or (None, tn) where A does not factorise"""
    from scipy.linalg import solve_triangular
    C = phi_n_k.shape[0]
    tn = np.trace(phi_n_k).real / C
    if not tn > 0:
        return None, tn
    A = phi_n_k + loading * tn * np.eye(C)
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return None, tn
    P = phi_y_bk - phi_n_k
    return solve_triangular(L.conj().T, solve_triangular(L, P, lower=True), lower=False), tn


def weights(phi_n, phi_y, counts, ref, loading, return_g=False):
    """-> (w complex128 [Nb, K, C], valid int32 [Nb, K]) (and g [Nb, K], NaN where no solve was made)"""
    Nb, K, C, _ = phi_y.shape
    raw = np.zeros((Nb, K, C), complex)
    valid = np.zeros((Nb, K), np.int32)
    gs = np.full((Nb, K), np.nan)
    for k in range(K):
        for b in range(Nb):
            G, tn = solve_bin(phi_n[k], phi_y[b, k], loading)
            if G is None:
                continue
            g = np.trace(G).real
            gs[b, k] = g
            if counts[0] > 0 and counts[1 + b] > 0 and tn > 0 and g > G_MIN:
                valid[b, k] = 1
                raw[b, k] = G[:, ref] / g
    w = np.zeros((Nb, K, C), complex)
    e_ref = np.zeros(C, complex)
    e_ref[ref] = 1.0
    for k in range(K):
        ok = np.flatnonzero(valid[:, k])
        for b in range(Nb):
            before = ok[ok <= b]
            w[b, k] = raw[before[-1], k] if len(before) else raw[ok[0], k] if len(ok) else e_ref
    return (w, valid, gs) if return_g else (w, valid)


def identity_weights(Nb, K, C, ref):
    w = np.zeros((Nb, K, C), complex)
    w[:, :, ref] = 1.0
    return w


def apply(x, w, NF, Bf):
    """x [C, n], w [Nb, K, C] -> y float64 [n]; w is rounded to fp32 once, as the device holds it"""
    xw = widen(x)
    n = xw.shape[-1]
    X = stft(xw, NF)
    C, Tf, K = X.shape
    Hs = NF // 2
    w32 = np.asarray(w).astype(np.complex64).astype(np.complex128)
    Y = np.zeros((Tf, K), complex)
    for c in range(C):                                # in channel order
        Y = Y + np.conj(w32[np.arange(Tf) // Bf, :, c]) * X[c]
    f = np.fft.irfft(Y, NF, axis=-1) * window(NF)     # (irfft drops the imaginary parts of the two real bins)
    y = f[:-1, Hs:] + f[1:, :Hs]                      # segment j = f_j's second half + f_j+1's first half
    return y.reshape(-1)[:n]


def geometry(frame_ms, block_ms, pad_ms, top_db, fs):
    """-> (NF, Bf, hang, ratio) as las.beamform derives them from the flags"""
    NF = BR.next_pow2(int(np.ceil(frame_ms * fs / 1000.0 - 1e-9)))
    hop_ms = 1000.0 * (NF // 2) / fs
    return NF, max(1, int(round(block_ms / hop_ms))), int(round(pad_ms / hop_ms)), 10.0 ** (-top_db / 10.0)


def enhance(x, ref, NF, Bf, ratio, floor, hang, loading):
    """the four calls chained as las.beamform chains them -> (y float64 [n], dict of the intermediate results)"""
    m, e = mask(x, ref, NF, ratio, floor, hang)
    cnt, phi_n, phi_y = cov(x, m, NF, Bf)
    w, valid = weights(phi_n, phi_y, cnt, ref, loading)
    return apply(x, w, NF, Bf), dict(m=m, energy=e, counts=cnt, phi_n=phi_n, phi_y=phi_y, w=w, valid=valid)


# ---- the recording ---------------------------------------------------------------------------------------------------------------------

def delayed(s, d):
    """s delayed by d samples (fractional), through the spectrum of the zero-padded signal"""
    N = BR.next_pow2(len(s) + 1024)
    S = np.fft.rfft(s, N)
    return np.fft.irfft(S * np.exp(-2j * np.pi * np.arange(len(S)) * d / N), N)[:len(s)]


VOICE_DELAYS = (0.0, 7.3, -12.6, 3.4)
VOICE2_DELAYS = (0.0, -9.4, 4.7, 15.2)
INTERFERER_DELAYS = (0.0, -5.5, 9.2, -20.7)


def recording(seconds=6.0, fs=16000, delays=(VOICE_DELAYS,), interferer=INTERFERER_DELAYS, interferer_db=0.0, sensor_db=-20.0, lead=1.5,
              tail=1.0, seed=0, level=0.05):
    """beamform_ref.array_recording's voices (AR(1) coloured noise, poles 0.9 and 0.5) at FRACTIONAL delays, one after the other in equal
    shares of [lead, seconds - tail) -- the first `lead` and the last `tail` seconds are voice-free -- plus a directional interferer
    (AR(1), pole 0.5) from its own delays at interferer_db against a voice, throughout, plus independent white sensor noise at
    sensor_db.  -> (x float32 [C, n], clean float64 [n] = the voices as channel 0 hears them, voice int [n]: the talker, -1 = none)"""
    rng = np.random.RandomState(seed)
    n = int(seconds * fs)
    C = len(delays[0])
    poles = (0.9, 0.5)
    a0, a1 = int(lead * fs), n - int(tail * fs)
    voice = np.full(n, -1)
    x = np.zeros((C, n))
    clean = np.zeros(n)
    for v, dl in enumerate(delays):
        s0, s1 = a0 + (a1 - a0) * v // len(delays), a0 + (a1 - a0) * (v + 1) // len(delays)
        voice[s0:s1] = v
        s = BR.ar1(rng, n, poles[v % 2]) * level * (voice == v)
        for c in range(C):
            x[c] += delayed(s, dl[c])
        clean += delayed(s, dl[0])
    if interferer is not None:
        s = BR.ar1(rng, n, 0.5) * level * 10.0 ** (interferer_db / 20.0)
        for c in range(C):
            x[c] += delayed(s, interferer[c])
    x += level * 10.0 ** (sensor_db / 20.0) * rng.randn(C, n)
    return x.astype(np.float32), clean, voice


def delay_sum_true(x, delays, L=8000):
    """beamform_ref.delay_sum with the true delays rounded, equal weights: the ideal fixed beamformer of this file"""
    C, n = x.shape
    Wn = BR.windows(n, L)
    tau = np.repeat(np.round(np.asarray(delays)).astype(np.int64)[:, None], Wn, axis=1)
    return BR.delay_sum(x, tau, np.full((C, Wn), 1.0 / C, np.float32), L)


def inside(voice, v, NF):
    """the samples of talker v at least a frame away from where it starts and ends"""
    idx = np.flatnonzero(voice == v)
    on = np.zeros(len(voice), bool)
    on[idx[0] + NF:idx[-1] + 1 - NF] = True
    return on
