"""Yardsticks of the reverberation / noise tests (not a test module).

ref64: preprocess.reverberate / noise_gain / mix_noise, the float64 statement, on the fp32 values the device reads (samples, taps,
noise; snr_db as the fp32 the plan holds).  ref32: the same arithmetic with every product and every sum rounded to float32, the taps
in ascending order: how far a correct fp32 evaluation sits from float64 on a given input -- the unit the GPU parity bar is expressed
in.  Neither is used by the product."""
import numpy as np

import frontend_ref as R
from frontend_ref import pp

F = np.float32
FS = 16000


def noise_signal(n, seed, rms=0.1):
    """n samples of white noise at the given rms, float32"""
    return (rms * np.random.RandomState(seed).randn(int(n))).astype(F)


def response(K, delay, seed):
    """a K-tap response as the bank holds it: a decaying Gaussian tail around a direct path at `delay`, unit energy, float32"""
    rng = np.random.RandomState(seed)
    h = 0.2 * rng.randn(K) * np.exp(-4.0 * np.arange(K) / max(K, 1))
    h[delay] = 1.0
    return pp.normalize_rir(h).astype(F)


def reverb64(x, h, delay):
    return pp.reverberate(np.asarray(x, F).astype(np.float64), np.asarray(h, F).astype(np.float64), delay)


def reverb32_batch(xs, hs, delays):
    """the fp32 evaluation of a batch in one sweep over the taps (ascending k): row u is reverberate(xs[u], hs[u], delays[u]) with
    acc = acc + x * h[k], every product and every sum rounded to float32.  Rows with fewer taps add exact zeros at the end."""
    n = len(xs)
    nmax, K = max(len(x) for x in xs), max(len(h) for h in hs)
    Z = np.zeros((n, nmax + K - 1), F)                               # Z[u, j] = x_u[j - (K - 1) + D_u]: tap k of output m reads Z[m + K - 1 - k]
    H = np.zeros((n, K), F)
    for u, (x, h, d) in enumerate(zip(xs, hs, delays)):
        j0 = K - 1 - d
        Z[u, j0:j0 + len(x)] = x
        H[u, :len(h)] = h
    acc = np.zeros((n, nmax), F)
    for k in range(K):
        acc = acc + Z[:, K - 1 - k:K - 1 - k + nmax] * H[:, k:k + 1]
    assert acc.dtype == F
    return [acc[u, :len(x)] for u, x in enumerate(xs)]


def reverb_gap(xs, hs, delays):
    """(float64 reference per row, max |ref32 - ref64| per row)"""
    r64 = [reverb64(x, h, d) for x, h, d in zip(xs, hs, delays)]
    r32 = reverb32_batch(xs, hs, delays)
    return r64, [float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(r32, r64)]


def gain64(s, noise, off, snr_db):
    return pp.noise_gain(np.asarray(s, F).astype(np.float64), np.asarray(noise, F).astype(np.float64), off, float(F(snr_db)))


def mix64(s, noise, off, snr_db):
    return pp.mix_noise(np.asarray(s, F).astype(np.float64), np.asarray(noise, F).astype(np.float64), off, float(F(snr_db)))


def mix32(s, noise, off, snr_db):
    """mix_noise in float32: the two mean squares, the gain and s + g v, every product and sum rounded to float32"""
    s, noise = np.asarray(s, F), np.asarray(noise, F)
    v = noise[(int(off) + np.arange(len(s), dtype=np.int64)) % len(noise)]
    Ps, Pn = np.sum(s * s, dtype=F) / F(len(s)), np.sum(v * v, dtype=F) / F(len(s))
    if Ps == 0 or Pn == 0:
        return s.copy()
    g = np.sqrt(Ps / (Pn * F(10.0) ** (F(snr_db) / F(10.0))), dtype=F)
    y = s + F(g) * v
    assert y.dtype == F
    return y


def mix_gap(s, noise, off, snr_db):
    r64 = mix64(s, noise, off, snr_db)
    return r64, float(np.abs(mix32(s, noise, off, snr_db).astype(np.float64) - r64).max())


def snr_of(y, s):
    """10 log10(mean s^2 / mean (y - s)^2) in float64"""
    y, s = np.asarray(y, np.float64), np.asarray(s, np.float64)
    return 10.0 * np.log10(np.mean(s * s) / np.mean((y - s) ** 2))


def make_corpus(root, name, waves):
    """<root>/<name>/spk/chap: the waveforms as 16 kHz .npy recordings with a transcript, as preprocess.data_preparation walks it"""
    d = root / name / "spk" / "chap"
    d.mkdir(parents=True)
    with open(d / "spk-chap.trans.txt", "w") as f:
        for i, w in enumerate(waves):
            np.save(str(d / ("spk-chap-%04d.npy" % i)), w)
            f.write("spk-chap-%04d HELLO WORLD\n" % i)
    return str(root / name)


def fe_args():
    return R.fe_args(FS, "mfcc", 13, True)
