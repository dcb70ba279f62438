"""Yardsticks of the resampler tests (not a test module).

ref64: preprocess.resample, the float64 statement.  ref32: the same taps read from the same fp32 table (preprocess.resample_table
rounded once, what the device reads), multiplied and accumulated in float32 numpy in ascending tap order: how far a correct fp32
evaluation sits from float64 on a given input -- the unit the GPU parity bar is expressed in.  Neither is used by the product."""
import numpy as np

import frontend_ref as R
from frontend_ref import pp

F = np.float32
# source rates of the tests, all to 16 kHz: speed 0.9, speed 1.1, telephone, 48 kHz, and 44.1 kHz (L = 160: the table read from global memory)
RATES = (14400, 17600, 8000, 48000, 44100)
TABLE = {14400: (10, 9, 54), 17600: (10, 11, 58), 8000: (2, 1, 54), 48000: (1, 3, 158), 44100: (160, 441, 144), 22050: (320, 441, 72),
         11025: (640, 441, 54)}                                      # fs_in -> (L, M, K) at fs_out = 16000


def signals(fs, int16, lengths, seed=0):
    """frontend_ref.signals' recipe at these lengths: noise and noise + chirp, amplitude <= 0.4, no pure tones"""
    return R.signals(fs, int16, seed=seed, lengths=tuple(int(n) for n in lengths))


def make_corpus(root, name, waves):
    """<root>/<name>/spk/chap: the waveforms as 16 kHz .npy recordings with a transcript, as preprocess.data_preparation walks it"""
    d = root / name / "spk" / "chap"
    d.mkdir(parents=True)
    with open(d / "spk-chap.trans.txt", "w") as f:
        for i, w in enumerate(waves):
            np.save(str(d / ("spk-chap-%04d.npy" % i)), w)
            f.write("spk-chap-%04d HELLO WORLD\n" % i)
    return str(root / name)


def ref64(wave, fs_in, fs_out, gain=1.0):
    return pp.resample(R._as_float64(wave), fs_in, fs_out, gain)


def ref32(wave, fs_in, fs_out, gain=None):
    wave = np.asarray(wave)
    x = wave.astype(F) / F(32767) if wave.dtype.kind == "i" else wave.astype(F)
    if fs_in == fs_out:
        return x if gain is None else F(gain) * x
    L, M, W, h = pp.resample_table(fs_in, fs_out)
    h = h.astype(F)
    n_out = pp.resample_out_len(len(x), L, M)
    xp = np.concatenate([np.zeros(W - 1, F), x, np.zeros(W + 1, F)])
    mM = np.arange(n_out, dtype=np.int64) * M
    n0, p = mM // L, mM % L
    acc = np.zeros(n_out, F)
    for i in range(2 * W):                                          # ascending taps, every product and every sum rounded to fp32
        acc = acc + xp[n0 + i] * h[p, i]
    assert acc.dtype == F
    return acc if gain is None else F(gain) * acc


def gap(wave, fs_in, fs_out, gain=None):
    """max |ref32 - ref64| on this input"""
    r64 = ref64(wave, fs_in, fs_out, 1.0 if gain is None else float(F(gain)))
    return float(np.abs(ref32(wave, fs_in, fs_out, gain).astype(np.float64) - r64).max())
