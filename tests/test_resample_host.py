"""Host side of the resampler (no GPU): the float64 statement in preprocess.py (table, lengths, what it does to tones), the refusals of
las_resample that come before any launch, preprocess.py --augmentation through the CPU front end, and utils.augmentation."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import frontend_ref as R
import helpers
import preprocess as pp
import resample_ref as RR
from las import _hip
from las import frontend as FE

FS = 16000


# ---- the definition ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs_in", sorted(RR.TABLE))
def test_table_sizes_and_row_sums(fs_in):
    L, M, W, h = pp.resample_table(fs_in, FS)
    assert (L, M, 2 * W) == RR.TABLE[fs_in]
    assert h.shape == (L, 2 * W) and h.dtype == np.float64
    assert np.abs(h.sum(1) - 1).max() <= 1e-14
    c = 0.92 * min(1.0, L / M)
    assert W == math.ceil(24 / c)
    # the centre tap of phase 0 sits at distance 0: the largest weight, close to c
    assert np.argmax(h[0]) == W - 1 and abs(h[0, W - 1] - c) < 1e-3 * c


def test_output_length_and_equal_rates():
    rng = np.random.RandomState(0)
    for fs_in in RR.TABLE:
        L, M, _ = RR.TABLE[fs_in]
        for n in (1, 7, 441, 442, 1000):
            assert len(pp.resample(rng.randn(n), fs_in, FS)) == -((-n * L) // M) == pp.resample_out_len(n, L, M)
    x = rng.randn(100)
    assert np.array_equal(pp.resample(x, FS, FS, 0.7), 0.7 * x)
    assert np.array_equal(pp.resample(x, FS, FS), x)
    assert np.array_equal(pp.speed_perturb(x, FS, 1.0, 2.0), 2.0 * x)
    assert len(pp.speed_perturb(x, FS, 0.9)) == math.ceil(100 * 10 / 9) and len(pp.speed_perturb(x, FS, 1.1)) == math.ceil(100 * 10 / 11)
    assert np.array_equal(pp.speed_perturb(x, FS, 0.9, 0.5), pp.resample(x, 14400, FS, 0.5))


@pytest.mark.parametrize("fs_in", sorted(RR.TABLE))
def test_a_constant_stays_constant(fs_in):
    L, M, K = RR.TABLE[fs_in]
    y = pp.resample(np.full(3000, 0.25), fs_in, FS)
    skip = math.ceil(K * L / M) + 2
    assert len(y) > 4 * skip
    assert np.abs(y[skip:-skip] - 0.25).max() <= 1e-12


# ---- quality, on the float64 statement ---------------------------------------------------------------------------------------------
def _tone(fs_in, f, n=6000):
    """(interior of the resampled unit sine at f Hz, the analytic sine there)"""
    L, M, K = RR.TABLE[fs_in]
    y = pp.resample(np.sin(2 * np.pi * f * np.arange(n) / fs_in), fs_in, FS)
    skip = math.ceil(K * L / M) + 2
    m = np.arange(len(y))[skip:-skip]
    assert len(m) > 500
    return y[skip:-skip], np.sin(2 * np.pi * f * m / FS)


@pytest.mark.parametrize("fs_in", sorted(RR.TABLE))
def test_passband_tones_come_back(fs_in):
    """a unit sine at 25 % (75 %) of the narrower band comes back within 2e-5 (5e-5) of the analytic sine; measured 5.2e-6 and 1.3e-5
    at worst over the seven ratios, the bars are about 4x that and still below the 3e-5 step of a 16-bit file where it matters"""
    nyq = min(fs_in, FS) / 2
    for frac, bar in ((0.25, 2e-5), (0.75, 5e-5)):
        y, want = _tone(fs_in, frac * nyq)
        err = float(np.abs(y - want).max())
        print("fs_in %d tone at %.0f Hz: err %.2e (bar %.0e)" % (fs_in, frac * nyq, err, bar))
        assert err <= bar


@pytest.mark.parametrize("fs_in,f", [(48000, 10000.0), (44100, 10000.0), (22050, 10000.0), (17600, 8400.0)])
def test_stopband_tone_is_removed(fs_in, f):
    """a unit sine above the new Nyquist (and below the source's: 8400 Hz for 17600 Hz) comes out at 5e-5 at most (measured 6e-6)"""
    assert FS / 2 < f < fs_in / 2
    y, _ = _tone(fs_in, f)
    amp = float(np.abs(y).max())
    print("fs_in %d tone at %.0f Hz: amplitude %.2e" % (fs_in, f, amp))
    assert amp <= 5e-5


def test_ref32_tracks_ref64():
    """the float32 yardstick is the same arithmetic (gap of order 1e-7 on signals of amplitude 0.4) and is not float64 in disguise"""
    for fs_in in (14400, 48000, 44100):
        for int16 in (False, True):
            for w in RR.signals(fs_in, int16, (7, 300, 2500)):
                g = RR.gap(w, fs_in, FS)
                assert g < 2e-6
                assert len(w) < 300 or g > 0
    w = RR.signals(FS, False, (500,))[0]
    assert np.array_equal(RR.ref32(w, FS, FS), w)
    assert np.array_equal(RR.ref32(w, FS, FS, 0.5), np.float32(0.5) * w)


# ---- the C entry -------------------------------------------------------------------------------------------------------------------
def test_out_len():
    l = _hip.lib()
    for fs_in, (L, M, _) in RR.TABLE.items():
        for n in (0, 1, 7, M - 1, M, M + 1, 16037, 2 ** 31 - 2, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 40 + 12345):
            assert l.las_resample_out_len(n, L, M) == -((-n * L) // M) == pp.resample_out_len(n, L, M), (fs_in, n)
    assert l.las_resample_out_len(-1, 1, 1) < 0 and l.las_resample_out_len(5, 0, 1) < 0 and l.las_resample_out_len(5, 1, 0) < 0
    r = FE.Resampler(44100, FS)
    assert (r.L, r.M, r.W, r.K) == (160, 441, 72, 144) and r.out_len(441) == 160 and r.out_len(442) == 161
    assert r.table.dtype == np.float32 and np.array_equal(r.table, pp.resample_table(44100, FS)[3].astype(np.float32))


def test_tile_query():
    """las_resample_tile: a multiple of the 256-thread workgroup for every supported ratio, 0 for what las_resample refuses"""
    l = _hip.lib()
    for fs_in, (L, M, K) in RR.TABLE.items():
        t = l.las_resample_tile(L, M, K // 2)
        assert t >= 256 and t % 256 == 0, (fs_in, t)
    assert l.las_resample_tile(0, 1, 27) == 0 and l.las_resample_tile(1, 1, 0) == 0 and l.las_resample_tile(1, 1, 513) == 0
    assert l.las_resample_tile(1, 64, 512) == 0                      # 256 outputs would read 255 * 64 + 1024 samples


def test_c_entry_validates_before_any_launch():
    """las_resample refuses bad arguments on the host (nothing here is a device pointer: a launch would fault)"""
    l = _hip.lib()
    dummy = ctypes.c_void_p(256)

    def call(ns=(16037, 7), **over):
        host = (ctypes.c_int * len(ns))(*ns)
        kw = dict(in_=dummy, in_i16=0, ld_in=16040, n_in=dummy, n_in_host=host, n=len(ns), L=10, M=9, W=27, table=dummy, gain=None,
                  out=dummy, ld_out=17824, n_out=None)
        kw.update(over)
        a = _hip.ResampleArgs(**kw)
        return l.las_resample(ctypes.byref(a), None), l.las_last_error()

    rc = l.las_resample(None, None)
    assert rc < 0 and b"null argument struct" in l.las_last_error()
    for ptr in ("in_", "n_in", "table", "out"):
        rc, msg = call(**{ptr: None})
        assert rc < 0 and b"null pointer" in msg, ptr
    rc, msg = call(L=0)
    assert rc < 0 and b"0/9" in msg
    rc, msg = call(M=-3)
    assert rc < 0 and b"10/-3" in msg
    rc, msg = call(W=0)
    assert rc < 0 and b"W=0" in msg
    rc, msg = call(W=513)
    assert rc < 0 and b"W=513" in msg and b"1024" in msg
    rc, msg = call(L=2048, M=2047, W=512)
    assert rc < 0 and b"2048/2047" in msg and b"entries" in msg     # L * 2W > 2^20
    rc, msg = call(L=1, M=64, W=512)
    assert rc < 0 and b"1/64" in msg and b"staging" in msg
    rc, msg = call(n=0)
    assert rc < 0 and b"n=0" in msg
    rc, msg = call(n=65536)
    assert rc < 0 and b"n=65536" in msg
    rc, msg = call(ns=(16037, 0))
    assert rc < 0 and b"utterance 1 has 0 samples" in msg
    rc, msg = call(ns=(16041, 7))
    assert rc < 0 and b"utterance 0 has 16041 samples" in msg        # longer than the row pitch
    rc, msg = call(ld_out=17818)                                     # ceil(16037 * 10 / 9) = 17819
    assert rc < 0 and b"17819" in msg and b"ld_out=17818" in msg
    rc, msg = call(ld_out=2 ** 31)
    assert rc < 0 and b"ld_out" in msg
    rc, msg = call(table=ctypes.c_void_p(260))
    assert rc < 0 and b"8-byte" in msg                               # rows are read two taps per load
    rc, msg = call(L=1, M=1, ld_out=16036)                           # the gain-only path checks its lengths too
    assert rc < 0 and b"ld_out=16036" in msg


# ---- preprocess.py --augmentation, CPU front end -----------------------------------------------------------------------------------
def _child(argv):
    return subprocess.run([sys.executable] + argv, cwd=helpers.PKG, env=dict(os.environ), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=300)


def test_preprocess_augmentation_cpu(tmp_path):
    import joblib
    waves = RR.signals(FS, False, (4000, 9037, 3000))
    train, dev = RR.make_corpus(tmp_path, "train", waves[:2]), RR.make_corpus(tmp_path, "dev", waves[2:])
    out = {}
    for aug in ("True", "False"):
        out[aug] = tmp_path / ("feats_" + aug)
        r = _child(["preprocess.py", "--augmentation", aug, "--frontend", "cpu", "--unit", "char", "--feat_dim", "13",
                    "--train_100hr_corpus_dir", train, "--dev_data_dir", dev, "--test_data_dir", str(tmp_path / "none"), "--feat_dir", str(out[aug])])
        assert r.returncode == 0, r.stderr[-2000:]
    plain = sorted(os.listdir(out["False"]))
    assert not [f for f in plain if f.startswith("speed_")]
    speed_files = ["speed_%s-%s" % (s, kind) for s in ("0.9", "1.1") for kind in ("featlen.npy", "feats.pkl")]
    assert sorted(os.listdir(out["True"])) == sorted(plain + speed_files)
    a = R.fe_args(FS, "mfcc", 13, True)
    for f in plain:                                                   # the plain dumps are what they are without the flag
        if f.endswith("feats.pkl"):
            for x, y in zip(joblib.load(str(out["True"] / f)), joblib.load(str(out["False"] / f))):
                assert np.array_equal(x, y)
    for s, (L, M) in (("0.9", (10, 9)), ("1.1", (10, 11))):
        feats = joblib.load(str(out["True"] / ("speed_%s-feats.pkl" % s)))
        featlen = np.load(str(out["True"] / ("speed_%s-featlen.npy" % s)))
        assert len(feats) == len(featlen) == 2                        # the train split's two recordings: the dev split is not perturbed
        for w, f, t in zip(waves[:2], feats, featlen):
            assert t == FE.frame_count(math.ceil(len(w) * L / M), 400, 160) == len(f)
            assert np.array_equal(f, R.ref64(pp.speed_perturb(w.astype(float), FS, float(s)), a))
    # a corpus with a dev split only: nothing to perturb
    only_dev = tmp_path / "feats_dev"
    r = _child(["preprocess.py", "--augmentation", "True", "--frontend", "cpu", "--unit", "char", "--feat_dim", "13", "--train_100hr_corpus_dir",
                str(tmp_path / "none"), "--dev_data_dir", dev, "--test_data_dir", str(tmp_path / "none"), "--feat_dir", str(only_dev)])
    assert r.returncode == 0, r.stderr[-2000:]
    assert os.listdir(only_dev) and not [f for f in os.listdir(only_dev) if f.startswith("speed_")]


# ---- utils.augmentation ------------------------------------------------------------------------------------------------------------
def test_speed_and_volume_augmentation_files(tmp_path):
    from scipy.io import wavfile
    from utils import augmentation as A
    src = tmp_path / "src"
    src.mkdir()
    waves = RR.signals(FS, True, (1200, 2001))
    files = [str(src / "utt0.wav"), str(src / "utt1.take2.npy")]       # (.npy: raw 16 kHz samples, as read_audio takes them)
    wavfile.write(files[0], FS, waves[0])
    np.save(files[1], waves[1].astype(float) / 32767)
    stems = ["utt0", "utt1.take2"]
    for speed, (L, M) in ((0.9, (10, 9)), (1.1, (10, 11))):
        got = A.SpeedAugmentation(files, str(tmp_path / "speed_aug"), speed)
        assert got == [str(tmp_path / ("speed_aug_%s" % speed) / ("%s_%s.wav" % (st, speed))) for st in stems]
        for w, p in zip(waves, got):
            fs, y = wavfile.read(p)
            want = pp.speed_perturb(w.astype(float) / 32767, FS, speed)
            assert fs == FS and y.dtype == np.int16 and len(y) == math.ceil(len(w) * L / M) == len(want)
            assert np.array_equal(y, np.round(np.clip(want, -1, 1) * 32767).astype(np.int16))
            back, fs_back = pp.read_audio(p)                          # a result is a source again
            assert fs_back == FS and np.array_equal(back, y.astype(float) / 32767)
    got = A.VolumeAugmentation(files, str(tmp_path / "vol_aug"), [0.8, 1.5])
    assert len(got) == 2
    gains = []
    for w, p, st in zip(waves, got, stems):
        folder, name = os.path.split(p)
        assert folder == str(tmp_path / "vol_aug") and name.startswith(st + "_") and name.endswith(".wav")
        g = float(name[len(st) + 1:-4])                               # the gain is in the name, to two decimals
        assert 0.8 <= g <= 1.5 and abs(g * 100 - round(g * 100)) < 1e-9
        gains.append(g)
        fs, y = wavfile.read(p)
        assert fs == FS and y.dtype == np.int16 and len(y) == len(w)
        assert np.array_equal(y, np.round(np.clip(g * (w.astype(float) / 32767), -1, 1) * 32767).astype(np.int16))
