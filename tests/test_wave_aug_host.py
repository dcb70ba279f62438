"""Host side of the reverberation / noise augmentation (no GPU): the float64 statement in preprocess.py, the plan of las.augment, the
refusals of las_reverb and las_noise_mix that come before any launch, and preprocess.py --noisy_copies through the CPU front end."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import frontend_ref as R
import helpers
import preprocess as pp
import wave_aug_ref as WR
from las import _hip
from las import frontend as FE

FS = 16000


# ---- the definition ----------------------------------------------------------------------------------------------------------------
def test_reverberate_is_an_aligned_convolution():
    rng = np.random.RandomState(0)
    x, h = rng.randn(50), rng.randn(7)
    full = np.convolve(x, h)
    for d in range(len(h)):
        y = pp.reverberate(x, h, d)
        assert len(y) == len(x) and y.dtype == np.float64
        assert np.array_equal(y, full[d:d + len(x)])
        want = [sum(h[k] * x[m + d - k] for k in range(len(h)) if 0 <= m + d - k < len(x)) for m in range(len(x))]
        assert np.abs(y - np.asarray(want)).max() <= 1e-13
        e = np.zeros(len(h))
        e[d] = 1.0
        assert np.array_equal(pp.reverberate(x, e, d), x)             # a unit impulse at `delay` returns the input
    assert len(pp.reverberate(x[:3], rng.randn(40), 17)) == 3          # a response longer than the recording
    assert len(pp.reverberate(x[:1], h, 0)) == 1
    for bad in (-1, len(h)):
        with pytest.raises(ValueError):
            pp.reverberate(x, h, bad)


def test_rir_delay_and_normalisation():
    assert pp.rir_delay([0.1, -0.9, 0.9, 0.2]) == 1                   # the FIRST sample of largest |h|
    assert pp.rir_delay([3.0]) == 0
    h = pp.normalize_rir([3.0, -4.0])
    assert h.dtype == np.float64 and np.array_equal(h, [0.6, -0.8])
    assert abs(np.sum(pp.normalize_rir(np.random.RandomState(1).randn(999)) ** 2) - 1) <= 1e-14
    with pytest.raises(ValueError):
        pp.normalize_rir(np.zeros(5))


@pytest.mark.parametrize("snr_db", [-5.0, 0.0, 12.5, 20.0])
def test_mix_noise_reaches_the_requested_snr(snr_db):
    rng = np.random.RandomState(2)
    s, noise = 0.1 * rng.randn(3000), 0.7 * rng.randn(10000)
    y = pp.mix_noise(s, noise, 1234, snr_db)
    assert len(y) == len(s)
    assert abs(WR.snr_of(y, s) - snr_db) <= 1e-9
    g = pp.noise_gain(s, noise, 1234, snr_db)
    assert np.array_equal(y, s + g * noise[1234:4234])


def test_mix_noise_wraps_and_measures_the_segment_it_uses():
    rng = np.random.RandomState(3)
    s = 0.1 * rng.randn(1000)
    noise = np.concatenate([0.01 * rng.randn(300), 5.0 * rng.randn(40)])        # loud at the end: Pn depends on what is used
    y = pp.mix_noise(s, noise, 330, 10.0)
    v = noise[(330 + np.arange(1000)) % 340]
    assert np.array_equal(v[:10], noise[330:340]) and np.array_equal(v[10:350], noise)
    g = np.sqrt(np.mean(s * s) / (np.mean(v * v) * 10.0))
    assert np.abs(y - (s + g * v)).max() <= 1e-15 and abs(WR.snr_of(y, s) - 10.0) <= 1e-9
    short = pp.mix_noise(s[:5], noise, 0, 10.0)                       # five quiet samples of the noise only
    assert abs(WR.snr_of(short, s[:5]) - 10.0) <= 1e-9
    for bad in (-1, 340):
        with pytest.raises(ValueError):
            pp.mix_noise(s, noise, bad, 10.0)


def test_silence_gives_a_copy():
    rng = np.random.RandomState(4)
    s, noise = 0.1 * rng.randn(100), rng.randn(30)
    y = pp.mix_noise(np.zeros(100), noise, 0, 5.0)
    assert np.array_equal(y, np.zeros(100)) and pp.noise_gain(np.zeros(100), noise, 0, 5.0) == 0.0
    y = pp.mix_noise(s, np.zeros(30), 7, 5.0)
    assert np.array_equal(y, s) and y is not s
    quiet = np.concatenate([np.zeros(200), rng.randn(10)])            # the segment used is silent, the recording is not
    assert np.array_equal(pp.mix_noise(s, quiet, 0, 5.0), s)


def test_synthetic_rir_is_seeded_and_decays_as_asked():
    a, b, c = pp.synthetic_rir(FS, 0.4, 5), pp.synthetic_rir(FS, 0.4, 5), pp.synthetic_rir(FS, 0.4, 6)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert len(a) == 6400 and a[0] == 1.0 and pp.rir_delay(a) == 0 and a.dtype == np.float64
    assert len(pp.synthetic_rir(FS, 0.4, 5, length_s=0.1)) == 1600 and len(pp.synthetic_rir(FS, 2.0, 5)) == pp.RIR_MAX
    for rt60 in (0.2, 0.5, 0.8):
        h = pp.synthetic_rir(FS, rt60, 7, length_s=1.0)
        e = np.cumsum((h[1:] ** 2)[::-1])[::-1]                       # Schroeder's backward integral of the tail
        db = 10 * np.log10(e / e[0])
        t = np.arange(1, len(h)) / FS
        fit = (db < -5) & (db > -35)
        measured = -60.0 / np.polyfit(t[fit], db[fit], 1)[0]
        print("rt60 %.2f measured %.4f" % (rt60, measured))
        assert abs(measured - rt60) <= 0.1 * rt60


# ---- the plan ----------------------------------------------------------------------------------------------------------------------
def _augmenter(**kw):
    from las.augment import WaveAugmenter
    rirs = [pp.synthetic_rir(FS, 0.1, i, length_s=0.02) for i in range(3)]
    noises = [WR.noise_signal(n, 10 + i) for i, n in enumerate((700, 5000))]
    return WaveAugmenter(FS, rirs=rirs, noises=noises, **kw)


def _rows(p):
    return np.stack([p.rir_idx, p.noise_idx, p.noise_off, p.snr_db.view(np.int32)], 1)


def test_plan_is_reproducible_and_independent_of_the_batch_split():
    aug = _augmenter(seed=11)
    whole = aug.plan(40, 5)
    assert np.array_equal(_rows(whole), _rows(aug.plan(40, 5))) and np.array_equal(_rows(whole), _rows(_augmenter(seed=11).plan(40, 5)))
    assert not np.array_equal(_rows(whole), _rows(aug.plan(40, 6))) and not np.array_equal(_rows(whole), _rows(_augmenter(seed=12).plan(40, 5)))
    parts = [aug.plan(7, 5, row0=0, rows_global=40), aug.plan(20, 5, row0=7, rows_global=40), aug.plan(13, 5, row0=27)]
    assert np.array_equal(np.concatenate([_rows(p) for p in parts]), _rows(whole))
    assert np.array_equal(_rows(aug.plan(3, 5, row0=30, rows_global=1000)), _rows(whole)[30:33])
    assert whole.rir_idx.dtype == whole.noise_idx.dtype == whole.noise_off.dtype == np.int32 and whole.snr_db.dtype == np.float32
    assert set(whole.rir_idx.tolist()) == {-1, 0, 1, 2} and set(whole.noise_idx.tolist()) == {0, 1}      # reverb_prob 0.5, noise_prob 1
    assert (whole.snr_db >= 5).all() and (whole.snr_db <= 20).all() and len(set(whole.snr_db.tolist())) == 40
    lens = np.asarray([700, 5000])[whole.noise_idx]
    assert (whole.noise_off >= 0).all() and (whole.noise_off < lens).all() and whole.noise_off.max() >= 700
    with pytest.raises(ValueError):
        aug.plan(5, 0, row0=38, rows_global=40)


def test_plan_respects_probabilities_zero_and_one_and_missing_banks():
    from las.augment import WaveAugmenter
    p = _augmenter(reverb_prob=0.0, noise_prob=0.0).plan(64, 1)
    assert (p.rir_idx == -1).all() and (p.noise_idx == -1).all() and (p.noise_off == 0).all()
    p = _augmenter(reverb_prob=1.0, noise_prob=1.0, snr_db=(7, 7)).plan(64, 1)
    assert (p.rir_idx >= 0).all() and (p.noise_idx >= 0).all() and (p.snr_db == 7).all()
    only_noise = WaveAugmenter(FS, noises=[WR.noise_signal(100, 0)], reverb_prob=1.0)
    p = only_noise.plan(16, 0)
    assert (p.rir_idx == -1).all() and (p.noise_idx == 0).all()
    aug = _augmenter()
    assert aug.rir_bank.dtype == np.float32 and aug.rir_bank.shape == (3, 320) and aug.noise_bank.shape == (2, 5000)
    assert np.abs((aug.rir_bank.astype(np.float64) ** 2).sum(1) - 1).max() < 1e-6 and aug.rir_delay == [0, 0, 0]
    f = aug.fixed_plan(4, rir_idx=2, noise_idx=[0, 1, -1, 0], snr_db=3.0)
    assert f.rir_idx.tolist() == [2] * 4 and f.noise_idx.tolist() == [0, 1, -1, 0] and f.snr_db.tolist() == [3.0] * 4
    for bad in (dict(snr_db=(9, 3)), dict(reverb_prob=1.5), dict(noise_prob=-0.1)):
        with pytest.raises(ValueError):
            _augmenter(**bad)


# ---- the C entries -----------------------------------------------------------------------------------------------------------------
def _ints(v):
    return (ctypes.c_int * len(v))(*v)


def test_queries():
    l = _hip.lib()
    tile, chunk, ntile = l.las_reverb_tile(), l.las_reverb_tap_chunk(), l.las_noise_mix_tile()
    assert tile >= 256 and tile % 256 == 0 and chunk >= 8 and chunk % 8 == 0 and ntile >= 256
    assert l.las_noise_mix_workspace_bytes(0, 100) == 0 and l.las_noise_mix_workspace_bytes(1, 0) == 0
    assert l.las_noise_mix_workspace_bytes(1, 2 ** 31) == 0
    a, b = l.las_noise_mix_workspace_bytes(64, ntile), l.las_noise_mix_workspace_bytes(64, ntile + 1)      # one tile, two tiles per row
    assert 64 * 16 + 64 * 4 <= a and b >= a + 64 * 16 and l.las_noise_mix_workspace_bytes(128, ntile) >= a + 64 * 20


def test_reverb_validates_before_any_launch():
    """las_reverb refuses bad arguments on the host (nothing here is a device pointer: a launch would fault)"""
    l = _hip.lib()
    P = ctypes.c_void_p

    def call(ns=(1000, 7), lens=(300, 16384), delays=(0, 16383), idx=(1, -1), **over):
        kw = dict(in_=P(1 << 20), ld_in=1000, n_in=P(256), n=len(ns), rir=P(512), ld_rir=16384, rir_len=P(768), rir_delay=P(1024), n_rir=len(lens),
                  rir_idx=P(1280), out=P(1 << 24), ld_out=1000, n_in_host=_ints(ns), rir_len_host=_ints(lens), rir_delay_host=_ints(delays),
                  rir_idx_host=_ints(idx))
        kw.update(over)
        rc = l.las_reverb(kw["in_"], kw["ld_in"], kw["n_in"], kw["n_in_host"], kw["n"], kw["rir"], kw["ld_rir"], kw["rir_len"], kw["rir_len_host"],
                          kw["rir_delay"], kw["rir_delay_host"], kw["n_rir"], kw["rir_idx"], kw["rir_idx_host"], kw["out"], kw["ld_out"], None)
        return rc, l.las_last_error()

    for ptr in ("in_", "n_in", "n_in_host", "rir", "rir_len", "rir_len_host", "rir_delay", "rir_delay_host", "rir_idx", "rir_idx_host", "out"):
        rc, msg = call(**{ptr: None})
        assert rc < 0 and b"las_reverb: null pointer" in msg, ptr
    for n in (0, 65536):
        rc, msg = call(n=n)
        assert rc < 0 and b"n=%d" % n in msg
    rc, msg = call(n_rir=0)
    assert rc < 0 and b"bank of 0 responses" in msg
    rc, msg = call(ld_out=0)
    assert rc < 0 and b"ld_out=0" in msg
    rc, msg = call(lens=(300, 0), delays=(0, 0))
    assert rc < 0 and b"response 1 has 0 taps" in msg
    rc, msg = call(lens=(300, 16385))
    assert rc < 0 and b"response 1 has 16385 taps" in msg and b"16384" in msg
    rc, msg = call(ld_rir=296)
    assert rc < 0 and b"response 0 has 300 taps" in msg and b"pitch 296" in msg
    rc, msg = call(delays=(300, 0))
    assert rc < 0 and b"response 0 has its direct path at 300 (0..299)" in msg
    rc, msg = call(delays=(-1, 0))
    assert rc < 0 and b"direct path at -1" in msg
    rc, msg = call(idx=(2, -1))
    assert rc < 0 and b"utterance 0 takes response 2 (-1..1)" in msg
    rc, msg = call(idx=(0, -2))
    assert rc < 0 and b"utterance 1 takes response -2" in msg
    rc, msg = call(ns=(1000, 0))
    assert rc < 0 and b"utterance 1 has 0 samples" in msg
    rc, msg = call(ns=(1001, 7))
    assert rc < 0 and b"utterance 0 has 1001 samples" in msg
    rc, msg = call(ns=(1000, 7), ld_out=999)                           # the output row is shorter than the recording
    assert rc < 0 and b"utterance 0 has 1000 samples" in msg and b"=999" in msg
    for out in ((1 << 20), (1 << 20) + 4 * 1999, (1 << 20) - 4 * 1999):
        rc, msg = call(out=P(out))
        assert rc < 0 and b"in and out overlap" in msg, out
    # (a call that passes every check would launch: with the fake pointers above that is left to the GPU tests)


def test_noise_mix_validates_before_any_launch():
    l = _hip.lib()
    P = ctypes.c_void_p

    def call(ns=(1000, 7), lens=(300, 5000), idx=(1, -1), offs=(4999, 0), snr=(10.0, 0.0), **over):
        kw = dict(in_=P(1 << 20), ld_in=1000, n_in=P(256), n=len(ns), noise=P(512), ld_noise=5000, noise_len=P(768), n_noise=len(lens),
                  noise_idx=P(1024), noise_off=P(1280), snr_db=P(1536), out=P(1 << 24), ld_out=1000, gain_out=None, ws=P(1 << 28),
                  ws_bytes=l.las_noise_mix_workspace_bytes(len(ns), 1000), n_in_host=_ints(ns), noise_len_host=_ints(lens),
                  noise_idx_host=_ints(idx), noise_off_host=_ints(offs), snr_db_host=(ctypes.c_float * len(snr))(*snr))
        kw.update(over)
        rc = l.las_noise_mix(kw["in_"], kw["ld_in"], kw["n_in"], kw["n_in_host"], kw["n"], kw["noise"], kw["ld_noise"], kw["noise_len"],
                             kw["noise_len_host"], kw["n_noise"], kw["noise_idx"], kw["noise_idx_host"], kw["noise_off"], kw["noise_off_host"],
                             kw["snr_db"], kw["snr_db_host"], kw["out"], kw["ld_out"], kw["gain_out"], kw["ws"], kw["ws_bytes"], None)
        return rc, l.las_last_error()

    for ptr in ("in_", "n_in", "n_in_host", "noise", "noise_len", "noise_len_host", "noise_idx", "noise_idx_host", "noise_off", "noise_off_host",
                "snr_db", "snr_db_host", "out", "ws"):
        rc, msg = call(**{ptr: None})
        assert rc < 0 and b"las_noise_mix: null pointer" in msg, ptr
    for n in (0, 65536):
        rc, msg = call(n=n)
        assert rc < 0 and b"n=%d" % n in msg
    rc, msg = call(n_noise=0)
    assert rc < 0 and b"bank of 0 noises" in msg
    rc, msg = call(ld_noise=0)
    assert rc < 0 and b"ld_noise=0" in msg
    rc, msg = call(lens=(0, 5000))
    assert rc < 0 and b"noise 0 has 0 samples" in msg
    rc, msg = call(lens=(300, 5001))
    assert rc < 0 and b"noise 1 has 5001 samples" in msg and b"pitch 5000" in msg
    rc, msg = call(idx=(2, -1))
    assert rc < 0 and b"utterance 0 takes noise 2 (-1..1)" in msg
    rc, msg = call(ns=(1000, 1001))
    assert rc < 0 and b"utterance 1 has 1001 samples" in msg
    rc, msg = call(ns=(0, 7))
    assert rc < 0 and b"utterance 0 has 0 samples" in msg
    rc, msg = call(offs=(5000, 0))
    assert rc < 0 and b"utterance 0 starts at sample 5000 of noise 1 (0..4999)" in msg
    rc, msg = call(offs=(-1, 0))
    assert rc < 0 and b"starts at sample -1" in msg
    rc, msg = call(idx=(0, -1), offs=(300, 0))                         # inside the other noise, behind this one
    assert rc < 0 and b"of noise 0 (0..299)" in msg
    for bad in (float("nan"), float("inf"), -float("inf")):
        rc, msg = call(snr=(bad, 0.0))
        assert rc < 0 and b"utterance 0 at snr_db=" in msg and b"finite" in msg
    rc, msg = call(ws_bytes=l.las_noise_mix_workspace_bytes(2, 1000) - 1)
    assert rc < 0 and b"workspace of" in msg and b"needed" in msg
    rc, msg = call(ws=P((1 << 28) + 4))
    assert rc < 0 and b"8-byte aligned" in msg
    rc, msg = call(out=P((1 << 20) + 4000))                            # overlapping, but not the same buffer
    assert rc < 0 and b"overlap" in msg
    rc, msg = call(out=P(1 << 20), ld_in=1008)                         # in place needs one pitch
    assert rc < 0 and b"in place" in msg
    # rows without noise do not have their offset and SNR checked: nothing reads them
    rc, msg = call(idx=(1, -1), offs=(0, -7), snr=(3.0, float("nan")), ws_bytes=0)
    assert rc < 0 and b"workspace" in msg                             # (stopped by the next check instead)


# ---- preprocess.py --noisy_copies, CPU front end ---------------------------------------------------------------------------------------
def _child(argv):
    return subprocess.run([sys.executable] + argv, cwd=helpers.PKG, env=dict(os.environ), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=300)


def test_preprocess_noisy_copies_cpu(tmp_path):
    import joblib
    from las.arguments import parse_args
    waves = [WR.noise_signal(n, i) for i, n in enumerate((4000, 9037, 3000))]
    train, dev = WR.make_corpus(tmp_path, "train", waves[:2]), WR.make_corpus(tmp_path, "dev", waves[2:])
    noise_dir = tmp_path / "noises"
    noise_dir.mkdir()
    np.save(str(noise_dir / "hum.npy"), WR.noise_signal(2500, 99).astype(float))
    out = tmp_path / "feats"
    flags = ["--augmentation", "True", "--frontend", "cpu", "--unit", "char", "--feat_dim", "13", "--train_100hr_corpus_dir", train, "--dev_data_dir",
             dev, "--test_data_dir", str(tmp_path / "none"), "--feat_dir", str(out), "--noisy_copies", "1", "--rir_synthetic", "2", "--rt60", "0.05,0.1",
             "--noise_dir", str(noise_dir), "--snr_range", "0,10", "--reverb_prob", "1.0", "--seed", "3"]
    r = _child(["preprocess.py"] + flags)
    assert r.returncode == 0, r.stderr[-2000:]
    names = sorted(os.listdir(out))
    assert [f for f in names if f.startswith("noisy_")] == ["noisy_0-featlen.npy", "noisy_0-feats.pkl"]
    assert [f for f in names if f.startswith("speed_")]                # beside the speed dumps
    feats, featlen = joblib.load(str(out / "noisy_0-feats.pkl")), np.load(str(out / "noisy_0-featlen.npy"))
    clean = joblib.load(str(out / "train-100-feats.pkl"))
    assert len(feats) == len(featlen) == 2                             # the train split's two recordings: the dev split is not augmented
    a, args = WR.fe_args(), parse_args(flags)
    aug = pp.wave_augmenter(args)
    assert len(aug.rirs) == 2 and len(aug.noises) == 1
    plan = aug.plan(2, 0)
    assert (plan.rir_idx >= 0).all() and (plan.noise_idx == 0).all()
    for u, (w, f, t) in enumerate(zip(waves[:2], feats, featlen)):
        assert t == FE.frame_count(len(w), 400, 160) == len(f) == len(clean[u])        # lengths and frame counts stay
        assert f.dtype == np.float32 and not np.array_equal(f, clean[u])
        assert np.array_equal(f, R.ref64(pp.augment_wave(w.astype(float), aug, plan, u), a))
    # --noisy_copies without a bank is refused; without --augmentation nothing is written
    r = _child(["preprocess.py"] + flags[:flags.index("--rir_synthetic")] + ["--feat_dir", str(tmp_path / "f2")])
    assert r.returncode != 0 and "needs a bank" in r.stderr
    r = _child(["preprocess.py", "--augmentation", "False"] + flags[2:flags.index("--feat_dir")] + ["--feat_dir", str(tmp_path / "f3")] + flags[flags.index("--noisy_copies"):])
    assert r.returncode == 0 and not [f for f in os.listdir(tmp_path / "f3") if f.startswith("noisy_")]
