"""Host side of the audio front end (no GPU): the float32 yardstick against the float64 restatement, the frame-count formula, the
refusals that come before any launch, and the tables the kernels read."""
import ctypes

import numpy as np
import pytest

import frontend_ref as R
import preprocess as pp
from las import _hip
from las import frontend as FE


def test_ref64_is_process_audios(tmp_path):
    """the in-memory float64 reference of these tests is preprocess.process_audios on the same samples (16 kHz .npy recordings)"""
    waves = R.signals(16000, False, seed=3, lengths=(720, 4000, 16037))
    paths = []
    for i, w in enumerate(waves):
        paths.append(str(tmp_path / ("u%d.npy" % i)))
        np.save(paths[-1], w)
    for ft, fd, cm in (("mfcc", 13, True), ("fbank", 40, True), ("mfcc", 20, False)):
        a = R.fe_args(16000, ft, fd, cm)
        feats, lens = pp.process_audios(paths, a)
        for w, f, l in zip(waves, feats, lens):
            r = R.ref64(w, a)
            assert r.shape == f.shape and l == len(r)
            assert np.array_equal(r, f)


@pytest.mark.parametrize("int16", [False, True])
@pytest.mark.parametrize("ft,fd", [("mfcc", 13), ("mfcc", 20), ("fbank", 40)])
def test_float32_evaluation_tracks_float64(ft, fd, int16):
    """ref32 is the same algorithm: on broadband signals it stays within 1e-3 of float64 (features of magnitude 1-14 carried through
    ~1e3 fp32 operations of relative error 6e-8 each, CMVN dividing by standard deviations of order 1; measured 2e-6 to 7e-5) and is
    not float64 in disguise (the gap is not 0)."""
    for fs in (16000, 8000):
        for cm in (True, False):
            a = R.fe_args(fs, ft, fd, cm)
            gaps = []
            for w in R.signals(fs, int16, seed=1):
                r64, r32 = R.ref64(w, a), R.ref32(w, a)
                assert r32.shape == r64.shape and r32.dtype == np.float32
                gaps.append(float(np.abs(r32.astype(np.float64) - r64).max()))
            print(ft, fd, fs, cm, int16, ["%.2e" % g for g in gaps])
            assert max(gaps) < 1e-3
            assert max(gaps) > 0


def test_frame_count_formula():
    for fs, fl_ms, st_ms in ((16000, 25, 10), (8000, 25, 10), (16000, 20, 10), (16000, 32, 8)):
        fl, step = FE.frame_geometry(fs, fl_ms, st_ms)
        assert fl == int(np.round(fs * fl_ms / 1000)) and step == int(np.round(fs * st_ms / 1000))
        for n in (fl - 1, fl, fl + step - 1, fl + step, fl + step + 1, fl + 2 * step, 16037, 32000):
            frames = pp.stack_frames(np.zeros(n), fs, fl_ms / 1000, st_ms / 1000)
            assert FE.frame_count(n, fl, step) == frames.shape[0], (fs, n)
    fe = FE.FeatureExtractor(R.fe_args())
    assert fe.frame_counts([560, 720, 4000, 16037, 32000]).tolist() == [1, 2, 22, 97, 197]
    assert fe.frame_counts([560]).dtype == np.int32


def test_host_refusals():
    with pytest.raises(ValueError, match="512"):
        FE.FeatureExtractor(R.fe_args(frame_length=40))               # 640 samples at 16 kHz
    FE.FeatureExtractor(R.fe_args(frame_length=32))                   # 512 samples: fits
    FE.FeatureExtractor(R.fe_args(fs=8000, frame_length=40))          # 320 samples
    fe = FE.FeatureExtractor(R.fe_args())
    with pytest.raises(ValueError, match="too short"):
        fe.frame_counts([32000, 559])                                 # one full frame, which the formula drops: no frame
    with pytest.raises(ValueError, match="too short"):
        fe.frame_counts([100])
    with pytest.raises(ValueError):
        FE.FeatureExtractor(R.fe_args(feat_type="mfcc", feat_dim=41))
    with pytest.raises(ValueError):
        FE.FeatureExtractor(R.fe_args(feat_type="plp"))


def test_c_entry_validates_before_any_launch():
    """las_frontend refuses bad arguments on the host (nothing here is a device pointer: a launch would fault)"""
    l = _hip.lib()
    ns = (ctypes.c_int * 2)(32000, 559)
    dummy = ctypes.c_void_p(256)

    def call(**over):
        kw = dict(samples=dummy, samples_i16=0, ld_samples=32000, n_samples=dummy, n_samples_host=ns, n=2, Tmax=197, fl=400, step=160,
                  feat_type=0, feat_dim=13, num_filters=40, cmvn=1, twiddle=dummy, fb=dummy, fb_range=dummy, dct=dummy, out=dummy,
                  ws=dummy, ws_bytes=1 << 30)
        kw.update(over)
        a = _hip.FrontendArgs(**kw)
        return l.las_frontend(ctypes.byref(a), None), l.las_last_error()

    rc, msg = call()
    assert rc < 0 and b"utterance 1" in msg                           # too short for one frame
    rc, msg = call(fl=513)
    assert rc < 0 and b"513" in msg
    rc, msg = call(n=1, Tmax=100)
    assert rc < 0 and b"Tmax" in msg
    rc, msg = call(n=1, feat_dim=41)
    assert rc < 0 and b"feat_dim" in msg
    rc, msg = call(n=1, ws_bytes=16)
    assert rc < 0 and b"workspace" in msg
    assert l.las_frontend_workspace_bytes(2, 197, 13, 0) == 0
    assert l.las_frontend_workspace_bytes(2, 197, 13, 1) >= 2 * 197 * 13 * 4 + 2 * 13 * 8


@pytest.mark.parametrize("fs", [16000, 8000])
def test_tables_are_the_float64_tables_rounded(fs):
    from scipy.fftpack import dct
    for ft, fd in (("mfcc", 13), ("mfcc", 20), ("mfcc", 40), ("fbank", 40), ("fbank", 23)):
        t = FE.host_tables(fs, ft, fd)
        nf = 40 if ft == "mfcc" else fd
        fb = pp.filterbanks(nf, 257, fs, 0, fs / 2).astype(np.float32)
        assert t["fb"].dtype == np.float32 and np.array_equal(t["fb"], fb)
        for j in range(nf):                                           # the bin ranges cover every non-zero weight
            lo, hi = t["fb_range"][j]
            mask = np.ones(257, bool)
            mask[lo:hi + 1] = False
            assert not fb[j][mask].any()
        if ft == "mfcc":
            M = dct(np.eye(nf), type=2, norm="ortho", axis=0)[:fd]
            assert t["dct"].shape == (fd, nf) and t["dct"].dtype == np.float32
            assert np.array_equal(t["dct"], M.astype(np.float32))
            # ... which is the closed form s_c cos(pi c (2j + 1) / (2 nf)), s_0 = sqrt(1 / nf), s_c = sqrt(2 / nf) (entries below 1/4:
            # an fp32 rounding is at most 2^-27)
            c, j = np.arange(fd)[:, None], np.arange(nf)[None, :]
            closed = np.cos(np.pi * c * (2 * j + 1) / (2 * nf)) * np.sqrt(2.0 / nf)
            closed[0] *= np.sqrt(0.5)
            assert np.abs(t["dct"].astype(np.float64) - closed).max() <= 2.0 ** -26
        else:
            assert t["dct"] is None
        k = np.arange(257)
        assert np.array_equal(t["twiddle"], np.stack([np.cos(2 * np.pi * k / 512), -np.sin(2 * np.pi * k / 512)], 1).astype(np.float32))
