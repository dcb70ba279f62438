"""The resampler on the device (csrc/resample.hip through las.frontend.Resampler and FeatureExtractor.extract(rate=, speed=, gain=))
against the float64 statement in preprocess.py, and the entry points built on it.

Shapes: one batch of five rows per ratio -- 7 samples (shorter than the filter's half width), W, one sample less and one more than the
input a workgroup's tile of outputs covers, and 16037 (several tiles, ragged).  The parity bar of a case is max |gpu - float64| <=
max(4 x gap, 1e-6), gap = tests/resample_ref.py's float32 numpy evaluation against float64 on the same batch (two correct fp32
evaluations can sit on opposite sides of float64, and the device's fmaf chain rounds once per tap where numpy rounds twice); gap is
about 1e-7 and a wrong tap, phase or edge shows as 1e-3 or more, so the floor hides nothing.  With LAS_RESAMPLE_PARITY_OUT set every
case appends its record to that file (profiles/resample_parity.jsonl is such a run)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import frontend_ref as R
import helpers
import resample_ref as RR

pytestmark = pytest.mark.gpu

FS = 16000
_resamplers, _batches, _refs, _extractors = {}, {}, {}, {}


def _rs(fs_in):
    from las.frontend import Resampler
    if fs_in not in _resamplers:
        _resamplers[fs_in] = Resampler(fs_in, FS)
    return _resamplers[fs_in]


def _lengths(fs_in):
    r = _rs(fs_in)
    span = math.ceil(r.tile() * r.M / r.L)                            # input samples under one tile of outputs
    return (7, r.W, span - 1, span + 1, 16037)


def _waves(fs_in, int16):
    if (fs_in, int16) not in _batches:
        _batches[(fs_in, int16)] = RR.signals(fs_in, int16, _lengths(fs_in))
    return _batches[(fs_in, int16)]


def _ref(fs_in, int16):
    """(float64 reference per row, the float32 evaluation's gap per row), computed once per case"""
    if (fs_in, int16) not in _refs:
        ws = _waves(fs_in, int16)
        _refs[(fs_in, int16)] = ([RR.ref64(w, fs_in, FS) for w in ws], [RR.gap(w, fs_in, FS) for w in ws])
    return _refs[(fs_in, int16)]


def _fe(a=None):
    from las.frontend import FeatureExtractor
    a = a or R.fe_args(FS, "mfcc", 13, True)
    key = (a.sample_rate, a.feat_type, a.feat_dim, a.cmvn)
    if key not in _extractors:
        _extractors[key] = FeatureExtractor(a)
    return _extractors[key]


@pytest.mark.parametrize("int16", [False, True], ids=["float", "int16"])
@pytest.mark.parametrize("fs_in", RR.RATES)
def test_parity_and_structure(fs_in, int16):
    import torch
    r = _rs(fs_in)
    waves = _waves(fs_in, int16)
    r64, gaps = _ref(fs_in, int16)
    want_len = [r.out_len(len(w)) for w in waves]
    assert want_len == [len(x) for x in r64]
    ld_out = (max(want_len) + 7 + 24) & ~7                            # some columns behind the longest row, too
    poisoned = torch.full((5, ld_out), float("nan"), device="cuda")
    out, n_out = r(waves, out=poisoned)
    torch.cuda.synchronize()
    assert out.data_ptr() == poisoned.data_ptr() and out.dtype == torch.float32
    assert n_out.dtype == torch.int32 and n_out.cpu().tolist() == want_len
    assert not torch.isnan(out).any()
    o = out.cpu().numpy()
    errs = []
    for u in range(5):
        assert (o[u, want_len[u]:] == 0).all()                        # exactly 0 behind n_out[u]
        assert (o[u, :want_len[u]] != 0).any()
        errs.append(float(np.abs(o[u, :want_len[u]].astype(np.float64) - r64[u]).max()))
    bar = max(4 * max(gaps), 1e-6)
    rec = dict(fs_in=fs_in, fs_out=FS, L=r.L, M=r.M, K=r.K, tile=r.tile(), input="int16" if int16 else "float", lengths=[len(w) for w in waves],
               err=max(errs), gap=max(gaps), bar=bar, err_per_utt=errs, gap_per_utt=gaps)
    print(json.dumps(rec))
    if os.environ.get("LAS_RESAMPLE_PARITY_OUT"):
        with open(os.environ["LAS_RESAMPLE_PARITY_OUT"], "a") as f:
            f.write(json.dumps(rec) + "\n")
    assert max(errs) <= bar, rec


def test_gain():
    import torch
    # L = M = 1, no gain, fp32 input: a bit copy (the sign of a zero included)
    w = [x.copy() for x in _waves(14400, False)]
    w[0][:2] = np.asarray([-0.0, 0.0], np.float32)
    same = _rs(FS)
    assert (same.L, same.M) == (1, 1)
    out, n_out = same(w)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert n_out.cpu().tolist() == [len(x) for x in w]
    for u, x in enumerate(w):
        assert np.array_equal(o[u, :len(x)].view(np.int32), x.view(np.int32)) and (o[u, len(x):] == 0).all()
    half, _ = same(w, gain=0.5)
    assert torch.equal(half, 0.5 * out)
    assert np.signbit(half.cpu().numpy()[0, 0])                       # -0 * 0.5 stays -0
    # int16 input through the gain-only path: value / 32767, as las_frontend converts
    wi = _waves(14400, True)
    oi, _ = same(wi)
    assert np.array_equal(oi.cpu().numpy()[4, :16037], wi[4].astype(np.float32) / np.float32(32767))
    # a resampled batch: gain 0.5 = 0.5 x the gain-1 result, bit for bit; gain 1 = no gain; a vector is applied per row
    for fs_in in (14400, 44100):
        r = _rs(fs_in)
        ws = _waves(fs_in, False)
        plain, _ = r(ws)
        one, _ = r(ws, gain=1.0)
        half, _ = r(ws, gain=0.5)
        g = np.asarray([0.5, 2.0, 1.0, 0.25, -1.5], np.float32)
        each, n_out = r(ws, gain=g)
        torch.cuda.synchronize()
        assert torch.equal(one, plain) and torch.equal(half, 0.5 * plain)
        assert torch.equal(each, torch.from_numpy(g).cuda()[:, None] * plain)
        assert n_out.cpu().tolist() == [r.out_len(len(x)) for x in ws]


@pytest.mark.parametrize("fs_in,int16", [(14400, False), (48000, True), (44100, False), (FS, True)])
def test_determinism_and_batch_independence(fs_in, int16):
    import torch
    r = _rs(fs_in)
    waves = _waves(fs_in if fs_in != FS else 14400, int16)
    out, n_out = r(waves)
    again, _ = r(waves)
    torch.cuda.synchronize()
    assert torch.equal(out, again)                                    # two runs: the same bits
    lens = n_out.cpu().tolist()
    for u, w in enumerate(waves):
        alone, n1 = r([w])
        assert n1.cpu().tolist() == [lens[u]]
        assert torch.equal(alone[0, :lens[u]], out[u, :lens[u]]), u   # alone = inside the batch, bit for bit


# ---- in front of las_frontend ------------------------------------------------------------------------------------------------------
def _feature_case(waves, eff, **kw):
    """extract(waves, **kw) against frontend_ref.ref64 of the float64-resampled recordings; the bar's gap is the float32 resampling
    followed by the float32 front end against the same float64 result"""
    import torch
    a = R.fe_args(FS, "mfcc", 13, True)
    fe = _fe(a)
    cube, lens = fe.extract(waves, **kw)
    torch.cuda.synchronize()
    c = cube.cpu().numpy()
    assert not np.isnan(c).any() and lens.dtype == np.int32
    errs, gaps = [], []
    for u, w in enumerate(waves):
        n_rs = math.ceil(len(w) * FS / eff)
        assert lens[u] == (n_rs - 400) // 160                         # the host formula on the resampled length
        r64 = R.ref64(RR.ref64(w, eff, FS), a)
        assert len(r64) == lens[u]
        gaps.append(float(np.abs(R.ref32(RR.ref32(w, eff, FS), a).astype(np.float64) - r64).max()))
        errs.append(float(np.abs(c[u, :lens[u]].astype(np.float64) - r64).max()))
        assert (c[u, lens[u]:] == 0).all()
    bar = max(4 * max(gaps), 1e-5)
    print(json.dumps(dict(eff=eff, err=max(errs), gap=max(gaps), bar=bar, err_per_utt=errs, gap_per_utt=gaps)))
    assert max(errs) <= bar
    return cube, lens


def test_extract_at_another_rate():
    _feature_case(RR.signals(48000, False, (1700, 2200, 12000, 48111)), 48000, rate=48000)
    _feature_case(RR.signals(48000, True, (1700, 12000)), 48000, rate=[48000, 48000])


def test_extract_speed_perturbed():
    import torch
    waves = RR.signals(FS, False, (560, 720, 4000, 16037))
    cube, lens = _feature_case(waves, 14400, speed=0.9)
    same, lens2 = _fe().extract(waves, rate=14400)                    # `speed s` is "declared at fs * s"
    assert torch.equal(cube, same) and lens.tolist() == lens2.tolist()
    _feature_case(waves[1:], 17600, speed=1.1)
    with pytest.raises(ValueError, match="too short"):
        _fe().extract([waves[0][:559]], speed=1.1)                    # 509 samples after resampling: refused on the host


def test_extract_mixed_rates_and_defaults():
    import torch
    fe = _fe()
    rates = [16000, 16000, 8000, 8000, 48000]
    waves = [RR.signals(fs, False, (n,), seed=i)[0] for i, (fs, n) in enumerate(zip(rates, (720, 4000, 2000, 8037, 12000)))]
    cube, lens = fe.extract(waves, rate=rates)
    gains = [1.0, 0.5, 2.0, 0.25, 1.5]
    gcube, glens = fe.extract(waves, rate=rates, gain=gains)
    assert lens.tolist() == glens.tolist() == [2, 22, 22, 97, 22]
    for u, (w, fs) in enumerate(zip(waves, rates)):
        alone, l1 = fe.extract([w], rate=fs)
        assert l1[0] == lens[u] and torch.equal(alone[0], cube[u, :lens[u]]), u       # one by one = inside the batch, bit for bit
        galone, _ = fe.extract([w], rate=fs, gain=gains[u])
        assert torch.equal(galone[0], gcube[u, :lens[u]]), u
    # the defaults are the path without the resampler; a rate equal to the extractor's and a gain of 1 change no bit
    w16 = R.signals(FS, False, seed=0)
    old, lo = fe.extract(w16)
    for kw in (dict(rate=None, speed=1.0, gain=None), dict(rate=FS), dict(rate=[FS] * 5, speed=1.0), dict(gain=1.0)):
        new, ln = fe.extract(w16, **kw)
        assert torch.equal(old, new) and lo.tolist() == ln.tolist(), kw
    wi = R.signals(FS, True, seed=0)
    old, _ = fe.extract(wi)
    new, _ = fe.extract(wi, gain=1.0)                                 # int16 rows converted by the gain-only path: the same value / 32767
    assert torch.equal(old, new)


# ---- entry points ------------------------------------------------------------------------------------------------------------------
def _child(argv):
    return subprocess.run([sys.executable] + argv, cwd=helpers.PKG, env=dict(os.environ), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=300)


def test_transcribe_synthetic_reads_files_at_other_rates(tmp_path):
    from scipy.io import wavfile
    a, b = str(tmp_path / "phone.wav"), str(tmp_path / "studio.wav")
    wavfile.write(a, 8000, RR.signals(8000, True, (9000,))[0])
    wavfile.write(b, 48000, RR.signals(48000, False, (50000,))[0])
    r = _child(["transcribe.py", "--synthetic", "True", "--unit", "char", "--enc_type", "pblstm", "--cell", "lstm", "--enc_units", "64",
                "--dec_units", "64", "--num_dec_layers", "1", "--embedding_size", "32", "--attention_size", "32", "--beam_size", "4",
                "--feat_dim", "13", "--decode_batch", "2", a, b])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.split("\n")
    assert lines[-1] == "" and len(lines) - 1 == 2, r.stdout           # one hypothesis (possibly empty) per file


def test_preprocess_augmentation_gpu_writes_the_cpu_dumps(tmp_path):
    import joblib
    waves = RR.signals(FS, False, (4000, 9037))
    train = RR.make_corpus(tmp_path, "train", waves)
    out = {}
    for mode in ("cpu", "gpu"):
        out[mode] = tmp_path / mode
        r = _child(["preprocess.py", "--augmentation", "True", "--frontend", mode, "--unit", "char", "--feat_dim", "13", "--train_100hr_corpus_dir",
                    train, "--dev_data_dir", str(tmp_path / "none"), "--test_data_dir", str(tmp_path / "none"), "--feat_dir", str(out[mode])])
        assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(out["cpu"])) == sorted(os.listdir(out["gpu"]))
    a = R.fe_args(FS, "mfcc", 13, True)
    for s, eff in (("0.9", 14400), ("1.1", 17600)):
        name = "speed_%s-" % s
        assert np.array_equal(np.load(str(out["cpu"] / (name + "featlen.npy"))), np.load(str(out["gpu"] / (name + "featlen.npy"))))
        fc, fg = joblib.load(str(out["cpu"] / (name + "feats.pkl"))), joblib.load(str(out["gpu"] / (name + "feats.pkl")))
        assert len(fc) == len(fg) == 2
        for w, c, g in zip(waves, fc, fg):
            assert c.shape == g.shape and g.dtype == np.float32
            gap = float(np.abs(R.ref32(RR.ref32(w, eff, FS), a).astype(np.float64) - c).max())
            bar = max(4 * gap, 1e-5)
            err = float(np.abs(g.astype(np.float64) - c).max())
            print("preprocess speed %s gpu vs cpu: err %.3e bar %.3e" % (s, err, bar))
            assert err <= bar
