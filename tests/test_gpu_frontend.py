"""The audio front end on the device (csrc/frontend.hip through las.frontend.FeatureExtractor) against the float64 restatement in
preprocess.py, and the path from audio to text built on it.

The parity bar of a case is not a constant: max |gpu - float64| <= 4 x the gap of tests/frontend_ref.py's float32 numpy evaluation on
the same batch (two correct fp32 evaluations with different FFT factorisation and summation order can each sit a full gap from
float64 on opposite sides; a further 2x covers logf against numpy's log), never tighter than 1e-5 absolute.  With LAS_FRONTEND_PARITY_OUT
set, every case appends its measured error and gap to that file (profiles/frontend_parity.jsonl is such a run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import frontend_ref as R
import helpers

pytestmark = pytest.mark.gpu

_extractors, _batches, _refs = {}, {}, {}


def _fe(a):
    from las.frontend import FeatureExtractor
    key = (a.sample_rate, a.feat_type, a.feat_dim, a.cmvn)
    if key not in _extractors:
        _extractors[key] = FeatureExtractor(a)
    return _extractors[key]


def _waves(fs, int16):
    if (fs, int16) not in _batches:
        _batches[(fs, int16)] = R.signals(fs, int16, seed=0)
    return _batches[(fs, int16)]


def _ref(fs, int16, a):
    """(float64 reference per utterance, float32 evaluation's gap over the batch), computed once per case"""
    key = (fs, int16, a.feat_type, a.feat_dim, a.cmvn)
    if key not in _refs:
        r64 = [R.ref64(w, a) for w in _waves(fs, int16)]
        gaps = [R.gap(w, a) for w in _waves(fs, int16)]
        _refs[key] = (r64, gaps)
    return _refs[key]


def _errors(cube, lens, r64):
    c = cube.cpu().numpy()
    errs = []
    for u, r in enumerate(r64):
        assert lens[u] == len(r)
        errs.append(float(np.abs(c[u, :lens[u]].astype(np.float64) - r).max()))
    return errs


@pytest.mark.parametrize("int16", [False, True], ids=["float", "int16"])
@pytest.mark.parametrize("fs", [16000, 8000])
@pytest.mark.parametrize("cmvn", [True, False], ids=["cmvn", "raw"])
@pytest.mark.parametrize("ft,fd", [("mfcc", 13), ("mfcc", 20), ("fbank", 40)])
def test_parity_against_float64(ft, fd, cmvn, fs, int16):
    import torch
    a = R.fe_args(fs, ft, fd, cmvn)
    waves = _waves(fs, int16)
    r64, gaps = _ref(fs, int16, a)
    cube, lens = _fe(a).extract(waves)
    torch.cuda.synchronize()
    assert cube.dtype == torch.float32 and cube.is_cuda
    assert tuple(cube.shape) == ((5, max(lens), fd, 3) if cmvn else (5, max(lens), fd))
    assert lens.dtype == np.int32 and not torch.isnan(cube).any()
    errs = _errors(cube, lens, r64)
    bar = max(4 * max(gaps), 1e-5)
    rec = dict(feat=ft, dim=fd, cmvn=cmvn, fs=fs, input="int16" if int16 else "float", err=max(errs), gap=max(gaps), bar=bar,
               err_per_utt=errs, gap_per_utt=gaps)
    print(json.dumps(rec))
    if os.environ.get("LAS_FRONTEND_PARITY_OUT"):
        with open(os.environ["LAS_FRONTEND_PARITY_OUT"], "a") as f:
            f.write(json.dumps(rec) + "\n")
    assert max(errs) <= bar, rec


@pytest.mark.parametrize("cmvn", [True, False], ids=["cmvn", "raw"])
def test_structure_frame_counts_and_zero_tail(cmvn):
    import torch
    a = R.fe_args(16000, "mfcc", 13, cmvn)
    fe = _fe(a)
    waves = _waves(16000, False)
    T = int(fe.frame_counts([len(w) for w in waves]).max())
    poisoned = torch.full((5, T, 13, 3) if cmvn else (5, T, 13), float("nan"), device="cuda")
    cube, lens = fe.extract(waves, out=poisoned)
    torch.cuda.synchronize()
    assert cube.data_ptr() == poisoned.data_ptr()
    fl, step = 400, 160
    assert lens.tolist() == [int(np.floor((len(w) - fl) / step)) for w in waves] == [1, 2, 22, 97, 197]
    assert not torch.isnan(cube).any()
    for u in range(5):
        assert (cube[u, lens[u]:] == 0).all()                         # exactly 0 behind T_u
        assert (cube[u, :lens[u]] != 0).any() or (cmvn and lens[u] == 1)
    if cmvn:
        assert (cube[0, 0] == 0).all()                                # one frame: x - mean = 0, divided by 2^-30, and its derivatives


@pytest.mark.parametrize("ft,fd,cmvn,int16", [("mfcc", 13, True, False), ("fbank", 40, True, True), ("mfcc", 20, False, False)])
def test_batch_independence_and_determinism(ft, fd, cmvn, int16):
    import torch
    fe = _fe(R.fe_args(16000, ft, fd, cmvn))
    waves = _waves(16000, int16)
    cube, lens = fe.extract(waves)
    again, _ = fe.extract(waves)
    torch.cuda.synchronize()
    assert torch.equal(cube, again)                                   # two runs: the same bits
    for u, w in enumerate(waves):
        alone, l1 = fe.extract([w])
        assert l1[0] == lens[u] and alone.shape[1] == lens[u]
        assert torch.equal(alone[0], cube[u, :lens[u]]), u            # alone = inside the batch, bit for bit


def test_decode_batch_takes_device_cubes():
    """BeamSearch.decode_batch on three device-resident cubes from FeatureExtractor = the same cubes copied to host arrays and fed
    through the host path: the same token ids and the same scores, bit for bit"""
    import torch
    from las import layers as L
    from las import variables as V
    from las.beam_search import BeamSearch
    from las.las import LAS, Listener, Speller
    from utils.tokenizer import CharEncoder
    tok = CharEncoder()
    args = helpers.make_args(enc_units=64, num_enc_layers=2, dec_units=64, num_dec_layers=1, embedding_size=32, attention_size=32,
                             beam_size=4, enc_type="pblstm", vocab_size=tok.get_vocab_size(), feat_dim=13, convert_rate=0.35)
    L.set_cell("lstm")
    L.set_precision("f32")
    V.reset_default_store(device="cuda:0", seed=5)
    las = LAS(args, Listener, Speller, tok.token_to_id)
    las.build_variables()
    bs = BeamSearch(args, las, tok.token_to_id, None)
    fe = _fe(R.fe_args(16000, "mfcc", 13, True))
    waves = [_waves(16000, False)[i] for i in (2, 3, 4)]
    cube, lens = fe.extract(waves)
    dev_xs = [(cube[u:u + 1, :lens[u]], np.asarray([lens[u]], np.int32)) for u in range(3)]
    host = cube.cpu().numpy()
    host_xs = [(host[u:u + 1, :lens[u]].copy(), np.asarray([lens[u]], np.int32)) for u in range(3)]
    r_dev = bs.decode_batch(None, dev_xs)
    r_host = bs.decode_batch(None, host_xs)
    assert len(r_dev) == len(r_host) == 3
    for bd, bh in zip(r_dev, r_host):
        assert len(bd) == len(bh) and len(bd) >= 1
        for sd, sh in zip(bd, bh):
            assert list(sd.token_ids) == list(sh.token_ids)
            assert float(sd.log_prob) == float(sh.log_prob)
    # ... and through decode_batches (the encoders of a batch under the search of the one before)
    r2 = list(bs.decode_batches(None, iter([dev_xs, dev_xs[:2]])))
    assert [list(b[-1].token_ids) for b in r2[0]] == [list(b[-1].token_ids) for b in r_host]
    assert [list(b[-1].token_ids) for b in r2[1]] == [list(b[-1].token_ids) for b in r_host[:2]]


def _child(argv, cwd=None):
    env = dict(os.environ)
    return subprocess.run([sys.executable] + argv, cwd=cwd or helpers.PKG, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)


def test_transcribe_synthetic_child_process():
    r = _child(["transcribe.py", "--synthetic", "True", "--unit", "char", "--enc_type", "pblstm", "--cell", "lstm", "--enc_units", "64",
                "--dec_units", "64", "--num_dec_layers", "1", "--embedding_size", "32", "--attention_size", "32", "--beam_size", "4",
                "--feat_dim", "13", "--decode_batch", "2", "--max_steps", "5"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.split("\n")
    assert lines[-1] == "" and len(lines) - 1 == 5, r.stdout           # one hypothesis (possibly empty) per utterance


def test_preprocess_frontend_gpu_writes_the_cpu_dumps(tmp_path):
    """preprocess.py --frontend gpu on two generated recordings: the same dump files as --frontend cpu, features within the parity bar"""
    import joblib
    corpus = tmp_path / "corpus" / "spk" / "chap"
    corpus.mkdir(parents=True)
    waves = [_waves(16000, False)[i] for i in (2, 3)]
    with open(corpus / "spk-chap.trans.txt", "w") as f:
        for i, w in enumerate(waves):
            np.save(str(corpus / ("spk-chap-%04d.npy" % i)), w)
            f.write("spk-chap-%04d HELLO WORLD\n" % i)
    out = {}
    for mode in ("cpu", "gpu"):
        out[mode] = tmp_path / mode
        r = _child(["preprocess.py", "--frontend", mode, "--unit", "char", "--feat_dim", "13", "--dev_data_dir", str(tmp_path / "corpus"),
                    "--train_100hr_corpus_dir", str(tmp_path / "none"), "--test_data_dir", str(tmp_path / "none"), "--feat_dir", str(out[mode])])
        assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(out["cpu"])) == sorted(os.listdir(out["gpu"]))
    fc, fg = joblib.load(str(out["cpu"] / "dev-feats.pkl")), joblib.load(str(out["gpu"] / "dev-feats.pkl"))
    assert np.array_equal(np.load(str(out["cpu"] / "dev-featlen.npy")), np.load(str(out["gpu"] / "dev-featlen.npy")))
    a = R.fe_args(16000, "mfcc", 13, True)
    assert len(fc) == len(fg) == 2
    for w, c, g in zip(waves, fc, fg):
        assert c.shape == g.shape and g.dtype == np.float32
        bar = max(4 * R.gap(w, a), 1e-5)
        err = float(np.abs(g.astype(np.float64) - c).max())
        print("preprocess gpu vs cpu: err %.3e bar %.3e" % (err, bar))
        assert err <= bar
