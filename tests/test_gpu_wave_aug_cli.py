"""The entry points of the reverberation / noise augmentation on the device: preprocess.py --noisy_copies through the HIP front end writes
what the CPU front end writes, and transcribe.py --noise_file / --rir_file transcribes the files in that condition."""
import os
import subprocess
import sys

import numpy as np
import pytest

import frontend_ref as R
import helpers
import wave_aug_ref as WR
from frontend_ref import pp

pytestmark = pytest.mark.gpu

FS = 16000


def _child(argv):
    return subprocess.run([sys.executable] + argv, cwd=helpers.PKG, env=dict(os.environ), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=300)


def test_preprocess_noisy_copies_gpu_writes_the_cpu_dumps(tmp_path):
    """the same plan on both front ends: equal featlen, features within the tolerance of tests/test_gpu_frontend.py's parity test,
    max(4 x gap, 1e-5), gap = the float32 augmentation and front end against the float64 ones on the same recording"""
    import joblib
    from las.arguments import parse_args
    waves = [WR.noise_signal(n, 20 + i) for i, n in enumerate((4000, 9037))]
    train = WR.make_corpus(tmp_path, "train", waves)
    noise_dir = tmp_path / "noises"
    noise_dir.mkdir()
    np.save(str(noise_dir / "hum.npy"), WR.noise_signal(2500, 98, rms=0.3).astype(float))
    out, flags = {}, None
    for mode in ("cpu", "gpu"):
        out[mode] = tmp_path / mode
        flags = ["--augmentation", "True", "--frontend", mode, "--unit", "char", "--feat_dim", "13", "--train_100hr_corpus_dir", train,
                 "--dev_data_dir", str(tmp_path / "none"), "--test_data_dir", str(tmp_path / "none"), "--feat_dir", str(out[mode]),
                 "--noisy_copies", "1", "--rir_synthetic", "2", "--rt60", "0.03,0.06", "--noise_dir", str(noise_dir), "--snr_range", "5,15",
                 "--reverb_prob", "1.0", "--seed", "4"]
        r = _child(["preprocess.py"] + flags)
        assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(out["cpu"])) == sorted(os.listdir(out["gpu"]))
    assert np.array_equal(np.load(str(out["cpu"] / "noisy_0-featlen.npy")), np.load(str(out["gpu"] / "noisy_0-featlen.npy")))
    fc, fg = joblib.load(str(out["cpu"] / "noisy_0-feats.pkl")), joblib.load(str(out["gpu"] / "noisy_0-feats.pkl"))
    assert len(fc) == len(fg) == 2
    a = WR.fe_args()
    aug = pp.wave_augmenter(parse_args(flags))
    plan = aug.plan(2, 0)
    for u, (w, c, g) in enumerate(zip(waves, fc, fg)):
        assert c.shape == g.shape and g.dtype == np.float32
        r, v = plan.rir_idx[u], plan.noise_idx[u]
        assert r >= 0 and v == 0
        y32 = WR.reverb32_batch([w], [aug.rir_bank[r, :aug.rir_len[r]]], [aug.rir_delay[r]])[0]
        y32 = WR.mix32(y32, aug.noise_bank[v, :aug.noise_len[v]], int(plan.noise_off[u]), plan.snr_db[u])
        gap = float(np.abs(R.ref32(y32, a).astype(np.float64) - c).max())
        bar = max(4 * gap, 1e-5)
        err = float(np.abs(g.astype(np.float64) - c).max())
        print("preprocess noisy_0 gpu vs cpu, utterance %d: err %.3e gap %.3e bar %.3e" % (u, err, gap, bar))
        assert err <= bar


def test_transcribe_in_a_condition(tmp_path):
    from scipy.io import wavfile
    a, b = str(tmp_path / "one.wav"), str(tmp_path / "two.wav")
    wavfile.write(a, FS, R.signals(FS, True, lengths=(9000,))[0])
    wavfile.write(b, 8000, R.signals(8000, False, lengths=(7000,))[0])
    noise, room = str(tmp_path / "cafe.wav"), str(tmp_path / "room.npy")
    wavfile.write(noise, 8000, WR.noise_signal(3000, 5, rms=0.2))
    np.save(room, pp.synthetic_rir(FS, 0.05, 1))
    model = ["transcribe.py", "--synthetic", "True", "--unit", "char", "--enc_type", "pblstm", "--cell", "lstm", "--enc_units", "64", "--dec_units", "64",
             "--num_dec_layers", "1", "--embedding_size", "32", "--attention_size", "32", "--beam_size", "4", "--feat_dim", "13", "--decode_batch", "2"]
    plain = _child(model + [a, b])
    assert plain.returncode == 0, plain.stderr[-2000:]
    again = _child(model + ["--snr_db", "3"] + [a, b])                 # without a noise or room file the other flag changes nothing
    assert again.returncode == 0 and again.stdout == plain.stdout
    both = _child(model + ["--noise_file", noise, "--snr_db", "10", "--rir_file", room, a, b])
    assert both.returncode == 0, both.stderr[-2000:]
    for r in (plain, both):
        lines = r.stdout.split("\n")
        assert lines[-1] == "" and len(lines) - 1 == 2, r.stdout       # one hypothesis (possibly empty) per file
