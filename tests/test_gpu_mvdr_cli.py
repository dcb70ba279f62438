"""transcribe.py --beamform True --bf_method mvdr end to end, as child processes on a small random model.  The recording is the
generated one of tests/mvdr_ref.py (C = 4, a voice at the fractional delays [0, 7.3, -12.6, 3.4], a directional interferer at 0 dB from
[0, -5.5, 9.2, -20.7], sensor noise 20 dB below), saved as .npy and as a 16-bit .wav, at --mvdr_top_db 2.2 (tests/test_mvdr_host.py says
why).  The bar on the written file is the host test's: a correlation of 0.95 with the clean voice over the voice-active samples.  One
channel alone is at 0.71 and the ideal sum of four at sqrt(4 / 5) = 0.894, so --bf_method delaysum on the same file stays under it:
the flag selects the method."""
import os

import numpy as np
import pytest

import helpers  # noqa: F401
import diarize_ref as DR
import mvdr_ref as R
from test_gpu_frontend import _child
from test_gpu_timestamps import MODEL

pytestmark = pytest.mark.gpu

ARGV = ["transcribe.py", "--synthetic", "True"] + MODEL
MVDR = ["--beamform", "True", "--bf_method", "mvdr"]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from scipy.io import wavfile
    d = tmp_path_factory.mktemp("mvdr")
    x, clean, voice = R.recording()
    npy, wav, mono = str(d / "array.npy"), str(d / "array.wav"), str(d / "mono.npy")
    np.save(npy, x.T)
    wavfile.write(wav, 16000, np.round(np.clip(x.T, -1, 1) * 32767).astype(np.int16))
    np.save(mono, DR.two_voices()[:40000])
    return dict(npy=npy, wav=wav, mono=mono, x=x, clean=clean, on=R.inside(voice, 0, 512), n=x.shape[1], dir=str(d))


def _written(files, out):
    from scipy.io import wavfile
    fs, y = wavfile.read(os.path.join(out, "array.wav"))
    assert fs == 16000 and y.dtype == np.int16 and y.shape == (files["n"],)
    return y


@pytest.mark.parametrize("kind", ["npy", "wav"])
def test_array_file_is_transcribed_and_the_written_wav_is_clean(files, kind):
    out = os.path.join(files["dir"], "out_" + kind)
    r = _child(ARGV + MVDR + ["--mvdr_top_db", "2.2", "--beamform_wav", out, files[kind]])
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(r.stdout.split("\n")) == 2 and r.stdout.endswith("\n")              # one line for the one file
    assert "--mvdr_top_db" not in r.stderr                                         # no warning: the mask left noise and speech
    y = _written(files, out)
    corr = np.corrcoef(y[files["on"]].astype(np.float64), files["clean"][files["on"]])[0, 1]
    print("mvdr, %s: correlation with the clean voice %.4f" % (kind, corr))
    assert corr >= 0.95


def test_delaysum_on_the_same_file_stays_under_the_bar(files):
    out = os.path.join(files["dir"], "out_delaysum")
    r = _child(ARGV + ["--beamform", "True", "--bf_method", "delaysum", "--beamform_wav", out, files["npy"]])
    assert r.returncode == 0, r.stderr[-2000:]
    y = _written(files, out)
    corr = np.corrcoef(y[files["on"]].astype(np.float64), files["clean"][files["on"]])[0, 1]
    print("delaysum: correlation with the clean voice %.4f" % corr)
    assert corr < 0.95


def test_a_mono_file_prints_what_it_prints_without_the_flag(files):
    a = _child(ARGV + [files["mono"]])
    b = _child(ARGV + MVDR + [files["mono"]])
    assert a.returncode == 0 and b.returncode == 0, (a.stderr[-1000:], b.stderr[-1000:])
    assert a.stdout == b.stdout and a.stdout.strip()


def test_an_all_speech_file_comes_out_as_its_reference_channel_with_the_warning(files):
    out = os.path.join(files["dir"], "out_all_speech")
    r = _child(ARGV + MVDR + ["--mvdr_top_db", "200", "--bf_ref", "2", "--beamform_wav", out, files["npy"]])
    assert r.returncode == 0, r.stderr[-2000:]
    warning = [line for line in r.stderr.split("\n") if "--mvdr_top_db" in line]
    assert len(warning) == 1 and "every frame" in warning[0] and "channel 2" in warning[0]
    y = _written(files, out)
    want = np.round(np.clip(files["x"][2].astype(np.float64), -1, 1) * 32767)
    assert np.abs(y - want).max() <= 1                                # the reference channel, to the 16-bit file's last bit


@pytest.mark.parametrize("flags,message", [
    (["--mvdr_top_db", "3"], "--mvdr_top_db sets the beamformer of --beamform True --bf_method mvdr"),
    (["--beamform", "True", "--mvdr_block_ms", "500"], "--mvdr_block_ms sets the beamformer of --bf_method mvdr: give both"),
    (["--bf_method", "mvdr"], "--bf_method mvdr chooses the beamformer of --beamform True: give both"),
    (MVDR + ["--bf_window_ms", "250"], "--bf_window_ms sets the delay tracker of --bf_method delaysum and would do nothing"),
    (MVDR + ["--mvdr_loading", "0"], "--mvdr_loading 0.0: a finite number > 0"),
    (MVDR + ["--mvdr_frame_ms", "nan"], "--mvdr_frame_ms nan")])
def test_refusals_exit_before_any_audio_is_read(flags, message):
    r = _child(ARGV + flags + ["no_such_file.wav"])
    assert r.returncode != 0 and message in r.stderr and "no_such_file" not in r.stderr.split("ValueError")[-1]
    assert r.stdout == ""


def test_a_frame_the_transform_does_not_take_is_refused_at_load_time(files):
    r = _child(ARGV + MVDR + ["--mvdr_frame_ms", "100", files["npy"]])
    assert r.returncode != 0 and "--mvdr_frame_ms 100" in r.stderr and r.stdout == ""
