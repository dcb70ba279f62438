"""transcribe.py --beamform True end to end, as child processes on a small random model.  The array recording is the generated
one of tests/beamform_ref.py (C = 4, delays [0, 7, -12, 3] then [0, -5, 9, -20]) at 5 dB per channel, saved as .npy and as a 16-bit .wav.
Why 5 dB and not the host test's 0 dB: the correlation of y with the clean source is sqrt(S / (S + N)); at 0 dB even the ideal sum of
four channels reaches only sqrt(4 / 5) = 0.894, so 0.9 would test nothing there.  At 5 dB one channel alone is at sqrt(3.16 / 4.16) = 0.87,
BELOW the bar, and the beamformed signal (about 5.8 dB better) at 0.96: the bar separates a working beamformer from a channel passed
through or summed at wrong delays."""
import os

import numpy as np
import pytest

import helpers  # noqa: F401
import beamform_ref as R
import diarize_ref as DR
from test_gpu_frontend import _child
from test_gpu_timestamps import MODEL, _json_lines

pytestmark = pytest.mark.gpu

ARGV = ["transcribe.py", "--synthetic", "True"] + MODEL
REFUSED = "has %d channels: mono recordings only"


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from scipy.io import wavfile
    d = tmp_path_factory.mktemp("beamform")
    x, clean, voice, delays = R.array_recording(snr_db=5.0)
    y_ref = R.enhance(x, 0, 8000, 160, 16384, 0.01)[0]
    assert np.corrcoef(y_ref, clean)[0, 1] > 0.9 > np.corrcoef(x[0], clean)[0, 1]        # the restatement clears the bar, one channel does not
    npy, wav = str(d / "array.npy"), str(d / "array.wav")
    np.save(npy, x.T)
    wavfile.write(wav, 16000, np.round(np.clip(x.T, -1, 1) * 32767).astype(np.int16))
    two = DR.two_voices()
    pair = np.stack([two, np.concatenate([np.zeros(5, two.dtype), two[:-5]])], axis=1)  # the second channel delayed by 5 samples
    meeting, mono = str(d / "meeting.npy"), str(d / "mono.npy")
    np.save(meeting, pair)
    np.save(mono, two[:40000])
    return dict(npy=npy, wav=wav, clean=clean, n=x.shape[1], meeting=meeting, mono=mono, dir=str(d))


@pytest.mark.parametrize("kind", ["npy", "wav"])
def test_array_file_is_transcribed_and_the_beamformed_wav_is_clean(files, kind):
    from scipy.io import wavfile
    out = os.path.join(files["dir"], "out_" + kind)
    r = _child(ARGV + ["--beamform", "True", "--beamform_wav", out, files[kind]])
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(r.stdout.split("\n")) == 2 and r.stdout.endswith("\n")              # one line for the one file
    fs, y = wavfile.read(os.path.join(out, "array.wav"))
    assert fs == 16000 and y.dtype == np.int16 and y.shape == (files["n"],)
    corr = np.corrcoef(y.astype(np.float64), files["clean"])[0, 1]
    print("correlation with the clean source: %.4f" % corr)
    assert corr > 0.9


def test_segment_diarize_beamform_on_a_two_channel_meeting(files):
    r = _child(ARGV + ["--segment", "True", "--diarize", "True", "--beamform", "True", files["meeting"]])
    assert r.returncode == 0, r.stderr[-2000:]
    o = _json_lines(r.stdout)[0]
    assert o["speakers"] == 2 and [s["speaker"] for s in o["segments"]] == [1, 2, 1, 2]


def test_without_the_flag_a_multi_channel_file_is_refused_as_before(files):
    r = _child(ARGV + [files["npy"]])
    assert r.returncode != 0 and (files["npy"] + " " + REFUSED % 4) in r.stderr and r.stdout == ""


def test_a_mono_file_prints_what_it_prints_without_the_flag(files):
    a = _child(ARGV + [files["mono"]])
    b = _child(ARGV + ["--beamform", "True", files["mono"]])
    assert a.returncode == 0 and b.returncode == 0, (a.stderr[-1000:], b.stderr[-1000:])
    assert a.stdout == b.stdout and a.stdout.strip()


@pytest.mark.parametrize("flags,message", [
    (["--bf_window_ms", "250"], "--bf_window_ms sets the beamformer of --beamform True: give both"),
    (["--bf_ref", "1"], "--bf_ref sets the beamformer of --beamform True: give both"),
    (["--beamform_wav", "out"], "--beamform_wav sets the beamformer of --beamform True: give both"),
    (["--beamform", "True", "--bf_window_ms", "0"], "--bf_window_ms 0.0, --bf_max_delay_ms 10.0: positive numbers of milliseconds"),
    (["--beamform", "True", "--bf_max_delay_ms", "nan"], "positive numbers of milliseconds"),
    (["--beamform", "True", "--bf_jump_penalty", "-0.5"], "--bf_jump_penalty -0.5: a finite penalty >= 0"),
    (["--beamform", "True", "--bf_ref", "-1"], "--bf_ref -1: a channel, 0 to 15")])
def test_refusals_exit_before_any_audio_is_read(flags, message):
    r = _child(ARGV + flags + ["no_such_file.wav"])
    assert r.returncode != 0 and message in r.stderr and "no_such_file" not in r.stderr.split("ValueError")[-1]
    assert r.stdout == ""


def test_a_reference_channel_the_file_does_not_have_is_refused_at_load_time(files):
    r = _child(ARGV + ["--beamform", "True", "--bf_ref", "4", files["npy"]])
    assert r.returncode != 0 and "--bf_ref 4: the recording has the channels 0 to 3" in r.stderr and r.stdout == ""
