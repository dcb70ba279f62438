"""transcribe.py --segment True --diarize True end to end, as child processes on a small random model, on the generated
two-voice recording of tests/diarize_ref.py: voice A 3.0 s, voice B 2.5 s abutting, silence, A 2.0 s, silence, B 3.0 s.  The host test
tests/test_diarize_host.py holds the same recording to its margins through the float64 front end."""
import numpy as np
import pytest

import helpers  # noqa: F401
import diarize_ref as R
from test_gpu_frontend import _child
from test_gpu_timestamps import MODEL, _json_lines

pytestmark = pytest.mark.gpu

ARGV = ["transcribe.py", "--synthetic", "True"] + MODEL + ["--segment", "True", "--diarize", "True"]


@pytest.fixture(scope="module")
def recording(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("diarize") / "meeting.npy")
    np.save(path, R.two_voices())
    return path


def test_two_voices_are_found_and_labelled(recording, tmp_path):
    rttm = str(tmp_path / "out.rttm")
    r = _child(ARGV + ["--rttm", rttm, recording])
    assert r.returncode == 0, r.stderr[-2000:]
    objs = _json_lines(r.stdout)
    assert len(objs) == 1 and list(objs[0]) == ["text", "score", "speakers", "segments"]
    o = objs[0]
    assert o["speakers"] == 2 and len(o["segments"]) == 4
    assert [s["speaker"] for s in o["segments"]] == [1, 2, 1, 2]
    assert all(list(s) == ["start", "end", "text", "score", "speaker"] for s in o["segments"])
    assert abs(o["segments"][1]["start"] - 3.0) <= 0.15                  # one hop, one frame and slack
    assert abs(o["segments"][0]["end"] - 3.0) <= 0.15 and o["segments"][0]["start"] == 0.0
    assert o["text"] == " ".join(s["text"] for s in o["segments"])
    lines = open(rttm).read().split("\n")
    assert lines[-1] == "" and len(lines) == 5
    for ln, s in zip(lines, o["segments"]):
        assert ln == "SPEAKER meeting 1 %.3f %.3f <NA> <NA> S%d <NA> <NA>" % (s["start"], s["end"] - s["start"], s["speaker"])


def test_num_speakers_one_labels_every_segment_one(recording):
    r = _child(ARGV + ["--num_speakers", "1", recording])
    assert r.returncode == 0, r.stderr[-2000:]
    o = _json_lines(r.stdout)[0]
    assert o["speakers"] == 1 and [s["speaker"] for s in o["segments"]] == [1, 1, 1, 1]


def test_words_carry_the_speaker(recording):
    r = _child(ARGV + ["--ctc", "True", "--timestamps", "True", recording])
    assert r.returncode == 0, r.stderr[-2000:]
    o = _json_lines(r.stdout)[0]
    assert [s["speaker"] for s in o["segments"]] == [1, 2, 1, 2] and o["speakers"] == 2
    for s in o["segments"]:
        assert all(w["speaker"] == s["speaker"] for w in s["words"])
    assert o["words"] == [w for s in o["segments"] for w in s["words"]]


def test_without_the_flag_the_output_is_what_it_was(recording):
    r = _child(["transcribe.py", "--synthetic", "True"] + MODEL + ["--segment", "True", recording])
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(r.stdout.split("\n")) == 2 and not r.stdout.startswith("{")      # plain text: one line per file


@pytest.mark.parametrize("flags,message", [
    (["--diarize", "True"], "--diarize labels the segments of --segment True: give both"),
    (["--segment", "True", "--diarize", "True", "--ctc", "True", "--keywords", "k.txt"], "--diarize labels the segments a search transcribes, --keywords"),
    (["--segment", "True", "--diarize", "True", "--ctc", "True", "--align_text", "refs.txt"], "--diarize labels the segments a search transcribes, --align_text")])
def test_refusals_exit_before_any_audio_is_read(flags, message):
    r = _child(["transcribe.py", "--synthetic", "True"] + MODEL + flags + ["no_such_file.wav"])
    assert r.returncode != 0 and message in r.stderr and "no_such_file" not in r.stderr.split("ValueError")[-1]
    assert r.stdout == ""
