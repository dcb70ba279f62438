"""transcribe.py --nbest / --confidence / --mbr end to end, as child processes on a small random model."""
import numpy as np
import pytest

import helpers  # noqa: F401
from test_gpu_frontend import _child
from test_gpu_long_form import MAX_SEGMENT_S, RATE, _recording
from test_gpu_timestamps import MODEL, _json_lines

pytestmark = pytest.mark.gpu

ARGV = ["transcribe.py", "--synthetic", "True"] + MODEL + ["--max_steps", "3"]
# beam 4: four fp32 posteriors, each rounded once (2^-24 relative), added by at most four fp32 additions (2^-24 each): a sum of them
# exceeds the exact sum, 1, by less than 8 x 2^-24 < 1e-6
ONE = 1.0 + 1e-6


@pytest.fixture(scope="module")
def annotated():
    r = _child(ARGV + ["--nbest", "3", "--confidence", "True"])
    assert r.returncode == 0, r.stderr[-2000:]
    return _json_lines(r.stdout)


def test_nbest_and_confidence_lines(annotated):
    assert len(annotated) == 3                                            # one JSON object per utterance
    for o in annotated:
        assert set(o) == {"text", "score", "confidence", "words", "nbest"}
        assert 0.0 < o["confidence"] <= 1.0
        assert " ".join(w["word"] for w in o["words"]) == o["text"]
        for w in o["words"]:
            assert set(w) == {"word", "confidence"} and o["confidence"] <= w["confidence"] <= ONE, (w, o["confidence"])
        nb = o["nbest"]
        assert 1 <= len(nb) <= 3 and all(set(h) == {"text", "score", "posterior"} for h in nb)
        post = [h["posterior"] for h in nb]
        assert post == sorted(post, reverse=True) and all(0.0 < p <= 1.0 for p in post) and sum(post) <= ONE
        assert nb[0]["text"] == o["text"] and nb[0]["posterior"] == o["confidence"] and nb[0]["score"] == o["score"]
    assert any(len(o["nbest"]) > 1 for o in annotated)


def test_mbr_with_a_collapsed_posterior_prints_the_one_best(annotated):
    """--nbest_scale 1e4 sharpens the posterior onto the search's 1-best until no other hypothesis has the smaller risk: the same texts"""
    r = _child(ARGV + ["--nbest", "3", "--confidence", "True", "--mbr", "True", "--nbest_scale", "1e4"])
    assert r.returncode == 0, r.stderr[-2000:]
    objs = _json_lines(r.stdout)
    assert [o["text"] for o in objs] == [o["text"] for o in annotated]


def test_without_the_flags_the_plain_lines_and_no_import(annotated):
    """none of the new flags: the plain-text path, line for line the texts of the annotated run, and las.nbest is never imported"""
    code = ("import sys; sys.argv = %r; import transcribe; transcribe.main(); "
            "sys.stderr.write('NBEST_IMPORTED=%%s\\n' %% ('las.nbest' in sys.modules))" % (ARGV,))
    r = _child(["-c", code])
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split("\n") == [o["text"] for o in annotated] + [""]
    assert "NBEST_IMPORTED=False" in r.stderr


def test_segment_composes(tmp_path):
    """--segment with every flag at once (and --timestamps): one line per file; a file's confidence is the least of its segments', its
    words are the segments' in order and carry times and confidences; the silent file has no confidence"""
    speech, silent = str(tmp_path / "speech.npy"), str(tmp_path / "silent.npy")
    np.save(speech, _recording())
    np.save(silent, np.zeros(3 * RATE, np.float32))
    r = _child(["transcribe.py", "--synthetic", "True", "--ctc", "True"] + MODEL +
               ["--segment", "True", "--max_segment_s", str(MAX_SEGMENT_S), "--confidence", "True", "--nbest", "2", "--mbr", "True",
                "--timestamps", "True", speech, silent])
    assert r.returncode == 0, r.stderr[-2000:]
    objs = _json_lines(r.stdout)
    assert len(objs) == 2 and all(set(o) == {"text", "score", "confidence", "words", "segments"} for o in objs)
    o = objs[0]
    assert len(o["segments"]) == 4
    assert all(set(s) == {"start", "end", "text", "score", "confidence", "words", "nbest"} for s in o["segments"])
    assert o["confidence"] == min(s["confidence"] for s in o["segments"])
    assert o["words"] == [w for s in o["segments"] for w in s["words"]] and o["text"] == " ".join(s["text"] for s in o["segments"])
    for s in o["segments"]:
        assert " ".join(w["word"] for w in s["words"]) == " ".join(s["text"].split())
        for w in s["words"]:
            assert set(w) == {"word", "start", "end", "confidence"} and s["confidence"] <= w["confidence"] <= ONE
            assert w["start"] is None or s["start"] <= w["start"] <= w["end"] <= s["end"]
    assert {k: objs[1][k] for k in ("text", "confidence", "words", "segments")} == {"text": "", "confidence": None, "words": [], "segments": []}
