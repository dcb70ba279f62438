"""transcribe.py --segment end to end, as child processes on a small random model: the segments are the restatement's plan
(tests/vad_ref.py), every segment decodes to what its slice decodes to as a file of its own, times stay inside their segment, a silent
file gives an empty line."""
import numpy as np
import pytest

import helpers  # noqa: F401
import vad_ref as R
from test_gpu_frontend import _child
from test_gpu_timestamps import MODEL, _json_lines

pytestmark = pytest.mark.gpu

RATE, FL, STEP = 16000, 400, 160
MAX_SEGMENT_S = 2.0


def _recording():
    """three bursts, the middle one 2 s long: its run (2 s + 2 x 200 ms of padding) is over --max_segment_s 2.0 and is cut once"""
    rng = np.random.RandomState(7)
    z = lambda s: np.zeros(int(s * RATE), np.float32)
    b = lambda s: (0.1 * rng.randn(int(s * RATE))).astype(np.float32)
    return np.concatenate([z(0.6), b(1.0), z(0.6), b(2.0), z(0.6), b(1.0), z(0.5)])


def test_transcribe_segment_child_processes(tmp_path):
    wave = _recording()
    e, _, runs = R.vad(wave, FL, STEP, 1e-4, FL * 1e-7, 20, 10)           # the flags' defaults: 40 dB, -70 dB, 200 ms, 100 ms
    max_frames = int((MAX_SEGMENT_S * RATE - FL) // STEP) + 1
    segs = R.plan_segments(runs, e, max_frames)
    assert len(runs) == 3 and len(segs) == 4 and runs[1][1] - runs[1][0] > max_frames      # one cut
    ranges = R.sample_ranges(segs, FL, STEP, len(wave))
    speech, silent = str(tmp_path / "speech.npy"), str(tmp_path / "silent.npy")
    np.save(speech, wave)
    np.save(silent, np.zeros(3 * RATE, np.float32))
    argv = ["transcribe.py", "--synthetic", "True", "--ctc", "True"] + MODEL + ["--decode_batch", "1"]
    seg_flags = ["--segment", "True", "--max_segment_s", str(MAX_SEGMENT_S)]

    r = _child(argv + seg_flags + ["--timestamps", "True", speech, silent])
    assert r.returncode == 0, r.stderr[-2000:]
    objs = _json_lines(r.stdout)
    assert len(objs) == 2 and all(set(o) == {"text", "score", "words", "segments"} for o in objs)
    o = objs[0]
    assert [(s["start"], s["end"]) for s in o["segments"]] == [(s0 / float(RATE), s1 / float(RATE)) for s0, s1 in ranges]
    assert all(set(s) == {"start", "end", "text", "score", "words"} for s in o["segments"])
    prev_end = 0.0
    for s in o["segments"]:                                               # ordered, no overlap (a cut's two sides share fl - step samples)
        assert prev_end - (FL - STEP) / float(RATE) - 1e-9 <= s["start"] < s["end"] <= len(wave) / float(RATE)
        prev_end = s["end"]
        assert " ".join(w["word"] for w in s["words"]) == " ".join(s["text"].split())
        for w in s["words"]:
            if w["start"] is None:
                assert w["end"] is None and s["score"] is None
                continue
            assert s["start"] <= w["start"] <= w["end"] <= s["end"], (w, s["start"], s["end"])
    for a, b in zip(segs, segs[1:]):
        assert a[1] <= b[0]                                               # in frames the segments never overlap
    assert o["text"] == " ".join(s["text"] for s in o["segments"])
    assert o["words"] == [w for s in o["segments"] for w in s["words"]]
    scores = [s["score"] for s in o["segments"]]
    assert o["score"] is None if any(x is None for x in scores) else abs(o["score"] - sum(scores)) <= 1e-9 * abs(sum(scores))
    assert {k: objs[1][k] for k in ("text", "words", "segments")} == {"text": "", "words": [], "segments": []}

    # every segment's text is what its slice gives as a file of its own
    slices = []
    for k, (s0, s1) in enumerate(ranges):
        slices.append(str(tmp_path / ("slice%d.npy" % k)))
        np.save(slices[-1], wave[s0:s1])
    r = _child(argv + slices)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split("\n") == [s["text"] for s in o["segments"]] + [""]

    # plain mode: the same texts, one line per file, an empty line for the silent one
    r = _child(argv + seg_flags + [speech, silent])
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split("\n") == [o["text"], "", ""]


def test_voice_activity_object_matches_the_restatement():
    """las.vad.VoiceActivity: recordings at two sample rates in one call, an int16 one among them; the sample ranges are the
    restatement's plan at each recording's own frame geometry"""
    from las import vad as V
    from las.arguments import parse_args
    args = parse_args([])
    args.max_segment_s = MAX_SEGMENT_S
    va = V.VoiceActivity(args, device="cuda")
    w16 = _recording()
    w8 = R.bursts(8000, 2, seed=3)[0]
    i16 = np.clip(np.round(R.bursts(16000, 1, burst_s=3.0, seed=5)[0] * 32767), -32768, 32767).astype(np.int16)
    waves, rates = [w16, w8, i16, np.zeros(100, np.float32)], [16000, 8000, 16000, 8000]
    got = va.segments_batch(waves, rates)
    for w, fs, g in zip(waves, rates, got):
        fl, step = va.geometry(fs)
        e, _, runs = R.vad(w, fl, step, va.ratio, va.floor(fl), va.hang, va.min_run)
        assert g == R.sample_ranges(R.plan_segments(runs, e, va.max_frames(fs)), fl, step, len(w))
    assert [len(g) for g in got] == [4, 2, 2, 0]
    assert va.segments(w16, 16000) == got[0]
