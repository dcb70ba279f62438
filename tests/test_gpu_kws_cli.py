"""Keyword search from the command line: transcribe.py --keywords on the synthetic model in child processes -- one JSON
object per file, hits sorted and inside the recording, the same hits as the Python API gives on the same seed -- the refusals, which
come right after parsing, and a run without the flag, which never imports las.kws."""
import json
import math

import pytest

import helpers  # noqa: F401
from test_gpu_ctc_search_cli import MODEL
from test_gpu_frontend import _child

pytestmark = pytest.mark.gpu
PHRASES = ["AB", "HELLO", "E", "NEW YORK"]
ARGV = ["transcribe.py", "--synthetic", "True", "--max_steps", "3"] + MODEL


def _kwfile(tmp_path):
    f = tmp_path / "keywords.txt"
    f.write_text("# a phrase per line\n" + "\n".join(PHRASES[:2]) + "\n\n" + "\n".join(p.lower() for p in PHRASES[2:]) + "\n")
    return str(f)


# transcribe.main with BeamSearch.keyword_search's results (the Python API's) written to stderr beside what main prints
RECORDING = ("import sys, json; sys.argv = %r; import transcribe; from las.beam_search import BeamSearch; inner = BeamSearch.keyword_search\n"
             "def recording(self, *a, **k):\n"
             "    r = inner(self, *a, **k)\n"
             "    sys.stderr.write('API_HITS=' + json.dumps(r.hits) + '\\n')\n"
             "    return r\n"
             "BeamSearch.keyword_search = recording; transcribe.main()\n")


def test_keywords_cli_against_the_python_api(tmp_path):
    import transcribe
    from las import align as A
    from las import kws as KW
    from utils.tokenizer import CharEncoder
    flags = ["--ctc", "True", "--keywords", _kwfile(tmp_path), "--keyword_threshold", "-50", "--keyword_max_hits", "3"]
    r = _child(ARGV + flags)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 3                                                       # one JSON line per utterance
    args = transcribe.build_parser().parse_args(MODEL)
    durations = [len(w) / float(args.sample_rate) for w in transcribe.synthetic_audio(3, args.sample_rate, args.seed + 2)]
    n_hits = 0
    for ln, dur in zip(lines, durations):
        d = json.loads(ln)
        assert list(d) == ["hits"]
        keys = [(h["start"], PHRASES.index(h["keyword"])) for h in d["hits"]]
        assert keys == sorted(keys)                                              # by start, then by the phrase's place in the list
        per_phrase = {}
        for h in d["hits"]:
            assert set(h) == {"keyword", "start", "end", "score", "confidence"}
            assert 0 <= h["start"] < h["end"] <= dur
            L = len(h["keyword"])                                                # (the char unit: one token per character)
            assert -50.0 * L <= h["score"] <= 0.0 and h["confidence"] == math.exp(h["score"] / L)
            per_phrase[h["keyword"]] = per_phrase.get(h["keyword"], 0) + 1
        assert all(v <= 3 for v in per_phrase.values())                          # --keyword_max_hits
        n_hits += len(d["hits"])
    assert n_hits > 0
    # the Python API on the same seed: the same bytes on stdout, and BeamSearch.keyword_search's hits by the stated rule
    r2 = _child(["-c", RECORDING % (ARGV + flags,)])
    assert r2.returncode == 0, r2.stderr[-2000:]
    assert r2.stdout == r.stdout
    api = [hits for ln in r2.stderr.splitlines() if ln.startswith("API_HITS=") for hits in json.loads(ln[len("API_HITS="):])]
    assert len(api) == 3
    tok = CharEncoder()
    kw = KW.KeywordList([tok.encode(p, with_eos=False) for p in PHRASES], PHRASES, tok.get_vocab_size())
    frame_s = A.frame_seconds(args, "pblstm")
    for ln, dur, hits in zip(lines, durations, api):
        assert json.loads(ln)["hits"] == KW.timed_hits(hits, kw, frame_s, dur)


@pytest.mark.parametrize("extra, msg", [
    ([], "--ctc True"),
    (["--ctc", "True", "--align_text", "refs.txt"], "--keywords skips the search"),
    (["--ctc", "True", "--segment", "True"], "--keywords skips the search"),
    (["--ctc", "True", "--timestamps", "True"], "--keywords skips the search"),
    (["--ctc", "True", "--nbest", "2"], "--keywords skips the search"),
    (["--ctc", "True", "--confidence", "True"], "--keywords skips the search"),
    (["--ctc", "True", "--mbr", "True"], "--keywords skips the search"),
    (["--ctc", "True", "--keyword_max_hits", "9"], "--keyword_max_hits"),
    (["--ctc", "True", "--keyword_threshold", "nan"], "--keyword_threshold")])
def test_keywords_cli_refusals(tmp_path, extra, msg):
    """--keywords without --ctc True, and with every flag it cannot be combined with: a ValueError that names the flag right after
    parsing -- before the logging is set up, a model is built or any audio is made"""
    r = _child(ARGV + ["--keywords", _kwfile(tmp_path)] + extra)
    assert r.returncode != 0 and "ValueError" in r.stderr and msg in r.stderr, (extra, r.stderr[-1500:])
    assert all(f in r.stderr for f in extra[2:3]) and r.stdout == "" and "INFO" not in r.stderr


def test_keywords_cli_missing_file(tmp_path):
    r = _child(ARGV + ["--ctc", "True", "--keywords", str(tmp_path / "absent.txt")])
    assert r.returncode != 0 and "no such file" in r.stderr and r.stdout == ""


def test_without_the_flag_the_plain_lines_and_no_import():
    """a run without --keywords: plain hypotheses, the same bytes as a run in which las.kws cannot be imported at all"""
    flags = ["--ctc", "True", "--beam_size", "4"]
    r = _child(ARGV + flags)
    assert r.returncode == 0, r.stderr[-1500:]
    lines = r.stdout.splitlines()
    assert len(lines) == 3 and not any(ln.startswith("{") for ln in lines)
    code = ("import sys; sys.argv = %r; sys.modules['las.kws'] = None; import transcribe; transcribe.main(); "
            "sys.stderr.write('KWS_IMPORTED=%%s\\n' %% (sys.modules.get('las.kws') is not None))" % (ARGV + flags,))
    r2 = _child(["-c", code])
    assert r2.returncode == 0, r2.stderr[-2000:]
    assert r2.stdout == r.stdout and "KWS_IMPORTED=False" in r2.stderr
