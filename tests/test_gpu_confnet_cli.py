"""transcribe.py --confusion_network / --cn_decode and decode.py --cn_decode end to end, as child processes on a small random
model."""
import os
import subprocess
import sys

import pytest

import helpers  # noqa: F401
from test_gpu_frontend import _child
from test_gpu_timestamps import MODEL, _json_lines

pytestmark = pytest.mark.gpu

ARGV = ["transcribe.py", "--synthetic", "True"] + MODEL + ["--max_steps", "3"]
# beam 4: at most four fp32 posteriors, each rounded once, added by at most four fp32 additions: a mass exceeds 1 by less than 1e-6
ONE = 1.0 + 1e-6


@pytest.fixture(scope="module")
def networks():
    """beam 4 and --cn_alternatives 8: every alternative of every bin is printed"""
    r = _child(ARGV + ["--confusion_network", "True", "--nbest", "4", "--cn_alternatives", "8"])
    assert r.returncode == 0, r.stderr[-2000:]
    return _json_lines(r.stdout)


def _is_path(words, bins):
    """can `words` be read off the bins in order, one alternative (a word or "") per bin?"""
    reach = {0}                                                        # the words consumed after the bins so far
    for alts in bins:
        have = set(a["word"] for a in alts)
        reach = set(j for j in reach if "" in have) | set(j + 1 for j in reach if j < len(words) and words[j] in have)
    return len(words) in reach


def test_every_listed_hypothesis_is_a_path_through_the_bins(networks):
    assert len(networks) == 3
    for o in networks:
        assert set(o) == {"text", "score", "nbest", "network"}
        assert o["nbest"][0]["text"] == o["text"] and o["nbest"][0]["score"] == o["score"]      # --nbest beside it is unchanged
        for alts in o["network"]:
            assert 1 <= len(alts) <= 4 and all(set(a) == {"word", "p"} for a in alts)
            p = [a["p"] for a in alts]
            assert p == sorted(p, reverse=True) and all(0.0 < x <= ONE for x in p) and sum(p) <= ONE
            assert len(set(a["word"] for a in alts)) == len(alts)
        for h in o["nbest"]:
            assert _is_path(h["text"].split(), o["network"]), (h["text"], o["network"])
        assert len(o["network"]) >= len(o["text"].split())
    assert any(len(alts) > 1 for o in networks for alts in o["network"])


def test_cn_decode_prints_the_first_alternatives(networks):
    r = _child(ARGV + ["--confusion_network", "True", "--cn_decode", "True", "--confidence", "True"])
    assert r.returncode == 0, r.stderr[-2000:]
    objs = _json_lines(r.stdout)
    assert len(objs) == 3
    for o, ref in zip(objs, networks):
        assert set(o) == {"text", "score", "confidence", "words", "network"} and o["score"] is None
        assert o["network"] == [alts[:3] for alts in ref["network"]]    # the default of three alternatives, the same bins
        first = [alts[0] for alts in o["network"] if alts[0]["word"] != ""]
        assert o["text"] == " ".join(a["word"] for a in first)
        assert o["words"] == [{"word": a["word"], "confidence": a["p"]} for a in first]
        assert o["confidence"] == (min(a["p"] for a in first) if first else None)


def test_without_the_flags_the_plain_lines_and_no_import(networks):
    code = ("import sys; sys.argv = %r; import transcribe; transcribe.main(); "
            "sys.stderr.write('NBEST_IMPORTED=%%s\\n' %% ('las.nbest' in sys.modules))" % (ARGV,))
    r = _child(["-c", code])
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split("\n") == [o["text"] for o in networks] + [""]
    assert "NBEST_IMPORTED=False" in r.stderr


def _hyps(stdout):
    return [line.split("HYP | ", 1)[1] for line in stdout.splitlines() if "HYP | " in line]


def test_decode_cn_decode(tmp_path):
    """decode.py --cn_decode: with the posterior collapsed onto the 1-best (--nbest_scale 1e4) every bin's first alternative is the
    1-best's word or its EPS, so the consensus lines -- and the corpus WER -- are the plain run's"""
    cmd = [sys.executable, os.path.join(helpers.PKG, "decode.py"), "--synthetic", "True", "--save_dir", str(tmp_path / "none"), "--max_steps", "2",
           "--verbose", "1"] + MODEL
    run = lambda *flags: subprocess.run(cmd + list(flags), capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    plain, sharp = run(), run("--cn_decode", "True", "--nbest_scale", "1e4")
    for r in (plain, sharp):
        assert r.returncode == 0 and "Dev WER" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert len(_hyps(plain.stdout)) == 2 and _hyps(sharp.stdout) == [" ".join(h.split()) for h in _hyps(plain.stdout)]
    wer = lambda out: [line.split("Dev WER: ", 1)[1] for line in out.splitlines() if "Dev WER: " in line]
    assert wer(sharp.stdout) == wer(plain.stdout)
