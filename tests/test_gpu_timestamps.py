"""Word timestamps end to end: BeamSearch.align on a small random model against the float64 restatement applied to the
device's own CTC log-probabilities, the retained inputs of a search, and transcribe.py's --timestamps / --align_text."""
import json
import os

import numpy as np
import pytest

import ctc_align_ref as R
import helpers
import test_gpu_ctc_decode as D
from test_gpu_frontend import _child

pytestmark = pytest.mark.gpu

MODEL = ["--unit", "char", "--enc_type", "pblstm", "--cell", "lstm", "--enc_units", "64", "--dec_units", "64", "--num_dec_layers", "1",
         "--embedding_size", "32", "--attention_size", "32", "--beam_size", "4", "--feat_dim", "13", "--decode_batch", "2"]


def _check_against_restatement(lp, enc_lens, toks, scores, spans):
    lp = lp.cpu().numpy()
    for u, labels in enumerate(toks):
        ref = R.align(lp[u], labels, int(enc_lens[u]))
        assert scores[u] == ref.score, (u, scores[u], ref.score)
        assert spans[u] == [(int(a), int(b)) for a, b in zip(ref.first, ref.last)]


@pytest.mark.parametrize("enc_type,cell", [("pblstm", "lstm"), ("cnn", "rnn")])
def test_align_matches_restatement_on_the_devices_log_probs(enc_type, cell):
    args, p0, bs = D._model(enc_type, cell, enc_units=16, ctc_decode_weight=0.0)
    utts = D._utts(args)                                                  # 64, 48, 56 input frames -> 16, 12, 14 encoder frames
    encs, enc_lens, _, h_one, ctc_lp = bs._run_encoders(None, utts)
    assert ctc_lp is None                                                 # weight 0: the search would not have run the head
    lp = bs._ctc_log_probs(encs, h_one)
    toks = [[5, 6, 6, 3, 9, 2], [], list(range(3, 3 + 20))]               # a repeat and <EOS>; nothing; more tokens than frames
    scores, spans = bs.align(encs, enc_lens, toks, h_one=h_one)
    _check_against_restatement(lp, enc_lens, toks, scores, spans)
    assert np.isfinite(scores[0]) and np.isfinite(scores[1]) and scores[2] == -np.inf and spans[1] == []
    assert all(0 <= a <= b < int(enc_lens[0]) for a, b in spans[0]) and all(p[1] < q[0] for p, q in zip(spans[0], spans[0][1:]))


def test_align_without_the_head_raises():
    args, p0, bs = D._model("pblstm", "lstm", enc_units=16, ctc=False, ctc_decode_weight=0.0)
    encs, enc_lens, _, h_one, _ = bs._run_encoders(None, D._utts(args))
    with pytest.raises(ValueError, match="needs the CTC head"):
        bs.align(encs, enc_lens, [[5], [6], [7]], h_one=h_one)


def test_search_retains_the_log_probs_and_align_reuses_them():
    """after a joint CTC-attention search the head is not run a second time; nothing is retained unless asked for"""
    args, p0, bs = D._model("pblstm", "lstm", enc_units=16)
    utts = D._utts(args)
    assert bs.decode_batch(None, utts).align_inputs is None
    calls = []
    head = bs._ctc_log_probs
    bs._ctc_log_probs = lambda *a, **k: calls.append(1) or head(*a, **k)
    bs.retain_align = True
    for results in [bs.decode_batch(None, utts)] + list(bs.decode_batches(None, [utts[:2], utts[2:]])):
        n_search = len(calls)
        k = results.align_inputs
        assert k is not None and k.ctc_lp is not None and len(k.encs) == len(results)
        toks = [list(r[-1].token_ids[1:]) if r else [] for r in results]
        scores, spans = bs.align_results(results)
        assert len(calls) == n_search                                     # the search's log-probabilities were reused
        _check_against_restatement(k.ctc_lp, k.enc_lens, toks, scores, spans)
    assert len(calls) == 3                                                # one per searched batch
    # a search that did not need the head retains the encoder outputs; align runs the head then
    bs.ctc_weight = 0.0
    results = bs.decode_batch(None, utts)
    assert results.align_inputs.ctc_lp is None
    n_search = len(calls)
    bs.align_results(results)
    assert len(calls) == n_search + 1


def _json_lines(stdout):
    lines = stdout.split("\n")
    assert lines[-1] == ""
    return [json.loads(x) for x in lines[:-1]]


def test_transcribe_timestamps_child_process():
    import transcribe
    from las.arguments import parse_args
    base = parse_args([])
    durations = [len(w) / float(base.sample_rate) for w in transcribe.synthetic_audio(2, base.sample_rate, base.seed + 2)]
    argv = ["transcribe.py", "--synthetic", "True", "--ctc", "True"] + MODEL + ["--max_steps", "2"]
    r = _child(argv + ["--timestamps", "True"])
    assert r.returncode == 0, r.stderr[-2000:]
    objs = _json_lines(r.stdout)
    assert len(objs) == 2
    for o, dur in zip(objs, durations):
        assert set(o) == {"text", "score", "words"}
        assert " ".join(w["word"] for w in o["words"]) == o["text"]
        prev_end = 0.0
        for w in o["words"]:
            if w["start"] is None:
                assert w["end"] is None and o["score"] is None
                continue
            assert 0 <= w["start"] < w["end"] <= dur + 1e-9 and w["start"] >= prev_end - 1e-9, (w, dur)
            prev_end = w["end"]
    # without the flag: today's plain lines, the same text
    r = _child(argv)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split("\n") == [o["text"] for o in objs] + [""]


def test_transcribe_align_text_child_process(tmp_path):
    rng = np.random.RandomState(1)
    long_, short = str(tmp_path / "long.npy"), str(tmp_path / "short.npy")
    np.save(long_, (0.1 * rng.randn(3 * 16000)).astype(np.float32))       # 3 s: 74 encoder frames for 18 tokens
    np.save(short, (0.1 * rng.randn(4800)).astype(np.float32))            # 0.3 s: too few frames for its transcript
    refs = tmp_path / "refs.txt"
    refs.write_text("HELLO WORLD AGAIN\nTHIS ONE CANNOT FIT\n")
    argv = ["transcribe.py", "--synthetic", "True", "--ctc", "True"] + MODEL
    r = _child(argv + ["--align_text", str(refs), long_, short])
    assert r.returncode == 0, r.stderr[-2000:]
    objs = _json_lines(r.stdout)
    assert [o["text"] for o in objs] == ["HELLO WORLD AGAIN", "THIS ONE CANNOT FIT"]
    assert [[w["word"] for w in o["words"]] for o in objs] == [["HELLO", "WORLD", "AGAIN"], ["THIS", "ONE", "CANNOT", "FIT"]]
    prev_end = 0.0
    for w in objs[0]["words"]:
        assert 0 <= w["start"] < w["end"] <= 3.0 and w["start"] >= prev_end
        prev_end = w["end"]
    assert objs[0]["score"] is not None and objs[0]["score"] < 0
    assert objs[1]["score"] is None and all(w["start"] is None and w["end"] is None for w in objs[1]["words"])
    # a line count that differs from the number of files
    r = _child(argv + ["--align_text", str(refs), long_])
    assert r.returncode != 0 and "2 lines for 1 audio files" in r.stderr


def test_transcribe_timestamps_needs_the_head():
    r = _child(["transcribe.py", "--synthetic", "True"] + MODEL + ["--timestamps", "True", os.path.join("no", "such", "file.wav")])
    assert r.returncode != 0 and "needs the CTC head" in r.stderr and "No such file" not in r.stderr
