"""CTC-only decoding from the entry points: BeamSearch.ctc_decode_batch on a real encoder batch against the restatement fed
the same logits, transcribe.py / decode.py with `--decoder ctc` (greedy, beam, --ngram_lm, --nbest / --confidence, --timestamps), the
refusals, and `--decoder attention` = no flag, by bytes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ctc_search_ref as R
from helpers import PKG, synthetic_batch

pytestmark = pytest.mark.gpu
HEAD_SCALE = 40.0             # the random head's weights times this: frames with clear winners, so that the margins below hold


def _model(**over):
    import test_gpu_ctc as C
    from oracle import las_oracle as O
    from las import layers as L, variables as V
    from las.las import LAS, Listener, Speller
    from las.beam_search import BeamSearch
    from utils.tokenizer import CharEncoder
    args = C._cfg_args("pblstm", "add", **dict(dict(convert_rate=0.3, beam_size=4, apply_lm=False, ctc_decode_weight=0.0, decoder="ctc"), **over))
    p0 = O.init_params(args, seed=11, cell="lstm", enc_type="pblstm")
    head = C._head_params(args, 2 * args.enc_units)
    head["Speller/dense/kernel"] = head["Speller/dense/kernel"] * np.float32(HEAD_SCALE)
    p0.update(head)
    L.set_cell("lstm")
    L.set_precision("f32")
    st = V.reset_default_store(device="cuda")
    st.load(p0)
    las = LAS(args, Listener, Speller, CharEncoder().token_to_id)
    las.build_variables()
    return args, BeamSearch(args, las, CharEncoder().token_to_id, None)


def _utts(args):
    return [synthetic_batch(1, T, 12, args.vocab_size, seed=8 + k)[0] for k, T in enumerate((64, 48, 56))]


def _head(bs, utts):
    with torch.no_grad():
        encs, enc_lens, _, h_one, _ = bs._run_encoders(None, utts)
        z = bs._ctc_logits(encs, h_one)
    torch.cuda.synchronize()
    return z.cpu().numpy(), [min(int(l), h.shape[1]) for l, h in zip(enc_lens, encs)]


def test_ctc_decode_batch_matches_the_restatement_on_the_same_logits():
    """beam 4 with a trigram and a length bonus, then greedy: token lists, their order and the scores against the float64 restatement
    over the head's own logits; the result lists have decode_batch's shape (ascending, best last, <SOS> in front, log_prob = total)"""
    import ngram_ref as G
    from las.ngram import NgramLM
    sc_tol = 4.0 * R.measured_tolerance()[1]
    args, bs = _model(ctc_len_bonus=0.5)
    V = args.vocab_size
    utts = _utts(args)
    z, T = _head(bs, utts)
    assert z.shape[2] == V + 1 and len(set(T)) > 1
    grams = G.random_model(np.random.RandomState(3), V, 3)
    lm = NgramLM(grams, 3, V, bs.start_id, bs.end_id, 0)
    for fused in (False, True):
        bs.set_ngram(lm if fused else None, R.LM_WEIGHT if fused else 0.0)
        gain = R.gram_gain(grams, 3, R.LM_WEIGHT, bs.start_id) if fused else None
        res = bs.ctc_decode_batch(None, utts)
        assert len(res) == len(utts) and res.align_inputs is None
        for u, r in enumerate(res):
            hyps, margin = R.beam_search(R.frame_summary(z[u], T[u], min(args.ctc_cand, V)), 4, bs.end_id, gain, 0.5)
            print("utterance", u, "fused", fused, "margin", margin, "best", hyps[0])
            assert margin >= R.MARGIN
            got = [(list(h.token_ids), float(h.log_prob)) for h in reversed(r)]
            assert [g[0] for g in got] == [[bs.start_id] + h[0] for h in hyps]
            for g, h in zip(got, hyps):
                assert abs(g[1] - h[1]) <= sc_tol
    bs.set_ngram(None, 0.0)
    # greedy
    args1, bs1 = _model(beam_size=1)
    z1, T1 = _head(bs1, utts)
    res = bs1.ctc_decode_batch(None, utts)
    for u, r in enumerate(res):
        s = R.frame_summary(z1[u], T1[u], 1)
        toks, score = R.greedy(s["best"], s["best_lp"], V)
        assert len(r) == 1 and list(r[0].token_ids) == [bs1.start_id] + toks
        assert abs(float(r[0].log_prob) - score) <= sc_tol
    # alignment inputs are retained on request, and align_results reads them
    bs1.retain_align = True
    res = bs1.ctc_decode_batch(None, utts)
    assert res.align_inputs is not None and res.align_inputs.ctc_lp is not None
    scores, spans = bs1.align_results(res)
    assert len(spans) == len(utts) and all(len(sp) == len(r[-1].token_ids) - 1 for sp, r in zip(spans, res))


def test_ctc_decode_batch_refusals():
    args, bs = _model()
    utts = _utts(args)
    for field, value, msg in (("ctc", False, "--ctc True"), ("ctc_decode_weight", 0.3, "--ctc_decode_weight"), ("beam_size", 65, "--beam_size"),
                              ("ctc_cand", 65, "--ctc_cand"), ("decoder", "attention", None)):
        keep = getattr(args, field)
        setattr(args, field, value)
        try:
            if msg is None:                                              # (the method does not depend on the flag: it IS the CTC search)
                continue
            with pytest.raises(ValueError, match=msg):
                bs.ctc_decode_batch(None, utts)
        finally:
            setattr(args, field, keep)
    assert len(bs.ctc_decode_batch(None, utts)) == len(utts)


# ---- command lines ------------------------------------------------------------------------------------------------------------------
MODEL = ["--unit", "char", "--feat_dim", "13", "--enc_type", "pblstm", "--enc_units", "64", "--num_enc_layers", "2", "--dec_units", "64",
         "--num_dec_layers", "1", "--attention_size", "32", "--embedding_size", "32", "--cell", "lstm"]


def _transcribe(tmp_path, *flags):
    cmd = [sys.executable, os.path.join(PKG, "transcribe.py"), "--synthetic", "True", "--max_steps", "3", "--save_dir", str(tmp_path / "none")]
    return subprocess.run(cmd + MODEL + list(flags), capture_output=True, text=True, timeout=600, cwd=str(tmp_path))


def test_transcribe_cli_ctc_greedy_and_beam(tmp_path):
    import test_gpu_ngram as TN
    r = _transcribe(tmp_path, "--ctc", "True", "--decoder", "ctc", "--beam_size", "1")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert len(r.stdout.splitlines()) == 3
    r = _transcribe(tmp_path, "--ctc", "True", "--decoder", "ctc", "--beam_size", "4", "--ngram_lm", TN._arpa(tmp_path), "--ngram_weight", "0.5",
                    "--nbest", "3", "--confidence", "True", "--timestamps", "True", "--ctc_len_bonus", "0.5")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 3
    for ln in lines:
        d = json.loads(ln)
        assert set(d) >= {"text", "score", "words", "nbest", "confidence"} and 1 <= len(d["nbest"]) <= 3
        assert d["nbest"][0]["posterior"] is not None


def test_transcribe_cli_ctc_refusals(tmp_path):
    import test_gpu_ngram as TN
    for flags, msg in ((["--decoder", "ctc"], "--ctc True"), (["--ctc", "True", "--decoder", "ctc", "--apply_lm", "True"], "--apply_lm"),
                       (["--ctc", "True", "--decoder", "ctc", "--beam_size", "1", "--ngram_lm", TN._arpa(tmp_path), "--ngram_weight", "1.0"],
                        "greedy"), (["--decoder", "transducer"], "--decoder")):
        r = _transcribe(tmp_path, *flags)
        assert r.returncode != 0 and "ValueError" in r.stderr and msg in r.stderr, (flags, r.stderr[-1500:])


def test_decoder_attention_is_the_default_by_bytes(tmp_path):
    a = _transcribe(tmp_path, "--ctc", "True", "--beam_size", "4")
    b = _transcribe(tmp_path, "--ctc", "True", "--beam_size", "4", "--decoder", "attention")
    assert a.returncode == 0 and b.returncode == 0, a.stderr[-1500:] + b.stderr[-1500:]
    assert a.stdout == b.stdout and len(a.stdout.splitlines()) == 3


def test_decode_cli_ctc(tmp_path):
    cmd = [sys.executable, os.path.join(PKG, "decode.py"), "--synthetic", "True", "--save_dir", str(tmp_path / "none"), "--ctc", "True",
           "--decoder", "ctc", "--beam_size", "4"] + MODEL
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0 and "Dev WER" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
