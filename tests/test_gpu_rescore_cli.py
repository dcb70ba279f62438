"""Two-pass decoding from the entry points, on the small f32 model of test_gpu_ctc_search_cli with ragged utterances:
BeamSearch.score_hypotheses against the float64 oracle Speller under teacher forcing, the attention search's own 1-best against the
teacher-forced loop, chunks that split utterances, ctc_decode_batch with --rescore attention against the restatement, and the command
lines.

The bound of every comparison with the oracle or the step-by-step search is 2 L eps: L the scored length, eps the tolerance the
Speller parity test (test_gpu_las_parity.TOL) allows the f32 logits; log-softmax is 2-Lipschitz in the sup norm, so L terms move by at
most 2 L eps when every logit moves by at most eps."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rescore_ref as R
import test_gpu_ctc_search_cli as C
from helpers import PKG

pytestmark = pytest.mark.gpu
W = 0.3


def _eps():
    import test_gpu_las_parity as P
    return P.TOL[("f32", "lstm")]["logits"]


@functools.lru_cache(maxsize=None)
def _first_pass():
    """the model, its encoder outputs and the CTC search's lists (no rescoring), scored once by score_hypotheses (rows = 64, with the
    step terms): shared by the tests below and left unchanged"""
    args, bs = C._model()
    utts = C._utts(args)
    with torch.no_grad():
        encs, enc_lens, _, _, _ = bs._run_encoders(None, utts)
    res = bs.ctc_decode_batch(None, utts)
    token_lists = [[list(h.token_ids[1:]) for h in reversed(r)] for r in res]            # best first, no <SOS>
    firsts = [[float(h.log_prob) for h in reversed(r)] for r in res]
    att, steps = bs.score_hypotheses(encs, enc_lens, token_lists, rows=64, return_steps=True)
    torch.cuda.synchronize()
    assert len({h.shape[1] for h in encs}) > 1 and all(len(t) >= 1 for t in token_lists)
    return dict(args=args, bs=bs, utts=utts, encs=encs, enc_lens=enc_lens, res=res, token_lists=token_lists, firsts=firsts, att=att, steps=steps)


def _oracle_scores(f):
    """oracle.las_oracle.speller_forward in float64 under teacher forcing on the device's encoder outputs -> per utterance, per
    hypothesis the float64 log-probabilities of its scored string"""
    from oracle import las_oracle as O
    args, bs = f["args"], f["bs"]
    p = O.to_torch(O.init_params(args, seed=11, cell="lstm", enc_type="pblstm"), dtype=torch.float64)      # (_model's Speller weights)
    out = []
    for u, tl in enumerate(f["token_lists"]):
        strings = [R.scored_string(t, bs.end_id) for t in tl]
        U = max(len(s) for s in strings)
        teacher = torch.full((len(strings), U), bs.end_id, dtype=torch.long)
        for k, s in enumerate(strings):
            teacher[k, :len(s)] = torch.tensor(s)
        enc = f["encs"][u].detach().cpu().to(torch.float64).expand(len(strings), -1, -1).contiguous()
        el = np.full(len(strings), float(f["enc_lens"][u]), np.float64)
        with torch.no_grad():
            logits, _ = O.speller_forward(enc, el, U, p, args, "lstm", teacher=teacher, is_training=True)
        lp = torch.log_softmax(logits, -1).gather(2, teacher[..., None])[..., 0].numpy()
        out.append([lp[k, :len(s)] for k, s in enumerate(strings)])
    return out


def test_score_hypotheses_against_the_float64_oracle():
    f = _first_pass()
    eps = _eps()
    worst = 0.0
    for u, per_hyp in enumerate(_oracle_scores(f)):
        for k, lp in enumerate(per_hyp):
            L = len(lp)
            assert len(f["steps"][u][k]) == L == len(R.scored_string(f["token_lists"][u][k], f["bs"].end_id))
            d_att = abs(f["att"][u][k] - float(lp.sum()))
            d_step = float(np.abs(f["steps"][u][k].astype(np.float64) - lp).max())
            worst = max(worst, d_att / (2 * L * eps))
            print("utterance %d hypothesis %d: L = %d, |att - oracle| = %.3g (allowed %.3g), worst step %.3g" % (u, k, L, d_att, 2 * L * eps, d_step))
            assert d_att <= 2 * L * eps and d_step <= 2 * eps
    print("largest deviation seen, as a share of the bound 2 L eps: %.3g" % worst)


def test_teacher_forced_loop_agrees_with_the_step_by_step_search():
    """The attention search's own 1-best (beam 4, no LM, no CTC weight) scored by score_hypotheses.  The search ranks by the sum of RAW
    logits, score_hypotheses gives log-probabilities: the two differ by the steps' log-sum-exp, which is read off the
    teacher-forced loop's own logits -- log_prob = sum of the step terms + sum of lse, within 2 L eps; and the raw logits of the two
    loops agree token by token.  A hypothesis that does not end in EOS is scored with one appended: that last term is left out."""
    from las import rescore
    f = _first_pass()
    eps = _eps()
    args_a, bs_a = C._model(decoder="attention")
    res = bs_a.decode_batch(None, f["utts"])
    best = [list(r[-1].token_ids[1:]) for r in res]
    assert all(len(b) >= 1 for b in best)
    with torch.no_grad():
        encs, enc_lens, _, _, _ = bs_a._run_encoders(None, f["utts"])
    att, steps = bs_a.score_hypotheses(encs, enc_lens, [[b] for b in best], return_steps=True)
    strings = [[R.scored_string(b, bs_a.end_id)] for b in best]
    (c0, logits, y, lens), = list(rescore.teacher_forced_logits(bs_a, encs, enc_lens, strings, rows=64))
    z = logits.cpu().numpy().astype(np.float64)                                          # [3, U, V]
    for u, b in enumerate(best):
        L = len(b)                                                                       # the search's own tokens (an appended EOS is not its)
        assert strings[u][0][:L] == b and len(strings[u][0]) in (L, L + 1)
        raw = sum(z[u, t, b[t]] for t in range(L))
        lse = [float(np.log(np.exp(z[u, t] - z[u, t].max()).sum()) + z[u, t].max()) for t in range(L)]
        got = float(np.sum(steps[u][0][:L].astype(np.float64))) + sum(lse)
        lp = float(res[u][-1].log_prob)
        print("utterance %d: L = %d, search log_prob %.6f, teacher-forced raw sum %.6f, terms + lse %.6f (allowed %.3g)" % (u, L, lp, raw, got, 2 * L * eps))
        assert abs(raw - lp) <= 2 * L * eps and abs(got - lp) <= 2 * L * eps
        if len(strings[u][0]) == L:
            assert abs(att[u][0] + sum(lse) - lp) <= 2 * L * eps


def test_chunks_that_split_utterances_and_mix_encoder_lengths():
    from las import rescore
    f = _first_pass()
    eps = _eps()
    att3, steps3 = f["bs"].score_hypotheses(f["encs"], f["enc_lens"], f["token_lists"], rows=3, return_steps=True)
    assert sum(len(t) for t in f["token_lists"]) > 3 and any(len(t) % 3 for t in f["token_lists"])      # (a chunk splits an utterance)
    for u, tl in enumerate(f["token_lists"]):
        for k, t in enumerate(tl):
            L = len(R.scored_string(t, f["bs"].end_id))
            assert abs(att3[u][k] - f["att"][u][k]) <= 2 * L * eps and len(steps3[u][k]) == L
    o3 = rescore.rerank(f["firsts"], att3, W)[1]
    o64 = rescore.rerank(f["firsts"], f["att"], W)[1]
    assert o3 == o64


def test_ctc_decode_batch_with_attention_rescoring():
    f = _first_pass()
    att_tol = 4.0 * R.measured_tolerance()[1]
    args, bs = C._model(rescore="attention", rescore_ctc_weight=W)
    bs.retain_align = True
    res = bs.ctc_decode_batch(None, f["utts"])
    assert len(res) == len(f["utts"]) and res.align_inputs is not None and len(res.rescored) == len(res)
    for u, r in enumerate(res):
        got = [list(h.token_ids) for h in reversed(r)]                                   # best first
        resc = list(reversed(res.rescored[u]))
        assert len(resc) == len(got) == len(f["token_lists"][u])
        ranks = [d["first_rank"] for d in resc]
        assert sorted(ranks) == list(range(len(got)))                                    # a permutation of the first pass' list
        for g, d in zip(got, resc):
            assert g == [bs.start_id] + f["token_lists"][u][d["first_rank"]]
            assert abs(d["first"] - f["firsts"][u][d["first_rank"]]) <= att_tol
        first = np.zeros(len(got), np.float32)
        att = np.zeros(len(got), np.float64)
        for d in resc:
            first[d["first_rank"]], att[d["first_rank"]] = d["first"], d["att"]
        tot, order = R.rank(first, att, W)                                               # the restatement fed `first` and `att`
        assert ranks == order, (u, ranks, order)
        for h, d in zip(reversed(r), resc):
            assert float(h.log_prob) == d["total"] and abs(d["total"] - float(tot[d["first_rank"]])) <= att_tol
            L = len(R.scored_string(f["token_lists"][u][d["first_rank"]], bs.end_id))
            assert abs(d["att"] - f["att"][u][d["first_rank"]]) <= 2 * L * _eps()
    scores, spans = bs.align_results(res)
    assert len(spans) == len(res) and all(len(sp) == len(r[-1].token_ids) - 1 for sp, r in zip(spans, res))
    # w = 1 reproduces the first pass' order
    args.rescore_ctc_weight = 1.0
    res1 = bs.ctc_decode_batch(None, f["utts"])
    for u, r in enumerate(res1):
        assert [list(h.token_ids[1:]) for h in reversed(r)] == f["token_lists"][u]
        assert [d["first_rank"] for d in reversed(res1.rescored[u])] == list(range(len(r)))
    # the method refuses what the flags refuse
    args.rescore_ctc_weight = 1.5
    with pytest.raises(ValueError, match="--rescore_ctc_weight"):
        bs.ctc_decode_batch(None, f["utts"])


# ---- command lines ------------------------------------------------------------------------------------------------------------------
CTC = ["--ctc", "True", "--decoder", "ctc", "--beam_size", "4"]
RESCORE = CTC + ["--rescore", "attention", "--rescore_ctc_weight", "0.3"]


def test_transcribe_cli_rescore_nbest_timestamps(tmp_path):
    r = C._transcribe(tmp_path, *(RESCORE + ["--nbest", "3", "--timestamps", "True"]))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 3
    for ln in lines:
        d = json.loads(ln)
        assert set(d) >= {"text", "score", "words", "nbest"} and 1 <= len(d["nbest"]) <= 3
        for e in d["nbest"]:
            assert set(e) >= {"text", "score", "posterior", "ctc_score", "att_score"}
            assert e["ctc_score"] is not None and e["att_score"] is not None and e["att_score"] < 0
            assert abs(e["score"] - (0.7 * e["att_score"] + 0.3 * e["ctc_score"])) <= 1e-4 * max(1.0, abs(e["score"]))


def test_decode_cli_rescore(tmp_path):
    cmd = [sys.executable, os.path.join(PKG, "decode.py"), "--synthetic", "True", "--save_dir", str(tmp_path / "none")] + RESCORE + C.MODEL
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0 and "Dev WER" in r.stdout + r.stderr, r.stdout[-2000:] + r.stderr[-2000:]


def test_cli_rescore_refusals(tmp_path):
    for flags, msg in ((["--ctc", "True", "--rescore", "attention"], "--rescore"),
                       (["--ctc", "True", "--decoder", "ctc", "--beam_size", "1", "--rescore", "attention"], "--beam_size 1"),
                       (CTC + ["--rescore", "attention", "--rescore_ctc_weight", "1.5"], "--rescore_ctc_weight"),
                       (CTC + ["--rescore", "attention", "--rescore_ctc_weight", "nan"], "--rescore_ctc_weight"),
                       (CTC + ["--rescore", "rnnlm"], "--rescore")):
        r = C._transcribe(tmp_path, *flags)
        assert r.returncode != 0 and "ValueError" in r.stderr and msg in r.stderr, (flags, r.stderr[-1500:])


def test_rescore_none_is_the_default_by_bytes(tmp_path):
    a = C._transcribe(tmp_path, *CTC)
    b = C._transcribe(tmp_path, *(CTC + ["--rescore", "none"]))
    assert a.returncode == 0 and b.returncode == 0, a.stderr[-1500:] + b.stderr[-1500:]
    assert a.stdout == b.stdout and len(a.stdout.splitlines()) == 3
