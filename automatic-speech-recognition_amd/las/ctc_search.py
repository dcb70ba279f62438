"""las.ctc_search -- transcripts from the CTC head alone: the frame summary, the greedy collapse and the CTC prefix beam
search with n-gram shallow fusion (las_ctc_frame_topk, las_ctc_greedy, las_ctc_beam_search, csrc/ctc_search.hip), without one Speller
step.  frame_topk / greedy / beam_search take the head's frame-major logits on the device and the encoded lengths on the host: one
upload (the lengths), the launches, one read-back.  decode_batch is BeamSearch.ctc_decode_batch: the encoders, the head product, the
search, and the result lists decode_batch returns.  The reference has no counterpart."""
import numpy as np
import torch

from las import _hip

MAX_BEAM = 64
MAX_CAND = 64
DECODERS = ("attention", "ctc")
RESCORERS = ("none", "attention")
MAX_RESCORE_ROWS = 1024


def check_args(args, force=False):
    """--decoder and what `--decoder ctc` refuses, before anything is built or launched; -> True for the CTC search.  force: the
    refusals whatever --decoder says (ctc_decode_batch IS the CTC search)"""
    dec = str(getattr(args, "decoder", "attention") or "attention").lower()
    if dec not in DECODERS:
        raise ValueError("--decoder %r: one of %s" % (dec, " | ".join(DECODERS)))
    res = rescorer(args)
    if dec != "ctc" and not force:
        if res != "none":
            raise ValueError("--rescore %s re-ranks the CTC search's N-best list: it needs --decoder ctc" % res)
        return False
    if not getattr(args, "ctc", False):
        raise ValueError("--decoder ctc needs the CTC head: decode with --ctc True (a model trained with --ctc)")
    if getattr(args, "apply_lm", False):
        raise ValueError("--decoder ctc: --apply_lm fuses the RNN LM into the Speller's search; the CTC search takes --ngram_lm")
    if (getattr(args, "hotwords", "") or "") or float(getattr(args, "hotword_weight", 0.0) or 0.0) != 0.0:
        raise ValueError("--decoder ctc: --hotwords biases the Speller's search; the CTC search has no hotword boosting")
    if float(getattr(args, "ctc_decode_weight", 0.0) or 0.0) > 0:
        raise ValueError("--decoder ctc: --ctc_decode_weight re-ranks the Speller's search with the head; here the head is the search")
    if res == "none":                                                  # (coverage counts the attention decoder's alignments)
        from las import coverage
        coverage.refuse_without_attention(args, "--decoder ctc without --rescore attention")
    K = int(args.beam_size)
    if not 1 <= K <= MAX_BEAM:
        raise ValueError("--decoder ctc: --beam_size between 1 and %d (got %d)" % (MAX_BEAM, K))
    lm_on = bool(getattr(args, "ngram_lm", "") or "") and float(getattr(args, "ngram_weight", 0.0) or 0.0) > 0
    if K == 1 and lm_on:
        raise ValueError("--decoder ctc --beam_size 1 is the greedy collapse: it has no search to fuse --ngram_lm into")
    _cand_flag(args)
    if not np.isfinite(float(getattr(args, "ctc_len_bonus", 0.0) or 0.0)):
        raise ValueError("--ctc_len_bonus must be finite")
    if res != "none":
        if K == 1:
            raise ValueError("--rescore %s --beam_size 1: the greedy collapse gives one hypothesis, nothing to re-rank" % res)
        w = float(getattr(args, "rescore_ctc_weight", 0.5))
        if not np.isfinite(w) or not 0.0 <= w <= 1.0:
            raise ValueError("--rescore_ctc_weight inside [0, 1] (got %r)" % (w,))
        rows = int(getattr(args, "rescore_rows", 64))
        if not 1 <= rows <= MAX_RESCORE_ROWS:
            raise ValueError("--rescore_rows between 1 and %d (got %d)" % (MAX_RESCORE_ROWS, rows))
    return True


def rescorer(args):
    """--rescore: none | attention"""
    res = str(getattr(args, "rescore", "none") or "none").lower()
    if res not in RESCORERS:
        raise ValueError("--rescore %r: one of %s" % (res, " | ".join(RESCORERS)))
    return res


def _cand_flag(args):
    c = int(getattr(args, "ctc_cand", 32))
    if not 1 <= c <= MAX_CAND:
        raise ValueError("--ctc_cand between 1 and %d (got %d)" % (MAX_CAND, c))
    return c


def cand(args):
    """C = min(--ctc_cand, V)"""
    return min(_cand_flag(args), int(args.vocab_size))


def _prepare(logits, enc_lens):
    if logits.dim() != 3 or logits.dtype != torch.float32:
        raise ValueError("ctc_search: logits are float32 [n, Tp, V + 1]")
    _hip.require_gpu(logits)
    logits = logits.contiguous()
    n, Tp, Vc = logits.shape
    if len(enc_lens) != n:
        raise ValueError("ctc_search: %d utterances, %d lengths" % (n, len(enc_lens)))
    lens = torch.as_tensor(np.asarray(enc_lens, np.int64).clip(0, Tp).astype(np.int32)).to(logits.device)
    return logits, lens, n, Tp, Vc


def _summary(logits, lens, n, Tp, Vc, C):
    """las_ctc_frame_topk into ONE int32 buffer [best | best_lp | blank_lp | cand_tok | cand_lp] (the float parts as bits)"""
    F = n * Tp
    buf = torch.zeros(3 * F + 2 * F * C, dtype=torch.int32, device=logits.device)
    v = dict(best=buf[:F], best_lp=buf[F:2 * F].view(torch.float32), blank_lp=buf[2 * F:3 * F].view(torch.float32),
             cand_tok=buf[3 * F:3 * F + F * C], cand_lp=buf[3 * F + F * C:].view(torch.float32))
    _hip.check(_hip.lib().las_ctc_frame_topk(_hip.p(logits), _hip.p(lens), n, Tp, Vc, C, _hip.p(v["cand_tok"]) if C else None,
                                             _hip.p(v["cand_lp"]) if C else None, _hip.p(v["blank_lp"]), _hip.p(v["best"]),
                                             _hip.p(v["best_lp"]), _hip.stream()), "las_ctc_frame_topk")
    return buf, v


def frame_topk(logits, enc_lens, C):
    """-> per utterance a dict of numpy arrays over its T'_u frames: best, best_lp, blank_lp, cand_tok [T', C], cand_lp [T', C]"""
    logits, lens, n, Tp, Vc = _prepare(logits, enc_lens)
    C = int(C)
    if not 1 <= C <= min(MAX_CAND, Vc - 1):
        raise ValueError("ctc_search.frame_topk: 1 <= C <= min(%d, V) (got %d)" % (MAX_CAND, C))
    buf, _ = _summary(logits, lens, n, Tp, Vc, C)
    h = buf.cpu().numpy()
    F = n * Tp
    best, blp, bl = h[:F].reshape(n, Tp), h[F:2 * F].view(np.float32).reshape(n, Tp), h[2 * F:3 * F].view(np.float32).reshape(n, Tp)
    ct, cl = h[3 * F:3 * F + F * C].reshape(n, Tp, C), h[3 * F + F * C:].view(np.float32).reshape(n, Tp, C)
    T = lens.cpu().tolist()
    return [dict(best=best[u, :T[u]].copy(), best_lp=blp[u, :T[u]].copy(), blank_lp=bl[u, :T[u]].copy(), cand_tok=ct[u, :T[u]].copy(),
                 cand_lp=cl[u, :T[u]].copy()) for u in range(n)]


def greedy(logits, enc_lens):
    """-> per utterance (tokens, score): the collapsed argmax path and the float64 sum of its log-probabilities"""
    logits, lens, n, Tp, Vc = _prepare(logits, enc_lens)
    _, v = _summary(logits, lens, n, Tp, Vc, 0)
    out = torch.zeros(2 * n + n + n * Tp, dtype=torch.int32, device=logits.device)     # [scores (fp64 bits, 8-byte aligned) | lens | tokens]
    sc, ln, tokens = out[:2 * n], out[2 * n:3 * n], out[3 * n:]
    _hip.check(_hip.lib().las_ctc_greedy(_hip.p(v["best"]), _hip.p(v["best_lp"]), _hip.p(lens), n, Tp, Vc - 1, _hip.p(tokens), _hip.p(ln),
                                         _hip.p(sc), _hip.stream()), "las_ctc_greedy")
    h = out.cpu().numpy()
    hs, hl, tok = h[:2 * n].view(np.float64), h[2 * n:3 * n], h[3 * n:].reshape(n, Tp)
    return [(tok[u, :hl[u]].tolist(), float(hs[u])) for u in range(n)]


def beam_search(logits, enc_lens, K, C, eos_id, lm=None, lm_weight=0.0, len_bonus=0.0, sos_id=1):
    """-> per utterance [(tokens, total)] best first, at most K: the CTC prefix beam search over the C best classes of every frame.
    lm: a las.ngram.NgramLM fused at lm_weight (None or weight 0: none)."""
    logits, lens, n, Tp, Vc = _prepare(logits, enc_lens)
    K, C, V = int(K), int(C), Vc - 1
    if not 1 <= K <= MAX_BEAM:
        raise ValueError("ctc_search.beam_search: 1 <= K <= %d (got %d)" % (MAX_BEAM, K))
    if not 1 <= C <= min(MAX_CAND, V):
        raise ValueError("ctc_search.beam_search: 1 <= C <= min(%d, V) (got %d)" % (MAX_CAND, C))
    if not np.isfinite(float(len_bonus)):
        raise ValueError("ctc_search.beam_search: the length bonus must be finite")
    lib = _hip.lib()
    tab, M, E, order, start = None, 0, 0, 0, 0
    if lm is not None and float(lm_weight) > 0:
        if lm.vocab_size != V:
            raise ValueError("ctc_search.beam_search: the LM is over %d tokens, the head over %d" % (lm.vocab_size, V))
        tab, M, E, order = lm.to(logits.device, float(lm_weight)), lm.num_nodes, lm.num_entries, lm.order
        start = lm.step(0, sos_id)
    _, v = _summary(logits, lens, n, Tp, Vc, C)
    out = torch.zeros(n * K * Tp + 2 * n * K + n, dtype=torch.int32, device=logits.device)       # [tokens | lens | totals (bits) | nhyp]
    o_len, o_tot, o_nh = n * K * Tp, n * K * Tp + n * K, n * K * Tp + 2 * n * K
    nbytes = lib.las_ctc_beam_workspace_bytes(n, Tp, K, C)
    ws = _hip.workspace(logits.device, nbytes, "ctc_search")
    t = (lambda k: _hip.p(tab[k])) if tab is not None else (lambda k: None)
    _hip.check(lib.las_ctc_beam_search(_hip.p(v["cand_tok"]), _hip.p(v["cand_lp"]), _hip.p(v["blank_lp"]), _hip.p(lens), n, Tp, V, K, C,
                                       int(eos_id), float(len_bonus), t("child_off"), t("child_tok"), t("child_lp"), t("child_next"),
                                       t("bow"), t("bo"), t("uni_lp"), t("uni_next"), M, E, order, start, _hip.p(out[:o_len]),
                                       _hip.p(out[o_len:o_tot]), _hip.p(out[o_tot:o_nh]), _hip.p(out[o_nh:]), _hip.p(ws), nbytes,
                                       _hip.stream()), "las_ctc_beam_search")
    h = out.cpu().numpy()
    tok, hl = h[:o_len].reshape(n, K, Tp), h[o_len:o_tot].reshape(n, K)
    tot, nh = h[o_tot:o_nh].view(np.float32).reshape(n, K), h[o_nh:]
    return [[(tok[u, k, :hl[u, k]].tolist(), float(tot[u, k])) for k in range(int(nh[u]))] for u in range(n)]


def decode_batch(bs, sess, xs_list):
    """BeamSearch.ctc_decode_batch: encoders, head product, greedy (beam_size 1) or prefix beam search -> decode_batch's result lists:
    per utterance the BeamStates ascending (best last), <SOS> in front, log_prob = the total (greedy: the path's log-probability)."""
    from las.beam_search import AlignInputs, BeamState, _Results
    args = bs.args
    check_args(args, force=True)
    bs.need_ctc_head("--decoder ctc")
    with torch.no_grad():
        encs, enc_lens, _, h_one, ctc_lp = bs._run_encoders(sess, xs_list)
        z = bs._ctc_logits(encs, h_one)
        T = [min(int(l), h.shape[1]) for l, h in zip(enc_lens, encs)]
        if bs.retain_align and ctc_lp is None:                         # the class-major copy only when an alignment will ask for it
            ctc_lp = bs._ctc_class_major(z)
        K = int(args.beam_size)
        if K == 1:
            hyps = [[h] for h in greedy(z, T)]
        else:
            hyps = beam_search(z, T, K, cand(args), bs.end_id, bs.ngram, bs.ngram_weight, float(getattr(args, "ctc_len_bonus", 0.0) or 0.0),
                               bs.start_id)
    _hip.check_status(z.device)
    if rescorer(args) != "none":                                       # the second pass (las.rescore is imported only here)
        from las import rescore
        return rescore.rescored_results(bs, encs, enc_lens, hyps, AlignInputs(encs, enc_lens, h_one, ctc_lp) if bs.retain_align else None)
    results = _Results([BeamState([bs.start_id] + list(tokens), np.float32(score) if K > 1 else score, [], None, None)
                        for tokens, score in reversed(hs)] for hs in hyps)
    results.align_inputs = AlignInputs(encs, enc_lens, h_one, ctc_lp) if bs.retain_align else None
    return results


def decode_batches(bs, sess, batches):
    """ctc_decode_batch over a sequence of batches (a batch may be a callable that makes it, as for decode_batches)"""
    for xs_list in batches:
        yield decode_batch(bs, sess, xs_list() if callable(xs_list) else xs_list)
