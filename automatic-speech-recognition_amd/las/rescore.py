"""las.rescore -- two-pass decoding: the attention decoder SCORES the hypotheses of the CTC prefix search under teacher
forcing and the list is re-ranked by (1 - w) attention + w first pass (las_rescore_score, las_rescore_rank, csrc/rescore.hip).  A
hypothesis is a known token string, so the second pass is the batched Speller loop training uses -- las_speller_fwd with explicit
tokens_in over chunks of at most `rows` hypotheses -- and one kernel that reads the per-hypothesis log-likelihoods off its logits in
place.  Imported only under `--rescore attention` (and by BeamSearch.score_hypotheses).  The reference has no counterpart."""
import numpy as np
import torch

from las import _hip

MAX_K = 64
MAX_ROWS = 1024


def scored_string(tokens, eos_id):
    """the string the attention decoder is asked about: the tokens (no <SOS>) through the first EOS; without one, the tokens plus EOS --
    the likelihood that the transcript ends there.  The empty hypothesis scores [EOS]."""
    toks = [int(t) for t in tokens]
    if eos_id in toks:
        return toks[:toks.index(eos_id) + 1]
    return toks + [int(eos_id)]


def score_rows(logits, y, lens, return_steps=False, out=None):
    """las_rescore_score over logits taken in place: a float32 device view [R, U, V] with a contiguous last axis and any row / step
    strides (the Speller's permuted time-major buffer, or a batch-major one); y int32 [R, ldy >= U] and lens int32 [R] on the device
    -> (att float64 [R], step_lp float32 [R, ldy] or None), both on the device.  step_lp entries at t >= lens[r] are NaN (not written).
    out: a contiguous float64 [R] tensor that receives att (every entry is written)."""
    if logits.dim() != 3 or logits.dtype != torch.float32 or logits.stride(2) != 1 and logits.shape[2] > 1:
        raise ValueError("rescore.score_rows: logits are a float32 view [R, U, V] with a contiguous last axis")
    _hip.require_gpu(logits, y, lens)
    R, U, V = logits.shape
    if y.dtype != torch.int32 or lens.dtype != torch.int32 or y.dim() != 2 or y.shape[0] != R or y.stride(1) != 1 or lens.shape != (R,):
        raise ValueError("rescore.score_rows: y int32 [R, ldy], lens int32 [R]")
    lens = lens.contiguous()
    dev = logits.device
    att = torch.empty(R, dtype=torch.float64, device=dev) if out is None else out
    if att.dtype != torch.float64 or att.shape != (R,) or not att.is_contiguous() or att.device != dev:
        raise ValueError("rescore.score_rows: out is a contiguous float64 [R] tensor on the logits' device")
    steps, ws, nbytes = None, None, 0
    if return_steps:
        steps = torch.full((R, y.stride(0)), float("nan"), dtype=torch.float32, device=dev)
    else:
        nbytes = _hip.lib().las_rescore_workspace_bytes(R, U)
        ws = _hip.workspace(dev, nbytes, "rescore")
    _hip.check(_hip.lib().las_rescore_score(_hip.p(logits), logits.stride(0), logits.stride(1), _hip.p(y), y.stride(0), _hip.p(lens), R, U, V,
                                            _hip.p(att), _hip.p(steps), _hip.p(ws), nbytes, _hip.stream()), "las_rescore_score")
    return att, steps


def _rank_device(first, att, nhyp, n, K, w, total, order):
    _hip.check(_hip.lib().las_rescore_rank(_hip.p(first), _hip.p(att), _hip.p(nhyp), n, K, float(w), _hip.p(total), _hip.p(order),
                                           _hip.stream()), "las_rescore_rank")


def _check_weight(w):
    w = float(w)
    if not np.isfinite(w) or not 0.0 <= w <= 1.0:
        raise ValueError("rescore: the first pass' weight is inside [0, 1] (got %r)" % (w,))
    return w


def rerank(first_scores, att, w, device=None):
    """las_rescore_rank: first_scores[u] / att[u] = the first-pass scores and attention log-likelihoods of utterance u's hypotheses in
    first-pass order (at most 64) -> (totals, orders) per utterance: totals[u][k] = float32((1 - w) att + w first), orders[u] = the
    slots by descending total (ties: the lower slot; NaN last)."""
    w = _check_weight(w)
    n = len(first_scores)
    if n == 0 or len(att) != n or any(len(a) != len(f) for a, f in zip(att, first_scores)):
        raise ValueError("rescore.rerank: %d utterances of first-pass scores, %d of attention scores, list by list of one length" % (n, len(att)))
    K = max(1, max(len(f) for f in first_scores))
    if K > MAX_K:
        raise ValueError("rescore.rerank: at most %d hypotheses per utterance (got %d)" % (MAX_K, K))
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    host = np.zeros(4 * n * K + n, np.int32)                           # [att (fp64 bits) | first (fp32 bits) | total | nhyp]: order is the output's
    h_att, h_first, h_nh = host[:2 * n * K].view(np.float64).reshape(n, K), host[2 * n * K:3 * n * K].view(np.float32).reshape(n, K), host[4 * n * K:]
    for u in range(n):
        nh = len(first_scores[u])
        h_nh[u] = nh
        h_att[u, :nh] = np.asarray(att[u], np.float64)
        h_first[u, :nh] = np.asarray(first_scores[u], np.float32)
    d = torch.from_numpy(host).to(dev)
    order = torch.zeros(n * K, dtype=torch.int32, device=dev)
    _rank_device(d[2 * n * K:3 * n * K], d[:2 * n * K], d[4 * n * K:], n, K, w, d[3 * n * K:4 * n * K], order)
    tot = d[3 * n * K:4 * n * K].cpu().numpy().view(np.float32).reshape(n, K)
    od = order.cpu().numpy().reshape(n, K)
    return [tot[u, :h_nh[u]].copy() for u in range(n)], [od[u, :h_nh[u]].tolist() for u in range(n)]


def _check_rows(rows):
    rows = int(rows)
    if not 1 <= rows <= MAX_ROWS:
        raise ValueError("rescore: between 1 and %d rows per Speller call (got %d)" % (MAX_ROWS, rows))
    return rows


def teacher_forced_logits(bs, encs, enc_lens, strings, rows=64, with_alphas=False):
    """The second pass' Speller calls: the rows -- strings[u][k], utterance by utterance -- in chunks of at most `rows`; a chunk may hold
    several utterances and may split one.  Yields per chunk (first row, logits [B, U, V] (a view of the time-major buffer), y int32
    [B, U], lens int32 [B]): U = the chunk's longest string, the encoder block of a row its utterance's output zero-padded to the
    chunk's longest (enc_len masks the rest), tokens_in[0] = <SOS>, tokens_in[t] = s[t - 1].  No dropout mask and no variational noise
    (BeamSearch's decode step passes none either), no in-loop logits, no gradient.  The logits buffer is rows * U * V * 4 bytes.
    with_alphas: every chunk is followed by the Speller's time-major alignments [U, B, T'] and the rows' enc_len int32 [B] (what
    las_coverage_rows reads)."""
    rows = _check_rows(rows)
    if len(encs) != len(strings) or len(enc_lens) != len(strings):
        raise ValueError("rescore: %d encoder outputs, %d lengths, %d hypothesis lists" % (len(encs), len(enc_lens), len(strings)))
    dev = encs[0].device
    flat = [(u, s) for u, ss in enumerate(strings) for s in ss]
    V = int(bs.args.vocab_size)
    for u, s in flat:
        if not s or min(s) < 0 or max(s) >= V:
            raise ValueError("rescore: utterance %d: a scored string is empty or holds a token outside [0, %d)" % (u, V))
    Hd = encs[0].shape[2]
    for c0 in range(0, len(flat), rows):
        chunk = flat[c0:c0 + rows]
        B = len(chunk)
        utts = sorted({u for u, _ in chunk})
        slot = {u: i for i, u in enumerate(utts)}
        U = max(len(s) for _, s in chunk)
        Tp = max(encs[u].shape[1] for u in utts)
        host = np.zeros((2 * U + 3) * B, np.int32)                     # [tokens_in (U B) | y (B U) | lens | enc_len | utterance slot]
        tin, y = host[:U * B].reshape(U, B), host[U * B:2 * U * B].reshape(B, U)
        lens, el, us = host[2 * U * B:2 * U * B + B], host[2 * U * B + B:2 * U * B + 2 * B], host[2 * U * B + 2 * B:]
        tin[:] = bs.end_id                                             # (behind a row's end: any token; its steps are not scored)
        tin[0] = bs.start_id
        for i, (u, s) in enumerate(chunk):
            L = len(s)
            y[i, :L] = s
            tin[1:L, i] = s[:L - 1]
            lens[i], el[i], us[i] = L, int(float(enc_lens[u])), slot[u]
        d = torch.from_numpy(host).to(dev)
        enc_u = torch.zeros(len(utts), Tp, Hd, device=dev)
        for u in utts:
            enc_u[slot[u], :encs[u].shape[1]] = encs[u][0]
        enc = enc_u.index_select(0, d[2 * U * B + 2 * B:].long())       # the encoder block repeated per row, as training has it
        prepared = {"B": B, "U": U, "enc_len_i32": d[2 * U * B + B:2 * U * B + 2 * B], "tokens_in": d[:U * B].view(U, B), "step_logits": False,
                    "emb_mask": None, "emb_noise": None}
        with torch.no_grad():
            try:
                logits, _, alphas = bs.speller(enc, None, U, is_training=False, prepared=prepared)
            except RuntimeError as e:
                raise ValueError("rescore: the Speller refuses the chunk's geometry (%d rows, %d encoder frames, %d steps): %s" % (B, Tp, U, e))
        out = (c0, logits, d[U * B:2 * U * B].view(B, U), d[2 * U * B:2 * U * B + B])
        yield out + (alphas.permute(1, 0, 2), prepared["enc_len_i32"]) if with_alphas else out


def _score_device(bs, encs, enc_lens, strings, rows, return_steps, cover=None):
    """-> (att float64 [N] on the device, the N rows in utterance order; per row its step terms (a device tensor) or None); with a
    coverage setting `cover` a third item: the rows' (covered, over, frames) int32 [N, 3] on the device -- las_coverage_rows on the
    teacher-forced alignments of the scored string's steps"""
    N = sum(len(s) for s in strings)
    att = torch.empty(N, dtype=torch.float64, device=encs[0].device)
    steps, counts = [], []
    for chunk in teacher_forced_logits(bs, encs, enc_lens, strings, rows, with_alphas=cover is not None):
        c0, logits, y, lens = chunk[:4]
        _, st = score_rows(logits, y, lens, return_steps, out=att[c0:c0 + logits.shape[0]])
        if return_steps:
            steps.append(st)
        if cover is not None:
            from las import coverage
            alphas, el = chunk[4], chunk[5]
            counts.append(torch.cat([coverage.rows_counts(alphas, lens, el, cover.tau, cover.kappa),
                                     el.clamp(0, alphas.shape[2]).unsqueeze(1)], 1))
    if cover is not None:
        return att, (steps if return_steps else None), torch.cat(counts, 0)
    return att, (steps if return_steps else None)


def attention_scores(bs, encs, enc_lens, token_lists, rows=64, return_steps=False):
    """The attention decoder's log-likelihood of every hypothesis: encs / enc_lens as BeamSearch._run_encoders returns them,
    token_lists[u] = utterance u's hypotheses (token ids, no <SOS>) -> att[u][k] (float), with return_steps also steps[u][k] = the
    float32 log-probabilities of the scored string's tokens (scored_string: through the first EOS, or with one appended).  One
    read-back."""
    strings = [[scored_string(t, bs.end_id) for t in tl] for tl in token_lists]
    if not any(strings):
        return ([[] for _ in strings], [[] for _ in strings]) if return_steps else [[] for _ in strings]
    att, steps = _score_device(bs, encs, enc_lens, strings, rows, return_steps)
    rows = _check_rows(rows)
    if return_steps:                                                   # (one buffer: the scores' bits, then every chunk's step terms)
        both = torch.cat([att.view(torch.int32)] + [s.reshape(-1).view(torch.int32) for s in steps]).cpu().numpy()
        h, hs, o = both[:2 * att.shape[0]].view(np.float64), [], 2 * att.shape[0]
        for s in steps:
            hs.append(both[o:o + s.numel()].view(np.float32).reshape(s.shape))
            o += s.numel()
    else:
        h = att.cpu().numpy()
    _hip.check_status(att.device)
    out_a, out_s, i = [], [], 0
    for ss in strings:                                                 # (row i is row i % rows of chunk i // rows)
        out_a.append([float(h[i + k]) for k in range(len(ss))])
        if return_steps:
            out_s.append([hs[(i + k) // rows][(i + k) % rows, :len(s)].copy() for k, s in enumerate(ss)])
        i += len(ss)
    return (out_a, out_s) if return_steps else out_a


def rescored_results(bs, encs, enc_lens, hyps, kept):
    """ctc_decode_batch's second pass: hyps[u] = the first pass' [(tokens, score)] best first -> decode_batch's result lists re-ranked by
    total = (1 - w) att + w first: ascending, best last, <SOS> in front, log_prob = total; `rescored[u]` lists, aligned with the
    returned order, dicts first / att / total / first_rank.  Scores and ranks come back in one read-back."""
    from las.beam_search import BeamState, _Results
    args = bs.args
    w = _check_weight(getattr(args, "rescore_ctc_weight", 0.5))
    rows = _check_rows(getattr(args, "rescore_rows", 64))
    n = len(hyps)
    K = max(1, max(len(h) for h in hyps))
    if K > MAX_K:
        raise ValueError("rescore: at most %d hypotheses per utterance (got %d)" % (MAX_K, K))
    strings = [[scored_string(t, bs.end_id) for t, _ in hs] for hs in hyps]
    N = sum(len(s) for s in strings)
    results = _Results([] for _ in range(n))
    results.align_inputs = kept
    results.rescored = [[] for _ in range(n)]
    if N == 0:
        return results
    dev = encs[0].device
    cover = getattr(bs, "coverage", None)                              # (the counts of the teacher-forced alignments)
    if cover is None:
        att_flat, _ = _score_device(bs, encs, enc_lens, strings, rows, False)
        att_raw = cnt = None
    else:
        att_raw, _, cnt = _score_device(bs, encs, enc_lens, strings, rows, False, cover)
        # att + fl32(w_c covered) - fl32(w_o over): the two products are float32 roundings, the sums are float64
        cf = cnt[:, :2].to(torch.float32)
        att_flat = att_raw + ((cf[:, 0] * float(np.float32(cover.w_c))).double() - (cf[:, 1] * float(np.float32(cover.w_o))).double())
        att_raw, cnt = att_raw.cpu().numpy(), cnt.cpu().numpy()
    host = np.zeros(n * K + n + N, np.int32)                           # [first (fp32 bits) | nhyp | the rows' slots u K + k]
    h_first, h_nh, h_pos = host[:n * K].view(np.float32).reshape(n, K), host[n * K:n * K + n], host[n * K + n:]
    i = 0
    for u, hs in enumerate(hyps):
        h_nh[u] = len(hs)
        h_first[u, :len(hs)] = [sc for _, sc in hs]
        h_pos[i:i + len(hs)] = u * K + np.arange(len(hs))
        i += len(hs)
    d = torch.from_numpy(host).to(dev)
    out = torch.zeros(4 * n * K, dtype=torch.int32, device=dev)        # [att (fp64 bits, 8-byte aligned) | total (fp32 bits) | order]
    att = out[:2 * n * K].view(torch.float64)
    att.index_copy_(0, d[n * K + n:].long(), att_flat)
    _rank_device(d[:n * K], att, d[n * K:n * K + n], n, K, w, out[2 * n * K:3 * n * K], out[3 * n * K:])
    h = out.cpu().numpy()
    _hip.check_status(dev)
    h_att, h_tot, h_ord = h[:2 * n * K].view(np.float64).reshape(n, K), h[2 * n * K:3 * n * K].view(np.float32).reshape(n, K), h[3 * n * K:].reshape(n, K)
    base = np.concatenate(([0], np.cumsum([len(hs) for hs in hyps])))
    for u, hs in enumerate(hyps):
        for k in reversed(h_ord[u, :len(hs)].tolist()):                # ascending: the best last
            results[u].append(BeamState([bs.start_id] + list(hs[k][0]), np.float32(h_tot[u, k]), [], None, None))
            results.rescored[u].append(dict(first=float(hs[k][1]), att=float(h_att[u, k]), total=float(h_tot[u, k]), first_rank=int(k)))
            if cnt is not None:                                        # att: with the coverage term; att_score: the decoder's own
                row = int(base[u]) + k
                results[u][-1].coverage = tuple(int(x) for x in cnt[row])
                results.rescored[u][-1].update(att_score=float(att_raw[row]), coverage=results[u][-1].coverage)
    return results
