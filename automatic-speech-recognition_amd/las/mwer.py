"""las.mwer -- minimum word error rate training (Prabhavalkar et al. 2018): the expected number of word errors over K
hypotheses per utterance and its gradient on the Speller's logits (las_mwer_loss, csrc/mwer.hip), the hypotheses' error counts through
the N-best distance kernel (las_nbest_risk), and the rows of the `--mwer` branch of LAS._train_step_impl: every utterance's encoder
output is repeated to S = K + 1 Speller rows, slots 0 .. K-1 the hypotheses (given, or drawn inside the loop), slot K the teacher-forced
reference whose cross entropy keeps the model where it is.  Imported only under `--mwer`.  The reference has no counterpart."""
import numpy as np
import torch

from las import _hip
from las import nbest
from las.rescore import scored_string

MAX_HYPS = 63                      # + the reference's slot: 64 rows per utterance, the ceiling of las_mwer_loss and of las_nbest_risk
EOS_ID = 2                         # utils/tokenizer.py SPECIAL_TOKENS
MODES = {"nbest": 0, "sample": 1}


def eos_of(id_to_token):
    for i, t in (id_to_token or {}).items():
        if t == "<EOS>":
            return int(i)
    return EOS_ID


def check_flags(args, dp=None):
    """--mwer against what it cannot go with: a ValueError before anything is enqueued.  -> (K, unit, norm or "")"""
    K, unit, norm = int(getattr(args, "mwer_hyps", 4)), str(getattr(args, "mwer_unit", "word")), str(getattr(args, "mwer_norm", "") or "")
    if not 1 <= K <= MAX_HYPS:
        raise ValueError("--mwer_hyps %d: between 1 and %d (with the reference's slot an utterance has at most 64 rows)" % (K, MAX_HYPS))
    if unit not in ("word", "token"):
        raise ValueError("--mwer_unit %s: word or token" % unit)
    if norm not in ("", "sample", "nbest"):
        raise ValueError("--mwer_norm %s: sample or nbest" % norm)
    if dp is not None:
        raise ValueError("--mwer: data-parallel training is not built (the expected word errors are normalised per rank)")
    if bool(getattr(args, "ctc", False)):
        raise ValueError("--mwer with --ctc: the CTC term over the repeated rows is not built; fine-tune with one of them")
    if int(getattr(args, "mwer_extra_steps", 4)) < 0:
        raise ValueError("--mwer_extra_steps %d: not negative" % int(args.mwer_extra_steps))
    return K, unit, norm


# ---- error counts ----------------------------------------------------------------------------------------------------------------------
def _cut(tokens, eos_id):
    """the string a row stands for, without its EOS: rescore.scored_string's rule (through the first EOS, or all of it)"""
    return scored_string(tokens, eos_id)[:-1]


def _distances(symbol_lists):
    """las_nbest_risk with zero weights over symbol_lists[u] = [reference, hypotheses ...] -> (dist int32 [n, K', K'] on the device, K')"""
    m = nbest._pack(symbol_lists, [np.zeros(len(t), np.float32) for t in symbol_lists])
    n, K = m["n"], m["K"]
    out = torch.zeros(n * K * K + n * K + n, dtype=torch.int32, device=m["dev"])
    nbest._risk(m, out)
    return out[:n * K * K].view(n, K, K), K


def word_errors(ref_tokens, hyp_token_lists, id_to_token, unit, mwer_unit="word", eos_id=None, distance=None):
    """err[u][k] (float32 arrays) = the edit distance between hypothesis k of utterance u and its reference, in words (mwer_unit
    "word": the words las.nbest.word_symbols makes of the tokens under `unit`) or in tokens ("token").  Strings end at their first EOS.
    The reference sits in slot 0 of a las_nbest_risk call with zero weights, the hypotheses behind it: err = dist[u, 0, 1:].  One
    upload, one call, one read-back.  distance (tests): a function (a, b) -> edit distance that replaces the device call."""
    if mwer_unit not in ("word", "token"):
        raise ValueError("mwer.word_errors: mwer_unit %s: word or token" % mwer_unit)
    eos = eos_of(id_to_token) if eos_id is None else int(eos_id)
    lists = [[_cut(r, eos)] + [_cut(h, eos) for h in hs] for r, hs in zip(ref_tokens, hyp_token_lists)]
    if mwer_unit == "word" and not id_to_token:
        raise ValueError("mwer.word_errors: counting words needs the tokenizer's id_to_token (or use mwer_unit token)")
    symbols, _ = nbest.word_symbols(lists, id_to_token, unit if mwer_unit == "word" else "token")
    if distance is not None:
        return [np.asarray([distance(s[0], h) for h in s[1:]], np.float32) for s in symbols]
    if not symbols:
        return []
    dist, _ = _distances(symbols)
    d = dist.cpu().numpy()
    return [d[u, 0, 1:len(s)].astype(np.float32) for u, s in enumerate(symbols)]


# ---- the loss --------------------------------------------------------------------------------------------------------------------------
def loss_rows(logits, y, lens, nhyp, err, S, mode, scale, grad=True):
    """las_mwer_loss over logits taken in place: a float32 device view [n S, U, V] with a contiguous last axis (the Speller's permuted
    time-major buffer); y int32 [n S, ldy >= U], lens int32 [n S], nhyp int32 [n], err float32 [n S], scale float32 [1], all on the
    device -> dict(loss [1], risk [n], seq_lp float64 [n S] (NaN: an absent slot), post, coef [n S], dlogits (the logits' strides) or
    None).  No synchronisation."""
    if logits.dim() != 3 or logits.dtype != torch.float32 or logits.stride(2) != 1 and logits.shape[2] > 1:
        raise ValueError("mwer.loss_rows: logits are a float32 view [R, U, V] with a contiguous last axis")
    _hip.require_gpu(logits, y, lens, nhyp, err, scale)
    R, U, V = logits.shape
    n = R // S
    if n * S != R or y.dtype != torch.int32 or y.shape[0] != R or y.stride(1) != 1 or lens.shape != (R,) or nhyp.shape != (n,) or err.shape != (R,):
        raise ValueError("mwer.loss_rows: %d rows are not n x %d slots, or y / lens / nhyp / err do not match them" % (R, S))
    dev = logits.device
    f = torch.empty(2 * R + n + 1, device=dev)
    post, coef, risk, loss = f[:R], f[R:2 * R], f[2 * R:2 * R + n], f[2 * R + n:]
    seq_lp = torch.full((R,), float("nan"), dtype=torch.float64, device=dev)
    dl = torch.empty_strided(logits.shape, logits.stride(), device=dev) if grad else None
    lib = _hip.lib()
    nbytes = lib.las_mwer_workspace_bytes(n, S, U)
    ws = _hip.workspace(dev, nbytes, "mwer")
    _hip.check(lib.las_mwer_loss(_hip.p(logits), logits.stride(0), logits.stride(1), V, _hip.p(y), y.stride(0), _hip.p(lens.contiguous()),
                                 _hip.p(nhyp.contiguous()), _hip.p(err.contiguous()), n, S, U, int(mode), _hip.p(scale), _hip.p(seq_lp),
                                 _hip.p(post), _hip.p(coef), _hip.p(risk), _hip.p(loss), _hip.p(dl), _hip.p(ws), nbytes, _hip.stream()),
               "las_mwer_loss")
    return dict(loss=loss, risk=risk, seq_lp=seq_lp, post=post, coef=coef, dlogits=dl)


# ---- the rows of a --mwer step ---------------------------------------------------------------------------------------------------------
class Rows(object):
    """what LAS._train_step_impl's --mwer branch carries from the set-up in front of the Listener to the loss behind the Speller"""


def check_step(las, hyps, n):
    """what a --mwer step refuses, on the host before anything is enqueued: the flags (check_flags), a word count without a tokenizer,
    hypothesis lists that do not fit the batch or hold a token outside the vocabulary.  -> the strings the hypotheses are scored as
    (scored_string: through the first EOS, or with one appended), None when they are drawn"""
    a = las.args
    K, unit, _ = check_flags(a, las.dp)
    if unit == "word" and not las.id_to_token:
        raise ValueError("--mwer_unit word needs the tokenizer's id_to_token (LAS(args, ..., id_to_token)); --mwer_unit token does not")
    if hyps is None:
        return None
    V, eos = int(a.vocab_size), eos_of(las.id_to_token)
    if len(hyps) != n or any(len(h) > K for h in hyps):
        raise ValueError("--mwer: %d hypothesis lists for %d utterances, at most --mwer_hyps %d each" % (len(hyps), n, K))
    strings = [[scored_string(h, eos) for h in hs] for hs in hyps]
    for u, ss in enumerate(strings):
        for s in ss:
            if min(s) < 0 or max(s) >= V:
                raise ValueError("--mwer: utterance %d: a hypothesis holds a token outside [0, %d)" % (u, V))
    return strings


def plan_rows(las, y, tokenlen, dec_steps, strings, dev):
    """Host half, before the Listener: the geometry (n utterances x S = K + 1 rows, U steps), the rows' labels and lengths and the
    hypothesis counts on the device.  strings = check_step's: per utterance at most K scored strings (slots behind them are fed the
    reference and ignored), or None = the hypothesis slots are drawn inside the Speller loop.  y int32 [n, >= dec_steps] on the
    device, tokenlen on the host."""
    a = las.args
    K, unit, norm = check_flags(a, las.dp)
    n = int(y.shape[0])
    m = Rows()
    m.K, m.S, m.n, m.unit, m.eos, m.sampling = K, K + 1, n, unit, eos_of(las.id_to_token), strings is None
    m.mode = MODES[norm or ("sample" if strings is None else "nbest")]
    S = m.S
    tl = np.asarray(torch.as_tensor(tokenlen).cpu()).astype(np.int32).reshape(-1)
    if strings is None:
        U = int(dec_steps) + int(getattr(a, "mwer_extra_steps", 4))
        host = np.zeros(n + n * S, np.int32)
        host[:n] = K
        host[n:].reshape(n, S)[:] = tl[:, None]
        block = None
    else:
        U = max([int(dec_steps)] + [len(s) for ss in strings for s in ss])
        host = np.zeros(n + n * S + n * K * U, np.int32)               # [nhyp | lens (n S) | the hypotheses' labels (n K U)]
        lens, block = host[n:n + n * S].reshape(n, S), host[n + n * S:].reshape(n, K, U)
        lens[:] = tl[:, None]
        for u, ss in enumerate(strings):
            host[u] = len(ss)
            for k, s in enumerate(ss):
                lens[u, k] = len(s)
                block[u, k, :len(s)] = s
    d = torch.from_numpy(host).pin_memory().to(dev, non_blocking=True)
    m.U, m.nhyp, m.lens = U, d[:n], d[n:n + n * S]
    w = min(int(y.shape[1]), int(dec_steps))
    ref = torch.zeros(n, U, dtype=torch.int32, device=dev)
    ref[:, :w] = y[:, :w]
    m.y_ref = ref                                                      # the reference's labels over U steps (PAD behind its end)
    rows = ref[:, None, :].repeat(1, S, 1)
    if block is not None:
        present = torch.arange(K, device=dev)[None, :] < m.nhyp[:, None]
        rows[:, :K] = torch.where(present[:, :, None], d[n + n * S:].view(n, K, U), rows[:, :K])
    m.y = rows.view(n * S, U)
    return m


def prepare_speller(m, speller, enc_len, dev):
    """the Speller's `prepared` dict for the n S rows: teacher forcing along every row's labels (the reference in slot K and in unused
    slots, the hypotheses in theirs), per-row dropout masks and variational noise as in any train step; drawn hypotheses: the token
    entering steps 1 .. of their slots is -2 (the loop's own Gumbel arg-max draw, written back) and the loop projects at every step"""
    rows_len = torch.as_tensor(enc_len).to(torch.float64).reshape(-1).repeat_interleave(m.S)
    prep = speller.prepare(m.n * m.S, rows_len, m.U, dev, m.y, True, np.ones(m.U, bool), None)
    if m.sampling and m.U > 1:
        prep["tokens_in"][1:].view(m.U - 1, m.n, m.S)[:, :, :m.K] = -2
        prep["step_logits"] = 1
    return prep


def resolve_samples(m, tokens_in):
    """behind the Speller: the drawn rows' labels and lengths from the tokens the loop wrote back.  The token scored at step t is the one
    that enters step t + 1; the last step scores EOS (scored_string's rule: the likelihood that the transcript ends there).  len =
    through the first EOS.  Device arithmetic only."""
    if not m.sampling:
        return
    R, U, dev = m.n * m.S, m.U, tokens_in.device
    yh = torch.cat([tokens_in[1:], torch.full((1, R), m.eos, dtype=torch.int32, device=dev)], 0).t()
    before = ((yh == m.eos).cumsum(1) == 0)                           # the steps in front of the first EOS
    first = before.sum(1).to(torch.int32)
    yh = torch.where(before | (torch.arange(U, device=dev)[None, :] == first[:, None]), yh, torch.zeros_like(yh))
    hyp = (torch.arange(R, device=dev) % m.S) < m.K
    m.y = torch.where(hyp[:, None], yh, m.y).contiguous()
    m.lens = torch.where(hyp, first + 1, m.lens)


def row_errors(m, id_to_token, unit):
    """-> err float32 [n S] on the device: the hypothesis slots' distances to the reference, 0 in the reference's slot.  Token unit: the
    labels never leave the device; word unit: one read-back of the labels for the word mapping."""
    n, S, K, U = m.n, m.S, m.K, m.U
    dev = m.y.device
    order = torch.cat([torch.tensor([K]), torch.arange(K)]).to(dev)     # the reference first, as las_nbest_risk's slot 0
    y = m.y.view(n, S, U).index_select(1, order).contiguous()
    ln = (m.lens.view(n, S).index_select(1, order) - 1).clamp_(min=0).contiguous()   # (every string ends in its EOS: not counted)
    err = torch.zeros(n, S, device=dev)
    if m.unit == "token":
        dist = torch.zeros(n * S * S + n * S + n, dtype=torch.int32, device=dev)
        pk = dict(n=n, K=S, U=U, tok=y, len=ln, nhyp=(m.nhyp + 1).contiguous(), w=torch.zeros(n * S, device=dev))
        nbest._risk(pk, dist)
        err[:, :K] = dist[:n * S * S].view(n, S, S)[:, 0, 1:].to(torch.float32)
    else:
        host = torch.cat([y.reshape(-1), ln.reshape(-1), m.nhyp]).cpu().numpy()
        hy, hl, nh = host[:n * S * U].reshape(n, S, U), host[n * S * U:n * S * U + n * S].reshape(n, S), host[n * S * U + n * S:]
        lists = [[hy[u, k, :hl[u, k]].tolist() for k in range(1 + int(nh[u]))] for u in range(n)]
        symbols, _ = nbest.word_symbols(lists, id_to_token, unit)
        dist, Kp = _distances(symbols)
        err[:, :Kp - 1] = dist[:, 0, 1:].to(torch.float32)
    return err.view(n * S)
