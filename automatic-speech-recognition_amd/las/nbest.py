"""las.nbest -- what the N-best list of a search says beyond its first entry: posteriors over the hypotheses, the
minimum-Bayes-risk hypothesis under the token edit distance, and token / word confidences (las_nbest_risk, las_nbest_confidence,
csrc/nbest.hip).  The posteriors are host arithmetic on <= beam_size scores per utterance; everything quadratic in the list -- the
pairwise distances and the alignments to the pivot -- runs on the device.  The reference has no counterpart."""
import numpy as np
import torch

from las import _hip


def hypotheses(results, eos_id):
    """BeamSearch results (per utterance the ranked BeamStates, best LAST) -> (token_lists, scores, lens), per utterance and best
    FIRST: token_lists[u][k] = token_ids[1:] cut at the first EOS (what convert_idx_to_string prints), scores[u][k] = log_prob,
    lens[u][k] = len(token_ids) - 1, the length the search's length normalisation divides by."""
    token_lists, scores, lens = [], [], []
    for r in results:
        tl, sc, ln = [], [], []
        for b in reversed(r):
            ids = [int(t) for t in b.token_ids[1:]]
            ln.append(len(ids))
            if eos_id in ids:
                ids = ids[:ids.index(eos_id)]
            tl.append(ids)
            sc.append(float(b.log_prob))
        token_lists.append(tl)
        scores.append(sc)
        lens.append(ln)
    return token_lists, scores, lens


def posteriors(scores, lens, scale=1.0):
    """softmax over one utterance's hypotheses of scale * key, key = the search's own final ranking key (BeamSearch._decode_tail:
    score / length while beam_search.NORM holds, else the score), so the top posterior is the search's 1-best.  float64 numpy, rounded
    to fp32 once.  Non-finite keys weigh 0; if every key is non-finite the weights are uniform."""
    from las import beam_search
    sc = np.asarray(scores, np.float64)
    if sc.size == 0:
        return np.zeros(0, np.float32)
    with np.errstate(all="ignore"):
        key = sc / np.maximum(np.asarray(lens, np.float64), 1.0) if beam_search.NORM else sc
        ok = np.isfinite(key)
        if not ok.any():
            return np.full(sc.size, 1.0 / sc.size).astype(np.float32)
        z = np.where(ok, float(scale) * key, -np.inf)
        e = np.where(ok, np.exp(z - z[ok].max()), 0.0)
    return (e / e.sum()).astype(np.float32)


def _pack(token_lists, weights, pivot=None):
    """one host buffer [len (n K) | nhyp (n) | pivot (n) | w (n K, fp32 bits) | tok (n K U)] -> its device copy and the views"""
    n = len(token_lists)
    if n == 0 or len(weights) != n:
        raise ValueError("nbest: %d utterances, %d weight rows" % (n, len(weights)))
    K = max(1, max(len(t) for t in token_lists))
    U = max(1, max((len(h) for t in token_lists for h in t), default=1))
    host = np.zeros(n * K + 2 * n + n * K + n * K * U, np.int32)
    o_nh, o_pv, o_w, o_tok = n * K, n * K + n, n * K + 2 * n, 2 * n * K + 2 * n
    ln = host[:o_nh].reshape(n, K)
    w = host[o_w:o_tok].view(np.float32).reshape(n, K)
    tok = host[o_tok:].reshape(n, K, U)
    host[o_pv:o_w] = -1 if pivot is None else np.asarray(pivot, np.int32)
    for u, (hyps, wu) in enumerate(zip(token_lists, weights)):
        if len(wu) != len(hyps):
            raise ValueError("nbest: utterance %d has %d hypotheses and %d weights" % (u, len(hyps), len(wu)))
        host[o_nh + u] = len(hyps)
        w[u, :len(hyps)] = np.asarray(wu, np.float32)
        for k, h in enumerate(hyps):
            ln[u, k] = len(h)
            tok[u, k, :len(h)] = np.asarray(h, np.int64)
    dev = torch.device("cuda", torch.cuda.current_device())
    d = torch.from_numpy(host).to(dev)
    return dict(n=n, K=K, U=U, dev=dev, len=d[:o_nh], nhyp=d[o_nh:o_pv], pivot=d[o_pv:o_w], w=d[o_w:o_tok], tok=d[o_tok:])


def _risk(m, out):
    """las_nbest_risk into out [n K K dist | n K risk bits | n pick] (int32 on the device)"""
    n, K = m["n"], m["K"]
    dist, risk, pick = out[:n * K * K], out[n * K * K:n * K * K + n * K], out[n * K * K + n * K:n * K * K + n * K + n]
    _hip.check(_hip.lib().las_nbest_risk(_hip.p(m["tok"]), _hip.p(m["len"]), _hip.p(m["nhyp"]), _hip.p(m["w"]), n, K, m["U"], _hip.p(dist),
                                         _hip.p(risk), _hip.p(pick), _hip.stream()), "las_nbest_risk")
    return pick


def _confidence(m, pivot, conf, match):
    n, K, U = m["n"], m["K"], m["U"]
    lib = _hip.lib()
    nbytes = lib.las_nbest_workspace_bytes(n, K, U)
    ws = _hip.workspace(m["dev"], nbytes, "nbest")
    _hip.check(lib.las_nbest_confidence(_hip.p(m["tok"]), _hip.p(m["len"]), _hip.p(m["nhyp"]), _hip.p(m["w"]), _hip.p(pivot), n, K, U,
                                        _hip.p(match), _hip.p(conf), _hip.p(ws), nbytes, _hip.stream()), "las_nbest_confidence")


def _unpack_risk(m, host, token_lists):
    n, K = m["n"], m["K"]
    dist = host[:n * K * K].reshape(n, K, K)
    risk = host[n * K * K:n * K * K + n * K].view(np.float32).reshape(n, K)
    pick = host[n * K * K + n * K:n * K * K + n * K + n]
    nh = [len(t) for t in token_lists]
    return [dist[u, :nh[u], :nh[u]].copy() for u in range(n)], [risk[u, :nh[u]].copy() for u in range(n)], [int(x) for x in pick]


def _unpack_conf(m, conf, match, token_lists, pivot):
    n = m["n"]
    confs, matches = [], []
    for u in range(n):
        pv, nh = int(pivot[u]), len(token_lists[u])
        if pv < 0 or pv >= nh:
            confs.append(None)
            matches.append(None)
            continue
        La = len(token_lists[u][pv])
        confs.append(conf[u, :La].copy())
        matches.append(match[u, :nh, :La].copy())
    return confs, matches


def consensus(token_lists, weights):
    """token_lists[u] = the hypotheses (token id lists) of utterance u, weights[u] their posteriors -> (dist, risk, pick): per
    utterance the [nh, nh] int32 token edit distances, the [nh] fp32 expected distance of every hypothesis to the list, and the index
    of least risk (-1 for an empty list).  One upload, one call, one read-back."""
    m = _pack(token_lists, weights)
    n, K = m["n"], m["K"]
    out = torch.zeros(n * K * K + n * K + n, dtype=torch.int32, device=m["dev"])
    _risk(m, out)
    return _unpack_risk(m, out.cpu().numpy(), token_lists)


def token_confidence(token_lists, weights, pivot):
    """-> (conf, match): conf[u] [len of the pivot] fp32 = the posterior mass of the hypotheses whose alignment to hypothesis pivot[u]
    matches that token, match[u] [nh, len] int8 the matches themselves; None, None where pivot[u] is -1.  One upload, one call, one
    read-back."""
    m = _pack(token_lists, weights, pivot)
    n, K, U = m["n"], m["K"], m["U"]
    conf = torch.zeros(n, U, device=m["dev"])
    match = torch.zeros(n, K, U, dtype=torch.int8, device=m["dev"])
    _confidence(m, m["pivot"], conf, match)
    return _unpack_conf(m, conf.cpu().numpy(), match.cpu().numpy(), token_lists, pivot)


def consensus_confidence(token_lists, weights):
    """consensus() and token_confidence() about its pick, back to back: pick never leaves the device between the two calls.
    -> (dist, risk, pick, conf, match)"""
    m = _pack(token_lists, weights)
    n, K, U = m["n"], m["K"], m["U"]
    out = torch.zeros(n * K * K + n * K + n + n * U, dtype=torch.int32, device=m["dev"])
    match = torch.zeros(n, K, U, dtype=torch.int8, device=m["dev"])
    pick = _risk(m, out)
    conf = out[n * K * K + n * K + n:].view(torch.float32).view(n, U)
    _confidence(m, pick, conf, match)
    host = out.cpu().numpy()
    dist, risk, picks = _unpack_risk(m, host, token_lists)
    confs, matches = _unpack_conf(m, host[n * K * K + n * K + n:].view(np.float32).reshape(n, U), match.cpu().numpy(), token_lists, picks)
    return dist, risk, picks, confs, matches


def word_confidence(tokens, conf, id_to_token, unit):
    """[{"word", "confidence"}] of one hypothesis: exactly the words las.align.words makes of the same tokens (char: split at <SPACE>;
    subword: a word ends at a token ending in </w>; <EOS> and everything behind it make no word), a word's confidence = the MINIMUM
    over its tokens' (a word is as sure as its least sure piece); <SPACE> contributes to no word."""
    out, text, lo = [], "", None

    def flush():
        nonlocal text, lo
        if text:
            out.append({"word": text, "confidence": lo})
        text, lo = "", None

    for tok, c in zip(tokens, conf):
        piece = id_to_token[int(tok)]
        if piece == "<EOS>":
            break
        ends = False
        if unit == "char":
            if piece == "<SPACE>":
                flush()
                continue
        elif unit == "subword" and piece.endswith("</w>"):
            piece, ends = piece[:-len("</w>")], True
        if piece.strip():
            text += piece.strip() if unit == "subword" else piece
            lo = float(c) if lo is None else min(lo, float(c))
        if ends:
            flush()
    flush()
    return out


class Annotator(object):
    """what transcribe.py / decode.py do with a batch of results under --nbest / --confidence / --mbr"""

    def __init__(self, args, eos_id):
        self.nbest, self.confidence, self.mbr = int(args.nbest), bool(args.confidence), bool(args.mbr)
        self.scale, self.eos_id = float(args.nbest_scale), eos_id
        if self.nbest < 0 or self.nbest > int(args.beam_size):
            raise ValueError("--nbest %d: between 0 and --beam_size %d" % (self.nbest, int(args.beam_size)))
        self.active = bool(self.nbest or self.confidence or self.mbr)

    def annotate(self, results):
        """-> per utterance a dict: index (into the best-first list; -1: the search returned nothing), state (the BeamState to print),
        tokens (cut at EOS), posterior, conf (per token, with --confidence), nbest [(tokens, score, posterior)]"""
        token_lists, scores, lens = hypotheses(results, self.eos_id)
        weights = [posteriors(s, l, self.scale) for s, l in zip(scores, lens)]
        n = len(results)
        picks, confs = [0 if t else -1 for t in token_lists], [None] * n
        if n and self.mbr and self.confidence:
            _, _, picks, confs, _ = consensus_confidence(token_lists, weights)
        elif n and self.mbr:
            _, _, picks = consensus(token_lists, weights)
        elif n and self.confidence:
            confs, _ = token_confidence(token_lists, weights, picks)
        out = []
        for u, r in enumerate(results):
            k = picks[u]
            if k < 0:
                out.append(dict(index=-1, state=None, tokens=[], posterior=None, conf=[], nbest=[]))
                continue
            out.append(dict(index=k, state=r[len(r) - 1 - k], tokens=token_lists[u][k], posterior=float(weights[u][k]),
                            conf=confs[u] if confs[u] is not None else [],
                            nbest=[(token_lists[u][j], scores[u][j], float(weights[u][j])) for j in range(min(self.nbest, len(r)))]))
        return out
