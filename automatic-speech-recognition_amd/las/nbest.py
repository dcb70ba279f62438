"""las.nbest -- what the N-best list of a search says beyond its first entry: posteriors over the hypotheses, the
minimum-Bayes-risk hypothesis under the token edit distance, and token / word confidences (las_nbest_risk, las_nbest_confidence,
csrc/nbest.hip).  The posteriors are host arithmetic on <= beam_size scores per utterance; everything quadratic in the list -- the
pairwise distances and the alignments to the pivot -- runs on the device.  DESIGN 7q adds the list's confusion network
(las_nbest_network): word symbols, the multi-alignment and the per-bin masses on the device, the bins' alternatives and the consensus
on the host.  The reference has no counterpart."""
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


EPS = -1                                                               # include/las_hip.h K10h: "no word here"
MAX_BINS = 2048


def _word_pieces(tokens, id_to_token, unit):
    """[(text, token tuple)] of one hypothesis: word_confidence's loop (so las.align.words' words), with the tokens that spell the word"""
    out, text, ids = [], "", []

    def flush():
        nonlocal text, ids
        if text:
            out.append((text, tuple(ids)))
        text, ids = "", []

    for tok in tokens:
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
            ids.append(int(tok))
        elif ends and text:
            ids.append(int(tok))                                       # (a bare </w>: it still ends the spelling)
        if ends:
            flush()
    flush()
    return out


def word_symbols(token_lists, id_to_token, unit):
    """token_lists[u][k] = token ids -> (symbol_lists, words): every hypothesis split into exactly the words las.align.words /
    word_confidence make of the same tokens, a word's identity its printed text (two segmentations of one word are one symbol); ids are
    given per utterance in order of first appearance, best hypothesis first; words[u][id] = (text, the token tuple of its first
    appearance).  unit "token": the identity mapping, words[u][id] = (the token's piece, (id,))."""
    symbol_lists, words = [], []
    for hyps in token_lists:
        if unit == "token":
            symbol_lists.append([[int(t) for t in h] for h in hyps])
            words.append({int(t): (id_to_token[int(t)], (int(t),)) for h in hyps for t in h})
            continue
        ids, table, sl = {}, [], []
        for h in hyps:
            row = []
            for text, toks in _word_pieces(h, id_to_token, unit):
                if text not in ids:
                    ids[text] = len(table)
                    table.append((text, toks))
                row.append(ids[text])
            sl.append(row)
        symbol_lists.append(sl)
        words.append(table)
    return symbol_lists, words


def network(symbol_lists, weights, max_bins=None):
    """the confusion network of every utterance (las_nbest_network): symbol_lists[u] = the hypotheses (symbol id lists, best
    first), weights[u] their posteriors -> per utterance dict(cols [nh, B] int32 the multi-alignment matrix (EPS = -1; rows of
    hypotheses that were not merged hold EPS), merged [nh] int8, best [B] int32, post [B] fp32).  max_bins None: min(2048, the largest
    sum of lengths of an utterance), so nothing overflows below the ceiling.  One upload, one call, one read-back."""
    m = _pack(symbol_lists, weights)
    n, K, U = m["n"], m["K"], m["U"]
    if max_bins is None:
        max_bins = min(MAX_BINS, max(1, max(sum(len(h) for h in t) for t in symbol_lists)))
    mb = int(max_bins)
    o_nb, o_best, o_post, o_mg = n * K * mb, n * K * mb + n, n * K * mb + n + n * mb, n * K * mb + n + 2 * n * mb
    out = torch.zeros(o_mg + (n * K + 3) // 4, dtype=torch.int32, device=m["dev"])
    lib = _hip.lib()
    nbytes = lib.las_nbest_network_workspace_bytes(n, K, U, mb)
    ws = _hip.workspace(m["dev"], nbytes, "nbest_network")
    _hip.check(lib.las_nbest_network(_hip.p(m["tok"]), _hip.p(m["len"]), _hip.p(m["nhyp"]), _hip.p(m["w"]), n, K, U, mb, _hip.p(out[:o_nb]),
                                     _hip.p(out[o_nb:o_best]), _hip.p(out[o_mg:]), _hip.p(out[o_best:o_post]), _hip.p(out[o_post:o_mg]),
                                     _hip.p(ws), nbytes, _hip.stream()), "las_nbest_network")
    host = out.cpu().numpy()
    cols, nbins = host[:o_nb].reshape(n, K, mb), host[o_nb:o_best]
    best, post = host[o_best:o_post].reshape(n, mb), host[o_post:o_mg].view(np.float32).reshape(n, mb)
    merged = host[o_mg:].view(np.int8)[:n * K].reshape(n, K)
    nets = []
    for u, hyps in enumerate(symbol_lists):
        nh, B = len(hyps), int(nbins[u])
        mg = merged[u, :nh].copy()
        c = cols[u, :nh, :B].copy()
        c[mg == 0] = EPS
        nets.append(dict(cols=c, merged=mg, best=best[u, :B].copy(), post=post[u, :B].copy()))
    return nets


def bins(net, weights, words, top):
    """one utterance's network -> per bin the `top` alternatives [{"word", "p"}] by mass, largest first, on equal mass the symbol whose
    first contributing hypothesis ranks higher (the first one is the kernel's best / post: the same fp32 sums in the same order); EPS
    is the word "".  words = word_symbols' table of the utterance."""
    cols, merged = net["cols"], net["merged"]
    w = np.asarray(weights, np.float32)
    out = []
    for i in range(cols.shape[1]):
        mass = {}
        for k in range(cols.shape[0]):
            if merged[k]:
                s = int(cols[k, i])
                mass[s] = np.float32(mass.get(s, np.float32(0)) + w[k])
        ranked = sorted(mass.items(), key=lambda e: -e[1])             # (stable: the dict holds the symbols by first contributing slot)
        out.append([{"word": "" if s == EPS else words[s][0], "p": float(p)} for s, p in ranked[:int(top)]])
    return out


class Annotator(object):
    """what transcribe.py / decode.py do with a batch of results under --nbest / --confidence / --mbr / --confusion_network / --cn_decode"""

    def __init__(self, args, eos_id, id_to_token=None):
        self.nbest, self.confidence, self.mbr = int(args.nbest), bool(args.confidence), bool(args.mbr)
        self.scale, self.eos_id = float(args.nbest_scale), eos_id
        if self.nbest < 0 or self.nbest > int(args.beam_size):
            raise ValueError("--nbest %d: between 0 and --beam_size %d" % (self.nbest, int(args.beam_size)))
        # (a namespace from before these flags has none of them: everything off)
        self.cn, self.cn_decode = bool(getattr(args, "confusion_network", False)), bool(getattr(args, "cn_decode", False))
        self.cn_top, self.cn_unit = int(getattr(args, "cn_alternatives", 3)), str(getattr(args, "cn_unit", "word"))
        self.id_to_token, self.unit = id_to_token, str(getattr(args, "unit", "char")).lower()
        if self.cn or self.cn_decode:
            from las.arguments import check_confusion_flags
            check_confusion_flags(args)
            if id_to_token is None:
                raise ValueError("--confusion_network / --cn_decode: the Annotator needs the tokenizer's id_to_token")
        self.active = bool(self.nbest or self.confidence or self.mbr or self.cn or self.cn_decode)

    def _networks(self, token_lists, weights, out):
        """--confusion_network / --cn_decode: one las_nbest_network call for the batch; adds network (the bins) and, under --cn_decode,
        consensus = dict(words, conf, tokens, text) to every utterance's dict"""
        from las.utils import convert_idx_to_string
        unit = self.unit if self.cn_unit == "word" else "token"
        symbol_lists, words = word_symbols(token_lists, self.id_to_token, unit)
        nets = network(symbol_lists, weights) if token_lists else []
        space = [i for i in range(len(self.id_to_token)) if self.id_to_token[i] == "<SPACE>"] if unit == "char" else []
        for u, (net, d) in enumerate(zip(nets, out)):
            d["network"] = bins(net, weights[u], words[u], self.cn_top)
            if not self.cn_decode:
                continue
            keep = [i for i in range(len(net["best"])) if net["best"][i] != EPS]
            texts = [words[u][int(net["best"][i])][0] for i in keep]
            tokens = []
            for j, i in enumerate(keep):
                if j and space:
                    tokens.append(space[0])
                tokens.extend(words[u][int(net["best"][i])][1])
            text = convert_idx_to_string(tokens, self.id_to_token, self.unit) if unit == "token" else " ".join(texts)
            d["consensus"] = dict(words=texts, conf=[float(net["post"][i]) for i in keep], tokens=tokens, text=text)

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
        elif n and self.confidence and not self.cn_decode:             # (under --cn_decode the words' confidences are the bin masses)
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
        if n and (self.cn or self.cn_decode):
            self._networks(token_lists, weights, out)
        return out
