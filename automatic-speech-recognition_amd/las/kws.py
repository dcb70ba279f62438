"""las.kws -- keyword search (spoken-term detection) on the CTC head: where in a recording is a listed phrase said, and how
sure is the model?  The host side of las_kws_search (csrc/kws.hip, include/las_hip.h K10j).

--hotwords nudges a search towards a phrase list; this asks the head's posteriors directly, so a name the search got wrong is still
found.  A hit's score is the log-likelihood ratio of the phrase's best path against the frame-wise best path over the same frames:
<= 0, and 0.0 when the phrase is what the head's greedy path says there.  The reference has no counterpart."""
import collections
import math

import numpy as np

MAX_TOKENS = 32                          # the kernel's: one state per lane, S = 2 L - 1 <= 63
MAX_HITS = 8
MAX_PHRASES_PER_CALL = 65535
SERIES_BYTES = 256 << 20                 # budget of the optional end series ([n, P, T'] fp64 + int32) per call: phrases are chunked under it

KeywordResult = collections.namedtuple("KeywordResult", "hits best_score best_span count end_score end_start")
# hits[u]: [{"keyword": index, "start_frame", "end_frame", "score"}] sorted by start frame, then phrase index;  best_score f64 [n, P],
# best_span int32 [n, P, 2] (start, end), count int32 [n, P, 2] (kept, total closed);  end_score f64 / end_start int32 [n, P, T'] or None


class KeywordList(object):
    """phrases: non-empty lists of token ids (never SOS or PAD, below vocab_size); texts: what to print for them"""

    def __init__(self, phrases, texts=None, vocab_size=None, sos_id=1, pad_id=0):
        phrases = list(phrases)
        if not phrases:
            raise ValueError("KeywordList: no phrases")
        if texts is not None and len(texts) != len(phrases):
            raise ValueError("KeywordList: %d phrases, %d texts" % (len(phrases), len(texts)))
        self.vocab_size = None if vocab_size is None else int(vocab_size)
        self.phrases = []
        for k, ph in enumerate(phrases):
            name = "phrase %d %r" % (k, list(ph) if not isinstance(ph, str) else ph)
            if isinstance(ph, str):
                raise ValueError("KeywordList: %s is text; phrases are lists of token ids (KeywordList.from_file encodes text)" % name)
            ph = list(ph)
            if len(ph) == 0:
                raise ValueError("KeywordList: %s is empty" % name)
            if len(ph) > MAX_TOKENS:
                raise ValueError("KeywordList: %s has %d tokens; at most %d" % (name, len(ph), MAX_TOKENS))
            for t in ph:
                if int(t) != t:
                    raise ValueError("KeywordList: %s holds %r, not a token id" % (name, t))
                if int(t) < 0 or (self.vocab_size is not None and int(t) >= self.vocab_size):
                    raise ValueError("KeywordList: %s holds token %d outside [0, %s)" % (name, int(t), self.vocab_size))
                if int(t) in (sos_id, pad_id):
                    raise ValueError("KeywordList: %s holds <SOS> / <PAD> (token %d)" % (name, int(t)))
            self.phrases.append([int(t) for t in ph])
        self.texts = [str(t) for t in texts] if texts is not None else [" ".join(str(t) for t in ph) for ph in self.phrases]

    def __len__(self):
        return len(self.phrases)

    @classmethod
    def from_file(cls, path, tokenizer, vocab_size):
        """one phrase per line; blank lines and lines starting with '#' are skipped; a line is upper-cased like the transcripts, its
        whitespace collapsed, and encoded with tokenizer.encode(line, with_eos=False) (the line rules of ContextGraph.from_file)"""
        import os
        if not path or not os.path.isfile(path):
            raise ValueError("keywords: no such file %r" % (path,))
        phrases, texts = [], []
        with open(path, encoding="utf-8") as f:
            for ln, line in enumerate(f, 1):
                text = line.strip()
                if not text or text.startswith("#"):
                    continue
                text = " ".join(text.upper().split())
                try:
                    ids = list(tokenizer.encode(text, with_eos=False))
                except KeyError as e:       # the char unit: a character outside its 30 symbols
                    raise ValueError("keywords %s, line %d: character %s is not in the vocabulary (%r)" % (path, ln, e, text))
                if not ids:
                    raise ValueError("keywords %s, line %d: %r encodes to no token" % (path, ln, text))
                try:
                    cls([ids], [text], vocab_size)
                except ValueError as e:
                    raise ValueError("keywords %s, line %d (%r): %s" % (path, ln, text, e))
                phrases.append(ids)
                texts.append(text)
        if not phrases:
            raise ValueError("keywords %s holds no phrase" % path)
        return cls(phrases, texts, vocab_size)


def keyword_search(lp, enc_lens, keywords, threshold_per_token, max_hits=4, series=False, series_bytes=SERIES_BYTES):
    """Search every phrase of `keywords` in every utterance.  lp: the device's class-major log-probabilities [n, V + 1, T'] (fp32,
    BeamSearch._ctc_log_probs); enc_lens [n]: frames per utterance; thr[p] = threshold_per_token x L_p (nats; a hit needs score >= thr).
    -> KeywordResult.  Per call: one upload (lengths, tokens and thresholds in one buffer), one las_kws_search, one read-back; one call
    unless the phrases are chunked -- at most 65535 a call, and with `series` as many as keep the series under `series_bytes`."""
    import torch
    from las import _hip
    _hip.require_gpu(lp)
    if lp.dim() != 3 or lp.dtype != torch.float32 or not lp.is_contiguous():
        raise ValueError("keyword_search: lp must be a contiguous fp32 [n, V + 1, T'] tensor")
    n, Vc, Tp = lp.shape
    if len(enc_lens) != n:
        raise ValueError("keyword_search: %d utterances, %d lengths" % (n, len(enc_lens)))
    H = int(max_hits)
    if not 1 <= H <= MAX_HITS:
        raise ValueError("keyword_search: max_hits must be in [1, %d] (got %r)" % (MAX_HITS, max_hits))
    tpt = float(threshold_per_token)
    if math.isnan(tpt):
        raise ValueError("keyword_search: the threshold is not a number")
    phrases = keywords.phrases
    for k, ph in enumerate(phrases):
        if max(ph) > Vc - 2:
            raise ValueError("keyword_search: phrase %d %r holds token %d, the head has classes 0 .. %d and the blank" % (k, ph, max(ph), Vc - 2))
    P = len(phrases)
    chunk = MAX_PHRASES_PER_CALL
    if series:
        chunk = min(chunk, max(1, int(series_bytes) // (n * Tp * 12)))
    parts = [_search_chunk(lp, enc_lens, phrases[p0:p0 + chunk], tpt, H, series) for p0 in range(0, P, chunk)]
    cat = lambda i: np.concatenate([q[i] for q in parts], axis=1)
    hs, he, hsc, cnt, bsc, bsp = (cat(i) for i in range(6))
    es, et = (cat(6), cat(7)) if series else (None, None)
    hits = []
    for u in range(n):
        found = [{"keyword": p, "start_frame": int(hs[u, p, k]), "end_frame": int(he[u, p, k]), "score": float(hsc[u, p, k])}
                 for p in range(P) for k in range(int(cnt[u, p, 0]))]
        found.sort(key=lambda h: (h["start_frame"], h["keyword"]))
        hits.append(found)
    return KeywordResult(hits, bsc, bsp, cnt, es, et)


def _search_chunk(lp, enc_lens, phrases, tpt, H, series):
    """one las_kws_search call -> numpy (hit_start, hit_end, hit_score [n, P, H], count [n, P, 2], best_score [n, P], best_span [n, P, 2],
    end_score, end_start [n, P, T'] or None)"""
    import torch
    from las import _hip
    n, Vc, Tp = lp.shape
    dev = lp.device
    P = len(phrases)
    U = max(len(ph) for ph in phrases)
    host = np.zeros(n + 2 * P + P * U, np.int32)              # [enc_len (n) | y_len (P) | thr (P, fp32 bits) | y (P, U)]
    host[:n] = [int(x) for x in enc_lens]
    host[n:n + P] = [len(ph) for ph in phrases]
    host[n + P:n + 2 * P].view(np.float32)[:] = [np.float32(tpt) * np.float32(len(ph)) for ph in phrases]
    y = host[n + 2 * P:].reshape(P, U)
    for k, ph in enumerate(phrases):
        y[k, :len(ph)] = ph
    meta = torch.from_numpy(host).to(dev)
    # one output buffer, the fp64 sections first: [hit_score | best_score | end_score] [hit_start | hit_end | count | best_span | end_start]
    n64 = n * P * H + n * P + (n * P * Tp if series else 0)
    n32 = 2 * n * P * H + 4 * n * P + (n * P * Tp if series else 0)
    out = torch.empty(8 * n64 + 4 * n32, dtype=torch.uint8, device=dev)
    base = out.data_ptr()
    o64 = [0, n * P * H, n * P * H + n * P]
    o32 = [0, n * P * H, 2 * n * P * H, 2 * n * P * H + 2 * n * P, 2 * n * P * H + 4 * n * P]
    p64 = lambda i: _hip.c_void_p(base + 8 * o64[i])
    p32 = lambda i: _hip.c_void_p(base + 8 * n64 + 4 * o32[i])
    lib = _hip.lib()
    ws = _hip.workspace(dev, lib.las_kws_workspace_bytes(n, Tp), "kws")
    _hip.check(lib.las_kws_search(_hip.p(lp), Vc, Tp, _hip.p(meta[:n]), n, _hip.p(meta[n + 2 * P:]), U, _hip.p(meta[n:n + P]),
                                  _hip.p(meta[n + P:n + 2 * P]), P, U, H, p32(0), p32(1), p64(0), p32(2), p64(1), p32(3),
                                  p64(2) if series else None, p32(4) if series else None, _hip.p(ws), ws.numel(), _hip.stream()),
               "las_kws_search")
    raw = out.cpu().numpy()
    f64, i32 = raw[:8 * n64].view(np.float64), raw[8 * n64:].view(np.int32)
    return (i32[o32[0]:o32[1]].reshape(n, P, H), i32[o32[1]:o32[2]].reshape(n, P, H), f64[o64[0]:o64[1]].reshape(n, P, H),
            i32[o32[2]:o32[3]].reshape(n, P, 2), f64[o64[1]:o64[2]].reshape(n, P), i32[o32[3]:o32[4]].reshape(n, P, 2),
            f64[o64[2]:].reshape(n, P, Tp) if series else None, i32[o32[4]:].reshape(n, P, Tp) if series else None)


def timed_hits(hits, keywords, frame_s, duration_s):
    """one utterance's hits as transcribe.py prints them: [{"keyword": text, "start", "end", "score", "confidence"}], in the given order.
    start = start_frame x frame_s, end = min((end_frame + 1) x frame_s, duration_s), confidence = exp(score / L)"""
    out = []
    for h in hits:
        L = len(keywords.phrases[h["keyword"]])
        out.append({"keyword": keywords.texts[h["keyword"]], "start": h["start_frame"] * frame_s,
                    "end": min((h["end_frame"] + 1) * frame_s, duration_s), "score": h["score"], "confidence": math.exp(h["score"] / L)})
    return out
