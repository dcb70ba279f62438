"""CPU restatement of n-gram LM shallow fusion (las/ngram.py, csrc/ngram.hip) WITHOUT a trie or node numbers: everything
is read from the `grams` dict {token tuple: (log10 p, log10 bow)} and a hypothesis' token history (SOS first).  numpy only.

  logp64       the textbook recursion in float64: log p(v | h) = logp(h, v) if stored, else bow(h) [0 if h is not stored] + log p(v | h[1:])
  row_gains32  the device's float32 operation order: over the contexts h of the history from the longest (order - 1 tokens) to the empty
               one, acc = 0; a stored (h, v) ends the descent with g = fl32(acc + wlp(h, v)); a stored h that does not hold v gives
               acc = fl32(acc + wbow(h)); a context that is not stored adds nothing.  wlp / wbow = fl32(w ln10 log10 x), computed in
               float64 and rounded once.  The score is fl32(score + g): two adds per token."""
import math

import numpy as np

LN10 = math.log(10.0)


def _context(history, order):
    h = tuple(int(t) for t in history)
    return h[len(h) - (order - 1):] if (order > 1 and len(h) >= order - 1) else (h if order > 1 else ())


def logp64(grams, history, v, order=None):
    """log10 p(v | history) in float64; the context is the last order - 1 tokens of the history (order: the longest stored n-gram's)"""
    if order is None:
        order = max(len(k) for k in grams)
    h = _context(history, order)
    total = 0.0
    while True:
        if h + (v,) in grams:
            return total + float(grams[h + (v,)][0])
        if not h:
            raise KeyError("token %d has no unigram" % v)
        if h in grams:
            total += float(grams[h][1])
        h = h[1:]


def scaled(w, x):
    """fl32(w ln10 x): the product in float64, one rounding"""
    return np.float32((np.float64(w) * np.float64(LN10)) * np.float64(x))


def state_of(grams, order, history):
    """the longest suffix of the history (at most order - 1 tokens) that is a stored n-gram of order < `order`: the hypothesis' state"""
    h = _context(history, order)
    while h and h not in grams:
        h = h[1:]
    return h


def row_gains32(grams, order, w, history, V):
    """float32 [V]: the gain of every candidate v of a hypothesis with this history, in the device's operation order"""
    ctx = _context(history, order)
    out = np.zeros(V, np.float32)
    for v in range(V):
        acc, h = np.float32(0.0), ctx
        while True:
            e = grams.get(h + (v,))
            if e is not None:
                out[v] = np.float32(acc + scaled(w, e[0]))
                break
            assert h, "token %d has no unigram" % v
            if h in grams:
                acc = np.float32(acc + scaled(w, grams[h][1]))
            h = h[1:]
    return out


def partial_sums64(grams, order, w, history, v):
    """the float64 partial sums of w ln10 x over the terms row_gains32 adds for candidate v (every term itself included)"""
    h, total, out = _context(history, order), 0.0, []
    c = w * LN10
    while True:
        e = grams.get(h + (v,))
        if e is not None:
            out += [c * e[0], total + c * e[0]]
            return out
        assert h, "token %d has no unigram" % v
        if h in grams:
            total += c * grams[h][1]
            out += [c * grams[h][1], total]
        h = h[1:]


def random_model(rng, V, order, fan=3):
    """a sparse, prefix-closed random model: dense unigrams; every higher-order n-gram extends a stored one, so its prefix is stored while
    its suffix usually is not (contexts whose suffixes are missing); for about a third of them the suffix n-gram is stored too where ITS
    prefix is (a token stored at two levels of one chain).  log10 p in [-3, -0.05], log10 bow in [-1, 0] or absent (0)."""
    lp = lambda: -float(rng.uniform(0.05, 3.0))
    bw = lambda k: (-float(rng.uniform(0.0, 1.0)) if (k < order and rng.rand() < 0.8) else 0.0)
    grams = {(v,): (lp(), bw(1)) for v in range(V)}
    level = list(grams)
    for k in range(2, order + 1):
        new = []
        for i in rng.permutation(len(level))[:max(2, min(len(level), 40) // 2)]:
            for v in rng.choice(V, size=min(V, fan), replace=False):
                key = level[i] + (int(v),)
                if key not in grams:
                    grams[key] = (lp(), bw(k))
                    new.append(key)
                suf = key[1:]
                if rng.rand() < 0.35 and len(suf) > 1 and suf not in grams and suf[:-1] in grams:
                    grams[suf] = (lp(), bw(k - 1))
        level = new
    return grams


def random_string(rng, grams, order, V, n, start):
    """token string of n tokens after `start` that follows stored n-grams more often than not (so that deep states are reached)"""
    by_ctx = {}
    for key in grams:
        by_ctx.setdefault(key[:-1], []).append(key[-1])
    s = [start]
    for _ in range(n):
        h = state_of(grams, order, s)
        kids = by_ctx.get(h, []) if h else []
        s.append(int(kids[rng.randint(len(kids))]) if (kids and rng.rand() < 0.65) else int(rng.randint(V)))
    return s


def apply_row(scores_row, g):
    """scores + gains as the device adds them: one float32 add per token"""
    return (np.asarray(scores_row, np.float32) + np.asarray(g, np.float32)).astype(np.float32)


def total64(grams, order, w, tokens):
    """sum of w ln10 logp64 over the tokens of a hypothesis (tokens[0] = SOS is the history's start and is not scored)"""
    tokens = [int(t) for t in tokens]
    return sum(w * LN10 * logp64(grams, tokens[:i], tokens[i], order) for i in range(1, len(tokens)))


def wrap_step(step_fn, grams, order, w):
    """step_fn whose logits carry the LM's gains.  The wrapped state is (inner state, the PARENT's history or None at the first step);
    a row's history is its parent's plus the token that entered the step (SOS at the first)."""
    cache = {}

    def nstep(prev_ids, prev_al, states):
        logits, new, alphas = step_fn(prev_ids, prev_al, [st[0] for st in states])
        logits = np.array(logits, dtype=np.float32, copy=True)
        nxt = []
        for i, st in enumerate(states):
            hist = (() if st[1] is None else st[1]) + (int(prev_ids[i]),)
            key = hist[-(order - 1):] if order > 1 else ()
            if key not in cache:
                cache[key] = row_gains32(grams, order, w, hist, logits.shape[1])
            logits[i] = apply_row(logits[i], cache[key])
            nxt.append((new[i], hist))
        return logits, nxt, alphas
    return nstep


def ngram_beam_search(step_fn, init_state, n_frames, dec_step, beam_size, start_id, end_id, grams, order, w, lp=None, T=None, lam=0.0,
                      phrases=None, beta=0.0, topn=64):
    """oracle.beam_search with the n-gram LM fused into the logits; with lam > 0 the joint CTC-attention search
    (ctc_prefix_ref.joint_beam_search), with phrases the biased one (bias_ref.biased_beam_search) on top -- the wrapped step function
    goes into each of them unchanged, so the CTC bank cut and the hotword bonus see LM-fused logits"""
    from oracle import las_oracle as O
    fn, init = wrap_step(step_fn, grams, order, w), (init_state, None)
    if phrases:
        import bias_ref as B
        return B.biased_beam_search(fn, init, n_frames, dec_step, beam_size, start_id, end_id, phrases, beta, lp, T, lam, topn)
    if lam > 0:
        import ctc_prefix_ref as R
        return R.joint_beam_search(fn, init, n_frames, dec_step, beam_size, start_id, end_id, lp, T, lam, topn)
    return O.beam_search(fn, init, n_frames, dec_step, beam_size, start_id, end_id, topn=topn)
