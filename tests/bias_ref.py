"""CPU restatement of contextual biasing (las/bias.py, csrc/bias.hip) WITHOUT a trie: a brute-force walker over the phrase
list, and the biased beam search built on the oracle's beam_search.  numpy only.

The walker's state is the matched token string m (a tuple): always a proper or whole prefix of some phrase, or empty.
  base(m) = the length of the longest prefix of m (m included) that is a whole phrase, 0 if none
  pend(m) = fl32(beta) * fl32(len(m) - base(m))
On token v:
  1. m + (v,) is a prefix of some phrase:              t = m + (v,),  gain beta
  2. else m is not empty and (v,) starts some phrase:  t = (v,),      gain fl32(beta - pend(m))
  3. else:                                             t = (),        gain -pend(m); from the empty match nothing, and no add
  4. t is a whole phrase that no other phrase extends: t = ().  The bonus is kept.
All gains are float32; a gain of 0 is "no add" (x + 0 would turn a -0 into +0)."""
import numpy as np


def _is_prefix(phrases, m):
    n = len(m)
    return any(len(p) >= n and tuple(p[:n]) == m for p in phrases)


def _pend(phrases, beta, m):
    base = 0
    for k in range(1, len(m) + 1):
        if any(tuple(p) == m[:k] for p in phrases):
            base = k
    return np.float32(beta) * np.float32(len(m) - base)


def walk(phrases, beta, m, v):
    """one transition: (match m, token v) -> (new match, gain as float32; 0 = no add)"""
    beta = np.float32(beta)
    m = tuple(m)
    t = m + (v,)
    if _is_prefix(phrases, t):
        gain = beta
    elif m and _is_prefix(phrases, (v,)):
        t, gain = (v,), np.float32(beta - _pend(phrases, beta, m))
    else:
        t, gain = (), (np.float32(-_pend(phrases, beta, m)) if m else np.float32(0.0))
    if t and any(tuple(p) == t for p in phrases) and not any(len(p) > len(t) and tuple(p[:len(t)]) == t for p in phrases):
        t = ()
    return t, gain


def gains(phrases, beta, tokens):
    """the float32 gain of every token of `tokens` (no SOS), walked from the empty match"""
    m, out = (), []
    for v in tokens:
        m, g = walk(phrases, beta, m, int(v))
        out.append(g)
    return np.asarray(out, np.float32)


def match_after(phrases, beta, tokens):
    m = ()
    for v in tokens:
        m, _ = walk(phrases, beta, m, int(v))
    return m


def bonus(phrases, beta, tokens):
    """the total bonus of a token string (no SOS): the float64 sum of its float32 gains"""
    return float(np.sum(gains(phrases, beta, tokens).astype(np.float64)))


def row_gains(phrases, beta, m, V):
    """the gain of every candidate v in [0, V) of a hypothesis whose match is m: float32 [V]"""
    m = tuple(m)
    k = len(m)
    ext = sorted({int(p[k]) for p in phrases if len(p) > k and tuple(p[:k]) == m and 0 <= p[k] < V})
    starts = sorted({int(p[0]) for p in phrases if 0 <= p[0] < V})
    if not m:
        g = np.zeros(V, np.float32)
    else:
        pend = _pend(phrases, beta, m)
        g = np.full(V, -pend, np.float32)                           # rule 3
        g[starts] = np.float32(np.float32(beta) - pend)             # rule 2
    g[ext] = np.float32(beta)                                       # rule 1
    return g


def row_gains_by_walking(phrases, beta, m, V):
    """the same, one walk() per candidate (slow: the check of row_gains)"""
    return np.asarray([walk(phrases, beta, m, v)[1] for v in range(V)], np.float32)


def apply_row(scores_row, g):
    """scores + gains as the device adds them: one float32 add where the gain is not 0, the value untouched elsewhere"""
    out = np.array(scores_row, dtype=np.float32, copy=True)
    nz = g != 0
    out[nz] = (out[nz] + g[nz]).astype(np.float32)
    return out


def biased_beam_search(step_fn, init_state, n_frames, dec_step, beam_size, start_id, end_id, phrases, beta, lp=None, T=None, lam=0.0,
                       topn=64):
    """oracle.beam_search with the hotword bonus: the wrapped step_fn's state carries (decoder state, the match of the hypothesis'
    PARENT or None at the first step[, the parent's CTC state]); every row's match is advanced by the token that entered the step and
    the row's candidates score logit [joint CTC-attention score when lam > 0: ctc_prefix_ref.joint_scores] + gain, float32.  The
    search's top-`topn` cut then works on the biased score."""
    from oracle import las_oracle as O
    import ctc_prefix_ref as R
    phrases = [list(p) for p in phrases]

    def bstep(prev_ids, prev_al, states):
        logits, new, alphas = step_fn(prev_ids, prev_al, [st[0] for st in states])
        logits = np.array(logits, dtype=np.float32, copy=True)
        out = np.empty_like(logits)
        nxt = []
        for i, st in enumerate(states):
            first = st[1] is None
            m = () if first else walk(phrases, beta, st[1], int(prev_ids[i]))[0]
            row, h = logits[i], None
            if lam > 0:
                h = R.empty_state(lp, T) if first else R.advance(st[2], prev_ids[i], lp, T)
                row = R.joint_scores(row, h, end_id, lp, T, lam, topn)
            out[i] = apply_row(row, row_gains(phrases, beta, m, row.shape[0]))
            nxt.append((new[i], m, h))
        return out, nxt, alphas

    return O.beam_search(bstep, (init_state, None, None), n_frames, dec_step, beam_size, start_id, end_id, topn=topn)
