"""CPU restatement of the CTC prefix scorer of joint CTC-attention beam search (the equations of ESPnet's CTCPrefixScore,
Watanabe et al. 2017 Algorithm 2, with EOS scored as an ordinary final label) and of the joint search built on the oracle's
beam_search.  numpy, float64 by default.  lp: log-probabilities [T', V + 1] of one utterance (time-major here), blank = class V."""
import numpy as np

LOGZERO = -1e10


class State(object):
    """CTC state of a hypothesis h: r^n_t(h), r^b_t(h) for t < T, psi(h), last label (-1: the empty prefix)."""

    def __init__(self, rn, rb, psi, last):
        self.rn, self.rb, self.psi, self.last = rn, rb, psi, last


def empty_state(lp, T, dtype=np.float64):
    lp = np.asarray(lp, dtype)
    blank = lp.shape[1] - 1
    return State(np.full(T, LOGZERO, dtype), np.cumsum(lp[:T, blank]), dtype(0.0), -1)


def _phi(s, c):
    return s.rb if c == s.last else np.logaddexp(s.rb, s.rn)


def psi(s, c, lp, T):
    """prefix score psi(h.c) of a candidate c != EOS"""
    lp = np.asarray(lp, s.rb.dtype)
    start = lp[0, c] if s.last < 0 else LOGZERO
    terms = _phi(s, c)[:T - 1] + lp[1:T, c]
    return np.logaddexp.reduce(np.concatenate([[start], terms]).astype(s.rb.dtype))


def advance(s, c, lp, T):
    """the state of h.c"""
    lp = np.asarray(lp, s.rb.dtype)
    blank = lp.shape[1] - 1
    phi = _phi(s, c)
    rn = np.empty(T, s.rb.dtype)
    rb = np.empty(T, s.rb.dtype)
    rn[0] = lp[0, c] if s.last < 0 else LOGZERO
    rb[0] = LOGZERO
    for t in range(1, T):
        rn[t] = np.logaddexp(rn[t - 1], phi[t - 1]) + lp[t, c]
        rb[t] = np.logaddexp(rb[t - 1], rn[t - 1]) + lp[t, blank]
    return State(rn, rb, psi(s, c, lp, T), c)


def eos_score(s, eos, lp, T):
    """the EOS candidate: the full-sequence log-probability of h.EOS"""
    e = advance(s, eos, lp, T)
    return np.logaddexp(e.rn[T - 1], e.rb[T - 1])


def prefix_score(s, c, eos, lp, T):
    return eos_score(s, eos, lp, T) if c == eos else psi(s, c, lp, T)


def candidate_bank(logits, topn=64):
    """the top-`topn` tokens of one row by (logit, token id)"""
    logits = np.asarray(logits)
    if logits.shape[0] <= topn:
        return np.arange(logits.shape[0])
    return np.lexsort((np.arange(logits.shape[0]), logits))[-topn:]


def joint_scores(logits_row, s, eos, lp, T, lam, topn=64):
    """logit + lam * (psi(h.c) - psi(h)) in float32 for the row's candidates, -inf for every other token"""
    out = np.full(logits_row.shape, -np.inf, np.float32)
    for c in candidate_bank(logits_row, topn):
        d = np.float32(prefix_score(s, int(c), eos, lp, T) - s.psi)
        out[c] = np.float32(np.float32(logits_row[c]) + np.float32(np.float32(lam) * d))
    return out


def joint_beam_search(step_fn, init_state, n_frames, dec_step, beam_size, start_id, end_id, lp, T, lam, topn=64,
                      lm_fn=None, lm_init=None, lm_weight=0.0):
    """oracle.beam_search with the CTC prefix scores: the wrapped step_fn's state carries (decoder state, the parent's CTC state, LM
    state); every row's CTC state is advanced by the token that entered the step (prev_ids[i]; the empty prefix at the first step)
    and the row's candidates score logit [+ lm_weight x LM logit] + lam x (psi(h.c) - psi(h))."""
    from oracle import las_oracle as O

    def jstep(prev_ids, prev_al, states):
        logits, new, alphas = step_fn(prev_ids, prev_al, [st[0] for st in states])
        logits = np.array(logits, dtype=np.float32, copy=True)
        lm_states = None
        if lm_fn is not None:
            lm_out, lm_states = lm_fn([max(i - 2, 0) for i in prev_ids], [st[2] for st in states])
            logits[:, 2:] += np.asarray(lm_out, np.float32) * np.float32(lm_weight)
        out = np.empty_like(logits)
        nxt = []
        for i, st in enumerate(states):
            h = empty_state(lp, T) if st[1] is None else advance(st[1], prev_ids[i], lp, T)
            out[i] = joint_scores(logits[i], h, end_id, lp, T, lam, topn)
            nxt.append((new[i], h, None if lm_states is None else lm_states[i]))
        return out, nxt, alphas

    res = O.beam_search(jstep, (init_state, None, lm_init), n_frames, dec_step, beam_size, start_id, end_id, topn=topn)
    return res
