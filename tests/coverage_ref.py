"""CPU restatement of attention coverage (las/coverage.py, csrc/coverage.hip) in numpy float32, and the beam search with
the coverage gain built on the oracle's.

For a hypothesis with alignments alpha_1 .. alpha_t over its utterance's T' encoder frames (enc_len, clamped to [0, Tp]):
  cum_t[j]  = fl32(cum_{t-1}[j] + alpha_t[j]), cum_0 = 0            (every j < Tp; one float32 add per step and frame, in step order)
  covered_t = #{ j < T' : cum_t[j] > tau },  over_t = #{ j < T' : cum_t[j] > kappa }      (a NaN never counts)
  dc = covered_t - covered_{t-1}, do = over_t - over_{t-1};  g = fl32( fl32(w_c dc) - fl32(w_o do) );  score = fl32(score + g)
A state is (cum float32 [Tp], covered float32, over float32): the counts are float32 words, as in the device's state row."""
import numpy as np

f32 = np.float32


def empty_state(Tp):
    return np.zeros(int(Tp), f32), f32(0.0), f32(0.0)


def advance(state, alpha, enc_len, tau, kappa):
    """one step: (state, the step's alignment [Tp]) -> (new state, dc, do), dc / do float32"""
    cum0, c0, o0 = state
    alpha = np.asarray(alpha, f32)
    Tp = alpha.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        cum = (np.asarray(cum0, f32) + alpha).astype(f32)
        L = min(max(int(enc_len), 0), Tp)
        c = f32(np.count_nonzero(cum[:L] > f32(tau)))
        o = f32(np.count_nonzero(cum[:L] > f32(kappa)))
        return (cum, c, o), f32(c - f32(c0)), f32(o - f32(o0))


def gain(w_c, w_o, dc, do):
    with np.errstate(invalid="ignore", over="ignore"):
        return f32(f32(f32(w_c) * f32(dc)) - f32(f32(w_o) * f32(do)))


def counts(atts, enc_len, tau, kappa):
    """(covered, over) of a finished hypothesis from its alignments in step order (a BeamState's att list WITHOUT its all-zero item 0
    -- adding zeros changes nothing, so the whole list may be passed too)"""
    atts = [np.asarray(a, f32) for a in atts]
    st = empty_state(atts[0].shape[0])
    for a in atts:
        st, _, _ = advance(st, a, enc_len, tau, kappa)
    return int(st[1]), int(st[2])


def gains(atts, enc_len, w_c, w_o, tau, kappa):
    """the float32 gain of every step of a hypothesis"""
    atts = [np.asarray(a, f32) for a in atts]
    st, out = empty_state(atts[0].shape[0]), []
    for a in atts:
        st, dc, do = advance(st, a, enc_len, tau, kappa)
        out.append(gain(w_c, w_o, dc, do))
    return np.asarray(out, f32)


def margin(cum, enc_len, tau, kappa):
    """the least distance of a counted cum value from a threshold"""
    L = min(max(int(enc_len), 0), cum.shape[0])
    if L == 0:
        return np.inf
    c = cum[:L].astype(np.float64)
    return float(min(np.min(np.abs(c - float(f32(tau)))), np.min(np.abs(c - float(f32(kappa))))))


def covered_beam_search(step_fn, init_state, n_frames, dec_step, beam_size, start_id, end_id, enc_len, w_c, w_o, tau, kappa, topn=64):
    """oracle.las_oracle.beam_search's control flow (its Hyp and select_best_k) with the coverage gain: every live row's state is
    advanced by the step's alignment and the gain is added to the PARENT's running sum before its candidates are formed, so a
    candidate scores fl32(fl32(sum + g) + logit).  This cannot be a step_fn wrapper as in bias_ref.py: a wrapper could only add g to
    the logits, which gives fl32(sum + fl32(logit + g)) -- another rounding sequence than the device's.  With w_c = w_o = 0 the sum is
    left alone and the search is the oracle's, exactly.
    A Hyp's dec_state is (decoder state, coverage state).  -> (hypotheses ascending as the oracle returns them, the least distance of
    any counted cum value of any hypothesis in any step's bank from tau or kappa)."""
    from oracle import las_oracle as O
    scored = f32(w_c) != 0 or f32(w_o) != 0
    beam_set = [O.Hyp([start_id], 0, [np.zeros(n_frames)], (init_state, empty_state(n_frames)), None)] * beam_size
    selected, t, least = [], 0, np.inf
    while t < dec_step and len(selected) < beam_size:
        prev_ids = [b.token_ids[-1] for b in beam_set]
        prev_al = [b.att[-1] for b in beam_set]
        logits, states, alphas = step_fn(prev_ids, prev_al, [b.dec_state[0] for b in beam_set])
        logits = np.array(logits, dtype=np.float32, copy=True)
        num_beam = len(beam_set) if t > 0 else 1
        bank = []
        for i in range(num_beam):
            par = beam_set[i]
            cov, dc, do = advance(par.dec_state[1], alphas[i], enc_len, tau, kappa)
            least = min(least, margin(cov[0], enc_len, tau, kappa))
            base = f32(f32(par.log_prob) + gain(w_c, w_o, dc, do)) if scored else par.log_prob
            topk = np.argsort(logits[i])[-topn:]
            for j in range(len(topk)):
                if t > 0 and topk[j] == start_id:
                    continue
                bank.append(O.Hyp(par.token_ids + [int(topk[j])], base + logits[i][topk[j]], par.att + [alphas[i]], (states[i], cov), None))
        beam_set = []
        for b in O.select_best_k(bank, beam_size):
            (selected if b.token_ids[-1] == end_id else beam_set).append(b)
        t += 1
    if t == dec_step:
        selected.extend(beam_set)
    return O.select_best_k(selected, beam_size), least
