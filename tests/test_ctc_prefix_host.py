"""The CPU restatement of joint CTC-attention decoding (tests/ctc_prefix_ref.py): prefix scores telescope to the CTC log-likelihood,
and with weight 0 the joint search is the oracle's search."""
import numpy as np
import torch
import torch.nn.functional as F

import ctc_prefix_ref as R


def _log_probs(T, V, seed):
    rng = np.random.RandomState(seed)
    return torch.log_softmax(torch.tensor(rng.randn(T, V + 1) * 2.0), -1).numpy()


def _ctc_nll(lp, labels):
    T = lp.shape[0]
    return float(F.ctc_loss(torch.tensor(lp)[:, None], torch.tensor([labels]), [T], [len(labels)], blank=lp.shape[1] - 1,
                            reduction="sum", zero_infinity=False))


def test_chained_prefix_scores_equal_ctc_log_likelihood():
    """Summing the deltas psi(h.c) - psi(h) along c1 .. ck EOS gives log p_ctc(c1 .. ck EOS) = -ctc_loss (blank = V), in float64"""
    V, eos = 30, 2
    for T, labels, seed in ((40, [5, 7, 7, 9, 2], 0), (12, [3, 3, 3, 2], 1), (25, [4, 11, 4, 28, 17, 6, 2], 2), (1, [2], 3),
                            (6, [8, 2], 4)):
        lp = _log_probs(T, V, seed)
        s = R.empty_state(lp, T)
        total = 0.0
        for c in labels[:-1]:
            total += R.psi(s, c, lp, T) - s.psi
            s = R.advance(s, c, lp, T)
        total += R.eos_score(s, eos, lp, T) - s.psi
        assert abs(total - (-_ctc_nll(lp, labels))) < 1e-9 * max(1.0, abs(total)), (T, labels, total, -_ctc_nll(lp, labels))


def test_impossible_extensions_get_logzero():
    """A prefix longer than the frames, or repeats that do not fit, score ~LOGZERO (finite), not -inf"""
    V = 30
    lp = _log_probs(3, V, 5)
    s = R.empty_state(lp, 3)
    for c in (4, 5, 6):
        s = R.advance(s, c, lp, 3)
    v = R.psi(s, 7, lp, 3)
    assert np.isfinite(v) and v < -1e9
    s = R.advance(R.empty_state(lp, 3), 4, lp, 3)
    assert R.psi(s, 4, lp, 3) > -1e9                                          # 4 4 needs a blank between: 3 frames
    s = R.advance(s, 4, lp, 3)
    assert R.psi(s, 4, lp, 3) < -1e9 and R.eos_score(s, 2, lp, 3) < -1e9      # 4 4 4 / 4 4 EOS: 5 / 4 frames


def _toy_step_fn(V, seed):
    """a deterministic stand-in for the Speller: logits are a function of the hypothesis' token history (carried as its state)"""
    def step_fn(prev_ids, prev_al, states):
        logits, new = [], []
        for tok, st in zip(prev_ids, states):
            hist = st + (int(tok),)
            rng = np.random.RandomState(hash(hist) % (2 ** 31))
            lg = (rng.randn(V) * 2.0).astype(np.float32)
            lg[2] += 0.3 * len(hist)                       # EOS gets likelier with length
            logits.append(lg)
            new.append(hist)
        return np.stack(logits), new, np.zeros((len(prev_ids), 4), np.float32)
    return step_fn


def test_joint_search_with_weight_zero_is_the_oracle_search():
    from oracle import las_oracle as O
    V, T = 30, 20
    lp = _log_probs(T, V, 7)
    for beam in (3, 5):
        ref = O.beam_search(_toy_step_fn(V, 1), (), 4, 12, beam, 1, 2)
        got = R.joint_beam_search(_toy_step_fn(V, 1), (), 4, 12, beam, 1, 2, lp, T, 0.0)
        assert [h.token_ids for h in got] == [h.token_ids for h in ref]
        assert [h.log_prob for h in got] == [h.log_prob for h in ref]
        moved = R.joint_beam_search(_toy_step_fn(V, 1), (), 4, 12, beam, 1, 2, lp, T, 0.5)
        assert len(moved) == len(ref)


def test_candidate_bank_ties_follow_token_id():
    lg = np.zeros(100, np.float32)
    lg[:10] = 1.0
    bank = set(R.candidate_bank(lg).tolist())
    assert set(range(10)) <= bank and set(range(46, 100)) <= bank and len(bank) == 64
