"""CTC-only decoding on the CPU: the numpy restatement (tests/ctc_search_ref.py) against enumeration and F.ctc_loss, its
rules one by one, the n-gram gain against tests/ngram_ref.py, the flags and their refusals, and the decision margin of every case the
device tests run (a seed whose margin falls below ctc_search_ref.MARGIN is replaced HERE; no device case is skipped for a near tie)."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ctc_search_ref as R
import ngram_ref as G
from helpers import make_args

NO_EOS = 99                                                              # an EOS id no token has: nothing is closed


def _collapse(path, blank):
    return tuple(k for k, _ in itertools.groupby(path) if k != blank)


def _enumerate(lp, blank):
    """{collapsed string: log of the summed probability of every path that collapses to it} over all Vc ** T paths"""
    T, Vc = lp.shape
    mass = {}
    for path in itertools.product(range(Vc), repeat=T):
        s = float(sum(lp[t, c] for t, c in enumerate(path)))
        key = _collapse(path, blank)
        mass[key] = np.logaddexp(mass[key], s) if key in mass else s
    return mass


def _full_summary(z):
    T, Vc = z.shape
    return R.frame_summary(z, T, Vc - 1)


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5])
def test_exhaustive_search_equals_enumeration_and_ctc_loss(T):
    """V = 2, C = V, K >= the number of reachable prefixes, nothing closed: every prefix' total is the log-sum over all 3 ** T paths
    that collapse to it, and minus F.ctc_loss of that label sequence in float64"""
    rng = np.random.RandomState(T)
    z = (rng.randn(T, 3) * 1.5).astype(np.float32)
    s = _full_summary(z)
    hyps, _ = R.beam_search(s, 64, NO_EOS)
    lp = torch.log_softmax(torch.tensor(z, dtype=torch.float64), dim=1)
    mass = _enumerate(lp.numpy(), 2)
    assert len(hyps) == len(mass) <= 64 and {tuple(h[0]) for h in hyps} == set(mass)
    assert [h[1] for h in hyps] == sorted((h[1] for h in hyps), reverse=True)
    for toks, total in hyps:
        assert total == pytest.approx(mass[tuple(toks)], abs=1e-9)
        if toks:
            nll = F.ctc_loss(lp[:, None], torch.tensor([toks]), [T], [len(toks)], blank=2, reduction="sum").item()
            assert total == pytest.approx(-nll, abs=1e-9)


def test_greedy_is_the_collapsed_argmax_path():
    rng = np.random.RandomState(3)
    for Vc, T in ((3, 40), (31, 65), (5001, 20)):
        z = rng.randn(T, Vc).astype(np.float32)
        z[:, Vc - 1] += 1.0
        z[5:9] = z[4]                                                    # a run of one class
        s = _full_summary(z) if Vc < 100 else R.frame_summary(z, T, 8)
        toks, score = R.greedy(s["best"], s["best_lp"], Vc - 1)
        path = np.argmax(z, axis=1)
        assert toks == list(_collapse(path.tolist(), Vc - 1))
        lp = torch.log_softmax(torch.tensor(z, dtype=torch.float64), dim=1).numpy()
        assert score == pytest.approx(float(lp[np.arange(T), path].sum()), abs=1e-9)


def _peaked(classes, Vc, hi=12.0):
    """frames that put (almost) all mass on the given classes"""
    z = np.zeros((len(classes), Vc), np.float32)
    for t, c in enumerate(classes):
        z[t, c] = hi
    return z


def test_repeats_a_a_is_one_token_a_blank_a_is_two():
    V, a = 4, 1
    best = lambda classes: R.beam_search(_full_summary(_peaked(classes, V + 1)), 4, NO_EOS)[0][0][0]
    assert best([a, a]) == [a]
    assert best([a, V, a]) == [a, a]
    assert best([a, a, V, V, a, a]) == [a, a]
    assert best([a, 2, a]) == [a, 2, a]
    for classes in ([a, a], [a, V, a]):
        s = _full_summary(_peaked(classes, V + 1))
        assert R.greedy(s["best"], s["best_lp"], V)[0] == best(classes)


def test_all_blank_input_gives_the_empty_hypothesis():
    V = 4
    s = _full_summary(_peaked([V] * 6, V + 1))
    hyps, _ = R.beam_search(s, 4, R.EOS)
    assert hyps[0][0] == [] and hyps[0][1] == pytest.approx(0.0, abs=1e-3)
    assert R.greedy(s["best"], s["best_lp"], V)[0] == []
    only = np.full((5, V + 1), -np.inf, np.float32)                      # nothing but blank has mass: the empty hypothesis alone
    only[:, V] = 0.0
    hyps, margin = R.beam_search(_full_summary(only), 4, R.EOS)
    assert hyps == [([], 0.0)] and margin == np.inf
    hyps, _ = R.beam_search(R.frame_summary(np.zeros((0, V + 1), np.float32), 0, V), 4, R.EOS)      # no frame at all
    assert hyps == [([], 0.0)]


def test_a_closed_prefix_is_never_extended():
    """with EOS closing: no beam entry of any frame has a token behind EOS; closing removes the extensions of a closed prefix and
    leaves every kept prefix' own mass as it is (an exhaustive search, nothing pruned)"""
    rng = np.random.RandomState(7)
    V, T, eos = 3, 5, R.EOS
    z = (rng.randn(T, V + 1) * 1.5).astype(np.float32)
    z[2, eos] += 3.0
    trace = []
    hyps, _ = R.beam_search(_full_summary(z), 400, eos, trace=trace)
    assert any(eos in l for b in trace for l, _ in b)
    for b in trace:
        for l, _ in b:
            assert eos not in l[:-1]
    open_hyps, _ = R.beam_search(_full_summary(z), 400, NO_EOS)
    open_mass = {tuple(h[0]): h[1] for h in open_hyps}
    for toks, total in hyps:
        assert total == pytest.approx(open_mass[tuple(toks)], abs=1e-9)   # (closing removes extensions, not the prefix' own mass)
    assert len(hyps) < len(open_hyps)


def test_reentry_case_keeps_one_entry_per_prefix():
    """the hand-made case: (2, 0) leaves the beam after frame 3 and is back after frame 4 while (2, 0, 2) stays; no beam of any frame
    lists a prefix twice, and the margin holds"""
    z, K, C, eos = R.reentry_case()
    trace = []
    hyps, margin = R.beam_search(R.frame_summary(z, z.shape[0], C), K, eos, trace=trace)
    assert (3, 4, (2, 0), (2, 0, 2)) in R.reentries(trace)
    for b in trace:
        assert len({l for l, _ in b}) == len(b) <= K
    assert margin >= R.MARGIN
    assert [h[0] for h in hyps] == [[2, 0, 2, 0], [2, 0], [2, 2, 0], [2, 0, 2]]
    # the re-entered prefix carries the mass of BOTH its ways back: staying out of the beam loses what it had, but the extension of
    # (2,) by 0 at frame 4 and nothing else makes its p_nb -- K large enough for no pruning gives enumeration's value instead
    full, _ = R.beam_search(R.frame_summary(z, z.shape[0], C), 400, eos)
    lp = torch.log_softmax(torch.tensor(z, dtype=torch.float64), dim=1).numpy()
    mass = _enumerate(lp, 3)
    for toks, total in full:
        assert total == pytest.approx(mass[tuple(toks)], abs=1e-9)


@pytest.mark.parametrize("order", [1, 2, 3])
def test_ngram_fusion_adds_the_back_off_score_per_new_token(order):
    """gain = ngram_ref's row gain of that token; an exhaustive fused search gives enumeration's mass plus, per token, the last of
    ngram_ref.partial_sums64; weight 0 equals no LM; the gain read from the TABLES (TableGain) is the gain read from the dict"""
    from las.ngram import NgramLM
    rng = np.random.RandomState(20 + order)
    V, T, w, beta = 3, 4, 0.7, 0.25
    grams = G.random_model(rng, V, order, fan=2)
    gain = R.gram_gain(grams, order, w, R.SOS)
    lm = NgramLM(grams, order, V, R.SOS, R.EOS, 0)
    table = R.TableGain(lm.tables(w), lm.num_nodes, lm.num_entries, order, lm.step(0, R.SOS))
    for prefix in [(), (0,), (2, 1), (1, 1, 0), (0, 2, 1, 2)]:
        row = G.row_gains32(grams, order, w, (R.SOS,) + prefix, V)
        for c in range(V):
            assert gain(prefix, c) == row[c] == table(prefix, c)
            assert float(gain(prefix, c)) == pytest.approx(G.partial_sums64(grams, order, w, (R.SOS,) + prefix, c)[-1], abs=1e-5)
    z = (rng.randn(T, V + 1) * 1.5).astype(np.float32)
    s = _full_summary(z)
    hyps, _ = R.beam_search(s, 400, NO_EOS, gain, beta)
    lp = torch.log_softmax(torch.tensor(z, dtype=torch.float64), dim=1).numpy()
    mass = _enumerate(lp, V)
    assert {tuple(h[0]) for h in hyps} == set(mass)
    for toks, total in hyps:
        lm_sum = sum(G.partial_sums64(grams, order, w, (R.SOS,) + tuple(toks[:i]), toks[i])[-1] + beta for i in range(len(toks)))
        assert total == pytest.approx(mass[tuple(toks)] + lm_sum, abs=1e-4)
    plain, _ = R.beam_search(s, 400, NO_EOS)
    zero, _ = R.beam_search(s, 400, NO_EOS, R.gram_gain(grams, order, 0.0, R.SOS))
    assert zero == plain and hyps != plain


def test_flags_and_refusals():
    from las import ctc_search as CS
    a = make_args()
    assert (a.decoder, a.ctc_cand, a.ctc_len_bonus) == ("attention", 32, 0.0)
    assert CS.check_args(a) is False                                    # the default: the Speller's search, nothing of this runs
    ok = dict(decoder="ctc", ctc=True, beam_size=4)
    assert CS.check_args(make_args(**ok)) is True
    assert CS.check_args(make_args(**dict(ok, beam_size=1))) is True    # greedy
    assert CS.check_args(make_args(**dict(ok, ngram_lm="lm.arpa", ngram_weight=0.5))) is True
    assert CS.check_args(make_args(**dict(ok, beam_size=1, ngram_lm="lm.arpa", ngram_weight=0.0))) is True      # (weight 0: the LM is off)
    a = make_args(**dict(ok, ctc_cand=64, vocab_size=30))
    assert CS.cand(a) == 30
    for bad, msg in ((dict(decoder="rnnt"), "--decoder"), (dict(ctc=False), "--ctc True"), (dict(apply_lm=True), "--apply_lm"),
                     (dict(hotwords="words.txt"), "--hotwords"), (dict(hotword_weight=1.0), "--hotwords"),
                     (dict(ctc_decode_weight=0.3), "--ctc_decode_weight"),
                     (dict(beam_size=1, ngram_lm="lm.arpa", ngram_weight=0.5), "greedy"), (dict(beam_size=65), "--beam_size"),
                     (dict(beam_size=0), "--beam_size"), (dict(ctc_cand=0), "--ctc_cand"), (dict(ctc_cand=65), "--ctc_cand"),
                     (dict(ctc_len_bonus=float("inf")), "--ctc_len_bonus")):
        with pytest.raises(ValueError, match=msg):
            CS.check_args(make_args(**dict(ok, **bad)))


def test_every_device_case_keeps_its_decision_margin():
    """the case list of tests/test_gpu_ctc_search.py: every utterance's least decision margin (pruning cuts and final ranks, float64)
    is at least MARGIN; the list covers the shapes the kernels branch on; the float32 restatement ranks the same token lists, and the
    largest float32 - float64 differences are what the device tolerance is 4x of (printed: DESIGN 7n quotes them)"""
    assert {c["Vc"] for c in R.CASES} == {3, 31, 5001}
    assert {c["Tp"] for c in R.CASES} == {7, 65, 160} and {1, 2, 7, 65, 160} <= {T for c in R.CASES for T in c["lens"]}
    assert {c["K"] for c in R.CASES} == {2, 16, 64}
    assert {c["C"] for c in R.CASES} >= {1, 2, 32, 30} and all(c["C"] <= min(64, c["Vc"] - 1) for c in R.CASES)
    assert {c["order"] for c in R.CASES} == {0, 1, 3}
    for c in R.CASES:
        assert len(set(c["lens"])) > 1 and max(c["lens"]) <= c["Tp"]      # ragged
        for u, (_, _, hyps, margin) in enumerate(R.run_case(c["name"])):
            print(c["name"], u, "margin", margin, "hypotheses", len(hyps))
            assert margin >= R.MARGIN, (c["name"], u, margin)
    assert any(len(r[2]) < c["K"] for c in R.CASES for r in R.run_case(c["name"]))       # a beam that ends short of K
    lp_diff, sc_diff = R.measured_tolerance()
    print("float32 (kernel order) against float64: log-probabilities %.3e, scores %.3e" % (lp_diff, sc_diff))
    assert 0 < lp_diff < 1e-3 and 0 < sc_diff < R.MARGIN / 4             # 4x the difference stays below the margin the ranks keep
