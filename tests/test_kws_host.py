"""The keyword-search contract (include/las_hip.h K10j) on the CPU: the float64 restatement tests/kws_ref.py on a case worked
by hand, on planted phrases, on its tie and overflow rules, and las.kws.KeywordList.  tests/test_gpu_kws.py holds the kernel to the
same restatement, for equality.

The case worked by hand: Vc = 4 (classes 0, 1, 2 and the blank 3), T = 6, phrase [0, 1]: states s0 = label 0, s1 = the blank between,
s2 = label 1 (0 != 1: the step s0 -> s2 is allowed).  Relative emissions e = lp - frame maximum (every lp below is e - 0.5):

    t             0    1    2    3    4    5
    class 0      -2    0    0   -1   -3   -2
    class 1      -3   -2   -1   -2    0   -1
    class 2       0   -4   -4   -4   -4    0
    blank        -1   -1   -2    0   -1   -2

    t = 0: s0 = fresh (0, 0) - 2 = (-2, start 0); s1, s2 = (-inf, -1)                                      end (-inf, -1)
    t = 1: s0: stay -2, fresh 0 > -2 -> (0, 1) + 0 = (0, 1);  s1: from s0 (-2, 0) - 1 = (-3, 0);
           s2: skip from s0 (-2, 0) - 2 = (-4, 0)                                                          end (-4, 0)
    t = 2: s0: stay 0, fresh 0 > 0 is false -> (0, 1);  s1: s0's 0 > -3 -> (0, 1) - 2 = (-2, 1);
           s2: stay -4, s1's -3 > -4, s0's 0 > -3 -> (0, 1) - 1 = (-1, 1)                                  end (-1, 1)
    t = 3: s0: (0, 1) - 1 = (-1, 1);  s1: s0's 0 > -2 -> (0, 1) + 0 = (0, 1);
           s2: stay -1, s1's -2 no, s0's 0 > -1 -> (0, 1) - 2 = (-2, 1)                                    end (-2, 1)
    t = 4: s0: stay -1, fresh -> (0, 4) - 3 = (-3, 4);  s1: stay 0 -> (0, 1) - 1 = (-1, 1);
           s2: stay -2, s1's 0 > -2 -> (0, 1) + 0 = (0, 1)                                                 end (0, 1)
    t = 5: s0: fresh (0, 5) - 2 = (-2, 5);  s1: (-1, 1) - 2 = (-3, 1);  s2: stay (0, 1) - 1 = (-1, 1)      end (-1, 1)

    end_score = [-inf, -4, -1, -2, 0, -1], end_start = [-1, 0, 1, 1, 1, 1]: the head's greedy path says 0 0 blank 1 over frames 1 .. 4,
    and the series is exactly 0.0 at t = 4 with start 1.
    thr = -1.0 x 2 = -2: candidates t = 2 (-1), 3 (-2), 4 (0), 5 (-1), all with start 1.  t = 2 opens (-1, 1, 2); t = 3 overlaps (1 <= 2)
    and scores lower: dropped; t = 4 overlaps and scores higher: the open hit becomes (0, 1, 4); t = 5 overlaps (1 <= 4), lower: dropped;
    at T the hit closes: ONE hit, frames 1 .. 4, score 0.0; count = (1, 1); best = (0.0, 1, 4)."""
import numpy as np
import pytest
import torch

import helpers  # noqa: F401
import kws_ref as R

HAND_E = np.array([[-2, 0, 0, -1, -3, -2], [-3, -2, -1, -2, 0, -1], [0, -4, -4, -4, -4, 0], [-1, -1, -2, 0, -1, -2]], np.float32)


def hand_case():
    return (HAND_E - np.float32(0.5)).astype(np.float32), [0, 1]


def test_case_worked_by_hand():
    lp, phrase = hand_case()
    r = R.search(lp, phrase, 6, -2.0, 4)
    assert list(r.end_score) == [-np.inf, -4.0, -1.0, -2.0, 0.0, -1.0]
    assert list(r.end_start) == [-1, 0, 1, 1, 1, 1]
    assert r.hits == [(1, 4, 0.0)] and (r.kept, r.total) == (1, 1) and r.best == (0.0, 1, 4)
    # a shorter row: frames 0 .. 3 only
    r = R.search(lp, phrase, 4, -2.0, 4, Tp=6)
    assert list(r.end_score) == [-np.inf, -4.0, -1.0, -2.0, -np.inf, -np.inf] and list(r.end_start) == [-1, 0, 1, 1, -1, -1]
    assert r.hits == [(1, 2, -1.0)] and r.best == (-1.0, 1, 2)


# ---- the planted case (shared with tests/test_gpu_kws.py) -----------------------------------------------------------------------------
PLANTED_SEED = 3
PLANTED_PHRASES = [[3, 7, 9], [11, 11, 14, 2, 11], [20, 21]]         # disjoint label sets; the second needs a blank between its repeats


def planted_case(seed=PLANTED_SEED):
    """-> lp [2, 31, 90] fp32, lens, phrases, want[u][p] = (start, end).  Logits are uniform(0, 1) plus 6.0 on a chosen path: per
    utterance one window for every phrase (label runs of one to three frames, blank runs between them -- at least one frame between
    repeated labels), and the blank on every frame outside the windows.  Flat frames outside the windows would not do: with all logits
    in (0, 1) every class is within one nat of the frame's best, and any L labels over any L frames would pass -1.0 x L.  With the blank
    planted there the arg-max of the frame before each window is not the window's first label, and a path that leaves the planted one
    pays more than 5 nats for every frame it does so in (6 + uniform against uniform)."""
    rng = np.random.RandomState(seed)
    Vc, Tp, lens = 31, 90, [90, 61]
    logits = rng.uniform(0, 1, size=(2, Vc, Tp)).astype(np.float32)
    want = []
    for u, T in enumerate(lens):
        path = np.full(Tp, Vc - 1, np.int64)
        t = int(rng.randint(1, 4))
        spans = {}
        for p in rng.permutation(len(PLANTED_PHRASES)):
            ph = PLANTED_PHRASES[p]
            a = t
            for j, c in enumerate(ph):
                if j:
                    gap = int(rng.randint(0, 3))
                    t += max(gap, 1) if ph[j - 1] == c else gap          # (the blank run: path[] holds the blank already)
                r = int(rng.randint(1, 4))
                path[t:t + r] = c
                t += r
            spans[int(p)] = (a, t - 1)
            t += int(rng.randint(1, 5))
        assert t <= T, (t, T)
        logits[u, path, np.arange(Tp)] += np.float32(6.0)
        want.append([spans[p] for p in range(len(PLANTED_PHRASES))])
    lp = torch.log_softmax(torch.tensor(logits), 1).numpy()
    for u in range(2):
        for p, (a, b) in enumerate(want[u]):
            assert int(lp[u, :, a - 1].argmax()) != PLANTED_PHRASES[p][0]
    return lp, lens, PLANTED_PHRASES, want


def test_planted_phrases_are_found_exactly():
    lp, lens, phrases, want = planted_case()
    for u, T in enumerate(lens):
        for p, ph in enumerate(phrases):
            r = R.search(lp[u], ph, T, -1.0 * len(ph), 4)
            a, b = want[u][p]
            assert r.hits == [(a, b, 0.0)], (u, p, r.hits, want[u][p])     # exactly the planted span, score exactly 0.0, no other hit
            assert (r.kept, r.total) == (1, 1) and r.best == (0.0, a, b)
            assert r.end_score[b] == 0.0 and r.end_start[b] == a


# ---- properties ----------------------------------------------------------------------------------------------------------------------
def _lp(rng, Vc, Tp, scale=2.0):
    return torch.log_softmax(torch.tensor(rng.randn(Tp, Vc) * scale, dtype=torch.float32), -1).t().contiguous().numpy()


def test_every_finite_score_is_at_most_zero():
    rng = np.random.RandomState(0)
    lp = _lp(rng, 12, 40)
    for ph in ([4], [1, 2], [5, 5, 5], [0, 3, 3, 7, 10, 2]):
        r = R.search(lp, ph, 37, -np.inf, 8)
        fin = np.isfinite(r.end_score)
        need = len(ph) + sum(a == b for a, b in zip(ph, ph[1:])) - 1      # the first frame at which the end state can be reached
        assert not fin[:need].any() and fin[need:37].all() and not fin[37:].any()
        assert np.all(r.end_score[fin] <= 0.0) and np.all(r.end_start[fin] >= 0) and np.all(r.end_start[~fin] == -1)
        assert all(sc <= 0.0 and 0 <= a <= b < 37 for a, b, sc in r.hits) and r.best[0] <= 0.0
        assert r.best[0] == r.end_score[fin].max() and r.total >= r.kept == len(r.hits)
        assert [h[0] for h in r.hits] == sorted(h[0] for h in r.hits)       # time order


def test_uniform_lp_ties():
    """every path scores 0.0: the series is zero from the first reachable frame on, every start is frame 0 (staying in the first label
    beats a fresh start on the tie), every candidate overlaps the open hit and replaces it (the later end on a tie): one hit (0, T - 1)"""
    Vc, T = 6, 23
    lp = np.full((Vc, 30), np.float32(np.log(1.0 / Vc)), np.float32)
    for ph in ([2], [0, 1], [3, 3], [4, 0, 0, 4, 1]):
        need = len(ph) + sum(a == b for a, b in zip(ph, ph[1:])) - 1
        for thr in (-np.inf, -1.0, 0.0):
            r = R.search(lp, ph, T, thr, 2)
            assert np.all(r.end_score[:need] == -np.inf) and np.all(r.end_score[need:T] == 0.0) and np.all(r.end_start[need:T] == 0)
            assert r.hits == [(0, T - 1, 0.0)] and (r.kept, r.total) == (1, 1) and r.best == (0.0, 0, T - 1)
    r = R.search(lp, [1, 1, 1], 4, -np.inf, 2)                              # five frames needed, four there: the end is never reached
    assert r.hits == [] and (r.kept, r.total) == (0, 0) and r.best == (-np.inf, -1, -1) and np.all(r.end_score == -np.inf)


OVERFLOW_SCORES = [-0.375, -0.125, -0.625, -0.25, -0.5]                     # at frames 3, 8, 13, 18, 23


def overflow_case():
    """Vc = 8, phrase [5]: class 0 is every frame's arg-max at lp = 0; label 5 is at -20 except in five single frames"""
    lp = np.full((8, 28), np.float32(-30.0), np.float32)
    lp[0] = 0.0
    lp[5] = -20.0
    for k, sc in enumerate(OVERFLOW_SCORES):
        lp[5, 3 + 5 * k] = sc
    return lp, [5]


def test_kept_list_overflow():
    lp, ph = overflow_case()
    hit = lambda k: (3 + 5 * k, 3 + 5 * k, OVERFLOW_SCORES[k])
    r = R.search(lp, ph, 28, -1.0, 8)
    assert r.hits == [hit(k) for k in range(5)] and r.total == 5
    # H = 2: hits 0, 1 fill the list; 2 (-0.625) is not above the weakest (-0.375): dropped; 3 (-0.25) replaces hit 0 and is appended;
    # 4 (-0.5) is not above the weakest (-0.25): dropped
    r = R.search(lp, ph, 28, -1.0, 2)
    assert r.hits == [hit(1), hit(3)] and (r.kept, r.total) == (2, 5)
    r = R.search(lp, ph, 28, -1.0, 1)
    assert r.hits == [hit(1)] and (r.kept, r.total) == (1, 5)
    assert r.best == (-0.125, 8, 8)
    # equal scores: the earliest among equals is the weakest, and a closing hit must be STRICTLY greater to get in
    kept, total = R.hits_of(np.array([-1.0, -9.0, -1.0, -9.0, -1.0, -9.0, -0.5]), np.array([0, 1, 2, 3, 4, 5, 6]), -2.0, 2)
    assert kept == [(2, 2, -1.0), (6, 6, -0.5)] and total == 4


def test_unsearchable_phrases():
    lp = np.zeros((6, 9), np.float32)
    for ph in ([], [0] * 33, [1, 5, 2], [3, -1]):
        r = R.search(lp, ph, 9, -np.inf, 4)
        assert r.hits == [] and (r.kept, r.total) == (0, 0) and r.best == (-np.inf, -1, -1)
        assert np.all(r.end_score == -np.inf) and np.all(r.end_start == -1)


# ---- las.kws.KeywordList -----------------------------------------------------------------------------------------------------------------
def test_keyword_list_validation():
    from las.kws import KeywordList
    k = KeywordList([[5, 6], [7]], ["AB", "C"], vocab_size=30)
    assert len(k) == 2 and k.phrases == [[5, 6], [7]] and k.texts == ["AB", "C"]
    assert KeywordList([[5, 6]]).texts == ["5 6"]
    for bad, msg in (([], "no phrases"), ([[]], "is empty"), ([[0, 5]], "<SOS> / <PAD>"), ([[1]], "<SOS> / <PAD>"), ([[30]], "outside"),
                     ([[-2]], "outside"), (["AB"], "is text"), ([[5] * 33], "33 tokens"), ([[2.5]], "not a token id")):
        with pytest.raises(ValueError, match=msg):
            KeywordList(bad, vocab_size=30)
    with pytest.raises(ValueError, match="phrase 1 .* has 33 tokens"):                    # the error names the phrase
        KeywordList([[5], [6] * 33], vocab_size=30)
    with pytest.raises(ValueError, match="2 phrases, 1 texts"):
        KeywordList([[5], [6]], ["A"], vocab_size=30)


def test_keyword_list_from_file(tmp_path):
    from las.kws import KeywordList
    from utils.tokenizer import CharEncoder
    tok = CharEncoder()
    V = tok.get_vocab_size()
    f = tmp_path / "kw.txt"
    f.write_text("# names\n\nnew   york\n  \nBOSTON\n# trailing comment\n")
    k = KeywordList.from_file(str(f), tok, V)
    assert k.texts == ["NEW YORK", "BOSTON"]
    assert k.phrases == [tok.encode("NEW YORK", with_eos=False), tok.encode("BOSTON", with_eos=False)]
    f.write_text("BOSTON\n# x\nNEW_YORK\n")
    with pytest.raises(ValueError, match="line 3: character .* is not in the vocabulary"):
        KeywordList.from_file(str(f), tok, V)
    f.write_text("BOSTON\n\n" + "A" * 33 + "\n")
    with pytest.raises(ValueError, match="line 3 .*33 tokens"):
        KeywordList.from_file(str(f), tok, V)
    f.write_text("A" * 32 + "\n")
    assert len(KeywordList.from_file(str(f), tok, V).phrases[0]) == 32
    f.write_text("# nothing\n\n")
    with pytest.raises(ValueError, match="holds no phrase"):
        KeywordList.from_file(str(f), tok, V)
    with pytest.raises(ValueError, match="no such file"):
        KeywordList.from_file(str(tmp_path / "absent.txt"), tok, V)
