"""CPU checks of the word-timestamp feature: the float64 restatement of las_ctc_align (tests/ctc_align_ref.py) against
exhaustive enumeration, the tie rule on a case written out by hand, and the host bookkeeping of las.align (words, frame_seconds)."""
import itertools

import numpy as np
import pytest

import ctc_align_ref as R
import helpers  # noqa: F401  (puts the package on sys.path)
from las import align as A

BLANK = 3           # 3-class alphabet plus blank


def _collapse(path):
    out, prev = [], None
    for c in path:
        if c != prev and c != BLANK:
            out.append(c)
        prev = c
    return tuple(out)


def test_restatement_matches_exhaustive_enumeration():
    """every T <= 6, every label sequence of L <= 3 over three classes (repeats included): the restatement's optimum is the maximum over
    ALL alignments (each summed in frame order in float64: the same additions, so equal bits), its path is valid and scores that optimum,
    and the sequences with no alignment are reported"""
    rng = np.random.RandomState(0)
    n_unalignable = 0
    for T in range(1, 7):
        lp = np.log(rng.dirichlet(np.ones(4), size=T).T).astype(np.float32)           # [4, T]
        best = {}
        for path in itertools.product(range(4), repeat=T):
            s = np.float64(lp[path[0], 0])
            for t in range(1, T):
                s = s + np.float64(lp[path[t], t])
            k = _collapse(path)
            if k not in best or s > best[k]:
                best[k] = float(s)
        for L in range(4):
            for labels in itertools.product(range(3), repeat=L):
                got = R.align(lp, labels, T)
                if labels not in best:
                    n_unalignable += 1
                    repeats = sum(a == b for a, b in zip(labels, labels[1:]))
                    assert L + repeats > T
                    assert got.score == -np.inf and got.states is None
                    assert list(got.first) == [-1] * L and list(got.last) == [-1] * L
                    continue
                assert got.score == best[labels], (T, labels)
                assert R.check_path(lp, labels, T, got.states) == got.score
                for j in range(L):
                    on = np.nonzero(got.states == 2 * j + 1)[0]
                    assert got.first[j] == on[0] and got.last[j] == on[-1] and len(on) == on[-1] - on[0] + 1
    assert n_unalignable > 0


def test_bad_labels_are_unalignable():
    lp = np.zeros((4, 5), np.float32)
    for labels in ([3], [-1], [0, 4]):
        assert R.align(lp, labels, 5).score == -np.inf


def test_uniform_lp_gives_the_path_the_tie_rule_dictates():
    """All paths tie, so every reachable (t, s) holds the same bits and the rule alone picks the path.  Worked by hand for labels
    (0, 1), S = 5 states: reachable at t = 0: {0, 1}; t = 1: {0, 1, 2, 3} (3 by the skip 1 -> 3); t >= 2: all.  The final state is 4 (2L
    wins the tie with 2L-1).  A step STAYS whenever (t-1, s) is reachable, so walking back from (T-1, 4) the path stays in 4 down to
    t = 2; (1, 4) is unreachable, so it came from s-1 = 3 at t = 1; (0, 3) and (0, 2) are unreachable, so that came by the skip from
    (0, 1).  The path climbs as early as it can and rests in the final blank."""
    lp = np.full((3, 8), np.log(1.0 / 3.0), np.float32)
    a = R.align(lp, [0, 1], 6)
    assert list(a.states) == [1, 3, 4, 4, 4, 4] and list(a.first) == [0, 1] and list(a.last) == [0, 1]
    assert list(R.align(lp, [0, 1], 4).states) == [1, 3, 4, 4]
    assert list(R.align(lp, [0, 1], 2).states) == [1, 3]                  # only 2L-1 is reachable at the end
    # labels (0, 0): no skip between equal labels, the blank between them is compulsory.  T = 3: reachable {0,1}, {0,1,2}, {0..3}; state 4
    # is unreachable at the end, so the final state is 3 and the only path is 1, 2, 3.  T = 2: nothing reaches 3 or 4.
    a = R.align(lp, [0, 0], 3)
    assert list(a.states) == [1, 2, 3] and list(a.first) == [0, 2] and list(a.last) == [0, 2]
    assert R.align(lp, [0, 0], 2).score == -np.inf
    # no labels: all blanks, the sum of the blank column in frame order
    a = R.align(lp, [], 3)
    assert list(a.states) == [0, 0, 0] and a.score == float(np.float64(lp[2, 0]) + np.float64(lp[2, 1]) + np.float64(lp[2, 2]))
    assert R.check_path(lp, [], 3, a.states) == a.score


# ---- las.align.words / frame_seconds
def _char_table():
    from utils.tokenizer import CharEncoder
    return CharEncoder()


def test_words_char_unit():
    from las.utils import convert_idx_to_string
    tok = _char_table()
    ids = tok.encode(" HI  YOU ", with_eos=True) + tok.encode("XX", with_eos=False)       # leading / doubled / trailing spaces, junk behind EOS
    spans = [(2 * i, 2 * i + 1) for i in range(len(ids))]
    w = A.words(ids, spans, tok.id_to_token, "char", 0.04, 0.69)
    assert [x["word"] for x in w] == ["HI", "YOU"]
    assert " ".join(x["word"] for x in w) == convert_idx_to_string(ids, tok.id_to_token, "char")
    # " HI  YOU ": H = token 1 (frames 2-3), I = token 2 (4-5); Y, O, U = tokens 5, 6, 7 (frames 10-15)
    assert w[0]["start"] == pytest.approx(2 * 0.04) and w[0]["end"] == pytest.approx(6 * 0.04)
    assert w[1]["start"] == pytest.approx(10 * 0.04) and w[1]["end"] == pytest.approx(16 * 0.04)
    # the end is capped at the recording's duration
    assert A.words(ids, spans, tok.id_to_token, "char", 0.04, 0.61)[1]["end"] == 0.61
    # an utterance that could not be aligned: the words, without times
    w = A.words(ids, [(-1, -1)] * len(ids), tok.id_to_token, "char", 0.04, 1.0)
    assert [(x["word"], x["start"], x["end"]) for x in w] == [("HI", None, None), ("YOU", None, None)]
    # an empty hypothesis, and one that is only <EOS>
    assert A.words([], [], tok.id_to_token, "char", 0.04, 1.0) == []
    assert A.words([2], [(0, 0)], tok.id_to_token, "char", 0.04, 1.0) == []


def test_words_subword_unit():
    from las.utils import convert_idx_to_string
    id_to_token = {0: "<PAD>", 1: "<SOS>", 2: "<EOS>", 3: "he", 4: "llo</w>", 5: "a</w>", 6: "wor", 7: "ld</w>", 8: "tail"}
    ids = [3, 4, 5, 6, 7, 8, 2, 5]                        # "hello a world tail" <EOS> junk
    spans = [(0, 1), (2, 2), (5, 5), (7, 8), (9, 9), (11, 12), (13, 13), (14, 14)]
    w = A.words(ids, spans, id_to_token, "subword", 0.08, 100.0)
    assert [x["word"] for x in w] == ["hello", "a", "world", "tail"]           # (a last word without </w> still counts, as in the text)
    assert " ".join(x["word"] for x in w) == convert_idx_to_string(ids, id_to_token, "subword")
    assert [(x["start"], x["end"]) for x in w] == [pytest.approx((0.0, 3 * 0.08)), pytest.approx((5 * 0.08, 6 * 0.08)),
                                                    pytest.approx((7 * 0.08, 10 * 0.08)), pytest.approx((11 * 0.08, 13 * 0.08))]
    w = A.words(ids, [(-1, -1)] * len(ids), id_to_token, "subword", 0.08, 100.0)
    assert all(x["start"] is None and x["end"] is None for x in w) and len(w) == 4
    assert A.words([2], [(0, 0)], id_to_token, "subword", 0.08, 1.0) == []


@pytest.mark.parametrize("layers", [1, 2, 3])
def test_frame_seconds_follows_the_listeners_halvings(layers):
    from las.las import Listener
    args = helpers.make_args(num_enc_layers=layers, frame_step=10)
    for enc_type in ("pblstm", "cnn"):
        red = A.time_reduction(args, enc_type)
        assert red == (2 ** layers if enc_type == "pblstm" else 4)
        # the listener's own length rule on a length the halvings divide: frames in / frames out
        n = 2 ** 6 * 5
        assert float(Listener(args).output_length([n], enc_type)[0]) * red == n
        assert A.frame_seconds(args, enc_type) == pytest.approx(0.010 * red)
    args.frame_step = 20
    assert A.frame_seconds(args, "pblstm") == pytest.approx(0.020 * 2 ** layers)
