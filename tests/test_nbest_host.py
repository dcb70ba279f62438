"""N-best consensus, host side: the numpy restatement tests/nbest_ref.py against las.utils.edit_distance and against the
properties of an edit distance and of an alignment; las.nbest's posteriors and word segmentation; the new flags."""
import itertools

import numpy as np
import pytest

import helpers  # noqa: F401
import nbest_ref as R
from las import align as A
from las import beam_search
from las import nbest as NB
from las.arguments import parse_args
from las.utils import convert_idx_to_string, edit_distance
from utils.tokenizer import CharEncoder


def _rand_seq(rng, vocab, max_len):
    return list(rng.randint(0, vocab, size=rng.randint(0, max_len + 1)))


def test_distance_equals_las_utils_edit_distance():
    rng = np.random.RandomState(0)
    for vocab, max_len in ((2, 6), (3, 20), (50, 40)):
        for _ in range(60):
            a, b = _rand_seq(rng, vocab, max_len), _rand_seq(rng, vocab, max_len)
            want = edit_distance(a, b)[0]
            assert R.distance(a, b) == want
            assert np.array_equal(R.table(a, b), R.table_fast(a, b))           # the literal table and its row-at-a-time form


def test_symmetry_and_triangle_inequality():
    rng = np.random.RandomState(1)
    for _ in range(80):
        a, b, c = (_rand_seq(rng, 3, 12) for _ in range(3))
        assert R.distance(a, b) == R.distance(b, a)
        assert R.distance(a, a) == 0
        assert R.distance(a, c) <= R.distance(a, b) + R.distance(b, c)


def test_alignment_is_consistent_on_all_short_binary_strings():
    """every pair over {0, 1} up to length 4: along the traced path, matches m, substitutions s, unmatched pivot tokens d and skipped
    hypothesis tokens e obey m + s + d = len(a), m + s + e = len(b), s + d + e = D -- so with m and D known:
    2 (m + D) >= len(a) + len(b) >= 2 m + D, and every matched position holds equal tokens in order"""
    strs = [list(s) for L in range(5) for s in itertools.product((0, 1), repeat=L)]
    for a in strs:
        for b in strs:
            D = R.table(a, b)
            match = R.backtrace(a, b, D)
            m, d = int(match.sum()), int(D[len(a), len(b)])
            assert 2 * m + d <= len(a) + len(b) <= 2 * (m + d)
            assert d >= abs(len(a) - len(b)) and m <= min(len(a), len(b)) and max(len(a), len(b)) - m <= d
            # the matched tokens of a form a common subsequence of a and b
            sub = [a[i] for i in range(len(a)) if match[i]]
            it = iter(b)
            assert all(any(x == y for y in it) for x in sub)
            if a == b:
                assert match.all()


def test_backtrace_prefers_the_diagonal():
    assert list(R.backtrace([7, 7, 7, 7], [7, 7])) == [0, 0, 1, 1]
    # abab against baba: distance 2 (not four substitutions); at (4, 4) neither diagonal rule holds, the last b of the pivot stays unmatched
    assert R.distance([1, 2, 1, 2], [2, 1, 2, 1]) == 2
    assert list(R.backtrace([1, 2, 1, 2], [2, 1, 2, 1])) == [1, 1, 1, 0]


def test_restatement_risk_and_confidence():
    hyps = [[1, 2, 3], [1, 2], [1, 5, 3], []]
    w = np.asarray([0.4, 0.3, 0.2, 0.1], np.float32)
    dist, risk, pick = R.risk(hyps, w)
    assert dist.tolist() == [[0, 1, 1, 3], [1, 0, 2, 2], [1, 2, 0, 3], [3, 2, 3, 0]]
    assert risk[0] == np.float32(np.float32(np.float32(0.3) + np.float32(0.2)) + np.float32(np.float32(0.1) * np.float32(3)))
    assert pick == 0
    match, conf = R.confidence(hyps, w, 0)
    assert match.tolist() == [[1, 1, 1], [1, 1, 0], [1, 0, 1], [0, 0, 0]]
    assert conf[0] == np.float32(np.float32(np.float32(0.4) + np.float32(0.3)) + np.float32(0.2))
    assert R.confidence(hyps, w, -1) == (None, None) and R.risk([], [])[2] == -1


def test_posteriors():
    sc, ln = [-3.0, -4.4, -9.0, -2.6], [3, 4, 6, 2]
    p = NB.posteriors(sc, ln)
    assert p.dtype == np.float32 and abs(float(p.astype(np.float64).sum()) - 1.0) < 1e-6 and np.all(p > 0)
    key = np.asarray(sc) / np.asarray(ln) if beam_search.NORM else np.asarray(sc)
    assert int(np.argmax(p)) == int(np.argmax(key))
    want = np.exp(key - key.max())
    assert np.allclose(p, want / want.sum(), rtol=1e-6)
    assert np.array_equal(NB.posteriors(sc, ln, scale=0.0), np.full(4, 0.25, np.float32))
    sharp = NB.posteriors(sc, ln, scale=1e4)
    assert sharp[int(np.argmax(key))] == 1.0 and sharp.sum() == 1.0
    p = NB.posteriors([-3.0, -np.inf, np.nan, -4.0], [3, 3, 3, 3])
    assert p[1] == 0 and p[2] == 0 and abs(float(p.sum()) - 1.0) < 1e-6
    assert np.array_equal(NB.posteriors([-np.inf, np.nan], [2, 2]), np.full(2, 0.5, np.float32))
    assert NB.posteriors([], []).shape == (0,)


class _State(object):
    def __init__(self, token_ids, log_prob):
        self.token_ids, self.log_prob = token_ids, np.float32(log_prob)


def test_hypotheses_are_best_first_and_cut_at_eos_and_the_top_posterior_is_the_searchs_choice():
    """the search ranks by score / (len(token_ids) - 1), best LAST (BeamSearch._decode_tail): the argmax of the posteriors is that one"""
    rng = np.random.RandomState(4)
    results = []
    for _ in range(20):
        states = [_State([1] + list(rng.randint(3, 30, size=rng.randint(1, 9))) + ([2] if rng.rand() < 0.7 else []), -rng.uniform(0.5, 20.0))
                  for _ in range(rng.randint(1, 6))]
        key = [float(s.log_prob) / (len(s.token_ids) - 1) if beam_search.NORM else float(s.log_prob) for s in states]
        results.append([states[i] for i in np.argsort(np.asarray(key), kind="stable")])
    results.append([])
    results.append([_State([1, 5, 2, 7, 2], -1.0)])
    token_lists, scores, lens = NB.hypotheses(results, 2)
    assert token_lists[-1] == [[5]] and lens[-1] == [4] and token_lists[-2] == [] and scores[-2] == []
    for r, tl, sc, ln in zip(results, token_lists, scores, lens):
        assert sc == [float(s.log_prob) for s in reversed(r)] and ln == [len(s.token_ids) - 1 for s in reversed(r)]
        w = NB.posteriors(sc, ln)
        if len(r) > 1:
            assert w[0] == w.max()
        for t, s in zip(tl, reversed(r)):
            ids = list(s.token_ids[1:])
            assert t == (ids[:ids.index(2)] if 2 in ids else ids)


def _same_words(ids, id_to_token, unit):
    conf = [0.01 * (k + 1) for k in range(len(ids))]
    spans = [(k, k) for k in range(len(ids))]
    timed = A.words(ids, spans, id_to_token, unit, 1.0, 1e9)
    sure = NB.word_confidence(ids, conf, id_to_token, unit)
    assert [w["word"] for w in sure] == [w["word"] for w in timed]
    assert " ".join(w["word"] for w in sure) == convert_idx_to_string(ids, id_to_token, unit)
    # a word's confidence is the minimum over its tokens = (conf rises along the list) that of the word's first token: its start frame
    for s, t in zip(sure, timed):
        assert s["confidence"] == pytest.approx(0.01 * (t["start"] + 1))
    return sure


def test_word_confidence_segments_like_align_words():
    tok = CharEncoder()
    sp, eos = tok.token_to_id["<SPACE>"], tok.token_to_id["<EOS>"]
    enc = lambda s: tok.encode(s, with_eos=False)
    for ids in (enc("HELLO WORLD"), [sp, sp] + enc("A") + [sp, sp, sp] + enc("BC") + [sp], enc("AB CD") + [eos] + enc("EF GH"), [eos], [],
                [sp], enc("X") + [eos]):
        _same_words(ids, tok.id_to_token, "char")
    w = NB.word_confidence(enc("AB CD"), [0.9, 0.5, 0.1, 0.8, 0.7], tok.id_to_token, "char")     # <SPACE>'s 0.1 belongs to no word
    assert w == [{"word": "AB", "confidence": 0.5}, {"word": "CD", "confidence": 0.7}]
    id_to_token = {0: "<PAD>", 1: "<SOS>", 2: "<EOS>", 3: "he", 4: "llo</w>", 5: "a</w>", 6: "wor", 7: "ld</w>", 8: "tail"}
    for ids in ([3, 4, 5, 6, 7], [3, 4, 6, 7, 8], [3, 4, 2, 5, 5], [8], [5, 5, 5], [2], []):            # a trailing unfinished subword; EOS mid-list
        _same_words(ids, id_to_token, "subword")
    w = NB.word_confidence([3, 4, 8], [0.9, 0.4, 0.6], id_to_token, "subword")
    assert w == [{"word": "hello", "confidence": 0.4}, {"word": "tail", "confidence": 0.6}]


def test_flags_default_to_off():
    a = parse_args([])
    assert a.nbest == 0 and a.confidence is False and a.mbr is False and a.nbest_scale == 1.0
    a = parse_args(["--nbest", "3", "--confidence", "True", "--mbr", "True", "--nbest_scale", "0.5", "--beam_size", "4"])
    assert a.nbest == 3 and a.confidence is True and a.mbr is True and a.nbest_scale == 0.5
    assert NB.Annotator(a, 2).active and not NB.Annotator(parse_args([]), 2).active
    a.nbest = 5
    with pytest.raises(ValueError, match="--nbest 5"):
        NB.Annotator(a, 2)
