"""Contextual biasing on the host: las.bias.ContextGraph's flat trie tables against the brute-force phrase-list walker of
tests/bias_ref.py, gain for gain and by bytes; the named cases; the refusals; the hotword file."""
import numpy as np
import pytest

import bias_ref as B
from las.bias import MAX_V, ContextGraph, from_args


def _table_gains(g, tokens):
    """the tables driven as the kernel drives them"""
    s, out = 0, []
    for v in tokens:
        s, gain = g.step(s, int(v))
        out.append(gain)
    return np.asarray(out, np.float32), s


def _same(phrases, beta, tokens):
    g = ContextGraph(phrases, beta, vocab_size=16)
    got, _ = _table_gains(g, tokens)
    want = B.gains(phrases, beta, tokens)
    assert got.tobytes() == want.tobytes(), (phrases, beta, list(tokens), got, want)
    return got


def test_tables_against_the_brute_force_walker_on_random_phrase_sets():
    """3000 random cases over a 5-token alphabet (tokens 2 .. 6), 12-token strings: every gain equal by bytes (the sign of a zero gain
    included: both sides pay -pend = -0 for a mismatch on a phrase end with children)"""
    rng = np.random.RandomState(0)
    for case in range(3000):
        phrases = [list(rng.randint(2, 7, size=rng.randint(1, 5))) for _ in range(rng.randint(1, 6))]
        beta = [0.5, 1.5, 2.0, 0.3, 1.7][case % 5]
        _same(phrases, beta, rng.randint(2, 7, size=12))


def test_row_gains_of_the_reference_agree_with_its_walker():
    """bias_ref.row_gains (the candidates' gains by class) against one walk per candidate, by bytes"""
    rng = np.random.RandomState(2)
    for case in range(300):
        phrases = [list(rng.randint(2, 7, size=rng.randint(1, 5))) for _ in range(rng.randint(1, 6))]
        m = B.match_after(phrases, 0.3, rng.randint(2, 7, size=rng.randint(0, 6)))
        assert B.row_gains(phrases, 0.3, m, 9).tobytes() == B.row_gains_by_walking(phrases, 0.3, m, 9).tobytes(), (phrases, m)


def test_tables_shape_and_order():
    g = ContextGraph([[5, 3], [5, 2, 4], [3], [5, 3]], 1.5, vocab_size=8)
    assert g.num_nodes == 6 and g.child_off.dtype == np.int32 and g.child_off.shape == (7,)
    assert g.child_tok.dtype == g.child_next.dtype == np.int32 and g.gdef.dtype == g.groot.dtype == np.float32 and g.beta.dtype == np.float32
    for s in range(g.num_nodes):
        toks = g.child_tok[g.child_off[s]:g.child_off[s + 1]]
        assert np.all(np.diff(toks) > 0)                                  # ascending, no duplicates
    assert g.child_off[-1] == g.child_tok.size == g.child_next.size == 5
    assert list(g.child_tok[:2]) == [3, 5] and g.child_next[0] == 0      # rule 4: [3] is a childless phrase end
    assert g.phrases == [[5, 3], [5, 2, 4], [3]]                           # duplicates collapse
    assert np.all(g.gdef <= 0) and np.array_equal(g.groot, (g.beta + g.gdef).astype(np.float32))


def test_named_cases():
    # a phrase that is a prefix of another: NEW YORK / NEW YORK CITY
    ph = [[2, 3], [2, 3, 4]]
    assert list(_same(ph, 2.0, [2, 3, 4, 5])) == [2.0, 2.0, 2.0, 0.0]
    assert list(_same(ph, 2.0, [2, 3, 5, 5])) == [2.0, 2.0, 0.0, 0.0]       # the phrase end keeps its bonus (pend = 0)
    assert list(_same(ph, 2.0, [2, 3, 2, 5])) == [2.0, 2.0, 2.0, -2.0]      # ... and a new match starts from it at a root child
    g = ContextGraph(ph, 2.0, vocab_size=8)
    _, s = _table_gains(g, [2, 3])
    assert s != 0 and g.gdef[s] == 0 and g.groot[s] == 2.0
    # single-token phrases: back at the root at once
    assert list(_same([[4], [6]], 1.5, [4, 4, 6, 5, 4])) == [1.5, 1.5, 1.5, 0.0, 1.5]
    # duplicates
    assert _same([[2, 3], [2, 3]], 1.5, [2, 3, 2, 3]).tobytes() == _same([[2, 3]], 1.5, [2, 3, 2, 3]).tobytes()
    # a repeated token inside a phrase; no fail links: after A A the third A restarts the match at ITS position only
    assert list(_same([[2, 2, 3]], 1.0, [2, 2, 2, 3])) == [1.0, 1.0, -1.0, -1.0]
    assert list(_same([[2, 2, 3]], 1.0, [2, 2, 3])) == [1.0, 1.0, 1.0]
    # the failing token restarts a match (rule 2), an unknown token pays back (rule 3), EOS is an ordinary token
    assert list(_same([[2, 3, 4], [5, 6]], 0.5, [2, 3, 5, 6])) == [0.5, 0.5, -0.5, 0.5]
    assert list(_same([[3, 4, 5]], 0.5, [3, 4, 2])) == [0.5, 0.5, -1.0]


def test_total_bonus_is_never_negative():
    """with a weight whose small multiples are exact in float32 the sum is exactly >= 0 (and = beta x the tokens of the completed
    phrases); for any weight a payback is one rounding of k x beta, so the sum stays above -k beta 2^-23"""
    rng = np.random.RandomState(1)
    for case in range(1000):
        phrases = [list(rng.randint(2, 7, size=rng.randint(1, 5))) for _ in range(rng.randint(1, 6))]
        toks = rng.randint(2, 7, size=12)
        for beta in (1.5, 0.3):
            gs = B.gains(phrases, beta, toks)
            total = B.bonus(phrases, beta, toks)
            for k in range(1, 13):
                part = float(np.sum(gs[:k].astype(np.float64)))
                assert part >= (0.0 if beta == 1.5 else -12 * beta * 2.0 ** -23), (phrases, list(toks), k, part)
            if beta == 1.5 and B.match_after(phrases, beta, toks) == ():
                assert total == pytest.approx(1.5 * round(total / 1.5)) and total >= 0


def test_refusals():
    with pytest.raises(ValueError, match=r"phrase 1 \[\] is empty"):
        ContextGraph([[2], []], 1.0, vocab_size=8)
    with pytest.raises(ValueError, match=r"phrase 0 \[2, 8\].*outside \[0, 8\)"):
        ContextGraph([[2, 8]], 1.0, vocab_size=8)
    with pytest.raises(ValueError, match=r"\[3, -1\].*outside"):
        ContextGraph([[3, -1]], 1.0, vocab_size=8)
    with pytest.raises(ValueError, match=r"\[4, 1\].*SOS"):
        ContextGraph([[4, 1]], 1.0, vocab_size=8)
    with pytest.raises(ValueError, match=r"\[0\].*PAD"):
        ContextGraph([[0]], 1.0, vocab_size=8)
    for w in (-0.5, float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError, match="weight"):
            ContextGraph([[2]], w, vocab_size=8)
    with pytest.raises(ValueError, match="vocab_size"):
        ContextGraph([[2]], 1.0, vocab_size=MAX_V + 1)
    import las.bias as LB
    saved = LB.MAX_NODES, LB.MAX_ROOT_FANOUT
    try:
        LB.MAX_NODES = 4
        with pytest.raises(ValueError, match=r"phrase 1 \[5, 6\].*nodes"):
            ContextGraph([[2, 3, 4], [5, 6]], 1.0, vocab_size=8)
        LB.MAX_NODES, LB.MAX_ROOT_FANOUT = saved[0], 2
        with pytest.raises(ValueError, match=r"phrase 2 \[4\].*phrase-initial"):
            ContextGraph([[2], [3], [4]], 1.0, vocab_size=8)
    finally:
        LB.MAX_NODES, LB.MAX_ROOT_FANOUT = saved
    assert not ContextGraph([[2]], 0.0, vocab_size=8).active and not ContextGraph([], 1.0, vocab_size=8).active
    assert ContextGraph([[2]], 1.0, vocab_size=8).active


def test_from_file(tmp_path):
    from utils.tokenizer import CharEncoder
    tok = CharEncoder()
    f = tmp_path / "hot.txt"
    f.write_text("# names\n\nnew york\n  NEW YORK CITY  \n#zurich\nAda\nnew   york\n")
    g = ContextGraph.from_file(str(f), tok, 2.0, 30)
    enc = lambda t: tok.encode(t, with_eos=False)
    assert g.phrases == [enc("NEW YORK"), enc("NEW YORK CITY"), enc("ADA")]
    assert g.beta == np.float32(2.0) and g.vocab_size == 30
    f.write_text("OK\n# fine\nR2D2\n")
    with pytest.raises(ValueError, match=r"line 3"):
        ContextGraph.from_file(str(f), tok, 2.0, 30)
    with pytest.raises(ValueError, match="no such file"):
        ContextGraph.from_file(str(tmp_path / "absent.txt"), tok, 2.0, 30)


def test_flags(tmp_path):
    from las.arguments import parse_args
    a = parse_args([])
    assert a.hotwords == "" and a.hotword_weight == 0.0 and from_args(a) is None
    f = tmp_path / "hot.txt"
    f.write_text("ADA\n")
    a = parse_args(["--unit", "char", "--hotwords", str(f), "--hotword_weight", "2.0"])
    a.vocab_size = 30
    g = from_args(a)
    assert g.active and g.phrases == [[4, 7, 4]]
    a.hotword_weight = 0.0
    assert from_args(a) is None                                            # a file and weight 0: off
    a.hotword_weight, a.hotwords = 2.0, ""
    with pytest.raises(ValueError, match="--hotwords FILE"):
        from_args(a)
    a.hotwords = str(tmp_path / "absent.txt")
    with pytest.raises(ValueError, match="no such file"):
        from_args(a)
    a.hotword_weight = -1.0
    with pytest.raises(ValueError, match="hotword_weight"):
        from_args(a)
