"""N-gram LM shallow fusion on the host: las.ngram.NgramLM's tables and walker against the trie-free restatement of
tests/ngram_ref.py, gain for gain and by bytes; the rounding bound against float64; the ARPA reader and its refusals; train_ngram.py's
Witten-Bell estimates; the flags."""
import math
import sys

import numpy as np
import pytest

import ngram_ref as G
from helpers import PKG
from las import ngram as NG
from las.ngram import NgramLM, from_args, write_arpa

SOS, EOS, PAD = 1, 2, 0


def _models():
    for V in (5, 30, 257):
        for order in (1, 2, 3, 4):
            for seed in range(25):
                yield V, order, seed


def test_tables_and_walker_against_the_restatement_on_random_models():
    """300 random sparse prefix-closed models (V in {5, 30, 257}, order 1 .. 4; contexts whose suffixes are missing; tokens stored at two
    levels of one chain), along random token strings: the node after every token is the longest suffix of the history that is a node
    (brute force on the dict), every candidate's gain equals ngram_ref.row_gains32 by bytes, and
    |row_gains32 - w ln10 logp64| <= (order + 2) 2^-24 max |partial sums|: every table value is one rounding of its term and all terms
    have one sign (log p <= 0, and the models' bow <= 0), so those roundings sum to at most one unit of the largest partial sum; the
    chain's order - 1 accumulations (the first, onto 0, is exact) and the final add are at most one each."""
    n_models = n_two_levels = n_missing_suffix = n_deep = 0
    for V, order, seed in _models():
        rng = np.random.RandomState(1000 * V + 10 * order + seed)
        grams = G.random_model(rng, V, order)
        w = [0.5, 1.0, 0.3, 2.0, 0.7][seed % 5]
        lm = NgramLM(grams, order, V, SOS, EOS, PAD)
        assert lm.grams == grams and lm.num_nodes == 1 + sum(1 for k in grams if len(k) < order)
        n_models += 1
        n_missing_suffix += any(len(k) > 1 and k[1:] not in grams for k in grams)
        toks = G.random_string(rng, grams, order, V, 12 if V == 257 else 20, SOS)
        node = 0
        for i in range(len(toks)):
            node = lm.step(node, toks[i])
            hist = toks[:i + 1]
            state = G.state_of(grams, order, hist)
            assert lm.nodes[node] == state, (V, order, seed, hist, lm.nodes[node], state)
            n_deep += len(state) == order - 1 and order > 2
            got = lm.row_gains(node, w)
            want = G.row_gains32(grams, order, w, hist, V)
            assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), (V, order, seed, hist)
            for v in (range(V) if V < 257 else rng.randint(V, size=24)):
                v = int(v)
                exact = w * G.LN10 * G.logp64(grams, hist, v, order)
                parts = G.partial_sums64(grams, order, w, hist, v)
                assert abs(float(want[v]) - exact) <= (order + 2) * 2.0 ** -24 * max(abs(x) for x in parts), (V, order, seed, hist, v)
                ctx = G._context(hist, order)
                n_two_levels += sum(1 for k in range(len(ctx) + 1) if ctx[k:] + (v,) in grams) >= 2 and len(ctx) >= 1
    assert n_models == 300 and n_missing_suffix > 100 and n_two_levels > 100 and n_deep > 100


def test_tables_shape_order_and_limits():
    grams = {(0,): (-99.0, 0.0), (1,): (-99.0, -0.5), (2,): (-1.0, 0.0), (3,): (-0.5, -0.25), (4,): (-0.7, 0.0),
             (1, 3): (-0.1, -0.2), (3, 4): (-0.3, 0.0), (3, 2): (-0.4, 0.0), (1, 3, 4): (-0.05, 0.0), (1, 3, 2): (-0.06, 0.0)}
    lm = NgramLM(grams, 3, 5)
    assert lm.num_nodes == 1 + 5 + 3 and lm.num_entries == 5
    assert lm.child_off.dtype == np.int32 and lm.child_off.shape == (lm.num_nodes + 1,) and lm.child_off[1] == 0   # the root's list is empty
    for a in (lm.child_tok, lm.child_next, lm.bo, lm.uni_next):
        assert a.dtype == np.int32
    for a in (lm.child_lp, lm.bow, lm.uni_lp):
        assert a.dtype == np.float32
    assert lm.bow.shape == lm.bo.shape == (lm.num_nodes,) and lm.uni_lp.shape == lm.uni_next.shape == (5,)
    for s in range(lm.num_nodes):
        assert np.all(np.diff(lm.child_tok[lm.child_off[s]:lm.child_off[s + 1]]) > 0)
    n13, n34 = lm._node_of[(1, 3)], lm._node_of[(3, 4)]
    assert lm.bo[n13] == lm._node_of[(3,)] and lm.bo[lm._node_of[(3,)]] == 0 and lm.bo[0] == 0
    assert lm.step(0, SOS) == lm._node_of[(1,)] and lm.step(lm._node_of[(1,)], 3) == n13
    assert lm.step(n13, 4) == n34                                     # the trigram's next: the longest suffix that is a node
    assert lm.step(n13, 2) == lm._node_of[(3, 2)] and lm.step(n34, 4) == lm._node_of[(4,)]
    assert lm.step(n13, -1) == 0 and lm.step(n13, 5) == 0            # a token outside [0, V) goes to the root
    t = lm.tables(0.5)
    assert t["child_lp"].dtype == np.float32 and t["child_lp"][0] == np.float32(0.5 * math.log(10.0) * lm._lp64[0])
    assert NgramLM({(v,): (-1.0, 0.0) for v in range(5)}, 1, 5).num_nodes == 1               # order 1: M = 1, E = 0
    with pytest.raises(ValueError, match="order"):
        NgramLM(grams, 7, 5)
    with pytest.raises(ValueError, match="vocab_size"):
        NgramLM(grams, 3, NG.MAX_V + 1)
    with pytest.raises(ValueError, match=r"token 4 has no unigram"):
        NgramLM({k: v for k, v in grams.items() if k != (4,)}, 3, 5)
    with pytest.raises(ValueError, match=r"\(1, 3, 2\) is stored, its prefix \(1, 3\) is not"):
        NgramLM({k: v for k, v in grams.items() if k != (1, 3)}, 3, 5)
    with pytest.raises(ValueError, match="positive"):
        NgramLM({**grams, (2,): (0.5, 0.0)}, 3, 5)
    with pytest.raises(ValueError, match="not finite"):
        NgramLM({**grams, (2,): (float("nan"), 0.0)}, 3, 5)
    saved = NG.MAX_NODES
    try:
        NG.MAX_NODES = 8
        with pytest.raises(ValueError, match="nodes"):
            NgramLM(grams, 3, 5)
    finally:
        NG.MAX_NODES = saved
    filled = NgramLM({(2,): (-1.0, 0.0), (3,): (-1.0, 0.0)}, 2, 5, unk_logp=-2.5)            # <unk> fills what is missing
    assert filled.grams[(4,)] == (-2.5, 0.0) and filled.grams[(0,)] == (-2.5, 0.0)
    assert NgramLM({(v,): (-1.0, 0.0) for v in (2, 3, 4)}, 2, 5).grams[(1,)] == (-99.0, 0.0)  # PAD and SOS: -99


def _arpa(tmp_path, body, name="m.arpa"):
    f = tmp_path / name
    f.write_text(body)
    return str(f)


T2I = {"<PAD>": 0, "<SOS>": 1, "<EOS>": 2, "<SPACE>": 3, "A": 4, "B": 5}
I2T = {i: t for t, i in T2I.items()}
GOOD = "\\data\\\nngram 1=5\nngram 2=2\n\n\\1-grams:\n-99\t<s>\t-0.5\n-1\t</s>\n-0.5 <SPACE> -0.25\n-0.7\tA\n-0.8\tB\n\n\\2-grams:\n" \
       "-0.1\t<s> A\n-0.2\t<SPACE> B\n\n\\end\\\n"


def test_arpa_round_trip_and_refusals(tmp_path):
    rng = np.random.RandomState(5)
    grams = G.random_model(rng, 6, 3)
    path = str(tmp_path / "rt.arpa")
    write_arpa(path, grams, 3, I2T, SOS, EOS)
    lm = NgramLM.from_arpa(path, T2I, 6)
    assert lm.grams == grams and lm.order == 3                        # the same floats back
    write_arpa(str(tmp_path / "rt2.arpa"), lm.grams, lm.order, I2T, SOS, EOS)
    assert open(path).read() == open(str(tmp_path / "rt2.arpa")).read()
    lm = NgramLM.from_arpa(_arpa(tmp_path, GOOD), T2I, 6)
    assert lm.order == 2 and lm.grams[(1, 4)] == (-0.1, 0.0) and lm.grams[(3,)] == (-0.5, -0.25) and lm.grams[(0,)] == (-99.0, 0.0)
    # <unk>: fills the missing unigrams, higher-order n-grams that hold it are skipped (and counted)
    unk = GOOD.replace("-0.8\tB\n", "-3\t<unk>\n").replace("-0.2\t<SPACE> B", "-0.2\t<SPACE> <unk>")
    lm = NgramLM.from_arpa(_arpa(tmp_path, unk), T2I, 6)
    assert lm.grams[(5,)] == (-3.0, 0.0) and (3, 5) not in lm.grams and len([k for k in lm.grams if len(k) == 2]) == 1
    cases = [
        (GOOD.replace("ngram 2=2", "ngram 2=3"), r"line 12.*2 2-grams, the header says 3"),
        (GOOD.replace("-0.7\tA", "-0.7\tQ"), r"line 9.*unknown token 'Q'"),
        (GOOD.replace("-0.2\t<SPACE> B", "-0.1\t<s> A"), r"line 14.*duplicate"),
        (GOOD.replace("-0.7\tA", "nan\tA"), r"line 9.*not finite"),
        (GOOD.replace("-0.7\tA", "-0.7\tA\tinf"), r"line 9.*not finite"),
        (GOOD.replace("-0.7\tA", "0.7\tA"), r"line 9.*positive"),
        (GOOD.replace("-0.8\tB\n", "").replace("ngram 1=5", "ngram 1=4").replace("<SPACE> B", "B A"), r"line 13.*'B A' is stored, its prefix 'B' is not"),
        (GOOD.replace("ngram 2=2", "ngram 2=2\nngram 7=1"), r"line 4.*order 7"),
        (GOOD.replace("-0.7\tA", "-0.7\tA B C"), r"line 9.*fields"),
        (GOOD.replace("\\end\\", ""), r"cut short"),
    ]
    for k, (body, msg) in enumerate(cases):
        with pytest.raises(ValueError, match=msg):
            NgramLM.from_arpa(_arpa(tmp_path, body, "bad%d.arpa" % k), T2I, 6)
    with pytest.raises(ValueError, match=r"line 10.*id 5 outside \[0, 5\)"):
        NgramLM.from_arpa(_arpa(tmp_path, GOOD), T2I, 5)
    with pytest.raises(ValueError, match=r"token 5 has no unigram"):
        NgramLM.from_arpa(_arpa(tmp_path, GOOD.replace("-0.8\tB\n", "").replace("ngram 1=5", "ngram 1=4").replace("<SPACE> B", "<SPACE> A")), T2I, 6)
    with pytest.raises(ValueError, match="16384"):
        NgramLM.from_arpa(_arpa(tmp_path, GOOD), T2I, NG.MAX_V + 1)
    with pytest.raises(ValueError, match="no such file"):
        NgramLM.from_arpa(str(tmp_path / "absent.arpa"), T2I, 6)
    saved = NG.MAX_NODES
    try:
        NG.MAX_NODES = 4
        with pytest.raises(ValueError, match="nodes"):
            NgramLM.from_arpa(_arpa(tmp_path, GOOD), T2I, 6)
    finally:
        NG.MAX_NODES = saved


def _corpus(n_lines=200, seed=3):
    rng = np.random.RandomState(seed)
    words = ["THE", "CAT", "SAT", "ON", "A", "MAT", "AND", "RAN", "TO", "DOG"]
    return [" ".join(words[i] for i in rng.randint(len(words), size=rng.randint(2, 7))) for _ in range(n_lines)]


@pytest.mark.parametrize("order", [1, 2, 3])
def test_train_ngram_distributions_sum_to_one(tmp_path, order):
    """train_ngram.py on a 200-line synthetic corpus: for EVERY node (the root, every stored context) the probabilities of the V - 2
    tokens other than PAD and SOS sum to 1 within 1e-9 (Witten-Bell interpolation in back-off form), and the file parses back"""
    sys.path.insert(0, PKG)
    import train_ngram
    from utils.tokenizer import CharEncoder
    tok = CharEncoder()
    data, out = tmp_path / "text.txt", tmp_path / "lm.arpa"
    data.write_text("\n".join(_corpus()) + "\n\n")
    train_ngram.main(["--data_file", str(data), "--order", str(order), "--unit", "char", "--output", str(out)])
    lm = NgramLM.from_arpa(str(out), tok.token_to_id, 30)
    assert lm.order == order and lm.grams[(SOS,)][0] == -99.0 and lm.grams[(PAD,)] == (-99.0, 0.0)
    direct = train_ngram.estimate(train_ngram.encode_lines(_corpus(), tok, SOS), order, 30)
    assert {k: v for k, v in lm.grams.items() if k != (PAD,)} == direct
    assert order == 1 or lm.grams[(SOS,)][1] < 0                      # <s> keeps its back-off
    assert lm.num_nodes > (30 if order > 1 else 0)
    for node in lm.nodes:
        total = sum(10.0 ** G.logp64(lm.grams, node, v, order) for v in range(30) if v not in (PAD, SOS))
        assert abs(total - 1.0) < 1e-9, (node, total)
    with pytest.raises(ValueError, match="line 2"):
        train_ngram.encode_lines(["OK", "R2D2"], tok, SOS)


def test_flags_and_constructor_refusals(tmp_path):
    from las.arguments import parse_args
    a = parse_args([])
    assert a.ngram_lm == "" and a.ngram_weight == 0.0 and from_args(a) is None
    f = _arpa(tmp_path, GOOD.replace("<SPACE> B", "<SPACE> A").replace("-0.8\tB\n", "-3\t<unk>\n"))
    a = parse_args(["--unit", "char", "--ngram_lm", f, "--ngram_weight", "0.5"])
    a.vocab_size = 30
    lm = from_args(a)
    assert lm.order == 2 and lm.vocab_size == 30 and lm.grams[(29,)] == (-3.0, 0.0)
    a.ngram_weight = 0.0
    assert from_args(a) is None                                       # a file and weight 0: off
    a.ngram_weight, a.ngram_lm = 0.5, ""
    with pytest.raises(ValueError, match="--ngram_lm FILE"):
        from_args(a)
    a.ngram_lm = str(tmp_path / "absent.arpa")
    with pytest.raises(ValueError, match="no such file"):
        from_args(a)
    for w in (-1.0, float("nan"), float("inf")):
        a.ngram_weight = w
        with pytest.raises(ValueError, match="ngram_weight"):
            from_args(a)

    # the BeamSearch constructor refuses before it touches a device
    from las.beam_search import BeamSearch
    from utils.tokenizer import CharEncoder

    class _Las(object):
        listener = speller = None
    for kw, msg in ((dict(ngram_weight=0.5), "--ngram_lm FILE"), (dict(ngram_lm=str(tmp_path / "absent.arpa"), ngram_weight=0.5), "no such file"),
                    (dict(ngram_lm=f, ngram_weight=-0.5), "ngram_weight"), (dict(ngram_lm=f, ngram_weight=float("nan")), "ngram_weight")):
        a = parse_args(["--unit", "char", "--beam_size", "4"])
        a.vocab_size = 30
        for k, v in kw.items():
            setattr(a, k, v)
        with pytest.raises(ValueError, match=msg):
            BeamSearch(a, _Las(), CharEncoder().token_to_id, None)
    a = parse_args(["--unit", "char", "--beam_size", "4", "--ngram_lm", f, "--ngram_weight", "0.5"])
    a.vocab_size = 30
    bs = BeamSearch(a, _Las(), CharEncoder().token_to_id, None)
    assert bs.ngram is not None and bs.ngram_weight == 0.5
    bs.set_ngram(None, 0)
    assert bs.ngram is None and bs.ngram_weight == 0.0
    with pytest.raises(ValueError, match="vocabulary"):
        bs.set_ngram(NgramLM({(v,): (-1.0, 0.0) for v in range(5)}, 1, 5), 1.0)
    with pytest.raises(ValueError, match="weight"):
        bs.set_ngram(lm, -1.0)
    a.ngram_weight = 0.0
    assert BeamSearch(a, _Las(), CharEncoder().token_to_id, None).ngram is None
