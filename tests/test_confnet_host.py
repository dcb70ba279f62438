"""N-best confusion networks, host side: the numpy restatement tests/confnet_ref.py against the properties of the
construction and hand-made cases; las.nbest's word symbols and bins; the new flags and their refusals.  Nothing here needs a GPU."""
import argparse

import numpy as np
import pytest

import helpers  # noqa: F401
import confnet_ref as C
import nbest_ref as R
from las import align as A
from las import nbest as NB
from las.arguments import check_confusion_flags, parse_args
from utils.tokenizer import CharEncoder

a, b, c, d, e, x, y = 1, 2, 3, 4, 5, 6, 7
EPS = C.EPS


def _rand_utt(rng, vocab, max_len, max_nh):
    hyps = [list(rng.randint(0, vocab, size=rng.randint(0, max_len + 1))) for _ in range(rng.randint(1, max_nh + 1))]
    w = rng.uniform(0.01, 1.0, size=len(hyps))
    return hyps, (w / w.sum()).astype(np.float32)


def _consensus(net):
    return [int(s) for s in net["best"] if s != EPS]


def test_one_hypothesis_gives_its_tokens_as_bins():
    for h in ([4, 9, 4, 7], [5], []):
        net = C.network([h], [0.7], 16)
        assert net["nbins"] == len(h) and list(net["cols"][0]) == h and list(net["best"]) == h and list(net["merged"]) == [1]
        assert np.all(net["post"] == np.float32(0.7))


def test_identical_hypotheses_give_the_same_bins_with_the_summed_mass():
    h = [3, 1, 4, 1, 5]
    w = np.asarray([0.5, 0.25, 0.125], np.float32)                     # (sums exact in fp32)
    net = C.network([h, h, h], w, 16)
    assert net["nbins"] == 5 and all(list(r) == h for r in net["cols"]) and list(net["best"]) == h
    assert np.all(net["post"] == np.float32(0.875)) and net["costs"][1:] == [0, 0]


def test_merging_the_second_hypothesis_costs_their_edit_distance():
    """bins of one symbol without EPS: has() is token equality and cup is 1, the table is Levenshtein's"""
    rng = np.random.RandomState(0)
    for vocab in (2, 3, 50):
        for _ in range(60):
            hyps, w = _rand_utt(rng, vocab, 14, 2)
            if len(hyps) == 2:
                assert C.network(hyps, w, 64)["costs"][1] == R.distance(hyps[0], hyps[1])


def test_rows_without_eps_are_the_hypotheses_and_masses_add_up():
    rng = np.random.RandomState(1)
    for vocab in (2, 3, 40):
        for _ in range(50):
            hyps, w = _rand_utt(rng, vocab, 12, 6)
            net = C.network(hyps, w, 128, mode="f64")
            assert list(net["merged"]) == [1] * len(hyps) and net["cols"].shape == (len(hyps), net["nbins"])
            for k, h in enumerate(hyps):
                assert [int(s) for s in net["cols"][k] if s != EPS] == h
            total = np.float64(0)
            for k in range(len(hyps)):
                total += np.float64(w[k])
            for i in range(net["nbins"]):
                m = C.masses(net["cols"], net["merged"], w, i)
                assert sum(m.values()) == pytest.approx(total, rel=1e-12)
                assert net["post"][i] == max(m.values()) and m[int(net["best"][i])] == net["post"][i]
            # the literal table and its row-at-a-time form
            syms = [set(int(s) for s in net["cols"][:, i]) for i in range(net["nbins"])]
            probe = list(rng.randint(0, vocab, size=7))
            assert np.array_equal(C.table(syms, probe), C.table_literal(syms, probe))


def test_hand_made_case_1():
    hyps = [[a, b, c], [a, c], [a, x, c]]
    net = C.network(hyps, [0.4, 0.35, 0.25], 8)
    assert net["cols"].tolist() == [[a, b, c], [a, EPS, c], [a, x, c]]         # bins [a] [b, EPS, x] [c]
    assert _consensus(net) == [a, b, c]
    net = C.network(hyps, [0.3, 0.45, 0.25], 8)
    assert net["cols"].tolist() == [[a, b, c], [a, EPS, c], [a, x, c]] and _consensus(net) == [a, c]


def test_hand_made_case_2_the_consensus_is_no_listed_hypothesis():
    hyps = [[a, b, c, d], [a, x, c, y], [e, b, c, y]]
    net = C.network(hyps, [0.4, 0.3, 0.3], 8)
    assert _consensus(net) == [a, b, c, y] and _consensus(net) not in hyps


def test_the_tie_rule():
    """equal masses: the symbol whose first contributing slot is lower wins -- also when that symbol is EPS"""
    q = np.float32(0.25)
    net = C.network([[a, b], [a, x], [a, x], [a, b]], [q, q, q, q], 8)
    assert list(net["best"]) == [a, b] and net["post"][1] == np.float32(0.5)
    net = C.network([[a, x], [a, b], [a, b], [a, x]], [q, q, q, q], 8)
    assert list(net["best"]) == [a, x]
    net = C.network([[a], [a, b]], [0.5, 0.5], 8)                     # EPS (slot 0) against b (slot 1)
    assert net["cols"].tolist() == [[a, EPS], [a, b]] and list(net["best"]) == [a, EPS]
    net = C.network([[a, b], [a]], [0.5, 0.5], 8)
    assert list(net["best"]) == [a, b]
    net = C.network([[a, b], [a], [a]], [0.4, 0.3, 0.3], 8)           # a larger mass beats the earlier slot
    assert list(net["best"]) == [a, EPS]


def test_the_overflow_rule():
    hyps = [[1, 2, 3, 4, 5], [1, 2, 3], [1, 9, 3, 4], [7, 7, 1, 2, 3, 4], [1, 2, 3, 4]]
    w = np.asarray([0.3, 0.25, 0.2, 0.15, 0.1], np.float32)
    net = C.network(hyps, w, 4)                                        # hypothesis 0 is longer than max_bins
    assert list(net["merged"]) == [0, 1, 1, 0, 1] and net["nbins"] == 4
    assert net["cols"][[1, 2, 4]].tolist() == [[1, 2, 3, EPS], [1, 9, 3, 4], [1, 2, 3, 4]]
    assert list(net["best"]) == [1, 2, 3, 4]
    assert net["post"][1] == np.float32(np.float32(0.25) + np.float32(0.1)) and net["post"][3] == np.float32(np.float32(0.2) + np.float32(0.1))
    # the network of the merged ones alone is the same: a hypothesis that is left out leaves no trace
    alone = C.network([hyps[1], hyps[2], hyps[4]], w[[1, 2, 4]], 4)
    assert np.array_equal(alone["cols"], net["cols"][[1, 2, 4]]) and np.array_equal(alone["post"], net["post"])
    assert C.network(hyps, w, 6)["merged"].tolist() == [1, 1, 1, 0, 1]


ID_TO_TOKEN = {0: "<PAD>", 1: "<SOS>", 2: "<EOS>", 3: "he", 4: "llo</w>", 5: "a</w>", 6: "wor", 7: "ld</w>", 8: "tail", 9: "hello</w>",
               10: "h", 11: "ello</w>", 12: "</w>"}


def test_word_symbols_segment_like_align_words():
    tok = CharEncoder()
    sp, eos = tok.token_to_id["<SPACE>"], tok.token_to_id["<EOS>"]
    enc = lambda s: tok.encode(s, with_eos=False)
    cases = [(tok.id_to_token, "char", [enc("HELLO WORLD"), [sp, sp] + enc("A") + [sp, sp, sp] + enc("BC") + [sp], enc("HELLO A") + [eos] +
                                        enc("X"), [], [sp], enc("WORLD HELLO")]),
             (ID_TO_TOKEN, "subword", [[3, 4, 5, 6, 7], [9, 5, 6, 7, 8], [10, 11, 2, 5], [8], [5, 5, 5], [], [3, 4, 12, 5]])]
    for id_to_token, unit, hyps in cases:
        (sl,), (words,) = NB.word_symbols([hyps], id_to_token, unit)
        seen = []
        for h, row in zip(hyps, sl):
            want = [w["word"] for w in A.words(h, [(0, 0)] * len(h), id_to_token, unit, 1.0, 1e9)]
            assert [words[s][0] for s in row] == want
            for s in row:
                if s not in seen:
                    seen.append(s)
        assert seen == list(range(len(words)))                         # ids in order of first appearance, best hypothesis first
        assert len(set(t for t, _ in words)) == len(words)             # one id per printed text
    (sl,), (words,) = NB.word_symbols([[[3, 4, 5], [9, 5], [10, 11]]], ID_TO_TOKEN, "subword")
    assert sl == [[0, 1], [0, 1], [0]] and words == [("hello", (3, 4)), ("a", (5,))]     # three segmentations of one word agree
    (sl,), (words,) = NB.word_symbols([[[3, 4, 5], [9]]], ID_TO_TOKEN, "token")
    assert sl == [[3, 4, 5], [9]] and words[9] == ("hello</w>", (9,))
    sl, words = NB.word_symbols([[enc("AB")], [enc("CD AB")]], tok.id_to_token, "char")      # ids are per utterance
    assert sl == [[[0]], [[0, 1]]] and words[0][0][0] == "AB" and words[1][0][0] == "CD"


def test_bins_list_the_alternatives_under_the_tie_rule():
    net = C.network([[0, 1, 2], [0, 2], [0, 3, 2]], [0.4, 0.35, 0.25], 8)
    words = [("flour", (5,)), ("the", (6,)), ("rises", (7,)), ("flower", (8,))]
    w = np.asarray([0.4, 0.35, 0.25], np.float32)
    got = NB.bins(net, w, words, 3)
    assert [[e["word"] for e in bin_] for bin_ in got] == [["flour"], ["the", "", "flower"], ["rises"]]
    assert got[1][0]["p"] == float(np.float32(0.4)) and got[1][1]["p"] == float(np.float32(0.35))
    assert [[e["word"] for e in bin_] for bin_ in NB.bins(net, w, words, 1)] == [["flour"], ["the"], ["rises"]]
    for i, bin_ in enumerate(NB.bins(net, w, words, 8)):               # the first alternative is best / post
        assert bin_[0]["p"] == float(net["post"][i])
    q = np.float32(0.25)
    tie = C.network([[0], [1], [1], [0]], [q, q, q, q], 8)
    assert [e["word"] for e in NB.bins(tie, [q] * 4, words, 2)[0]] == ["flour", "the"]


def test_flags_defaults_and_refusals():
    args = parse_args([])
    assert args.confusion_network is False and args.cn_decode is False and args.cn_alternatives == 3 and args.cn_unit == "word"
    assert check_confusion_flags(args) is False and not NB.Annotator(args, 2).active
    on = ["--confusion_network", "True"]
    args = parse_args(on + ["--cn_decode", "True", "--cn_alternatives", "8", "--cn_unit", "token"])
    assert args.confusion_network is True and args.cn_decode is True and args.cn_alternatives == 8 and args.cn_unit == "token"
    assert check_confusion_flags(args) is True
    ann = NB.Annotator(args, 2, ID_TO_TOKEN)
    assert ann.active and ann.cn and ann.cn_decode and ann.cn_top == 8 and ann.cn_unit == "token"
    with pytest.raises(ValueError, match="id_to_token"):
        NB.Annotator(args, 2)

    def ns(argv, **more):
        n = parse_args(argv)
        for k, v in dict(dict(keywords=None, timestamps=False, align_text=None), **more).items():     # (transcribe.py's own flags)
            setattr(n, k, v)
        return n
    for n, text in ((ns(["--cn_decode", "True", "--mbr", "True"]), "--mbr"),
                    (ns(["--cn_decode", "True"], timestamps=True), "--timestamps"),
                    (ns(["--cn_decode", "True"], align_text="refs.txt"), "--align_text"),
                    (ns(on, keywords="names.txt"), "--keywords"),
                    (ns(["--cn_decode", "True"], keywords="names.txt"), "--keywords"),
                    (ns(on + ["--cn_alternatives", "0"]), "--cn_alternatives"),
                    (ns(on + ["--cn_alternatives", "9"]), "--cn_alternatives"),
                    (ns(["--cn_decode", "True", "--cn_unit", "phone"]), "--cn_unit")):
        with pytest.raises(ValueError, match=text):
            check_confusion_flags(n)
        with pytest.raises(ValueError, match=text):
            NB.Annotator(n, 2, ID_TO_TOKEN)
    # --confusion_network alone goes with --mbr and --timestamps; without the two flags nothing is refused
    assert check_confusion_flags(ns(on + ["--mbr", "True"], timestamps=True)) is True
    assert check_confusion_flags(ns(["--mbr", "True", "--cn_alternatives", "99", "--cn_unit", "phone"], keywords="k", timestamps=True)) is False


class _State(object):
    def __init__(self, token_ids, log_prob):
        self.token_ids, self.log_prob = token_ids, np.float32(log_prob)


def test_annotator_without_the_new_flags_returns_what_it_returned():
    """a namespace from before the flags (none of the four attributes): the dicts of --nbest alone, key for key, and no launch (this
    test runs without a GPU)"""
    full = parse_args(["--nbest", "2", "--beam_size", "4"])
    bare = argparse.Namespace(**{k: v for k, v in vars(full).items() if not k.startswith("cn_") and k != "confusion_network"})
    results = [[_State([1, 7, 8, 2], -3.0), _State([1, 7, 9, 2], -1.0)], [], [_State([1, 5, 2, 6], -0.5)]]
    for args in (bare, full):
        ann = NB.Annotator(args, 2)
        assert ann.active and not ann.cn and not ann.cn_decode
        out = ann.annotate(results)
        assert [sorted(o) for o in out] == [["conf", "index", "nbest", "posterior", "state", "tokens"]] * 3
        assert out[0]["index"] == 0 and out[0]["state"] is results[0][1] and out[0]["tokens"] == [7, 9] and out[0]["conf"] == []
        assert [t for t, _, _ in out[0]["nbest"]] == [[7, 9], [7, 8]] and out[0]["nbest"][0][2] == out[0]["posterior"]
        assert out[1] == dict(index=-1, state=None, tokens=[], posterior=None, conf=[], nbest=[])
        assert out[2]["tokens"] == [5] and out[2]["posterior"] == 1.0
