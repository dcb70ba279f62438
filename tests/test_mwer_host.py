"""The MWER restatement (tests/mwer_ref.py) checked on the CPU against what it restates: central finite differences of its own float64
loss, an independent derivation through torch autograd, the zero sums the gradient must have, and hand-written word error counts."""
import numpy as np
import pytest
import torch

import helpers  # noqa: F401  (puts the package on sys.path)
import mwer_ref as M
import nbest_ref as NB


def _small(seed, equal=False):
    rng = np.random.RandomState(seed)
    n, K, U, V = 2, 3, 3, 5
    z = rng.randn(n * K, U, V) * 1.5
    y = rng.randint(0, V, size=(n * K, U)).astype(np.int32)
    lens = np.array([3, 2, 1, 3, 0, 2], np.int32)
    nhyp = np.array([3, 2], np.int32)
    err = np.array([0, 2, 5, 1, 3, 9], np.float32)
    if equal:
        err[:] = 2
    return dict(z=z, y=y, lens=lens, nhyp=nhyp, err=err, K=K)


@pytest.mark.parametrize("mode", [0, 1])
def test_float64_gradient_is_the_finite_difference_of_the_float64_loss(mode):
    """(a) mode 0: of the expected error count itself; mode 1: of the score-function surrogate (mwer_ref.surrogate64) -- the sampling
    estimate's loss, a mean of error counts, does not depend on the logits"""
    d = _small(3)
    scale = np.float32(0.5)
    g = M.mwer(d["z"], d["y"], d["lens"], d["nhyp"], d["err"], d["K"], mode, scale, np.float64)["dlogits"]
    eps, worst = 1e-6, 0.0
    for idx in np.ndindex(*d["z"].shape):
        zp, zm = d["z"].copy(), d["z"].copy()
        zp[idx] += eps
        zm[idx] -= eps
        fd = (M.surrogate64(zp, d["y"], d["lens"], d["nhyp"], d["err"], d["K"], mode, scale)
              - M.surrogate64(zm, d["y"], d["lens"], d["nhyp"], d["err"], d["K"], mode, scale)) / (2 * eps)
        worst = max(worst, abs(fd - g[idx]))
    print("mode", mode, "max |finite difference - gradient|", worst, "largest gradient", np.abs(g).max())
    assert np.abs(g).max() > 1e-2 and worst < 1e-8


@pytest.mark.parametrize("mode", [0, 1])
def test_float64_restatement_equals_torch_autograd(mode):
    """(b) log_softmax, a gather, a softmax over the live slots and the expected-risk formula, differentiated by autograd"""
    d = _small(4)
    scale = np.float32(0.25)
    ref = M.mwer(d["z"], d["y"], d["lens"], d["nhyp"], d["err"], d["K"], mode, scale, np.float64)
    z = torch.tensor(d["z"], dtype=torch.float64, requires_grad=True)
    lp = torch.log_softmax(z, -1)
    K = d["K"]
    total, seq_all = 0.0, {}
    for u, nh in enumerate(d["nhyp"]):
        rows = list(range(u * K, u * K + int(nh)))
        seq = torch.stack([sum((lp[r, t, int(d["y"][r, t])] for t in range(int(d["lens"][r]))), torch.zeros((), dtype=torch.float64)) for r in rows])
        e = torch.tensor(d["err"][rows], dtype=torch.float64)
        if mode == 0:
            post = torch.softmax(seq, 0)
            risk = (post * e).sum()
            total = total + risk
            assert np.allclose(post.detach().numpy(), ref["post"][rows], rtol=1e-12, atol=0)
        else:
            risk = e.mean()
            total = total + (((e - e.mean()) / len(rows)) * seq).sum()
        assert abs(float(risk.detach()) - ref["risk"][u]) < 1e-12
        for r, s in zip(rows, seq):
            seq_all[r] = float(s.detach())
    (float(scale) * total).backward()
    for r, s in seq_all.items():
        assert abs(s - ref["seq_lp"][r]) < 1e-12
    assert np.isnan(ref["seq_lp"][5]) and np.isnan(ref["post"][5])                # the absent slot of utterance 1: not written
    assert np.abs(z.grad.numpy() - ref["dlogits"]).max() < 1e-13
    if mode == 0:
        assert abs(float(scale) * float(total.detach()) - float(ref["loss"])) < 1e-13


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("ft", [np.float64, np.float32])
def test_gradient_rows_and_coefficients_sum_to_zero(mode, ft):
    """(c) softmax - onehot sums to 0 over the classes, post (err - Wbar) over the slots"""
    d = _small(5)
    o = M.mwer(d["z"].astype(np.float32), d["y"], d["lens"], d["nhyp"], d["err"], d["K"], mode, np.float32(1.0), ft)
    eps = 1e-6 if ft is np.float32 else 1e-15
    assert np.abs(o["dlogits"].astype(np.float64).sum(-1)).max() < eps * 5
    for u, nh in enumerate(d["nhyp"]):
        c = o["coef"][u * d["K"]:u * d["K"] + int(nh)].astype(np.float64)
        assert abs(c.sum()) < eps * 10 and np.abs(c).max() > 1e-5
    same = _small(5, equal=True)
    o = M.mwer(same["z"].astype(np.float32), same["y"], same["lens"], same["nhyp"], same["err"], same["K"], mode, np.float32(1.0), ft)
    assert (o["dlogits"] == 0).all() and (o["coef"][np.isfinite(o["coef"])] == 0).all()     # equal errors: exactly nothing to learn


def test_measured_tolerance_is_small_and_every_case_has_a_gradient():
    tol = M.measured_tolerance()
    print(tol)
    assert all(0 < tol[k] < 1e-4 for k in M.OUTPUTS)
    for case in M.CASES:
        o = M.run_case(case["name"])
        if not case.get("equal") and case["K"] > 1 and max(case["nhyp"]) > 1:
            assert np.abs(o["dlogits"]).max() > 1e-4, case["name"]


def test_word_errors_of_hand_written_examples():
    """(d) through the numpy Levenshtein distance of tests/nbest_ref.py"""
    from las import mwer
    from utils.tokenizer import CharEncoder
    enc = CharEncoder()
    t = lambda s, eos=True: enc.encode(s, eos)
    ref = [t("THE CAT SAT"), t("A B")]
    hyps = [[t("THE CAT SAT"), t("THE BAT SAT"), t("CAT SAT") + t("JUNK AFTER THE END"), t("THE CAT SAT ON IT", False), t("THECAT SAT")],
            [t(""), t("A B C")]]
    err = mwer.word_errors(ref, hyps, enc.id_to_token, "char", "word", distance=NB.distance)
    assert [e.tolist() for e in err] == [[0, 1, 1, 2, 2], [2, 1]]
    err = mwer.word_errors(ref, hyps, enc.id_to_token, "char", "token", distance=NB.distance)
    assert [e.tolist() for e in err] == [[0, 1, 4, 6, 1], [3, 2]]
    sub = {0: "<PAD>", 1: "<SOS>", 2: "<EOS>", 3: "th", 4: "e</w>", 5: "cat</w>", 6: "c", 7: "at</w>", 8: "dog</w>"}
    ref = [[3, 4, 5, 2]]                                                         # "the cat"
    hyps = [[[3, 4, 6, 7, 2], [3, 4, 8], [5, 2, 8, 8], []]]                       # another spelling of it; "the dog"; "cat"; nothing
    err = mwer.word_errors(ref, hyps, sub, "subword", "word", distance=NB.distance)
    assert err[0].tolist() == [0, 1, 1, 2]
    err = mwer.word_errors(ref, hyps, sub, "subword", "token", distance=NB.distance)
    assert err[0].tolist() == [2, 1, 2, 3]
    with pytest.raises(ValueError, match="id_to_token"):
        mwer.word_errors(ref, hyps, {}, "subword", "word", distance=NB.distance)


def test_flags_and_refusals():
    from las import mwer
    from las.arguments import parse_args
    a = parse_args([])
    assert (a.mwer, a.mwer_hyps, a.mwer_ce_weight, a.mwer_unit, a.mwer_norm, a.mwer_extra_steps) == (False, 4, 0.01, "word", "", 4)
    a = parse_args(["--mwer", "True", "--mwer_hyps", "2", "--mwer_unit", "token", "--mwer_norm", "nbest"])
    assert mwer.check_flags(a) == (2, "token", "nbest")
    for flags, msg in ((["--mwer_hyps", "64"], "between 1 and 63"), (["--mwer_hyps", "0"], "between 1 and 63"), (["--ctc", "True"], "--ctc"),
                       (["--mwer_unit", "char"], "word or token"), (["--mwer_norm", "all"], "sample or nbest"),
                       (["--mwer_extra_steps", "-1"], "not negative")):
        with pytest.raises(ValueError, match=msg):
            mwer.check_flags(parse_args(["--mwer", "True"] + flags))
    with pytest.raises(ValueError, match="data-parallel"):
        mwer.check_flags(a, dp=object())
