"""Two-pass decoding on the CPU: the restatement tests/rescore_ref.py against torch's log-softmax, its edge values, the
re-ranking rules, the margins and shapes of the device case lists, and the flags' refusals (las.ctc_search.check_args)."""
import numpy as np
import pytest
import torch

import rescore_ref as R
from helpers import make_args

EOS = 2


def test_scored_string_rule():
    assert R.scored_string([5, 6, EOS, 7, EOS], EOS) == [5, 6, EOS]              # EOS inside: through the first one
    assert R.scored_string([5, 6, EOS], EOS) == [5, 6, EOS]                      # at the end: as it is
    assert R.scored_string([5, 6], EOS) == [5, 6, EOS]                           # absent: appended
    assert R.scored_string([], EOS) == [EOS]                                     # the empty hypothesis scores [EOS]
    assert R.scored_string([EOS], EOS) == [EOS]
    from las import rescore                                                      # (the module's rule is the same one)
    for toks in ([5, 6, EOS, 7, EOS], [5, 6, EOS], [5, 6], [], [EOS], np.array([4, 4, 4])):
        assert rescore.scored_string(toks, EOS) == R.scored_string(toks, EOS)


def test_scores_equal_torch_log_softmax_in_float64():
    rng = np.random.RandomState(0)
    for Rr, U, V in ((1, 1, 2), (4, 5, 31), (3, 7, 300)):
        z = (rng.randn(Rr, U, V) * 3).astype(np.float32)
        y = rng.randint(0, V, size=(Rr, U + 2)).astype(np.int32)
        lens = rng.randint(0, U + 1, size=Rr)
        lens[0] = U
        att, terms = R.scores(z, y, lens)
        lp = torch.log_softmax(torch.tensor(z, dtype=torch.float64), -1).gather(2, torch.tensor(y[:, :U]).long()[..., None])[..., 0].numpy()
        for r in range(Rr):
            L = int(lens[r])
            assert np.allclose(terms[r, :L], lp[r, :L], rtol=0, atol=1e-12)
            assert np.isnan(terms[r, L:]).all()
            assert abs(att[r] - lp[r, :L].sum()) <= 1e-11
        a32, t32 = R.scores(z, y, lens, np.float32)                              # the float32 mode: the same numbers to float32 accuracy
        assert t32.dtype == np.float32 and np.nanmax(np.abs(t32 - terms)) < 1e-5 and np.abs(a32 - att).max() < 1e-4


def test_scores_edge_values():
    z = np.zeros((4, 2, 5), np.float32)
    z[0, :, 1:3] = -np.inf                                                       # -inf columns beside the label: finite
    z[1, 0, 3] = -np.inf                                                         # ... under the label: -inf
    z[2, 1, :] = -np.inf                                                         # a step without mass: -inf, not NaN
    y = np.array([[0, 4], [3, 0], [0, 0], [5, -1]], np.int32)                    # row 3: labels outside [0, V)
    for ft in (np.float64, np.float32):
        att, terms = R.scores(z, y, [2, 2, 2, 2], ft)
        assert np.allclose(terms[0], -np.log(3.0), atol=1e-6) and np.isfinite(att[0])
        assert np.isneginf(terms[1, 0]) and np.isfinite(terms[1, 1]) and np.isneginf(att[1])
        assert np.isfinite(terms[2, 0]) and np.isneginf(terms[2, 1]) and np.isneginf(att[2])
        assert np.isneginf(terms[3]).all() and np.isneginf(att[3])
        assert not np.isnan(att).any()
        att0, _ = R.scores(z, y, [0, 0, 0, 0], ft)                               # nothing scored: 0
        assert (att0 == 0).all()
    att, _ = R.scores(z, y, [-3, 9, 1, 1])                                       # lengths are clamped to [0, U]
    assert att[0] == 0 and np.isneginf(att[1])


def test_rank_rules():
    first = np.array([-1.0, -2.0, -3.0, -4.0], np.float32)
    att = np.array([-9.0, -2.5, -7.0, -1.0])
    assert R.rank(first, att, 1.0)[1] == [0, 1, 2, 3]                            # w = 1: the first pass' order
    assert R.rank(first, att, 0.0)[1] == [3, 1, 2, 0]                            # w = 0: by att
    tot, order = R.rank(first, att, 0.3)
    assert tot.dtype == np.float32 and np.array_equal(tot, (0.7 * att + 0.3 * first.astype(np.float64)).astype(np.float32))
    assert order == sorted(range(4), key=lambda k: -tot[k])
    first = np.array([-1.0, -5.0, -1.0, -5.0], np.float32)                       # exact ties go to the lower slot
    att = np.array([-2.0, -1.0, -2.0, -1.0])
    assert R.rank(first, att, 0.5)[1] == [0, 2, 1, 3]
    att = np.array([np.nan, -1.0, np.nan, -50.0])                                # NaN comes last, in slot order
    assert R.rank(first, att, 0.5)[1] == [1, 3, 0, 2]
    att = np.array([-np.inf, -1.0, -np.inf, -50.0])                              # -inf ranks below every number, ties to the lower slot
    assert R.rank(first, att, 0.5)[1] == [1, 3, 0, 2]
    assert R.rank(first[:0], att[:0], 0.5)[1] == []


def test_every_device_case_keeps_its_margin():
    """the case lists of tests/test_gpu_rescore.py: adjacent float64 totals lie at least MARGIN apart, apart from the arranged exact ties;
    the lists cover the shapes the kernel branches on; the float32 restatement ranks as the float64 one, and the largest float32 -
    float64 differences are what the device tolerance is 4x of (printed: DESIGN 7o quotes them)"""
    for case in R.SCORE_CASES:
        d = R.case_data(case["name"])
        att, terms, tot, order = R.run_case(case["name"])
        m = R.margin(R.totals64(d["first"], att, R.CASE_W))
        print(case["name"], "margin", m)
        assert m >= R.MARGIN, (case["name"], m)
        assert case["ldy"] > case["U"] and d["lens"].max() == case["U"] and (case["R"] < 2 or d["lens"].min() == 0)
        if case["R"] >= 5:
            assert np.isfinite(att[[0, 2]]).all() and np.isneginf(att[[3, 4]]).all() and not np.isnan(att).any()
            assert np.isneginf(d["z"][2]).any() and np.abs(d["z"][0]).min() > 9e3
    assert {c["R"] for c in R.SCORE_CASES} == {1, 5, 37} and {c["U"] for c in R.SCORE_CASES} == {1, 2, 9}
    Vs = {c["V"] for c in R.SCORE_CASES}
    assert Vs >= {2, 3, 31, 257, 5001, 16384} and min(v for v in Vs if v > R.REGS_CLASSES) == R.REGS_CLASSES + 1 and R.REGS_CLASSES - 1 in Vs
    assert {c["layout"] for c in R.SCORE_CASES} == {"tm", "bm"}
    for case in R.RANK_CASES:
        d = R.rank_case_data(case["name"])
        for w in R.RANK_WEIGHTS:
            for u, nh in enumerate(d["nhyp"]):
                m = R.margin(R.totals64(d["first"][u, :nh], d["att"][u, :nh], w), d["ties"].get(u, ()))
                assert m >= R.MARGIN, (case["name"], w, u, m)
        if case["K"] >= 2:
            tot, order = R.rank(d["first"][0, :d["nhyp"][0]], d["att"][0, :d["nhyp"][0]], 0.3)
            assert order.index(0) + 1 == order.index(case["K"] - 1)             # the arranged tie: the lower slot, then its twin
        if case["K"] >= 16:
            assert order[-1] == 5                                                # the NaN slot
    assert {c["K"] for c in R.RANK_CASES} == {1, 2, 16, 64} and all(0 in c["nhyp"] for c in R.RANK_CASES)
    step_tol, att_tol = R.measured_tolerance()
    print("float32 restatement against float64: step terms %.3g, att / totals %.3g" % (step_tol, att_tol))
    assert 0 < step_tol < 1e-2 and 0 < att_tol < 1e-1


def test_flag_refusals():
    from las import ctc_search as CS
    a = make_args()
    assert (a.rescore, a.rescore_ctc_weight, a.rescore_rows) == ("none", 0.5, 64)
    assert CS.check_args(a) is False                                             # the default: nothing of this runs
    ok = dict(decoder="ctc", ctc=True, beam_size=4, rescore="attention")
    assert CS.check_args(make_args(**ok)) is True
    assert CS.check_args(make_args(**dict(ok, rescore="none", beam_size=1))) is True
    for w in (0.0, 1.0):
        assert CS.check_args(make_args(**dict(ok, rescore_ctc_weight=w))) is True
    for rows in (1, 1024):
        assert CS.check_args(make_args(**dict(ok, rescore_rows=rows))) is True
    for bad, msg in ((dict(decoder="attention"), "--decoder ctc"), (dict(beam_size=1), "--beam_size 1"),
                     (dict(rescore_ctc_weight=-0.1), "--rescore_ctc_weight"), (dict(rescore_ctc_weight=1.5), "--rescore_ctc_weight"),
                     (dict(rescore_ctc_weight=float("nan")), "--rescore_ctc_weight"),
                     (dict(rescore_ctc_weight=float("inf")), "--rescore_ctc_weight"), (dict(rescore="lm"), "--rescore"),
                     (dict(rescore_rows=0), "--rescore_rows"), (dict(rescore_rows=1025), "--rescore_rows"), (dict(ctc=False), "--ctc True")):
        with pytest.raises(ValueError, match=msg):
            CS.check_args(make_args(**dict(ok, **bad)))
    from las import rescore
    for w in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError, match="weight"):
            rescore.rerank([[0.0]], [[0.0]], w)
    with pytest.raises(ValueError, match="rows"):
        list(rescore.teacher_forced_logits(None, [None], [1], [[[EOS]]], rows=0))
