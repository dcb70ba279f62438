"""Two-pass decoding: las_rescore_score and las_rescore_rank through the C ABI against the numpy restatement
(tests/rescore_ref.py) on the same logits.  The order is EQUAL; step terms, att and totals are within 4x the largest difference between
the restatement in float32 with the kernel's operation order and in float64, measured on the CPU over the case list
(rescore_ref.measured_tolerance) -- the factor covers the device's expf / logf against numpy's.  -inf is -inf on both sides.  Every
output buffer is filled with sentinels (NaN in the float ones): what lies beyond a length, nhyp[u] or U must keep them, and the logits
of steps nobody may read are NaN."""
import numpy as np
import pytest
import torch

import rescore_ref as R

pytestmark = pytest.mark.gpu
SENT = -7


def _score(z, y, lens, layout, steps=True, ws_bytes=None, expect_fail=None, U=None, ldy=None):
    """las_rescore_score over z [R, U, V] laid out time-major (tm: [U, R, V], sb = V, st = R V) or batch-major (bm) -> (att [R + 1],
    step_lp [R, ldy] or None) as numpy, sentinels where nothing was written"""
    from las import _hip
    lib = _hip.lib()
    Rr, Uz, V = z.shape
    U = Uz if U is None else U
    y = np.ascontiguousarray(y, np.int32)
    ldy = y.shape[1] if ldy is None else ldy
    zz = np.array(z, np.float32, copy=True)
    for r in range(Rr):
        zz[r, max(0, min(int(lens[r]), Uz)):] = np.nan                          # nobody may read a step at or beyond the row's length
    if layout == "tm":
        dz = torch.as_tensor(np.ascontiguousarray(zz.transpose(1, 0, 2))).cuda()
        sb, st = V, Rr * V
    else:
        dz = torch.as_tensor(zz).cuda()
        sb, st = Uz * V, V
    dy, dl = torch.as_tensor(y).cuda(), torch.as_tensor(np.asarray(lens, np.int32)).cuda()
    att = torch.full((Rr + 1,), float("nan"), dtype=torch.float64, device="cuda")
    sl = torch.full((Rr, y.shape[1]), float("nan"), device="cuda") if steps else None
    need = lib.las_rescore_workspace_bytes(Rr, U)
    ws = None if steps else torch.zeros(max(need, 8), dtype=torch.uint8, device="cuda")
    rc = lib.las_rescore_score(_hip.p(dz), sb, st, _hip.p(dy), ldy, _hip.p(dl), Rr, U, V, _hip.p(att), _hip.p(sl), _hip.p(ws),
                               (0 if steps else need) if ws_bytes is None else ws_bytes, _hip.stream())
    if expect_fail is not None:
        assert rc < 0 and expect_fail in lib.las_last_error().decode(), (rc, lib.las_last_error())
        return None
    _hip.check(rc, "las_rescore_score")
    torch.cuda.synchronize()
    return att.cpu().numpy(), (sl.cpu().numpy() if steps else None)


def _rank(first, att, nhyp, w, K=None, expect_fail=None):
    """las_rescore_rank over [n, K] -> (total, order) as numpy, sentinels where nothing was written"""
    from las import _hip
    lib = _hip.lib()
    n, Kk = first.shape
    K = Kk if K is None else K
    df, da = torch.as_tensor(np.ascontiguousarray(first, np.float32)).cuda(), torch.as_tensor(np.ascontiguousarray(att, np.float64)).cuda()
    dn = torch.as_tensor(np.asarray(nhyp, np.int32)).cuda()
    tot = torch.full((n, Kk), float("nan"), device="cuda")
    order = torch.full((n, Kk), SENT, dtype=torch.int32, device="cuda")
    rc = lib.las_rescore_rank(_hip.p(df), _hip.p(da), _hip.p(dn), n, K, float(w), _hip.p(tot), _hip.p(order), _hip.stream())
    if expect_fail is not None:
        assert rc < 0 and expect_fail in lib.las_last_error().decode(), (rc, lib.las_last_error())
        return None
    _hip.check(rc, "las_rescore_rank")
    torch.cuda.synchronize()
    return tot.cpu().numpy(), order.cpu().numpy()


def _close(got, ref, tol, what):
    """finite where the restatement is finite and within tol; -inf where it is -inf; -> the largest deviation"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.array_equal(np.isneginf(got), np.isneginf(ref)) and not np.isnan(got).any() and not np.isposinf(got).any(), what
    fin = np.isfinite(ref)
    d = float(np.abs(got[fin] - ref[fin]).max()) if fin.any() else 0.0
    print(what, "max |device - float64|", d, "allowed", tol)
    assert d <= tol, (what, d, tol)
    return d


@pytest.mark.parametrize("name", [c["name"] for c in R.SCORE_CASES])
def test_score_cases_match_the_restatement(name):
    case = next(c for c in R.SCORE_CASES if c["name"] == name)
    d = R.case_data(name)
    step_tol, att_tol = (4.0 * t for t in R.measured_tolerance())
    att64, terms64, tot64, order64 = R.run_case(name)
    Rr, U = case["R"], case["U"]
    att, sl = _score(d["z"], d["y"], d["lens"], case["layout"], steps=True)
    assert np.isnan(att[Rr])                                                     # the sentinel behind the last row
    _close(att[:Rr], att64, att_tol, name + " att")
    for r in range(Rr):
        L = int(d["lens"][r])
        _close(sl[r, :L], terms64[r, :L], step_tol, "%s row %d steps" % (name, r))
        assert np.isnan(sl[r, L:]).all(), (name, r)                              # beyond the length and beyond U: not written
        s = 0.0
        for x in sl[r, :L]:
            s += float(x)
        assert att[r] == s or (np.isneginf(att[r]) and np.isneginf(s)), (name, r)   # att IS the float64 sum of the float32 terms, in order
    assert (att[:Rr][d["lens"] == 0] == 0).all()
    # without step_lp the terms pass through the workspace: the same bits
    att_ws, none = _score(d["z"], d["y"], d["lens"], case["layout"], steps=False)
    assert none is None and att_ws.tobytes() == att.tobytes()
    # the same bits twice
    att2, sl2 = _score(d["z"], d["y"], d["lens"], case["layout"], steps=True)
    assert att2.tobytes() == att.tobytes() and sl2.tobytes() == sl.tobytes()
    # the other layout reads the same values
    att3, sl3 = _score(d["z"], d["y"], d["lens"], "bm" if case["layout"] == "tm" else "tm", steps=True)
    assert att3.tobytes() == att.tobytes() and sl3.tobytes() == sl.tobytes()
    # the rows ranked as one utterance from the DEVICE's att: the restatement's order (the case keeps MARGIN), its totals
    tot, order = _rank(d["first"][None], att[None, :Rr], [Rr], R.CASE_W)
    assert order[0].tolist() == order64, name
    _close(tot[0], tot64, att_tol, name + " totals")
    # a permuted batch permutes the results
    perm = np.random.RandomState(5).permutation(Rr)
    att_p, sl_p = _score(d["z"][perm], d["y"][perm], d["lens"][perm], case["layout"], steps=True)
    assert att_p[:Rr].tobytes() == att[:Rr][perm].tobytes() and sl_p.tobytes() == sl[perm].tobytes()


@pytest.mark.parametrize("name", [c["name"] for c in R.RANK_CASES])
def test_rank_cases_match_the_restatement(name):
    case = next(c for c in R.RANK_CASES if c["name"] == name)
    d = R.rank_case_data(name)
    _, att_tol = (4.0 * t for t in R.measured_tolerance())
    n, K = len(d["nhyp"]), case["K"]
    for w in R.RANK_WEIGHTS:
        tots, orders = R.rank_batch(d["first"], d["att"], d["nhyp"], w)
        tot, order = _rank(d["first"], d["att"], d["nhyp"], w)
        for u in range(n):
            nh = int(d["nhyp"][u])
            assert order[u, :nh].tolist() == orders[u], (name, w, u)
            assert (order[u, nh:] == SENT).all() and np.isnan(tot[u, nh:]).all(), (name, w, u)     # slots at and beyond nhyp: not written
            nan = np.isnan(tots[u])
            assert np.array_equal(np.isnan(tot[u, :nh]), nan), (name, w, u)
            if (~nan).any():
                dev = float(np.abs(tot[u, :nh][~nan].astype(np.float64) - tots[u][~nan].astype(np.float64)).max())
                print(name, "w", w, "utterance", u, "max |device - restatement| totals", dev, "allowed", att_tol)
                assert dev <= att_tol
        if K >= 2 and w == 0.3:
            o = order[0, :d["nhyp"][0]].tolist()
            assert o.index(0) + 1 == o.index(K - 1)                              # the arranged tie: the lower slot first
        tot2, order2 = _rank(d["first"], d["att"], d["nhyp"], w)
        assert tot2.tobytes() == tot.tobytes() and order2.tobytes() == order.tobytes()
        perm = np.random.RandomState(6).permutation(n)
        tot_p, order_p = _rank(d["first"][perm], d["att"][perm], d["nhyp"][perm], w)
        assert tot_p.tobytes() == tot[perm].tobytes() and order_p.tobytes() == order[perm].tobytes()
    # w = 1 is the first pass' order wherever its scores descend; w = 0 the order by att
    first = -np.arange(K, dtype=np.float32)[None]
    att = np.random.RandomState(7).permutation(K).astype(np.float64)[None] * -3.0
    assert _rank(first, att, [K], 1.0)[1][0].tolist() == list(range(K))
    assert _rank(first, att, [K], 0.0)[1][0].tolist() == np.argsort(-att[0], kind="stable").tolist()


def test_lengths_and_counts_are_clamped():
    d = R.case_data("r5-u2-v3")
    lens = np.array([-4, 9, 2, 1, 2], np.int32)
    att, sl = _score(d["z"], d["y"], np.clip(lens, 0, 2), "bm")
    att_c, sl_c = _score(d["z"], d["y"], lens, "bm")
    assert att_c.tobytes() == att.tobytes() and sl_c.tobytes() == sl.tobytes()
    r = R.rank_case_data("k2")
    nh = np.array([5, -1, 0, 2], np.int32)
    tot, order = _rank(np.nan_to_num(r["first"]), np.nan_to_num(r["att"]), nh, 0.3)
    tot_c, order_c = _rank(np.nan_to_num(r["first"]), np.nan_to_num(r["att"]), np.clip(nh, 0, 2), 0.3)
    assert tot.tobytes() == tot_c.tobytes() and order.tobytes() == order_c.tobytes()


def test_refusals():
    d = R.case_data("r5-u2-v3")
    z, y, lens = d["z"], d["y"], d["lens"]
    _score(z, y, lens, "bm", ldy=1, expect_fail="ldy")
    _score(z, y, lens, "bm", U=0, expect_fail="bad dims")
    _score(z, y, lens, "bm", steps=False, ws_bytes=4, expect_fail="workspace")
    from las import _hip
    lib = _hip.lib()
    assert lib.las_rescore_score(None, 3, 6, None, 3, None, 5, 2, 3, None, None, None, 0, _hip.stream()) < 0
    assert "null pointer" in lib.las_last_error().decode()
    assert lib.las_rescore_workspace_bytes(5, 2) == 40 and lib.las_rescore_workspace_bytes(0, 2) == 0
    r = R.rank_case_data("k2")
    f, a, nh = np.nan_to_num(r["first"]), np.nan_to_num(r["att"]), r["nhyp"]
    for w in (-0.1, 1.5, float("nan"), float("inf")):
        _rank(f, a, nh, w, expect_fail="weight")
    _rank(f, a, nh, 0.5, K=0, expect_fail="K")
    _rank(f, a, nh, 0.5, K=65, expect_fail="K")
    assert lib.las_rescore_rank(None, None, None, 1, 1, 0.5, None, None, _hip.stream()) < 0
    # the host layer's own refusals
    from las import rescore
    with pytest.raises(ValueError, match="64"):
        rescore.rerank([[0.0] * 65], [[0.0] * 65], 0.5)
    with pytest.raises(ValueError, match="float32 view"):
        rescore.score_rows(torch.zeros(2, 2, 4, device="cuda").permute(0, 2, 1), torch.zeros(2, 4, dtype=torch.int32, device="cuda"),
                           torch.zeros(2, dtype=torch.int32, device="cuda"))


def test_host_wrappers_agree_with_the_c_calls():
    """las.rescore.score_rows on a permuted time-major view and las.rescore.rerank on ragged lists: what the raw calls gave"""
    from las import rescore
    name = "r37-u9-v31"
    d = R.case_data(name)
    att, sl = _score(d["z"], d["y"], d["lens"], "tm")
    zz = np.array(d["z"], copy=True)
    tm = torch.as_tensor(np.ascontiguousarray(zz.transpose(1, 0, 2))).cuda()
    for steps in (True, False):
        a, s = rescore.score_rows(tm.permute(1, 0, 2), torch.as_tensor(d["y"]).cuda(), torch.as_tensor(d["lens"]).cuda(), return_steps=steps)
        assert a.cpu().numpy().tobytes() == att[:-1].tobytes()
        assert (s is None) if not steps else (s.cpu().numpy().tobytes() == sl.tobytes())
    r = R.rank_case_data("k16")
    firsts = [r["first"][u, :nh].tolist() for u, nh in enumerate(r["nhyp"])]
    atts = [r["att"][u, :nh].tolist() for u, nh in enumerate(r["nhyp"])]
    tots, orders = rescore.rerank(firsts, atts, 0.3)
    want_t, want_o = R.rank_batch(r["first"], r["att"], r["nhyp"], 0.3)
    assert orders == want_o
    for t, wt in zip(tots, want_t):
        assert np.array_equal(np.isnan(t), np.isnan(wt)) and np.allclose(t[~np.isnan(t)], wt[~np.isnan(wt)], rtol=0, atol=4.0 * R.measured_tolerance()[1])
