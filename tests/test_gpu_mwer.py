"""MWER loss: las_mwer_loss through the C ABI against the numpy restatement (tests/mwer_ref.py) on the same logits.  Every
output is within 4x the largest difference between the restatement in float32 with the kernel's operation order and in float64,
measured on the CPU over the case list (mwer_ref.measured_tolerance) -- the factor covers the device's expf / logf against numpy's, as
in tests/test_gpu_rescore.py.  -inf is -inf on both sides.  The logits of steps at or beyond a row's length and of absent slots are
NaN, and so are their labels' neighbours in the output buffers: what nobody may write keeps its sentinel, what the contract zeroes is
exactly 0."""
import numpy as np
import pytest
import torch

import mwer_ref as M

pytestmark = pytest.mark.gpu
PAD_ROWS, PAD_V = 1, 3                 # the logits / dlogits buffers are wider and longer than [n K, U, V]


def _call(d, case, mode=None, grad=True, outs=True, expect_fail=None, **over):
    """las_mwer_loss over a case's data -> dict of numpy outputs (sentinels where nothing was written).  The logits lie in a padded
    buffer (rows of V + PAD_V floats, PAD_ROWS more rows), time-major or batch-major; over: arguments replaced for the refusal tests."""
    from las import _hip
    lib = _hip.lib()
    n, K, U, V = case["n"], case["K"], case["U"], case["V"]
    R, Vp, Rp = n * K, V + PAD_V, n * K + PAD_ROWS
    z = np.full((Rp, U, Vp), np.nan, np.float32)
    z[:R, :, :V] = d["z"]
    for r in range(R):
        if r % K >= d["nhyp"][r // K]:
            z[r] = np.nan                                                        # an absent slot: nobody may read it
        else:
            z[r, max(0, min(int(d["lens"][r]), U)):] = np.nan                    # nor a step at or beyond the row's length
    lens, err = np.array(d["lens"], np.int32), np.array(d["err"], np.float32)
    for r in range(R):
        if r % K >= d["nhyp"][r // K]:
            lens[r], err[r] = 1 << 30, np.nan
    if case["layout"] == "tm":
        dz = torch.as_tensor(np.ascontiguousarray(z.transpose(1, 0, 2))).cuda()
        sb, st = Vp, Rp * Vp
        dl = torch.full((U, Rp, Vp), float("nan"), device="cuda")
    else:
        dz = torch.as_tensor(z).cuda()
        sb, st = U * Vp, Vp
        dl = torch.full((Rp, U, Vp), float("nan"), device="cuda")
    dy, dlen = torch.as_tensor(np.ascontiguousarray(d["y"], np.int32)).cuda(), torch.as_tensor(lens).cuda()
    dnh, derr = torch.as_tensor(np.asarray(d["nhyp"], np.int32)).cuda(), torch.as_tensor(err).cuda()
    scale = torch.full((1,), float(M.SCALE), device="cuda")
    seq_lp = torch.full((R + 1,), float("nan"), dtype=torch.float64, device="cuda")
    post, coef = torch.full((R + 1,), float("nan"), device="cuda"), torch.full((R + 1,), float("nan"), device="cuda")
    risk, loss = torch.full((n + 1,), float("nan"), device="cuda"), torch.full((2,), float("nan"), device="cuda")
    a = dict(n=n, K=K, U=U, V=V, ldy=d["y"].shape[1], sb=sb, st=st, mode=case["mode"] if mode is None else mode)
    a.update({k: v for k, v in over.items() if k != "ws_bytes"})
    need = lib.las_mwer_workspace_bytes(n, K, U)
    ws = torch.zeros(max(need, 8) + 8, dtype=torch.uint8, device="cuda")
    o = (lambda t: _hip.p(t)) if outs else (lambda t: None)
    rc = lib.las_mwer_loss(_hip.p(dz), a["sb"], a["st"], a["V"], _hip.p(dy), a["ldy"], _hip.p(dlen), _hip.p(dnh), _hip.p(derr), a["n"], a["K"],
                           a["U"], a["mode"], _hip.p(scale), o(seq_lp), o(post), o(coef), o(risk), _hip.p(loss), _hip.p(dl) if grad else None,
                           _hip.p(ws), over.get("ws_bytes", need), _hip.stream())
    if expect_fail is not None:
        assert rc < 0 and expect_fail in lib.las_last_error().decode(), (rc, lib.las_last_error())
        torch.cuda.synchronize()
        for t in (seq_lp, post, coef, risk, loss, dl):                           # nothing was launched: every sentinel is still there
            assert bool(torch.isnan(t).all())
        return None
    _hip.check(rc, "las_mwer_loss")
    torch.cuda.synchronize()
    g = dl.cpu().numpy()
    g = g.transpose(1, 0, 2) if case["layout"] == "tm" else g
    return dict(seq_lp=seq_lp.cpu().numpy(), post=post.cpu().numpy(), coef=coef.cpu().numpy(), risk=risk.cpu().numpy(),
                loss=loss.cpu().numpy(), dl=g)


def _check(name, got, ref, case, d, tol):
    n, K, U, V = case["n"], case["K"], case["U"], case["V"]
    R = n * K
    assert np.isnan(got["seq_lp"][R]) and np.isnan(got["post"][R]) and np.isnan(got["coef"][R]) and np.isnan(got["risk"][n]) and np.isnan(got["loss"][1])
    for k in ("seq_lp", "post", "coef"):                                         # (NaN = not written: the same slots as the restatement's)
        dv = M.max_diff(got[k][:R], ref[k], name + " " + k)
        print(name, k, "max |device - float64|", dv, "allowed", tol[k])
        assert dv <= tol[k], (name, k, dv, tol[k])
    for k, x in (("risk", got["risk"][:n]), ("loss", got["loss"][:1])):
        dv = M.max_diff(x, ref[k], name + " " + k)
        print(name, k, "max |device - float64|", dv, "allowed", tol[k])
        assert dv <= tol[k], (name, k, dv, tol[k])
    g = got["dl"]
    assert np.isnan(g[R:]).all() and np.isnan(g[:, :, V:]).all(), name            # beyond [n K, U, V]: not written
    body = g[:R, :, :V]
    assert np.isfinite(body).all(), name                                         # every element inside is written, none NaN / inf
    dv = M.max_diff(body, ref["dlogits"], name + " dlogits")
    print(name, "dlogits max |device - float64|", dv, "allowed", tol["dlogits"])
    assert dv <= tol["dlogits"], (name, dv, tol["dlogits"])
    for r in range(R):
        absent = r % K >= d["nhyp"][r // K]
        L = 0 if absent else int(d["lens"][r])
        assert (body[r, L:] == 0).all(), (name, r)                               # exact zeros at t >= len and in absent slots
        if not absent and (got["post"][r] == 0 or got["coef"][r] == 0):
            assert (body[r] == 0).all(), (name, r)


@pytest.mark.parametrize("name", [c["name"] for c in M.CASES])
def test_cases_match_the_restatement(name):
    case = next(c for c in M.CASES if c["name"] == name)
    d = M.case_data(name)
    tol = {k: 4.0 * v for k, v in M.measured_tolerance().items()}
    ref = M.run_case(name)
    got = _call(d, case)
    _check(name, got, ref, case, d, tol)
    if case.get("equal"):
        assert (got["dl"][:case["n"] * case["K"], :, :case["V"]] == 0).all() and (got["coef"][np.isfinite(got["coef"])] == 0).all()
    if case.get("sp") and case["mode"] == 0:
        assert got["post"][1] == 0 and got["post"][2] == 0 and got["post"][4] == 0 and np.isneginf(got["seq_lp"][[1, 2, 4]]).all()
        assert got["seq_lp"][3] == 0 and (got["dl"][0, :, :case["V"]] != 0).any()
    # the same bits twice
    again = _call(d, case)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), (name, k)
    # the other layout reads the same values and writes the same gradient
    other = _call(d, dict(case, layout="bm" if case["layout"] == "tm" else "tm"))
    for k in got:
        assert got[k].tobytes() == other[k].tobytes(), (name, k)
    # the other mode on the same data
    m2 = 1 - case["mode"]
    ref2 = M.mwer(d["z"], d["y"], d["lens"], d["nhyp"], d["err"], case["K"], m2, M.SCALE, np.float64)
    _check(name + " mode %d" % m2, _call(d, case, mode=m2), ref2, case, d, tol)
    # without a gradient, and without the optional outputs: the loss is the same bits
    nog = _call(d, case, grad=False)
    assert np.isnan(nog["dl"]).all() and all(nog[k].tobytes() == got[k].tobytes() for k in ("seq_lp", "post", "coef", "risk", "loss"))
    bare = _call(d, case, outs=False)
    assert bare["loss"].tobytes() == got["loss"].tobytes() and bare["dl"].tobytes() == got["dl"].tobytes() and np.isnan(bare["post"]).all()


def test_refusals_launch_nothing():
    case = next(c for c in M.CASES if c["name"] == "v30-m0-sp")
    d = M.case_data(case["name"])
    from las import _hip
    need = _hip.lib().las_mwer_workspace_bytes(case["n"], case["K"], case["U"])
    assert need == case["n"] * 8 + (2 * case["n"] * case["K"] * case["U"] + case["n"] * case["K"]) * 4
    assert _hip.lib().las_mwer_workspace_bytes(0, 1, 1) == 0
    for over, msg in ((dict(K=0), "1 <= K <= 64"), (dict(K=65), "1 <= K <= 64"), (dict(U=0), "1 <= U <= 1024"), (dict(U=1025), "1 <= U <= 1024"),
                      (dict(V=0), "bad dims"), (dict(n=0), "bad dims"), (dict(n=1 << 20, K=64, U=32), "at most 2^31 - 1"),
                      (dict(ldy=case["U"] - 1), "ldy ="), (dict(sb=-1), "negative stride"), (dict(mode=2), "mode is 0"),
                      (dict(ws_bytes=need - 1), "a workspace of %d bytes is needed" % need)):
        _call(d, case, expect_fail=msg, **over)
