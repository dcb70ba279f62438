"""tf.layers.batch_normalization (+ the ReLU behind it) in training mode through las_bn_relu_fwd / las_bn_relu_bwd (csrc/bn.hip; reference
las/layers.py:114-116,155-161) against torch's batch_norm + relu on the same tensors: output, input / gamma / beta gradients, the moving
statistics' update, at the run.sh recipe's size ([48 x 319, 512]), at ragged sizes and on a 4-D NHWC block; and the layer-level switch.

Below those: the C ABI itself against the float64 reference of tests/bn_ref.py, one case per row of its TABLE (row-block, column-block
and data edges), the moving statistics over several launches, the capped apply grid, the refusals, and las.layers.bn around the kernels.
The bar of an output is not a constant: max(4 x gap, floor), gap = the distance of bn_ref's two fp32 evaluations from float64 on the same
case (bn_ref.bars; nothing in it comes from the device).  Every case prints a BN-FRACTION line (error / bar per output; each must be
<= 1); with LAS_BN_PARITY_OUT set it appends the record to that file (profiles/bn_parity.jsonl is such a run).
tests/test_bn_ref_host.py shows without a device that these bars tell nine planted defects from the kernel's arithmetic."""
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import bn_ref as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape,relu", [((15312, 512), True), ((37, 64), True), ((1276, 512), False), ((5, 9, 7, 8), True), ((300, 132), True)])
def test_bn_relu_kernels_match_torch(shape, relu):
    from las.layers import _BNReLU
    g = torch.Generator().manual_seed(sum(shape))
    C = shape[-1]
    x = (torch.randn(*shape, generator=g) * 0.7 + 0.3).cuda()
    x2 = x.reshape(-1, C).contiguous().requires_grad_(True)
    gamma = (torch.rand(C, generator=g) + 0.5).cuda().requires_grad_(True)
    beta = (torch.randn(C, generator=g) * 0.2).cuda().requires_grad_(True)
    mm, mv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    y = _BNReLU.apply(x2, gamma, beta, mm, mv, relu)
    w = torch.randn(x2.shape, generator=g).cuda()
    dx, dg, db = torch.autograd.grad((y * w).sum(), (x2, gamma, beta))
    xr = x2.detach().clone().requires_grad_(True)
    gr, br = gamma.detach().clone().requires_grad_(True), beta.detach().clone().requires_grad_(True)
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    yr = torch.nn.functional.batch_norm(xr, rm, rv, gr, br, training=True, momentum=0.01, eps=1e-3)
    if relu:
        yr = torch.relu(yr)
    dxr, dgr, dbr = torch.autograd.grad((yr * w).sum(), (xr, gr, br))
    assert (y - yr).abs().max().item() < 2e-5
    if relu:
        assert float(y.min()) >= 0.0
    # (a handful of outputs within rounding of the ReLU's kink may fall on the other side: compare the gradients where both masks agree)
    same = ((y > 0) == (yr > 0)) if relu else torch.ones_like(y, dtype=torch.bool)
    assert float((~same).float().mean()) < 1e-5
    scale = dxr.abs().max().item()
    assert ((dx - dxr) * same).abs().max().item() < 2e-4 * scale + 1e-6
    assert (dg - dgr).abs().max().item() < 2e-4 * max(1.0, dgr.abs().max().item())
    assert (db - dbr).abs().max().item() < 2e-4 * max(1.0, dbr.abs().max().item())
    assert (mm - rm).abs().max().item() < 1e-6 and (mv - rv).abs().max().item() < 1e-5


def test_cnn_listener_step_equals_the_torch_batch_norm_path():
    """the layer-level switch: one train step of the CNN listener (apply_bn on: conv2d bn + two bn per recurrent layer) with the kernels ==
    the same step through torch's batch norm (LAS_NO_BN_KERNEL), parity mode"""
    from helpers import make_args, synthetic_batch
    from las import layers as L, variables as V
    from las.las import LAS, Listener, Speller
    from oracle import las_oracle as O
    args = make_args(enc_type="cnn", enc_units=64, num_enc_layers=2, num_enc_channels=8, dec_units=64, num_dec_layers=1, embedding_size=32,
                     attention_size=32, apply_bn=True, lr=1e-3)
    xs, ys = synthetic_batch(4, 45, 8, 30, seed=3)
    p0 = O.init_params(args, seed=13, cell="lstm", enc_type="cnn")
    out = {}
    for on in (True, False):
        saved = L.BN_KERNEL
        L.BN_KERNEL = on
        try:
            L.set_cell("lstm"); L.set_precision("f32")
            st = V.reset_default_store(device="cuda"); st.load(p0)
            las = LAS(args, Listener, Speller, {})
            loss = float(las.train(xs, ys)[0])
            torch.cuda.synchronize()
            out[on] = (loss, st.flat_grad.clone(), {k: v.clone() for k, v in st.buffers.items()})
        finally:
            L.BN_KERNEL = saved
    assert abs(out[True][0] - out[False][0]) < 1e-5
    g1, g0 = out[True][1], out[False][1]
    assert (g1 - g0).abs().max().item() < 5e-3 * g0.abs().max().item()             # (ReLU-kink flips: see tests/test_gpu_run_sh_recipe.py)
    for k in out[False][2]:
        assert (out[True][2][k] - out[False][2][k]).abs().max().item() < 1e-5, k


# ------------------------------------------------------------------------------------------------ the C ABI against tests/bn_ref.py
SENT, GUARD = -77.0, 64
NAN = float("nan")


def _guarded(values, n):
    """n floats (values, or NaN where an output goes) followed by GUARD sentinel floats"""
    t = torch.full((n + GUARD,), SENT, dtype=torch.float32, device="cuda")
    if values is None:
        t[:n] = NAN
    else:
        t[:n] = torch.from_numpy(np.ascontiguousarray(values, np.float32).reshape(-1)).cuda()
    return t


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _ws(rows, C, extra=0):
    """a workspace of exactly the bytes asked for (+ extra), every byte 0xff: read as floats, NaN"""
    from las import _hip
    return torch.full((int(_hip.lib().las_bn_workspace_bytes(rows, C)) + extra,), 255, dtype=torch.uint8, device="cuda")


def _fwd(x, rows, C, gamma, beta, mean, rstd, mm, mv, relu, y, ws, ws_bytes=None):
    from las import _hip
    rc = _hip.lib().las_bn_relu_fwd(_hip.p(x), rows, C, _hip.p(gamma), _hip.p(beta), R.EPS, _hip.p(mean), _hip.p(rstd), _hip.p(mm), _hip.p(mv),
                                    R.MOMENTUM, int(relu), _hip.p(y), _hip.p(ws), ws.numel() if ws_bytes is None else ws_bytes, _hip.stream())
    torch.cuda.synchronize()
    return rc


def _bwd(x, y, dy, rows, C, gamma, mean, rstd, relu, dx, dgamma, dbeta, ws, ws_bytes=None):
    from las import _hip
    rc = _hip.lib().las_bn_relu_bwd(_hip.p(x), _hip.p(y), _hip.p(dy), rows, C, _hip.p(gamma), _hip.p(mean), _hip.p(rstd), int(relu), _hip.p(dx),
                                    _hip.p(dgamma), _hip.p(dbeta), _hip.p(ws), ws.numel() if ws_bytes is None else ws_bytes, _hip.stream())
    torch.cuda.synchronize()
    return rc


class _Device(object):
    """a case's inputs on the device: x and dy with guard floats behind rows x C"""

    def __init__(self, case):
        self.rows, self.C, self.relu, self.n = case["rows"], case["C"], case["relu"], case["rows"] * case["C"]
        self.x, self.dy = _guarded(case["x"], self.n), _guarded(case["dy"], self.n)
        self.gamma, self.beta = _dev(case["gamma"]), _dev(case["beta"])
        self.case = case

    def forward(self, moving=True, extra_ws=0):
        """one las_bn_relu_fwd on NaN-filled outputs -> dict of device tensors (y with its guard)"""
        o = {"y": _guarded(None, self.n), "mean": torch.full((self.C,), NAN, device="cuda"), "rstd": torch.full((self.C,), NAN, device="cuda"),
             "mm": _dev(self.case["mm0"]) if moving else None, "mv": _dev(self.case["mv0"]) if moving else None}
        assert _fwd(self.x, self.rows, self.C, self.gamma, self.beta, o["mean"], o["rstd"], o["mm"], o["mv"], self.relu, o["y"],
                    _ws(self.rows, self.C, extra_ws)) == 0
        return o

    def backward(self, f, dgamma, dbeta):
        dx = _guarded(None, self.n)
        assert _bwd(self.x, f["y"], self.dy, self.rows, self.C, self.gamma, f["mean"], f["rstd"], self.relu, dx, dgamma, dbeta,
                    _ws(self.rows, self.C)) == 0
        return dx

    def host(self, f, dx, dgamma, dbeta):
        h = {k: f[k].cpu().numpy() for k in ("mean", "rstd", "mm", "mv")}
        h["y"], h["dx"] = (t[:self.n].cpu().numpy().reshape(self.rows, self.C) for t in (f["y"], dx))
        h["dgamma"], h["dbeta"] = dgamma.cpu().numpy(), dbeta.cpu().numpy()
        return h


def _guards_hold(*tensors):
    return all(bool((t[-GUARD:] == SENT).all()) for t in tensors)


def _record(rec):
    print("BN-FRACTION %s " % rec["case"] + " ".join("%s=%.3f" % (k, rec["fraction"][k]) for k in sorted(rec["fraction"])))
    if os.environ.get("LAS_BN_PARITY_OUT"):
        with open(os.environ["LAS_BN_PARITY_OUT"], "a") as f:
            f.write(json.dumps(rec) + "\n")


@pytest.mark.parametrize("row", R.TABLE, ids=R.row_id)
def test_c_abi_against_float64(row):
    prep = R.table_case(row)
    case, ref, gap, bar = prep
    rows, C = case["rows"], case["C"]
    d = _Device(case)
    f = d.forward()
    dg, db = _dev(case["dgamma0"]), _dev(case["dbeta0"])
    dx = d.backward(f, dg, db)
    got = d.host(f, dx, dg, db)
    # containment: every output element written, nothing behind rows x C touched
    for k in ("y", "dx", "mean", "rstd"):
        assert not np.isnan(got[k]).any(), k
    assert _guards_hold(d.x, d.dy, f["y"], dx)
    if case["relu"]:
        assert float(got["y"].min()) >= 0.0
    # parity, the reference on the kernel's own mask; the mask itself away from the kink; exact zeros on constant columns
    frac, flips, nonzero = R.judge(prep, got)
    _record({"case": R.row_id(row), "rows": rows, "C": C, "relu": int(case["relu"]), "kind": case["kind"], "fraction": frac,
             "gap": gap, "bar": bar, "error": {k: frac[k] * bar[k] for k in frac}, "mask_flips": flips})
    assert set(frac) == set(R.OUTPUTS)
    assert max(frac.values()) <= 1.0, frac
    assert flips == 0 and nonzero == 0
    # the gradient buffers are added into: a second backward on the same buffers adds the same amount again.  Its bar is twice the
    # first's (the sums' own error enters twice; each of the two additions rounds within the first bar's share for it)
    dx2 = d.backward(f, dg, db)
    r = R.run(R.reference, case, mask=got["y"] > 0)
    for k, t, init in (("dgamma", dg, case["dgamma0"]), ("dbeta", db, case["dbeta0"])):
        twice = 2.0 * (r[k] - init.astype(np.float64)) + init
        assert float(np.abs(t.cpu().numpy() - twice).max()) <= 2.0 * bar[k], k
    assert torch.equal(dx2, dx)                                        # ... and the same dx bits
    dx3 = d.backward(f, None, None)                                    # no gradient buffers: the same dx bits
    assert torch.equal(dx3, dx)
    # no moving buffers, a larger workspace full of NaN: the same y, mean and rstd bits
    f2 = d.forward(moving=False, extra_ws=4096)
    assert all(torch.equal(f2[k], f[k]) for k in ("y", "mean", "rstd"))
    # two runs: the same bits in every output
    f3 = d.forward()
    assert all(torch.equal(f3[k], f[k]) for k in ("y", "mean", "rstd", "mm", "mv"))
    assert _guards_hold(d.x, d.dy, f2["y"], f3["y"], dx2, dx3)


def test_moving_statistics_over_five_launches():
    """five launches on the same moving buffers, five different inputs (rows = 257, C = 68): after every one both buffers against the
    float64 recurrence, which never sees the fp32 state; the bar by the same rule from the two fp32 recurrences"""
    rows, C = 257, 68
    mm, mv = torch.full((C,), R.MM0, device="cuda"), torch.full((C,), R.MV0, device="cuda")
    state = {"ref": (np.full(C, R.MM0), np.full(C, R.MV0)), "eval32": (np.full(C, R.MM0, np.float32), np.full(C, R.MV0, np.float32)),
             "emulate32": (np.full(C, R.MM0, np.float32), np.full(C, R.MV0, np.float32))}
    fns = {"ref": R.reference, "eval32": R.eval32, "emulate32": R.emulate32}
    for step, kind in enumerate(("plain", "offset", "tiny", "outlier", "plain")):
        case = R.make_case((rows, C, 1, kind), seed=900 + step)
        for k in state:
            o = fns[k](case["x"], case["gamma"], case["beta"], None, True, mm=state[k][0], mv=state[k][1])
            state[k] = (o["mm"], o["mv"])
        x = _guarded(case["x"], rows * C)
        y, mean, rstd = _guarded(None, rows * C), torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
        assert _fwd(x, rows, C, _dev(case["gamma"]), _dev(case["beta"]), mean, rstd, mm, mv, 1, y, _ws(rows, C)) == 0
        frac = {}
        for i, (name, t) in enumerate((("mm", mm), ("mv", mv))):
            gap = max(float(np.abs(state[k][i].astype(np.float64) - state["ref"][i]).max()) for k in ("eval32", "emulate32"))
            frac[name] = float(np.abs(t.cpu().numpy().astype(np.float64) - state["ref"][i]).max()) / max(4.0 * gap, 1e-6)
        _record({"case": "moving-step%d-%s" % (step, kind), "rows": rows, "C": C, "fraction": frac})
        assert max(frac.values()) <= 1.0, (step, frac)


def test_capped_apply_grid():
    """rows = 65552, C = 512: n4 = 8 390 656 float4 elements, just over the 8192 x 1024 the apply kernels' grids are capped at (the
    grid-stride loop wraps at row 16384), 257 row blocks, the last with 16 rows.  Generated, referenced and judged one 64-column block
    at a time (bn_ref.make_chunk; four blocks in flight): statistics, gradients, y and dx in full -- the first and last rows and the
    rows around the wrap included."""
    rows, C, W = 65552, 512, R.COLS
    assert rows * (C // 4) == 8192 * 1024 + 2048 and rows % R.BLOCK == 16
    nchunk = C // W
    with ThreadPoolExecutor(4) as pool:
        chunks = list(pool.map(lambda k: R.make_chunk(rows, k), range(nchunk)))
    cat = lambda key: np.concatenate([c[key] for c in chunks], axis=-1)
    whole = {"rows": rows, "C": C, "relu": True, "x": cat("x"), "dy": cat("dy"), "gamma": cat("gamma"), "beta": cat("beta"), "mm0": cat("mm0"),
             "mv0": cat("mv0")}
    dg0, db0 = cat("dgamma0"), cat("dbeta0")
    del chunks
    d = _Device(whole)
    del whole["x"], whole["dy"]
    f = d.forward()
    dg, db = _dev(dg0), _dev(db0)
    dx = d.backward(f, dg, db)
    assert _guards_hold(d.x, d.dy, f["y"], dx)
    got = d.host(f, dx, dg, db)
    for k in ("y", "dx", "mean", "rstd"):
        assert not np.isnan(got[k]).any(), k

    def one(k):
        prep = R.prepare(R.make_chunk(rows, k))
        sl = slice(k * W, (k + 1) * W)
        return R.judge(prep, {key: np.ascontiguousarray(v[..., sl]) for key, v in got.items()})

    with ThreadPoolExecutor(4) as pool:
        res = list(pool.map(one, range(nchunk)))
    frac = {k: max(r[0][k] for r in res) for k in R.OUTPUTS}
    _record({"case": "capped-grid-65552x512", "rows": rows, "C": C, "relu": 1, "kind": "plain", "fraction": frac,
             "mask_flips": sum(r[1] for r in res)})
    assert max(frac.values()) <= 1.0, frac
    assert sum(r[1] for r in res) == 0


def test_refusals_before_any_launch():
    """bad arguments: < 0, a las_last_error text, and no output touched"""
    from las import _hip
    rows, C = 8, 8
    n = rows * C
    big = lambda: torch.full((n + 8,), SENT, device="cuda")
    x, y, dy, dx = big(), big(), big(), big()
    small = lambda: torch.full((C + 4,), SENT, device="cuda")
    gamma, beta, mean, rstd, mm, mv, dg, db = (small() for _ in range(8))
    ws = _ws(rows, C)
    need = ws.numel()
    outputs = (y, dx, mean, rstd, mm, mv, dg, db)

    def refused(rc, text):
        msg = _hip.lib().las_last_error() or b""
        assert rc < 0 and text in msg, (rc, msg)
        assert all(bool((t == SENT).all()) for t in outputs)

    fwd = lambda **k: _fwd(k.get("x", x), k.get("rows", rows), k.get("C", C), k.get("gamma", gamma), beta, mean, rstd, k.get("mm", mm),
                           k.get("mv", mv), 1, k.get("y", y), ws, k.get("ws_bytes"))
    bwd = lambda **k: _bwd(k.get("x", x), k.get("y", y), k.get("dy", dy), k.get("rows", rows), k.get("C", C), k.get("gamma", gamma),
                           k.get("mean", mean), k.get("rstd", rstd), k.get("relu", 1), k.get("dx", dx), dg, db, ws, k.get("ws_bytes"))
    for call, name in ((fwd, b"las_bn_relu_fwd"), (bwd, b"las_bn_relu_bwd")):
        refused(call(C=6), name)                                       # C % 4 != 0
        refused(call(rows=0), name)
        refused(call(ws_bytes=need - 1), b"workspace")
    refused(fwd(mm=None), b"go together")                              # one moving pointer without the other
    refused(fwd(mv=None), b"go together")
    refused(_bwd(x, None, dy, rows, C, gamma, mean, rstd, 1, dx, dg, db, ws), b"needs y")
    bufs = {"x": x, "y": y, "dy": dy, "dx": dx, "gamma": gamma, "mean": mean, "rstd": rstd}
    for k in ("x", "y", "gamma"):                                      # a pointer offset by 4 bytes
        refused(fwd(**{k: bufs[k][1:]}), b"alignment")
    for k in ("x", "y", "dy", "dx", "gamma", "mean", "rstd"):
        refused(bwd(**{k: bufs[k][1:]}), b"alignment")
    # ... and the same buffers, unshifted, are served
    assert fwd() == 0 and bwd() == 0 and bwd(relu=0, y=None) == 0
    assert not bool((y[:n] == SENT).any()) and not bool((dx[:n] == SENT).any()) and bool((y[n:] == SENT).all()) and bool((dx[n:] == SENT).all())


# ------------------------------------------------------------------------------------------------ las.layers.bn around the kernels
def _layer_inputs(shape, seed):
    rng = np.random.RandomState(seed)
    C = shape[-1]
    xs = [(rng.randn(*shape) * s + m).astype(np.float32) for s, m in ((0.7, 0.3), (1.5, -2.0), (0.2, 5.0), (1.0, 0.0))]
    return xs, rng.uniform(0.5, 1.5, C).astype(np.float32), (rng.randn(C) * 0.2).astype(np.float32)


def _fresh_store(gamma, beta):
    from las import variables as V
    st = V.reset_default_store(device="cuda")
    st.load({"t/gamma": gamma, "t/beta": beta})
    return st


@pytest.mark.parametrize("shape,nhwc", [((5, 53, 68), False), ((3, 9, 7, 12), True)], ids=["rank3", "rank4-nhwc"])
def test_layer_eval_after_three_training_calls(shape, nhwc, monkeypatch):
    """three training calls on different inputs, then bn(x, False): the float64 inference formula on the buffers that bn_ref.moving
    predicts from (0, 1); the bar from the two fp32 evaluations of the same chain"""
    from las import layers as L
    xs, gamma, beta = _layer_inputs(shape, 7 + len(shape))
    C = shape[-1]
    st = _fresh_store(gamma, beta)
    calls = []
    orig = L._BNReLU.apply
    monkeypatch.setattr(L._BNReLU, "apply", staticmethod(lambda *a: (calls.append(a[0].shape), orig(*a))[1]))

    def dev(a):
        t = torch.from_numpy(a).cuda()
        if nhwc:                                                       # what conv2d hands over: an NCHW block permuted to NHWC
            t = t.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
            assert not t.is_contiguous()
        return t

    state = {"ref": (np.zeros(C), np.ones(C)), "eval32": (np.zeros(C, np.float32), np.ones(C, np.float32)),
             "emulate32": (np.zeros(C, np.float32), np.ones(C, np.float32))}
    fns = {"ref": R.reference, "eval32": R.eval32, "emulate32": R.emulate32}
    for x in xs[:3]:
        L.bn(dev(x), True, scope="t", relu=True)
        for k in state:
            o = fns[k](x.reshape(-1, C), gamma, beta, None, True, mm=state[k][0], mv=state[k][1])
            state[k] = (o["mm"], o["mv"])
    assert len(calls) == 3 and all(tuple(c) == (int(np.prod(shape[:-1])), C) for c in calls)
    for relu in (True, False):
        y = L.bn(dev(xs[3]), False, scope="t", relu=relu)
        torch.cuda.synchronize()
        assert tuple(y.shape) == shape and len(calls) == 3             # (inference does not go through the kernels)
        ref = R.eval_infer(xs[3], gamma, beta, state["ref"][0], state["ref"][1], relu)
        gap = max(float(np.abs(R.eval_infer32(xs[3], gamma, beta, state[k][0], state[k][1], relu).astype(np.float64) - ref).max())
                  for k in ("eval32", "emulate32"))
        err = float(np.abs(y.detach().cpu().numpy().astype(np.float64) - ref).max())
        _record({"case": "layer-eval-%s-%s" % ("nhwc" if nhwc else "rank3", "relu" if relu else "lin"), "fraction": {"y": err / max(4.0 * gap, 1e-6)}})
        assert err <= max(4.0 * gap, 1e-6)
    for i, name in enumerate(("t/moving_mean", "t/moving_variance")):
        gap = max(float(np.abs(state[k][i].astype(np.float64) - state["ref"][i]).max()) for k in ("eval32", "emulate32"))
        assert float(np.abs(st.buffers[name].cpu().numpy() - state["ref"][i]).max()) <= max(4.0 * gap, 1e-6), name


@pytest.mark.parametrize("shape", [(1, 8), (37, 6)], ids=["rows1", "C6"])
def test_layer_fallback_shapes(shape, monkeypatch):
    """the two shapes the predicate keeps away from the kernels (one row; C % 4 != 0): the float64 result through the library path"""
    from las import layers as L
    xs, gamma, beta = _layer_inputs(shape, 23)
    C = shape[-1]
    st = _fresh_store(gamma, beta)
    calls = []
    orig = L._BNReLU.apply
    monkeypatch.setattr(L._BNReLU, "apply", staticmethod(lambda *a: (calls.append(a[0].shape), orig(*a))[1]))
    x = torch.from_numpy(xs[0]).cuda().requires_grad_(True)
    y = L.bn(x, True, scope="t", relu=True)
    w = torch.from_numpy(xs[1]).cuda()
    (dx,) = torch.autograd.grad((y * w).sum(), (x,))
    torch.cuda.synchronize()
    assert not calls
    case = {"x": xs[0], "gamma": gamma, "beta": beta, "dy": xs[1], "relu": True, "dgamma0": None, "dbeta0": None, "mm0": np.zeros(C, np.float32),
            "mv0": np.ones(C, np.float32)}
    ref = R.run(R.reference, case, mask=y.detach().cpu().numpy() > 0)
    bar = R.bars(case)
    got = {"y": y.detach().cpu().numpy(), "dx": dx.cpu().numpy(), "mm": st.buffers["t/moving_mean"].cpu().numpy(),
           "mv": st.buffers["t/moving_variance"].cpu().numpy()}
    err = R.distance(got, ref, keys=tuple(got))
    print("BN-FALLBACK %s " % (shape,) + " ".join("%s: error %.3g bar %.3g" % (k, err[k], bar[k]) for k in err))
    assert all(err[k] <= bar[k] for k in err), (err, bar)


@pytest.mark.parametrize("prec,expected", [("f32", 6), ("bf16", 6)])
def test_cnn_listener_calls_that_reach_the_kernels(prec, expected, monkeypatch):
    """one train step of the CNN listener with apply_bn (the sizes of test_cnn_listener_step_equals_the_torch_batch_norm_path): how
    many of its 2 + 2 x num_enc_layers training-mode batch normalisations reach las_bn_relu_fwd.  Parity mode: all of them.  Speed
    mode: all of them as well -- the conv blocks and the dense outputs in front of a batch normalisation stay fp32 there (pinned: a
    bf16 hand-over would fail the predicate of las.layers.bn and send the site to torch's kernels without a word)."""
    from helpers import make_args, synthetic_batch
    from las import layers as L, variables as V
    from las.las import LAS, Listener, Speller
    from oracle import las_oracle as O
    args = make_args(enc_type="cnn", enc_units=64, num_enc_layers=2, num_enc_channels=8, dec_units=64, num_dec_layers=1, embedding_size=32,
                     attention_size=32, apply_bn=True, lr=1e-3)
    xs, ys = synthetic_batch(4, 45, 8, 30, seed=3)
    p0 = O.init_params(args, seed=13, cell="lstm", enc_type="cnn")
    calls, sites = [], []
    orig, orig_bn = L._BNReLU.apply, L.bn
    monkeypatch.setattr(L._BNReLU, "apply", staticmethod(lambda *a: (calls.append(a[0].dtype), orig(*a))[1]))
    monkeypatch.setattr(L, "bn", lambda inputs, is_training, *a, **k: (sites.append((inputs.dtype, bool(is_training))),
                                                                       orig_bn(inputs, is_training, *a, **k))[1])
    try:
        L.set_cell("lstm"); L.set_precision(prec)
        st = V.reset_default_store(device="cuda"); st.load(p0)
        las = LAS(args, Listener, Speller, {})
        loss = float(las.train(xs, ys)[0])
        torch.cuda.synchronize()
    finally:
        L.set_precision("f32")
    training = [d for d, on in sites if on]                            # (build_variables walks the listener once in inference mode)
    print("BN-CALLS %s: %d of %d training-mode batch normalisations reach the kernels; input dtypes %s"
          % (prec, len(calls), len(training), sorted(set(map(str, training)))))
    assert np.isfinite(loss) and len(training) == 2 + 2 * args.num_enc_layers
    assert len(calls) == expected and all(d == torch.float32 for d in calls)
