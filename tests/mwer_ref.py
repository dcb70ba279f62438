"""CPU restatement of the MWER loss (csrc/mwer.hip, las/mwer.py): every output of las_mwer_loss from the same logits.  numpy
only.  `ft`: np.float64 is the restatement proper (nothing rounded to fp32 anywhere); np.float32 is the same arithmetic in the device's
number formats AND operation order (the lanes' strided partial sums and the butterfly of the log-sum-exp, fp32 step terms, float64
per-utterance arithmetic rounded to fp32 where the kernel stores it, the fp32 gradient), which is what the device tolerance is measured
from (measured_tolerance, tests/test_gpu_mwer.py) -- the convention of tests/rescore_ref.py."""
import functools

import numpy as np


# ---- log-sum-exp ---------------------------------------------------------------------------------------------------------------------
def _lse32(z):
    """[N, V] float32 -> [N] float32: m + logf(s), s summed as the kernel sums it: 64 lanes, lane i adds classes i, i + 64, ... in order
    from 0; a xor butterfly (32 .. 1).  Rows whose maximum is -inf give -inf."""
    N, V = z.shape
    m = z.max(axis=1)
    dead = np.isneginf(m)
    ms = np.where(dead, np.float32(0), m).astype(np.float32)
    with np.errstate(all="ignore"):
        e = np.exp((z - ms[:, None]).astype(np.float32)).astype(np.float32)
    rows = -(-V // 64)
    e = np.concatenate([e, np.zeros((N, rows * 64 - V), np.float32)], 1).reshape(N, rows, 64)
    part = np.zeros((N, 64), np.float32)
    for r in range(rows):
        part = (part + e[:, r]).astype(np.float32)
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        part = (part + part[:, idx ^ o]).astype(np.float32)
    with np.errstate(all="ignore"):
        lse = (ms + np.log(part[:, 0]).astype(np.float32)).astype(np.float32)
    return np.where(dead, np.float32(-np.inf), lse).astype(np.float32)


def _lse64(z):
    z64 = z.astype(np.float64)
    m = z64.max(axis=1)
    dead = np.isneginf(m)
    ms = np.where(dead, 0.0, m)
    with np.errstate(all="ignore"):
        lse = ms + np.log(np.exp(z64 - ms[:, None]).sum(axis=1))
    return np.where(dead, -np.inf, lse)


# ---- the loss ------------------------------------------------------------------------------------------------------------------------
def mwer(z, y, lens, nhyp, err, K, mode, scale, ft=np.float64, grad=True):
    """z [n K, U, V] logits (float32 values; steps t >= lens[r] and the rows of absent slots are never looked at, whatever they hold),
    y [n K, >= U], lens [n K], nhyp [n], err [n K] float32, scale a float32 -> dict of
      seq_lp float64 [n K]  (NaN for an absent slot: not written),  post, coef [n K] and risk [n] (ft; NaN for an absent slot),
      loss (ft scalar),  lse [n K, U] (ft; NaN where nothing is computed),  dlogits [n K, U, V] (ft) with grad."""
    f32 = ft is np.float32
    z = np.asarray(z, np.float32 if f32 else np.float64)               # (float64 logits: the finite differences of the host test)
    R, U, V = z.shape
    n = R // K
    assert n * K == R
    lens = np.clip(np.asarray(lens, np.int64), 0, U)
    nhyp = np.clip(np.asarray(nhyp, np.int64), 0, K)
    err = np.asarray(err, np.float32).astype(np.float64)
    sc = np.float64(np.float32(scale))
    seq_lp = np.full(R, np.nan)
    post, coef = np.full(R, np.nan, ft), np.full(R, np.nan, ft)
    gate = np.zeros(R, np.float32 if f32 else np.float64)             # the coefficient the gradient uses (0: an exact-zero row)
    risk = np.zeros(n, np.float64)
    lse = np.full((R, U), np.nan, ft)
    term = np.full((R, U), np.nan, ft)
    live = [(r, t) for r in range(R) if r % K < nhyp[r // K] for t in range(int(lens[r]))]
    if live:
        rows = np.stack([z[r, t] for r, t in live])
        l = (_lse32 if f32 else _lse64)(rows)
        for (r, t), lv in zip(live, l):
            lse[r, t] = lv
            c = int(y[r, t])
            if 0 <= c < V and not np.isneginf(lv):
                with np.errstate(all="ignore"):
                    term[r, t] = ft(ft(z[r, t, c]) - ft(lv))
            else:
                term[r, t] = -np.inf
    for u in range(n):
        nh = int(nhyp[u])
        if nh == 0:
            continue
        rr = np.arange(u * K, u * K + nh)
        for r in rr:
            s = np.float64(0.0)
            for t in range(int(lens[r])):
                s = s + np.float64(term[r, t])
            seq_lp[r] = s
        e = err[rr]
        with np.errstate(all="ignore"):
            if mode == 0:
                m = seq_lp[rr].max()
                ex = np.exp(seq_lp[rr] - m) if m > -np.inf else np.zeros(nh)
                s = np.float64(0.0)
                for j in range(nh):
                    s = s + ex[j]
                p = ex / s if s > 0 else np.zeros(nh)
                rk, c = np.float64(0.0), np.zeros(nh)
                for j in range(nh):
                    rk = rk + p[j] * e[j]
                for k in range(nh):
                    d = np.float64(0.0)
                    for j in range(nh):
                        d = d + p[j] * (e[k] - e[j])
                    c[k] = sc * p[k] * d
            else:
                p = np.full(nh, 1.0 / np.float64(nh))
                rk = np.float64(0.0)
                for j in range(nh):
                    rk = rk + e[j]
                rk = rk / np.float64(nh)
                c = sc * (e - rk) / np.float64(nh)
        risk[u] = rk
        post[rr], coef[rr] = p.astype(ft), c.astype(ft)
        gate[rr] = np.where(post[rr] == 0, 0, coef[rr])
    part = np.zeros(64)
    for u in range(n):
        part[u % 64] += risk[u]
    tot = np.float64(0.0)
    for i in range(64):
        tot = tot + part[i]
    out = dict(seq_lp=seq_lp, post=post, coef=coef, risk=risk.astype(ft), loss=ft(sc * tot), lse=lse)
    if grad:
        dl = np.zeros((R, U, V), ft)
        for r, t in live:
            if gate[r] == 0 or np.isneginf(lse[r, t]):
                continue
            with np.errstate(all="ignore"):
                p = np.exp((z[r, t].astype(ft) - lse[r, t]).astype(ft)).astype(ft)
            oh = np.zeros(V, ft)
            c = int(y[r, t])
            if 0 <= c < V:
                oh[c] = 1
            dl[r, t] = (gate[r] * (oh - p).astype(ft)).astype(ft)
        out["dlogits"] = dl
    return out


def surrogate64(z, y, lens, nhyp, err, K, mode, scale):
    """the float64 scalar whose gradient with respect to the logits las_mwer_loss returns: mode 0 the loss itself, scale sum_u sum_k
    post err; mode 1 (the sampling estimate, whose loss -- the mean error count -- does not depend on the logits) the score-function
    form scale sum_u sum_k (err - mean err) / nhyp * seq_lp, the coefficients held constant"""
    o = mwer(z, y, lens, nhyp, err, K, mode, scale, np.float64, grad=False)
    if mode == 0:
        return float(o["loss"])
    n = len(nhyp)
    e = np.asarray(err, np.float64)
    s = 0.0
    for u in range(n):
        nh = int(nhyp[u])
        if nh:
            rr = np.arange(u * K, u * K + nh)
            s += float(np.sum((e[rr] - e[rr].mean()) / nh * o["seq_lp"][rr]))
    return float(np.float32(scale)) * s


# ---- the case list of the device test --------------------------------------------------------------------------------------------------
# name, n, K, U, ldy, V, layout (tm: the Speller's time-major [U, n K, V] buffer; bm: batch-major), mode, nhyp, seed, logit scale, and
#   sp     the special rows of utterance 0 (K = 5, U >= 2): slot 1 has a -inf logit at its label of step 0 (mode 0: post = 0), slot 2 a
#          label outside [0, V) at step 0, slot 3 len = 0, slot 4 a step 0 without mass (all -inf)
#   equal  all error counts equal: the gradient is exactly zero everywhere
# V: 1, 30, 64 | 65 (registers: 1 value a lane | 16), 1024 | 1025 (16 | 80), 5000, 5120 | 5121 (80 | 128), 8192 | 8193 (128 | streamed).
# U of 1 .. 7, K of 1 .. 5, n of 1 .. 3; nhyp < K, = 0 and = 1; ldy > U; both layouts and modes.
CASES = [
    dict(name="v1", n=1, K=1, U=1, ldy=2, V=1, layout="tm", mode=0, nhyp=[1], seed=1, zs=2.0),
    dict(name="v30-m0-sp", n=3, K=5, U=5, ldy=7, V=30, layout="tm", mode=0, nhyp=[5, 0, 3], seed=2, zs=2.0, sp=True),
    dict(name="v30-m1-sp", n=3, K=5, U=5, ldy=5, V=30, layout="bm", mode=1, nhyp=[5, 0, 3], seed=3, zs=2.0, sp=True),
    dict(name="v30-m0-equal", n=2, K=3, U=4, ldy=4, V=30, layout="bm", mode=0, nhyp=[3, 2], seed=4, zs=2.0, equal=True),
    dict(name="v30-m1-equal", n=2, K=3, U=4, ldy=6, V=30, layout="tm", mode=1, nhyp=[3, 2], seed=5, zs=2.0, equal=True),
    dict(name="v64", n=2, K=4, U=6, ldy=6, V=64, layout="bm", mode=0, nhyp=[4, 2], seed=6, zs=3.0),
    dict(name="v65", n=2, K=3, U=3, ldy=4, V=65, layout="tm", mode=1, nhyp=[3, 1], seed=7, zs=3.0),
    dict(name="v1024", n=1, K=2, U=2, ldy=3, V=1024, layout="tm", mode=0, nhyp=[2], seed=8, zs=2.0),
    dict(name="v1025", n=2, K=2, U=2, ldy=2, V=1025, layout="bm", mode=0, nhyp=[2, 1], seed=9, zs=2.0),
    dict(name="v5000", n=2, K=3, U=7, ldy=9, V=5000, layout="tm", mode=0, nhyp=[3, 2], seed=10, zs=2.0),
    dict(name="v5120", n=1, K=2, U=3, ldy=3, V=5120, layout="bm", mode=1, nhyp=[2], seed=11, zs=2.0),
    dict(name="v5121", n=1, K=3, U=2, ldy=4, V=5121, layout="tm", mode=0, nhyp=[3], seed=12, zs=2.0),
    dict(name="v8192", n=1, K=2, U=2, ldy=2, V=8192, layout="tm", mode=0, nhyp=[2], seed=13, zs=2.0),
    dict(name="v8193", n=2, K=2, U=1, ldy=3, V=8193, layout="bm", mode=0, nhyp=[1, 2], seed=14, zs=2.0),
]
BAD_LABEL = -7                    # y beyond U
SCALE = np.float32(0.37)


@functools.lru_cache(maxsize=None)
def case_data(name):
    """-> dict z [n K, U, V] float32, y [n K, ldy] int32, lens [n K] int32, nhyp [n] int32, err [n K] float32.  lens are ragged, U in
    slot 0 of every utterance.  Cached, shared and left unchanged."""
    case = next(c for c in CASES if c["name"] == name)
    rng = np.random.RandomState(7000 + case["seed"])
    n, K, U, V, ldy = case["n"], case["K"], case["U"], case["V"], case["ldy"]
    R = n * K
    z = (rng.randn(R, U, V) * case["zs"]).astype(np.float32)
    y = np.full((R, ldy), BAD_LABEL, np.int32)
    y[:, :U] = rng.randint(0, V, size=(R, U))
    # every label about as likely as the rest of its row together (lse of N(0, zs^2) logits ~ log V + zs^2 / 2): the hypotheses' log-
    # likelihoods differ by a few nats, so that the posterior is spread over them and the gradient is of ordinary size
    np.put_along_axis(z, y[:, :U, None].astype(np.int64), np.take_along_axis(z, y[:, :U, None].astype(np.int64), 2)
                      + np.float32(np.log(V) + case["zs"] ** 2 / 2), 2)
    lens = rng.randint(1, U + 1, size=R).astype(np.int32)
    lens[0::K] = U
    err = rng.randint(0, 7, size=R).astype(np.float32)
    if case.get("equal"):
        err[:] = 3.0
    else:
        err[0::K] = 0.0                                                # (slot 0 right, another slot wrong: never all equal)
        if K > 1:
            err[1::K] = 2.0
    if case.get("sp"):
        assert K == 5 and U >= 2
        z[1, 0, y[1, 0]] = -np.inf
        y[2, 0] = V
        lens[3] = 0
        z[4, 0, :] = -np.inf
        lens[1] = lens[2] = lens[4] = U
        err[3] = 4.0                                                   # (the empty string is the likeliest: it differs from slot 0's errors)
    return dict(z=z, y=y, lens=lens, nhyp=np.asarray(case["nhyp"], np.int32), err=err)


@functools.lru_cache(maxsize=None)
def run_case(name, f32=False):
    """the restatement over a case; cached, shared and left unchanged"""
    case = next(c for c in CASES if c["name"] == name)
    d = case_data(name)
    return mwer(d["z"], d["y"], d["lens"], d["nhyp"], d["err"], case["K"], case["mode"], SCALE, np.float32 if f32 else np.float64)


OUTPUTS = ("seq_lp", "post", "coef", "risk", "loss", "dlogits")


def max_diff(a, b, what=""):
    """the largest |a - b| over the entries where b is finite; NaN (not written) and -inf must sit in the same places"""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isneginf(a), np.isneginf(b)) and not np.isposinf(a).any(), what
    fin = np.isfinite(b)
    return float(np.abs(a[fin] - b[fin]).max()) if fin.any() else 0.0


@functools.lru_cache(maxsize=None)
def measured_tolerance():
    """-> {output: the largest absolute difference between the float32 restatement (the kernel's operation order) and the float64 one
    over the case list}"""
    tol = {k: 0.0 for k in OUTPUTS}
    for case in CASES:
        a, b = run_case(case["name"], True), run_case(case["name"], False)
        for k in OUTPUTS:
            tol[k] = max(tol[k], max_diff(a[k], b[k], case["name"] + " " + k))
    return tol
