"""CPU restatement of csrc/bn.hip (las_bn_relu_fwd / las_bn_relu_bwd = tf.layers.batch_normalization over the last axis in training
mode, momentum 0.99, epsilon 1e-3, + the ReLU behind it), numpy only, on the fp32 arrays the kernel is handed; eps and momentum cross
the C ABI as `float` and are rounded to fp32 first.

    mean = sum x / n                var = sum (x - mean)^2 / n  (biased)         rstd = 1 / sqrt(var + eps)
    xhat = (x - mean) rstd          y = [relu](gamma xhat + beta)                g = dy (y > 0 if relu)
    dbeta += sum g                  dgamma += sum g xhat                         dx = gamma rstd (g - sum g / n - xhat sum g xhat / n)
    moving_mean' = (1 - m) moving_mean + m mean
    moving_var'  = (1 - m) moving_var + m var n / (n - 1)                         (n > 1; var itself at n = 1)

reference()   float64.
eval32()      the same formulas in plain float32 numpy: whole-column two-pass, no blocking (columns made contiguous first, so that
              numpy's own pairwise summation applies; over the leading axis of a row-major array it would add 4099 rows one by one).
emulate32()   float32 with the kernel's rounding points: 256-row blocks of 16 row lanes x 16 rows (a lane adds its rows i x 16 + lane
              in order, the lanes are added in order), the block's mean, then its centred sum of squares (fused multiply-add), Chan's
              combination of the blocks in block order; the backward sums per lane, per block, then in block order.
gap()         per output, the larger of the two fp32 evaluations' distances to reference().  Both are references: neither is the
              code under test.  bars() turns it into the bar a device result is held to: max(4 x gap, floor) -- two correct fp32
              evaluations can each sit a full gap from float64 on opposite sides, a further 2 covers sqrtf, the division and the
              compiler's choice of fused multiply-adds against numpy's; floor = 1e-6 absolute (y, mean, rstd, moving buffers),
              1e-6 x the reference's largest magnitude (dx, dgamma, dbeta).  No bar is taken from the device's output.

The moving variance: the kernel feeds n / (n - 1) x var into it at every call site (moving(bessel=True)).  TF 1.13 does so on its
fused path, which only rank-4 inputs take (the two conv sites); the rank-3 [B, T, C] sites of the recurrent layers go through
nn.moments, which is biased (moving(bessel=False)).  bessel_deviation() gives the size of the difference; it is left as it is
(DESIGN section 4, K3b)."""
import functools

import numpy as np

F32, F64 = np.float32, np.float64
EPS, MOMENTUM = 1e-3, 0.01
BLOCK, LANES, PER_LANE = 256, 16, 16          # rows of a statistics block = row lanes x rows a thread holds (csrc/bn.hip BN_RL, BN_MAXR)
COLS = 64                                      # columns of a statistics workgroup
MM0, MV0 = 0.25, 3.0                           # where make_case starts the moving buffers
FORWARD = ("mean", "rstd", "y", "mm", "mv")
BACKWARD = ("dx", "dgamma", "dbeta")
OUTPUTS = FORWARD + BACKWARD
KINDS = ("plain", "offset", "tiny", "const", "outlier")
MUTANTS = ("one_pass_var", "moving_var_biased", "rstd_from_unbiased", "drop_tail_block", "tail_columns_unreduced", "inv_rows_per_block",
           "relu_mask_ge", "grads_overwrite", "moving_not_updated")

# (rows, C, relu, data kind): what tests/test_gpu_bn.py runs.  Two neighbouring rows differ in one field.  Rows: 2 and 15 (less than
# one lane's worth), 16 / 17 (one row per lane / one lane with two), 255 / 256 / 257 and 513 (one block short of a row, full, one
# row into the next), 4099 (17 blocks, the last with 3 rows).  Columns: 4 and 8 (one and two float4 lanes), 60 / 64 / 68 and 132 (a
# column block short of a lane, full, one lane into the next), 256 / 260 (the finalize kernels' 256 threads) and 512 (run.sh's).
TABLE = [
    (2, 4, 1, "plain"),
    (2, 4, 0, "plain"),
    (15, 4, 0, "plain"),
    (15, 8, 0, "plain"),
    (16, 8, 0, "plain"),
    (16, 8, 1, "plain"),
    (17, 8, 1, "plain"),
    (17, 60, 1, "plain"),
    (17, 60, 1, "tiny"),
    (255, 60, 1, "tiny"),
    (255, 64, 1, "tiny"),
    (256, 64, 1, "tiny"),
    (256, 64, 1, "const"),
    (257, 64, 1, "const"),
    (257, 68, 1, "const"),
    (257, 68, 0, "const"),
    (257, 68, 0, "offset"),
    (257, 132, 0, "offset"),
    (513, 132, 0, "offset"),
    (513, 132, 1, "offset"),
    (513, 132, 1, "outlier"),
    (513, 260, 1, "outlier"),
    (4099, 260, 1, "outlier"),
    (4099, 260, 1, "plain"),
    (4099, 256, 1, "plain"),
    (4099, 512, 1, "plain"),
]


def f32(v):
    """the value a C `float` argument takes"""
    return float(F32(v))


def row_id(row):
    return "%dx%d-%s-%s" % (row[0], row[1], "relu" if row[2] else "lin", row[3])


# ---------------------------------------------------------------------------------------------------------------- float64
def moving(mean, var, n, mm, mv, momentum=MOMENTUM, bessel=True):
    """one update of the moving statistics in float64 -> (moving_mean', moving_var').  bessel=True is the kernel's documented choice
    (var n / (n - 1) for n > 1, else var); bessel=False is TF 1.13's non-fused rule, which nothing runs against the kernel."""
    m = f32(momentum)
    mean, var, mm, mv = (np.asarray(a, F64) for a in (mean, var, mm, mv))
    fed = var * (float(n) / (n - 1.0)) if (bessel and n > 1) else var
    return (1.0 - m) * mm + m * mean, (1.0 - m) * mv + m * fed


def reference(x, gamma, beta, dy, relu, mask=None, eps=EPS, dgamma0=None, dbeta0=None, mm=None, mv=None, momentum=MOMENTUM):
    """float64 on the fp32 inputs -> dict: mean, var (biased), rstd, y, pre (y before the ReLU), mask, and with dy: dx, dgamma, dbeta (dgamma0 / dbeta0 + the
    sums: what a buffer that held them holds afterwards); with mm / mv: the moving buffers after one update (bessel=True).
    mask=None: the ReLU's mask is this function's own y > 0; a given mask is used as it is (the device test hands over the kernel's
    own y > 0, so that a flip at the kink does not spill into the gradients)."""
    x, gamma, beta = (np.asarray(a, F64) for a in (x, gamma, beta))
    n = x.shape[0]
    mean = x.mean(axis=0)
    xc = x - mean
    var = (xc * xc).mean(axis=0)
    rstd = 1.0 / np.sqrt(var + f32(eps))
    xhat = xc * rstd
    y = xhat * gamma + beta
    own = y > 0
    out = {"mean": mean, "var": var, "rstd": rstd, "pre": y, "y": np.where(own, y, 0.0) if relu else y, "mask": own if (mask is None or not relu) else np.asarray(mask, bool)}
    if mm is not None:
        out["mm"], out["mv"] = moving(mean, var, n, mm, mv, momentum, bessel=True)
    if dy is not None:
        g = np.asarray(dy, F64)
        if relu:
            g = g * out["mask"]
        sb, sg = g.sum(axis=0), (g * xhat).sum(axis=0)
        out["dx"] = gamma * rstd * (g - sb / n - xhat * (sg / n))
        out["dbeta"] = sb + (0.0 if dbeta0 is None else np.asarray(dbeta0, F64))
        out["dgamma"] = sg + (0.0 if dgamma0 is None else np.asarray(dgamma0, F64))
    return out


def eval_infer(x, gamma, beta, mm, mv, relu, eps=EPS):
    """float64 inference-mode batch norm on given moving buffers (what las.layers.bn(x, False) states)"""
    x, gamma, beta, mm, mv = (np.asarray(a, F64) for a in (x, gamma, beta, mm, mv))
    y = (x - mm) / np.sqrt(mv + f32(eps)) * gamma + beta
    return np.maximum(y, 0.0) if relu else y


def eval_infer32(x, gamma, beta, mm, mv, relu, eps=EPS):
    """eval_infer()'s formula in float32"""
    x, gamma, beta, mm, mv = (np.asarray(a, F32) for a in (x, gamma, beta, mm, mv))
    y = (x - mm) / np.sqrt(mv + F32(eps)) * gamma + beta
    return np.maximum(y, F32(0.0)) if relu else y


def bessel_deviation(n, var=1.0, momentum=MOMENTUM):
    """moving(bessel=True) - moving(bessel=False) in the moving variance after one update, for a batch variance `var` over n rows"""
    a = moving(0.0, var, n, 0.0, 1.0, momentum, bessel=True)[1]
    b = moving(0.0, var, n, 0.0, 1.0, momentum, bessel=False)[1]
    return float(a - b)


# ---------------------------------------------------------------------------------------------------------------- float32
def _moving32(mean, var_fed, mm, mv, momentum):
    m = F32(momentum)
    keep = F32(1.0) - m
    return keep * np.asarray(mm, F32) + m * mean, keep * np.asarray(mv, F32) + m * var_fed


def eval32(x, gamma, beta, dy, relu, mask=None, eps=EPS, dgamma0=None, dbeta0=None, mm=None, mv=None, momentum=MOMENTUM):
    """reference()'s formulas in plain float32: whole-column two-pass, no blocking"""
    x, gamma, beta = (np.asarray(a, F32) for a in (x, gamma, beta))
    n = x.shape[0]
    nf = F32(n)
    xt = np.ascontiguousarray(x.T)                                         # [C, rows]: the sums below run along the contiguous axis
    mean = xt.sum(axis=1, dtype=F32) / nf
    xc = xt - mean[:, None]
    var = (xc * xc).sum(axis=1, dtype=F32) / nf
    rstd = F32(1.0) / np.sqrt(var + F32(eps))
    xhat = xc * rstd[:, None]
    y = xhat * gamma[:, None] + beta[:, None]
    own = y > 0
    if relu:
        y = np.where(own, y, F32(0.0))
    out = {"mean": mean, "var": var, "rstd": rstd, "y": np.ascontiguousarray(y.T)}
    if mm is not None:
        out["mm"], out["mv"] = _moving32(mean, var * (nf / (nf - F32(1.0))) if n > 1 else var, mm, mv, momentum)
    if dy is not None:
        g = np.ascontiguousarray(np.asarray(dy, F32).T)
        if relu:
            g = g * (own if mask is None else np.asarray(mask, bool).T)
        sb, sg = g.sum(axis=1, dtype=F32), (g * xhat).sum(axis=1, dtype=F32)
        inv = F32(1.0) / nf
        dx = (gamma * rstd)[:, None] * (g - (sb * inv)[:, None] - xhat * (sg * inv)[:, None])
        out["dx"] = np.ascontiguousarray(dx.T)
        out["dbeta"] = sb if dbeta0 is None else np.asarray(dbeta0, F32) + sb
        out["dgamma"] = sg if dgamma0 is None else np.asarray(dgamma0, F32) + sg
    return out


def _fma(a, b, c):
    """fused multiply-add of fp32 arrays: the product is exact in float64, one rounding to float64 and one to fp32"""
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def _blocks(a, S):
    """[rows, C] -> [S, PER_LANE, LANES, C], padded with zeros (row i x 16 + lane of a block at [i, lane])"""
    rows, C = a.shape
    pad = np.zeros((S * BLOCK, C), F32)
    pad[:rows] = a
    return pad.reshape(S, PER_LANE, LANES, C)


def _lane_sum(b):
    """[S, PER_LANE, LANES, C] -> [S, C]: every lane adds its rows in order, then the lanes are added in order"""
    acc = np.zeros(b.shape[:1] + b.shape[2:], F32)
    for i in range(PER_LANE):
        acc = acc + b[:, i]
    tot = np.zeros((b.shape[0], b.shape[3]), F32)
    for q in range(LANES):
        tot = tot + acc[:, q]
    return tot


def emulate32(x, gamma, beta, dy, relu, mask=None, eps=EPS, dgamma0=None, dbeta0=None, mm=None, mv=None, momentum=MOMENTUM, mutant=None):
    """float32 with the kernel's rounding points (see the module's header); mutant: one planted defect out of MUTANTS"""
    assert mutant is None or mutant in MUTANTS, mutant
    x, gamma, beta = (np.asarray(a, F32) for a in (x, gamma, beta))
    rows, C = x.shape
    S = (rows + BLOCK - 1) // BLOCK
    S_used = rows // BLOCK if (mutant == "drop_tail_block" and rows >= BLOCK) else S
    nrow = np.minimum(BLOCK, rows - BLOCK * np.arange(S)).astype(F32)
    valid = (np.arange(S * BLOCK) < rows).reshape(S, PER_LANE, LANES, 1)
    xb = _blocks(x, S)
    # statistics: the block's mean, then its centred sum of squares
    bmean = _lane_sum(xb) / nrow[:, None]
    d = np.where(valid, xb - bmean[:, None, None, :], F32(0.0))
    q2 = np.zeros((S, LANES, C), F32)
    for i in range(PER_LANE):
        q2 = _fma(d[:, i], d[:, i], q2)
    bm2 = np.zeros((S, C), F32)
    for q in range(LANES):
        bm2 = bm2 + q2[:, q]
    # Chan's combination in block order
    n, mu, m2 = F32(0.0), np.zeros(C, F32), np.zeros(C, F32)
    for s in range(S_used):
        nb = nrow[s]
        nt = n + nb
        dl = bmean[s] - mu
        mu = mu + dl * (nb / nt)
        m2 = m2 + (bm2[s] + dl * dl * (n * nb / nt))
        n = nt
    if mutant == "one_pass_var":
        xt = np.ascontiguousarray(x.T)
        m2 = ((xt * xt).sum(axis=1, dtype=F32) / n - mu * mu) * n
    if mutant == "tail_columns_unreduced":
        mu[C // COLS * COLS:] = 0.0
        m2[C // COLS * COLS:] = 0.0
    var = m2 / n
    unb = m2 / (n - F32(1.0)) if n > 1 else var
    rstd = F32(1.0) / np.sqrt((unb if mutant == "rstd_from_unbiased" else var) + F32(eps))
    out = {"mean": mu, "var": var, "rstd": rstd}
    if mm is not None:
        if mutant == "moving_not_updated":
            out["mm"], out["mv"] = np.asarray(mm, F32).copy(), np.asarray(mv, F32).copy()
        else:
            out["mm"], out["mv"] = _moving32(mu, var if mutant == "moving_var_biased" else unb, mm, mv, momentum)
    xhat = (x - mu) * rstd
    y = xhat * gamma + beta
    if relu:
        y = np.maximum(y, F32(0.0))
    out["y"] = y
    if dy is not None:
        g = np.asarray(dy, F32)
        if relu:
            g = np.where((y >= 0) if mutant == "relu_mask_ge" else (y > 0) if mask is None else np.asarray(mask, bool), g, F32(0.0))
        gb, hb = _blocks(g, S), _blocks(xhat, S)
        sbl, sgl = np.zeros((S, LANES, C), F32), np.zeros((S, LANES, C), F32)
        for i in range(PER_LANE):
            sbl = sbl + gb[:, i]
            sgl = _fma(gb[:, i], hb[:, i], sgl)
        pb, pg = np.zeros((S, C), F32), np.zeros((S, C), F32)
        for q in range(LANES):
            pb, pg = pb + sbl[:, q], pg + sgl[:, q]
        sb, sg = np.zeros(C, F32), np.zeros(C, F32)
        for s in range(S_used):
            sb, sg = sb + pb[s], sg + pg[s]
        inv = F32(1.0) / F32(BLOCK if mutant == "inv_rows_per_block" else rows)
        out["dx"] = (gamma * rstd) * (g - sb * inv - xhat * sg * inv)
        keep = mutant != "grads_overwrite"
        out["dbeta"] = sb if (dbeta0 is None or not keep) else np.asarray(dbeta0, F32) + sb
        out["dgamma"] = sg if (dgamma0 is None or not keep) else np.asarray(dgamma0, F32) + sg
    return out


# ---------------------------------------------------------------------------------------------------------------- cases and bars
def make_case(row, seed=None):
    """deterministic fp32 inputs of a TABLE row (seed: other inputs of the same shape and kind)"""
    rows, C, relu, kind = row
    rng = np.random.RandomState((1000 * rows + 7 * C + 3 * KINDS.index(kind) + int(relu) if seed is None else seed) % (2 ** 31))
    gamma = rng.uniform(0.5, 1.5, C)
    beta = rng.randn(C) * 0.2
    const_cols = np.zeros(C, bool)
    if kind == "plain":
        x = rng.randn(rows, C) * 0.7 + 0.3
    elif kind == "offset":
        x = rng.permutation(np.linspace(100.0, 300.0, C)) + 0.5 * rng.randn(rows, C)
    elif kind == "tiny":
        x = 1e-3 * rng.randn(rows, C)
    elif kind == "const":
        x = rng.randn(rows, C) * 0.7 + 0.3
        const_cols[::4] = True
        x[:, const_cols] = 2.5
        beta[const_cols] = 0.0
    elif kind == "outlier":
        x = rng.randn(rows, C)
        x[rows // 2] = 1e4
    else:
        raise ValueError(kind)
    dy = rng.randn(rows, C) + 0.5
    f = lambda a: np.ascontiguousarray(a, dtype=F32)
    return {"row": tuple(row), "rows": rows, "C": C, "relu": bool(relu), "kind": kind, "x": f(x), "gamma": f(gamma), "beta": f(beta), "dy": f(dy),
            "dgamma0": f(rng.uniform(0.5, 1.5, C)), "dbeta0": f(rng.uniform(-1.5, -0.5, C)), "mm0": np.full(C, MM0, F32),
            "mv0": np.full(C, MV0, F32), "const_cols": const_cols}


def run(fn, case, mask=None, **kw):
    """fn (reference / eval32 / emulate32) on a case's inputs, gradient and moving buffers included"""
    return fn(case["x"], case["gamma"], case["beta"], case["dy"], case["relu"], mask=mask, dgamma0=case["dgamma0"], dbeta0=case["dbeta0"],
              mm=case["mm0"], mv=case["mv0"], **kw)


def distance(out, ref, keys=OUTPUTS):
    """{output: max |out - ref|} (NaN or inf anywhere -> inf)"""
    res = {}
    for k in keys:
        if k not in out or k not in ref:
            continue
        e = np.abs(np.asarray(out[k], F64) - ref[k])
        res[k] = float(e.max()) if np.all(np.isfinite(e)) else float("inf")
    return res


def gap(case, ref=None):
    """{output: the larger of eval32's and emulate32's distance to reference()}, every evaluation on the reference's own ReLU mask"""
    ref = run(reference, case) if ref is None else ref
    a, b = distance(run(eval32, case, mask=ref["mask"]), ref), distance(run(emulate32, case, mask=ref["mask"]), ref)
    return {k: max(a[k], b[k]) for k in a}


def floors(ref):
    fl = {k: 1e-6 for k in FORWARD}
    fl.update({k: 1e-6 * float(np.abs(ref[k]).max()) for k in BACKWARD if k in ref})
    return fl


def bars(case, ref=None, g=None):
    """{output: max(4 x gap, floor)} -- the bar a device result is held to (see the module's header)"""
    ref = run(reference, case) if ref is None else ref
    g, fl = gap(case, ref) if g is None else g, floors(ref)
    return {k: max(4.0 * g[k], fl[k]) for k in g}


def prepare(case):
    """(case, reference on its own mask, gap, bars)"""
    ref = run(reference, case)
    g = gap(case, ref)
    return case, ref, g, bars(case, ref, g)


@functools.lru_cache(maxsize=None)
def table_case(row):
    """prepare() of a TABLE row, computed once and left unchanged"""
    return prepare(make_case(row))


def judge(prep, out):
    """A result `out` (the device's, or an emulation's) for a prepared case, the way tests/test_gpu_bn.py judges it: the reference is
    handed the result's own mask y > 0 -> ({output: error / bar}, mask disagreements outside the kink, non-zeros on the constant columns)."""
    case, ref, _, bar = prep
    own = np.asarray(out["y"]) > 0
    r = run(reference, case, mask=own) if case["relu"] else ref
    err = distance(out, r)
    far = np.abs(ref["pre"]) > bar["y"]
    flips = int(np.count_nonzero((own != ref["mask"]) & far)) if case["relu"] else 0
    nonzero = int(np.count_nonzero(np.asarray(out["y"])[:, case["const_cols"]]))
    return {k: (err[k] / bar[k]) for k in err}, flips, nonzero


def kink_share(row):
    """the share of elements within the y bar of the ReLU's kink (constant columns left out): where the device's mask may differ"""
    case, ref, _, bar = table_case(tuple(row))
    y = ref["pre"][:, ~case["const_cols"]]
    return float(np.count_nonzero(np.abs(y) <= bar["y"])) / y.size


def make_chunk(rows, chunk, relu=True, width=COLS, seed=65552):
    """the `plain` case of columns [chunk x width, (chunk + 1) x width) of a wide input, from a counter-based seed: a large case is
    generated, referenced and judged one column block at a time (every formula above is per column)"""
    rng = np.random.Generator(np.random.Philox(key=seed + chunk))
    f = lambda a: np.ascontiguousarray(a, dtype=F32)
    x = rng.standard_normal((rows, width), dtype=F32) * F32(0.7) + F32(0.3)
    dy = rng.standard_normal((rows, width), dtype=F32) + F32(0.5)
    return {"row": (rows, width, int(relu), "plain"), "rows": rows, "C": width, "relu": bool(relu), "kind": "plain", "x": x,
            "gamma": f(rng.uniform(0.5, 1.5, width)), "beta": f(rng.standard_normal(width) * 0.2), "dy": dy, "dgamma0": f(rng.uniform(0.5, 1.5, width)),
            "dbeta0": f(rng.uniform(-1.5, -0.5, width)), "mm0": np.full(width, MM0, F32), "mv0": np.full(width, MV0, F32),
            "const_cols": np.zeros(width, bool)}
