"""Float64 references for the loss and dropout kernels: las_ce_loss (csrc/loss_opt.hip), las_ctc_loss (csrc/ctc.hip) and
las_dropout_pair_fwd / _bwd (csrc/common.hip).  No device, no file outside the repository; tests/test_loss_ref_host.py checks
everything here on the CPU, tests/test_gpu_ce_loss.py, test_gpu_ctc.py, test_gpu_ctc_edges.py and test_gpu_dropout.py use it.

  ce_ref           label-smoothed masked cross-entropy in float64: per-row ce * mask, the mask, sums[3], the gradient
  ce_emulate       the same with the kernel's fp32 rounding points (fp32 max, lane-strided fp32 sums, fp32 exp / log); only ever used
                   to DERIVE a bound, never as a reference
  ctc_ref          per-row torch.nn.functional.ctc_loss in float64 (nll, d nll / d logits)
  ctc_blank_only   closed form for L = 0: nll = -sum_t log p_blank
  ctc_single_path  closed form for L = k labels of ONE class at T = 2k - 1: label and blank alternate, exactly one path
  ctc_emulate      the kernel's recursion: fp64 carry, fp32 exp / log of the differences, fp32 log-softmax and posterior sums
  dropout_masks    the two directions' keep masks, splitmix64 in numpy uint64, element by element what the kernels draw

BOUNDS.  A bound is never taken from kernel output.  Two kinds:

  CE, a case "of the standing form" (logits ~ 2 N(0,1), V <= 8192, scale = 1 / n_tokens with n_tokens > 1): the bounds of
      test_ce_loss_with_the_row_in_registers_matches_float64, CE_LOSS_REL = 2e-6 on the loss relative to max(1, |loss|) and
      CE_GRAD_ABS = 2e-7 on the gradient.
  CE, any other case (scale 1, peaky rows, V = 8193): 4 x the worst |ce_emulate - ce_ref| over seeds 0..19 of the case's own generator
      (ce_bound; the loss error relative to max(1, |loss|), the gradient error absolute).  CE_BOUNDS records the values derived on
      the CPU; test_loss_ref_host.py re-derives them.
  CTC, T' <= 319: CTC_NLL_REL = 1e-5 relative to max(1, |nll|) and CTC_GRAD_ABS = 1e-5 absolute (tests/test_gpu_ctc.py, the range
      already measured).
  CTC, T' > 319 or peaky logits: max(1e-5, 4 x the worst |ctc_emulate - ctc_ref| over seeds 0..19) (ctc_bound, CTC_BOUNDS).

Derived bound (loss rel, grad abs) and, beside it, the worst error seen on an MI355X in the test that uses it:

  CE  scale1-v30           4.259e-07 / 1.005e-06      observed 3.5e-08 / 1.7e-07
  CE  rows1-v30            5.803e-07 / 5.859e-07      observed 1.2e-08 / 1.7e-07
  CE  rows2-v30            4.941e-07 / 6.120e-07      observed 2.5e-09 / 1.7e-07
  CE  rows3-v30            2.986e-07 / 6.120e-07      observed 1.8e-09 / 1.7e-07
  CE  rows5-v30            4.231e-07 / 6.234e-07      observed 1.9e-08 / 1.7e-07
  CE  rows1025-v30         7.830e-07 / 1.828e-06      observed 2.0e-08 / 3.0e-07
  CE  peaky-v30            3.232e-07 / 1.440e-05      observed 4.3e-08 / 1.4e-06
  CE  peaky-v5000          3.047e-07 / 3.039e-05      observed 3.8e-08 / 5.7e-06
  CE  pm80-v30             9.075e-07 / 1.005e-06      observed 2.1e-08 / 1.7e-07
  CE  v8193                3.699e-07 / 7.208e-08      observed 2.2e-08 / 7.2e-09
  CE  standing form        2e-6 / 2e-7 (not derived: the standing test's)      observed 2.8e-07 / 3.1e-08 (worst case)
  CTC max-L511-T540        1.000e-05 / 1.000e-05      observed 3.1e-08 / 1.0e-06
  CTC wide-U511-T540       1.000e-05 / 1.000e-05      observed 7.2e-09 / 2.5e-07
  CTC chain1-L200-T420     1.000e-05 / 1.000e-05      observed 3.9e-08 / 2.7e-07
  CTC chain2-L200-T420     1.000e-05 / 1.000e-05      observed 1.3e-08 / 5.2e-07
  CTC peaky-T160           1.000e-05 / 1.600e-05      observed 3.2e-08 / 2.0e-06
  CTC T' <= 319            1e-5 / 1e-5 (not derived: the standing test's)      observed 8.7e-08 / 6.2e-07 (worst case)
"""
import numpy as np

F32 = np.float32
CE_LOSS_REL, CE_GRAD_ABS = 2e-6, 2e-7
CTC_NLL_REL, CTC_GRAD_ABS = 1e-5, 1e-5
SEEDS = 20


# ================================================================================================ cross-entropy
def _soft(y, V, e):
    """soft targets [R, V] in float64; a label outside [0, V) has no one-hot term"""
    R = y.shape[0]
    soft = np.full((R, V), e / V, np.float64)
    ok = (y >= 0) & (y < V)
    soft[np.nonzero(ok)[0], y[ok]] += 1.0 - e
    return soft, ok


def ce_ref(logits, y, V, eps, smooth_bits, scale):
    """logits [..., V], y [...] int -> (ce * mask [...], mask [...], sums [3], grad [..., V]), all float64.
    bit 0 of smooth_bits: label smoothing with eps; bit 1: every position counts (mask = 1), otherwise mask = (y != 0).
    ce = lse - (1 - e) ly - (e / V) sum_k l_k, ly = 0 for a label outside [0, V); grad = scale mask (softmax - soft);
    sums = (sum ce mask, sum mask, scale sum ce mask)."""
    shape = np.shape(y)
    l = np.asarray(logits, np.float64).reshape(-1, V)
    yy = np.asarray(y, np.int64).reshape(-1)
    e = float(eps) if smooth_bits & 1 else 0.0
    mask = np.ones(yy.shape, np.float64) if smooth_bits & 2 else (yy != 0).astype(np.float64)
    m = l.max(-1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(l - m).sum(-1))
    soft, ok = _soft(yy, V, e)
    ly = np.where(ok, l[np.arange(len(yy)), np.clip(yy, 0, V - 1)], 0.0)
    ce = (lse - (1.0 - e) * ly - (e / V) * l.sum(-1)) * mask
    grad = float(scale) * mask[:, None] * (np.exp(l - lse[:, None]) - soft)
    sums = np.array([ce.sum(), mask.sum(), ce.sum() * float(scale)])
    return ce.reshape(shape), mask.reshape(shape), sums, grad.reshape(shape + (V,))


def _lane_sum32(x):
    """fp32 sum over the last axis the way a wave does it: lane j adds its elements j, j + 64, ... in order, then a tree over 64 lanes"""
    n = x.shape[-1]
    pad = (-n) % 64
    x = np.concatenate([x, np.zeros(x.shape[:-1] + (pad,), F32)], -1).reshape(x.shape[:-1] + (-1, 64))
    acc = np.zeros(x.shape[:-2] + (64,), F32)
    for i in range(x.shape[-2]):
        acc = acc + x[..., i, :]
    w = 32
    while w:
        acc = acc[..., :w] + acc[..., w:2 * w]
        w //= 2
    return acc[..., 0]


def _seq_sum32(x):
    s = F32(0)
    for v in np.asarray(x, F32).reshape(-1):
        s = F32(s + v)
    return s


def ce_emulate(logits, y, V, eps, smooth_bits, scale):
    """ce_ref with the kernel's rounding points: every operation in fp32 (max, lane-strided sums, exp, log, the products)"""
    shape = np.shape(y)
    l = np.asarray(logits, F32).reshape(-1, V)
    yy = np.asarray(y, np.int64).reshape(-1)
    e = F32(eps) if smooth_bits & 1 else F32(0)
    mask = np.ones(yy.shape, F32) if smooth_bits & 2 else (yy != 0).astype(F32)
    m = l.max(-1)
    lsum = _lane_sum32(l)
    se = _lane_sum32(np.exp(l - m[:, None]))
    lse = m + np.log(se)
    ok = (yy >= 0) & (yy < V)
    ly = np.where(ok, l[np.arange(len(yy)), np.clip(yy, 0, V - 1)], F32(0)).astype(F32)
    ce = ((lse - (F32(1) - e) * ly) - (e / F32(V)) * lsum) * mask
    soft = np.full(l.shape, e / F32(V), F32)
    soft[np.nonzero(ok)[0], yy[ok]] += F32(1) - e
    sc = F32(scale) * mask
    grad = sc[:, None] * (np.exp(l - lse[:, None]) - soft)
    # sum2_kernel: thread i adds rows i, i + 1024, ...; a tree over each wave; the 16 wave partials in order
    part = np.zeros((2, 1024), F32)
    for i in range(0, len(ce), 1024):
        n = min(1024, len(ce) - i)
        part[0, :n] += ce[i:i + n]
        part[1, :n] += mask[i:i + n]
    waves = _lane_sum32(part.reshape(2, 16, 64))
    t0, t1 = _seq_sum32(waves[0]), _seq_sum32(waves[1])
    sums = np.array([t0, t1, F32(t0 * F32(scale))], F32)
    assert ce.dtype == F32 and grad.dtype == F32
    return ce.reshape(shape), mask.reshape(shape), sums, grad.reshape(shape + (V,))


def ce_case(kind, seed):
    """the generators of the cases whose bound is derived: -> dict(logits [R, V] fp32, y [R], V, eps, smooth, scale)"""
    rng = np.random.RandomState(1000 + seed)
    R, V, mult = {"scale1-v30": (6, 30, 2.0), "rows1-v30": (1, 30, 2.0), "rows2-v30": (2, 30, 2.0), "rows3-v30": (3, 30, 2.0),
                  "rows5-v30": (5, 30, 2.0), "rows1025-v30": (1025, 30, 2.0), "peaky-v30": (6, 30, 40.0), "peaky-v5000": (6, 5000, 40.0),
                  "pm80-v30": (6, 30, 2.0), "v8193": (6, 8193, 2.0)}[kind]
    l = rng.randn(R, V) * mult
    if kind == "pm80-v30":                                # one logit at +80, the rest of the row at -80
        l[2] = -80.0
        l[2, rng.randint(V)] = 80.0
    y = rng.randint(1, V, size=R)
    if R > 1:
        y[1] = V - 1                                      # a label on the last class
    if R > 1000:
        y[rng.rand(R) < 0.1] = 0                          # PAD rows throughout, but not the last row: it is the only one of
        y[R - 1] = 7                                      # sum2_kernel's second trip, and a PAD row would add nothing there
    elif R > 2:
        y[R - 1] = 0                                      # one PAD row
    n = max(1, int((y != 0).sum()))
    scale = 1.0 / n if kind == "v8193" else 1.0           # (v8193: the standing form but for V; every other kind: scale 1)
    return dict(logits=l.astype(F32), y=y.astype(np.int32), V=V, eps=0.01, smooth=1, scale=scale)


def ce_errors(got_sums, got_grad, ref):
    """(loss error relative to max(1, |loss|) over sums[0] and sums[2], gradient error absolute)"""
    _, _, sums, grad = ref
    loss = max(abs(float(got_sums[k]) - sums[k]) / max(1.0, abs(sums[k])) for k in (0, 2))
    return loss, float(np.abs(np.asarray(got_grad, np.float64) - grad).max())


def ce_bound(kind, seeds=SEEDS):
    """4 x the worst |ce_emulate - ce_ref| over `seeds` draws of ce_case(kind): (loss rel, grad abs)"""
    worst = [0.0, 0.0]
    for s in range(seeds):
        c = ce_case(kind, s)
        a = (c["logits"], c["y"], c["V"], c["eps"], c["smooth"], c["scale"])
        _, _, sums, grad = ce_emulate(*a)
        e = ce_errors(sums, grad, ce_ref(*a))
        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
    return 4.0 * worst[0], 4.0 * worst[1]


CE_KINDS = ("scale1-v30", "rows1-v30", "rows2-v30", "rows3-v30", "rows5-v30", "rows1025-v30", "peaky-v30", "peaky-v5000", "pm80-v30", "v8193")
CE_BOUNDS = {               # kind: (loss rel, grad abs) = ce_bound(kind)
    "scale1-v30": (4.259e-07, 1.005e-06),
    "rows1-v30": (5.803e-07, 5.859e-07),
    "rows2-v30": (4.941e-07, 6.120e-07),
    "rows3-v30": (2.986e-07, 6.120e-07),
    "rows5-v30": (4.231e-07, 6.234e-07),
    "rows1025-v30": (7.830e-07, 1.828e-06),
    "peaky-v30": (3.232e-07, 1.440e-05),
    "peaky-v5000": (3.047e-07, 3.039e-05),
    "pm80-v30": (9.075e-07, 1.005e-06),
    "v8193": (3.699e-07, 7.208e-08),
}


# ================================================================================================ CTC
def ctc_ref(logits, labs, enc_len):
    """per-row nll and d(sum nll)/d logits, float64 on the CPU; None for rows torch cannot align (nll = inf)."""
    import torch
    import torch.nn.functional as F
    B, Tp, Vc = logits.shape
    nll, grad = [], []
    for b in range(B):
        x = torch.tensor(logits[b:b + 1], dtype=torch.float64, requires_grad=True)
        lp = torch.log_softmax(x, -1).transpose(0, 1)
        tg = torch.tensor(labs[b] if labs[b] else [0], dtype=torch.long).reshape(1, -1)
        l = F.ctc_loss(lp, tg, torch.tensor([int(enc_len[b])]), torch.tensor([len(labs[b])]), blank=Vc - 1, reduction="none",
                       zero_infinity=False)
        if not torch.isfinite(l).all():
            nll.append(float("inf"))
            grad.append(None)
            continue
        l.sum().backward()
        nll.append(float(l.detach()[0]))
        grad.append(x.grad[0].numpy())
    return nll, grad


def _log_softmax64(x):
    x = np.asarray(x, np.float64)
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def _path_form(logits, T, path):
    """nll and gradient of the single alignment `path` over the first T frames of logits [T', Vc]"""
    lp = _log_softmax64(logits[:T])
    grad = np.zeros(np.shape(logits), np.float64)
    grad[:T] = np.exp(lp)
    grad[np.arange(T), path] -= 1.0
    return float(-lp[np.arange(T), path].sum()), grad


def ctc_blank_only(logits, T):
    """L = 0: every frame emits the blank (the last class).  -> (nll, gradient [T', Vc], zero behind T)"""
    return _path_form(logits, T, np.full(T, np.shape(logits)[-1] - 1))


def ctc_single_path(logits, cls, k):
    """L = k labels, all of class cls, at T = 2k - 1 frames: cls, blank, cls, ..., cls is the only alignment"""
    T = 2 * k - 1
    path = np.full(T, np.shape(logits)[-1] - 1)
    path[0::2] = cls
    return _path_form(logits, T, path)


def _exp32(d):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.exp(np.asarray(d).astype(F32))


def _lse_n(*terms):
    """log(sum exp) of fp64 terms: fp64 maximum, fp32 exp of the differences, fp32 sum, fp32 log (lse2 / lse3 of csrc/ctc.hip)"""
    m = terms[0]
    for t in terms[1:]:
        m = np.maximum(m, t)
    with np.errstate(invalid="ignore", divide="ignore"):
        acc = None
        for t in terms:
            v = _exp32(t - m)
            acc = v if acc is None else (acc + v).astype(F32)
        out = m + np.log(acc).astype(np.float64)
    return np.where(np.isneginf(m), -np.inf, out)


def ctc_emulate(logits, labels, T):
    """one row, logits [T', Vc] fp32, labels a list, T frames -> (nll, gradient [T', Vc] fp32).  The kernels' rounding points: fp32
    log-softmax, log alpha / log beta carried in fp64 with fp32 exp / log of the differences, fp32 posteriors summed in fp32."""
    x = np.asarray(logits, F32)
    Tp, Vc = x.shape
    grad = np.zeros((Tp, Vc), F32)
    L = len(labels)
    S = 2 * L + 1
    if T <= 0:
        return (0.0 if L == 0 else np.inf), grad
    ext = np.full(S, Vc - 1, np.int64)
    ext[1::2] = labels
    xt = x[:T]
    m = xt.max(-1)
    lse = m + np.log(_lane_sum32(np.exp(xt - m[:, None])))
    glp = (xt[:, ext] - lse[:, None]).astype(np.float64)          # fp32 values
    s = np.arange(S)
    skip_in = (s & 1).astype(bool) & (s >= 3)
    skip_in[3:] &= ext[3:] != ext[1:-2]
    skip_out = np.zeros(S, bool)
    skip_out[:-2] = skip_in[2:]
    ninf = np.full(2, -np.inf)
    alpha = np.full((T, S), -np.inf)
    alpha[0, :min(S, 2)] = glp[0, :min(S, 2)]
    for t in range(1, T):
        p = np.concatenate([ninf, alpha[t - 1]])
        alpha[t] = _lse_n(p[2:], p[1:-1], np.where(skip_in, p[:-2], -np.inf)) + glp[t]
    logp = float(_lse_n(alpha[T - 1, S - 1], alpha[T - 1, S - 2])) if S >= 2 else float(alpha[T - 1, S - 1])
    if np.isneginf(logp):
        return np.inf, grad
    bt = np.where(s >= S - 2, 0.0, -np.inf)
    gam = np.zeros((T, Vc), F32)
    for t in range(T - 1, -1, -1):
        pr = _exp32(alpha[t] + bt - logp)
        np.add.at(gam[t], ext, pr)
        q = np.concatenate([glp[t] + bt, ninf])
        bt = _lse_n(q[:-2], q[1:-1], np.where(skip_out, q[2:], -np.inf))
    grad[:T] = np.exp(xt - lse[:, None]) - gam
    return float(F32(-logp)), grad


def no_adjacent_repeats(rng, n, lo, hi):
    """n labels in [lo, hi), no two neighbours equal"""
    lab = rng.randint(lo, hi, size=n)
    for i in range(1, n):
        while lab[i] == lab[i - 1]:
            lab[i] = rng.randint(lo, hi)
    return [int(v) for v in lab]


def ctc_case(kind, seed):
    """the generators of the CTC cases whose bound is derived: -> (logits [T', Vc] fp32, labels, T)"""
    rng = np.random.RandomState(2000 + seed)
    if kind == "max-L511-T540":
        Tp, Vc, lab = 540, 31, no_adjacent_repeats(rng, 511, 1, 30)
    elif kind == "wide-U511-T540":
        Tp, Vc, lab = 540, 31, [int(v) for v in rng.randint(1, 30, size=3)]
    elif kind == "chain1-L200-T420":
        Tp, Vc, lab = 420, 3, [1] * 200
    elif kind == "chain2-L200-T420":
        Tp, Vc, lab = 420, 4, [int(v) for v in rng.randint(1, 3, size=200)]
    elif kind == "peaky-T160":
        Tp, Vc = 160, 31
        lab = [int(v) for v in rng.randint(1, 30, size=40)]
        lab[2] = lab[1]
    else:
        raise KeyError(kind)
    logits = (rng.randn(Tp, Vc) * (30.0 if kind == "peaky-T160" else 2.0)).astype(F32)
    return logits, lab, Tp


def ctc_errors(nll, grad, nll_r, grad_r):
    return abs(nll - nll_r) / max(1.0, abs(nll_r)), float(np.abs(np.asarray(grad, np.float64) - grad_r).max())


def ctc_bound(kind, seeds=SEEDS):
    """max(1e-5, 4 x the worst |ctc_emulate - ctc_ref| over `seeds` draws of ctc_case(kind)): (nll rel, grad abs)"""
    worst = [0.0, 0.0]
    for sd in range(seeds):
        logits, lab, T = ctc_case(kind, sd)
        nll_r, grad_r = ctc_ref(logits[None], [lab], [T])
        assert np.isfinite(nll_r[0]), (kind, sd)
        e = ctc_errors(*ctc_emulate(logits, lab, T), nll_r[0], grad_r[0])
        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
    return max(CTC_NLL_REL, 4.0 * worst[0]), max(CTC_GRAD_ABS, 4.0 * worst[1])


CTC_KINDS = ("max-L511-T540", "wide-U511-T540", "chain1-L200-T420", "chain2-L200-T420", "peaky-T160")
CTC_BOUNDS = {              # kind: (nll rel, grad abs) = ctc_bound(kind); 1e-5 is the floor the standing test sets
    "max-L511-T540": (1.000e-05, 1.000e-05),
    "wide-U511-T540": (1.000e-05, 1.000e-05),
    "chain1-L200-T420": (1.000e-05, 1.000e-05),
    "chain2-L200-T420": (1.000e-05, 1.000e-05),
    "peaky-T160": (1.000e-05, 1.600e-05),
}


# ================================================================================================ dropout
GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M1, _M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def splitmix64_mix(z):
    """the output function of splitmix64 on an array of states (uint64, wrapping)"""
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
    return z ^ (z >> np.uint64(31))


def drop_bits(seed, direction, quad):
    """64 mask bits of quad (four elements) of one direction"""
    quad = np.asarray(quad, np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + GOLDEN * (np.uint64(2) * quad + np.uint64(direction + 1))
    return splitmix64_mix(z)


def drop_threshold(keep):
    """an element is kept iff its 16-bit slice is below floor(float32(keep) * 65536 + 0.5)"""
    t = float(F32(keep)) * 65536.0 + 0.5
    return 65536 if t >= 65536.0 else int(t)


def dropout_masks(seed, rows, K, keep):
    """-> (m_fw, m_bw) bool [rows, K]: quad = r * ceil(K / 4) + c // 4, element c % 4 takes bits 16 e .. 16 e + 15"""
    qpr = (K + 3) // 4
    quad = np.arange(rows * qpr, dtype=np.uint64)
    thr = np.uint64(drop_threshold(keep))
    out = []
    for d in (0, 1):
        bits = drop_bits(seed, d, quad)
        sl = np.stack([(bits >> np.uint64(16 * e)) & np.uint64(0xffff) for e in range(4)], -1)
        out.append((sl < thr).reshape(rows, qpr * 4)[:, :K])
    return out[0], out[1]
