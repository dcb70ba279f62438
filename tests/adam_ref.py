"""CPU restatement of K9 (csrc/loss_opt.hip: las_sumsq + las_clip_adam = tf.clip_by_global_norm + tf.train.AdamOptimizer in its
epsilon-hat form), numpy float64, taking EXACTLY what the kernel is handed: the buffers, the fp32 sum of squares it reads (or None),
and the scalars that cross the C ABI as `float` -- clip, lr_t, beta1, beta2, eps are rounded to fp32 first (1 - 0.999f differs from
0.001 by 1.3e-5 relative: far outside the bounds below).

    gs     = clip / max(sqrt(sumsq), clip)            (clip > 0; else 1)
    gc     = g gs
    m'     = b1 m + (1 - b1) gc
    v'     = b2 v + (1 - b2) gc^2
    theta' = theta - lr_t m' / (sqrt(v') + eps)

Bounds of an fp32 evaluation of these expressions against this reference, per element, by counting roundings u = 2^-24 (IEEE sqrtf and
division: the library is built without fast-math; FMA contraction only removes roundings; 1.f - b1 and 1.f - b2 are exact in fp32):

    m'      2^-22 (|b1 m| + |(1 - b1) gc|)               gs carries sqrtf and the division (2u), g gs one more, the sum one (the
                                                         device fuses the product with 1 - b1 into it); the b1 m term its product
                                                         and the sum
    v'      2^-21 (b2 v + (1 - b2) gc^2)                 gc is squared: its error counts twice, then two products and the sum
    theta'  2^-23 |theta'| + 3 2^-22 |theta' - theta| + 2^-22 lr_t (|b1 m| + |(1 - b1) gc|) / (sqrt(v') + eps)
                                                         the final subtraction; the update carries sqrt(v') (half of 8u, and sqrtf),
                                                         + eps, lr_t m' and the division -- and m', whose 4u are 4u of
                                                         |b1 m| + |(1 - b1) gc|, NOT of |m'| (see below)
    sumsq   relative d 2^-24, d = ceil(n / (4 262144)) + 40
                                                         a thread's chain of n / (4 x 1024 x 256) float4 terms, four products and three
                                                         sums per float4, the tail, and three reduction trees (block 8 + 2, final 6 + 4 + 16
                                                         at the very most); every term is >= 0, so the bound is relative

The theta' row as first written was 2^-23 |theta'| + 2^-20 |theta' - theta|: 16u on the update, 4u of them for m'.  That counts
the roundings of m' as relative to m' itself.  They are relative to the two terms m' is the sum of, and where b1 m and (1 - b1) gc
cancel (|m'| a hundredth of the terms: one element in a few hundred when g changes sign between steps) the update is small and the
error it inherits from m' is not.  The fp32 emulation shows it without a GPU: at n = 3000003 (the order of the grid-stride case of
tests/test_gpu_optimizer.py) it reaches 1.33 times the first form on elements with |theta| ~ 1e-5 and |m'| = 0.03 (|b1 m| + ...),
while every element without cancellation stays below 0.5.  So the 4u that belong to m' are taken out of the 16u on |theta' - theta|
and charged to what they are proportional to; without cancellation the two forms are the same number.

The bounds are relative: they assume that no intermediate leaves fp32's normal range (|gc| >= 1e-17 or gc = 0 exactly).
A numpy fp32 emulation of the kernel's expression order (tests/test_adam_ref_host.py; one rounding per operation, one more than the
device, which fuses (1 - b1) gc and gc (1 - b2) gc into the sums) stays within 0.78 (m'), 0.72 (v') and 0.50 (theta') of these bounds
over 6 steps at n = 100003 with |g| over nine decades; the same file shows that six plausible mistakes in the kernel land 10^3 to
10^10 times outside them.  Measured on the MI355X (tests/test_gpu_optimizer.py, n up to 6291459, clip binding): 0.69 (m'), 0.69 (v'),
0.4999 (theta'); las_sumsq 1.2e-7 relative against a bound of 2.4e-6.

A trajectory of several steps is another matter: see Trajectory below."""
import math

import numpy as np

M_BOUND, V_BOUND = 2.0 ** -22, 2.0 ** -21
TH_BOUND, UPD_BOUND, M_UPD_BOUND = 2.0 ** -23, 3 * 2.0 ** -22, 2.0 ** -22


def f32(x):
    """the value a C `float` argument takes"""
    return float(np.float32(x))


def lr_t(lr, t, b1=0.9, b2=0.999):
    """the bias-corrected rate of step t (1-based), in double as the host computes it before it crosses the ABI"""
    return lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)


def sumsq_ref(g):
    g = np.asarray(g, np.float64).reshape(-1)
    return float(np.sum(g * g))


def sumsq_bound(n):
    """relative bound of las_sumsq over n elements"""
    return (math.ceil(n / (4.0 * 262144)) + 40) * 2.0 ** -24


def clip_scale(sumsq, clip):
    clip = f32(clip)
    if clip <= 0.0:
        return 1.0
    return clip / max(math.sqrt(float(sumsq)), clip)


def step(theta, g, m, v, sumsq, clip, lr_t, b1, b2, eps):
    """-> theta', m', v', terms.  terms: 'm' = |b1 m| + |(1 - b1) gc|, 'v' = b2 v + (1 - b2) gc^2, 'upd' = |theta' - theta|
    'm_upd' = lr_t terms['m'] / (sqrt(v') + eps) (what the bounds are multiples of) and 'gs'."""
    theta, g, m, v = (np.asarray(a, np.float64) for a in (theta, g, m, v))
    lr_t, b1, b2, eps = f32(lr_t), f32(b1), f32(b2), f32(eps)
    if f32(clip) > 0.0 and sumsq is None:
        raise ValueError("clipping needs the sum of squares")
    gs = clip_scale(sumsq, clip) if f32(clip) > 0.0 else 1.0
    gc = g * gs
    m2 = b1 * m + (1.0 - b1) * gc
    v2 = b2 * v + (1.0 - b2) * gc * gc
    theta2 = theta - lr_t * m2 / (np.sqrt(v2) + eps)
    tm = np.abs(b1 * m) + np.abs((1.0 - b1) * gc)
    terms = {"m": tm, "v": v2, "upd": np.abs(theta2 - theta), "m_upd": lr_t * tm / (np.sqrt(v2) + eps), "gs": gs}
    return theta2, m2, v2, terms


def _ratio(err, bound):
    """max over the elements of err / bound; an element whose bound is 0 must be exact"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    if err.size == 0:
        return 0.0
    r = np.where(err == 0.0, 0.0, err / np.maximum(bound, 1e-300))
    return float(np.max(r)) if np.all(np.isfinite(r)) else float("inf")


def bounds(ref):
    """the per-element bounds of one step: {'m', 'v', 'theta'}; ref = step(...)'s return value"""
    theta2, m2, v2, terms = ref
    return {"m": M_BOUND * terms["m"], "v": V_BOUND * terms["v"],
            "theta": TH_BOUND * np.abs(theta2) + UPD_BOUND * terms["upd"] + M_UPD_BOUND * terms["m_upd"]}


def ratios(theta_d, m_d, v_d, ref, bound=None):
    """Worst error of an fp32 result (theta', m', v' arrays) as a multiple of the bounds above (or of `bound`, a dict like bounds());
    ref = step(...)'s return value.  Every entry must be <= 1."""
    bound = bounds(ref) if bound is None else bound
    return {k: _ratio(np.abs(np.asarray(d, np.float64) - r), bound[k]) for k, d, r in (("m", m_d, ref[1]), ("v", v_d, ref[2]), ("theta", theta_d, ref[0]))}


class Trajectory(object):
    """A float64 trajectory that never sees the fp32 state, with the bound of an fp32 trajectory's distance from it.  A step's own
    bound is not enough here: what m and v inherit from the step before is b1 / b2 times THAT step's error, however small this step's
    terms are, and theta' inherits both through the update.  To first order (x 1.001 for the rest; the errors are ~1e-6 relative):

        E_m'     = b1 E_m + bound_m                       E_v' = b2 E_v + bound_v
        E_theta' = E_theta + bound_theta + lr_t (b1 E_m + |m'| b2 E_v / (2 sqrt(v'))) / (sqrt(v') + eps)"""

    def __init__(self, theta, m, v):
        self.state = tuple(np.array(a, np.float64) for a in (theta, m, v))
        self.err = {k: np.zeros_like(self.state[0]) for k in ("theta", "m", "v")}

    def step(self, g, sumsq, clip, lr_t, b1, b2, eps):
        ref = step(self.state[0], g, self.state[1], self.state[2], sumsq, clip, lr_t, b1, b2, eps)
        b, e = bounds(ref), self.err
        sv = np.sqrt(ref[2])
        with np.errstate(divide="ignore", invalid="ignore"):
            dv = np.where(sv > 0, np.abs(ref[1]) * f32(b2) * e["v"] / (2.0 * sv), 0.0)
        carried = f32(lr_t) * (f32(b1) * e["m"] + dv) / (sv + f32(eps))
        self.err = {"theta": 1.001 * (e["theta"] + b["theta"] + carried), "m": f32(b1) * e["m"] + b["m"], "v": f32(b2) * e["v"] + b["v"]}
        self.state = ref[:3]
        self.ref = ref
        return ref

    def ratios(self, theta_d, m_d, v_d):
        return ratios(theta_d, m_d, v_d, self.ref, bound=self.err)
