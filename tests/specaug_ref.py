"""The statement of "apply a SpecAugment plan" (include/las_hip.h las_specaug) in numpy: float64, and the same formula evaluated in
float32 -- the yardstick of the device's bar (tests/test_gpu_specaug.py: max |gpu - float64| <= max(4 x gap, 1e-6)).

A plan row is {len, w0, w, 0, (f0, fw) x mF, (t0, tw) x mT}.  Frames t >= len, frames under a time mask and bins under a frequency
mask are +0 by a select (whatever lies underneath, NaN included).  Elsewhere output frame t reads the source at an exact rational
position: on the left of the control point (t <= w0 + w) i0 = (t w0) // (w0 + w), r = (t w0) % (w0 + w); on the right
i0 = w0 + ((t - w0 - w)(len - 1 - w0)) // (len - 1 - w0 - w), r the remainder; the value is x[i0] + (r / den)(x[i0 + 1] - x[i0]), and
x[i0] itself (x[i0 + 1] unread) when r == 0.  w == 0 is no warp."""
import numpy as np


def source_frames(length, w0, w):
    """(i0, r, den) int64 arrays over the output frames 0 .. length - 1"""
    t = np.arange(length, dtype=np.int64)
    if w == 0:
        return t, np.zeros(length, np.int64), np.ones(length, np.int64)
    assert 1 <= w0 <= length - 2 and 1 <= w0 + w <= length - 2, (length, w0, w)
    left = t <= w0 + w
    num = np.where(left, t * w0, (t - (w0 + w)) * (length - 1 - w0))
    den = np.where(left, w0 + w, length - 1 - w0 - w)
    return np.where(left, 0, w0) + num // den, num % den, den


def masks(row, T, F, mF, mT):
    """(frame mask [T], bin mask [F]) of a plan row: True = zero"""
    length = int(row[0])
    tm = np.arange(T) >= length
    fm = np.zeros(F, bool)
    for m in range(mF):
        f0, fw = int(row[4 + 2 * m]), int(row[5 + 2 * m])
        assert 0 <= f0 and 0 <= fw and f0 + fw <= F
        fm[f0:f0 + fw] = True
    for m in range(mT):
        t0, tw = int(row[4 + 2 * mF + 2 * m]), int(row[5 + 2 * mF + 2 * m])
        assert 0 <= t0 and 0 <= tw and t0 + tw <= length
        tm[t0:t0 + tw] = True
    return tm, fm


def apply(x, plan, mF, mT, dtype=np.float64):
    """x [B, T, F, C] (any float type) -> the augmented cube in `dtype`: every operation of the formula rounded to `dtype` (float32:
    frac = r / den, d = x[i0 + 1] - x[i0], frac * d, + x[i0]: one rounding more than the device's fmaf)."""
    x = np.asarray(x)
    B, T, F, C = x.shape
    out = np.zeros((B, T, F, C), dtype)
    for b in range(B):
        row = np.asarray(plan[b])
        length = int(row[0])
        assert 0 <= length <= T
        if length == 0:
            continue
        i0, r, den = source_frames(length, int(row[1]), int(row[2]))
        xs = x[b, :length].astype(dtype)
        y = xs[i0].copy()                                             # r == 0: a bit copy
        k = np.nonzero(r)[0]
        if len(k):
            frac = (r[k].astype(dtype) / den[k].astype(dtype))[:, None, None]
            x0, x1 = xs[i0[k]], xs[i0[k] + 1]
            y[k] = (frac * (x1 - x0)).astype(dtype) + x0
        tm, fm = masks(row, T, F, mF, mT)
        y[tm[:length]] = 0
        y[:, fm] = 0
        out[b, :length] = y
    return out


def ref64(x, plan, mF, mT):
    return apply(x, plan, mF, mT, np.float64)


def ref32(x, plan, mF, mT):
    return apply(np.asarray(x, np.float32), plan, mF, mT, np.float32)


def gap(x, plan, mF, mT):
    """max |float32 evaluation - float64| over the elements where both are finite numbers"""
    with np.errstate(invalid="ignore"):
        a, b = ref32(x, plan, mF, mT).astype(np.float64), ref64(x, plan, mF, mT)
    return float(np.nanmax(np.abs(a - b))) if a.size else 0.0


def make_plan(rows, mF, mT):
    """int32 [B, ldp] from rows of (len, w0, w, [(f0, fw), ...], [(t0, tw), ...]); missing masks are zero-width"""
    ldp = (4 + 2 * (mF + mT) + 3) & ~3
    plan = np.zeros((len(rows), ldp), np.int32)
    for b, (length, w0, w, fms, tms) in enumerate(rows):
        assert len(fms) <= mF and len(tms) <= mT
        plan[b, :3] = (length, w0, w)
        for m, (f0, fw) in enumerate(fms):
            plan[b, 4 + 2 * m:6 + 2 * m] = (f0, fw)
        for m, (t0, tw) in enumerate(tms):
            plan[b, 4 + 2 * mF + 2 * m:6 + 2 * mF + 2 * m] = (t0, tw)
    return plan
