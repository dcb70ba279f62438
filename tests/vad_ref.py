"""Numpy restatement of las_vad (include/las_hip.h K15) and of las.vad.plan_segments, written from the contract's words and
not from the kernels': the energies by a sequential double accumulation, the dilation as a window, the runs as maximal stretches."""
import numpy as np


def to_f32(x):
    """what the entry reads: fp32 as it is, int16 as value / 32767 in fp32 (as las_frontend)"""
    x = np.asarray(x)
    if x.dtype == np.int16:
        return x.astype(np.float32) / np.float32(32767)
    return x.astype(np.float32)


def frame_count(n, fl, step):
    return (n - fl) // step if n >= fl else 0


def energies(x, fl, step):
    """e[t] = sum over the frame's samples in ascending order of x x, from 0, in double (the product of two widened fp32 is exact).
    The loop runs over the position inside the frame and is vectorised over the frames: each frame's sum is still sequential."""
    x = to_f32(x).astype(np.float64)
    T = frame_count(len(x), fl, step)
    e = np.zeros(T, np.float64)
    first = np.arange(T) * step
    for i in range(fl):
        v = x[first + i]
        e = e + v * v
    return e


def flags(e, ratio, floor, hang):
    """(emax, raw, dilated)"""
    T = len(e)
    emax = float(e.max()) if T else 0.0
    thr = max(emax * ratio, floor)
    raw = (e >= thr) & (e > 0)
    s = np.zeros(T, bool)
    for t in range(T):
        s[t] = raw[max(0, t - hang):min(T, t + hang + 1)].any()
    return emax, raw, s


def runs_of(s, min_run):
    """maximal stretches [a, b) of a boolean sequence, those shorter than min_run dropped"""
    out, t, T = [], 0, len(s)
    while t < T:
        if s[t]:
            a = t
            while t < T and s[t]:
                t += 1
            if t - a >= min_run:
                out.append((a, t))
        else:
            t += 1
    return out


def vad(x, fl, step, ratio, floor, hang, min_run):
    """-> (e float64 [T], emax, runs [(a, b)])"""
    e = energies(x, fl, step)
    emax, _, s = flags(e, ratio, floor, hang)
    return e, emax, runs_of(s, min_run)


def max_runs(T, hang):
    return -(-T // (2 * hang + 2))


def plan_segments(runs, energy, max_frames):
    """a run of at most max_frames frames is one segment; a longer one [a, b) is cut at the quietest frame of [a + max_frames // 2,
    min(a + max_frames, b - 2)] (the first one on a tie), [a, c) is emitted and the rule goes on from c"""
    assert max_frames >= 4
    out = []
    for a, b in runs:
        a, b = int(a), int(b)
        while b - a > max_frames:
            best = None
            for t in range(a + max_frames // 2, min(a + max_frames, b - 2) + 1):
                if best is None or energy[t] < energy[best]:
                    best = t
            out.append((a, best))
            a = best
        out.append((a, b))
    return out


def sample_ranges(segments, fl, step, n):
    return [(a * step, min((b - 1) * step + fl, n)) for a, b in segments]


def bursts(rate, n_bursts, burst_s=1.0, gap_s=0.6, floor_amp=0.0, seed=0, lead_s=0.6):
    """(wave float32, [(first sample, end sample)] of the bursts): 0.1 randn bursts between stretches of exact zeros (or of a floor_amp
    randn floor)"""
    rng = np.random.RandomState(seed)
    parts, truth, pos = [], [], 0

    def quiet(n):
        return (floor_amp * rng.randn(n)).astype(np.float32) if floor_amp else np.zeros(n, np.float32)

    parts.append(quiet(int(lead_s * rate)))
    pos += len(parts[-1])
    for _ in range(n_bursts):
        b = (0.1 * rng.randn(int(burst_s * rate))).astype(np.float32)
        truth.append((pos, pos + len(b)))
        parts.append(b)
        pos += len(b)
        parts.append(quiet(int(gap_s * rate)))
        pos += len(parts[-1])
    return np.concatenate(parts), truth
