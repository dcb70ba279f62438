"""tests/adam_ref.py, the float64 restatement the GPU optimiser tests (test_gpu_optimizer.py) hold las_sumsq / las_clip_adam to:
it equals the oracle's clip_by_global_norm + adam_tf, an fp32 emulation of the kernel's expression order passes its bounds, and six
plausible mistakes in the kernel fail them -- after ONE step and after five -- so the bounds discriminate.  No GPU involved."""
import math

import numpy as np
import pytest

import adam_ref as R
from helpers import ROOT  # noqa: F401  (puts the repository on sys.path)

F = np.float32
B1, B2, EPS, LR = 0.9, 0.999, 1e-8, 1e-3
N = 100003


def make_g(rng, n):
    """gradients over nine decades (|g| ~ eps = 1e-8 and below included), every seventh exactly zero; log-uniform magnitudes, so that no
    intermediate of the update leaves fp32's normal range"""
    g = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-9, 0, n)).astype(F)
    g[::7] = 0
    return g


def emulate(th, g, m, v, sumsq, clip, lr_t, b1=B1, b2=B2, eps=EPS, mut=None):
    """clip_adam_kernel in numpy fp32, one rounding per operation (no FMA); mut: one of the mistakes below"""
    b1, b2, eps, lr_t, clip = F(b1), F(b2), F(eps), F(lr_t), F(clip)
    gs = F(1)
    if clip > 0 and mut != "no_clip":
        gs = clip / max(np.sqrt(F(sumsq)), clip)
    if mut == "swap_betas":
        b1, b2 = b2, b1
    gc = g * gs
    m2 = b1 * m + (F(1) - b1) * gc
    v2 = b2 * v + (F(1) - b2) * gc * gc
    den = np.sqrt(v2 + eps) if mut == "eps_in_sqrt" else np.sqrt(v2) + eps
    th2 = th - lr_t * m2 / den
    assert th2.dtype == F and m2.dtype == F and v2.dtype == F
    if mut == "no_tail":
        k = len(th) // 4 * 4
        th2[k:], m2[k:], v2[k:] = th[k:], m[k:], v[k:]
    if mut == "no_writeback":
        m2, v2 = m, v
    return th2, m2, v2


def run(mut, clip, steps, n=N, t0=0, seed=1, trajectory=None):
    """-> the worst ratios (adam_ref.ratios) of every step, the reference applied to the emulation's own state before the step;
    trajectory: a list that receives every step's ratios against adam_ref.Trajectory, which never sees that state"""
    rng = np.random.RandomState(seed)
    th, m, v = rng.randn(n).astype(F), np.zeros(n, F), np.zeros(n, F)
    pure = R.Trajectory(th, m, v)
    out = []
    for s in range(steps):
        g = make_g(rng, n)
        t = t0 + s + 1
        lr_t = R.lr_t(LR, t)
        ss = F(R.sumsq_ref(g))
        ref = R.step(th, g, m, v, ss, clip, lr_t, B1, B2, EPS)
        th2, m2, v2 = emulate(th, g, m, v, ss, clip, LR if mut == "lr_not_lr_t" else lr_t, mut=mut)
        out.append(R.ratios(th2, m2, v2, ref))
        pure.step(g, ss, clip, lr_t, B1, B2, EPS)
        if trajectory is not None:
            trajectory.append(pure.ratios(th2, m2, v2))
        th, m, v = th2, m2, v2
    return out


def test_reference_equals_the_oracle_in_float64():
    """adam_ref.step against oracle.clip_by_global_norm + oracle.adam_tf, 5 steps, float64 on both sides (the oracle is handed the
    fp32-rounded scalars adam_ref rounds to, and the learning rate whose bias correction gives the rounded lr_t)"""
    import torch
    from oracle import las_oracle as O
    rng = np.random.RandomState(5)
    n = 4099
    b1, b2, eps = R.f32(B1), R.f32(B2), R.f32(EPS)
    for clip in (0.0, 0.5, 1e3):
        th, m, v = rng.randn(n), np.zeros(n), np.zeros(n)
        tho, mo, vo = (torch.tensor(a, dtype=torch.float64) for a in (th, m, v))
        for t in range(1, 6):
            g = make_g(rng, n).astype(np.float64)
            lrt = R.f32(R.lr_t(LR, t))
            ss = R.sumsq_ref(g)
            th, m, v, terms = R.step(th, g, m, v, ss if clip > 0 else None, clip, lrt, B1, B2, EPS)
            go = torch.tensor(g)
            if clip > 0:
                (go,), norm = O.clip_by_global_norm([go], R.f32(clip))
                assert abs(norm - math.sqrt(ss)) <= 1e-12 * norm
                assert (norm > clip) == (terms["gs"] < 1.0)
            lr_for_oracle = lrt * (1.0 - b1 ** t) / math.sqrt(1.0 - b2 ** t)        # adam_tf derives lr_t itself
            tho, mo, vo = O.adam_tf(tho, go, mo, vo, t, lr_for_oracle, b1, b2, eps)
            assert np.all(np.abs(m - mo.numpy()) <= 1e-12 * terms["m"]), (clip, t)
            assert np.all(np.abs(v - vo.numpy()) <= 1e-12 * terms["v"]), (clip, t)
            assert np.all(np.abs(th - tho.numpy()) <= 1e-12 * np.abs(th)), (clip, t)
        assert np.abs(m).max() > 0 and np.all(v[1::7] > 0)


def test_sumsq_ref_and_scalars():
    g = np.array([3.0, -4.0, 0.0], F)
    assert R.sumsq_ref(g) == 25.0 and R.sumsq_ref(np.zeros(0, F)) == 0.0
    assert R.clip_scale(25.0, 0.0) == 1.0 and R.clip_scale(25.0, 10.0) == 1.0 and R.clip_scale(25.0, 2.5) == 0.5
    assert R.f32(0.999) != 0.999 and abs((1.0 - R.f32(0.999)) / 0.001 - 1.0) > 1e-5       # why the scalars are rounded first
    assert R.sumsq_bound(1) == 41 * 2.0 ** -24 and R.sumsq_bound(4 * 262144 + 1) == 42 * 2.0 ** -24
    with pytest.raises(ValueError):
        R.step(g, g, g, g, None, 1.0, 1e-3, B1, B2, EPS)


@pytest.mark.parametrize("clip", [0.0, 0.5, 1e3], ids=["clip_off", "clip_binding", "clip_not_binding"])
@pytest.mark.parametrize("t0", [0, 60000])
def test_fp32_emulation_of_the_kernel_passes_the_bounds(clip, t0):
    rng = np.random.RandomState(1)
    rng.randn(N)
    norm = math.sqrt(R.sumsq_ref(make_g(rng, N)))
    assert (norm > 50 * clip) if clip == 0.5 else (norm < clip or clip == 0.0)           # ~100 x clip / well inside it
    worst, traj = {}, []
    for r in run(None, clip, 6, t0=t0, trajectory=traj):
        for k, x in r.items():
            worst[k] = max(worst.get(k, 0.0), x)
    print("clip %g t0 %d: worst ratio to the bounds %s, of the trajectory after 5 steps %s" % (clip, t0, worst, traj[4]))
    assert worst["m"] <= 1.0 and worst["v"] <= 1.0 and worst["theta"] <= 1.0, worst
    assert max(traj[4].values()) <= 1.0, traj[4]


def test_the_theta_bound_charges_the_error_of_m_to_its_terms():
    """adam_ref's docstring: at n = 3000003 a correct fp32 evaluation leaves 2^-23 |theta'| + 2^-20 |update| where b1 m and (1 - b1) gc
    cancel; with m' charged to |b1 m| + |(1 - b1) gc| it stays inside, and the two forms agree where nothing cancels"""
    rng = np.random.RandomState(2)
    n = 3000003
    th, m, v = rng.randn(n).astype(F), np.zeros(n, F), np.zeros(n, F)
    worst_first, worst = 0.0, 0.0
    for s in range(4):
        g = make_g(rng, n)
        ss = F(R.sumsq_ref(g))
        ref = R.step(th, g, m, v, ss, 0.5, R.lr_t(LR, s + 1), B1, B2, EPS)
        th, m, v = emulate(th, g, m, v, ss, 0.5, R.lr_t(LR, s + 1))
        err = np.abs(th.astype(np.float64) - ref[0])
        worst_first = max(worst_first, float(np.max(err / (2.0 ** -23 * np.abs(ref[0]) + 2.0 ** -20 * ref[3]["upd"] + 1e-300))))
        worst = max(worst, R.ratios(th, m, v, ref)["theta"])
        if s == 0:                                                      # m = 0 going in, nothing cancels: m' is as large as its terms
            assert np.allclose(R.UPD_BOUND * ref[3]["upd"] + R.M_UPD_BOUND * ref[3]["m_upd"], 2.0 ** -20 * ref[3]["upd"], rtol=1e-6, atol=1e-20)
    print("theta: %.2f x the first form, %.2f x the bound" % (worst_first, worst))
    assert worst_first > 1.0 and worst <= 1.0


MUTATIONS = ["no_clip", "swap_betas", "eps_in_sqrt", "lr_not_lr_t", "no_tail", "no_writeback"]


@pytest.mark.parametrize("mut", MUTATIONS)
def test_a_mistake_in_the_kernel_fails_the_bounds(mut):
    """each mutation of the emulation, clip binding (norm ~ 100 x clip): over the bounds after ONE step and after five"""
    clip = 0.5
    assert max(max(r.values()) for r in run(None, clip, 5)) <= 1.0                       # the same run without the mistake passes
    traj = []
    r = run(mut, clip, 5, trajectory=traj)
    first, last = r[0], r[4]
    print(mut, "step 1:", first, "step 5:", last, "trajectory, step 5:", traj[4])
    if mut == "no_writeback":
        # m = v = 0 going in and coming out: every step computes the right theta FROM THE BUFFERS IT FINDS, so theta passes the per-step
        # check at every step; the moment buffers are wrong at once, and theta leaves the float64 trajectory from step 2 on (only)
        assert all(x["theta"] <= 1.0 for x in r) and first["m"] > 1e3 and first["v"] > 1e3
        assert traj[0]["theta"] <= 1.0 and traj[1]["theta"] > 1e3
    else:
        assert max(first.values()) > 1e3, first
    assert max(last.values()) > 1e3 and max(traj[4].values()) > 1e3, (last, traj[4])


def test_a_mistake_is_invisible_to_a_loose_check_of_the_first_step():
    """why this file exists: at step 1 from m = v = 0 the update is ~ lr sign(g) whatever the clip scale is and whatever happens to m and v afterwards -- for every
    |g| well above eps / (gs sqrt(1 - b2)) = 3e-5 here -- so |theta' - oracle| < 2e-4 at lr = 1e-3 (the train-step parity tests) passes
    these mutations (swapped betas move the first update by lr and do not)"""
    for mut in ("no_clip", "no_writeback"):
        rng = np.random.RandomState(1)
        th, z = rng.randn(N).astype(F), np.zeros(N, F)
        g = make_g(rng, N)
        ss = F(R.sumsq_ref(g))
        ref = R.step(th, g, z, z, ss, 0.5, R.lr_t(LR, 1), B1, B2, EPS)[0]
        got = emulate(th, g, z, z, ss, 0.5, R.lr_t(LR, 1), mut=mut)[0]
        assert np.abs(got - ref)[np.abs(g) > 1e-3].max() < 2e-4
