"""Host side of SpecAugment (no GPU): the plan recipe of las.specaug.SpecAugment.plan, the numpy statement of "apply a plan"
(tests/specaug_ref.py), the refusals of las_specaug that come before any launch, and the new flags."""
import ctypes

import numpy as np
import pytest

import helpers
import specaug_ref as SR
from las import _hip
from las.specaug import SpecAugment


def _args(**over):
    kw = dict(feat_dim=40, seed=5, specaug_time_warp=5)
    kw.update(over)
    return helpers.make_args(**kw)


# ---- the plan recipe ---------------------------------------------------------------------------------------------------------------
def _mixed_lengths(W, n=2000):
    rng = np.random.RandomState(3)
    lens = rng.randint(1, 400, size=n)
    lens[:8] = (1, 2, 2 * W + 2, 2 * W + 3, 2 * W + 4, 3, 399, 2 * W + 1)
    return lens


@pytest.mark.parametrize("over", [dict(), dict(specaug_time_ratio=0.2, specaug_time_width=30, specaug_freq_width=7, specaug_freq_masks=3, specaug_time_masks=1),
                                  dict(specaug_time_warp=0, specaug_freq_masks=0, specaug_time_masks=0)], ids=["defaults", "narrow", "nothing"])
def test_every_draw_is_inside_its_range(over):
    a = _args(**over)
    sa = SpecAugment(a)
    W, F, mF, mT = sa.W, sa.F, sa.mF, sa.mT
    assert sa.Fw == (13 if a.specaug_freq_width < 0 else a.specaug_freq_width) and sa.ldp % 4 == 0 and sa.ldp >= 4 + 2 * (mF + mT)
    lens = _mixed_lengths(W)
    plan = sa.plan(lens, step=17)
    assert plan.dtype == np.int32 and plan.shape == (2000, sa.ldp)
    assert np.array_equal(plan[:, 0], lens) and (plan[:, 3] == 0).all() and (plan[:, 4 + 2 * (mF + mT):] == 0).all()
    w0, w = plan[:, 1].astype(int), plan[:, 2].astype(int)
    short = lens < 2 * W + 3
    assert short[:3].all() and not short[3] and (w[short] == 0).all() and (w0[short] == 0).all()       # len 1, 2, 2W + 2 | 2W + 3
    if W:
        long_ = ~short
        assert (w0[long_] >= W + 1).all() and (w0[long_] < lens[long_] - W - 1).all() and (np.abs(w[long_]) <= W).all()
        assert w[long_].min() == -W and w[long_].max() == W              # both ends of the range are drawn over ~1900 rows
        assert (w0[long_] == W + 1).any() and (w0[long_] == lens[long_] - W - 2).any()
        k = long_ & (w != 0)                                             # what the entry asks of a warp
        assert (w0[k] + w[k] >= 1).all() and (w0[k] + w[k] <= lens[k] - 2).all() and (w0[k] <= lens[k] - 2).all()
    else:
        assert (w == 0).all()
    for m in range(mF):
        f0, fw = plan[:, 4 + 2 * m], plan[:, 5 + 2 * m]
        assert fw.min() == 0 and fw.max() == sa.Fw and (f0 >= 0).all() and (f0 + fw <= F).all()
        assert (f0 + fw == F).any() and (f0 == 0).any()
    for m in range(mT):
        t0, tw = plan[:, 4 + 2 * mF + 2 * m], plan[:, 5 + 2 * mF + 2 * m]
        cap = np.minimum(sa.Tw, np.floor(sa.p * lens)).astype(int)
        assert (tw >= 0).all() and (tw <= cap).all() and (tw == cap).any() and (t0 >= 0).all() and (t0 + tw <= lens).all()
        assert tw.max() == min(sa.Tw, int(sa.p * 399))


def test_plan_is_keyed_by_seed_and_step_and_sharding_does_not_change_it():
    sa = SpecAugment(_args())
    lens = np.asarray([50, 13, 12, 200, 77, 1, 300, 64])
    p = sa.plan(lens, 3, 0, 8)
    assert np.array_equal(p, sa.plan(lens, 3, 0, 8)) and np.array_equal(p, sa.plan(lens, 3))
    assert np.array_equal(p, SpecAugment(_args()).plan(lens, 3))          # no state in the object
    assert not np.array_equal(p, sa.plan(lens, 4))
    assert not np.array_equal(p, SpecAugment(_args(seed=6)).plan(lens, 3))
    assert np.array_equal(p[4:], sa.plan(lens[4:], 3, 4, 8))              # the sharding identity
    assert np.array_equal(p[:4], sa.plan(lens[:4], 3, 0, 8)) and np.array_equal(p[2:5], sa.plan(lens[2:5], 3, 2))
    with pytest.raises(ValueError, match="global batch"):
        sa.plan(lens, 3, 4, 8)
    # the recipe of the docstring, restated for one row
    u = np.random.Generator(np.random.Philox(key=np.array([5, 3], np.uint64))).random((8, sa.n_draws))[3]
    idx = lambda x, n: min(int(np.floor(x * n)), n - 1)
    W, n = sa.W, 200
    want = [n, W + 1 + idx(u[0], n - 2 * W - 2), idx(u[1], 2 * W + 1) - W, 0]
    for m in range(2):
        fw = idx(u[2 + 2 * m], sa.Fw + 1)
        want += [idx(u[3 + 2 * m], 40 - fw + 1), fw]
    for m in range(2):
        tw = idx(u[6 + 2 * m], min(sa.Tw, n) + 1)
        want += [idx(u[7 + 2 * m], n - tw + 1), tw]
    assert p[3].tolist() == want


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def test_reference_identity_and_control_points():
    rng = np.random.RandomState(0)
    x = rng.randn(2, 30, 5, 3).astype(np.float32)
    ident = SR.make_plan([(30, 0, 0, [], []), (30, 7, 0, [(2, 0)], [(30, 0)])], 1, 1)
    for f in (SR.ref64, SR.ref32):
        assert np.array_equal(f(x, ident, 1, 1), x)
    for w0, w in ((10, 4), (10, -4), (1, 27), (28, -27)):
        i0, r, den = SR.source_frames(30, w0, w)
        assert (i0[0], r[0]) == (0, 0) and (i0[w0 + w], r[w0 + w]) == (w0, 0) and (i0[29], r[29]) == (29, 0)
        pos = i0 + r / den
        assert (np.diff(pos) > 0).all() and (i0[r > 0] + 1 <= 29).all()
        y = SR.ref64(x, SR.make_plan([(30, w0, w, [], []), (20, 0, 0, [], [])], 0, 0), 0, 0)
        assert np.array_equal(y[0, [0, w0 + w, 29]], x[0, [0, w0, 29]].astype(np.float64))
        assert np.array_equal(y[1, :20], x[1, :20]) and (y[1, 20:] == 0).all()
    # a ramp warps onto the piecewise-linear map itself; masks select zeros over NaN
    ramp = np.broadcast_to(np.arange(30, dtype=np.float64)[None, :, None, None], (1, 30, 5, 3)).copy()
    i0, r, den = SR.source_frames(30, 10, 4)
    assert np.allclose(SR.ref64(ramp, SR.make_plan([(30, 10, 4, [], [])], 0, 0), 0, 0)[0, :, 0, 0], i0 + r / den, rtol=0, atol=1e-12)
    xn = x.copy()
    xn[0, 3:6] = np.nan
    xn[0, :, 4] = np.nan
    y = SR.ref32(xn, SR.make_plan([(30, 0, 0, [(4, 1)], [(3, 3)]), (30, 0, 0, [], [])], 1, 1), 1, 1)
    assert not np.isnan(y).any() and (y[0, 3:6] == 0).all() and (y[0, :, 4] == 0).all() and np.array_equal(y[0, 6:, :4], x[0, 6:, :4])
    assert 0 < SR.gap(x, SR.make_plan([(30, 10, 4, [], []), (30, 10, -4, [], [])], 0, 0), 0, 0) < 2e-6


# ---- the C entry -------------------------------------------------------------------------------------------------------------------
def test_c_entry_validates_before_any_launch():
    """las_specaug refuses bad arguments on the host (nothing here is a device pointer: a launch would fault)"""
    l = _hip.lib()
    assert l.las_specaug_tile() >= 8
    B, T, F, C, mF, mT = 2, 100, 13, 3, 2, 2
    nbytes = B * T * F * C * 4
    base = 1 << 20

    def call(rows=None, **over):
        rows = rows or [(100, 40, -3, [(0, 4), (9, 4)], [(0, 10), (90, 10)]), (60, 0, 0, [], [(60, 0)])]
        plan = SR.make_plan(rows, over.get("mF", mF), over.get("mT", mT))
        kw = dict(in_=ctypes.c_void_p(base), out=ctypes.c_void_p(base + nbytes), plan=ctypes.c_void_p(256),
                  plan_host=plan.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ldp=plan.shape[1], B=B, Tmax=T, F=F, C=C, mF=mF, mT=mT)
        kw.update(over)
        a = _hip.SpecAugArgs(**kw)
        return l.las_specaug(ctypes.byref(a), None), l.las_last_error()

    rc = l.las_specaug(None, None)
    assert rc < 0 and b"null argument struct" in l.las_last_error()
    for ptr in ("in_", "out", "plan", "plan_host"):
        rc, msg = call(**{ptr: None})
        assert rc < 0 and b"null pointer" in msg, ptr
    for off in (0, 4, nbytes - 4, -nbytes + 4):                          # out inside, over the head or over the tail of in
        rc, msg = call(out=ctypes.c_void_p(base + off))
        assert rc < 0 and b"overlap" in msg, off
    rc, msg = call(B=0)
    assert rc < 0 and b"B=0" in msg
    rc, msg = call(B=65536)
    assert rc < 0 and b"B=65536" in msg
    rc, msg = call(Tmax=32769)
    assert rc < 0 and b"Tmax=32769" in msg
    rc, msg = call(F=0)
    assert rc < 0 and b"F=0" in msg
    rc, msg = call(C=0)
    assert rc < 0 and b"C=0" in msg
    rc, msg = call(mF=17, ldp=64)
    assert rc < 0 and b"mF=17" in msg
    rc, msg = call(mT=17, ldp=64)
    assert rc < 0 and b"mT=17" in msg
    rc, msg = call(ldp=8)                                                # 4 + 2 (2 + 2) = 12
    assert rc < 0 and b"ldp=8" in msg and b"12" in msg
    rc, msg = call(ldp=14)
    assert rc < 0 and b"ldp=14" in msg                                   # no multiple of 4
    rc, msg = call(rows=[(100, 0, 0, [], []), (101, 0, 0, [], [])])
    assert rc < 0 and b"row 1 has len=101" in msg
    rc, msg = call(rows=[(-1, 0, 0, [], []), (5, 0, 0, [], [])])
    assert rc < 0 and b"row 0 has len=-1" in msg
    rc, msg = call(rows=[(100, 0, 0, [], [(95, 6)]), (60, 0, 0, [], [])])
    assert rc < 0 and b"row 0 time mask 0 t0=95, tw=6" in msg             # a mask past len
    rc, msg = call(rows=[(100, 0, 0, [], []), (60, 0, 0, [], [(0, 0), (61, 0)])])
    assert rc < 0 and b"row 1 time mask 1 t0=61" in msg
    rc, msg = call(rows=[(100, 0, 0, [(0, 0), (10, 4)], []), (60, 0, 0, [], [])])
    assert rc < 0 and b"row 0 frequency mask 1 f0=10, fw=4" in msg        # past F = 13
    rc, msg = call(rows=[(100, 0, 0, [(-1, 2)], []), (60, 0, 0, [], [])])
    assert rc < 0 and b"frequency mask 0 f0=-1" in msg
    for w0, w in ((0, 3), (3, -3), (99, -5), (95, 4), (98, 1)):           # an empty left or right segment
        rc, msg = call(rows=[(100, 40, 2, [], []), (100, w0, w, [], [])])
        assert rc < 0 and b"row 1 warp" in msg and ("w0=%d, w=%d" % (w0, w)).encode() in msg and b"empty segment" in msg, (w0, w)
    rc, msg = call(rows=[(2, 1, 1, [], []), (60, 0, 0, [], [])])
    assert rc < 0 and b"row 0 warp" in msg                               # too short for any warp


# ---- the flags ---------------------------------------------------------------------------------------------------------------------
def test_flags():
    from las.arguments import parse_args, reference_flag_names
    a = parse_args([])
    assert a.spec_augment is False
    assert (a.specaug_time_warp, a.specaug_freq_masks, a.specaug_freq_width, a.specaug_time_masks, a.specaug_time_width, a.specaug_time_ratio) == \
        (80, 2, -1, 2, 100, 1.0)
    a = parse_args(["--spec_augment", "True", "--specaug_time_warp", "40", "--specaug_freq_masks", "1", "--specaug_freq_width", "15",
                    "--specaug_time_masks", "3", "--specaug_time_width", "50", "--specaug_time_ratio", "0.2", "--feat_dim", "80"])
    assert a.spec_augment is True
    sa = SpecAugment(a)
    assert (sa.W, sa.mF, sa.Fw, sa.mT, sa.Tw, sa.p, sa.F) == (40, 1, 15, 3, 50, 0.2, 80)
    assert SpecAugment(parse_args(["--feat_dim", "80"])).Fw == 26 and SpecAugment(parse_args(["--feat_dim", "2"])).Fw == 1
    assert not [n for n in reference_flag_names() if n.startswith("spec")]        # the reference's table is as it was
    with pytest.raises(ValueError, match="masks"):
        SpecAugment(parse_args(["--specaug_time_masks", "17"]))
