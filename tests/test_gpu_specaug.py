"""SpecAugment on the device (csrc/specaug.hip through las.specaug.SpecAugment) against the float64 statement in tests/specaug_ref.py,
and LAS.train / train_stacked with --spec_augment True.

Shapes: batches of five ragged rows, len = 1, 2 W + 3 (the shortest row that warps), one frame less and one more than a workgroup's
tile, two tiles and a frame, for W = 2, with Tmax = the longest + 3; F x C = 13 x 3, 39 x 3 (39 and 117 floats per frame: rows, tiles
and frames start on any 4-byte boundary), 40 x 3 (a multiple of 4) and 5 x 1 (a 16-byte store spans frames).  The parity bar of a
case is max |gpu - float64| <= max(4 x gap, 1e-6), gap = the float32 numpy evaluation against float64 on the same batch (the
project's rule for fp32 kernels: two correct fp32 evaluations can sit on opposite sides of float64, and the device's fmaf rounds once
where numpy rounds twice); the inputs are O(1), gap is about 2e-7 and a wrong frame or bin shows as O(1)."""
import json

import numpy as np
import pytest

import helpers
import specaug_ref as SR

pytestmark = pytest.mark.gpu

W = 2
SHAPES = [(13, 3), (39, 3), (40, 3), (5, 1)]
VARIANTS = ["stretch", "squeeze", "still", "bare"]
_cache = {}


def _sa(F, mF, mT):
    from las.specaug import SpecAugment
    key = (F, mF, mT)
    if key not in _cache:
        _cache[key] = SpecAugment(helpers.make_args(feat_dim=F, specaug_time_warp=W, specaug_freq_masks=mF, specaug_time_masks=mT, seed=3))
    return _cache[key]


def _lens():
    from las import _hip
    tile = int(_hip.lib().las_specaug_tile())
    assert tile >= 2 * W + 4
    return [1, 2 * W + 3, tile - 1, tile + 1, 2 * tile + 1]


def _case(F, C, variant):
    """(x [5, Tmax, F, C] float32 with finite noise behind every len, plan, mF, mT, float64 reference, gap): computed once per case"""
    key = ("case", F, C, variant)
    if key in _cache:
        return _cache[key]
    lens = _lens()
    Tmax = max(lens) + 3
    rng = np.random.RandomState(F * 7 + C + VARIANTS.index(variant))
    x = rng.randn(5, Tmax, F, C).astype(np.float32)
    rows = []
    for b, n in enumerate(lens):
        warps = n >= 2 * W + 3
        lo, hi = W + 1, n - W - 2                                      # both ends of w0's range [W + 1, len - W - 1)
        if variant == "stretch":                                       # w = +W, w0 at the low end; masks touching every edge
            fa, fb = (2, 3) if F >= 8 else (1, 1)
            rows.append((n, lo if warps else 0, W if warps else 0, [(0, fa), (F - fb, fb)], [(0, min(2, n)), (n - min(3, n), min(3, n))]))
        elif variant == "squeeze":                                     # w = -W, w0 at the high end; two overlapping masks each
            rows.append((n, hi if warps else 0, -W if warps else 0, [(1, min(3, F - 1)), (2, min(3, F - 2))],
                         [(n // 3, min(4, n - n // 3)), (n // 3 + 2 if n // 3 + 2 <= n else n, min(4, max(n - n // 3 - 2, 0)))]))
        elif variant == "still":                                       # w = 0 (w0 is ignored); zero-width masks at both ends and a real one
            rows.append((n, 0, 0, [(0, 0), (F, 0)], [(n, 0), (n // 2, min(2, n - n // 2))]))
        else:                                                          # mF = mT = 0; w mixed over the rows, w0 alternating between its ends
            w = (0, W, -W, W, -W)[b] if warps else 0
            rows.append((n, (lo, hi)[b % 2] if w else 0, w, [], []))
    mF, mT = (0, 0) if variant == "bare" else (2, 2)
    plan = SR.make_plan(rows, mF, mT)
    r64 = SR.ref64(x, plan, mF, mT)
    _cache[key] = (x, plan, mF, mT, r64, SR.gap(x, plan, mF, mT))
    return _cache[key]


def _zero_mask(plan, shape, mF, mT):
    """True where out must be exactly 0: behind len, under a time mask, under a frequency mask"""
    B, T, F, C = shape
    z = np.zeros(shape, bool)
    for b in range(B):
        tm, fm = SR.masks(plan[b], T, F, mF, mT)
        z[b, tm] = True
        z[b, :, fm] = True
    return z


def _run(x, plan, mF, mT, out=None):
    import torch
    y = _sa(x.shape[2], mF, mT).apply(torch.from_numpy(np.ascontiguousarray(x)).cuda(), plan, out=out)
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("F,C", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_parity_and_structure(F, C, variant):
    import torch
    x, plan, mF, mT, r64, gap = _case(F, C, variant)
    poisoned = torch.full(x.shape, float("nan"), device="cuda")
    y = _run(x, plan, mF, mT, out=poisoned)
    assert y.data_ptr() == poisoned.data_ptr()
    o = y.cpu().numpy()
    assert not np.isnan(o).any()                                       # every element of out is written
    z = _zero_mask(plan, x.shape, mF, mT)
    assert (o[z].view(np.int32) == 0).all()                            # +0.0f exactly
    assert (o[~z] != 0).all()
    err = float(np.abs(o.astype(np.float64) - r64).max())
    bar = max(4 * gap, 1e-6)
    print(json.dumps(dict(F=F, C=C, variant=variant, lens=plan[:, 0].tolist(), err=err, gap=gap, bar=bar)))
    assert err <= bar
    for b in range(5):
        if plan[b, 2] == 0:                                            # no warp: a bit copy outside the masks
            assert np.array_equal(o[b][~z[b]].view(np.int32), x[b][~z[b]].view(np.int32)), b
    if variant != "still":
        assert gap > 0 and (plan[1:, 2] != 0).any()                    # the case does interpolate


def _poison(x, plan, mF, mT):
    """x with NaN wherever the kernel has no business reading: behind len, every bin under a frequency mask, and every source frame
    that no unmasked output frame reads -- the frames under a time mask, frame i0 + 1 of an output with r == 0, what a squeeze skips"""
    xp = x.copy()
    B, T, F, C = x.shape
    for b in range(B):
        n, w0, w = (int(v) for v in plan[b, :3])
        tm, fm = SR.masks(plan[b], T, F, mF, mT)
        read = np.zeros(T, bool)
        if n:
            i0, r, _ = SR.source_frames(n, w0, w)
            keep = ~tm[:n]
            read[i0[keep]] = True
            read[(i0 + 1)[keep & (r > 0)]] = True
        xp[b, ~read] = np.nan
        xp[b, :, fm] = np.nan
    return xp


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("F,C", [(39, 3), (5, 1)], ids=["39x3", "5x1"])
def test_poison_is_not_read(F, C, variant):
    x, plan, mF, mT, _, _ = _case(F, C, variant)
    xp = _poison(x, plan, mF, mT)
    assert np.isnan(xp).any() and np.isnan(xp[:, -3:]).all()
    for b in range(5):                                                 # frame i0 + 1 of the last frame (r == 0) is poison
        assert np.isnan(xp[b, plan[b, 0]]).all()
    if variant == "still":                                             # w == 0: every frame has r == 0, and its successor under a mask is poison
        assert np.isnan(xp[4, plan[4, 0] // 2]).all()
    clean = _run(x, plan, mF, mT).clone()
    got = _run(xp, plan, mF, mT)
    assert not got.isnan().any()
    assert np.array_equal(got.cpu().numpy().view(np.int32), clean.cpu().numpy().view(np.int32))


@pytest.mark.parametrize("F,C", [(13, 3), (40, 3), (5, 1)], ids=["13x3", "40x3", "5x1"])
def test_determinism_and_batch_independence(F, C):
    for variant in ("stretch", "squeeze"):
        x, plan, mF, mT, _, _ = _case(F, C, variant)
        a = _run(x, plan, mF, mT).clone()
        b = _run(x, plan, mF, mT)
        assert np.array_equal(a.cpu().numpy().view(np.int32), b.cpu().numpy().view(np.int32))      # two runs: the same bits
        o = a.cpu().numpy()
        for u in range(5):
            n = int(plan[u, 0])
            alone = _run(x[u:u + 1, :n], plan[u:u + 1], mF, mT).cpu().numpy()                      # (another Tmax: other tiles, another alignment)
            assert np.array_equal(alone[0].view(np.int32), o[u, :n].view(np.int32)), (variant, u)
            alone = _run(x[u:u + 1], plan[u:u + 1], mF, mT).cpu().numpy()
            assert np.array_equal(alone[0].view(np.int32), o[u].view(np.int32)), (variant, u)


def test_call_is_apply_of_the_plan_of_the_step():
    import torch
    from las import _hip
    from las.specaug import SpecAugment
    a = helpers.make_args(feat_dim=13, spec_augment=True, specaug_time_warp=5, specaug_time_width=20, seed=9)
    sa = SpecAugment(a)
    (audio, audiolen), _ = helpers.synthetic_batch(6, 150, 8, 30, seed=2)
    xd = torch.from_numpy(audio).cuda()
    got = sa(xd, audiolen, step=7).clone()
    plan = sa.plan(audiolen, 7)
    assert (plan[:, 2] != 0).any() and (plan[:, 5] > 0).any() and (plan[:, 9] > 0).any()
    want = sa.apply(xd, plan).clone()
    other = sa(xd, audiolen, step=8).clone()
    # rows 3..5 as the second of two data-parallel ranks would run them
    shard = sa(xd[3:].contiguous(), audiolen[3:], step=7, row0=3, rows_global=6).clone()
    torch.cuda.synchronize()
    assert torch.equal(got, want) and not torch.equal(got, other) and torch.equal(shard, got[3:])
    assert got.data_ptr() != xd.data_ptr() and torch.equal(xd.cpu(), torch.from_numpy(audio))      # the input is left as it was
    assert any(k[1].startswith("specaug") for k in _hip._ws_cache)                                  # the result lives in the tagged workspace
    r64 = SR.ref64(audio, plan, sa.mF, sa.mT)
    assert float(np.abs(got.cpu().numpy() - r64).max()) <= max(4 * SR.gap(audio, plan, sa.mF, sa.mT), 1e-6)
    with pytest.raises(RuntimeError, match="overlap"):
        sa.apply(xd, plan, out=xd)
    with pytest.raises(RuntimeError, match="ROCm device"):
        sa.apply(torch.from_numpy(audio), plan)


# ---- the train step ----------------------------------------------------------------------------------------------------------------
def _model_args(**over):
    kw = dict(enc_units=64, num_enc_layers=2, dec_units=64, num_dec_layers=1, embedding_size=32, attention_size=32,
              specaug_time_warp=5, specaug_time_width=10, specaug_freq_width=4, seed=4)
    kw.update(over)
    return helpers.make_args(**kw)


class _Recorder:
    """stands in front of a Listener and keeps what it is fed"""

    def __init__(self, listener):
        self._listener, self.seen = listener, []

    def __call__(self, audio, *a, **k):
        self.seen.append(audio.detach().clone())
        return self._listener(audio, *a, **k)

    def __getattr__(self, name):
        return getattr(self._listener, name)


def _train(args, batches, steps=1, stacked=False):
    """fresh model from one seed -> (losses of `steps` steps on the same batch, the cubes the Listener was fed)"""
    import torch
    from las import layers as L, variables as V
    from las.las import LAS, Listener, Speller
    from oracle import las_oracle as O
    p0 = O.init_params(args, seed=11, cell="lstm", enc_type="pblstm")
    L.set_cell("lstm")
    L.set_precision("f32")
    st = V.reset_default_store(device="cuda")
    st.load(p0)
    las = LAS(args, Listener, Speller, {})
    las.listener = _Recorder(las.listener)
    losses = []
    for _ in range(steps):
        out = las.train_stacked(batches) if stacked else las.train(*batches)
        torch.cuda.synchronize()
        las.check_status()
        if las.recovered_steps:
            out = las.last_out
        losses.append(float(out[0]))
    return losses, las.listener.seen, las


def _ws_epochs():
    from las import _hip
    return {k: v for k, v in _hip._ws_epoch.items() if k[1].startswith("specaug")}


def test_train_step_with_and_without_the_flag():
    import argparse
    xs, ys = helpers.synthetic_batch(3, 40, 6, 30, seed=5)
    on = _model_args(spec_augment=True)
    l1, seen1, las = _train(on, (xs, ys), steps=2)
    l2, seen2, _ = _train(on, (xs, ys), steps=2)
    assert l1 == l2 and all(np.isfinite(l1))                           # two fresh models from one seed: the same bits over two steps
    assert all(bool((a == b).all()) for a, b in zip(seen1, seen2))
    assert not bool((seen1[0] == seen1[1]).all())                      # another step, another plan
    plan = las.specaug.plan(xs[1], 0)
    assert (plan[:, 2] != 0).any() and plan[:, 5::2][:, :4].sum() > 0
    # the flag-off model fed the float32 statement of the same plan
    epochs = _ws_epochs()
    aug = SR.ref32(xs[0], plan, las.specaug.mF, las.specaug.mT)
    assert float(np.abs(seen1[0].cpu().numpy() - aug).max()) < 1e-5
    off = _model_args()
    (l_ref,), _, _ = _train(off, ((aug, xs[1]), ys))
    bar = 1e-4 * max(1.0, abs(l_ref))                                  # the project's f32 loss parity bar (tests/test_gpu_las_parity.py)
    print("loss: flag on %.7f, flag off on the reference's cube %.7f" % (l1[0], l_ref))
    assert abs(l1[0] - l_ref) < bar
    (l_raw,), seen_raw, las_off = _train(off, (xs, ys))
    print("loss: flag off on the raw batch %.7f" % l_raw)
    # the augmentation is not a no-op.  (A freshly initialised model's loss sits near log(vocabulary) whatever it hears: the oracle gives
    # 3.40516 on the raw batch and 3.40523 on the augmented one, less than the parity bar apart -- so the statement about the cube
    # above is the sharp one, and here the loss must simply move, and further than it is from the reference-fed model's)
    assert l1[0] != l_raw and abs(l1[0] - l_ref) < abs(l1[0] - l_raw)
    # flag off: the namespace of the parent commit (no specaug attribute at all) gives the same bits, and nothing of las.specaug ran
    bare = argparse.Namespace(**{k: v for k, v in vars(off).items() if not k.startswith("spec")})
    assert not hasattr(bare, "spec_augment")
    (l_bare,), seen_bare, las_bare = _train(bare, (xs, ys))
    assert l_bare == l_raw and bool((seen_bare[0].cpu() == seen_raw[0].cpu()).all())
    assert np.array_equal(seen_raw[0].cpu().numpy(), xs[0])
    assert las_off.specaug is None and las_bare.specaug is None and _ws_epochs() == epochs      # no workspace asked for


def test_train_stacked_numbers_its_shards_rows_in_rank_order():
    import torch
    a = _model_args(spec_augment=True)
    xa, ya = helpers.synthetic_batch(3, 40, 6, 30, seed=6)
    xb, yb = helpers.synthetic_batch(3, 40, 6, 30, seed=7)
    l_st, seen_st, las = _train(a, [(xa, ya), (xb, yb)], stacked=True)
    xc = (np.concatenate([xa[0], xb[0]]), np.concatenate([xa[1], xb[1]]))
    yc = (np.concatenate([ya[0], yb[0]]), np.concatenate([ya[1], yb[1]]))
    l_cat, seen_cat, _ = _train(a, (xc, yc))
    assert l_st == l_cat and torch.equal(seen_st[0], seen_cat[0])
    # ... and they are the rows two data-parallel ranks holding one shard each would draw and apply
    sa = las.specaug
    p0, p1 = sa.plan(xa[1], 0, 0, 6), sa.plan(xb[1], 0, 3, 6)
    assert np.array_equal(np.concatenate([p0, p1]), sa.plan(xc[1], 0))
    r0 = sa.apply(torch.from_numpy(xa[0]).cuda(), p0).clone()
    r1 = sa.apply(torch.from_numpy(xb[0]).cuda(), p1).clone()
    torch.cuda.synchronize()
    assert torch.equal(torch.cat([r0, r1]), seen_st[0])
    assert not torch.equal(r1, sa.apply(torch.from_numpy(xb[0]).cuda(), sa.plan(xb[1], 0)))         # rows 0..2 are not rows 3..5
