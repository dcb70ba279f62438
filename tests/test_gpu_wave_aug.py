"""Room reverberation and additive noise on the device (csrc/wave_aug.hip through las.augment.WaveAugmenter and
FeatureExtractor.extract(augment=)) against the float64 statement in preprocess.py.

The parity bar of a case is max |gpu - float64| <= max(4 x gap, 1e-6), gap = tests/wave_aug_ref.py's float32 numpy evaluation against
float64 on the same batch: it is computed from the two references alone.  The device sums the taps in ascending order in one fmaf chain
(one rounding per tap where numpy rounds twice), so it sits within a gap of float64 itself; a dropped, doubled or shifted tap shows as
1e-3 or more on these inputs (0.1-rms noise, unit-energy responses).  Shapes: response lengths around the tap chunk a workgroup stages
(las_reverb_tap_chunk) and one of 8,000 taps; utterance lengths around the tile of outputs it owns (las_reverb_tile) and around the
reduction tile of las_noise_mix; several tiles, ragged, in one batch with rows that take no response."""
import json

import numpy as np
import pytest

import frontend_ref as R
import wave_aug_ref as WR
from frontend_ref import pp

pytestmark = pytest.mark.gpu

FS = 16000
_cases, _extractors = {}, {}


def _lib():
    from las import _hip
    return _hip.lib()


def _upload(rows, pad=24):
    """(float32 device tensor [n, ld] with NaN behind every row's length, the lengths)"""
    import torch
    ns = [len(r) for r in rows]
    host = np.full((len(rows), (max(ns) + 7 + pad) & ~7), np.nan, np.float32)
    for u, r in enumerate(rows):
        host[u, :ns[u]] = r
    return torch.from_numpy(host).cuda(), ns


def _reverb_case(K):
    """per response length: the augmenter (three responses, direct paths at 0, the middle, the last tap), the batch and the references"""
    if K not in _cases:
        from las.augment import WaveAugmenter
        l = _lib()
        tile = l.las_reverb_tile()
        delays = [0, K // 2, K - 1]
        aug = WaveAugmenter(FS, rirs=[WR.response(K, d, 100 + i) for i, d in enumerate(delays)])
        assert aug.rir_delay == delays and aug.rir_len.tolist() == [K] * 3
        lengths = sorted(set(n for n in (1, K - 1, tile - 1, tile, tile + 1, 3 * tile + 37) if n >= 1))
        xs, idx = [], []
        for i, n in enumerate(lengths):
            for r in range(3):
                xs.append(WR.noise_signal(n, 1000 * K + 10 * i + r))
                idx.append(r)
        for n in (tile + 5, 300):                                     # rows that take no response, a negative zero inside
            x = WR.noise_signal(n, 7 * K + n)
            x[:3] = np.asarray([-0.0, 0.0, -0.0], np.float32)
            xs.append(x)
            idx.append(-1)
        hs = [aug.rir_bank[r, :K] for r in idx]
        live = [u for u, r in enumerate(idx) if r >= 0]
        r64, gaps = WR.reverb_gap([xs[u] for u in live], [hs[u] for u in live], [delays[idx[u]] for u in live])
        _cases[K] = dict(aug=aug, xs=xs, idx=idx, live=live, r64=dict(zip(live, r64)), gaps=gaps, tile=tile, lengths=lengths)
    return _cases[K]


def _tap_lengths():
    chunk = _lib().las_reverb_tap_chunk()
    return [1, 2, chunk - 1, chunk, chunk + 1, 8000]


@pytest.mark.parametrize("which", range(6), ids=["1", "2", "chunk-1", "chunk", "chunk+1", "8000"])
def test_reverb_parity_and_structure(which):
    import torch
    K = _tap_lengths()[which]
    c = _reverb_case(K)
    aug, xs, idx = c["aug"], c["xs"], c["idx"]
    samples, ns = _upload(xs)
    out = torch.full_like(samples, float("nan"))
    plan = aug.fixed_plan(len(xs), rir_idx=idx)
    got = aug.apply(samples, ns, plan, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert not torch.isnan(out).any()                                 # every element written, no NaN behind a length read
    o = out.cpu().numpy()
    errs = []
    for u, x in enumerate(xs):
        assert (o[u, ns[u]:] == 0).all() and not np.signbit(o[u, ns[u]:]).any()          # exactly +0 behind the length
        if idx[u] < 0:
            assert np.array_equal(o[u, :ns[u]].view(np.int32), x.view(np.int32))        # a bit copy, the sign of a zero included
        else:
            errs.append(float(np.abs(o[u, :ns[u]].astype(np.float64) - c["r64"][u]).max()))
    bar = max(4 * max(c["gaps"]), 1e-6)
    rec = dict(entry="las_reverb", taps=K, delays=aug.rir_delay, tile=c["tile"], lengths=c["lengths"], err=max(errs), gap=max(c["gaps"]), bar=bar)
    print(json.dumps(rec))
    assert max(errs) <= bar, rec


def test_reverb_unit_impulse_returns_the_input_bits():
    import torch
    from las.augment import WaveAugmenter
    l = _lib()
    tile, chunk = l.las_reverb_tile(), l.las_reverb_tap_chunk()
    rirs = []
    for K, d in ((1, 0), (chunk + 3, 0), (chunk + 3, chunk + 2), (2 * chunk, chunk), (777, 400)):
        e = np.zeros(K)
        e[d] = 1.0
        rirs.append(e)
    aug = WaveAugmenter(FS, rirs=rirs)
    xs = [WR.noise_signal(n, 50 + i) for i, n in enumerate((1, 500, tile, tile + 1, 2 * tile + 9))]
    samples, ns = _upload(xs)
    out = aug.apply(samples, ns, aug.fixed_plan(5, rir_idx=[0, 1, 2, 3, 4]))
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    for u, x in enumerate(xs):
        assert np.array_equal(o[u, :ns[u]].view(np.int32), x.view(np.int32)), u
        assert (o[u, ns[u]:] == 0).all()


# ---- noise -------------------------------------------------------------------------------------------------------------------------
def _noise_case():
    if "noise" not in _cases:
        from las.augment import WaveAugmenter
        nt = _lib().las_noise_mix_tile()
        noises = [WR.noise_signal(1000, 1, rms=0.5), WR.noise_signal(3 * nt + 100, 2, rms=0.02), np.zeros(64, np.float32)]
        aug = WaveAugmenter(FS, noises=noises)
        # (length, noise, offset, snr): the noise shorter than the utterance; an offset whose wrap falls inside a tile; lengths around
        # the reduction's tile; a silent row; silent noise; rows without noise
        rows = [(1, 0, 999, 0.0), (nt - 1, 0, 0, -5.0), (nt, 0, 137, 0.0), (nt + 1, 0, 999, 20.0), (3 * nt + 37, 0, 501, 20.0),
                (nt + 300, 1, 3 * nt - 77, -5.0), (2 * nt + 5, 1, 0, 0.0), (700, 1, 3 * nt + 99, 20.0),
                (nt + 9, 0, 5, 10.0), (500, 2, 63, 10.0), (nt + 3, -1, 0, 0.0), (50, -1, 0, 0.0)]
        xs = [WR.noise_signal(n, 300 + i) for i, (n, _, _, _) in enumerate(rows)]
        xs[8][:] = 0.0                                                # the silent row
        xs[10][:2] = np.asarray([-0.0, 0.0], np.float32)
        refs = {}
        for u, (n, r, off, snr) in enumerate(rows):
            if r >= 0:
                y, gap = WR.mix_gap(xs[u], noises[r], off, snr)
                refs[u] = (y, gap, WR.gain64(xs[u], noises[r], off, snr))
        _cases["noise"] = dict(aug=aug, rows=rows, xs=xs, refs=refs, nt=nt)
    return _cases["noise"]


def _noise_plan(c):
    rows = c["rows"]
    return c["aug"].fixed_plan(len(rows), noise_idx=[r[1] for r in rows], noise_off=[r[2] for r in rows], snr_db=[r[3] for r in rows])


@pytest.mark.parametrize("in_place", [False, True], ids=["out", "in-place"])
def test_noise_mix_parity_gain_and_structure(in_place):
    import torch
    c = _noise_case()
    aug, rows, xs = c["aug"], c["rows"], c["xs"]
    samples, ns = _upload(xs)
    out = samples if in_place else torch.full_like(samples, float("nan"))
    gains = torch.full((len(xs),), float("nan"), device="cuda")
    got = aug.apply(samples, ns, _noise_plan(c), out=out, gain_out=gains)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and not torch.isnan(out).any() and not torch.isnan(gains).any()
    o, g = out.cpu().numpy(), gains.cpu().numpy()
    errs, gaps = [], []
    for u, (n, r, off, snr) in enumerate(rows):
        assert (o[u, n:] == 0).all()
        if r < 0 or u == 8 or r == 2:                                 # no noise, a silent row, silent noise: the input's bits, gain 0
            assert np.array_equal(o[u, :n].view(np.int32), xs[u].view(np.int32)) and g[u] == 0, u
            continue
        y64, gap, g64 = c["refs"][u]
        assert abs(float(g[u]) - g64) <= 2.0 ** -22 * g64, (u, float(g[u]), g64)
        errs.append(float(np.abs(o[u, :n].astype(np.float64) - y64).max()))
        gaps.append(gap)
        achieved = WR.snr_of(o[u, :n], xs[u])
        assert abs(achieved - snr) <= 0.01, (u, achieved, snr)
    bar = max(4 * max(gaps), 1e-6)
    rec = dict(entry="las_noise_mix", in_place=in_place, tile=c["nt"], lengths=[r[0] for r in rows], err=max(errs), gap=max(gaps), bar=bar)
    print(json.dumps(rec))
    assert max(errs) <= bar, rec


# ---- determinism, batch independence ----------------------------------------------------------------------------------------------
def test_determinism_and_batch_independence():
    import torch
    from las.augment import WaveAugmenter
    l, cn = _lib(), _noise_case()
    nt, tile, chunk = cn["nt"], l.las_reverb_tile(), l.las_reverb_tap_chunk()
    aug = WaveAugmenter(FS, rirs=[WR.response(K, d, 40 + K) for K, d in ((chunk + 1, 0), (300, 150), (2 * chunk + 5, 2 * chunk + 4))],
                        noises=cn["aug"].noises)
    lens = [1, 300, tile + 1, 2 * tile + 37, nt + 1, tile - 1]
    xs = [WR.noise_signal(n, 900 + i) for i, n in enumerate(lens)]
    plan = aug.fixed_plan(6, rir_idx=[0, 1, 2, -1, 1, 2], noise_idx=[0, 1, -1, 0, 1, 0], noise_off=[999, 7, 0, 500, 3 * nt, 31],
                          snr_db=[0.0, 5.0, 0.0, 20.0, -5.0, 12.0])
    samples, ns = _upload(xs)
    a = aug.apply(samples, ns, plan, out=torch.empty_like(samples))
    b = aug.apply(samples, ns, plan, out=torch.full_like(samples, float("nan")))
    torch.cuda.synchronize()
    assert torch.equal(a, b)                                          # two calls: the same bits
    perm = [4, 2, 5, 0, 3, 1]
    ps, pns = _upload([xs[u] for u in perm], pad=200)
    pplan = aug.fixed_plan(6, rir_idx=plan.rir_idx[perm], noise_idx=plan.noise_idx[perm], noise_off=plan.noise_off[perm], snr_db=plan.snr_db[perm])
    p = aug.apply(ps, pns, pplan, out=torch.empty_like(ps))
    for u in range(6):
        s1, n1 = _upload([xs[u]], pad=0)
        one = aug.fixed_plan(1, rir_idx=plan.rir_idx[u:u + 1], noise_idx=plan.noise_idx[u:u + 1], noise_off=plan.noise_off[u:u + 1],
                             snr_db=plan.snr_db[u:u + 1])
        alone = aug.apply(s1, n1, one, out=torch.empty_like(s1))
        assert torch.equal(alone[0, :lens[u]], a[u, :lens[u]]), u     # alone = inside the batch, bit for bit
        assert torch.equal(p[perm.index(u), :lens[u]], a[u, :lens[u]]), u              # ... and inside a permuted batch


# ---- in front of las_frontend ------------------------------------------------------------------------------------------------------
def _fe():
    from las.frontend import FeatureExtractor
    if "fe" not in _extractors:
        _extractors["fe"] = FeatureExtractor(WR.fe_args())
    return _extractors["fe"]


def _condition():
    if "cond" not in _cases:
        from las.augment import WaveAugmenter
        rirs = [pp.synthetic_rir(FS, 0.05, 3), pp.synthetic_rir(FS, 0.03, 4)]
        _cases["cond"] = WaveAugmenter(FS, rirs=rirs, noises=[WR.noise_signal(3000, 5, rms=0.3)], reverb_prob=1.0, snr_db=(5, 15), seed=9)
    return _cases["cond"]


def test_extract_with_a_plan_is_the_front_end_on_the_augmented_samples():
    import torch
    fe, aug = _fe(), _condition()
    waves = R.signals(FS, False, lengths=(560, 4000, 9037))
    plan = aug.plan(3, 2)
    assert (plan.rir_idx >= 0).all() and (plan.noise_idx == 0).all()
    cube, lens = fe.extract(waves, augment=plan)
    samples, ns = _upload(waves)
    noisy = aug.apply(samples, ns, plan).cpu().numpy()
    want, wlens = fe.extract([noisy[u, :ns[u]] for u in range(3)])
    plain, plens = fe.extract(waves)
    torch.cuda.synchronize()
    assert lens.tolist() == wlens.tolist() == plens.tolist()          # frame counts do not change
    assert torch.equal(cube, want) and not torch.equal(cube, plain)
    # int16 input is fp32 before the filter: the L = M = 1 copy of the resample path
    wi = R.signals(FS, True, lengths=(560, 4000, 9037))
    ci, _ = fe.extract(wi, augment=plan)
    cf, _ = fe.extract([w.astype(np.float32) / np.float32(32767) for w in wi], augment=plan)
    assert torch.equal(ci, cf)
    # a plan that changes nothing: the cube of a call without a plan
    none, nlens = fe.extract(waves, augment=aug.fixed_plan(3))
    assert torch.equal(none, plain) and nlens.tolist() == plens.tolist()
    with pytest.raises(ValueError, match="plan of 2 rows"):
        fe.extract(waves, augment=aug.fixed_plan(2))


def test_features_of_an_augmented_utterance_against_float64():
    """the tolerance of tests/test_gpu_frontend.py's parity test, max(4 x gap, 1e-5): gap = the float32 augmentation followed by the
    float32 front end against the float64 augmentation followed by the float64 front end, on the same utterance"""
    import torch
    fe, aug, a = _fe(), _condition(), WR.fe_args()
    w = R.signals(FS, False, lengths=(560, 720, 9037))[2]
    plan = aug.fixed_plan(1, rir_idx=0, noise_idx=0, noise_off=1234, snr_db=10.0)
    cube, lens = fe.extract([w], augment=plan)
    torch.cuda.synchronize()
    h32, v32 = aug.rir_bank[0, :aug.rir_len[0]], aug.noise_bank[0, :aug.noise_len[0]]
    r64 = R.ref64(pp.mix_noise(WR.reverb64(w, h32, aug.rir_delay[0]), v32.astype(np.float64), 1234, 10.0), a)
    y32 = WR.mix32(WR.reverb32_batch([w], [h32], [aug.rir_delay[0]])[0], v32, 1234, 10.0)
    gap = float(np.abs(R.ref32(y32, a).astype(np.float64) - r64).max())
    err = float(np.abs(cube[0, :lens[0]].cpu().numpy().astype(np.float64) - r64).max())
    bar = max(4 * gap, 1e-5)
    print(json.dumps(dict(case="augmented features", err=err, gap=gap, bar=bar)))
    assert len(r64) == lens[0] and err <= bar
