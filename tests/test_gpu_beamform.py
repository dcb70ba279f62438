"""las_gcc_phat, las_tdoa_track and las_delay_sum (csrc/beamform.hip, include/las_hip.h K18) on the device against the float64
numpy restatement tests/beamform_ref.py, at the smallest shapes at which each kernel can still go wrong, and the three chained on the
6 s array recording of tests/test_beamform_host.py.  The tracker's inputs are exactly representable (multiples of 2^-10, gamma 2^-7): its
delays must be equal element for element.  Every test prints its largest |got - ref| before it asserts."""
import functools

import numpy as np
import pytest

import helpers  # noqa: F401
import beamform_ref as R

pytestmark = pytest.mark.gpu

# Largest |got - ref| over this file's inputs, measured on an MI355X: MEASURED (r of las_gcc_phat at NF = 64 with int16 rows; 8.8e-8 at
# NF = 16384, y at most 9.5e-8, the weights 4.5e-8; the restatement's tracker weights come out equal).
# TOL = 16 x that, the margin of tests/test_gpu_diarize.py: room for another seed, nothing near an algorithmic error of 1e-2.
MEASURED = 1.023e-7
TOL = 16 * MEASURED
GARBAGE = 7                                           # finite garbage samples behind n in every row (ld = n + GARBAGE or more)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rows(x, n, ld, seed):
    """x [C, n] -> [C, ld] with finite garbage behind n"""
    rng = np.random.RandomState(seed)
    out = (rng.uniform(-0.9, 0.9, (x.shape[0], ld)) * (30000 if x.dtype == np.int16 else 1.0)).astype(x.dtype)
    out[:, :n] = x
    return out


def launch_gcc(rows, n, ref, L, D, NF):
    """rows [C, ld] on the host -> r float32 [C, Wn, 2 D + 1]; the output buffer carries a NaN tail that must stay"""
    import torch
    from las import _hip
    lib = _hip.lib()
    C, ld = rows.shape
    Wn = int(lib.las_bf_windows(n, L))
    assert Wn == R.windows(n, L)
    S = 2 * D + 1
    x, hann, tw = _dev(rows), _dev(R.hann(L)), _dev(R.twiddle(NF))
    r = torch.full((C * Wn * S + 5,), float("nan"), dtype=torch.float32, device="cuda")
    need = int(lib.las_bf_workspace_bytes(C, Wn, NF, D))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    _hip.check(lib.las_gcc_phat(_hip.p(x), int(rows.dtype == np.int16), ld, C, n, ref, L, D, NF, _hip.p(hann), _hip.p(tw), _hip.p(r), _hip.p(ws),
                                need, _hip.stream()), "las_gcc_phat")
    got = r.cpu().numpy()
    assert np.isnan(got[-5:]).all()
    return got[:-5].reshape(C, Wn, S)


def launch_track(r, ref, gamma):
    import torch
    from las import _hip
    lib = _hip.lib()
    C, Wn, S = r.shape
    D = (S - 1) // 2
    d_r = _dev(r.astype(np.float32))
    tau = torch.full((C * Wn + 3,), -77777, dtype=torch.int32, device="cuda")
    a = torch.full((C * Wn + 3,), float("nan"), dtype=torch.float32, device="cuda")
    need = int(lib.las_bf_workspace_bytes(C, Wn, 4, D))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    _hip.check(lib.las_tdoa_track(_hip.p(d_r), C, Wn, D, ref, float(gamma), _hip.p(tau), _hip.p(a), _hip.p(ws), need, _hip.stream()), "las_tdoa_track")
    t, w = tau.cpu().numpy(), a.cpu().numpy()
    assert (t[-3:] == -77777).all() and np.isnan(w[-3:]).all()
    return t[:-3].reshape(C, Wn), w[:-3].reshape(C, Wn)


def launch_sum(rows, n, L, tau, a):
    import torch
    from las import _hip
    lib = _hip.lib()
    C, ld = rows.shape
    Wn = tau.shape[1]
    x, d_tau, d_a = _dev(rows), _dev(tau.astype(np.int32)), _dev(a.astype(np.float32))
    y = torch.full((n + 9,), float("nan"), dtype=torch.float32, device="cuda")
    _hip.check(lib.las_delay_sum(_hip.p(x), int(rows.dtype == np.int16), ld, C, n, L, Wn, _hip.p(d_tau), _hip.p(d_a), _hip.p(y), _hip.stream()),
               "las_delay_sum")
    got = y.cpu().numpy()
    assert np.isnan(got[n:]).all()
    return got[:n]


def _close(got, ref, what):
    err = float(np.abs(np.asarray(got, np.float64) - ref).max())
    print("%s: max |got - ref| = %.3e (TOL %.3e)" % (what, err, TOL))
    assert np.isfinite(got).all(), what
    assert err <= TOL, (what, err)
    return err


# ---- las_gcc_phat ------------------------------------------------------------------------------------------------------------------------

def array_signal(C, n, i16, seed, silent=None):
    """white noise heard by channel c with a delay of ((5 c) mod 7) - 3 samples plus a little independent noise; channel `silent` is zeros"""
    rng = np.random.RandomState(seed)
    s = rng.randn(n + 16)
    x = np.stack([s[8 - (((5 * c) % 7) - 3):][:n] for c in range(C)]) * 0.1 + 0.02 * rng.randn(C, n)
    if silent is not None:
        x[silent] = 0.0
    return np.round(x * 8000).astype(np.int16) if i16 else x.astype(np.float32)


GCC_CASES = [
    # NF, L, D, C, ref, n, int16, silent channel
    (64, 62, 2, 2, 0, 1, False, None),                # L + D == NF; n = 1
    (64, 40, 20, 16, 15, 40, True, 3),                # D = L / 2; C = 16, the last channel the reference; n = L
    (64, 32, 1, 2, 1, 33, False, None),               # D = 1; n = L + 1
    (512, 400, 112, 3, 0, 1111, True, 2),             # L + D == NF; n no multiple of H
    (512, 300, 1, 2, 0, 777, False, 0),               # the REFERENCE is digital silence: r = 0 everywhere
    (16384, 16000, 384, 2, 1, 24005, False, None),    # L + D == NF at the largest transform
    (16384, 8000, 160, 16, 0, 9001, True, 7),         # the defaults at 16 kHz, sixteen channels
]


@functools.lru_cache(maxsize=None)
def gcc_case(i):
    NF, L, D, C, ref, n, i16, silent = GCC_CASES[i]
    x = array_signal(C, n, i16, seed=i, silent=silent)
    return x, R.gcc_phat(x, ref, L, D, NF)


@pytest.mark.parametrize("i", range(len(GCC_CASES)))
def test_gcc_phat(i):
    NF, L, D, C, ref, n, i16, silent = GCC_CASES[i]
    x, want = gcc_case(i)
    ld = n + GARBAGE + (i % 3)
    got = launch_gcc(_rows(x, n, ld, seed=100 + i), n, ref, L, D, NF)
    _close(got, want, "gcc %r" % (GCC_CASES[i],))
    if silent is not None:
        assert not got[silent].any() or silent == ref
        if silent == ref:
            assert not got.any()
    else:
        assert np.abs(got[ref, :, D] - 1.0).max() <= TOL


def test_gcc_phat_refusals():
    import torch
    from las import _hip
    lib = _hip.lib()
    x, hann, tw = _dev(np.zeros((2, 100), np.float32)), _dev(R.hann(40)), _dev(R.twiddle(64))
    r = torch.full((2 * 4 * 41,), float("nan"), dtype=torch.float32, device="cuda")
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    ok = dict(ld=100, C=2, n=100, ref=0, L=40, D=20, NF=64, ws_bytes=1 << 16)
    for bad in (dict(C=1), dict(C=17), dict(L=41), dict(D=0), dict(D=513), dict(NF=48), dict(NF=32), dict(NF=32768), dict(n=0), dict(n=101),
                dict(ref=2), dict(ref=-1), dict(ws_bytes=16)):
        k = dict(ok, **bad)
        rc = lib.las_gcc_phat(_hip.p(x), 0, k["ld"], k["C"], k["n"], k["ref"], k["L"], k["D"], k["NF"], _hip.p(hann), _hip.p(tw), _hip.p(r),
                              _hip.p(ws), k["ws_bytes"], _hip.stream())
        assert rc < 0 and lib.las_last_error(), bad
    torch.cuda.synchronize()
    assert np.isnan(r.cpu().numpy()).all()
    assert lib.las_bf_windows(0, 40) < 0 and lib.las_bf_windows(10, 41) < 0 and lib.las_bf_workspace_bytes(1, 1, 64, 1) == 0


# ---- las_tdoa_track ------------------------------------------------------------------------------------------------------------------------

TRACK_CASES = [
    # C, ref, Wn, D, gamma
    (2, 0, 1, 1, 2.0 ** -7),
    (3, 1, 2, 1, 2.0 ** -7),
    (2, 1, 300, 1, 2.0 ** -7),                        # 2 D + 1 = 3
    (4, 0, 300, 6, 2.0 ** -7),
    (2, 0, 40, 512, 2.0 ** -7),                       # 2 D + 1 = 1025: seventeen groups of 64 states, three backtrack chunks
    (16, 15, 50, 20, 0.0),                            # no penalty: every window's own peak (ties to the nearer predecessor)
    (3, 2, 50, 20, 64.0),                             # the path never moves
    (2, 0, 500, 40, 2.0 ** -5),                       # 81 states: more windows than one backtrack chunk holds
]


@functools.lru_cache(maxsize=None)
def track_case(i):
    C, ref, Wn, D, gamma = TRACK_CASES[i]
    r = R.exact_tracker_input(C, Wn, D, seed=10 + i)
    return r, R.tdoa_track(r, ref, gamma)


@pytest.mark.parametrize("i", range(len(TRACK_CASES)))
def test_tdoa_track(i):
    C, ref, Wn, D, gamma = TRACK_CASES[i]
    r, (tau, a) = track_case(i)
    got_tau, got_a = launch_track(r, ref, gamma)
    assert np.array_equal(got_tau, tau), TRACK_CASES[i]
    _close(got_a, a.astype(np.float64), "track weights %r" % (TRACK_CASES[i],))
    assert (got_tau[ref] == 0).all()
    if gamma == 64.0:
        assert (got_tau == got_tau[:, :1]).all()


def test_tdoa_track_zero_rows_give_the_reference_weight_one():
    r = R.exact_tracker_input(3, 6, 4, seed=1)
    r[:, 2] = 0.0
    r[:, 4] = -0.25
    tau, a = launch_track(r, 1, 2.0 ** -7)
    rt, ra = R.tdoa_track(r, 1, 2.0 ** -7)
    assert np.array_equal(tau, rt) and np.array_equal(a[:, [2, 4]], ra[:, [2, 4]])
    assert a[:, 2].tolist() == [0.0, 1.0, 0.0] and a[:, 4].tolist() == [0.0, 1.0, 0.0]


# ---- las_delay_sum -------------------------------------------------------------------------------------------------------------------------

SUM_CASES = [
    # C, n, L, largest |tau|, int16, ld - n
    (3, 50, 64, 45, False, 7),                        # Wn = 1; delays of -45 and +45: most reads lie before sample 0 or behind n
    (16, 1000, 64, 40, True, 9),                      # many windows, t at the exact window centres, sixteen channels
    (3, 4099, 400, 8, False, 5),                      # rows at an odd pitch, n no multiple of 4
    (4, 4096, 400, 8, False, 8),                      # aligned rows: the 16-byte loads at lags that are multiples of 4
]


@functools.lru_cache(maxsize=None)
def sum_case(i):
    C, n, L, T, i16, pad = SUM_CASES[i]
    rng = np.random.RandomState(50 + i)
    x = rng.uniform(-0.9, 0.9, (C, n))
    x = np.round(x * 30000).astype(np.int16) if i16 else x.astype(np.float32)
    Wn = R.windows(n, L)
    tau = rng.randint(-T, T + 1, (C, Wn)).astype(np.int32)
    tau[:, ::2] = 4 * (tau[:, ::2] // 4)
    tau[0, 0], tau[1, 0] = -T, T
    a = rng.uniform(0, 1, (C, Wn))
    a = (a / a.sum(axis=0)).astype(np.float32)
    return x, tau, a, R.delay_sum(x, tau, a, L)


@pytest.mark.parametrize("i", range(len(SUM_CASES)))
def test_delay_sum(i):
    C, n, L, T, i16, pad = SUM_CASES[i]
    x, tau, a, want = sum_case(i)
    got = launch_sum(_rows(x, n, n + pad, seed=200 + i), n, L, tau, a)
    assert np.abs(want).max() > 0.05                                  # (the case is not one whose reads all fall outside)
    _close(got, want, "delay_sum %r" % (SUM_CASES[i],))
    H, Wn, xw = L // 2, tau.shape[1], R.widen(x)
    for w in range(Wn):                               # at the centre of window w the output is that window's sum alone
        t = (w + 1) * H
        if t < n:
            only = sum(float(a[c, w]) * (xw[c, t + tau[c, w]] if 0 <= t + tau[c, w] < n else 0.0) for c in range(C))
            assert abs(got[t] - only) <= TOL


def test_delay_sum_refuses_a_wrong_window_count():
    from las import _hip
    x, tau, a, _ = sum_case(0)
    lib = _hip.lib()
    import torch
    y = torch.full((50,), float("nan"), dtype=torch.float32, device="cuda")
    d_x, d_tau, d_a = _dev(x), _dev(tau), _dev(a)
    rc = lib.las_delay_sum(_hip.p(d_x), 0, 50, 3, 50, 64, 2, _hip.p(d_tau), _hip.p(d_a), _hip.p(y), _hip.stream())
    assert rc < 0 and b"windows" in lib.las_last_error()
    assert np.isnan(y.cpu().numpy()).all()


# ---- the three chained ---------------------------------------------------------------------------------------------------------------------

L6, D6, NF6, GAMMA6 = 8000, 160, 16384, 0.01


@functools.lru_cache(maxsize=None)
def recording():
    x, clean, voice, delays = R.array_recording()
    return x, clean, voice, delays, R.enhance(x, 0, L6, D6, NF6, GAMMA6)


def chain(rows, n, NF=NF6):
    r = launch_gcc(rows, n, 0, L6, D6, NF)
    tau, a = launch_track(r, 0, GAMMA6)
    return r, tau, a, launch_sum(rows, n, L6, tau, a)


def test_chain_on_the_array_recording():
    x, clean, voice, delays, (y_ref, tau_ref, a_ref, r_ref) = recording()
    n = x.shape[1]
    r, tau, a, y = chain(_rows(x, n, n + GARBAGE, seed=1), n)
    _close(r, R.gcc_phat(x, 0, L6, D6, NF6), "chain r")
    for v in (0, 1):
        for w in R.active_windows(voice, L6, v):
            assert tau[:, w].tolist() == delays[v].tolist(), (v, w)
    assert np.array_equal(tau, tau_ref)                               # (the host test shows the path is 100 x the transform's error from changing)
    _close(a, a_ref.astype(np.float64), "chain a")
    _close(y, y_ref, "chain y")
    on = voice >= 0
    gain = R.snr_db(y, clean, on) - R.snr_db(x[0], clean, on)
    print("SNR gain %.2f dB" % gain)
    assert gain >= 5.0
    r2, tau2, a2, y2 = chain(_rows(x, n, n + GARBAGE, seed=1), n)     # a second call: the same bits
    assert np.array_equal(r, r2) and np.array_equal(tau, tau2) and np.array_equal(a, a2) and np.array_equal(y, y2)
    r3, tau3, a3, y3 = chain(_rows(x, n, n + 2 * GARBAGE + 1, seed=2), n)   # other garbage behind n, another pitch: nothing changes
    assert np.array_equal(r, r3) and np.array_equal(tau, tau3) and np.array_equal(a, a3) and np.array_equal(y, y3)


def test_beamformer_enhance_is_the_chain():
    import types
    from las import beamform as BF
    x, clean, voice, delays, _ = recording()
    n = x.shape[1]
    bf = BF.Beamformer(types.SimpleNamespace(bf_window_ms=500.0, bf_max_delay_ms=10.0, bf_jump_penalty=0.01, bf_ref=0), device="cuda")
    y, info = bf.enhance(x.T, 16000)
    assert (info["L"], info["D"], info["NF"], info["Wn"]) == (L6, D6, 8192, R.windows(n, L6))     # 8160 points fit 8192
    r, tau, a, y_chain = chain(_rows(x, n, n + GARBAGE, seed=1), n, NF=8192)
    assert y.dtype == np.float32 and np.array_equal(y, y_chain)
    t, w = BF.Beamformer.delays(info)
    assert np.array_equal(t, tau) and np.array_equal(w, a)
    with pytest.raises(ValueError, match="bf_window_ms of at most 330"):
        BF.geometry(500.0, 10.0, 48000)
    assert BF.geometry(330.0, 10.0, 48000) == (15840, 480, 16384) and BF.geometry(500.0, 10.0, 32000) == (16000, 320, 16384)
    assert BF.geometry(500.0, 10.0, 16000) == (8000, 160, 8192)
    with pytest.raises(ValueError, match="bf_ref 5"):
        BF.Beamformer(types.SimpleNamespace(bf_ref=5), device="cuda").enhance(x.T, 16000)


def test_beamformer_enhance_takes_int16_samples():
    """the int16 rows of a 16-bit file handed over as they are: widened on the device as v / 32767, the same bits as the chain on them"""
    import types
    from las import beamform as BF
    x = recording()[0]
    n = x.shape[1]
    q = np.round(np.clip(x, -1, 1) * 32767).astype(np.int16)
    y, info = BF.Beamformer(types.SimpleNamespace(), device="cuda").enhance(q.T, 16000)
    r, tau, a, y_chain = chain(_rows(q, n, n + GARBAGE, seed=3), n, NF=8192)
    assert np.array_equal(y, y_chain) and np.array_equal(BF.Beamformer.delays(info)[0], tau)
    _close(y, R.enhance(q, 0, L6, D6, 8192, GAMMA6)[0], "enhance int16 y")
