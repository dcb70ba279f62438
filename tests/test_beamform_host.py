"""The beamforming contract (include/las_hip.h K18) on its float64 numpy restatement alone (tests/beamform_ref.py): what the
tracker buys on a generated array recording, how far its decisions are from rounding, and the rules one by one.  No device."""
import functools

import numpy as np
import pytest

import helpers  # noqa: F401
import beamform_ref as R

L, D, NF, GAMMA = 8000, 160, 16384, 0.01
PAUSE = (1.0, 2.0)


@functools.lru_cache(maxsize=None)
def case(pause):
    """the 6 s recording: C = 4, delays [0, 7, -12, 3] then [0, -5, 9, -20], 0 dB per channel; -> (x, clean, voice, delays, y, tau, a, r fp32)"""
    x, clean, voice, delays = R.array_recording(pause=PAUSE if pause else None)
    y, tau, a, r = R.enhance(x, 0, L, D, NF, GAMMA)
    return x, clean, voice, delays, y, tau, a, r


def test_tracked_delays_equal_the_truth_in_every_fully_active_window():
    x, clean, voice, delays, y, tau, a, r = case(False)
    for v in (0, 1):
        ws = R.active_windows(voice, L, v)
        assert len(ws) >= 10
        for w in ws:
            assert tau[:, w].tolist() == delays[v].tolist(), (v, w)


def test_a_pause_does_not_throw_the_tracked_delays_but_throws_the_raw_peak():
    x, clean, voice, delays, y, tau, a, r = case(True)
    H = L // 2
    inside = [w for w in range(tau.shape[1]) if w * H >= PAUSE[0] * 16000 and w * H + L <= PAUSE[1] * 16000]
    assert len(inside) >= 3
    assert np.abs(tau[:, inside] - delays[0][:, None]).max() <= 8
    assert np.abs(R.raw_argmax(r)[:, inside] - delays[0][:, None]).max() > 40
    for v in (0, 1):
        for w in R.active_windows(voice, L, v):
            assert tau[:, w].tolist() == delays[v].tolist(), (v, w)


@pytest.mark.parametrize("pause", [False, True])
def test_the_path_does_not_hinge_on_rounding(pause):
    """r as float64, as fp32, and perturbed by uniform +-1e-4 (about 100 times the error of an fp32 transform) under three seeds"""
    x = case(pause)[0]
    tau = case(pause)[5]
    r64 = R.gcc_phat(x, 0, L, D, NF)
    paths = [np.stack([R.track_channel(r64[c], GAMMA) - D for c in range(1, 4)])]            # (track_channel rounds to fp32: the contract)
    score64 = []
    for c in range(1, 4):                                                                   # the recursion on the unrounded float64 r
        sc, bp = r64[c, 0].copy(), []
        for w in range(1, r64.shape[1]):
            mx, b = R._best_predecessor(sc, GAMMA)
            sc = r64[c, w] + mx
            bp.append(b)
        p = [int(sc.argmax())]
        for b in reversed(bp):
            p.append(int(b[p[-1]]))
        score64.append(np.asarray(p[::-1]) - D)
    paths.append(np.stack(score64))
    for seed in (0, 1, 2):
        noisy = r64 + np.random.RandomState(seed).uniform(-1e-4, 1e-4, r64.shape)
        paths.append(np.stack([R.track_channel(noisy[c], GAMMA) - D for c in range(1, 4)]))
    for p in paths:
        assert np.array_equal(p, tau[1:])


def test_snr_gain_over_the_active_samples():
    x, clean, voice, delays, y, tau, a, r = case(False)
    on = voice >= 0
    gain = R.snr_db(y, clean, on) - R.snr_db(x[0], clean, on)
    assert gain >= 5.0, gain                                          # (the ideal of four channels: 10 log10 4 = 6.02)


# ---- the rules ---------------------------------------------------------------------------------------------------------------------------

def test_back_pointer_ties_go_to_the_nearer_then_the_smaller_predecessor():
    mx, arg = R._best_predecessor(np.array([1.0, 0.0, 0.0, 0.0, 1.0]), 0.25)
    assert mx.tolist() == [1.0, 0.75, 0.5, 0.75, 1.0]
    assert arg.tolist() == [0, 0, 0, 4, 4]                            # state 2: 0 and 4 tie at distance 2 -> the smaller
    mx, arg = R._best_predecessor(np.array([0.5, 0.0, 0.25, 0.0, 0.0]), 0.125)
    assert mx[2] == 0.25 and arg[2] == 2                              # state 2: itself ties with 0 (0.5 - 2 x 0.125) -> the nearer
    assert mx[3] == 0.125 and arg[3] == 2                             # state 3: 2 (0.25 - 0.125) ties with 0 (0.5 - 0.375) -> the nearer
    mx, arg = R._best_predecessor(np.zeros(5), 0.0)
    assert arg.tolist() == [0, 1, 2, 3, 4]                            # everything ties: distance 0


def test_last_window_ties_go_to_the_smaller_lag_magnitude_then_the_smaller_lag():
    r = np.zeros((1, 7), np.float32)
    r[0, [1, 5]] = 1.0                                                # lags -2 and +2
    assert R.track_channel(r, 0.5).tolist() == [1]
    r[0, 4] = 1.0                                                     # and +1
    assert R.track_channel(r, 0.5).tolist() == [4]
    r2 = np.zeros((2, 7), np.float32)
    r2[0, 3] = 1.0
    r2[1, [0, 6]] = 1.0                                               # equal peaks at -3 and +3 behind a window at 0
    assert R.track_channel(r2, 0.0).tolist() == [3, 0]
    assert R.track_channel(r2, 1.0).tolist() == [3, 3]                # the penalty of 3 outweighs the peak


def test_large_penalty_never_moves_and_zero_penalty_is_the_raw_peak():
    r = R.exact_tracker_input(2, 30, 6, seed=3, ties=False)
    p = R.track_channel(r[0], 64.0)
    assert (p == p[0]).all()
    assert R.track_channel(r[1], 0.0).tolist()[-1] == int(r[1, -1].argmax())


def test_weights_sum_to_one_and_the_reference_counts_as_its_best_partner():
    x, clean, voice, delays, y, tau, a, r = case(True)
    assert np.abs(a.astype(np.float64).sum(axis=0) - 1.0).max() <= 4e-7
    assert (a >= 0).all()
    assert np.array_equal(a[0], a[1:].max(axis=0))


def test_a_window_of_digital_silence_gives_the_reference_weight_one():
    x = case(False)[0].copy()
    x[:, 16000:28000] = 0.0                                           # windows 4 and 5 lie wholly inside
    y, tau, a, r = R.enhance(x, 2, L, D, NF, GAMMA)
    assert not r[:, 4].any() and not r[:, 5].any()
    for w in (4, 5):
        assert a[:, w].tolist() == [0.0, 0.0, 1.0, 0.0]
    assert (tau[2] == 0).all()


def test_window_counts():
    H = L // 2
    assert [R.windows(n, L) for n in (1, L, L + 1, L + H, L + H + 1)] == [1, 1, 2, 2, 3]


def test_cross_fade_weights_are_one_at_both_ends_and_at_the_centres():
    n, Wn = 6 * 4000 + 17, R.windows(6 * 4000 + 17, L)
    w0, w1, f = R.fade(n, L, Wn)
    H = L // 2
    assert (f[:H + 1] == 0).all() and (w0[:H + 1] == 0).all()
    assert (f[Wn * H:] == 0).all() and (w0[Wn * H:] == Wn - 1).all()
    for w in range(Wn):
        assert f[(w + 1) * H] == 0 and w0[(w + 1) * H] == w           # the centre of window w
    assert f[H + H // 2] == 0.5 and w0[H + H // 2] == 0 and w1[H + H // 2] == 1


def test_delay_sum_of_identical_channels_with_zero_delays_returns_the_channel():
    rng = np.random.RandomState(0)
    s = rng.randn(3 * L + 5).astype(np.float32)
    x = np.stack([s, s, s, s])
    Wn = R.windows(len(s), L)
    a = np.full((4, Wn), 0.25, np.float32)
    y = R.delay_sum(x, np.zeros((4, Wn), np.int32), a, L)
    s = s.astype(np.float64)
    H = L // 2
    assert np.array_equal(y[:H + 1], s[:H + 1]) and np.array_equal(y[Wn * H:], s[Wn * H:])   # one window alone at both ends (4 x 0.25 s is exact)
    assert (np.abs(y - s) <= 4 * 2.0 ** -53 * np.abs(s)).all()         # (1 - f) s + f s: 1 - f, two products and the sum, each rounded once


def test_a_lagging_channel_peaks_at_its_positive_lag():
    rng = np.random.RandomState(1)
    s = rng.randn(1200)
    x = np.stack([s[20:1020], s[20 - 9:1020 - 9], s[20 + 4:1020 + 4]]).astype(np.float32)   # x_1[t] = s[t - 9], x_2[t] = s[t + 4]
    r = R.gcc_phat(x, 0, 400, 16, 512)
    assert (R.raw_argmax(r)[1] == 9).all() and (R.raw_argmax(r)[2] == -4).all()
    assert np.abs(r[0, :, 16] - 1.0).max() <= 1e-12 and np.abs(np.delete(r[0], 16, axis=1)).max() <= 1e-12
