"""The MVDR beamformer's contract (include/las_hip.h K19) on the host: the float64 restatement tests/mvdr_ref.py alone on the 6 s,
4-channel recording (a voice at fractional delays, a directional interferer at 0 dB, sensor noise 20 dB below), the contract's rules one
by one, and the flag refusals of las.cli.check_flags.  No device."""
import functools

import numpy as np
import pytest

import helpers  # noqa: F401
import beamform_ref as BR
import mvdr_ref as R

FS = 16000
# --mvdr_top_db 2.2 and not the default 25: the interferer is as loud as the voice, so a frame without the voice lies only 3 dB under a
# frame with it (and the loudest frame a little over that).  At 25 dB under the loudest frame EVERY frame of this recording is speech, no
# frame is left to learn the noise from (N0 = 0), and the beamformer falls back to the reference channel -- the test below shows it.
TOP_DB, LOADING = 2.2, 1e-3
NF, BF, HANG, RATIO = R.geometry(32.0, 2000.0, 100.0, TOP_DB, FS)     # 512, 125, 6


@functools.lru_cache(maxsize=None)
def one_voice():
    x, clean, voice = R.recording()
    y, info = R.enhance(x, 0, NF, BF, RATIO, 0.0, HANG, LOADING)
    return x, clean, voice, y, info


def frame_kinds(voice, v):
    """per frame: lies wholly inside talker v / wholly where nobody talks (frames that reach outside the recording: neither / the latter)"""
    n, Hs = len(voice), NF // 2
    Tf = R.frames(n, NF)
    inside = np.array([(t - 1) * Hs >= 0 and (t + 1) * Hs <= n and (voice[(t - 1) * Hs:(t + 1) * Hs] == v).all() for t in range(Tf)])
    silent = np.array([(voice[max(0, (t - 1) * Hs):min(n, (t + 1) * Hs)] == -1).all() for t in range(Tf)])
    return inside, silent


def test_geometry_of_the_defaults():
    assert (NF, BF, HANG) == (512, 125, 6) and abs(RATIO - 10 ** -0.22) < 1e-15
    assert R.geometry(32.0, 1000.0, 32.0, 25.0, FS)[:3] == (512, 62, 2)


def test_identity_weights_reconstruct_the_reference_channel():
    x = one_voice()[0]
    Tf = R.frames(x.shape[1], NF)
    for ref in (0, 3):
        y = R.apply(x, R.identity_weights(R.blocks(Tf, BF), NF // 2 + 1, 4, ref), NF, BF)
        err = np.abs(y - R.widen(x)[ref]).max()
        print("reconstruction of channel %d: %.2e" % (ref, err))
        assert err <= 1e-12
    w = np.sin(np.pi * (np.arange(NF) + 0.5) / NF)
    assert np.abs(w[:NF // 2] ** 2 + w[NF // 2:] ** 2 - 1.0).max() < 1e-15


def test_mask_on_the_recording():
    """no voiced frame missed; at most 5 % of the unvoiced frames called speech.  The dilation alone turns the `hang` frames on either side
    of the voice into speech: with the default --mvdr_pad_ms 100 (hang = 6) that is 12 of this recording's 155 unvoiced frames, 7.7 %, by
    construction, whatever the rule does.  The bound is therefore checked at hang = 2 (--mvdr_pad_ms 32, the prototype's), and at the
    default every frame wrongly called speech must lie within `hang` frames of a frame that holds voice."""
    x, clean, voice, y, info = one_voice()
    inside, silent = frame_kinds(voice, 0)
    m2, e = R.mask(x, 0, NF, RATIO, 0.0, 2)
    wrong2 = int((silent & (m2 == 1)).sum())
    print("hang 2: missed %d of %d voiced frames, %d of %d unvoiced frames called speech" % ((inside & (m2 == 0)).sum(), inside.sum(), wrong2, silent.sum()))
    assert inside.sum() > 200 and silent.sum() > 140
    assert not (inside & (m2 == 0)).any()
    assert wrong2 <= 0.05 * silent.sum()
    m6 = info["m"]
    assert not (inside & (m6 == 0)).any()
    wrong6 = np.flatnonzero(silent & (m6 == 1))
    some_voice = np.flatnonzero(~silent)
    assert all(np.abs(some_voice - t).min() <= HANG for t in wrong6)
    print("hang 6: %d of %d unvoiced frames called speech, all within 6 frames of the voice" % (len(wrong6), silent.sum()))


def test_the_default_top_db_leaves_no_noise_frame_at_0_db_and_the_reference_channel_comes_out():
    x = one_voice()[0]
    y, info = R.enhance(x, 0, NF, BF, 10.0 ** -2.5, 0.0, HANG, LOADING)
    assert info["m"].all() and info["counts"][0] == 0 and not info["valid"].any() and not info["phi_n"].any()
    assert np.abs(y - R.widen(x)[0]).max() <= 1e-12


def test_snr_and_correlation_on_the_recording():
    x, clean, voice, y, info = one_voice()
    on = R.inside(voice, 0, NF)
    ds = R.delay_sum_true(x, R.VOICE_DELAYS)
    snr0, snr_ds, snr = BR.snr_db(x[0], clean, on), BR.snr_db(ds, clean, on), BR.snr_db(y, clean, on)
    corr0, corr = np.corrcoef(x[0][on], clean[on])[0, 1], np.corrcoef(y[on], clean[on])[0, 1]
    print("SNR: channel 0 %.2f dB, delay-and-sum at the true delays rounded %.2f dB, MVDR %.2f dB (%.2f dB above); correlation %.4f -> %.4f"
          % (snr0, snr_ds, snr, snr - snr_ds, corr0, corr))
    assert abs(snr0) < 0.5 and 0.68 < corr0 < 0.74                    # the recording is what the bars were set for
    assert snr_ds <= 10 * np.log10(4) + 0.1                           # the fixed beamformer stays at its ideal 10 log10(C)
    assert snr >= snr_ds + 6.0
    assert corr >= 0.95
    cond = max(np.linalg.cond(info["phi_n"][k] + LOADING * np.trace(info["phi_n"][k]).real / 4 * np.eye(4)) for k in range(NF // 2 + 1))
    print("largest condition number of a loaded noise covariance: %.3g" % cond)
    assert cond < 1e5


def test_two_voices_with_blocks_of_one_second():
    x, clean, voice = R.recording(delays=(R.VOICE_DELAYS, R.VOICE2_DELAYS))
    nf, bf, hang, ratio = R.geometry(32.0, 1000.0, 100.0, TOP_DB, FS)
    assert bf == 62
    y, info = R.enhance(x, 0, nf, bf, ratio, 0.0, hang, LOADING)
    for v, dl in ((0, R.VOICE_DELAYS), (1, R.VOICE2_DELAYS)):
        on = R.inside(voice, v, nf)
        snr_ds, snr = BR.snr_db(R.delay_sum_true(x, dl), clean, on), BR.snr_db(y, clean, on)
        corr = np.corrcoef(y[on], clean[on])[0, 1]
        print("voice %d: delay-and-sum %.2f dB, MVDR %.2f dB, correlation %.4f" % (v, snr_ds, snr, corr))
        assert snr >= snr_ds + 6.0 and corr >= 0.95


# ---- the rules, one by one -----------------------------------------------------------------------------------------------------------

def test_frame_count_at_the_edges():
    for nf in (64, 512):
        Hs = nf // 2
        assert [R.frames(n, nf) for n in (1, Hs, Hs + 1, 2 * Hs, 2 * Hs + 1)] == [2, 2, 3, 3, 4]
    x = np.arange(1, 41, dtype=np.float64)[None]
    fr = R.frame_samples(x, 64, 0, R.frames(40, 64))                  # Hs + 8 samples: three frames, every sample in exactly two
    assert fr.shape == (1, 3, 64) and fr[0, 0, :32].sum() == 0 and (fr[0, 0, 32:] == x[0, :32]).all()
    assert (fr[0, 1, :40] == x[0]).all() and not fr[0, 1, 40:].any() and (fr[0, 2, :8] == x[0, 32:]).all() and not fr[0, 2, 8:].any()
    assert R.blocks(7, 3) == 3 and R.blocks(6, 3) == 2 and R.blocks(1, 9) == 1


def _burst_rows(n, where, amp=0.5):
    x = np.zeros((2, n), np.float32)
    for a, b in where:
        x[:, a:b] = amp
    return x


def test_hang_at_both_ends_and_the_threshold_taking_the_floor():
    Hs = 32
    x = _burst_rows(10 * Hs, [(0, Hs), (9 * Hs, 10 * Hs)])            # the first and the last segment are loud: frames 0, 1 and 9, 10
    m, e = R.mask(x, 0, 64, 0.5, 0.0, 2)
    assert len(m) == 11 and m.tolist() == [1, 1, 1, 1, 0, 0, 0, 1, 1, 1, 1]
    assert e[0] == 32 * 0.25 and e[1] == 32 * 0.25 and e[2] == 0
    m0, _ = R.mask(x, 0, 64, 0.5, 0.0, 0)
    assert m0.tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 1]
    x[:, 4 * Hs:5 * Hs] = 0.1                                         # a quiet burst: e = 0.32 in the frames 4 and 5
    assert R.mask(x, 0, 64, 0.01, 0.0, 0)[0].tolist() == [1, 1, 0, 0, 1, 1, 0, 0, 0, 1, 1]
    assert R.mask(x, 0, 64, 0.01, 1.0, 0)[0].tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 1]      # thr = max(0.08, 1.0): the floor
    assert not R.mask(np.zeros((2, 100), np.float32), 0, 64, 0.5, 0.0, 3)[0].any()              # e > 0 is part of the rule


def _noise_rows(C, n, seed):
    return (0.1 * np.random.RandomState(seed).randn(C, n)).astype(np.float32)


def test_covariances_are_hermitian_as_stored_and_sum_to_the_whole():
    x = _noise_rows(3, 700, 0)
    Tf = R.frames(700, 64)
    m = np.random.RandomState(1).uniform(0, 1, Tf).astype(np.float32)
    cnt, phi_n, phi_y = R.cov(x, m, 64, 5)
    for P in (phi_n, phi_y):
        assert np.array_equal(P, np.conj(np.swapaxes(P, -1, -2)))
        assert not np.diagonal(P, axis1=-2, axis2=-1).imag.any()
    assert abs(cnt[0] + cnt[1:].sum() - Tf) < 1e-9
    X = R.stft(R.widen(x), 64)
    whole = np.einsum("itk,jtk->kij", X, X.conj())
    assert np.abs(phi_n * cnt[0] + (phi_y * cnt[1:, None, None, None]).sum(axis=0) - whole).max() <= 1e-12 * np.abs(whole).max()


def test_no_noise_frame_and_a_block_without_speech():
    x = _noise_rows(2, 700, 2)
    Tf = R.frames(700, 64)
    cnt, phi_n, phi_y = R.cov(x, np.ones(Tf, np.float32), 64, 8)
    assert cnt[0] == 0 and not phi_n.any() and phi_y.any()
    w, valid = R.weights(phi_n, phi_y, cnt, 1, LOADING)
    assert not valid.any() and np.array_equal(w, R.identity_weights(len(cnt) - 1, 33, 2, 1))
    m = np.ones(Tf, np.float32)
    m[8:16] = 0                                                       # block 1 holds no speech
    cnt, phi_n, phi_y = R.cov(x, m, 64, 8)
    assert cnt[2] == 0 and cnt[0] == 8 and not phi_y[1].any() and phi_y[0].any() and phi_n.any()
    w, valid = R.weights(phi_n, phi_y, cnt, 0, LOADING)
    assert not valid[1].any()
    assert np.array_equal(w[1], w[0])                                 # the hold: block 0's weights


def _spd(C, seed, scale=1.0):
    rng = np.random.RandomState(seed)
    A = rng.randn(C, 2 * C) + 1j * rng.randn(C, 2 * C)
    return scale * (A @ A.conj().T) / (2 * C)


def test_the_hold_pass():
    C, K, Nb = 3, 33, 5
    phi_n = np.stack([_spd(C, k) for k in range(K)])
    phi_y = np.stack([np.stack([phi_n[k] + _spd(C, 100 * b + k) for k in range(K)]) for b in range(Nb)])
    cnt = np.array([10.0, 0.0, 4.0, 0.0, 3.0, 0.0])                   # the blocks 1 and 3 hold speech
    w, valid = R.weights(phi_n, phi_y, cnt, 2, LOADING)
    assert valid[:, 0].tolist() == [0, 1, 0, 1, 0]
    assert np.array_equal(w[0], w[1])                                 # a later block only in front of the first valid one
    assert np.array_equal(w[2], w[1]) and np.array_equal(w[4], w[3]) and not np.array_equal(w[3], w[1])      # an earlier one wins
    k = 7
    G, _ = R.solve_bin(phi_n[k], phi_y[1, k], LOADING)
    assert np.allclose(w[1, k], G[:, 2] / np.trace(G).real, rtol=0, atol=1e-14)
    A = phi_n[k] + LOADING * np.trace(phi_n[k]).real / C * np.eye(C)
    assert np.abs(A @ G - (phi_y[1, k] - phi_n[k])).max() < 1e-12
    none, valid = R.weights(phi_n, phi_y, np.array([10.0, 0, 0, 0, 0, 0]), 1, LOADING)
    assert not valid.any() and np.array_equal(none, R.identity_weights(Nb, K, C, 1))     # no valid block at all: e_ref


def test_g_on_either_side_of_the_bar_and_a_zero_noise_bin():
    C, K = 2, 33
    phi_n = np.stack([np.eye(C, dtype=complex)] * K)
    phi_n[5] = 0                                                      # a bin without noise: tn = 0
    phi_y = np.stack([phi_n.copy(), phi_n.copy()])
    for k in range(K):                                                # g = tr(eps I) / (1 + loading) = 2 eps / 1.001
        phi_y[0, k] = phi_n[k] + (2e-6 if k % 2 else 0.4e-6) * np.eye(C)
        phi_y[1, k] = phi_n[k] + 1e-3 * np.eye(C)
    w, valid, g = R.weights(phi_n, phi_y, np.array([5.0, 5.0, 5.0]), 0, LOADING, return_g=True)
    odd = np.arange(K) % 2 == 1
    assert (g[0, odd & (np.arange(K) != 5)] > 3e-6).all() and (g[0, ~odd] < 1e-6).all()
    assert valid[0, odd].tolist() == [0 if k == 5 else 1 for k in np.flatnonzero(odd)] and not valid[0, ~odd].any()
    assert valid[1].tolist() == [0 if k == 5 else 1 for k in range(K)]
    assert np.array_equal(w[:, 5], R.identity_weights(2, 1, C, 0)[:, 0]) and np.isnan(g[:, 5]).all()
    assert np.array_equal(w[0, 2], w[1, 2])                           # g under the bar: block 1's weights, the only valid ones
    assert np.allclose(w[1, 2], [0.5, 0.0])                           # P = eps I: the weight is e_ref / C


# ---- flags -----------------------------------------------------------------------------------------------------------------------------

def _check(argv):
    import transcribe
    from las import cli, vad
    parser = transcribe.build_parser()
    cli.add_flags(parser)
    vad.add_flags(parser, cli.str2bool)
    cli.add_diarize_flags(parser)
    cli.add_beamform_flags(parser)
    args = parser.parse_args(["--synthetic", "True"] + argv)
    return cli.check_flags(args, parser), args


def test_flags_default_to_delaysum_and_mvdr_fills_its_defaults():
    from las import cli
    assert set(cli.MVDR_DEFAULTS) == {"mvdr_frame_ms", "mvdr_block_ms", "mvdr_top_db", "mvdr_floor_db", "mvdr_pad_ms", "mvdr_loading"}
    _, args = _check(["--beamform", "True"])
    assert args.bf_method == "delaysum" and all(getattr(args, k) is None for k in cli.MVDR_DEFAULTS)
    _, args = _check(["--beamform", "True", "--bf_method", "mvdr", "--bf_ref", "1", "--vad_floor_db", "-60"])
    assert (args.mvdr_frame_ms, args.mvdr_block_ms, args.mvdr_top_db, args.mvdr_floor_db, args.mvdr_pad_ms, args.mvdr_loading, args.bf_ref) == \
           (32.0, 2000.0, 25.0, -60.0, 100.0, 1e-3, 1)
    _, args = _check(["--beamform", "True", "--bf_method", "mvdr", "--mvdr_floor_db", "-50", "--mvdr_top_db", "2.2"])
    assert (args.mvdr_floor_db, args.mvdr_top_db) == (-50.0, 2.2)


@pytest.mark.parametrize("argv,msg", [
    (["--mvdr_top_db", "3"], "--mvdr_top_db sets the beamformer of --beamform True --bf_method mvdr"),
    (["--beamform", "True", "--mvdr_loading", "0.01"], "--mvdr_loading sets the beamformer of --bf_method mvdr: give both"),
    (["--bf_method", "mvdr"], "--bf_method mvdr chooses the beamformer of --beamform True: give both"),
    (["--beamform", "True", "--bf_method", "mvdr", "--bf_window_ms", "250"], "--bf_window_ms sets the delay tracker"),
    (["--beamform", "True", "--bf_method", "mvdr", "--bf_max_delay_ms", "5"], "--bf_max_delay_ms sets the delay tracker"),
    (["--beamform", "True", "--bf_method", "mvdr", "--bf_jump_penalty", "0.1"], "--bf_jump_penalty sets the delay tracker"),
    (["--beamform", "True", "--bf_method", "mvdr", "--mvdr_frame_ms", "0"], "--mvdr_frame_ms 0.0: a finite number > 0"),
    (["--beamform", "True", "--bf_method", "mvdr", "--mvdr_block_ms", "nan"], "--mvdr_block_ms nan"),
    (["--beamform", "True", "--bf_method", "mvdr", "--mvdr_top_db", "-3"], "--mvdr_top_db -3.0"),
    (["--beamform", "True", "--bf_method", "mvdr", "--mvdr_top_db", "inf"], "--mvdr_top_db inf"),
    (["--beamform", "True", "--bf_method", "mvdr", "--mvdr_floor_db", "nan"], "--mvdr_floor_db nan"),
    (["--beamform", "True", "--bf_method", "mvdr", "--mvdr_pad_ms", "-1"], "--mvdr_pad_ms -1.0"),
    (["--beamform", "True", "--bf_method", "mvdr", "--mvdr_loading", "0"], "--mvdr_loading 0.0"),
    (["--beamform", "True", "--bf_method", "mvdr", "--mvdr_loading", "inf"], "--mvdr_loading inf")])
def test_flag_refusals(argv, msg):
    with pytest.raises(ValueError, match=msg):
        _check(argv)


def test_frame_length_outside_the_transform_names_the_flag():
    from las import beamform as BF
    assert BF.mvdr_geometry(32.0, 2000.0, 100.0, 16000) == (512, 125, 6)
    assert BF.mvdr_geometry(4.0, 2000.0, 100.0, 16000)[0] == 64 and BF.mvdr_geometry(64.0, 2000.0, 100.0, 16000)[0] == 1024
    for ms in (1.0, 65.0):
        with pytest.raises(ValueError, match="--mvdr_frame_ms"):
            BF.mvdr_geometry(ms, 2000.0, 100.0, 16000)
    assert BF.mvdr_geometry(32.0, 1.0, 0.0, 16000)[1:] == (1, 0)
    w, tw = BF.mvdr_tables(64)
    assert np.array_equal(w, R.window(64)) and np.array_equal(tw, R.twiddle(64))
