"""Host side of the voice-activity segmenter (no GPU): the numpy restatement (tests/vad_ref.py) on a signal whose answer is
known, las_vad_max_runs against brute force, the planner's cut rule, the refusals of las_vad that come before any launch, the flags."""
import argparse
import ctypes
import math

import numpy as np
import pytest

import helpers  # noqa: F401
import vad_ref as R
from las import _hip
from las import vad as V
from las.arguments import parse_args, str2bool


# ---- the restatement on a known signal -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("floor_amp", [0.0, 1e-4], ids=["zeros", "floor_60dB_down"])
def test_restatement_finds_one_run_per_burst(floor_amp):
    va = V.VoiceActivity(parse_args([]))
    rate = 16000
    fl, step = va.geometry(rate)
    assert (fl, step, va.hang, va.min_run, va.ratio) == (400, 160, 20, 10, 1e-4) and va.floor(fl) == 400 * 10.0 ** -7
    wave, truth = R.bursts(rate, 3, floor_amp=floor_amp, seed=4)
    e, emax, runs = R.vad(wave, fl, step, va.ratio, va.floor(fl), va.hang, va.min_run)
    assert emax == e.max() and len(e) == (len(wave) - fl) // step
    assert len(runs) == len(truth) == 3
    slack = va.hang + math.ceil(fl / step)
    for (a, b), (p0, p1) in zip(runs, truth):
        assert abs(a - p0 / step) <= slack and abs(b - p1 / step) <= slack, ((a, b), (p0 / step, p1 / step))
    # the energies are the plain float64 sums up to the rounding of 400 additions
    for t in (0, 100, len(e) - 1):
        x = wave[t * step:t * step + fl].astype(np.float64)
        assert abs(e[t] - np.sum(x * x)) <= 400 * 2.0 ** -53 * np.sum(x * x)
    # int16 is value / 32767 in fp32
    i16 = np.asarray([32767, -32768, 1, 0], np.int16)
    assert np.array_equal(R.to_f32(i16), np.asarray([1.0, np.float32(-32768) / np.float32(32767), np.float32(1) / np.float32(32767), 0.0], np.float32))


# ---- las_vad_max_runs -----------------------------------------------------------------------------------------------------------------
def test_max_runs_is_the_brute_force_maximum():
    lib = _hip.lib()
    for hang in range(3):
        for T in range(1, 15):
            full, best = (1 << T) - 1, 0
            for raw in range(1 << T):
                s = raw
                for d in range(1, hang + 1):
                    s |= (raw << d) | (raw >> d)
                s &= full
                best = max(best, bin(s & ~(s << 1)).count("1"))          # run starts
            assert lib.las_vad_max_runs(T, hang) == best == R.max_runs(T, hang) == -(-T // (2 * hang + 2)), (T, hang, best)
    assert lib.las_vad_max_runs(0, 3) == 0 and lib.las_vad_max_runs(-1, 0) < 0 and lib.las_vad_max_runs(5, -1) < 0
    assert lib.las_vad_max_runs(360000, 20) == 8572 and lib.las_vad_tile() >= 16
    assert lib.las_vad_workspace_bytes(1, 360000) > 8 * 360000 and lib.las_vad_workspace_bytes(0, 5) == 0


# ---- the planner ----------------------------------------------------------------------------------------------------------------------
def test_planner_cuts_at_the_quietest_frame():
    rng = np.random.RandomState(2)
    for max_frames in (4, 5, 16, 100):
        T = 1000
        energy = rng.rand(T)
        bounds = sorted(rng.choice(np.arange(0, T, 2), size=12, replace=False))
        runs = [(int(a), int(b)) for a, b in zip(bounds[0::2], bounds[1::2])] + [(T - max_frames - 1, T)]
        runs = sorted(set((a, b) for a, b in runs if b - a >= 2))
        runs = [r for k, r in enumerate(runs) if k == 0 or r[0] >= runs[k - 1][1]]
        segs = V.plan_segments(runs, energy, max_frames)
        assert segs == R.plan_segments(runs, energy, max_frames)
        assert all(2 <= b - a <= max_frames for a, b in segs)
        k = 0
        for a, b in runs:                                                 # the segments tile each run exactly
            assert segs[k][0] == a
            while segs[k][1] != b:
                assert segs[k][1] == segs[k + 1][0] and segs[k][1] < b
                k += 1
            k += 1
        assert k == len(segs)
    # the cut itself: the quietest frame of [a + max_frames // 2, a + max_frames]
    e = np.ones(100)
    e[[13, 17, 31]] = 0.5, 0.25, 0.1
    assert V.plan_segments([(5, 60)], e, 20) == [(5, 17), (17, 31), (31, 41), (41, 60)]      # 41: an all-equal window, its first frame
    e[:] = 1.0
    e[[20, 23]] = 0.5                                                     # a tie: the smaller t
    assert V.plan_segments([(10, 40)], e, 20) == [(10, 20), (20, 40)]
    assert V.plan_segments([(10, 30)], e, 20) == [(10, 30)]               # exactly max_frames: one segment
    # one frame over: the window stops at b - 2, so the rest keeps two frames
    e[:] = np.arange(100)[::-1]
    assert V.plan_segments([(0, 21)], e, 20) == [(0, 19), (19, 21)]
    with pytest.raises(ValueError):
        V.plan_segments([(0, 10)], e, 3)
    with pytest.raises(ValueError):
        V.plan_segments([(0, 1)], e, 20)
    assert R.sample_ranges([(0, 2), (5, 9)], 400, 160, 1700) == [(0, 560), (800, 1680)]
    assert R.sample_ranges([(5, 9)], 400, 160, 1600) == [(800, 1600)]


# ---- the C entry ----------------------------------------------------------------------------------------------------------------------
def test_c_entry_validates_before_any_launch():
    """las_vad refuses bad arguments on the host (nothing here is a device pointer: a launch would fault)"""
    l = _hip.lib()
    n, Tmax, fl, step, hang = 2, 100, 400, 160, 3
    ld = (Tmax + 2) * step + fl
    ok_ns = [Tmax * step + fl, 300]                                       # 100 frames, and a row too short for one (T = 0)

    def call(ns=None, **over):
        ns = ns if ns is not None else ok_ns
        kw = dict(samples=ctypes.c_void_p(1 << 20), samples_i16=0, ld_samples=ld, n_samples=ctypes.c_void_p(256),
                  n_samples_host=(ctypes.c_int * len(ns))(*ns), n=n, Tmax=Tmax, fl=fl, step=step, ratio=1e-4, floor=4e-5, hang=hang, min_run=2,
                  energy=None, emax=None, runs=ctypes.c_void_p(1 << 21), max_runs=int(l.las_vad_max_runs(Tmax, hang)),
                  n_runs=ctypes.c_void_p(1 << 22), ws=ctypes.c_void_p(1 << 23), ws_bytes=int(l.las_vad_workspace_bytes(n, Tmax)), stream=None)
        kw.update(over)
        order = ("samples", "samples_i16", "ld_samples", "n_samples", "n_samples_host", "n", "Tmax", "fl", "step", "ratio", "floor", "hang",
                 "min_run", "energy", "emax", "runs", "max_runs", "n_runs", "ws", "ws_bytes", "stream")
        return l.las_vad(*[kw[k] for k in order]), l.las_last_error()

    for ptr in ("samples", "n_samples", "n_samples_host", "runs", "n_runs", "ws"):
        rc, msg = call(ok_ns, **{ptr: None})
        assert rc < 0 and b"null pointer" in msg, ptr
    for bad, word in ((dict(n=0), b"n=0"), (dict(n=65536), b"n=65536"), (dict(Tmax=0), b"Tmax=0"), (dict(fl=0), b"frame of 0 samples"),
                      (dict(step=0), b"every 0"), (dict(hang=-1), b"hang=-1"), (dict(min_run=1), b"min_run=1"), (dict(min_run=0), b"min_run=0"),
                      (dict(ratio=0.0), b"ratio=0"), (dict(ratio=1.5), b"ratio=1.5"), (dict(ratio=float("nan")), b"ratio="),
                      (dict(floor=-1.0), b"floor=-1"), (dict(floor=float("inf")), b"floor=inf"), (dict(floor=float("nan")), b"floor="),
                      (dict(max_runs=int(l.las_vad_max_runs(Tmax, hang)) - 1), b"max_runs=12"), (dict(ld_samples=0), b"ld_samples=0"),
                      (dict(ld_samples=1 << 31), b"ld_samples=2147483648"),
                      (dict(ws_bytes=int(l.las_vad_workspace_bytes(n, Tmax)) - 1), b"workspace of")):
        rc, msg = call(ok_ns, **bad)
        assert rc < 0 and word in msg, (bad, msg)
    assert l.las_vad_max_runs(Tmax, hang) == 13
    rc, msg = call([ld + 1, 300])
    assert rc < 0 and b"recording 0 has %d samples" % (ld + 1) in msg
    rc, msg = call([ok_ns[0], 0])
    assert rc < 0 and b"recording 1 has 0 samples" in msg
    rc, msg = call([(Tmax + 1) * step + fl, 300])
    assert rc < 0 and b"recording 0 has 101 frames (Tmax=100)" in msg
    # ratio = 1 and floor = 0 are inside their ranges, a row too short for a frame is no error: the next refusal is the workspace's
    rc, msg = call(ok_ns, ratio=1.0, floor=0.0, ws_bytes=0)
    assert rc < 0 and b"workspace of 0 bytes" in msg


# ---- the flags ------------------------------------------------------------------------------------------------------------------------
def test_flags():
    p = argparse.ArgumentParser()
    V.add_flags(p, str2bool)
    a = p.parse_args([])
    assert (a.segment, a.vad_top_db, a.vad_floor_db, a.vad_pad_ms, a.vad_min_speech_ms, a.max_segment_s) == (False, 40, -70, 200, 100, 17.0)
    a = p.parse_args(["--segment", "True", "--vad_top_db", "30", "--vad_pad_ms", "55", "--vad_min_speech_ms", "5", "--max_segment_s", "2.5"])
    a.frame_length, a.frame_step = 25, 10
    va = V.VoiceActivity(a)
    assert a.segment is True and (va.ratio, va.hang, va.min_run) == (1e-3, 6, 2)      # min_run: at least 2
    assert va.max_frames(16000) == 248 and (247 * 160 + 400) / 16000 <= 2.5 < (248 * 160 + 400) / 16000
    assert va.geometry(8000) == (200, 80) and va.max_frames(8000) == 248              # the same milliseconds at any rate
    assert not hasattr(parse_args([]), "segment")                                     # las.arguments keeps the reference's table
    import transcribe
    with pytest.raises(ValueError, match="--segment"):
        transcribe.main(["--segment", "True", "--ctc", "True", "--align_text", "no_such_refs.txt", "no_such_file.wav"])
