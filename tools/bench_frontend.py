"""bench_frontend.py -- utterances/s of the device front end (las.frontend.FeatureExtractor.extract) next to the CPU restatement
(preprocess.py's float64 functions on the same arrays, one utterance per task on a pool of processes) and next to the decode rate
the README quotes: what share of a wav-to-text batch the front end is.

    python tools/bench_frontend.py [--out profiles/frontend_bench.json] [--utterances 64] [--frames 1274] [--reps 20] [--cpu-procs 16]

    python tools/bench_frontend.py --speed 0.9 --rate 44100 --out profiles/resample_bench.json

With --rate / --speed the recordings are generated at that source rate (speed s: at 16000 * s Hz) and extract() resamples them on the
device first: per case the las_resample launch is timed with device events next to las_frontend's three on the same batch, and the
whole extract() with a host clock.  No CPU comparison in that mode.

Per configuration (mfcc-13, fbank-40; float32 input): a warm-up, then `--reps` rounds that alternate the configurations; one round times
one extract() of the whole batch between device synchronisations with a host clock (upload + three launches: what a caller waits for)
and, around the launches alone, with device events on samples already resident (the kernels' share).  Medians and the spread are kept."""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "automatic-speech-recognition_amd")
sys.path.insert(0, PKG)

DECODE_RATE = (2400.0, 2880.0)            # README: beam-16 + LM decode, utterances/s (one batch at a time .. a stream of batches)


def fe_args(ft, fd):
    return SimpleNamespace(sample_rate=16000, frame_length=25, frame_step=10, feat_type=ft, feat_dim=fd, cmvn=True)


def _cpu_one(job):
    import preprocess as pp
    w, ft, fd = job
    if ft == "mfcc":
        f = pp.mfcc(w.astype(float), 16000, frame_length=0.025, frame_stride=0.01, num_cepstral=fd)
    else:
        f, _ = pp.mfe(w.astype(float), 16000, frame_length=0.025, frame_stride=0.01, num_filters=fd)
    return pp.extract_derivative_feature(pp.cmvn(f, True)).astype(np.float32).shape[0]


def med(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def timed_entry(name):
    """replace _hip.lib().<name> by a wrapper that brackets every call with device events; -> (events list, restore())"""
    import torch
    from las import _hip
    orig = getattr(_hip.lib(), name)
    ev = []

    def timed(*a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = orig(*a)
        e1.record()
        ev.append((e0, e1))
        return rc
    setattr(_hip._lib, name, timed)
    return ev, lambda: setattr(_hip._lib, name, orig)


def bench_resample(o):
    """extract(rate=eff) per effective source rate: the las_resample launch next to las_frontend's launches, device events"""
    import torch
    from las.frontend import FeatureExtractor
    n = o.utterances
    ns = 400 + 160 * o.frames
    cases = [("speed_%s" % s, int(round(16000 * s))) for s in o.speed] + [("rate_%d" % r, r) for r in o.rate]
    fe = FeatureExtractor(fe_args("mfcc", 13))
    res = {"utterances": n, "frames": o.frames, "samples_out": ns, "device": torch.cuda.get_device_name(0), "feat": "mfcc-13", "cases": {}}
    rng = np.random.RandomState(0)
    for name, eff in cases:
        r = fe.resampler(eff)
        n_src = ns * r.M // r.L
        while r.out_len(n_src) < ns:
            n_src += 1
        waves = [(0.1 * rng.randn(n_src)).astype(np.float32) for _ in range(n)]
        for _ in range(3):
            _, lens = fe.extract(waves, rate=eff)
        torch.cuda.synchronize()
        wall = []
        for _ in range(o.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fe.extract(waves, rate=eff)
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
        ev_r, undo_r = timed_entry("las_resample")
        ev_f, undo_f = timed_entry("las_frontend")
        try:
            for _ in range(o.reps):
                fe.extract(waves, rate=eff)
        finally:
            undo_r()
            undo_f()
        torch.cuda.synchronize()
        t_r = med([a.elapsed_time(b) * 1e-3 for a, b in ev_r])
        t_f = med([a.elapsed_time(b) * 1e-3 for a, b in ev_f])
        res["cases"][name] = {
            "fs_in": eff, "fs_out": 16000, "L": r.L, "M": r.M, "K": r.K, "tile": r.tile(), "table_bytes": int(r.table.nbytes),
            "samples_in": n_src, "frames": int(lens[0]), "resample_s": t_r, "frontend_s": t_f, "extract_s": med(wall),
            "resample_over_frontend": t_r["median"] / t_f["median"],
            "resample_gb_per_s": n * (n_src + r.out_len(n_src)) * 4 / t_r["median"] * 1e-9,
            "resample_gflop_per_s": 2.0 * n * r.out_len(n_src) * r.K / t_r["median"] * 1e-9}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rate", type=int, nargs="*", default=[], help="source sample rates to resample from (to 16 kHz) on the device")
    ap.add_argument("--speed", type=float, nargs="*", default=[], help="speed factors: recordings taken to be at 16000 * s Hz")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontend_bench.json"))
    ap.add_argument("--utterances", type=int, default=64)
    ap.add_argument("--frames", type=int, default=1274)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-procs", type=int, default=16)
    ap.add_argument("--cpu-reps", type=int, default=3)
    o = ap.parse_args()
    import torch
    from las.frontend import FeatureExtractor
    if not torch.cuda.is_available():
        raise SystemExit("bench_frontend.py measures on an MI355X: no device found")
    if o.rate or o.speed:
        res = bench_resample(o)
        print(json.dumps(res))
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
        return
    n = o.utterances
    ns = 400 + 160 * o.frames                                   # T = floor((ns - 400) / 160) = --frames (1274: 12.7 s of audio)
    rng = np.random.RandomState(0)
    waves = [(0.1 * rng.randn(ns)).astype(np.float32) for _ in range(n)]
    cfgs = [("mfcc", 13), ("fbank", 40)]
    fes = {c: FeatureExtractor(fe_args(*c)) for c in cfgs}
    frames = int(fes[cfgs[0]].frame_counts([ns])[0])
    for c in cfgs:                                              # warm-up: code objects, pinned staging buffers, scratch
        for _ in range(3):
            fes[c].extract(waves)
    torch.cuda.synchronize()
    wall = {c: [] for c in cfgs}
    for _ in range(o.reps):                                     # alternating rounds
        for c in cfgs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fes[c].extract(waves)
            torch.cuda.synchronize()
            wall[c].append(time.perf_counter() - t0)
    # the kernels alone: the same launches on samples that are already on the device
    from las import _hip
    kern = {c: [] for c in cfgs}
    calls = {}
    orig = _hip.lib().las_frontend
    for c in cfgs:
        ev = []

        def timed(a, st, ev=ev):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = orig(a, st)
            e1.record()
            ev.append((e0, e1))
            return rc
        calls[c] = (timed, ev)
    for _ in range(o.reps):
        for c in cfgs:
            timed, ev = calls[c]
            _hip._lib.las_frontend = timed
            try:
                fes[c].extract(waves)
            finally:
                _hip._lib.las_frontend = orig
    torch.cuda.synchronize()
    for c in cfgs:
        kern[c] = [a.elapsed_time(b) * 1e-3 for a, b in calls[c][1]]
    # the CPU restatement on the same arrays
    import multiprocessing as mp
    cpu = {c: [] for c in cfgs}
    with mp.get_context("spawn").Pool(o.cpu_procs) as pool:
        pool.map(_cpu_one, [(waves[0], "mfcc", 13)] * o.cpu_procs)       # start the workers
        for _ in range(o.cpu_reps):
            for c in cfgs:
                t0 = time.perf_counter()
                got = pool.map(_cpu_one, [(w, c[0], c[1]) for w in waves], chunksize=max(1, n // o.cpu_procs))
                cpu[c].append(time.perf_counter() - t0)
                assert all(g == frames for g in got)
    res = {"utterances": n, "samples": ns, "frames": frames, "device": torch.cuda.get_device_name(0), "cpu_procs": o.cpu_procs,
           "decode_utt_per_s_readme": list(DECODE_RATE), "configs": {}}
    for c in cfgs:
        w, k, p = med(wall[c]), med(kern[c]), med(cpu[c])
        res["configs"]["%s-%d" % c] = {
            "extract_s": w, "kernels_s": k, "cpu_s": p,
            "extract_utt_per_s": n / w["median"], "kernels_utt_per_s": n / k["median"], "cpu_utt_per_s": n / p["median"],
            "speedup_over_cpu": p["median"] / w["median"],
            "share_of_wav_to_text_batch": [w["median"] / (w["median"] + n / r) for r in DECODE_RATE]}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
    with open(o.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
