"""bench_augment.py -- the reverberation and noise launches (las.augment.WaveAugmenter, csrc/wave_aug.hip) alone, next to las_frontend's
launches on the same batch and next to the float64 statement on the host (preprocess.reverberate + mix_noise, one utterance at a time).

    python tools/bench_augment.py [--out profiles/augment_bench.json] [--utterances 64] [--seconds 10] [--rir-seconds 0.5] [--reps 5]

Workload: 64 utterances of 10 s at 16 kHz against room responses of 0.5 s (8,000 taps), every utterance reverberated and mixed with
noise.  After a warm-up, `--reps` calls of extract(waves, augment=plan): las_reverb, las_noise_mix and las_frontend are each bracketed
with device events (medians and spread kept), the whole call is timed with a host clock between device synchronisations.  The FIR's
useful work is 2 n N K flops (K taps for each of the n N outputs); its share of the fp32 vector peak is that over the median time over
157.3 TFLOP/s."""
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

FP32_VECTOR_PEAK = 157.3e12               # MI355X, flop/s


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_bench.json"))
    ap.add_argument("--utterances", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rir-seconds", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-utterances", type=int, default=2, help="utterances the host statement is timed on (it takes seconds each)")
    o = ap.parse_args()
    import torch
    import preprocess as pp
    from las import _hip
    from las.augment import WaveAugmenter
    from las.frontend import FeatureExtractor
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment.py measures on an MI355X: no device found")
    fs, n = 16000, o.utterances
    N, K = int(round(fs * o.seconds)), int(round(fs * o.rir_seconds))
    rng = np.random.RandomState(0)
    waves = [(0.1 * rng.randn(N)).astype(np.float32) for _ in range(n)]
    rirs = [pp.synthetic_rir(fs, o.rir_seconds, s, length_s=o.rir_seconds) for s in range(4)]
    noises = [0.3 * rng.randn(5 * fs) for _ in range(2)]
    aug = WaveAugmenter(fs, rirs=rirs, noises=noises, reverb_prob=1.0, noise_prob=1.0, seed=1)
    plan = aug.plan(n, 0)
    fe = FeatureExtractor(SimpleNamespace(sample_rate=fs, frame_length=25, frame_step=10, feat_type="mfcc", feat_dim=13, cmvn=True))
    for _ in range(3):                                          # warm-up: code objects, banks, pinned staging buffers, scratch
        _, lens = fe.extract(waves, augment=plan)
    torch.cuda.synchronize()
    wall = []
    for _ in range(o.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fe.extract(waves, augment=plan)
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
    names = ("las_reverb", "las_noise_mix", "las_frontend", "las_resample")
    timers = {k: timed_entry(k) for k in names}
    try:
        for _ in range(o.reps):
            fe.extract(waves, augment=plan)
    finally:
        for k in names:
            timers[k][1]()
    torch.cuda.synchronize()
    t = {k: med([a.elapsed_time(b) * 1e-3 for a, b in timers[k][0]]) for k in names}
    cpu_r, cpu_m = [], []
    for u in range(min(o.cpu_utterances, n)):
        x = waves[u].astype(float)
        t0 = time.perf_counter()
        y = pp.reverberate(x, aug.rirs[plan.rir_idx[u]], aug.rir_delay[plan.rir_idx[u]])
        t1 = time.perf_counter()
        pp.mix_noise(y, aug.noises[plan.noise_idx[u]], int(plan.noise_off[u]), float(plan.snr_db[u]))
        t2 = time.perf_counter()
        cpu_r.append(t1 - t0)
        cpu_m.append(t2 - t1)
    flops = 2.0 * n * N * K
    lib = _hip.lib()
    res = {"utterances": n, "samples": N, "taps": K, "frames": int(lens[0]), "device": torch.cuda.get_device_name(0), "feat": "mfcc-13",
           "reverb_tile": lib.las_reverb_tile(), "reverb_tap_chunk": lib.las_reverb_tap_chunk(), "noise_tile": lib.las_noise_mix_tile(),
           "reverb_s": t["las_reverb"], "noise_mix_s": t["las_noise_mix"], "frontend_s": t["las_frontend"], "copy_to_fp32_s": t["las_resample"],
           "extract_with_plan_s": med(wall),
           "reverb_flops": flops, "reverb_tflop_per_s": flops / t["las_reverb"]["median"] * 1e-12,
           "reverb_share_of_fp32_vector_peak": flops / t["las_reverb"]["median"] / FP32_VECTOR_PEAK,
           "noise_mix_gb_per_s": n * N * 4 * 4 / t["las_noise_mix"]["median"] * 1e-9,       # two reads of the samples, the noise, one write
           "reverb_over_frontend": t["las_reverb"]["median"] / t["las_frontend"]["median"],
           "cpu_reverberate_s_per_utterance": med(cpu_r), "cpu_mix_noise_s_per_utterance": med(cpu_m),
           "cpu_s_per_batch_one_process": n * (statistics.median(cpu_r) + statistics.median(cpu_m))}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
    with open(o.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
