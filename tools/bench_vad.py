"""bench_vad.py -- what voice-activity segmentation costs on the device: las_vad (six launches) on a generated one-hour, 16 kHz
recording next to a device-to-device copy of the same sample bytes.

    python tools/bench_vad.py [--out profiles/vad_bench.json] [--seconds 3600] [--rate 16000] [--reps 20]

The recording: bursts of 0.1 randn of 0.5-8 s between silences of 0.3-3 s with a floor 60 dB below them (the runs of a meeting), fp32
and int16, uploaded before the clock starts.  The las_vad call and, alternating with it, `copy_` of the sample buffer are bracketed
by device events, all of them enqueued behind a 4 ms spin so that the device, not the host's issue rate, is what the events see.
Medians of --reps.  The batch case puts the hour next to three recordings of 10-60 s in one call (a grid that is mostly padding)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "automatic-speech-recognition_amd")
sys.path.insert(0, PKG)


def med(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def recording(seconds, rate, seed):
    rng = np.random.RandomState(seed)
    n = int(seconds * rate)
    x = (1e-4 * rng.randn(n)).astype(np.float32)
    pos = 0
    while pos < n:
        pos += int(rng.uniform(0.3, 3.0) * rate)
        w = int(rng.uniform(0.5, 8.0) * rate)
        seg = x[pos:pos + w]
        seg += (0.1 * rng.randn(len(seg))).astype(np.float32)
        pos += w
    return x


def bench(o, waves, i16, fl, step, va):
    import torch
    from las import _hip
    from las.frontend import frame_count
    lib = _hip.lib()
    n, ns = len(waves), [len(w) for w in waves]
    ld = (max(ns) + 7) & ~7
    host = np.zeros((n, ld), np.int16 if i16 else np.float32)
    for u, w in enumerate(waves):
        host[u, :ns[u]] = np.clip(np.round(w * 32767), -32768, 32767).astype(np.int16) if i16 else w
    x = torch.from_numpy(host).cuda()
    y = torch.empty_like(x)
    d_ns = torch.tensor(ns, dtype=torch.int32, device="cuda")
    Tmax = max(frame_count(v, fl, step) for v in ns)
    max_runs = int(lib.las_vad_max_runs(Tmax, va.hang))
    runs = torch.empty((n, max_runs, 2), dtype=torch.int32, device="cuda")
    count = torch.empty(n, dtype=torch.int32, device="cuda")
    energy = torch.empty((n, Tmax), dtype=torch.float64, device="cuda")
    nbytes = int(lib.las_vad_workspace_bytes(n, Tmax))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    ns_host = (ctypes.c_int * n)(*ns)
    launch = lambda: _hip.check(lib.las_vad(_hip.p(x), int(i16), ld, _hip.p(d_ns), ns_host, n, Tmax, fl, step, va.ratio, va.floor(fl), va.hang,
                                            va.min_run, _hip.p(energy), None, _hip.p(runs), max_runs, _hip.p(count), _hip.p(ws), nbytes,
                                            _hip.stream()), "las_vad")
    copy = lambda: y.copy_(x)
    for _ in range(3):
        launch()
        copy()
    torch.cuda.synchronize()
    ev = {"vad": [], "copy": []}
    torch.cuda._sleep(10000000)
    for _ in range(o.reps):
        for name, fn in (("vad", launch), ("copy", copy)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            ev[name].append((e0, e1))
    torch.cuda.synchronize()
    t = {k: med([p.elapsed_time(q) * 1e-3 for p, q in v]) for k, v in ev.items()}
    sample_bytes = int(sum(ns)) * host.itemsize
    return {"recordings": n, "samples": int(sum(ns)), "padded_samples": n * ld, "frames_max": Tmax, "dtype": "int16" if i16 else "fp32",
            "fl": fl, "step": step, "hang": va.hang, "min_run": va.min_run, "tile": int(lib.las_vad_tile()), "runs": count.cpu().numpy().tolist()[:4],
            "sample_bytes": sample_bytes, "copied_bytes": x.numel() * host.itemsize, "vad_s": t["vad"], "copy_s": t["copy"],
            "vad_over_copy": t["vad"]["median"] / t["copy"]["median"],
            "vad_read_gb_per_s": sample_bytes / t["vad"]["median"] * 1e-9, "copy_gb_per_s": 2 * x.numel() * host.itemsize / t["copy"]["median"] * 1e-9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vad_bench.json"))
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--rate", type=int, default=16000)
    ap.add_argument("--reps", type=int, default=20)
    o = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_vad.py measures on an MI355X: no device found")
    from las import vad as V
    from las.arguments import parse_args
    va = V.VoiceActivity(parse_args([]), device="cuda")
    fl, step = va.geometry(o.rate)
    hour = recording(o.seconds, o.rate, 0)
    res = {"device": torch.cuda.get_device_name(0), "seconds": o.seconds, "rate": o.rate,
           "hour_fp32": bench(o, [hour], False, fl, step, va), "hour_int16": bench(o, [hour], True, fl, step, va)}
    rng = np.random.RandomState(1)
    res["hour_and_3_short_fp32"] = bench(o, [hour] + [recording(rng.uniform(10, 60), o.rate, 2 + k) for k in range(3)], False, fl, step, va)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
    with open(o.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
