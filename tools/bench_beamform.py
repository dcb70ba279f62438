"""bench_beamform.py -- what beamforming a microphone-array recording costs on the device: las_gcc_phat, las_tdoa_track and las_delay_sum
(csrc/beamform.hip) on a generated one-hour, 8-channel, 16 kHz recording, next to (a) a device-to-device copy of the samples
and (b) the float64 numpy restatement of the same three calls on the host (tests/beamform_ref.py), timed on the first --host_seconds of
the recording and scaled to its length (all three calls are linear in the length).

    python tools/bench_beamform.py [--out profiles/beamform_bench.json] [--seconds 3600] [--channels 8] [--reps 10] [--host_seconds 120]

The recording: four 'voices' (white noise through lfilter([1], [1, -a])) take turns of 2-20 s, each from its own set of integer delays
within +-40 samples, between pauses of 0-2 s; every channel adds independent white noise 10 dB below.  Each call is bracketed by device
events behind a 4 ms spin, as in bench_diarize.py; medians of --reps.  No target is fixed in advance: the file records what was measured."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "automatic-speech-recognition_amd")
sys.path.insert(0, PKG)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def med(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def recording(seconds, rate, C, seed):
    """-> x float32 [C, n]"""
    from scipy.signal import lfilter
    rng = np.random.RandomState(seed)
    n = int(seconds * rate)
    pad = 64
    colours = (0.9, 0.5, -0.6, 0.2)
    delays = rng.randint(-40, 41, size=(4, C))
    delays[:, 0] = 0
    voice = np.full(n, -1, np.int8)
    pos = 0
    while pos < n:
        w = int(rng.uniform(2.0, 20.0) * rate)
        voice[pos:pos + w] = rng.randint(4)
        pos += w + int(rng.uniform(0.0, 2.0) * rate)
    x = np.empty((C, n), np.float32)
    t = np.arange(n)
    src = []
    for a in colours:
        y = lfilter([1.0], [1.0, -a], rng.standard_normal(n + 2 * pad))
        src.append((0.05 * y / np.sqrt(np.mean(y * y))).astype(np.float32))
    for c in range(C):
        row = (0.05 * 10.0 ** -0.5) * rng.standard_normal(n).astype(np.float32)
        for v in range(4):
            on = np.flatnonzero(voice == v)
            row[on] += src[v][pad + on - delays[v, c]]
        x[c] = row
    return x


def timed(fns, reps):
    """{name: median ... of the device time of fn()} -- the calls alternate, each between two events behind a spin"""
    import torch
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in fns}
    for _ in range(reps):
        torch.cuda._sleep(10000000)
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            ev[name].append((e0, e1))
    torch.cuda.synchronize()
    return {k: med([p.elapsed_time(q) * 1e-3 for p, q in v]) for k, v in ev.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beamform_bench.json"))
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--rate", type=int, default=16000)
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host_seconds", type=float, default=120.0, help="length of the prefix the numpy restatement is timed on (0: skip it)")
    o = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_beamform.py measures on an MI355X: no device found")
    from las import _hip, beamform as BF
    lib = _hip.lib()
    D0 = BF.DEFAULTS
    L, D, NF = BF.geometry(D0["bf_window_ms"], D0["bf_max_delay_ms"], o.rate)
    gamma, ref, C = D0["bf_jump_penalty"], D0["bf_ref"], o.channels
    xh = recording(o.seconds, o.rate, C, 0)
    n = xh.shape[1]
    Wn = int(lib.las_bf_windows(n, L))
    x = torch.from_numpy(xh).cuda()
    hann, tw = (torch.from_numpy(t).cuda() for t in BF.tables(L, NF))
    r = torch.empty((C, Wn, 2 * D + 1), dtype=torch.float32, device="cuda")
    tau = torch.empty((C, Wn), dtype=torch.int32, device="cuda")
    a = torch.empty((C, Wn), dtype=torch.float32, device="cuda")
    y = torch.empty(n, dtype=torch.float32, device="cuda")
    nbytes = int(lib.las_bf_workspace_bytes(C, Wn, NF, D))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    gcc = lambda: _hip.check(lib.las_gcc_phat(_hip.p(x), 0, n, C, n, ref, L, D, NF, _hip.p(hann), _hip.p(tw), _hip.p(r), _hip.p(ws), nbytes,
                                              _hip.stream()), "las_gcc_phat")
    track = lambda: _hip.check(lib.las_tdoa_track(_hip.p(r), C, Wn, D, ref, gamma, _hip.p(tau), _hip.p(a), _hip.p(ws), nbytes, _hip.stream()),
                               "las_tdoa_track")
    dsum = lambda: _hip.check(lib.las_delay_sum(_hip.p(x), 0, n, C, n, L, Wn, _hip.p(tau), _hip.p(a), _hip.p(y), _hip.stream()), "las_delay_sum")
    copy_to = torch.empty_like(x)
    t = timed({"gcc_phat": gcc, "tdoa_track": track, "delay_sum": dsum, "copy": lambda: copy_to.copy_(x)}, o.reps)
    t0 = time.perf_counter()
    y_host = y.cpu().numpy()
    readback = time.perf_counter() - t0
    tau_h = tau.cpu().numpy()
    transforms = 2 * C * Wn
    res = {"device": torch.cuda.get_device_name(0), "seconds": o.seconds, "rate": o.rate, "channels": C, "samples": n, "L": L, "D": D, "NF": NF,
           "windows": Wn, "gamma": gamma, "transforms": transforms, "sample_bytes": int(xh.nbytes), "r_bytes": int(r.numel() * 4),
           "workspace_bytes": nbytes, "gcc_phat_s": t["gcc_phat"], "tdoa_track_s": t["tdoa_track"], "delay_sum_s": t["delay_sum"], "copy_s": t["copy"],
           "gcc_us_per_transform": t["gcc_phat"]["median"] / transforms * 1e6,
           "delay_sum_over_copy": t["delay_sum"]["median"] / t["copy"]["median"],
           "track_over_gcc": t["tdoa_track"]["median"] / t["gcc_phat"]["median"],
           "readback_y_s": readback, "y_rms": float(np.sqrt(np.mean(y_host.astype(np.float64) ** 2))),
           "lag_changes": int((np.diff(tau_h, axis=1) != 0).sum())}
    if o.host_seconds > 0:
        import beamform_ref as R
        m = min(n, int(o.host_seconds * o.rate))
        xp = xh[:, :m]
        t0 = time.perf_counter()
        r_ref = R.gcc_phat(xp, ref, L, D, NF)
        t1 = time.perf_counter()
        tau_ref, a_ref = R.tdoa_track(r_ref.astype(np.float32), ref, gamma)
        t2 = time.perf_counter()
        R.delay_sum(xp, tau_ref, a_ref, L)
        t3 = time.perf_counter()
        Wp = r_ref.shape[1] - 2                                           # (the prefix's last windows see zeros where the recording goes on)
        scale = n / float(m)
        res.update(host_prefix_seconds=m / float(o.rate), host_gcc_phat_s=t1 - t0, host_tdoa_track_s=t2 - t1, host_delay_sum_s=t3 - t2,
                   host_scaled_to_recording_s={"gcc_phat": (t1 - t0) * scale, "tdoa_track": (t2 - t1) * scale, "delay_sum": (t3 - t2) * scale},
                   r_max_abs_err=float(np.abs(r[:, :Wp].cpu().numpy() - r_ref[:, :Wp]).max()) if Wp > 0 else None,
                   host_over_device={"gcc_phat": (t1 - t0) * scale / t["gcc_phat"]["median"],
                                     "tdoa_track": (t2 - t1) * scale / t["tdoa_track"]["median"],
                                     "delay_sum": (t3 - t2) * scale / t["delay_sum"]["median"]})
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
    with open(o.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
