"""bench_specaug.py -- what SpecAugment costs on the device: the las_specaug launch alone next to a device-to-device copy of the same
cube, and a train step with --spec_augment on and off.

    python tools/bench_specaug.py [--out profiles/specaug_bench.json] [--rows 48] [--frames 1274] [--reps 20] [--step-rows 48] [--step-frames 1274]

Launch: B = --rows utterances of --frames frames (ragged lengths between half and all of it), F x C = 13 x 3 and 40 x 3, the plan of the
default policy (W = 80, two frequency masks up to feat_dim // 3, two time masks up to 100 frames), uploaded before the clock starts;
the launch and, alternating with it, `copy_` of the same cube into the same buffer are bracketed by device events, all of them enqueued
behind a 4 ms spin so that the device, not the host's issue rate, is what the events see.  Medians of --reps.
Step: LAS.train on bench.py's flagship configuration (pblstm 3 x 256 LSTM, bf16, synthetic batch), ONE model with the flag switched
off and on in alternating rounds; a round is --block steps timed by a host clock between device synchronisations.  Medians of --reps.
Every figure is a median over alternating rounds in one process, so the two sides of a ratio saw the same device state."""
import argparse
import ctypes
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


def bench_launch(o):
    import torch
    from helpers import make_args
    from las import _hip
    from las.specaug import SpecAugment
    res = {}
    rng = np.random.RandomState(0)
    lens = rng.randint(o.frames // 2, o.frames + 1, size=o.rows).astype(np.int32)
    lens[0] = o.frames
    for F, C in ((13, 3), (40, 3)):
        sa = SpecAugment(make_args(feat_dim=F, spec_augment=True))
        x = torch.randn(o.rows, o.frames, F, C, device="cuda")
        out = torch.empty_like(x)
        plan = sa.plan(lens, 0)
        dplan = torch.from_numpy(plan).cuda()
        a = _hip.SpecAugArgs(in_=x.data_ptr(), out=out.data_ptr(), plan=dplan.data_ptr(), plan_host=plan.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                             ldp=plan.shape[1], B=o.rows, Tmax=o.frames, F=F, C=C, mF=sa.mF, mT=sa.mT)
        launch = lambda: _hip.check(_hip.lib().las_specaug(ctypes.byref(a), _hip.stream()), "las_specaug")
        copy = lambda: out.copy_(x)
        for _ in range(3):
            launch()
            copy()
        torch.cuda.synchronize()
        ev = {"specaug": [], "copy": []}
        # The device first spins for about 4 ms while the host enqueues everything: the timed kernels then run back to back.  (Enqueued
        # into an idle queue, a 10 us kernel is measured with the host's time to issue it -- a ctypes call that validates 48 plan rows --
        # between the two events.)
        torch.cuda._sleep(10000000)
        for _ in range(o.reps):
            for name, fn in (("specaug", launch), ("copy", copy)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                ev[name].append((e0, e1))
        torch.cuda.synchronize()
        t = {k: med([p.elapsed_time(q) * 1e-3 for p, q in v]) for k, v in ev.items()}
        nbytes = x.numel() * 4
        res["%dx%d" % (F, C)] = {
            "rows": o.rows, "frames": o.frames, "F": F, "C": C, "bytes": nbytes, "tile": int(_hip.lib().las_specaug_tile()),
            "warped_rows": int((plan[:, 2] != 0).sum()), "specaug_s": t["specaug"], "copy_s": t["copy"],
            "specaug_over_copy": t["specaug"]["median"] / t["copy"]["median"],
            "specaug_gb_per_s": 2 * nbytes / t["specaug"]["median"] * 1e-9, "copy_gb_per_s": 2 * nbytes / t["copy"]["median"] * 1e-9}
    return res


def bench_step(o):
    import torch
    sys.path.insert(0, ROOT)
    from bench import bench_args
    from helpers import synthetic_batch
    from las import layers as L, variables as V
    from las.las import LAS, Listener, Speller
    L.set_cell("lstm")
    L.set_precision("bf16")
    V.reset_default_store(device="cuda", seed=0)
    args = bench_args("lstm")                                          # bench.py's flagship configuration
    las = LAS(args, Listener, Speller, {})
    las.build_variables()
    xs, ys = synthetic_batch(o.step_rows, o.step_frames, 256, args.vocab_size, seed=0, min_frac=0.834)
    xs = (torch.tensor(xs[0], device="cuda"), xs[1])
    ys = (torch.tensor(ys[0], device="cuda"), ys[1])
    times = {False: [], True: []}
    for it in range(o.reps + 2):                                       # ONE model; the flag is read at every step.  Two warm-up rounds
        for flag in (False, True):
            args.spec_augment = flag
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(o.block):
                las.train(xs, ys)
            torch.cuda.synchronize()
            if it >= 2:
                times[flag].append((time.perf_counter() - t0) / o.block)
    las.check_status()
    off, on = med(times[False]), med(times[True])
    return {"rows": o.step_rows, "frames": o.step_frames, "steps_per_sample": o.block, "config": "bench.py config 1 (pblstm 3 x 256 lstm, bf16, 13 x 3)",
            "recovered_steps": las.recovered_steps, "step_off_s": off, "step_on_s": on, "on_minus_off_s": on["median"] - off["median"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "specaug_bench.json"))
    ap.add_argument("--rows", type=int, default=48)
    ap.add_argument("--frames", type=int, default=1274)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-rows", type=int, default=48)
    ap.add_argument("--step-frames", type=int, default=1274)
    ap.add_argument("--block", type=int, default=4, help="train steps per timed sample")
    ap.add_argument("--no-step", action="store_true", help="the launch and the copy only")
    o = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_specaug.py measures on an MI355X: no device found")
    res = {"device": torch.cuda.get_device_name(0), "launch": bench_launch(o)}
    if not o.no_step:
        res["train_step"] = bench_step(o)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
    with open(o.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
