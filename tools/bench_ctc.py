#!/usr/bin/env python
"""Cost of joint CTC-attention training at the reference's run.sh recipe (bench.py's run_sh leg: B = 48, T = 1274, CNN listener, subword
units, bf16): ms per train step with --ctc off and on, both cells, through bench.py's side_step_bench protocol (synthetic batch resident
in HBM, warm-up, timed steps between synchronisations).  Writes profiles/ctc_bench.json.

  python tools/bench_ctc.py [--steps 5 --warmup 2 --cells rnn,lstm]
  python tools/bench_ctc.py --rocprof      # rnn runs with ctc on and off, each in a child under `rocprofv3 --kernel-trace --stats`: the
                                           # CTC kernels' ms per step and what the other kernels gained -> profiles/ctc_kernel_stats.csv,
                                           # profiles/ctc_kernel_share.json (+ the head's three products and its colsum, timed one by one)
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "automatic-speech-recognition_amd")]
PROF = os.path.join(ROOT, "profiles")
CTC_KERNELS = ("ctc_labels_kernel", "ctc_gather_kernel", "ctc_alpha_beta_kernel", "ctc_grad_kernel", "ctc_sum_kernel")


def run(cells, steps, warmup, ctc_modes, B=48, T=1274):
    import torch
    import bench
    base = bench.bench_args
    out = {}
    for ctc in ctc_modes:
        def args_with_ctc(cell, config=1, ctc=ctc):
            a = base(cell, config)
            a.ctc, a.ctc_weight = ctc, 0.2
            return a
        bench.bench_args = args_with_ctc
        try:
            for cell in cells:
                r = bench.side_step_bench(torch.device("cuda"), cell, "bf16", "run_sh", B, T, steps=steps, warmup=warmup)
                out["%s_ctc_%s" % (cell, "on" if ctc else "off")] = r["ms_per_step"]
                print(json.dumps({"cell": cell, "ctc": ctc, "ms_per_step": r["ms_per_step"], "dec_steps": r["dec_steps"]}), flush=True)
        finally:
            bench.bench_args = base
    for cell in cells:
        if "%s_ctc_on" % cell in out and "%s_ctc_off" % cell in out:
            out["%s_added_ms" % cell] = round(out["%s_ctc_on" % cell] - out["%s_ctc_off" % cell], 3)
    return out


def _trace(ctc, steps, warmup, d):
    """kernel name -> ns per step, from a child run under rocprofv3 --kernel-trace --stats (rnn cell, warm-up steps included)"""
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "ctc", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--cells", "rnn", "--ctc-mode", "on" if ctc else "off", "--steps", str(steps),
           "--warmup", str(warmup), "--no-write"]
    subprocess.check_call(cmd)
    stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)[0]
    rows = list(csv.DictReader(open(stats)))
    # per step over the TIMED steps only: the launches after the warm-up steps' last optimiser kernel (the first steps also hold
    # one-time work: library kernels tuned on first use)
    tr = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    trace = list(csv.DictReader(open(tr[0])))
    if not tr or "Kernel_Name" not in trace[0]:
        raise RuntimeError("rocprofv3 wrote no kernel trace with Kernel_Name / Start_Timestamp / End_Timestamp columns in %s" % d)
    trace.sort(key=lambda r: int(r["Start_Timestamp"]))
    ends = [i for i, r in enumerate(trace) if "clip_adam" in r["Kernel_Name"]]
    per = {}
    for r in trace[ends[warmup - 1] + 1:ends[-1] + 1]:
        per[r["Kernel_Name"]] = per.get(r["Kernel_Name"], 0.0) + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / steps
    return rows, per


def rocprof(steps, warmup, out_dir):
    """ctc on and off, each traced: the CTC kernels' ms per step, and what else the step gained (the head's products and colsum run
    through kernels the step already uses: their share is the difference of the two traces, kernel by kernel)"""
    with tempfile.TemporaryDirectory() as d_on, tempfile.TemporaryDirectory() as d_off:
        rows, on = _trace(True, steps, warmup, d_on)
        _, off = _trace(False, steps, warmup, d_off)
    with open(os.path.join(out_dir, "ctc_kernel_stats.csv"), "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0]))
        w.writeheader()
        w.writerows(rows)
    ms = lambda ns: round(ns / 1e6, 4)
    ctc = {k: v for k, v in on.items() if any(c in k for c in CTC_KERNELS)}
    diff = {k: on.get(k, 0.0) - off.get(k, 0.0) for k in set(on) | set(off) if k not in ctc}
    grown = {k[:120]: ms(v) for k, v in sorted(diff.items(), key=lambda kv: -kv[1]) if v > 2e4}
    share = {"steps_timed": steps, "cell": "rnn",
             "kernel_ms_per_step_ctc_off": ms(sum(off.values())), "kernel_ms_per_step_ctc_on": ms(sum(on.values())),
             "ctc_kernels_ms_per_step": ms(sum(ctc.values())),
             "ctc_kernels": {k[:120]: ms(v) for k, v in sorted(ctc.items(), key=lambda kv: -kv[1])},
             "other_kernels_grown_ms_per_step": grown}
    json.dump(share, open(os.path.join(out_dir, "ctc_kernel_share.json"), "w"), indent=1)
    print(json.dumps(share))


def products(reps=10, B=48, Tp=319, Hd=512, Vc=5001):
    """the head's three products (bf16 mode, run.sh sizes) one by one, ms each (event timing over `reps` launches)"""
    import torch
    from las import _hip
    dev = torch.device("cuda")
    enc, W = torch.randn(B * Tp, Hd, device=dev), torch.randn(Hd, Vc, device=dev) * 0.05
    b, d = torch.zeros(Vc, device=dev), torch.randn(B * Tp, Vc, device=dev) * 1e-3
    out, d_enc, dW, db = torch.empty(B * Tp, Vc, device=dev), torch.empty(B * Tp, Hd, device=dev), torch.zeros(Hd, Vc, device=dev), torch.zeros(Vc, device=dev)
    P = _hip.PREC_BF16
    M = B * Tp
    runs = {"forward enc.W+b": lambda: _hip.gemm(P, enc, W, out, False, False, M, Vc, Hd, Hd, Vc, Vc, bias=b),
            "d_enc = d.W^T": lambda: _hip.gemm(P, d, W, d_enc, False, True, M, Hd, Vc, Vc, Vc, Hd),
            "dW += enc^T.d": lambda: _hip.gemm(P, enc, d, dW, True, False, Hd, Vc, M, Hd, Vc, Vc, beta=1.0),
            "db += colsum(d)": lambda: _hip.colsum(d, M, Vc, Vc, db, beta=1.0)}
    res = {}
    for k, f in runs.items():
        f()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            f()
        e1.record()
        torch.cuda.synchronize()
        res[k] = round(e0.elapsed_time(e1) / reps, 4)
    print(json.dumps({"head_products_ms": res}))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cells", default="rnn,lstm")
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--ctc-mode", default="both", choices=["both", "on", "off"], help=argparse.SUPPRESS)
    ap.add_argument("--out", default=PROF, help="directory of the written files (default profiles/)")
    ap.add_argument("--no-write", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.rocprof:
        rocprof(a.steps, a.warmup, a.out)
        res = products()
        share = json.load(open(os.path.join(a.out, "ctc_kernel_share.json")))
        share["head_products_ms_each_bf16"] = res
        json.dump(share, open(os.path.join(a.out, "ctc_kernel_share.json"), "w"), indent=1)
        return
    res = run(a.cells.split(","), a.steps, a.warmup, {"both": (False, True), "on": (True,), "off": (False,)}[a.ctc_mode])
    print(json.dumps(res))
    if not a.no_write:
        json.dump(res, open(os.path.join(a.out, "ctc_bench.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
