#!/usr/bin/env python
"""Cost of keyword search at the recipe's decode sizes -- n = 64 utterances, T' = 319 encoder frames, Vc = 5001 classes --
for P = 16 and P = 1024 phrases of mixed lengths (1 to 32 tokens), on random log-probabilities.  Per P, by HIP events around the calls:
  call_us             las_kws_search (frame maxima + search), thr = -1.0 nat per token, H = 4, no series
  call_all_cand_us    the same with thr = -inf: every reachable frame is a candidate, the hit bookkeeping at its busiest
  call_series_us      thr = -1.0 per token with the end series stored ([n, P, T'] fp64 + int32; P = 16 only)
  api_ms              host clock around las.kws.keyword_search (upload, call, read-back), device synchronised at both ends
and once: log_softmax_us, las_ctc_log_softmax on the same batch (the launch every reader of the head pays already), for comparison.
Writes profiles/kws_bench.json.

  python tools/bench_kws.py [--reps 20]
  python tools/bench_kws.py --rocprof      # per P, the calls in a child of its own under `rocprofv3 --kernel-trace --stats`: the time of
                                           # each of the two kernels -> "kernels_us" of the same file, and the search's time per frame
"""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "automatic-speech-recognition_amd")]
PROF = os.path.join(ROOT, "profiles")
N, TP, VC = 64, 319, 5001
PS = (16, 1024)
LENGTHS = (1, 2, 3, 5, 8, 12, 17, 24, 32)


def _phrases(P, seed=7):
    import numpy as np
    rng = np.random.RandomState(seed)
    return [[int(c) for c in rng.randint(3, VC - 1, size=LENGTHS[k % len(LENGTHS)])] for k in range(P)]


def _batch():
    """-> logits [n, T', Vc] and class-major log-probabilities [n, Vc, T'] of them (las_ctc_log_softmax)"""
    import torch
    from las import _hip
    rng = torch.Generator(device="cuda").manual_seed(1)
    z = torch.randn(N, TP, VC, device="cuda", generator=rng)
    lp = torch.empty(N, VC, TP, device="cuda")
    _hip.check(_hip.lib().las_ctc_log_softmax(_hip.p(z), N, TP, VC, _hip.p(lp), _hip.stream()), "las_ctc_log_softmax")
    torch.cuda.synchronize()
    return z, lp


def _events(call, reps):
    import torch
    call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / reps * 1e3, 2)


def _caller(lp, phrases, per_token, H=4, series=False):
    """the C call alone on device-resident arguments -> (call, count tensor)"""
    import numpy as np
    import torch
    from las import _hip
    n, Vc, Tp = lp.shape
    P, U = len(phrases), max(len(ph) for ph in phrases)
    i32 = dict(dtype=torch.int32, device=lp.device)
    y = np.zeros((P, U), np.int32)
    for k, ph in enumerate(phrases):
        y[k, :len(ph)] = ph
    y, yl, el = torch.tensor(y, **i32), torch.tensor([len(ph) for ph in phrases], **i32), torch.full((n,), Tp, **i32)
    thr = torch.tensor(np.asarray([np.float32(per_token) * np.float32(len(ph)) for ph in phrases], np.float32), device=lp.device)
    hs, he, cnt, bsp = torch.empty(n, P, H, **i32), torch.empty(n, P, H, **i32), torch.empty(n, P, 2, **i32), torch.empty(n, P, 2, **i32)
    hsc, bsc = torch.empty(n, P, H, dtype=torch.float64, device=lp.device), torch.empty(n, P, dtype=torch.float64, device=lp.device)
    es = torch.empty(n, P, Tp, dtype=torch.float64, device=lp.device) if series else None
    et = torch.empty(n, P, Tp, **i32) if series else None
    lib = _hip.lib()
    ws = _hip.workspace(lp.device, lib.las_kws_workspace_bytes(n, Tp), "kws")

    def call():
        _hip.check(lib.las_kws_search(_hip.p(lp), Vc, Tp, _hip.p(el), n, _hip.p(y), U, _hip.p(yl), _hip.p(thr), P, U, H, _hip.p(hs), _hip.p(he),
                                      _hip.p(hsc), _hip.p(cnt), _hip.p(bsc), _hip.p(bsp), _hip.p(es), _hip.p(et), _hip.p(ws), ws.numel(),
                                      _hip.stream()), "las_kws_search")
    return call, cnt


def run(reps):
    import torch
    from las import _hip
    from las import kws as KW
    z, lp = _batch()
    out = {"n": N, "Tp": TP, "Vc": VC, "lengths": list(LENGTHS), "reps": reps, "P": {}}
    lp2 = torch.empty_like(lp)
    out["log_softmax_us"] = _events(lambda: _hip.check(_hip.lib().las_ctc_log_softmax(_hip.p(z), N, TP, VC, _hip.p(lp2), _hip.stream()),
                                                       "las_ctc_log_softmax"), reps)
    del lp2
    for P in PS:
        phrases = _phrases(P)
        r = {}
        call, cnt = _caller(lp, phrases, -1.0)
        r["call_us"] = _events(call, reps)
        r["hits_closed"] = int(cnt[:, :, 1].sum())
        call, cnt = _caller(lp, phrases, float("-inf"))
        r["call_all_cand_us"] = _events(call, reps)
        r["hits_closed_all_cand"] = int(cnt[:, :, 1].sum())
        if P == 16:
            call, _ = _caller(lp, phrases, -1.0, series=True)
            r["call_series_us"] = _events(call, reps)
        kw = KW.KeywordList(phrases)
        KW.keyword_search(lp, [TP] * N, kw, -1.0)
        api = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            KW.keyword_search(lp, [TP] * N, kw, -1.0)
            torch.cuda.synchronize()
            api.append(round((time.perf_counter() - t0) * 1e3, 3))
        r["api_ms"] = sorted(api)[len(api) // 2]
        out["P"][str(P)] = r
    return out


def child(P):
    """what the profiler watches: las_kws_search calls at one P"""
    _, lp = _batch()
    call, _ = _caller(lp, _phrases(P), -1.0)
    print("call_us", _events(call, 20))


def rocprof():
    res = {}
    for P in PS:
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "kws", "--", sys.executable,
                   os.path.abspath(__file__), "--child", str(P)]
            subprocess.run(cmd, check=True, timeout=600)
            stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            rows = list(csv.DictReader(open(stats[0])))
        k = {re.search(r"kws_\w+_kernel", r["Name"]).group(0): round(float(r["AverageNs"]) * 1e-3, 2) for r in rows if "kws_" in r["Name"]}
        k["search_ns_per_frame"] = round(k["kws_search_kernel"] * 1e3 / TP, 1)
        res[str(P)] = k
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--child", type=int, default=0, metavar="P")
    ap.add_argument("--out", default=PROF, help="directory of kws_bench.json")
    a = ap.parse_args()
    if a.child:
        child(a.child)
        sys.exit(0)
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "kws_bench.json")
    res = json.load(open(path)) if a.rocprof and os.path.exists(path) else {}
    if a.rocprof:
        res["kernels_us"] = rocprof()
    else:
        res = run(a.reps)
    print(json.dumps(res), flush=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
