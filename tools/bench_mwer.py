#!/usr/bin/env python
"""MWER training beside what it replaces.  One process, after warm-up, alternating per repetition:
  kernels   HIP events around las_mwer_loss (its three launches) and around las_ce_loss (its two) on the same logits: n K = 192 rows
            (n = 48 utterances, K = 4 slots, all present, full length), U = 100 steps, V in {30, 5000} and 1025 / 5121 (one class
            past a register instantiation's capacity), the Speller's time-major layout.  las_ce_loss reads the logits once and
            writes once; las_mwer_loss reads them twice and writes once: bytes moved over time are given for both beside the
            6.3 TB/s a streaming kernel can reach on the MI355X.
  steps     host clock, device synchronised at both ends, around LAS.train on one batch of B = 48 utterances (400 frames, char
            vocabulary, speed mode, lstm cells, 256 units) without --mwer and with --mwer True --mwer_hyps 4 --mwer_unit token / word
            (drawn hypotheses: 240 Speller rows, four more steps).
Medians of --reps (7) with the smallest and largest value beside them.  Writes profiles/mwer_bench.json.

  python tools/bench_mwer.py [--reps 7]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "automatic-speech-recognition_amd")]
PROF = os.path.join(ROOT, "profiles")
HBM_TBPS = 6.3


def _events(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return round(a.elapsed_time(b) * 1e3, 2)


def _stat(x):
    return {"median": sorted(x)[len(x) // 2], "min": min(x), "max": max(x)}


def kernels(reps, n=48, K=4, U=100):
    import torch
    from las import _hip
    lib, dev, out = _hip.lib(), torch.device("cuda", 0), {}
    R = n * K
    for V in (30, 1025, 5000, 5121):
        g = torch.Generator().manual_seed(V)
        tm = (torch.randn(U, R, V, generator=g) * 2).to(dev)                         # the Speller's time-major buffer
        logits = tm.permute(1, 0, 2)
        y = torch.randint(1, V, (R, U), generator=g, dtype=torch.int32).to(dev)
        lens = torch.full((R,), U, dtype=torch.int32, device=dev)
        nhyp = torch.full((n,), K, dtype=torch.int32, device=dev)
        err = torch.randint(0, 9, (R,), generator=g).float().to(dev)
        scale = torch.full((1,), 1.0 / n, device=dev)
        dl = torch.empty_strided(logits.shape, logits.stride(), device=dev)
        f = torch.empty(2 * R + n + 1, device=dev)
        seq = torch.empty(R, dtype=torch.float64, device=dev)
        nb = lib.las_mwer_workspace_bytes(n, K, U)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        sums = torch.empty(3, device=dev)
        nbc = lib.las_ce_loss_workspace_bytes(R, U)
        wsc = torch.empty(nbc, dtype=torch.uint8, device=dev)
        sb, st = logits.stride(0), logits.stride(1)

        def mwer(mode):
            _hip.check(lib.las_mwer_loss(_hip.p(logits), sb, st, V, _hip.p(y), U, _hip.p(lens), _hip.p(nhyp), _hip.p(err), n, K, U, mode,
                                         _hip.p(scale), _hip.p(seq), _hip.p(f[:R]), _hip.p(f[R:2 * R]), _hip.p(f[2 * R:2 * R + n]),
                                         _hip.p(f[2 * R + n:]), _hip.p(dl), _hip.p(ws), nb, _hip.stream()), "las_mwer_loss")

        def ce():
            _hip.check(lib.las_ce_loss(_hip.p(logits), sb, st, _hip.p(y), U, R, U, V, 0.01, 1 | 4, _hip.p(sums), _hip.p(scale), _hip.p(dl),
                                       _hip.p(wsc), nbc, _hip.stream()), "las_ce_loss")
        runs = {"mwer_nbest": lambda: mwer(0), "mwer_sample": lambda: mwer(1), "ce": ce, "copy": lambda: dl.copy_(logits)}
        for fn in runs.values():
            fn()
            fn()
        us = {k: [] for k in runs}
        for _ in range(reps):
            for k, fn in runs.items():
                us[k].append(_events(fn))
        nbytes = R * U * V * 4
        moved = {"mwer_nbest": 3 * nbytes, "mwer_sample": 3 * nbytes, "ce": 2 * nbytes, "copy": 2 * nbytes}
        out["V%d" % V] = {"rows": R, "U": U, "V": V, "logits_MB": round(nbytes / 1e6, 2),
                          "us": {k: _stat(v) for k, v in us.items()},
                          "TBps_moved": {k: round(moved[k] / (_stat(us[k])["median"] * 1e-6) / 1e12, 3) for k in runs},
                          "share_of_%.1f_TBps" % HBM_TBPS: {k: round(moved[k] / (_stat(us[k])["median"] * 1e-6) / 1e12 / HBM_TBPS, 3) for k in runs}}
    return out


def steps(reps, B=48, T=400):
    import torch
    from helpers import make_args, synthetic_batch
    from las import layers as L, variables as V
    from las.las import LAS, Listener, Speller
    from utils.tokenizer import CharEncoder
    xs, ys = synthetic_batch(B, T, 64, 30, seed=3)
    out = {"B": B, "frames": T, "steps": int(ys[1].max()), "ms": {}}
    forms = {"plain": dict(mwer=False), "mwer_token": dict(mwer=True, mwer_hyps=4, mwer_unit="token"),
             "mwer_word": dict(mwer=True, mwer_hyps=4, mwer_unit="word")}
    L.set_cell("lstm")
    L.set_precision("bf16")
    try:
        for name, over in forms.items():             # (one model at a time: the variable store is the process')
            a = make_args(enc_units=256, num_enc_layers=2, dec_units=256, num_dec_layers=1, embedding_size=128, attention_size=128, **over)
            V.reset_default_store(device="cuda", seed=1)
            las = LAS(a, Listener, Speller, CharEncoder().id_to_token)
            ms = []
            for i in range(3 + reps):                # three warm-up steps: variables, workspaces, code objects
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                las.train(xs, ys)
                torch.cuda.synchronize()
                if i >= 3:
                    ms.append(round((time.perf_counter() - t0) * 1e3, 3))
            las.check_status()
            out["ms"][name] = _stat(ms)
    finally:
        L.set_cell("rnn")
        L.set_precision("f32")
    out["mwer_over_plain"] = {k: round(out["ms"][k]["median"] / out["ms"]["plain"]["median"], 2) for k in out["ms"] if k != "plain"}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=PROF, help="directory of mwer_bench.json")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    res = {"kernels": kernels(a.reps), "steps": steps(a.reps)}
    print(json.dumps(res), flush=True)
    with open(os.path.join(a.out, "mwer_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
