#!/usr/bin/env python
"""Cost of joint CTC-attention beam search: device time per search step of decode_batch with --ctc_decode_weight 0 against
0.3, in alternating runs on one device (the protocol of tools/ab_bench.sh), at 256 and 1024 hypothesis rows (16 / 64 utterances x beam
16): a char model (V = 30) and the V = 5000 subword configuration, T = 1274 input frames -> T' = 160.  The step time is the search phase
of LAS_DECODE_TIMING (device synchronised at both ends) over the steps in which some utterance was still searching; each run records
that count and the per-part device times (parts_us, ctc = las_ctc_prefix_step with every row live).  Writes profiles/ctc_decode_bench.json.

  python tools/bench_ctc_decode.py [--reps 3]
  python tools/bench_ctc_decode.py --rocprof      # one char search at 256 rows with weight 0.3 in a child under `rocprofv3 --kernel-trace
                                                  # --stats`: the kernels' share -> profiles/ctc_decode_kernel_stats.csv
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
CONFIGS = {"char": dict(unit="char", vocab_size=30), "subword5000": dict(unit="subword", vocab_size=5000)}


def _searcher(cfg, lam):
    import torch
    from helpers import make_args
    from las import layers as L, variables as V
    from las.beam_search import BeamSearch
    from las.las import LAS, Listener, Speller
    args = make_args(enc_units=256, num_enc_layers=3, dec_units=512, num_dec_layers=1, embedding_size=128, attention_size=128,
                     beam_size=16, apply_lm=False, ctc=True, ctc_decode_weight=lam, seed=3, **CONFIGS[cfg])
    L.set_cell("lstm")
    L.set_precision("bf16")
    V.reset_default_store(device="cuda", seed=3)
    las = LAS(args, Listener, Speller, {})
    las.build_variables()
    tok = {"<SOS>": 1, "<EOS>": 2}
    bs = BeamSearch(args, las, tok, None)
    bs.measure = True
    torch.cuda.synchronize()
    return args, bs


def _utts(n, V):
    from helpers import synthetic_batch
    xs, _ = synthetic_batch(n, 1274, 8, V, seed=5, min_frac=1.0)
    return [(xs[0][i:i + 1], xs[1][i:i + 1]) for i in range(n)]


def step_us(cfg, lam, n):
    args, bs = _searcher(cfg, lam)
    utts = _utts(n, args.vocab_size)
    bs.decode_batch(None, utts)                      # warm-up: code objects, workspaces, the graph
    bs.decode_batch(None, utts)
    t = bs.last_timing
    # per step in which some utterance was still searching (the graph's last replay may run steps past every bound, which cost ~0)
    return round(t["searched"] / max(1, t["live_steps"]) * 1e6, 2), t["live_steps"], t["parts_us"]


def run(reps):
    out = {}
    for cfg in CONFIGS:
        for n in (16, 64):
            key = "%s_rows%d" % (cfg, n * 16)
            runs = {"lam0": [], "lam0.3": []}
            steps = {"lam0": [], "lam0.3": []}
            parts = {}
            for _ in range(reps):                    # alternating A / B on one device
                for lam, name in ((0.0, "lam0"), (0.3, "lam0.3")):
                    us, live, parts[name] = step_us(cfg, lam, n)
                    runs[name].append(us)
                    steps[name].append(live)
            out[key] = dict(runs, live_steps=steps, parts_us=parts, median_us={k: sorted(v)[len(v) // 2] for k, v in runs.items()})
            print(key, out[key], flush=True)
    return out


def rocprof(out):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "ctcdec", "--", sys.executable, os.path.abspath(__file__), "--child"]
        subprocess.run(cmd, check=True, timeout=900)
        stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        rows = list(csv.DictReader(open(stats[0])))
    with open(os.path.join(out, "ctc_decode_kernel_stats.csv"), "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0]))
        w.writeheader()
        w.writerows(rows)
    for r in rows:
        if "ctc" in r["Name"] or "beam" in r["Name"]:
            print(r["Name"][:60], r["Calls"], r["AverageNs"])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=PROF, help="directory of the output files")
    a = ap.parse_args()
    if a.child:
        step_us("char", 0.3, 16)
    elif a.rocprof:
        os.makedirs(a.out, exist_ok=True)
        rocprof(a.out)
    else:
        res = run(a.reps)
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "ctc_decode_bench.json"), "w") as f:
            json.dump(res, f, indent=1)
