#!/usr/bin/env python
"""bench_coverage.py -- what the coverage scorer costs in a search: device time per captured search step of decode_batch
without and with it, in alternating runs on one device, at decode.py's geometry -- 64 utterances x beam 16 = 1024 hypothesis rows,
bf16, T = 1274 input frames -> T' = 160 -- for the two configurations of tools/bench_bias.py: char (V = 30, the short form of the
step) and subword (V = 5000, the long form).

    python tools/bench_coverage.py [--out profiles/coverage_bench.json] [--reps 3]

The step time is the search phase of LAS_DECODE_TIMING (device synchronised at both ends) over the steps in which some utterance was
still searching, the median of --reps runs; `short_form` is recorded for both runs (the scorer must not switch it off); parts_us holds
the per-part device times, `coverage` = las_coverage_step alone with every row live, set beside the las_bias_step figure recorded in
profiles/bias_bench.json.  The `off` run executes none of the scorer's code: it is the parent commit's step, and bias_bench.json's
`off` figure -- the same configuration, measured before the scorer existed -- is copied next to it.  No pass / fail time."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "automatic-speech-recognition_amd")]

CONFIGS = {"char": dict(unit="char", vocab_size=30), "subword5000": dict(unit="subword", vocab_size=5000)}
SETTING = dict(w_c=0.3, w_o=0.7, tau=0.5, kappa=1.5)


def run(o, cfg, recorded):
    from helpers import make_args, synthetic_batch
    from las import layers as L, variables as V
    from las.beam_search import BeamSearch
    from las.las import LAS, Listener, Speller
    c = CONFIGS[cfg]
    args = make_args(enc_units=256, num_enc_layers=3, dec_units=512, num_dec_layers=1, embedding_size=128, attention_size=128,
                     beam_size=16, apply_lm=False, seed=3, unit=c["unit"], vocab_size=c["vocab_size"])
    L.set_cell("lstm")
    L.set_precision("bf16")
    V.reset_default_store(device="cuda", seed=3)
    las = LAS(args, Listener, Speller, {})
    las.build_variables()
    bs = BeamSearch(args, las, {"<SOS>": 1, "<EOS>": 2}, None)
    bs.measure = True
    xs, _ = synthetic_batch(o.utts, 1274, 8, args.vocab_size, seed=5, min_frac=1.0)
    utts = [(xs[0][i:i + 1], xs[1][i:i + 1]) for i in range(o.utts)]
    modes = (("off", None), ("on", SETTING))
    runs, info = {"off": [], "on": []}, {}
    for _, s in modes:                               # warm-up: code objects, workspaces, the graphs
        bs.set_coverage(**(s or {}))
        bs.decode_batch(None, utts)
    for _ in range(o.reps):                          # alternating A / B on one device
        for name, s in modes:
            bs.set_coverage(**(s or {}))
            res = bs.decode_batch(None, utts)
            t = bs.last_timing
            runs[name].append(round(t["searched"] / max(1, t["live_steps"]) * 1e6, 2))
            info[name] = dict(live_steps=t["live_steps"], rows=t["rows"], frames=t["frames"], graph=t["graph"], short_form=t["short_form"],
                              parts_us=t["parts_us"])
            if s is not None:
                best = [r[-1].coverage for r in res if r]
                info[name]["mean_coverage"] = round(sum(c_ / max(f, 1) for c_, _, f in best) / max(1, len(best)), 4)
                info[name]["mean_overattended"] = round(sum(o_ / max(f, 1) for _, o_, f in best) / max(1, len(best)), 4)
    med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
    rec = (recorded or {}).get(cfg, {})
    return {"utterances": o.utts, "beam": 16, "V": args.vocab_size, "setting": SETTING, "step_us": runs, "median_step_us": med,
            "added_us_per_step": round(med["on"] - med["off"], 2), "short_form": {k: info[k]["short_form"] for k in info},
            "coverage_kernel_us": info["on"]["parts_us"].get("coverage"),
            "recorded_in_bias_bench": {"parent_step_us": rec.get("median_step_us", {}).get("off"),
                                       "las_bias_step_us": rec.get("runs", {}).get("on", {}).get("parts_us", {}).get("bias")},
            "runs": info}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coverage_bench.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--utts", type=int, default=64)
    o = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_coverage.py measures on an MI355X: no device found")
    recorded = None
    path = os.path.join(ROOT, "profiles", "bias_bench.json")
    if os.path.exists(path):
        with open(path) as f:
            recorded = json.load(f)
    out = {"device": torch.cuda.get_device_name(0)}
    for cfg in CONFIGS:
        out[cfg] = run(o, cfg, recorded)
        print(cfg, json.dumps(out[cfg]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
    with open(o.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
