#!/usr/bin/env python
"""Two-pass decoding beside the two searches it joins: the 64-utterance, beam-16, V = 5000 batch of tools/bench_nbest.py
(the recipe's model with random weights and a CTC head, 1200 input frames).  One process, after two warm-up rounds of everything,
alternating per repetition:
  attention          host clock around BeamSearch.decode_batch, device synchronised at both ends
  ctc                ... around ctc_decode_batch (beam_size 16, --ctc_cand 32)
  ctc_rescore_64     ... with --rescore attention --rescore_rows 64
  ctc_rescore_256    ... with --rescore_rows 256
each as milliseconds per batch and utterances per second, and HIP events around las_rescore_score alone (its two launches, on buffers
made beforehand) on the first chunk of the batch's second pass (rows 64) next to a device copy of that chunk's logits buffer, the
memory-bound yardstick: the kernel reads the steps below each row's length once (bytes counted from the lengths), the copy reads and
writes the whole buffer.
Medians of --reps (5) with the smallest and largest value beside them.  Writes profiles/rescore_bench.json.

  python tools/bench_rescore.py [--reps 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "automatic-speech-recognition_amd")]
PROF = os.path.join(ROOT, "profiles")
W = 0.5


def run(reps):
    import numpy as np
    import torch
    import bench_ctc_search as B
    from las import _hip, rescore
    args, bs, utts = B._setup()

    def ctc(res, rows=64):
        args.rescore, args.rescore_ctc_weight, args.rescore_rows = res, W, rows
        try:
            return bs.ctc_decode_batch(None, utts)
        finally:
            args.rescore = "none"

    runs = {"attention": lambda: bs.decode_batch(None, utts), "ctc": lambda: ctc("none"), "ctc_rescore_64": lambda: ctc("attention", 64),
            "ctc_rescore_256": lambda: ctc("attention", 256)}
    out = {"n": B.N, "beam": B.BEAM, "V": B.V, "input_frames": B.T_IN, "cand": B.CAND, "weight": W, "refused": {}}
    for name in list(runs):                          # (a chunk geometry the Speller refuses is reported, not timed)
        try:
            runs[name]()
        except ValueError as e:
            out["refused"][name] = str(e)[:300]
            del runs[name]
    for fn in runs.values():                         # second warm-up round: code objects, workspaces, the search's graph
        fn()
    out["ms"] = {k: [] for k in runs}
    for _ in range(reps):                            # alternating runs in one process
        for name, fn in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            out["ms"][name].append(round((time.perf_counter() - t0) * 1e3, 3))
            if name.startswith("ctc_rescore"):
                moved = [sum(1 for i, d in enumerate(reversed(r)) if d["first_rank"] != i) for r in res.rescored]
                out.setdefault("hypotheses", {})[name] = {"per_utterance_mean": round(float(np.mean([len(r) for r in res])), 1),
                                                          "moved_mean": round(float(np.mean(moved)), 1),
                                                          "new_best": int(sum(1 for r in res.rescored if r and r[-1]["first_rank"] != 0))}
    # las_rescore_score alone on the first chunk of the second pass, next to a device copy of the chunk's logits buffer
    with torch.no_grad():
        encs, enc_lens, _, _, _ = bs._run_encoders(None, utts)
    first = ctc("none")
    strings = [[rescore.scored_string(h.token_ids[1:], bs.end_id) for h in reversed(r)] for r in first]
    c0, logits, y, lens = next(rescore.teacher_forced_logits(bs, encs, enc_lens, strings, rows=64))
    R_, U, V_ = logits.shape
    buf = logits.permute(1, 0, 2)                    # the Speller's time-major buffer itself
    assert buf.is_contiguous()
    dst = torch.empty_like(buf)
    read = int(lens.clamp(0, U).sum().item()) * V_ * 4
    kernel_us, copy_us = [], []
    att = torch.empty(R_, dtype=torch.float64, device=logits.device)
    nbytes = _hip.lib().las_rescore_workspace_bytes(R_, U)
    ws = _hip.workspace(logits.device, nbytes, "rescore")

    def score():
        _hip.check(_hip.lib().las_rescore_score(_hip.p(logits), logits.stride(0), logits.stride(1), _hip.p(y), y.stride(0), _hip.p(lens), R_, U,
                                                V_, _hip.p(att), None, _hip.p(ws), nbytes, _hip.stream()), "las_rescore_score")
    for _ in range(reps):
        kernel_us.append(B._events(score))
        copy_us.append(B._events(lambda: dst.copy_(buf)))
    stat = lambda x: {"median": sorted(x)[len(x) // 2], "min": min(x), "max": max(x)}
    k, c = stat(kernel_us), stat(copy_us)
    out["chunk"] = {"rows": R_, "U": U, "V": V_, "buffer_MB": round(buf.numel() * 4 / 1e6, 1), "read_MB": round(read / 1e6, 1),
                    "score_us": k, "copy_us": c, "score_over_copy_time": round(k["median"] / c["median"], 3),
                    "score_GBps_read": round(read / (k["median"] * 1e-6) / 1e9, 1),
                    "copy_GBps_read_plus_write": round(2 * buf.numel() * 4 / (c["median"] * 1e-6) / 1e9, 1)}
    out["summary"] = {n_: dict(stat(x), utt_per_s=round(B.N / (sorted(x)[len(x) // 2] * 1e-3), 1)) for n_, x in out["ms"].items()}
    if "ctc" in out["summary"]:
        for n_ in out["summary"]:
            if n_.startswith("ctc_rescore"):
                out["summary"][n_]["second_pass_ms"] = round(out["summary"][n_]["median"] - out["summary"]["ctc"]["median"], 3)
    _hip.check_status(logits.device)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=PROF, help="directory of rescore_bench.json")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    res = run(a.reps)
    print(json.dumps(res), flush=True)
    with open(os.path.join(a.out, "rescore_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
