#!/usr/bin/env python
"""Cost of the N-best consensus behind the search it follows: 64 utterances x beam 16 of the recipe's model with random
weights (V = 5000, 1200 input frames -> up to 199 decode steps), the N-best lists that search really returns.  One process, after two
warm-up rounds of everything, alternating per repetition:
  search_ms        host clock around decode_batch, device synchronised at both ends (BeamSearch.last_timing of one further, measured
                   search is kept beside it)
  call_ms          host clock around las.nbest.consensus + las.nbest.token_confidence (two uploads, four launches, two read-backs)
  chained_ms       host clock around las.nbest.consensus_confidence (one upload, four launches, pick stays on the device, one read-back)
  risk_dev_us      HIP events around 20 las_nbest_risk calls (pairs + risk kernels)
  conf_dev_us      HIP events around 20 las_nbest_confidence calls (align + trace kernels)
and once, because it takes seconds:
  oracle_s         tests/nbest_ref.py (numpy, one table row at a time) computing the same dist / risk / pick / match / conf on the host;
                   the results are compared for equality with the device's
Writes profiles/nbest_bench.json.

  python tools/bench_nbest.py [--reps 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "automatic-speech-recognition_amd")]
PROF = os.path.join(ROOT, "profiles")
N, BEAM, T_IN, V = 64, 16, 1200, 5000


def _setup():
    import torch
    from helpers import make_args, synthetic_batch
    from las import layers as L, variables as Vs
    from las.beam_search import BeamSearch
    from las.las import LAS, Listener, Speller
    args = make_args(enc_units=256, num_enc_layers=3, dec_units=512, num_dec_layers=1, embedding_size=128, attention_size=128,
                     beam_size=BEAM, apply_lm=False, ctc=False, ctc_decode_weight=0.0, seed=3, unit="subword", vocab_size=V)
    L.set_cell("lstm")
    L.set_precision("bf16")
    Vs.reset_default_store(device="cuda", seed=3)
    las = LAS(args, Listener, Speller, {})
    las.build_variables()
    bs = BeamSearch(args, las, {"<SOS>": 1, "<EOS>": 2}, None)
    xs, _ = synthetic_batch(N, T_IN, 8, V, seed=5, min_frac=1.0)
    utts = [(xs[0][i:i + 1], xs[1][i:i + 1]) for i in range(N)]
    torch.cuda.synchronize()
    return bs, utts


def _device_us(token_lists, weights, reps):
    """HIP events around the C calls alone, on the packed batch las.nbest uploads"""
    import torch
    from las import nbest as NB
    m = NB._pack(token_lists, weights)
    n, K, U = m["n"], m["K"], m["U"]
    out = torch.zeros(n * K * K + n * K + n, dtype=torch.int32, device=m["dev"])
    conf = torch.zeros(n, U, device=m["dev"])
    match = torch.zeros(n, K, U, dtype=torch.int8, device=m["dev"])
    pick = NB._risk(m, out)
    NB._confidence(m, pick, conf, match)
    res = []
    for fn in (lambda: NB._risk(m, out), lambda: NB._confidence(m, pick, conf, match)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        res.append(round(e0.elapsed_time(e1) / reps * 1e3, 2))
    return res, (n, K, U)


def _oracle(token_lists, weights):
    import nbest_ref as R
    t0 = time.perf_counter()
    out = []
    for hyps, w in zip(token_lists, weights):
        dist, risk, pick = R.risk(hyps, w)
        match, conf = R.confidence(hyps, w, pick)
        out.append((dist, risk, pick, match, conf))
    return time.perf_counter() - t0, out


def run(reps):
    import numpy as np
    import torch
    from las import nbest as NB
    bs, utts = _setup()

    def lists(results):
        token_lists, scores, lens = NB.hypotheses(results, 2)
        return token_lists, [NB.posteriors(s, l) for s, l in zip(scores, lens)]

    for _ in range(2):                               # warm-up: code objects, workspaces, the search's graph
        token_lists, weights = lists(bs.decode_batch(None, utts))
        NB.consensus(token_lists, weights)
        NB.token_confidence(token_lists, weights, [0 if t else -1 for t in token_lists])
        NB.consensus_confidence(token_lists, weights)
    out = {"n": N, "beam": BEAM, "V": V, "input_frames": T_IN, "search_ms": [], "call_ms": [], "chained_ms": [], "risk_dev_us": [],
           "conf_dev_us": []}
    for _ in range(reps):                            # alternating runs in one process
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        results = bs.decode_batch(None, utts)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        token_lists, weights = lists(results)
        t2 = time.perf_counter()
        dist, risk, pick = NB.consensus(token_lists, weights)
        conf, match = NB.token_confidence(token_lists, weights, pick)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        chained = NB.consensus_confidence(token_lists, weights)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        (risk_us, conf_us), shape = _device_us(token_lists, weights, 20)
        out["search_ms"].append(round((t1 - t0) * 1e3, 3))
        out["call_ms"].append(round((t3 - t2) * 1e3, 3))
        out["chained_ms"].append(round((t4 - t3) * 1e3, 3))
        out["risk_dev_us"].append(risk_us)
        out["conf_dev_us"].append(conf_us)
    bs.measure = True                                # one more search that leaves its phase timing in last_timing (extra waits: not timed above)
    bs.decode_batch(None, utts)
    bs.measure = False
    out["search_last_timing"] = {k: v for k, v in (bs.last_timing or {}).items() if k != "parts_us"}
    out["packed_n_K_U"] = list(shape)
    lens = [len(h) for t in token_lists for h in t]
    out["hypotheses"] = {"count": len(lens), "per_utterance_min": min(len(t) for t in token_lists),
                         "tokens_mean": round(float(np.mean(lens)), 1), "tokens_max": int(max(lens))}
    out["dp_cells"] = int(sum(len(a) * len(b) for t in token_lists for i, a in enumerate(t) for b in t[i + 1:])
                          + sum(len(t[p]) * len(b) for t, p in zip(token_lists, pick) if p >= 0 for b in t))
    oracle_s, ref = _oracle(token_lists, weights)
    for u, (d, r, p, m, c) in enumerate(ref):        # the timed results are the right ones
        assert np.array_equal(dist[u], d) and np.array_equal(risk[u].view(np.int32), r.view(np.int32)) and pick[u] == p
        assert np.array_equal(match[u], m) and np.array_equal(conf[u].view(np.int32), c.view(np.int32))
        assert chained[2][u] == p and np.array_equal(chained[3][u].view(np.int32), c.view(np.int32))
    out["oracle_s"] = round(oracle_s, 3)
    med = lambda v: sorted(v)[len(v) // 2]
    out["median"] = {k: med(out[k]) for k in ("search_ms", "call_ms", "chained_ms", "risk_dev_us", "conf_dev_us")}
    md = out["median"]
    out["call_share_of_search"] = round(md["call_ms"] / md["search_ms"], 4)
    out["chained_share_of_search"] = round(md["chained_ms"] / md["search_ms"], 4)
    out["device_share_of_search"] = round((md["risk_dev_us"] + md["conf_dev_us"]) * 1e-3 / md["search_ms"], 5)
    out["oracle_over_call"] = round(oracle_s * 1e3 / md["call_ms"], 1)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=PROF, help="directory of nbest_bench.json")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    res = run(a.reps)
    print(json.dumps(res), flush=True)
    with open(os.path.join(a.out, "nbest_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
