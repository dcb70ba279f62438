#!/usr/bin/env python
"""Cost of the N-best confusion network next to the consensus calls it stands beside (7l): tools/bench_nbest.py's batch -- 64
utterances x beam 16 of the recipe's model with random weights, the N-best lists that search really returns, tokens as symbols.  One
process, one search, two warm-up rounds of everything, then alternating per repetition:
  risk_dev_us      HIP events around 20 las_nbest_risk calls
  conf_dev_us      HIP events around 20 las_nbest_confidence calls
  network_dev_us   HIP events around 20 las_nbest_network calls (one launch, one wave per utterance)
  network_call_ms  host clock around las.nbest.network (one upload, one call, one read-back)
  ceiling_dev_us   las_nbest_network at the ceiling of K = 64 slots: 64 utterances of 64 noisy copies of a 60-symbol string
medians of the repetitions with [min, max].  Once: tests/confnet_ref.py on the first eight utterances, compared for equality.
Writes profiles/confnet_bench.json.

  python tools/bench_confnet.py [--reps 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "automatic-speech-recognition_amd")]
PROF = os.path.join(ROOT, "profiles")


def _events(fn, calls=20):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / calls * 1e3, 2)


def _network_call(token_lists, weights):
    """the packed batch and a closure that launches las_nbest_network on it"""
    import torch
    from las import _hip, nbest as NB
    m = NB._pack(token_lists, weights)
    n, K, U = m["n"], m["K"], m["U"]
    mb = min(NB.MAX_BINS, max(1, max(sum(len(h) for h in t) for t in token_lists)))
    i32 = dict(dtype=torch.int32, device=m["dev"])
    cols, nbins, best = torch.zeros(n, K, mb, **i32), torch.zeros(n, **i32), torch.zeros(n, mb, **i32)
    merged, post = torch.zeros(n, K, dtype=torch.int8, device=m["dev"]), torch.zeros(n, mb, device=m["dev"])
    lib = _hip.lib()
    nbytes = lib.las_nbest_network_workspace_bytes(n, K, U, mb)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=m["dev"])

    def call():
        _hip.check(lib.las_nbest_network(_hip.p(m["tok"]), _hip.p(m["len"]), _hip.p(m["nhyp"]), _hip.p(m["w"]), n, K, U, mb, _hip.p(cols),
                                         _hip.p(nbins), _hip.p(merged), _hip.p(best), _hip.p(post), _hip.p(ws), nbytes, _hip.stream()),
                   "las_nbest_network")
    return call, (n, K, U, mb), nbins


def _ceiling_batch(n=64, K=64, L=60, vocab=5000, seed=11):
    import numpy as np
    rng = np.random.RandomState(seed)
    utts, weights = [], []
    for _ in range(n):
        base = list(rng.randint(0, vocab, size=L))
        hyps = []
        for _ in range(K):
            h = list(base)
            for _ in range(6):                                         # a noisy copy: deletions, insertions, substitutions
                p, op = rng.randint(0, len(h)), rng.randint(0, 3)
                if op == 0 and len(h) > 1:
                    del h[p]
                elif op == 1:
                    h.insert(p, int(rng.randint(0, vocab)))
                else:
                    h[p] = int(rng.randint(0, vocab))
            hyps.append(h)
        w = rng.uniform(0.01, 1.0, size=K)
        utts.append(hyps)
        weights.append((w / w.sum()).astype(np.float32))
    return utts, weights


def run(reps):
    import numpy as np
    import torch
    import bench_nbest as BN
    import confnet_ref as C
    from las import nbest as NB
    bs, utts = BN._setup()
    token_lists, scores, lens = NB.hypotheses(bs.decode_batch(None, utts), 2)
    weights = [NB.posteriors(s, l) for s, l in zip(scores, lens)]
    m = NB._pack(token_lists, weights)
    n, K, U = m["n"], m["K"], m["U"]
    out7l = torch.zeros(n * K * K + n * K + n, dtype=torch.int32, device=m["dev"])
    conf, match = torch.zeros(n, U, device=m["dev"]), torch.zeros(n, K, U, dtype=torch.int8, device=m["dev"])
    pick = NB._risk(m, out7l)
    net_call, shape, nbins = _network_call(token_lists, weights)
    top_lists, top_weights = _ceiling_batch()
    top_call, top_shape, top_nbins = _network_call(top_lists, top_weights)
    fns = {"risk_dev_us": lambda: NB._risk(m, out7l), "conf_dev_us": lambda: NB._confidence(m, pick, conf, match),
           "network_dev_us": net_call, "ceiling_dev_us": top_call}
    for _ in range(2):                                                 # warm-up: code objects, workspaces
        for fn in fns.values():
            fn()
        NB.network(token_lists, weights)
    torch.cuda.synchronize()
    out = {"n": n, "beam": BN.BEAM, "packed_n_K_U_maxbins": list(shape), "ceiling_n_K_U_maxbins": list(top_shape)}
    series = {k: [] for k in list(fns) + ["network_call_ms"]}
    for _ in range(reps):                                              # alternating runs in one process
        for k, fn in fns.items():
            series[k].append(_events(fn))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nets = NB.network(token_lists, weights)
        series["network_call_ms"].append(round((time.perf_counter() - t0) * 1e3, 3))
    out["runs"] = series
    out["median_min_max"] = {k: [sorted(v)[len(v) // 2], min(v), max(v)] for k, v in series.items()}
    lens = [len(h) for t in token_lists for h in t]
    out["hypotheses"] = {"count": len(lens), "tokens_mean": round(float(np.mean(lens)), 1), "tokens_max": int(max(lens))}
    out["bins"] = {"mean": round(float(nbins.float().mean()), 1), "max": int(nbins.max()),
                   "ceiling_mean": round(float(top_nbins.float().mean()), 1), "ceiling_max": int(top_nbins.max())}
    t0 = time.perf_counter()
    for u in range(min(8, n)):                                         # the timed results are the right ones
        ref = C.network(token_lists[u], weights[u], shape[3], "f32")
        assert np.array_equal(nets[u]["cols"], ref["cols"]) and np.array_equal(nets[u]["best"], ref["best"])
        assert np.array_equal(nets[u]["post"].view(np.int32), ref["post"].view(np.int32))
    out["oracle_s_8_utterances"] = round(time.perf_counter() - t0, 3)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=PROF, help="directory of confnet_bench.json")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    res = run(a.reps)
    print(json.dumps(res), flush=True)
    with open(os.path.join(a.out, "confnet_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
