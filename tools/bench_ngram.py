#!/usr/bin/env python
"""bench_ngram.py -- what n-gram LM shallow fusion costs in a search: device time per captured search step of decode_batch
without and with a trigram LM, in alternating runs on one device, at decode.py's geometry -- 64 utterances x beam 16 = 1024 hypothesis
rows, V = 5000 (the subword configuration of tools/bench_bias.py: bf16, T = 1274 input frames -> T' = 160).

    python tools/bench_ngram.py [--out profiles/ngram_bench.json] [--reps 3] [--sentences 100] [--weight 0.5]

The LM: train_ngram's Witten-Bell trigram estimated from --sentences random token strings of 200-400 tokens drawn from a Zipf-like
distribution over the vocabulary (long sentences, so that </s> is as rare as any other token: with short ones the LM ends every
hypothesis of a random model within a few steps and there is no search left to time; the share of hypothesis positions whose node is a
two-token context is recorded).  The step time is the search phase of LAS_DECODE_TIMING
(device synchronised at both ends) over the steps in which some utterance was still searching; parts_us holds the per-part device times,
`ngram` = las_ngram_step alone with every row live.  At V = 5000 the step is the long form with and without the LM (the short form's
in-kernel projection stops at 8 tiles), so the difference is the added launch.  A second configuration, the char model (V = 30), shows
the other cost: without the LM its step is the short form, with it the logits are materialised."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "automatic-speech-recognition_amd")]


def trigram(n_sentences, V, seed=7):
    import train_ngram
    from las.ngram import NgramLM
    rng = np.random.RandomState(seed)
    p = 1.0 / np.arange(1, V - 2)
    p /= p.sum()
    sents = [[1] + list(3 + rng.choice(V - 3, size=rng.randint(200, 401), p=p)) + [2] for _ in range(n_sentences)]
    return NgramLM(train_ngram.estimate(sents, 3, V), 3, V)


def deep_share(lm, results):
    """share of the returned hypotheses' token positions whose node is a context of two tokens"""
    deep = total = 0
    for res in results:
        for h in res:
            s = 0
            for v in h.token_ids:
                s = lm.step(s, int(v))
                deep += len(lm.nodes[s]) >= 2
                total += 1
    return deep / max(1, total)


CONFIGS = {"subword5000": dict(unit="subword", vocab_size=5000), "char": dict(unit="char", vocab_size=30)}


def run(o, cfg):
    import torch
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
    lm = trigram(o.sentences, args.vocab_size)
    runs = {"off": [], "on": []}
    info = {}
    for m in (None, lm):                             # warm-up: code objects, workspaces, the graphs, the table upload
        bs.set_ngram(m, o.weight if m is not None else 0.0)
        bs.decode_batch(None, utts)
    for _ in range(o.reps):                          # alternating A / B on one device
        for name, m in (("off", None), ("on", lm)):
            bs.set_ngram(m, o.weight if m is not None else 0.0)
            res = bs.decode_batch(None, utts)
            t = bs.last_timing
            runs[name].append(round(t["searched"] / max(1, t["live_steps"]) * 1e6, 2))
            info[name] = dict(live_steps=t["live_steps"], rows=t["rows"], graph=t["graph"], short_form=t["short_form"], parts_us=t["parts_us"])
            if m is not None:
                info[name]["deep_share"] = round(deep_share(lm, res), 4)
    med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
    return {"utterances": o.utts, "beam": 16, "V": args.vocab_size, "order": lm.order, "sentences": o.sentences, "nodes": lm.num_nodes,
            "entries": lm.num_entries, "weight": o.weight, "step_us": runs, "median_step_us": med,
            "added_us_per_step": round(med["on"] - med["off"], 2), "runs": info}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ngram_bench.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sentences", type=int, default=100)
    ap.add_argument("--weight", type=float, default=0.5)
    ap.add_argument("--utts", type=int, default=64)
    o = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_ngram.py measures on an MI355X: no device found")
    out = {"device": torch.cuda.get_device_name(0)}
    for cfg in CONFIGS:
        out[cfg] = run(o, cfg)
        print(cfg, json.dumps(out[cfg]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
    with open(o.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
