"""CPU restatement of two-pass decoding (las/rescore.py, csrc/rescore.hip): the scored-string rule, the per-step
log-probabilities and per-hypothesis log-likelihoods read off teacher-forced logits, and the re-ranking.  numpy only.  `ft`: np.float64
is the restatement proper; np.float32 is the same arithmetic in the device's number format AND operation order (the lanes' strided
partial sums and the butterfly of the log-sum-exp, one rounding per add), which is what the device tolerance is measured from
(measured_tolerance, tests/test_gpu_rescore.py).  The re-ranking is float64 on the device too: rank() IS its arithmetic."""
import functools

import numpy as np

MARGIN = 1e-3                     # least gap (nats) between adjacent totals a GPU case must keep (tests/test_rescore_host.py asserts it)
REGS_CLASSES = 5120               # classes las_rescore_score keeps in registers (256 lanes x 20): a row up to here is read once


def scored_string(tokens, eos):
    """the tokens through the first EOS; without one, the tokens plus EOS"""
    toks = [int(t) for t in tokens]
    return toks[:toks.index(eos) + 1] if eos in toks else toks + [int(eos)]


# ---- scores -------------------------------------------------------------------------------------------------------------------------
def _lse32(z):
    """[N, V] float32 -> [N] float32: m + logf(s), s summed as the kernel sums it: 256 lanes, lane i adds classes i, i + 256, ... in
    order from 0; a xor butterfly (32 .. 1) inside each 64-lane wave; the four wave sums added in order from 0.  Rows whose maximum is
    -inf give -inf."""
    N, V = z.shape
    m = z.max(axis=1)
    dead = np.isneginf(m)
    ms = np.where(dead, np.float32(0), m).astype(np.float32)
    with np.errstate(all="ignore"):
        e = np.exp((z - ms[:, None]).astype(np.float32)).astype(np.float32)
    rows = -(-V // 256)
    e = np.concatenate([e, np.zeros((N, rows * 256 - V), np.float32)], 1).reshape(N, rows, 256)
    part = np.zeros((N, 256), np.float32)
    for r in range(rows):
        part = (part + e[:, r]).astype(np.float32)
    idx = np.arange(256)
    for o in (32, 16, 8, 4, 2, 1):
        part = (part + part[:, idx ^ o]).astype(np.float32)
    s = np.zeros(N, np.float32)
    for w in range(4):
        s = (s + part[:, 64 * w]).astype(np.float32)
    with np.errstate(all="ignore"):
        lse = (ms + np.log(s).astype(np.float32)).astype(np.float32)
    return np.where(dead, np.float32(-np.inf), lse).astype(np.float32)


def _lse64(z):
    z64 = z.astype(np.float64)
    m = z64.max(axis=1)
    dead = np.isneginf(m)
    ms = np.where(dead, 0.0, m)
    with np.errstate(all="ignore"):
        lse = ms + np.log(np.exp(z64 - ms[:, None]).sum(axis=1))
    return np.where(dead, -np.inf, lse)


def scores(z, y, lens, ft=np.float64):
    """z [R, U, V] logits (float32 values), y [R, >= U] labels, lens [R] (clamped to [0, U]) -> (att float64 [R], terms [R, U] of type
    ft, NaN at t >= lens[r]).  term = z[y] - lse, -inf where the step has no mass or the label lies outside [0, V); att = the sum of
    the terms in step order, in float64, from 0."""
    z = np.asarray(z, np.float32)
    R, U, V = z.shape
    lens = np.clip(np.asarray(lens, np.int64), 0, U)
    lse = (_lse32 if ft is np.float32 else _lse64)(z.reshape(R * U, V)).reshape(R, U)
    terms = np.full((R, U), np.nan, ft)
    att = np.zeros(R, np.float64)
    for r in range(R):
        for t in range(int(lens[r])):
            c = int(y[r, t])
            if 0 <= c < V and not np.isneginf(lse[r, t]):
                with np.errstate(all="ignore"):
                    terms[r, t] = ft(ft(z[r, t, c]) - ft(lse[r, t]))
            else:
                terms[r, t] = -np.inf
            att[r] += np.float64(terms[r, t])
    return att, terms


# ---- re-ranking ---------------------------------------------------------------------------------------------------------------------
def totals64(first, att, w):
    """(1 - w) att + w first in float64, unrounded"""
    with np.errstate(all="ignore"):
        return (1.0 - np.float64(w)) * np.asarray(att, np.float64) + np.float64(w) * np.asarray(first, np.float32).astype(np.float64)


def rank(first, att, w):
    """one utterance: first float32 [k], att float64 [k] -> (totals float32 [k], order): the slots by descending total, equal totals to
    the lower slot, NaN last in slot order"""
    with np.errstate(all="ignore"):
        tot = totals64(first, att, w).astype(np.float32)
    order = sorted(range(len(tot)), key=lambda k: (1, k) if np.isnan(tot[k]) else (0, -float(tot[k]), k))
    return tot, order


def margin(tot, ties=()):
    """the least gap between different adjacent finite totals of a ranked list; `ties`: sets of slots arranged to be exactly equal (their
    gap must BE 0 and is not counted).  -inf totals tie among themselves by construction and NaN has no gap."""
    tot = np.asarray(tot, np.float64)
    tied = {}
    for g, s in enumerate(ties):
        for k in s:
            tied[k] = g
    order = sorted((k for k in range(len(tot)) if np.isfinite(tot[k])), key=lambda k: (-tot[k], k))
    m = np.inf
    for a, b in zip(order, order[1:]):
        if a in tied and tied.get(b) == tied[a]:
            assert tot[a] == tot[b], "an arranged tie is not exact"
            continue
        m = min(m, tot[a] - tot[b])
    return m


# ---- the case lists of the device tests ---------------------------------------------------------------------------------------------
# name, R, U, ldy, V, layout (tm: the Speller's time-major [U, R, V] buffer; bm: batch-major [R, U, V]), seed, scale.  Every R of {1, 5,
# 37}, U of {1, 2, 9} with ldy > U, V of {2, 3, 31, 257, 5001, 16384} and 5119 / 5121 on either side of the register capacity, both
# layouts.  Cases of R >= 5 carry the special rows (case_data).  The R rows of a case are also ranked as ONE utterance (w = CASE_W)
# from the device's att: the seeds are chosen on the CPU so that the float64 totals keep MARGIN (test_rescore_host asserts it: a seed
# that falls below is replaced there, no case is skipped)
SCORE_CASES = [
    dict(name="r1-u1-v2", R=1, U=1, ldy=3, V=2, layout="tm", seed=1, scale=2.0),
    dict(name="r5-u2-v3", R=5, U=2, ldy=3, V=3, layout="bm", seed=2, scale=2.0),
    dict(name="r37-u9-v31", R=37, U=9, ldy=12, V=31, layout="tm", seed=3, scale=3.0),
    dict(name="r5-u9-v257", R=5, U=9, ldy=10, V=257, layout="bm", seed=4, scale=3.0),
    dict(name="r37-u2-v5001", R=37, U=2, ldy=5, V=5001, layout="tm", seed=5, scale=2.0),
    dict(name="r5-u9-v16384", R=5, U=9, ldy=11, V=16384, layout="tm", seed=6, scale=2.0),
    dict(name="r5-u2-v5119", R=5, U=2, ldy=4, V=5119, layout="bm", seed=7, scale=2.0),
    dict(name="r37-u1-v5121", R=37, U=1, ldy=2, V=5121, layout="tm", seed=13, scale=2.0),
]
CASE_W = 0.3
BAD_LABEL = -7                    # y beyond a row's length, and one of the out-of-range labels


@functools.lru_cache(maxsize=None)
def case_data(name):
    """-> dict z [R, U, V] float32, y [R, ldy] int32, lens [R] int32, first [R] float32.  lens are ragged with U (row 0) and, from two
    rows on, 0 (row 1).  With R >= 5: row 0 holds logits around +1e4 (even steps) and -1e4 (odd steps); row 2 has -inf columns beside
    its labels (finite); row 3's step 0 is all -inf (no mass: -inf, not NaN); row 4's labels are out of range (V at step 0, a negative
    one behind it); with R > 5, row 5's label at step 0 sits on a -inf column.  Cached, shared and left unchanged."""
    case = next(c for c in SCORE_CASES if c["name"] == name)
    rng = np.random.RandomState(3000 + case["seed"])
    R, U, V, ldy = case["R"], case["U"], case["V"], case["ldy"]
    z = (rng.randn(R, U, V) * case["scale"]).astype(np.float32)
    y = np.full((R, ldy), BAD_LABEL, np.int32)
    y[:, :U] = rng.randint(0, V, size=(R, U))
    lens = rng.randint(0, U + 1, size=R).astype(np.int32)
    lens[0] = U
    if R >= 2:
        lens[1] = 0
    if R >= 5:
        z[0, 0::2] += np.float32(1e4)
        z[0, 1::2] -= np.float32(1e4)
        lens[2:6] = np.maximum(lens[2:6], 1)
        lens[4] = U
        cols = rng.choice(V, size=max(1, V // 3), replace=False)
        y[2, :U] = rng.choice(np.setdiff1d(np.arange(V), cols), size=U)
        z[2][:, cols] = -np.inf
        z[3, 0, :] = -np.inf
        y[4, 0] = V
        if U > 1:
            y[4, 1] = BAD_LABEL
        if R > 5:
            z[5][:, cols] = -np.inf
            y[5, 0] = cols[0]
    first = (rng.randn(R) * 6.0 - 10.0).astype(np.float32)
    return dict(z=z, y=y, lens=lens, first=first)


@functools.lru_cache(maxsize=None)
def run_case(name, f32=False):
    """the restatement over a score case -> (att, terms, totals float32, order); cached, shared and left unchanged"""
    d = case_data(name)
    att, terms = scores(d["z"], d["y"], d["lens"], np.float32 if f32 else np.float64)
    tot, order = rank(d["first"], att, CASE_W)
    return att, terms, tot, order


# name, K, nhyp per utterance (ragged, 0 included), seed.  Utterance 0 of every case with K >= 2 holds an arranged exact tie (two
# bit-equal slots); from K = 16 on one slot of utterance 0 has a NaN attention score (ranked last)
RANK_CASES = [
    dict(name="k1", K=1, nhyp=[1, 0, 1], seed=1),
    dict(name="k2", K=2, nhyp=[2, 1, 0, 2], seed=2),
    dict(name="k16", K=16, nhyp=[16, 0, 7, 1, 16], seed=3),
    dict(name="k64", K=64, nhyp=[64, 33, 0, 64, 2], seed=4),
]
RANK_WEIGHTS = (0.0, 0.3, 1.0)


@functools.lru_cache(maxsize=None)
def rank_case_data(name):
    """-> dict first float32 [n, K], att float64 [n, K], nhyp int32 [n], ties {utterance: [set of slots]}; slots at and beyond nhyp[u]
    hold NaN (nobody may read them)"""
    case = next(c for c in RANK_CASES if c["name"] == name)
    rng = np.random.RandomState(4000 + case["seed"])
    K, nh = case["K"], np.asarray(case["nhyp"], np.int32)
    n = len(nh)
    first = (rng.randn(n, K) * 12.0 - 20.0).astype(np.float32)
    att = rng.randn(n, K) * 15.0 - 30.0
    ties = {}
    if K >= 2:
        a, b = 0, K - 1
        first[0, b], att[0, b] = first[0, a], att[0, a]
        ties[0] = [{a, b}]
    if K >= 16:
        att[0, 5] = np.nan
    for u in range(n):
        first[u, nh[u]:] = np.nan
        att[u, nh[u]:] = np.nan
    return dict(first=first, att=att, nhyp=nh, ties=ties)


def rank_batch(first, att, nhyp, w):
    """rank() per utterance of a [n, K] batch -> (totals, orders) as lists"""
    out = [rank(first[u, :nhyp[u]], att[u, :nhyp[u]], w) for u in range(len(nhyp))]
    return [o[0] for o in out], [o[1] for o in out]


@functools.lru_cache(maxsize=None)
def measured_tolerance():
    """-> (step_diff, att_diff): the largest absolute difference between the float32 restatement (the kernel's operation order) and the
    float64 one over the score cases, for the step terms and for att / the totals (the larger of the two).  -inf entries agree exactly
    (asserted) and do not count."""
    step_diff = att_diff = 0.0
    for case in SCORE_CASES:
        a64, t64, tot64, o64 = run_case(case["name"], False)
        a32, t32, tot32, o32 = run_case(case["name"], True)
        assert o64 == o32, case["name"]
        for x, yv in ((t64, t32), (a64, a32), (tot64, tot32)):
            assert np.array_equal(np.isfinite(x), np.isfinite(yv)) and np.array_equal(np.isneginf(x), np.isneginf(yv)), case["name"]
        fin = np.isfinite(t64)
        if fin.any():
            step_diff = max(step_diff, float(np.abs(t64[fin] - t32[fin].astype(np.float64)).max()))
        fin = np.isfinite(a64)
        if fin.any():
            att_diff = max(att_diff, float(np.abs(a64[fin] - a32[fin]).max()),
                           float(np.abs(tot64[fin].astype(np.float64) - tot32[fin].astype(np.float64)).max()))
    return step_diff, att_diff
