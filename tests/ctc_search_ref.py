"""CPU restatement of CTC-only decoding (las/ctc_search.py, csrc/ctc_search.hip): the frame summary, the greedy collapse and
the CTC prefix beam search (Hannun et al. 2014) with an optional n-gram gain, WITHOUT a trie: a prefix is a tuple of tokens and the
beam a dict keyed by it.  numpy only.  Every function takes `ft`: np.float64 is the restatement proper; np.float32 is the same
arithmetic in the device's number format AND operation order (the lanes' strided partial sums and the butterfly of the log-sum-exp, one
rounding per add), which is what the device tolerance is measured from (measured_tolerance, tests/test_gpu_ctc_search.py).

Classes: Vc = V + 1, blank = V.  Mass at or below LOGZERO is no mass: a sum with such a term is LOGZERO and logaddexp ignores it."""
import functools

import numpy as np

LOGZERO = -1e10
MARGIN = 1e-3                     # least decision margin (nats) a GPU case must keep (tests/test_ctc_search_host.py asserts it)


# ---- frame summary ------------------------------------------------------------------------------------------------------------------
def _lse32(z):
    """[T, Vc] float32 -> [T] float32: m + logf(s) with s summed as the kernel sums it: 256 lanes, lane i adds classes i, i + 256, ... in
    order; a xor butterfly (32 .. 1) inside each 64-lane wave; the four wave sums added in order from 0"""
    T, Vc = z.shape
    m = z.max(axis=1)
    with np.errstate(all="ignore"):
        e = np.exp((z - m[:, None]).astype(np.float32)).astype(np.float32)
    rows = -(-Vc // 256)
    e = np.concatenate([e, np.zeros((T, rows * 256 - Vc), np.float32)], 1).reshape(T, rows, 256)
    part = np.zeros((T, 256), np.float32)
    for r in range(rows):
        part = (part + e[:, r]).astype(np.float32)
    idx = np.arange(256)
    for o in (32, 16, 8, 4, 2, 1):
        part = (part + part[:, idx ^ o]).astype(np.float32)
    s = np.zeros(T, np.float32)
    for w in range(4):
        s = (s + part[:, 64 * w]).astype(np.float32)
    with np.errstate(all="ignore"):
        return (m + np.log(s).astype(np.float32)).astype(np.float32)


def frame_summary(z, T, C, ft=np.float64):
    """z [Tp, Vc] logits (float32 values), the first T frames -> dict of best [T], best_lp [T], blank_lp [T], cand_tok [T, C] (the C
    non-blank classes of largest logit, ties to the lower id, listed in ascending id), cand_lp [T, C]"""
    z = np.asarray(z, np.float32)[:T]
    V = z.shape[1] - 1
    if ft is np.float32:
        lse = _lse32(z)
    else:
        z64 = z.astype(np.float64)
        m = z64.max(axis=1)
        with np.errstate(all="ignore"):
            lse = m + np.log(np.exp(z64 - m[:, None]).sum(axis=1))
    zz = z.astype(ft)
    with np.errstate(all="ignore"):
        lp = (zz - lse[:, None]).astype(ft)
    best = np.argmax(z, axis=1).astype(np.int64)                         # (the first maximum: ties to the lower id)
    order = np.argsort(-z[:, :V], axis=1, kind="stable")[:, :C]          # (stable: ties to the lower id)
    cand = np.sort(order, axis=1)
    rows = np.arange(T)[:, None]
    return dict(best=best, best_lp=lp[np.arange(T), best], blank_lp=lp[:, V], cand_tok=cand, cand_lp=lp[rows, cand])


# ---- greedy -------------------------------------------------------------------------------------------------------------------------
def greedy(best, best_lp, blank):
    """-> (tokens, score): best[t] where it is no blank and differs from best[t - 1]; the float64 sum of best_lp in frame order"""
    toks, prev = [], None
    for b in best:
        b = int(b)
        if b != blank and b != prev:
            toks.append(b)
        prev = b
    s = 0.0
    for x in best_lp:
        s += float(x)
    return toks, s


# ---- arithmetic ---------------------------------------------------------------------------------------------------------------------
def _live(x):
    return x > LOGZERO


def zadd(a, b, ft):
    if not _live(a) or not _live(b):
        return ft(LOGZERO)
    r = ft(ft(a) + ft(b))
    return r if _live(r) else ft(LOGZERO)


def lae(a, b, ft):
    if not _live(a):
        return ft(b) if _live(b) else ft(LOGZERO)
    if not _live(b):
        return ft(a)
    mx, mn = (a, b) if a >= b else (b, a)
    return ft(ft(mx) + np.log1p(np.exp(ft(ft(mn) - ft(mx)))))


# ---- the n-gram gain ----------------------------------------------------------------------------------------------------------------
def gram_gain(grams, order, w, sos):
    """-> gain(prefix, c) = the float32 value las_ngram_step would add for token c to a hypothesis whose tokens are (sos,) + prefix: read
    from the `grams` dict by the history alone (ngram_ref.row_gains32's arithmetic, for one token)"""
    import ngram_ref as G
    cache = {}

    def gain(prefix, c):
        ctx = G._context((sos,) + tuple(prefix), order)
        key = (ctx, c)
        if key not in cache:
            acc, h = np.float32(0.0), ctx
            while True:
                e = grams.get(h + (c,))
                if e is not None:
                    cache[key] = np.float32(acc + G.scaled(w, e[0]))
                    break
                assert h, "token %d has no unigram" % c
                if h in grams:
                    acc = np.float32(acc + G.scaled(w, grams[h][1]))
                h = h[1:]
        return cache[key]
    return gain


class TableGain(object):
    """gain(prefix, c) read from trie TABLES as the kernel walks them (csrc/ngram_trie.h's clamps: child ranges inside [0, E), a next or
    bo outside [0, M) is the root): for tables that hold out-of-range entries, where no `grams` dict says what they mean"""

    def __init__(self, tables, M, E, order, start):
        self.t, self.M, self.E, self.order = tables, int(M), int(E), int(order)
        self.nodes = {(): int(start) if 0 <= int(start) < self.M else 0}

    def _walk(self, node, c):
        t, acc, q = self.t, np.float32(0.0), node
        for _ in range(self.order):
            if q == 0:
                break
            lo, hi = int(t["child_off"][q]), int(t["child_off"][q + 1])
            lo = min(max(lo, 0), self.E)
            hi = min(max(hi, lo), self.E)
            while lo < hi:                                               # (the kernel's own binary search, whatever the list holds)
                mid = lo + ((hi - lo) >> 1)
                tk = int(t["child_tok"][mid])
                if tk == c:
                    nx = int(t["child_next"][mid])
                    return np.float32(acc + t["child_lp"][mid]), (nx if 0 <= nx < self.M else 0)
                if tk < c:
                    lo = mid + 1
                else:
                    hi = mid
            acc = np.float32(acc + t["bow"][q])
            q = int(t["bo"][q])
            q = q if 0 <= q < self.M else 0
        nx = int(t["uni_next"][c])
        return np.float32(acc + t["uni_lp"][c]), (nx if 0 <= nx < self.M else 0)

    def node(self, prefix):
        prefix = tuple(prefix)
        if prefix not in self.nodes:
            self.nodes[prefix] = self._walk(self.node(prefix[:-1]), prefix[-1])[1]
        return self.nodes[prefix]

    def __call__(self, prefix, c):
        return self._walk(self.node(prefix), int(c))[0]


# ---- prefix beam search -------------------------------------------------------------------------------------------------------------
def beam_search(summary, K, eos, gain=None, beta=0.0, ft=np.float64, trace=None):
    """summary: frame_summary's dict (its T frames are searched) -> (hyps, margin): hyps = [(tokens, total)] best first, at most K;
    margin = the smallest gap between a kept and a dropped total at any pruning and between neighbours of the final list (inf if none).
    gain(prefix, c): the n-gram's pre-scaled score of c behind prefix (None: 0).  trace: a list that receives every frame's beam."""
    LZ = ft(LOGZERO)
    beta = ft(np.float32(beta))
    beam = [((), ft(0.0), LZ)]                                           # (prefix, p_b, p_nb), best first
    margin = np.inf
    T = len(summary["best"])

    def g_of(prefix, c):
        lm = ft(gain(prefix, c)) if gain is not None else None
        return beta if lm is None else ft(lm + beta)

    for t in range(T):
        toks, lps, yb = summary["cand_tok"][t], summary["cand_lp"][t], ft(summary["blank_lp"][t])
        new, rank = {}, {}
        for j, (l, pb, pnb) in enumerate(beam):                         # entries of the beam come first in every tie, in slot order
            new[l] = [LZ, LZ]
            rank[l] = (0, j, 0)
        for j, (l, pb, pnb) in enumerate(beam):
            tot = lae(pb, pnb, ft)
            last = l[-1] if l else None
            closed = last == eos
            new[l][0] = lae(new[l][0], zadd(yb, tot, ft), ft)
            for i, c in enumerate(toks):
                c, y = int(c), ft(lps[i])
                if closed and c != last:
                    continue
                if c == last:
                    new[l][1] = lae(new[l][1], zadd(y, pnb, ft), ft)
                    if closed:
                        continue
                    x = zadd(zadd(y, pb, ft), g_of(l, c), ft)
                else:
                    x = zadd(zadd(y, tot, ft), g_of(l, c), ft)
                ext = l + (c,)
                if ext not in new:
                    new[ext] = [LZ, LZ]
                    rank[ext] = (1, j, i)
                new[ext][1] = lae(new[ext][1], x, ft)
        totals = {l: lae(v[0], v[1], ft) for l, v in new.items()}
        alive = sorted((l for l in new if _live(totals[l])), key=lambda l: (-totals[l], rank[l]))
        if len(alive) > K:
            margin = min(margin, float(totals[alive[K - 1]]) - float(totals[alive[K]]))
        beam = [(l, new[l][0], new[l][1]) for l in alive[:K]]
        if trace is not None:
            trace.append([(l, float(totals[l])) for l in alive[:K]])
        if not beam:
            break
    hyps = [(list(l), float(lae(pb, pnb, ft))) for l, pb, pnb in beam]
    for a, b in zip(hyps, hyps[1:]):
        margin = min(margin, a[1] - b[1])
    return hyps, margin


# ---- the case list of the device tests ----------------------------------------------------------------------------------------------
SOS, EOS = 1, 2
# name, Vc, Tp, T'_u per utterance, K, C, seed, n-gram order (0: none), length bonus, logit scale.  Every Vc of {3, 31, 5001}, T' of
# {1, 2, 7, 65, 160} (ragged, 1 included), K of {2, 16, 64}, C of {1, 2, 32, V}; seeds chosen on the CPU so that every utterance keeps
# a decision margin >= MARGIN (test_ctc_search_host asserts it: a seed that falls below is replaced there, no case is skipped)
CASES = [
    dict(name="v2-k64", Vc=3, Tp=7, lens=[7, 1, 2, 5], K=64, C=2, seed=8, order=0, beta=0.0, scale=1.5),
    dict(name="v2-c1", Vc=3, Tp=65, lens=[65, 33, 1], K=2, C=1, seed=1, order=0, beta=0.0, scale=2.0),
    dict(name="v30-cV", Vc=31, Tp=7, lens=[5, 3, 1, 2], K=64, C=30, seed=332, order=0, beta=0.5, scale=12.0),
    dict(name="v30-k2", Vc=31, Tp=65, lens=[65, 1, 40], K=2, C=2, seed=3, order=0, beta=0.0, scale=3.0),
    dict(name="v30-k16-uni", Vc=31, Tp=65, lens=[64, 65, 2], K=16, C=30, seed=34, order=1, beta=0.0, scale=3.0),
    dict(name="v30-k16-tri", Vc=31, Tp=160, lens=[160, 97, 1, 7], K=16, C=30, seed=15, order=3, beta=0.25, scale=3.0),
    dict(name="v5000-k16", Vc=5001, Tp=160, lens=[160, 131, 1], K=16, C=32, seed=76, order=0, beta=0.0, scale=2.0),
    dict(name="v5000-k64-tri", Vc=5001, Tp=7, lens=[7, 2, 5], K=64, C=32, seed=17, order=3, beta=0.0, scale=2.0),
]
LM_WEIGHT = 0.7


def eos_of(V):
    return EOS if V > EOS else V - 1


def case_logits(case):
    """[n, Tp, Vc] float32: scaled noise, a raised blank, and per utterance a label string (with repeats and, now and then, EOS) laid
    along the frames so that searches find non-trivial prefixes; frames past T'_u hold NaN (nobody may read them)"""
    rng = np.random.RandomState(1000 + case["seed"])
    n, Tp, Vc = len(case["lens"]), case["Tp"], case["Vc"]
    V = Vc - 1
    z = (rng.randn(n, Tp, Vc) ** 3 * case["scale"]).astype(np.float32)   # (heavy tails: the largest logits of a frame lie well apart)
    z[:, :, V] = z[:, :, :V].max(axis=2) * rng.uniform(0.4, 1.4, size=(n, Tp)).astype(np.float32)   # (blank wins about four frames in ten)
    for u, T in enumerate(case["lens"]):
        t = 0
        while t < T:
            c = int(rng.randint(V)) if rng.rand() > 0.1 else eos_of(V)
            run = int(rng.randint(1, 4))
            if rng.rand() < 0.6:
                z[u, t:min(T, t + run), c] += np.float32(case["scale"] * 2.0)
            t += run + int(rng.randint(0, 3))
        z[u, T:] = np.nan
    return z


def case_model(case):
    """the n-gram of a case: (grams, order) or None"""
    if not case["order"]:
        return None
    import ngram_ref as G
    return G.random_model(np.random.RandomState(2000 + case["seed"]), case["Vc"] - 1, case["order"]), case["order"]


@functools.lru_cache(maxsize=None)
def run_case(name, f32=False):
    """the restatement over a case: per utterance (summary, greedy (tokens, score), hyps, margin); cached, shared and left unchanged"""
    case = next(c for c in CASES if c["name"] == name)
    ft = np.float32 if f32 else np.float64
    z = case_logits(case)
    V = case["Vc"] - 1
    model = case_model(case)
    gain = gram_gain(model[0], model[1], LM_WEIGHT, SOS) if model else None
    out = []
    for u, T in enumerate(case["lens"]):
        s = frame_summary(z[u], T, case["C"], ft)
        hyps, margin = beam_search(s, case["K"], eos_of(V), gain, case["beta"], ft)
        out.append((s, greedy(s["best"], s["best_lp"], V), hyps, margin))
    return out


@functools.lru_cache(maxsize=None)
def measured_tolerance():
    """-> (lp_diff, score_diff): the largest absolute difference between the float32 restatement (the kernel's operation order) and the
    float64 one over the case list, for the per-frame log-probabilities and for the hypothesis totals / greedy scores.  Totals are
    compared only where both runs rank the same token lists (they do wherever the margin holds; asserted)."""
    lp_diff = sc_diff = 0.0
    for case in CASES:
        for a, b in zip(run_case(case["name"], False), run_case(case["name"], True)):
            for k in ("best_lp", "blank_lp", "cand_lp"):
                d = np.abs(a[0][k].astype(np.float64) - b[0][k].astype(np.float64))
                lp_diff = max(lp_diff, float(d[np.isfinite(d)].max()) if d.size else 0.0)
            assert [h[0] for h in a[2]] == [h[0] for h in b[2]], case["name"]
            sc_diff = max([sc_diff, abs(a[1][1] - b[1][1])] + [abs(x[1] - y[1]) for x, y in zip(a[2], b[2])])
    return lp_diff, sc_diff


# ---- the re-entry case --------------------------------------------------------------------------------------------------------------
def reentry_case():
    """-> (z [5, 4], K, C, eos): V = 3, K = 4.  After frame 2 the beam holds (2, 0) and its descendant (2, 0, 2); frame 3 drops (2, 0)
    and keeps (2, 0, 2); frame 4 brings (2, 0) back as the extension of (2,) by token 0.  The prefix must be the SAME entry it was: the
    parent of (2, 0, 2).  eos = 99 closes nothing."""
    z = np.array([[-4.0, -1.8, 1.5, -3.8],
                  [5.0, 2.8, 4.1, 1.5],
                  [1.6, 1.5, 4.1, 3.1],
                  [1.9, -3.3, 3.9, -2.3],
                  [1.1, -2.6, -2.2, -2.7]], np.float32)
    return z, 4, 3, 99


def reentries(trace):
    """beam_search's trace -> [(frame left, frame back, prefix, descendant)]: a prefix in the beam after frame `left - 1`, absent after
    frames left .. back - 1, in it again after frame `back`, while a proper descendant was in the beam all the time"""
    out = []
    sets = [set(l for l, _ in b) for b in trace]
    for t in range(1, len(sets)):
        for p in sets[t - 1] - sets[t]:
            for tb in range(t + 1, len(sets)):
                if p in sets[tb]:
                    out += [(t, tb, p, d) for d in sets[t - 1]
                            if len(d) > len(p) and d[:len(p)] == p and all(d in sets[k] for k in range(t, tb + 1))]
                    break
    return out
