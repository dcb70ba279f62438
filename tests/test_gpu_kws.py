"""las_kws_search (include/las_hip.h K10j, csrc/kws.hip) against the float64 restatement tests/kws_ref.py.  The contract fixes the
arithmetic (one fp64 subtraction and one fp64 addition per state and frame, in frame order; an fp32 maximum, exact in any order) and
every tie rule, so hits, counts, best and the end series are compared for EQUALITY: that is the bound the contract derives, not a
measured one.  Entries the call does not write keep a sentinel."""
import functools
import math

import numpy as np
import pytest
import torch

import helpers  # noqa: F401
import kws_ref as R
import test_kws_host as HC

pytestmark = pytest.mark.gpu
SENTINEL = -77
SENTINEL_F = 123.0


def _launch(lp, lens, phrases, thr, H, U=None, series=True, ws_short=0, drop=None):
    """-> dict(rc, hit_start, hit_end, hit_score [n, P, H], count [n, P, 2], best_score [n, P], best_span [n, P, 2], end_score, end_start
    [n, P, Tp] or None).  lp: numpy [n, Vc, Tp] or a device tensor.  A phrase longer than U keeps its length in y_len and its first U
    labels in y.  drop: 'end_score' / 'end_start' -> that pointer alone is NULL."""
    from las import _hip
    d_lp = lp if torch.is_tensor(lp) else torch.tensor(np.ascontiguousarray(lp, np.float32), device="cuda")
    n, Vc, Tp = d_lp.shape
    P = len(phrases)
    U = max(1, max(len(ph) for ph in phrases)) if U is None else U
    y = np.zeros((P, U), np.int32)
    for k, ph in enumerate(phrases):
        y[k, :min(len(ph), U)] = ph[:U]
    i32 = dict(dtype=torch.int32, device="cuda")
    f64 = dict(dtype=torch.float64, device="cuda")
    d_len, d_y, d_yl = torch.tensor(lens, **i32), torch.tensor(y, **i32), torch.tensor([len(ph) for ph in phrases], **i32)
    d_thr = torch.tensor(np.asarray(thr, np.float32), device="cuda")
    o = dict(hit_start=torch.full((n, P, H if H > 0 else 1), SENTINEL, **i32), hit_end=torch.full((n, P, H if H > 0 else 1), SENTINEL, **i32),
             hit_score=torch.full((n, P, H if H > 0 else 1), SENTINEL_F, **f64), count=torch.full((n, P, 2), SENTINEL, **i32),
             best_score=torch.full((n, P), SENTINEL_F, **f64), best_span=torch.full((n, P, 2), SENTINEL, **i32),
             end_score=torch.full((n, P, Tp), SENTINEL_F, **f64) if series else None,
             end_start=torch.full((n, P, Tp), SENTINEL, **i32) if series else None)
    lib = _hip.lib()
    nbytes = lib.las_kws_workspace_bytes(n, Tp)
    ws = torch.zeros(max(nbytes, 256), dtype=torch.uint8, device="cuda")
    ptr = {k: (None if k == drop else _hip.p(v)) for k, v in o.items()}
    rc = lib.las_kws_search(_hip.p(d_lp), Vc, Tp, _hip.p(d_len), n, _hip.p(d_y), U, _hip.p(d_yl), _hip.p(d_thr), P, U, H, ptr["hit_start"],
                            ptr["hit_end"], ptr["hit_score"], ptr["count"], ptr["best_score"], ptr["best_span"], ptr["end_score"],
                            ptr["end_start"], _hip.p(ws), nbytes - ws_short, _hip.stream())
    torch.cuda.synchronize()
    out = {k: (None if v is None else v.cpu().numpy()) for k, v in o.items()}
    out["rc"] = rc
    return out


def _untouched(out):
    return all(np.all(v == (SENTINEL_F if v.dtype == np.float64 else SENTINEL)) for k, v in out.items() if k != "rc" and v is not None)


def _same_bits(a, b):
    for k in a:
        if k == "rc" or a[k] is None:
            continue
        x, y = (a[k].view(np.int64), b[k].view(np.int64)) if a[k].dtype == np.float64 else (a[k], b[k])
        assert np.array_equal(x, y), k


def _check(lp, lens, phrases, thr, H, out, U=None, cache=None):
    """every output of one launch against the restatement; -> (phrases x utterances with more closed hits than H, with no reachable end)"""
    assert out["rc"] == 0
    n, Vc, Tp = lp.shape
    U = max(1, max(len(ph) for ph in phrases)) if U is None else U
    cache = {} if cache is None else cache
    over = unreached = 0
    for u in range(n):
        T = min(max(int(lens[u]), 1), Tp)
        for p, ph in enumerate(phrases):
            key = (u, p)
            if key not in cache:                                                       # the series does not depend on thr and H
                cache[key] = R.search(lp[u], ph, T, -np.inf, 1, Tp=Tp, U=U)
            ref = cache[key]
            kept, total = R.hits_of(ref.end_score[:T], ref.end_start[:T], thr[p], H) if R.searchable(ph, Vc, U) else ([], 0)
            where = (u, p, ph)
            assert tuple(out["count"][u, p]) == (len(kept), total), (where, out["count"][u, p], len(kept), total)
            k = len(kept)
            assert [(int(a), int(b), float(c)) for a, b, c in zip(out["hit_start"][u, p, :k], out["hit_end"][u, p, :k],
                                                                    out["hit_score"][u, p, :k])] == kept, (where, kept)      # equal bits
            assert np.all(out["hit_start"][u, p, k:] == SENTINEL) and np.all(out["hit_end"][u, p, k:] == SENTINEL)
            assert np.all(out["hit_score"][u, p, k:] == SENTINEL_F)                    # entries at or beyond `kept` are not written
            assert (float(out["best_score"][u, p]), int(out["best_span"][u, p, 0]), int(out["best_span"][u, p, 1])) == ref.best, (where, ref.best)
            if out["end_score"] is not None:
                assert np.array_equal(out["end_score"][u, p], ref.end_score), (where, out["end_score"][u, p], ref.end_score)
                assert np.array_equal(out["end_start"][u, p], ref.end_start), (where, out["end_start"][u, p], ref.end_start)
            over += total > H
            unreached += ref.best[0] == -np.inf
    return over, unreached


def _lp(rng, n, Vc, Tp, scale=2.0):
    return torch.log_softmax(torch.tensor(rng.randn(n, Tp, Vc) * scale, dtype=torch.float32), -1).transpose(1, 2).contiguous().numpy()


def _labels(rng, L, Vc, repeats=False):
    out = []
    for j in range(L):
        c = int(rng.randint(0, Vc - 1))
        if repeats and j % 3 == 1:
            c = out[-1]
        while not repeats and out and c == out[-1]:
            c = int(rng.randint(0, Vc - 1))
        out.append(c)
    return out


LENGTHS = [1, 2, 3, 17, 32, 2, 3, 17, 32]             # S = 1, 3, 5, 33 (crosses a 32-lane half), 63 (every lane but one)
REPEATS = [False, False, True, False, True, True, False, True, False]


@pytest.mark.parametrize("Vc", [31, 5001])
@pytest.mark.parametrize("Tp", [1, 2, 7, 65, 160])
def test_matches_restatement(Tp, Vc):
    """three utterances of different enc_len per launch; P = 9, 5, 1 (the last workgroup partly empty); phrases with and without adjacent
    repeats; thr = -inf (every reachable frame is a candidate: the overlap rule is worked hardest) and a moderate threshold; H = 1, 2,
    8 with more closed hits than H; the series asked for and not; two runs give the same bits.  A phrase longer than a short row has no
    reachable end there and must say so."""
    rng = np.random.RandomState(Tp * 7 + Vc)
    lens = [Tp, max(1, Tp - 3), max(1, Tp // 2)]
    lp = _lp(rng, 3, Vc, Tp)
    d_lp = torch.tensor(lp, device="cuda")
    all_phrases = [_labels(rng, L, Vc, rep) for L, rep in zip(LENGTHS, REPEATS)]
    over = unreached = 0
    for P in (9, 5, 1):
        phrases = all_phrases[2:3] if P == 1 else all_phrases[:P]
        ninf = [-np.inf] * P
        moderate = [-2.5 * len(ph) for ph in phrases]
        cache = {}
        runs = ((ninf, 1), (ninf, 2), (ninf, 8), (moderate, 2)) if P == 9 else ((ninf, 2), (moderate, 8))
        for thr, H in runs:
            out = _launch(d_lp, lens, phrases, thr, H)
            a, b = _check(lp, lens, phrases, thr, H, out, cache=cache)
            over, unreached = over + a, unreached + b
        _same_bits(out, _launch(d_lp, lens, phrases, thr, H))                          # two runs: the same bits
        nos = _launch(d_lp, lens, phrases, thr, H, series=False)                       # the series is optional
        _check(lp, lens, phrases, thr, H, nos, cache=cache)
        for k in ("hit_start", "hit_end", "hit_score", "count", "best_score", "best_span"):
            assert np.array_equal(nos[k], out[k])
    if Tp >= 7:
        assert over > 0                                # (an L = 1 phrase closes a hit at nearly every frame under thr = -inf)
    if Tp <= 7:
        assert unreached > 0                           # L = 17, 32 do not fit


def test_ties_follow_the_rule():
    """a uniform lp (every path ties at 0.0) and an lp that is constant along t: exactly the restatement's hits; and the cases worked
    out in test_kws_host.py"""
    rng = np.random.RandomState(9)
    Vc, Tp = 6, 40
    lens = [40, 23, 9]
    phrases = [[0, 1, 1, 2, 0], [3, 3], [4, 0, 4, 0, 4, 0, 4], [2]]
    uniform = np.full((3, Vc, Tp), np.float32(np.log(1.0 / Vc)), np.float32)
    for thr in ([-np.inf] * 4, [0.0] * 4):
        out = _launch(uniform, lens, phrases, thr, 2)
        _check(uniform, lens, phrases, thr, 2, out)
    for u, T in enumerate(lens):                                                       # one hit (0, T - 1, 0.0) for every phrase
        assert np.all(out["count"][u] == 1) and np.all(out["hit_start"][u, :, 0] == 0) and np.all(out["hit_end"][u, :, 0] == T - 1)
        assert np.all(out["hit_score"][u, :, 0] == 0.0)
    const_t = np.repeat(_lp(rng, 3, Vc, 1), Tp, axis=2)
    for thr in ([-np.inf] * 4, [-2.0 * len(ph) for ph in phrases]):
        for H in (1, 8):
            _check(const_t, lens, phrases, thr, H, _launch(const_t, lens, phrases, thr, H))
    lp, ph = HC.hand_case()
    out = _launch(lp[None], [6], [ph], [-2.0], 4)
    _check(lp[None], [6], [ph], [-2.0], 4, out)
    assert list(out["end_score"][0, 0]) == [-np.inf, -4.0, -1.0, -2.0, 0.0, -1.0] and list(out["end_start"][0, 0]) == [-1, 0, 1, 1, 1, 1]
    assert (out["hit_start"][0, 0, 0], out["hit_end"][0, 0, 0], out["hit_score"][0, 0, 0]) == (1, 4, 0.0)


def test_kept_list_overflow():
    lp, ph = HC.overflow_case()
    for H, want in ((1, [1]), (2, [1, 3]), (8, [0, 1, 2, 3, 4])):
        out = _launch(lp[None], [28], [ph], [-1.0], H)
        _check(lp[None], [28], [ph], [-1.0], H, out)
        assert list(out["count"][0, 0]) == [len(want), 5]
        assert list(out["hit_start"][0, 0, :len(want)]) == [3 + 5 * k for k in want]
        assert list(out["hit_score"][0, 0, :len(want)]) == [HC.OVERFLOW_SCORES[k] for k in want]


def test_planted_phrases_are_found_exactly():
    lp, lens, phrases, want = HC.planted_case()
    thr = [-1.0 * len(ph) for ph in phrases]
    out = _launch(lp, lens, phrases, thr, 4)
    _check(lp, lens, phrases, thr, 4, out)
    for u in range(len(lens)):
        for p, (a, b) in enumerate(want[u]):
            assert list(out["count"][u, p]) == [1, 1]
            assert (out["hit_start"][u, p, 0], out["hit_end"][u, p, 0], out["hit_score"][u, p, 0]) == (a, b, 0.0)


def test_unsearchable_phrases_leave_their_neighbours_alone():
    """y_len 0 and 33, a label equal to the blank class, a negative label: count (0, 0), best -inf / -1 / -1 and a -inf / -1 series for
    the phrase in every utterance, the restatement's result for the phrases beside it, return code 0"""
    rng = np.random.RandomState(4)
    Vc, Tp = 31, 12
    lens = [12, 5]
    phrases = [_labels(rng, 3, Vc), [], _labels(rng, 2, Vc, repeats=True), [5] * 33, [1, Vc - 1, 2], _labels(rng, 4, Vc), [3, -1]]
    lp = _lp(rng, 2, Vc, Tp)
    thr = [-np.inf] * len(phrases)
    out = _launch(lp, lens, phrases, thr, 2, U=32)
    _check(lp, lens, phrases, thr, 2, out, U=32)
    for p in (1, 3, 4, 6):
        assert np.all(out["count"][:, p] == 0) and np.all(out["best_score"][:, p] == -np.inf) and np.all(out["best_span"][:, p] == -1)
        assert np.all(out["end_score"][:, p] == -np.inf) and np.all(out["end_start"][:, p] == -1)
    for p in (0, 2, 5):
        assert np.isfinite(out["best_score"][0, p])
    # a phrase longer than U (but not than 32) cannot be searched either
    longer = phrases[:1] + [_labels(rng, 5, Vc)]
    out = _launch(lp, lens, longer, [-np.inf] * 2, 2, U=4)
    _check(lp, lens, longer, [-np.inf] * 2, 2, out, U=4)
    assert np.all(out["count"][:, 1] == 0) and np.all(out["best_score"][:, 1] == -np.inf)


def test_refusals():
    """U = 33, T' = 2049, H = 0 and 9, one series pointer NULL, a short workspace: a nonzero return, a las_last_error text, and nothing
    launched (the outputs keep what the test put there)"""
    from las import _hip
    lib = _hip.lib()
    lp = np.zeros((1, 4, 8), np.float32)
    for kw, text, shape in ((dict(U=33), b"U=33", lp), (dict(), b"T' <= 2048", np.zeros((1, 4, 2049), np.float32)), (dict(H=0), b"H=0", lp),
                            (dict(H=9), b"H=9", lp), (dict(drop="end_score"), b"together", lp), (dict(drop="end_start"), b"together", lp),
                            (dict(ws_short=1), b"workspace too small", lp)):
        kw = dict(dict(H=2), **kw)
        out = _launch(shape, [8], [[0, 1]], [-1.0], **kw)
        assert out["rc"] != 0 and text in lib.las_last_error(), (kw, out["rc"], lib.las_last_error())
        assert _untouched(out), kw
    assert lib.las_kws_workspace_bytes(1, 8) >= 32


# ---- the Python entry points -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model_and_head():
    """the small f32 model with a CTC head of test_gpu_ctc_search_cli, its encoder outputs and the head's log-probabilities"""
    import test_gpu_ctc_search_cli as C
    args, bs = C._model()
    utts = C._utts(args)
    with torch.no_grad():
        encs, enc_lens, _, h_one, _ = bs._run_encoders(None, utts)
        lp = bs._ctc_log_probs(encs, h_one)
    torch.cuda.synchronize()
    return args, bs, encs, enc_lens, h_one, lp


def test_python_entry_points_return_the_raw_calls_hits():
    from las import kws as KW
    args, bs, encs, enc_lens, h_one, lp = _model_and_head()
    rng = np.random.RandomState(6)
    V = args.vocab_size
    assert lp.shape[1] == V + 1
    phrases = [[int(c) for c in rng.randint(2, V, size=L)] for L in (1, 2, 4, 3, 7)]
    kw = KW.KeywordList(phrases, ["w%d" % k for k in range(len(phrases))], vocab_size=V)
    lens = [int(x) for x in enc_lens]
    tpt, H = -50.0, 3
    raw = _launch(lp, lens, phrases, [np.float32(tpt) * np.float32(len(ph)) for ph in phrases], H)
    assert raw["rc"] == 0 and raw["count"][:, :, 0].sum() > 0
    want = []
    for u in range(len(lens)):
        found = [{"keyword": p, "start_frame": int(raw["hit_start"][u, p, k]), "end_frame": int(raw["hit_end"][u, p, k]),
                  "score": float(raw["hit_score"][u, p, k])} for p in range(len(phrases)) for k in range(raw["count"][u, p, 0])]
        want.append(sorted(found, key=lambda h: (h["start_frame"], h["keyword"])))
    a = KW.keyword_search(lp, lens, kw, tpt, max_hits=H)
    b = KW.keyword_search(lp, lens, kw, tpt, max_hits=H, series=True, series_bytes=1)             # one phrase per call: chunks
    c = bs.keyword_search(encs, enc_lens, kw, h_one, threshold_per_token=tpt, max_hits=H)        # runs the head itself
    d = bs.keyword_search(encs, enc_lens, kw, h_one, ctc_lp=lp, threshold_per_token=tpt, max_hits=H, series=True)
    for r in (a, b, c, d):
        assert r.hits == want
        assert np.array_equal(r.best_score, raw["best_score"]) and np.array_equal(r.best_span, raw["best_span"])
        assert np.array_equal(r.count, raw["count"])
    assert a.end_score is None and c.end_start is None
    for r in (b, d):
        assert np.array_equal(r.end_score, raw["end_score"]) and np.array_equal(r.end_start, raw["end_start"])
    # seconds, by the stated rule
    frame_s, duration = 0.04, 0.5
    timed = KW.timed_hits(want[0], kw, frame_s, duration)
    assert len(timed) == len(want[0]) > 0
    for h, t in zip(want[0], timed):
        L = len(phrases[h["keyword"]])
        assert t == {"keyword": "w%d" % h["keyword"], "start": h["start_frame"] * frame_s, "end": min((h["end_frame"] + 1) * frame_s, duration),
                     "score": h["score"], "confidence": math.exp(h["score"] / L)}    # what the entry points refuse
    with pytest.raises(ValueError, match="max_hits"):
        KW.keyword_search(lp, lens, kw, tpt, max_hits=9)
    with pytest.raises(ValueError, match="the blank"):
        KW.keyword_search(lp, lens, KW.KeywordList([[V]]), tpt)
    args.ctc = False
    try:
        with pytest.raises(ValueError, match="needs the CTC head"):
            bs.keyword_search(encs, enc_lens, kw, h_one)
    finally:
        args.ctc = True
