"""Attention coverage: las_coverage_step and las_coverage_rows against the numpy restatement (tests/coverage_ref.py) bit
for bit, decode_batch against the CPU search with the coverage gain, the counts and the score identity of every returned hypothesis,
the mode equivalences, the second pass' ranking and the command lines."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import coverage_ref as CR
from helpers import PKG, _oracle_fns, make_args, oracle_score_tokens, synthetic_batch

pytestmark = pytest.mark.gpu
SENT = 7.0                      # sentinel of what the kernel must not write
EOS = 2
WC, WO = 0.3, 0.7               # not float32-exact: the two products and their difference each round
f32 = np.float32


def _bits_equal(got, want):
    """the same float32 bits; where the expectation is a NaN any NaN passes (a NaN's payload is not part of the semantics)"""
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan])


# ---- 1. the kernels -----------------------------------------------------------------------------------------------------------------
def _width(Tp):
    return 4 * ((Tp + 2 + 3) // 4)


def _step(alphas, enc_len, par, score, t, nlive, done, dec_step, Umax, n, beam, W, w_c=WC, w_o=WO, tau=0.5, kappa=1.5):
    """one las_coverage_step launch over sentinel-filled outputs -> (cur [N, W], score [N], hist [Umax, N, 2]) as numpy"""
    from las import _hip
    N, Tp = alphas.shape
    d = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x), dtype=dt).cuda()
    i32 = torch.int32
    al, el, pr, sc = d(alphas, torch.float32), d(enc_len, i32), d(par, torch.float32), d(score, torch.float32)
    cur = torch.full((N, W), SENT, device="cuda")
    hist = torch.full((max(Umax, 1), N, 2), SENT, device="cuda")
    keep = [d(np.zeros(N), i32), d([t, 0], i32), d(nlive, i32), d(done, i32), d(dec_step, i32)]
    rc = _hip.lib().las_coverage_step(_hip.p(al), _hip.p(el), n, beam, Tp, _hip.p(sc), w_c, w_o, tau, kappa, _hip.p(hist), _hip.p(pr), _hip.p(cur),
                                      W, *[_hip.p(x) for x in keep], Umax, _hip.stream())
    _hip.check(rc, "las_coverage_step")
    torch.cuda.synchronize()
    return cur.cpu().numpy(), sc.cpu().numpy(), hist.cpu().numpy()


def _expect(alphas, enc_len, par, score, t, nlive, done, dec_step, Umax, n, beam, W, w_c=WC, w_o=WO, tau=0.5, kappa=1.5):
    """numpy: a live row's parent state (zeros at step 0) advanced by the row's alignment, its counts recorded, one float32 add of the
    gain to its running sum (none with zero weights); every other row keeps its bytes"""
    N, Tp = alphas.shape
    cur, sc, hist = np.full((N, W), SENT, f32), np.array(score, f32, copy=True), np.full((max(Umax, 1), N, 2), SENT, f32)
    for u in range(n):
        for j in range(beam):
            r = u * beam + j
            if t >= Umax or done[u] or t >= dec_step[u] or j >= (1 if t == 0 else nlive[u]):
                continue
            st = CR.empty_state(Tp) if t == 0 else (par[r, :Tp], par[r, Tp], par[r, Tp + 1])
            (cum, c, o), dc, do = CR.advance(st, alphas[r], enc_len[r], tau, kappa)
            cur[r, :Tp], cur[r, Tp], cur[r, Tp + 1], cur[r, Tp + 2:] = cum, c, o, 0.0
            hist[t, r] = (c, o)
            if f32(w_c) != 0 or f32(w_o) != 0:
                sc[r] = f32(sc[r] + CR.gain(w_c, w_o, dc, do))
    return cur, sc, hist


def _case(Tp, n, beam, seed):
    """alignments around 1 / 3 per frame and parents around the thresholds, so one step crosses tau and kappa in many frames; enc_len
    per row cycles through 0, 1, Tp - 1, Tp; the parents' counts are what their cum values give"""
    rng = np.random.RandomState(seed)
    N, W = n * beam, _width(Tp)
    alphas = (rng.rand(N, Tp) * 0.7).astype(f32)
    enc_len = np.array([(0, 1, Tp - 1, Tp)[(r + seed) % 4] for r in range(N)], np.int32)
    par = np.full((N, W), 123.0, f32)
    par[:, :Tp] = (rng.rand(N, Tp) * 1.8).astype(f32)
    for r in range(N):
        L = min(max(int(enc_len[r]), 0), Tp)
        par[r, Tp], par[r, Tp + 1] = np.count_nonzero(par[r, :L] > f32(0.5)), np.count_nonzero(par[r, :L] > f32(1.5))
    score = (rng.randn(N) * 3.0).astype(f32)
    return alphas, enc_len, par, score, W


@pytest.mark.parametrize("beam", [1, 4, 16])
@pytest.mark.parametrize("Tp", [1, 3, 4, 63, 64, 65, 257, 1023])
def test_coverage_step_matches_numpy_bit_for_bit(Tp, beam):
    """cur, the counts (state row and record) and score of every row, by bits: a step > 0 from valid parents; a NaN and an inf
    alignment; step 0 over a garbage parent; every way a row is not live (untouched rows keep the sentinel); zero weights (counts
    kept, score untouched); a state row that is no multiple of 16 bytes; two launches give the same bits"""
    n = 3
    N = n * beam
    alphas, enc_len, par, score, W = _case(Tp, n, beam, Tp + beam)
    live = dict(t=1, nlive=[beam] * n, done=[0] * n, dec_step=[1000] * n, Umax=8)
    base = dict(n=n, beam=beam, W=W)

    def check(alphas, enc_len, par, score, **kw):
        kw = dict(base, **dict(live, **kw))
        got = _step(alphas, enc_len, par, score, **kw)
        want = _expect(alphas, enc_len, par, score, **kw)
        for name, g, w in zip(("cur", "score", "hist"), got, want):
            assert _bits_equal(g, w), (name, kw, np.argwhere(g != w)[:6].tolist())
        return got, want

    got, want = check(alphas, enc_len, par, score)
    if Tp >= 63:
        assert np.any(want[0][:, Tp] != par[:, Tp]) and not _bits_equal(want[1], score)      # (the expectation is no identity)
    again = _step(alphas, enc_len, par, score, **dict(base, **live))
    assert all(_bits_equal(a, g) for a, g in zip(again, got))
    # a NaN and an inf alignment: the NaN never counts, the inf counts twice; a frame behind enc_len neither
    a2 = alphas.copy()
    a2[0, 0], a2[N - 1, Tp - 1] = np.nan, np.inf
    a2[N // 2, Tp // 2] = np.inf
    check(a2, np.full(N, Tp, np.int32), par, score)
    check(a2, enc_len, par, score)
    # step 0: slot 0 of every utterance only, from zeros whatever the parent holds
    garbage = np.full_like(par, np.nan)
    garbage[:, 1::2] = -3.0e38
    got0, want0 = check(alphas, enc_len, garbage, score, t=0)
    assert np.all(want0[0][::beam, Tp] >= 0)
    # liveness
    check(alphas, enc_len, par, score, nlive=[beam, min(2, beam), 0])
    check(alphas, enc_len, par, score, done=[0, 1, 0])
    check(alphas, enc_len, par, score, dec_step=[1000, 1, 2])
    got5, _ = check(alphas, enc_len, par, score, t=5, Umax=5)
    assert np.all(got5[0] == SENT) and _bits_equal(got5[1], score)
    # report only: the counts, and not a bit of the running sums
    gotz, _ = check(alphas, enc_len, par, score, w_c=0.0, w_o=0.0)
    assert _bits_equal(gotz[1], score) and _bits_equal(gotz[0], got[0])
    # one weight alone; enc_len outside [0, Tp] is clamped
    check(alphas, enc_len, par, score, w_o=0.0)
    check(alphas, np.where(np.arange(N) % 2 == 0, -5, Tp + 9).astype(np.int32), par, score, w_c=0.0)
    # rows of W + 1 floats: not whole 16-byte groups
    par1 = np.concatenate([par, np.full((N, 1), 55.0, f32)], 1)
    check(alphas, enc_len, par1, score, W=W + 1)


@pytest.mark.parametrize("Tp,beam", [(3, 4), (65, 4), (257, 16)])
def test_three_chained_steps_through_a_host_side_gather(Tp, beam):
    """steps 0, 1, 2 with the survivors' rows gathered on the host in between, as las_beam_loop_step gathers them; las_coverage_rows
    gives every final row's counts from its ancestry's alignments"""
    from las import coverage
    n, tau, kappa = 3, 0.5, 1.0
    N, W = n * beam, _width(Tp)
    rng = np.random.RandomState(Tp)
    enc_len = np.repeat(np.array([Tp, max(Tp - 1, 0), 1], np.int32), beam)
    live = dict(nlive=[beam] * n, done=[0] * n, dec_step=[1000] * n, Umax=3, n=n, beam=beam, W=W, tau=tau, kappa=kappa)
    par_d = par_h = np.zeros((N, W), f32)
    sc_d = sc_h = np.zeros(N, f32)
    path = np.zeros((3, N), np.int64)                                  # the row a final row's ancestor occupied at step t
    alphas = (rng.rand(3, N, Tp) * 0.9).astype(f32)
    for t in range(3):
        cur_d, sc_d, hist_d = _step(alphas[t], enc_len, par_d, sc_d, t=t, **live)
        cur_h, sc_h, hist_h = _expect(alphas[t], enc_len, par_h, sc_h, t=t, **live)
        assert _bits_equal(cur_d, cur_h) and _bits_equal(sc_d, sc_h) and _bits_equal(hist_d[t], hist_h[t])
        if t == 2:
            break
        # the gather: every slot takes a surviving row of its own utterance (at step 0 only slot 0 has one)
        src = np.concatenate([u * beam + (np.zeros(beam, np.int64) if t == 0 else rng.randint(0, beam, beam)) for u in range(n)])
        path[:t + 1] = path[:t + 1, src]
        path[t] = src
        par_d, par_h, sc_d, sc_h = cur_d[src], cur_h[src], sc_d[src], sc_h[src]
    path[2] = np.arange(N)
    own = np.stack([alphas[t, path[t]] for t in range(3)])             # [3, N, Tp]: every final row's own alignments
    counts = coverage.rows_counts(torch.as_tensor(own).cuda(), np.full(N, 3), enc_len, tau, kappa).cpu().numpy()
    assert np.array_equal(counts, cur_d[:, Tp:Tp + 2].astype(np.int32))
    assert np.any(counts[:, 1] > 0) and np.any(counts[:, 0] > counts[:, 1])


@pytest.mark.parametrize("U", [1, 2, 7])
def test_coverage_rows_matches_numpy(U):
    from las import coverage
    rng = np.random.RandomState(U)
    for Tp, R in ((1, 3), (64, 5), (257, 4), (1023, 2)):
        alphas = (rng.rand(U, R, Tp) * 0.6).astype(f32)
        if Tp > 1:
            alphas[0, 0, 1] = np.nan
        alphas[U - 1, R - 1, 0] = np.inf
        steps = np.array([(U, 0, U - 1, U + 3, -2)[r % 5] for r in range(R)])
        enc_len = np.array([(Tp, Tp - 1, 1, Tp + 4, 0)[(r + 1) % 5] for r in range(R)])
        got = coverage.rows_counts(torch.as_tensor(alphas).cuda(), steps, enc_len, 0.5, 1.5).cpu().numpy()
        for r in range(R):
            k = min(max(int(steps[r]), 0), U)
            want = CR.counts(list(alphas[:k, r]), enc_len[r], 0.5, 1.5) if k else (0, 0)
            assert tuple(got[r]) == want, (Tp, r, k, got[r], want)


def test_entry_points_refuse_bad_arguments():
    from las import _hip
    z, z2 = torch.zeros(64, device="cuda"), torch.zeros(64, device="cuda")
    zi = torch.zeros(64, dtype=torch.int32, device="cuda")

    def call(w_c=0.3, w_o=0.7, tau=0.5, kappa=1.5, W=8, st_out=z2, Tp=4):
        return _hip.lib().las_coverage_step(_hip.p(z), _hip.p(zi), 1, 2, Tp, _hip.p(z), w_c, w_o, tau, kappa, None, _hip.p(z), _hip.p(st_out), W,
                                            _hip.p(zi), _hip.p(zi), _hip.p(zi), _hip.p(zi), _hip.p(zi), 4, _hip.stream())
    for kw, msg in ((dict(w_c=-1.0), b"weights"), (dict(w_o=float("nan")), b"weights"), (dict(w_c=float("inf")), b"weights"),
                    (dict(tau=0.0), b"thresholds"), (dict(kappa=0.5), b"thresholds"), (dict(tau=float("nan")), b"thresholds"),
                    (dict(W=5), b"state_width"), (dict(st_out=z), b"differ"), (dict(Tp=0), b"bad dims")):
        assert call(**kw) < 0 and msg in _hip.lib().las_last_error(), kw
    assert _hip.lib().las_coverage_rows(_hip.p(z), 1, 2, 4, _hip.p(zi), _hip.p(zi), 0.5, 0.5, _hip.p(zi), _hip.stream()) < 0
    assert b"thresholds" in _hip.lib().las_last_error()
    assert _hip.lib().las_coverage_rows(_hip.p(z), 0, 2, 4, _hip.p(zi), _hip.p(zi), 0.5, 1.5, _hip.p(zi), _hip.stream()) < 0
    torch.cuda.synchronize()


# ---- 2. the search against the CPU search -------------------------------------------------------------------------------------------
# tau and kappa of the searches below: the small random-weight model attends almost evenly (an alignment is ~ 1 / T' per frame, T' = 10
# to 16) and its hypotheses are one or two tokens long, so the thresholds that a hypothesis crosses lie near 0.1 and 0.2.  Chosen on
# the CPU reference alone: with them every utterance below passes the margin condition for both vocabulary sizes.
TAU, KAPPA = 0.1, 0.2
FRAMES = (64, 48, 56, 40)


def _norm(h):
    return float(h.log_prob) / (len(h.token_ids) - 1)


def _hyps(res):
    return [[(list(h.token_ids), float(h.log_prob), h.coverage) for h in r] for r in res]


@functools.lru_cache(maxsize=None)
def _reference(V):
    """the CPU side, computed once per vocabulary size and left unchanged: per utterance the oracle's functions, its plain search and
    the search with the coverage gain (with the least distance of a counted cum value from a threshold)"""
    import test_gpu_ctc_decode as D
    from oracle import las_oracle as O
    args, p0, bs = D._model("pblstm", "lstm", ctc_decode_weight=0.0, vocab_size=V)
    utts = [synthetic_batch(1, T, 12, V, seed=8 + k)[0] for k, T in enumerate(FRAMES)]
    fns = [_oracle_fns(xs, p0, args, "lstm", None) for xs in utts]
    plain = [O.beam_search(f[0], f[3], f[4], f[5], 4, 1, EOS) for f in fns]
    refs = [CR.covered_beam_search(f[0], f[3], f[4], f[5], 4, 1, EOS, f[4], WC, WO, TAU, KAPPA) for f in fns]
    return dict(args=args, p0=p0, utts=utts, fns=fns, plain=plain, refs=refs)


def _search(V):
    """a fresh model on the device (the variable store is global: another test may have replaced it)"""
    import test_gpu_ctc_decode as D
    return D._model("pblstm", "lstm", ctc_decode_weight=0.0, vocab_size=V)[2]


@pytest.mark.parametrize("V", [30, 5000])
def test_decode_batch_matches_the_cpu_search_with_coverage(V):
    """f32 parity mode, char and subword vocabulary sizes.  An utterance is compared only if, on the CPU reference alone, no cum value
    of any hypothesis in any step's bank lies within 1e-4 of tau or kappa (the device's alignments differ from the oracle's in the last
    bits, and a count is a step function of them): a condition, not a tolerance.  At most a quarter of the utterances may be left out,
    and the weights must change the reference's best hypothesis of a compared utterance.  Tokens and counts exactly, scores within the
    f32 search tolerance of test_gpu_bias.py (5e-3)."""
    ref = _reference(V)
    compared = [m >= 1e-4 for _, m in ref["refs"]]
    changed = [list(r[-1].token_ids) != list(p[-1].token_ids) for (r, _), p in zip(ref["refs"], ref["plain"])]
    print("reference: margins", [m for _, m in ref["refs"]], "compared", compared, "changed", changed)
    assert len(compared) - sum(compared) <= len(compared) // 4
    assert any(c and d for c, d in zip(compared, changed))
    bs = _search(V)
    bs.set_coverage(WC, WO, TAU, KAPPA)
    batch = bs.decode_batch(None, ref["utts"])
    assert all(batch)
    some_over = False
    for u, (res, (want, _)) in enumerate(zip(batch, ref["refs"])):
        if not compared[u]:
            continue
        Tp = ref["fns"][u][4]
        got_best, ref_best = res[-1], want[-1]
        print("device", list(got_best.token_ids), float(got_best.log_prob), got_best.coverage, "reference", list(ref_best.token_ids), float(ref_best.log_prob))
        assert list(got_best.token_ids) == list(ref_best.token_ids)
        assert got_best.coverage == (int(ref_best.dec_state[1][1]), int(ref_best.dec_state[1][2]), Tp)
        assert float(got_best.log_prob) == pytest.approx(float(ref_best.log_prob), abs=5e-3)
        by_tokens = {tuple(h.token_ids): h for h in want}
        for h in res:                                                  # every hypothesis the two lists share
            w = by_tokens.get(tuple(h.token_ids))
            if w is not None:
                assert h.coverage[:2] == (int(w.dec_state[1][1]), int(w.dec_state[1][2]))
                assert float(h.log_prob) == pytest.approx(float(w.log_prob), abs=5e-3)
                some_over = some_over or h.coverage[1] > 0
    assert some_over                                                   # (both thresholds were crossed somewhere)
    bs.set_coverage()
    assert bs.coverage is None
    off = bs.decode_batch(None, ref["utts"])
    assert [[list(h.token_ids) for h in r] for r in off] != [[list(h.token_ids) for h in r] for r in batch]
    assert all(h.coverage is None for r in off for h in r)


# ---- 3. every returned hypothesis: its counts and its score ---------------------------------------------------------------------------
def _long_model(prec):
    """one LSTM layer, no raised EOS bias: hypotheses as long as the step bound (19 and 14 tokens), bf16 = the short form of the step"""
    from las import layers as L, variables as Vs
    from las.las import LAS, Listener, Speller
    from las.beam_search import BeamSearch
    from oracle import las_oracle as O
    from utils.tokenizer import CharEncoder
    args = make_args(enc_units=64, num_enc_layers=2, dec_units=64, num_dec_layers=1, embedding_size=32, attention_size=32, beam_size=4,
                     convert_rate=0.3, apply_lm=False)
    p0 = O.init_params(args, seed=11, cell="lstm")
    L.set_cell("lstm")
    L.set_precision(prec)
    st = Vs.reset_default_store(device="cuda")
    st.load(p0)
    las = LAS(args, Listener, Speller, CharEncoder().token_to_id)
    las.build_variables()
    utts = [synthetic_batch(1, T, 12, 30, seed=8 + k)[0] for k, T in enumerate((64, 48))]
    return args, p0, BeamSearch(args, las, CharEncoder().token_to_id, None), utts


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_every_hypothesis_counts_and_score_identity(prec):
    """counts = the numpy recomputation from the hypothesis' own alignments, exactly (and las_coverage_rows gives them too); log_prob =
    the oracle's unscored teacher-forced sum + the float32 gains of those alignments, within the tolerance test_gpu_bias.py uses for
    its bonus identity (5e-3 + 1e-4 |want|)"""
    from las import coverage, layers as L
    tau, kappa = 0.5, 1.0
    try:
        args, p0, bs, utts = _long_model(prec)
        bs.set_coverage(WC, WO, tau, kappa)
        batch = bs.decode_batch(None, utts)
        assert all(batch)
        worst, seen = 0.0, set()
        for xs, res in zip(utts, batch):
            for h in res:
                ids = list(h.token_ids)
                atts = [a.cpu().numpy() for a in h.att]
                assert len(atts) == len(ids) and not atts[0].any()
                covered, over, frames = h.coverage
                assert frames == atts[0].shape[0] and 0 <= over <= covered <= frames
                assert (covered, over) == CR.counts(atts[1:], frames, tau, kappa)
                own = torch.stack([a for a in h.att[1:]]).unsqueeze(1).contiguous()            # [len, 1, T']
                assert tuple(coverage.rows_counts(own, [len(ids) - 1], [frames], tau, kappa).cpu().numpy()[0]) == (covered, over)
                want, _ = oracle_score_tokens(xs, p0, args, "lstm", ids, prec=prec)
                want += float(np.sum(CR.gains(atts[1:], frames, WC, WO, tau, kappa).astype(np.float64)))
                worst = max(worst, abs(float(h.log_prob) - want))
                print(prec, len(ids) - 1, h.coverage, float(h.log_prob), want)
                assert abs(float(h.log_prob) - want) < 5e-3 + 1e-4 * abs(want), (ids, float(h.log_prob), want)
                seen.add((covered > 0, over > 0))
        print("largest |log_prob - (teacher-forced sum + gains)|: %.3g" % worst)
        assert (True, True) in seen                                    # (hypotheses that crossed both thresholds)
    finally:
        L.set_precision("f32")


# ---- 4. modes -------------------------------------------------------------------------------------------------------------------------
def test_batched_single_eager_graph_and_streamed_give_the_same_bits():
    ref = _reference(30)
    bs, utts = _search(30), ref["utts"]
    bs.set_coverage(WC, WO, TAU, KAPPA)
    batch = _hyps(bs.decode_batch(None, utts))
    assert all(batch) and all(c is not None for r in batch for _, _, c in r)
    assert _hyps([bs.decode(None, xs) for xs in utts]) == batch
    bs.use_graph = False
    try:
        assert _hyps(bs.decode_batch(None, utts)) == batch
    finally:
        bs.use_graph = True
    streamed = [r for res in bs.decode_batches(None, [utts[:2], utts[2:]]) for r in res]
    assert _hyps(streamed) == batch


def test_report_only_is_the_plain_search_and_the_short_form_stays():
    """bf16, one LSTM layer: the step is the short form without the flags, with a report and with weights; the report leaves tokens and
    scores bit-identical and adds the counts; "coverage" is a part of the step's timing"""
    from las import layers as L
    try:
        args, p0, bs, utts = _long_model("bf16")
        bs.measure = True
        off = bs.decode_batch(None, utts)
        assert bs.last_timing["short_form"] is True and set(bs.last_timing["parts_us"]) == {"speller", "beam"}
        bs.set_coverage(report=True)
        rep = bs.decode_batch(None, utts)
        parts = dict(bs.last_timing["parts_us"])
        assert bs.last_timing["short_form"] is True and set(parts) == {"speller", "coverage", "beam"} and parts["coverage"] > 0
        plain = lambda res: [[(list(h.token_ids), float(h.log_prob)) for h in r] for r in res]
        assert plain(rep) == plain(off)
        assert all(h.coverage is not None for r in rep for h in r) and all(h.coverage is None for r in off for h in r)
        bs.set_coverage(WC, WO, 0.5, 1.0)
        on = bs.decode_batch(None, utts)
        assert bs.last_timing["short_form"] is True and set(bs.last_timing["parts_us"]) == {"speller", "coverage", "beam"}
        assert plain(on) != plain(off)
        bs.set_coverage()
        bs.measure = False
        assert plain(bs.decode_batch(None, utts)) == plain(off)
    finally:
        L.set_precision("f32")


# ---- 5. the second pass ---------------------------------------------------------------------------------------------------------------
def test_rescoring_ranks_by_the_attention_score_with_the_coverage_term():
    """--rescore attention with a coverage setting: every listed hypothesis carries its counts; total and order are the restatement's
    from the returned att_score, the first-pass score and the counts; the counts are those of the plain report"""
    import rescore_ref as R
    import test_gpu_ctc_search_cli as C
    w, tau, kappa = 0.3, 0.1, 0.2
    args, bs = C._model(rescore="attention", rescore_ctc_weight=w)
    utts = C._utts(args)
    base = bs.ctc_decode_batch(None, utts)
    assert all("coverage" not in d for r in base.rescored for d in r)
    bs.set_coverage(2.0 * WC, WO, tau, kappa)
    res = bs.ctc_decode_batch(None, utts)
    any_counts = False
    for u, r in enumerate(res):
        resc = list(reversed(res.rescored[u]))                          # best first
        K = len(resc)
        first, att = np.zeros(K, np.float32), np.zeros(K, np.float64)
        for h, d in zip(reversed(r), resc):
            covered, over, frames = d["coverage"]
            assert h.coverage == d["coverage"] and 0 <= over <= covered <= frames
            any_counts = any_counts or covered > 0
            g = float(f32(f32(2.0 * WC) * f32(covered))) - float(f32(f32(WO) * f32(over)))
            assert d["att"] == d["att_score"] + g                      # (float64 sums of the two float32 products)
            first[d["first_rank"]], att[d["first_rank"]] = d["first"], d["att"]
        tot, order = R.rank(first, att, w)
        assert [d["first_rank"] for d in resc] == order
        for h, d in zip(reversed(r), resc):
            assert float(h.log_prob) == d["total"] and abs(d["total"] - float(tot[d["first_rank"]])) <= 4.0 * R.measured_tolerance()[1]
        # the unscored attention scores are those of the search without the setting
        plain = {d["first_rank"]: d["att"] for d in base.rescored[u]}
        assert all(d["att_score"] == plain[d["first_rank"]] for d in resc)
    assert any_counts


# ---- 6. command lines -----------------------------------------------------------------------------------------------------------------
MODEL = ["--unit", "char", "--feat_dim", "13", "--enc_type", "pblstm", "--enc_units", "64", "--num_enc_layers", "2", "--dec_units", "64",
         "--num_dec_layers", "1", "--attention_size", "32", "--embedding_size", "32", "--cell", "lstm", "--beam_size", "4"]


def test_transcribe_cli_reports_coverage(tmp_path):
    cmd = [sys.executable, os.path.join(PKG, "transcribe.py"), "--synthetic", "True", "--max_steps", "3", "--save_dir", str(tmp_path / "none"),
           "--coverage_report", "True", "--nbest", "2"] + MODEL
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 3
    for ln in lines:
        o = json.loads(ln)
        assert set(o) >= {"text", "score", "coverage", "overattended", "nbest"}
        for e in [o] + o["nbest"]:
            assert 0.0 <= e["overattended"] <= e["coverage"] <= 1.0


def test_decode_cli_with_a_coverage_weight(tmp_path):
    cmd = [sys.executable, os.path.join(PKG, "decode.py"), "--synthetic", "True", "--save_dir", str(tmp_path / "none"),
           "--coverage_weight", "0.3", "--overattend_weight", "0.7"] + MODEL
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0 and "Dev WER" in r.stdout and "Coverage: " in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
