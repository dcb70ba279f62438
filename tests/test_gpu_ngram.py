"""N-gram LM shallow fusion: las_ngram_step against the numpy restatement (tests/ngram_ref.py) bit for bit, its refusals,
decode_batch against the CPU search with the LM fused (alone, with the CTC scores, and with CTC and a hotword context), off = today's
search, and the command lines."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bias_ref as B
import ngram_ref as G
from helpers import PKG, oracle_score_tokens, synthetic_batch

pytestmark = pytest.mark.gpu
SENT = 7.0                      # canary of rows the kernel must not write
SOS, EOS, PAD = 1, 2, 0


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------------------
CHAIN = (3, 4, 6)               # the full-depth context is its last order - 1 tokens; token 7 is stored at EVERY level of that chain
WIDE = 5                        # node (5,) has more children than a workgroup has lanes (where V allows: V >= 257)


def _kernel_model(V, order, rng):
    grams = G.random_model(rng, V, order)
    lp = lambda: -float(rng.uniform(0.05, 3.0))
    if order > 1:
        ctx = CHAIN[-(order - 1):]
        for k in range(len(ctx)):                         # every suffix of the context, with its prefixes, is a node; each holds token 7
            for j in range(k + 1, len(ctx) + 1):
                grams.setdefault(ctx[k:j], (lp(), -float(rng.uniform(0.1, 1.0))))
            grams[ctx[k:] + (7,)] = (lp(), -0.25 if order > len(ctx) - k + 1 else 0.0)
        for v in range(min(V, 300)):
            grams.setdefault((WIDE, v), (lp(), 0.0 if order == 2 else -0.125))
        grams[(SOS, 9)] = (lp(), 0.0)
    return grams


def _launch(lm, w, V, scores, st_vals, tokens, t, nlive, done, dec_step, Umax, n, beam, W):
    from las import _hip
    N = n * beam
    d = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x), dtype=dt).cuda()
    i32 = torch.int32
    tab = lm.to("cuda", w)
    sc = d(scores, torch.float32)
    st_in = torch.full((N, W), 123.0, device="cuda")
    st_in[:, 0] = d(st_vals, torch.float32)
    st_out = torch.full((N, W), SENT, device="cuda")
    keep = [d(tokens, i32), d([t, 0], i32), d(nlive, i32), d(done, i32), d(dec_step, i32)]
    rc = _hip.lib().las_ngram_step(_hip.p(tab["child_off"]), _hip.p(tab["child_tok"]), _hip.p(tab["child_lp"]), _hip.p(tab["child_next"]),
                                   _hip.p(tab["bow"]), _hip.p(tab["bo"]), _hip.p(tab["uni_lp"]), _hip.p(tab["uni_next"]), lm.num_nodes,
                                   lm.num_entries, lm.order, _hip.p(sc), n, beam, V, _hip.p(st_in), _hip.p(st_out), W,
                                   *[_hip.p(x) for x in keep], Umax, _hip.stream())
    _hip.check(rc, "las_ngram_step")
    torch.cuda.synchronize()
    return sc.cpu().numpy(), st_out.cpu().numpy()


def _same_bits(got, want):
    return np.array_equal(np.asarray(got, np.float32).view(np.int32), np.asarray(want, np.float32).view(np.int32))


@pytest.mark.parametrize("order", [1, 2, 3, 4])
@pytest.mark.parametrize("V", [30, 257, 5000])
def test_ngram_step_matches_numpy_bit_for_bit(V, order):
    """Advanced node and every score of every row, by bytes; a node <-> its history through the model's node list.  One launch covers:
    SOS entering from the root; a chain of full depth whose every level stores token 7 (the deepest wins); node (5,) with 257 / 300
    children (V >= 257); contexts that back off through missing suffixes; random nodes and tokens; -inf and -0 entries.  Further launches:
    parent values -1, M, 2^30, NaN and entering tokens -1 and V; step 0; nlive / done / dec_step / Umax liveness (untouched rows keep
    their bytes, the state its canary); two launches give the same bytes.  Order 1 is M = 1, E = 0."""
    from las.ngram import NgramLM
    n, beam = 3, 4
    N = n * beam
    rng = np.random.RandomState(100 * order + V)
    grams = _kernel_model(V, order, rng)
    lm = NgramLM(grams, order, V, SOS, EOS, PAD)
    w = 0.7
    ids = {t: i for i, t in enumerate(lm.nodes)}
    M = lm.num_nodes
    assert (M, lm.num_entries) == (1, 0) if order == 1 else M > V
    ctx = CHAIN[-(order - 1):] if order > 1 else ()
    rows = [((), SOS), (ctx[:-1], ctx[-1] if ctx else 3), ((), WIDE), (ctx[:-1], 9), ((SOS,) if order > 1 else (), 9)]
    kids = {}
    for key in grams:
        kids.setdefault(key[:-1], []).append(key[-1])
    while len(rows) < N:                                                # random nodes, entering tokens that follow them or not
        par = lm.nodes[rng.randint(M)]
        c = kids.get(par) if par else None
        rows.append((par, int(c[rng.randint(len(c))]) if (c and rng.rand() < 0.7) else int(rng.randint(V))))
    parents = [r[0] for r in rows]
    tokens = np.array([r[1] for r in rows])
    st_vals = np.array([ids[p] for p in parents], np.float32)
    scores = (rng.randn(N, V) * 3.0).astype(np.float32)
    scores[rng.rand(N, V) < 0.02] = -np.inf
    scores[:, 7] = np.where(rng.rand(N) < 0.3, -np.inf, scores[:, 7])
    scores[0, 3] = -0.0
    live = dict(t=1, nlive=[beam] * n, done=[0] * n, dec_step=[1000] * n, Umax=1000)
    args = dict(n=n, beam=beam, W=4)
    cache = {}

    def expect(parents, tokens, t, nlive, done, dec_step, Umax, n, beam, W):
        sc = np.array(scores, np.float32, copy=True)
        st = np.full((n * beam, W), SENT, np.float32)
        for u in range(n):
            for j in range(beam):
                r = u * beam + j
                if t >= Umax or done[u] or t >= dec_step[u] or j >= (1 if t == 0 else nlive[u]):
                    continue
                hist = (() if (t == 0 or parents[r] is None) else parents[r]) + (int(tokens[r]),)
                state = G.state_of(grams, order, hist)
                st[r, 0] = ids[state]
                if state not in cache:
                    cache[state] = G.row_gains32(grams, order, w, hist, V)
                sc[r] = G.apply_row(sc[r], cache[state])
        return sc, st

    def check(parents, st_vals, tokens, **kw):
        kw = dict(args, **dict(live, **kw))
        got = _launch(lm, w, V, scores, st_vals, tokens, **kw)
        want = expect(parents, tokens, **kw)
        assert _same_bits(got[1], want[1]), (got[1][:, 0], want[1][:, 0])
        bad = np.nonzero(got[0].view(np.int32) != want[0].view(np.int32))
        assert bad[0].size == 0, (bad[0][:8], bad[1][:8], got[0][bad][:8], want[0][bad][:8])
        return got, want

    got, want = check(parents, st_vals, tokens)
    assert np.all(np.isneginf(got[0][np.isneginf(scores)])) and not _same_bits(want[0], scores)
    if order > 1:
        assert want[1][1, 0] == ids[ctx] and len(lm.nodes[int(want[1][1, 0])]) == order - 1         # the chain of full depth ...
        deep, shallow = grams[ctx + (7,)][0], grams[ctx[1:] + (7,)][0]
        if np.isfinite(scores[1, 7]):                                                                # ... and its token 7: the deeper entry
            assert got[0][1, 7] == np.float32(scores[1, 7] + G.scaled(w, deep)) and deep != shallow
        assert want[1][2, 0] == ids[(WIDE,)]
        fan = int(lm.child_off[ids[(WIDE,)] + 1] - lm.child_off[ids[(WIDE,)]])
        assert fan == min(V, 300) and (fan > 256 or V == 30)
    again = _launch(lm, w, V, scores, st_vals, tokens, **dict(args, **live))
    assert _same_bits(again[0], got[0]) and _same_bits(again[1], got[1])
    # values that are no node behave as the root; entering tokens outside [0, V) go to the root
    p2 = [None, None, None, None, None] + parents[5:]
    s2 = np.array([-1.0, M, 2.0 ** 30, np.nan, np.inf] + list(st_vals[5:]), np.float32)
    t2 = np.array([WIDE, WIDE, 7, WIDE, 7, -1, V, 2 ** 30, -2 ** 31] + list(tokens[9:]))
    check(p2, s2, t2)
    # liveness: step 0 (only j = 0, from the root, garbage in state_in), then every way a row is not live; one float per state row
    check(parents, st_vals, np.full(N, SOS), t=0, W=1)
    check(parents, st_vals, tokens, nlive=[beam, 2, 0])
    check(parents, st_vals, tokens, done=[0, 1, 0], W=1)
    check(parents, st_vals, tokens, dec_step=[1000, 1, 2])
    got, _ = check(parents, st_vals, tokens, t=5, Umax=5)
    assert _same_bits(got[0], scores) and np.all(got[1] == SENT)


def test_ngram_step_refusals():
    """one refusal per argument check, before anything is launched"""
    from las import _hip
    from las.ngram import NgramLM
    lm = NgramLM(_kernel_model(30, 2, np.random.RandomState(0)), 2, 30)
    tab = lm.to("cuda", 1.0)
    z = torch.zeros(64, device="cuda")
    zi = torch.zeros(64, dtype=torch.int32, device="cuda")
    z2 = torch.zeros(64, device="cuda")

    def call(M=lm.num_nodes, E=lm.num_entries, order=2, V=30, st_in=z, st_out=z2, W=1, tok=tab["child_tok"], uni=tab["uni_lp"], nutt=1):
        return _hip.lib().las_ngram_step(_hip.p(tab["child_off"]), _hip.p(tok), _hip.p(tab["child_lp"]), _hip.p(tab["child_next"]),
                                         _hip.p(tab["bow"]), _hip.p(tab["bo"]), _hip.p(uni), _hip.p(tab["uni_next"]), M, E, order,
                                         _hip.p(z), nutt, 2, V, _hip.p(st_in), _hip.p(st_out), W, _hip.p(zi), _hip.p(zi), _hip.p(zi),
                                         _hip.p(zi), _hip.p(zi), 4, _hip.stream())
    for kw, msg in ((dict(uni=None), b"null pointer"), (dict(tok=None), b"child tables"), (dict(E=-1), b"child tables"),
                    (dict(nutt=0), b"bad dims"), (dict(V=1), b"V <="), (dict(V=16385), b"V <="), (dict(M=0), b"nodes"),
                    (dict(M=(1 << 22) + 1), b"nodes"), (dict(order=0), b"order"), (dict(order=7), b"order"), (dict(W=0), b"state_width"),
                    (dict(st_out=z), b"differ")):
        assert call(**kw) < 0 and msg in _hip.lib().las_last_error(), kw
    assert call() == 0
    torch.cuda.synchronize()


# ---- 2. the search ------------------------------------------------------------------------------------------------------------------
# The weight of each configuration: the smallest of {0.5, 1, 2, 4} for which, on the CPU reference ALONE, (a) the LM changes the best
# hypothesis of at least one utterance and (b) at least two of the three utterances keep a length-normalised margin >= 0.05 between
# best and second best (DESIGN 7j's margin).  Both are asserted below before the device runs.
WEIGHT = {("pblstm", 0.0): 0.5, ("cnn", 0.3): 0.5}
WEIGHT_COMPOSED = 2.0
DISTRACTORS = [[SOS, 29, 28, 29, 27, EOS], [SOS, 26, 29, 3, 29, 28, EOS], [SOS, 27, 27, 26, EOS]]     # fixed sentences that occur in no hypothesis
ORDER = 3


def _norm(h):
    return float(h.log_prob) / (len(h.token_ids) - 1)


def _trigram(unfused):
    """train_ngram's trigram over the reference's second-best hypotheses (unfused search), as token strings, plus the distractors"""
    sys.path.insert(0, PKG)
    import train_ngram
    from las.ngram import NgramLM
    corpus = []
    for ref in unfused:
        if len(ref) > 1:
            ids = [int(t) for t in ref[-2].token_ids]
            corpus.append(ids if ids[-1] == EOS else ids + [EOS])
    assert corpus
    return NgramLM(train_ngram.estimate(corpus + DISTRACTORS, ORDER, 30, SOS, EOS, PAD), ORDER, 30, SOS, EOS, PAD)


def _preconditions(refs, unfused):
    changed = [list(r[-1].token_ids) != list(u[-1].token_ids) for r, u in zip(refs, unfused)]
    margins = [_norm(r[-1]) - _norm(r[-2]) if len(r) > 1 else np.inf for r in refs]
    print("reference: changed", changed, "margins", margins)
    return sum(changed) >= 1, sum(m >= 0.05 for m in margins) >= 2


def _compare_best(batch, refs):
    near_ties = 0
    for res, ref in zip(batch, refs):
        got_best, ref_best = res[-1], ref[-1]
        print("device", list(got_best.token_ids), float(got_best.log_prob), "reference", list(ref_best.token_ids), float(ref_best.log_prob))
        if list(got_best.token_ids) == list(ref_best.token_ids):
            assert float(got_best.log_prob) == pytest.approx(float(ref_best.log_prob), abs=5e-3)
        else:                                                            # a near tie at the end
            near_ties += 1
            assert abs(_norm(got_best) - _norm(ref_best)) < 5e-3
    assert near_ties <= 1


def _check_scores(utts, batch, fns, p0, args, cell, lam, lm, w, phrases=None, beta=0.0):
    """every returned hypothesis: log_prob = attention score [+ lam log p_ctc, closed hypotheses] + sum of w ln10 logp64 [+ bonus]"""
    import torch.nn.functional as F
    n_checked = 0
    for xs, res, f in zip(utts, batch, fns):
        lp, T = f[4], f[5]
        for h in res:
            ids = list(h.token_ids)
            want, _ = oracle_score_tokens(xs, p0, args, cell, ids)
            if lam > 0:
                if ids[-1] != EOS:
                    continue                                            # (the prefix score of an open hypothesis is no sequence probability)
                labels = ids[1:]
                nll = F.ctc_loss(torch.tensor(lp)[:T, None], torch.tensor([labels]), [T], [len(labels)], blank=args.vocab_size,
                                 reduction="sum").item() if len(labels) <= T else 1e10
                if nll >= 1e9:
                    continue
                want += lam * (-nll)
            want += G.total64(lm.grams, lm.order, w, ids)
            if phrases:
                want += B.bonus(phrases, beta, ids[1:])
            n_checked += 1
            assert abs(float(h.log_prob) - want) < 5e-3 + 1e-4 * abs(want), (ids, float(h.log_prob), want)
    assert n_checked > 0


@pytest.mark.parametrize("enc_type,cell,lam", [("pblstm", "lstm", 0.0), ("cnn", "rnn", 0.3)])
def test_decode_batch_with_ngram_matches_cpu_search(enc_type, cell, lam):
    """decode_batch with the LM against the CPU search whose step function carries the LM's gains (tests/ngram_ref.py; with lam > 0 the
    joint search, so the CTC bank is cut on LM-fused logits); every hypothesis' score is its attention score [+ lam x log p_ctc] + the
    LM's weighted log-probability; batched, one at a time, eager and streamed give the same bits; without the LM the search differs."""
    import test_gpu_bias as TB
    import test_gpu_ctc_decode as D
    args, p0, bs = D._model(enc_type, cell, ctc_decode_weight=lam)
    w = WEIGHT[(enc_type, lam)]
    utts = D._utts(args)
    fns = TB._cpu_fns(utts, p0, args, cell, lam)
    unfused = TB._reference_unbiased(fns, lam)
    lm = _trigram(unfused)
    refs = [G.ngram_beam_search(f[0], f[1], f[2], f[3], 4, SOS, EOS, lm.grams, ORDER, w, f[4], f[5], lam) for f in fns]
    a_ok, b_ok = _preconditions(refs, unfused)
    assert a_ok                                                          # (a) the LM changes a best hypothesis
    assert b_ok                                                          # (b) two of three keep a margin of 0.05

    bs.set_ngram(lm, w)
    batch = bs.decode_batch(None, utts)
    assert all(batch)
    _compare_best(batch, refs)
    _check_scores(utts, batch, fns, p0, args, cell, lam, lm, w)
    assert D._hyps([bs.decode(None, xs) for xs in utts]) == D._hyps(batch)
    bs.use_graph = False
    try:
        assert D._hyps(bs.decode_batch(None, utts)) == D._hyps(batch)
    finally:
        bs.use_graph = True
    streamed = [r for res in bs.decode_batches(None, [utts[:2], utts[2:]]) for r in res]
    assert D._hyps(streamed) == D._hyps(batch)
    # ... and the LM is what made the difference
    bs.set_ngram(None, 0)
    assert D._hyps(bs.decode_batch(None, utts)) != D._hyps(batch)


def test_decode_batch_with_ngram_hotwords_and_ctc_matches_composed_cpu_search():
    """all three on: the CPU search is bias_ref.biased_beam_search (CTC joint scores, then the hotword bonus) over the step function that
    carries the LM's gains -- the order of the device step"""
    import test_gpu_bias as TB
    import test_gpu_ctc_decode as D
    from las.bias import ContextGraph
    enc_type, cell, lam = "pblstm", "lstm", 0.3
    args, p0, bs = D._model(enc_type, cell, ctc_decode_weight=lam)
    w, beta = WEIGHT_COMPOSED, TB.BETA[enc_type]
    utts = D._utts(args)
    fns = TB._cpu_fns(utts, p0, args, cell, lam)
    unfused = TB._reference_unbiased(fns, lam)
    lm = _trigram(unfused)
    phrases = TB._phrases_from(unfused)
    assert len(phrases) > len(TB.DISTRACTORS)
    refs = [G.ngram_beam_search(f[0], f[1], f[2], f[3], 4, SOS, EOS, lm.grams, ORDER, w, f[4], f[5], lam, phrases, beta) for f in fns]
    a_ok, b_ok = _preconditions(refs, unfused)
    assert a_ok
    assert b_ok
    bs.set_ngram(lm, w)
    bs.set_context(ContextGraph(phrases, beta, vocab_size=args.vocab_size))
    batch = bs.decode_batch(None, utts)
    assert all(batch)
    _compare_best(batch, refs)
    _check_scores(utts, batch, fns, p0, args, cell, lam, lm, w, phrases, beta)
    bs.set_context(None)                                                 # the context made a difference on top of the LM, and the LM on top of it
    assert D._hyps(bs.decode_batch(None, utts)) != D._hyps(batch)
    bs.set_context(ContextGraph(phrases, beta, vocab_size=args.vocab_size))
    bs.set_ngram(None, 0)
    assert D._hyps(bs.decode_batch(None, utts)) != D._hyps(batch)


# ---- 3. off means off ---------------------------------------------------------------------------------------------------------------
def _arpa(tmp_path, order=3):
    """an ARPA file over the char vocabulary, written by train_ngram.py"""
    sys.path.insert(0, PKG)
    import train_ngram
    data, out = tmp_path / "text.txt", tmp_path / "lm.arpa"
    data.write_text("ADA LOVELACE\nnew york\nNEW YORK CITY\nTHE CAT SAT ON THE MAT\n")
    train_ngram.main(["--data_file", str(data), "--order", str(order), "--unit", "char", "--output", str(out)])
    return str(out)


def test_off_is_bit_identical(tmp_path):
    """no flag, a file with weight 0, and set_ngram(None, 0) after a fused search: the same hypotheses and scores, by bytes"""
    import test_gpu_ctc_decode as D
    f = _arpa(tmp_path)
    args, p0, bs = D._model("pblstm", "lstm", ctc_decode_weight=0.0)
    utts = D._utts(args)
    plain = D._hyps(bs.decode_batch(None, utts))
    assert any(plain) and bs.ngram is None
    args, p0, bs0 = D._model("pblstm", "lstm", ctc_decode_weight=0.0, ngram_lm=f, ngram_weight=0.0)
    assert bs0.ngram is None
    assert D._hyps(bs0.decode_batch(None, utts)) == plain
    args, p0, bs1 = D._model("pblstm", "lstm", ctc_decode_weight=0.0, ngram_lm=f, ngram_weight=1.0)
    assert bs1.ngram is not None and bs1.ngram_weight == 1.0 and bs1.ngram.order == 3
    assert D._hyps(bs1.decode_batch(None, utts)) != plain
    lm = bs1.ngram
    bs1.set_ngram(None, 0)
    assert D._hyps(bs1.decode_batch(None, utts)) == plain
    bs1.set_ngram(lm, 0.0)
    assert D._hyps(bs1.decode_batch(None, utts)) == plain


def test_search_without_an_lm_keeps_the_short_form(tmp_path):
    """bf16, one LSTM layer: with a file at weight 0 the step is still the short form (last_timing["short_form"]) and has no "ngram"
    part; with the LM it is the long form with its "ngram" part; after set_ngram(None, 0) the bits of the first search"""
    from las import layers as L, variables as V
    from las.las import LAS, Listener, Speller
    from las.beam_search import BeamSearch
    from las.ngram import NgramLM
    from oracle import las_oracle as O
    from utils.tokenizer import CharEncoder
    from helpers import make_args
    f = _arpa(tmp_path)
    args = make_args(enc_units=64, num_enc_layers=2, dec_units=64, num_dec_layers=1, embedding_size=32, attention_size=32, beam_size=4,
                     convert_rate=0.3, apply_lm=False, ngram_lm=f, ngram_weight=0.0)
    p0 = O.init_params(args, seed=11, cell="lstm")
    L.set_cell("lstm")
    L.set_precision("bf16")
    try:
        st = V.reset_default_store(device="cuda")
        st.load(p0)
        las = LAS(args, Listener, Speller, CharEncoder().token_to_id)
        las.build_variables()
        bs = BeamSearch(args, las, CharEncoder().token_to_id, None)
        assert bs.ngram is None
        utts = [synthetic_batch(1, T, 12, 30, seed=8 + k)[0] for k, T in enumerate((64, 48))]
        bs.measure = True
        off = bs.decode_batch(None, utts)
        assert bs.last_timing["short_form"] is True and set(bs.last_timing["parts_us"]) == {"speller", "beam"}
        bs.set_ngram(NgramLM.from_arpa(f, CharEncoder().token_to_id, 30), 1.0)
        bs.decode_batch(None, utts)
        parts_on = dict(bs.last_timing["parts_us"])
        assert bs.last_timing["short_form"] is False and set(parts_on) == {"speller", "ngram", "beam"} and parts_on["ngram"] > 0
        bs.set_ngram(None, 0)
        bs.measure = False
        assert [[(list(h.token_ids), float(h.log_prob)) for h in r] for r in bs.decode_batch(None, utts)] == \
               [[(list(h.token_ids), float(h.log_prob)) for h in r] for r in off]
    finally:
        L.set_precision("f32")


# ---- 4. command lines ---------------------------------------------------------------------------------------------------------------
MODEL = ["--unit", "char", "--feat_dim", "13", "--enc_type", "pblstm", "--enc_units", "64", "--num_enc_layers", "2", "--dec_units", "64",
         "--num_dec_layers", "1", "--attention_size", "32", "--embedding_size", "32", "--cell", "lstm", "--beam_size", "4"]


def test_transcribe_cli_with_ngram_lm(tmp_path):
    cmd = [sys.executable, os.path.join(PKG, "transcribe.py"), "--synthetic", "True", "--max_steps", "3", "--save_dir", str(tmp_path / "none"),
           "--ngram_lm", _arpa(tmp_path), "--ngram_weight", "1.0"] + MODEL
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert len(r.stdout.splitlines()) == 3
    r = subprocess.run(cmd + ["--ctc", "True", "--timestamps", "True"], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 3
    for ln in lines:
        assert set(json.loads(ln)) >= {"text", "score", "words"}


def test_transcribe_cli_with_ngram_lm_and_segments(tmp_path):
    cmd = [sys.executable, os.path.join(PKG, "transcribe.py"), "--synthetic", "True", "--max_steps", "3", "--save_dir", str(tmp_path / "none"),
           "--ngram_lm", _arpa(tmp_path), "--ngram_weight", "1.0"] + MODEL
    r = subprocess.run(cmd + ["--segment", "True"], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert len(r.stdout.splitlines()) == 3
    r = subprocess.run(cmd[:-len(MODEL) - 4] + ["--ngram_weight", "1.0"] + MODEL, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode != 0 and "ValueError" in r.stderr and "--ngram_lm FILE" in r.stderr


def test_decode_cli_with_ngram_lm(tmp_path):
    cmd = [sys.executable, os.path.join(PKG, "decode.py"), "--synthetic", "True", "--save_dir", str(tmp_path / "none"),
           "--ngram_lm", _arpa(tmp_path), "--ngram_weight", "1.0"] + MODEL
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0 and "Dev WER" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
