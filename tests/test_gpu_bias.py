"""Contextual biasing: las_bias_step against the numpy restatement (tests/bias_ref.py) bit for bit, decode_batch against
the CPU biased search, the bonus identity of the scores, off = today's search, the refusals and the command lines."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bias_ref as B
import ctc_prefix_ref as R
from helpers import PKG, _oracle_fns, oracle_score_tokens, synthetic_batch

pytestmark = pytest.mark.gpu
SENT = 7.0                      # sentinel of rows the kernel must not write
EOS = 2


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------------------
def _phrases(V, fanout):
    """fanout "one": a single phrase-initial token; "some": the named cases; "wide": more phrase-initial tokens than a workgroup has
    lanes -- 300 of them, or every token where the vocabulary has fewer (V = 257)"""
    if fanout == "one":
        return [[5, 6, 7], [5, 6], [5, 0, V - 1]]
    ph = [[5, 6, 7], [5, 6],                                 # [5, 6]: a phrase end WITH children
          [9, 10],                                           # childless: entering 10 goes back to the root
          [0, V - 1, 4], [V - 1, 11],                        # child tokens 0 and V - 1, under the root and below it
          [12, EOS],                                         # EOS is an ordinary token
          [20, 13, 3], [20, 15, 3], [20, 17, 3]]             # node (20,): sorted children 13, 15, 17
    if fanout == "wide":
        ph += [[v, 3] for v in range(min(V, 300)) if v not in (5, 9, 0, V - 1, 12, 20)]
    return ph


def _node_of(g, m):
    """the node of match m, by descending the tables from the root"""
    s = 0
    for v in m:
        lo, hi = int(g.child_off[s]), int(g.child_off[s + 1])
        k = lo + int(np.searchsorted(g.child_tok[lo:hi], v))
        assert k < hi and g.child_tok[k] == v, (m, v)
        s = int(g.child_next[k])
        assert s != 0, "the match %r is a childless phrase end: not a state" % (m,)
    return s


def _launch(g, V, scores, st_vals, tokens, t, nlive, done, dec_step, Umax, n, beam, W):
    from las import _hip
    N = n * beam
    d = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x), dtype=dt).cuda()
    i32 = torch.int32
    tab = g.to("cuda")
    sc = d(scores, torch.float32)
    st_in = torch.full((N, W), 123.0, device="cuda")
    st_in[:, 0] = d(st_vals, torch.float32)
    st_out = torch.full((N, W), SENT, device="cuda")
    keep = [d(tokens, i32), d([t, 0], i32), d(nlive, i32), d(done, i32), d(dec_step, i32)]
    rc = _hip.lib().las_bias_step(_hip.p(tab["child_off"]), _hip.p(tab["child_tok"]), _hip.p(tab["child_next"]), _hip.p(tab["gdef"]),
                                  _hip.p(tab["groot"]), float(g.beta), g.num_nodes, int(g.child_tok.size), _hip.p(sc), n, beam, V,
                                  _hip.p(st_in), _hip.p(st_out), W, *[_hip.p(x) for x in keep], Umax, _hip.stream())
    _hip.check(rc, "las_bias_step")
    torch.cuda.synchronize()
    return sc.cpu().numpy(), st_out.cpu().numpy()


def _expect(g, phrases, V, scores, parents, tokens, t, nlive, done, dec_step, Umax, n, beam, W):
    """numpy: the rows that are live get their parent's match (None: not a node, the root) advanced by the entering token and one
    float32 add per candidate; every other row keeps its bytes"""
    sc = np.array(scores, np.float32, copy=True)
    st = np.full((n * beam, W), SENT, np.float32)
    for u in range(n):
        for j in range(beam):
            r = u * beam + j
            if t >= Umax or done[u] or t >= dec_step[u] or j >= (1 if t == 0 else nlive[u]):
                continue
            par = () if (t == 0 or parents[r] is None) else parents[r]
            m, _ = B.walk(phrases, g.beta, par, int(tokens[r]))
            st[r, 0] = _node_of(g, m)
            sc[r] = B.apply_row(sc[r], B.row_gains(phrases, g.beta, m, V))
    return sc, st


def _same_bits(got, want):
    return np.array_equal(np.asarray(got, np.float32).view(np.int32), np.asarray(want, np.float32).view(np.int32))


@pytest.mark.parametrize("V,fanout", [(30, "one"), (30, "some"), (257, "one"), (257, "some"), (257, "wide"), (5000, "one"), (5000, "some"),
                                      (5000, "wide")])
def test_bias_step_matches_numpy_bit_for_bit(V, fanout):
    """Advanced node and every score of every row, by bytes.  One launch covers: at the root; mid-phrase (pend != 0); on a phrase end
    with children (non-root, pend = 0); an entering token that completes a childless phrase; a mismatch that restarts at a root child;
    a mismatch to the root; an entering EOS; child tokens 0 and V - 1; entering tokens below, between and above a node's sorted
    children; -inf entries.  Further launches: node values -1, M, NaN, inf and entering tokens outside [0, V); step 0; nlive / done /
    dec_step / Umax liveness (untouched rows keep the sentinel); two launches give the same bytes."""
    from las.bias import ContextGraph
    n, beam = 3, 4
    N = n * beam
    rng = np.random.RandomState(V)
    phrases = _phrases(V, fanout)
    g = ContextGraph(phrases, 1.7, vocab_size=V, sos_id=-1, pad_id=-1)           # (token 0 as a child: no specials at this level)
    fan = int(g.child_off[1])
    assert fan == len({p[0] for p in phrases}) and (fan == 1 if fanout == "one" else fan == 6 if fanout == "some" else fan > 256)
    if fanout == "one":
        rows = [((), 4), ((5,), 6), ((), 5), ((5, 6), 7), ((5,), 0), ((5, 0), V - 1), ((5,), 5), ((5,), 3), ((5, 6), EOS), ((5, 6), 5),
                ((5, 0), 5), ((), EOS)]
    else:
        rows = [((), 4), ((5,), 6), ((), 5), ((9,), 10), ((20,), 12), ((20,), 16), ((20,), 18), ((12,), EOS), ((0,), V - 1), ((5, 6), 7),
                ((20,), 15), ((V - 1,), 11)]
    parents = [r[0] for r in rows]
    tokens = np.array([r[1] for r in rows])
    st_vals = np.array([_node_of(g, m) for m in parents], np.float32)
    scores = (rng.randn(N, V) * 3.0).astype(np.float32)
    scores[:, [0, 5, 6, 13, V - 1]] = np.where(rng.rand(N, 5) < 0.5, -np.inf, scores[:, [0, 5, 6, 13, V - 1]])
    scores[rng.rand(N, V) < 0.02] = -np.inf
    scores[0, 3] = -0.0
    live = dict(t=1, nlive=[beam] * n, done=[0] * n, dec_step=[1000] * n, Umax=1000)
    args = dict(n=n, beam=beam, W=4)

    def check(parents, st_vals, tokens, **kw):
        kw = dict(args, **dict(live, **kw))
        got = _launch(g, V, scores, st_vals, tokens, **kw)
        want = _expect(g, phrases, V, scores, parents, tokens, **kw)
        assert _same_bits(got[1], want[1]), (got[1][:, 0], want[1][:, 0])
        bad = np.nonzero(got[0].view(np.int32) != want[0].view(np.int32))
        assert bad[0].size == 0, (bad[0][:8], bad[1][:8], got[0][bad][:8], want[0][bad][:8])
        return got, want

    got, want = check(parents, st_vals, tokens)
    assert np.all(np.isneginf(got[0][np.isneginf(scores)]))
    assert np.any(want[1][:, 0] != 0) and np.any(want[1][:, 0] == 0) and not _same_bits(want[0], scores)      # (the expectation is no identity)
    again = _launch(g, V, scores, st_vals, tokens, **dict(args, **live))
    assert _same_bits(again[0], got[0]) and _same_bits(again[1], got[1])
    # values that are no node behave as the root; entering tokens outside [0, V) take rule 3
    M = g.num_nodes
    mid = (5,)
    p2 = [None, None, None, None, None, mid, mid, mid, mid, (5, 6), (5, 6), None]
    s2 = np.array([-1.0, M, np.nan, np.inf, -np.inf] + [_node_of(g, m) for m in p2[5:11]] + [3.0e9], np.float32)
    t2 = np.array([5, 5, 5, 4, 5, -1, V, 2 ** 30, -2 ** 31, V, 6, 5])
    check(p2, s2, t2)
    # liveness: step 0 (only j = 0, from the root, garbage in state_in), then every way a row is not live; one float per state row
    check(parents, st_vals, np.array([1, 5, 5, 5, 5, 6, 6, 6, 4, 7, 7, 7]), t=0, W=1)
    check(parents, st_vals, tokens, nlive=[beam, 2, 0])
    check(parents, st_vals, tokens, done=[0, 1, 0], W=1)
    check(parents, st_vals, tokens, dec_step=[1000, 1, 2])
    got, _ = check(parents, st_vals, tokens, t=5, Umax=5)
    assert _same_bits(got[0], scores) and np.all(got[1] == SENT)


def test_bias_step_refusals():
    from las import _hip
    from las.bias import ContextGraph
    g = ContextGraph([[5, 6]], 1.0, vocab_size=30)
    tab = g.to("cuda")
    z = torch.zeros(64, device="cuda")
    zi = torch.zeros(64, dtype=torch.int32, device="cuda")
    z2 = torch.zeros(64, device="cuda")

    def call(beta=1.0, M=g.num_nodes, V=30, st_in=z, st_out=z2, W=1):
        return _hip.lib().las_bias_step(_hip.p(tab["child_off"]), _hip.p(tab["child_tok"]), _hip.p(tab["child_next"]), _hip.p(tab["gdef"]),
                                        _hip.p(tab["groot"]), beta, M, int(g.child_tok.size), _hip.p(z), 1, 2, V, _hip.p(st_in),
                                        _hip.p(st_out), W, _hip.p(zi), _hip.p(zi), _hip.p(zi), _hip.p(zi), _hip.p(zi), 4, _hip.stream())
    for kw, msg in ((dict(beta=0.0), b"weight"), (dict(beta=float("nan")), b"weight"), (dict(beta=float("inf")), b"weight"),
                    (dict(V=16385), b"V <="), (dict(M=0), b"nodes"), (dict(M=(1 << 22) + 1), b"nodes"), (dict(st_out=z), b"differ"),
                    (dict(W=0), b"state_width")):
        assert call(**kw) < 0 and msg in _hip.lib().las_last_error(), kw
    torch.cuda.synchronize()


# ---- 2. the search ------------------------------------------------------------------------------------------------------------------
BETA = {"pblstm": 0.5, "cnn": 0.25}
DISTRACTORS = [[29, 28, 29, 27], [26, 29]]          # occur in no hypothesis; their first tokens open matches that are paid back


def _norm(h):
    return float(h.log_prob) / (len(h.token_ids) - 1)


def _reference_unbiased(fns, lam):
    from oracle import las_oracle as O
    out = []
    for step_fn, init, Tp, dec_step, lp, T in fns:
        out.append(R.joint_beam_search(step_fn, init, Tp, dec_step, 4, 1, EOS, lp, T, lam) if lam > 0
                   else O.beam_search(step_fn, init, Tp, dec_step, 4, 1, EOS))
    return out


def _phrases_from(unbiased):
    """from the reference's UNBIASED search: of every utterance's second-best hypothesis the (up to) three tokens from the place where
    it leaves the best one, cut at a <PAD> / <SOS> (never part of a phrase); plus the distractors"""
    phrases = []
    for ref in unbiased:
        if len(ref) < 2:
            continue
        best, alt = list(ref[-1].token_ids[1:]), list(ref[-2].token_ids[1:])
        d = next((i for i, (a, b) in enumerate(zip(best, alt)) if a != b), min(len(best), len(alt)))
        piece = []
        for v in alt[d:d + 3]:
            if v in (0, 1):
                break
            piece.append(v)
        if piece and piece not in phrases:
            phrases.append(piece)
    return phrases + DISTRACTORS


def _cpu_fns(utts, p0, args, cell, lam):
    import test_gpu_ctc_decode as D
    fns = []
    for xs in utts:
        step_fn, _, _, init, Tp, dec_step = _oracle_fns(xs, p0, args, cell, None)
        lp, T = D._oracle_lp(xs, p0, args, cell) if lam > 0 else (None, None)
        fns.append((step_fn, init, Tp, dec_step, lp, T))
    return fns


@pytest.mark.parametrize("enc_type,cell,lam", [("pblstm", "lstm", 0.0), ("cnn", "rnn", 0.3)])
def test_decode_batch_biased_matches_cpu_biased_search(enc_type, cell, lam):
    """decode_batch with a hotword context against the CPU biased search (tests/bias_ref.py); every hypothesis' score is its attention
    score [+ weight x log p_ctc] + its bonus; one utterance at a time, eager steps and decode_batches give the same bits.
    The phrases come from the reference's unbiased search and are checked, on the reference alone, to change a best hypothesis (a) and
    to leave two of the three utterances a margin of 0.05 between best and second best (b)."""
    import torch.nn.functional as F
    import test_gpu_ctc_decode as D
    from las.bias import ContextGraph
    args, p0, bs = D._model(enc_type, cell, ctc_decode_weight=lam)
    beta = BETA[enc_type]
    utts = D._utts(args)
    fns = _cpu_fns(utts, p0, args, cell, lam)
    unbiased = _reference_unbiased(fns, lam)
    phrases = _phrases_from(unbiased)
    assert len(phrases) > len(DISTRACTORS)
    for ref in unbiased:
        for h in ref:
            ids = list(h.token_ids)
            assert not any(ids[i:i + len(p)] == p for p in DISTRACTORS for i in range(len(ids)))
    refs = [B.biased_beam_search(f[0], f[1], f[2], f[3], 4, 1, EOS, phrases, beta, f[4], f[5], lam) for f in fns]
    changed = [list(r[-1].token_ids) != list(u[-1].token_ids) for r, u in zip(refs, unbiased)]
    margins = [_norm(r[-1]) - _norm(r[-2]) if len(r) > 1 else np.inf for r in refs]
    print("reference: changed", changed, "margins", margins)
    assert sum(changed) >= 1                                             # (a)
    assert sum(m >= 0.05 for m in margins) >= 2                          # (b)

    bs.set_context(ContextGraph(phrases, beta, vocab_size=args.vocab_size))
    batch = bs.decode_batch(None, utts)
    assert all(batch)
    near_ties = 0
    for res, ref in zip(batch, refs):
        got_best, ref_best = res[-1], ref[-1]
        print("device", list(got_best.token_ids), float(got_best.log_prob), "reference", list(ref_best.token_ids), float(ref_best.log_prob))
        if list(got_best.token_ids) == list(ref_best.token_ids):
            assert float(got_best.log_prob) == pytest.approx(float(ref_best.log_prob), abs=5e-3)
        else:                                                            # a near tie at the end (test_gpu_ctc_decode._close)
            near_ties += 1
            assert abs(_norm(got_best) - _norm(ref_best)) < 5e-3
    assert near_ties <= 1
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
            want += B.bonus(phrases, beta, ids[1:])
            n_checked += 1
            assert abs(float(h.log_prob) - want) < 5e-3 + 1e-4 * abs(want), (ids, float(h.log_prob), want)
    assert n_checked > 0
    assert D._hyps([bs.decode(None, xs) for xs in utts]) == D._hyps(batch)
    bs.use_graph = False
    try:
        assert D._hyps(bs.decode_batch(None, utts)) == D._hyps(batch)
    finally:
        bs.use_graph = True
    streamed = [r for res in bs.decode_batches(None, [utts[:2], utts[2:]]) for r in res]
    assert D._hyps(streamed) == D._hyps(batch)
    # ... and the context is what made the difference
    bs.set_context(None)
    assert D._hyps(bs.decode_batch(None, utts)) != D._hyps(batch)


# ---- 3. off means off ---------------------------------------------------------------------------------------------------------------
def test_off_is_bit_identical(tmp_path):
    """no --hotwords, a file with weight 0, and set_context(None) after a biased search: the same hypotheses, bit for bit"""
    import test_gpu_ctc_decode as D
    from las.bias import ContextGraph
    f = tmp_path / "hot.txt"
    f.write_text("ADA\nNEW YORK\n")
    args, p0, bs = D._model("pblstm", "lstm", ctc_decode_weight=0.0)
    utts = D._utts(args)
    plain = D._hyps(bs.decode_batch(None, utts))
    assert any(plain) and bs.context is None
    args, p0, bs0 = D._model("pblstm", "lstm", ctc_decode_weight=0.0, hotwords=str(f), hotword_weight=0.0)
    assert bs0.context is None
    assert D._hyps(bs0.decode_batch(None, utts)) == plain
    args, p0, bs1 = D._model("pblstm", "lstm", ctc_decode_weight=0.0, hotwords=str(f), hotword_weight=2.0)
    assert bs1.context is not None and bs1.context.active
    assert D._hyps(bs1.decode_batch(None, utts)) != plain
    bs1.set_context(None)
    assert D._hyps(bs1.decode_batch(None, utts)) == plain
    bs1.set_context(ContextGraph([[4, 7, 4]], 0.0, vocab_size=30))
    assert D._hyps(bs1.decode_batch(None, utts)) == plain


def test_search_without_a_context_keeps_the_short_form(tmp_path):
    """bf16, one LSTM layer: with a file at weight 0 the step is still the short form (last_timing["short_form"]) and has no "bias"
    part; with a context it is the long form with its "bias" part; after set_context(None) the bits of the first search"""
    from las import layers as L, variables as V
    from las.las import LAS, Listener, Speller
    from las.beam_search import BeamSearch
    from las.bias import ContextGraph
    from oracle import las_oracle as O
    from utils.tokenizer import CharEncoder
    from helpers import make_args
    f = tmp_path / "hot.txt"
    f.write_text("ADA\n")
    args = make_args(enc_units=64, num_enc_layers=2, dec_units=64, num_dec_layers=1, embedding_size=32, attention_size=32, beam_size=4,
                     convert_rate=0.3, apply_lm=False, hotwords=str(f), hotword_weight=0.0)
    p0 = O.init_params(args, seed=11, cell="lstm")
    L.set_cell("lstm")
    L.set_precision("bf16")
    try:
        st = V.reset_default_store(device="cuda")
        st.load(p0)
        las = LAS(args, Listener, Speller, CharEncoder().token_to_id)
        las.build_variables()
        bs = BeamSearch(args, las, CharEncoder().token_to_id, None)
        assert bs.context is None
        utts = [synthetic_batch(1, T, 12, 30, seed=8 + k)[0] for k, T in enumerate((64, 48))]
        bs.measure = True
        off = bs.decode_batch(None, utts)
        assert bs.last_timing["short_form"] is True and set(bs.last_timing["parts_us"]) == {"speller", "beam"}
        bs.set_context(ContextGraph([[4, 7, 4]], 2.0, vocab_size=30))
        bs.decode_batch(None, utts)
        parts_on = dict(bs.last_timing["parts_us"])
        assert bs.last_timing["short_form"] is False and set(parts_on) == {"speller", "bias", "beam"} and parts_on["bias"] > 0
        bs.set_context(None)
        bs.measure = False
        assert [[(list(h.token_ids), float(h.log_prob)) for h in r] for r in bs.decode_batch(None, utts)] == \
               [[(list(h.token_ids), float(h.log_prob)) for h in r] for r in off]
    finally:
        L.set_precision("f32")


# ---- 4. refusals and command lines --------------------------------------------------------------------------------------------------
def test_refusals_before_any_launch(tmp_path):
    import test_gpu_ctc_decode as D
    with pytest.raises(ValueError, match="--hotwords FILE"):
        D._model("pblstm", "lstm", ctc_decode_weight=0.0, hotword_weight=2.0)
    with pytest.raises(ValueError, match="no such file"):
        D._model("pblstm", "lstm", ctc_decode_weight=0.0, hotwords=str(tmp_path / "absent.txt"), hotword_weight=2.0)
    f = tmp_path / "hot.txt"
    f.write_text("OK\nR2D2\n")
    with pytest.raises(ValueError, match="line 2"):
        D._model("pblstm", "lstm", ctc_decode_weight=0.0, hotwords=str(f), hotword_weight=2.0)
    args, p0, bs = D._model("pblstm", "lstm", ctc_decode_weight=0.0)
    from las.bias import ContextGraph
    with pytest.raises(ValueError, match="vocabulary"):
        bs.set_context(ContextGraph([[40, 41]], 1.0, vocab_size=64))


MODEL = ["--unit", "char", "--feat_dim", "13", "--enc_type", "pblstm", "--enc_units", "64", "--num_enc_layers", "2", "--dec_units", "64",
         "--num_dec_layers", "1", "--attention_size", "32", "--embedding_size", "32", "--cell", "lstm", "--beam_size", "4"]


def _hotfile(tmp_path):
    f = tmp_path / "hot.txt"
    f.write_text("# names\nADA LOVELACE\nnew york\nNEW YORK CITY\n")
    return str(f)


def test_transcribe_cli_with_hotwords(tmp_path):
    cmd = [sys.executable, os.path.join(PKG, "transcribe.py"), "--synthetic", "True", "--max_steps", "3", "--save_dir", str(tmp_path / "none"),
           "--hotwords", _hotfile(tmp_path), "--hotword_weight", "2.0"] + MODEL
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert len(r.stdout.splitlines()) == 3
    r = subprocess.run(cmd + ["--ctc", "True", "--timestamps", "True"], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 3
    for ln in lines:
        o = json.loads(ln)
        assert set(o) >= {"text", "score", "words"}
    r = subprocess.run(cmd[:-len(MODEL) - 4] + ["--hotword_weight", "2.0"] + MODEL, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode != 0 and "ValueError" in r.stderr and "--hotwords FILE" in r.stderr


def test_decode_cli_with_hotwords(tmp_path):
    cmd = [sys.executable, os.path.join(PKG, "decode.py"), "--synthetic", "True", "--save_dir", str(tmp_path / "none"),
           "--hotwords", _hotfile(tmp_path), "--hotword_weight", "2.0"] + MODEL
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0 and "Dev WER" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
