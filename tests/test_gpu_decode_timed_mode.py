"""Beam search IN THE MODE bench.py's `decode` object times (VERDICT r2 Weak #2): bench architecture (3 x pBLSTM-256 listener,
1 x LSTM-512 speller, additive attention 128), speed mode (bf16), >= 8 utterances x beam 16 = 128+ rows per step with the
2 x 512 char RNNLM fused in (BASELINE configs[4]), one captured step replayed as a HIP graph -- against the oracle's beam
search (reference las/beam_search.py:94-158, decode.py:131-149 restated) run in the oracle's bf16 arithmetic mode, and
graph replay against eager execution bit for bit.

Tolerance: the search ranks sums of raw logits; the speed mode's residual error against the bf16-mode oracle is ~5e-4 per
logit (test_gpu_full_scale.py), so normalised scores must agree to 5e-3 and the BEST hypothesis' token ids must be equal unless
the oracle's own top two hypotheses are closer than that tolerance (a near tie no arithmetic can be asked to resolve)."""
import numpy as np
import pytest
import torch

from helpers import lm_params, make_args, oracle_decode, oracle_lm, synthetic_batch

pytestmark = pytest.mark.gpu

NUTT, BEAM, T = 8, 16, 300


def _setup(prec, seed=17, eos_bias=0.4):
    from las import layers as L, variables as V
    from las.las import LAS, Listener, Speller
    from las.beam_search import BeamSearch
    from lang.char_rnn_model import CharRNN
    from oracle import las_oracle as O
    from utils.tokenizer import CharEncoder
    args = make_args(enc_units=256, num_enc_layers=3, dec_units=512, num_dec_layers=1, embedding_size=128, attention_size=128,
                     mode="add", beam_size=BEAM, convert_rate=0.166, apply_lm=True, lm_weight=0.5)
    p0 = O.init_params(args, seed=seed, cell="lstm")
    p0["Speller/decode/dense/bias"][2] = eos_bias     # 0.4: some hypotheses end before the step bound, some do not
    plm = lm_params(np.random.RandomState(8), 28, 0, 512, 2)
    for k in plm:
        plm[k] = (plm[k] * 0.3).astype(np.float32)
    L.set_cell("lstm"); L.set_precision(prec)
    st = V.reset_default_store(device="cuda"); st.load(p0); st.load(plm)
    tok = CharEncoder().token_to_id
    las = LAS(args, Listener, Speller, tok)
    lm = CharRNN(False, 1, 1, 28, 512, embedding_size=0, num_layers=2)
    bs = BeamSearch(args, las, tok, lm)
    # different lengths: different T' (38, 35, ...), different step bounds, masked frames in the shared [N, T'] buffers
    utts = [synthetic_batch(1, T - 23 * (k % 4), 8, 30, seed=60 + k)[0] for k in range(NUTT)]
    return args, p0, plm, bs, utts


def _norm(b):
    return float(b.log_prob) / (len(b.token_ids) - 1)


def test_bf16_beam16_lm_eight_utterances_match_the_bf16_oracle_and_graph_equals_eager():
    args, p0, plm, bs, utts = _setup("bf16")
    assert NUTT * BEAM >= 128                            # the row count of a search step (per-step kernels, not the one-launch training loop)
    bs.use_graph = True
    got = bs.decode_batch(None, utts)
    bs.use_graph = False
    eager = bs.decode_batch(None, utts)
    for g, e in zip(got, eager):                         # graph replay == eager, bit for bit
        assert [b.token_ids for b in g] == [b.token_ids for b in e]
        assert [float(b.log_prob) for b in g] == [float(b.log_prob) for b in e]
        assert torch.equal(g[-1].att[-1], e[-1].att[-1])
    # round 5: four hypotheses of an utterance per attention workgroup (LAS_SPELLER_ROWS_SHARE4; the default from 512 rows on) -- the same
    # arithmetic per row in the same order: bit-identical
    saved = bs.share_rows_from
    bs.share_rows_from = 1
    shared = bs.decode_batch(None, utts)
    bs.share_rows_from = saved
    for g, e in zip(got, shared):
        assert [b.token_ids for b in g] == [b.token_ids for b in e]
        assert [float(b.log_prob) for b in g] == [float(b.log_prob) for b in e]
        assert torch.equal(g[-1].att[-1], e[-1].att[-1])
    # the 5-launch step (Speller cell in one launch, both vocabulary projections inside the beam kernel)
    # against the 8-launch step (skinny cell product + finishing kernel with its own logits, LM projection as a GEMM on top)
    assert bs.fuse_projection
    bs.fuse_projection = False
    long_form = bs.decode_batch(None, utts)
    bs.fuse_projection = True
    agree = 0
    for g, l in zip(got, long_form):
        assert abs(_norm(g[-1]) - _norm(l[-1])) <= 2e-3
        agree += g[-1].token_ids == l[-1].token_ids
    assert agree >= NUTT - 1
    olm = (oracle_lm(plm, 0, 2), 512, 2)
    same, worst = 0, 0.0
    for u, (xs, res) in enumerate(zip(utts, got)):
        ref = oracle_decode(xs, p0, args, "lstm", BEAM, lm=olm, lm_weight=0.5, prec="bf16")
        assert len(res) > 0 and len(ref) > 0
        best, rbest = res[-1], ref[-1]
        d = abs(_norm(best) - _norm(rbest))
        worst = max(worst, d)
        assert d <= 5e-3, (u, _norm(best), _norm(rbest))
        if best.token_ids == rbest.token_ids:
            same += 1
            assert float(best.log_prob) == pytest.approx(float(rbest.log_prob), abs=5e-3 * (len(best.token_ids) - 1))
            assert np.abs(best.att[-1].cpu().numpy() - rbest.att[-1]).max() < 2e-3
        else:
            # only acceptable as a near tie IN THE ORACLE: its runner-up must be our best and within the tolerance of its best
            ids = [b.token_ids for b in ref]
            assert best.token_ids in ids, (u, "best hypothesis is not among the oracle's final beam")
            alt = ref[ids.index(best.token_ids)]
            assert abs(_norm(alt) - _norm(rbest)) <= 5e-3, (u, _norm(alt), _norm(rbest))
    print("bf16 decode, %d utterances x beam %d + LM: best hypothesis identical for %d / %d, worst normalised-score gap %.2e"
          % (NUTT, BEAM, same, NUTT, worst))
    assert same >= NUTT - 1


def test_f32_beam16_lm_at_the_bench_architecture_is_exact():
    """same search in the parity mode: token ids of every surviving hypothesis equal the oracle's (f32), scores to 2e-3"""
    args, p0, plm, bs, utts = _setup("f32")
    got = bs.decode_batch(None, utts[:3])
    olm = (oracle_lm(plm, 0, 2), 512, 2)
    for xs, res in zip(utts[:3], got):
        ref = oracle_decode(xs, p0, args, "lstm", BEAM, lm=olm, lm_weight=0.5)
        assert [b.token_ids for b in res] == [b.token_ids for b in ref]
        for a, b in zip(res, ref):
            assert float(a.log_prob) == pytest.approx(float(b.log_prob), abs=5e-3)


def test_bf16_utterances_of_different_lengths_one_ragged_encoder_pass_equals_one_encoder_each():
    """decode_batch over utterances of DIFFERENT (odd and even) lengths: the single encoder pass with per-row frame counts
    (las_rnn_seq_fwd with row_T) against one encoder per utterance -- side by side on several streams, and one after the other: hypotheses,
    scores and alignments must be bit-identical (every real frame of the ragged pass is the frame the utterance gets alone)."""
    args, p0, plm, bs, _ = _setup("bf16")
    utts = [synthetic_batch(1, T_, 8, 30, seed=60 + k)[0] for k, T_ in enumerate((300, 287, 251, 300, 199, 274))]
    res = {}
    for name, rg, par in (("ragged", True, True), ("streams", False, True), ("serial", False, False)):
        bs.ragged_encoder, bs.parallel_encoders = rg, par
        res[name] = bs.decode_batch(None, utts)
    bs.ragged_encoder = bs.parallel_encoders = True
    for other in ("streams", "serial"):
        for a, b in zip(res["ragged"], res[other]):
            assert [h.token_ids for h in a] == [h.token_ids for h in b], other
            assert [float(h.log_prob) for h in a] == [float(h.log_prob) for h in b], other
            assert torch.equal(a[-1].att[-1], b[-1].att[-1])


def test_forty_utterances_in_one_batch_equal_the_same_utterances_in_groups_of_eight():
    """decode.py's --decode_batch (default 64 since round 4: 1,300 instead of 720 utterances/s at 16) only changes how many hypothesis rows
    share a launch: 40 utterances x beam 16 = 640 rows in one device-resident search must give every utterance the hypotheses, scores and
    alignments it gets in a batch of 8 (rows never interact; the beam kernel ranks per utterance)."""
    args, p0, plm, bs, _ = _setup("bf16")
    utts = [synthetic_batch(1, 150 - 7 * (k % 5), 8, 30, seed=400 + k)[0] for k in range(40)]
    big = bs.decode_batch(None, utts)
    small = []
    for c0 in range(0, 40, 8):
        small += bs.decode_batch(None, utts[c0:c0 + 8])
    assert len(big) == len(small) == 40
    for u, (a, b) in enumerate(zip(big, small)):
        assert [h.token_ids for h in a] == [h.token_ids for h in b], u
        assert [float(h.log_prob) for h in a] == [float(h.log_prob) for h in b], u
        assert torch.equal(a[-1].att[-1], b[-1].att[-1]), u


def test_a_stream_of_batches_with_overlapped_encoders_equals_one_batch_at_a_time():
    """BeamSearch.decode_batches (what decode.py's loop runs since round 5): the encoders of batch k+1 run on a second stream under the
    search of batch k.  Five batches of different geometry (equal lengths, ragged lengths, a single utterance, different counts -- so the
    search's graph is re-captured while the next encoders are in flight) must give, batch by batch, bit for bit what decode_batch gives
    one batch at a time; run twice (the second pass reuses the first one's streams, workspaces and freed encoder buffers)."""
    args, p0, plm, bs, _ = _setup("bf16")
    mk = lambda T_, k: synthetic_batch(1, T_, 8, 30, seed=700 + k)[0]
    batches = [[mk(260, k) for k in range(6)],
               [mk(T_, 10 + k) for k, T_ in enumerate((300, 287, 251, 300, 199, 274, 131))],
               [mk(222, 20)],
               [mk(260, 30 + k) for k in range(6)],
               [mk(T_, 40 + k) for k, T_ in enumerate((97, 300, 188))]]
    want = [bs.decode_batch(None, b) for b in batches]
    for rnd in range(2):
        got = list(bs.decode_batches(None, iter(batches)))
        assert len(got) == len(want)
        for k, (gb, wb) in enumerate(zip(got, want)):
            assert len(gb) == len(wb) == len(batches[k])
            for a, b in zip(gb, wb):
                assert [h.token_ids for h in a] == [h.token_ids for h in b], (rnd, k)
                assert [float(h.log_prob) for h in a] == [float(h.log_prob) for h in b], (rnd, k)
                assert torch.equal(a[-1].att[-1], b[-1].att[-1]), (rnd, k)
    assert list(bs.decode_batches(None, [])) == []
    from las import _hip
    _hip.check_status()


def test_lm_state_copies_from_384_rows_on_change_nothing():
    """From 384 hypothesis rows on decode_batch keeps bf16 copies of the LM's recurrent state (written by the cells, gathered with the
    fp32 state) for the cells to read: 24 utterances x beam 16 = 384 rows with and without them must agree bit for bit."""
    args, p0, plm, bs, _ = _setup("bf16")
    utts = [synthetic_batch(1, 140 - 9 * (k % 4), 8, 30, seed=900 + k)[0] for k in range(24)]
    assert bs.lm_state_copies
    with_copies = bs.decode_batch(None, utts)
    bs.lm_state_copies = False
    without = bs.decode_batch(None, utts)
    bs.lm_state_copies = True
    for u, (a, b) in enumerate(zip(with_copies, without)):
        assert [h.token_ids for h in a] == [h.token_ids for h in b], u
        assert [float(h.log_prob) for h in a] == [float(h.log_prob) for h in b], u
        assert torch.equal(a[-1].att[-1], b[-1].att[-1]), u


def test_bf16_sixty_four_utterances_at_T_1274_match_the_bf16_oracle():
    """The geometry bench.py's decode `value` is quoted on since round 4: 64 utterances x beam 16 = 1024 hypothesis
    rows per step, T = 1274 frames (T' = 160), 2 x 512 LM fused in, one captured step replayed -- `lstm_cell_rows` at M = 1024, the
    attention rows at 1024 rows x 160 frames, the beam kernel over 64 utterances -- and, as in the bench, no hypothesis ends before the
    step bound: all 211 steps of the search run.  Three of the 64 utterances (first, one in the middle, last: different row blocks of every
    launch) against the oracle in its bf16 mode with the hoisted key projection, and the same three decoded in a batch of their own (the
    rows of a search never interact: bit-identical).

    With random weights the 16 final hypotheses of an utterance are 211-token sequences whose normalised scores lie within 1e-3 of each
    other (oracle: 0.3082 ... 0.3093), i.e. every one of the 211 prunings is a near tie and two correct searches need not keep the same
    sequences.  What is asserted therefore: (a) ARITHMETIC -- the score the search accumulated for its best hypothesis equals the oracle's
    teacher-forced score of the SAME 211 tokens (Speller logit + 0.5 x LM logit per step) to 1e-3 per token, and the last step's alignment
    to 2e-3; (b) SEARCH QUALITY -- the best normalised score is within 5e-3 of the best the oracle's own beam search finds."""
    from helpers import oracle_score_tokens
    args, p0, plm, bs, _ = _setup("bf16", eos_bias=0.0)
    n, Tf = 64, 1274
    utts = [synthetic_batch(1, Tf, 8, 30, seed=100 + k)[0] for k in range(n)]        # bench.py decode_bench's utterances
    got = bs.decode_batch(None, utts)
    assert len(got) == n and bs.use_graph
    pick = (0, 37, 63)
    alone = bs.decode_batch(None, [utts[u] for u in pick])
    olm = (oracle_lm(plm, 0, 2), 512, 2)
    worst_tf, worst_best = 0.0, 0.0
    for u, small in zip(pick, alone):
        res = got[u]
        assert [b.token_ids for b in res] == [b.token_ids for b in small], u
        assert [float(b.log_prob) for b in res] == [float(b.log_prob) for b in small], u
        best = res[-1]
        L_ = len(best.token_ids) - 1
        assert L_ == int(Tf * args.convert_rate) == 211 and best.att[-1].shape[-1] == 160          # the bench's search length and T'
        sc, atts = oracle_score_tokens(utts[u], p0, args, "lstm", best.token_ids, lm=olm, lm_weight=0.5, prec="bf16")
        worst_tf = max(worst_tf, abs(float(best.log_prob) - sc) / L_)
        assert abs(float(best.log_prob) - sc) <= 1e-3 * L_, (u, float(best.log_prob), sc)
        assert np.abs(best.att[-1].cpu().numpy() - atts[-1]).max() < 2e-3
        assert np.abs(best.att[L_ // 2].cpu().numpy() - atts[L_ // 2 - 1]).max() < 2e-3            # att[0] is the all-zero item
        ref = oracle_decode(utts[u], p0, args, "lstm", BEAM, lm=olm, lm_weight=0.5, prec="bf16", hoist=True)
        worst_best = max(worst_best, abs(_norm(best) - _norm(ref[-1])))
        assert abs(_norm(best) - _norm(ref[-1])) <= 5e-3, (u, _norm(best), _norm(ref[-1]))
    print("bf16 decode at the `value` geometry (64 utterances x beam 16, T = 1274, 211 steps): accumulated score vs the oracle's score of the "
          "same tokens %.2e per token (worst of %d utterances), best normalised score vs the oracle's search %.2e" % (worst_tf, len(pick), worst_best))
