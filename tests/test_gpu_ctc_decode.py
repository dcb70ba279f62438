"""Joint CTC-attention beam search: las_ctc_prefix_step / las_ctc_log_softmax against the CPU restatement
(tests/ctc_prefix_ref.py), decode_batch against the CPU joint search, the telescoping identity of the scores, weight 0 = today's search,
and decode.py's --ctc_decode_weight."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ctc_prefix_ref as R
from helpers import PKG, _oracle_fns, oracle_score_tokens, synthetic_batch
import test_gpu_ctc as C

pytestmark = pytest.mark.gpu
LAM = 0.3


def _tol(ref):
    return 1e-4 + 1e-5 * np.abs(ref)


def _width(Tp):
    return 4 * ((2 * Tp + 2 + 3) // 4)


def _run_step(lp_cm, lens, logits, st_in, tokens, beam, t, lam, end_id=2, nlive=None, done=None, dec_step=None, Umax=1000, fill=0.0):
    """one launch; by default every row is live (nlive = beam, nothing done, dec_step = Umax = 1000) and st_out starts as zeros (fill)"""
    from las import _hip
    n, Vc, Tp = lp_cm.shape
    V = Vc - 1
    N = n * beam
    d = lambda x, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(x), dtype=dt).cuda()
    i32 = torch.int32
    joint = torch.full((N, V), 7.0, device="cuda")
    st_out = torch.full((N, _width(Tp)), fill, device="cuda")
    args = [d(lp_cm), d(lens, i32), n, beam, Tp, V, end_id, d(logits), joint, lam, d(st_in), st_out, _width(Tp), d(tokens, i32),
            d([t, 0], i32), d([beam] * n if nlive is None else nlive, i32), d([0] * n if done is None else done, i32),
            d([1000] * n if dec_step is None else dec_step, i32), Umax]
    ptr = [(_hip.p(a) if torch.is_tensor(a) else a) for a in args]
    _hip.check(_hip.lib().las_ctc_prefix_step(*ptr, _hip.stream()), "las_ctc_prefix_step")
    torch.cuda.synchronize()
    return joint.cpu().numpy(), st_out.cpu().numpy()


def _state_row(s, Tp):
    row = np.zeros(_width(Tp), np.float32)
    T = len(s.rn)
    row[:T], row[Tp:Tp + T], row[2 * Tp], row[2 * Tp + 1] = s.rn, s.rb, s.psi, s.last
    return row


def _check_state(out_row, h, Tp):
    T = len(h.rn)
    for got, ref in ((out_row[:T], h.rn), (out_row[Tp:Tp + T], h.rb), (out_row[2 * Tp:2 * Tp + 1], np.array([h.psi]))):
        low = ref < -1e9
        assert np.all(got[low] < -1e9)
        assert np.all(np.abs(got[~low] - ref[~low]) <= _tol(ref[~low])), np.abs(got[~low] - ref[~low]).max()
    assert out_row[2 * Tp + 1] == h.last


@pytest.mark.parametrize("V", [30, 5000])
@pytest.mark.parametrize("Tp", [1, 7, 160, 319])
def test_prefix_step_matches_cpu_reference(V, Tp):
    """Advanced state and every candidate's joint score of hypotheses of several lengths (the empty one, repeated labels, longer than the
    frames), the EOS candidate, utterances of different T'_u in one launch; two runs give the same bits"""
    rng = np.random.RandomState(V + Tp)
    n, beam, eos = 3, 4, 2
    N = n * beam
    lens = [Tp, max(1, Tp - 3), max(1, Tp // 2)]
    lp_tm = torch.log_softmax(torch.tensor(rng.randn(n, Tp, V + 1) * 2.0, dtype=torch.float32), -1).numpy()
    logits = (rng.randn(N, V) * 3.0).astype(np.float32)
    tokens = np.zeros(N, np.int64)
    st_in = np.zeros((N, _width(Tp)), np.float32)
    parents = []
    for u in range(n):
        T = lens[u]
        lp = lp_tm[u].astype(np.float64)
        for j, glen in enumerate((0, 1, 3, T + 2)):
            r = u * beam + j
            g = list(rng.randint(3, V, size=glen))
            c = int(g[-1]) if (j == 2 and g) else int(rng.randint(3, V))
            s = R.empty_state(lp, T)
            for lab in g:
                s = R.advance(s, int(lab), lp, T)
            s = R.State(s.rn.astype(np.float32).astype(np.float64), s.rb.astype(np.float32).astype(np.float64),
                        np.float64(np.float32(s.psi)), s.last)               # what the device holds
            parents.append(s)
            tokens[r] = c
            st_in[r] = _state_row(s, Tp)
            if V > 64 and j < 2:
                logits[r, eos] = 50.0                                      # EOS in the bank of these rows
            if V > 64 and j == 2:
                logits[r, 100:170] = 60.0                                  # 70 equal logits across the cut: the 64 largest token ids
            if V > 64 and j == 1:
                # a token outside the attention top-64 whose CTC column is the best of the row: it stays out (-inf)
                bank = set(R.candidate_bank(logits[r]).tolist())
                out_tok = next(v for v in range(3, V) if v not in bank)
                lp_tm[u, :, out_tok] = 0.0
    lp_cm = np.ascontiguousarray(lp_tm.transpose(0, 2, 1))
    for t in (1, 0):
        joint, st_out = _run_step(lp_cm, lens, logits, st_in, tokens, beam, t, LAM)
        joint2, st_out2 = _run_step(lp_cm, lens, logits, st_in, tokens, beam, t, LAM)
        assert np.array_equal(joint.view(np.int32), joint2.view(np.int32)) and np.array_equal(st_out.view(np.int32), st_out2.view(np.int32))
        for u in range(n):
            T = lens[u]
            lp = lp_tm[u].astype(np.float64)
            for j in range(beam if t > 0 else 1):
                r = u * beam + j
                h = R.advance(parents[r], int(tokens[r]), lp, T) if t > 0 else R.empty_state(lp, T)
                if t == 0:
                    h.last = -1
                _check_state(st_out[r], h, Tp)
                bank = R.candidate_bank(logits[r])
                mask = np.zeros(V, bool)
                mask[bank] = True
                assert np.all(np.isneginf(joint[r][~mask])) and np.all(np.isfinite(joint[r][mask]))
                if V > 64 and j < 2:
                    assert mask[eos]
                if V > 64 and j == 2:
                    assert set(bank.tolist()) == set(range(106, 170))
                if h.psi < -1e9:
                    continue                                               # (LOGZERO - LOGZERO: rounding noise of 1e10-sized values)
                for v in bank:
                    ps = R.prefix_score(h, int(v), eos, lp, T)
                    if ps < -1e9:
                        assert joint[r, v] < logits[r, v] - LAM * 1e8
                        continue
                    ref = np.float32(logits[r, v]) + np.float32(LAM) * np.float32(ps - h.psi)
                    assert abs(joint[r, v] - ref) <= LAM * 2 * _tol(max(abs(ps), abs(h.psi))) + 1e-5 * abs(ref), (u, j, v, joint[r, v], ref)


@pytest.mark.parametrize("V", [30, 70])
def test_prefix_step_writes_live_rows_only(V):
    """The liveness rule of the per-step scorers, held directly: a row is written exactly when the pruning will rank it.  A row that is
    not live (step 0: every slot but 0; t >= Umax; a done utterance; t >= dec_step[u]; slot >= nlive[u]) keeps the sentinel bits in joint
    and state_out; a live row has the bits of the all-live launch of the same step.  V = 70 takes the top-64 bank kernel, which also
    writes -inf to its rows"""
    rng = np.random.RandomState(V)
    n, beam, Tp = 3, 4, 7
    N, SENT = n * beam, 7.0                                                # (joint's fill in _run_step; state_out gets the same)
    lens = [7, 4, 1]
    lp_cm = np.ascontiguousarray(torch.log_softmax(torch.tensor(rng.randn(n, Tp, V + 1) * 2.0, dtype=torch.float32), -1).numpy()
                                 .transpose(0, 2, 1))
    logits = (rng.randn(N, V) * 3.0).astype(np.float32)
    tokens = rng.randint(3, V, size=N)
    st_in = np.zeros((N, _width(Tp)), np.float32)
    st_in[:, :2 * Tp] = -np.abs(rng.randn(N, 2 * Tp)) * 3.0                  # any finite parent state: only the bits are compared
    st_in[:, 2 * Tp], st_in[:, 2 * Tp + 1] = -1.0, rng.randint(3, V, size=N)
    run = lambda t, **kw: _run_step(lp_cm, lens, logits, st_in, tokens, beam, t, LAM, fill=SENT, **kw)
    bits = lambda x: x.view(np.int32)
    full = {t: run(t) for t in (0, 1)}
    slot = np.tile(np.arange(beam), n)
    utt = np.repeat(np.arange(n), beam)
    assert not np.any(full[1][0] == SENT) and not np.any(full[1][1][:, 2 * Tp] == SENT)      # all-live: every row written
    cases = [(0, {}, slot == 0),
             (1, dict(nlive=[4, 2, 0]), slot < np.repeat([4, 2, 0], beam)),
             (1, dict(done=[0, 1, 0]), utt != 1),
             (1, dict(dec_step=[1000, 1, 2]), utt != 1),
             (1, dict(Umax=1), np.zeros(N, bool))]
    for t, kw, live in cases:
        joint, st_out = run(t, **kw)
        assert np.all(bits(joint[~live]) == bits(np.float32(SENT))) and np.all(bits(st_out[~live]) == bits(np.float32(SENT))), (t, kw)
        assert np.array_equal(bits(joint[live]), bits(full[t][0][live])) and np.array_equal(bits(st_out[live]), bits(full[t][1][live])), (t, kw)
        if live.any():
            assert not np.any(joint[live] == SENT) and not np.any(st_out[live][:, 2 * Tp] == SENT), (t, kw)


def test_log_softmax_is_class_major():
    from las import _hip
    rng = np.random.RandomState(3)
    for n, Tp, Vc in ((2, 70, 31), (1, 5, 5001)):
        x = torch.tensor(rng.randn(n, Tp, Vc) * 3.0, dtype=torch.float32).cuda()
        out = torch.empty(n, Vc, Tp, device="cuda")
        _hip.check(_hip.lib().las_ctc_log_softmax(_hip.p(x), n, Tp, Vc, _hip.p(out), _hip.stream()), "las_ctc_log_softmax")
        ref = torch.log_softmax(x.double(), -1).transpose(1, 2)
        assert (out.double() - ref).abs().max().item() < 2e-5


# ---- the search
def _oracle_lp(xs, p0, args, cell):
    """the CTC head's log-probabilities [T', V + 1] of one utterance from the oracle's listener (float64)"""
    from oracle import las_oracle as O
    po = O.to_torch(p0)
    with torch.no_grad():
        if str(args.enc_type).lower() == "cnn":
            class _Fresh(dict):
                def __missing__(self, k):
                    return torch.tensor(1.0 if k.endswith("moving_variance") else 0.0)
            h, el = O.cnn_listener(torch.tensor(xs[0]), xs[1], po, args, cell, False, buffers=_Fresh(fresh=True))
        else:
            h, el = O.pblstm_listener(torch.tensor(xs[0]).reshape(1, -1, 39), xs[1], po, args.num_enc_layers, cell)
        z = O._mm(h[0], po["Speller/dense/kernel"]).double() + po["Speller/dense/bias"].double()     # (the current arithmetic mode)
    return torch.log_softmax(z, -1).numpy(), int(np.asarray(el).reshape(-1)[0])


def _model(enc_type, cell, **over):
    from oracle import las_oracle as O
    from las import layers as L, variables as V
    from las.las import LAS, Listener, Speller
    from las.beam_search import BeamSearch
    from utils.tokenizer import CharEncoder
    args = C._cfg_args(enc_type, "add", **dict(dict(convert_rate=0.3, beam_size=4, apply_lm=False, ctc_decode_weight=LAM), **over))
    p0 = O.init_params(args, seed=11, cell=cell, enc_type=enc_type)
    p0["Speller/decode/dense/bias"][2] = 0.3                  # let some hypotheses end
    hidden = 2 * args.enc_units if enc_type == "pblstm" else args.enc_units
    if args.ctc:
        p0.update(C._head_params(args, hidden))
    L.set_cell(cell)
    L.set_precision("f32")
    st = V.reset_default_store(device="cuda")
    st.load(p0)
    las = LAS(args, Listener, Speller, CharEncoder().token_to_id)
    las.build_variables()
    return args, p0, BeamSearch(args, las, CharEncoder().token_to_id, None)


def _utts(args):
    return [synthetic_batch(1, T, 12, args.vocab_size, seed=8 + k)[0] for k, T in enumerate((64, 48, 56))]


def _hyps(res):
    return [[(list(h.token_ids), float(h.log_prob)) for h in r] for r in res]


@pytest.mark.parametrize("enc_type,cell", [("pblstm", "lstm"), ("cnn", "rnn")])
def test_decode_batch_joint_matches_cpu_joint_search(enc_type, cell):
    """decode_batch with the CTC head against the CPU joint search; one utterance at a time, eager steps and decode_batches give the
    same bits; every EOS-terminated hypothesis' score is its attention score + weight x log p_ctc (telescoping)"""
    args, p0, bs = _model(enc_type, cell)
    utts = _utts(args)
    batch = bs.decode_batch(None, utts)
    assert any(batch)
    assert _hyps([bs.decode(None, xs) for xs in utts]) == _hyps(batch)
    bs.use_graph = False
    assert _hyps(bs.decode_batch(None, utts)) == _hyps(batch)
    bs.use_graph = True
    streamed = [r for res in bs.decode_batches(None, [utts[:2], utts[2:]]) for r in res]
    assert _hyps(streamed) == _hyps(batch)
    n_eos = 0
    for xs, res in zip(utts, batch):
        lp, T = _oracle_lp(xs, p0, args, cell)
        step_fn, _, _, init, Tp, dec_step = _oracle_fns(xs, p0, args, cell, None)
        ref = R.joint_beam_search(step_fn, init, Tp, dec_step, 4, 1, 2, lp, T, LAM)
        got_best, ref_best = res[-1], ref[-1]
        if list(got_best.token_ids) == list(ref_best.token_ids):
            assert float(got_best.log_prob) == pytest.approx(float(ref_best.log_prob), abs=5e-3)
        else:                                                           # a near tie at the end: the margins must be within tolerance
            norm = lambda h: float(h.log_prob) / (len(h.token_ids) - 1)
            assert abs(norm(got_best) - norm(ref_best)) < 5e-3
        for h in res:
            ids = list(h.token_ids)
            if ids[-1] != 2:
                continue
            n_eos += 1
            att, _ = oracle_score_tokens(xs, p0, args, cell, ids)
            labels = ids[1:]
            nll = F.ctc_loss(torch.tensor(lp)[:T, None], torch.tensor([labels]), [T], [len(labels)], blank=args.vocab_size,
                             reduction="sum").item() if len(labels) <= T else 1e10
            if nll >= 1e9:
                continue
            want = att + LAM * (-nll)
            assert abs(float(h.log_prob) - want) < 5e-3 + 1e-4 * abs(want), (ids, float(h.log_prob), want)
    assert n_eos > 0


def test_weight_zero_is_bit_identical_to_a_model_without_the_head():
    outs = []
    for ctc in (True, False):
        args, p0, bs = _model("pblstm", "lstm", ctc=ctc, ctc_decode_weight=0.0)
        outs.append(_hyps(bs.decode_batch(None, _utts(args))))
    assert outs[0] == outs[1] and any(outs[0])


def test_refusals():
    """weight > 0 without --ctc, and a checkpoint without the head, raise ValueError before any launch"""
    with pytest.raises(ValueError, match="ctc"):
        _model("pblstm", "lstm", ctc=False)
    import tempfile
    from las import checkpoint
    with tempfile.TemporaryDirectory() as d:
        args, p0, bs = _model("pblstm", "lstm", ctc=False, ctc_decode_weight=0.0)
        checkpoint.save(d, 1)
        args, p0, bs = _model("pblstm", "lstm")
        with pytest.raises(ValueError, match="CTC head"):
            bs.restore_las(None, d, -1)


def test_decode_cli_with_ctc_decode_weight(tmp_path):
    cmd = [sys.executable, os.path.join(PKG, "decode.py"), "--synthetic", "True", "--unit", "char", "--feat_dim", "13", "--enc_type",
           "pblstm", "--enc_units", "64", "--num_enc_layers", "2", "--dec_units", "64", "--num_dec_layers", "1", "--attention_size", "32",
           "--embedding_size", "32", "--cell", "lstm", "--beam_size", "4", "--save_dir", str(tmp_path / "none"), "--ctc", "True",
           "--ctc_decode_weight", "0.3"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0 and "Dev WER" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run(cmd[:-4] + ["--ctc_decode_weight", "0.3"], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode != 0 and "ValueError" in r.stderr


def _close(res, ref, tol, all_tokens):
    """the device search against the CPU joint search: equal token sequences (all of them, or the best one), scores within tol; where the
    best sequences differ the two bests must be a near tie (equal normalised scores within tol)"""
    assert len(res) == len(ref) > 0
    if all_tokens:
        # (a hypothesis with more labels than frames scores ~LOGZERO: among such hypotheses the order is the rounding of 1e10-sized fp32
        #  values, not a ranking -- only the feasible ones are compared)
        res, ref = [h for h in res if float(h.log_prob) > -1e8], [h for h in ref if float(h.log_prob) > -1e8]
        assert res
        assert [list(h.token_ids) for h in res] == [list(h.token_ids) for h in ref]
        for a, b in zip(res, ref):
            assert float(a.log_prob) == pytest.approx(float(b.log_prob), abs=tol)
        return
    a, b = res[-1], ref[-1]
    if list(a.token_ids) == list(b.token_ids):
        assert float(a.log_prob) == pytest.approx(float(b.log_prob), abs=tol)
    else:
        norm = lambda h: float(h.log_prob) / (len(h.token_ids) - 1)
        assert abs(norm(a) - norm(b)) < tol


def _same_bits_every_way(bs, utts, batch, one_at_a_time):
    """one utterance at a time (optional), eager steps and decode_batches give the bits of decode_batch"""
    if one_at_a_time:
        assert _hyps([bs.decode(None, xs) for xs in utts]) == _hyps(batch)
    bs.use_graph = False
    try:
        assert _hyps(bs.decode_batch(None, utts)) == _hyps(batch)
    finally:
        bs.use_graph = True
    k = len(utts) // 2
    streamed = [r for res in bs.decode_batches(None, [utts[:k], utts[k:]]) for r in res]
    assert _hyps(streamed) == _hyps(bs.decode_batch(None, utts[:k]) + bs.decode_batch(None, utts[k:]))


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_joint_search_with_char_rnnlm_matches_cpu(prec):
    """--apply_lm with the CTC head: the 2 x 512 char RNNLM's term is part of the logit (joint_beam_search with lm_fn), beam 16.  bf16 runs
    24 utterances = 384 rows, where the LM's recurrent state follows the hypotheses as bf16 copies (the state-copy gather slots re-pointed
    every step, beside the CTC state's slot)"""
    from las import layers as L, variables as V
    from las.las import LAS, Listener, Speller
    from las.beam_search import BeamSearch
    from lang.char_rnn_model import CharRNN
    from oracle import las_oracle as O
    from utils.tokenizer import CharEncoder
    from helpers import lm_params, make_args, oracle_lm, oracle_mode_for
    cell = "lstm"
    args = make_args(enc_units=64, num_enc_layers=2, dec_units=128, num_dec_layers=1, embedding_size=64, attention_size=64,
                     beam_size=16, convert_rate=0.2, apply_lm=True, lm_weight=0.5, ctc=True, ctc_decode_weight=LAM)
    p0 = O.init_params(args, seed=33, cell=cell)
    p0["Speller/decode/dense/bias"][2] = 0.5
    p0.update(C._head_params(args, 2 * args.enc_units))
    plm = lm_params(np.random.RandomState(8), 28, 0, 512, 2)
    for k in plm:
        plm[k] = (plm[k] * 0.3).astype(np.float32)
    L.set_cell(cell)
    L.set_precision(prec)
    st = V.reset_default_store(device="cuda")
    st.load(p0)
    st.load(plm)
    las = LAS(args, Listener, Speller, CharEncoder().token_to_id)
    lm = CharRNN(False, 1, 1, 28, 512, embedding_size=0, num_layers=2)
    bs = BeamSearch(args, las, CharEncoder().token_to_id, lm)
    n = 24 if prec == "bf16" else 2
    if prec == "bf16":
        assert lm.twins_ok(lm.fusion_plan(np.float32(0.5)), n * 16)
    utts = [synthetic_batch(1, T, 8, 30, seed=40 + k)[0] for k, T in enumerate([60, 47] + [52 + (k % 5) * 3 for k in range(n - 2)])]
    batch = bs.decode_batch(None, utts)
    _same_bits_every_way(bs, utts, batch, one_at_a_time=prec == "f32")
    olm = (oracle_lm(plm, 0, 2), 512, 2)
    O.set_precision(*oracle_mode_for(args, prec))
    try:
        for xs, res in zip(utts[:2], batch[:2]):
            lp, T = _oracle_lp(xs, p0, args, cell)
            step_fn, lm_fn, lm0, init, Tp, dec_step = _oracle_fns(xs, p0, args, cell, olm)
            ref = R.joint_beam_search(step_fn, init, Tp, dec_step, 16, 1, 2, lp, T, LAM, lm_fn=lm_fn, lm_init=lm0, lm_weight=0.5)
            _close(res, ref, 5e-3 if prec == "f32" else 8e-2, all_tokens=prec == "f32")
    finally:
        O.set_precision("f32")


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_subword_v5000_location_aware_bank_binds(prec):
    """V = 5000, location-aware attention: the top-64 bank binds inside the search.  Token X has a low attention logit (outside every
    row's top 64) and the CTC head puts nearly all mass on it, so without the cut X would have the best joint score of the first step;
    no hypothesis contains it, and the search equals the CPU joint search"""
    from las import layers as L, variables as V
    from las.las import LAS, Listener, Speller
    from las.beam_search import BeamSearch
    from oracle import las_oracle as O
    from helpers import make_args, oracle_mode_for
    X = 4000
    args = make_args(enc_units=48, num_enc_layers=2, dec_units=64, num_dec_layers=1, embedding_size=32, attention_size=32, unit="subword",
                     vocab_size=5000, mode="loc", loc_kernel_size=7, loc_num_channels=3, beam_size=4, convert_rate=0.3, apply_lm=False,
                     ctc=True, ctc_decode_weight=LAM)
    p0 = O.init_params(args, seed=5, cell="lstm")
    p0["Speller/decode/dense/kernel"] = (p0["Speller/decode/dense/kernel"] * 6).astype(np.float32)
    p0["Speller/decode/dense/bias"][2] = 1.5
    p0["Speller/decode/dense/kernel"][:, X] = 0.0
    p0["Speller/decode/dense/bias"][X] = -8.0
    p0.update(C._head_params(args, 2 * args.enc_units))
    p0["Speller/dense/bias"][X] = 60.0
    L.set_cell("lstm")
    L.set_precision(prec)
    st = V.reset_default_store(device="cuda")
    st.load(p0)
    tok = {"<PAD>": 0, "<SOS>": 1, "<EOS>": 2}
    las = LAS(args, Listener, Speller, tok)
    bs = BeamSearch(args, las, tok, None)
    utts = [synthetic_batch(1, T, 8, 30, seed=3 + k)[0] for k, T in enumerate((37, 52))]
    got = bs.decode_batch(None, utts)
    _same_bits_every_way(bs, utts, got, one_at_a_time=prec == "f32")
    O.set_precision(*oracle_mode_for(args, prec))
    try:
        for xs, res in zip(utts, got):
            assert all(X not in h.token_ids for h in res)
            lp, T = _oracle_lp(xs, p0, args, "lstm")
            step_fn, _, _, init, Tp, dec_step = _oracle_fns(xs, p0, args, "lstm", None)
            lg0 = np.asarray(step_fn([1], [np.zeros(Tp, np.float32)], [init])[0][0], np.float32)
            assert X not in R.candidate_bank(lg0)
            no_cut = R.joint_scores(lg0, R.empty_state(lp, T), 2, lp, T, LAM, topn=args.vocab_size)
            assert int(np.argmax(no_cut)) == X                             # the construction binds
            ref = R.joint_beam_search(step_fn, init, Tp, dec_step, 4, 1, 2, lp, T, LAM)
            _close(res, ref, 2e-3 if prec == "f32" else 5e-2, all_tokens=prec == "f32")
    finally:
        O.set_precision("f32")
