"""The --mwer train step on the tiny synthetic model of the GPU step tests (V = 30, 30 frames, B = 2, K = 3; the references
have at most 8 steps, given hypotheses one more, drawn ones four more: U <= 12), fp32 parity mode: the loss kernels' plumbing against tests/mwer_ref.py, the step's gradient against a directional finite difference of
LAS.mwer_risk, its cross-entropy-only limit against the plain step, the drawn hypotheses, and what the step refuses."""
import numpy as np
import pytest
import torch

import mwer_ref as M
import nbest_ref as NB
from helpers import make_args, synthetic_batch

pytestmark = pytest.mark.gpu
CELL, K = "lstm", 3


def _args(**over):
    kw = dict(enc_units=64, num_enc_layers=2, dec_units=64, num_dec_layers=1, embedding_size=32, attention_size=32, mwer=True, mwer_hyps=K,
              mwer_unit="token", grad_clip=0.0, lr=0.0)
    kw.update(over)
    return make_args(**kw)


def _las(args, id_to_token=None):
    from las import layers as L, variables as V
    from las.las import LAS, Listener, Speller
    from oracle import las_oracle as O
    p0 = O.init_params(args, seed=2, cell=CELL)
    L.set_cell(CELL)
    L.set_precision("f32")
    st = V.reset_default_store(device="cuda")
    st.load(p0)
    return LAS(args, Listener, Speller, id_to_token or {}), st


def _batch():
    xs, ys = synthetic_batch(2, 30, 8, 30, seed=1)
    refs = [[int(t) for t in ys[0][u, :ys[1][u]]] for u in range(2)]
    # utterance 0: the reference itself, one substitution, a shorter string without its EOS; utterance 1: two hypotheses (one slot unused)
    h0 = [list(refs[0]), [refs[0][0] % 27 + 3] + refs[0][1:], refs[0][:1]]
    h1 = [refs[1][:-1] + [5, 2], [7] + refs[1]]
    return xs, ys, refs, [h0, h1]


def _step(las, st, xs, ys, **kw):
    out = las.train(xs, ys, **kw)
    torch.cuda.synchronize()
    las.check_status()
    assert las.recovered_steps == 0
    return out


def test_plumbing_dlogits_and_error_counts_match_the_restatement():
    from utils.tokenizer import CharEncoder
    xs, ys, refs, hyps = _batch()
    a = _args(lr=1e-3)
    las, st = _las(a)
    las.keep_mwer_logits = True
    loss, _, gs, logits, alphas, summ, _ = _step(las, st, xs, ys, hyps=hyps)
    r = las.last_mwer
    S, n = K + 1, 2
    z, y, lens, nh, err = (r[k].cpu().numpy() for k in ("logits", "y", "lens", "nhyp", "err"))
    assert z.shape[0] == n * S and nh.tolist() == [3, 2] and gs == 1 and logits.shape[0] == n
    # the error counts: token edit distances to the reference (strings without their EOS), 0 in the reference's and the unused slot
    want = np.zeros((n, S), np.float32)
    for u in range(n):
        for k, h in enumerate(hyps[u]):
            cut = h[:h.index(2)] if 2 in h else h
            want[u, k] = NB.distance(refs[u][:-1], cut)
    assert np.array_equal(err.reshape(n, S), want), (err, want)
    assert want[0].tolist() == [0, 1, len(refs[0]) - 2, 0]
    # the gradient on the logits: the restatement's MWER term over all rows, the reference rows' cross entropy in the reference's slot
    scale = np.float32(1.0 / n)
    ref = M.mwer(z, y, lens, nh, err, S, 0, scale, np.float64)
    g = ref["dlogits"].copy()
    U, V = z.shape[1], z.shape[2]
    ntok = np.float32((ys[0][:, :int(ys[1].max())] != 0).sum())
    ce_scale = np.float64(np.float32(a.mwer_ce_weight) * (np.float32(1.0) / (ntok + np.float32(1e-9))))
    ce = 0.0
    for u in range(n):
        zr = z[u * S + K].astype(np.float64)
        lse = np.log(np.exp(zr - zr.max(-1, keepdims=True)).sum(-1)) + zr.max(-1)
        for t in range(U):
            lab = int(ys[0][u, t]) if t < ys[0].shape[1] else 0
            if lab == 0:
                continue
            soft = np.full(V, 0.01 / V)
            soft[lab] += 0.99
            g[u * S + K, t] = ce_scale * (np.exp(zr[t] - lse[t]) - soft)
            ce += -(soft * (zr[t] - lse[t])).sum()
    tol = 4.0 * M.measured_tolerance()["dlogits"]
    d = float(np.abs(r["dlogits"].cpu().numpy() - g).max())
    print("step dlogits: max |device - float64|", d, "allowed", tol, "largest", np.abs(g).max())
    assert d <= tol and np.abs(ref["dlogits"]).max() > 1e-3
    assert abs(float(summ["mwer_risk"]) - float(ref["loss"])) <= 4.0 * M.measured_tolerance()["loss"]
    assert abs(float(summ["mwer_ce"]) - ce / float(ntok)) < 1e-4 * max(1.0, ce / float(ntok))
    assert abs(float(loss) - (float(ref["loss"]) + a.mwer_ce_weight * ce / float(ntok))) < 1e-5
    # the word count of the same hypotheses through the device's distance kernel
    from las import mwer
    enc = CharEncoder()
    werr = mwer.word_errors(refs, hyps, enc.id_to_token, "char", "word")
    wnp = mwer.word_errors(refs, hyps, enc.id_to_token, "char", "word", distance=NB.distance)
    assert [e.tolist() for e in werr] == [e.tolist() for e in wnp] and len(werr[0]) == 3 and len(werr[1]) == 2
    terr = mwer.word_errors(refs, hyps, enc.id_to_token, "char", "token")
    assert [e.tolist() for e in terr] == [want[0, :3].tolist(), want[1, :2].tolist()]


def _probe(args, xs, ys, d, eps, hyps=None):
    """-> (<flat_grad, d>, central difference of the loss along d): the gradient from one train step (lr = 0: nothing moves), the loss
    from mwer_risk under --mwer and from the step's own return value otherwise"""
    las, st = _las(args)
    _step(las, st, xs, ys, **({"hyps": hyps} if args.mwer else {}))
    theta, g = st.flat.detach().clone(), st.flat_grad.detach().clone()
    dd = d.to(theta.device)
    vals = []
    for sgn in (1.0, -1.0):
        with torch.no_grad():
            st.flat.copy_(theta + sgn * eps * dd)
        st.weights_changed()
        if args.mwer:
            vals.append(float(las.mwer_risk(xs, ys, hyps)[0]))
        else:
            vals.append(float(_step(las, st, xs, ys)[0]))
    return float((g.double() * dd.double()).sum()), (vals[0] - vals[1]) / (2 * eps)


def test_directional_derivative_against_the_plain_step():
    """<flat_grad, d> against (loss(theta + eps d) - loss(theta - eps d)) / 2 eps for one fixed random d, clipping off, dropout 0.  The bar
    is the plain cross-entropy step's own relative error in the same probe (same model, eps, d) times 4: the MWER step sums over S times
    the rows.  eps d moves every parameter by 2e-4 (d ~ N(0, 1)): the loss' fp32 rounding (~1e-6 relative) over 2 eps and the third-order
    term of the central difference both stay below a per cent of a derivative of the gradient's own size."""
    xs, ys, refs, hyps = _batch()
    las, st = _las(_args())
    las.build_variables()
    n = st.flat.numel()
    d = torch.randn(n, generator=torch.Generator().manual_seed(5))
    eps = 2e-4
    gd_p, fd_p = _probe(_args(mwer=False), xs, ys, d, eps)
    gd_m, fd_m = _probe(_args(), xs, ys, d, eps, hyps)
    rel_p, rel_m = abs(fd_p - gd_p) / abs(gd_p), abs(fd_m - gd_m) / abs(gd_m)
    print("plain step: <g, d> %.6g, difference quotient %.6g, relative error %.3g" % (gd_p, fd_p, rel_p))
    print("mwer step:  <g, d> %.6g, difference quotient %.6g, relative error %.3g" % (gd_m, fd_m, rel_m))
    assert rel_m <= 4.0 * rel_p, (rel_m, rel_p)


def test_cross_entropy_only_limit_equals_the_plain_step():
    """every hypothesis equal to the reference: all error counts are 0, the MWER term has no gradient, and with mwer_ce_weight = 1 the
    step's gradient is the plain step's -- the same terms summed over S times the rows (the tolerance of the parity tests for a
    re-ordered fp32 sum: 1e-3 of the largest entry)"""
    xs, ys, refs, _ = _batch()
    las, st = _las(_args(mwer_ce_weight=1.0))
    loss_m = float(_step(las, st, xs, ys, hyps=[[list(r)] * K for r in refs])[0])
    assert (las.last_mwer["err"] == 0).all() and float(las.last_mwer["loss"][0]) == 0.0
    g_m = st.flat_grad.detach().clone()
    las, st = _las(_args(mwer=False))
    loss_p = float(_step(las, st, xs, ys)[0])
    g_p = st.flat_grad.detach().clone()
    d = (g_m - g_p).abs().max().item()
    print("ce-only limit: max |difference| %.3g of %.3g" % (d, g_p.abs().max().item()))
    assert d <= 1e-3 * max(1.0, g_p.abs().max().item()) and g_p.abs().max().item() > 1e-3
    assert abs(loss_m - loss_p) < 1e-5 * max(1.0, abs(loss_p))


def test_drawn_hypotheses():
    xs, ys, refs, _ = _batch()
    S, n = K + 1, 2
    runs = []
    for _ in range(2):
        las, st = _las(_args())
        _, _, _, _, _, summ, _ = _step(las, st, xs, ys)
        r = las.last_mwer
        runs.append((r["y"].cpu().numpy(), r["lens"].cpu().numpy(), r["seq_lp"].cpu().numpy(), las))
    y, lens, seq_lp, las = runs[1]
    assert np.array_equal(runs[0][0], y) and np.array_equal(runs[0][1], lens)            # the same global step: the same tokens
    U = int(ys[1].max()) + 4
    assert y.shape == (n * S, U) and np.isfinite(float(summ["mwer_risk"]))
    hyps = []
    for u in range(n):
        rows = [y[u * S + k, :lens[u * S + k]].tolist() for k in range(K)]
        assert all(r[-1] == 2 and 2 not in r[:-1] and 0 < len(r) <= U for r in rows)
        assert len({tuple(r) for r in rows}) >= 2, rows                                   # the slots' draws differ
        assert y[u * S + K, :lens[u * S + K]].tolist() == refs[u]                         # the reference's slot is the reference
        hyps.append(rows)
    # the same strings, teacher-forced: the same log-likelihoods
    _, _, lp = las.mwer_risk(xs, ys, hyps)
    lp = lp.cpu().numpy()
    got, want = lp[:, :K], seq_lp.reshape(n, S)[:, :K]
    tol = 4.0 * M.measured_tolerance()["seq_lp"]
    d = float(np.abs(got - want).max())
    print("drawn against teacher-forced seq_lp: max difference", d, "allowed", tol)
    assert np.isfinite(want).all() and np.isnan(lp[:, K]).all() and d <= tol


def test_refusals():
    from las import variables as V
    xs, ys, refs, hyps = _batch()
    for over, kw, setdp, msg in ((dict(ctc=True), {}, False, "--ctc"), ({}, {}, True, "data-parallel"), (dict(mwer_hyps=64), {}, False, "between 1 and 63"),
                                 ({}, dict(hyps=[[refs[0][:1] + [30]], []]), False, "outside \\[0, 30\\)"),
                                 ({}, dict(hyps=[hyps[0] + hyps[0], []]), False, "at most --mwer_hyps")):
        las, st = _las(_args(**over))
        if setdp:
            las.dp = object()
        with pytest.raises(ValueError, match=msg):
            las.train(xs, ys, **kw)
        assert st.global_step == 0 and len(las._recent) == 0
    las, st = _las(_args())
    with pytest.raises(ValueError, match="train_stacked"):
        las.train_stacked([(xs, ys), (xs, ys)])
    with pytest.raises(ValueError, match="coins= / sampled="):
        las.train(xs, ys, coins=np.ones(8, bool))
    assert st.global_step == 0 and las.last_mwer is None
    las, st = _las(_args(mwer=False))
    with pytest.raises(ValueError, match="hyps="):
        las.train(xs, ys, hyps=hyps)
    with pytest.raises(ValueError, match="--mwer True"):
        las.mwer_risk(xs, ys, hyps)
