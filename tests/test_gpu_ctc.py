"""Joint CTC-attention training (reference las/las.py:75-77, 259-261, 335-349; tf.nn.ctc_loss): the las_ctc_loss kernels against
torch.nn.functional.ctc_loss in float64, and one LAS.train step with --ctc against the oracle's step plus the CTC term."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import grad_errors, make_args, oracle_mode_for, row_mode, synthetic_batch
from loss_ref import ctc_ref as _reference          # (per-row float64 torch ctc_loss: nll and gradient, None where torch cannot align)

pytestmark = pytest.mark.gpu


# ---- the kernels -------------------------------------------------------------------------------------------------------------
def _case(B, Tp, Vc, seed, drop):
    """logits, labels (forced repeats, a row with L = 0), ragged enc_len."""
    rng = np.random.RandomState(seed)
    logits = rng.randn(B, Tp, Vc).astype(np.float32) * 2.0
    U = max(2, Tp // 3)
    y = np.zeros((B, U + 2), np.int32)                   # (two spare columns: ldy > U)
    enc_len = rng.randint(max(1, Tp // 2), Tp + 1, size=B).astype(np.int32)
    enc_len[0] = Tp
    for b in range(B):
        if b == 1 % B and B > 1:
            continue                                      # row 1: no labels
        n = rng.randint(1, max(2, enc_len[b] // 3) + 1)
        n = min(n, U)
        lab = rng.randint(1, Vc - 1, size=n)
        if n >= 3:
            lab[2] = lab[1]                               # a forced repeat
        y[b, :n] = lab
    return logits, y, U, enc_len


def _labels(y, U, drop_row):
    labs = [[int(v) for v in row[:U] if v != 0] for row in y]
    if drop_row >= 0 and labs[drop_row]:
        labs[drop_row] = labs[drop_row][:-1]
    return labs


def _run(logits, y, U, enc_len, drop_row, dtype=torch.float32, scale=1.0):
    from las import las as LL
    dev = torch.device("cuda")
    lg = torch.tensor(logits, device=dev)
    yy = torch.tensor(y, device=dev)[:, :U]               # a view: pitch ldy = U + 2 > U columns
    loss, nll, grad = LL._ctc_loss(lg, yy, torch.tensor(enc_len, device=dev), drop_row,
                                   torch.tensor([scale], device=dev), grad_dtype=dtype)
    torch.cuda.synchronize()
    return float(loss[0]), nll.cpu().numpy(), grad.float().cpu().numpy()


SHAPES = [(3, 7, 31), (5, 40, 31), (48, 160, 31), (4, 319, 5001)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("drop", [False, True])
def test_kernel_matches_torch_ctc(shape, drop):
    B, Tp, Vc = shape
    logits, y, U, enc_len = _case(B, Tp, Vc, seed=B * 1000 + Tp + int(drop), drop=drop)
    drop_row = B - 1 if drop else -1
    labs = _labels(y, U + 2, drop_row)
    nll_r, grad_r = _reference(logits, labs, enc_len)
    loss, nll, grad = _run(logits, y, U, enc_len, drop_row, scale=0.5)
    for b in range(B):
        assert np.isfinite(nll_r[b]), (b, "the generated case must be alignable")
        assert abs(nll[b] - nll_r[b]) <= 1e-5 * max(1.0, abs(nll_r[b])), (b, nll[b], nll_r[b])
        T = int(enc_len[b])
        assert np.abs(grad[b, :T] - 0.5 * grad_r[b][:T]).max() < 1e-5, b
        assert (grad[b, T:] == 0).all(), b                            # exact zeros behind the row's frames
    assert abs(loss - 0.5 * sum(nll_r)) <= 1e-5 * max(1.0, 0.5 * sum(nll_r))
    # bf16 gradient: within one bf16 ulp of the rounded reference
    _, nll16, g16 = _run(logits, y, U, enc_len, drop_row, dtype=torch.bfloat16, scale=0.5)
    assert (nll16 == nll).all()
    for b in range(B):
        T = int(enc_len[b])
        r = 0.5 * grad_r[b][:T]
        ulp = np.exp2(np.floor(np.log2(np.maximum(np.abs(r), 1e-30))) - 7)
        assert (np.abs(g16[b, :T] - r) <= np.maximum(ulp, 1e-6)).all(), b
        assert (g16[b, T:] == 0).all()


def test_kernel_bit_identical_runs():
    logits, y, U, enc_len = _case(48, 160, 31, seed=5, drop=True)
    a = _run(logits, y, U, enc_len, 47)
    b = _run(logits, y, U, enc_len, 47)
    assert a[0] == b[0] and (a[1] == b[1]).all() and (a[2] == b[2]).all()


def test_repeat_infeasible_row_gives_inf_and_zero_gradient():
    B, Tp, Vc = 4, 12, 31
    logits, y, U, enc_len = _case(B, Tp, Vc, seed=9, drop=False)
    # row 2: 4 labels with 3 repeats need 7 frames; give it 5 (L = 4 <= 5: the host check lets it through)
    y2 = y.copy()
    y2[2] = 0
    y2[2, :4] = [5, 5, 5, 5]
    e2 = enc_len.copy()
    e2[2] = 5
    loss, nll, grad = _run(logits, y2, U, e2, -1)
    assert nll[2] == np.inf and (grad[2] == 0).all()
    _, nll_ok, grad_ok = _run(logits, y, U, enc_len, -1)
    for b in (0, 1, 3):
        assert nll[b] == nll_ok[b] and (grad[b] == grad_ok[b]).all()


# ---- one training step --------------------------------------------------------------------------------------------------------
def _head_params(args, hidden, seed=5):
    rng = np.random.RandomState(seed)
    Vc = args.vocab_size + 1
    lim = np.sqrt(6.0 / (hidden + Vc))
    return {"Speller/dense/kernel": rng.uniform(-lim, lim, (hidden, Vc)).astype(np.float32),
            "Speller/dense/bias": (rng.randn(Vc) * 0.1).astype(np.float32)}


def _oracle_ctc_step(p0, args, cell, xs, ys, coins):
    """oracle.train_step restated with the CTC term: the oracle's listener, speller_forward and las_loss, the head through the
    oracle's _mm, F.ctc_loss with the reference's last-label drop, clip_by_global_norm and adam_tf."""
    from oracle import las_oracle as O
    p = O.to_torch(p0, requires_grad=True)
    audio, audiolen = torch.tensor(xs[0]), xs[1]
    y, tokenlen = torch.tensor(ys[0]), ys[1]
    B = audio.shape[0]
    dec_steps = int(np.max(np.asarray(tokenlen)))
    if str(args.enc_type).lower() == "cnn":
        h, enc_len = O.cnn_listener(audio, audiolen, p, args, cell, True)
    else:
        h, enc_len = O.pblstm_listener(audio.reshape(B, -1, args.feat_dim * 3), audiolen, p, args.num_enc_layers, cell)
    logits, alphas = O.speller_forward(h, enc_len, dec_steps, p, args, cell, teacher=y, is_training=True, coins=coins)
    att = O.las_loss(logits, y, args.vocab_size, args.label_smoothing)
    ctc_logits = O._mm(h, p["Speller/dense/kernel"]) + p["Speller/dense/bias"]
    labs = _labels(np.asarray(ys[0]), ys[0].shape[1], B - 1)
    flat = torch.tensor([v for l in labs for v in l], dtype=torch.long)
    lens = torch.tensor([len(l) for l in labs])
    il = torch.as_tensor(np.asarray(enc_len, np.float64)).to(torch.int64).reshape(-1)
    nll = F.ctc_loss(torch.log_softmax(ctc_logits, -1).transpose(0, 1), flat, il, lens, blank=args.vocab_size, reduction="none")
    loss = att + args.ctc_weight * nll.mean()
    names = sorted(p)
    grads = torch.autograd.grad(loss, [p[n] for n in names], allow_unused=True)
    grads = [g if g is not None else torch.zeros_like(p[n]) for g, n in zip(grads, names)]
    gdict = dict(zip(names, grads))
    if args.grad_clip > 0:
        grads, _ = O.clip_by_global_norm(grads, args.grad_clip)
    lr = O.scheduled_learning_rate(args.lr, 0)
    newp = {n: O.adam_tf(p[n].detach(), g, torch.zeros_like(g), torch.zeros_like(g), 1, lr)[0] for n, g in zip(names, grads)}
    return float(loss), logits.detach(), gdict, newp


def _hip_step(args, cell, prec, p0, xs, ys, coins):
    from las import _hip, layers as L, variables as V
    from las.las import LAS, Listener, Speller
    L.set_cell(cell)
    L.set_precision(prec)
    st = V.reset_default_store(device="cuda")
    st.load(p0)
    las = LAS(args, Listener, Speller, {})
    out = las.train(xs, ys, coins=coins)
    torch.cuda.synchronize()
    las.check_status()
    if las.recovered_steps:
        out = las.last_out
    fam = _hip.speller_last_variant()
    return dict(loss=float(out[0]), logits=out[3].cpu(), summ=out[5], fam=fam, las=las,
                grads={n: st.vars[n].grad.detach().cpu().clone() for n in st.order},
                params={n: st.vars[n].detach().cpu().clone() for n in st.order})


TOL = {("f32", "lstm"): dict(logits=5e-4, loss=1e-4, grad=2e-3), ("f32", "rnn"): dict(logits=5e-4, loss=1e-4, grad=2e-3),
       ("bf16", "lstm"): dict(logits=4e-3, loss=2e-3, grad=2e-2), ("bf16", "rnn"): dict(logits=3e-2, loss=5e-3, grad=0.1)}

CONFIGS = [
    # enc_type, cell, mode, prec
    ("pblstm", "rnn", "add", "f32"),
    ("pblstm", "lstm", "loc", "f32"),
    ("pblstm", "rnn", "loc", "f32"),
    ("pblstm", "lstm", "add", "bf16"),
    ("pblstm", "rnn", "add", "bf16"),
    ("cnn", "lstm", "add", "f32"),
    ("cnn", "rnn", "loc", "f32"),
]


def _drop_zero_gradient_biases(errs, g_o, grads, prec):
    """The CNN listener's dense layers feed a normalisation (las/layers.py:155-161), so their biases have an identically zero gradient: both
    sides hold the rounding noise of a cancelling sum there.  Held to an absolute bound, as tests/test_gpu_run_sh_recipe.py does."""
    for n in [k for k in errs if k.startswith("Listener/blstm_") and k.endswith("/dense/bias")]:
        assert float(g_o[n].abs().max()) < 1e-4 and float(grads[n].abs().max()) < (1e-4 if prec == "f32" else 5e-3), n
        del errs[n]


def _cfg_args(enc_type, mode, **over):
    H = 64
    a = dict(enc_type=enc_type, enc_units=H, num_enc_layers=2, dec_units=64, num_dec_layers=1, embedding_size=32,
             attention_size=32, mode=mode, loc_kernel_size=11, loc_num_channels=3, lr=1e-3, grad_clip=5.0, ctc=True, ctc_weight=0.3)
    if enc_type == "cnn":
        a.update(num_enc_channels=8, apply_bn=False)     # (the CNN sizes of tests/test_gpu_las_parity.py)
    a.update(over)
    return make_args(**a)


@pytest.mark.parametrize("cfg", CONFIGS)
def test_train_step_with_ctc_matches_oracle(cfg):
    from oracle import las_oracle as O
    enc_type, cell, mode, prec = cfg
    args = _cfg_args(enc_type, mode)
    xs, ys = synthetic_batch(5, 64, 12, args.vocab_size, seed=7)
    U = int(ys[1].max())
    coins = np.ones(U, bool)
    p0 = O.init_params(args, seed=11, cell=cell, enc_type=enc_type)
    hidden = 2 * args.enc_units if enc_type == "pblstm" else args.enc_units
    p0.update(_head_params(args, hidden))
    r = _hip_step(args, cell, prec, p0, xs, ys, coins)
    O.set_precision(*oracle_mode_for(args, prec, rows=row_mode(r["fam"])))
    try:
        loss_o, logits_o, g_o, newp = _oracle_ctc_step(p0, args, cell, xs, ys, coins)
    finally:
        O.set_precision("f32")
    tol = TOL[(prec, cell)]
    assert set(r["grads"]) == set(g_o)
    assert (r["logits"] - logits_o).abs().max().item() < tol["logits"]
    assert abs(r["loss"] - loss_o) < tol["loss"] * max(1.0, abs(loss_o)), (r["loss"], loss_o)
    assert abs(float(r["summ"]["att_loss"]) + 0.3 * float(r["summ"]["ctc_loss"]) - r["loss"]) < 1e-4 * max(1.0, r["loss"])
    errs = grad_errors(dict(names=sorted(g_o), g_o=g_o, grads=r["grads"]))
    if enc_type == "cnn":
        _drop_zero_gradient_biases(errs, g_o, r["grads"], prec)
    for n, e in errs.items():
        assert e < tol["grad"], (n, e)
    assert r["grads"]["Speller/dense/kernel"].abs().max() > 0
    if prec == "f32":
        for n in errs:                  # (Adam's first step is ~lr * sign(g): a zero-gradient bias's update is the sign of noise)
            assert (r["params"][n] - newp[n]).abs().max().item() < 2e-4, n


def test_ctc_weight_zero_leaves_shared_gradients_bit_identical():
    from oracle import las_oracle as O
    args = _cfg_args("pblstm", "add", ctc_weight=0.0)
    xs, ys = synthetic_batch(5, 64, 12, args.vocab_size, seed=3)
    coins = np.ones(int(ys[1].max()), bool)
    p0 = O.init_params(args, seed=11, cell="lstm", enc_type="pblstm")
    p_head = dict(p0, **_head_params(args, 2 * args.enc_units))
    on = _hip_step(args, "lstm", "bf16", p_head, xs, ys, coins)
    args_off = _cfg_args("pblstm", "add", ctc=False)
    off = _hip_step(args_off, "lstm", "bf16", p0, xs, ys, coins)
    for n, g in off["grads"].items():
        assert torch.equal(on["grads"][n], g), n
    for n in ("Speller/dense/kernel", "Speller/dense/bias"):
        assert (on["grads"][n] == 0).all()
    assert on["loss"] == off["loss"]


def test_stacked_batches_equal_one_concatenated_batch():
    """The global-batch rule: train_stacked of two batches is train on their concatenation (the drop and the division by the row
    count belong to the whole batch)."""
    from oracle import las_oracle as O
    args = _cfg_args("pblstm", "add")
    xa, ya = synthetic_batch(3, 64, 12, args.vocab_size, seed=21)
    xb, yb = synthetic_batch(3, 64, 12, args.vocab_size, seed=22)
    p0 = dict(O.init_params(args, seed=11, cell="rnn", enc_type="pblstm"), **_head_params(args, 2 * args.enc_units))
    U = int(max(ya[1].max(), yb[1].max()))
    coins = np.ones(U, bool)
    from las import layers as L, variables as V
    from las.las import LAS, Listener, Speller
    L.set_cell("rnn")
    L.set_precision("f32")
    st = V.reset_default_store(device="cuda")
    st.load(p0)
    las = LAS(args, Listener, Speller, {})
    out = las.train_stacked([(xa, ya), (xb, yb)], coins=coins)
    torch.cuda.synchronize()
    g1 = {n: st.vars[n].grad.detach().cpu().clone() for n in st.order}
    xs = (np.concatenate([xa[0], xb[0]]), np.concatenate([xa[1], xb[1]]))
    ys = (np.concatenate([ya[0], yb[0]]), np.concatenate([ya[1], yb[1]]))
    r = _hip_step(args, "rnn", "f32", p0, xs, ys, coins)
    for n, g in r["grads"].items():
        assert torch.equal(g, g1[n]), n
    assert float(out[0]) == r["loss"]


def test_label_longer_than_frames_raises_before_launch():
    from oracle import las_oracle as O
    from las import layers as L, variables as V
    from las.las import LAS, Listener, Speller
    args = _cfg_args("pblstm", "add", num_enc_layers=3)
    xs, ys = synthetic_batch(3, 64, 16, args.vocab_size, seed=4)     # T' = 8, labels ~ 0.15 T = 10
    p0 = dict(O.init_params(args, seed=11, cell="rnn", enc_type="pblstm"), **_head_params(args, 2 * args.enc_units))
    L.set_cell("rnn")
    L.set_precision("f32")
    st = V.reset_default_store(device="cuda")
    st.load(p0)
    las = LAS(args, Listener, Speller, {})
    with pytest.raises(ValueError, match="not enough time"):
        las.train(xs, ys)
    assert st.global_step == 0 and st.flat is None                   # nothing was built or launched


def test_inference_and_checkpoint_ignore_the_head(tmp_path):
    from oracle import las_oracle as O
    from las import checkpoint, layers as L, variables as V
    from las.las import LAS, Listener, Speller
    args = _cfg_args("pblstm", "add", convert_rate=0.3)
    xs, ys = synthetic_batch(3, 64, 12, args.vocab_size, seed=8)
    p0 = O.init_params(args, seed=11, cell="lstm", enc_type="pblstm")
    L.set_cell("lstm")
    L.set_precision("f32")
    # train one step with the head, save
    st = V.reset_default_store(device="cuda")
    st.load(dict(p0, **_head_params(args, 2 * args.enc_units)))
    las = LAS(args, Listener, Speller, {})
    las.train(xs, ys, coins=np.ones(int(ys[1].max()), bool))
    torch.cuda.synchronize()
    path = checkpoint.save(str(tmp_path), 1)
    saved = {n: st.vars[n].detach().cpu().clone() for n in st.order}
    lg_on, y_on = las.inference(xs)
    # the same weights in a model built with ctc (round trip) and without it (decode.py's case)
    outs = []
    for ctc in (True, False):
        a = _cfg_args("pblstm", "add", convert_rate=0.3, ctc=ctc)
        st = V.reset_default_store(device="cuda")
        m = LAS(a, Listener, Speller, {})
        m.build_variables()
        assert checkpoint.restore(str(tmp_path), 1) == path
        for n in st.order:
            assert torch.equal(st.vars[n].detach().cpu(), saved[n]), n
        assert ("Speller/dense/kernel" in st.vars) == ctc
        outs.append(m.inference(xs))
    for lg, yh in outs:
        assert torch.equal(lg.cpu(), lg_on.cpu()) and torch.equal(yh.cpu(), y_on.cpu())
