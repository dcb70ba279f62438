"""K9 (csrc/loss_opt.hip: las_sumsq + las_clip_adam) past its first step: the kernels alone on the shapes and edges where a
vectorised, grid-strided update goes wrong, then inside LAS.train and the char RNNLM over several steps -- every launch held to
tests/adam_ref.py (float64, the bounds derived there by counting fp32 roundings) applied to the device's own state and gradients, so
the 2e-3 gradient tolerance of the parity tests does not enter.  tests/test_adam_ref_host.py shows that these bounds tell a wrong
clip scale, swapped betas, a misplaced eps, lr for lr_t, a skipped tail and moments that are not written back from a correct kernel."""
import math

import numpy as np
import pytest
import torch

import adam_ref as R
from helpers import make_args, synthetic_batch

pytestmark = pytest.mark.gpu

B1, B2, EPS, LR = 0.9, 0.999, 1e-8, 1e-3
SENT = -77.0
WRAP = 3 * 2048 * 256 * 4 + 3          # more float4 elements than the 2048 x 256 threads las_clip_adam launches at most: the grid-stride loop wraps


def make_g(rng, n):
    """gradients over nine decades (|g| ~ eps and below included), every seventh exactly zero (tests/test_adam_ref_host.py make_g)"""
    g = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-9, 0, n)).astype(np.float32)
    g[::7] = 0
    return g


def _buf(values, n):
    """n values followed by sentinels up to n + 4 rounded up (>= 4 sentinel floats behind the data)"""
    t = torch.full(((n + 4 + 3) // 4 * 4,), SENT, dtype=torch.float32, device="cuda")
    t[:n] = torch.from_numpy(np.asarray(values, np.float32))
    return t


def _sumsq(g, n, out=None, ws=None, ws_bytes=None):
    from las import _hip
    lib = _hip.lib()
    out = torch.full((1,), SENT, device="cuda") if out is None else out
    need = int(lib.las_sumsq_workspace_bytes(n))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda") if ws is None else ws
    rc = lib.las_sumsq(_hip.p(g), n, _hip.p(out), _hip.p(ws), need if ws_bytes is None else ws_bytes, _hip.stream())
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 262144 * 4 - 1, 262144 * 4 + 5, 11000003])
def test_sumsq_matches_float64(n):
    rng = np.random.RandomState(n % 1000)
    g = (rng.randn(n) * 10.0 ** rng.uniform(-4, 1, n)).astype(np.float32)
    gd = _buf(g, n)
    rc, out = _sumsq(gd, n)                                   # `out` holds a sentinel: it is assigned, not accumulated into
    assert rc == 0
    ref = R.sumsq_ref(g)
    got = float(out.item())
    print("sumsq n=%d: relative error %.3g, bound %.3g" % (n, abs(got - ref) / ref, R.sumsq_bound(n)))
    assert abs(got - ref) <= R.sumsq_bound(n) * ref
    rc2, out2 = _sumsq(gd, n)
    assert rc2 == 0 and torch.equal(out, out2)                # fixed-order reduction: the same bits
    assert float(gd[n:].min()) == SENT and float(gd[n:].max()) == SENT


def test_sumsq_edges():
    from las import _hip
    gd = _buf(np.ones(8), 8)
    rc, out = _sumsq(gd, 0)
    assert rc == 0 and float(out.item()) == 0.0               # n = 0: out[0] = 0
    out = torch.full((1,), SENT, device="cuda")
    rc, _ = _sumsq(gd[1:], 4, out=out)                        # g offset by one float: refused without a launch
    assert rc < 0 and float(out.item()) == SENT
    assert b"aligned" in _hip.lib().las_last_error()
    need = int(_hip.lib().las_sumsq_workspace_bytes(8))
    rc, _ = _sumsq(gd, 8, out=out, ws_bytes=need - 1)         # workspace too small
    assert rc < 0 and float(out.item()) == SENT
    rc, _ = _sumsq(gd, 8, out=out)
    assert rc == 0 and float(out.item()) == 8.0


def _adam(th, g, m, v, n, sumsq, clip, lr_t, status=None, guard=None, applied=None):
    from las import _hip
    rc = _hip.lib().las_clip_adam(_hip.p(th), _hip.p(g), _hip.p(m), _hip.p(v), n, _hip.p(sumsq), clip, lr_t, B1, B2, EPS,
                                  _hip.p(status), _hip.p(guard), _hip.p(applied), _hip.stream())
    torch.cuda.synchronize()
    return rc


def _run_adam(n, mode, steps=5, t0=0, words=True):
    """`steps` consecutive launches on the same buffers, fresh gradients every step; after EVERY launch the three buffers against
    adam_ref.step applied to what the device held before it, and against a float64 trajectory that never sees the device's state"""
    rng = np.random.RandomState(n % 997 + 17 * len(mode))
    theta0 = rng.randn(n).astype(np.float32)
    th, m, v = _buf(theta0, n), _buf(np.zeros(n), n), _buf(np.zeros(n), n)
    small = n <= 7                                            # a handful of elements: the last one is given a gradient of 0.25 .. 1.25
    norm0 = 0.25 if small else math.sqrt(R.sumsq_ref(make_g(np.random.RandomState(5), n)))
    clip = {"off": 0.0, "binding": R.f32(norm0 / 100.0), "loose": R.f32(norm0 * 1e3)}[mode]
    status = torch.zeros(2, dtype=torch.int32, device="cuda") if words else None
    guard = torch.zeros(1, device="cuda") if words else None
    applied = torch.zeros(1, dtype=torch.int32, device="cuda") if words else None
    pure = R.Trajectory(theta0, np.zeros(n), np.zeros(n))
    worst, worst_traj, bound = {}, {}, 0
    for s in range(steps):
        g = make_g(rng, n)
        if small:
            g[-1] = np.float32(0.25 * (s + 1) * (-1) ** s)    # the last (tail) element always moves
        gd = _buf(g, n)
        sumsq, ss = None, None
        if clip > 0:
            rc, sumsq = _sumsq(gd, n)
            assert rc == 0
            ss = float(sumsq.item())
            bound += int(math.sqrt(ss) > clip)
        lr_t = R.lr_t(LR, t0 + s + 1)
        before = [x[:n].cpu().numpy() for x in (th, m, v)]
        if s == 2:                                            # two runs from the same state: the same bits
            th2, m2, v2 = th.clone(), m.clone(), v.clone()
            assert _adam(th2, gd, m2, v2, n, sumsq, clip, lr_t) == 0
        assert _adam(th, gd, m, v, n, sumsq, clip, lr_t, status, guard, applied) == 0
        if s == 2:
            assert torch.equal(th, th2) and torch.equal(m, m2) and torch.equal(v, v2)
        got = [x[:n].cpu().numpy() for x in (th, m, v)]
        ref = R.step(before[0], g, before[1], before[2], ss, clip, lr_t, B1, B2, EPS)
        for k, x in R.ratios(got[0], got[1], got[2], ref).items():
            worst[k] = max(worst.get(k, 0.0), x)
        pure.step(g, ss, clip, lr_t, B1, B2, EPS)
        for k, x in pure.ratios(*got).items():
            worst_traj[k] = max(worst_traj.get(k, 0.0), x)
        for x in (th, m, v, gd):                              # nothing written behind the n elements
            assert float(x[n:].min()) == SENT and float(x[n:].max()) == SENT
        if words:
            assert int(applied.item()) == s + 1 and int(status[0].item()) == 0
        assert np.all(np.isfinite(got[0]))
    print("clip_adam n=%d %s t0=%d: worst ratio to the bounds %s, of the trajectory %s" % (n, mode, t0, worst, worst_traj))
    assert max(worst.values()) <= 1.0, worst
    assert max(worst_traj.values()) <= 1.0, worst_traj        # the moments persist between launches
    zero = np.arange(n) % 7 == 0                              # g = 0 from the start: theta, m, v stay exactly
    if small:
        zero[-1] = False
    assert np.array_equal(got[0][zero], theta0[zero]) and not got[1][zero].any() and not got[2][zero].any()
    if not small:
        assert np.all(got[2][~zero] > 0) and np.mean(got[0][~zero] != theta0[~zero]) > 0.9
    if mode == "binding":
        assert bound == steps
    if mode == "loose":
        assert bound == 0


@pytest.mark.parametrize("mode", ["off", "binding", "loose"])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 7, 1000, 1001, 1002, 1003, WRAP])
def test_clip_adam_five_launches_match_float64(n, mode):
    _run_adam(n, mode, words=(n % 2 == 0))                   # odd n: applied = status = guard = NULL, the kernel still runs


def test_clip_adam_late_steps():
    _run_adam(1001, "binding", steps=3, t0=60000)


def test_clip_adam_refuses_bad_arguments():
    n = 8
    th, g, m, v = _buf(np.ones(n), n), _buf(np.ones(n), n), _buf(np.zeros(n), n), _buf(np.zeros(n), n)
    keep = [x.clone() for x in (th, m, v)]
    assert _adam(th, g, m, v, n, None, 1.0, 1e-3) < 0                      # clipping without the sum of squares
    for bad in range(4):
        a = [th, g, m, v]
        a[bad] = a[bad][1:]
        assert _adam(a[0], a[1], a[2], a[3], 4, None, 0.0, 1e-3) < 0      # a buffer offset by one float
    assert all(torch.equal(x, y) for x, y in zip((th, m, v), keep))
    assert _adam(th, g, m, v, n, None, 0.0, 1e-3) == 0 and not torch.equal(th, keep[0])


# ---- the optimiser inside LAS.train ----------------------------------------------------------------------------------------------------
GRAD_TOL = 2e-3          # tests/test_gpu_las_parity.py TOL[("f32", "lstm")]["grad"]
# grad_clip values: the float64 global norm of the oracle's gradients for this model and these batches is 0.49 .. 0.55 over the four
# steps (CPU oracle, f32 mode), so 5.0 never binds and 0.05 always does, by a factor of ten (asserted below on the device's own gradients)
CLIP_LOOSE, CLIP_BINDING = 5.0, 0.05


def _named_mask(st):
    mask = np.zeros(st.flat.numel(), bool)
    for n in st.order:
        mask[st.offsets[n]:st.offsets[n] + st.vars[n].numel()] = True
    return mask


def _check_store_step(st, before, clip, lr_t, sumsq_dev, tag):
    """the three assertions on a store after an optimiser step: padding, sum of squares, update.  -> float64 gradient norm"""
    named = _named_mask(st)
    grad = st.flat_grad.cpu().numpy()
    after = [x.cpu().numpy() for x in (st.flat, st.adam_m, st.adam_v)]
    assert (~named).sum() > 0, "the layout has no padding slot: pick variable sizes that are not multiples of 4"
    for name, a in (("flat_grad", grad), ("flat", after[0]), ("adam_m", after[1]), ("adam_v", after[2])):
        assert not a[~named].any(), (tag, name, "padding slot written")
    ref_ss = sum(R.sumsq_ref(grad[st.offsets[n]:st.offsets[n] + st.vars[n].numel()]) for n in st.order)
    if sumsq_dev is not None:
        print("%s: sumsq relative error %.3g, bound %.3g" % (tag, abs(sumsq_dev - ref_ss) / ref_ss, R.sumsq_bound(grad.size)))
        assert abs(sumsq_dev - ref_ss) <= R.sumsq_bound(grad.size) * ref_ss, tag
    ref = R.step(before[0], grad, before[1], before[2], sumsq_dev, clip, lr_t, B1, B2, EPS)
    r = R.ratios(after[0], after[1], after[2], ref)
    print("%s: norm %.4g clip %g gs %.4g, worst ratio to the bounds %s" % (tag, math.sqrt(ref_ss), clip, ref[3]["gs"], r))
    assert max(r.values()) <= 1.0, (tag, r)
    assert np.abs(after[1]).max() > 0 and after[2].max() > 0
    return math.sqrt(ref_ss)


def _train_steps(prec, grad_clip, steps=4, global_step=0, B=5, T=37, U_max=9):
    from las import layers as L, variables as V
    from las.las import LAS, Listener, Speller
    from oracle import las_oracle as O
    cell = "lstm"
    args = make_args(enc_units=64, num_enc_layers=2, dec_units=64, num_dec_layers=1, embedding_size=32, attention_size=32, mode="add",
                     loc_kernel_size=11, loc_num_channels=3, lr=1e-3, grad_clip=grad_clip)
    p0 = O.init_params(args, seed=11, cell=cell)
    L.set_cell(cell)
    L.set_precision(prec)
    try:
        st = V.reset_default_store(device="cuda")
        st.load(p0)
        st.global_step = global_step
        las = LAS(args, Listener, Speller, {})
        las.build_variables()
        st.flatten()
        norms, compared = [], 0
        for k in range(steps):
            xs, ys = synthetic_batch(B, T, U_max, args.vocab_size, seed=100 + k)
            coins = np.ones(int(ys[1].max()), bool)
            gs = st.global_step
            before = [x.clone().cpu().numpy() for x in (st.flat, st.adam_m, st.adam_v)]
            applied0 = int(st.applied.item()) if st.applied is not None else 0
            lost0 = las.recovered_steps
            las.train(xs, ys, coins=coins)
            torch.cuda.synchronize()
            las.check_status()
            assert st.global_step == gs + 1
            if las.recovered_steps != lost0:
                # the step lost its co-residency and was re-run (helpers.train_step_pair): the launch counters moved twice
                print("step %d was lost and re-run: not compared" % gs)
                continue
            assert int(st.applied.item()) == applied0 + 1
            lr_t = R.lr_t(O.scheduled_learning_rate(args.lr, gs), gs + 1)
            tag = "%s clip %g step %d" % (prec, grad_clip, gs)
            norms.append(_check_store_step(st, before, grad_clip, lr_t, float(las.last_grad_sumsq.item()), tag))
            compared += 1
            if prec == "f32" and k >= 1:
                # the forward and backward of step k ran on the weights step k - 1 wrote: the oracle's gradients at the device's
                # pre-step parameters
                pk = {n: before[0][st.offsets[n]:st.offsets[n] + st.vars[n].numel()].reshape(tuple(st.vars[n].shape)) for n in st.order}
                po = O.to_torch(pk, requires_grad=True)
                z = {n: torch.zeros_like(v) for n, v in po.items()}
                g_o = O.train_step(po, z, {n: torch.zeros_like(v) for n, v in po.items()}, gs, (torch.tensor(xs[0]), xs[1]),
                                   (torch.tensor(ys[0]), ys[1]), args, cell, coins=coins)[3]
                for n in st.order:
                    go, g = g_o[n], st.vars[n].grad.detach().cpu()
                    err = (g - go).abs().max().item() / max(go.abs().max().item(), 1e-3)
                    assert err < GRAD_TOL, (tag, n, err)
        assert compared >= steps - 1
        return norms
    finally:
        L.set_cell("rnn")
        L.set_precision("f32")


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_train_steps_apply_the_reference_update_clip_binding(prec):
    norms = _train_steps(prec, CLIP_BINDING)
    assert all(n > CLIP_BINDING for n in norms), norms


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_train_steps_apply_the_reference_update_clip_loose(prec):
    norms = _train_steps(prec, CLIP_LOOSE)
    assert any(n < CLIP_LOOSE for n in norms), norms


def test_train_steps_late_in_the_schedule():
    """global_step = 120000: the decayed learning rate (0.5 ** 0.7 of lr) and the bias correction of t = 120001 reach the kernel"""
    from oracle import las_oracle as O
    assert abs(O.scheduled_learning_rate(1e-3, 120000) / 1e-3 - 0.5 ** 0.7) < 1e-12
    _train_steps("f32", CLIP_LOOSE, steps=2, global_step=120000)


@pytest.mark.parametrize("clip", [5.0, 0.02])
def test_lm_train_steps_apply_the_reference_update(clip):
    """the char RNNLM (lang/char_rnn_model.py), the second caller of K9: its store has the same flat buckets; the sum of squares its
    step read is not kept, so it is taken again from the gradients the step left (las_sumsq is bit-reproducible, asserted above)"""
    from las import layers as L, variables as V
    from lang.char_rnn_model import CharRNN
    Vn, H, NL, B, U = 27, 24, 2, 5, 7          # (27: the output bias and the embedding do not fill their last 16 bytes)
    L.set_precision("f32")
    st = V.VariableStore(device="cuda", seed=3)
    lm = CharRNN(True, B, U, Vn, H, max_grad_norm=clip, embedding_size=13, num_layers=NL, learning_rate=2e-3, store=st)
    lm.params()
    st.flatten()
    rng = np.random.RandomState(0)
    state, norms = None, []
    for it in range(3):
        x, y = rng.randint(0, Vn, size=(B, U)), rng.randint(0, Vn, size=(B, U))
        before = [a.clone().cpu().numpy() for a in (st.flat, st.adam_m, st.adam_v)]
        t = lm.global_step + 1
        _, state = lm.train_step(x, y, state)
        torch.cuda.synchronize()
        assert lm.global_step == t
        rc, ss = _sumsq(st.flat_grad, st.flat.numel())
        assert rc == 0
        norms.append(_check_store_step(st, before, clip, R.lr_t(2e-3, t), float(ss.item()), "lm clip %g step %d" % (clip, t)))
    assert all(n > clip for n in norms) if clip < 1 else all(n < clip for n in norms), norms
