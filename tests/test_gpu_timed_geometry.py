"""Parity and determinism AT THE GEOMETRY bench.py TIMES (VERDICT r2 "next round" item 1): B = 48 utterances of T = 1274
frames on the bench architecture, speed mode.  At this size the oracle needs minutes per step, so the checks are the
size-independent properties the path offers:

  * row independence: the reference model has no cross-utterance arithmetic in its forward pass (las/las.py:93-117 run every
    utterance through the same weights; the only batch-wide quantity is the loss normaliser, las/las.py:329-331), so the rows
    of the B = 48 step must equal the same utterances run as twelve B = 4 steps -- which ARE oracle-checked
    (test_gpu_full_scale.py) -- and the B = 48 gradient must equal the token-weighted sum of the twelve;
  * bitwise run-to-run determinism of three optimiser steps (SURVEY section 5 "race detection": the step depends on five
    cross-stream hand-overs guarded by spin-waits; DESIGN section 4 claims "no atomics, bit-reproducible");
  * the same three steps with every cross-stream hand-over switched off (whole x-projections, whole GEMMs between the BPTT
    sweeps, no held side stream, one-stream tail) within the split-K tolerance.
"""
import numpy as np
import pytest
import torch

from helpers import expect_handovers, make_args, synthetic_batch

pytestmark = pytest.mark.gpu

B, T = 48, 1274


def bench_arch(**over):
    kw = dict(enc_units=256, num_enc_layers=3, dec_units=512, num_dec_layers=1, embedding_size=128, attention_size=128,
              mode="add", lr=1e-3, grad_clip=5.0, label_smoothing=True, vocab_size=30)
    kw.update(over)
    return make_args(**kw)


def _fresh(args, p0):
    from las import layers as L, variables as V
    from las.las import LAS, Listener, Speller
    L.set_cell("lstm")
    L.set_precision("bf16")
    st = V.reset_default_store(device="cuda")
    st.load(p0)
    return LAS(args, Listener, Speller, {}), st


def _sub(xs, ys, lo, hi):
    return (xs[0][lo:hi], xs[1][lo:hi]), (ys[0][lo:hi], ys[1][lo:hi])


def test_b48_rows_equal_twelve_b4_batches():
    from oracle import las_oracle as O
    args = bench_arch()
    xs, ys = synthetic_batch(B, T, 256, 30, seed=7, min_frac=0.834)
    p0 = O.init_params(args, seed=3, cell="lstm")
    las, st = _fresh(args, p0)
    _, _, _, logits, alphas, _, _ = las.train(xs, ys)
    torch.cuda.synchronize()
    las.check_status()
    v = expect_handovers(las, "lstm", B)
    assert v["dense_chunks"] == 3, v                  # every dense + tanh between two sweeps follows the next layer's time chunks
    assert (v["sweeps_fwd"], v["xproj_chunks"], v["sweeps_bwd"], v["dout_chunks"]) == (4, 4, 4, 3), v    # = profiles/*_kernel_stats.csv: 3 of 4 BPTT launches CH = true
    logits, alphas, g48 = logits.cpu(), alphas.cpu(), st.flat_grad.cpu().clone()
    assert alphas.shape[-1] == 160
    n_tot = int((ys[0][:, :int(ys[1].max())] != 0).sum())
    gsum = torch.zeros_like(g48)
    worst_l = worst_a = 0.0
    for k in range(B // 4):
        xk, yk = _sub(xs, ys, 4 * k, 4 * k + 4)
        las_k, st_k = _fresh(args, p0)
        _, _, _, lk, ak, _, _ = las_k.train(xk, yk)
        torch.cuda.synchronize()
        las_k.check_status()
        expect_handovers(las_k, "lstm", 4)            # the oracle-checked B = 4 steps run the same schedule
        Uk = int(yk[1].max())
        n_k = int((yk[0][:, :Uk] != 0).sum())
        gsum += st_k.flat_grad.cpu() * (n_k / n_tot)
        # every decode step an utterance owns (t < its token count) must not depend on who else is in the batch
        for i in range(4):
            n_i = int(yk[1][i])
            worst_l = max(worst_l, (lk[i, :n_i].cpu() - logits[4 * k + i, :n_i]).abs().max().item())
            worst_a = max(worst_a, (ak[i, :n_i].cpu() - alphas[4 * k + i, :n_i]).abs().max().item())
    gerr = (g48 - gsum).abs().max().item() / g48.abs().max().item()
    print("B=48 vs 12 x B=4: logits %.2e alphas %.2e flat_grad %.2e (of max |g| %.3e)" % (worst_l, worst_a, gerr, g48.abs().max().item()))
    assert worst_l <= 1e-5 and worst_a <= 1e-5, (worst_l, worst_a)
    assert gerr <= 2e-3, gerr


def _three_steps(args, p0, xs, ys, handovers=True, prepared=True):
    from las import layers as L
    las, st = _fresh(args, p0)
    out = []
    for i in range(3):
        loss = las.train(xs, ys)[0]
        expect_handovers(las, "lstm", B, on=handovers)
        # round 5: from a model's second step on, every sweep (4 forward + 4 BPTT) finds its weight pack and a clean exchange state
        # prepared by ONE launch at the start of the step (las_rnn_seq_prepare) -- no pack launch on the chain
        assert las.last_variants["prepared_sweeps"] == (8 if (prepared and i > 0) else 0), (i, las.last_variants)
        if L.TAIL_WINDOW:
            # the bottom layer's weight gradients in windows of TAIL_WINDOW sweep steps, which FOLLOW the last BPTT sweep on the side stream when
            # it publishes its progress (with the hand-overs off: the same launches behind the sweep -- same arithmetic)
            nwin = -(-T // L.TAIL_WINDOW)
            assert las.last_variants["tail_windows"] == nwin and las.last_variants["tail_follow"] == (1 if handovers else 0), las.last_variants
        else:
            assert las.last_variants["tail_windows"] == 0
        if not out:
            torch.cuda.synchronize()
            g0 = st.flat_grad.clone()
        out.append(loss)
    torch.cuda.synchronize()
    las.check_status()
    return st.flat.clone(), g0, [float(v) for v in out]


def test_three_b48_steps_are_bit_reproducible_and_independent_of_the_hand_overs():
    from las import layers as L
    from oracle import las_oracle as O
    args = bench_arch(scheduled_sampling=True)       # what bench.py runs (rate 1.0 at step 0: teacher forcing, sampler path armed)
    xs, ys = synthetic_batch(B, T, 256, 30, seed=0, min_frac=0.834)
    p0 = O.init_params(args, seed=0, cell="lstm")
    f1, g1, l1 = _three_steps(args, p0, xs, ys)
    f2, g2, l2 = _three_steps(args, p0, xs, ys)
    assert l1 == l2, (l1, l2)
    assert torch.equal(g1, g2), "first-step gradient differs between two identical runs: max %.3e" % (g1 - g2).abs().max().item()
    assert torch.equal(f1, f2), "parameters after 3 steps differ between two identical runs: max %.3e" % (f1 - f2).abs().max().item()
    handovers_off = dict(XPROJ_CHUNK_STEPS=0, DOUT_CHUNK_ROWS=0, HOLD_SIDE=False, TAIL_TWO_STREAMS=False)
    with L.schedule(**handovers_off):
        f3, g3, l3 = _three_steps(args, p0, xs, ys, handovers=False)      # (asserts that nothing was handed over)
    # ... and with every sweep packing for itself (rounds 1-4's launches): the prepared workspaces must change nothing, bit for bit
    with L.schedule(PREPARED_SWEEPS=False):
        f4, g4, l4 = _three_steps(args, p0, xs, ys, prepared=False)
    assert l1 == l4 and torch.equal(g1, g4) and torch.equal(f1, f4), "prepared sweep workspaces changed the result"
    # round 5, off by default (no gain, las/layers.py TAIL_WINDOW): the end-of-step tail in windows that FOLLOW the last BPTT sweep
    # (las_rnn_seq_bwd's progress -> las_wait_words_min -> las_wgrad_ih_hh_window on the side stream).  The windows are the arithmetic,
    # following is the schedule: with the hand-overs off the same window launches run behind the sweep -- bitwise equal; against the
    # one-launch tail the split of the contraction differs (tolerance)
    with L.schedule(TAIL_WINDOW=160):
        f5, g5, l5 = _three_steps(args, p0, xs, ys)
        with L.schedule(**handovers_off):
            f6, g6, l6 = _three_steps(args, p0, xs, ys, handovers=False)
    assert l5 == l6 and torch.equal(g5, g6), "tail windows: following the sweep changed the result"
    assert (g5 - g1).abs().max().item() <= 2e-3 * g1.abs().max().item() and abs(l5[0] - l1[0]) <= 1e-5 * max(1.0, abs(l1[0]))
    gerr = (g1 - g3).abs().max().item() / g1.abs().max().item()
    print("hand-overs on vs off: first-step gradient %.2e of max |g| (bitwise equal: %s), losses %s vs %s"
          % (gerr, torch.equal(g1, g3), l1, l3))
    assert gerr <= 2e-3, gerr
    assert abs(l1[0] - l3[0]) <= 1e-5 * max(1.0, abs(l1[0]))
    # after three Adam steps (lr 1e-3, sign-like updates of near-zero gradients) parameters may differ by a few lr at most
    assert (f1 - f3).abs().max().item() <= 6.5e-3
    assert all(abs(a - b) <= 2e-3 * max(1.0, abs(a)) for a, b in zip(l1, l3)), (l1, l3)


def test_train_eval_train_uses_the_updated_recurrent_weights():
    """a store's FIRST train step builds its shadows one by one and leaves the begin_step event unconsumed; an
    inference right after it (outside any train step) triggers las_rnn_seq_prepare on the side stream -- which must be ordered behind
    las_clip_adam, not behind that stale event, or the next step's eight sweeps run on W_hh packs made from the weights of BEFORE the
    update.  The sequence train -> inference -> train -> train must equal, bit for bit, the same sequence with every sweep packing
    for itself (PREPARED_SWEEPS off), at a small geometry (the hazard is in the host logic, not in the size)."""
    from las import layers as L
    from oracle import las_oracle as O
    args = bench_arch()
    xs, ys = synthetic_batch(8, 320, 40, 30, seed=5, min_frac=0.9)
    p0 = O.init_params(args, seed=4, cell="lstm")

    def run(prepared):
        with L.schedule(PREPARED_SWEEPS=prepared):
            las, st = _fresh(args, p0)
            losses, used = [], []
            losses.append(float(las.train(xs, ys)[0]))
            used.append(dict(las.last_variants))
            _, y_hat = las.inference(xs)                   # no begin_step: the prepare it triggers must wait for the optimiser
            losses.append(float(las.train(xs, ys)[0]))
            used.append(dict(las.last_variants))
            losses.append(float(las.train(xs, ys)[0]))
            used.append(dict(las.last_variants))
            torch.cuda.synchronize()
            las.check_status()
            return losses, st.flat.clone(), y_hat.cpu(), used

    l_ref, f_ref, y_ref, _ = run(False)
    l_new, f_new, y_new, used = run(True)
    assert used[2]["prepared_sweeps"] > 0, used          # the prepared path really ran in the steps after the inference
    assert torch.equal(y_ref, y_new)
    assert l_ref == l_new, (l_ref, l_new)
    assert torch.equal(f_ref, f_new), "parameters differ: max %.3e" % (f_ref - f_new).abs().max().item()


@pytest.mark.parametrize("rows", [5, 8])
def test_two_steps_with_on_device_sampling_are_bit_reproducible_when_the_batch_does_not_fill_its_row_tile(rows):
    """Round 6 finding: with B = 5 or 8 rows of a 16-row tile (64-unit sweeps) and on-device scheduled sampling the SECOND step of a run
    differed by ~2e-6 between identical runs in the two bottom layers' gradients.  Cause: the forward sweep's helper waves stored the results of
    the rows past the end of the batch to the last valid row's addresses, and a few dozen of those copies differed from the real row by one
    bf16 ulp in the saved gates -- the store that landed last decided what BPTT read.  Those rows no longer store (csrc/rnn_seq.hip)."""
    from las import layers as L, variables as V
    from las.las import LAS, Listener, Speller
    from oracle import las_oracle as O
    args = make_args(enc_units=64, num_enc_layers=2, dec_units=128, num_dec_layers=1, embedding_size=64, attention_size=64, mode="add", lr=1e-3,
                     grad_clip=5.0, label_smoothing=True, vocab_size=30, scheduled_sampling=True, warmup_step=0, max_step=8)
    xs, ys = synthetic_batch(rows, 96, 24, 30, seed=43, min_frac=0.8)
    p0 = O.init_params(args, seed=2, cell="lstm")
    coins = np.random.RandomState(0).rand(int(ys[1].max())) < 0.5

    def two():
        L.set_cell("lstm"); L.set_precision("bf16")
        st = V.reset_default_store(device="cuda"); st.load(p0)
        las = LAS(args, Listener, Speller, {})
        for _ in range(2):
            st.global_step = 3
            las.train(xs, ys, coins=coins)
        torch.cuda.synchronize()
        las.check_status()
        return st.flat_grad.clone(), st.flat.clone()

    ref = two()
    for _ in range(5):
        cur = two()
        assert torch.equal(ref[0], cur[0]) and torch.equal(ref[1], cur[1]), "second-step gradient differs between identical runs: %.3e" % (ref[0] - cur[0]).abs().max().item()
