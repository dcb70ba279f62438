"""las_ctc_loss (csrc/ctc.hip) through the C ABI at its edges, against tests/loss_ref.py: label counts at the wave borders of the
S = 2L + 1 states, the maximum L = 511 (16 waves), a wide and nearly empty label block, U = 0, rows of one and of no frame, the
single-path alignment and its infeasible neighbour, chains of a hundred and more repeats, labels out of range, the dropped last
label, peaky logits; fp32 and bf16 gradients everywhere.

References: per-row float64 torch.nn.functional.ctc_loss (loss_ref.ctc_ref), and the closed forms where no dynamic programme is
needed.  Bounds: 1e-5 relative nll / 1e-5 absolute gradient for T' <= 319 (the standing ones of tests/test_gpu_ctc.py); for T' > 319
and the peaky case loss_ref.CTC_BOUNDS (derived on the CPU).  The nll, gradient and workspace buffers carry canaries behind them.
Every case prints a CTC-ERROR line."""
import numpy as np
import pytest
import torch

import loss_ref as R

pytestmark = pytest.mark.gpu

CANARY, GUARD = -77.0, 64
STANDING = (R.CTC_NLL_REL, R.CTC_GRAD_ABS)
SCALE = 0.5


def _ctc(logits, y, U, enc_len, drop=-1, dtype=torch.float32, scale=SCALE, ldy=None):
    """one las_ctc_loss call on guarded buffers -> (rc, loss, nll [B], gradient [B, T', Vc] as float32; None after a refusal)"""
    from las import _hip
    lib = _hip.lib()
    B, Tp, Vc = logits.shape
    ldy = y.shape[1] if ldy is None else ldy
    lg = torch.from_numpy(np.ascontiguousarray(logits, np.float32)).cuda()
    yy = torch.from_numpy(np.ascontiguousarray(y, np.int32)).cuda()
    el = torch.tensor(np.asarray(enc_len, np.int32), device="cuda")
    n = B * Tp * Vc
    nll = torch.full((B + GUARD,), CANARY, device="cuda")
    loss = torch.full((1 + GUARD,), CANARY, device="cuda")
    grad = torch.full((n + GUARD,), CANARY, device="cuda").to(dtype)
    need = int(lib.las_ctc_workspace_bytes(B, Tp, U))
    ws = torch.full((max(need, 1) + GUARD,), 255, dtype=torch.uint8, device="cuda")
    sc = torch.tensor([scale], dtype=torch.float32, device="cuda")
    rc = lib.las_ctc_loss(_hip.p(lg), Tp * Vc, Vc, Vc, _hip.p(yy), ldy, U, _hip.p(el), B, Tp, int(drop), _hip.p(nll), _hip.p(loss), _hip.p(sc),
                          _hip.p(grad), _hip._dt(grad), Tp * Vc, Vc, _hip.p(ws), need, _hip.stream())
    torch.cuda.synchronize()
    assert bool((nll[B:] == CANARY).all()) and bool((loss[1:] == CANARY).all()) and bool((grad[n:].float() == CANARY).all())
    assert bool((ws[need:] == 255).all())
    if rc != 0:
        assert bool((nll == CANARY).all()) and bool((loss == CANARY).all()) and bool((grad.float() == CANARY).all()) and bool((ws == 255).all())
        return rc, None, None, None
    return rc, float(loss[0]), nll[:B].cpu().numpy(), grad[:n].float().cpu().numpy().reshape(B, Tp, Vc)


def _labels(y, U, drop):
    labs = [[int(v) for v in row[:U] if v != 0] for row in y]
    if drop >= 0 and labs[drop]:
        labs[drop] = labs[drop][:-1]
    return labs


def _y(labs, U, ldy=None, fill=0):
    y = np.full((len(labs), U if ldy is None else ldy), fill, np.int32)
    for b, l in enumerate(labs):
        y[b, :U] = 0
        y[b, :len(l)] = l
    return y


def _check(name, logits, y, U, enc_len, drop=-1, bound=STANDING, inf_rows=(), refs=None):
    """run fp32 and bf16, compare every row.  inf_rows: rows that must come out nll = inf with a zero gradient row; refs: {row: (nll,
    gradient)} closed forms that replace the dynamic programme; every other row must be alignable in the reference."""
    B, Tp, Vc = logits.shape
    labs = _labels(y, U, drop)
    T = np.minimum(np.asarray(enc_len), Tp)
    rc, loss, nll, grad = _ctc(logits, y, U, enc_len, drop)
    assert rc == 0
    worst = [0.0, 0.0]
    want = []
    for b in range(B):
        if b in inf_rows:
            assert nll[b] == np.inf and (grad[b] == 0).all(), (name, b)
            want.append(None)
            continue
        if refs and b in refs:
            nll_r, grad_r = refs[b]
        elif T[b] == 0:
            assert not labs[b]
            nll_r, grad_r = 0.0, np.zeros((Tp, Vc))
        else:
            n_, g_ = R.ctc_ref(logits[b:b + 1], [labs[b]], [T[b]])
            nll_r, grad_r = n_[0], g_[0]
        assert np.isfinite(nll_r), (name, b, "the case must be alignable")
        want.append(grad_r)
        e = R.ctc_errors(float(nll[b]), grad[b, :T[b]], nll_r, SCALE * grad_r[:T[b]]) if T[b] else (abs(float(nll[b]) - nll_r), 0.0)
        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
        assert (grad[b, T[b]:] == 0).all(), (name, b)                          # exact zeros behind the row's frames
    print("CTC-ERROR %s nll %.3e (bound %.3e) grad %.3e (bound %.3e)" % (name, worst[0], bound[0], worst[1], bound[1]))
    assert worst[0] <= bound[0] and worst[1] <= bound[1], (name, worst, bound)
    if not inf_rows:
        assert abs(loss - SCALE * float(nll.astype(np.float64).sum())) <= 1e-6 * max(1.0, abs(loss))
    else:
        assert loss == np.inf
    # bf16 gradient: the same nll bits, every element within one bf16 ulp of the reference
    rc, _, nll16, g16 = _ctc(logits, y, U, enc_len, drop, dtype=torch.bfloat16)
    assert rc == 0 and (nll16 == nll).all()
    for b in range(B):
        if want[b] is None:
            assert (g16[b] == 0).all()
            continue
        r = SCALE * want[b][:T[b]]
        ulp = np.exp2(np.floor(np.log2(np.maximum(np.abs(r), 1e-30))) - 7)
        assert (np.abs(g16[b, :T[b]] - r) <= np.maximum(ulp, 1e-6)).all(), (name, b)
        assert (g16[b, T[b]:] == 0).all()
    return nll, grad


def _logits(B, Tp, Vc, seed, mult=2.0):
    return (np.random.RandomState(seed).randn(B, Tp, Vc) * mult).astype(np.float32)


@pytest.mark.parametrize("L", [31, 32, 33, 95, 96, 127, 128])
def test_label_counts_at_the_wave_borders_of_the_states(L):
    """S = 2L + 1 around 64, 192 and 256 (L = 32: one state in the second wave); T' = L + 40, three rows: L labels drawn freely, L - 1
    labels on fewer frames, L labels without neighbours alike on L + 5 frames"""
    Tp, Vc = L + 40, 31
    rng = np.random.RandomState(L)
    labs = [[int(v) for v in rng.randint(1, Vc - 1, size=L)], [int(v) for v in rng.randint(1, Vc - 1, size=L - 1)],
            R.no_adjacent_repeats(rng, L, 1, Vc - 1)]
    _check("wave-border-L%d" % L, _logits(3, Tp, Vc, L + 1), _y(labs, L, ldy=L + 2, fill=9), L, [Tp, Tp - 7, L + 5])     # (spare columns: labels that must not be read)


def test_maximum_label_count_sixteen_waves():
    """L = 511 on T' = 540 frames, no two neighbours alike: S = 1023 states, nt = 1024 threads; a second row with 300 labels"""
    logits, lab, Tp = R.ctc_case("max-L511-T540", 100)
    rng = np.random.RandomState(7)
    labs = [lab, R.no_adjacent_repeats(rng, 300, 1, 30)]
    lg = np.stack([logits, _logits(1, Tp, 31, 8)[0]])
    _check("max-L511-T540", lg, _y(labs, 511), 511, [Tp, Tp - 10], bound=R.CTC_BOUNDS["max-L511-T540"])


def test_wide_label_block_nearly_empty():
    """U = 511 columns, three labels in row 0 (spread over the columns: the compaction crosses waves), none in row 1"""
    logits, lab, Tp = R.ctc_case("wide-U511-T540", 100)
    y = np.zeros((2, 511), np.int32)
    y[0, [5, 200, 510]] = lab
    lg = np.stack([logits, _logits(1, Tp, 31, 9)[0]])
    _check("wide-U511-T540", lg, y, 511, [Tp, Tp], bound=R.CTC_BOUNDS["wide-U511-T540"])


def test_more_than_511_label_columns_is_refused_before_any_launch():
    from las import _hip
    rc = _ctc(_logits(1, 8, 31, 1), np.zeros((1, 512), np.int32), 512, [8])[0]           # (_ctc checks that nothing was written)
    assert rc == -1 and b"at most 511" in (_hip.lib().las_last_error() or b"")


def test_no_label_columns_at_all():
    """U = 0 with ldy = 2 (the two columns hold labels that must not be read): nll = -sum log p_blank, the gradient softmax - [blank]"""
    B, Tp, Vc = 3, 9, 31
    logits = _logits(B, Tp, Vc, 3)
    enc_len = [9, 4, 1]
    refs = {b: R.ctc_blank_only(logits[b], enc_len[b]) for b in range(B)}
    y = np.full((B, 2), 5, np.int32)
    nll, grad = _check("U0", logits, y, 0, enc_len, refs=refs)
    soft = np.exp(logits.astype(np.float64) - np.log(np.exp(logits.astype(np.float64)).sum(-1, keepdims=True)))
    for b in range(B):                                                         # off the blank: the plain softmax, nothing subtracted
        assert np.abs(grad[b, :enc_len[b], :Vc - 1] - SCALE * soft[b, :enc_len[b], :Vc - 1]).max() < 1e-6


def test_rows_of_one_frame_and_of_none():
    """enc_len = 1 with L = 1 and L = 0; enc_len = 0 with L = 0 (nll = 0, zero row) and with L = 2 (inf, zero row); enc_len > T' clamped"""
    B, Tp, Vc, U = 5, 6, 31, 3
    logits = _logits(B, Tp, Vc, 4)
    labs = [[7], [], [], [3, 9], [4, 4]]
    enc_len = [1, 1, 0, 0, Tp + 5]
    refs = {0: R.ctc_single_path(logits[0], 7, 1), 1: R.ctc_blank_only(logits[1], 1)}
    nll, grad = _check("short-rows", logits, _y(labs, U), U, enc_len, inf_rows=(3,), refs=refs)
    assert nll[2] == 0.0 and (grad[2] == 0).all()


def test_single_path_and_its_infeasible_neighbour():
    """six labels of one class on 11 frames: one alignment, the closed form; on 10 frames: inf and a zero row, the other rows' bits
    unchanged"""
    B, Tp, Vc, U = 3, 13, 31, 6
    logits = _logits(B, Tp, Vc, 5)
    labs = [[9] * 6, [2, 2, 5], [1, 8, 8, 8]]
    y = _y(labs, U)
    nll, grad = _check("single-path", logits, y, U, [11, 13, 12], refs={0: R.ctc_single_path(logits[0], 9, 6)})
    nll2, grad2 = _check("single-path-T10", logits, y, U, [10, 13, 12], inf_rows=(0,))
    for b in (1, 2):
        assert nll2[b] == nll[b] and (grad2[b] == grad[b]).all()


@pytest.mark.parametrize("kind", ["chain1-L200-T420", "chain2-L200-T420"])
def test_long_chains_of_one_class(kind):
    """the posterior sums walk a class's repeats through nxt_sh.  Vc = 3 leaves ONE usable class (0 is PAD, 2 the blank): 200 labels of
    class 1, one chain of 200.  Two classes need Vc = 4: 200 labels drawn from {1, 2}, two chains of about 100."""
    logits, lab, Tp = R.ctc_case(kind, 100)
    _check(kind, logits[None], _y([lab], 200), 200, [Tp], bound=R.CTC_BOUNDS[kind])


def test_labels_out_of_range():
    """the blank's id Vc - 1 and -4 as labels: inf and a zero row each; the rows beside them keep their bits"""
    B, Tp, Vc, U = 4, 12, 31, 4
    logits = _logits(B, Tp, Vc, 6)
    labs = [[3, 3, 7], [5, 6], [8], [1, 2, 2, 4]]
    good = _y(labs, U)
    bad = good.copy()
    bad[1, 1], bad[2, 0] = Vc - 1, -4
    enc_len = [12, 11, 10, 12]
    nll, grad = _check("bad-labels", logits, bad, U, enc_len, inf_rows=(1, 2))
    nll_ok, grad_ok = _check("bad-labels-valid", logits, good, U, enc_len)
    for b in (0, 3):
        assert nll[b] == nll_ok[b] and (grad[b] == grad_ok[b]).all()


@pytest.mark.parametrize("row", [1, 2])
def test_dropped_last_label_on_rows_with_one_label_and_with_none(row):
    """drop_last_row on a row whose only label goes (L becomes 0: the blank-only closed form) and on a row that has none"""
    B, Tp, Vc, U = 3, 10, 31, 3
    logits = _logits(B, Tp, Vc, 7)
    labs = [[4, 4, 6], [9], []]
    enc_len = [10, 8, 9]
    _check("drop-row%d" % row, logits, _y(labs, U), U, enc_len, drop=row, refs={row: R.ctc_blank_only(logits[row], enc_len[row])})


def test_peaky_logits():
    logits, lab, Tp = R.ctc_case("peaky-T160", 100)
    lg = np.stack([logits, _logits(1, Tp, 31, 10, mult=30.0)[0]])
    _check("peaky-T160", lg, _y([lab, lab[:17]], 40), 40, [Tp, 90], bound=R.CTC_BOUNDS["peaky-T160"])
