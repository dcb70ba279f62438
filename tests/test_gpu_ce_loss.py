"""las_ce_loss (csrc/loss_opt.hip) through the C ABI against the float64 reference of tests/loss_ref.py: the dispatch borders between
the streaming kernel and ce_rows_reg_kernel<40 | 80 | 128>, the row counts around sum2_kernel's stride, every flag combination of
`smooth`, value-only calls, padded strided views, labels outside [0, V), peaky rows, bit reproducibility and the refusals.

Every output buffer carries canaries: in front of and behind the gradient view and in every gap of it, behind sums[3], behind the
workspace's bytes.  The bounds are loss_ref's (its docstring): the standing 2e-6 / 2e-7 where a case has the standing form, otherwise
loss_ref.CE_BOUNDS, derived on the CPU from the fp32 emulation.  Every case prints a CE-ERROR line (error and bound)."""
import numpy as np
import pytest
import torch

import loss_ref as R

pytestmark = pytest.mark.gpu

CANARY, GUARD = -77.0, 64
EPS = 0.01


class _Call(object):
    """one las_ce_loss call on guarded buffers.  logits [B, U, V] fp32 and y [B, U] on the host; sb / st: the element strides of the
    (b, t) rows in the logits AND the gradient buffer (default: the time-major [U, B, V] buffer seen through its [B, U, V] view)."""

    def __init__(self, logits, y, V, sb=None, st=None, ldy=None):
        B, U = y.shape
        self.B, self.U, self.V = B, U, V
        self.sb, self.st = (V, B * V) if sb is None else (sb, st)
        self.ldy = U if ldy is None else ldy
        self.idx = (np.arange(B)[:, None, None] * self.sb + np.arange(U)[None, :, None] * self.st + np.arange(V)[None, None, :])
        assert len(np.unique(self.idx)) == self.idx.size                       # no two elements share an address
        self.span = int(self.idx.max()) + 1
        host = np.full(self.span + GUARD, CANARY, np.float32)
        host[self.idx] = logits
        self.logits = torch.from_numpy(host).cuda()
        yh = np.full((B, self.ldy), 1, np.int32)                              # (the spare columns hold a valid label: reading one would count)
        yh[:, :U] = y
        self.y = torch.from_numpy(yh).cuda()
        self.gap = np.ones(GUARD + self.span + GUARD, bool)
        self.gap[GUARD + self.idx] = False

    def run(self, smooth, scale, grad=True, sums0=None, ws_short=0, ldy=None, scale_ptr=True, into=None):
        """-> (rc, sums [3] float32, gradient [B, U, V] or None).  sums0: what sums holds before the call (default NaN)."""
        from las import _hip
        lib = _hip.lib()
        B, U, V = self.B, self.U, self.V
        if into is None:
            self.sums = torch.full((3 + GUARD,), CANARY, device="cuda")
            self.sums[:3] = torch.tensor([float("nan")] * 3 if sums0 is None else sums0)
            self.g = torch.full((GUARD + self.span + GUARD,), CANARY, device="cuda") if grad else None
        need = int(lib.las_ce_loss_workspace_bytes(B, U))
        self.ws = torch.full((need + GUARD,), 255, dtype=torch.uint8, device="cuda")
        sc = torch.tensor([scale], dtype=torch.float32, device="cuda") if scale_ptr else None
        rc = lib.las_ce_loss(_hip.p(self.logits), self.sb, self.st, _hip.p(self.y), self.ldy if ldy is None else ldy, B, U, V, EPS, smooth,
                             _hip.p(self.sums), _hip.p(sc), _hip.p(self.g[GUARD:]) if grad else None, _hip.p(self.ws), need - ws_short,
                             _hip.stream())
        torch.cuda.synchronize()
        assert bool((self.sums[3:] == CANARY).all()) and bool((self.ws[need:] == 255).all())
        g = None
        if grad:
            gh = self.g.cpu().numpy()
            assert (gh[self.gap] == CANARY).all()                              # in front, behind, and every gap of the view
            g = gh[GUARD + self.idx]
        return rc, self.sums[:3].cpu().numpy(), g

    def untouched(self):
        """after a refused call: sums, the gradient buffer and every workspace byte as they were filled"""
        return (bool(torch.isnan(self.sums[:3]).all()) and bool((self.sums[3:] == CANARY).all()) and bool((self.ws == 255).all())
                and (self.g is None or bool((self.g == CANARY).all())))


def _draw(B, U, V, seed, mult=2.0, pad=True):
    rng = np.random.RandomState(seed)
    logits = (rng.randn(B, U, V) * mult).astype(np.float32)
    y = rng.randint(1, V, size=(B, U)).astype(np.int32) if V > 1 else np.zeros((B, U), np.int32)
    y.reshape(-1)[1 % (B * U)] = V - 1                                         # a label on the last class
    if pad and B * U > 2:
        y.reshape(-1)[B * U - 2] = 0                                           # one PAD row
    return logits, y


def _tokens(y, smooth):
    return y.size if smooth & 2 else int((y != 0).sum())


def _judge(name, sums, grad, ref, bound, keys=(0, 2)):
    """error against the float64 reference, printed, then held to `bound` = (loss rel, grad abs)"""
    _, _, rs, rg = ref
    loss = max(abs(float(sums[k]) - rs[k]) / max(1.0, abs(rs[k])) for k in keys)
    gerr = float(np.abs(grad.astype(np.float64) - rg).max()) if grad is not None else 0.0
    print("CE-ERROR %s loss %.3e (bound %.3e) grad %.3e (bound %.3e)" % (name, loss, bound[0], gerr, bound[1]))
    assert not np.isnan(sums[list(keys)]).any() and (grad is None or not np.isnan(grad).any())
    assert loss <= bound[0] and gerr <= bound[1], (name, loss, gerr, bound)
    return loss, gerr


STANDING = (R.CE_LOSS_REL, R.CE_GRAD_ABS)
BORDERS = [1, 2, 63, 64, 65, 1024, 1025, 2560, 2561, 5120, 5121, 8192, 8193]


@pytest.mark.parametrize("V", BORDERS)
def test_dispatch_borders(V):
    """B U = 6 through the time-major buffer, a label on the last class, one PAD row, sums written (bit 2).  V <= 2 also with bit 1
    (every position counts): at V = 1 the only class is PAD and nothing else would count."""
    B, U = 2, 3
    if V == 8193:                                                             # not the standing form: loss_ref's generator and its derived bound
        c = R.ce_case("v8193", 100)
        logits, y, scale, bound = c["logits"].reshape(B, U, V), c["y"].reshape(B, U), c["scale"], R.CE_BOUNDS["v8193"]
    else:
        logits, y = _draw(B, U, V, seed=V)
        scale, bound = None, STANDING
    call = _Call(logits, y, V)
    for smooth in ([5, 7] if V <= 2 else [5]):
        n = _tokens(y, smooth)
        s = scale if scale is not None else 1.0 / max(n, 1)
        rc, sums, grad = call.run(smooth, s)
        assert rc == 0 and sums[1] == n
        _judge("border-V%d-smooth%d" % (V, smooth), sums, grad, R.ce_ref(logits, y, V, EPS, smooth, s), bound)


@pytest.mark.parametrize("BU", [(1, 1), (1, 2), (3, 1), (1, 5), (41, 25)])
def test_row_count_edges(BU):
    """B U = 1, 2, 3, 5 (a partly filled block of four rows) and 1025 (sum2_kernel's 1024 threads take a second trip) at V = 30,
    scale 1: loss_ref.CE_BOUNDS['rowsN-v30']"""
    B, U = BU
    kind = "rows%d-v30" % (B * U)
    c = R.ce_case(kind, 100)
    logits, y = c["logits"].reshape(B, U, 30), c["y"].reshape(B, U)
    rc, sums, grad = _Call(logits, y, 30).run(5, c["scale"])
    assert rc == 0 and sums[1] == _tokens(y, 1)
    _judge(kind, sums, grad, R.ce_ref(logits, y, 30, EPS, 1, c["scale"]), R.CE_BOUNDS[kind])


@pytest.mark.parametrize("V", [30, 1500])
@pytest.mark.parametrize("smooth", [0, 1, 2, 3])
def test_flags_accumulate_without_bit_2_and_assign_with_it(V, smooth):
    B, U = 2, 3
    logits, y = _draw(B, U, V, seed=40 + smooth)
    n = _tokens(y, smooth)
    scale = 1.0 / n
    ref = R.ce_ref(logits, y, V, EPS, smooth, scale)
    call = _Call(logits, y, V)
    # with bit 2: all three assigned over NaN, sums[1] the token count
    rc, sums, grad = call.run(smooth | 4, scale)
    assert rc == 0 and sums[1] == n
    _judge("flags-V%d-smooth%d-set" % (V, smooth), sums, grad, ref, STANDING)
    total = sums[0]
    # without bit 2: sums[0..1] += (one fp32 addition of the same total), sums[2] untouched; a second call on the same buffer adds again
    rc, acc, grad2 = call.run(smooth, scale, sums0=[5.0, -3.0, CANARY])
    assert rc == 0 and acc[2] == CANARY and acc[1] == n - 3.0 and (grad2 == grad).all()
    assert acc[0] == np.float32(5.0) + total
    rc, acc2, grad3 = call.run(smooth, scale, into=True)
    assert rc == 0 and acc2[2] == CANARY and acc2[1] == 2 * n - 3.0 and (grad3 == grad).all()
    assert acc2[0] == acc[0] + total
    assert abs(float(acc2[0]) - (5.0 + 2.0 * ref[2][0])) <= R.CE_LOSS_REL * max(1.0, abs(5.0 + 2.0 * ref[2][0]))


@pytest.mark.parametrize("V", [30, 1025, 5000, 9000])
def test_value_only_call_gives_the_same_sum_bits(V):
    logits, y = _draw(2, 3, V, seed=V + 1)
    call = _Call(logits, y, V)
    rc, sums, _ = call.run(5, 0.2)
    rc2, sums_v, none = call.run(5, 0.2, grad=False)
    assert rc == 0 and rc2 == 0 and none is None and (sums_v == sums).all()
    rc3, sums_a, _ = call.run(1, 0.2, grad=False, sums0=[0.0, 0.0, CANARY], scale_ptr=False)      # accumulate mode needs no scale at all
    assert rc3 == 0 and sums_a[0] == sums[0] and sums_a[1] == sums[1] and sums_a[2] == CANARY


@pytest.mark.parametrize("V", [30, 1500])
def test_padded_strided_view(V):
    """st = V + 3, sb = U st + 5 (the MWER step's padded rows), ldy = U + 2: every gap of the gradient view keeps its canary (checked in
    _Call.run) and the result has the bits of the dense call"""
    B, U = 3, 4
    logits, y = _draw(B, U, V, seed=V + 2)
    n = _tokens(y, 1)
    st = V + 3
    rc, sums, grad = _Call(logits, y, V, sb=U * st + 5, st=st, ldy=U + 2).run(5, 1.0 / n)
    assert rc == 0 and sums[1] == n
    _judge("strided-V%d" % V, sums, grad, R.ce_ref(logits, y, V, EPS, 1, 1.0 / n), STANDING)
    rc, sums_d, grad_d = _Call(logits, y, V).run(5, 1.0 / n)
    assert rc == 0 and (sums_d == sums).all() and (grad_d == grad).all()


@pytest.mark.parametrize("V", [30, 1500])
def test_labels_out_of_range(V):
    """labels V, V + 7 and -1: no one-hot term, ly = 0, the position counts (it is not PAD); the rows beside them keep the bits of a
    run in which those labels are valid"""
    B, U = 2, 4
    logits, y = _draw(B, U, V, seed=V + 3)
    bad = y.copy()
    where = [(0, 2), (1, 0), (1, 3)]
    for (b, t), v in zip(where, (V, V + 7, -1)):
        bad[b, t] = v
        y[b, t] = 3
    n = _tokens(bad, 1)
    assert n == _tokens(y, 1)
    rc, sums, grad = _Call(logits, bad, V).run(5, 1.0 / n)
    assert rc == 0 and sums[1] == n
    _judge("bad-labels-V%d" % V, sums, grad, R.ce_ref(logits, bad, V, EPS, 1, 1.0 / n), STANDING)
    rc, _, grad_ok = _Call(logits, y, V).run(5, 1.0 / n)
    keep = np.ones((B, U), bool)
    for b, t in where:
        keep[b, t] = False
    assert rc == 0 and (grad[keep] == grad_ok[keep]).all() and not (grad[~keep] == grad_ok[~keep]).all()


@pytest.mark.parametrize("kind", ["scale1-v30", "peaky-v30", "peaky-v5000", "pm80-v30"])
def test_scale_one_and_peaky_rows(kind):
    """scale 1; logits x 20 at V = 30 and V = 5000; a row with one logit at +80 and the rest at -80"""
    c = R.ce_case(kind, 100)
    B, U, V = 2, 3, c["V"]
    logits, y = c["logits"].reshape(B, U, V), c["y"].reshape(B, U)
    rc, sums, grad = _Call(logits, y, V).run(5, c["scale"])
    assert rc == 0
    _judge(kind, sums, grad, R.ce_ref(logits, y, V, EPS, 1, c["scale"]), R.CE_BOUNDS[kind])


def test_two_runs_give_the_same_bits():
    V = 5121
    logits, y = _draw(2, 3, V, seed=9)
    call = _Call(logits, y, V)
    a, b = call.run(5, 0.2), call.run(5, 0.2)
    assert a[0] == 0 and b[0] == 0 and (a[1] == b[1]).all() and (a[2] == b[2]).all()


def test_refusals_before_any_launch():
    """each returns -1 with a las_last_error text and leaves sums, the gradient buffer and the workspace as they were"""
    from las import _hip
    V = 30
    logits, y = _draw(2, 3, V, seed=11)
    call = _Call(logits, y, V)

    def refused(rc, text):
        msg = _hip.lib().las_last_error() or b""
        assert rc == -1 and text in msg, (rc, msg)
        assert call.untouched()

    refused(call.run(5, 0.2, ldy=2)[0], b"bad arguments")                      # ldy < U
    refused(call.run(5, 0.2, ws_short=1)[0], b"workspace")
    refused(call.run(1, 0.2, scale_ptr=False)[0], b"dlogits needs scale_ptr")
    refused(call.run(5, 0.2, grad=False, scale_ptr=False)[0], b"bit 2")        # (the row kernel used to run before this was seen)
    assert call.run(5, 0.2)[0] == 0 and not call.untouched()
