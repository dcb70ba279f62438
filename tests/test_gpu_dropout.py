"""Input dropout of a bidirectional layer in one launch (las_dropout_pair_fwd / _bwd; reference las/layers.py:37-47: fw_cell and bw_cell in
separate DropoutWrappers, input_keep_prob = 1 - dropout_rate, default --dropout_rate 0.5, las/arguments.py:76-78).  tf.nn.dropout's Philox
stream is not contractual (the reference fixes no seed): what is checked is the distribution, the scaling, the independence of the two
directions' masks, the zero padding, reproducibility under a seed, that backward applies EXACTLY the forward's masks, and a train step.

The masks themselves are a pure function of (seed, direction, quad) -- splitmix64, a 16-bit slice per element -- so every forward and
backward case is also compared element by element, bit for bit, with tests/loss_ref.py's dropout_masks; among them a block of more
quads than the capped grid has threads (the grid-stride loop), keep = 1 (identity), no rows, and an unaligned output pitch."""
import numpy as np
import pytest
import torch

import loss_ref as R
from helpers import make_args, synthetic_batch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype,out_bf16,K,ld", [(torch.float32, True, 39, 64), (torch.bfloat16, True, 512, 512), (torch.float32, False, 39, 40),
                                                 (torch.bfloat16, True, 100, 128), (torch.float32, False, 128, 128)])
@pytest.mark.parametrize("keep", [0.5, 0.9])
def test_dropout_pair_distribution_padding_and_backward(dtype, out_bf16, K, ld, keep):
    from las.layers import _DropoutPair
    g = torch.Generator().manual_seed(K + int(keep * 10))
    x = (torch.randn(7, 301, K, generator=g) + 3.0).to(dtype).cuda().requires_grad_(True)        # (no zeros in the input: a zero output IS a dropped element)
    yf, yb = _DropoutPair.apply(x, keep, 12345, out_bf16, ld)
    assert yf.shape == (7, 301, ld) and yf.dtype == (torch.bfloat16 if out_bf16 else torch.float32)
    if ld > K:
        assert float(yf[..., K:].abs().max()) == 0 and float(yb[..., K:].abs().max()) == 0
    mf, mb = (yf[..., :K] != 0), (yb[..., :K] != 0)
    n = mf.numel()
    for m in (mf, mb):
        frac = m.float().mean().item()
        assert abs(frac - keep) < 5 * np.sqrt(keep * (1 - keep) / n) + 2e-5, frac          # (+ the 16-bit threshold's resolution)
    both = (mf & mb).float().mean().item()
    assert abs(both - keep * keep) < 5 * np.sqrt(0.25 / n) + 1e-4, both                     # the two directions' masks are independent
    # kept elements are x / keep (in the output's precision)
    ref = (x.detach().float() / keep)
    ref = ref.to(torch.bfloat16).float() if out_bf16 else ref
    assert torch.equal(torch.where(mf, yf[..., :K].float(), ref), ref) and torch.equal(torch.where(mb, yb[..., :K].float(), ref), ref)
    # ... and exactly: the masks are loss_ref's, element by element; kept values are x * float32(1 / keep) rounded to the output's type
    mf_r, mb_r = (torch.from_numpy(m).view(7, 301, K) for m in R.dropout_masks(12345, 7 * 301, K, keep))
    assert torch.equal(mf.cpu(), mf_r) and torch.equal(mb.cpu(), mb_r)
    for yd, m in ((yf, mf_r), (yb, mb_r)):
        assert torch.equal(yd[..., :K].float().cpu(), _scaled(x.detach().float().cpu(), m, keep, yd.dtype))
    # same seed -> same masks; another seed -> other masks
    yf2, yb2 = _DropoutPair.apply(x, keep, 12345, out_bf16, ld)
    assert torch.equal(yf, yf2) and torch.equal(yb, yb2)
    yf3, _ = _DropoutPair.apply(x, keep, 12346, out_bf16, ld)
    assert not torch.equal(yf, yf3)
    # backward: dx = (m_fw g_fw + m_bw g_bw) / keep with the forward's masks
    gf = torch.randn(7, 301, ld, generator=g).to(yf.dtype).cuda()
    gb = torch.randn(7, 301, ld, generator=g).to(yf.dtype).cuda()
    (dx,) = torch.autograd.grad((yf, yb), x, (gf, gb))
    want = (mf.float() * gf[..., :K].float() + mb.float() * gb[..., :K].float()) / keep
    tol = 2e-2 if dtype == torch.bfloat16 else 1e-6
    assert dx.dtype == dtype and (dx.float() - want).abs().max().item() <= tol * max(1.0, want.abs().max().item())
    # ... and exactly, with loss_ref's masks: (m_fw g_fw + m_bw g_bw) * float32(1 / keep) in fp32, rounded to dx's type
    exact = _scaled(torch.where(mf_r, gf[..., :K].float().cpu(), torch.zeros(())) + torch.where(mb_r, gb[..., :K].float().cpu(), torch.zeros(())),
                    None, keep, dtype)
    assert torch.equal(dx.float().cpu(), exact)


def _scaled(v, mask, keep, dtype):
    """v * float32(1 / keep) in fp32 where mask (None: everywhere), zero elsewhere, rounded to dtype and back to fp32"""
    s = torch.from_numpy(np.asarray(np.float32(1.0) / np.float32(keep), np.float32))
    out = v.float() * s
    if mask is not None:
        out = torch.where(mask, out, torch.zeros(()))
    return out.to(dtype).float()


SENT, GUARD = -77.0, 64


def _guarded(n, dtype):
    return torch.full((n + GUARD,), SENT, device="cuda").to(dtype)


def _fwd(x, rows, K, ldx, yf, yb, ldy, keep, seed):
    from las import _hip
    rc = _hip.lib().las_dropout_pair_fwd(_hip.p(x), _hip._dt(x), rows, K, ldx, _hip.p(yf), _hip.p(yb), _hip._dt(yf), ldy, float(keep), int(seed),
                                         _hip.stream())
    torch.cuda.synchronize()
    return rc


def _bwd(gf, gb, ldg, rows, K, dx, lddx, keep, seed):
    from las import _hip
    rc = _hip.lib().las_dropout_pair_bwd(_hip.p(gf), _hip.p(gb), _hip._dt(gf), ldg, rows, K, _hip.p(dx), _hip._dt(dx), lddx, float(keep), int(seed),
                                         _hip.stream())
    torch.cuda.synchronize()
    return rc


def test_grid_stride_loop_forward_and_backward_exact():
    """rows = 16400, K = 509, ld = 512: 2 099 200 quads, 2 048 more than the 8192 x 256 threads the launches are capped at, in the forward
    (quads of the padded pitch) and in the backward (16400 x 128 quads of K) alike; fp32 in, bf16 out; seed 2^61 + 5.  Every element
    against loss_ref's masks, canaries behind every output."""
    rows, K, ld, keep, seed = 16400, 509, 512, 0.9, (1 << 61) + 5
    assert rows * (ld // 4) == 8192 * 256 + 2048 == rows * ((K + 3) // 4)
    g = torch.Generator().manual_seed(3)
    xh = torch.randn(rows, K, generator=g) + 3.0
    mf, mb = (torch.from_numpy(m) for m in R.dropout_masks(seed, rows, K, keep))
    x = xh.cuda()
    yf, yb = _guarded(rows * ld, torch.bfloat16), _guarded(rows * ld, torch.bfloat16)
    assert _fwd(x, rows, K, K, yf, yb, ld, keep, seed) == 0
    for yd, m in ((yf, mf), (yb, mb)):
        assert bool((yd[rows * ld:].float() == SENT).all())
        got = yd[:rows * ld].view(rows, ld).float().cpu()
        assert bool((got[:, K:] == 0).all())
        want = _scaled(xh, m, keep, torch.bfloat16)
        assert torch.equal(got[:, :K], want), ("first differing row", int((got[:, :K] != want).any(1).nonzero()[0]))
    del yf, yb, x
    gfh, gbh = torch.randn(rows, ld, generator=g), torch.randn(rows, ld, generator=g)
    dx = _guarded(rows * K, torch.bfloat16)
    assert _bwd(gfh.cuda(), gbh.cuda(), ld, rows, K, dx, K, keep, seed) == 0
    assert bool((dx[rows * K:].float() == SENT).all())
    want = _scaled(torch.where(mf, gfh[:, :K], torch.zeros(())) + torch.where(mb, gbh[:, :K], torch.zeros(())), None, keep, torch.bfloat16)
    got = dx[:rows * K].view(rows, K).float().cpu()
    assert torch.equal(got, want), ("first differing row", int((got != want).any(1).nonzero()[0]))


@pytest.mark.parametrize("dtype,out_bf16,K,ld", [(torch.float32, False, 39, 40), (torch.float32, True, 39, 64), (torch.bfloat16, True, 100, 128)])
def test_keep_one_is_the_identity(dtype, out_bf16, K, ld):
    """keep = 1.0: threshold 65536, above every 16-bit slice; scale 1: an exact copy (in the output's type) and zero padding, both ways"""
    from las.layers import _DropoutPair
    g = torch.Generator().manual_seed(K)
    x = (torch.randn(5, 33, K, generator=g) + 3.0).to(dtype).cuda().requires_grad_(True)
    yf, yb = _DropoutPair.apply(x, 1.0, 99, out_bf16, ld)
    want = x.detach().float().to(yf.dtype)
    for yd in (yf, yb):
        assert torch.equal(yd[..., :K], want) and bool((yd[..., K:] == 0).all())
    gf = torch.randn(5, 33, ld, generator=g).to(yf.dtype).cuda()
    gb = torch.randn(5, 33, ld, generator=g).to(yf.dtype).cuda()
    (dx,) = torch.autograd.grad((yf, yb), x, (gf, gb))
    assert torch.equal(dx, (gf[..., :K].float() + gb[..., :K].float()).to(dtype))


def test_no_rows_returns_zero_and_launches_nothing():
    K, ld = 39, 40
    x, yf, yb, dx = _guarded(K, torch.float32), _guarded(ld, torch.float32), _guarded(ld, torch.float32), _guarded(K, torch.float32)
    assert _fwd(x, 0, K, K, yf, yb, ld, 0.5, 1) == 0 and _bwd(yf, yb, ld, 0, K, dx, K, 0.5, 1) == 0
    assert all(bool((t == SENT).all()) for t in (yf, yb, dx))


def test_output_pitch_that_is_no_multiple_of_four_is_refused():
    from las import _hip
    rows, K = 3, 39
    x, yf, yb = _guarded(rows * K, torch.float32), _guarded(rows * 42, torch.float32), _guarded(rows * 42, torch.float32)
    for ldy in (41, 42, 43):
        assert _fwd(x, rows, K, K, yf, yb, ldy, 0.5, 1) == -1 and b"multiple of 4" in (_hip.lib().las_last_error() or b"")
        assert bool((yf == SENT).all()) and bool((yb == SENT).all())
    assert _fwd(x, rows, K, K, yf, yb, 40, 0.5, 1) == 0 and not bool((yf[:rows * 40] == SENT).any()) and bool((yf[rows * 40:] == SENT).all())


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_train_step_at_the_reference_default_dropout_rate(prec):
    """--dropout_rate 0.5 (the reference's default): the listener's recurrent layers draw their two masks in one launch per layer; the step
    trains (finite loss, every gradient finite and non-zero), is reproducible under torch.manual_seed, and differs from the no-dropout step."""
    from las import layers as L, variables as V
    from las.las import LAS, Listener, Speller
    from oracle import las_oracle as O
    args = make_args(enc_units=128, num_enc_layers=2, dec_units=128, num_dec_layers=1, embedding_size=64, attention_size=64, dropout_rate=0.5, lr=1e-3)
    xs, ys = synthetic_batch(6, 64, 12, 30, seed=2, min_frac=0.8)
    p0 = O.init_params(args, seed=1, cell="lstm")

    def step(rate, seed):
        args.dropout_rate = rate
        L.set_cell("lstm"); L.set_precision(prec)
        st = V.reset_default_store(device="cuda"); st.load(p0)
        torch.manual_seed(seed)
        las = LAS(args, Listener, Speller, {})
        loss = float(las.train(xs, ys)[0])
        torch.cuda.synchronize()
        las.check_status()
        return loss, st.flat_grad.clone()

    l1, g1 = step(0.5, 7)
    l2, g2 = step(0.5, 7)
    l3, g3 = step(0.5, 8)
    l0, g0 = step(0.0, 7)
    assert np.isfinite(l1) and bool(torch.isfinite(g1).all()) and float(g1.abs().max()) > 0
    assert l1 == l2 and torch.equal(g1, g2)
    assert l1 != l3 and l1 != l0
