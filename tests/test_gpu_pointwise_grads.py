"""The small gradient kernels of the C ABI that no test called directly: las_tanh_bwd_dt in its mixed fp32 / bf16 forms,
las_gemm_kk_tanhgrad (the dX product with the Tanh gradient fused in) and las_lstm_pointwise_bwd, each against float64 on the stored
operands."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENT = 7.0


def _half_ulp_bf16(x):
    """half the spacing of bf16 (8 significant bits) at |x|"""
    x = np.abs(np.asarray(x, np.float64))
    return np.where(x > 0, 2.0 ** (np.floor(np.log2(np.maximum(x, 1e-300))) - 8), 0.0)


@pytest.mark.parametrize("rows,cols,pitches", [(1, 1, (3, 2, 5)), (77, 130, (131, 136, 150)), (48 * 160, 512, (520, 513, 640)), (5, 7, (8, 9, 11))])
@pytest.mark.parametrize("key", range(8))
def test_tanh_bwd_mixed_types_and_pitches(rows, cols, pitches, key):
    """dX = dY (1 - Y^2); Y, dY, dX each fp32 or bf16 with three different pitches larger than cols.  fp32 output: 2^-22 |ref| (1 - Y^2 in
    one fused rounding, the product, slack of two); bf16 output: half a bf16 ulp of the reference on top."""
    from las import _hip
    dts = [torch.bfloat16 if key & b else torch.float32 for b in (4, 2, 1)]
    g = torch.Generator().manual_seed(rows + cols + key)
    ldy, lddy, lddx = pitches
    Y = torch.tanh(torch.randn(rows, ldy, generator=g) * 2.0).to(dts[0])
    Y.view(-1)[::11] = 1.0                                    # saturated: the factor is exactly 0
    Y.view(-1)[5::13] = -1.0
    Y.view(-1)[3::17] = 0.0                                   # factor exactly 1
    dY = (torch.randn(rows, lddy, generator=g) * 10.0 ** torch.randint(-3, 2, (rows, lddy), generator=g).float()).to(dts[1])
    Y, dY = Y.cuda(), dY.cuda()
    dX = torch.full((rows, lddx), SENT, dtype=dts[2], device="cuda")
    _hip.tanh_bwd(Y, ldy, dY, lddy, dX, lddx, rows, cols)
    torch.cuda.synchronize()
    y, dy = Y[:, :cols].double().cpu().numpy(), dY[:, :cols].double().cpu().numpy()
    ref = dy * (1.0 - y * y)
    got = dX[:, :cols].double().cpu().numpy()
    bound = 2.0 ** -22 * np.abs(ref) + (_half_ulp_bf16(ref) if dts[2] == torch.bfloat16 else 0.0)
    err = np.abs(got - ref)
    worst = float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))))
    print("tanh_bwd %s rows %d cols %d: worst error / bound %.3f" % ([str(d)[6:] for d in dts], rows, cols, worst))
    assert worst <= 1.0
    assert (dX[:, cols:].float() == SENT).all()              # the pitch gap of the destination is not written
    assert (ref == 0).any() and (got[ref == 0] == 0).all()


@pytest.mark.parametrize("out", ["bf16", "f32"])
@pytest.mark.parametrize("M,N,K", [(300, 2048, 512), (257, 132, 128), (6200, 2048, 192)])
def test_gemm_kk_tanhgrad_matches_float64(M, N, K, out):
    """C = (A B^T + bias) (1 - y^2): the tolerance of test_gemm_kk_bf16_operands_k_contiguous (fp32 accumulation over K, half a bf16 ulp
    of the result for a bf16 C); without y the bits of las_gemm_kk"""
    from las import _hip
    g = torch.Generator().manual_seed(M + N + K)
    A = (torch.randn(M, K + 8, generator=g) * 0.5).to(torch.bfloat16).cuda()
    B = (torch.randn(N, K, generator=g) * 0.5).to(torch.bfloat16).cuda()
    bias = torch.randn(N, generator=g).cuda()
    ldy = N + 12
    y = torch.tanh(torch.randn(M, ldy, generator=g) * 1.5)
    y.view(-1)[::7] = 1.0
    y.view(-1)[3::11] = -1.0
    y.view(-1)[5::13] = 0.0
    y = y.to(torch.bfloat16).cuda()
    dt = torch.bfloat16 if out == "bf16" else torch.float32
    C = torch.full((M, N + 4), SENT, dtype=dt, device="cuda")
    _hip.gemm_kk(A, B, C, M, N, K, K + 8, K, N + 4, bias=bias, tanh_y=y, ldy=ldy)
    torch.cuda.synchronize()
    yy = y[:, :N].double().cpu()
    plain = A[:, :K].double().cpu() @ B.double().cpu().t() + bias.double().cpu()
    ref = plain * (1.0 - yy * yy)
    got = C[:, :N].double().cpu()
    tol = 2e-5 * K ** 0.5 + (4e-3 * ref.abs().max().item() if out == "bf16" else 0)
    err = (got - ref).abs().max().item()
    print("gemm_kk_tanhgrad %s: max error %.3g, tolerance %.3g (without the factor the error would be %.3g)"
          % ((M, N, K, out), err, tol + 1e-4, (plain - ref).abs().max().item()))
    assert err < tol + 1e-4
    assert (plain - ref).abs().max().item() > 100 * (tol + 1e-4)           # the factor matters at this tolerance
    assert (got[yy.abs() == 1.0] == 0).all() and (yy.abs() == 1.0).any() and (yy == 0).any()
    assert (C[:, N:].float() == SENT).all()                                # nothing written past column N
    # y = NULL: las_gemm_kk itself
    C0 = torch.full((M, N + 4), SENT, dtype=dt, device="cuda")
    C1 = torch.full((M, N + 4), SENT, dtype=dt, device="cuda")
    _hip.gemm_kk(A, B, C0, M, N, K, K + 8, K, N + 4, bias=bias)
    _hip.check(_hip.lib().las_gemm_kk_tanhgrad(M, N, K, _hip.p(A), K + 8, _hip.p(B), K, _hip.p(C1), _hip.DT_BF16 if out == "bf16" else _hip.DT_F32,
                                               N + 4, _hip.p(bias), 0, None, 0, _hip.stream()), "las_gemm_kk_tanhgrad")
    torch.cuda.synchronize()
    assert torch.equal(C0, C1)
    # where y = 0 the fused result is the plain product's value
    assert torch.equal(C[:, :N][(yy == 0).cuda()], C0[:, :N][(yy == 0).cuda()])


@pytest.mark.parametrize("fb", [0.0, 1.0])
@pytest.mark.parametrize("with_dc", [True, False])
@pytest.mark.parametrize("N,H", [(1, 1), (5, 24), (48, 512), (1100, 512)])        # 1100 x 512 > 2048 x 256 threads: the grid-stride loop wraps
def test_lstm_pointwise_bwd_matches_float64_autograd(N, H, with_dc, fb):
    """dz, dc_prev of c' = c sigmoid(f + fb) + sigmoid(i) tanh(j), h' = tanh(c') sigmoid(o) (gate order i, j, f, o) for the loss
    sum(dh h') + sum(dc_in c').  sigmoid_acc / tanh_acc are held to 1e-5 on O(1) values by the forward test
    (test_pointwise_rows_equals_lookup_add_then_pointwise): 1e-5 max(1, |dh|max + |dc_in|max) absolute here."""
    from las import _hip
    g = torch.Generator().manual_seed(N * 3 + H + int(with_dc) + int(fb))
    z = torch.randn(N, 4 * H, generator=g) * 2.0
    z.view(-1)[::19] = 20.0                                   # saturated gates
    z.view(-1)[7::23] = -20.0
    c = torch.randn(N, H, generator=g)
    dh = torch.randn(N, H, generator=g)
    dc_in = torch.randn(N, H, generator=g) * 0.5 if with_dc else None
    zd, cd = z.double().requires_grad_(True), c.double().requires_grad_(True)
    i, j, f, o = zd[:, :H], zd[:, H:2 * H], zd[:, 2 * H:3 * H], zd[:, 3 * H:]
    c2 = cd * torch.sigmoid(f + fb) + torch.sigmoid(i) * torch.tanh(j)
    h2 = torch.tanh(c2) * torch.sigmoid(o)
    loss = (dh.double() * h2).sum() + ((dc_in.double() * c2).sum() if with_dc else 0.0)
    dz_ref, dc_ref = torch.autograd.grad(loss, [zd, cd])
    dz = torch.full((N, 4 * H), SENT, device="cuda")
    dcp = torch.full((N, H), SENT, device="cuda")
    zc, cc, dhc = z.cuda(), c.cuda(), dh.cuda()
    dcc = dc_in.cuda() if with_dc else None
    _hip.check(_hip.lib().las_lstm_pointwise_bwd(_hip.p(zc), _hip.p(cc), _hip.p(dhc), _hip.p(dcc), N, H, fb, _hip.p(dz), _hip.p(dcp),
                                                 _hip.stream()), "las_lstm_pointwise_bwd")
    torch.cuda.synchronize()
    tol = 1e-5 * max(1.0, dh.abs().max().item() + (dc_in.abs().max().item() if with_dc else 0.0))
    e_dz = (dz.double().cpu() - dz_ref).abs()
    e_dc = (dcp.double().cpu() - dc_ref).abs().max().item()
    per_gate = [e_dz[:, k * H:(k + 1) * H].max().item() for k in range(4)]
    print("lstm_pointwise_bwd N %d H %d dc_in %s fb %g: max error dz (i, j, f, o) %s, dc_prev %.3g, tolerance %.3g" % (N, H, with_dc, fb, per_gate, e_dc, tol))
    assert max(per_gate) < tol and e_dc < tol
    for k in range(4):                                        # every gate's gradient is large enough for the tolerance to bite
        assert dz_ref[:, k * H:(k + 1) * H].abs().max().item() > (1e3 * tol if N * H > 100 else 0.0)
    # the forget gate's bias matters at this tolerance
    if fb and N * H > 100:
        c2b = cd * torch.sigmoid(f) + torch.sigmoid(i) * torch.tanh(j)
        lb = (dh.double() * torch.tanh(c2b) * torch.sigmoid(o)).sum() + ((dc_in.double() * c2b).sum() if with_dc else 0.0)
        assert (torch.autograd.grad(lb, [zd])[0] - dz_ref).abs().max().item() > 1e3 * tol
