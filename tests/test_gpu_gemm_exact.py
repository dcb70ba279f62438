"""las_gemm / las_gemm_dt (csrc/gemm.hip), every planned kernel against float64 -- exactly.

The table tests/gemm_cases.py holds a case for every plan the dispatch can reach (tests/test_gemm_plan_host.py proves that without a
GPU).  Each case runs here with operands for which fp32 arithmetic is exact: A and B from {-3, -2, -1, 1, 2, 3}, C0 and bias integers in
[-8, 8], alpha in {1, 2}, beta in {0, 1, -1}.  Every operand is exact in bf16 (rounding while staging is the identity), every product an
integer of magnitude <= 9, and every partial sum in ANY order of association -- the MFMA's, the four waves' LDS reduction of the skinny
kernel, split-K partials and their reduce -- an integer below 2 * 9 * 4100 + 16 < 2^24, hence exact in fp32.  So the result must EQUAL
the float64 reference bit for bit, in both precisions: the tolerance is zero, derived and not measured.  No operand is zero, so one
dropped, doubled or wrongly masked contraction row, a wrong k tail or two swapped rows of a register transpose moves a result by >= 1.
Pitch padding and everything in front of an operand's offset are NaN (a tail that is read and not zero-filled turns the output into
NaN), C lies in a wider and taller tensor of sentinels that must survive, and the plan the library answers for the very tensors that
are launched must be the one the table records -- so every case names the kernel it ran.

What integers cannot show is below them: the fp32 -> bf16 rounding of the staging paths (round-to-nearest-even, on random operands and
on operands that are all ties) and the alpha / beta / bias / tanh epilogue of each kernel family."""
import numpy as np
import pytest
import torch

import gemm_cases as G

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _ints(shape, gen, lo=1, hi=3):
    """random integers of magnitude lo..hi, either sign, as fp32"""
    mag = torch.randint(lo, hi + 1, shape, generator=gen)
    sign = torch.randint(0, 2, shape, generator=gen) * 2 - 1
    return (mag * sign).float()


def _place(values, rows, cols, ld, off, batch, dtype):
    """values [batch, rows, cols] inside a flat tensor: `off` elements in, row pitch ld, batch stride rows * ld; NaN everywhere else
    (in front of the offset, in the pitch padding and in eight elements behind the last row)"""
    flat = torch.full((off + batch * rows * ld + 8,), NAN)
    flat[off:off + batch * rows * ld].view(batch, rows, ld)[:, :, :cols] = values
    return flat.to(dtype).cuda()


def _setup(c, A, B, C0):
    """device tensors and the keyword arguments _hip.gemm / _hip.gemm_plan take for case c with operand values A [batch, a_rows, a_cols],
    B likewise, C0 [batch, M, N]: C is the top left corner of a [batch, M + 2, N + 4] tensor of sentinels (7.0)"""
    g = G.geometry(c)
    dt = torch.bfloat16 if c.in_dtype == G.BF16 else torch.float32
    Ad = _place(A, g["a_rows"], g["a_cols"], g["lda"], c.off_a, c.batch, dt)
    Bd = _place(B, g["b_rows"], g["b_cols"], g["ldb"], c.off_b, c.batch, dt)
    Cfull = torch.full((c.batch, c.M + 2, c.N + 4), 7.0)
    Cfull[:, :c.M, :c.N] = C0
    kw = dict(transA=bool(c.tA), transB=bool(c.tB), M=c.M, N=c.N, K=c.K, lda=g["lda"], ldb=g["ldb"], ldc=c.N + 4, batch=c.batch,
              strideA=g["strideA"], strideB=g["strideB"], strideC=(c.M + 2) * (c.N + 4) if c.batch > 1 else 0,
              mask_period=c.mask_period, mask_skip=c.mask_skip, a_off=c.off_a, b_off=c.off_b)
    return Ad, Bd, Cfull.cuda(), kw


def _contract(c, A, B):
    """float64 op(A) . op(B) per batch entry, masked contraction rows zeroed"""
    a = A.double().transpose(1, 2) if c.tA else A.double()
    b = B.double().transpose(1, 2) if c.tB else B.double()
    if c.mask_period:
        keep = torch.tensor([(k % c.mask_period) != c.mask_skip for k in range(c.K)], dtype=torch.float64)
        a = a * keep
    return a @ b


def _sentinels_untouched(Cd, c):
    Cc = Cd.cpu()
    return bool((Cc[:, c.M:, :] == 7.0).all()) and bool((Cc[:, :, c.N:] == 7.0).all())


def _recorded_plan(c):
    return (G.KERNELS[c.plan[0]],) + tuple(c.plan[1:])


def _integer_case(c, seed):
    gen = torch.Generator().manual_seed(seed)
    g = G.geometry(c)
    A = _ints((c.batch, g["a_rows"], g["a_cols"]), gen)
    B = _ints((c.batch, g["b_rows"], g["b_cols"]), gen)
    C0 = torch.randint(-8, 9, (c.batch, c.M, c.N), generator=gen).float()
    bias = torch.randint(-8, 9, (c.N,), generator=gen).float() if c.bias else None
    ref = c.alpha * _contract(c, A, B) + c.beta * C0.double()
    if bias is not None:
        ref = ref + bias.double()
    return A, B, C0, bias, ref


def _run_integer_case(c, seed):
    from las import _hip
    A, B, C0, bias, ref = _integer_case(c, seed)
    assert ref.abs().max().item() < 2 ** 24 and 2 * 9 * c.K + 16 < 2 ** 24          # the exactness argument holds for this case
    Ad, Bd, Cd, kw = _setup(c, A, B, C0)
    biasd = None if bias is None else bias.cuda()
    plan = _hip.gemm_plan(c.prec, Ad, Bd, **kw)
    assert tuple(plan) == _recorded_plan(c), (G.case_id(c), plan)
    _hip.gemm(c.prec, Ad, Bd, Cd, alpha=float(c.alpha), beta=float(c.beta), bias=biasd, **kw)
    torch.cuda.synchronize()
    return Cd, ref, (Ad, Bd, biasd, kw)


@pytest.mark.parametrize("idx", range(len(G.RUN_CASES)), ids=[G.case_id(c) for c in G.RUN_CASES])
def test_every_planned_kernel_equals_float64_on_integer_operands(idx):
    c = G.RUN_CASES[idx]
    Cd, ref, _ = _run_integer_case(c, 1000 + idx)
    got = Cd[:, :c.M, :c.N].cpu().double()
    if not torch.equal(got, ref):
        bad = ((got != ref) | got.isnan()).nonzero()
        first = [(int(b), int(r), int(k), got[b, r, k].item(), ref[b, r, k].item()) for b, r, k in bad[:8]]
        pytest.fail("%s: %d of %d outputs differ; rows %s, columns %s; first (batch, row, col, got, want): %s"
                    % (_recorded_plan(c), len(bad), ref.numel(), sorted(set(bad[:, 1].tolist()))[:12], sorted(set(bad[:, 2].tolist()))[:12], first))
    assert _sentinels_untouched(Cd, c), "%s wrote outside C[:M, :N]" % (_recorded_plan(c),)


@pytest.mark.parametrize("idx", range(len(G.REFUSED_CASES)), ids=[G.case_id(c) for c in G.REFUSED_CASES])
def test_refused_calls_are_refused_by_the_plan_and_by_the_launch(idx):
    from las import _hip
    c = G.REFUSED_CASES[idx]
    A, B, C0, bias, _ = _integer_case(c, 5000 + idx)
    Ad, Bd, Cd, kw = _setup(c, A, B, C0)
    with pytest.raises(RuntimeError) as e_plan:
        _hip.gemm_plan(c.prec, Ad, Bd, **kw)
    with pytest.raises(RuntimeError) as e_run:
        _hip.gemm(c.prec, Ad, Bd, Cd, alpha=float(c.alpha), beta=float(c.beta), bias=None if bias is None else bias.cuda(), **kw)
    assert "rc=-1" in str(e_plan.value) and "rc=-1" in str(e_run.value)
    assert c.plan in str(e_plan.value) and c.plan in str(e_run.value)
    torch.cuda.synchronize()
    assert torch.equal(Cd[:, :c.M, :c.N].cpu(), C0) and _sentinels_untouched(Cd, c)           # nothing was launched


def test_split_k_and_z_grouped_products_repeat_bit_for_bit():
    """Exactness implies it; one explicit assertion: the same call twice, the same bits (split-K through the z-grouped grid with its
    fixed-order reduce, a z-grouped batch with a second round of eight, the skinny kernel's K slices)."""
    picked = []
    for want in (lambda p, c: p[0] == 2 and p[5] == 1 and p[6] > 1, lambda p, c: p[5] == 1 and c.batch == 9,
                 lambda p, c: p[0] == 5 and p[6] > 1, lambda p, c: p[0] == 3 and p[6] > 1):
        picked.append(next(i for i, c in enumerate(G.RUN_CASES) if want(c.plan, c)))
    for idx in picked:
        c = G.RUN_CASES[idx]
        C1, _, _ = _run_integer_case(c, 1000 + idx)
        C2, _, _ = _run_integer_case(c, 1000 + idx)
        assert torch.equal(C1.cpu(), C2.cpu()), G.case_id(c)


# ---- rounding: fp32 operands in bf16 mode -----------------------------------------------------------------------------------------------
# One case per staging path that converts, over the tile shapes of the generic and the branch-free kernel:
#   (name, tA, tB, M, N, K, alignment, kernel, tile_m, loader, what it stages)
ROUNDING = (
    ("generic48_NN", 0, 0, 33, 72, 100, "odd", "bf16_generic", 48, 0, "A: tile_sstore k-contiguous, B: tile_sstore row-contiguous"),
    ("generic64_TT", 1, 1, 68, 72, 100, "odd", "bf16_generic", 64, 0, "A: tile_sstore row-contiguous, B: tile_sstore k-contiguous"),
    ("generic128_NN", 0, 0, 130, 132, 100, "offset", "bf16_generic", 128, 0, "both tile_sstore branches at 128 x 128"),
    ("fast64_NN", 0, 0, 68, 72, 100, "aligned", "bf16_fast", 64, 1, "A: pack_k4, B: transpose4(float4)"),
    ("fast64_TT", 1, 1, 68, 72, 100, "aligned", "bf16_fast", 64, 2, "A: transpose4(float4), B: pack_k4"),
    ("fast128_TN", 1, 0, 132, 132, 100, "aligned", "bf16_fast", 128, 0, "both transpose4(float4) at 128 x 128"),
    ("fast128_NT", 0, 1, 132, 132, 100, "aligned", "bf16_fast", 128, 3, "both pack_k4 at 128 x 128"),
)


def _ties(shape, gen):
    """fp32 values halfway between two bf16 neighbours: low 16 bits 0x8000, the upper halves those of random normal bf16 values (even
    and odd mixed) -- round-to-nearest-even goes up for the odd ones and down for the even ones; truncation and round-half-up each miss
    half of them by a whole bf16 ulp"""
    hi = (torch.randn(shape, generator=gen) * 0.5).to(torch.bfloat16).view(torch.int16).to(torch.int32) & 0xFFFF
    bits = (hi.long() << 16) | 0x8000
    x = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32).view(torch.float32)
    assert (hi & 1).float().mean().item() > 0.25 and (1 - (hi & 1)).float().mean().item() > 0.25
    return x


@pytest.mark.parametrize("operands", ["randn", "ties"])
@pytest.mark.parametrize("case", ROUNDING, ids=[r[0] for r in ROUNDING])
def test_bf16_mode_rounds_fp32_operands_to_nearest_even(case, operands):
    """Reference: float64 on x.to(torch.bfloat16) (torch rounds to nearest even).  Tolerance: the suite's bound for fp32 accumulation of
    exact bf16 products, 3e-6 sqrt(K) max(1, |ref|) (test_gpu_gemm.py test_weight_gradient_form_bf16_tn); a truncating or half-up
    conversion is off by 2^-9 relative per operand, orders of magnitude above it on the tie set."""
    from las import _hip
    name, tA, tB, M, N, K, al, kernel, tile_m, loader, _ = case
    pa, oa = G.place(M if tA else K, al)
    pb, ob = G.place(K if tB else N, al)
    c = G.Case(1, G.F32, tA, tB, M, N, K, 1, 0, 0, pa, pb, oa, ob, 1, 0, 0, None)
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    g = G.geometry(c)
    make = (lambda s: torch.randn(s, generator=gen) * 0.5) if operands == "randn" else (lambda s: _ties(s, gen))
    A, B = make((1, g["a_rows"], g["a_cols"])), make((1, g["b_rows"], g["b_cols"]))
    Ad, Bd, Cd, kw = _setup(c, A, B, torch.zeros(1, M, N))
    plan = _hip.gemm_plan(1, Ad, Bd, **kw)
    assert (plan.kernel, plan.tile_m, plan.loader, plan.in_bf16) == (kernel, tile_m, loader, 0), plan
    _hip.gemm(1, Ad, Bd, Cd, **kw)
    ref = _contract(c, A.to(torch.bfloat16), B.to(torch.bfloat16))
    err = (Cd[:, :M, :N].cpu().double() - ref).abs().max().item()
    tol = 3e-6 * K ** 0.5 * max(1.0, ref.abs().max().item())
    print("rounding %s %s: max err %.3e, tol %.3e, max|ref| %.3f" % (name, operands, err, tol, ref.abs().max().item()))
    assert err < tol, (name, operands, err, tol)
    assert _sentinels_untouched(Cd, c)


# ---- epilogue: alpha, beta, bias, tanh ------------------------------------------------------------------------------------------------
# (name, prec, M, N, K, alignment, kernel, splitk > 1, the tanh it ends in)
EPILOGUE = (
    ("generic_bf16", 1, 33, 72, 36, "odd", "bf16_generic", False, "tanhf"),
    ("fast_bf16", 1, 68, 72, 36, "aligned", "bf16_fast", False, "tanh_fast"),
    ("mf32", 0, 68, 72, 36, "aligned", "mf32", False, "tanhf"),
    ("mf32_skinny", 0, 33, 72, 100, "odd", "mf32_skinny", False, "tanhf"),
    ("fast_bf16_splitk", 1, 68, 72, 2100, "aligned", "bf16_fast", True, "tanhf"),
)
# Largest |kernel - float64 tanh(float64 argument)| over the EPILOGUE cases, measured on an MI355X, and the bound held here: 4 x the
# measurement (the margin is for arguments the cases do not sample).  Not derivable: tanh_fast is a rcp of an exp2 approximation and
# tanhf the device library's.  Measured: tanhf 1.4357e-07 (generic_bf16 9.86e-08, mf32 1.44e-07, mf32_skinny 9.21e-08, fast_bf16_splitk
# 1.38e-07), tanh_fast 1.9191e-07 (fast_bf16); the bounds are 5.74e-07 and 7.68e-07.
TANH_MEASURED = {"tanhf": 1.4357e-07, "tanh_fast": 1.9191e-07}
TANH_BOUND = {k: 4 * v for k, v in TANH_MEASURED.items()}


@pytest.mark.parametrize("case", EPILOGUE, ids=[e[0] for e in EPILOGUE])
def test_epilogue_alpha_beta_bias_tanh(case):
    """C = tanh(0.37 A.B + bias + 0.5 C0) with integer operands: A is +-1 on about 19 of its K contraction rows' entries per row and 0
    elsewhere, B is +-1, so the accumulator is an exact integer of a few units and the argument spans about [-4, 4]; bias and C0 are
    real.  The whole error is the epilogue's: fp32 alpha / bias / beta arithmetic and the tanh.  Bounds (TANH_BOUND): 4 x the largest
    error measured over these cases on an MI355X -- tanhf (generic bf16, exact-fp32, skinny, split-K reduce) measured 1.4357e-07,
    bound 5.74e-07; tanh_fast (branch-free bf16 kernel) measured 1.9191e-07, bound 7.68e-07."""
    from las import _hip
    name, prec, M, N, K, al, kernel, split, fn = case
    pa, oa = G.place(K, al)
    pb, ob = G.place(N, al)
    c = G.Case(prec, G.F32, 0, 0, M, N, K, 1, 0, 0, pa, pb, oa, ob, 1, 0, 1, None)
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    A = _ints((1, M, K), gen, 1, 1) * (torch.rand((1, M, K), generator=gen) < min(1.0, 19.0 / K)).float()
    B = _ints((1, K, N), gen, 1, 1)
    C0 = torch.randn(1, M, N, generator=gen)
    bias = torch.randn(N, generator=gen) * 0.5
    Ad, Bd, Cd, kw = _setup(c, A, B, C0)
    plan = _hip.gemm_plan(prec, Ad, Bd, **kw)
    assert plan.kernel == kernel and (plan.splitk > 1) == split, plan
    _hip.gemm(prec, Ad, Bd, Cd, alpha=0.37, beta=0.5, bias=bias.cuda(), act=_hip.ACT_TANH, **kw)
    arg = float(np.float32(0.37)) * _contract(c, A, B) + bias.double() + 0.5 * C0.double()
    assert arg.min().item() < -3.5 and arg.max().item() > 3.5 and arg.abs().max().item() < 9, (arg.min().item(), arg.max().item())
    err = (Cd[:, :M, :N].cpu().double() - torch.tanh(arg)).abs().max().item()
    print("epilogue %s (%s): max err %.4e, argument in [%.2f, %.2f]" % (name, fn, err, arg.min().item(), arg.max().item()))
    assert err <= TANH_BOUND[fn], (name, fn, err, TANH_BOUND[fn])
    assert _sentinels_untouched(Cd, c)
