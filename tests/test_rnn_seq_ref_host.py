"""The Listener sweeps' rounded-operand reference (tests/rnn_seq_ref.py) checked without a GPU: it is the oracle when its roundings are
off; its bounds are four times what an fp32 evaluation of the same recurrence is away from it; eight plausible kernel mistakes land
outside them; and the case tables of tests/test_gpu_rnn_seq_matrix.py cover every kernel the plan can reach."""
import functools

import pytest
import torch

import helpers  # noqa: F401  (sys.path)
import rnn_seq_ref as RR
import test_gpu_rnn_seq_matrix as M
import test_rnn_seq_plan as G

ALL_CASES = M.MATRIX + M.CHUNK_CASES
DISTINCT_KERNELS = 63          # distinct (cell, H, P, rows per tile, kernel) the grid reaches: a new instantiation needs a new case


@pytest.mark.parametrize("cell", ["lstm", "rnn"])
@pytest.mark.parametrize("reverse", [False, True])
def test_reference_without_roundings_is_the_oracle(cell, reverse):
    from oracle import las_oracle as O
    B, T, H = 5, 7, 24
    GH = (4 if cell == "lstm" else 1) * H
    g = torch.Generator().manual_seed(3)
    xp = torch.randn(B, T, GH, generator=g, dtype=torch.float64)
    whh = torch.randn(H, GH, generator=g, dtype=torch.float64) * 0.3
    R = torch.randn(B, T, H, generator=g, dtype=torch.float64)
    x = xp.clone().requires_grad_(True)
    kernel = torch.cat([torch.eye(GH, dtype=torch.float64), whh], 0)
    h = O._run_dir(x, kernel, torch.zeros(GH, dtype=torch.float64), cell, reverse=reverse)
    (h * R).sum().backward()
    for P, ks in ((1, False), (2, True)):
        ref = RR.reference(xp, whh, R, cell, reverse, rounding=False, P=P, ksplit=ks)
        assert (ref["h"] - h.detach()).abs().max().item() < 1e-12
        assert (ref["dz"] - x.grad).abs().max().item() < 1e-12
        assert (ref["db"] - x.grad.sum((0, 1))).abs().max().item() < 1e-12


@functools.lru_cache(maxsize=None)
def _emulation(case, mutate=None, seed=None):
    return M.case_reference(case, fn=RR.emulate_fp32, mutate=mutate, seed=seed)


def _residual_distance(emu, ref):
    return max(RR.bias_residual_distance(RR.bias_residual(emu[d], RR.DB_INIT[d]), RR.bias_residual(ref[d])) for d in range(2))


def _worst(case, mutate=None):
    ref, emu = M._reference(case), _emulation(case, mutate)
    out = {}
    for d in range(2):
        for k, v in RR.distances(emu[d], ref[d]).items():
            out[k] = max(out.get(k, 0.0), v)
    if M.short_k_split(case):
        out["db_res"] = _residual_distance(emu, ref)
        if mutate is None:           # the bound's measurement: more inputs of the same shape (what a tie does to the residual depends on where it falls)
            for seed in RR.RESIDUAL_SEEDS:
                out["db_res"] = max(out["db_res"], _residual_distance(_emulation(case, None, seed), M.case_reference(case, seed=seed)))
    return out


def test_bounds_are_four_times_the_fp32_emulation_distance():
    """MEASURED is the worst distance of emulate_fp32 from the float64 reference over all cases; BOUNDS is four times that.  The figures
    depend on the order in which the host's BLAS sums a dot product only through bf16 ties that round the other way, so what is asserted
    is that this host's emulation is inside the recorded bounds; the fresh figures are printed."""
    worst = {}
    for case in ALL_CASES:
        for k, v in _worst(case).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("emulate_fp32 vs float64 reference:", {k: "%.3e" % v for k, v in worst.items()})
    assert set(worst) == set(RR.BOUNDS)
    for k, v in worst.items():
        assert RR.BOUNDS[k] == 4.0 * RR.MEASURED[k] and RR.MEASURED[k] > 0
        assert v <= RR.BOUNDS[k], (k, v, RR.BOUNDS[k])


@pytest.mark.parametrize("mutate", RR.MUTATIONS)
def test_mutation_leaves_the_bounds(mutate):
    """Each mistake, applied to the fp32 emulation, is outside the bound of at least one quantity in every case it applies to.

    db_after_rounding is the exception that had to be narrowed.  Against the bound of db it reaches 0.05 to 0.30 of it in all 23 K-split
    cases, and no input can change that: the mistake moves a bias sum by at most 2^-9 of sum |dZ|, a bf16 tie that rounds the other way
    moves it by as much, and the bound is four times the latter.  What separates it is the rounding residual itself (rnn_seq_ref.bias_residual,
    exactly zero under the mistake) on sweeps of one or two steps, in the median over the columns (bias_residual_distance says why not in the
    maximum): there the emulation's residual is within 5e-6 of the reference's and the mistake 1e-4 to 2e-3 away; from T = 9 on the emulation's own residual is as far from the reference's as zero is (0.02 against 0.02 at
    LSTM H = 512, 0.075 against 0.075 at the tanh cell's H = 512).  So the mutation applies to the K-split cases with T <= 2."""
    missed, n = [], 0
    for case in ALL_CASES:
        cell, H, B, T, _, _, P, kf, rf, kb, rbw, launches = case
        if not RR.mutation_applies(mutate, "lstm" if cell else "rnn", B, T, P, rbw, kb.startswith("BWD_KS"), launches):
            continue
        n += 1
        w = _worst(case, mutate)
        if not any(v > RR.BOUNDS[k] for k, v in w.items()):
            missed.append((case[:6], {k: "%.2f" % (v / RR.BOUNDS[k]) for k, v in w.items()}))
    assert n > 0
    assert not missed, "%s stays inside every bound in %d of %d cases: %s" % (mutate, len(missed), n, missed)


def _grid_tuples():
    from las import _hip
    out = set()
    for prec, cell, H, B, fl, P in G.grid():
        for bwd in (False, True):
            for mode in (0, M.MODE_ROWS, M.MODE_CHUNKS, M.MODE_CHUNKS | M.MODE_PROGRESS):
                k, p, rows, _ = _hip.rnn_seq_plan_kernel(cell, prec, B, H, fl | (_hip.seq_p(P) if P else 0), bwd, mode)
                if prec == 0:
                    assert (k, p, rows) == ("NONE", 0, 0)            # the fp32 paths have no SweepKernel
                elif k != "NONE":
                    out.add((cell, H, p, rows, k))
    return out


def test_case_tables_cover_every_planned_kernel():
    from las import _hip
    claimed = set()
    for case in ALL_CASES:
        cell, H, B, T, fl, p, P, kf, rf, kb, rbw, launches = case
        flags = M.case_flags(case)
        max_tiles = (256 // P // 8) * 8 // 2                         # row tiles per launch on the MI355X's 256 compute units
        assert _hip.rnn_seq_plan_kernel(cell, 1, B, H, flags, False) == (kf, P, rf, -(-(-(-B // rf)) // max_tiles)), case
        assert _hip.rnn_seq_plan_kernel(cell, 1, B, H, flags, True) == (kb, P, rbw, launches), case
        claimed.update(M.case_claims(case))
    for cell, H, B, T, p, mode, P, kern, rows in M.MODE_CASES:
        assert _hip.rnn_seq_plan_kernel(cell, 1, B, H, M.seq_p(p) if p else 0, kern.startswith("BWD"), mode)[:3] == (kern, P, rows)
        claimed.add((cell, H, P, rows, kern))
    reach = _grid_tuples()
    assert len(reach) == DISTINCT_KERNELS
    assert reach - claimed == set(), "planned kernels without a case: %s" % sorted(reach - claimed)
    assert claimed - reach == set()
    for c in M.FLAG_BASES:                                            # the placement flags leave the plan's kernel alone
        for extra in (M.NO_WARMERS, M.AGENT_GRANULES):
            for bwd in (False, True):
                assert _hip.rnn_seq_plan_kernel(c[0], 1, c[2], c[1], M.case_flags(c) | extra, bwd) == \
                    _hip.rnn_seq_plan_kernel(c[0], 1, c[2], c[1], M.case_flags(c), bwd)


def test_plan_kernel_agrees_with_the_mode_queries():
    """the query reads the same plan as the four *_ok queries: a mode's variant is planned exactly where its query says yes"""
    from las import _hip
    for prec, cell, H, B, fl, P in G.grid():
        flags = fl | (_hip.seq_p(P) if P else 0)
        rows_ok, ch_ok = _hip.rnn_seq_fwd_rows_ok(cell, prec, B, H, flags), _hip.rnn_seq_bwd_chunks_ok(cell, prec, B, H, flags)
        assert (_hip.rnn_seq_plan_kernel(cell, prec, B, H, flags, False, M.MODE_ROWS)[0] == "FWD_HW8_RAGGED") == rows_ok
        if ch_ok:
            assert _hip.rnn_seq_plan_kernel(cell, prec, B, H, flags, True, M.MODE_CHUNKS)[0] == "BWD_KS8_CH"
            assert _hip.rnn_seq_plan_kernel(cell, prec, B, H, flags, True, M.MODE_CHUNKS | M.MODE_PROGRESS)[0] == "BWD_KS8_CH_PG"
