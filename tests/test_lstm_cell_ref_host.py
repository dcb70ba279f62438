"""tests/lstm_cell_ref.py without a GPU: the float64 restatement against a plain torch cell, the tolerances of
tests/test_gpu_lstm_cell_rows.py against the errors the las_lstm_cell_rows kernels could make at that test's own inputs, and the case
tables against las_lstm_cell_rows_plan (host arithmetic: the dispatch decision both launchers share)."""
import ctypes

import pytest
import torch

import helpers  # noqa: F401  (sys.path)
import lstm_cell_ref as R


def test_reference_is_the_basic_lstm_cell_on_rounded_operands():
    """against torch's float64 ops written out independently (lang/char_rnn_model.py:57-66: i, j, f, o; forget bias inside the sigmoid)"""
    p = R.make_problem("L1x", 9, 64, 32)
    r = R.lstm_cell_ref(p)
    zin = torch.cat([R.rnd(p["x"]), R.rnd(p["h"])], 1).double()
    z = zin @ torch.cat([R.rnd(p["Wx"]), R.rnd(p["Wh"])], 0).double() + p["bias"].double()
    i, j, f, o = z.chunk(4, 1)
    c = p["c_prev"].double() * torch.sigmoid(f + 1.0) + torch.sigmoid(i) * torch.tanh(j)
    assert (r["c"] - c).abs().max() < 1e-12 and (r["h"] - torch.tanh(c) * torch.sigmoid(o)).abs().max() < 1e-12
    assert r["gates"].shape == (9, 128) and r["h_bf16"].dtype == torch.bfloat16
    # one-hot: ids 0 and 1 clamp to row 0, V + 1 is the last row; a prefix is the same rows
    p = R.make_problem("L0", 9, 0, 32)
    assert p["ids"][:3].tolist() == [0, 1, R.V + 1]
    z = R.rnd(p["h"][:3]).double() @ R.rnd(p["Wh"]).double() + p["bias"].double() + p["xrows"].double()[[0, 0, R.V - 1]]
    i, j, f, o = z.chunk(4, 1)
    c = p["c_prev"][:3].double() * torch.sigmoid(f) + torch.sigmoid(i) * torch.tanh(j)
    assert (R.lstm_cell_ref(p, M=3)["c"] - c).abs().max() < 1e-12 and torch.equal(R.lstm_cell_ref(p, M=3)["c"], R.lstm_cell_ref(p)["c"][:3])


def _ref_cases():
    """the launches test_gpu_lstm_cell_rows.py holds to the reference: every single case at ROWS rows, both problems of one pair case"""
    out = [(form, R.ROWS, I, H, padded) for form, I, H, padded in R.SINGLE_CASES]
    (fa, Ma, Ia, Ha), (fb, Mb, Hb), _, padded, _ = R.PAIR_CASES[R.PAIR_REF_CASE]
    return out + [(fa, Ma, Ia, Ha, padded), (fb, Mb, 0, Hb, padded)]


@pytest.mark.parametrize("mutate", R.MUTATIONS)
def test_tolerances_catch_the_planted_errors(mutate):
    """Each planted error moves some element of c' or h' by at least 10 x the tolerance of the path it is checked on (2e-5 exact, 2e-3
    fast), in every case it can occur in: the factor of 10 is room for the kernel's own rounding.  (h_rows_at_ld_H counts the padding
    columns as zeros; the GPU test fills them with NaN, which no output may show.)"""
    seen = 0
    for form, M, I, H, padded in _ref_cases():
        if not R.mutation_applies(mutate, form, padded):
            continue
        p = R.make_problem(form, M, I, H)
        good, bad = R.lstm_cell_ref(p), R.lstm_cell_ref(p, mutate=mutate)
        moved = max((good[k] - bad[k]).abs().max().item() for k in ("c", "h"))
        ratio = moved / R.tol(form)
        print("%-26s %-4s M=%d I=%d H=%d: moves %.3e = %.0f x tolerance" % (mutate, form, M, I, H, moved, ratio))
        assert ratio >= 10.0, (mutate, form, I, H, moved)
        if mutate == "last_row_from_row_before":      # ... and it is the last row that moves
            assert (good["c"][:M - 1] - bad["c"][:M - 1]).abs().max().item() == 0.0
        seen += 1
    assert seen > 0


def _plan(a, b=None):
    from las import _hip
    return _hip.lib().las_lstm_cell_rows_plan(None if a is None else ctypes.byref(a), None if b is None else ctypes.byref(b))


def _single_args(form, M, I, H, padded):
    return R.fill_args(form, M, I, H, I + (R.PAD if padded else 0), H + (R.PAD if padded else 0), R.FAKE_PTRS)


def pair_args(case, ptr_a=R.FAKE_PTRS, ptr_b=R.FAKE_PTRS):
    (fa, Ma, Ia, Ha), (fb, Mb, Hb), _, padded, _ = case
    pad = R.PAD if padded else 0
    return R.fill_args(fa, Ma, Ia, Ha, Ia + pad, Ha + pad, ptr_a), R.fill_args(fb, Mb, 0, Hb, 0, Hb + pad, ptr_b)


def test_tables_name_the_plan_and_reach_every_code_of_a_shipping_build():
    """las_lstm_cell_rows_plan over fake, aligned pointers (it dereferences none) gives every table row the code the row names, and the
    tables together reach every value the decision returns in a shipping build.  The 128-row pair kernel is not among them: only the
    development switch LAS_DEV_LB_PAIR_ROWS selects it, and the shipping library does not export that switch."""
    from las import _hip
    assert not hasattr(_hip.lib(), "las_dev_lstm_cell_pair_rows")
    reached = set()
    for form, I, H, padded in R.SINGLE_CASES:
        for M in R.PREFIXES:
            want = R.PLAN_BY_PREFIX[form][M]
            got = _plan(_single_args(form, M, I, H, padded))
            assert (got < 0) if want == R.REFUSED else (got == want), (form, I, H, M, got, want)
            reached.add(want)
    for case in R.PAIR_CASES:
        a, b = pair_args(case)
        assert _plan(a, b) == case[2], (case, _plan(a, b))
        assert _plan(a) >= 0 and _plan(b) >= 0          # served as two launches, each problem is served
        reached.add(case[2])
    for name in R.REFUSALS:
        a = R.refusal_args(name, R.FAKE_PTRS)
        assert _plan(a) < 0, name
        if a is not None:                               # ... and as either problem of a pair
            ok = pair_args(R.PAIR_CASES[0])
            assert _plan(a, ok[1]) < 0 and _plan(ok[0], a) < 0, name
    assert reached == R.SHIPPING_PLAN_CODES, (sorted(reached), sorted(R.SHIPPING_PLAN_CODES))
    # the boundaries of the single launch, each side of each
    for M, want in ((127, 0), (128, 32), (256, 32), (257, 64), (512, 64), (513, 128)):
        assert _plan(_single_args("S", M, 160, 64, False)) == want
    for M, want in ((256, 0), (257, 64)):              # fp32 x AND h
        assert _plan(_single_args("L1", M, 160, 64, False)) == want
    # bf16 h / h_out_bf16 in either problem keep a pair away from the unpipelined pair kernel, which knows neither
    a, b = pair_args((("S", 200, 160, 64), ("L0b", 200, 64), 0, False, ""))
    b.M = 64
    assert _plan(a, b) < 0                               # (b alone is refused below 128 rows)
    a, b = pair_args((("S", 40, 160, 64), ("L0b", 200, 64), 0, False, ""))
    assert _plan(a, b) == R.TWO                          # a below 128 rows: no pipelined pair, and b's h_out_bf16 needs the pipelined body
