"""tests/bn_ref.py without a device: the float64 reference is torch's float64 batch norm; the fp32 emulation of csrc/bn.hip stays within
the bars of every table row; each planted defect leaves them on at least one row (so the device table of tests/test_gpu_bn.py can see
it); the share of elements at the ReLU's kink is capped; and the table keeps every launch-geometry class."""
import numpy as np
import pytest
import torch

import bn_ref as R

IDS = [R.row_id(r) for r in R.TABLE]


@pytest.mark.parametrize("row", [R.TABLE[0], R.TABLE[8], R.TABLE[15], R.TABLE[16], R.TABLE[21]], ids=R.row_id)
def test_reference_is_torch_float64_batch_norm(row):
    case = R.make_case(row)
    ref = R.run(R.reference, case)
    t = lambda a: torch.tensor(np.asarray(a, np.float64))
    x, gamma, beta = (t(case[k]).requires_grad_(True) for k in ("x", "gamma", "beta"))
    mm, mv = t(case["mm0"]), t(case["mv0"])
    y = torch.nn.functional.batch_norm(x, mm, mv, gamma, beta, training=True, momentum=R.f32(R.MOMENTUM), eps=R.f32(R.EPS))
    if case["relu"]:
        y = torch.relu(y)
    dx, dg, db = torch.autograd.grad((y * t(case["dy"])).sum(), (x, gamma, beta))
    xd = x.detach()
    got = {"y": y.detach(), "dx": dx, "dgamma": dg + t(case["dgamma0"]), "dbeta": db + t(case["dbeta0"]), "mean": xd.mean(0),
           "var": xd.var(0, unbiased=False), "rstd": 1.0 / torch.sqrt(xd.var(0, unbiased=False) + R.f32(R.EPS)), "mm": mm, "mv": mv}
    for k, v in got.items():
        scale = max(1.0, float(np.abs(ref[k]).max()))
        assert float(np.abs(v.numpy() - ref[k]).max()) <= 1e-12 * scale, k


def test_moving_rules():
    mean, var = np.array([0.5, -2.0]), np.array([4.0, 0.25])
    m = R.f32(0.01)
    a = R.moving(mean, var, 5, [0.25, 0.25], [3.0, 3.0])
    b = R.moving(mean, var, 5, [0.25, 0.25], [3.0, 3.0], bessel=False)
    assert np.allclose(a[0], b[0], rtol=0, atol=0) and np.allclose(a[0], (1 - m) * 0.25 + m * mean, rtol=0, atol=1e-15)
    assert np.allclose(a[1], (1 - m) * 3.0 + m * var * 1.25, rtol=0, atol=1e-15)
    assert np.allclose(b[1], (1 - m) * 3.0 + m * var, rtol=0, atol=1e-15)
    one = R.moving(mean, var, 1, [0.25, 0.25], [3.0, 3.0])
    assert np.array_equal(one[1], R.moving(mean, var, 1, [0.25, 0.25], [3.0, 3.0], bessel=False)[1])     # n = 1: var itself
    # the documented deviation from TF 1.13's rank-3 sites: momentum x var / (n - 1)
    assert abs(R.bessel_deviation(15312) - m / 15311.0) < 1e-15
    assert abs(R.bessel_deviation(15312) / (m * 1.0) - 6.5e-5) < 1e-6


@pytest.mark.parametrize("row", R.TABLE, ids=IDS)
def test_clean_emulation_within_the_bars(row):
    case, ref, gap, bar = R.table_case(row)
    frac, flips, nonzero = R.judge(R.table_case(row), R.run(R.emulate32, case))
    print("BN-EMULATED %s " % R.row_id(row) + " ".join("%s=%.3f" % (k, frac[k]) for k in R.OUTPUTS))
    assert set(frac) == set(R.OUTPUTS)
    assert all(np.isfinite(bar[k]) and bar[k] > 0 for k in R.OUTPUTS)
    assert max(frac.values()) <= 1.0, frac
    assert flips == 0 and nonzero == 0


def test_every_mutant_leaves_the_bars_on_some_row():
    caught = {}
    for m in R.MUTANTS:
        caught[m] = []
        for row in R.TABLE:
            case = R.table_case(row)[0]
            frac, flips, nonzero = R.judge(R.table_case(row), R.run(R.emulate32, case, mutant=m))
            worst = max(frac, key=lambda k: frac[k])
            if frac[worst] > 1.0 or flips or nonzero:
                caught[m].append((R.row_id(row), worst, frac[worst]))
        print("BN-MUTANT %s: %d rows: %s" % (m, len(caught[m]), ", ".join("%s (%s x%.3g)" % c for c in caught[m])))
    assert all(caught[m] for m in R.MUTANTS), [m for m in R.MUTANTS if not caught[m]]


@pytest.mark.parametrize("row", R.TABLE, ids=IDS)
def test_kink_share_is_capped(row):
    """a condition on the table's data, with the reference alone: at most 1e-3 of a row's elements lie within the y bar of the kink"""
    share = R.kink_share(row)
    print("BN-KINK %s share %.3g (y bar %.3g)" % (R.row_id(row), share, R.table_case(row)[3]["y"]))
    assert share <= 1e-3


def test_table_covers_the_launch_geometry():
    rows, cols = [r[0] for r in R.TABLE], [r[1] for r in R.TABLE]
    for name, hit in (("rows % 256 == 0", [r for r in rows if r % 256 == 0]), ("rows % 256 == 1", [r for r in rows if r > 256 and r % 256 == 1]),
                      ("rows % 256 == 255", [r for r in rows if r % 256 == 255]), ("rows < 16", [r for r in rows if r < 16]),
                      ("rows == 16", [r for r in rows if r == 16]), ("rows == 17", [r for r in rows if r == 17]),
                      ("C < 64", [c for c in cols if c < 64]), ("C == 64", [c for c in cols if c == 64]),
                      ("C % 64 != 0", [c for c in cols if c > 64 and c % 64]), ("C > 256", [c for c in cols if c > 256])):
        assert hit, name
    assert all(c % 4 == 0 for c in cols)
    assert set(r[2] for r in R.TABLE) == {0, 1} and set(r[3] for r in R.TABLE) == set(R.KINDS)
    for kind in R.KINDS:
        mine = [r for r in R.TABLE if r[3] == kind]
        assert any(r[0] % R.BLOCK for r in mine), kind                   # a ragged last row block
        assert any(r[1] % R.COLS for r in mine), kind                    # a ragged last column block
    for a, b in zip(R.TABLE, R.TABLE[1:]):
        assert sum(x != y for x, y in zip(a, b)) == 1, (a, b)            # neighbours differ in one field
    assert len(set(R.TABLE)) == len(R.TABLE)


def test_const_columns_are_exactly_zero_in_the_reference():
    row = next(r for r in R.TABLE if r[3] == "const")
    case, ref, _, _ = R.table_case(row)
    assert case["const_cols"].any() and not case["const_cols"].all()
    assert np.count_nonzero(ref["pre"][:, case["const_cols"]]) == 0
    assert np.abs(case["dy"][:, case["const_cols"]]).min() > 0
