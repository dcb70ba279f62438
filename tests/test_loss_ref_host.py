"""tests/loss_ref.py on the CPU: the float64 references of the loss and dropout kernels against torch and against published values,
the closed forms against the dynamic programme, the emulations inside sane distance of the references, and the recorded bounds
re-derived."""
import numpy as np
import pytest
import torch

import loss_ref as R


# ------------------------------------------------------------------------------------------------ cross-entropy
@pytest.mark.parametrize("V", [1, 2, 30, 65, 1025])
@pytest.mark.parametrize("bits", [0, 1, 2, 3])
def test_ce_ref_matches_torch_log_softmax(V, bits):
    rng = np.random.RandomState(V * 4 + bits)
    B, U = 3, 5
    logits = (rng.randn(B, U, V) * 2.0).astype(np.float32)
    y = rng.randint(0, V, size=(B, U))
    y[0, 0], y[1, 1] = V - 1, 0
    eps, scale = 0.01, 0.37
    ce, mask, sums, grad = R.ce_ref(logits, y, V, eps, bits, scale)
    x = torch.tensor(logits, dtype=torch.float64, requires_grad=True)
    logp = torch.log_softmax(x, -1)
    e = eps if bits & 1 else 0.0
    soft = (1 - e) * torch.nn.functional.one_hot(torch.tensor(y), V).double() + e / V
    m = torch.ones(B, U, dtype=torch.float64) if bits & 2 else torch.tensor(y != 0, dtype=torch.float64)
    ce_t = -(soft * logp).sum(-1) * m
    (ce_t.sum() * scale).backward()
    assert np.abs(ce - ce_t.detach().numpy()).max() < 1e-12 and (mask == m.numpy()).all()
    assert np.abs(grad - x.grad.numpy()).max() < 1e-14
    tot = float(ce_t.detach().sum())
    assert abs(sums[0] - tot) < 1e-11 and sums[1] == float(m.sum()) and abs(sums[2] - scale * tot) < 1e-11


def test_ce_ref_label_out_of_range_has_no_one_hot_term():
    rng = np.random.RandomState(3)
    V = 7
    logits = rng.randn(4, V)
    ce, mask, _, grad = R.ce_ref(logits, np.array([V, V + 7, -1, 2]), V, 0.01, 1, 1.0)
    lp = np.log(np.exp(logits) / np.exp(logits).sum(-1, keepdims=True))
    assert (mask == 1).all()                                              # (a label that is not 0 counts)
    for r in range(3):
        assert abs(ce[r] - (logits[r].max() + np.log(np.exp(logits[r] - logits[r].max()).sum()) - 0.01 / V * logits[r].sum())) < 1e-12
        assert np.abs(grad[r] - (np.exp(lp[r]) - 0.01 / V)).max() < 1e-14
    assert abs(grad[3].sum()) < 1e-14 and abs(grad[:3].sum(-1) - 0.99).max() < 1e-12


@pytest.mark.parametrize("kind", R.CE_KINDS)
def test_ce_emulation_is_fp32_close_and_the_recorded_bound_is_its_four_fold(kind):
    c = R.ce_case(kind, 0)
    a = (c["logits"], c["y"], c["V"], c["eps"], c["smooth"], c["scale"])
    ce_e, mask_e, sums_e, grad_e = R.ce_emulate(*a)
    ce, mask, sums, grad = R.ce_ref(*a)
    assert (mask_e == mask).all() and sums_e[1] == sums[1]
    assert np.abs(ce_e - ce).max() <= 64 * np.finfo(np.float32).eps * max(1.0, np.abs(ce).max())
    got = R.ce_bound(kind)
    for g, rec in zip(got, R.CE_BOUNDS[kind]):                            # (a host with other fp32 exp / log bits may differ a little)
        assert 0.5 * rec <= g <= 2.0 * rec, (kind, got, R.CE_BOUNDS[kind])


def test_ce_bounds_cover_every_kind():
    assert set(R.CE_BOUNDS) == set(R.CE_KINDS) and set(R.CTC_BOUNDS) == set(R.CTC_KINDS)


# ------------------------------------------------------------------------------------------------ CTC
def test_ctc_blank_only_closed_form_matches_torch():
    rng = np.random.RandomState(5)
    logits = (rng.randn(9, 6) * 2.0).astype(np.float32)
    for T in (1, 4, 9):
        nll, grad = R.ctc_blank_only(logits, T)
        nll_r, grad_r = R.ctc_ref(logits[None], [[]], [T])
        assert abs(nll - nll_r[0]) < 1e-12 and np.abs(grad - grad_r[0]).max() < 1e-12 and (grad[T:] == 0).all()


@pytest.mark.parametrize("k", [1, 2, 6])
def test_ctc_single_path_closed_form_matches_torch(k):
    rng = np.random.RandomState(k)
    T = 2 * k - 1
    logits = (rng.randn(T + 2, 31) * 2.0).astype(np.float32)
    nll, grad = R.ctc_single_path(logits, 7, k)
    nll_r, grad_r = R.ctc_ref(logits[None], [[7] * k], [T])
    assert abs(nll - nll_r[0]) < 1e-12 and np.abs(grad - grad_r[0]).max() < 1e-12
    if k > 1:                                                             # one frame fewer: no alignment
        assert R.ctc_ref(logits[None], [[7] * k], [T - 1])[0][0] == np.inf
        assert R.ctc_emulate(logits, [7] * k, T - 1)[0] == np.inf


@pytest.mark.parametrize("case", [([], 5), ([3], 1), ([3, 3, 4, 4, 4, 9], 14), ([1, 2] * 20, 70)])
def test_ctc_emulation_is_close_to_the_reference(case):
    lab, T = case
    rng = np.random.RandomState(T)
    logits = (rng.randn(T + 3, 31) * 2.0).astype(np.float32)
    nll, grad = R.ctc_emulate(logits, lab, T)
    nll_r, grad_r = R.ctc_ref(logits[None], [lab], [T])
    assert abs(nll - nll_r[0]) <= 1e-5 * max(1.0, abs(nll_r[0])) and np.abs(grad - grad_r[0]).max() < 1e-5
    assert (grad[T:] == 0).all()


@pytest.mark.parametrize("kind", [k for k in R.CTC_KINDS if k != "max-L511-T540"])
def test_ctc_recorded_bound_is_rederived(kind):
    got = R.ctc_bound(kind)
    for g, rec in zip(got, R.CTC_BOUNDS[kind]):
        assert 0.5 * rec <= g <= 2.0 * rec, (kind, got, R.CTC_BOUNDS[kind])


def test_ctc_recorded_bound_at_the_maximum_is_rederived_on_four_seeds():
    """(the full 20 seeds take six seconds; four of them already show that 4 x the emulation's error stays below the 1e-5 floor)"""
    assert R.ctc_bound("max-L511-T540", seeds=4) == R.CTC_BOUNDS["max-L511-T540"] == (1e-5, 1e-5)


def test_no_adjacent_repeats_generator():
    lab = R.no_adjacent_repeats(np.random.RandomState(0), 511, 1, 30)
    assert len(lab) == 511 and all(a != b for a, b in zip(lab, lab[1:])) and min(lab) >= 1 and max(lab) <= 29


# ------------------------------------------------------------------------------------------------ dropout
def test_splitmix64_published_sequence_for_state_zero():
    """the first three outputs of splitmix64 seeded with 0: seed 0 quad 0 dir 0, quad 0 dir 1, quad 1 dir 0"""
    want = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    got = [int(R.drop_bits(0, 0, 0)), int(R.drop_bits(0, 1, 0)), int(R.drop_bits(0, 0, 1))]
    assert got == want
    state = np.uint64(0)
    for w in want:                                                        # ... and as the generator is published: state += golden, mix
        with np.errstate(over="ignore"):
            state = np.uint64(state + R.GOLDEN)
        assert int(R.splitmix64_mix(state)) == w


def test_drop_thresholds():
    assert [R.drop_threshold(k) for k in (0.5, 0.9, 1.0, 0.1)] == [32768, 58982, 65536, 6554]


def test_masks_layout_quads_and_slices():
    seed, rows, K = (1 << 61) + 5, 3, 10                                  # ceil(K / 4) = 3 quads per row, the last half used
    mf, mb = R.dropout_masks(seed, rows, K, 0.5)
    assert mf.shape == mb.shape == (rows, K) and mf.dtype == bool
    for r in range(rows):
        for c in range(K):
            for d, m in ((0, mf), (1, mb)):
                z = (seed + 0x9E3779B97F4A7C15 * (2 * (r * 3 + c // 4) + d + 1)) & (2 ** 64 - 1)      # python integers
                z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
                z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
                z ^= z >> 31
                assert bool(m[r, c]) == (((z >> (16 * (c % 4))) & 0xffff) < 32768), (r, c, d)
    assert R.dropout_masks(seed, rows, K, 1.0)[0].all() and R.dropout_masks(seed, rows, K, 1.0)[1].all()


@pytest.mark.parametrize("K", [39, 512, 100, 128])
@pytest.mark.parametrize("keep", [0.5, 0.9])
def test_reference_masks_alone_stay_inside_the_five_sigma_band(K, keep):
    """the band tests/test_gpu_dropout.py holds the kernels to, on the reference's own masks at that test's sizes"""
    mf, mb = R.dropout_masks(12345, 7 * 301, K, keep)
    n = mf.size
    for m in (mf, mb):
        assert abs(m.mean() - keep) < 5 * np.sqrt(keep * (1 - keep) / n) + 2e-5
    assert abs((mf & mb).mean() - keep * keep) < 5 * np.sqrt(0.25 / n) + 1e-4
    assert not (mf == mb).all()
