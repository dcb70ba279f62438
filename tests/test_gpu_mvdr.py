"""las_mvdr_mask, las_mvdr_cov, las_mvdr_weights and las_mvdr_apply (csrc/mvdr.hip, include/las_hip.h K19) on the device against
the float64 numpy restatement tests/mvdr_ref.py, each call ALONE: its inputs come from the restatement, not from the previous kernel (cov
gets the reference m, weights the reference covariances, apply the reference w), so that no tolerance has to absorb the solve's
conditioning.  The shapes are the smallest at which each kernel can still go wrong.  m, energy, counts and valid must be equal element
for element; values are compared as |got - ref| <= TOL x max |ref| per call, and every test prints its largest difference before it asserts.
Every call is run twice and must give the same bits.  One chained test runs las.beamform's enhance on the 6 s recording of
tests/test_mvdr_host.py and holds the device's y to that file's bars."""
import functools
import types

import numpy as np
import pytest

import helpers  # noqa: F401
import beamform_ref as BR
import mvdr_ref as R

pytestmark = pytest.mark.gpu

# Largest |got - ref| / max |ref| over this file's inputs, measured on an MI355X, one per call: the covariances (fp32 products and tile
# sums against float64 sums), the weights (double against double), y (fp32 transforms against float64 ones).
# TOL = 16 x that, the margin of tests/test_gpu_beamform.py.  A covariance or a y over 1e-5, or weights over 1e-9, would be an
# algorithmic difference to be found, not a tolerance to be set.
# (cov: NF = 512, nine channels, fractional m; weights: NF = 1024, sixteen channels; y: NF = 1024, identity weights.)
MEASURED = {"cov": 3.167e-7, "weights": 2.968e-13, "y": 2.002e-7}
TOL = {k: 16 * v for k, v in MEASURED.items()}
GARBAGE = 7                                           # finite garbage samples behind n in every row
LOADING = 1e-3


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rows(x, n, ld, seed):
    rng = np.random.RandomState(seed)
    out = (rng.uniform(-0.9, 0.9, (x.shape[0], ld)) * (30000 if x.dtype == np.int16 else 1.0)).astype(x.dtype)
    out[:, :n] = x
    return out


def _nan(count, dtype="float64"):
    import torch
    return torch.full((count,), float("nan"), dtype=getattr(torch, dtype), device="cuda")


def _cplx(a):
    """interleaved (re, im) doubles -> complex128"""
    return a[..., 0] + 1j * a[..., 1]


def _pairs(z):
    z = np.asarray(z, np.complex128)
    return np.stack([z.real, z.imag], axis=-1)


def _ws(C, Tf, NF, Bf):
    import torch
    from las import _hip
    need = int(_hip.lib().las_mvdr_workspace_bytes(C, Tf, NF, Bf))
    assert need > 0
    return torch.empty(need, dtype=torch.uint8, device="cuda"), need


def _close(got, ref, what, kind):
    scale = float(np.abs(ref).max())
    err = float(np.abs(np.asarray(got) - ref).max())
    rel = err / scale if scale > 0 else err
    print("%s: max |got - ref| = %.3e = %.3e x max |ref| (TOL %.3e)" % (what, err, rel, TOL[kind]))
    assert np.isfinite(got).all(), what
    assert err <= TOL[kind] * scale, (what, err, scale)
    return rel


def launch_mask(rows, n, ref, NF, ratio, floor, hang, want_energy=True):
    import torch
    from las import _hip
    lib = _hip.lib()
    C, ld = rows.shape
    Tf = int(lib.las_mvdr_frames(n, NF))
    assert Tf == R.frames(n, NF)
    x = _dev(rows)
    ws, need = _ws(C, Tf, NF, 1)
    out = []
    for _ in range(2):
        m, e = _nan(Tf + 3, "float32"), _nan(Tf + 3)
        _hip.check(lib.las_mvdr_mask(_hip.p(x), int(rows.dtype == np.int16), ld, C, n, ref, NF, float(ratio), float(floor), hang, _hip.p(m),
                                     _hip.p(e) if want_energy else None, _hip.p(ws), need, _hip.stream()), "las_mvdr_mask")
        gm, ge = m.cpu().numpy(), e.cpu().numpy()
        assert np.isnan(gm[Tf:]).all() and np.isnan(ge[Tf:]).all()
        out.append((gm[:Tf], ge[:Tf]))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1], equal_nan=True)
    return out[0]


def launch_cov(rows, n, NF, Bf, m):
    from las import _hip
    lib = _hip.lib()
    C, ld = rows.shape
    Tf, K = R.frames(n, NF), NF // 2 + 1
    Nb = int(lib.las_mvdr_blocks(Tf, Bf))
    assert Nb == R.blocks(Tf, Bf)
    x, d_m, win, tw = _dev(rows), _dev(np.asarray(m, np.float32)), _dev(R.window(NF)), _dev(R.twiddle(NF))
    ws, need = _ws(C, Tf, NF, Bf)
    out = []
    for _ in range(2):
        cnt, pn, py = _nan(1 + Nb + 3), _nan(K * C * C * 2 + 4), _nan(Nb * K * C * C * 2 + 4)
        _hip.check(lib.las_mvdr_cov(_hip.p(x), int(rows.dtype == np.int16), ld, C, n, NF, Bf, _hip.p(d_m), _hip.p(win), _hip.p(tw), _hip.p(cnt),
                                    _hip.p(pn), _hip.p(py), _hip.p(ws), need, _hip.stream()), "las_mvdr_cov")
        c, a, b = cnt.cpu().numpy(), pn.cpu().numpy(), py.cpu().numpy()
        assert np.isnan(c[1 + Nb:]).all() and np.isnan(a[-4:]).all() and np.isnan(b[-4:]).all()
        out.append((c[:1 + Nb], _cplx(a[:-4].reshape(K, C, C, 2)), _cplx(b[:-4].reshape(Nb, K, C, C, 2))))
    assert all(np.array_equal(p, q) for p, q in zip(*out))
    return out[0]


def launch_weights(phi_n, phi_y, counts, ref, loading):
    import torch
    from las import _hip
    lib = _hip.lib()
    Nb, K, C, _ = phi_y.shape
    NF = 2 * (K - 1)
    pn, py, cnt = _dev(_pairs(phi_n)), _dev(_pairs(phi_y)), _dev(np.asarray(counts, np.float64))
    out = []
    for _ in range(2):
        w = _nan(Nb * K * C * 2 + 6)
        valid = torch.full((Nb * K + 3,), -7, dtype=torch.int32, device="cuda")
        _hip.check(lib.las_mvdr_weights(_hip.p(pn), _hip.p(py), _hip.p(cnt), C, NF, Nb, ref, float(loading), _hip.p(w), _hip.p(valid),
                                        _hip.stream()), "las_mvdr_weights")
        gw, gv = w.cpu().numpy(), valid.cpu().numpy()
        assert np.isnan(gw[-6:]).all() and (gv[-3:] == -7).all()
        out.append((_cplx(gw[:-6].reshape(Nb, K, C, 2)), gv[:-3].reshape(Nb, K)))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    return out[0]


def launch_apply(rows, n, NF, Bf, w):
    from las import _hip
    lib = _hip.lib()
    C, ld = rows.shape
    Tf = R.frames(n, NF)
    x, d_w, win, tw = _dev(rows), _dev(_pairs(w)), _dev(R.window(NF)), _dev(R.twiddle(NF))
    ws, need = _ws(C, Tf, NF, Bf)
    out = []
    for _ in range(2):
        y = _nan(n + 9, "float32")
        _hip.check(lib.las_mvdr_apply(_hip.p(x), int(rows.dtype == np.int16), ld, C, n, NF, Bf, _hip.p(d_w), _hip.p(win), _hip.p(tw), _hip.p(y),
                                      _hip.p(ws), need, _hip.stream()), "las_mvdr_apply")
        got = y.cpu().numpy()
        assert np.isnan(got[n:]).all()
        out.append(got[:n])
    assert np.array_equal(out[0], out[1])
    return out[0]


def signal(C, n, i16, seed, silent=None):
    """a coloured source heard by channel c with a delay of ((5 c) mod 7) - 3 samples, louder in the middle third, plus independent noise"""
    rng = np.random.RandomState(seed)
    s = BR.ar1(rng, n + 16, 0.7) * (0.3 + 1.0 * ((np.arange(n + 16) > n // 3) & (np.arange(n + 16) < 2 * n // 3)))
    x = np.stack([s[8 - (((5 * c) % 7) - 3):][:n] for c in range(C)]) * 0.1 + 0.03 * rng.randn(C, n)
    if silent is not None:
        x[silent] = 0.0
    return np.round(x * 8000).astype(np.int16) if i16 else x.astype(np.float32)


# ---- las_mvdr_mask ---------------------------------------------------------------------------------------------------------------------

MASK_CASES = [
    # NF, C, ref, n, int16, ratio, floor, hang
    (64, 2, 0, 1, False, 0.5, 0.0, 0),                # n = 1: two frames, both hold the one sample
    (64, 2, 1, 32, True, 0.5, 0.0, 1),                # n = Hs
    (64, 16, 15, 33, False, 0.9, 0.0, 0),             # n = Hs + 1: the third frame holds one sample; the last channel
    (64, 3, 0, 1301, True, 0.4, 0.0, 2),              # n no multiple of Hs; the dilation
    (1024, 2, 1, 20000, False, 0.4, 0.0, 3),
    (1024, 4, 3, 5000, True, 0.001, 0.3, 0),          # the floor is the threshold
    (64, 2, 0, 2000, False, 0.5, 0.0, 100),           # a dilation longer than the recording: all speech
]


@pytest.mark.parametrize("i", range(len(MASK_CASES)))
def test_mask(i):
    NF, C, ref, n, i16, ratio, floor, hang = MASK_CASES[i]
    x = signal(C, n, i16, seed=i)
    m_ref, e_ref = R.mask(x, ref, NF, ratio, floor, hang)
    m, e = launch_mask(_rows(x, n, n + GARBAGE + i % 3, seed=100 + i), n, ref, NF, ratio, floor, hang)
    print("mask %r: %d of %d frames speech" % (MASK_CASES[i], int(m.sum()), len(m)))
    assert np.array_equal(e, e_ref) and np.array_equal(m, m_ref)
    if i == 5:
        assert e_ref.max() * ratio < floor and 0 < m.sum() < len(m)
    if i in (3, 4):
        assert 0 < m.sum() < len(m)
    m2, e2 = launch_mask(_rows(x, n, n + GARBAGE, seed=300 + i), n, ref, NF, ratio, floor, hang, want_energy=False)
    assert np.array_equal(m2, m_ref) and np.isnan(e2).all()           # energy = NULL: nothing is written there


def test_mask_of_a_silent_reference_is_all_noise():
    x = signal(3, 700, False, seed=9, silent=1)
    m, e = launch_mask(_rows(x, 700, 710, seed=1), 700, 1, 64, 0.5, 0.0, 2)
    assert not m.any() and not e.any()


# ---- las_mvdr_cov ----------------------------------------------------------------------------------------------------------------------

COV_CASES = [
    # NF, C, n, Bf, int16, m (0, 1, "frac", "rule"), silent channel
    (64, 2, 1, 1, False, "frac", None),               # n = 1; Bf = 1
    (64, 2, 32, 5, True, 1, None),                    # n = Hs; Bf >= Tf; all speech: N0 = 0
    (64, 3, 33, 2, False, 0, None),                   # n = Hs + 1; Tf = 3 no multiple of Bf; all noise: every M_b = 0; C = 3 in four rows
    (64, 16, 1301, 25, True, "frac", 3),              # sixteen channels, one silent; tiles of 8 frames, the last one short
    (64, 5, 1301, 1, False, "rule", None),            # Bf = 1: a block per frame
    (512, 9, 3000, 7, False, "frac", None),           # nine channels in sixteen rows: three bin slices
    (1024, 16, 2500, 4, True, "rule", None),          # the largest frame and array: five bin slices
    (1024, 8, 6000, 100, False, "frac", 0),           # two bin slices; Bf >= Tf
    (64, 4, 40000, 1000, True, "rule", None),         # tiles of 256 frames: the longest fp32 sums
]


@functools.lru_cache(maxsize=None)
def cov_case(i):
    NF, C, n, Bf, i16, kind, silent = COV_CASES[i]
    x = signal(C, n, i16, seed=20 + i, silent=silent)
    Tf = R.frames(n, NF)
    if kind == "frac":
        m = np.random.RandomState(i).uniform(0, 1, Tf).astype(np.float32)
        m[::5] = 0.0
        m[1::7] = 1.0
    elif kind == "rule":
        m = R.mask(x, C - 1, NF, 0.4, 0.0, 1)[0]
    else:
        m = np.full(Tf, float(kind), np.float32)
    return x, m, R.cov(x, m, NF, Bf)


@pytest.mark.parametrize("i", range(len(COV_CASES)))
def test_cov(i):
    NF, C, n, Bf, i16, kind, silent = COV_CASES[i]
    x, m, (cnt_ref, pn_ref, py_ref) = cov_case(i)
    cnt, pn, py = launch_cov(_rows(x, n, n + GARBAGE + i % 3, seed=400 + i), n, NF, Bf, m)
    assert np.array_equal(cnt, cnt_ref), COV_CASES[i]
    assert np.isfinite(pn).all() and np.isfinite(py).all()
    rel = lambda got, ref: np.abs(got - ref).max() / np.abs(ref).max() if ref.any() else np.abs(got).max()
    worst = max([rel(pn, pn_ref)] + [rel(py[b], py_ref[b]) for b in range(len(cnt) - 1)])       # (a block against that block's own scale)
    print("cov %r: max |got - ref| = %.3e x max |ref| of phi_n or of a block of phi_y (TOL %.3e)" % (COV_CASES[i], worst, TOL["cov"]))
    assert worst <= TOL["cov"], COV_CASES[i]
    for P in (pn, py):                                # Hermitian as stored
        assert np.array_equal(P, np.conj(np.swapaxes(P, -1, -2))) and not np.diagonal(P, axis1=-2, axis2=-1).imag.any()
    if kind == 1:
        assert cnt[0] == 0 and not pn.any()
    if kind == 0:
        assert not cnt[1:].any() and not py.any() and pn.any()
    if silent is not None:
        assert not pn[:, silent].any() and not pn[:, :, silent].any() and not py[:, :, silent].any() and not py[:, :, :, silent].any()


# ---- las_mvdr_weights ------------------------------------------------------------------------------------------------------------------

def _spd(C, rng, scale=1.0):
    A = rng.randn(C, 2 * C) + 1j * rng.randn(C, 2 * C)
    return scale * (A @ A.conj().T) / (2 * C)


@functools.lru_cache(maxsize=None)
def weights_case(i):
    """-> (phi_n, phi_y, counts, ref, w, valid, g)"""
    rng = np.random.RandomState(60 + i)
    if i < 4:                                         # covariances of a recording, from the restatement
        NF, C, n, Bf, ref = [(64, 2, 1301, 7, 0), (64, 16, 1301, 9, 15), (1024, 16, 6000, 3, 0), (64, 3, 9000, 1, 2)][i]
        x = signal(C, n, i == 1, seed=40 + i)
        m = R.mask(x, ref, NF, 0.4, 0.0, 1)[0]
        if i == 0:
            m[:] = 1.0
            m[:4] = m[14:21] = 0.0                    # block 2 without speech, between two with speech
        cnt, phi_n, phi_y = R.cov(x, m, NF, Bf)
    else:                                             # built: a silent reference, a zero noise bin, blocks without speech, N0 = 0
        C, K, Nb, ref = [(4, 33, 6, 3), (2, 513, 3, 1), (16, 33, 4, 0)][i - 4]
        sn = 10.0 ** rng.uniform(-6, 0, K)            # the bins' levels; the speech part 0.01 to 10 times the noise: g well over the bar
        phi_n = np.stack([_spd(C, rng, sn[k]) for k in range(K)])
        phi_y = np.stack([np.stack([phi_n[k] + _spd(C, rng, sn[k] * 10.0 ** rng.uniform(-2, 1)) for k in range(K)]) for _ in range(Nb)])
        cnt = np.concatenate([[50.0], rng.randint(1, 9, Nb).astype(np.float64)])
        if i == 4:
            cnt[[1, 3, 4]] = 0.0                      # the first block and two in the middle hold no speech
            phi_y[[0, 2, 3]] = 0.0
            phi_n[5] = 0.0                            # a bin without noise
            phi_n[7][:, ref] = phi_n[7][ref, :] = 0.0     # a silent reference channel in one bin
            phi_y[:, 7][:, :, ref] = 0.0
            phi_y[:, 7][:, ref, :] = 0.0
        if i == 6:
            cnt[0] = 0.0                              # no noise frame at all
            phi_n[:] = 0.0
    w, valid, g = R.weights(phi_n, phi_y, cnt, ref, LOADING, return_g=True)
    return phi_n, phi_y, cnt, ref, w, valid, g


@pytest.mark.parametrize("i", range(7))
def test_weights(i):
    phi_n, phi_y, cnt, ref, w_ref, valid_ref, g = weights_case(i)
    ok = np.isfinite(g)
    assert ((g[ok] >= 1e-5) | (g[ok] <= 1e-7)).all()                  # every g a factor 10 away from the bar of 1e-6
    w, valid = launch_weights(phi_n, phi_y, cnt, ref, LOADING)
    print("weights case %d: %d of %d (block, bin) valid" % (i, int(valid.sum()), valid.size))
    assert np.array_equal(valid, valid_ref)
    _close(w, w_ref, "weights case %d" % i, "weights")
    if i == 0:
        assert valid[1].any() and not valid[2].any() and valid[3].any() and np.array_equal(w[2], w[1])
    if i == 4:
        assert not valid[0].any() and not valid[:, 5].any() and (w[:, 5, ref] == 1).all() and np.abs(w[:, 5]).sum() == w.shape[0]
        assert np.array_equal(w[0], w[1]) and np.array_equal(w[3], w[1]) and np.array_equal(w[2], w[1])
    if i == 6:
        assert not valid.any() and np.array_equal(w, R.identity_weights(*w.shape, ref))


# ---- las_mvdr_apply --------------------------------------------------------------------------------------------------------------------

APPLY_CASES = [
    # NF, C, n, Bf, int16, ref of the identity run
    (64, 2, 1, 1, False, 0),
    (64, 2, 32, 3, True, 1),                          # n = Hs; Bf >= Tf
    (64, 16, 33, 2, False, 15),                       # n = Hs + 1; Tf = 3 no multiple of Bf
    (64, 3, 1301, 5, True, 2),                        # three workgroups, the last one short; the block changes inside a workgroup
    (512, 9, 9000, 1, False, 0),                      # a block per frame
    (1024, 16, 9000, 7, True, 15),                    # the largest LDS footprint
    (1024, 2, 20001, 1000, False, 1),
]


@functools.lru_cache(maxsize=None)
def apply_case(i):
    NF, C, n, Bf, i16, ref = APPLY_CASES[i]
    x = signal(C, n, i16, seed=70 + i, silent=1 if i == 3 else None)
    Nb, K = R.blocks(R.frames(n, NF), Bf), NF // 2 + 1
    rng = np.random.RandomState(i)
    w = (rng.randn(Nb, K, C) + 1j * rng.randn(Nb, K, C)) / C
    if n == 1:                                        # one output sample IS max |ref|: random weights can cancel it to any fraction of the
        w[:] = (0.8 - 0.3j) / C                       # samples it is made of (here 1e-3), and the fp32 error goes with those, not with it
    return x, w, R.apply(x, w, NF, Bf)


@pytest.mark.parametrize("i", range(len(APPLY_CASES)))
def test_apply(i):
    NF, C, n, Bf, i16, ref = APPLY_CASES[i]
    x, w, y_ref = apply_case(i)
    rows = _rows(x, n, n + GARBAGE + i % 3, seed=500 + i)
    y = launch_apply(rows, n, NF, Bf, w)
    _close(y, y_ref, "apply %r" % (APPLY_CASES[i],), "y")
    back = launch_apply(rows, n, NF, Bf, R.identity_weights(w.shape[0], w.shape[1], C, ref))
    _close(back, R.widen(x)[ref], "apply %r, identity weights" % (APPLY_CASES[i],), "y")


# ---- refusals --------------------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing():
    import torch
    from las import _hip
    lib = _hip.lib()
    n, NF, C, Bf = 700, 64, 2, 5
    Tf, K = R.frames(n, NF), NF // 2 + 1
    Nb = R.blocks(Tf, Bf)
    x, win, tw = _dev(np.zeros((C, n), np.float32)), _dev(R.window(NF)), _dev(R.twiddle(NF))
    ws, need = _ws(C, Tf, NF, Bf)
    m, e, y = _nan(Tf, "float32"), _nan(Tf), _nan(n, "float32")
    cnt, pn, py, w = _nan(1 + Nb), _nan(K * C * C * 2), _nan(Nb * K * C * C * 2), _nan(Nb * K * C * 2)
    valid = torch.full((Nb * K,), -7, dtype=torch.int32, device="cuda")
    st, P = _hip.stream(), _hip.p
    ok = dict(ld=n, C=C, n=n, ref=0, NF=NF, ratio=0.5, floor=0.0, hang=1, Bf=Bf, ws=need, Nb=Nb, loading=1e-3)
    for bad in (dict(C=1), dict(C=17), dict(NF=32), dict(NF=2048), dict(NF=96), dict(n=0), dict(n=n + 1), dict(ref=2), dict(ref=-1), dict(ratio=0.0),
                dict(ratio=1.5), dict(ratio=float("nan")), dict(floor=-1.0), dict(floor=float("inf")), dict(hang=-1), dict(ws=16)):
        k = dict(ok, **bad)
        assert lib.las_mvdr_mask(P(x), 0, k["ld"], k["C"], k["n"], k["ref"], k["NF"], k["ratio"], k["floor"], k["hang"], P(m), P(e), P(ws), k["ws"],
                                 st) < 0 and lib.las_last_error(), bad
    for bad in (dict(C=1), dict(C=17), dict(NF=32), dict(NF=2048), dict(n=0), dict(n=n + 1), dict(Bf=0), dict(ws=need - 1)):
        k = dict(ok, **bad)
        assert lib.las_mvdr_cov(P(x), 0, k["ld"], k["C"], k["n"], k["NF"], k["Bf"], P(m), P(win), P(tw), P(cnt), P(pn), P(py), P(ws), k["ws"], st) < 0, bad
        assert lib.las_mvdr_apply(P(x), 0, k["ld"], k["C"], k["n"], k["NF"], k["Bf"], P(w), P(win), P(tw), P(y), P(ws),
                                  16 if "ws" in bad else k["ws"], st) < 0 and lib.las_last_error(), bad
    for bad in (dict(C=1), dict(C=17), dict(NF=32), dict(Nb=0), dict(ref=2), dict(loading=0.0), dict(loading=float("nan")), dict(loading=float("inf"))):
        k = dict(ok, **bad)
        assert lib.las_mvdr_weights(P(pn), P(py), P(cnt), k["C"], k["NF"], k["Nb"], k["ref"], k["loading"], P(w), P(valid), st) < 0, bad
    assert lib.las_mvdr_cov(P(x), 0, n, C, n, NF, Bf, None, P(win), P(tw), P(cnt), P(pn), P(py), P(ws), need, st) < 0
    torch.cuda.synchronize()
    for t in (m, e, y, cnt, pn, py, w):
        assert np.isnan(t.cpu().numpy()).all()
    assert (valid.cpu().numpy() == -7).all()
    assert lib.las_mvdr_frames(0, 64) < 0 and lib.las_mvdr_frames(10, 48) < 0 and lib.las_mvdr_frames(10, 2048) < 0
    assert lib.las_mvdr_blocks(0, 1) < 0 and lib.las_mvdr_blocks(5, 0) < 0 and lib.las_mvdr_workspace_bytes(1, 10, 64, 1) == 0
    assert [lib.las_mvdr_frames(v, 64) for v in (1, 32, 33)] == [2, 2, 3]


# ---- the four chained ------------------------------------------------------------------------------------------------------------------

def test_enhance_on_the_recording_reaches_the_host_bars():
    from las import beamform as BF
    x, clean, voice = R.recording()
    n = x.shape[1]
    args = types.SimpleNamespace(bf_method="mvdr", bf_ref=0, mvdr_top_db=2.2)
    y, info = BF.Beamformer(args, device="cuda").enhance(x.T, 16000)
    assert y.dtype == np.float32 and y.shape == (n,)
    assert (info["NF"], info["Bf"], info["hang"], info["Tf"], info["Nb"]) == (512, 125, 6, R.frames(n, 512), 4)
    m, counts, valid = BF.Beamformer.statistics(info)
    m_ref, _ = R.mask(x, 0, 512, 10.0 ** -0.22, 512 * 1e-7, 6)
    assert np.array_equal(m, m_ref) and np.array_equal(counts, R.counts_of(m_ref, 125))
    assert valid.shape == (4, 257) and valid[:3].mean() > 0.9 and not valid[3].any()     # the last block holds no speech
    on = R.inside(voice, 0, 512)
    snr_ds, snr = BR.snr_db(R.delay_sum_true(x, R.VOICE_DELAYS), clean, on), BR.snr_db(y, clean, on)
    corr = np.corrcoef(y[on], clean[on])[0, 1]
    y_ref = R.enhance(x, 0, 512, 125, 10.0 ** -0.22, 512 * 1e-7, 6, 1e-3)[0]
    print("enhance: delay-and-sum %.2f dB, MVDR on the device %.2f dB, correlation %.4f; max |y - restatement| = %.3e of %.3e"
          % (snr_ds, snr, corr, np.abs(y - y_ref).max(), np.abs(y_ref).max()))
    assert snr >= snr_ds + 6.0 and corr >= 0.95
    q = np.round(np.clip(x, -1, 1) * 32767).astype(np.int16)          # the int16 rows of a 16-bit file, and another reference channel
    y3, info3 = BF.Beamformer(types.SimpleNamespace(bf_method="mvdr", bf_ref=3, mvdr_top_db=2.2), device="cuda").enhance(q.T, 16000)
    clean3 = R.delayed(clean, R.VOICE_DELAYS[3])
    assert np.corrcoef(y3[on], clean3[on])[0, 1] >= 0.95
    with pytest.raises(ValueError, match="bf_ref 5"):
        BF.Beamformer(types.SimpleNamespace(bf_method="mvdr", bf_ref=5), device="cuda").enhance(x.T, 16000)
