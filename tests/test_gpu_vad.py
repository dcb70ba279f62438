"""las_vad (include/las_hip.h K15, csrc/vad.hip) against the numpy restatement tests/vad_ref.py.  The contract fixes the arithmetic (one
double rounding per sample, in sample order; one double multiply for the threshold) and everything behind the energies is integer
work, so the energy bits, emax, n_runs and the runs are compared for EQUALITY: that is the bound the contract derives, not a measured
one."""
import ctypes

import numpy as np
import pytest
import torch

import helpers  # noqa: F401
import vad_ref as R

pytestmark = pytest.mark.gpu
SENTINEL = -77
GEOMETRIES = [(400, 160), (200, 80)]


def _launch(rows, fl, step, ratio, floor, hang, min_run, want_energy=True, want_emax=True, extra_T=0):
    """rows: list of 1-D arrays, all float32 or all int16 -> (energy [n, Tmax] or None, emax [n] or None, runs [n, max_runs, 2] with
    SENTINEL where nothing was written, n_runs [n]); energy and emax start as NaN"""
    from las import _hip
    lib = _hip.lib()
    i16 = rows[0].dtype == np.int16
    assert all(r.dtype == (np.int16 if i16 else np.float32) for r in rows)
    n, ns = len(rows), [len(r) for r in rows]
    ld = max(ns) + 3                                                      # (no multiple of anything: rows start on any 4-byte boundary)
    host = np.full((n, ld), 12345 if i16 else 9.0, rows[0].dtype)         # loud padding: samples behind n_u must not be read
    for u, r in enumerate(rows):
        host[u, :ns[u]] = r
    Tmax = max(1, max(R.frame_count(x, fl, step) for x in ns)) + extra_T
    max_runs = int(lib.las_vad_max_runs(Tmax, hang))
    d_rows = torch.from_numpy(host).cuda()
    d_ns = torch.tensor(ns, dtype=torch.int32, device="cuda")
    energy = torch.full((n, Tmax), float("nan"), dtype=torch.float64, device="cuda") if want_energy else None
    emax = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda") if want_emax else None
    runs = torch.full((n, max_runs, 2), SENTINEL, dtype=torch.int32, device="cuda")
    n_runs = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
    nbytes = int(lib.las_vad_workspace_bytes(n, Tmax))
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    rc = lib.las_vad(_hip.p(d_rows), int(i16), ld, _hip.p(d_ns), (ctypes.c_int * n)(*ns), n, Tmax, fl, step, ratio, floor, hang, min_run,
                     _hip.p(energy), _hip.p(emax), _hip.p(runs), max_runs, _hip.p(n_runs), _hip.p(ws), nbytes, _hip.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.las_last_error()
    return (None if energy is None else energy.cpu().numpy(), None if emax is None else emax.cpu().numpy(), runs.cpu().numpy(),
            n_runs.cpu().numpy())


def _check(rows, fl, step, ratio, floor, hang, min_run, out):
    """-> the reference's runs per row"""
    energy, emax, runs, n_runs = out
    want = []
    for u, x in enumerate(rows):
        e, m, rr = R.vad(x, fl, step, ratio, floor, hang, min_run)
        T = len(e)
        if energy is not None:
            assert np.array_equal(energy[u, :T].view(np.int64), e.view(np.int64)), (u, np.flatnonzero(energy[u, :T] != e)[:5])    # equal bits
            assert (energy[u, T:].view(np.int64) == 0).all()              # +0.0 behind T_u
        if emax is not None:
            assert emax[u] == m, (u, emax[u], m)
        assert n_runs[u] == len(rr), (u, n_runs[u], rr, runs[u, :max(n_runs[u], 0)].tolist())
        assert runs[u, :len(rr)].tolist() == [list(r) for r in rr], (u, runs[u, :len(rr)].tolist(), rr)
        assert (runs[u, len(rr):] == SENTINEL).all()                      # entries behind the count are not written
        assert len(rr) <= R.max_runs(T, hang)
        want.append(rr)
    return want


def _noise_with_bursts(rng, T, fl, step, i16, extra=0):
    """T frames of a quiet floor with loud bursts at random places (float32 or int16)"""
    n = T * step + fl + extra
    x = 1e-3 * rng.randn(n)
    pos = 0
    while pos < n:                                                        # bursts of 1..12 steps, gaps of 1..30 steps
        pos += rng.randint(1, 30 * step)
        w = rng.randint(1, 12 * step)
        x[pos:pos + w] += 0.2 * rng.randn(len(x[pos:pos + w]))
        pos += w
    if i16:
        return np.clip(np.round(x * 32767), -32768, 32767).astype(np.int16)
    return x.astype(np.float32)


def _impulses(T, fl, step, first_frames, width=3):
    """zeros with single loud samples: an impulse at sample step k + fl - 1 lies in the frames k .. k + width - 1 exactly (fl = 400,
    step = 160: width = 3).  -> a waveform of T frames whose raw frames are the union of [k, k + width) over first_frames"""
    x = np.zeros(T * step + fl, np.float32)
    for k in first_frames:
        assert 0 <= k and k + width <= T
        x[step * k + fl - 1] = 0.5
    return x


def _raw_frames(x, fl, step, ratio, floor):
    e = R.energies(x, fl, step)
    return np.flatnonzero(R.flags(e, ratio, floor, 0)[1]).tolist()


# ---- the issue's shapes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i16", [False, True], ids=["fp32", "int16"])
@pytest.mark.parametrize("fl,step", GEOMETRIES)
def test_tile_edges(fl, step, i16):
    from las import _hip
    tile = _hip.lib().las_vad_tile()
    rng = np.random.RandomState(fl + i16)
    rows = [_noise_with_bursts(rng, T, fl, step, i16, extra=k * 7) for k, T in enumerate((tile - 1, tile, tile + 1, 2 * tile + 3))]
    args = (fl, step, 1e-2, fl * 1e-7, 3, 4)
    want = _check(rows, *args, _launch(rows, *args))
    assert sum(len(r) for r in want) >= 4                                 # the signal does hold runs
    # a row alone gives what it gives inside the batch (bits), and two calls give the same bits
    batch = _launch(rows, *args)
    for u, x in enumerate(rows):
        alone = _launch([x], *args)
        T = R.frame_count(len(x), fl, step)
        assert np.array_equal(alone[0][0, :T].view(np.int64), batch[0][u, :T].view(np.int64)) and alone[1][0] == batch[1][u]
        assert alone[3][0] == batch[3][u] and np.array_equal(alone[2][0, :alone[3][0]], batch[2][u, :batch[3][u]])
    again = _launch(rows, *args)
    for a, b in zip(batch, again):
        assert np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if b.dtype == np.float64 else b)


@pytest.mark.parametrize("fl,step", GEOMETRIES)
def test_no_frame_one_frame_silence_and_all_speech(fl, step):
    rng = np.random.RandomState(1)
    loud = (0.1 * rng.randn(150 * step + fl)).astype(np.float32)
    rows = [loud[:fl - 1], loud[:fl + step], np.zeros(90 * step + fl, np.float32), loud, loud[:fl + 2 * step]]      # T = 0, 1, 90, 150, 2
    args = (fl, step, 1e-4, fl * 1e-7, 5, 2)
    want = _check(rows, *args, _launch(rows, *args, extra_T=9))           # (Tmax past the longest row: zeros behind every T_u)
    assert want == [[], [], [], [(0, 150)], [(0, 2)]]                     # one frame is under min_run = 2; two frames are a run
    # the floor alone silences a quiet recording; ratio = 1 keeps the loudest frame only
    quiet = (1e-5 * rng.randn(90 * step + fl)).astype(np.float32)
    assert _check([quiet, loud], *args, _launch([quiet, loud], *args)) == [[], [(0, 150)]]
    args = (fl, step, 1.0, 0.0, 1, 2)
    want = _check([loud], *args, _launch([loud], *args))
    t = int(np.argmax(R.energies(loud, fl, step)))
    assert want == [[(t - 1, t + 2)]]


@pytest.mark.parametrize("hang", [0, 2, 5])
def test_designed_runs(hang):
    """runs at frame 0 and at frame T - 1, over a tile boundary, gaps of 2 hang (joined) and 2 hang + 1 (kept), runs of min_run - 1
    (dropped) and min_run (kept) -- the restatement's runs are asserted to be the designed ones, so each case is really there"""
    from las import _hip
    tile = _hip.lib().las_vad_tile()
    fl, step, T = 400, 160, 3 * tile + 10
    G = 2 * hang
    a1 = 20
    a2 = a1 + 3 + G                                                       # raw 20..22 and a2..a2+2: a gap of exactly 2 hang frames -> joined
    a3 = a2 + 3 + G + 1                                                   # a gap of 2 hang + 1 -> a run of its own
    b = tile - 2                                                          # raw tile-2 .. tile: straddles the boundary (needs a3 + 3 + G < b - hang)
    c = 2 * tile - hang - 1 if hang else 2 * tile - 1                     # its dilation crosses the next boundary
    firsts = [0, a1, a2, a3, b, c, T - 3]
    assert a3 + 3 + 2 * hang + 1 < b and c + 3 + 2 * hang + 1 < T - 3
    x = _impulses(T, fl, step, firsts)
    args = (fl, step, 0.5, 0.0, hang, 3 + 2 * hang)                       # min_run = a full interior run of one impulse
    assert _raw_frames(x, fl, step, 0.5, 0.0) == sorted(set(t for k in firsts for t in range(k, k + 3)))
    want = _check([x], *args, _launch([x], *args))
    assert want == [[(0, 3 + hang), (a1 - hang, a2 + 3 + hang), (a3 - hang, a3 + 3 + hang), (b - hang, b + 3 + hang), (c - hang, c + 3 + hang),
                     (T - 3 - hang, T)][(1 if hang else 0):(-1 if hang else None)]]      # the clipped end runs are hang short of min_run
    # with min_run = 2 the runs clipped at frame 0 and at frame T stay, whatever hang is
    args = args[:5] + (2,)
    assert _check([x], *args, _launch([x], *args)) == [[(0, 3 + hang), (a1 - hang, a2 + 3 + hang), (a3 - hang, a3 + 3 + hang), (b - hang, b + 3 + hang),
                                                        (c - hang, c + 3 + hang), (T - 3 - hang, T)]]
    args = args[:5] + (3 + 2 * hang,)
    # one frame more of min_run drops every single-impulse run; the joined one stays
    args = args[:5] + (3 + 2 * hang + 1,)
    assert _check([x], *args, _launch([x], *args)) == [[(a1 - hang, a2 + 3 + hang)]]
    if hang == 0:
        # a two-frame cluster (an impulse where only two frames overlap) next to the three-frame ones
        y = x.copy()
        y[step * 39 + 100] = 0.5                                          # sample 6340: frames 38..39 at (400, 160)
        rawf = _raw_frames(y, fl, step, 0.5, 0.0)
        assert 38 in rawf and 39 in rawf and 37 not in rawf and 40 not in rawf
        args = (fl, step, 0.5, 0.0, 0, 3)
        want = _check([y], *args, _launch([y], *args))[0]
        assert (38, 40) not in want and (a3, a3 + 3) in want              # min_run - 1 frames dropped, min_run frames kept
        args = (fl, step, 0.5, 0.0, 0, 2)
        assert (38, 40) in _check([y], *args, _launch([y], *args))[0]


def test_null_energy_and_null_emax():
    rng = np.random.RandomState(5)
    rows = [_noise_with_bursts(rng, T, 400, 160, False) for T in (70, 130)]
    args = (400, 160, 1e-2, 4e-5, 3, 4)
    full = _launch(rows, *args)
    _check(rows, *args, full)
    for we, wm in ((False, True), (True, False), (False, False)):
        out = _launch(rows, *args, want_energy=we, want_emax=wm)
        _check(rows, *args, out)
        assert np.array_equal(out[2], full[2]) and np.array_equal(out[3], full[3])


# ---- the other paths of the kernels ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fl,step", [(1200, 480), (13000, 5000), (100, 333), (7, 1)],
                         ids=["staged_in_passes", "unstaged", "step_over_frame", "odd_and_tiny"])
def test_other_frame_geometries(fl, step):
    """48 kHz frames do not fit the staging buffer 64 at a time (passes of fewer frames), frames longer than the buffer are read from
    memory, a step longer than the frame leaves samples unread, an odd step needs no padding"""
    rng = np.random.RandomState(step)
    rows = [_noise_with_bursts(rng, T, fl, step, False, extra=5) for T in (70, 64, 3)]
    args = (fl, step, 1e-2, fl * 1e-7, 2, 2)
    _check(rows, *args, _launch(rows, *args))


def test_many_tiles_and_many_runs():
    """more than 1024 tiles (the row scan carries between its passes) and more than 1024 runs before and after the length filter (so
    does the compaction): impulses every 7 frames, every third one louder, two long silences"""
    from las import _hip
    tile = _hip.lib().las_vad_tile()
    fl, step = 200, 80
    T = 1024 * tile + 70
    firsts = [k for k in range(0, T - 3, 7)]
    x = np.zeros(T * step + fl, np.float32)
    for j, k in enumerate(firsts):                                        # (fl = 200, step = 80: an impulse at 80 k + 199 is in frames k .. k + 2)
        x[step * k + fl - 1] = 0.5 if j % 3 else 0.75
    x[step * 9000:step * 12000] = 0.0                                     # a long silence over many tiles
    x[step * 30:step * 200] = 0.0
    for hang, min_run, ratio in ((0, 2, 0.3), (1, 6, 0.3), (1, 5, 0.9), (2, 2, 0.3)):
        args = (fl, step, ratio, 0.0, hang, min_run)
        want = _check([x, x[:step * 5000]], *args, _launch([x, x[:step * 5000]], *args))
        if hang == 0:
            assert len(want[0]) > 1500
        if (hang, min_run) == (1, 6):
            assert want[0] == [] or len(want[0]) < 50
        if ratio == 0.9:
            assert 1024 < len(want[0]) < 4000                              # only the louder third passes: runs of 5 frames, far apart
