"""Host logic of the Listener's train-step schedule in las.layers: the two-ended chunk partition, the switch context manager and the
hand-over record.  No GPU and no library: importing las.layers must not load liblas_hip.so."""
import subprocess
import sys

import pytest

from helpers import PKG
from las import _hip, layers as L


def test_importing_layers_loads_no_library():
    code = "import sys; sys.path.insert(0, %r); from las import _hip, layers; assert _hip._lib is None and layers._SWITCHES" % PKG
    subprocess.run([sys.executable, "-c", code], check=True)      # (a fresh process: other tests of this one have loaded the library)


def _todays_formula(k, c, T):
    """the four lines that stood at each of the four chunked products before they shared _chunk_frames"""
    th = (T + 1) // 2
    lo0, lo1 = k * c, min((k + 1) * c, th)
    hi0, hi1 = max(T - lo1, lo1), T - lo0
    return lo0, lo1 - lo0, hi0, hi1 - hi0


@pytest.mark.parametrize("c", [1, 2, 16, 64])
def test_chunk_frames_partition_every_sequence_from_both_ends(c):
    for T in range(1, 301):
        th = -(-T // 2)
        nch = -(-th // c)
        seen = [0] * T
        for k in range(nch):
            lo0, nlo, hi0, nhi = L._chunk_frames(k, c, T)
            assert (lo0, nlo, hi0, nhi) == _todays_formula(k, c, T), (T, c, k)
            assert nlo >= 0 and nhi >= 0, (T, c, k)
            # the low range: c steps from t = k c, ending at ceil(T / 2)
            assert (lo0, lo0 + nlo) == (k * c, min((k + 1) * c, th)), (T, c, k)
            # the high range: its mirror image [T - lo1, T - lo0), clipped at the low range's end
            assert (hi0, hi0 + nhi) == (max(T - (lo0 + nlo), lo0 + nlo), T - lo0), (T, c, k)
            for t in list(range(lo0, lo0 + nlo)) + list(range(hi0, hi0 + nhi)):
                seen[t] += 1
        assert seen == [1] * T, (T, c, seen)
        assert L._Handover(c, T, None).nchunks == nch


def _switches():
    return {k: getattr(L, k) for k in L._SWITCHES}


def test_schedule_restores_every_switch_after_exit_and_after_an_exception():
    before = _switches()
    with L.schedule(XPROJ_CHUNK_STEPS=0, HOLD_SIDE=False, TAIL_WINDOW=160):
        assert (L.XPROJ_CHUNK_STEPS, L.HOLD_SIDE, L.TAIL_WINDOW) == (0, False, 160)
        assert {k: v for k, v in _switches().items() if k not in ("XPROJ_CHUNK_STEPS", "HOLD_SIDE", "TAIL_WINDOW")} == \
               {k: v for k, v in before.items() if k not in ("XPROJ_CHUNK_STEPS", "HOLD_SIDE", "TAIL_WINDOW")}
    assert _switches() == before
    with pytest.raises(ZeroDivisionError):
        with L.schedule(DOUT_CHUNK_ROWS=0, PREPARED_SWEEPS=False):
            assert (L.DOUT_CHUNK_ROWS, L.PREPARED_SWEEPS) == (0, False)
            1 / 0
    assert _switches() == before


def test_schedule_nests():
    before = _switches()
    with L.schedule(TAIL_WINDOW=160, DOUT_CHUNK_ROWS=32):
        with L.schedule(TAIL_WINDOW=64, HOLD_SIDE=False):
            assert (L.TAIL_WINDOW, L.DOUT_CHUNK_ROWS, L.HOLD_SIDE) == (64, 32, False)
        assert (L.TAIL_WINDOW, L.DOUT_CHUNK_ROWS, L.HOLD_SIDE) == (160, 32, before["HOLD_SIDE"])
    assert _switches() == before


def test_schedule_refuses_a_name_that_is_not_a_switch():
    before = _switches()
    for name in ("NO_SUCH_SWITCH", "VARIANTS", "DENSE_CHUNKS", "TAIL_ONE_LAUNCH", "DROPOUT_KERNEL", "DIRECT_GRADS"):
        with pytest.raises(ValueError):
            with L.schedule(**{name: 0, "TAIL_WINDOW": 160}):
                pass
        assert not hasattr(L, name) or name == "VARIANTS"
    assert _switches() == before


def test_fallback_schedule_sets_what_a_rerun_needs_and_restores_it():
    before, flags = _switches(), _hip.speller_flags
    with L.schedule(XPROJ_CHUNK_STEPS=64, DOUT_CHUNK_ROWS=64, TAIL_WINDOW=160, HOLD_SIDE=True, PREPARED_SWEEPS=True):
        inside = _switches()
        with L.fallback_schedule():
            assert (L.XPROJ_CHUNK_STEPS, L.DOUT_CHUNK_ROWS, L.TAIL_WINDOW) == (0, 0, 0)
            assert L.HOLD_SIDE is False and L.PREPARED_SWEEPS is False
            assert _hip.speller_flags == flags | _hip.SPELLER_NO_FUSED_STEP
            assert {k: v for k, v in _switches().items() if k not in ("XPROJ_CHUNK_STEPS", "DOUT_CHUNK_ROWS", "TAIL_WINDOW", "HOLD_SIDE", "PREPARED_SWEEPS")} == \
                   {k: v for k, v in inside.items() if k not in ("XPROJ_CHUNK_STEPS", "DOUT_CHUNK_ROWS", "TAIL_WINDOW", "HOLD_SIDE", "PREPARED_SWEEPS")}
        assert _switches() == inside and _hip.speller_flags == flags
        with pytest.raises(ZeroDivisionError):
            with L.fallback_schedule():
                1 / 0
        assert _switches() == inside and _hip.speller_flags == flags
        with L.fallback_schedule(False):                      # (a step that is not a re-run: nothing changes)
            assert _switches() == inside and _hip.speller_flags == flags
    assert _switches() == before and _hip.speller_flags == flags


@pytest.mark.parametrize("steps,frames", [(64, 320), (64, 64), (16, 33), (1, 1)])
def test_handover_finish_runs_the_remaining_chunks_in_order_and_never_chunk_0(steps, frames):
    ran = []
    rec = L._Handover(steps, frames, ran.append)
    assert rec.nchunks == -(-(-(-frames // 2)) // steps)
    rec.finish()
    assert ran == list(range(1, rec.nchunks))
    assert (rec.steps, rec.frames, rec.keep_alive, rec.flag, rec.holder) == (steps, frames, (), None, None)


def test_reset_handovers_empties_every_registry_and_names_the_chunked_ones_that_were_left():
    L._XCHUNK[1] = L._DCHUNK[2] = L._Handover(64, 320, None)
    L._TANH_OUT[3] = None
    L._DPRE.add(4)
    assert sorted(L._reset_handovers()) == ["_DCHUNK", "_XCHUNK"]
    assert not (L._XCHUNK or L._DCHUNK or L._DOUT_CHUNKS or L._TANH_OUT or L._DPRE or L._EXPECT_DPRE)
    L._DOUT_CHUNKS[5] = L._Handover(64, 320, None)
    with pytest.raises(RuntimeError, match="_DOUT_CHUNKS"):
        L.check_handovers_consumed()
    L.check_handovers_consumed()                             # (the failed check cleared it)
