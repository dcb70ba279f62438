"""The Listener sweep's host-side queries, pinned.  las_rnn_seq_plan (its x_chunks, rows, dout_chunks and progress_words) and
las_rnn_seq_workspace_bytes are pure host arithmetic (no GPU needed) and must describe the kernel that the sweep launches: a chunked forward, a ragged forward and a chunked / progress-publishing BPTT are correct only on the kernel
that honours the mode.  The answers over a grid of precisions, cells, H, B, flags and cluster-width overrides are compared with a
recorded table (tests/golden/rnn_seq_plan.json).

The table assumes a device of 256 compute units (the MI355X); a host without a GPU reports the same count."""
import ctypes
import json
import os

import helpers  # noqa: F401  (sys.path)
from helpers import ROOT

PRECS = (0, 1)                      # LAS_PREC_F32, LAS_PREC_BF16
CELLS = (0, 1)                      # LAS_CELL_RNN, LAS_CELL_LSTM
HS = (64, 128, 256, 512)
BS = (1, 8, 48, 64, 96, 97, 144, 192, 256, 560)
NO_KSPLIT, NO_HELPER_WAVES, ROWS16 = 2, 4, 8
FLAGS = (0, NO_KSPLIT, NO_HELPER_WAVES, ROWS16, NO_HELPER_WAVES | ROWS16)
PS = (0, 1, 2, 4, 8)                # LAS_SEQ_P override (0: none)


def grid():
    for prec in PRECS:
        for cell in CELLS:
            for H in HS:
                for B in BS:
                    for fl in FLAGS:
                        for P in PS:
                            yield prec, cell, H, B, fl, P


def answers(l, prec, cell, H, B, flags):
    from las import _hip
    fwd, bwd = _hip.RnnSeqPlanInfo(), _hip.RnnSeqPlanInfo()
    assert l.las_rnn_seq_plan(cell, prec, B, H, flags, 0, 0, ctypes.byref(fwd)) == 0
    assert l.las_rnn_seq_plan(cell, prec, B, H, flags, 1, 0, ctypes.byref(bwd)) == 0
    return [fwd.x_chunks, fwd.rows, bwd.dout_chunks, bwd.progress_words]


def _table():
    with open(os.path.join(ROOT, "tests", "golden", "rnn_seq_plan.json")) as f:
        return json.load(f)


def test_sweep_queries_match_recorded_table():
    from las import _hip
    l = _hip.lib()
    tab = _table()
    assert tab["cus"] == 256
    rows = tab["rows"]
    assert [tuple(r[:6]) for r in rows] == list(grid())
    bad = []
    for r in rows:
        prec, cell, H, B, fl, P = r[:6]
        got = answers(l, prec, cell, H, B, fl | (_hip.seq_p(P) if P else 0))
        if got != r[6:]:
            bad.append((r[:6], r[6:], got))
    assert not bad, "%d of %d answers differ from the table, e.g. %s" % (len(bad), len(rows), bad[:5])
    for prec, cell, H, B, nbytes in tab["ws"]:
        assert l.las_rnn_seq_workspace_bytes(cell, prec, H, B) == nbytes, (prec, cell, H, B)
    assert len(tab["ws"]) == len(PRECS) * len(CELLS) * len(HS) * len(BS)


# the cluster widths instantiated per (cell, H) in csrc/rnn_seq.hip (SWEEP_INSTS)
INSTANTIATED = {(1, 64): (1,), (1, 128): (1, 2), (1, 256): (2, 4), (1, 512): (8,),
                (0, 64): (1,), (0, 128): (1,), (0, 256): (1, 2), (0, 512): (2, 4)}


def test_override_of_an_uninstantiated_width_describes_the_width_that_runs():
    """LAS_SEQ_P(p) naming a width without kernels: the sweep runs on the next narrower instantiated width, and the queries answer
    for that width (all zero where there is none)."""
    from las import _hip
    l = _hip.lib()
    n = 0
    for prec, cell, H, B, fl, P in grid():
        if not P or P in INSTANTIATED[(cell, H)]:
            continue
        got = answers(l, prec, cell, H, B, fl | _hip.seq_p(P))
        runs = [q for q in INSTANTIATED[(cell, H)] if q < P]
        want = answers(l, prec, cell, H, B, fl | _hip.seq_p(max(runs))) if runs else [0, 0, 0, 0]
        assert got == want, ((prec, cell, H, B, fl, P), got, want)
        n += got != [0, 0, 0, 0]
    assert n == 196            # the grid points whose answers the plan changed (the queries used to answer 0 at such a width)
