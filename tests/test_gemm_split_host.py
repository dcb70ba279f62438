"""las_gemm's split rule, pinned.  las_gemm_workspace_bytes is pure host arithmetic (no GPU needed): the scratch the deterministic
split-K of las_gemm / las_gemm_dt wants for a product.  Query and launch follow ONE rule in csrc/gemm.hip (gemm_split); Python sizes
the scratch from the query, so its answers over a grid of shapes are compared with a table recorded from the library before the two
copies of the rule were merged (tests/golden/gemm_workspace.json)."""
import itertools
import json
import os

import helpers  # noqa: F401  (sys.path)
from helpers import ROOT

PRECS = (0, 1)                      # LAS_PREC_F32, LAS_PREC_BF16
MS = (1, 17, 39, 48, 49, 64, 65, 127, 128, 512, 4100)
NS = (30, 64, 128, 1152, 2048)
KS = (0, 511, 512, 2047, 2048, 4095, 4096, 20011)
BATCHES = (1, 5)
WS_CAP = 256 << 20                  # include/las_hip.h LAS_GEMM_WS_CAP


def test_workspace_query_matches_recorded_table():
    from las import _hip
    l = _hip.lib()
    assert _hip.GEMM_WS_BYTES == WS_CAP
    with open(os.path.join(ROOT, "tests", "golden", "gemm_workspace.json")) as f:
        tab = json.load(f)
    assert (tuple(tab["prec"]), tuple(tab["M"]), tuple(tab["N"]), tuple(tab["K"]), tuple(tab["batch"])) == (PRECS, MS, NS, KS, BATCHES)
    grid = list(itertools.product(PRECS, MS, NS, KS, BATCHES))
    assert len(tab["bytes"]) == len(grid)
    bad = []
    for (prec, M, N, K, batch), want in zip(grid, tab["bytes"]):
        got = int(l.las_gemm_workspace_bytes(prec, M, N, K, batch))
        if got != want:
            bad.append(((prec, M, N, K, batch), want, got))
        # whole [M][N] fp32 partials, or the cap
        assert got == 0 or got % (4 * M * N) == 0 or got == WS_CAP, ((prec, M, N, K, batch), got)
    assert not bad, "%d of %d answers differ from the table, e.g. %s" % (len(bad), len(grid), bad[:5])
    assert sum(1 for v in tab["bytes"] if v) == 484          # the table is not all zeros
