"""las_gemm's dispatch, held to its case table (no GPU).  las_gemm_plan is the host function las_gemm_dt launches from (csrc/gemm.hip
gemm_plan): enumerated over a grid of shapes, types, transposes, batches, masks and operand alignments it names every plan the grid
can reach -- (kernel, tile, loader, operand type, grid order, one | batch | split, masked?) -- and the table tests/gemm_cases.py, which
tests/test_gpu_gemm_exact.py runs bit for bit on the GPU, must hold exactly that set: a kernel or branch added to the dispatch without
a case fails here, and so does a change of the dispatch rule (every case records the plan it was written for)."""
import collections

import helpers  # noqa: F401  (sys.path)
import gemm_cases as G


def _lib():
    from las import _hip
    return _hip.lib(), _hip.GemmPlanInfo


def test_the_table_covers_exactly_the_plans_the_grid_reaches():
    lib, info = _lib()
    plans, refusals = G.enumerate_grid(lib, info)
    table = {}
    for c in G.RUN_CASES:
        st, ans = G.query(lib, info, c)
        assert st == "ok", (G.case_id(c), ans)
        table.setdefault(G.plan_key(ans, c), c)
    missing, extra = sorted(set(plans) - set(table)), sorted(set(table) - set(plans))
    assert not missing, "plans of the grid without a case: %s" % [(k, G.case_id(plans[k])) for k in missing[:8]]
    assert not extra, "cases whose plan the grid does not reach (extend the grid): %s" % [(k, G.case_id(table[k])) for k in extra[:8]]
    assert len(table) == 195                                         # the count when the table was written: 195 plans
    # every kernel family, tile, loader and grid order is among them
    assert {k[:3] for k in table} >= {("bf16_generic", 48, 64), ("bf16_generic", 64, 64), ("bf16_generic", 128, 128), ("bf16_fast", 64, 64),
                                      ("bf16_fast", 128, 128), ("tn_tr", 64, 128), ("tn_tr", 128, 128), ("mf32", 64, 64), ("mf32", 128, 128),
                                      ("mf32_skinny", 16, 32), ("mf32_skinny", 32, 32), ("mf32_skinny", 48, 32), ("mf32_skinny", 64, 32)}
    assert {(k[0], k[3], k[4]) for k in table if k[0] == "bf16_fast"} == {("bf16_fast", ld, bf) for ld in range(4) for bf in (0, 1)}
    assert {(k[0], k[3]) for k in table if k[0].startswith("mf32")} == {(n, ld) for n in ("mf32", "mf32_skinny") for ld in range(5)}
    assert {k[5] for k in table} == {0, 1, 2}
    # refusals are a set of their own, and the table holds a refused call for every reason the grid meets
    want = {}
    for c in G.REFUSED_CASES:
        st, ans = G.query(lib, info, c)
        assert st == "refused" and ans == c.plan, (G.case_id(c), st, ans)
        want[ans] = c
    assert set(refusals) == set(want), (sorted(refusals), sorted(want))
    assert len(refusals) == 4 and not set(refusals) & {str(k) for k in plans}


def test_every_case_answers_the_plan_it_records_and_splits_with_the_scratch_query():
    lib, info = _lib()
    assert len({G.case_id(c) for c in G.CASES}) == len(G.CASES)
    bad = []
    for c in G.RUN_CASES:
        st, ans = G.query(lib, info, c)
        if st != "ok" or ans != c.plan:
            bad.append((G.case_id(c), c.plan, ans))
            continue
        p = dict(zip(G.PLAN_FIELDS, ans))
        ws = int(lib.las_gemm_workspace_bytes(c.prec, c.M, c.N, c.K, c.batch))
        assert (p["splitk"] > 1) == (ws != 0), (G.case_id(c), p, ws)
        if p["splitk"] > 1:
            assert p["kchunk"] % 32 == 0 and (p["splitk"] - 1) * p["kchunk"] < c.K <= p["splitk"] * p["kchunk"], (G.case_id(c), p)
            assert ws == 4 * c.M * c.N * p["splitk"] or ws == 256 << 20, (G.case_id(c), p, ws)
            st0, ans0 = G.query(lib, info, c, 0)                    # without scratch the product runs unsplit
            assert st0 == "ok" and dict(zip(G.PLAN_FIELDS, ans0))["splitk"] == 1, (G.case_id(c), ans0)
        else:
            assert p["kchunk"] == c.K, (G.case_id(c), p)
        assert p["in_bf16"] == int(c.in_dtype == G.BF16)
        nx, ny = -(-c.N // p["tile_n"]), (1 if p["kernel"] == 5 else -(-c.M // p["tile_m"]))
        z = p["splitk"] if p["splitk"] > 1 else c.batch
        want = {0: (nx, ny, z), 1: (nx * ny * (-(-z // 8) * 8), 1, 1), 2: (nx * (-(-ny // 8) * 8), 1, 1)}[p["grid_order"]]
        assert (p["grid_x"], p["grid_y"], p["grid_z"]) == want, (G.case_id(c), p, want)
    assert not bad, "%d cases answer another plan than the table records, e.g. %s" % (len(bad), bad[:4])


def test_the_table_holds_the_cases_no_plan_asks_for_by_itself():
    plans = [dict(zip(G.PLAN_FIELDS, c.plan), c=c) for c in G.RUN_CASES]
    zg = collections.Counter((G.KERNELS[p["kernel"]], p["c"].batch) for p in plans if p["grid_order"] == 1 and p["splitk"] == 1)
    assert zg["bf16_fast", 5] and zg["bf16_fast", 9] and zg["tn_tr", 5] and zg["tn_tr", 9], zg          # second round of eight: batch 9
    assert any(p["grid_order"] == 1 and p["splitk"] > 1 for p in plans)
    assert any(p["grid_order"] == 2 and p["tile_m"] == 64 and p["c"].M == 4100 for p in plans)      # 65 row blocks
    assert any(p["grid_order"] == 2 and p["tile_m"] == 128 and p["c"].M == 8200 for p in plans)
    # the mask: both skips, K no multiple of the period, alone / batched / split on every kernel that serves it
    for kern, tiles in (("bf16_generic", (48, 64, 128)), ("mf32", (64, 128)), ("mf32_skinny", (16, 32, 48, 64))):
        for tm in tiles:
            for how in ("one", "batch", "split"):
                got = {p["c"].mask_skip for p in plans if G.KERNELS[p["kernel"]] == kern and p["tile_m"] == tm and p["c"].mask_period
                       and p["c"].K % p["c"].mask_period and G.plan_key(p["c"].plan, p["c"])[6] == how}
                assert got == {0, 3}, (kern, tm, how, got)
    assert any(p["c"].mask_period and p["splitk"] > 1 and p["c"].K == 4100 and p["tile_m"] in (48, 64) for p in plans)
    # the generic loader: vector and scalar loads, k- and row-contiguous, for A and for B, under every kernel that uses it
    seen = collections.defaultdict(set)
    for p in plans:
        if p["kernel"] == 1 or (p["kernel"] in (4, 5) and p["loader"] == 0):
            if p["c"].K:
                a, b = G.loader_branches(p["c"])
                seen[G.KERNELS[p["kernel"]], "A"].add(a)
                seen[G.KERNELS[p["kernel"]], "B"].add(b)
    for kern in ("bf16_generic", "mf32", "mf32_skinny"):
        for op in "AB":
            assert seen[kern, op] == {"vec_k", "scalar_k", "vec_row", "scalar_row"}, (kern, op, seen[kern, op])
    assert {G.KERNELS[p["kernel"]] for p in plans if p["c"].K == 0} == {"bf16_generic", "mf32", "mf32_skinny"}
    assert any(p["in_bf16"] and p["c"].M <= 48 and p["tile_m"] == 64 for p in plans)                # no 48-row branch-free tile
    # exactness needs |partial sums| < 2^24: operands in [-3, 3], C0 and bias in [-8, 8], alpha <= 2
    assert all(2 * 9 * c.K + 16 < 2 ** 24 and c.alpha in (1, 2) and c.beta in (0, 1, -1) for c in G.CASES)
