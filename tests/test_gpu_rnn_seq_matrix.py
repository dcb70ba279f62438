"""Every bf16 Listener sweep kernel the plan can reach (csrc/rnn_seq.hip plan_sweep), one table row per (cell, H, P, rows per tile,
kernel), against the rounded-operand float64 reference of tests/rnn_seq_ref.py at the bounds recorded there.  Each case asks
las_rnn_seq_plan which kernel its launch gets and asserts that it is the one the row names BEFORE it launches;
tests/test_rnn_seq_ref_host.py checks without a GPU that the tables cover every tuple the plan's grid reaches.

The tables are plain data and this module imports without touching the device."""
import functools

import pytest
import torch

import helpers  # noqa: F401  (sys.path)
import rnn_seq_ref as RR

LSTM, RNN = 1, 0
NO_KSPLIT, NO_HELPER_WAVES, ROWS16, NO_WARMERS, AGENT_GRANULES = 2, 4, 8, 16, 1
MODE_ROWS, MODE_CHUNKS, MODE_PROGRESS = 1, 2, 4

# (cell, H, B, T, flags, LAS_SEQ_P override, P, forward kernel, its rows per tile, BPTT kernel, its rows per tile, row-chunk launches)
# Rows: B in {3, 8, 9} on 8-row tiles, {5, 16, 17} on 16-row tiles (less than a tile, one tile, a ragged second tile); the 16-row tile is
# forced by LAS_SEQ_ROWS16 once per width and by a batch past 8 x max_tiles elsewhere (B = 130 at P = 8, B = 260 at P = 4).  Frames: T = 1,
# T = 2 and an odd T in 9..13 (both exchange slots reused several times).  Two neighbouring rows of a width differ in one plan field.
MATRIX = [
    (1, 64, 5, 11, 0, 0, 1, "FWD_HW16", 16, "BWD_PLAIN", 16, 1),
    (1, 64, 17, 2, 4, 0, 1, "FWD_PLAIN", 16, "BWD_PLAIN", 16, 1),
    (1, 128, 16, 9, 0, 1, 1, "FWD_PLAIN", 16, "BWD_PLAIN", 16, 1),
    (1, 128, 3, 13, 0, 0, 2, "FWD_HW8", 8, "BWD_KS8", 8, 1),
    (1, 128, 9, 1, 0, 0, 2, "FWD_HW8", 8, "BWD_KS8", 8, 1),
    (1, 128, 17, 11, 8, 0, 2, "FWD_HW16", 16, "BWD_KS16", 16, 1),
    (1, 128, 5, 9, 6, 0, 2, "FWD_PLAIN", 16, "BWD_PLAIN", 16, 1),
    (1, 128, 16, 2, 12, 0, 2, "FWD_PLAIN", 16, "BWD_KS16", 16, 1),
    (1, 256, 9, 11, 0, 0, 4, "FWD_HW8", 8, "BWD_KS8", 8, 1),
    (1, 256, 8, 2, 0, 0, 4, "FWD_HW8", 8, "BWD_KS8", 8, 1),
    (1, 256, 5, 9, 8, 0, 4, "FWD_HW16", 16, "BWD_KS16", 16, 1),
    (1, 256, 17, 13, 6, 0, 4, "FWD_PLAIN", 16, "BWD_PLAIN", 16, 1),
    (1, 256, 260, 3, 0, 0, 4, "FWD_HW16", 16, "BWD_KS16", 16, 1),
    (1, 256, 9, 9, 0, 2, 2, "FWD_PLAIN", 16, "BWD_KS8", 8, 1),
    (1, 256, 17, 11, 8, 2, 2, "FWD_PLAIN", 16, "BWD_KS16", 16, 1),
    (1, 256, 5, 2, 2, 2, 2, "FWD_PLAIN", 16, "BWD_PLAIN", 16, 1),
    (1, 512, 3, 9, 0, 0, 8, "FWD_PLAIN", 16, "BWD_KS8", 8, 1),
    (1, 512, 9, 2, 0, 0, 8, "FWD_PLAIN", 16, "BWD_KS8", 8, 1),
    (1, 512, 130, 3, 0, 0, 8, "FWD_PLAIN", 16, "BWD_KS16", 16, 1),
    (1, 512, 17, 11, 8, 0, 8, "FWD_PLAIN", 16, "BWD_KS16", 16, 1),
    (1, 512, 5, 9, 2, 0, 8, "FWD_PLAIN", 16, "BWD_PLAIN", 16, 1),
    (0, 64, 5, 11, 0, 0, 1, "FWD_PLAIN", 16, "BWD_PLAIN", 16, 1),
    (0, 128, 17, 9, 0, 0, 1, "FWD_HW16", 16, "BWD_PLAIN", 16, 1),
    (0, 128, 16, 2, 4, 0, 1, "FWD_PLAIN", 16, "BWD_PLAIN", 16, 1),
    (0, 256, 5, 13, 0, 1, 1, "FWD_HW16", 16, "BWD_PLAIN", 16, 1),
    (0, 256, 17, 1, 4, 1, 1, "FWD_PLAIN", 16, "BWD_PLAIN", 16, 1),
    (0, 256, 9, 11, 0, 0, 2, "FWD_HW16", 16, "BWD_KS8", 8, 1),
    (0, 256, 3, 2, 0, 0, 2, "FWD_HW16", 16, "BWD_KS8", 8, 1),
    (0, 256, 17, 9, 8, 0, 2, "FWD_HW16", 16, "BWD_KS16", 16, 1),
    (0, 256, 5, 9, 6, 0, 2, "FWD_PLAIN", 16, "BWD_PLAIN", 16, 1),
    (0, 512, 8, 9, 0, 2, 2, "FWD_PLAIN", 16, "BWD_KS8", 8, 1),
    (0, 512, 16, 11, 8, 2, 2, "FWD_PLAIN", 16, "BWD_KS16", 16, 1),
    (0, 512, 5, 2, 2, 2, 2, "FWD_PLAIN", 16, "BWD_PLAIN", 16, 1),
    (0, 512, 9, 13, 0, 0, 4, "FWD_HW16", 16, "BWD_KS8", 8, 1),
    (0, 512, 16, 9, 8, 0, 4, "FWD_HW16", 16, "BWD_KS16", 16, 1),
    (0, 512, 17, 2, 6, 0, 4, "FWD_PLAIN", 16, "BWD_PLAIN", 16, 1),
]
# more row tiles than one launch holds: swept in two row-chunk launches, both directions, bias sums across the chunks
CHUNK_CASES = [
    (1, 256, 560, 5, 0, 0, 4, "FWD_HW16", 16, "BWD_KS16", 16, 2),
    (1, 512, 260, 3, 8, 0, 8, "FWD_PLAIN", 16, "BWD_KS16", 16, 2),
]
# (cell, H, B, T, LAS_SEQ_P override, mode, P, kernel, rows per tile): the variants a call's mode selects.  The ragged forward exists where
# the 8-row helper-wave kernel does: the LSTM at H = 128 and 256 (the tanh cell has 16-row helper waves only, the LSTM at H = 512 none --
# the completeness check of tests/test_rnn_seq_ref_host.py shows that no other width plans it)
MODE_CASES = [
    (1, 128, 9, 11, 0, 1, 2, "FWD_HW8_RAGGED", 8),
    (1, 256, 11, 9, 0, 1, 4, "FWD_HW8_RAGGED", 8),
    (1, 128, 9, 11, 0, 2, 2, "BWD_KS8_CH", 8),
    (1, 128, 9, 11, 0, 6, 2, "BWD_KS8_CH_PG", 8),
    (1, 256, 9, 9, 2, 2, 2, "BWD_KS8_CH", 8),
    (1, 256, 9, 9, 2, 6, 2, "BWD_KS8_CH_PG", 8),
    (1, 256, 11, 9, 0, 2, 4, "BWD_KS8_CH", 8),
    (1, 256, 11, 9, 0, 6, 4, "BWD_KS8_CH_PG", 8),
    (1, 512, 9, 9, 0, 2, 8, "BWD_KS8_CH", 8),
    (1, 512, 9, 9, 0, 6, 8, "BWD_KS8_CH_PG", 8),
    (0, 256, 9, 11, 0, 2, 2, "BWD_KS8_CH", 8),
    (0, 256, 9, 11, 0, 6, 2, "BWD_KS8_CH_PG", 8),
    (0, 512, 9, 9, 2, 2, 2, "BWD_KS8_CH", 8),
    (0, 512, 9, 9, 2, 6, 2, "BWD_KS8_CH_PG", 8),
    (0, 512, 11, 9, 0, 2, 4, "BWD_KS8_CH", 8),
    (0, 512, 11, 9, 0, 6, 4, "BWD_KS8_CH_PG", 8),
]


def seq_p(p):
    return (int(p) & 0xf) << 8


def case_flags(case):
    return case[4] | (seq_p(case[5]) if case[5] else 0)


def case_claims(case):
    """the (cell, H, P, rows per tile, kernel) tuples a MATRIX / CHUNK_CASES row claims"""
    cell, H, _, _, _, _, P, kf, rf, kb, rbw, _ = case
    return [(cell, H, P, rf, kf), (cell, H, P, rbw, kb)]


def short_k_split(case):
    """the cases whose bias sums' rounding residual is comparable with the reference's (rnn_seq_ref.bias_residual)"""
    return case[9].startswith("BWD_KS") and case[3] <= 2


def case_seed(case):
    return 1000 * case[1] + 31 * case[2] + case[3] + 7 * case[0]


@functools.lru_cache(maxsize=None)
def case_inputs(case, seed=None):
    cell, H, B, T = case[:4]
    return RR.make_inputs("lstm" if cell else "rnn", B, T, H, case_seed(case) if seed is None else seed)


def case_reference(case, fn=RR.reference, row_T=None, seed=None, **kw):
    """both directions of the reference (or of the emulation) for a MATRIX / CHUNK_CASES row (seed: other inputs of the same shape)"""
    cell, H, B, T, _, _, P, kf, rf, kb, rbw, _ = case
    xp, whh, R = case_inputs(case, seed)
    max_tiles = (256 // P // 8) * 8 // 2
    return [fn(xp[:, :, d], whh[d], R[:, :, d * H:(d + 1) * H], "lstm" if cell else "rnn", bool(d), P=P, ksplit=kb.startswith("BWD_KS"),
               row_T=row_T, rows_per_tile=rbw, launch_rows=max_tiles * rbw, **kw) for d in range(2)]


@functools.lru_cache(maxsize=None)
def _reference(case):
    return case_reference(case)


def _assert_planned(case, flags, mode_f=0, mode_b=0):
    from las import _hip
    cell, H, B, T, _, _, P, kf, rf, kb, rbw, n = case
    assert _hip.rnn_seq_plan_kernel(cell, 1, B, H, flags, False, mode_f)[:3] == (kf, P, rf), (case, flags)
    got = _hip.rnn_seq_plan_kernel(cell, 1, B, H, flags, True, mode_b)
    assert got == (kb, P, rbw, n), (case, flags, got)


def _sweep(case, flags, rows=None, fwd_kw=None, bwd_kw=None):
    """las_rnn_seq_fwd, then las_rnn_seq_bwd (with both bias gradients) on the same buffers (batch rows `rows` of the case's inputs).  The frame pitch of h and of
    the upstream gradient leaves one pad frame per row; the bias sums accumulate onto non-zero values.
    -> dict of CPU tensors: h [B, T, 2 H], c [B, T, 2, H], act (saved gates), dz [B, T, 2, G H], db [2][G H] (minus their initial values)"""
    from las import _hip
    cell, H, B, T = case[:4]
    xp, whh, R = case_inputs(case)
    if rows is not None:
        xp, R = xp[rows], R[rows]
        B = xp.shape[0]
    G = 4 if cell else 1
    GH = G * H
    dev = "cuda"
    bf = torch.bfloat16
    gates = xp.to(dev).to(bf).contiguous()
    w0, w1 = whh[0].to(dev), whh[1].to(dev)
    Tp = T + 1
    out = torch.zeros(B, Tp, 2 * H, device=dev, dtype=bf)
    cst = torch.zeros(B, T, 2, H, device=dev, dtype=bf) if cell else None
    _hip.check_status()
    _hip.rnn_seq_fwd(cell, 1, B, T, H, gates, w0, w1, GH, out, 2 * H, Tp * 2 * H, cst, flags=flags, **(fwd_kw or {}))
    act = gates.clone()
    dout = torch.zeros(B, Tp, 2 * H, device=dev, dtype=bf)
    dout[:, :T] = R.to(dev).to(bf)
    init = RR.DB_INIT
    db = [torch.full((GH,), v, device=dev) for v in init]
    _hip.rnn_seq_bwd(cell, 1, B, T, H, gates, w0, w1, GH, out, 2 * H, Tp * 2 * H, cst, dout, 2 * H, Tp * 2 * H, db_fw=db[0], db_bw=db[1],
                     flags=flags, **(bwd_kw or {}))
    torch.cuda.synchronize()
    _hip.check_status()                                            # the status word is clean
    assert bool((out[:, T:].view(torch.int16) == 0).all()), "pad frame written"
    return {"h": out[:, :T].cpu(), "c": cst.cpu() if cell else None, "act": act.cpu(), "dz": gates.cpu(),
            "db": [(db[d].cpu().double() - init[d]) for d in range(2)]}


def _split(res, H, d):
    """direction d of a _sweep result, in the reference's layout"""
    return {"h": res["h"][:, :, d * H:(d + 1) * H].double(), "c": None if res["c"] is None else res["c"][:, :, d].double(),
            "dz": res["dz"][:, :, d].double(), "db": res["db"][d]}


def _check_against_reference(case, res, ref, tag):
    H = case[1]
    worst = {}
    for d in range(2):
        for k, v in RR.distances(_split(res, H, d), ref[d]).items():
            worst[k] = max(worst.get(k, 0.0), v)
        if short_k_split(case):      # the K-split kernels sum the bias gradient BEFORE dZ is rounded: the residual against the stored dZ says so
            got = res["db"][d] - res["dz"][:, :, d].double().sum((0, 1))
            worst["db_res"] = max(worst.get("db_res", 0.0), RR.bias_residual_distance(got, RR.bias_residual(ref[d])))
    print("MATRIX-FRACTION %s %s " % (tag, (case,)) + " ".join("%s=%.3f" % (k, worst[k] / RR.BOUNDS[k]) for k in sorted(worst)))
    for k, v in worst.items():
        assert v <= RR.BOUNDS[k], (tag, case, k, v, RR.BOUNDS[k])


def _same_bits(a, b, names=("h", "c", "act", "dz")):
    for k in names:
        assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("case", MATRIX, ids=lambda c: "-".join(str(x) for x in c[:6]))
def test_planned_kernel_matches_reference(case):
    """h on every real frame, c, dZ and both bias sums of the kernel pair the row names, against the float64 reference with the kernels'
    rounding points; pad frames stay bit-zero; the status word stays clean."""
    flags = case_flags(case)
    _assert_planned(case, flags)
    res = _sweep(case, flags)
    _check_against_reference(case, res, _reference(case), "matrix")


# one case per kernel family: helper-wave forward + K-split BPTT on 8-row tiles, the plain kernels on a cluster, 16-row tiles of the tanh cell
FLAG_BASES = [MATRIX[8], MATRIX[11], MATRIX[28]]


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [NO_WARMERS, AGENT_GRANULES])
@pytest.mark.parametrize("case", FLAG_BASES, ids=lambda c: "-".join(str(x) for x in c[:6]))
def test_placement_flags_change_no_bit(case, extra):
    """LAS_SEQ_NO_WARMERS removes the L2 warmer workgroups, LAS_SEQ_AGENT_GRANULES the same-XCD store scope of the granules: placement and
    transport, not arithmetic.  The same kernels must run and every result, bias sums included, must be the same bits."""
    flags = case_flags(case)
    _assert_planned(case, flags)
    _assert_planned(case, flags | extra)
    a, b = _sweep(case, flags), _sweep(case, flags | extra)
    _same_bits(a, b)
    for d in range(2):
        assert torch.equal(a["db"][d], b["db"][d])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CHUNK_CASES, ids=lambda c: "-".join(str(x) for x in c[:6]))
def test_row_chunks_both_directions(case):
    """A batch with more row tiles than one launch holds: forward, BPTT and the bias sums over BOTH row-chunk launches against the
    reference; and rows of the first launch, of the second and the ragged tail equal the same rows swept as a small batch of the same
    16-row tiling, bit for bit (rows do not interact)."""
    cell, H, B, T = case[:4]
    flags = case_flags(case)
    _assert_planned(case, flags)
    res = _sweep(case, flags)
    _check_against_reference(case, res, _reference(case), "row-chunks")
    from las import _hip
    P, rbw = case[6], case[10]
    per_launch = (256 // P // 8) * 8 // 2 * rbw
    assert per_launch < B
    tail0 = (B - 1) // 16 * 16
    for r0, r1 in ((0, 16), (per_launch, min(per_launch + 16, B)), (tail0, B)):
        n = r1 - r0
        small = flags | ROWS16
        assert _hip.rnn_seq_plan_kernel(cell, 1, n, H, small, False)[:3] == (case[7], P, case[8])
        assert _hip.rnn_seq_plan_kernel(cell, 1, n, H, small, True)[:3] == (case[9], P, rbw)
        part = _sweep(case, small, rows=slice(r0, r1))
        for k in ("h", "c", "act", "dz"):
            assert torch.equal(part[k], res[k][r0:r1]), (k, r0, r1)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in MODE_CASES if c[5] == MODE_ROWS], ids=lambda c: "-".join(str(x) for x in c[:6]))
def test_ragged_forward_outside_the_default_width(case):
    """FWD_HW8_RAGGED with row_T (one row of a single frame): every real frame equals the reference swept with the same row lengths and,
    bit for bit, the row swept alone at its own length; behind a row's end h and c are zero."""
    from las import _hip
    cell, H, B, T, p, mode, P, kern, rbt = case
    flags = seq_p(p) if p else 0
    assert _hip.rnn_seq_plan_kernel(cell, 1, B, H, flags, False, MODE_ROWS)[:3] == (kern, P, rbt)
    assert _hip.rnn_seq_fwd_rows_ok(cell, 1, B, H, flags)
    lens = [T, 1, T - 2, 2, T, 3, T - 1, 5, 1, 4, T][:B]
    full = (cell, H, B, T, 0, p, P, "FWD_HW8", 8, "BWD_KS8", 8, 1)
    xp, whh, R = case_inputs(full)
    dev, bf, GH = "cuda", torch.bfloat16, 4 * H
    w0, w1 = whh[0].to(dev), whh[1].to(dev)
    row_T = torch.tensor(lens, dtype=torch.int32, device=dev)
    out = torch.full((B, T, 2 * H), 7.0, device=dev, dtype=bf)
    cst = torch.full((B, T, 2, H), 7.0, device=dev, dtype=bf)
    _hip.rnn_seq_fwd(cell, 1, B, T, H, xp.to(dev).to(bf), w0, w1, GH, out, 2 * H, T * 2 * H, cst, flags=flags, row_T=row_T)
    torch.cuda.synchronize()
    _hip.check_status()
    worst = {"h": 0.0, "c": 0.0}
    for d in range(2):
        r = RR.reference(xp[:, :, d], whh[d], None, "lstm", bool(d), P=P, row_T=lens)
        got = {"h": out[:, :, d * H:(d + 1) * H].cpu().double(), "c": cst[:, :, d].cpu().double()}
        for k, v in RR.distances(got, r).items():
            worst[k] = max(worst[k], v)
    print("MATRIX-FRACTION ragged %s " % (case,) + " ".join("%s=%.3f" % (k, worst[k] / RR.BOUNDS[k]) for k in sorted(worst)))
    assert worst["h"] <= RR.BOUNDS["h"] and worst["c"] <= RR.BOUNDS["c"], (case, worst)
    for b, n in enumerate(lens):
        o1 = torch.empty(1, n, 2 * H, device=dev, dtype=bf)
        c1 = torch.empty(1, n, 2, H, device=dev, dtype=bf)
        _hip.rnn_seq_fwd(cell, 1, 1, n, H, xp[b:b + 1, :n].to(dev).to(bf).contiguous(), w0, w1, GH, o1, 2 * H, n * 2 * H, c1, flags=flags)
        assert torch.equal(out[b, :n], o1[0]) and torch.equal(cst[b, :n], c1[0]), (b, n)
        assert bool((out[b, n:] == 0).all()) and bool((cst[b, n:] == 0).all()), (b, n)
    _hip.check_status()


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in MODE_CASES if c[5] & MODE_CHUNKS], ids=lambda c: "-".join(str(x) for x in c[:6]))
def test_chunk_aware_bptt_equals_the_plain_k_split_sweep(case):
    """BWD_KS8_CH / BWD_KS8_CH_PG with every chunk flagged complete before the launch (the waiting itself is test_gpu_rnn_seq.py's): dZ and
    the bias sums are the bits of BWD_KS8 on the same inputs; the progress words end at T."""
    from las import _hip
    cell, H, B, T, p, mode, P, kern, rbt = case
    flags = seq_p(p) if p else 0
    assert _hip.rnn_seq_plan_kernel(cell, 1, B, H, flags, True, mode)[:3] == (kern, P, rbt)
    assert _hip.rnn_seq_plan_kernel(cell, 1, B, H, flags, True, 0)[:3] == ("BWD_KS8", P, rbt)
    assert _hip.rnn_seq_bwd_chunks_ok(cell, 1, B, H, flags)
    full = (cell, H, B, T, 0, p, P, "", 0, "BWD_KS8", 8, 1)
    base = _sweep(full, flags)
    flag = torch.full((1,), 1000, dtype=torch.int32, device="cuda")
    kw = dict(chunk_flag=flag, chunk_rows=4, n_rows=T)
    prog = None
    if mode & MODE_PROGRESS:
        nw = _hip.rnn_seq_bwd_progress_words(cell, 1, B, H, flags)
        assert nw == 2 * ((B + 7) // 8) * P
        prog = torch.zeros(nw, dtype=torch.int32, device="cuda")
        kw.update(progress=prog, progress_steps=4)
    got = _sweep(full, flags, bwd_kw=kw)
    _same_bits(base, got)
    for d in range(2):
        assert torch.equal(base["db"][d], got["db"][d]), d
    if prog is not None:
        assert int(prog.min()) == T and int(prog.max()) == T


@pytest.mark.gpu
@pytest.mark.parametrize("case", [MATRIX[3], MATRIX[33]], ids=lambda c: "-".join(str(x) for x in c[:6]))
def test_chunked_forward_equals_the_unchunked_one(case):
    """las_rnn_seq_fwd with x_chunk_flag outside H = 256 (LSTM H = 128 on 8-row tiles, the tanh cell at H = 512 on 16-row tiles) with every chunk
    flagged complete before the launch: the same kernel, the same bits."""
    from las import _hip
    cell, H, B, T = case[:4]
    flags = case_flags(case)
    _assert_planned(case, flags)
    assert _hip.rnn_seq_fwd_chunks_ok(cell, 1, B, H, flags)
    flag = torch.full((1,), 1000, dtype=torch.int32, device="cuda")
    a = _sweep(case, flags)
    b = _sweep(case, flags, fwd_kw=dict(chunk_flag=flag, chunk_steps=4))
    _same_bits(a, b)
