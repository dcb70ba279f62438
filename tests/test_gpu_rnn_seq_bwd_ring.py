"""The K-split BPTT sweep (csrc/rnn_seq.hip rnn_seq_bwd_ks_kernel) at the edges of its operand pipeline: sweeps shorter than, equal to and
just past the number of steps it keeps in flight, chunk boundaries at every distance from the step that is being computed, and a producer
that delivers the upstream gradient while the sweep runs.

The kernel's arithmetic is fixed (the order of the MFMAs and of every fp32 addition), so dZ and the bias sums of the cases below are held
to the bits recorded in tests/golden/bptt_bits_parent.json (tools/record_bptt_bits.py wrote it, on the commit before the W_hh fragments moved
to the accumulation registers), and to the float64 reference of tests/rnn_seq_ref.py, which says WHICH frame went wrong where a hash only
says that one did."""
import functools
import hashlib
import json
import os

import pytest
import torch

import helpers  # noqa: F401  (sys.path)
import rnn_seq_ref as RR
import test_gpu_rnn_seq_matrix as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bptt_bits_parent.json")

# rows in the format of test_gpu_rnn_seq_matrix.MATRIX
GOLDEN_CASES = (
    [(1, 256, B, T, 0, 0, 4, "FWD_HW8", 8, "BWD_KS8", 8, 1) for B in (1, 9) for T in (1, 2, 3, 4, 5, 7)]
    + [(1, 128, 9, 5, 0, 0, 2, "FWD_HW8", 8, "BWD_KS8", 8, 1),
       (1, 512, 9, 5, 0, 0, 8, "FWD_PLAIN", 16, "BWD_KS8", 8, 1),
       (0, 256, 9, 5, 0, 0, 2, "FWD_HW16", 16, "BWD_KS8", 8, 1),
       (0, 512, 9, 5, 0, 0, 4, "FWD_HW16", 16, "BWD_KS8", 8, 1),
       (1, 256, 17, 5, M.ROWS16, 0, 4, "FWD_HW16", 16, "BWD_KS16", 16, 1)])


def case_id(case):
    return "-".join(str(x) for x in case[:6])


def _sha(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def result_bits(res):
    """sha256 of dZ (bf16) per direction and of both bias sums (float64 of the fp32 sums, minus their initial values)"""
    return {"dz": [_sha(res["dz"][:, :, d]) for d in range(2)], "db": [_sha(res["db"][d]) for d in range(2)]}


@functools.lru_cache(maxsize=None)
def swept(case):
    from las import _hip
    flags = M.case_flags(case)
    cell, H, B = case[:3]
    assert _hip.rnn_seq_plan_kernel(cell, 1, B, H, flags, True, 0) == (case[9], case[6], case[10], 1), case
    return M._sweep(case, flags)


@pytest.mark.gpu
@pytest.mark.parametrize("case", GOLDEN_CASES, ids=case_id)
def test_recorded_bits_are_reproduced(case):
    """dZ of both directions and both bias sums hash to what the parent commit's kernel wrote for the same seeded inputs."""
    want = json.load(open(GOLDEN))["cases"][case_id(case)]
    assert result_bits(swept(case)) == want, case


@pytest.mark.gpu
@pytest.mark.parametrize("case", GOLDEN_CASES, ids=case_id)
def test_short_sweeps_match_the_reference(case):
    """the same sweeps against the float64 reference at rnn_seq_ref.BOUNDS"""
    M._check_against_reference(case, swept(case), M.case_reference(case), "bwd-ring")


def _ring_case(T):
    return (1, 256, 9, T, 0, 0, 4, "FWD_HW8", 8, "BWD_KS8", 8, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [M.MODE_CHUNKS, M.MODE_CHUNKS | M.MODE_PROGRESS], ids=["CH", "CH_PG"])
@pytest.mark.parametrize("chunk_rows", [1, 2])
@pytest.mark.parametrize("T", [3, 4, 5, 6])
def test_chunk_boundaries_at_every_distance_give_the_plain_bits(T, chunk_rows, mode):
    """BWD_KS8_CH / BWD_KS8_CH_PG with every chunk flagged before the launch and chunks of one and two frames, so that a chunk boundary lies
    between the step being computed and each of the steps whose operands are in flight: the bits of BWD_KS8; progress ends at T."""
    from las import _hip
    case = _ring_case(T)
    cell, H, B = case[:3]
    kern = "BWD_KS8_CH_PG" if mode & M.MODE_PROGRESS else "BWD_KS8_CH"
    assert _hip.rnn_seq_plan_kernel(cell, 1, B, H, 0, True, mode)[:3] == (kern, 4, 8)
    assert _hip.rnn_seq_bwd_chunks_ok(cell, 1, B, H, 0)
    base = swept(case)
    flag = torch.full((1,), 1000, dtype=torch.int32, device="cuda")
    kw = dict(chunk_flag=flag, chunk_rows=chunk_rows, n_rows=T)
    prog = None
    if mode & M.MODE_PROGRESS:
        prog = torch.zeros(_hip.rnn_seq_bwd_progress_words(cell, 1, B, H, 0), dtype=torch.int32, device="cuda")
        kw.update(progress=prog, progress_steps=2)
    got = M._sweep(case, 0, bwd_kw=kw)
    M._same_bits(base, got)
    for d in range(2):
        assert torch.equal(base["db"][d], got["db"][d]), d
    if prog is not None:
        assert int(prog.min()) == T and int(prog.max()) == T


@pytest.mark.gpu
def test_a_late_producer_is_waited_for_frame_by_frame():
    """The upstream gradient arrives in chunks of two frames from both ends of the sequence, written by another stream WHILE the sweep runs
    (frames not yet delivered hold NaN).  The producer never waits for the sweep; the sweep's wait is bounded (a.spin).  dZ and the bias
    sums are the bits of BWD_KS8 over the complete gradient and the status word stays clean."""
    from las import _hip
    case = _ring_case(12)
    cell, H, B, T = case[:4]
    c, GH = 2, 4 * H
    base = swept(case)
    xp, whh, R = M.case_inputs(case)
    bf = torch.bfloat16
    gates = xp.cuda().to(bf).contiguous()
    w0, w1 = whh[0].cuda(), whh[1].cuda()
    Tp = T + 1
    out = torch.zeros(B, Tp, 2 * H, device="cuda", dtype=bf)
    cst = torch.zeros(B, T, 2, H, device="cuda", dtype=bf)
    _hip.rnn_seq_fwd(cell, 1, B, T, H, gates, w0, w1, GH, out, 2 * H, Tp * 2 * H, cst)
    dfull = torch.zeros(B, Tp, 2 * H, device="cuda", dtype=bf)
    dfull[:, :T] = R.cuda().to(bf)
    dout = torch.full_like(dfull, float("nan"))
    dout[:, T:] = 0
    th = (T + 1) // 2
    nch = (th + c - 1) // c
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()

    def put(k):
        lo0, lo1 = k * c, min((k + 1) * c, th)
        hi0, hi1 = max(T - lo1, lo1), T - lo0
        dout[:, lo0:lo1] = dfull[:, lo0:lo1]
        dout[:, hi0:hi1] = dfull[:, hi0:hi1]
        if k:
            _hip.set_word(flag, k + 1)

    put(0)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for k in range(1, nch):
            torch.cuda._sleep(400000)
            put(k)
    db = [torch.full((GH,), v, device="cuda") for v in RR.DB_INIT]
    _hip.rnn_seq_bwd(cell, 1, B, T, H, gates, w0, w1, GH, out, 2 * H, Tp * 2 * H, cst, dout, 2 * H, Tp * 2 * H, db_fw=db[0], db_bw=db[1],
                     chunk_flag=flag, chunk_rows=c, n_rows=T)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    _hip.check_status()
    assert torch.equal(gates.cpu(), base["dz"])
    for d in range(2):
        assert torch.equal(db[d].cpu().double() - RR.DB_INIT[d], base["db"][d]), d
