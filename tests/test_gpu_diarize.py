"""las_bic_change and las_bic_cluster (include/las_hip.h K17, csrc/diarize.hip) against the numpy restatement tests/diarize_ref.py.

Values (v, dist, merge_val) are compared with |got - ref| <= TOL (1 + |ref|).  The largest such ratio measured on an MI355X over this
file's inputs is MEASURED below; TOL is 16 times it (another summation order, FMA contraction).  Decisions (peak flags, merge pairs,
labels, counts) are compared for equality; every decision of the restatement on these inputs keeps a margin of MARGIN (1 + |value|) --
asserted here on the restatement alone, before the device is asked -- so TOL sits more than 100 times under the margin.  The exact
ties are built from identical bits and left to the index rule."""
import ctypes
import functools

import numpy as np
import pytest

import helpers  # noqa: F401
import diarize_ref as R

pytestmark = pytest.mark.gpu

MEASURED = 4.479e-11    # the largest ratio on an MI355X over this file's inputs (v at D = 20, w = 2, hop = 1, masked)
TOL = 16 * MEASURED     # 7.17e-10: more than a million times under MARGIN
MARGIN = 1e-3
FLOOR = 1e-4
SENT_I, SENT_B = -77, 0x5A
LAST_RATIO = {"max": 0.0}                                                 # the largest |got - ref| / (1 + |ref|) this process has seen


def _close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    inf = ~np.isfinite(ref)
    assert np.array_equal(got[inf], ref[inf]), what                       # (-inf under nmin: the same on both sides)
    if (~inf).any():
        ratio = float(np.max(np.abs(got[~inf] - ref[~inf]) / (1 + np.abs(ref[~inf]))))
        LAST_RATIO["max"] = max(LAST_RATIO["max"], ratio)
        print("ratio %-40s %.3e" % (what, ratio))
        assert ratio <= TOL, (what, ratio)


# ---- the change curve ---------------------------------------------------------------------------------------------------------------------
CHANGE_CASES = [(D, w, hop, masked) for D in (1, 13, 20) for w in (2, 20) for hop in (1, 7) for masked in (False, True)]
CHANGE_LAMBDA = {2: 0.2, 20: 1.0}                                         # w -> lambda (two frames a side only peak under a small penalty)
CHANGE_SEED = {(1, 2, 1, False): 1, (1, 2, 1, True): 18, (1, 2, 7, False): 3, (1, 20, 1, False): 1, (13, 2, 1, False): 41, (13, 2, 1, True): 98,
               (13, 2, 7, False): 1, (20, 2, 1, False): 142, (20, 2, 1, True): 1, (20, 2, 7, False): 2, (20, 20, 1, True): 1}   # case -> seed offset


@functools.lru_cache(maxsize=None)
def change_input(D, w, hop, masked):
    """-> (feat [N, ld] with NaN in every column >= D and in every row outside the sequences, mask or None, seq_off, seq_len, nmin).
    Sequences of 2w - 1 (no candidate), 2w (one), 2w + hop - 1, 2w + hop and 257 frames in two 'recordings' (the curve knows none),
    gaps of NaN rows between them.  The seeds are chosen (on the CPU) so that the restatement meets MARGIN on every case.  The
    frames: Gaussian 'voices' that change every 40-90 frames (real peaks), column 0 with mean -300, a stretch of constant frames in
    the long sequence.  The mask: random, with a stretch of zeros longer than a window."""
    rng = np.random.RandomState(1000 * D + 10 * w + hop + (5 if masked else 0) + 100000 * CHANGE_SEED.get((D, w, hop, masked), 0))
    lens = [2 * w - 1, 2 * w, 257, 2 * w + hop - 1, 2 * w + hop, 257]
    ld = D + 3
    rows, seq_off, pos = [], [], 2
    rows.append(np.full((2, ld), np.nan, np.float32))
    for n in lens:
        x = np.full((n, ld), np.nan, np.float32)
        t = 0
        while t < n:
            m = rng.randint(40, 90)
            A = rng.randn(D, D) * 0.4 + np.eye(D)
            x[t:t + m, :D] = (rng.randn(len(x[t:t + m]), D) @ A.T + rng.randn(D) * 1.5).astype(np.float32)
            t += m
        x[:, 0] -= 300.0
        if n == 257:
            x[120:150, :D] = x[120, :D]                                   # constant frames: the floor keeps them regular
        seq_off.append(pos)
        rows.append(x)
        pos += n
        gap = rng.randint(1, 4)
        rows.append(np.full((gap, ld), np.nan, np.float32))
        pos += gap
    feat = np.concatenate(rows)
    mask = None
    if masked:
        mask = (rng.rand(len(feat)) < 0.8).astype(np.uint8)
        o = seq_off[2]
        mask[o + 60:o + 60 + w + 3] = 0                                   # a window side under nmin
        mask[o + 200:o + 203] = 7                                         # (any non-zero value counts)
    return feat, mask, seq_off, lens, max(1, (w + 1) // 2)


@functools.lru_cache(maxsize=None)
def change_reference(D, w, hop, masked):
    feat, mask, seq_off, lens, nmin = change_input(D, w, hop, masked)
    R_ = -(-w // hop)
    vs = [R.change_curve(feat, mask, o, n, D, w, hop, nmin, CHANGE_LAMBDA[w], FLOOR) for o, n in zip(seq_off, lens)]
    return vs, [R.peaks(v, R_) for v in vs], min([R.peak_margin(v, R_) for v in vs if len(v)])


def _launch_change(feat, mask, seq_off, lens, D, w, hop, nmin, lam=None, floor=FLOOR, tail=5):
    import torch
    from las import _hip
    lib = _hip.lib()
    S = len(lens)
    lam = CHANGE_LAMBDA.get(w, 1.0) if lam is None else lam
    counts = [int(lib.las_bic_candidates(n, w, hop)) for n in lens]
    assert w < 1 or hop < 1 or counts == [R.candidates(n, w, hop) for n in lens]
    counts = [max(c, 0) for c in counts]
    cand_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    total = int(cand_off[-1])
    d_feat = torch.from_numpy(feat).cuda()
    d_mask = None if mask is None else torch.from_numpy(mask).cuda()
    d_off = torch.tensor(seq_off, dtype=torch.int32, device="cuda")
    d_cand = torch.from_numpy(cand_off).cuda()
    v = torch.full((total + tail,), -12345.5, dtype=torch.float64, device="cuda")
    peak = torch.full((total + tail,), SENT_B, dtype=torch.uint8, device="cuda")
    rc = lib.las_bic_change(_hip.p(d_feat), feat.shape[0], feat.shape[1], D, _hip.p(d_mask), _hip.p(d_off), _hip.p(d_cand),
                            (ctypes.c_int * S)(*seq_off), (ctypes.c_int * S)(*lens), S, w, hop, nmin, lam, floor, _hip.p(v), _hip.p(peak),
                            _hip.stream())
    torch.cuda.synchronize()
    return rc, v.cpu().numpy(), peak.cpu().numpy(), cand_off


@pytest.mark.parametrize("D,w,hop,masked", CHANGE_CASES, ids=["D%d-w%d-hop%d-%s" % (c[0], c[1], c[2], "mask" if c[3] else "nomask") for c in CHANGE_CASES])
def test_change_curve(D, w, hop, masked):
    from las import _hip
    feat, mask, seq_off, lens, nmin = change_input(D, w, hop, masked)
    vs, flags, margin = change_reference(D, w, hop, masked)
    assert margin >= MARGIN, margin                                       # the restatement's own decisions are not close calls
    assert [len(v) for v in vs[:2]] == [0, 1] and len(vs[3]) == 1 and len(vs[4]) == 2
    assert sum(int(f.sum()) for f in flags) >= 2                          # the curves do hold peaks
    if masked:
        assert np.isinf(vs[2]).any() and np.isfinite(vs[2]).any()         # a window under nmin, next to windows that count
    rc, v, peak, cand_off = _launch_change(feat, mask, seq_off, lens, D, w, hop, nmin)
    assert rc == 0, _hip.lib().las_last_error()
    total = cand_off[-1]
    assert (v[total:] == -12345.5).all() and (peak[total:] == SENT_B).all()      # nothing behind the last candidate is written
    _close(v[:total], np.concatenate(vs), "v D=%d w=%d hop=%d" % (D, w, hop))
    assert np.array_equal(peak[:total], np.concatenate(flags))
    # a sequence alone gives the bits it gives in the call, and two calls give the same bits
    rc, v2, peak2, _ = _launch_change(feat, mask, seq_off, lens, D, w, hop, nmin)
    assert rc == 0 and np.array_equal(v2.view(np.int64), v.view(np.int64)) and np.array_equal(peak2, peak)
    rc, v1, peak1, c1 = _launch_change(feat, mask, seq_off[5:], lens[5:], D, w, hop, nmin)
    assert rc == 0 and np.array_equal(v1[:c1[-1]].view(np.int64), v[cand_off[5]:total].view(np.int64))
    assert np.array_equal(peak1[:c1[-1]], peak[cand_off[5]:total])


def test_change_refusals():
    from las import _hip
    feat, mask, seq_off, lens, nmin = change_input(13, 20, 7, False)
    for kw, msg in ((dict(w=1), b"w=1"), (dict(hop=0), b"hop=0"), (dict(nmin=0), b"nmin=0"), (dict(D=21), b"D=21"), (dict(floor=-1.0), b"floor"),
                    (dict(lens=lens[:5] + [9999]), b"sequence 5")):
        a = dict(feat=feat, mask=mask, seq_off=seq_off, lens=lens, D=13, w=20, hop=7, nmin=nmin)
        a.update(kw)
        rc, v, peak, cand_off = _launch_change(**a)
        assert rc < 0 and msg in _hip.lib().las_last_error(), (kw, _hip.lib().las_last_error())
        assert (v == -12345.5).all() and (peak == SENT_B).all()


# ---- the clustering -----------------------------------------------------------------------------------------------------------------------
CLUSTER_SHAPES = {1: (13, 11, 4), 2: (20, 12, 4), 5: (13, 11, 4), 33: (13, 16, 4), 70: (13, 46, 8)}          # S -> (D, seed, voices)


@functools.lru_cache(maxsize=None)
def cluster_input(S, tie=False):
    """-> (feat [N, ld], mask, seq_off, seq_len, D): S units of 2 D + 5 .. 160 frames drawn from four (S = 70: eight) Gaussian 'voices', NaN between
    the units and behind column D, a random mask over the even units (every unit keeps D + 2 masked frames).  tie: three units of
    identical bits in front (S = 3)."""
    D, seed, nv = CLUSTER_SHAPES.get(S, (5, 16, 4))
    rng = np.random.RandomState(seed)                                     # (seeds chosen on the CPU: the restatement meets MARGIN)
    ld = D + 2
    voices = [(rng.randn(D) * 1.2, rng.randn(D, D) * 0.35 + np.eye(D)) for _ in range(nv)]
    rows, seq_off, lens, pos = [np.full((1, ld), np.nan, np.float32)], [], [], 1
    first = None
    for s in range(S):
        n = int(rng.randint(2 * D + 5, 160))
        mu, A = voices[rng.randint(nv)]
        x = np.full((n, ld), np.nan, np.float32)
        x[:, :D] = (rng.randn(n, D) @ A.T + mu).astype(np.float32)
        if tie:
            first = x if first is None else first
            x = first.copy()
        seq_off.append(pos)
        lens.append(len(x))
        rows += [x, np.full((1, ld), np.nan, np.float32)]
        pos += len(x) + 1
    feat = np.concatenate(rows)
    mask = np.ones(len(feat), np.uint8)
    if not tie:
        for s in range(0, S, 2):
            m = (rng.rand(lens[s]) < 0.7).astype(np.uint8)
            m[:D + 2] = 1
            mask[seq_off[s]:seq_off[s] + lens[s]] = m
    return feat, mask, seq_off, lens, D


@functools.lru_cache(maxsize=None)
def cluster_reference(S, K, tie=False):
    feat, mask, seq_off, lens, D = cluster_input(S, tie)
    units = [R.stats(feat, mask, o, o + n, D) for o, n in zip(seq_off, lens)]
    return R.cluster(units, K, 1.0, FLOOR)


def _launch_cluster(feat, mask, seq_off, lens, D, rec_off, K, n_masked=None, lam=1.0, floor=FLOOR, want=True):
    import torch
    from las import _hip
    lib = _hip.lib()
    S, n_rec = len(lens), len(rec_off) - 1
    Smax = max(1, min(max(np.diff(rec_off)), 1024))
    if n_masked is None and mask is not None:
        n_masked = [int((mask[o:o + n] != 0).sum()) for o, n in zip(seq_off, lens)]
    n_masked = None if n_masked is False else n_masked                    # (False: a mask without its host counts)
    ci = lambda xs: None if xs is None else (ctypes.c_int * len(xs))(*[int(x) for x in xs])
    dev = lambda xs: torch.tensor([int(x) for x in xs], dtype=torch.int32, device="cuda")
    d_feat = torch.from_numpy(feat).cuda()
    d_mask = None if mask is None else torch.from_numpy(mask).cuda()
    d_off, d_len, d_rec = dev(seq_off), dev(lens), dev(rec_off)
    label = torch.full((S,), SENT_I, dtype=torch.int32, device="cuda")
    ncl = torch.full((n_rec,), SENT_I, dtype=torch.int32, device="cuda")
    dist = torch.full((S, Smax), float("nan"), dtype=torch.float64, device="cuda") if want else None
    merges = torch.full((S, 2), SENT_I, dtype=torch.int32, device="cuda") if want else None
    mval = torch.full((S,), float("nan"), dtype=torch.float64, device="cuda") if want else None
    nm = torch.full((n_rec,), SENT_I, dtype=torch.int32, device="cuda") if want else None
    nbytes = int(lib.las_bic_cluster_workspace_bytes(min(S, 1 << 20), Smax, D)) or 256
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    rc = lib.las_bic_cluster(_hip.p(d_feat), feat.shape[0], feat.shape[1], D, _hip.p(d_mask), _hip.p(d_off), _hip.p(d_len), _hip.p(d_rec),
                             ci(seq_off), ci(lens), ci(n_masked), S, ci(rec_off), n_rec, K, lam, floor, _hip.p(label), _hip.p(ncl), _hip.p(dist),
                             _hip.p(merges), _hip.p(mval), _hip.p(nm), _hip.p(ws), nbytes, _hip.stream())
    torch.cuda.synchronize()
    c = lambda t: None if t is None else t.cpu().numpy()
    return rc, dict(label=c(label), n_clusters=c(ncl), dist=c(dist), merges=c(merges), merge_val=c(mval), n_merges=c(nm))


def _check_recording(out, ref, base, rc_index, Sr, what):
    """recording rc_index = the units [base, base + Sr) of the call `out` against its restatement"""
    assert out["label"][base:base + Sr].tolist() == ref.label, what
    assert out["n_clusters"][rc_index] == ref.n_clusters and out["n_merges"][rc_index] == len(ref.merges), what
    row0 = base - rc_index
    assert out["merges"][row0:row0 + len(ref.merges)].tolist() == [list(m) for m in ref.merges], what
    assert (out["merges"][row0 + len(ref.merges):row0 + Sr - 1] == SENT_I).all() and np.isnan(out["merge_val"][row0 + len(ref.merges):row0 + Sr - 1]).all()
    if ref.merges:
        _close(out["merge_val"][row0:row0 + len(ref.merges)], ref.merge_val, "merge_val " + what)
    d = out["dist"][base:base + Sr, :Sr]
    upper = np.triu(np.ones((Sr, Sr), bool), 1)
    assert np.isnan(d[~upper]).all(), what                                # only i < j is written
    if Sr > 1:
        _close(d[upper], ref.dist[upper], "dist " + what)


@pytest.mark.parametrize("K", [0, 1, 3])
@pytest.mark.parametrize("S", [1, 2, 5, 33, 70])
def test_cluster(S, K):
    from las import _hip
    feat, mask, seq_off, lens, D = cluster_input(S)
    ref = cluster_reference(S, K)
    assert ref.margin >= MARGIN, ref.margin
    if S >= 33 and K == 0:
        assert 2 <= ref.n_clusters <= 12 and len(ref.merges) >= S - 12    # the loop really runs, and really stops on the sign
    rc, out = _launch_cluster(feat, mask, seq_off, lens, D, [0, S], K)
    assert rc == 0, _hip.lib().las_last_error()
    _check_recording(out, ref, 0, 0, S, "S=%d K=%d" % (S, K))
    rc, again = _launch_cluster(feat, mask, seq_off, lens, D, [0, S], K)
    assert rc == 0
    for k in out:                                                         # two calls give the same bits
        assert np.array_equal(out[k].view(np.int64) if out[k].dtype == np.float64 else out[k],
                              again[k].view(np.int64) if again[k].dtype == np.float64 else again[k]), k
    rc, bare = _launch_cluster(feat, mask, seq_off, lens, D, [0, S], K, want=False)      # the optional outputs left out
    assert rc == 0 and np.array_equal(bare["label"], out["label"]) and np.array_equal(bare["n_clusters"], out["n_clusters"])


def test_cluster_identical_units_tie():
    feat, mask, seq_off, lens, D = cluster_input(3, tie=True)
    ref = cluster_reference(3, 0, tie=True)
    assert ref.merges == [(0, 1), (0, 2)] and ref.dist[0, 1] == ref.dist[0, 2] == ref.dist[1, 2]
    rc, out = _launch_cluster(feat, None, seq_off, lens, D, [0, 3], 0)
    assert rc == 0
    _check_recording(out, ref, 0, 0, 3, "tie")
    d = out["dist"]
    assert d[0, 1] == d[0, 2] == d[1, 2]                                  # identical bits in, identical bits out


def test_cluster_batch_of_two_recordings_gives_each_its_own_bits():
    a, b = cluster_input(33), cluster_input(5)
    Da = a[4]
    assert Da == b[4]
    feat = np.concatenate([a[0], b[0]])
    mask = np.concatenate([a[1], b[1]])
    seq_off = list(a[2]) + [o + len(a[0]) for o in b[2]]
    lens = list(a[3]) + list(b[3])
    rc, both = _launch_cluster(feat, mask, seq_off, lens, Da, [0, 33, 38], 0)
    assert rc == 0
    _check_recording(both, cluster_reference(33, 0), 0, 0, 33, "batch/33")
    _check_recording(both, cluster_reference(5, 0), 33, 1, 5, "batch/5")
    for (inp, base, r, Sr) in ((a, 0, 0, 33), (b, 33, 1, 5)):
        rc, alone = _launch_cluster(inp[0], inp[1], inp[2], inp[3], Da, [0, Sr], 0)
        assert rc == 0
        bits = lambda x: x.view(np.int64)
        assert np.array_equal(alone["label"], both["label"][base:base + Sr]) and alone["n_clusters"][0] == both["n_clusters"][r]
        assert alone["n_merges"][0] == both["n_merges"][r]
        m = alone["n_merges"][0]
        assert np.array_equal(alone["merges"][:m], both["merges"][base - r:base - r + m])
        assert np.array_equal(bits(alone["merge_val"][:m]), bits(both["merge_val"][base - r:base - r + m]))
        up = np.triu(np.ones((Sr, Sr), bool), 1)
        assert np.array_equal(bits(alone["dist"][:, :Sr][up]), bits(both["dist"][base:base + Sr, :Sr][up]))


def _untouched(out):
    return all((out[k] == SENT_I).all() for k in ("label", "n_clusters", "merges", "n_merges")) and \
        np.isnan(out["dist"]).all() and np.isnan(out["merge_val"]).all()


def test_cluster_refusals_leave_the_outputs_alone():
    from las import _hip
    lib = _hip.lib()
    feat, mask, seq_off, lens, D = cluster_input(5)
    empty = mask.copy()
    empty[seq_off[3]:seq_off[3] + lens[3]] = 0                            # a unit with no masked frame
    rc, out = _launch_cluster(feat, empty, seq_off, lens, D, [0, 5], 0)
    assert rc < 0 and b"unit 3 has 0 masked frames" in lib.las_last_error() and _untouched(out)
    rc, out = _launch_cluster(feat, mask, seq_off, lens, D, [0, 5], 0, n_masked=False)          # a mask without the host counts
    assert rc < 0 and b"n_masked_host" in lib.las_last_error() and _untouched(out)
    rc, out = _launch_cluster(feat, mask, seq_off, lens, D, [0, 5], -1)
    assert rc < 0 and b"K=-1" in lib.las_last_error() and _untouched(out)
    rc, out = _launch_cluster(feat, mask, seq_off, lens[:4] + [0], D, [0, 5], 0)
    assert rc < 0 and b"sequence 4" in lib.las_last_error() and _untouched(out)
    # 1025 units in one recording: an error, not a fault
    many = np.random.RandomState(2).randn(1025, 4).astype(np.float32)
    rc, out = _launch_cluster(many, None, list(range(1025)), [1] * 1025, 3, [0, 1025], 0)
    assert rc < 0 and b"1025 units" in lib.las_last_error() and _untouched(out)
    assert lib.las_bic_cluster_workspace_bytes(1025, 1025, 3) == 0 and lib.las_bic_cluster_workspace_bytes(1024, 1024, 20) > 0
