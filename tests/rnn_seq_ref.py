"""CPU restatement of the speed-mode Listener sweep (csrc/rnn_seq.hip, SWEEP_BF16): the forward sweep and BPTT of ONE direction in
float64, with a rounding to bf16 (round to nearest even, las_common.h:42 f2bf / :48 f2bf2) at exactly the points where the kernels round.
Between two rounding points the arithmetic is float64 here and fp32 on the device.  Gate order i, j, f, o (layers.py:31 BasicLSTMCell).

Rounding points, read off the kernels (file:line of automatic-speech-recognition_amd/csrc/):

  operands as handed over
    x-projection          bf16 in HBM: the caller rounds it; the kernels widen it exactly (rnn_seq.hip:384 BfRef, :664 to_ring)
    upstream gradient     likewise (rnn_seq.hip:993, :1258)
    W_hh                  rounded ONCE when packed into MFMA fragments: rnn_seq.hip:1588 (pack_whh_body: forward and plain BPTT),
                          :1552 (pack_whh_ks_body: K-split BPTT); products accumulate in fp32 (mfma_bf16_16x16x32)
  forward (rnn_seq_fwd_bf16_kernel, rnn_seq_fwd_hw_kernel: the same points in both)
    h_t                   rounded where it is produced, :445 / :880 (hb = f2bf(h)); that ONE bf16 value is what goes into the LDS tile of the
                          next step (:446 / :894), into the partners' granules (:449 / :884) and -- the fp32 copy rounds to the same value --
                          into HBM (:488 BfRef, :743 / :753 pack4)
    c_t                   CARRIED IN fp32 (cst[j][r], :437-438 / :870-873); only the stored copy is rounded (:486, :742).  BPTT reads the
                          stored copy (below), the forward recurrence never does
    activated gates       stored rounded (:484-485, :734-736); fp32 inside the step
    forget bias           added to the f pre-activation in fp32 (:435 / :868)
    ragged rows           at frames t >= row_T[row] c and h are forced to zero BEFORE they are carried / rounded (:872, :877)
  BPTT (rnn_seq_bwd_bf16_kernel = BWD_PLAIN, rnn_seq_bwd_ks_kernel = BWD_KS*)
    saved gates, c_t, c_{t-1}, h_t (tanh cell)   read back from their bf16 stores (:996-1000, :1258-1266): tanh(c_t) is taken of the ROUNDED c
    dh = dout + dh_rec    fp32 (:1017, :1297); the carried dc is fp32 (:1025, :1306)
    dZ                    rounded where it is stored: :1036 (f2bf -> LDS tile, granules, and :1097 the same value to HBM), :1318 (f2bf2 -> LDS
                          tile and :1478 HBM).  The ROUNDED dZ is the operand of dh_rec = dZ . W_hh^T
    dh_rec, K-split       every member multiplies its own gate columns only; the partial sums it computes for units ANOTHER member owns travel
                          as bf16 (:1392 / :1427 f2bf2(acc[mo])), the member's own partial stays fp32 (:1408 / :1459).  With P members a unit's
                          dh_rec is one fp32 partial + (P - 1) bf16-rounded ones.  BWD_PLAIN all-gathers dZ instead: one fp32 sum
    bias sums             BWD_KS*: column sums of the UNROUNDED dZ in fp32 (:1321-1322 bsum, before f2bf2's result is used), per tile into
                          bpart (:1507), summed over tiles -- all row chunks -- and added to db by bias_finish_kernel (:1513-1522).
                          BWD_PLAIN: column sums of the STORED (rounded) dZ, las_colsum_dt behind the sweep (:2103-2109)

sweep_dir(..., dt=torch.float64) is the reference; emulate_fp32 is the same code in torch float32 on the CPU (one rounding per operation,
dot products in whatever order the CPU's BLAS takes), with the device's transcendental forms -- sigmoid_fast / tanh_fast,
las_common.h:92-97: 1 / (1 + exp2(-log2(e) x)) and 1 - 2 / (1 + exp2(2 log2(e) x)) -- because tanh_fast carries an ABSOLUTE error of an fp32
ulp of 1, which tanhf does not.  Where the two disagree by more than fp32 noise a value sat close enough to a bf16 tie that it rounded
the other way: one bf16 ulp of that value, and what follows from it.  That, not fp32 noise, is what the bounds below measure.

BOUNDS (per quantity, in units of max(1, largest |reference| of that quantity in the case) = 4 x MEASURED, the worst distance between
emulate_fp32 and the float64 reference over every case of tests/test_gpu_rnn_seq_matrix.py (MATRIX, CHUNK_CASES, MODE_CASES; both
directions; tests/test_rnn_seq_ref_host.py measures them again and prints them).  The factor 4 covers the kernels' summation order (K in
quarters, members' partials) and v_exp_f32 / v_rcp_f32 (~1 ulp each).  Nothing here comes from a GPU run."""
import torch

LOG2E = 1.4426950408889634

# worst |emulate_fp32 - float64 reference| / max(1, max |reference|) over all matrix cases, per quantity
# (h: a tie in the tanh cell at H = 256 that the recurrence amplifies to 2.6 bf16 ulps of 1; dz, db: the tanh cell at H = 512)
MEASURED = {"h": 0.01025390625, "c": 0.003937007874015748, "dz": 0.007194244604316547, "db": 0.003647327958785617,
            # the bias sums' rounding residual (bias_residual_distance: a median over columns, in absolute units) over the K-split cases with
            # T <= 2, each on its own seed and on RESIDUAL_SEEDS; the worst is the LSTM at H = 128, B = 16, T = 2 on seed 0
            "db_res": 4.6390625766390414e-06}
RESIDUAL_SEEDS = (0, 1, 2, 3, 4)
BOUNDS = {k: 4.0 * v for k, v in MEASURED.items()}

MUTATIONS = ("stale_h", "ragged_row0", "drop_kquarter", "swap_ij", "no_forget_bias", "reverse_off_by_one", "db_last_chunk", "db_after_rounding")


def rb(x):
    """round to bf16 and back (RNE)"""
    return x.to(torch.bfloat16).to(x.dtype)


def _sigmoid(x, fast):
    if fast:
        return torch.reciprocal(1.0 + torch.exp2(-LOG2E * x))
    return torch.sigmoid(x)


def _tanh(x, fast):
    if fast:
        return 1.0 - 2.0 * torch.reciprocal(1.0 + torch.exp2((2.0 * LOG2E) * x))
    return torch.tanh(x)


def mutation_applies(name, cell, B, T, P, rows_per_tile, ksplit, launches):
    """whether a mutation changes anything a sweep of this shape computes (a T = 1 sweep exchanges nothing, ...)"""
    return {"stale_h": P > 1 and T >= 2, "ragged_row0": B % rows_per_tile > 1 and T >= 2, "drop_kquarter": T >= 2,
            "swap_ij": cell == "lstm", "no_forget_bias": cell == "lstm" and T >= 2, "reverse_off_by_one": T >= 2,
            "db_last_chunk": launches > 1, "db_after_rounding": ksplit and T <= 2}[name]


def sweep_dir(xp, whh, dout, cell, reverse, dt=torch.float64, rounding=True, P=1, ksplit=False, forget_bias=1.0, row_T=None,
              rows_per_tile=16, launch_rows=None, fast=False, mutate=None):
    """One direction.  xp [B, T, G H] x-projection, whh [H, G H], dout [B, T, H] upstream gradient (None: forward only).
    P: cluster width; ksplit: BPTT by the K-split kernels (bf16 partials between members, bias sums before the rounding) or the plain one.
    rows_per_tile / launch_rows (rows per row-chunk launch) only place the mutations: rows do not interact.
    -> dict h, c (stored copies, [B, T, H]; c None for the tanh cell), act (saved gates), dz [B, T, G H], db [G H]."""
    B, T, GH = xp.shape
    H = whh.shape[0]
    G = GH // H
    assert G == (4 if cell == "lstm" else 1)
    r = rb if rounding else (lambda v: v)
    xp = r(xp.to(dt))
    W = r(whh.to(dt))
    fb = forget_bias
    swap = mutate == "swap_ij"
    if mutate == "no_forget_bias":
        fb = 0.0
    UPM = H // P
    order = list(range(T - 1, -1, -1) if reverse else range(T))
    src = list(order)
    if mutate == "reverse_off_by_one" and reverse:
        src = [max(t - 1, 0) for t in order]          # the sweep's frame pointer starts one frame early
    rowT = None if row_T is None else torch.as_tensor(row_T).reshape(B, 1)
    hs = [None] * T
    cs = [None] * T
    acts = [None] * T
    h = torch.zeros(B, H, dtype=dt)
    hprev2 = torch.zeros(B, H, dtype=dt)
    c = torch.zeros(B, H, dtype=dt)
    s_bad = min(2, T - 1)                              # the step the one-step mutations strike
    for s, t in enumerate(order):
        hin = h
        if mutate == "stale_h" and s == s_bad:         # member P - 1's slice of h_{s-1} never arrived: the slot still holds h_{s-2}... of two steps ago
            hin = h.clone()
            hin[:, (P - 1) * UPM:] = hprev2[:, (P - 1) * UPM:]
        if mutate == "ragged_row0" and B % rows_per_tile > 1 and s >= 1:
            hin = h.clone()
            hin[B - 1] = h[(B - 1) // rows_per_tile * rows_per_tile]
        rec = hin @ W
        if mutate == "drop_kquarter" and s == s_bad:   # member 0's product without its last K quarter
            cols = torch.arange(GH).reshape(G, H)[:, :UPM].reshape(-1)
            k0 = 3 * H // 4
            rec[:, cols] = rec[:, cols] - hin[:, k0:] @ W[k0:][:, cols]
        pre = xp[:, src[s]] + rec
        if cell == "lstm":
            zi, zj, zf, zo = pre.chunk(4, -1)
            if swap:
                zi, zj = zj, zi
            gi, gj, gf, go = _sigmoid(zi, fast), _tanh(zj, fast), _sigmoid(zf + fb, fast), _sigmoid(zo, fast)
            cn = c * gf + gi * gj
            hn = _tanh(cn, fast) * go
            if rowT is not None:
                live = t < rowT
                cn = torch.where(live, cn, torch.zeros_like(cn))
                hn = torch.where(live, hn, torch.zeros_like(hn))
            c = cn
            cs[t] = r(cn)
            acts[t] = r(torch.cat([gi, gj, gf, go], -1))
        else:
            hn = _tanh(pre, fast)
            if rowT is not None:
                hn = torch.where(t < rowT, hn, torch.zeros_like(hn))
            acts[t] = None
        hprev2 = h
        h = r(hn)
        hs[t] = h
    res = {"h": torch.stack(hs, 1), "c": torch.stack(cs, 1) if cell == "lstm" else None,
           "act": torch.stack(acts, 1) if cell == "lstm" else None, "dz": None, "db": None}
    if dout is None:
        return res
    dout = r(dout.to(dt))
    dzs = [None] * T
    dhr = torch.zeros(B, H, dtype=dt)
    dcc = torch.zeros(B, H, dtype=dt)
    db = torch.zeros(GH, dtype=dt)
    nrows = B
    if mutate == "db_last_chunk" and launch_rows and B > launch_rows:
        nrows = (B - 1) // launch_rows * launch_rows    # bias_finish_kernel stops at the first launch's tiles
    Wt = W.t()                                          # [G H, H]
    zero = torch.zeros(B, H, dtype=dt)
    for s, t in enumerate(reversed(order)):
        tp = t + 1 if reverse else t - 1                # the frame the forward sweep visited before t
        dh = dout[:, t] + dhr
        if cell == "lstm":
            gi, gj, gf, go = res["act"][:, t].chunk(4, -1)
            cprev = res["c"][:, tp] if 0 <= tp < T else zero
            tc = _tanh(res["c"][:, t], fast)
            dc = dcc + dh * go * (1.0 - tc * tc)
            dcc = dc * gf
            dz = torch.cat([dc * gj * gi * (1.0 - gi), dc * gi * (1.0 - gj * gj), dc * cprev * gf * (1.0 - gf), dh * tc * go * (1.0 - go)], -1)
        else:
            hh = res["h"][:, t]
            dz = dh * (1.0 - hh * hh)
        dzr = r(dz)
        dzs[t] = dzr
        db = db + (dzr if (not ksplit or mutate == "db_after_rounding") else dz)[:nrows].sum(0)
        if ksplit and P > 1:
            dhr = torch.zeros(B, H, dtype=dt)
            for m in range(P):                          # member m's gate columns: its K slice
                cols = torch.arange(GH).reshape(G, H)[:, m * UPM:(m + 1) * UPM].reshape(-1)
                part = dzr[:, cols] @ Wt[cols]          # [B, H]: partial dh of ALL units
                own = part[:, m * UPM:(m + 1) * UPM].clone()
                part = r(part)                          # what leaves the member is bf16 ...
                part[:, m * UPM:(m + 1) * UPM] = own    # ... its own tile stays fp32
                dhr = dhr + part
        else:
            dhr = dzr @ Wt
    res["dz"] = torch.stack(dzs, 1)
    res["db"] = db
    return res


def reference(xp, whh, dout, cell, reverse, **kw):
    """the float64 reference with the kernels' rounding points"""
    return sweep_dir(xp, whh, dout, cell, reverse, dt=torch.float64, **kw)


def emulate_fp32(xp, whh, dout, cell, reverse, mutate=None, **kw):
    """the same recurrence in fp32 with the same rounding points and the device's sigmoid / tanh forms; `mutate`: one of MUTATIONS"""
    return sweep_dir(xp, whh, dout, cell, reverse, dt=torch.float32, fast=True, mutate=mutate, **kw)


def distances(got, ref):
    """{quantity: max |got - ref| / max(1, max |ref|)} over h, c, dz, db (those both sides have)"""
    out = {}
    for k in ("h", "c", "dz", "db"):
        if ref.get(k) is None or got.get(k) is None:
            continue
        a, b = got[k].double(), ref[k].double()
        out[k] = (a - b).abs().max().item() / max(1.0, b.abs().max().item())
    return out


DB_INIT = (0.5, -0.25)        # what the matrix cases' bias sums are accumulated onto (forward, backward direction)


def bias_residual(res, init=None):
    """db minus the column sums of the stored (rounded) dZ: what the K-split kernels' bias sums gain by summing BEFORE the rounding.  The max
    norm of db cannot tell the two apart (the residual is at most 2^-9 of sum |dZ|, a tie that rounds the other way moves db by as much), so
    it is a quantity of its own.  It is only comparable while the sweep is short: a tie in h at step s shifts every later dZ of that row
    by ~2^-9 relative, and the rounding errors of those terms are then unrelated to the reference's.
    init: the fp32 value the sums were added to (bias_finish_kernel: db[col] += acc, one fp32 rounding at the magnitude of init + acc) and
    that the caller took off again: the fp32 emulation is given the same."""
    db = res["db"]
    if init is not None:
        db = (torch.tensor(init, dtype=torch.float32) + db.float()).double() - init
    return db.double() - res["dz"].double().sum((0, 1))


def bias_residual_distance(got, ref):
    """MEDIAN over the G H columns of |residual - reference residual|.  Not the maximum: one dZ that sits on a bf16 tie and rounds the other
    way moves its column's residual by a whole bf16 ulp of that dZ -- 2^-9 for a dZ in [0.25, 0.5) -- which is as much as the whole
    residual of a column.  A legitimate fp32 evaluation has a few such columns (the emulation reaches 1.9e-3 and 3.8e-3 in the maximum on
    three of six seeds of the LSTM cases with T = 2, where the seed first measured gave 4.6e-4), a sum taken after the rounding is off in
    every column.  The median is at fp32 noise in the first case (1e-8 to 5e-6; the upper end when a tie at the sweep's first step shifts a
    whole row of the second) and at the size of the residual, 1e-4 to 2e-3, in the second."""
    return (got - ref).abs().median().item()


def make_inputs(cell, B, T, H, seed):
    """The matrix cases' inputs: x-projection ~ 0.8 N(0, 1), W_hh uniform at 1.5 x the Glorot limit, upstream gradient N(0, 1); the
    x-projection and the gradient already rounded to bf16, as the sweeps are handed them.  -> xp [B, T, 2, G H], [whh_fw, whh_bw], R [B, T, 2 H]"""
    G = 4 if cell == "lstm" else 1
    g = torch.Generator().manual_seed(seed)
    xp = (torch.randn(B, T, 2, G * H, generator=g) * 0.8).to(torch.bfloat16).float()
    lim = (6.0 / (H + G * H)) ** 0.5 * 1.5
    whh = [(torch.rand(H, G * H, generator=g) * 2 - 1) * lim for _ in range(2)]
    R = torch.randn(B, T, 2 * H, generator=g).to(torch.bfloat16).float()
    return xp, whh, R
