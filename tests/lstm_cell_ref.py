"""float64 restatement of one las_lstm_cell_rows launch (csrc/loss_opt.hip, csrc/lstm_cell_rows.h), and the case tables of
tests/test_gpu_lstm_cell_rows.py and tests/test_lstm_cell_ref_host.py.

    z  = rnd(x) . rnd(Wx) + rnd(h) . rnd(Wh) + bias  [+ xrows[max(ids - id_shift, 0)]]        rnd = round-to-nearest-even to bf16
    i, j, f, o = the four column blocks of z (TF gate order);  c' = c * sigmoid(f + fb) + sigmoid(i) * tanh(j);  h' = tanh(c') * sigmoid(o)

The tables are plain data and this module imports without touching the device."""
import torch

from las import _hip

TOL_EXACT, TOL_FAST = 2e-5, 2e-3       # tests/test_gpu_lm.py's: expf / tanhf, and the Speller's approximated transcendentals (fast)
V, ID_SHIFT = 28, 2                    # the one-hot first layer: ids 0 .. V + 1, ids below the shift clamp to row 0
GUARD = 128                            # guard rows behind row M of every row buffer
ROWS = 520                             # rows generated per single-launch case
PREFIXES = (5, 33, 127, 128, 256, 257, 512, 513, 520)
PAD = 8                                # ldx = I + PAD, ldh = H + PAD in the padded cases

PAIR, B_BF16, TWO = _hip.LSTM_CELL_PLAN_PAIR, _hip.LSTM_CELL_PLAN_B_BF16, _hip.LSTM_CELL_PLAN_TWO
REFUSED = -1

# the problem forms, as the beam search builds them (x / h: element type of the rows or None; hb: h_out_bf16 is asked for)
FORMS = {
    "S": dict(x="bf16", h=None, onehot=False, fast=1, fb=1.0, gates=True, hb=False),      # the Speller's step
    "L0": dict(x=None, h="f32", onehot=True, fast=0, fb=0.0, gates=False, hb=False),      # the LM's first layer
    "L1": dict(x="f32", h="f32", onehot=False, fast=0, fb=0.0, gates=False, hb=False),    # an upper LM layer
    "L0b": dict(x=None, h="bf16", onehot=True, fast=0, fb=0.0, gates=False, hb=True),     # ... reading / leaving bf16 state copies
    "L1b": dict(x="bf16", h="bf16", onehot=False, fast=0, fb=0.0, gates=False, hb=True),
    "L1x": dict(x="f32", h="f32", onehot=False, fast=0, fb=1.0, gates=True, hb=False),    # the exact path with fb and gates_out
    # first problems of the pair table only
    "Sf": dict(x="f32", h=None, onehot=False, fast=1, fb=1.0, gates=True, hb=False),      # S with fp32 x: no pair kernel
    "Sh": dict(x="bf16", h="bf16", onehot=False, fast=1, fb=1.0, gates=True, hb=True),    # S plus bf16 h and h_out_bf16
}

# plan codes by row prefix: rows per workgroup of the pipelined body, 0 = the unpipelined body, REFUSED
_BY_M = {5: 0, 33: 0, 127: 0, 128: 32, 256: 32, 257: 64, 512: 64, 513: 128, 520: 128}
_BY_M_F32_XH = {**_BY_M, 128: 0, 256: 0}                             # fp32 x AND h at M <= 256 stay unpipelined
_BY_M_BF16 = {**_BY_M, 5: REFUSED, 33: REFUSED, 127: REFUSED}        # bf16 h / h_out_bf16: the pipelined body only
PLAN_BY_PREFIX = {"S": _BY_M, "L0": _BY_M, "L1": _BY_M_F32_XH, "L1x": _BY_M_F32_XH, "L0b": _BY_M_BF16, "L1b": _BY_M_BF16}

# (form, I, H, padded rows).  (544, 96): the unpipelined body's x chunks 512 + 32, the pipelined body's 4 x 128 + 32 and a 96-column h
# chunk (six chunks); (160, 64): 128 + 32 and 64, three chunks -- the pipelined body's trailing half runs empty; (288, 64) for S: three
# chunks; H alone for the one-hot forms: one chunk, at H = 32 one K step
SINGLE_CASES = [
    ("S", 544, 96, True), ("S", 160, 64, False), ("S", 288, 64, True),
    ("L0", 0, 96, False), ("L0", 0, 32, True),
    ("L1", 544, 96, False), ("L1", 160, 64, True),
    ("L0b", 0, 96, True), ("L0b", 0, 32, False),
    ("L1b", 544, 96, True), ("L1b", 160, 64, False),
    ("L1x", 544, 96, False), ("L1x", 160, 64, True),
]

# ((form, M, I, H) of a, (form, M, H) of b, plan code, padded rows, what the row is for)
PAIR_CASES = [
    (("S", 40, 160, 64), ("L0", 40, 96), PAIR, False, "unpipelined pair, b wider"),
    (("S", 40, 160, 96), ("L0", 40, 64), PAIR, True, "unpipelined pair, a wider"),
    (("S", 70, 160, 64), ("L0", 33, 64), PAIR, False, "unpipelined pair, a taller"),
    (("S", 33, 160, 64), ("L0", 70, 64), PAIR, True, "unpipelined pair, b taller"),
    (("S", 200, 288, 64), ("L0", 200, 96), PAIR | 32, False, "pipelined pair, 32 rows, fp32 second problem, ragged"),
    (("S", 200, 288, 64), ("L0b", 200, 96), PAIR | 32 | B_BF16, True, "pipelined pair, 32 rows, bf16 second problem"),
    (("S", 300, 160, 96), ("L0b", 300, 64), PAIR | 64 | B_BF16, False, "pipelined pair, 64 rows, ragged"),
    (("S", 513, 160, 64), ("L0", 513, 96), PAIR | 64, True, "pipelined pair, 64 rows, one ragged row"),
    (("S", 300, 160, 64), ("L0", 200, 64), PAIR | 64, False, "pipelined pair, 64 rows by the larger M"),
    (("S", 200, 160, 64), ("L0", 64, 64), PAIR, True, "unpipelined pair (b below 128 rows)"),
    (("L1", 200, 160, 64), ("L0", 200, 64), TWO, False, "two launches: a not fast"),
    (("Sf", 200, 160, 64), ("L0", 200, 64), TWO, True, "two launches: a's x fp32"),
    (("Sh", 200, 160, 64), ("L0", 64, 64), TWO, False, "two launches: bf16 h / h_out_bf16 never reach the unpipelined pair kernel"),
]
PAIR_REF_CASE = 4                      # the pair case that is also held to lstm_cell_ref, both problems

# arguments every launch and the query refuse
REFUSALS = ("x_and_xrows", "xrows_without_ids", "I_not_32", "H_not_32", "ldh_not_8_bf16_h", "mixed_rows_h_bf16", "null_struct")

# every value the dispatch decision returns in a shipping build.  (PAIR | 128 exists only behind the development switch
# LAS_DEV_LB_PAIR_ROWS, which the shipping library does not export: not reachable, not in the tables.)
SHIPPING_PLAN_CODES = {REFUSED, 0, 32, 64, 128, PAIR, PAIR | 32, PAIR | 32 | B_BF16, PAIR | 64, PAIR | 64 | B_BF16, TWO}


def tol(form):
    return TOL_FAST if FORMS[form]["fast"] else TOL_EXACT


def rnd(t):
    """round to nearest even to bf16, back in fp32"""
    return t.to(torch.bfloat16).to(torch.float32)


def make_problem(form, M, I, H, seed=None):
    """CPU operands of one problem: N(0, 1) rows, N(0, 0.08^2) weights, N(0, 0.1^2) bias.  The draws depend on the geometry and on which
    parts the form has, not on its element types: L0 / L0b and L1 / L1b / L1x see the same numbers."""
    f = FORMS[form]
    g = torch.Generator(device="cpu").manual_seed(1000 * I + H if seed is None else seed)
    p = dict(form=form, M=M, I=I, H=H)
    p["bias"] = torch.randn(4 * H, generator=g) * 0.1
    p["c_prev"] = torch.randn(M, H, generator=g)
    p["x"] = torch.randn(M, I, generator=g) if f["x"] else None
    p["Wx"] = torch.randn(I, 4 * H, generator=g) * 0.08 if f["x"] else None
    p["h"] = torch.randn(M, H, generator=g) if f["h"] else None
    p["Wh"] = torch.randn(H, 4 * H, generator=g) * 0.08 if f["h"] else None
    if f["onehot"]:
        p["xrows"] = torch.randn(V, 4 * H, generator=g) * 0.08         # fp32 rows: the kernel looks them up without rounding
        ids = torch.randint(0, V + ID_SHIFT, (M,), generator=g).to(torch.int32)
        ids[0], ids[1], ids[2], ids[M - 1] = 0, 1, V + 1, V + 1         # both clamped ids and the last row, in every prefix
        p["ids"] = ids
    else:
        p["xrows"] = p["ids"] = None
    return p


MUTATIONS = ("drop_last_kstep_x", "drop_last_kstep_h", "h_first_kstep_from_x", "swap_j_f", "no_fb", "id_shift_plus_one",
             "last_row_from_row_before", "h_rows_at_ld_H")


def mutation_applies(mutate, form, padded):
    f = FORMS[form]
    return {"drop_last_kstep_x": bool(f["x"]), "drop_last_kstep_h": bool(f["h"]), "h_first_kstep_from_x": bool(f["x"] and f["h"]),
            "swap_j_f": True, "no_fb": f["fb"] != 0.0, "id_shift_plus_one": f["onehot"], "last_row_from_row_before": True,
            "h_rows_at_ld_H": bool(f["h"]) and padded}[mutate]


def lstm_cell_ref(p, M=None, mutate=None):
    """float64 c', h', activated gates [M, 4H] and h' rounded to bf16 of the first M rows of problem p.  mutate: one planted error of
    MUTATIONS (what a wrong kernel could compute), for the host test's sensitivity check."""
    f = FORMS[p["form"]]
    M = p["M"] if M is None else M
    H, I = p["H"], p["I"]
    c_prev = p["c_prev"][:M].double()
    x = rnd(p["x"][:M]).double() if f["x"] else None
    h = rnd(p["h"][:M]).double() if f["h"] else None
    ids = p["ids"][:M].long() if f["onehot"] else None
    if mutate == "h_rows_at_ld_H":        # row r read at r * H of the padded buffer [M, H + PAD] (padding counted as 0 here; the tests fill it with NaN)
        flat = torch.cat([h, torch.zeros(M, PAD, dtype=torch.float64)], 1).reshape(-1)
        h = flat[:M * H].reshape(M, H)
    if mutate == "h_first_kstep_from_x":
        h = torch.cat([x[:, :32], h[:, 32:]], 1)
    if mutate == "last_row_from_row_before":
        def shift_last(t):
            t = t.clone()
            t[M - 1] = t[M - 2]
            return t
        c_prev, x, h, ids = (None if t is None else shift_last(t) for t in (c_prev, x, h, ids))
    z = p["bias"].double().expand(M, 4 * H).clone()
    if x is not None:
        W = rnd(p["Wx"]).double()
        z += x[:, :I - 32] @ W[:I - 32] if mutate == "drop_last_kstep_x" else x @ W
    if h is not None:
        W = rnd(p["Wh"]).double()
        z += h[:, :H - 32] @ W[:H - 32] if mutate == "drop_last_kstep_h" else h @ W
    if ids is not None:
        shift = ID_SHIFT + (1 if mutate == "id_shift_plus_one" else 0)
        z += p["xrows"].double().index_select(0, (ids - shift).clamp_min(0))
    i, j, fg, o = z.split(H, 1)
    if mutate == "swap_j_f":
        j, fg = fg, j
    gi, gj, gf, go = torch.sigmoid(i), torch.tanh(j), torch.sigmoid(fg + (0.0 if mutate == "no_fb" else f["fb"])), torch.sigmoid(o)
    c = c_prev * gf + gi * gj
    hn = torch.tanh(c) * go
    return dict(c=c, h=hn, gates=torch.cat([gi, gj, gf, go], 1), h_bf16=hn.to(torch.float32).to(torch.bfloat16))


def fill_args(form, M, I, H, ldx, ldh, ptr):
    """las_lstm_cell_args of a problem over the addresses ptr[name] (x, h, Wx, Wh, bias, c_prev, ids, xrows, c_out, h_out, gates_out,
    h_out_bf16): device pointers on the GPU, any 16-byte aligned numbers for the plan query, which dereferences none"""
    f = FORMS[form]
    a = _hip.LstmCellArgs()
    if f["x"]:
        a.x, a.x_bf16, a.ldx, a.I, a.Wx = ptr["x"], int(f["x"] == "bf16"), ldx, I, ptr["Wx"]
    if f["h"]:
        a.h, a.h_bf16, a.ldh, a.Wh = ptr["h"], int(f["h"] == "bf16"), ldh, ptr["Wh"]
    if f["onehot"]:
        a.ids, a.id_shift, a.xrows = ptr["ids"], ID_SHIFT, ptr["xrows"]
    a.bias, a.c_prev, a.fb = ptr["bias"], ptr["c_prev"], f["fb"]
    a.c_out, a.h_out, a.M, a.H, a.fast = ptr["c_out"], ptr["h_out"], M, H, f["fast"]
    a.gates_out = ptr["gates_out"] if f["gates"] else None
    a.h_out_bf16 = ptr["h_out_bf16"] if f["hb"] else None
    return a


FAKE_PTRS = {n: 0x10000 * (k + 1) for k, n in enumerate(("x", "h", "Wx", "Wh", "bias", "c_prev", "ids", "xrows", "c_out", "h_out", "gates_out",
                                                          "h_out_bf16"))}


def refusal_args(name, ptr, M=200, I=160, H=64):
    """the arguments of REFUSALS[name] over ptr (None: the NULL struct): an L1 / L1b problem with one thing wrong"""
    if name == "null_struct":
        return None
    form = "L1b" if name == "ldh_not_8_bf16_h" else "L1"
    a = fill_args(form, M, I, H, I, H, ptr)
    if name == "x_and_xrows":
        a.ids, a.id_shift, a.xrows = ptr["ids"], ID_SHIFT, ptr["xrows"]
    elif name == "xrows_without_ids":
        a.x, a.Wx, a.I, a.ldx, a.xrows = None, None, 0, 0, ptr["xrows"]
    elif name == "I_not_32":
        a.I = I - 16
    elif name == "H_not_32":
        a.H = H - 16
    elif name == "ldh_not_8_bf16_h":
        a.ldh = H + 4
    elif name == "mixed_rows_h_bf16":       # fp32 x with bf16 h: the pipelined body takes one element type
        a.h_bf16 = 1
    else:
        raise KeyError(name)
    return a
