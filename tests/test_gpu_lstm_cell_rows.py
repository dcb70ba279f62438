"""Every device body of las_lstm_cell_rows (csrc/lstm_cell_rows.h: the unpipelined 32-row body, the pipelined body at 32 / 64 / 128 rows,
the unpipelined and the pipelined pair kernel) against the float64 restatement of tests/lstm_cell_ref.py, against each other bit for bit,
and the paired launch (las_lstm_cell_rows_pair_args) against its two single launches.  Each launch first asks las_lstm_cell_rows_plan
which body it gets and asserts the one tests/lstm_cell_ref.py's tables name; tests/test_lstm_cell_ref_host.py shows without a GPU that
the tables reach every plan code of a shipping build and that the tolerances catch the errors these kernels could make.

Every output buffer has GUARD rows of a sentinel bit pattern behind row M, x and h have GUARD rows of NaN behind row M and NaN in their
padding columns: no guard row may change and no NaN may reach an output."""
import ctypes
import functools

import pytest
import torch

import helpers  # noqa: F401  (sys.path)
import lstm_cell_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT32, SENT16 = 0x5a5a5a5a, 0x5a5a          # (a finite float / bf16: a guard row copied into an output row would not hide as NaN)
OUTS = ("c_out", "h_out", "gates_out", "h_out_bf16")


def _lib():
    from las import _hip
    return _hip.lib()


def _stream():
    from las import _hip
    return _hip.stream()


class Weights:
    """what all row prefixes of a problem share: packed weights, bias, the one-hot input's rows"""

    def __init__(self, p):
        from las import _hip
        H, I = p["H"], p["I"]
        self.Wx = _hip.skinny_pack(p["Wx"].to(DEV), I, 4 * H) if p["Wx"] is not None else None
        self.Wh = _hip.skinny_pack(p["Wh"].to(DEV), H, 4 * H) if p["Wh"] is not None else None
        self.bias = p["bias"].to(DEV)
        self.xrows = p["xrows"].to(DEV).contiguous() if p["xrows"] is not None else None


class Launch:
    """device operands and sentinel-filled outputs of the first M rows of problem p"""

    def __init__(self, p, w, M, padded):
        f = R.FORMS[p["form"]]
        self.p, self.w, self.M, self.form = p, w, M, p["form"]
        H, I, pad = p["H"], p["I"], R.PAD if padded else 0
        self.ldx, self.ldh = I + pad, H + pad

        def rows(t, kind, ld):      # [M + GUARD, ld] of NaN with the M rows in its upper left corner
            if t is None:
                return None
            buf = torch.full((M + R.GUARD, ld), float("nan"), dtype=torch.bfloat16 if kind == "bf16" else torch.float32, device=DEV)
            buf[:M, :t.shape[1]] = t[:M].to(DEV).to(buf.dtype)
            return buf
        self.x, self.h = rows(p["x"], f["x"], self.ldx), rows(p["h"], f["h"], self.ldh)
        self.c_prev = rows(p["c_prev"], "f32", H)
        self.ids = p["ids"][:M].to(DEV).contiguous() if p["ids"] is not None else None
        self.out = {"c_out": self._sent(H), "h_out": self._sent(H), "gates_out": self._sent(4 * H) if f["gates"] else None,
                    "h_out_bf16": self._sent(H, True) if f["hb"] else None}

    def _sent(self, width, bf16=False):
        if bf16:
            return torch.full((self.M + R.GUARD, width), SENT16, dtype=torch.int16, device=DEV).view(torch.bfloat16)
        return torch.full((self.M + R.GUARD, width), SENT32, dtype=torch.int32, device=DEV).view(torch.float32)

    def ptrs(self):
        t = dict(x=self.x, h=self.h, Wx=self.w.Wx, Wh=self.w.Wh, bias=self.w.bias, c_prev=self.c_prev, ids=self.ids, xrows=self.w.xrows, **self.out)
        return {k: (None if v is None else v.data_ptr()) for k, v in t.items()}

    def args(self):
        return R.fill_args(self.form, self.M, self.p["I"], self.p["H"], self.ldx, self.ldh, self.ptrs())

    @staticmethod
    def _bits(t):
        return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)

    def untouched_from(self, row):
        """every output buffer still holds the sentinel from `row` on"""
        return all(bool((self._bits(t)[row:] == (SENT16 if t.dtype == torch.bfloat16 else SENT32)).all()) for t in self.out.values() if t is not None)

    def results(self):
        """the M written rows of every output, after the guard-row and NaN checks"""
        torch.cuda.synchronize()
        assert self.untouched_from(self.M), "a guard row behind row M was written"
        res = {k: t[:self.M] for k, t in self.out.items() if t is not None}
        for k, t in res.items():
            assert not bool(torch.isnan(t.float()).any()), "NaN in %s: padding or guard rows of x / h were read" % k
        if "h_out_bf16" in res:
            assert torch.equal(self._bits(res["h_out_bf16"]), self._bits(res["h_out"].to(torch.bfloat16))), "h_out_bf16 is not h_out rounded to nearest even"
        return res


def _plan(a, b=None):
    return _lib().las_lstm_cell_rows_plan(None if a is None else ctypes.byref(a), None if b is None else ctypes.byref(b))


def _same_bits(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and torch.equal(Launch._bits(x.contiguous()), Launch._bits(y.contiguous()))


def _errors(res, ref, form):
    """max |kernel - float64 reference| per output, printed and held to the form's tolerance"""
    errs = {k: (res[k].double().cpu() - ref[r]).abs().max().item() for k, r in (("c_out", "c"), ("h_out", "h"), ("gates_out", "gates")) if k in res}
    print("    %-4s max error %s (tolerance %.0e)" % (form, "  ".join("%s %.2e" % kv for kv in errs.items()), R.tol(form)))
    for k, e in errs.items():
        assert e < R.tol(form), (form, k, e)


@functools.lru_cache(maxsize=None)
def _problem(form, M, I, H):
    p = R.make_problem(form, M, I, H)
    return p, Weights(p)


@functools.lru_cache(maxsize=None)
def _single(form, I, H, padded, M):
    """one single launch of the case's first M rows, planned as the table says: its outputs, or None where the table says refused"""
    p, w = _problem(form, R.ROWS, I, H)
    L = Launch(p, w, M, padded)
    a = L.args()
    want, got = R.PLAN_BY_PREFIX[form][M], _plan(a)
    print("    %-4s I=%d H=%d M=%d: plan %d" % (form, I, H, M, got))
    if want == R.REFUSED:
        assert got < 0, (form, M, got)
        assert _lib().las_lstm_cell_rows_args(ctypes.byref(a), _stream()) < 0
        torch.cuda.synchronize()
        assert L.untouched_from(0), "a refused call wrote an output"
        return None
    assert got == want, (form, M, got, want)                        # BEFORE the launch: the body the table names
    assert _lib().las_lstm_cell_rows_args(ctypes.byref(a), _stream()) == 0
    return L.results()


@pytest.mark.parametrize("case", R.SINGLE_CASES, ids=lambda c: "%s-%d-%d%s" % (c[0], c[1], c[2], "-padded" if c[3] else ""))
def test_bodies_agree_bit_for_bit_and_match_float64(case):
    """(a) The row prefixes of one set of ROWS rows run through the unpipelined body and the pipelined body at 32, 64 and 128 rows per
    workgroup, on both sides of 127 / 128, 256 / 257 and 512 / 513.  Rows do not depend on each other, so every prefix's rows must be,
    bit for bit, the same rows of the longest prefix (the kernels' stated contract); that one is held to the float64 reference."""
    form, I, H, padded = case
    full = _single(form, I, H, padded, R.ROWS)
    for M in R.PREFIXES[:-1]:
        res = _single(form, I, H, padded, M)
        if res is None:
            continue
        assert sorted(res) == sorted(full)
        for k in res:
            assert _same_bits(res[k], full[k][:M]), "%s: rows of M = %d differ from the same rows of M = %d" % (k, M, R.ROWS)
    _errors(full, R.lstm_cell_ref(_problem(form, R.ROWS, I, H)[0]), form)


@pytest.mark.parametrize("f32,bf16,I,H", [("L0", "L0b", 0, 96), ("L0", "L0b", 0, 32), ("L1", "L1b", 544, 96), ("L1", "L1b", 160, 64)])
def test_bf16_row_copies_give_the_fp32_rows_results(f32, bf16, I, H):
    """bf16 x / h are the staging's own rounding of the fp32 rows: c' and h' of the two forms are bit-identical (with the prefixes
    above: in every body)"""
    pad = {c[:3]: c[3] for c in R.SINGLE_CASES}
    a, b = _single(f32, I, H, pad[(f32, I, H)], R.ROWS), _single(bf16, I, H, pad[(bf16, I, H)], R.ROWS)
    assert _same_bits(a["c_out"], b["c_out"]) and _same_bits(a["h_out"], b["h_out"])


@pytest.mark.parametrize("n", range(len(R.PAIR_CASES)), ids=lambda n: "%d-%s" % (n, R.PAIR_CASES[n][4].split(":")[0].split(",")[0].replace(" ", "_")))
def test_pair_equals_its_two_single_launches(n):
    """(b) las_lstm_cell_rows_pair_args(a, b) into one set of buffers, las_lstm_cell_rows_args(a) and (b) into another: every output of
    both problems bit for bit the same, no guard row touched -- with the two problems differing in width and in rows (the pair grid
    covers the larger; the other's surplus workgroups must leave), and where no pair kernel exists (two launches).  Below 128 rows the
    single launch runs lstm_cell_rows_body with its chunk prefetch (PIPE) and the pair kernel runs it without: the first four rows and
    the tenth are also the comparison of those two."""
    (fa, Ma, Ia, Ha), (fb, Mb, Hb), want, padded, what = R.PAIR_CASES[n]
    (pa, wa), (pb, wb) = _problem(fa, Ma, Ia, Ha), _problem(fb, Mb, 0, Hb)
    pair = Launch(pa, wa, Ma, padded), Launch(pb, wb, Mb, padded)
    a, b = pair[0].args(), pair[1].args()
    got = _plan(a, b)
    print("    %s: plan 0x%x" % (what, got))
    assert got == want, (what, got, want)                            # BEFORE the launch
    assert _lib().las_lstm_cell_rows_pair_args(ctypes.byref(a), ctypes.byref(b), _stream()) == 0
    res = pair[0].results(), pair[1].results()
    for k, (L0, r2) in enumerate(zip((Launch(pa, wa, Ma, padded), Launch(pb, wb, Mb, padded)), res)):
        s = L0.args()
        assert _plan(s) >= 0
        assert _lib().las_lstm_cell_rows_args(ctypes.byref(s), _stream()) == 0
        r1 = L0.results()
        assert sorted(r1) == sorted(r2)
        for name in r1:
            assert _same_bits(r1[name], r2[name]), "problem %s, %s: the pair differs from the single launch" % ("ab"[k], name)
    if R.FORMS[fa]["hb"]:
        assert "h_out_bf16" in res[0]                               # (results() has checked that it is h_out rounded)
    if n == R.PAIR_REF_CASE:
        _errors(res[0], R.lstm_cell_ref(pa), fa)
        _errors(res[1], R.lstm_cell_ref(pb), fb)


@pytest.mark.parametrize("name", R.REFUSALS)
def test_refusals_launch_nothing(name):
    """(c) negative from the launch, from the pair entry with the arguments as either problem, and from the query; every output buffer
    still all sentinel"""
    lib, M, I, H = _lib(), 200, 160, 64
    form = "L1b" if name == "ldh_not_8_bf16_h" else "L1"
    p, w = _problem(form, M, I, H)
    L = Launch(p, w, M, False)
    ptr = L.ptrs()
    ids, xrows = torch.zeros(M, dtype=torch.int32, device=DEV), torch.zeros(R.V, 4 * H, device=DEV)
    ptr["ids"], ptr["xrows"] = ids.data_ptr(), xrows.data_ptr()
    a = R.refusal_args(name, ptr, M, I, H)
    ok = Launch(*_problem("S", M, I, H), M, False)
    g = ok.args()
    assert _plan(g) >= 0 and _plan(a) < 0                           # BEFORE any call that could launch
    if a is not None:
        assert _plan(a, g) < 0 and _plan(g, a) < 0
    assert lib.las_lstm_cell_rows_args(None if a is None else ctypes.byref(a), _stream()) < 0
    assert lib.las_lstm_cell_rows_pair_args(ctypes.byref(g), None if a is None else ctypes.byref(a), _stream()) < 0
    assert lib.las_lstm_cell_rows_pair_args(None if a is None else ctypes.byref(a), ctypes.byref(g), _stream()) < 0
    torch.cuda.synchronize()
    assert L.untouched_from(0) and ok.untouched_from(0), "a refused call wrote an output"
