"""Which kernel family serves las_speller_fwd / las_speller_bwd, pinned per geometry and flag: one
forward and one backward through the Speller module per row, and the exact family lists the library reports (_hip.speller_last_variant).

The families: the one-launch loop (`loop`), the prefetching bf16 rows (`pf_rows`), the generic bf16 rows (`bf_rows`), the fp32-operand
rows (`f32_rows`) and the wide per-step path (`wide`); `skinny_cell0` / `skinny_upper_cells`: the cell products on packed MFMA fragments;
`loc`: location-aware attention.  The two passes may differ (B = 64 LSTM: the forward product needs more column tiles than the loop's
product workgroups hold)."""
import numpy as np
import pytest
import torch

from helpers import make_args

pytestmark = pytest.mark.gpu

BENCH = dict(NL=1, D=512, A=128, Hd=512, E=128, B=48, Tp=160, U=5, loc=None)        # bench.py's Speller (D = Hd = 512, T' = 160)
CONFIG3 = dict(BENCH, B=8, loc=(201, 10))                                           # BASELINE configs[3]: location-aware K = 201, C = 10
RUN_SH = dict(NL=2, D=1024, A=128, Hd=512, E=256, B=4, Tp=319, U=4, loc=(201, 10))  # the reference's run.sh recipe

LOOP = ["loop", "skinny_cell0"]
PF = ["pf_rows", "skinny_cell0"]

# (name, cell, prec, flags (las._hip attribute names), geometry, forward families, backward families)
ROWS = [
    ("bench", "lstm", "bf16", (), BENCH, LOOP, LOOP),
    ("bench", "rnn", "bf16", (), BENCH, LOOP, LOOP),
    ("bench", "lstm", "f32", (), BENCH, ["f32_rows"], ["f32_rows"]),
    ("bench", "rnn", "f32", (), BENCH, ["f32_rows"], ["f32_rows"]),
    ("bench_no_fused_step", "lstm", "bf16", ("SPELLER_NO_FUSED_STEP",), BENCH, PF, PF),
    ("bench_no_pf_rows", "lstm", "bf16", ("SPELLER_NO_PF_ROWS",), BENCH, ["bf_rows", "skinny_cell0"], ["bf_rows", "skinny_cell0"]),
    ("bench_no_bf_rows", "lstm", "bf16", ("SPELLER_NO_BF_ROWS",), BENCH, ["f32_rows", "skinny_cell0"], ["f32_rows", "skinny_cell0"]),
    ("bench_wide", "lstm", "bf16", ("SPELLER_WIDE",), BENCH, ["skinny_cell0", "wide"], ["skinny_cell0", "wide"]),
    ("bench_no_wide", "lstm", "bf16", ("SPELLER_NO_WIDE",), BENCH, LOOP, LOOP),
    ("bench_b64", "lstm", "bf16", (), dict(BENCH, B=64), PF, LOOP),                 # 5 x 24 column tiles < 128; 3 x 24 >= 64
    ("bench_u3", "lstm", "bf16", (), dict(BENCH, U=3), PF, PF),                      # the loop takes U >= 4
    ("config3", "lstm", "bf16", (), CONFIG3, LOOP + ["loc"], LOOP + ["loc"]),
    ("config3", "lstm", "f32", (), CONFIG3, ["loc", "wide"], ["loc", "wide"]),
    ("loc_tp240", "lstm", "bf16", (), dict(CONFIG3, B=4, Tp=240), ["skinny_cell0", "loc", "wide"], ["skinny_cell0", "loc", "wide"]),
    ("run_sh", "lstm", "bf16", (), RUN_SH, ["skinny_cell0", "loc", "skinny_upper_cells", "wide"],
     ["skinny_cell0", "loc", "skinny_upper_cells", "wide"]),
    ("run_sh", "rnn", "f32", (), RUN_SH, ["loc", "wide"], ["loc", "wide"]),
    ("run_sh_no_wide", "lstm", "bf16", ("SPELLER_NO_WIDE",), RUN_SH, ["f32_rows", "skinny_cell0", "loc"], ["f32_rows", "skinny_cell0", "loc"]),
    ("small_add", "lstm", "f32", (), dict(NL=1, D=64, A=32, Hd=32, E=32, B=3, Tp=21, U=5, loc=None), ["f32_rows"], ["f32_rows"]),
]


def _families(flags, prec, cell, NL, D, A, Hd, E, B, Tp, U, loc, V=30):
    from las import _hip, layers as L, variables as Vs
    from las.las import Speller
    saved = _hip.speller_flags
    _hip.speller_flags = flags
    try:
        L.set_cell(cell)
        L.set_precision(prec)
        Vs.reset_default_store(device="cuda", seed=3)
        args = make_args(enc_units=Hd, num_enc_layers=2, dec_units=D, num_dec_layers=NL, embedding_size=E, attention_size=A, mode="add",
                         vocab_size=V, enc_type="cnn")                       # (enc_type cnn: the Speller's hidden_dim is enc_units)
        if loc is not None:
            args.mode, args.loc_kernel_size, args.loc_num_channels = "loc", loc[0], loc[1]
        sp = Speller(args)
        rng = np.random.RandomState(1)
        enc = torch.tensor(rng.randn(B, Tp, Hd).astype(np.float32) * 0.5, device="cuda", requires_grad=True)
        enc_len = rng.randint(Tp // 2, Tp + 1, size=B)
        enc_len[0] = Tp
        y = rng.randint(3, V, size=(B, U))
        logits, _, _ = sp(enc, enc_len, U, teacher=y, is_training=True, coins=np.ones(U, bool))
        fam = _hip.speller_last_variant()
        logits.sum().backward()
        _hip.join_side_stream()
        torch.cuda.synchronize()
        _hip.check_status()
        fam["bwd"] = _hip.speller_last_variant()["bwd"]
        return fam
    finally:
        _hip.speller_flags = saved


@pytest.mark.parametrize("row", ROWS, ids=["%s-%s-%s" % r[:3] for r in ROWS])
def test_speller_kernel_family_selection(row):
    from las import _hip
    name, cell, prec, flag_names, g, fwd, bwd = row
    flags = 0
    for n in flag_names:
        flags |= getattr(_hip, n)
    fam = _families(flags, prec, cell, g["NL"], g["D"], g["A"], g["Hd"], g["E"], g["B"], g["Tp"], g["U"], g["loc"])
    print("families %s: %s" % (row[:3], fam))
    assert fam == {"fwd": fwd, "bwd": bwd}, (row[:3], fam)
