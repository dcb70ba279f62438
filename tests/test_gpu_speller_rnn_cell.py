"""The Speller's per-utterance bf16 families with the tanh cell (CELL = BasicRNNCell, the reference's default): the one-launch loop, the
prefetching rows, the generic bf16 rows, the fp32-operand rows and the skinny cell product in front of them, one table row per (geometry,
flags), against the oracle's Speller (tests/speller_ref.py) at a bound measured per case ON THE ORACLE: MARGIN x the distance the oracle's own
outputs move when its encoder input moves by 1e-5.  Each case asserts the families the plan chose (worked out from csrc/speller_plan.h for 256
compute units) BEFORE it compares anything, then the status word, then logits, alignments and every gradient in relative L2 and max norm.
tests/test_speller_ref_host.py shows without a GPU that the smallest kernel mistakes lie above that bound on these very shapes' classes.

What the table reaches that no LSTM test does: G = 1 gate columns (32 column tiles at D = 512: most product workgroups of the forward loop hold
only clamped, masked-out tiles), the forward loop at B = 64 .. 128 (R = 8 .. 16 row workgroups per group; the LSTM's stops at B = 48), a
forward loop in front of prefetching gradient rows (B = 96, 128), the generic bf16 rows with two layers.

The table is plain data and this module imports without touching the device.

Tolerance: MEASURED below.

MEASURED (MI355X, MARGIN = 4 kept: every family is within 0.5 of the bound, i.e. within 2 x the floor; the status word was clean and every
planned family was the one its row names).  Per case: the largest error as a fraction of its bound and the quantity it is on (gmax/ = max
norm, grad/ = relative L2 of a gradient tensor), then error / floor for the logits, the alignments, the worst gradient tensor (relative L2) and
the worst max-norm figure.  The gradient of dense/bias (floor 0, bound 6.1e-5) differed by at most 6.0e-7; |alphas.sum(-1) - 1| <= 3.6e-7.
The fp32-operand rows (no_bf_rows) are compared with the oracle's fp32-row mode, whose floor is about half the bf16 rows'.
  case       shape-flags                              worst        | logits            | alphas            | gradients         | max norm
  row        1-512-128-256-5-37-6-False               0.18 (gmax/embedding) | 9.1e-04 / 3.1e-03 | 2.3e-04 / 1.6e-03 | 4.0e-03 / 9.2e-03 | 5.2e-03 / 9.4e-03
  row        1-512-128-256-5-37-6-False-no_fused_step 0.15 (gmax/embedding) | 9.5e-04 / 3.1e-03 | 2.3e-04 / 1.6e-03 | 3.7e-03 / 9.2e-03 | 5.0e-03 / 9.4e-03
  row        1-512-128-256-5-37-6-False-no_pf_rows    0.24 (gmax/enc) | 9.5e-04 / 3.1e-03 | 2.3e-04 / 1.6e-03 | 4.9e-03 / 9.2e-03 | 8.1e-03 / 9.4e-03
  row        1-512-128-256-5-37-6-False-no_bf_rows    0.23 (grad/embedding) | 1.1e-03 / 2.8e-03 | 2.8e-04 / 9.6e-04 | 4.6e-03 / 5.7e-03 | 4.4e-03 / 5.5e-03
  row        1-512-128-256-4-160-6-False              0.18 (gmax/basic_rnn_cell/kernel) | 3.2e-04 / 3.7e-03 | 1.6e-05 / 2.1e-03 | 6.7e-03 / 1.2e-02 | 8.2e-03 / 1.4e-02
  row        1-512-128-256-4-160-6-False-no_fused_step 0.17 (gmax/basic_rnn_cell/kernel) | 3.1e-04 / 3.7e-03 | 3.5e-06 / 2.1e-03 | 6.3e-03 / 1.2e-02 | 8.2e-03 / 1.4e-02
  row        1-512-128-256-4-160-6-False-no_pf_rows   0.18 (grad/embedding) | 3.1e-04 / 3.7e-03 | 3.5e-06 / 2.1e-03 | 6.2e-03 / 1.2e-02 | 7.7e-03 / 1.4e-02
  row        1-512-128-256-4-160-6-False-no_bf_rows   0.28 (gmax/attention/dense_1/kernel) | 9.4e-04 / 2.9e-03 | 1.2e-04 / 9.3e-04 | 5.7e-03 / 8.3e-03 | 8.0e-03 / 1.0e-02
  row        1-512-128-256-3-131-5-True               0.35 (gmax/enc) | 4.2e-04 / 3.0e-03 | 1.4e-04 / 1.1e-03 | 9.5e-03 / 8.4e-03 | 1.3e-02 / 9.2e-03
  row        1-512-128-256-3-131-5-True-no_fused_step 0.35 (gmax/enc) | 4.2e-04 / 3.0e-03 | 1.4e-04 / 1.1e-03 | 9.5e-03 / 8.4e-03 | 1.3e-02 / 9.2e-03
  row        1-512-128-256-3-131-5-True-no_pf_rows    0.20 (gmax/embedding) | 4.2e-04 / 3.0e-03 | 1.4e-04 / 1.1e-03 | 4.1e-03 / 8.4e-03 | 4.5e-03 / 9.2e-03
  row        1-512-128-256-3-131-5-True-no_bf_rows    0.24 (grad/attention/dense_1/kernel) | 1.1e-03 / 2.6e-03 | 4.6e-05 / 7.7e-04 | 4.5e-03 / 8.0e-03 | 5.3e-03 / 9.9e-03
  row        1-512-128-256-3-181-4-False              0.30 (logits_max) | 1.5e-03 / 3.3e-03 | 1.8e-04 / 1.6e-03 | 4.1e-03 / 7.1e-03 | 4.1e-03 / 1.1e-02
  row        1-512-128-256-3-181-4-False-no_fused_step 0.30 (logits_max) | 1.5e-03 / 3.3e-03 | 1.8e-04 / 1.6e-03 | 4.1e-03 / 7.1e-03 | 4.1e-03 / 1.1e-02
  row        1-512-128-256-3-181-4-False-no_pf_rows   0.30 (logits_max) | 1.5e-03 / 3.3e-03 | 1.8e-04 / 1.6e-03 | 3.4e-03 / 7.1e-03 | 4.7e-03 / 1.1e-02
  row        1-512-128-256-3-181-4-False-no_bf_rows   0.25 (gmax/attention/dense_1/kernel) | 1.6e-04 / 2.3e-03 | 6.6e-07 / 7.5e-04 | 2.9e-03 / 3.7e-03 | 7.2e-03 / 7.5e-03
  row        1-512-128-256-2-214-4-True               0.31 (gmax/attention/dense/kernel) | 8.0e-04 / 3.2e-03 | 5.3e-04 / 1.8e-03 | 4.3e-03 / 7.5e-03 | 5.3e-03 / 1.0e-02
  row        1-512-128-256-2-214-4-True-no_fused_step 0.31 (gmax/attention/dense/kernel) | 8.0e-04 / 3.2e-03 | 5.3e-04 / 1.8e-03 | 4.3e-03 / 7.5e-03 | 5.3e-03 / 1.0e-02
  row        1-512-128-256-2-214-4-True-no_pf_rows    0.23 (gmax/attention/dense/kernel) | 8.0e-04 / 3.2e-03 | 5.3e-04 / 1.8e-03 | 4.4e-03 / 7.5e-03 | 5.2e-03 / 1.0e-02
  row        1-512-128-256-2-214-4-True-no_bf_rows    0.45 (gmax/attention/dense_1/kernel) | 1.3e-03 / 2.9e-03 | 2.3e-04 / 1.2e-03 | 3.6e-03 / 3.7e-03 | 7.1e-03 / 4.4e-03
  row        1-512-128-256-2-230-4-False              0.20 (gmax/embedding) | 6.4e-04 / 3.1e-03 | 2.8e-04 / 2.0e-03 | 2.9e-03 / 8.2e-03 | 4.1e-03 / 1.1e-02
  row        1-512-128-256-2-230-4-False-no_bf_rows   0.49 (gmax/attention/dense_1/kernel) | 3.8e-07 / 3.0e-03 | 7.5e-07 / 1.2e-03 | 2.9e-03 / 3.8e-03 | 5.8e-03 / 4.6e-03
  row        1-512-128-256-9-160-6-False              0.25 (gmax/embedding) | 1.0e-03 / 3.4e-03 | 4.1e-04 / 2.0e-03 | 3.5e-03 / 8.0e-03 | 4.6e-03 / 9.2e-03
  row        1-512-128-256-17-160-6-True              0.13 (gmax/enc) | 3.5e-04 / 3.7e-03 | 9.6e-05 / 2.1e-03 | 2.2e-03 / 7.5e-03 | 2.9e-03 / 7.6e-03
  row        1-512-128-256-48-160-6-False             0.12 (gmax/enc) | 5.6e-04 / 3.3e-03 | 1.4e-04 / 1.9e-03 | 2.4e-03 / 7.7e-03 | 3.2e-03 / 7.5e-03
  row        1-512-128-256-64-160-4-False             0.12 (gmax/embedding) | 4.9e-04 / 3.1e-03 | 1.1e-04 / 1.9e-03 | 2.3e-03 / 6.4e-03 | 2.9e-03 / 7.7e-03
  row        1-512-128-256-96-80-5-False              0.12 (gmax/embedding) | 8.1e-04 / 3.3e-03 | 2.1e-04 / 1.7e-03 | 2.3e-03 / 6.5e-03 | 4.3e-03 / 1.0e-02
  row        1-512-128-256-128-40-4-False             0.10 (gmax/embedding) | 4.3e-04 / 3.1e-03 | 1.0e-04 / 1.6e-03 | 1.6e-03 / 6.3e-03 | 2.0e-03 / 6.6e-03
  row        1-96-136-36-3-70-5-False                 0.26 (gmax/embedding) | 5.0e-08 / 2.1e-03 | 4.8e-07 / 1.7e-03 | 2.5e-03 / 4.7e-03 | 3.4e-03 / 5.3e-03
  row        2-64-32-64-4-21-7-True-no_wide           0.20 (gmax/multi_rnn_cell/cell_0/basic_rnn_cell/kernel) | 5.0e-04 / 3.6e-03 | 4.3e-05 / 1.5e-03 | 3.7e-03 / 8.1e-03 | 4.4e-03 / 1.1e-02
  row        1-512-128-256-5-37-6-False-loc201x10     0.29 (gmax/attention/conv1d/bias) | 1.4e-06 / 3.4e-03 | 3.9e-06 / 2.3e-03 | 7.3e-03 / 6.9e-03 | 8.8e-03 / 8.6e-03
  row        1-512-128-256-17-131-5-True-loc201x10    0.24 (grad/attention/conv1d/bias) | 8.5e-04 / 3.2e-03 | 2.3e-04 / 2.3e-03 | 8.9e-03 / 9.8e-03 | 9.3e-03 / 1.0e-02
  row        1-128-64-64-9-181-4-True-loc7x3          0.29 (grad/attention/conv1d/kernel) | 2.5e-06 / 2.3e-03 | 8.5e-07 / 1.3e-03 | 3.0e-03 / 5.2e-03 | 3.8e-03 / 5.9e-03
  short      1-512-128-256-5-37-6-False               0.17 (gmax/embedding) | 8.4e-04 / 3.1e-03 | 2.3e-04 / 1.5e-03 | 4.6e-03 / 9.5e-03 | 5.3e-03 / 1.0e-02
  saved      1-512-128-256-5-37-6-False-loc201x10     0.29 (gmax/attention/conv1d/bias) | 1.4e-06 / 3.4e-03 | 3.9e-06 / 2.3e-03 | 7.3e-03 / 6.9e-03 | 8.8e-03 / 8.6e-03
  recomputed 1-512-128-256-5-37-6-False-loc201x10     0.29 (grad/attention/conv1d/bias) | 1.4e-06 / 3.4e-03 | 3.9e-06 / 2.3e-03 | 8.0e-03 / 6.9e-03 | 7.1e-03 / 8.6e-03
No family needed more than the floor itself on the logits and alignments; the gradients of the three-utterance cases (T' = 131) come closest
to their own floor (9.5e-3 against 8.4e-3, bound 3.4e-2).  No defect was found: the tanh cell's kernels compute what the oracle computes."""
import pytest

import helpers  # noqa: F401  (sys.path)
import speller_ref as SR
from helpers import row_mode

LOOP, PF, BF, F32 = (["loop", "skinny_cell0"], ["pf_rows", "skinny_cell0"], ["bf_rows", "skinny_cell0"], ["f32_rows", "skinny_cell0"])
LOOPLOC = ["loop", "skinny_cell0", "loc"]

# shape = (NL, D, A, H, B, T', U, mixed sampling, loc): H = 256 is Hd = 512, the bench geometry
T37 = (1, 512, 128, 256, 5, 37, 6, False, None)          # frames per wave NE = 8
T160 = (1, 512, 128, 256, 4, 160, 6, False, None)        # NE = 10, what bench.py times
T131 = (1, 512, 128, 256, 3, 131, 5, True, None)         # NE = 10, ragged, sampled tokens
T181 = (1, 512, 128, 256, 3, 181, 4, False, None)        # NE = 12
T214 = (1, 512, 128, 256, 2, 214, 4, True, None)         # NE = 14
T230 = (1, 512, 128, 256, 2, 230, 4, False, None)        # T' > 224: no prefetching rows, no loop
LOC37 = (1, 512, 128, 256, 5, 37, 6, False, (201, 10))   # the reference's K = 201, C = 10: both borders of the filter clipped

# (shape, flags (las._hip attribute names), forward families, backward families)
ROWS = []
for _s in (T37, T160, T131, T181, T214):
    ROWS += [(_s, (), LOOP, LOOP), (_s, ("SPELLER_NO_FUSED_STEP",), PF, PF), (_s, ("SPELLER_NO_PF_ROWS",), BF, BF),
             (_s, ("SPELLER_NO_BF_ROWS",), F32, F32)]
ROWS += [
    (T230, (), BF, BF),
    (T230, ("SPELLER_NO_BF_ROWS",), F32, F32),
    # rows per XCD group: utterance b = 8 r + x is tile row r of group x; R = cdiv(B, 8) row workgroups beside pn = 32 - R product workgroups.
    # Forward: 32 column tiles <= 5 pn up to the planner's R = 16.  Backward: 64 column tiles <= 3 pn needs R <= 10.
    ((1, 512, 128, 256, 9, 160, 6, False, None), (), LOOP, LOOP),       # R = 2, one group a row short
    ((1, 512, 128, 256, 17, 160, 6, True, None), (), LOOP, LOOP),       # R = 3
    ((1, 512, 128, 256, 48, 160, 6, False, None), (), LOOP, LOOP),      # R = 6
    ((1, 512, 128, 256, 64, 160, 4, False, None), (), LOOP, LOOP),      # R = 8: the LSTM's forward is on pf_rows here
    ((1, 512, 128, 256, 96, 80, 5, False, None), (), LOOP, PF),         # R = 12: 3 x 20 < 64
    ((1, 512, 128, 256, 128, 40, 4, False, None), (), LOOP, PF),        # R = 16, the planner's limit
    ((1, 96, 136, 36, 3, 70, 5, False, None), (), BF, BF),              # attention width > 128: two 16-byte chunks per lane
    ((2, 64, 32, 64, 4, 21, 7, True, None), ("SPELLER_NO_WIDE",), BF, BF),   # two layers off the wide path
    (LOC37, (), LOOPLOC, LOOPLOC),
    ((1, 512, 128, 256, 17, 131, 5, True, (201, 10)), (), LOOPLOC, LOOPLOC),
    ((1, 128, 64, 64, 9, 181, 4, True, (7, 3)), (), LOOPLOC, LOOPLOC),
]
LOC_GRADS = (SR.CONV_W, SR.CONV_B, SR.LOC_WF)


def row_id(row):
    return "-".join(str(x) for x in row[0][:8]) + ("-loc%dx%d" % row[0][8] if row[0][8] else "") + "".join("-" + f[8:].lower() for f in row[1])


def row_rows(row):
    """the oracle's row arithmetic of a table row (helpers.row_mode of the families it names)"""
    return row_mode({"fwd": row[2], "bwd": row[3]})


def _flags(names):
    from las import _hip
    f = 0
    for n in names:
        f |= getattr(_hip, n)
    return f


def _run_and_check(row, variant=None, tag="row"):
    """forward + backward on the device; the families, then the status word, then every quantity against the oracle at bound(floor)"""
    from las import _hip
    shape, flag_names, fwd, bwd = row
    got, fam = SR.run_hip("rnn", shape, _flags(flag_names), SR.weights("rnn", shape), SR.case_inputs("rnn", shape, variant))
    assert fam == {"fwd": fwd, "bwd": bwd}, (row_id(row), fam)
    _hip.check_status()
    rows = row_mode(fam)
    ref, fl = SR.base_of("rnn", shape, rows, variant), SR.floor_of("rnn", shape, rows, variant)
    assert set(ref["grads"]) <= set(got["grads"])
    err, bnd = SR.errors(got, ref), SR.bound(fl)
    worst = max((k for k in bnd if fl[k] > 0), key=lambda k: err[k] / bnd[k])
    print("RNN-CELL-FRACTION %s %s worst %s = %.2f of the bound; error / floor: logits %.1e / %.1e alphas %.1e / %.1e gradients %.1e / %.1e "
          "max-norm %.1e / %.1e; %s %.1e; alpha_sum %.1e" % (
              tag, row_id(row), worst, err[worst] / bnd[worst], err["logits"], fl["logits"], err["alphas"], fl["alphas"],
              max(err[k] for k in fl if k.startswith("grad/")), max(fl[k] for k in fl if k.startswith("grad/")),
              max(err[k] for k in fl if "max" in k), max(fl[k] for k in fl if "max" in k),
              "dense/bias", err["grad/" + SR.VOCAB_B], err["alpha_sum"]))
    assert not SR.violations(err, bnd), (row_id(row), SR.violations(err, bnd))
    return got, ref, fam


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_planned_tanh_cell_family_matches_oracle(row):
    got, ref, fam = _run_and_check(row)
    if row[0][8] is not None:
        assert "loop" in fam["fwd"] and "loc" in fam["fwd"] and "loop" in fam["bwd"] and "loc" in fam["bwd"], fam
        for n in LOC_GRADS:
            assert float(ref["grads"][n].abs().max()) > 0 and float(got["grads"][n].abs().max()) > 0, n


@pytest.mark.gpu
def test_short_utterance_in_the_loop():
    """An utterance of SHORT_LEN = 3 frames that share one key (speller_ref.inputs, variant "short": each frame carries a third of the context):
    the input on which an attention mask that is off by one frame is 10x the bound (tests/test_speller_ref_host.py)."""
    _run_and_check((T37, (), LOOP, LOOP), variant="short", tag="short")


@pytest.mark.gpu
def test_location_aware_gradient_loop_with_and_without_the_saved_activations():
    """tests/test_gpu_speller_bf16.py's test of the same name, for the tanh cell: with las.SAVE_ACTIVATIONS off the gradient rows recompute
    tanh(keys + q + f . Wf) and the conv outputs instead of reading the forward's fp16 copies (act_save).  Same forward bit for bit,
    gradients equal up to the fp16 rounding of the activations, both within the bound of the oracle, and not the same bits."""
    import torch
    from las import las as LL
    row = (LOC37, (), LOOPLOC, LOOPLOC)
    assert LL.SAVE_ACTIVATIONS, "the default is to save"
    a, ref, _ = _run_and_check(row, tag="saved")
    LL.SAVE_ACTIVATIONS = False
    try:
        b, _, _ = _run_and_check(row, tag="recomputed")
    finally:
        LL.SAVE_ACTIVATIONS = True
    assert torch.equal(a["logits"], b["logits"]) and torch.equal(a["alphas"], b["alphas"])
    differ = 0
    for n in sorted(ref["grads"]):
        scale = max(ref["grads"][n].abs().max().item(), 1e-3)
        assert (a["grads"][n] - b["grads"][n]).abs().max().item() / scale < 1e-2, n
        differ += int(not torch.equal(a["grads"][n], b["grads"][n]))
    assert differ > 0, "the two gradient loops are different kernel paths: identical bits mean the switch did nothing"
