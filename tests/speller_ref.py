"""The Speller alone against the project's oracle (oracle.speller_forward in its bf16-operand mode), with a bound that is MEASURED ON THE
ORACLE per case instead of a guessed constant (not a test module; tests/test_speller_ref_host.py and tests/test_gpu_speller_rnn_cell.py use it).

A case is (cell, shape): shape = (NL, D, A, H, B, T', U, mixed sampling, loc) with H the Listener's enc_units (the pyramid hands the Speller
Hd = 2 H), loc = None (additive attention) or (K, C) (location-aware: filter taps, channels); E = 64, V = 30 throughout.

  * weights(cell, shape) / inputs(shape): one fixed set of weights and inputs per case.  The weights are oracle.init_params with the biases the
    initialiser leaves at zero drawn from U(-0.25, 0.25) (a zero bias hides every bias-indexing mistake) and, for location-aware attention,
    a filter of the size a trained model has (U(-2, 2): with the initialiser's +-0.05 the location term is 1e-2 of the energies' other terms
    and nothing that goes wrong in it would show).  The inputs follow tests/test_gpu_speller_bf16.py::_run.
  * run_oracle: logits, alignments and every gradient of sum(logits * w).
  * errors(got, ref): relative L2 and max-norm distances.
  * floor: how far the ORACLE's own outputs move when the encoder input moves by 1e-5 (two draws, the larger distance per quantity).  In
    bf16-operand arithmetic that is not a slope but the flip floor: an input that moves by 1e-5 flips the bf16 rounding of a few operands, and
    each flip is a 2^-9 relative change that the tanh recurrence carries on.  A correct kernel (other accumulation order, fast transcendentals)
    differs from the oracle by flips of the same kind, so its distance is a small multiple of the floor: bound(floor) = MARGIN x floor.
  * MUTATIONS: the smallest realistic kernel mistakes (one row / column / tile / tap / frame / token wrong), stated as edits of the oracle's
    inputs.  tests/test_speller_ref_host.py shows on the CPU that every one of them lies ABOVE bound(floor), i.e. that a kernel within the
    bound cannot have made one of them."""
import functools

import numpy as np
import torch

from helpers import make_args

E, V = 64, 30
SHORT_LEN = 3

# bound = MARGIN x floor.  4 is what the LSTM tests' stated tolerances amount to over the LSTM's floor measured the same way (logits 5e-3
# over 1.4e-3, gradients 2e-2 over 4.2e-3).  Measured against the oracle only, never against the kernels.
MARGIN = 4.0
# a quantity whose floor is exactly 0 does not depend on the arithmetic of the recurrence at all (the gradient of Speller/decode/dense/bias
# is sum_{b, u} w[b, u, :] whatever the model does): both sides add the same <= 1024 fp32 terms in some order, whose worst-case relative
# difference (against the largest partial sum) is 1024 x 2^-24
FP32_SUM_SLACK = 1024 * 2.0 ** -24
ALPHA_SUM_TOL = 1e-4

ATT = "Speller/decode/attention/"
CONV_W, CONV_B, LOC_WF = ATT + "conv1d/kernel", ATT + "conv1d/bias", ATT + "dense_2/kernel"
EMB, VOCAB_W, VOCAB_B = "embedding/embedding_matrix", "Speller/decode/dense/kernel", "Speller/decode/dense/bias"


def speller_args(shape):
    NL, D, A, H, B, Tp, U, mixed, loc = shape
    args = make_args(enc_units=H, num_enc_layers=2, dec_units=D, num_dec_layers=NL, embedding_size=E, attention_size=A, mode="add",
                     vocab_size=V, enc_type="pblstm")
    if loc is not None:
        args.mode, args.loc_kernel_size, args.loc_num_channels = "loc", loc[0], loc[1]
    return args


def cell_names(cell, NL):
    """[(kernel, bias)] of the decoder cell's layers"""
    from oracle import las_oracle as O
    cs = O.cell_scope(cell)
    bases = ["Speller/decode/%s/" % cs] if NL == 1 else ["Speller/decode/multi_rnn_cell/cell_%d/%s/" % (l, cs) for l in range(NL)]
    return [(b + "kernel", b + "bias") for b in bases]


@functools.lru_cache(maxsize=None)
def weights(cell, shape):
    """{TF name: float32 array} of the Speller's variables (read-only: run_oracle and the mutations copy)"""
    from oracle import las_oracle as O
    p = O.init_params(speller_args(shape), seed=3, cell=cell)
    p = {n: v for n, v in p.items() if not n.startswith("Listener/")}
    rng = np.random.RandomState(17)
    for n in sorted(p):
        if n.endswith("/bias"):
            p[n] = rng.uniform(-0.25, 0.25, p[n].shape).astype(np.float32)
    if CONV_W in p:
        p[CONV_W] = rng.uniform(-2.0, 2.0, p[CONV_W].shape).astype(np.float32)
    for v in p.values():
        v.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def inputs(shape, variant=None, cell=None):
    """encoder output, lengths, teacher tokens, coins / sampled tokens and the weights w of the scalar sum(logits * w) that is differentiated.
    variant "short" (needs the cell: it is built on weights(cell, shape)): utterance 0 is SHORT_LEN frames long and its frames are
    frame 0 plus a random vector from the null space of the key projection -- equal keys, hence equal shares of the attention, but
    different values, so every one of its frames carries a third of the context.  (With random frames the attention of these weights is a
    peak of 0.96-0.999 on ONE frame, and whether a frame matters at all is the luck of the draw.)"""
    NL, D, A, H, B, Tp, U, mixed, loc = shape
    rng = np.random.RandomState(1)
    x = {"enc": rng.randn(B, Tp, 2 * H).astype(np.float32) * 0.5}
    x["enc_len"] = rng.randint(Tp // 2, Tp + 1, size=B)
    if variant == "short":
        q, _ = np.linalg.qr(weights(cell, shape)[ATT + "dense/kernel"].astype(np.float64))         # [Hd, A]: the directions the keys see
        d = np.random.RandomState(5).randn(SHORT_LEN, 2 * H) * 0.5
        x["enc"][0, :SHORT_LEN] = (x["enc"][0, 0].astype(np.float64) + d - (d @ q) @ q.T).astype(np.float32)
        x["enc_len"][0] = SHORT_LEN
    else:
        assert variant is None, variant
    x["y"] = rng.randint(3, V, size=(B, U))
    x["coins"], x["sampled"] = np.ones(U, bool), None
    if mixed:
        x["coins"] = rng.rand(U) < 0.5
        x["sampled"] = rng.randint(3, V, size=(B, U)).astype(np.int32)
    x["w"] = rng.randn(B, U, V).astype(np.float32)
    for v in x.values():
        if v is not None:
            v.setflags(write=False)
    return x


def run_oracle(cell, shape, rows, weights, inputs, mutate=None):
    """oracle.speller_forward + backward of sum(logits * w) in set_precision("bf16", rows) on the CPU.  mutate(weights, inputs) edits private
    copies first.  -> {"logits" [B, U, V], "alphas" [B, U, T'], "grads" {name: tensor, "enc": tensor}}"""
    from oracle import las_oracle as O
    if mutate is not None:
        weights = {n: np.array(v) for n, v in weights.items()}
        inputs = {n: None if v is None else np.array(v) for n, v in inputs.items()}
        mutate(weights, inputs)
    U = shape[6]
    O.set_precision("bf16", rows)
    try:
        po = O.to_torch(weights, requires_grad=True)
        enc = torch.tensor(np.asarray(inputs["enc"]), requires_grad=True)
        sampled = inputs["sampled"]
        lo, ao = O.speller_forward(enc, np.asarray(inputs["enc_len"]).astype(np.float64), U, po, speller_args(shape), cell,
                                   teacher=torch.tensor(np.asarray(inputs["y"])), is_training=True, coins=np.asarray(inputs["coins"]),
                                   sampled=None if sampled is None else torch.tensor(np.asarray(sampled)))
        (lo * torch.tensor(np.asarray(inputs["w"]))).sum().backward()
    finally:
        O.set_precision("f32")
    grads = {n: po[n].grad for n in po if po[n].grad is not None}
    grads["enc"] = enc.grad
    return {"logits": lo.detach(), "alphas": ao.detach(), "grads": grads}


def run_hip(cell, shape, flags, weights, inputs):
    """The Speller module (las_speller_fwd / las_speller_bwd) in speed mode on the same weights and inputs.
    -> (result as run_oracle's, {"fwd": families, "bwd": families} as _hip.speller_last_variant reports them).  The status word is the caller's."""
    from las import _hip, layers as L, variables as Vs
    from las.las import Speller
    U = shape[6]
    saved = _hip.speller_flags
    _hip.speller_flags = flags
    try:
        L.set_cell(cell)
        L.set_precision("bf16")
        st = Vs.reset_default_store(device="cuda", seed=3)
        st.load({n: np.array(v) for n, v in weights.items()})        # (writable copies: the case's arrays are read-only)
        sp = Speller(speller_args(shape))
        enc = torch.tensor(np.asarray(inputs["enc"]), device="cuda", requires_grad=True)
        x = {n: None if v is None else np.array(v) for n, v in inputs.items()}         # (writable copies, as above)
        logits, _, alphas = sp(enc, x["enc_len"], U, teacher=x["y"], is_training=True, coins=x["coins"], sampled=x["sampled"])
        fam = _hip.speller_last_variant()
        (logits * torch.tensor(np.asarray(inputs["w"])).cuda()).sum().backward()
        _hip.join_side_stream()
        torch.cuda.synchronize()
        fam["bwd"] = _hip.speller_last_variant()["bwd"]
        assert list(st.order) == list(weights), "the Speller created a variable the case does not supply"
        grads = {n: st.vars[n].grad.detach().cpu().clone() for n in st.order}
        grads["enc"] = enc.grad.detach().cpu().clone()
        return {"logits": logits.detach().cpu(), "alphas": alphas.detach().cpu(), "grads": grads}, fam
    finally:
        _hip.speller_flags = saved


def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-12))


def errors(got, ref):
    """{quantity: distance} of a result from a reference result:
      logits, alphas, grad/<name>          relative L2: |got - ref| / (|ref| + 1e-12)
      logits_max, alphas_max, gmax/<name>  the max-norm figures of tests/test_gpu_speller_bf16.py: |.|_max over max(1, |logits|_max); plain;
                                           over max(|gradient|_max, 1e-3)
      alpha_sum                            max |alphas.sum(-1) - 1| of `got`
    Only the gradients `ref` has are compared (a caller checks set(ref) <= set(got) itself)."""
    e = {"logits": _rel_l2(got["logits"], ref["logits"]), "alphas": _rel_l2(got["alphas"], ref["alphas"])}
    e["logits_max"] = float((got["logits"] - ref["logits"]).abs().max()) / max(1.0, float(ref["logits"].abs().max()))
    e["alphas_max"] = float((got["alphas"] - ref["alphas"]).abs().max())
    e["alpha_sum"] = float((got["alphas"].sum(-1) - 1).abs().max())
    for n in sorted(ref["grads"]):
        g, r = got["grads"][n], ref["grads"][n]
        e["grad/" + n] = _rel_l2(g, r)
        e["gmax/" + n] = float((g - r).abs().max()) / max(float(r.abs().max()), 1e-3)
    return e


FLOOR_SEEDS = (101, 202)
FLOOR_STEP = 1e-5


def floor(cell, shape, rows, weights, inputs, base=None):
    """The element-wise larger of errors(oracle(perturbed), oracle(base)) over two runs whose encoder input is moved by 1e-5 * randn."""
    base = run_oracle(cell, shape, rows, weights, inputs) if base is None else base
    out = {}
    for seed in FLOOR_SEEDS:
        def nudge(w, x, seed=seed):
            x["enc"] = x["enc"] + np.float32(FLOOR_STEP) * np.random.RandomState(seed).randn(*x["enc"].shape).astype(np.float32)
        e = errors(run_oracle(cell, shape, rows, weights, inputs, mutate=nudge), base)
        for k, v in e.items():
            out[k] = max(out.get(k, 0.0), v)
    del out["alpha_sum"]
    return out


def bound(floor):
    """{quantity: MARGIN x floor} (a floor of exactly 0: FP32_SUM_SLACK)"""
    return {k: (MARGIN * v if v > 0 else FP32_SUM_SLACK) for k, v in floor.items()}


def violations(err, bnd):
    """the quantities of `err` above their bound (and the alignment rows that do not sum to 1): [(quantity, error, bound)]"""
    bad = [(k, err[k], bnd[k]) for k in sorted(bnd) if not err[k] <= bnd[k]]
    if not err["alpha_sum"] < ALPHA_SUM_TOL:
        bad.append(("alpha_sum", err["alpha_sum"], ALPHA_SUM_TOL))
    return bad


# ---- the cached forms the tests share: one oracle run and one floor per (cell, shape, row arithmetic), never modified ----
def case_inputs(cell, shape, variant=None):
    return inputs(shape, variant, cell if variant else None)


@functools.lru_cache(maxsize=None)
def base_of(cell, shape, rows="bf", variant=None):
    return run_oracle(cell, shape, rows, weights(cell, shape), case_inputs(cell, shape, variant))


@functools.lru_cache(maxsize=None)
def floor_of(cell, shape, rows="bf", variant=None):
    return floor(cell, shape, rows, weights(cell, shape), case_inputs(cell, shape, variant), base=base_of(cell, shape, rows, variant))


# ---- mutations ----
# Every mutation changes the decoder state of some step, hence the logits and -- through h, tanh'(h), the query and the alignments of the
# later steps -- every gradient tensor except the one listed in UNREACHABLE; the per-mutation exclusions are tensors on which the edit's effect is
# second order for a stated reason.
UNREACHABLE = {VOCAB_B: "its gradient is sum_{b, u} w[b, u, :], whatever the model computes: floor 0, error 0"}


def _cell0(cell, shape):
    return cell_names(cell, shape[0])[0]


def _unit_columns(cell, shape, units):
    """the gate columns of hidden units `units` of the cell kernel / bias: one column per unit for the tanh cell, the unit's i, j, f and o
    columns for the LSTM (a kernel that gets unit d wrong gets all of d's gates wrong; ONE gate column of one LSTM unit moves the outputs
    by less than the flip floor -- measured 0.2-0.7 of the bound -- and no tolerance could tell it from rounding)"""
    D, G = shape[1], 4 if cell == "lstm" else 1
    return np.concatenate([g * D + np.asarray(units) for g in range(G)])


def _k_row(cell, shape):
    def f(w, x):
        w[_cell0(cell, shape)[0]][100] = 0            # a context row of [token | context | h] (E = 64 <= 100 < E + Hd)
    return f


def _k_col(cell, shape):
    def f(w, x):
        w[_cell0(cell, shape)[0]][:, _unit_columns(cell, shape, [shape[1] // 3])] = 0
    return f


def _k_rows_tail(cell, shape):
    def f(w, x):
        w[_cell0(cell, shape)[0]][-32:] = 0           # one 32-deep k-step of the recurrent part
    return f


def _k_cols_tail(cell, shape):
    def f(w, x):
        w[_cell0(cell, shape)[0]][:, _unit_columns(cell, shape, np.arange(shape[1] - 16, shape[1]))] = 0      # the last 16-column tile
    return f


def _bias_tile(cell, shape):
    def f(w, x):
        w[_cell0(cell, shape)[1]][_unit_columns(cell, shape, np.arange(16, 32))] = 0
    return f


def _enc_len(cell, shape):
    def f(w, x):
        x["enc_len"][0] -= 1                          # the attention mask one frame short for one utterance
    return f


def _coin(cell, shape):
    def f(w, x):
        x["coins"][0] = not x["coins"][0]             # step 1 reads the other token (teacher / sampled) in every row
    return f


def _conv_tap(cell, shape):
    def f(w, x):
        w[CONV_W][(shape[8][0] - 1) // 2] = 0         # the centre tap: f[t'] loses alpha_{t-1}[t'] w[centre]
    return f


def _wf_channel(cell, shape):
    def f(w, x):
        w[LOC_WF][0] = 0
    return f


_any = lambda cell, shape: True
_mixed = lambda cell, shape: bool(shape[7])
_loc = lambda cell, shape: shape[8] is not None

# name -> (applies(cell, shape), edit(cell, shape) -> f(weights, inputs), input variant, {gradient tensor it need not move: the reason})
# enc_len_minus_1 is measured on the "short" inputs: on the random lengths (T' / 2 .. T') the last frame of one utterance carries 1 / 30 to
# 1 / 150 of one row's context, and dropping it moves the batch's logits by a tenth of the bound -- what an off-by-one mask does to
# a SHORT utterance is what a test can see, so that is the input of this row (and of one row of the GPU table).
_EQUAL_KEYS = {n: "the short utterance's frames have equal keys, so its alignment is 1 / n whatever the query and u are: the only utterance "
                  "the edit touches sends no gradient through its attention to this tensor (additive attention; measured 0.02-0.2 of the bound)"
               for n in ("Speller/while/decode/attention/Variable", ATT + "dense_1/kernel")}
MUTATIONS = {
    "k_row_zeroed": (_any, _k_row, None, {}),
    "column_zeroed": (_any, _k_col, None, {}),
    "last_32_k_rows_zeroed": (_any, _k_rows_tail, None, {}),
    "last_16_columns_zeroed": (_any, _k_cols_tail, None, {}),
    "bias_tile_zeroed": (_any, _bias_tile, None, {}),
    "enc_len_minus_1": (_any, _enc_len, "short", _EQUAL_KEYS),
    "coin_flipped": (_mixed, _coin, None, {}),
    "conv_tap_zeroed": (_loc, _conv_tap, None, {}),
    "wf_channel_zeroed": (_loc, _wf_channel, None, {}),
}


def mutation_errors(cell, shape, name, rows="bf"):
    """-> (errors of the mutated oracle against the unmutated one, the floor of the inputs the mutation is measured on)"""
    applies, edit, variant, _ = MUTATIONS[name]
    assert applies(cell, shape), (name, shape)
    got = run_oracle(cell, shape, rows, weights(cell, shape), case_inputs(cell, shape, variant), mutate=edit(cell, shape))
    return errors(got, base_of(cell, shape, rows, variant)), floor_of(cell, shape, rows, variant)
