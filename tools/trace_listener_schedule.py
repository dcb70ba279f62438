#!/usr/bin/env python
"""What the Listener's host schedule enqueues, and what the step computes: one JSON line per case, to be compared between two commits
with `diff` (training is bit-reproducible run to run, so the comparison needs no tolerance).

The loaded library is wrapped in a recording proxy: every las_* call is noted as [symbol, current stream (main / side / chain / comm /
other), integer arguments] -- pointers only as "p" (set) or "0" (null); an argument struct contributes its integer fields.  Each case runs
three LAS.train steps under torch.manual_seed(0) at B = 8, T = 320 (13 x 3 features, up to 40 labels), vocab 30, dec_units 128, additive
attention, and records the call list of step 2, las.last_variants of each step, the three losses as hex floats and sha256 of the bytes of
the flat parameter and gradient buckets after each step.  Case 7 also runs the pyramid once forward and backward on an UNFLATTENED store (the
nodes' returned-gradient branches), in both precisions, and records the calls and the gradients' hashes.

Only names that every commit since the hand-overs exist has (_hip.lib, _hip.aux_streams, make_args, synthetic_batch, LAS.train, setattr
on the switches): the same file runs on an older checkout.

    python tools/trace_listener_schedule.py OUT.jsonl [case numbers ...]
    diff profiles/listener_schedule_refactor/parent.jsonl profiles/listener_schedule_refactor/this.jsonl"""
import ctypes, hashlib, json, os, sys, warnings
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "automatic-speech-recognition_amd"), os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)
import torch
from helpers import make_args, synthetic_batch
from las import _hip, layers as L, variables as V
from las.las import LAS, Listener, Speller
from oracle import las_oracle as O
warnings.simplefilter("ignore")

B, T = 8, 320
_INTS = (ctypes.c_int, ctypes.c_uint, ctypes.c_long, ctypes.c_ulong, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_size_t)


def _struct(s):
    out = []
    for name, typ in s._fields_:
        v = getattr(s, name)
        if typ in _INTS:
            out.append(int(v))
        elif typ is ctypes.c_float or typ is ctypes.c_double:
            out.append(float(v).hex())
        else:
            out.append("p" if v else "0")
    return out


def _arg(a, typ):
    if isinstance(a, ctypes.Array) and issubclass(a._type_, ctypes.Structure):
        return [_struct(s) for s in a]
    obj = getattr(a, "_obj", None)                       # ctypes.byref(struct)
    if isinstance(obj, ctypes.Structure):
        return _struct(obj)
    if typ in _INTS:
        return int(a)
    if typ is ctypes.c_float or typ is ctypes.c_double:
        return float(a).hex()
    if a is None or (isinstance(a, int) and a == 0) or (hasattr(a, "value") and not a.value):
        return "0"
    return "p"


class Recorder:
    """stands in for the ctypes library object: las_* calls go through, and are noted while `calls` is a list"""

    def __init__(self, real, streams):
        self._real, self._streams, self.calls = real, streams, None

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("las_"):
            return fn
        types = fn.argtypes or ()

        def call(*args):
            if self.calls is not None:
                cur = torch.cuda.current_stream().cuda_stream
                where = self._streams.get(cur, "main" if cur == torch.cuda.default_stream().cuda_stream else "other")
                self.calls.append([name, where] + [_arg(a, types[i] if i < len(types) else None) for i, a in enumerate(args)])
            return fn(*args)

        return call


def _sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().float().cpu().contiguous().numpy().tobytes()).hexdigest()


def train_case(rec, cell, prec, switches=None, **arch):
    kw = dict(enc_units=256, num_enc_layers=3, dec_units=128, num_dec_layers=1, embedding_size=64, attention_size=64, mode="add", lr=1e-3,
              grad_clip=5.0, label_smoothing=True, vocab_size=30)
    kw.update(arch)
    args = make_args(**kw)
    enc_type = str(args.enc_type).lower()
    xs, ys = synthetic_batch(B, T, 40, 30, seed=5, min_frac=0.9)
    p0 = O.init_params(args, seed=4, cell=cell, enc_type=enc_type)
    saved = {k: getattr(L, k) for k in (switches or {})}
    for k, v in (switches or {}).items():
        setattr(L, k, v)
    try:
        torch.manual_seed(0)
        L.set_cell(cell); L.set_precision(prec)
        st = V.reset_default_store(device="cuda"); st.load(p0)
        las = LAS(args, Listener, Speller, {})
        out = {"losses": [], "variants": [], "flat": [], "flat_grad": []}
        for step in range(3):
            rec.calls = [] if step == 1 else None
            loss = las.train(xs, ys)[0]
            torch.cuda.synchronize()
            if step == 1:
                out["calls"], rec.calls = rec.calls, None
            las.check_status()
            out["losses"].append(float(loss).hex())
            out["variants"].append(dict(las.last_variants))
            out["flat"].append(_sha(st.flat))
            out["flat_grad"].append(_sha(st.flat_grad))
        out["recovered_steps"] = las.recovered_steps
        return out
    finally:
        for k, v in saved.items():
            setattr(L, k, v)
        L.set_cell("rnn"); L.set_precision("f32")


def unflattened_pyramid(rec, prec, H=64, layers=2):
    """pBLSTMLayer forward + backward on a store that was never flattened: every node RETURNS its weight gradients"""
    g = torch.Generator().manual_seed(21)
    x = torch.randn(B, T, 39, generator=g).cuda()
    L.set_cell("lstm"); L.set_precision(prec)
    try:
        st = V.reset_default_store(device="cuda", seed=3)
        L.pBLSTMLayer(x, [T] * B, layers, H, 0.0, True)            # creates the variables
        _hip.join_side_stream()
        y, _, _ = L.pBLSTMLayer(x, [T] * B, layers, H, 0.0, True)
        dy = torch.randn(y.shape, generator=g).cuda() * 0.1
        rec.calls = []
        y.backward(dy)
        _hip.join_side_stream()
        torch.cuda.synchronize()
        calls, rec.calls = rec.calls, None
        _hip.check_status()
        return {"calls": calls, "grads": {n: _sha(st.vars[n].grad) for n in st.order}}
    finally:
        L.set_cell("rnn"); L.set_precision("f32")


def main():
    out_path = sys.argv[1]
    only = [int(a) for a in sys.argv[2:]]
    torch.cuda.set_device(0)
    real = _hip.lib()
    aux = _hip.aux_streams(torch.device("cuda", 0))
    rec = Recorder(real, {s.cuda_stream: n for n, s in aux.items()})
    _hip._lib = rec
    off = dict(XPROJ_CHUNK_STEPS=0, DOUT_CHUNK_ROWS=0, HOLD_SIDE=False, TAIL_TWO_STREAMS=False)
    cases = [(1, lambda: train_case(rec, "lstm", "bf16")),
             (2, lambda: train_case(rec, "lstm", "bf16", dropout_rate=0.1)),
             (3, lambda: train_case(rec, "lstm", "bf16", switches=dict(TAIL_WINDOW=64))),
             (4, lambda: train_case(rec, "lstm", "bf16", switches=off)),
             (5, lambda: train_case(rec, "lstm", "bf16", enc_units=64, num_enc_layers=2)),
             (6, lambda: train_case(rec, "rnn", "bf16", num_enc_layers=2)),
             (7, lambda: dict(train_case(rec, "lstm", "f32", enc_units=64, num_enc_layers=2),
                              unflattened_f32=unflattened_pyramid(rec, "f32"), unflattened_bf16=unflattened_pyramid(rec, "bf16"))),
             (8, lambda: train_case(rec, "lstm", "bf16", enc_type="cnn", enc_units=64, num_enc_layers=2, num_enc_channels=8))]
    with open(out_path, "w") as f:
        for n, run in cases:
            if only and n not in only:
                continue
            r = run()
            f.write(json.dumps(dict(case=n, **r), sort_keys=True) + "\n")
            f.flush()
            print("case %d: losses %s variants %s calls %d" % (n, r["losses"], r["variants"][1], len(r["calls"])), flush=True)


if __name__ == "__main__":
    main()
