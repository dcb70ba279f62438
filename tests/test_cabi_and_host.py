"""CPU-side checks of the boundary: the C-ABI library builds for gfx950 without a GPU, loads, and exports
exactly the symbols include/las_hip.h declares (no compute calls here); the host logic around it."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import helpers
from helpers import ROOT, PKG


@pytest.fixture(scope="module")
def libpath():
    subprocess.check_call(["make", "-C", os.path.join(PKG, "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    p = os.path.join(PKG, "lib", "liblas_hip.so")
    assert os.path.exists(p)
    return p


def _header_symbols():
    src = open(os.path.join(ROOT, "include", "las_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(las_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol(libpath):
    lib = ctypes.CDLL(libpath)
    names = _header_symbols()
    assert len(names) >= 18
    for n in names:
        assert hasattr(lib, n), "liblas_hip.so lacks %s" % n
    from las import _hip
    assert sorted(_hip.declared_symbols()) == names          # the ctypes table covers the whole header
    l = _hip.lib()
    hdr = open(os.path.join(helpers.ROOT, 'include', 'las_hip.h')).read()
    assert l.las_version() == _hip.ABI_VERSION == int(re.search(r'#define LAS_HIP_ABI_VERSION (\d+)', hdr).group(1))   # header, library, binding
    assert l.las_last_error() is not None
    # workspace queries are pure host arithmetic: callable without a GPU
    assert l.las_rnn_seq_workspace_bytes(1, 1, 256, 48) >= 2 * 4 * 256 * 256 * 4
    assert l.las_colsum_workspace_bytes(100) == 64 * 100 * 4
    assert l.las_speller_workspace_bytes(48, 160, 512, 128, 512, 1, 128, 30, 200, 1) > 0


def _sweep_args(_hip, **fields):
    """A las_rnn_seq_args that passes every check of both passes' common part (LSTM, bf16, H = 64, B = 8, T = 4) over fake, 16-byte
    aligned pointers: a call that is refused dereferences none of them."""
    a = _hip.RnnSeqArgs(cell=_hip.CELL_LSTM, prec=_hip.PREC_BF16, B=8, T=4, H=64, gates=0x10000, whh_fw=0x20000, whh_bw=0x30000, ldw=256,
                        out=0x40000, ld_out=128, out_bstride=4 * 128, cstate=0x50000, forget_bias=1.0, ws=0x60000,
                        ws_bytes=_hip.lib().las_rnn_seq_workspace_bytes(_hip.CELL_LSTM, _hip.PREC_BF16, 64, 8))
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def test_argument_validation_happens_before_any_launch(libpath):
    from las import _hip
    l = _hip.lib()
    rc = l.las_gemm(7, 0, 0, 4, 4, 4, 1.0, None, 4, 0, None, 4, 0, 0.0, None, 4, 0, None, 0, 1, 0, 0, None, 0, None)
    assert rc < 0 and b"bad prec" in l.las_last_error()
    rc = l.las_rnn_seq_fwd(ctypes.byref(_hip.RnnSeqArgs(cell=1, prec=0, B=0, T=4, H=8, ldw=8, ld_out=16, forget_bias=1.0)), None)
    assert rc < 0 and b"las_rnn_seq_fwd" in l.las_last_error()
    # One field of the argument struct each, refused by the check it belongs to.  A refusal (< 0) returns in front of the call's first
    # launch; a launch would give a hipError_t (> 0) without a device, and read the fake pointers with one.
    dout = dict(dout=0x70000, ld_dout=128, dout_bstride=4 * 128)
    for fn, fields, msg in (
            (l.las_rnn_seq_fwd, dict(row_T=0x80000, x_chunk_flag=0x90000, x_chunk_steps=2), b"las_rnn_seq_fwd: row_T and x_chunk_flag"),
            (l.las_rnn_seq_bwd, dict(dout, progress=0x80000, progress_steps=2), b"las_rnn_seq_bwd: progress needs a chunked upstream gradient"),
            (l.las_rnn_seq_fwd, dict(dout=0x70000), b"las_rnn_seq_fwd: a BPTT-only field"),
            (l.las_rnn_seq_bwd, dict(dout, row_T=0x80000), b"las_rnn_seq_bwd: a forward-only field"),
            (l.las_rnn_seq_bwd, dict(dout, ld_dout=127), b"las_rnn_seq_bwd: bad dout"),
            (l.las_rnn_seq_bwd, dict(dout, dout_chunk_flag=0x80000, dout_chunk_rows=3, dout_rows=4), b"las_rnn_seq_bwd: bad chunk geometry"),
            (l.las_rnn_seq_fwd, dict(ws_bytes=_sweep_args(_hip).ws_bytes - 1), b"workspace too small"),
            (l.las_rnn_seq_bwd, dict(dout, ws_bytes=_sweep_args(_hip).ws_bytes - 1), b"workspace too small")):
        rc = fn(ctypes.byref(_sweep_args(_hip, **fields)), None)
        assert rc < 0 and msg in l.las_last_error(), (fields, rc, l.las_last_error())
    assert l.las_rnn_seq_fwd(None, None) < 0 and b"las_rnn_seq_fwd: null argument struct" in l.las_last_error()
    assert l.las_rnn_seq_bwd(None, None) < 0 and b"las_rnn_seq_bwd: null argument struct" in l.las_last_error()


# include/las_hip.h's argument structs and the ctypes classes las/_hip.py lays out by hand for them
ABI_STRUCTS = {"las_gemm_plan_info": "GemmPlanInfo", "las_seq_prepare_desc": "SeqPrepareDesc", "las_rnn_seq_plan_info": "RnnSeqPlanInfo", "las_rnn_seq_args": "RnnSeqArgs",
               "las_speller_fwd_args": "SpellerFwdArgs", "las_speller_bwd_args": "SpellerBwdArgs", "las_shadow_desc": "ShadowDesc",
               "las_lstm_cell_args": "LstmCellArgs", "las_beam_loop_args": "BeamLoopArgs", "las_input_config": "InputConfig",
               "las_input_batch": "InputBatch", "las_frontend_args": "FrontendArgs", "las_resample_args": "ResampleArgs",
               "las_specaug_args": "SpecAugArgs"}


def test_ctypes_structures_have_the_layout_the_compiler_gives_the_header(tmp_path):
    """LAS_HIP_ABI_VERSION catches a stale library, not a slip in a hand-written _fields_ list: tests/native/abi_layout_main.cpp, built
    host-only with the Makefile's compiler, prints sizeof of every struct the header declares and offsetof / sizeof of every field, and
    each line must be what ctypes computes for the matching class (a Python field `in_` is the C field `in`; a nested struct is one
    field)."""
    from las import _hip
    exe = str(tmp_path / "abi_layout")
    r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-host-only", "-O1", "-std=c++17",
                        os.path.join(ROOT, "tests", "native", "abi_layout_main.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    sizes, fields = {}, {}
    for line in subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines():
        w = line.split()
        if w[0] == "struct":
            sizes[w[1]] = int(w[2])
        else:
            fields.setdefault(w[1], []).append((w[2], int(w[3]), int(w[4])))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "las_hip.h")).read(), flags=re.S)
    assert sorted(sizes) == sorted(ABI_STRUCTS) == sorted(re.findall(r"^}\s*(las_\w+);", hdr, flags=re.M))    # the program covers the header
    for cname, pyname in ABI_STRUCTS.items():
        cls = getattr(_hip, pyname)
        got = [(n.rstrip("_"), getattr(cls, n).offset, getattr(cls, n).size) for n, *_ in cls._fields_]
        assert got == fields[cname], (cname, [x for x in zip(got, fields[cname]) if x[0] != x[1]][:3], len(got), len(fields[cname]))
        assert ctypes.sizeof(cls) == sizes[cname], cname


def test_product_path_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("CPU-only check")
    from las import layers as L, variables as V
    from las.las import LAS, Listener, Speller
    V.reset_default_store()
    args = helpers.make_args(enc_units=8, dec_units=8, num_dec_layers=1)
    las = LAS(args, Listener, Speller, {})
    xs, ys = helpers.synthetic_batch(2, 8, 4, 30)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        las.train(xs, ys)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        L.dense(torch.zeros(2, 4), torch.zeros(4, 4))


def test_variable_store_flatten_and_checkpoint_roundtrip(tmp_path):
    from las import variables as V, checkpoint
    st = V.reset_default_store(device="cpu", seed=3)
    a = st.get("x/kernel", (3, 5))
    b = st.get("x/bias", (5,), init="zeros")
    u = st.get("u", (7,), init="uniform1")
    assert st.get("x/kernel") is a and float(a.abs().max()) <= (6 / 8) ** 0.5 + 1e-6 and float(u.abs().max()) <= 1
    with pytest.raises(ValueError):
        st.get("x/kernel", (5, 3))
    before = {n: st.vars[n].detach().clone() for n in st.order}
    st.flatten()
    assert st.flat.numel() % 4 == 0 and all(torch.equal(st.vars[n].detach(), before[n]) for n in st.order)
    assert all(st.offsets[n] % 4 == 0 for n in st.order)                       # 16-byte aligned views
    (a.sum() * 2 + (b * 3).sum()).backward()
    assert float(st.flat_grad.sum()) == 2 * 15 + 3 * 5                          # grads land in the flat bucket
    st.adam_m.fill_(0.5); st.global_step = 42
    path = checkpoint.save(str(tmp_path), 3)
    assert path.endswith("las_E3") and checkpoint.latest_checkpoint(str(tmp_path)) == path
    st2 = V.reset_default_store(device="cpu", seed=9)
    for n in st.order:
        st2.get(n, tuple(before[n].shape))
    assert checkpoint.restore(str(tmp_path), -1) == path
    assert st2.global_step == 42 and float(st2.adam_m[0]) == 0.5
    assert all(torch.equal(st2.vars[n].detach(), before[n]) for n in st.order)
    assert checkpoint.restore(str(tmp_path), 99) is None


def test_a_checkpoint_that_carries_pickled_code_is_refused(tmp_path):
    """checkpoint.restore loads with weights_only=True: a file at a checkpoint path whose pickle would call a function on load is rejected
    by the unpickler instead of executing it."""
    import pickle
    from las import variables as V, checkpoint
    V.reset_default_store(device="cpu", seed=1).get("w", (2,))
    marker = tmp_path / "ran"

    class Evil:
        def __reduce__(self):
            return (open, (str(marker), "w"))

    torch.save({"params": {"w": torch.zeros(2)}, "global_step": 0, "buffers": {}, "extra": Evil()}, str(tmp_path / "las_E1"))
    with pytest.raises(pickle.UnpicklingError):
        checkpoint.restore(str(tmp_path), 1)
    assert not marker.exists()


def test_schedules_match_oracle():
    from las import variables as V
    from las.las import LAS, Listener, Speller
    from oracle import las_oracle as O
    V.reset_default_store(device="cpu")
    args = helpers.make_args(scheduled_sampling=True)
    las = LAS(args, Listener, Speller, {})
    for gs in (0, 49999, 50000, 123456, 10 ** 7):
        assert las._scheduled_learning_rate(global_step=gs) == O.scheduled_learning_rate(args.lr, gs)
    for gs in (0, 100000, 250000, 500000, 900000):
        assert las.speller._scheduled_sampling(gs) == O.scheduled_sampling_rate(gs, args.warmup_step, args.max_step, args.min_rate)


def test_listener_output_length_matches_the_layers():
    """LAS.train uploads the encoder lengths before the Listener runs (host preparation); the helper must agree with what
    pBLSTMLayer / CNNLayer return (reference las/layers.py:94,:127-129)."""
    import numpy as np
    import torch
    from helpers import make_args
    from las.las import Listener
    a = make_args(num_enc_layers=3)
    n = np.array([1274, 1273, 1000, 7, 1])
    got = Listener(a).output_length(n, "pblstm")
    want = torch.as_tensor(n).to(torch.float64)
    for _ in range(3):
        want = (want + want % 2) / 2
    assert torch.equal(got, want) and got.dtype == torch.float64
    got_cnn = Listener(a).output_length(n, "cnn")
    want = torch.as_tensor(n).to(torch.float64)
    for _ in range(2):
        want = (want + want % 2) / 2
    assert torch.equal(got_cnn, want)


def test_bench_gpus_n_self_launch_refuses_without_enough_devices():
    """`python bench.py --gpus N` with WORLD_SIZE unset must start N ranks itself (torch.distributed.run children); with
    fewer than N devices visible it exits non-zero with a message instead of silently running one rank."""
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 2 and "--gpus 2 requested" in r.stderr and '"metric"' not in r.stdout
    # under a launcher the rank count must agree with --gpus
    env2 = dict(env, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=300, env=env2)
    assert r.returncode != 0 and "WORLD_SIZE=2" in (r.stderr + r.stdout)


def test_bench_dump_outputs_float32_within_budget_and_reproducible(tmp_path):
    """bench.py --dump-outputs: every array float32, an oversized one replaced by the same seeded sample in every run, 64 MB at most
    in all -- here at config 3's vocabulary (V = 5000: the logits alone are 183 MB)."""
    import importlib.util
    import types
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    g = torch.Generator().manual_seed(0)
    las = types.SimpleNamespace(last_out=(torch.tensor(3.25), None, 25, torch.randn(48, 191, 5000, generator=g),
                                          torch.rand(48, 191, 160, generator=g), {}, 1.0))
    st = types.SimpleNamespace(flat=torch.randn(9679776, generator=g), flat_grad=torch.randn(9679776, generator=g))
    runs = []
    for k in range(2):
        d = str(tmp_path / ("d%d" % k))
        bench.dump_outputs(d, las, st)
        runs.append({f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))})
        assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64e6
    assert sorted(runs[0]) == ["alphas.npy", "grads_sample.npy", "logits_sample.npy", "loss.npy", "params.npy"]
    for f, a in runs[0].items():
        assert a.dtype == np.float32 and np.array_equal(a, runs[1][f]), f
    assert float(runs[0]["loss.npy"]) == 3.25 and np.array_equal(runs[0]["params.npy"], st.flat.numpy())
    assert runs[0]["logits_sample.npy"].size == bench.DUMP_CAP["logits"]
    assert np.isin(runs[0]["logits_sample.npy"], las.last_out[3].numpy()).all()


def test_sampling_seed_is_per_rank_and_per_step():
    from las.parallel import sampling_seed
    seen = {sampling_seed(s, r) for s in range(50) for r in range(8)}
    assert len(seen) == 400


def test_timed_speller_loop_kernels_leave_room_for_a_foreign_wave_on_every_cu():
    """The one-launch Speller loops put one 1024-thread workgroup on EVERY compute unit and poll each other: all of them must be
    resident at once.  At 121-128 VGPRs per lane such a workgroup needs a CU's whole register file and could not share the CU with a
    single small wave of anybody else.  The compiler's report of the shipped object (csrc/build/speller.res, written by the Makefile)
    must show the additive-attention kernels of the timed geometry (T' <= 160: NE = 8, 10; lstm and rnn cells) at <= 120.  (A budget,
    not a cure: the exchange time-outs seen when several processes share one device -- tests/test_gpu_zz_eight_ranks_host.py -- occur at
    120 registers too.)"""
    import re
    res = os.path.join(ROOT, "automatic-speech-recognition_amd", "csrc", "build", "speller.res")
    if not os.path.exists(res):
        pytest.skip("no compiler report next to the object (the library was not built by csrc/Makefile here)")
    cur, vg = None, {}
    for line in open(res):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
        m = re.search(r"\bVGPRs: (\d+)", line)
        if m and cur:
            vg[cur] = int(m.group(1))
    seen = 0
    for name, n in vg.items():
        m = re.match(r"_Z19dec_loop_(fwd|bwd)_kernelILi([01])ELi(8|10)ELb0EEv6DecDev", name)
        if m:
            seen += 1
            assert n <= 120, (name, n)
    assert seen == 8, sorted(vg)
