"""Joint CTC-attention training beyond one step on one process: two data-parallel ranks, the reference's run.sh recipe at its sizes,
train.py / test.py with --ctc True, and beam search on a --ctc model."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import PKG, ROOT, grad_errors, make_args, row_mode, oracle_mode_for, synthetic_batch
import test_gpu_ctc as C

pytestmark = pytest.mark.gpu


def _dp_args():
    return make_args(enc_units=64, num_enc_layers=1, dec_units=64, num_dec_layers=1, embedding_size=32, attention_size=32, lr=1e-3,
                     ctc=True, ctc_weight=0.3)


def _dp_params(args):
    from oracle import las_oracle as O
    return dict(O.init_params(args, seed=7, cell="lstm"), **C._head_params(args, 2 * args.enc_units))


def _batches():
    # (a different lock-step global batch per step; the ranks' shards are rows rank, rank + 2, ...)
    return [synthetic_batch(6, 48 + 8 * k, 10, 30, seed=31 + k) for k in range(2)]


def _dp_worker(rank, world, port, out_path):
    for p in (PKG, ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from las import _hip, layers as L, variables as V
    from las.las import LAS, Listener, Speller
    from las.parallel import DataParallel
    _hip.speller_flags = _hip.SPELLER_NO_FUSED_STEP        # (two processes on one GPU: tests/test_gpu_dp.py)
    args = _dp_args()
    L.set_cell("lstm")
    L.set_precision("f32")
    st = V.reset_default_store(device="cuda:0")
    st.load(_dp_params(args))
    las = LAS(args, Listener, Speller, {})
    las.dp = DataParallel()
    las.build_variables()
    las.dp.broadcast_(st.flat)
    losses = []
    for xs, ys in _batches():
        sl = slice(rank, None, world)
        losses.append(float(las.train((xs[0][sl], xs[1][sl]), (ys[0][sl], ys[1][sl]))[0]))
    torch.cuda.synchronize()
    las.check_status()
    torch.save({"flat": st.flat.cpu(), "m": st.adam_m.cpu(), "v": st.adam_v.cpu(), "loss": losses}, out_path + ".%d" % rank)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_equal_stacked_and_concatenated_batches(tmp_path):
    """The global-batch rule under data parallelism: the dropped label belongs to the last rank's last row and the CTC term is divided by the
    global row count, so two ranks equal train_stacked of their shards, which equals train on the concatenated batch."""
    import torch.multiprocessing as mp
    from las import layers as L, variables as V
    from las.las import LAS, Listener, Speller
    out = str(tmp_path / "dp.pt")
    mp.spawn(_dp_worker, args=(2, 29300 + os.getpid() % 300, out), nprocs=2, join=True)
    got, got1 = torch.load(out + ".0"), torch.load(out + ".1")
    for k in ("flat", "m", "v"):
        assert torch.equal(got[k], got1[k]), k
    args = _dp_args()
    res = {}
    for form in ("stacked", "concatenated"):
        L.set_cell("lstm")
        L.set_precision("f32")
        st = V.reset_default_store(device="cuda")
        st.load(_dp_params(args))
        las = LAS(args, Listener, Speller, {})
        losses = []
        for xs, ys in _batches():
            shards = [((xs[0][r::2], xs[1][r::2]), (ys[0][r::2], ys[1][r::2])) for r in range(2)]
            if form == "stacked":
                losses.append(float(las.train_stacked(shards)[0]))
            else:
                xs_c = (np.concatenate([s[0][0] for s in shards]), np.concatenate([s[0][1] for s in shards]))
                ys_c = (np.concatenate([s[1][0] for s in shards]), np.concatenate([s[1][1] for s in shards]))
                losses.append(float(las.train(xs_c, ys_c)[0]))
        torch.cuda.synchronize()
        res[form] = (losses, st.flat.cpu().clone(), st.adam_m.cpu().clone(), st.adam_v.cpu().clone())
    ls, flat_s, m_s, v_s = res["stacked"]
    lc, flat_c, m_c, v_c = res["concatenated"]
    assert ls == lc and torch.equal(flat_s, flat_c) and torch.equal(m_s, m_c) and torch.equal(v_s, v_c)
    # the ranks against the single process (tolerances of tests/test_gpu_dp.py, f32)
    assert max(abs(a - b) for a, b in zip(got["loss"], ls)) < 2e-4
    assert (got["flat"] - flat_s).abs().max().item() < 6e-4
    assert (got["m"] - m_s).abs().max().item() < 1e-5 * max(1.0, m_s.abs().max().item())
    assert (got["v"] - v_s).abs().max().item() < 1e-6 * max(1.0, v_s.abs().max().item())


def test_run_sh_recipe_step_with_ctc_matches_oracle():
    """One step at the reference's run.sh recipe (tests/test_gpu_run_sh_recipe.py): B = 4, T = 1274 -> T' = 319, U ~ 190, V = 5000, with
    the CTC head [512, 5001].  Tolerances: that file's f32 row, and its absolute bound on the dense biases in front of a normalisation."""
    from oracle import las_oracle as O
    from test_gpu_run_sh_recipe import TOL, V, run_sh_args
    args = run_sh_args(ctc=True, ctc_weight=0.3)
    xs, ys = synthetic_batch(4, 1274, 256, V, seed=21, min_frac=0.834)
    U = int(ys[1].max())
    assert 150 < U <= 200
    coins = np.ones(U, bool)
    p0 = dict(O.init_params(args, seed=17, cell="rnn", enc_type="cnn"), **C._head_params(args, args.enc_units))
    r = C._hip_step(args, "rnn", "f32", p0, xs, ys, coins)
    O.set_precision(*oracle_mode_for(args, "f32", rows=row_mode(r["fam"])))
    try:
        loss_o, logits_o, g_o, newp = C._oracle_ctc_step(p0, args, "rnn", xs, ys, coins)
    finally:
        O.set_precision("f32")
    tol = TOL["f32"]
    assert (r["logits"] - logits_o).abs().max().item() < tol["logits"]
    assert abs(r["loss"] - loss_o) < tol["loss"] * max(1.0, abs(loss_o)), (r["loss"], loss_o)
    errs = grad_errors(dict(names=sorted(g_o), g_o=g_o, grads=r["grads"]))
    C._drop_zero_gradient_biases(errs, g_o, r["grads"], "f32")
    for n, e in errs.items():
        assert e < tol["grad"], (n, e)


def _cli(script, extra, tmp):
    cmd = [sys.executable, os.path.join(PKG, script), "--unit", "char", "--feat_dim", "13", "--enc_type", "pblstm",
           "--enc_units", "64", "--num_enc_layers", "2", "--dec_units", "64", "--num_dec_layers", "1",
           "--attention_size", "32", "--embedding_size", "32", "--dropout_rate", "0", "--cell", "lstm",
           "--tfrecord_dir", os.path.join(tmp, "rec"), "--save_dir", os.path.join(tmp, "model"),
           "--log_dir", os.path.join(tmp, "log"), "--feat_dir", os.path.join(tmp, "nofeats")] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=tmp)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_train_and_test_cli_with_ctc(tmp_path):
    """train.py --ctc True for two steps (tests/test_gpu_cli.py pattern), then test.py on that checkpoint with and without --ctc"""
    import tfrecord_data_loader as tdl
    tmp = str(tmp_path)
    os.makedirs(os.path.join(tmp, "rec"))
    rng = np.random.RandomState(0)
    lens = rng.randint(60, 120, size=8)
    feats = [rng.randn(n, 13, 3).astype(np.float32) for n in lens]
    toks = [np.r_[rng.randint(3, 30, size=max(2, n // 12)), 2].astype(np.int64) for n in lens]
    tdl.create_tfrecords(feats, toks, os.path.join(tmp, "rec", "train-100"), num_files=1)
    tdl.create_tfrecords(feats[:4], toks[:4], os.path.join(tmp, "rec", "dev"), num_files=1)
    out = _cli("train.py", ["--max_steps", "2", "--ctc", "True", "--ctc_weight", "0.3"], tmp)
    assert "Step: 1," in out and "Step: 2," in out
    assert os.path.exists(os.path.join(tmp, "model", "las_E1"))
    sd = torch.load(os.path.join(tmp, "model", "las_E1"), map_location="cpu", weights_only=True)
    assert "Speller/dense/kernel" in sd["params"] and float(sd["params"]["Speller/dense/kernel"].abs().max()) > 0
    a = _cli("test.py", ["--ctc", "True"], tmp)
    b = _cli("test.py", [], tmp)
    assert "total utterances: 4" in a and "total utterances: 4" in b
    pick = lambda o: [l.split("INFO:")[-1] for l in o.splitlines() if "WER" in l]
    assert pick(a) == pick(b)


def test_beam_search_ignores_the_head():
    """BeamSearch on a --ctc model gives exactly the hypotheses of the same weights built without the head"""
    from oracle import las_oracle as O
    from las import layers as L, variables as V
    from las.beam_search import BeamSearch
    from las.las import LAS, Listener, Speller
    from utils.tokenizer import CharEncoder
    outs = []
    for ctc in (True, False):
        args = C._cfg_args("pblstm", "add", ctc=ctc, convert_rate=0.3, beam_size=4, apply_lm=False)
        p0 = O.init_params(args, seed=11, cell="lstm", enc_type="pblstm")
        if ctc:
            p0.update(C._head_params(args, 2 * args.enc_units))
        L.set_cell("lstm")
        L.set_precision("f32")
        st = V.reset_default_store(device="cuda")
        st.load(p0)
        las = LAS(args, Listener, Speller, CharEncoder().token_to_id)
        las.build_variables()
        assert ("Speller/dense/kernel" in st.vars) == ctc
        utts = [synthetic_batch(1, T, 12, args.vocab_size, seed=8 + k)[0] for k, T in enumerate((64, 48, 56))]
        bs = BeamSearch(args, las, CharEncoder().token_to_id, None)
        outs.append([[(list(h.token_ids), float(h.log_prob)) for h in res] for res in bs.decode_batch(None, utts)])
    assert outs[0] == outs[1] and any(outs[0])
