"""bench_mvdr.py -- what the MVDR beamformer costs on the device: las_mvdr_mask, las_mvdr_cov, las_mvdr_weights and las_mvdr_apply
(csrc/mvdr.hip) on the generated one-hour, 8-channel, 16 kHz recording of tools/bench_beamform.py extended by one directional
interferer, next to (a) a device-to-device copy of the samples and (b) the float64 numpy restatement of the same four calls on the host
(tests/mvdr_ref.py), timed on the first --host_seconds of the recording and scaled to its length (all four calls are linear in it).

    python tools/bench_mvdr.py [--out profiles/mvdr_bench.json] [--seconds 3600] [--channels 8] [--reps 10] [--host_seconds 20]

The interferer is coloured noise (pole 0.5) from its own integer delays, 6 dB under a voice, throughout; --top_db 4 then separates the
frames with a voice from those without (the default of 25 would call every frame speech and the solve would have nothing to do).  Each
call is bracketed by device events behind a spin, as in bench_beamform.py; medians of --reps.  No target is fixed in advance: the file
records what was measured."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "automatic-speech-recognition_amd")
sys.path.insert(0, PKG)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def add_interferer(x, seed, level_db=-6.0):
    """x [C, n] += one directional source: AR(1) with pole 0.5 from its own delays within +-40 samples"""
    from scipy.signal import lfilter
    rng = np.random.RandomState(seed)
    C, n = x.shape
    pad = 64
    delays = rng.randint(-40, 41, size=C)
    delays[0] = 0
    s = lfilter([1.0], [1.0, -0.5], rng.standard_normal(n + 2 * pad))
    s = (0.05 * 10.0 ** (level_db / 20.0) * s / np.sqrt(np.mean(s * s))).astype(np.float32)
    for c in range(C):
        x[c] += s[pad - delays[c]:pad - delays[c] + n]
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mvdr_bench.json"))
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--rate", type=int, default=16000)
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--top_db", type=float, default=4.0)
    ap.add_argument("--host_seconds", type=float, default=20.0, help="length of the prefix the numpy restatement is timed on (0: skip it)")
    o = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mvdr.py measures on an MI355X: no device found")
    import bench_beamform as BB
    from las import _hip, beamform as BF
    from las.cli import BEAMFORM_DEFAULTS, MVDR_DEFAULTS as D0
    lib = _hip.lib()
    NF, Bf, hang = BF.mvdr_geometry(D0["mvdr_frame_ms"], D0["mvdr_block_ms"], D0["mvdr_pad_ms"], o.rate)
    ratio, floor, loading, ref, C = 10.0 ** (-o.top_db / 10.0), NF * 1e-7, D0["mvdr_loading"], BEAMFORM_DEFAULTS["bf_ref"], o.channels
    xh = add_interferer(BB.recording(o.seconds, o.rate, C, 0), 1)
    n = xh.shape[1]
    Tf = int(lib.las_mvdr_frames(n, NF))
    Nb, K = int(lib.las_mvdr_blocks(Tf, Bf)), NF // 2 + 1
    x = torch.from_numpy(xh).cuda()
    win, tw = (torch.from_numpy(t).cuda() for t in BF.mvdr_tables(NF))
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")
    m = torch.empty(Tf, dtype=torch.float32, device="cuda")
    counts, phi_n, phi_y, w = f64(1 + Nb), f64(K, C, C, 2), f64(Nb, K, C, C, 2), f64(Nb, K, C, 2)
    valid = torch.empty((Nb, K), dtype=torch.int32, device="cuda")
    y = torch.empty(n, dtype=torch.float32, device="cuda")
    nbytes = int(lib.las_mvdr_workspace_bytes(C, Tf, NF, Bf))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    P, st = _hip.p, _hip.stream
    mask = lambda: _hip.check(lib.las_mvdr_mask(P(x), 0, n, C, n, ref, NF, ratio, floor, hang, P(m), None, P(ws), nbytes, st()), "las_mvdr_mask")
    cov = lambda: _hip.check(lib.las_mvdr_cov(P(x), 0, n, C, n, NF, Bf, P(m), P(win), P(tw), P(counts), P(phi_n), P(phi_y), P(ws), nbytes, st()),
                             "las_mvdr_cov")
    wts = lambda: _hip.check(lib.las_mvdr_weights(P(phi_n), P(phi_y), P(counts), C, NF, Nb, ref, loading, P(w), P(valid), st()), "las_mvdr_weights")
    app = lambda: _hip.check(lib.las_mvdr_apply(P(x), 0, n, C, n, NF, Bf, P(w), P(win), P(tw), P(y), P(ws), nbytes, st()), "las_mvdr_apply")
    copy_to = torch.empty_like(x)
    t = BB.timed({"mask": mask, "cov": cov, "weights": wts, "apply": app, "copy": lambda: copy_to.copy_(x)}, o.reps)
    del copy_to
    m_h, cnt_h, valid_h = m.cpu().numpy(), counts.cpu().numpy(), valid.cpu().numpy()
    y_h = y.cpu().numpy()
    med = {k: v["median"] for k, v in t.items()}
    res = {"device": torch.cuda.get_device_name(0), "seconds": o.seconds, "rate": o.rate, "channels": C, "samples": n, "NF": NF, "Bf": Bf, "hang": hang,
           "frames": Tf, "blocks": Nb, "bins": K, "top_db": o.top_db, "loading": loading, "solves": Nb * K,
           "sample_bytes": int(xh.nbytes), "phi_y_bytes": int(phi_y.numel() * 8), "w_bytes": int(w.numel() * 8), "workspace_bytes": nbytes,
           "mask_s": t["mask"], "cov_s": t["cov"], "weights_s": t["weights"], "apply_s": t["apply"], "copy_s": t["copy"],
           "total_s": med["mask"] + med["cov"] + med["weights"] + med["apply"],
           "over_copy": {k: med[k] / med["copy"] for k in ("mask", "cov", "weights", "apply")},
           "cov_us_per_frame": med["cov"] / Tf * 1e6, "apply_us_per_frame": med["apply"] / Tf * 1e6,
           "weights_ns_per_solve": med["weights"] / (Nb * K) * 1e9,
           "speech_frames": float(m_h.mean()), "N0": float(cnt_h[0]), "valid_share": float(valid_h.mean()),
           "y_rms": float(np.sqrt(np.mean(y_h.astype(np.float64) ** 2))), "y_finite": bool(np.isfinite(y_h).all())}
    if o.host_seconds > 0:
        import mvdr_ref as R
        p = min(n, int(o.host_seconds * o.rate))
        xp = xh[:, :p]
        t0 = time.perf_counter()
        m_ref, _ = R.mask(xp, ref, NF, ratio, floor, hang)
        t1 = time.perf_counter()
        cnt_ref, pn_ref, py_ref = R.cov(xp, m_ref, NF, Bf)
        t2 = time.perf_counter()
        w_ref, valid_ref = R.weights(pn_ref, py_ref, cnt_ref, ref, loading)
        t3 = time.perf_counter()
        R.apply(xp, w_ref, NF, Bf)
        t4 = time.perf_counter()
        scale = n / float(p)
        host = {"mask": (t1 - t0) * scale, "cov": (t2 - t1) * scale, "weights": (t3 - t2) * scale, "apply": (t4 - t3) * scale}
        res.update(host_prefix_seconds=p / float(o.rate), host_scaled_to_recording_s=host,
                   host_over_device={k: host[k] / med[k] for k in host})
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
    with open(o.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
