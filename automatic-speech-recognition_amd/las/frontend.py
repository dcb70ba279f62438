"""las.frontend -- the audio front end on the device: a batch of waveforms -> the feature cube the Listener takes.

`FeatureExtractor(args).extract(waves)` is `preprocess.process_audios` (reference preprocess.py:71-86) for a batch of utterances of
different lengths in one call of las_frontend (csrc/frontend.hip): frames, 512-point power spectrum, mel filters, log + DCT (mfcc),
CMVN, the two derivative channels.  preprocess.py stays the float64 statement of the arithmetic; the tables the kernels read (mel
filterbank, DCT-II, twiddles) are computed from it in double on the host and rounded to fp32 once."""
import ctypes
import os
import sys

import numpy as np
import torch

from las import _hip

NFFT, NBINS, MFCC_FILTERS, MAX_FILTERS = 512, 257, 40, 128


def _preprocess():
    try:
        import preprocess
    except ImportError:                               # (imported as a package from outside the project directory)
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        import preprocess
    return preprocess


def frame_geometry(fs, frame_length_ms, frame_step_ms):
    """(samples per frame, samples per step) exactly as preprocess.stack_frames rounds them"""
    fl = int(np.round(fs * (frame_length_ms / 1000)))
    step = int(np.round(fs * (frame_step_ms / 1000)))
    return fl, step


def frame_count(n, fl, step):
    """preprocess.stack_frames: floor((n - fl) / step) -- the last full frame is dropped, as speechpy does"""
    return (n - fl) // step if n >= fl else 0


def host_tables(fs, feat_type, feat_dim):
    """{fb [nf, 257], fb_range int32 [nf, 2], dct [feat_dim, nf] or None, twiddle [257, 2]}, float32 roundings of float64 tables"""
    pp = _preprocess()
    if feat_type not in ("mfcc", "fbank"):
        raise ValueError(feat_type)
    nf = MFCC_FILTERS if feat_type == "mfcc" else int(feat_dim)
    if not 1 <= nf <= MAX_FILTERS:
        raise ValueError("the front end takes 1..%d mel filters (feat_dim %d)" % (MAX_FILTERS, feat_dim))
    if feat_type == "mfcc" and not 1 <= feat_dim <= MFCC_FILTERS:
        raise ValueError("mfcc keeps 1..%d cepstral coefficients (feat_dim %d)" % (MFCC_FILTERS, feat_dim))
    fb64 = pp.filterbanks(nf, NBINS, fs, 0, fs / 2)
    fb = fb64.astype(np.float32)
    rng = np.zeros((nf, 2), np.int32)
    for j in range(nf):
        nz = np.nonzero(fb[j])[0]
        rng[j] = (nz[0], nz[-1]) if len(nz) else (1, 0)
    dct = None
    if feat_type == "mfcc":
        # the orthonormal DCT-II preprocess.mfcc applies (scipy's, in double), as a matrix: row c = the weights of coefficient c
        from scipy.fftpack import dct as _dct
        dct = _dct(np.eye(nf), type=2, norm="ortho", axis=0)[:feat_dim].astype(np.float32)
    k = np.arange(NBINS, dtype=np.float64)
    tw = np.stack([np.cos(2 * np.pi * k / NFFT), -np.sin(2 * np.pi * k / NFFT)], 1).astype(np.float32)
    return {"fb": fb, "fb_range": rng, "dct": dct, "twiddle": tw, "num_filters": nf}


class FeatureExtractor:
    """reads sample_rate, frame_length, frame_step (ms), feat_type, feat_dim and cmvn from the flag namespace (las.arguments)"""

    def __init__(self, args, device=None):
        self.fs = int(args.sample_rate)
        self.feat_type = str(args.feat_type)
        self.feat_dim = int(args.feat_dim)
        self.cmvn = bool(args.cmvn)
        self.fl, self.step = frame_geometry(self.fs, args.frame_length, args.frame_step)
        if self.fl > NFFT:
            raise ValueError("a frame of %d samples (%d ms at %d Hz) does not fit the %d-point spectrum" % (self.fl, args.frame_length, self.fs, NFFT))
        if self.fl < 1 or self.step < 1:
            raise ValueError("frame of %d samples every %d" % (self.fl, self.step))
        self.tables = host_tables(self.fs, self.feat_type, self.feat_dim)
        self.device = device
        self._dev_tables = {}
        self._pinned = {}                     # device -> [[buffer, event of its last upload], ...]: two alternating staging buffers
        self._turn = 0

    # -- host side ---------------------------------------------------------------------------------------------------------------
    def frame_counts(self, n_samples):
        """int32 frame counts; ValueError for an utterance too short for one frame (before any launch)"""
        lens = np.asarray([frame_count(int(n), self.fl, self.step) for n in n_samples], np.int32)
        for u, t in enumerate(lens):
            if t < 1:
                raise ValueError("utterance %d has %d samples: too short for one frame (%d samples every %d; the last full frame is dropped)"
                                 % (u, int(n_samples[u]), self.fl, self.step))
        return lens

    @staticmethod
    def _as_numpy(w):
        if isinstance(w, torch.Tensor):
            w = w.detach().cpu().numpy()
        w = np.asarray(w)
        if w.ndim != 1:
            raise ValueError("a waveform is a 1-D array (got shape %s)" % (w.shape,))
        return w

    def _tables_on(self, dev):
        key = _hip._devkey(dev)
        t = self._dev_tables.get(key)
        if t is None:
            t = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(dev) if isinstance(v, np.ndarray) else v) for k, v in self.tables.items()}
            self._dev_tables[key] = t
        return t

    def _staging(self, dev, nbytes):
        """a pinned host buffer nobody is copying from: two alternate, each waits for ITS last upload only (an event, not the device)"""
        key = _hip._devkey(dev)
        slots = self._pinned.setdefault(key, [[None, None], [None, None]])
        self._turn ^= 1
        slot = slots[self._turn]
        if slot[1] is not None:
            slot[1].synchronize()
        if slot[0] is None or slot[0].numel() < nbytes:
            slot[0] = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8).pin_memory()
        return slot

    # -- the device path ---------------------------------------------------------------------------------------------------------
    def extract(self, waves, out=None):
        """waves: list of 1-D numpy arrays / tensors, float or int16 (int16: value / 32767, as read_audio scales 16-bit files).
        -> (cube, lens): cube float32 on the device, [n, Tmax, feat_dim, 3] (with cmvn) or [n, Tmax, feat_dim] (without), zeros behind
        each utterance's frames; lens int32 frame counts on the host.  One upload, launches on the current stream, no synchronisation.
        out: an optional contiguous float32 device tensor of exactly that shape to write into (every element of it is written)."""
        dev = torch.device(self.device if self.device is not None else "cuda")
        if dev.type != "cuda":
            raise RuntimeError("las.frontend needs a ROCm device (got %s); the CPU statement of the arithmetic is preprocess.process_audios" % dev)
        ws_np = [self._as_numpy(w) for w in waves]
        if not ws_np:
            raise ValueError("no waveforms")
        i16 = all(w.dtype == np.int16 for w in ws_np)
        if any(w.dtype.kind != "f" and w.dtype != np.int16 for w in ws_np):
            raise ValueError("waveforms are float or int16 arrays")
        if not i16 and any(w.dtype == np.int16 for w in ws_np):       # a mixed batch: the int16 rows scaled here as the kernel would
            ws_np = [(w.astype(np.float32) / np.float32(32767)) if w.dtype == np.int16 else w for w in ws_np]
        n = len(ws_np)
        ns = np.asarray([len(w) for w in ws_np], np.int32)
        lens = self.frame_counts(ns)
        Tmax, Nmax = int(lens.max()), int(ns.max())
        es = 2 if i16 else 4
        ld = (Nmax + 7) & ~7
        head = (4 * n + 255) & ~255
        nbytes = head + n * ld * es
        slot = self._staging(dev, nbytes)
        host = slot[0][:nbytes].numpy()
        host[:4 * n].view(np.int32)[:] = ns
        rows = host[head:].view(np.int16 if i16 else np.float32).reshape(n, ld)
        for u, w in enumerate(ws_np):
            rows[u, :ns[u]] = w                                       # (float64 / float16 input is rounded to fp32 here)
            rows[u, ns[u]:] = 0
        with torch.cuda.device(dev):
            buf = slot[0][:nbytes].to(dev, non_blocking=True)
            slot[1] = torch.cuda.Event()
            slot[1].record()
            D = self.feat_dim
            shape = (n, Tmax, D, 3) if self.cmvn else (n, Tmax, D)
            if out is None:
                out = torch.empty(shape, dtype=torch.float32, device=dev)
            elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
                raise ValueError("out must be a contiguous float32 device tensor of shape %s" % (shape,))
            need = int(_hip.lib().las_frontend_workspace_bytes(n, Tmax, D, int(self.cmvn)))
            ws = _hip.workspace(dev, need, _hip._tag("frontend")) if need else None
            t = self._tables_on(dev)
            ns_host = (ctypes.c_int * n)(*[int(x) for x in ns])
            a = _hip.FrontendArgs(
                samples=buf.data_ptr() + head, samples_i16=int(i16), ld_samples=ld, n_samples=buf.data_ptr(), n_samples_host=ns_host,
                n=n, Tmax=Tmax, fl=self.fl, step=self.step, feat_type=0 if self.feat_type == "mfcc" else 1, feat_dim=D,
                num_filters=t["num_filters"], cmvn=int(self.cmvn), twiddle=t["twiddle"].data_ptr(), fb=t["fb"].data_ptr(),
                fb_range=t["fb_range"].data_ptr(), dct=t["dct"].data_ptr() if t["dct"] is not None else None,
                out=out.data_ptr(), ws=ws.data_ptr() if ws is not None else None, ws_bytes=ws.numel() if ws is not None else 0)
            _hip.check(_hip.lib().las_frontend(ctypes.byref(a), _hip.stream()), "las_frontend")
        return out, lens
