"""las.frontend -- the audio front end on the device: a batch of waveforms -> the feature cube the Listener takes.

`FeatureExtractor(args).extract(waves)` is `preprocess.process_audios` (reference preprocess.py:71-86) for a batch of utterances of
different lengths in one call of las_frontend (csrc/frontend.hip): frames, 512-point power spectrum, mel filters, log + DCT (mfcc),
CMVN, the two derivative channels.  preprocess.py stays the float64 statement of the arithmetic; the tables the kernels read (mel
filterbank, DCT-II, twiddles) are computed from it in double on the host and rounded to fp32 once.

`Resampler(fs_in, fs_out)` is `preprocess.resample` in one launch of las_resample (csrc/resample.hip): a band-limited polyphase
resampler with a per-utterance gain.  `extract(waves, rate=..., speed=..., gain=...)` puts it in front of las_frontend: recordings at
another sample rate, and the reference's speed / volume augmentation (sox `speed s` = declared at fs * s, resampled to fs)."""
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


def _align(n, a=256):
    return (int(n) + a - 1) & ~(a - 1)


class Resampler:
    """fs_in -> fs_out on the device.  Holds L, M, W (K = 2W taps) and the fp32 rounding of preprocess.resample_table's float64 table."""

    def __init__(self, fs_in, fs_out, device=None):
        self.fs_in, self.fs_out = int(fs_in), int(fs_out)
        self.L, self.M, self.W, h = _preprocess().resample_table(self.fs_in, self.fs_out)
        self.K = 2 * self.W
        self.table = np.ascontiguousarray(h, dtype=np.float32)
        self.device = device
        self._dev_table = {}

    def out_len(self, n):
        """ceil(n L / M): samples of the resampled recording"""
        return int(_hip.lib().las_resample_out_len(int(n), self.L, self.M))

    def tile(self):
        """consecutive outputs of one utterance a workgroup of las_resample owns"""
        return int(_hip.lib().las_resample_tile(self.L, self.M, self.W))

    def _table_on(self, dev):
        key = _hip._devkey(dev)
        t = self._dev_table.get(key)
        if t is None:
            t = self._dev_table[key] = torch.from_numpy(self.table).to(dev)
        return t

    def launch(self, dev, src, i16, ld_in, n_in, n_in_host, n, out, ld_out, gain=None, n_out=None):
        """las_resample on the current stream; src, n_in, out, gain and n_out are device addresses (ints), n_in_host a sequence"""
        ns_host = (ctypes.c_int * n)(*[int(x) for x in n_in_host])
        a = _hip.ResampleArgs(in_=src, in_i16=int(i16), ld_in=int(ld_in), n_in=n_in, n_in_host=ns_host, n=n, L=self.L, M=self.M, W=self.W,
                              table=self._table_on(dev).data_ptr(), gain=gain, out=out, ld_out=int(ld_out), n_out=n_out)
        _hip.check(_hip.lib().las_resample(ctypes.byref(a), _hip.stream()), "las_resample")

    def __call__(self, waves, gain=None, out=None):
        """waves: list of 1-D float or int16 arrays -> (samples float32 [n, ld_out] on the device, zeros behind each row's length;
        lengths int32 [n] on the device, written by the kernel).  gain: None, a scalar or one value per row.  out: an optional
        contiguous float32 device tensor [n, ld_out >= the longest result] to write into (every element of it is written)."""
        dev = torch.device(self.device if self.device is not None else "cuda")
        if dev.type != "cuda":
            raise RuntimeError("las.frontend needs a ROCm device (got %s); the CPU statement of the arithmetic is preprocess.resample" % dev)
        ws_np = [FeatureExtractor._as_numpy(w) for w in waves]
        if not ws_np:
            raise ValueError("no waveforms")
        if any(w.dtype.kind != "f" and w.dtype != np.int16 for w in ws_np):
            raise ValueError("waveforms are float or int16 arrays")
        i16 = all(w.dtype == np.int16 for w in ws_np)
        if not i16:
            ws_np = [(w.astype(np.float32) / np.float32(32767)) if w.dtype == np.int16 else w for w in ws_np]
        n = len(ws_np)
        ns = [len(w) for w in ws_np]
        if min(ns) < 1:
            raise ValueError("an empty waveform")
        ld = (max(ns) + 7) & ~7
        rows = np.zeros((n, ld), np.int16 if i16 else np.float32)
        for u, w in enumerate(ws_np):
            rows[u, :ns[u]] = w
        need = max(self.out_len(x) for x in ns)
        with torch.cuda.device(dev):
            src = torch.from_numpy(rows).to(dev)
            n_in = torch.tensor(ns, dtype=torch.int32).to(dev)
            g = None
            if gain is not None:
                g = torch.from_numpy(np.broadcast_to(np.asarray(gain, np.float32), (n,)).copy()).to(dev)
            if out is None:
                out = torch.empty((n, (need + 7) & ~7), dtype=torch.float32, device=dev)
            elif out.dim() != 2 or out.shape[0] != n or out.shape[1] < need or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
                raise ValueError("out must be a contiguous float32 device tensor [%d, >= %d]" % (n, need))
            n_out = torch.empty(n, dtype=torch.int32, device=dev)
            self.launch(dev, src.data_ptr(), i16, ld, n_in.data_ptr(), ns, n, out.data_ptr(), out.shape[1],
                        gain=g.data_ptr() if g is not None else None, n_out=n_out.data_ptr())
        return out, n_out


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
        self._resamplers = {}                 # (fs_in, fs_out) -> Resampler

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

    def resampler(self, fs_in):
        key = (int(fs_in), self.fs)
        r = self._resamplers.get(key)
        if r is None:
            r = self._resamplers[key] = Resampler(key[0], key[1], self.device)
        return r

    @staticmethod
    def _per_row(v, n, what, kind):
        a = np.asarray(v, kind)
        if a.ndim > 1 or (a.ndim == 1 and len(a) != n):
            raise ValueError("%s is a scalar or one value per utterance (%d), got shape %s" % (what, n, a.shape))
        return np.broadcast_to(a, (n,))

    # -- the device path ---------------------------------------------------------------------------------------------------------
    def extract(self, waves, out=None, rate=None, speed=1.0, gain=None, augment=None):
        """waves: list of 1-D numpy arrays / tensors, float or int16 (int16: value / 32767, as read_audio scales 16-bit files).
        -> (cube, lens): cube float32 on the device, [n, Tmax, feat_dim, 3] (with cmvn) or [n, Tmax, feat_dim] (without), zeros behind
        each utterance's frames; lens int32 frame counts on the host.  One upload, launches on the current stream, no synchronisation.
        out: an optional contiguous float32 device tensor of exactly that shape to write into (every element of it is written).
        rate: the recordings' sample rate(s), a scalar or one per utterance (default: self.fs); speed: sox's `speed` -- row u is taken
        to be at int(round(rate_u * speed)) Hz; gain: a scalar or one factor per utterance.  When every effective rate is self.fs and
        no gain is given, nothing is resampled and the launches are those of the defaults.  Otherwise EVERY row goes through
        las_resample, one call per run of consecutive rows at one effective rate, into an fp32 sample buffer that las_frontend then
        reads (it takes one buffer): a row already at self.fs takes the L = M = 1 kernel, which filters nothing -- with no gain a
        bit copy, at the price of one more launch per such run.  Frame counts come from the resampled lengths, on the host, before
        any launch.
        augment: a las.augment.AugPlan (WaveAugmenter.plan) or None.  With a plan every row takes the resample path too (so the samples
        are fp32), and the fp32 sample buffer then goes through las_reverb and las_noise_mix (one more small upload, up to four more
        launches) before las_frontend reads it: room reverberation, then noise at the drawn SNR.  Lengths and frame counts do not change."""
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
        eff = np.full(n, self.fs, np.int64)
        if rate is not None or speed != 1.0:
            r = self._per_row(self.fs if rate is None else rate, n, "rate", np.float64)
            eff = np.asarray([int(round(float(x) * float(speed))) for x in r], np.int64)
            if eff.min() < 1:
                raise ValueError("effective sample rates %s" % (eff.tolist(),))
        gains = None if gain is None else self._per_row(gain, n, "gain", np.float32)
        resampled = gains is not None or augment is not None or bool((eff != self.fs).any())
        ns_fe = ns
        if resampled:
            if int(ns.min()) < 1:
                raise ValueError("an empty waveform")
            ns_fe = np.asarray([self.resampler(eff[u]).out_len(ns[u]) for u in range(n)], np.int32)
        lens = self.frame_counts(ns_fe)                               # (of the resampled lengths)
        Tmax, Nmax = int(lens.max()), int(ns.max())
        es = 2 if i16 else 4
        ld = (Nmax + 7) & ~7
        head = _align(4 * n) + (_align(4 * n) if gains is not None else 0)
        nbytes = head + n * ld * es
        slot = self._staging(dev, nbytes)
        host = slot[0][:nbytes].numpy()
        host[:4 * n].view(np.int32)[:] = ns
        if gains is not None:
            host[_align(4 * n):_align(4 * n) + 4 * n].view(np.float32)[:] = gains
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
            samples, n_samples = buf.data_ptr() + head, buf.data_ptr()
            if resampled:
                # [resampled lengths int32 [n] | fp32 samples [n, ld_fe]]; rows at self.fs take the gain-only path (a copy)
                ld_fe = (int(ns_fe.max()) + 7) & ~7
                rs = _hip.workspace(dev, _align(4 * n) + 4 * n * ld_fe, _hip._tag("frontend_resample"))
                u0 = 0
                while u0 < n:
                    u1 = u0 + 1
                    while u1 < n and eff[u1] == eff[u0]:
                        u1 += 1
                    self.resampler(eff[u0]).launch(
                        dev, samples + u0 * ld * es, i16, ld, n_samples + 4 * u0, ns[u0:u1], u1 - u0,
                        rs.data_ptr() + _align(4 * n) + 4 * u0 * ld_fe, ld_fe,
                        gain=buf.data_ptr() + _align(4 * n) + 4 * u0 if gains is not None else None, n_out=rs.data_ptr() + 4 * u0)
                    u0 = u1
                samples, n_samples, i16, ld = rs.data_ptr() + _align(4 * n), rs.data_ptr(), False, ld_fe
                if augment is not None:
                    if len(augment) != n or augment.augmenter.fs != self.fs:
                        raise ValueError("augment: a plan of %d rows at %d Hz for %d utterances at %d Hz" % (len(augment), augment.augmenter.fs, n, self.fs))
                    clean = rs[_align(4 * n):_align(4 * n) + 4 * n * ld_fe].view(torch.float32).view(n, ld_fe)
                    samples = augment.augmenter.apply(clean, ns_fe, augment).data_ptr()
            ns_host = (ctypes.c_int * n)(*[int(x) for x in ns_fe])
            a = _hip.FrontendArgs(
                samples=samples, samples_i16=int(i16), ld_samples=ld, n_samples=n_samples, n_samples_host=ns_host,
                n=n, Tmax=Tmax, fl=self.fl, step=self.step, feat_type=0 if self.feat_type == "mfcc" else 1, feat_dim=D,
                num_filters=t["num_filters"], cmvn=int(self.cmvn), twiddle=t["twiddle"].data_ptr(), fb=t["fb"].data_ptr(),
                fb_range=t["fb_range"].data_ptr(), dct=t["dct"].data_ptr() if t["dct"] is not None else None,
                out=out.data_ptr(), ws=ws.data_ptr() if ws is not None else None, ws_bytes=ws.numel() if ws is not None else 0)
            _hip.check(_hip.lib().las_frontend(ctypes.byref(a), _hip.stream()), "las_frontend")
        return out, lens
