"""las.augment -- multi-condition training data on the device: room reverberation and additive noise at a drawn signal-to-noise ratio,
between the resampler and the front end (csrc/wave_aug.hip: las_reverb, las_noise_mix).  What Kaldi's reverberate_data_dir.py and the
RIR / noise stages of ESPnet and Lhotse do on the CPU.

The kernels apply a PLAN and draw nothing; `WaveAugmenter.plan` draws it on the host, keyed by (seed, step) only, a row's draw
depending on its global index and not on the batch it arrives in (as las.specaug does).  preprocess.reverberate / mix_noise are the
float64 statement of the arithmetic; preprocess.augment_wave applies a plan's row with them.  Nothing imports this module unless a
plan is asked for: `FeatureExtractor.extract(..., augment=plan)`, preprocess.py --noisy_copies, transcribe.py --noise_file / --rir_file."""
import ctypes

import numpy as np
import torch

from las import _hip
from las.frontend import _preprocess

RIR_MAX = 16384         # csrc/wave_aug.hip: taps of one response (one second at 16 kHz)
N_DRAWS = 6


def _index(u, n):
    """floor(u * n) for u in [0, 1), kept below n"""
    return np.minimum(np.floor(u * n).astype(np.int64), np.maximum(n - 1, 0))


def _bank(rows):
    """float32 [len(rows), ld] (ld a multiple of 8, zeros behind each row) and the int32 lengths"""
    lens = np.asarray([len(r) for r in rows], np.int32)
    ld = (int(lens.max()) + 7) & ~7
    bank = np.zeros((len(rows), ld), np.float32)
    for i, r in enumerate(rows):
        bank[i, :len(r)] = r
    return bank, lens


class AugPlan:
    """per utterance: rir_idx, noise_idx (int32, -1 = none), noise_off (int32), snr_db (float32); `augmenter` holds the banks"""

    def __init__(self, augmenter, rir_idx, noise_idx, noise_off, snr_db):
        self.augmenter = augmenter
        self.rir_idx = np.ascontiguousarray(rir_idx, dtype=np.int32)
        self.noise_idx = np.ascontiguousarray(noise_idx, dtype=np.int32)
        self.noise_off = np.ascontiguousarray(noise_off, dtype=np.int32)
        self.snr_db = np.ascontiguousarray(snr_db, dtype=np.float32)
        n = len(self.rir_idx)
        if not (self.rir_idx.shape == self.noise_idx.shape == self.noise_off.shape == self.snr_db.shape == (n,)):
            raise ValueError("a plan holds one rir_idx, noise_idx, noise_off and snr_db per utterance")

    def __len__(self):
        return len(self.rir_idx)


class WaveAugmenter:
    """rirs, noises: lists of 1-D arrays at fs Hz.  A response is cut to 16384 taps, scaled to unit energy in float64
    (preprocess.normalize_rir) and aligned at its direct path (preprocess.rir_delay); both banks are rounded to fp32 and uploaded once
    per device."""

    def __init__(self, fs, rirs=None, noises=None, snr_db=(5, 20), reverb_prob=0.5, noise_prob=1.0, seed=0, device=None):
        pp = _preprocess()
        self.fs = int(fs)
        self.rirs = [pp.normalize_rir(np.asarray(h, dtype=float)[:RIR_MAX]) for h in (rirs or [])]
        self.rir_delay = [pp.rir_delay(h) for h in self.rirs]
        self._rir_delay = np.asarray(self.rir_delay, np.int32)
        self.noises = [np.asarray(v, dtype=float) for v in (noises or [])]
        if any(v.ndim != 1 or len(v) < 1 for v in self.noises):
            raise ValueError("a noise recording is a non-empty 1-D array")
        self.snr_lo, self.snr_hi = float(snr_db[0]), float(snr_db[1])
        self.reverb_prob, self.noise_prob = float(reverb_prob), float(noise_prob)
        if not (np.isfinite([self.snr_lo, self.snr_hi]).all() and self.snr_lo <= self.snr_hi):
            raise ValueError("snr_db is (lo, hi), finite, lo <= hi (got %s)" % (snr_db,))
        if not (0.0 <= self.reverb_prob <= 1.0 and 0.0 <= self.noise_prob <= 1.0):
            raise ValueError("reverb_prob %g and noise_prob %g are probabilities" % (self.reverb_prob, self.noise_prob))
        self.seed = int(seed)
        self.device = device
        self.rir_bank, self.rir_len = _bank(self.rirs) if self.rirs else (None, None)
        self.noise_bank, self.noise_len = _bank(self.noises) if self.noises else (None, None)
        self._dev = {}                        # device -> the banks, their lengths and delays as device tensors
        self._pinned = {}                     # device -> two alternating pinned staging buffers, each with the event of its last upload
        self._turn = 0

    # -- the draws (host) --------------------------------------------------------------------------------------------------------
    def plan(self, n, step, row0=0, rows_global=None):
        """the draws of rows [row0, row0 + n) of a global batch.  The recipe:

          u = numpy.random.Generator(numpy.random.Philox(key=[seed mod 2^64, step mod 2^64])).random((rows_global, 6)), float64 in [0, 1),
          filled row by row; the caller's row b is row row0 + b of that block (rows_global defaults to row0 + n), so a global row draws
          the same numbers however the batch is split.  With idx(u, n) = min(floor(u n), n - 1):
            rir_idx   = idx(u[1], R) if u[0] < reverb_prob and there are R > 0 responses, else -1
            noise_idx = idx(u[3], N) if u[2] < noise_prob and there are N > 0 noises, else -1
            noise_off = idx(u[4], len(noise[noise_idx])) (0 without noise)
            snr_db    = float32(lo + u[5] (hi - lo))
        All six numbers are drawn either way."""
        n, row0 = int(n), int(row0)
        rows_global = row0 + n if rows_global is None else int(rows_global)
        if n < 0 or row0 < 0 or row0 + n > rows_global:
            raise ValueError("augment: rows [%d, %d) of a global batch of %d" % (row0, row0 + n, rows_global))
        key = np.array([self.seed % (1 << 64), int(step) % (1 << 64)], dtype=np.uint64)
        u = np.random.Generator(np.random.Philox(key=key)).random((rows_global, N_DRAWS))[row0:row0 + n]
        R, N = len(self.rirs), len(self.noises)
        rir_idx = np.where((u[:, 0] < self.reverb_prob) & (R > 0), _index(u[:, 1], np.int64(R)), -1)
        noise_idx = np.where((u[:, 2] < self.noise_prob) & (N > 0), _index(u[:, 3], np.int64(N)), -1)
        lens = self.noise_len.astype(np.int64)[np.maximum(noise_idx, 0)] if N else np.ones(n, np.int64)
        noise_off = np.where(noise_idx >= 0, _index(u[:, 4], lens), 0)
        snr = (self.snr_lo + u[:, 5] * (self.snr_hi - self.snr_lo)).astype(np.float32)
        return AugPlan(self, rir_idx, noise_idx, noise_off, snr)

    def fixed_plan(self, n, rir_idx=-1, noise_idx=-1, noise_off=0, snr_db=0.0):
        """a plan that draws nothing: the same choice (or one per row) for n utterances"""
        b = lambda v, t: np.broadcast_to(np.asarray(v, t), (int(n),)).copy()
        return AugPlan(self, b(rir_idx, np.int32), b(noise_idx, np.int32), b(noise_off, np.int32), b(snr_db, np.float32))

    # -- the device path ---------------------------------------------------------------------------------------------------------
    def _banks_on(self, dev):
        key = _hip._devkey(dev)
        d = self._dev.get(key)
        if d is None:
            up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            d = self._dev[key] = {"rir": up(self.rir_bank), "rir_len": up(self.rir_len),
                                  "rir_delay": up(self._rir_delay if self.rirs else None),
                                  "noise": up(self.noise_bank), "noise_len": up(self.noise_len)}
        return d

    def _staging(self, dev, nbytes):
        """a pinned host buffer nobody is copying from: two alternate, each waits for ITS last upload only (an event, not the device)"""
        slots = self._pinned.setdefault(_hip._devkey(dev), [[None, None], [None, None]])
        self._turn ^= 1
        slot = slots[self._turn]
        if slot[1] is not None:
            slot[1].synchronize()
        if slot[0] is None or slot[0].numel() < nbytes:
            slot[0] = torch.empty(max(nbytes, 4096), dtype=torch.uint8).pin_memory()
        return slot

    def apply(self, samples, n_samples, plan, out=None, gain_out=None):
        """las_reverb, then las_noise_mix, of a plan on the current stream: one pinned asynchronous upload of the lengths and the plan
        (20 bytes per utterance), the launches, no synchronisation.  samples: a contiguous float32 device tensor [n, ld]; n_samples: the
        rows' lengths on the host.  Returns a tensor of samples' shape in the 'augment' workspace -- valid until the next call on this
        stream -- or `out`, a contiguous float32 device tensor of that shape that does not overlap samples.  Every element of it is
        written: the augmented recording, zeros behind its length.  gain_out: an optional float32 device tensor [n] for the noise gains."""
        if not torch.is_tensor(samples) or not samples.is_cuda:
            raise RuntimeError("las.augment needs a tensor on a ROCm device; the CPU statement of the arithmetic is preprocess.augment_wave")
        if samples.dtype != torch.float32 or samples.dim() != 2 or not samples.is_contiguous():
            raise ValueError("augment: samples is a contiguous float32 [n, ld] tensor (got %s %s)" % (samples.dtype, tuple(samples.shape)))
        if plan.augmenter is not self:
            raise ValueError("augment: the plan was drawn by another WaveAugmenter (its indices point into that one's banks)")
        n, ld = samples.shape
        ns = np.asarray(n_samples, np.int32).reshape(-1)
        if len(ns) != n or len(plan) != n:
            raise ValueError("augment: %d rows, %d lengths, a plan of %d" % (n, len(ns), len(plan)))
        if self.rir_bank is None and self.noise_bank is None:
            raise ValueError("augment: neither responses nor noises to apply")
        if (self.rir_bank is None and (plan.rir_idx >= 0).any()) or (self.noise_bank is None and (plan.noise_idx >= 0).any()):
            raise ValueError("augment: the plan names a bank this augmenter does not have")
        dev = samples.device
        lib = _hip.lib()
        pi = ctypes.POINTER(ctypes.c_int)
        with torch.cuda.device(dev):
            if out is None:
                ws = _hip.workspace(dev, samples.numel() * 4, _hip._tag("augment"))
                out = ws[:samples.numel() * 4].view(torch.float32).view(samples.shape)
            elif tuple(out.shape) != tuple(samples.shape) or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
                raise ValueError("out must be a contiguous float32 device tensor of shape %s" % (tuple(samples.shape),))
            slot = self._staging(dev, 20 * n)
            host = slot[0][:20 * n].numpy().view(np.int32).reshape(5, n)
            host[0], host[1], host[2], host[3] = ns, plan.rir_idx, plan.noise_idx, plan.noise_off
            host[4] = plan.snr_db.view(np.int32)
            d = slot[0][:20 * n].to(dev, non_blocking=True)
            slot[1] = torch.cuda.Event()
            slot[1].record()
            base = d.data_ptr()
            b = self._banks_on(dev)
            src = samples
            if self.rir_bank is not None:
                _hip.check(lib.las_reverb(src.data_ptr(), ld, base, ns.ctypes.data_as(pi), n, b["rir"].data_ptr(), self.rir_bank.shape[1],
                                          b["rir_len"].data_ptr(), self.rir_len.ctypes.data_as(pi), b["rir_delay"].data_ptr(),
                                          self._rir_delay.ctypes.data_as(pi), len(self.rirs), base + 4 * n,
                                          plan.rir_idx.ctypes.data_as(pi), out.data_ptr(), ld, _hip.stream()), "las_reverb")
                src = out
            if self.noise_bank is not None:
                need = int(lib.las_noise_mix_workspace_bytes(n, ld))
                nws = _hip.workspace(dev, need, _hip._tag("noise_mix"))
                _hip.check(lib.las_noise_mix(src.data_ptr(), ld, base, ns.ctypes.data_as(pi), n, b["noise"].data_ptr(), self.noise_bank.shape[1],
                                             b["noise_len"].data_ptr(), self.noise_len.ctypes.data_as(pi), len(self.noises), base + 8 * n,
                                             plan.noise_idx.ctypes.data_as(pi), base + 12 * n, plan.noise_off.ctypes.data_as(pi), base + 16 * n,
                                             plan.snr_db.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), out.data_ptr(), ld,
                                             gain_out.data_ptr() if gain_out is not None else None, nws.data_ptr(), nws.numel(),
                                             _hip.stream()), "las_noise_mix")
        return out
