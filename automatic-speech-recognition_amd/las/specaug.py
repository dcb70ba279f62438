"""las.specaug -- SpecAugment (Park et al., 2019) on the device, between the feeder and the Listener: one time warp, mF frequency
masks and mT time masks per utterance of the [B, T, feat_dim, 3] cube, in one launch of las_specaug (csrc/specaug.hip).

The kernel applies a PLAN and draws nothing; `SpecAugment.plan` draws the plan on the host, keyed by (args.seed, step) only, so a
step that LAS._recover re-runs from the raw batch gets the masks it had.  tests/specaug_ref.py is the float64 statement of "apply a
plan".  Off unless --spec_augment True; inference, beam search and the evaluation entry points never augment."""
import ctypes

import numpy as np
import torch

from las import _hip

MASKS_MAX = 16          # csrc/specaug.hip
T_MAX = 32768


def _index(u, n):
    """floor(u * n) for u in [0, 1), kept below n (the float64 product of the largest u and an n that is no power of two rounds to n)"""
    return np.minimum(np.floor(u * n).astype(np.int64), np.maximum(n - 1, 0))


class SpecAugment:
    """reads seed, feat_dim and the specaug_* flags from the flag namespace (las.arguments)"""

    def __init__(self, args, device=None):
        self.seed = int(getattr(args, "seed", 0))
        self.F = int(args.feat_dim)
        self.W = int(args.specaug_time_warp)
        self.mF = int(args.specaug_freq_masks)
        self.mT = int(args.specaug_time_masks)
        fw = int(args.specaug_freq_width)
        self.Fw = min(max(1, self.F // 3) if fw < 0 else fw, self.F)
        self.Tw = int(args.specaug_time_width)
        self.p = float(args.specaug_time_ratio)
        if self.W < 0 or self.Tw < 0 or not 0.0 <= self.p <= 1.0:
            raise ValueError("specaug: time warp %d, time mask width %d (>= 0 each), time ratio %g (0..1)" % (self.W, self.Tw, self.p))
        if not (0 <= self.mF <= MASKS_MAX and 0 <= self.mT <= MASKS_MAX):
            raise ValueError("specaug: %d frequency and %d time masks (0..%d each)" % (self.mF, self.mT, MASKS_MAX))
        self.n_draws = 2 + 2 * self.mF + 2 * self.mT
        self.ldp = (4 + 2 * (self.mF + self.mT) + 3) & ~3
        self.device = device
        self._pinned = {}                     # device -> two alternating pinned staging buffers, each with the event of its last upload
        self._turn = 0

    # -- the draws (host) --------------------------------------------------------------------------------------------------------
    def plan(self, lens, step, row0=0, rows_global=None):
        """int32 [B, ldp], row b = {len, w0, w, 0, (f0, fw) x mF, (t0, tw) x mT}, zeros up to ldp (a multiple of 4).  The recipe:

          u = numpy.random.Generator(numpy.random.Philox(key=[seed mod 2^64, step mod 2^64])).random((rows_global, n_draws)),
          float64 in [0, 1), n_draws = 2 + 2 mF + 2 mT, filled row by row.  The caller's row b is row row0 + b of that block
          (rows_global defaults to row0 + B; a counter-based generator fills row r from r and n_draws alone, so a global row draws
          the same numbers however the batch is sharded).  With idx(u, n) = min(floor(u n), n - 1) and len = lens[b], W, Fw, Tw, p
          the flags:
            warp   len < 2 W + 3 or W == 0:  w0 = w = 0 (no warp).  Otherwise w0 = W + 1 + idx(u[0], len - 2 W - 2), uniform in
                   [W + 1, len - W - 1), and w = idx(u[1], 2 W + 1) - W, uniform in [-W, W].  (u[0], u[1] are drawn either way.)
            freq   mask m = 0 .. mF - 1:  fw = idx(u[2 + 2 m], Fw + 1), f0 = idx(u[3 + 2 m], F - fw + 1)
            time   mask m = 0 .. mT - 1, k = 2 + 2 mF + 2 m:  tw = idx(u[k], min(Tw, floor(p len)) + 1), t0 = idx(u[k + 1], len - tw + 1)
        Fw is --specaug_freq_width, max(1, feat_dim // 3) when that is -1, and at most feat_dim."""
        lens = np.asarray(torch.as_tensor(lens).cpu() if torch.is_tensor(lens) else lens, np.int64).reshape(-1)
        B = len(lens)
        rows_global = row0 + B if rows_global is None else int(rows_global)
        if row0 < 0 or row0 + B > rows_global:
            raise ValueError("specaug: rows [%d, %d) of a global batch of %d" % (row0, row0 + B, rows_global))
        if B and (lens.min() < 0 or lens.max() > T_MAX):
            raise ValueError("specaug: utterance lengths %d..%d (0..%d)" % (lens.min(), lens.max(), T_MAX))
        key = np.array([self.seed % (1 << 64), int(step) % (1 << 64)], dtype=np.uint64)
        u = np.random.Generator(np.random.Philox(key=key)).random((rows_global, self.n_draws))[row0:row0 + B]
        W, F, mF = self.W, self.F, self.mF
        plan = np.zeros((B, self.ldp), np.int32)
        plan[:, 0] = lens
        warped = (lens >= 2 * W + 3) & (W > 0)
        w0 = W + 1 + _index(u[:, 0], lens - 2 * W - 2)
        w = _index(u[:, 1], np.int64(2 * W + 1)) - W
        plan[:, 1] = np.where(warped, w0, 0)
        plan[:, 2] = np.where(warped, w, 0)
        for m in range(mF):
            fw = _index(u[:, 2 + 2 * m], np.int64(self.Fw + 1))
            plan[:, 4 + 2 * m] = _index(u[:, 3 + 2 * m], F - fw + 1)
            plan[:, 5 + 2 * m] = fw
        cap = np.minimum(self.Tw, np.floor(self.p * lens).astype(np.int64))
        for m in range(self.mT):
            k = 2 + 2 * mF + 2 * m
            tw = _index(u[:, k], cap + 1)
            plan[:, 4 + 2 * mF + 2 * m] = _index(u[:, k + 1], lens - tw + 1)
            plan[:, 5 + 2 * mF + 2 * m] = tw
        return plan

    # -- the device path ---------------------------------------------------------------------------------------------------------
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

    def apply(self, audio, plan, out=None):
        """las_specaug of a host plan (int32 [B, ldp'], any ldp' the entry takes, mF and mT this object's) on the current stream:
        one pinned asynchronous upload of the plan, one launch, no synchronisation.  audio: a contiguous float32 device tensor
        [B, T, F, C] (or [B, T, F]).  Returns a tensor of audio's shape in the 'specaug' workspace -- valid until the next call on this
        stream -- or `out`, a contiguous float32 device tensor of that shape that does not overlap audio."""
        if not torch.is_tensor(audio) or not audio.is_cuda:
            raise RuntimeError("las.specaug needs a tensor on a ROCm device; the CPU statement of the arithmetic is tests/specaug_ref.py")
        if audio.dtype != torch.float32 or audio.dim() not in (3, 4) or not audio.is_contiguous():
            raise ValueError("specaug: audio is a contiguous float32 [B, T, F, C] tensor (got %s %s)" % (audio.dtype, tuple(audio.shape)))
        plan = np.ascontiguousarray(plan, dtype=np.int32)
        B, T, F = audio.shape[:3]
        C = audio.shape[3] if audio.dim() == 4 else 1
        if plan.ndim != 2 or plan.shape[0] != B:
            raise ValueError("specaug: a plan of shape %s for %d utterances" % (plan.shape, B))
        dev = audio.device
        nbytes = plan.nbytes
        with torch.cuda.device(dev):
            if out is None:
                ws = _hip.workspace(dev, audio.numel() * 4, _hip._tag("specaug"))
                out = ws[:audio.numel() * 4].view(torch.float32).view(audio.shape)
            elif tuple(out.shape) != tuple(audio.shape) or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
                raise ValueError("out must be a contiguous float32 device tensor of shape %s" % (tuple(audio.shape),))
            slot = self._staging(dev, nbytes)
            host = slot[0][:nbytes].numpy().view(np.int32).reshape(plan.shape)
            host[:] = plan
            dplan = slot[0][:nbytes].to(dev, non_blocking=True)
            slot[1] = torch.cuda.Event()
            slot[1].record()
            a = _hip.SpecAugArgs(in_=audio.data_ptr(), out=out.data_ptr(), plan=dplan.data_ptr(),
                                 plan_host=plan.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ldp=plan.shape[1], B=B, Tmax=T, F=F, C=C,
                                 mF=self.mF, mT=self.mT)
            _hip.check(_hip.lib().las_specaug(ctypes.byref(a), _hip.stream()), "las_specaug")
        return out

    def __call__(self, audio, audiolen, step, row0=0, rows_global=None):
        """the augmented cube of a train step: apply(audio, plan(audiolen, step, row0, rows_global))"""
        return self.apply(audio, self.plan(audiolen, step, row0, rows_global))
