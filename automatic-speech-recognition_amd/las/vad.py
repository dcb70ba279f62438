"""las.vad -- long recordings: an energy voice-activity detector and segmenter on the device (las_vad, csrc/vad.hip).

`VoiceActivity(args).runs(waves, rate)` finds, per recording, the runs of frames that hold speech: the front end's frames, the frame
energy in double, a threshold relative to the recording's peak (--vad_top_db) over an absolute floor (--vad_floor_db), a dilation by
--vad_pad_ms and a minimum run of --vad_min_speech_ms.  `plan_segments` (host code) cuts runs longer than the training cap
(--max_segment_s) at their quietest frame; `segments(wave, rate)` returns the sample ranges transcribe.py decodes one by one."""
import ctypes
import math

import numpy as np
import torch

from las import _hip
from las.frontend import FeatureExtractor, frame_count, frame_geometry

DEFAULTS = dict(vad_top_db=40.0, vad_floor_db=-70.0, vad_pad_ms=200.0, vad_min_speech_ms=100.0, max_segment_s=17.0)


def add_flags(parser, str2bool):
    """the segmentation flags of transcribe.py (its own parser: las.arguments keeps the reference's table)"""
    parser.add_argument("--segment", type=str2bool, default=False, help="Segment each file by voice activity before decoding (long recordings).")
    parser.add_argument("--vad_top_db", type=float, default=DEFAULTS["vad_top_db"], help="Speech = frames within this many dB of the file's loudest frame.")
    parser.add_argument("--vad_floor_db", type=float, default=DEFAULTS["vad_floor_db"], help="Absolute floor: mean sample power (dB re full scale) below which nothing is speech.")
    parser.add_argument("--vad_pad_ms", type=float, default=DEFAULTS["vad_pad_ms"], help="Padding around speech; gaps of at most twice this are joined.")
    parser.add_argument("--vad_min_speech_ms", type=float, default=DEFAULTS["vad_min_speech_ms"], help="Shorter runs are dropped.")
    parser.add_argument("--max_segment_s", type=float, default=DEFAULTS["max_segment_s"], help="Longer runs are cut at their quietest frame (the training cap).")


def plan_segments(runs, energy, max_frames):
    """runs [(a, b)] in frames -> segments [(a, b)].  A run of at most max_frames frames is one segment.  A longer run [a, b) is cut
    repeatedly at c = argmin energy[t] over t in [a + max_frames // 2, min(a + max_frames, b - 2)], the smallest t on a tie: [a, c)
    is emitted and the rule continues from c.  (b - 2: what is left keeps the two frames every segment needs; a + max_frames < b - 1
    otherwise, and the window is the plain one.)  energy is only read for runs that are cut."""
    max_frames = int(max_frames)
    if max_frames < 4:
        raise ValueError("max_frames=%d: a cut needs max_frames // 2 >= 2 frames on its left" % max_frames)
    out = []
    for a, b in runs:
        a, b = int(a), int(b)
        if b - a < 2:
            raise ValueError("a run of %d frames: every segment has at least 2" % (b - a))
        while b - a > max_frames:
            lo, hi = a + max_frames // 2, min(a + max_frames, b - 2)
            c = lo + int(np.argmin(np.asarray(energy[lo:hi + 1])))      # (argmin returns the first of equal minima)
            out.append((a, c))
            a = c
        out.append((a, b))
    return out


class VoiceActivity:
    """reads frame_length, frame_step (ms) and the --vad_* / --max_segment_s flags from the namespace (defaults where it has none)"""

    def __init__(self, args, device=None):
        self.frame_length, self.frame_step = float(args.frame_length), float(args.frame_step)
        g = lambda k: float(getattr(args, k, DEFAULTS[k]))
        self.top_db, self.floor_db, self.pad_ms, self.min_speech_ms, self.max_segment_s = \
            g("vad_top_db"), g("vad_floor_db"), g("vad_pad_ms"), g("vad_min_speech_ms"), g("max_segment_s")
        if not self.top_db >= 0 or not math.isfinite(self.top_db):
            raise ValueError("--vad_top_db %r: a non-negative number of dB below the peak" % self.top_db)
        if not math.isfinite(self.floor_db):
            raise ValueError("--vad_floor_db %r" % self.floor_db)
        if self.pad_ms < 0 or self.min_speech_ms < 0 or not self.max_segment_s > 0:
            raise ValueError("--vad_pad_ms %r, --vad_min_speech_ms %r (>= 0), --max_segment_s %r (> 0)" % (self.pad_ms, self.min_speech_ms, self.max_segment_s))
        self.ratio = 10.0 ** (-self.top_db / 10.0)
        self.hang = int(round(self.pad_ms / self.frame_step))
        self.min_run = max(2, int(math.ceil(self.min_speech_ms / self.frame_step)))
        self.device = device
        self.energies = []                    # of the last runs() call: per recording None, or its frame energies when asked for
        self.kept = []                        # of the last runs(keep=True) call: per recording (energies, peak) on the device

    def geometry(self, rate):
        fl, step = frame_geometry(int(rate), self.frame_length, self.frame_step)
        if fl < 1 or step < 1:
            raise ValueError("frame of %d samples every %d at %d Hz" % (fl, step, int(rate)))
        return fl, step

    def floor(self, fl):
        """the absolute threshold on a frame's energy: fl samples at a mean power of --vad_floor_db"""
        return fl * 10.0 ** (self.floor_db / 10.0)

    def max_frames(self, rate):
        """frames of the longest segment: its (r - 1) step + fl samples last at most --max_segment_s"""
        fl, step = self.geometry(rate)
        return max(4, int((self.max_segment_s * int(rate) - fl) // step) + 1)

    def runs(self, waves, rate, energy_over=None, keep=False):
        """waves: list of 1-D float or int16 arrays; rate: a scalar or one sample rate per recording.  -> per recording an int array
        [k, 2] of runs [a, b) in frames of ITS rate's geometry (so a run means the same milliseconds at any rate).  One upload and
        one las_vad call per group of recordings at one sample rate; one wait for the counts and the runs.  energy_over: a frame
        count (or a function of the rate) -- the energies of a recording with a run longer than that are read back into
        self.energies (the planner cuts such runs); nothing else leaves the device.  keep: every recording's energies and peak stay
        on the device in self.kept, for speech_mask."""
        dev = torch.device(self.device if self.device is not None else "cuda")
        if dev.type != "cuda":
            raise RuntimeError("las.vad needs a ROCm device (got %s); there is no CPU fallback" % dev)
        ws_np = [FeatureExtractor._as_numpy(w) for w in waves]
        if not ws_np:
            raise ValueError("no waveforms")
        if any(w.dtype.kind != "f" and w.dtype != np.int16 for w in ws_np):
            raise ValueError("waveforms are float or int16 arrays")
        if min(len(w) for w in ws_np) < 1:
            raise ValueError("an empty waveform")
        rates = [int(r) for r in np.broadcast_to(np.asarray(rate), (len(ws_np),))]
        out = [None] * len(ws_np)
        self.energies = [None] * len(ws_np)
        self.kept = [None] * len(ws_np)
        lib = _hip.lib()
        with torch.cuda.device(dev):
            for fs in sorted(set(rates)):
                idx = [u for u, r in enumerate(rates) if r == fs]
                fl, step = self.geometry(fs)
                group = [ws_np[u] for u in idx]
                i16 = all(w.dtype == np.int16 for w in group)
                if not i16:
                    group = [(w.astype(np.float32) / np.float32(32767)) if w.dtype == np.int16 else w for w in group]
                n = len(group)
                ns = [len(w) for w in group]
                Ts = [frame_count(x, fl, step) for x in ns]
                Tmax, ld = max(1, max(Ts)), (max(ns) + 7) & ~7
                host = np.zeros((n, ld), np.int16 if i16 else np.float32)
                for k, w in enumerate(group):
                    host[k, :ns[k]] = w                               # (float64 / float16 input is rounded to fp32 here)
                d_rows = torch.from_numpy(host).to(dev)
                d_ns = torch.tensor(ns, dtype=torch.int32).to(dev)
                max_runs = int(lib.las_vad_max_runs(Tmax, self.hang))
                d_runs = torch.empty((n, max_runs, 2), dtype=torch.int32, device=dev)
                d_count = torch.empty(n, dtype=torch.int32, device=dev)
                d_energy = torch.empty((n, Tmax), dtype=torch.float64, device=dev)
                d_emax = torch.empty(n, dtype=torch.float64, device=dev) if keep else None
                need = int(lib.las_vad_workspace_bytes(n, Tmax))
                ws = _hip.workspace(dev, need, _hip._tag("vad"))
                ns_host = (ctypes.c_int * n)(*ns)
                _hip.check(lib.las_vad(_hip.p(d_rows), int(i16), ld, _hip.p(d_ns), ns_host, n, Tmax, fl, step, self.ratio, self.floor(fl),
                                       self.hang, self.min_run, _hip.p(d_energy), _hip.p(d_emax), _hip.p(d_runs), max_runs, _hip.p(d_count),
                                       _hip.p(ws), ws.numel(), _hip.stream()), "las_vad")
                counts = d_count.cpu().numpy()
                got = d_runs[:, :max(1, int(counts.max()))].cpu().numpy()
                limit = energy_over(fs) if callable(energy_over) else energy_over
                for k, u in enumerate(idx):
                    out[u] = got[k, :counts[k]].copy()
                    if keep:
                        self.kept[u] = (d_energy[k, :Ts[k]], d_emax[k], self.floor(fl))
                    if limit is not None and len(out[u]) and int((out[u][:, 1] - out[u][:, 0]).max()) > int(limit):
                        self.energies[u] = d_energy[k, :Ts[k]].cpu().numpy()
        return out

    def speech_mask(self, u):
        """recording u of the last runs(keep=True) call -> a bool device tensor over its frames: las_vad's raw frames, energy >= max(peak
        x ratio, floor) and > 0 (the runs are these frames padded and joined); computed on the device, nothing is read back"""
        if u >= len(self.kept) or self.kept[u] is None:
            raise RuntimeError("speech_mask(%d): the last runs() call kept nothing on the device (keep=True)" % u)
        e, emax, floor = self.kept[u]
        thr = torch.clamp(emax * self.ratio, min=floor)                    # (one double multiply, as the kernel's)
        return (e >= thr) & (e > 0)

    def segments_batch(self, waves, rate):
        """per recording [(s0, s1)] sample ranges: segment [a, b) in frames covers samples [a step, min((b - 1) step + fl, n))"""
        rates = [int(r) for r in np.broadcast_to(np.asarray(rate), (len(waves),))]
        runs = self.runs(waves, rates, energy_over=self.max_frames)
        out = []
        for u, w in enumerate(waves):
            fl, step = self.geometry(rates[u])
            segs = plan_segments(runs[u], self.energies[u], self.max_frames(rates[u]))
            out.append([(a * step, min((b - 1) * step + fl, len(w))) for a, b in segs])
        return out

    def segments(self, wave, rate):
        return self.segments_batch([wave], rate)[0]
