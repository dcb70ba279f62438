"""las.diarize -- who spoke when, without a trained model (las_bic_change, las_bic_cluster, csrc/diarize.hip).

`Diarizer(args).diarize(wave, rate, runs, speech_mask)` takes the speech runs and the speech frames las.vad found in a recording, extracts
the 13 static MFCCs of every run on the device, finds the speaker changes inside each run as the peaks of the delta-BIC curve between two
adjacent windows of --diar_window_ms (every --diar_hop_ms), splits the runs there and clusters all pieces of the recording
agglomeratively under the same criterion: until no merge lowers the BIC, or down to --num_speakers clusters.  Only frames of the speech
mask count in a Gaussian (the padding las.vad puts around speech is digital silence in a clean recording, and two pieces of one voice
with different amounts of it look like two speakers).  `segments` puts the pieces through las.vad.plan_segments for transcribe.py.

Nobody has measured a diarization error rate for any default here.  Not built: overlapped speech, speaker embeddings, re-segmentation."""
import ctypes
import math
import types

import numpy as np
import torch

from las import _hip
from las.cli import add_diarize_flags
from las.frontend import FeatureExtractor
from las.vad import plan_segments

DEFAULTS = dict(num_speakers=0, diar_window_ms=1000.0, diar_hop_ms=100.0, diar_change_lambda=1.0, diar_cluster_lambda=1.0)
STATIC = 13                                   # the static cepstral coefficients the Gaussians are over
FLOOR = 1e-4                                  # added to the covariance's diagonal
MAX_UNITS = 1024                              # include/las_hip.h LAS_BIC_MAX_UNITS


def add_flags(parser, str2bool=None):
    """the diarization flags of transcribe.py (the table lives in las.cli, which must not import this module for a run without them)"""
    add_diarize_flags(parser)


def rttm_line(stem, start, duration, speaker):
    """one segment in NIST's RTTM: SPEAKER <file> 1 <start> <duration> <NA> <NA> S<k> <NA> <NA>"""
    return "SPEAKER %s 1 %.3f %.3f <NA> <NA> S%d <NA> <NA>" % (stem, start, duration, speaker)


def split_run(run, flags, w, hop):
    """a run [a, b) in VAD frames and the peak flags of its candidates -> its sub-runs: candidate c cuts at VAD frame a + w + c hop"""
    a, b = int(run[0]), int(run[1])
    edges = [a] + [a + w + int(c) * hop for c in np.flatnonzero(flags)] + [b]
    return list(zip(edges[:-1], edges[1:]))


class Diarizer:
    """reads sample_rate, frame_length, frame_step (ms) and the --num_speakers / --diar_* flags from the namespace (defaults where it has none)"""

    def __init__(self, args, device=None):
        g = lambda k: getattr(args, k, DEFAULTS[k])
        self.K = int(g("num_speakers"))
        self.window_ms, self.hop_ms = float(g("diar_window_ms")), float(g("diar_hop_ms"))
        self.change_lambda, self.cluster_lambda = float(g("diar_change_lambda")), float(g("diar_cluster_lambda"))
        check_values(self.K, self.window_ms, self.hop_ms, self.change_lambda, self.cluster_lambda)
        self.frame_step = float(args.frame_step)
        self.w = max(2, int(round(self.window_ms / self.frame_step)))
        self.hop = max(1, int(round(self.hop_ms / self.frame_step)))
        self.D = STATIC
        self.nmin = max(self.D + 1, self.w // 2)
        self.device = device
        # a front end of the diarizer's own: 39 cepstra without CMVN, of which the first 13 are the static coefficients
        self.fe = FeatureExtractor(types.SimpleNamespace(sample_rate=args.sample_rate, frame_length=args.frame_length, frame_step=args.frame_step,
                                                         feat_type="mfcc", feat_dim=39, cmvn=False), device=device)
        self.batch_floats = 1 << 26           # padded cube elements per front-end call

    # -- features --------------------------------------------------------------------------------------------------------------------------
    def features(self, wave, rate, runs, speech_mask, fl, step):
        """-> (feat fp32 [N, D], mask uint8 [N], frames per run): run [a, b) is samples [a step, (b - 1) step + fl) and gives b - a - 1
        front-end frames, local frame t = VAD frame a + t; the runs' frames packed one behind the other, all on the device"""
        wave = FeatureExtractor._as_numpy(wave)
        feats, masks, Ts = [], [], []
        group, width = [], 0
        runs = [(int(a), int(b)) for a, b in runs]

        def flush():
            if not group:
                return
            cube, lens = self.fe.extract([wave[a * step:(b - 1) * step + fl] for a, b in group], rate=rate)
            for r, (a, b) in enumerate(group):
                T = min(int(lens[r]), b - a - 1)                          # (another sample rate: the resampled run may round to a frame more)
                feats.append(cube[r, :T, :self.D])
                masks.append(speech_mask[a:a + T])
                Ts.append(T)
            del group[:]

        for a, b in runs:
            if group and (len(group) + 1) * max(width, b - a) * 39 > self.batch_floats:
                flush()
                width = 0
            group.append((a, b))
            width = max(width, b - a)
        flush()
        return torch.cat(feats).contiguous(), torch.cat(masks).to(torch.uint8).contiguous(), Ts

    # -- the two calls -------------------------------------------------------------------------------------------------------------------------
    def change_points(self, feat, mask, seq_off, seq_len):
        """-> per sequence the uint8 peak flags of its candidates (host); one las_bic_change call, one wait"""
        lib = _hip.lib()
        S = len(seq_off)
        counts = [int(lib.las_bic_candidates(int(l), self.w, self.hop)) for l in seq_len]
        cand_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        total = int(cand_off[-1])
        if total == 0:
            return [np.zeros(0, np.uint8) for _ in range(S)]
        dev = feat.device
        d_idx = torch.from_numpy(np.concatenate([np.asarray(seq_off, np.int32), cand_off])).to(dev)
        v = torch.empty(total, dtype=torch.float64, device=dev)
        peak = torch.empty(total, dtype=torch.uint8, device=dev)
        off_h, len_h = (ctypes.c_int * S)(*[int(x) for x in seq_off]), (ctypes.c_int * S)(*[int(x) for x in seq_len])
        _hip.check(lib.las_bic_change(_hip.p(feat), feat.shape[0], feat.stride(0), self.D, _hip.p(mask), d_idx.data_ptr(),
                                      d_idx.data_ptr() + 4 * S, off_h, len_h, S, self.w, self.hop, self.nmin, self.change_lambda, FLOOR,
                                      _hip.p(v), _hip.p(peak), _hip.stream()), "las_bic_change")
        flags = peak.cpu().numpy()
        return [flags[cand_off[s]:cand_off[s + 1]] for s in range(S)]

    def cluster(self, feat, mask, seq_off, seq_len, n_masked):
        """the units of ONE recording -> (labels, number of clusters); one las_bic_cluster call, one wait"""
        lib = _hip.lib()
        S = len(seq_off)
        if S > MAX_UNITS:
            raise ValueError("%d pieces of speech in one recording: las_bic_cluster takes %d (raise --diar_change_lambda or split the file)" % (S, MAX_UNITS))
        dev = feat.device
        d_idx = torch.from_numpy(np.concatenate([np.asarray(seq_off, np.int32), np.asarray(seq_len, np.int32), np.asarray([0, S], np.int32)])).to(dev)
        out = torch.empty(S + 1, dtype=torch.int32, device=dev)
        need = int(lib.las_bic_cluster_workspace_bytes(S, S, self.D))
        ws = _hip.workspace(dev, need, _hip._tag("diarize"))
        ci = lambda xs: (ctypes.c_int * len(xs))(*[int(x) for x in xs])
        _hip.check(lib.las_bic_cluster(_hip.p(feat), feat.shape[0], feat.stride(0), self.D, _hip.p(mask), d_idx.data_ptr(), d_idx.data_ptr() + 4 * S,
                                       d_idx.data_ptr() + 8 * S, ci(seq_off), ci(seq_len), ci(n_masked), S, ci([0, S]), 1, self.K, self.cluster_lambda,
                                       FLOOR, out.data_ptr(), out.data_ptr() + 4 * S, None, None, None, None, _hip.p(ws), ws.numel(),
                                       _hip.stream()), "las_bic_cluster")
        got = out.cpu().numpy()
        return got[:S].tolist(), int(got[S])

    # -- a recording ---------------------------------------------------------------------------------------------------------------------------
    def diarize(self, wave, rate, runs, speech_mask, geometry=None):
        """wave at `rate` Hz, runs [(a, b)] in VAD frames (las.vad.VoiceActivity.runs), speech_mask a device tensor over the recording's
        VAD frames (VoiceActivity.speech_mask) -> (units [(a, b)] in VAD frames, in time order; labels: per unit its speaker, from 0 in
        the order of first appearance).  geometry: (fl, step) of the VAD frames at `rate` (default: the front end's at its own rate)."""
        dev = torch.device(self.device if self.device is not None else "cuda")
        if dev.type != "cuda":
            raise RuntimeError("las.diarize needs a ROCm device (got %s); there is no CPU fallback" % dev)
        runs = [(int(a), int(b)) for a, b in runs]
        if not runs:
            return [], []
        fl, step = geometry if geometry is not None else (self.fe.fl, self.fe.step)
        with torch.cuda.device(dev):
            feat, mask, Ts = self.features(wave, rate, runs, speech_mask, fl, step)
            row0 = np.concatenate([[0], np.cumsum(Ts)]).astype(np.int64)
            flags = self.change_points(feat, mask, row0[:-1], Ts)
            units, seq_off, seq_len = [], [], []
            for r, run in enumerate(runs):
                for a, b in split_run(run, flags[r], self.w, self.hop):
                    units.append((a, b))
                    seq_off.append(int(row0[r]) + a - run[0])
                    seq_len.append(min(b, run[0] + Ts[r]) - a)            # (the run's last VAD frame starts no front-end frame)
            # a piece without a speech frame (a run that is all padding but for its last VAD frame) counts all its frames
            csum = torch.cat([torch.zeros(1, dtype=torch.int32, device=dev), torch.cumsum(mask.to(torch.int32), 0, dtype=torch.int32)])
            edges = torch.from_numpy(np.asarray([seq_off, [o + l for o, l in zip(seq_off, seq_len)]], np.int64)).to(dev)
            n_masked = (csum[edges[1]] - csum[edges[0]]).cpu().numpy()
            for s in np.flatnonzero(n_masked == 0):
                mask[seq_off[s]:seq_off[s] + seq_len[s]] = 1
                n_masked[s] = seq_len[s]
            labels, _ = self.cluster(feat, mask, seq_off, seq_len, n_masked)
        return units, labels

    def segments(self, va, wave, rate):
        """transcribe.py's cut of one recording: las.vad's runs, split and labelled, every piece through las.vad.plan_segments ->
        (sample ranges, the speaker of each, 1-based; the number of speakers)"""
        runs = va.runs([wave], rate, energy_over=va.max_frames, keep=True)[0]
        fl, step = va.geometry(rate)
        units, labels = self.diarize(wave, rate, runs, va.speech_mask(0), geometry=(fl, step))
        ranges, speakers = [], []
        for unit, k in zip(units, labels):
            for a, b in plan_segments([unit], va.energies[0], va.max_frames(rate)):
                ranges.append((a * step, min((b - 1) * step + fl, len(wave))))
                speakers.append(k + 1)
        return ranges, speakers, len(set(labels))


def check_values(K, window_ms, hop_ms, change_lambda, cluster_lambda):
    if K < 0 or K > MAX_UNITS:
        raise ValueError("--num_speakers %d: 0 (decide by BIC) to %d" % (K, MAX_UNITS))
    if not (math.isfinite(window_ms) and math.isfinite(hop_ms) and window_ms > 0 and hop_ms > 0):
        raise ValueError("--diar_window_ms %r, --diar_hop_ms %r: positive numbers of milliseconds" % (window_ms, hop_ms))
    if not (math.isfinite(change_lambda) and math.isfinite(cluster_lambda)):
        raise ValueError("--diar_change_lambda %r, --diar_cluster_lambda %r: finite penalty weights" % (change_lambda, cluster_lambda))
