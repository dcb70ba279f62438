"""las.beamform -- a microphone-array recording to one channel, without a trained model.  Two methods, --bf_method:

delaysum (las_gcc_phat, las_tdoa_track, las_delay_sum, csrc/beamform.hip).  BeamformIt's scheme (Anguera et al. 2007): per
window of --bf_window_ms (every half window) the delay of every channel against the reference channel --bf_ref is the peak of the
PHAT-weighted cross-correlation within --bf_max_delay_ms; a Viterbi pass over the windows (--bf_jump_penalty per sample of lag per
window) keeps a pause or a burst of noise from throwing the delays; the channels are shifted by whole samples, weighted by their
coherence with the reference, summed and cross-faded between window centres.  A fixed beamformer: at most 10 log10(C) dB, and only
against noise that is independent between the microphones.

mvdr (las_mvdr_mask, las_mvdr_cov, las_mvdr_weights, las_mvdr_apply, csrc/mvdr.hip).  A mask-driven MVDR beamformer in the
STFT domain, in Souden's reference-channel form (Souden et al. 2010): frames of --mvdr_frame_ms under a sine window, every half frame;
the frames of --bf_ref within --mvdr_top_db of its loudest frame (over --mvdr_floor_db, widened by --mvdr_pad_ms) are speech, the
others train the noise covariance per bin; the speech covariance is taken per block of --mvdr_block_ms, the weights per block and bin
are (A^-1 (phi_y - phi_n))[:, ref] / tr(A^-1 (phi_y - phi_n)) with A = phi_n + --mvdr_loading x its mean diagonal, and the output is
the inverse STFT of the weighted channels.  No geometry, no delay estimate, no steering vector: sub-sample delays come for free,
and a directional disturbance (a fan, a television, a second talker who is silent while the noise is learned) is cancelled, which
delay-and-sum cannot do.  A recording the mask calls all speech or all noise comes out as its reference channel, with a warning.

`Beamformer(args).enhance(audio[n, C], fs)` -> (mono float32 [n], info): one upload, three (delaysum) or four (mvdr) calls, one
read-back of y; everything else stays on the device (delaysum: info["tau"], info["a"], read back by `Beamformer.delays(info)`; mvdr:
info["m"], info["counts"], info["valid"], read back by `Beamformer.statistics(info)`).

Nobody has measured a word error rate with either, and no default has been tuned on a real room.  Not built: N-best peak lists, noise
thresholding and an automatic reference channel (delaysum); online or recursive covariance updates, GEV / rank-1 variants, a learned
mask, cross-fades between blocks, and handing y to the front end on the device instead of through the host (mvdr)."""
import math

import numpy as np
import torch

from las import _hip
from las.cli import BEAMFORM_DEFAULTS as DEFAULTS
from las.cli import MVDR_DEFAULTS

MAX_CHANNELS, MAX_FFT, MAX_LAG = 16, 16384, 512      # include/las_hip.h LAS_BF_*
MVDR_MIN_FFT, MVDR_MAX_FFT = 64, 1024                 # include/las_hip.h K19, LAS_MVDR_MAX_FFT


def check_values(window_ms, max_delay_ms, jump_penalty, ref):
    if not (math.isfinite(window_ms) and math.isfinite(max_delay_ms) and window_ms > 0 and max_delay_ms > 0):
        raise ValueError("--bf_window_ms %r, --bf_max_delay_ms %r: positive numbers of milliseconds" % (window_ms, max_delay_ms))
    if not (math.isfinite(jump_penalty) and jump_penalty >= 0):
        raise ValueError("--bf_jump_penalty %r: a finite penalty >= 0 per sample of lag per window" % (jump_penalty,))
    if ref < 0 or ref >= MAX_CHANNELS:
        raise ValueError("--bf_ref %d: a channel, 0 to %d" % (ref, MAX_CHANNELS - 1))


def geometry(window_ms, max_delay_ms, fs):
    """-> (L, D, NF): the window (even), the largest lag and the FFT length in samples at fs Hz"""
    L = 2 * int(round(window_ms * fs / 2000.0))
    D = int(math.ceil(max_delay_ms * fs / 1000.0 - 1e-9))
    if L < 2 or D < 1:
        raise ValueError("--bf_window_ms %g, --bf_max_delay_ms %g at %d Hz: a window of %d samples and a largest lag of %d (at least 2 and 1)"
                         % (window_ms, max_delay_ms, fs, L, D))
    NF = 1
    while NF < L + D:
        NF *= 2
    if NF > MAX_FFT or D > MAX_LAG:
        raise ValueError("--bf_window_ms %g and --bf_max_delay_ms %g at %d Hz need a transform of %d points and lags up to %d: at most %d and %d "
                         "(the defaults fit up to 32 kHz; a 48 kHz file needs --bf_window_ms of at most 330)"
                         % (window_ms, max_delay_ms, fs, NF, D, MAX_FFT, MAX_LAG))
    return L, D, NF


def check_mvdr_values(frame_ms, block_ms, top_db, floor_db, pad_ms, loading):
    for flag, v in (("mvdr_frame_ms", frame_ms), ("mvdr_block_ms", block_ms), ("mvdr_top_db", top_db), ("mvdr_loading", loading)):
        if not (math.isfinite(v) and v > 0):
            raise ValueError("--%s %r: a finite number > 0" % (flag, v))
    if not (math.isfinite(pad_ms) and pad_ms >= 0):
        raise ValueError("--mvdr_pad_ms %r: a finite number of milliseconds >= 0" % (pad_ms,))
    if not math.isfinite(floor_db):
        raise ValueError("--mvdr_floor_db %r: a finite number of dB" % (floor_db,))
    if not 10.0 ** (-top_db / 10.0) > 0.0:
        raise ValueError("--mvdr_top_db %r: more dB than a double holds" % (top_db,))


def mvdr_geometry(frame_ms, block_ms, pad_ms, fs):
    """-> (NF, Bf, hang): the frame (a power of two), the frames per block and the mask's dilation in frames at fs Hz"""
    want = int(math.ceil(frame_ms * fs / 1000.0 - 1e-9))
    NF = 1
    while NF < want:
        NF *= 2
    if NF < MVDR_MIN_FFT or NF > MVDR_MAX_FFT:
        raise ValueError("--mvdr_frame_ms %g at %d Hz is a frame of %d samples: %d to %d (%g to %g ms)"
                         % (frame_ms, fs, NF, MVDR_MIN_FFT, MVDR_MAX_FFT, (MVDR_MIN_FFT // 2 + 1) * 1000.0 / fs, MVDR_MAX_FFT * 1000.0 / fs))
    hop_ms = 1000.0 * (NF // 2) / fs
    return NF, max(1, int(round(block_ms / hop_ms))), int(round(pad_ms / hop_ms))


def twiddle(NF):
    """exp(-2 pi i k / NF), k = 0 .. NF / 2, float64 [NF / 2 + 1, 2]: the table of csrc/bf_fft.h's transform"""
    k = np.arange(NF // 2 + 1)
    return np.stack([np.cos(2.0 * np.pi * k / NF), -np.sin(2.0 * np.pi * k / NF)], axis=1)


def mvdr_tables(NF):
    """(win float64 [NF], twiddle float64 [NF / 2 + 1, 2]) as las_mvdr_cov and las_mvdr_apply take them"""
    return np.sin(np.pi * (np.arange(NF) + 0.5) / NF), twiddle(NF)


def tables(L, NF):
    """(hann float64 [L], twiddle float64 [NF / 2 + 1, 2]) as las_gcc_phat takes them"""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(L) + 0.5) / L), twiddle(NF)


class Beamformer:
    """reads the --bf_* flags from the namespace (defaults where it has none)"""

    def __init__(self, args, device=None):
        g = lambda k: DEFAULTS[k] if getattr(args, k, None) is None else getattr(args, k)
        self.window_ms, self.max_delay_ms = float(g("bf_window_ms")), float(g("bf_max_delay_ms"))
        self.gamma, self.ref = float(g("bf_jump_penalty")), int(g("bf_ref"))
        check_values(self.window_ms, self.max_delay_ms, self.gamma, self.ref)
        self.method = getattr(args, "bf_method", None) or "delaysum"
        if self.method not in ("delaysum", "mvdr"):
            raise ValueError("--bf_method %r: delaysum or mvdr" % (self.method,))
        if self.method == "mvdr":
            m = lambda k: MVDR_DEFAULTS[k] if getattr(args, k, None) is None else getattr(args, k)
            floor_db = m("mvdr_floor_db")
            if floor_db is None:
                floor_db = getattr(args, "vad_floor_db", None)
            self.frame_ms, self.block_ms, self.top_db = float(m("mvdr_frame_ms")), float(m("mvdr_block_ms")), float(m("mvdr_top_db"))
            self.floor_db = -70.0 if floor_db is None else float(floor_db)             # (las.vad.DEFAULTS["vad_floor_db"])
            self.pad_ms, self.loading = float(m("mvdr_pad_ms")), float(m("mvdr_loading"))
            check_mvdr_values(self.frame_ms, self.block_ms, self.top_db, self.floor_db, self.pad_ms, self.loading)
        self.device = device
        self._tables = {}                             # (L, NF) -> the two tables on the device

    def _open(self, audio, entry, geometry):
        """what both methods begin with: the checks of the device and of audio [n, C] against the limits of `entry` and --bf_ref, the
        method's geometry() (which may refuse) and the one upload -> (dev, x [C, n] int16 or float32 on it, i16, n, C, the geometry)"""
        dev = torch.device(self.device if self.device is not None else "cuda")
        if dev.type != "cuda":
            raise RuntimeError("las.beamform needs a ROCm device (got %s); there is no CPU fallback" % dev)
        audio = np.asarray(audio)
        if audio.ndim != 2 or audio.shape[1] < 2 or audio.shape[0] < 1:
            raise ValueError("enhance takes audio [n, C >= 2], got %s" % (audio.shape,))
        n, C = audio.shape
        if C > MAX_CHANNELS:
            raise ValueError("%d channels: %s takes %d" % (C, entry, MAX_CHANNELS))
        if self.ref >= C:
            raise ValueError("--bf_ref %d: the recording has the channels 0 to %d" % (self.ref, C - 1))
        geo = geometry()
        i16 = audio.dtype == np.int16
        rows = np.ascontiguousarray(audio.T if i16 else audio.T.astype(np.float32, copy=False))
        return dev, torch.from_numpy(rows).to(dev), i16, n, C, geo            # the one upload

    def enhance(self, audio, fs):
        """audio [n, C] (int16 or float; C >= 2) at fs Hz -> (y float32 numpy [n], info)"""
        if self.method == "mvdr":
            return self.enhance_mvdr(audio, fs)
        dev, x, i16, n, C, (L, D, NF) = self._open(audio, "las_gcc_phat", lambda: geometry(self.window_ms, self.max_delay_ms, int(fs)))
        lib = _hip.lib()
        Wn = int(lib.las_bf_windows(n, L))
        with torch.cuda.device(dev):
            if (L, NF) not in self._tables:
                self._tables[(L, NF)] = tuple(torch.from_numpy(t).to(dev) for t in tables(L, NF))
            hann, tw = self._tables[(L, NF)]
            r = torch.empty((C, Wn, 2 * D + 1), dtype=torch.float32, device=dev)
            tau = torch.empty((C, Wn), dtype=torch.int32, device=dev)
            a = torch.empty((C, Wn), dtype=torch.float32, device=dev)
            y = torch.empty(n, dtype=torch.float32, device=dev)
            ws = _hip.workspace(dev, int(lib.las_bf_workspace_bytes(C, Wn, NF, D)), _hip._tag("beamform"))
            _hip.check(lib.las_gcc_phat(_hip.p(x), int(i16), n, C, n, self.ref, L, D, NF, _hip.p(hann), _hip.p(tw), _hip.p(r), _hip.p(ws),
                                        ws.numel(), _hip.stream()), "las_gcc_phat")
            _hip.check(lib.las_tdoa_track(_hip.p(r), C, Wn, D, self.ref, self.gamma, _hip.p(tau), _hip.p(a), _hip.p(ws), ws.numel(),
                                          _hip.stream()), "las_tdoa_track")
            _hip.check(lib.las_delay_sum(_hip.p(x), int(i16), n, C, n, L, Wn, _hip.p(tau), _hip.p(a), _hip.p(y), _hip.stream()), "las_delay_sum")
            out = y.cpu().numpy()                                         # the one read-back (and the one wait)
        return out, dict(tau=tau, a=a, Wn=Wn, C=C, n=n, fs=int(fs), L=L, H=L // 2, D=D, NF=NF, ref=self.ref, gamma=self.gamma)

    def enhance_mvdr(self, audio, fs):
        """--bf_method mvdr: one upload, the four calls of K19, one read-back of y; a one-line warning on stderr where the mask leaves no
        noise frame or no speech frame (a second, small read-back: the counts)"""
        dev, x, i16, n, C, (NF, Bf, hang) = self._open(audio, "las_mvdr_cov",
                                                       lambda: mvdr_geometry(self.frame_ms, self.block_ms, self.pad_ms, int(fs)))
        ratio, floor = 10.0 ** (-self.top_db / 10.0), NF * 10.0 ** (self.floor_db / 10.0)
        lib = _hip.lib()
        Tf = int(lib.las_mvdr_frames(n, NF))
        Nb, K = int(lib.las_mvdr_blocks(Tf, Bf)), NF // 2 + 1
        with torch.cuda.device(dev):
            if ("mvdr", NF) not in self._tables:
                self._tables[("mvdr", NF)] = tuple(torch.from_numpy(t).to(dev) for t in mvdr_tables(NF))
            win, tw = self._tables[("mvdr", NF)]
            m = torch.empty(Tf, dtype=torch.float32, device=dev)
            counts = torch.empty(1 + Nb, dtype=torch.float64, device=dev)
            phi_n = torch.empty((K, C, C, 2), dtype=torch.float64, device=dev)
            phi_y = torch.empty((Nb, K, C, C, 2), dtype=torch.float64, device=dev)
            w = torch.empty((Nb, K, C, 2), dtype=torch.float64, device=dev)
            valid = torch.empty((Nb, K), dtype=torch.int32, device=dev)
            y = torch.empty(n, dtype=torch.float32, device=dev)
            ws = _hip.workspace(dev, int(lib.las_mvdr_workspace_bytes(C, Tf, NF, Bf)), _hip._tag("mvdr"))
            _hip.check(lib.las_mvdr_mask(_hip.p(x), int(i16), n, C, n, self.ref, NF, ratio, floor, hang, _hip.p(m), None, _hip.p(ws), ws.numel(),
                                         _hip.stream()), "las_mvdr_mask")
            _hip.check(lib.las_mvdr_cov(_hip.p(x), int(i16), n, C, n, NF, Bf, _hip.p(m), _hip.p(win), _hip.p(tw), _hip.p(counts), _hip.p(phi_n),
                                        _hip.p(phi_y), _hip.p(ws), ws.numel(), _hip.stream()), "las_mvdr_cov")
            _hip.check(lib.las_mvdr_weights(_hip.p(phi_n), _hip.p(phi_y), _hip.p(counts), C, NF, Nb, self.ref, self.loading, _hip.p(w),
                                            _hip.p(valid), _hip.stream()), "las_mvdr_weights")
            _hip.check(lib.las_mvdr_apply(_hip.p(x), int(i16), n, C, n, NF, Bf, _hip.p(w), _hip.p(win), _hip.p(tw), _hip.p(y), _hip.p(ws),
                                          ws.numel(), _hip.stream()), "las_mvdr_apply")
            out = y.cpu().numpy()                                         # the one read-back (and the one wait)
            cnt = counts.cpu().numpy()
        if not cnt[0] > 0 or not (cnt[1:] > 0).any():
            import sys
            print("las.beamform: the mask of --mvdr_top_db %g calls %s frame of this recording %s: it comes out as channel %d (a smaller "
                  "--mvdr_top_db leaves frames to learn the noise from)" % (self.top_db, "every" if not cnt[0] > 0 else "no",
                                                                           "speech", self.ref), file=sys.stderr)
        return out, dict(m=m, counts=counts, valid=valid, w=w, Tf=Tf, Nb=Nb, NF=NF, Bf=Bf, K=K, C=C, n=n, fs=int(fs), hang=hang, ratio=ratio,
                         floor=floor, ref=self.ref, loading=self.loading)

    @staticmethod
    def statistics(info):
        """(m float32 [Tf], counts float64 [1 + Nb], valid int32 [Nb, K]) of an mvdr run on the host: a second read-back"""
        return info["m"].cpu().numpy(), info["counts"].cpu().numpy(), info["valid"].cpu().numpy()

    @staticmethod
    def delays(info):
        """(tau int32 [C, Wn], a float32 [C, Wn]) on the host: a second read-back, for who wants to look at them"""
        return info["tau"].cpu().numpy(), info["a"].cpu().numpy()


def write_wav(path, y, fs):
    """16-bit at the file's rate, clipped to full scale"""
    from scipy.io import wavfile
    wavfile.write(path, int(fs), np.round(np.clip(np.asarray(y, np.float64), -1.0, 1.0) * 32767.0).astype(np.int16))
