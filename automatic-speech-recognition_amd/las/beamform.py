"""las.beamform -- a microphone-array recording to one channel, without a trained model (las_gcc_phat, las_tdoa_track, las_delay_sum,
csrc/beamform.hip).  BeamformIt's scheme (Anguera et al. 2007): per window of --bf_window_ms (every half window) the delay of
every channel against the reference channel --bf_ref is the peak of the PHAT-weighted cross-correlation within --bf_max_delay_ms; a
Viterbi pass over the windows (--bf_jump_penalty per sample of lag per window) keeps a pause or a burst of noise from throwing the
delays; the channels are shifted by whole samples, weighted by their coherence with the reference, summed and cross-faded between
window centres.

`Beamformer(args).enhance(audio[n, C], fs)` -> (mono float32 [n], info): one upload, three calls, one read-back of y; the delays and
weights stay on the device (info["tau"], info["a"]) and are read back only by who asks (`Beamformer.delays(info)`).

Nobody has measured a word error rate with it, and no default has been tuned on a real room.  Not built: fractional delays, N-best
peak lists, noise thresholding, an automatic reference channel, MVDR."""
import math

import numpy as np
import torch

from las import _hip
from las.cli import BEAMFORM_DEFAULTS as DEFAULTS

MAX_CHANNELS, MAX_FFT, MAX_LAG = 16, 16384, 512      # include/las_hip.h LAS_BF_*


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


def tables(L, NF):
    """(hann float64 [L], twiddle float64 [NF / 2 + 1, 2]) as las_gcc_phat takes them"""
    hann = 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(L) + 0.5) / L)
    k = np.arange(NF // 2 + 1)
    return hann, np.stack([np.cos(2.0 * np.pi * k / NF), -np.sin(2.0 * np.pi * k / NF)], axis=1)


class Beamformer:
    """reads the --bf_* flags from the namespace (defaults where it has none)"""

    def __init__(self, args, device=None):
        g = lambda k: DEFAULTS[k] if getattr(args, k, None) is None else getattr(args, k)
        self.window_ms, self.max_delay_ms = float(g("bf_window_ms")), float(g("bf_max_delay_ms"))
        self.gamma, self.ref = float(g("bf_jump_penalty")), int(g("bf_ref"))
        check_values(self.window_ms, self.max_delay_ms, self.gamma, self.ref)
        self.device = device
        self._tables = {}                             # (L, NF) -> the two tables on the device

    def enhance(self, audio, fs):
        """audio [n, C] (int16 or float; C >= 2) at fs Hz -> (y float32 numpy [n], info)"""
        dev = torch.device(self.device if self.device is not None else "cuda")
        if dev.type != "cuda":
            raise RuntimeError("las.beamform needs a ROCm device (got %s); there is no CPU fallback" % dev)
        audio = np.asarray(audio)
        if audio.ndim != 2 or audio.shape[1] < 2 or audio.shape[0] < 1:
            raise ValueError("enhance takes audio [n, C >= 2], got %s" % (audio.shape,))
        n, C = audio.shape
        if C > MAX_CHANNELS:
            raise ValueError("%d channels: las_gcc_phat takes %d" % (C, MAX_CHANNELS))
        if self.ref >= C:
            raise ValueError("--bf_ref %d: the recording has the channels 0 to %d" % (self.ref, C - 1))
        L, D, NF = geometry(self.window_ms, self.max_delay_ms, int(fs))
        i16 = audio.dtype == np.int16
        rows = np.ascontiguousarray(audio.T if i16 else audio.T.astype(np.float32, copy=False))
        lib = _hip.lib()
        Wn = int(lib.las_bf_windows(n, L))
        with torch.cuda.device(dev):
            x = torch.from_numpy(rows).to(dev)                            # the one upload
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

    @staticmethod
    def delays(info):
        """(tau int32 [C, Wn], a float32 [C, Wn]) on the host: a second read-back, for who wants to look at them"""
        return info["tau"].cpu().numpy(), info["a"].cpu().numpy()


def write_wav(path, y, fs):
    """16-bit at the file's rate, clipped to full scale"""
    from scipy.io import wavfile
    wavfile.write(path, int(fs), np.round(np.clip(np.asarray(y, np.float64), -1.0, 1.0) * 32767.0).astype(np.int16))
