"""utils/augmentation.py -- speed and volume perturbation from audio files to audio files, on the CPU.

The arithmetic is preprocess.py's float64 statement: speed s declares the recording to be at fs * s Hz and resamples it back to fs
(preprocess.speed_perturb), volume multiplies by a gain.  Sources are read with preprocess.read_audio; results are always 16-bit
.wav files, whatever the source's format, so a result can be read back by read_audio.  preprocess.py --augmentation does not use
these functions: it perturbs in memory (or on the device) and writes features only."""
import os

import numpy as np

from preprocess import read_audio, speed_perturb


def _stem(path):
    return os.path.splitext(os.path.basename(path))[0]


def _save_wav16(path, samples, fs):
    """float samples as 16-bit PCM: full scale 1.0 = 32767 (what read_audio divides by), values beyond it clipped"""
    from scipy.io import wavfile
    pcm = np.rint(np.clip(samples, -1.0, 1.0) * 32767.0).astype(np.int16)
    wavfile.write(path, int(fs), pcm)


def SpeedAugmentation(filelist, target_folder, speed):
    """Writes <target_folder>_<speed>/<stem>_<speed>.wav for every path in filelist and returns those paths in filelist's order."""
    folder = "%s_%s" % (target_folder, speed)
    os.makedirs(folder, exist_ok=True)
    written = [os.path.join(folder, "%s_%s.wav" % (_stem(src), speed)) for src in filelist]
    for src, dst in zip(filelist, written):
        samples, fs = read_audio(src)
        _save_wav16(dst, speed_perturb(samples, fs, speed), fs)
    return written


def VolumeAugmentation(filelist, target_folder, vol_range):
    """Writes <target_folder>/<stem>_<gain>.wav for every path in filelist, each with its own gain drawn uniformly from
    [vol_range[0], vol_range[1]], and returns those paths in filelist's order.  The gain is fixed to two decimals before it is
    applied, so the number in the file name is exactly the factor the samples were multiplied by."""
    os.makedirs(target_folder, exist_ok=True)
    lo, hi = float(vol_range[0]), float(vol_range[1])
    written = []
    for src in filelist:
        gain = round(float(np.random.uniform(lo, hi)), 2)
        samples, fs = read_audio(src)
        dst = os.path.join(target_folder, "%s_%s.wav" % (_stem(src), gain))
        _save_wav16(dst, gain * samples, fs)
        written.append(dst)
    return written
