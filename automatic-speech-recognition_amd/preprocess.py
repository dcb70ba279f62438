"""preprocess.py -- feature extraction entry point (counterpart of the reference's preprocess.py:50-108): MFCC / log-mel
filterbank + CMVN + delta / delta-delta cube [T, feat_dim, 3], tokenisation, dumps that create_tfrecord / decode.py read.

PARITY STATUS: unpinned.  The reference delegates the arithmetic to `speechpy` (speechpy.feature.mfcc / mfe,
speechpy.processing.cmvn, speechpy.feature.extract_derivative_feature; unpinned in requirements.txt) and reads audio with
`soundfile`; neither is installed in the build image and neither can be fetched.  The functions below RESTATE speechpy
2.4's published algorithm as called at reference preprocess.py:71-86 (frame stacking without zero padding and with a
rectangular window, 512-point power spectrum / fft_length, 40 triangular mel filters from 300 Hz -- speechpy's
`low_freq or 300` turns the default 0 into 300 -- log, orthonormal DCT-II, c0 replaced by log frame energy; CMVN with
variance normalisation and eps 2^-30; derivatives over a +-2 window taken ALONG THE FEATURE AXIS exactly as speechpy's
`derivative_extraction` pads and slides along axis 1).  This file is the float64 STATEMENT of the arithmetic:
csrc/frontend.hip evaluates the same steps on the device for a batch of utterances (las.frontend.FeatureExtractor; transcribe.py feeds
the search from it, `--frontend gpu` writes this entry point's dumps through it) and is tested against the functions below."""
import math
import os
import string
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def frequency_to_mel(f):
    return 1127.0 * np.log(1.0 + f / 700.0)


def mel_to_frequency(mel):
    return 700.0 * (np.exp(mel / 1127.0) - 1.0)


def _triangle(x, left, middle, right):
    out = np.zeros(x.shape)
    first_half = np.logical_and(left < x, x <= middle)
    out[first_half] = (x[first_half] - left) / (middle - left)
    second_half = np.logical_and(middle <= x, x < right)
    out[second_half] = (right - x[second_half]) / (right - middle)
    return out


def filterbanks(num_filter, coefficients, sampling_freq, low_freq=None, high_freq=None):
    high_freq = high_freq or sampling_freq / 2
    low_freq = low_freq or 300                                   # speechpy: a low frequency of 0 becomes 300 Hz
    mels = np.linspace(frequency_to_mel(low_freq), frequency_to_mel(high_freq), num_filter + 2)
    hertz = mel_to_frequency(mels)
    freq_index = (np.floor((coefficients + 1) * hertz / sampling_freq)).astype(int)
    fb = np.zeros([num_filter, coefficients])
    for i in range(num_filter):
        left, middle, right = int(freq_index[i]), int(freq_index[i + 1]), int(freq_index[i + 2])
        z = np.linspace(left, right, num=right - left + 1)
        fb[i, left:right + 1] = _triangle(z, left=left, middle=middle, right=right)
    return fb


def stack_frames(sig, sampling_frequency, frame_length, frame_stride):
    """speechpy.processing.stack_frames(..., filter=ones, zero_padding=False)"""
    n = sig.shape[0]
    fl = int(np.round(sampling_frequency * frame_length))
    fs = float(np.round(sampling_frequency * frame_stride))
    numframes = int(math.floor((n - fl) / fs))
    if numframes < 1:
        return np.zeros((0, fl))
    idx = np.tile(np.arange(0, fl), (numframes, 1)) + np.tile(np.arange(0, numframes * fs, fs), (fl, 1)).T
    return sig[np.array(idx, dtype=np.int32)]


def _zero_handling(x):
    return np.where(x == 0, np.finfo(float).eps, x)


def mfe(signal, sampling_frequency, frame_length=0.020, frame_stride=0.01, num_filters=40, fft_length=512, low_frequency=0,
        high_frequency=None):
    signal = signal.astype(float)
    frames = stack_frames(signal, sampling_frequency, frame_length, frame_stride)
    high_frequency = high_frequency or sampling_frequency / 2
    power_spectrum = 1.0 / fft_length * np.square(np.absolute(np.fft.rfft(frames, fft_length)))
    coefficients = power_spectrum.shape[1]
    frame_energies = _zero_handling(np.sum(power_spectrum, 1))
    fb = filterbanks(num_filters, coefficients, sampling_frequency, low_frequency, high_frequency)
    features = _zero_handling(np.dot(power_spectrum, fb.T))
    return features, frame_energies


def mfcc(signal, sampling_frequency, frame_length=0.020, frame_stride=0.01, num_cepstral=13, num_filters=40, fft_length=512,
         low_frequency=0, high_frequency=None, dc_elimination=True):
    from scipy.fftpack import dct
    feature, energy = mfe(signal, sampling_frequency, frame_length, frame_stride, num_filters, fft_length, low_frequency, high_frequency)
    if len(feature) == 0:
        return np.empty((0, num_cepstral))
    feature = np.log(feature)
    feature = dct(feature, type=2, axis=-1, norm='ortho')[:, :num_cepstral]
    if dc_elimination:
        feature[:, 0] = np.log(energy)
    return feature


def cmvn(vec, variance_normalization=False):
    eps = 2 ** -30
    mean_subtracted = vec - np.mean(vec, axis=0)
    if variance_normalization:
        return mean_subtracted / (np.std(mean_subtracted, axis=0) + eps)
    return mean_subtracted


def derivative_extraction(feat, DeltaWindows):
    rows, cols = feat.shape
    DIF = np.zeros(feat.shape, dtype=feat.dtype)
    Scale = 0
    FEAT = np.pad(feat, ((0, 0), (DeltaWindows, DeltaWindows)), 'edge')       # padded (and differenced) along the feature axis
    for i in range(DeltaWindows):
        offset = DeltaWindows
        Range = i + 1
        dif = Range * FEAT[:, offset + Range:offset + Range + cols] - FEAT[:, offset - Range:offset - Range + cols]
        Scale += 2 * np.power(Range, 2)
        DIF += dif
    return DIF / Scale


def extract_derivative_feature(feature):
    first = derivative_extraction(feature, DeltaWindows=2)
    second = derivative_extraction(first, DeltaWindows=2)
    return np.concatenate((feature[:, :, None], first[:, :, None], second[:, :, None]), axis=2)


def read_audio(path):
    """(samples float, sampling rate).  .wav through scipy; .npy as raw 16 kHz samples; .flac needs `soundfile` (the
    reference's reader, preprocess.py:68), which this image does not have."""
    if path.endswith(".npy"):
        return np.load(path).astype(float), 16000
    if path.endswith(".wav"):
        from scipy.io import wavfile
        fs, a = wavfile.read(path)
        if a.dtype.kind == "i":
            a = a.astype(float) / np.iinfo(a.dtype).max
        return a.astype(float), fs
    try:
        import soundfile as sf
    except ImportError:
        raise RuntimeError("reading %s needs the `soundfile` package (not available offline); convert to .wav" % path)
    return sf.read(path)


RESAMPLE_ROLLOFF, RESAMPLE_ZEROS, RESAMPLE_BETA = 0.92, 24, 10.0
SPEEDS = (0.9, 1.1)                                              # reference preprocess.py:160


def resample_table(fs_in, fs_out):
    """The band-limited resampler's polyphase table (float64): (L, M, W, h [L, 2W]).  fs_out / fs_in = L / M in lowest terms; the
    filter is a sinc cut at c = 0.92 x the narrower band's Nyquist under a Kaiser window (beta 10) of 24 zero crossings a side, i.e.
    W = ceil(24 / c) input samples.  Row p holds the 2W taps of an output that falls p / L of a sample behind input sample n0: tap i
    weighs x[n0 - W + 1 + i], at distance d = p / L + (W - 1) - i.  Every row is divided by its sum (a constant stays constant)."""
    fs_in, fs_out = int(fs_in), int(fs_out)
    if fs_in < 1 or fs_out < 1:
        raise ValueError("sample rates are positive (got %d -> %d)" % (fs_in, fs_out))
    g = math.gcd(fs_in, fs_out)
    L, M = fs_out // g, fs_in // g
    c = RESAMPLE_ROLLOFF * min(1.0, L / M)
    W = int(math.ceil(RESAMPLE_ZEROS / c))
    d = np.arange(L, dtype=float)[:, None] / L + (W - 1) - np.arange(2 * W, dtype=float)[None, :]
    u = d * c / RESAMPLE_ZEROS
    inside = np.abs(u) < 1
    kaiser = np.where(inside, np.i0(RESAMPLE_BETA * np.sqrt(np.where(inside, 1 - u * u, 0.0))) / np.i0(RESAMPLE_BETA), 0.0)
    h = c * np.sinc(c * d) * kaiser
    return L, M, W, h / h.sum(1, keepdims=True)


def resample_out_len(n, L, M):
    return (int(n) * L + M - 1) // M                             # ceil(n L / M), in integers


def resample(x, fs_in, fs_out, gain=1.0):
    """x (1-D, float64) from fs_in to fs_out: ceil(n L / M) samples, y[m] = gain * sum_i x[n0 - W + 1 + i] h[p, i] with
    n0 = (m M) // L, p = (m M) % L and x zero outside the recording.  Equal rates: gain * x, unfiltered."""
    x = np.asarray(x, dtype=float)
    if x.ndim != 1:
        raise ValueError("a waveform is a 1-D array (got shape %s)" % (x.shape,))
    if int(fs_in) == int(fs_out):
        return gain * x
    L, M, W, h = resample_table(fs_in, fs_out)
    n_out = resample_out_len(len(x), L, M)
    xp = np.concatenate([np.zeros(W - 1), x, np.zeros(W + 1)])    # xp[k] = x[k - W + 1]
    y = np.empty(n_out)
    taps = np.arange(2 * W, dtype=np.int64)[None, :]
    for m0 in range(0, n_out, 8192):                             # (blocks: the gathered [outputs, taps] matrix stays small)
        mM = np.arange(m0, min(m0 + 8192, n_out), dtype=np.int64) * M
        y[m0:m0 + len(mM)] = np.sum(xp[(mM // L)[:, None] + taps] * h[mM % L], axis=1)
    return gain * y


def speed_perturb(x, fs, speed, gain=1.0):
    """sox's `speed s`: the recording declared to be at fs * s Hz, resampled back to fs (0.9 at 16 kHz: 14400 -> 16000)"""
    return resample(x, int(round(fs * speed)), fs, gain)


# ---- multi-condition data: room reverberation and additive noise (csrc/wave_aug.hip evaluates the same in fp32) ----------------------
RIR_MAX = 16384                                                  # taps las_reverb takes (one second at 16 kHz)


def rir_delay(h):
    """the direct path of a room response: the index of the first sample of largest |h|"""
    return int(np.argmax(np.abs(np.asarray(h, dtype=float))))


def normalize_rir(h):
    """h scaled in float64 to unit energy (sum h^2 = 1), so that reverberation does not change the level much"""
    h = np.asarray(h, dtype=float)
    e = float(np.sum(h * h))
    if h.ndim != 1 or len(h) < 1 or not e > 0:
        raise ValueError("a room response is a 1-D array with some energy")
    return h / math.sqrt(e)


def reverberate(x, h, delay):
    """y[m] = sum_{k < K} h[k] x[m + delay - k] for m in [0, len(x)), x zero outside the recording: the output has the input's length
    and the direct path (tap `delay`) does not shift the speech"""
    x, h = np.asarray(x, dtype=float), np.asarray(h, dtype=float)
    if x.ndim != 1 or h.ndim != 1 or len(h) < 1 or not 0 <= int(delay) < len(h):
        raise ValueError("reverberate: 1-D arrays and 0 <= delay < len(h) (got %s, %s, %s)" % (x.shape, h.shape, delay))
    if len(x) == 0:
        return x.copy()
    return np.convolve(x, h)[int(delay):int(delay) + len(x)]


def _noise_segment(s, noise, offset):
    s, noise = np.asarray(s, dtype=float), np.asarray(noise, dtype=float)
    if s.ndim != 1 or noise.ndim != 1 or len(noise) < 1 or not 0 <= int(offset) < len(noise):
        raise ValueError("mix_noise: 1-D arrays and 0 <= offset < len(noise) (got %s, %s, %s)" % (s.shape, noise.shape, offset))
    return s, noise[(int(offset) + np.arange(len(s), dtype=np.int64)) % len(noise)]


def noise_gain(s, noise, offset, snr_db):
    """g = sqrt(Ps / (Pn 10^(snr_db / 10))) with Ps = mean(s^2) over the recording and Pn = mean(v^2) over the noise segment actually
    used, v[m] = noise[(offset + m) mod len(noise)]; 0 when either is silent"""
    s, v = _noise_segment(s, noise, offset)
    if len(s) == 0:
        return 0.0
    Ps, Pn = float(np.mean(s * s)), float(np.mean(v * v))
    if Ps == 0 or Pn == 0:
        return 0.0
    return math.sqrt(Ps / (Pn * 10.0 ** (float(snr_db) / 10.0)))


def mix_noise(s, noise, offset, snr_db):
    """y = s + g v, g = noise_gain(...): the noise, wrapped around, at snr_db under the recording; a silent recording or a silent
    segment gives a copy of s"""
    g = noise_gain(s, noise, offset, snr_db)
    s, v = _noise_segment(s, noise, offset)
    return s.copy() if g == 0 else s + g * v


def synthetic_rir(fs, rt60, seed, length_s=None):
    """a room response without a room: a unit direct path at sample 0 and, behind it, seeded Gaussian noise under an exponential
    envelope that reaches -60 dB at rt60 seconds (Polack's model); length_s defaults to rt60, at most RIR_MAX taps"""
    fs, rt60 = int(fs), float(rt60)
    if fs < 1 or not rt60 > 0:
        raise ValueError("synthetic_rir: fs=%d, rt60=%g" % (fs, rt60))
    n = int(round(fs * (rt60 if length_s is None else float(length_s))))
    n = min(max(n, 1), RIR_MAX)
    t = np.arange(n, dtype=float) / fs
    h = 0.1 * np.random.RandomState(int(seed)).randn(n) * 10.0 ** (-3.0 * t / rt60)      # amplitude x 10^-3 = -60 dB at t = rt60
    h[0] = 1.0
    return h


def load_bank(path, fs):
    """the .wav / .npy files of a directory (sorted by name) as float64 arrays at fs Hz: read_audio, first channel, resampled if need be"""
    bank = []
    for name in sorted(os.listdir(path)):
        if name.endswith(".wav") or name.endswith(".npy"):
            a, f = read_audio(os.path.join(path, name))
            if a.ndim > 1:
                a = a[:, 0]
            bank.append(resample(a, int(f), int(fs)))
    if not bank:
        raise ValueError("no .wav / .npy files in %s" % path)
    return bank


def _pair(text, what):
    lo, hi = (float(v) for v in str(text).split(","))
    if hi < lo:
        raise ValueError("%s is lo,hi (got %s)" % (what, text))
    return lo, hi


def wave_augmenter(args, device=None):
    """the las.augment.WaveAugmenter of the --rir_dir / --rir_synthetic / --rt60 / --noise_dir / --snr_range / --reverb_prob flags (None
    when they name no bank).  Its plan is drawn on the host: the CPU and the device front end augment from the same plan."""
    from las.augment import WaveAugmenter
    fs = int(args.sample_rate)
    rirs = load_bank(args.rir_dir, fs) if args.rir_dir else []
    if int(args.rir_synthetic) > 0:
        lo, hi = _pair(args.rt60, "--rt60")
        rng = np.random.RandomState(int(args.seed) + 7)
        rirs = rirs + [synthetic_rir(fs, rng.uniform(lo, hi), int(args.seed) + 1000 + i) for i in range(int(args.rir_synthetic))]
    noises = load_bank(args.noise_dir, fs) if args.noise_dir else []
    if not rirs and not noises:
        return None
    return WaveAugmenter(fs, rirs=rirs or None, noises=noises or None, snr_db=_pair(args.snr_range, "--snr_range"), reverb_prob=args.reverb_prob,
                         seed=int(args.seed), device=device)


def augment_wave(audio, aug, plan, u):
    """row u of a plan applied in float64: reverberate with the bank's (normalised) response, then mix_noise"""
    if plan.rir_idx[u] >= 0:
        h = aug.rirs[plan.rir_idx[u]]
        audio = reverberate(audio, h, aug.rir_delay[plan.rir_idx[u]])
    if plan.noise_idx[u] >= 0:
        audio = mix_noise(audio, aug.noises[plan.noise_idx[u]], int(plan.noise_off[u]), float(plan.snr_db[u]))
    return audio


def process_audios(audio_path, args, speed=1.0, augment=None, step=0):
    """reference preprocess.py:50-91.  Returns (feats: list of float32 [L, feat_dim, 3] (or [L, feat_dim] without --cmvn), featlen).
    speed != 1: every recording through speed_perturb first (the reference's speed augmentation, without the audio files between).
    augment (a las.augment.WaveAugmenter): recording u, brought to --sample_rate, takes row u of augment.plan(len(audio_path), step) in
    float64 (augment_wave) -- the noisy copies of --noisy_copies."""
    feats, featlen = [], []
    plan = augment.plan(len(audio_path), step) if augment is not None else None
    for u, p in enumerate(audio_path):
        audio, fs = read_audio(p)
        if speed != 1.0:
            audio = speed_perturb(audio, fs, speed)
        if plan is not None:
            audio, fs = augment_wave(resample(audio, fs, args.sample_rate), augment, plan, u), int(args.sample_rate)
        if args.feat_type == 'mfcc':
            feat = mfcc(audio, fs, frame_length=args.frame_length / 1000, frame_stride=args.frame_step / 1000, num_cepstral=args.feat_dim)
        elif args.feat_type == 'fbank':
            feat, _ = mfe(audio, fs, frame_length=args.frame_length / 1000, frame_stride=args.frame_step / 1000, num_filters=args.feat_dim)
        else:
            raise ValueError(args.feat_type)
        if args.cmvn:
            feat = cmvn(feat, True)
            feat = extract_derivative_feature(feat)
        feats.append(feat.astype(np.float32))
        featlen.append(len(feats[-1]))
    return feats, featlen


def process_audios_gpu(audio_path, args, batch=64, speed=1.0, augment=None, step=0):
    """process_audios through the device front end: `batch` utterances per las_frontend call, the same lists of float32 arrays.  The
    kernels' tables are built for args.sample_rate: a file at another rate is resampled to it on the device (las_resample), and so is
    every file when speed != 1 (speed_perturb's arithmetic in fp32).  augment: the rows [c0, c0 + batch) of the same plan the CPU
    front end draws, applied by las_reverb and las_noise_mix between the resampler and the front end"""
    from las.frontend import FeatureExtractor
    fe = FeatureExtractor(args)
    feats, featlen = [], []
    for c0 in range(0, len(audio_path), batch):
        plan = augment.plan(len(audio_path[c0:c0 + batch]), step, row0=c0, rows_global=len(audio_path)) if augment is not None else None
        waves, rates = [], []
        for p in audio_path[c0:c0 + batch]:
            audio, fs = read_audio(p)
            waves.append(audio)
            rates.append(int(fs))
        cube, lens = fe.extract(waves, rate=rates, speed=speed) if plan is None else fe.extract(waves, rate=rates, speed=speed, augment=plan)
        cube = cube.cpu().numpy()
        for u, t in enumerate(lens):
            feats.append(cube[u, :t].copy())
            featlen.append(int(t))
    return feats, featlen


def process_texts(texts, tokenizer):
    """reference preprocess.py:93-108: strip punctuation, encode with EOS."""
    tokens, tokenlen = [], []
    for sentence in texts:
        sentence = sentence.translate(str.maketrans('', '', string.punctuation))
        tokens.append(tokenizer.encode(sentence, with_eos=True))
        tokenlen.append(len(tokens[-1]))
    return tokens, np.array(tokenlen).astype(np.int32)


def data_preparation(libri_path):
    """reference preprocess.py:26-48: walk speaker/chapter folders, pair every transcript line with its audio file."""
    from glob import glob
    texts, audio_path = [], []
    for path in sorted(glob(libri_path + "/*/*")):
        tp = glob(path + "/*txt")
        if not tp:
            continue
        for line in open(tp[0]).readlines():
            line_ = line.split(" ")
            base = path + "/" + line_[0]
            ext = next((e for e in (".wav", ".npy") if os.path.exists(base + e)), ".flac")       # (.npy: raw 16 kHz samples, read_audio)
            audio_path.append(base + ext)
            texts.append(line[len(line_[0]) + 1:-1].replace("'", ""))
    return texts, audio_path


def main():
    import joblib
    from las.arguments import parse_args
    from utils.tokenizer import CharEncoder, SubwordEncoder
    args = parse_args()
    if args.frontend not in ("cpu", "gpu"):
        raise ValueError("--frontend is cpu or gpu (got %s)" % args.frontend)
    tokenizer = CharEncoder() if args.unit.lower() == "char" else SubwordEncoder(args.subword_dir)
    os.makedirs(args.feat_dir, exist_ok=True)
    for split, path in (("train-100", args.train_100hr_corpus_dir), ("dev", args.dev_data_dir), ("test", args.test_data_dir)):
        if not os.path.isdir(path):
            continue
        texts, audio_path = data_preparation(path)
        process = process_audios_gpu if args.frontend == "gpu" else process_audios
        feats, featlen = process(audio_path, args)
        tokens, tokenlen = process_texts(texts, tokenizer)
        joblib.dump(feats, os.path.join(args.feat_dir, "%s-feats.pkl" % split))
        np.save(os.path.join(args.feat_dir, "%s-featlen.npy" % split), np.asarray(featlen))
        np.save(os.path.join(args.feat_dir, "%s-%ss.npy" % (split, args.unit)), np.asarray(tokens, dtype=object), allow_pickle=True)
        np.save(os.path.join(args.feat_dir, "%s-%slen.npy" % (split, args.unit)), tokenlen)
        print("%s: %d utterances -> %s" % (split, len(feats), args.feat_dir))
        if args.augmentation and "train" in split:               # reference preprocess.py:157-167, straight from the recordings
            for s in SPEEDS:
                feats, featlen = process(audio_path, args, speed=s)
                joblib.dump(feats, os.path.join(args.feat_dir, "speed_%s-feats.pkl" % s))
                np.save(os.path.join(args.feat_dir, "speed_%s-featlen.npy" % s), np.asarray(featlen))
                print("speed_%s: %d utterances -> %s" % (s, len(feats), args.feat_dir))
            if int(args.noisy_copies) > 0:                       # multi-condition copies: reverberation and noise, drawn per (seed, copy)
                aug = wave_augmenter(args)
                if aug is None:
                    raise ValueError("--noisy_copies needs a bank: --rir_dir, --rir_synthetic N or --noise_dir")
                for k in range(int(args.noisy_copies)):
                    feats, featlen = process(audio_path, args, augment=aug, step=k)
                    joblib.dump(feats, os.path.join(args.feat_dir, "noisy_%d-feats.pkl" % k))
                    np.save(os.path.join(args.feat_dir, "noisy_%d-featlen.npy" % k), np.asarray(featlen))
                    print("noisy_%d: %d utterances -> %s" % (k, len(feats), args.feat_dir))


if __name__ == "__main__":
    main()
