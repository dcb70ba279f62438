"""transcribe.py -- from audio to text: .wav / .npy files -> one hypothesis per line.

    python transcribe.py [model / checkpoint / LM / CTC flags of decode.py] a.wav b.wav ...
    python transcribe.py --synthetic True            (random weights, generated noise "audio": runs with no data)
    python transcribe.py --synthetic True a.wav ...  (random weights on the given files: the audio path without a checkpoint)
    python transcribe.py --ctc True --timestamps True a.wav ...        (one JSON object per line: text, score, word times)
    python transcribe.py --ctc True --align_text refs.txt a.wav ...    (forced alignment: line k of refs.txt is the transcript of file k)
    python transcribe.py --segment True meeting.wav ...                (long recordings: cut at the silences first, one line per file)
    python transcribe.py --hotwords names.txt --hotword_weight 2.0 a.wav ...   (contextual biasing: the search boosts the listed phrases)
    python transcribe.py --ngram_lm lm.arpa --ngram_weight 0.5 a.wav ...       (n-gram LM shallow fusion: train_ngram.py writes lm.arpa)
    python transcribe.py --nbest 5 --confidence True --mbr True a.wav ...      (N-best consensus: alternatives, confidences, MBR choice)
    python transcribe.py --confusion_network True --cn_decode True a.wav ...   (word alternatives per position, and their consensus)
    python transcribe.py --ctc True --decoder ctc --beam_size 16 a.wav ...     (the CTC head alone: prefix beam search, greedy with --beam_size 1)
    python transcribe.py --noise_file cafe.wav --snr_db 10 --rir_file room.wav a.wav ...   (the files as they would sound in that condition)
    python transcribe.py --ctc True --keywords names.txt a.wav ...     (keyword search: where the CTC head hears a listed phrase, no search)
    python transcribe.py --coverage_report True a.wav ...              (JSON lines with the shares of attended / over-attended encoder frames)
    python transcribe.py --coverage_weight 0.3 --overattend_weight 0.7 a.wav ...   (attention coverage scored in the beam search)
    python transcribe.py --segment True --diarize True meeting.wav ...  (who spoke when: every segment labelled with its speaker)
    python transcribe.py --beamform True array.wav ...                 (microphone arrays: delay-and-sum to one channel first)
    python transcribe.py --beamform True --bf_method mvdr array.wav ...   (... or a mask-driven MVDR beamformer: cancels directional noise)

With --timestamps the best hypothesis is aligned to the encoder frames by the CTC head (las.align, csrc/ctc_align.hip: a Viterbi pass
over the head's log-probabilities) and every line is {"text", "score", "words": [{"word", "start", "end"}]}: times in seconds, None when
the hypothesis has more tokens than the recording has frames; score = the log-probability of the best alignment path (None likewise).
--align_text skips the search and aligns the given transcripts.

With --segment every file is first cut into segments by an energy voice-activity detector on the device (las.vad, csrc/vad.hip: speech =
frames within --vad_top_db of the file's loudest and over --vad_floor_db, padded by --vad_pad_ms, runs under --vad_min_speech_ms
dropped, runs over --max_segment_s -- the training cap -- cut at their quietest frame).  The segments of all files form one stream that
goes through the front end and the search --decode_batch at a time, as files do otherwise.  A file's line is its segments' hypotheses
joined by one space (an empty line for a silent file); with --timestamps it is {"text", "score", "words", "segments": [{"start", "end",
"text", "score", "words"}]}: word times offset by the segment's start, score = the sum of the segment scores (None if one is None).

With --nbest K, --confidence True or --mbr True (las.nbest, csrc/nbest.hip; any of them switches to JSON lines, none needs the CTC head)
the search's whole ranked list is used: posteriors = softmax over the list of --nbest_scale x the search's ranking key; --nbest adds
"nbest": [{"text", "score", "posterior"}], best first; --confidence adds "confidence" = the printed hypothesis' posterior and "words":
[{"word", "confidence"}] (with --timestamps the same word objects carry start, end and confidence), a word's confidence = the least
posterior mass that agrees with one of its tokens; --mbr prints the hypothesis of least expected token edit distance instead of the
top-scoring one, and --timestamps / --confidence then describe that one.  Without --timestamps "score" is the search's score.  With
--segment a file's confidence is the minimum over its segments, its words are concatenated and "nbest" stays with the segments.

With --confusion_network True (las.nbest.network, las_nbest_network; JSON lines) the ranked list is merged, best first, into a confusion
network and every line carries "network": [[{"word", "p"}, ...], ...]: per position the --cn_alternatives (1 to 8, default 3) words of
largest posterior mass, "" = no word here; --cn_unit token keeps the tokenizer's pieces instead of words.  --cn_decode True prints the
network's consensus -- the first alternative of every position, "" left out, joined by one space -- instead of the 1-best; no search
produced that text, so "score" is null, and with --confidence "words" carry the positions' masses and "confidence" is their minimum.
Both go with either decoder, --rescore, --segment (a file's network is its segments' positions in order) and --nbest / --confidence /
--mbr; --cn_decode cannot be combined with --mbr, --timestamps or --align_text, neither flag with --keywords.

With --noise_file and / or --rir_file (las.augment, csrc/wave_aug.hip) every recording is convolved with the room response and mixed
with the noise at --snr_db on the device, between the resampler and the front end: a model's robustness checked without writing audio
files.  The noise starts at its first sample and wraps around; both files are resampled to --sample_rate.  Without the two flags
las.augment is not imported and the output is what it was.

With --keywords FILE (las.kws, csrc/kws.hip; the phrase-file format of --hotwords) the search is skipped, as with --align_text: the
listener, the head, and one las_kws_search per batch.  Every file's line is {"hits": [{"keyword", "start", "end", "score",
"confidence"}]}, sorted by start, then by the phrase's place in the list: score = the log-likelihood ratio of the phrase's best path
against the head's frame-wise best path over the same frames (<= 0), confidence = exp(score / tokens of the phrase).  A hit needs
score >= --keyword_threshold x tokens (default -1.0 nat per token, not measured on a trained model); --keyword_max_hits (1 to 8) hits
are kept per file and phrase.  It cannot be combined with --align_text, --segment, --timestamps, --nbest, --confidence, --mbr,
--confusion_network or --cn_decode.

With --coverage_weight / --overattend_weight (las.coverage, csrc/coverage.hip) the beam search adds --coverage_weight for
every encoder frame whose accumulated attention rises above --coverage_threshold and takes --overattend_weight for every frame that
rises above --overattend_threshold; plain text stays plain text, and every JSON record (and listed N-best hypothesis) carries
"coverage" and "overattended", the two shares of the utterance's -- under --segment the segment's -- encoder frames.
--coverage_report True counts with whatever weights and switches to JSON lines.  With --rescore attention the term joins the second
pass' attention score.  --keywords, --align_text and --decoder ctc without --rescore attention run no attention decoder and refuse
the flags; --cn_decode prints a text no search produced and carries no coverage fields.

With --segment True --diarize True (las.diarize, csrc/diarize.hip; JSON lines) every speech run of the detector is split where
the speaker changes -- the peaks of the delta-BIC curve between two adjacent windows of --diar_window_ms, every --diar_hop_ms, full-
covariance Gaussians over the 13 static MFCCs of the detector's speech frames, penalty weight --diar_change_lambda -- and the pieces of
a file are clustered agglomeratively under the same criterion (--diar_cluster_lambda) until no merge lowers the BIC, or down to
--num_speakers.  The pieces then go through the --max_segment_s cut as runs do.  Every segment record gains "speaker" (1, 2, ... in the
order of first appearance), the file's line "speakers" (the count), and with --timestamps / --confidence every word object "speaker";
--rttm FILE also writes `SPEAKER <file stem> 1 <start> <duration> <NA> <NA> S<k> <NA> <NA>` per segment.  No trained model is involved
and nobody has measured a diarization error rate for the defaults; overlapped speech is not handled.  --diarize needs --segment and
cannot be combined with --keywords or --align_text.  Without it las.diarize is not imported and the output is what it was.

With --beamform True (las.beamform, csrc/beamform.hip) a file with two to sixteen channels -- a .wav, or a .npy of shape [n, C] --
is accepted: at its own sample rate, before anything else sees it, the delay of every channel against the reference channel --bf_ref
is taken per window of --bf_window_ms (every half window) from the peak of the PHAT-weighted cross-correlation within
--bf_max_delay_ms, the delays are smoothed over the windows by a Viterbi pass (--bf_jump_penalty per sample of lag per window), and the
channels are shifted by whole samples, weighted by their coherence with the reference, and summed.  The mono result takes the path of
any mono file (resampling, --segment, --diarize, --noise_file, --rir_file, the front end, the search); a mono file passes through
untouched; the output records are what they are without the flag.  --beamform_wav DIR also writes every beamformed file as
DIR/<stem>.wav, 16-bit at the file's rate.  No trained model is involved, nobody has measured a word error rate with it, and no
default has been tuned on a real room.  A --bf_* value or --beamform_wav without --beamform True is refused before audio is read;
without the flag las.beamform is not imported and a multi-channel file is refused as before.

With --beamform True --bf_method mvdr (csrc/mvdr.hip) the channels are combined by an MVDR beamformer in the STFT domain
instead: frames of --mvdr_frame_ms (the next power of two samples; 32) every half frame; the frames of --bf_ref within --mvdr_top_db (25)
of its loudest frame and over --mvdr_floor_db (as --vad_floor_db), widened by --mvdr_pad_ms (100), are speech and every other frame
trains the noise covariance; the speech covariance and the weights are taken per block of --mvdr_block_ms (2000), with
--mvdr_loading (1e-3) on the noise covariance's diagonal.  It needs no delays and no geometry and cancels a directional disturbance,
which delay-and-sum cannot.  A file whose mask leaves no noise frame or no speech frame comes out as its reference channel, with a
one-line warning on stderr that names --mvdr_top_db (a disturbance as loud as the talker needs a small value, a few dB).  A --mvdr_*
value without --bf_method mvdr, --bf_method mvdr without --beamform True, and --bf_window_ms, --bf_max_delay_ms or --bf_jump_penalty
with --bf_method mvdr are refused before audio is read.  Everything downstream is as with delay-and-sum.  Not built: online or
recursive covariance updates, GEV / rank-1 variants, a learned mask, cross-fades between blocks, and handing y to the front end on
the device.

The files are read with preprocess.read_audio (.flac needs `soundfile`), `--decode_batch` of them at a time go through the device front
end (las.frontend.FeatureExtractor: waveform -> feature cube, csrc/frontend.hip; a file at another rate than --sample_rate is resampled
on the device first, csrc/resample.hip) and stay on the device for BeamSearch.decode_batches:
the extraction and the encoders of batch k+1 run under the search of batch k.  The reference has no such entry point (its decode.py reads
the feature dumps of preprocess.py); the model side is decode.py's."""
import collections
import json
import logging
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from las import align as A                                         # noqa: E402
from las import transcript as T                                    # noqa: E402
from las import vad as VAD                                         # noqa: E402
from las.arguments import build_parser, str2bool                   # noqa: E402
from las.cli import add_beamform_flags, add_diarize_flags, add_flags, build_search, check_flags, encoded_batches, make_tokenizer   # noqa: E402
from las.frontend import FeatureExtractor                          # noqa: E402
from preprocess import read_audio                                  # noqa: E402


def synthetic_audio(n, fs, seed):
    """n noise "recordings" of 1-3 s (broadband, so every mel band is populated)"""
    rng = np.random.RandomState(seed)
    return [(0.1 * rng.randn(int(fs * rng.uniform(1.0, 3.0)))).astype(np.float32) for _ in range(n)]


def main(argv=None):
    import torch
    parser = build_parser()
    add_flags(parser)
    VAD.add_flags(parser, str2bool)
    add_diarize_flags(parser)
    add_beamform_flags(parser)
    args = parser.parse_args(argv)
    mode = check_flags(args, parser)
    logging.basicConfig(stream=sys.stderr, format='%(asctime)s %(levelname)s:%(message)s', level=logging.INFO, datefmt='%I:%M:%S')
    tokenizer = make_tokenizer(args)
    if mode.kind == "keywords":                                        # (las.kws is imported only when the flag is given)
        from las import kws as KW
        keywords = KW.KeywordList.from_file(args.keywords, tokenizer, args.vocab_size)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    heads = [flag for flag, on in (("--timestamps", args.timestamps), ("--keywords", mode.kind == "keywords")) if on]
    _, bs, _, search = build_search(args, dev, mode.ctc_only, restore_las=not args.synthetic, restore_lm_weights=not args.synthetic,
                                    need_head=heads, tokenizer=tokenizer)       # (need_head: refused before any audio is read)
    ann = None
    if mode.annotate:                                                  # (las.nbest is imported only when one of its flags is given)
        from las import nbest as NB
        ann = NB.Annotator(args, bs.end_id, tokenizer.id_to_token)
    fe = FeatureExtractor(args, device=dev)
    condition = None
    if args.noise_file or args.rir_file:                               # (las.augment is imported only when one of its flags is given)
        from las.augment import WaveAugmenter
        from preprocess import resample

        def bank(path):
            a, fs = read_audio(path)
            return [resample(a if a.ndim == 1 else a[:, 0], int(fs), int(args.sample_rate))]
        if not np.isfinite(args.snr_db):
            raise ValueError("--snr_db %s" % args.snr_db)
        condition = WaveAugmenter(args.sample_rate, rirs=bank(args.rir_file) if args.rir_file else None,
                                  noises=bank(args.noise_file) if args.noise_file else None, device=dev)

    def extract(chunk):
        plan = None if condition is None else condition.fixed_plan(len(chunk), rir_idx=0 if args.rir_file else -1,
                                                                   noise_idx=0 if args.noise_file else -1, snr_db=args.snr_db)
        return fe.extract([w for w, _ in chunk], rate=[fs for _, fs in chunk], augment=plan)

    count = len(args.audio)
    waves = None
    if args.synthetic and not args.audio:
        count = args.max_steps if args.max_steps >= 0 else 8
        waves = synthetic_audio(count, args.sample_rate, args.seed + 2)
    if mode.kind == "align":
        with open(args.align_text) as f:
            texts = [line.strip() for line in f.read().splitlines()]
        if len(texts) != count:
            raise ValueError("--align_text %s holds %d lines for %d audio files" % (args.align_text, len(texts), count))

    durations = collections.deque()                                    # seconds per file, in the order of the results

    beamformer = None
    if args.beamform:                                                  # (las.beamform is imported only when the flag is given)
        from las import beamform as BF
        beamformer = BF.Beamformer(args, device=dev)
        if args.beamform_wav:
            os.makedirs(args.beamform_wav, exist_ok=True)

    def load(i):
        audio, fs = (waves[i], args.sample_rate) if waves is not None else read_audio(args.audio[i])
        if beamformer is not None and audio.ndim == 2 and audio.shape[1] >= 2:      # one upload, three (mvdr: four) calls, one read-back per file
            audio, _ = beamformer.enhance(audio, int(fs))
            if args.beamform_wav:
                BF.write_wav(os.path.join(args.beamform_wav, os.path.splitext(os.path.basename(args.audio[i]))[0] + ".wav"), audio, fs)
        if audio.ndim != 1:
            raise ValueError("%s has %d channels: mono recordings only" % (args.audio[i], audio.shape[1]))
        durations.append(len(audio) / float(fs))
        return audio, int(fs)

    frame_s = A.frame_seconds(args, args.enc_type)
    record = lambda *rec: T.record(args, tokenizer.id_to_token, frame_s, *rec)
    if args.segment:
        va = VAD.VoiceActivity(args, device=dev)
        files = T.FileAssembler(record, mode.json, args.timestamps, ann is not None and ann.confidence, ann is not None and ann.cn)
        cut, sink = lambda audio, fs: files.add_file(va.segments(audio, fs), fs), files.take     # (one las_vad call and one wait per file)
        if args.diarize:                                               # (las.diarize is imported only when the flag is given)
            from las import diarize as DZ
            dz, rttm = DZ.Diarizer(args, device=dev), []

            def cut(audio, fs):                                        # las_vad, las_bic_change and las_bic_cluster: three waits per file
                ranges, speakers, count = dz.segments(va, audio, fs)
                stem = os.path.splitext(os.path.basename(args.audio[len(durations) - 1]))[0] if waves is None else "synthetic%d" % (len(durations) - 1)
                rttm.extend(DZ.rttm_line(stem, s0 / float(fs), (s1 - s0) / float(fs), k) for (s0, s1), k in zip(ranges, speakers))
                return files.add_file(ranges, fs, speakers=(speakers, count))
    else:
        def cut(audio, fs):
            return [(0, len(audio))]

        def sink(tokens, score, span, extra):
            d = record(tokens, score, span, extra, durations.popleft())
            print(json.dumps(d) if mode.json else d["text"])
    batches = T.batches(load, count, max(1, int(args.decode_batch)), extract, cut)
    if mode.kind == "search":
        bs.retain_align = bool(args.timestamps)
        T.run(search, batches, lambda results: T.choose(args, bs, ann, results, tokenizer.id_to_token), sink)
        if args.segment:
            files.emit_finished()                                      # (trailing silent files; no file at all is left unfinished)
            assert not files.files
    elif mode.kind == "keywords":                                      # the listener and the head, no search; one JSON object per file
        for encs, enc_lens, h_one, ctc_lp in encoded_batches(bs, batches):
            found = bs.keyword_search(encs, enc_lens, keywords, h_one=h_one, ctc_lp=ctc_lp, threshold_per_token=args.keyword_threshold,
                                      max_hits=args.keyword_max_hits)
            for hits in found.hits:
                print(json.dumps({"hits": KW.timed_hits(hits, keywords, frame_s, durations.popleft())}))
    else:                                                              # forced alignment: the listener and the head, no search
        done = 0
        for encs, enc_lens, h_one, ctc_lp in encoded_batches(bs, batches):
            token_lists = [tokenizer.encode(t, with_eos=True) for t in texts[done:done + len(encs)]]
            done += len(encs)
            for tokens, score, span in zip(token_lists, *bs.align(encs, enc_lens, token_lists, h_one=h_one, ctc_lp=ctc_lp)):
                sink(tokens, score, span, {})
    if args.segment and args.diarize and args.rttm:
        with open(args.rttm, "w") as f:
            f.write("".join(line + "\n" for line in rttm))
    sys.stdout.flush()


if __name__ == "__main__":
    main()
