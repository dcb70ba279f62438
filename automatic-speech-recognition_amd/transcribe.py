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
from las import layers, variables                                  # noqa: E402
from las import align as A                                         # noqa: E402
from las import vad as VAD                                         # noqa: E402
from las.arguments import build_parser, check_confusion_flags, str2bool   # noqa: E402
from las.beam_search import BeamSearch                             # noqa: E402
from las.frontend import FeatureExtractor                          # noqa: E402
from las.las import LAS, Listener, Speller                         # noqa: E402
from las.utils import convert_idx_to_string                        # noqa: E402
from preprocess import read_audio                                  # noqa: E402
from utils.tokenizer import CharEncoder, SubwordEncoder            # noqa: E402


def synthetic_audio(n, fs, seed):
    """n noise "recordings" of 1-3 s (broadband, so every mel band is populated)"""
    rng = np.random.RandomState(seed)
    return [(0.1 * rng.randn(int(fs * rng.uniform(1.0, 3.0)))).astype(np.float32) for _ in range(n)]


def annotated(args, bs, ann, results, id_to_token):
    """--nbest / --confidence / --mbr: per utterance (tokens of the hypothesis to print, its score, its frame spans or None, the extra
    JSON fields).  One consensus call for the batch (las.nbest.Annotator), and -- with --timestamps -- one alignment of the chosen
    hypotheses; score = the alignment's with --timestamps (as without these flags), else the search's."""
    from las import nbest as NB
    notes = ann.annotate(results)
    token_lists = [list(a["state"].token_ids[1:]) if a["state"] is not None else [] for a in notes]
    if args.timestamps:
        scores, spans = bs.align_results(results, token_lists)
    else:
        scores, spans = [float(a["state"].log_prob) if a["state"] is not None else None for a in notes], [None] * len(notes)
    out = []
    rescored = getattr(results, "rescored", None)                      # --rescore attention: both passes' scores of every listed hypothesis
    for u, (a, tokens, score, span) in enumerate(zip(notes, token_lists, scores, spans)):
        extra = {}
        if ann.cn:
            extra["network"] = a.get("network", [])
        if ann.cn_decode:                                              # the consensus: a text no search produced, so it has no score
            cons = a.get("consensus", dict(words=[], conf=[], tokens=[], text=""))
            extra["text"], score = cons["text"], None
            if ann.confidence:
                extra["confidence"] = min(cons["conf"]) if cons["conf"] else None
                extra["word_conf"] = [{"word": w, "confidence": c} for w, c in zip(cons["words"], cons["conf"])]
        elif ann.confidence:
            extra["confidence"] = a["posterior"]
            extra["word_conf"] = NB.word_confidence(a["tokens"], a["conf"], id_to_token, args.unit)
        if ann.nbest:
            extra["nbest"] = [{"text": convert_idx_to_string(t, id_to_token, args.unit), "score": sc if np.isfinite(sc) else None,
                               "posterior": p} for t, sc, p in a["nbest"]]
            if rescored is not None:
                for j, e in enumerate(extra["nbest"]):                 # (the list is best first, the results ascend)
                    d = rescored[u][len(rescored[u]) - 1 - j]
                    e["ctc_score"], e["att_score"] = (x if np.isfinite(x) else None for x in (d["first"], d["att"]))
        out.append((tokens, score, span, extra))
    return out


def json_fields(args, tokens, score, span, extra, id_to_token, frame_s, duration):
    """the JSON object of one utterance (or segment) under --nbest / --confidence / --mbr: text, score, [confidence], [words], [nbest]"""
    d = {"text": convert_idx_to_string(tokens, id_to_token, args.unit), "score": score if score is not None and np.isfinite(score) else None}
    words = A.words(tokens, span, id_to_token, args.unit, frame_s, duration) if span is not None else None
    if "word_conf" in extra:
        d["confidence"] = extra["confidence"]
        if words is None:
            words = extra["word_conf"]
        else:                                                          # (the same segmentation: the two lists zip)
            for w, c in zip(words, extra["word_conf"]):
                w["confidence"] = c["confidence"]
    if words is not None:
        d["words"] = words
    if "nbest" in extra:
        d["nbest"] = extra["nbest"]
    if "text" in extra:                                                # --cn_decode
        d["text"] = extra["text"]
    if "network" in extra:
        d["network"] = extra["network"]
    return d


def main(argv=None):
    import torch
    from decode import load_lm, restore_lm
    parser = build_parser()
    parser.add_argument("audio", nargs="*", help=".wav / .npy files to transcribe")
    parser.add_argument("--timestamps", type=str2bool, default=False, help="One JSON object per line with word times (needs --ctc True).")
    parser.add_argument("--align_text", type=str, default=None, metavar="FILE",
                        help="Forced alignment: one transcript per audio file, in order; skips the search, implies --timestamps True.")
    parser.add_argument("--keywords", type=str, default=None, metavar="FILE",
                        help="Keyword search: one phrase per line ('#' comments); skips the search and prints, per audio file, one JSON "
                             "object with the places the CTC head hears a phrase (needs --ctc True).")
    parser.add_argument("--keyword_threshold", type=float, default=-1.0,
                        help="A hit needs a score of at least this many nats per token of its phrase (the score is the phrase's "
                             "log-likelihood ratio against the head's frame-wise best path: <= 0).  The default of -1.0 is a guess: "
                             "nobody has measured it on a trained model.")
    parser.add_argument("--keyword_max_hits", type=int, default=4, help="Hits kept per file and phrase, the strongest (1 to 8).")
    VAD.add_flags(parser, str2bool)
    args = parser.parse_args(argv)
    network = check_confusion_flags(args)
    if args.keywords is not None:
        if not args.ctc:
            raise ValueError("--keywords needs the CTC head: decode with --ctc True (a model trained with --ctc)")
        for flag, on, why in (("--align_text", args.align_text is not None, "aligns a given transcript"),
                              ("--segment", args.segment, "cuts the recordings first; searching the segments is not built"),
                              ("--timestamps", args.timestamps, "times the search's hypothesis"),
                              ("--nbest", args.nbest, "reads the search's N-best list"),
                              ("--confidence", args.confidence, "reads the search's N-best list"),
                              ("--mbr", args.mbr, "reads the search's N-best list")):
            if on:
                raise ValueError("--keywords skips the search and prints keyword hits only, %s %s: use one of them" % (flag, why))
        if not 1 <= args.keyword_max_hits <= 8:
            raise ValueError("--keyword_max_hits must be in [1, 8] (got %d)" % args.keyword_max_hits)
        if np.isnan(args.keyword_threshold):
            raise ValueError("--keyword_threshold is not a number")
        args.hotwords, args.hotword_weight = "", 0.0              # (no search: nothing to bias)
        args.ngram_lm, args.ngram_weight = "", 0.0                # (... and nothing to fuse an LM into)
    if args.segment and args.align_text is not None:
        raise ValueError("--segment cuts the recordings, --align_text aligns one transcript per whole file: use one of them")
    if args.align_text is not None:
        args.timestamps = True
        args.hotwords, args.hotword_weight = "", 0.0              # (no search: nothing to bias)
        args.ngram_lm, args.ngram_weight = "", 0.0                # (... and nothing to fuse an LM into)
    ctc_only = False
    if args.decoder != "attention" or args.rescore != "none":          # (las.ctc_search is imported only when one of the flags is given)
        from las import ctc_search
        ctc_only = ctc_search.check_args(args) and args.align_text is None
    if args.timestamps and not args.ctc:
        raise ValueError("--timestamps needs the CTC head: decode with --ctc True (a model trained with --ctc)")
    consensus = bool(args.nbest or args.confidence or args.mbr or network)
    if consensus and args.align_text is not None:
        raise ValueError("--nbest / --confidence / --mbr%s read the search's N-best list, --align_text skips the search: use one of them"
                         % (" / --confusion_network" if network else ""))
    logging.basicConfig(stream=sys.stderr, format='%(asctime)s %(levelname)s:%(message)s', level=logging.INFO, datefmt='%I:%M:%S')
    if not args.synthetic and not args.audio:
        parser.error("no audio files (or --synthetic True)")
    if not args.cmvn:
        raise ValueError("the Listener takes the CMVN'd cube [T, feat_dim, 3]: transcribe with --cmvn True")
    tokenizer = CharEncoder() if args.unit.lower() == "char" else SubwordEncoder(args.subword_dir)
    args.vocab_size = tokenizer.get_vocab_size()
    id_to_token, token_to_id = tokenizer.id_to_token, tokenizer.token_to_id
    keywords = None
    if args.keywords is not None:                                      # (las.kws is imported only when the flag is given)
        from las import kws as KW
        keywords = KW.KeywordList.from_file(args.keywords, tokenizer, args.vocab_size)
    layers.set_cell(args.cell)
    layers.set_precision(args.dtype)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    variables.reset_default_store(device=dev, seed=args.seed)
    las = LAS(args, Listener, Speller, token_to_id)
    lm = result = None
    if args.apply_lm:
        st = variables.default_store()
        if args.synthetic and not os.path.exists(os.path.join(args.lm_dir, "result.json")):
            from lang.char_rnn_model import CharRNN
            lm = CharRNN(False, 1, 1, 28, 512, embedding_size=0, num_layers=2, store=st)
        else:
            lm, result = load_lm(args.lm_dir, st)
        lm.params()
    las.build_variables()
    bs = BeamSearch(args, las, token_to_id, lm)
    if not args.synthetic:
        logging.info("LAS restored: {}".format(bs.restore_las(None, args.save_dir, args.restore_epoch)))
        if result is not None:
            restore_lm(lm, result['best_model'])
    if args.timestamps:
        bs.need_ctc_head("--timestamps")                              # (a checkpoint without the head: refused before any audio is read)
    if keywords is not None:
        bs.need_ctc_head("--keywords")
    ann = None
    if consensus:                                                      # (las.nbest is imported only when one of its flags is given)
        from las import nbest as NB
        ann = NB.Annotator(args, bs.end_id, id_to_token)
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
        waves, rates = [w for w, _ in chunk], [fs for _, fs in chunk]
        if condition is None:
            return fe.extract(waves, rate=rates)
        plan = condition.fixed_plan(len(chunk), rir_idx=0 if args.rir_file else -1, noise_idx=0 if args.noise_file else -1, snr_db=args.snr_db)
        return fe.extract(waves, rate=rates, augment=plan)

    search = bs.ctc_decode_batches if ctc_only else bs.decode_batches  # --decoder: the CTC head alone, or the Speller's search
    if args.synthetic and not args.audio:
        count = args.max_steps if args.max_steps >= 0 else 8
        waves = synthetic_audio(count, args.sample_rate, args.seed + 2)
    else:
        waves = None
        count = len(args.audio)
    nb = max(1, int(args.decode_batch))
    texts = None
    if args.align_text is not None:
        with open(args.align_text) as f:
            texts = [line.strip() for line in f.read().splitlines()]
        if len(texts) != count:
            raise ValueError("--align_text %s holds %d lines for %d audio files" % (args.align_text, len(texts), count))
    durations = collections.deque()                                    # seconds per utterance, in the order of the results
    frame_s = A.frame_seconds(args, args.enc_type)

    def load(i):
        if waves is not None:
            return waves[i], args.sample_rate
        audio, fs = read_audio(args.audio[i])
        if audio.ndim != 1:
            raise ValueError("%s has %d channels: mono recordings only" % (args.audio[i], audio.shape[1]))
        return audio, int(fs)

    def batches():
        for c0 in range(0, count, nb):
            chunk = [load(i) for i in range(c0, min(c0 + nb, count))]          # (host work: file reads)
            durations.extend(len(w) / float(fs) for w, fs in chunk)

            def make(chunk=chunk):
                # called by decode_batches on the encoders' stream: one upload + three launches (one more per sample rate that is not
                # --sample_rate), the cube never leaves the device
                cube, lens = extract(chunk)
                return [(cube[u:u + 1, :lens[u]], lens[u:u + 1]) for u in range(len(chunk))]
            yield make

    def timed_lines(token_lists, scores, spans):
        for tokens, score, span in zip(token_lists, scores, spans):
            print(json.dumps({"text": convert_idx_to_string(tokens, id_to_token, args.unit),
                              "score": score if np.isfinite(score) else None,
                              "words": A.words(tokens, span, id_to_token, args.unit, frame_s, durations.popleft())}))

    if args.segment:
        return transcribe_segmented(args, bs, extract, VAD.VoiceActivity(args, device=dev), load, count, nb, id_to_token, frame_s, ann,
                                    search)
    if keywords is not None:
        # keyword search: the listener and the head, no search; one JSON object per file
        for make in batches():
            with torch.no_grad():
                encs, enc_lens, _, h_one, ctc_lp = bs._run_encoders(None, make())
            found = bs.keyword_search(encs, enc_lens, keywords, h_one=h_one, ctc_lp=ctc_lp, threshold_per_token=args.keyword_threshold,
                                      max_hits=args.keyword_max_hits)
            for hits in found.hits:
                print(json.dumps({"hits": KW.timed_hits(hits, keywords, frame_s, durations.popleft())}))
        sys.stdout.flush()
        return
    if texts is not None:
        # forced alignment: the listener and the head, no search
        done = 0
        for make in batches():
            with torch.no_grad():
                encs, enc_lens, _, h_one, ctc_lp = bs._run_encoders(None, make())
            token_lists = [tokenizer.encode(t, with_eos=True) for t in texts[done:done + len(encs)]]
            done += len(encs)
            timed_lines(token_lists, *bs.align(encs, enc_lens, token_lists, h_one=h_one, ctc_lp=ctc_lp))
        sys.stdout.flush()
        return
    bs.retain_align = bool(args.timestamps)
    for results in search(None, batches()):
        if ann is not None:
            for tokens, score, span, extra in annotated(args, bs, ann, results, id_to_token):
                print(json.dumps(json_fields(args, tokens, score, span, extra, id_to_token, frame_s, durations.popleft())))
            continue
        if args.timestamps:
            token_lists = [list(r[-1].token_ids[1:]) if r else [] for r in results]
            timed_lines(token_lists, *bs.align_results(results, token_lists))
            continue
        for beam_states in results:
            print(convert_idx_to_string(beam_states[-1].token_ids[1:], id_to_token, args.unit))
    sys.stdout.flush()


def transcribe_segmented(args, bs, extract, va, load, count, nb, id_to_token, frame_s, ann=None, search=None):
    """--segment: every file cut by las.vad at its own sample rate, the segments of all files as one stream through the front end and
    the search, nb at a time (a batch may span files and rates); one output line per file, in file order.  ann (--nbest / --confidence /
    --mbr): JSON lines; a file's confidence is the minimum over its segments, its words are concatenated, nbest stays per segment"""
    files = collections.deque()                                        # [segments (start s, end s) of a file, its results so far]

    def batches():
        chunk = []

        def flush():
            def make(chunk=chunk[:]):
                cube, lens = extract(chunk)
                return [(cube[u:u + 1, :lens[u]], lens[u:u + 1]) for u in range(len(chunk))]
            del chunk[:]
            return make

        for i in range(count):
            audio, fs = load(i)
            ranges = va.segments(audio, fs)                            # (one upload, one las_vad call, one wait per file)
            files.append(([(s0 / float(fs), s1 / float(fs)) for s0, s1 in ranges], []))
            for s0, s1 in ranges:
                chunk.append((audio[s0:s1], fs))
                if len(chunk) == nb:
                    yield flush()
        if chunk:
            yield flush()

    def emit_finished():
        while files and len(files[0][1]) == len(files[0][0]):
            spans, done = files.popleft()
            text = " ".join(d["text"] for d in done)
            if ann is not None:
                scores = [d["score"] for d in done]
                line = {"text": text, "score": None if any(x is None for x in scores) else float(sum(scores))}
                if ann.confidence:
                    conf = [d["confidence"] for d in done if d["confidence"] is not None]
                    line["confidence"] = min(conf) if conf else None
                if ann.confidence or args.timestamps:
                    line["words"] = [w for d in done for w in d["words"]]
                if ann.cn:                                             # a file's network: its segments' bins in order
                    line["network"] = [b for d in done for b in d["network"]]
                line["segments"] = done
                print(json.dumps(line))
                continue
            if not args.timestamps:
                print(text)
                continue
            scores = [d["score"] for d in done]
            print(json.dumps({"text": text, "score": None if any(x is None for x in scores) else float(sum(scores)),
                              "words": [w for d in done for w in d["words"]], "segments": done}))

    def take(tokens, score=None, span=None, extra=None):
        emit_finished()                                                # (silent files in front of this segment's file)
        spans, done = files[0]                                         # results arrive in stream order: the first unfinished file
        t0, t1 = spans[len(done)]
        d = {"text": convert_idx_to_string(tokens, id_to_token, args.unit)}
        if extra is not None:
            d = json_fields(args, tokens, score, span, extra, id_to_token, frame_s, t1 - t0)
            for w in d.get("words", []) if args.timestamps else []:    # file time, clipped to the segment's end
                if w["start"] is not None:
                    w["start"], w["end"] = min(t0 + w["start"], t1), min(t0 + w["end"], t1)
            d = dict([("start", t0), ("end", t1)] + list(d.items()))
        elif args.timestamps:
            ws = A.words(tokens, span, id_to_token, args.unit, frame_s, t1 - t0)
            for w in ws:                                               # file time, clipped to the segment's end
                if w["start"] is not None:
                    w["start"], w["end"] = min(t0 + w["start"], t1), min(t0 + w["end"], t1)
            d = {"start": t0, "end": t1, "text": d["text"], "score": score if np.isfinite(score) else None, "words": ws}
        done.append(d)
        emit_finished()

    bs.retain_align = bool(args.timestamps)
    for results in (search or bs.decode_batches)(None, batches()):
        if ann is not None:
            for tokens, score, span, extra in annotated(args, bs, ann, results, id_to_token):
                take(tokens, score, span, extra)
            continue
        token_lists = [list(r[-1].token_ids[1:]) if r else [] for r in results]
        if args.timestamps:
            for tokens, score, span in zip(token_lists, *bs.align_results(results, token_lists)):
                take(tokens, score, span)
        else:
            for tokens in token_lists:
                take(tokens)
    emit_finished()                                                    # (trailing silent files; no file at all is left unfinished)
    assert not files
    sys.stdout.flush()


if __name__ == "__main__":
    main()
