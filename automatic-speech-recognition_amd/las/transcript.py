"""las.transcript -- what transcribe.py prints, as host code (no device, no model): `choose` turns a batch of search results into (tokens,
score, span, extra) per utterance, `record` one of them into the JSON object of an utterance or segment, `FileAssembler` the segments of
--segment into one line per file; `batches` and `run` are the stream in and the loop over the results.  Key order is contract."""
import collections
import json

import numpy as np

from las import align as A
from las.utils import convert_idx_to_string


def choose(args, bs, ann, results, id_to_token):
    """a batch of results -> per utterance (tokens of the hypothesis to print, its score, its frame spans or None, the extra JSON fields).
    Without an Annotator: the best hypothesis (none: the empty text), aligned under --timestamps (extra = {}), else extra = None: plain text.
    With one: one consensus call for the batch and, with --timestamps, one alignment of the chosen; score = the alignment's, else the search's."""
    if ann is None:
        token_lists = [list(r[-1].token_ids[1:]) if r else [] for r in results]
        cov = [_coverage_fields(r[-1] if r else None) for r in results]          # ({} unless the coverage scorer ran)
        if not args.timestamps:
            if getattr(args, "coverage_report", False) or getattr(args, "diarize", False):   # JSON lines: the search's score [and the two shares]
                return [(tokens, float(r[-1].log_prob) if r else None, None, c) for tokens, r, c in zip(token_lists, results, cov)]
            return [(tokens, None, None, None) for tokens in token_lists]
        return [(tokens, score, span, c) for tokens, score, span, c in zip(token_lists, *bs.align_results(results, token_lists), cov)]
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
        extra = {} if ann.cn_decode else _coverage_fields(a["state"])  # (the consensus is a text no search produced: no coverage)
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
            for j, e in enumerate(extra["nbest"]):                     # (the list is best first, the results ascend)
                e.update(_coverage_fields(results[u][len(results[u]) - 1 - j] if j < len(results[u]) else None))
            if rescored is not None:
                for j, e in enumerate(extra["nbest"]):                 # (the list is best first, the results ascend)
                    d = rescored[u][len(rescored[u]) - 1 - j]
                    e["ctc_score"], e["att_score"] = (x if np.isfinite(x) else None for x in (d["first"], d["att"]))
        out.append((tokens, score, span, extra))
    return out


def _coverage_fields(state):
    """{"coverage", "overattended"} of a hypothesis the coverage scorer counted, else {}"""
    cov = getattr(state, "coverage", None)
    if cov is None:
        return {}
    from las import coverage
    return coverage.fields(cov)


def record(args, id_to_token, frame_s, tokens, score, span, extra, duration, segment=None):
    """the object of one utterance, or of the segment (start s, end s) of a file: [start, end], text, score, [coverage, overattended],
    [confidence], [words], [nbest], [network].  A segment's word times are shifted into file time and clipped to its end.  extra None: the text alone"""
    text = convert_idx_to_string(tokens, id_to_token, args.unit)
    if extra is None:
        return {"text": text}
    d = {} if segment is None else {"start": segment[0], "end": segment[1]}
    d["text"], d["score"] = text, score if score is not None and np.isfinite(score) else None
    for k in ("coverage", "overattended"):
        if k in extra:
            d[k] = extra[k]
    words = A.words(tokens, span, id_to_token, args.unit, frame_s, duration) if span is not None else None
    for w in words if words is not None and segment is not None else []:
        if w["start"] is not None:
            w["start"], w["end"] = min(segment[0] + w["start"], segment[1]), min(segment[0] + w["end"], segment[1])
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


class FileAssembler(object):
    """--segment: one output line per file, in file order, from the records of its segments as they arrive in stream order.
    make(tokens, score, span, extra, duration, segment) is `record` with its first arguments bound."""

    def __init__(self, make, as_json, words=False, confidence=False, network=False):
        self.make, self.as_json, self.words, self.confidence, self.network = make, as_json, words or confidence, confidence, network
        self.files = collections.deque()                               # [segments (start s, end s) of a file, its records so far, speakers]

    def add_file(self, ranges, fs, speakers=None):                     # (sample ranges at fs Hz; before their results arrive; -> ranges)
        """speakers (--diarize): (the 1-based speaker of every range, the file's number of speakers) -- every segment record and
        every word object then carry "speaker", the file's line "speakers" """
        self.files.append(([(s0 / float(fs), s1 / float(fs)) for s0, s1 in ranges], [], speakers))
        return ranges

    def take(self, tokens, score, span, extra):
        self.emit_finished()                                           # (silent files in front of this segment's file)
        spans, done, speakers = self.files[0]                          # results arrive in stream order: the first unfinished file
        t0, t1 = spans[len(done)]
        d = self.make(tokens, score, span, extra, t1 - t0, (t0, t1))
        if speakers is not None:
            d["speaker"] = speakers[0][len(done)]
            for w in d.get("words", []):
                w["speaker"] = d["speaker"]
        done.append(d)
        self.emit_finished()

    def emit_finished(self):
        """a finished file's line: the texts joined by one space; as JSON the summed score (None if one is None), [the least
        confidence], [the words], [the network's bins] in order, and the segments' own records"""
        while self.files and len(self.files[0][1]) == len(self.files[0][0]):
            spans, done, speakers = self.files.popleft()
            text = " ".join(d["text"] for d in done)
            if not self.as_json:
                print(text)
                continue
            scores = [d["score"] for d in done]
            line = {"text": text, "score": None if any(x is None for x in scores) else float(sum(scores))}
            if self.confidence:
                conf = [d["confidence"] for d in done if d["confidence"] is not None]
                line["confidence"] = min(conf) if conf else None
            if self.words:
                line["words"] = [w for d in done for w in d["words"]]
            if self.network:
                line["network"] = [b for d in done for b in d["network"]]
            if speakers is not None:
                line["speakers"] = speakers[1]
            line["segments"] = done
            print(json.dumps(line))


def batches(load, count, nb, extract, cut):
    """the utterances, nb at a time: of file i, load(i) -> (audio, fs), the sample ranges cut(audio, fs) in order (a batch may span files and
    rates).  decode_batches makes a batch on the encoders' stream: one upload + three launches (one more per other sample rate), all on the device"""
    def deferred(chunk):
        def make():
            cube, lens = extract(chunk)
            return [(cube[u:u + 1, :lens[u]], lens[u:u + 1]) for u in range(len(chunk))]
        return make

    chunk = []
    for i in range(count):
        audio, fs = load(i)                                            # (host work: file reads)
        for s0, s1 in cut(audio, fs):
            chunk.append((audio[s0:s1], fs))
            if len(chunk) == nb:
                yield deferred(chunk)
                chunk = []
    if chunk:
        yield deferred(chunk)


def run(search, batches, chooser, sink):
    """the result loop of every searching mode: sink(tokens, score, span, extra) per utterance, in stream order"""
    for results in search(None, batches):
        for rec in chooser(results):
            sink(*rec)
