"""transcribe.py's host side without a GPU: the records and file lines of las.transcript on hand-made search results, and
the flag check of las.cli.  Every expected string was printed by the entry point as it was before the two modules existed, from the
same fakes (its json_fields / annotated / timed_lines / transcribe_segmented, its main for the refusals): the bytes of the output and
the refusal a combination of flags gets are the contract.  Strings are compared as json.dumps wrote them, so the key order is held."""
import argparse
import json

import numpy as np
import pytest

import helpers  # noqa: F401
from las import cli
from las import transcript as T
from utils.tokenizer import CharEncoder

ENC = CharEncoder()
ID = ENC.id_to_token
FRAME_S = 0.04
INF = float("inf")


class State(object):
    def __init__(self, text, log_prob):
        self.token_ids, self.log_prob = [1] + ENC.encode(text, with_eos=True), log_prob


class Results(list):
    """a search's result list: per utterance its hypotheses, best last; --rescore attention adds .rescored"""


class StubSearch(object):
    """of BeamSearch what the output reads: align_results hands out prepared (scores, spans), one pair per batch, and keeps the
    token lists it was asked to align"""

    def __init__(self, *aligned):
        self.aligned, self.asked, self.retain_align = list(aligned), [], False

    def align_results(self, results, token_lists):
        self.asked.append(token_lists)
        return self.aligned.pop(0)


class StubAnnotator(object):
    """las.nbest.Annotator's flags, and prepared notes per batch"""

    def __init__(self, notes, nbest=0, confidence=False, cn=False, cn_decode=False):
        self.notes, self.nbest, self.confidence, self.cn, self.cn_decode = list(notes), nbest, confidence, cn, cn_decode

    def annotate(self, results):
        return self.notes.pop(0)


def note(state, posterior=None, conf=(), nbest=(), **more):
    tokens = list(state.token_ids[1:]) if state is not None else []
    return dict(dict(index=0 if state is not None else -1, state=state, tokens=tokens, posterior=posterior, conf=list(conf),
                     nbest=list(nbest)), **more)


def spans_of(text, first=0, gap=1):
    """frame spans of text's tokens and its <EOS>: token k takes frames first + k (gap + 1) .. + gap"""
    return [(first + k * (gap + 1), first + k * (gap + 1) + gap) for k in range(len(text) + 1)]


HI, AB = State("HI YO", -0.5), State("AB", -1.25)
UNALIGNED = [(-1, -1)] * 6
NETWORK = [[{"word": "HI", "p": 0.75}, {"word": "", "p": 0.25}], [{"word": "YO", "p": 0.5}, {"word": "YOU", "p": 0.5}]]
NBEST = [(HI.token_ids[1:], -0.5, 0.625), (AB.token_ids[1:], -INF, 0.375)]


def record_cases():
    """name -> (args.timestamps, StubSearch, StubAnnotator or None, results, durations)"""
    rescored = Results([[AB, HI]])
    rescored.rescored = [[dict(first=-2.5, att=-INF), dict(first=-1.5, att=-0.75)]]     # (ascending, as the results)
    consensus = dict(words=["HI", "YOU"], conf=[0.75, 0.5], tokens=[], text="HI YOU")
    return {
        "plain": (False, StubSearch(), None, Results([[AB, HI], []]), [0.37, 1.0]),
        "timestamps": (True, StubSearch(([-3.25], [spans_of("HI YO")])), None, Results([[AB, HI]]), [0.37]),
        "unalignable": (True, StubSearch(([-INF], [UNALIGNED])), None, Results([[AB, HI]]), [0.37]),
        "confidence": (False, StubSearch(), StubAnnotator([[note(HI, 0.625, [0.9, 0.8, 1.0, 0.7, 0.6, 1.0])]], confidence=True),
                       Results([[AB, HI]]), [0.37]),
        "confidence_timestamps": (True, StubSearch(([-3.25], [spans_of("HI YO")])),
                                  StubAnnotator([[note(HI, 0.625, [0.9, 0.8, 1.0, 0.7, 0.6, 1.0])]], confidence=True),
                                  Results([[AB, HI]]), [0.37]),
        "nbest_rescored": (False, StubSearch(), StubAnnotator([[note(HI, 0.625, nbest=NBEST)]], nbest=2), rescored, [0.37]),
        "nbest": (False, StubSearch(), StubAnnotator([[note(HI, 0.625, nbest=NBEST)]], nbest=2), Results([[AB, HI]]), [0.37]),
        "network": (False, StubSearch(), StubAnnotator([[note(HI, 0.625, network=NETWORK)]], cn=True), Results([[AB, HI]]), [0.37]),
        "consensus": (False, StubSearch(),
                      StubAnnotator([[note(HI, 0.625, network=NETWORK, consensus=consensus),
                                      note(AB, 1.0, network=[], consensus=dict(words=[], conf=[], tokens=[], text=""))]],
                                    confidence=True, cn=True, cn_decode=True), Results([[AB, HI], [AB]]), [0.37, 1.0]),
        "nothing_found": (False, StubSearch(), StubAnnotator([[note(None)]], nbest=2, confidence=True), Results([[]]), [0.37]),
    }


# (plain, second utterance: the search returned nothing -- an empty line, as every other mode prints; the entry point of before raised
# IndexError there)
RECORDS = {'confidence': ['{"text": "HI YO", "score": -0.5, "confidence": 0.625, "words": [{"word": "HI", "confidence": 0.8}, {"word": "YO", "confidence": '
                '0.6}]}'],
 'confidence_timestamps': ['{"text": "HI YO", "score": -3.25, "confidence": 0.625, "words": [{"word": "HI", "start": 0.0, "end": 0.16, '
                           '"confidence": 0.8}, {"word": "YO", "start": 0.24, "end": 0.37, "confidence": 0.6}]}'],
 'consensus': ['{"text": "HI YOU", "score": null, "confidence": 0.5, "words": [{"word": "HI", "confidence": 0.75}, {"word": "YOU", "confidence": '
               '0.5}], "network": [[{"word": "HI", "p": 0.75}, {"word": "", "p": 0.25}], [{"word": "YO", "p": 0.5}, {"word": "YOU", "p": 0.5}]]}',
               '{"text": "", "score": null, "confidence": null, "words": [], "network": []}'],
 'nbest': ['{"text": "HI YO", "score": -0.5, "nbest": [{"text": "HI YO", "score": -0.5, "posterior": 0.625}, {"text": "AB", "score": null, '
           '"posterior": 0.375}]}'],
 'nbest_rescored': ['{"text": "HI YO", "score": -0.5, "nbest": [{"text": "HI YO", "score": -0.5, "posterior": 0.625, "ctc_score": -1.5, '
                    '"att_score": -0.75}, {"text": "AB", "score": null, "posterior": 0.375, "ctc_score": -2.5, "att_score": null}]}'],
 'network': ['{"text": "HI YO", "score": -0.5, "network": [[{"word": "HI", "p": 0.75}, {"word": "", "p": 0.25}], [{"word": "YO", "p": 0.5}, '
             '{"word": "YOU", "p": 0.5}]]}'],
 'nothing_found': ['{"text": "", "score": null, "confidence": null, "words": [], "nbest": []}'],
 'plain': ['HI YO', ''],
 'timestamps': ['{"text": "HI YO", "score": -3.25, "words": [{"word": "HI", "start": 0.0, "end": 0.16}, {"word": "YO", "start": 0.24, "end": '
                '0.37}]}'],
 'unalignable': ['{"text": "HI YO", "score": null, "words": [{"word": "HI", "start": null, "end": null}, {"word": "YO", "start": null, "end": '
                 'null}]}']}


def lines_of(case):
    timestamps, bs, ann, results, durations = case
    args = argparse.Namespace(unit="char", timestamps=timestamps)
    out = []
    for rec, duration in zip(T.choose(args, bs, ann, results, ID), durations):
        d = T.record(args, ID, FRAME_S, *rec, duration)
        out.append(d["text"] if ann is None and not timestamps else json.dumps(d))
    return out


@pytest.mark.parametrize("name", sorted(RECORDS))
def test_records(name):
    assert lines_of(record_cases()[name]) == RECORDS[name]


def test_record_cases_are_all_pinned():
    assert sorted(RECORDS) == sorted(record_cases())


# ---- --segment: five files, the first, the third and the last silent -------------------------------------------------------------------
RATES = [16000, 8000, 16000, 8000, 16000]
RANGES = [[], [(1234, 20000), (24000, 30001)], [], [(800, 4000)], []]


class StubVad(object):
    def __init__(self):
        self.left = [list(r) for r in RANGES]

    def segments(self, audio, fs):
        return self.left.pop(0)


def segment_cases():
    """name -> (args.timestamps, StubSearch, StubAnnotator or None, the results of the two batches).  Segment 1 of file 1 is unalignable
    (timestamps) or has no hypothesis (annotated); the words of segment 0 of file 1 reach past its end: frames 290 .. at 0.04 s"""
    late = [(0, 1), (2, 2), (3, 3), (290, 291), (292, 300), (301, 301)]
    batches = [Results([[AB, HI], [HI]]), Results([[AB]])]
    return {
        "plain": (False, StubSearch(), None, batches),
        "timestamps": (True, StubSearch(([-3.25, -INF], [late, UNALIGNED]), ([-1.5], [spans_of("AB", 2)])), None, batches),
        "annotated": (True, StubSearch(([-3.25, -INF], [late, []]), ([-1.5], [spans_of("AB", 2)])),
                      StubAnnotator([[note(HI, 0.625, [0.9, 0.8, 1.0, 0.7, 0.6, 1.0], network=NETWORK), note(None, network=[])],
                                     [note(AB, 0.875, [0.5, 0.25, 1.0], network=NETWORK[:1])]], confidence=True, cn=True),
                      [Results([[AB, HI], []]), Results([[AB]])]),
    }


SEGMENTS = {'annotated': ['{"text": "", "score": 0.0, "confidence": null, "words": [], "network": [], "segments": []}',
               '{"text": "HI YO ", "score": null, "confidence": 0.625, "words": [{"word": "HI", "start": 0.15425, "end": 0.27425, "confidence": '
               '0.8}, {"word": "YO", "start": 2.5, "end": 2.5, "confidence": 0.6}], "network": [[{"word": "HI", "p": 0.75}, {"word": "", "p": '
               '0.25}], [{"word": "YO", "p": 0.5}, {"word": "YOU", "p": 0.5}]], "segments": [{"start": 0.15425, "end": 2.5, "text": "HI YO", '
               '"score": -3.25, "confidence": 0.625, "words": [{"word": "HI", "start": 0.15425, "end": 0.27425, "confidence": 0.8}, {"word": "YO", '
               '"start": 2.5, "end": 2.5, "confidence": 0.6}], "network": [[{"word": "HI", "p": 0.75}, {"word": "", "p": 0.25}], [{"word": "YO", '
               '"p": 0.5}, {"word": "YOU", "p": 0.5}]]}, {"start": 3.0, "end": 3.750125, "text": "", "score": null, "confidence": null, "words": '
               '[], "network": []}]}',
               '{"text": "", "score": 0.0, "confidence": null, "words": [], "network": [], "segments": []}',
               '{"text": "AB", "score": -1.5, "confidence": 0.875, "words": [{"word": "AB", "start": 0.18, "end": 0.33999999999999997, '
               '"confidence": 0.25}], "network": [[{"word": "HI", "p": 0.75}, {"word": "", "p": 0.25}]], "segments": [{"start": 0.1, "end": 0.5, '
               '"text": "AB", "score": -1.5, "confidence": 0.875, "words": [{"word": "AB", "start": 0.18, "end": 0.33999999999999997, '
               '"confidence": 0.25}], "network": [[{"word": "HI", "p": 0.75}, {"word": "", "p": 0.25}]]}]}',
               '{"text": "", "score": 0.0, "confidence": null, "words": [], "network": [], "segments": []}'],
 'plain': ['', 'HI YO HI YO', '', 'AB', ''],
 'timestamps': ['{"text": "", "score": 0.0, "words": [], "segments": []}',
                '{"text": "HI YO HI YO", "score": null, "words": [{"word": "HI", "start": 0.15425, "end": 0.27425}, {"word": "YO", "start": 2.5, '
                '"end": 2.5}, {"word": "HI", "start": null, "end": null}, {"word": "YO", "start": null, "end": null}], "segments": [{"start": '
                '0.15425, "end": 2.5, "text": "HI YO", "score": -3.25, "words": [{"word": "HI", "start": 0.15425, "end": 0.27425}, {"word": "YO", '
                '"start": 2.5, "end": 2.5}]}, {"start": 3.0, "end": 3.750125, "text": "HI YO", "score": null, "words": [{"word": "HI", "start": '
                'null, "end": null}, {"word": "YO", "start": null, "end": null}]}]}',
                '{"text": "", "score": 0.0, "words": [], "segments": []}',
                '{"text": "AB", "score": -1.5, "words": [{"word": "AB", "start": 0.18, "end": 0.33999999999999997}], "segments": [{"start": 0.1, '
                '"end": 0.5, "text": "AB", "score": -1.5, "words": [{"word": "AB", "start": 0.18, "end": 0.33999999999999997}]}]}',
                '{"text": "", "score": 0.0, "words": [], "segments": []}']}


def fake_search(per_batch):
    def search(sess, batches):
        for make, results in zip(batches, per_batch):                  # (zip asks `batches` first: as decode_batches, it drains them)
            yield results
    return search


def segmented_lines(case, capsys):
    timestamps, bs, ann, per_batch = case
    args = argparse.Namespace(unit="char", timestamps=timestamps)
    files = T.FileAssembler(lambda *a: T.record(args, ID, FRAME_S, *a), timestamps or ann is not None, timestamps,
                            ann is not None and ann.confidence, ann is not None and ann.cn)
    va = StubVad()
    load = lambda i: (np.zeros(40000, np.float32), RATES[i])
    batches = T.batches(load, len(RATES), 2, None, lambda audio, fs: files.add_file(va.segments(audio, fs), fs))
    T.run(fake_search(per_batch), batches, lambda results: T.choose(args, bs, ann, results, ID), files.take)
    files.emit_finished()
    assert not files.files                                             # nothing is left in the deque
    return capsys.readouterr().out.splitlines()


@pytest.mark.parametrize("name", sorted(SEGMENTS))
def test_file_lines(name, capsys):
    assert segmented_lines(segment_cases()[name], capsys) == SEGMENTS[name]


def test_file_lines_clip_sum_and_minimum(capsys):
    """what the pinned strings hold, said once: a word behind its segment's end is clipped to it, one null score makes the file's
    null, the file's confidence is the least of the segments that have one"""
    lines = [json.loads(ln) for ln in segmented_lines(segment_cases()["annotated"], capsys)]
    assert [ln["text"] for ln in lines] == ["", "HI YO ", "", "AB", ""] and sorted(SEGMENTS) == sorted(segment_cases())
    seg = lines[1]["segments"][0]
    assert seg["words"][1]["start"] == seg["words"][1]["end"] == seg["end"] == 20000 / 8000.0
    assert lines[1]["score"] is None and lines[3]["score"] == -1.5
    assert lines[1]["segments"][1]["confidence"] is None and lines[1]["confidence"] == 0.625 and lines[0]["confidence"] is None


def test_batches_cut_the_stream_in_order():
    chunks = []
    makes = list(T.batches(lambda i: (np.arange(10) + 100 * i, 8000 + i), 3, 2, lambda chunk: chunks.append(chunk),
                           lambda audio, fs: [(0, 4), (6, 10)] if fs != 8001 else []))
    assert len(makes) == 2 and not chunks                              # (nothing is extracted before the search asks)
    for make in makes:
        with pytest.raises(TypeError):                                 # (the stub returns no cube)
            make()
    got = [[(list(w), fs) for w, fs in chunk] for chunk in chunks]
    assert got == [[([0, 1, 2, 3], 8000), ([6, 7, 8, 9], 8000)], [([200, 201, 202, 203], 8002), ([206, 207, 208, 209], 8002)]]


# ---- the flags: which refusal a combination gets ---------------------------------------------------------------------------------------
KW = ["--ctc", "True", "--keywords", "k.txt", "a.wav"]
ALIGN = ["--ctc", "True", "--align_text", "refs.txt", "a.wav"]
REFUSALS = [(['--ctc', 'True', '--keywords', 'k.txt', 'a.wav', '--align_text', 'refs.txt'],
  '--keywords skips the search and prints keyword hits only, --align_text aligns a given transcript: use one of them'),
 (['--ctc', 'True', '--keywords', 'k.txt', 'a.wav', '--segment', 'True'],
  '--keywords skips the search and prints keyword hits only, --segment cuts the recordings first; searching the segments is not built: use one of '
  'them'),
 (['--ctc', 'True', '--keywords', 'k.txt', 'a.wav', '--timestamps', 'True'],
  "--keywords skips the search and prints keyword hits only, --timestamps times the search's hypothesis: use one of them"),
 (['--ctc', 'True', '--keywords', 'k.txt', 'a.wav', '--nbest', '2'],
  "--keywords skips the search and prints keyword hits only, --nbest reads the search's N-best list: use one of them"),
 (['--ctc', 'True', '--keywords', 'k.txt', 'a.wav', '--confidence', 'True'],
  "--keywords skips the search and prints keyword hits only, --confidence reads the search's N-best list: use one of them"),
 (['--ctc', 'True', '--keywords', 'k.txt', 'a.wav', '--mbr', 'True'],
  "--keywords skips the search and prints keyword hits only, --mbr reads the search's N-best list: use one of them"),
 (['--ctc', 'True', '--keywords', 'k.txt', 'a.wav', '--keyword_max_hits', '0'], '--keyword_max_hits must be in [1, 8] (got 0)'),
 (['--ctc', 'True', '--keywords', 'k.txt', 'a.wav', '--keyword_max_hits', '9'], '--keyword_max_hits must be in [1, 8] (got 9)'),
 (['--ctc', 'True', '--keywords', 'k.txt', 'a.wav', '--keyword_threshold', 'nan'], '--keyword_threshold is not a number'),
 (['--ctc', 'True', '--keywords', 'k.txt', 'a.wav', '--confusion_network', 'True'],
  "--keywords skips the search and prints keyword hits only, --confusion_network / --cn_decode read the search's N-best list: use one of them"),
 (['--ctc', 'True', '--keywords', 'k.txt', 'a.wav', '--cn_decode', 'True'],
  "--keywords skips the search and prints keyword hits only, --confusion_network / --cn_decode read the search's N-best list: use one of them"),
 (['--keywords', 'k.txt', 'a.wav'], '--keywords needs the CTC head: decode with --ctc True (a model trained with --ctc)'),
 (['--ctc', 'True', '--segment', 'True', '--align_text', 'refs.txt', 'a.wav'],
  '--segment cuts the recordings, --align_text aligns one transcript per whole file: use one of them'),
 (['--timestamps', 'True', 'a.wav'], '--timestamps needs the CTC head: decode with --ctc True (a model trained with --ctc)'),
 (['--ctc', 'True', '--align_text', 'refs.txt', 'a.wav', '--nbest', '2'],
  "--nbest / --confidence / --mbr read the search's N-best list, --align_text skips the search: use one of them"),
 (['--ctc', 'True', '--align_text', 'refs.txt', 'a.wav', '--confidence', 'True'],
  "--nbest / --confidence / --mbr read the search's N-best list, --align_text skips the search: use one of them"),
 (['--ctc', 'True', '--align_text', 'refs.txt', 'a.wav', '--mbr', 'True'],
  "--nbest / --confidence / --mbr read the search's N-best list, --align_text skips the search: use one of them"),
 (['--ctc', 'True', '--align_text', 'refs.txt', 'a.wav', '--confusion_network', 'True'],
  "--nbest / --confidence / --mbr / --confusion_network read the search's N-best list, --align_text skips the search: use one of them"),
 (['--ctc', 'True', '--align_text', 'refs.txt', 'a.wav', '--cn_decode', 'True'],
  '--cn_decode prints a hypothesis no search produced; aligning it (--timestamps / --align_text) is not built'),
 (['--cn_decode', 'True', '--mbr', 'True', 'a.wav'],
  "--cn_decode prints the network's consensus, --mbr the listed hypothesis of least risk: use one of them"),
 (['--ctc', 'True', '--cn_decode', 'True', '--timestamps', 'True', 'a.wav'],
  '--cn_decode prints a hypothesis no search produced; aligning it (--timestamps / --align_text) is not built'),
 (['--confusion_network', 'True', '--cn_alternatives', '9', 'a.wav'], '--cn_alternatives must be in [1, 8] (got 9)'),
 (['--rescore', 'attention', 'a.wav'], "--rescore attention re-ranks the CTC search's N-best list: it needs --decoder ctc"),
 (['--decoder', 'ctc', 'a.wav'], '--decoder ctc needs the CTC head: decode with --ctc True (a model trained with --ctc)'),
 (['--cmvn', 'False', 'a.wav'], "the Listener takes the CMVN'd cube [T, feat_dim, 3]: transcribe with --cmvn True"),
 ([], 'error: no audio files (or --synthetic True)'),
 (['--ctc', 'True', '--keywords', 'k.txt', 'a.wav', '--segment', 'True', '--align_text', 'refs.txt'],
  '--keywords skips the search and prints keyword hits only, --align_text aligns a given transcript: use one of them'),
 (['--keywords', 'k.txt', '--timestamps', 'True', 'a.wav'], '--keywords needs the CTC head: decode with --ctc True (a model trained with --ctc)'),
 (['--segment', 'True', '--align_text', 'refs.txt', '--decoder', 'ctc', 'a.wav'],
  '--segment cuts the recordings, --align_text aligns one transcript per whole file: use one of them'),
 (['--align_text', 'refs.txt', '--nbest', '2', 'a.wav'], '--timestamps needs the CTC head: decode with --ctc True (a model trained with --ctc)'),
 (['--ctc', 'True', '--align_text', 'refs.txt', 'a.wav', '--nbest', '2', '--decoder', 'ctc', '--apply_lm', 'True'],
  "--decoder ctc: --apply_lm fuses the RNN LM into the Speller's search; the CTC search takes --ngram_lm"),
 (['--cmvn', 'False'], 'error: no audio files (or --synthetic True)'),
 (['--ctc', 'True', '--keywords', 'k.txt', 'a.wav', '--cn_decode', 'True', '--mbr', 'True'],
  "--keywords skips the search and prints keyword hits only, --confusion_network / --cn_decode read the search's N-best list: use one of them"),
 (['--ctc', 'True', '--keywords', 'k.txt', 'a.wav', '--keyword_max_hits', '0', '--nbest', '2'],
  "--keywords skips the search and prints keyword hits only, --nbest reads the search's N-best list: use one of them"),
 (['--timestamps', 'True', '--cmvn', 'False', 'a.wav'], '--timestamps needs the CTC head: decode with --ctc True (a model trained with --ctc)'),
 (['--ctc', 'True', '--keywords', 'k.txt', 'a.wav', '--keyword_threshold', 'nan', '--decoder', 'ctc', '--apply_lm', 'True'],
  '--keyword_threshold is not a number'),
 (['--ctc', 'True', '--align_text', 'refs.txt', 'a.wav', '--confusion_network', 'True', '--nbest', '2', '--segment', 'True'],
  '--segment cuts the recordings, --align_text aligns one transcript per whole file: use one of them'),
 (['--ctc', 'True', '--timestamps', 'True', '--rescore', 'attention'],
  "--rescore attention re-ranks the CTC search's N-best list: it needs --decoder ctc")]


@pytest.mark.parametrize("argv,message", REFUSALS, ids=[" ".join(a) for a, _ in REFUSALS])
def test_refusals(argv, message, capsys):
    import transcribe
    if message.startswith("error:"):                                   # (the parser's own: usage on stderr, exit status 2)
        with pytest.raises(SystemExit):
            transcribe.main(argv)
        assert capsys.readouterr().err.rstrip().endswith(message)
        return
    with pytest.raises(ValueError) as e:
        transcribe.main(argv)
    assert str(e.value) == message


def _mode(argv):
    import transcribe
    from las import vad
    parser = transcribe.build_parser()
    cli.add_flags(parser)
    vad.add_flags(parser, cli.str2bool)
    args = parser.parse_args(argv)
    return cli.check_flags(args, parser), args


def test_mode_record():
    biased = ["--hotwords", "names.txt", "--hotword_weight", "2.0", "--ngram_lm", "lm.arpa", "--ngram_weight", "0.5"]
    mode, args = _mode(["a.wav"] + biased)
    assert mode == cli.Mode(kind="search", ctc_only=False, annotate=False, json=False)
    assert (args.hotwords, args.hotword_weight, args.ngram_lm, args.ngram_weight, args.timestamps) == ("names.txt", 2.0, "lm.arpa", 0.5, False)
    mode, args = _mode(ALIGN + biased + ["--decoder", "ctc", "--beam_size", "4"])
    assert mode == cli.Mode(kind="align", ctc_only=False, annotate=False, json=True) and args.timestamps is True
    assert (args.hotwords, args.hotword_weight, args.ngram_lm, args.ngram_weight) == ("", 0.0, "", 0.0)
    mode, args = _mode(KW + biased)
    assert mode == cli.Mode(kind="keywords", ctc_only=False, annotate=False, json=True) and args.timestamps is False
    assert (args.hotwords, args.hotword_weight, args.ngram_lm, args.ngram_weight) == ("", 0.0, "", 0.0)
    assert _mode(["a.wav", "--ctc", "True", "--decoder", "ctc", "--beam_size", "4"])[0] == cli.Mode("search", True, False, False)
    assert _mode(["a.wav", "--ctc", "True", "--timestamps", "True"])[0] == cli.Mode("search", False, False, True)
    assert _mode(["a.wav", "--nbest", "2"])[0] == cli.Mode("search", False, True, True)
    assert _mode(["a.wav", "--confusion_network", "True"])[0] == cli.Mode("search", False, True, True)
