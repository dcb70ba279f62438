"""Attention coverage without a GPU: properties of the numpy restatement (tests/coverage_ref.py), the flag refusals, the
JSON fields of las.transcript, and header / binding / version in step."""
import argparse
import json
import os
import re

import numpy as np
import pytest

import coverage_ref as CR
import helpers
from helpers import PKG, ROOT, _oracle_fns, make_args, synthetic_batch

EOS = 2


# ---- 1. the reference -----------------------------------------------------------------------------------------------------------------
def test_reference_counts_are_monotone_and_ordered():
    """non-negative alignments: covered and over never fall, covered <= frames, over <= covered; frames >= enc_len and NaNs never count"""
    rng = np.random.RandomState(3)
    for Tp, L in ((1, 1), (7, 5), (64, 64), (65, 0), (130, 129)):
        st, prev = CR.empty_state(Tp), (0, 0)
        for t in range(40):
            a = rng.rand(Tp).astype(np.float32)
            a /= max(a.sum(), 1e-6) / 3.0                              # (peaked enough to cross both thresholds within the steps)
            st, dc, do = CR.advance(st, a, L, 0.5, 1.5)
            c, o = int(st[1]), int(st[2])
            assert c >= prev[0] and o >= prev[1] and dc == c - prev[0] and do == o - prev[1]
            assert o <= c <= L
            prev = (c, o)
        assert (prev[0] > 0) == (L > 0)                                # (... and the run did count something where it could)
    st, _, _ = CR.advance(CR.empty_state(4), np.array([np.nan, np.inf, 2.0, 2.0], np.float32), 3, 0.5, 1.5)
    assert (int(st[1]), int(st[2])) == (2, 2)                          # NaN: no; inf: both; the frame behind enc_len: no
    assert CR.counts([np.full(4, 0.3), np.full(4, 0.3)], 9, 0.5, 1.5) == (4, 0)       # enc_len is clamped to Tp


def test_reference_gain_rounds_each_product_then_the_difference():
    f = np.float32
    g = CR.gain(0.3, 0.7, f(5), f(3))
    assert g == f(f(f(0.3) * f(5)) - f(f(0.7) * f(3))) and g.dtype == np.float32
    assert CR.gain(0.0, 0.0, f(5), f(3)) == 0


def _small_model(V=30):
    from oracle import las_oracle as O
    args = make_args(enc_units=16, num_enc_layers=2, dec_units=16, num_dec_layers=1, embedding_size=8, attention_size=8, beam_size=4,
                     convert_rate=0.3, apply_lm=False, vocab_size=V)
    p0 = O.init_params(args, seed=11, cell="lstm")
    p0["Speller/decode/dense/bias"][2] = 0.3                            # let some hypotheses end
    return args, p0


def test_zero_weights_give_the_oracles_search_exactly():
    """... and weights change it; every returned hypothesis' state holds the counts of its own alignments"""
    from oracle import las_oracle as O
    args, p0 = _small_model()
    differs = 0
    for k, T in enumerate((64, 48)):
        xs = synthetic_batch(1, T, 12, 30, seed=8 + k)[0]
        step_fn, _, _, init, Tp, dec_step = _oracle_fns(xs, p0, args, "lstm", None)
        want = O.beam_search(step_fn, init, Tp, dec_step, 4, 1, EOS)
        got, _ = CR.covered_beam_search(step_fn, init, Tp, dec_step, 4, 1, EOS, Tp, 0.0, 0.0, 0.5, 1.5)
        assert [(h.token_ids, h.log_prob) for h in got] == [(h.token_ids, h.log_prob) for h in want]
        assert all(type(a.log_prob) is type(b.log_prob) for a, b in zip(got, want))
        on, _ = CR.covered_beam_search(step_fn, init, Tp, dec_step, 4, 1, EOS, Tp, 0.3, 0.7, 0.05, 0.15)
        differs += [(h.token_ids, float(h.log_prob)) for h in on] != [(h.token_ids, float(h.log_prob)) for h in want]
        for h in on:
            cum, c, o = h.dec_state[1]
            assert (int(c), int(o)) == CR.counts(h.att[1:], Tp, 0.05, 0.15) and 0 <= o <= c <= Tp
            base = sum(np.float64(x) for x in CR.gains(h.att[1:], Tp, 0.3, 0.7, 0.05, 0.15))
            assert abs(base - (0.3 * c - 0.7 * o)) < 1e-4              # the gains telescope to the final counts
    assert differs


# ---- 2. flags -------------------------------------------------------------------------------------------------------------------------
def _parse(argv):
    from las.arguments import build_parser, str2bool
    from las import cli, vad
    parser = build_parser()
    cli.add_flags(parser)
    vad.add_flags(parser, str2bool)
    return parser.parse_args(argv), parser


def test_flags_are_off_by_default():
    from las import coverage
    args, parser = _parse(["--synthetic", "True"])
    assert (args.coverage_weight, args.coverage_threshold, args.overattend_weight, args.overattend_threshold, args.coverage_report) == \
           (0.0, 0.5, 0.0, 1.5, False)
    assert coverage.from_args(args) is None and coverage.from_args(argparse.Namespace()) is None
    from las import cli
    assert cli.check_flags(args, parser).json is False                 # plain text stays plain text
    args, parser = _parse(["--synthetic", "True", "--coverage_weight", "0.3"])
    assert cli.check_flags(args, parser).json is False and coverage.from_args(args) == coverage.Setting(0.3, 0.0, 0.5, 1.5, False)
    args, parser = _parse(["--synthetic", "True", "--coverage_report", "True"])
    assert cli.check_flags(args, parser).json is True and coverage.from_args(args).report


@pytest.mark.parametrize("argv,msg", [
    (["--coverage_weight", "-0.1"], "coverage weight"), (["--coverage_weight", "nan"], "coverage weight"),
    (["--overattend_weight", "inf"], "overattend weight"), (["--overattend_weight", "-1"], "overattend weight"),
    (["--coverage_threshold", "0"], "coverage threshold"), (["--coverage_threshold", "-1", "--coverage_report", "True"], "coverage threshold"),
    (["--overattend_threshold", "0.5"], "over-attention threshold"), (["--overattend_threshold", "0.25", "--coverage_weight", "1"], "over-attention"),
    (["--coverage_threshold", "nan"], "coverage threshold"),
    (["--ctc", "True", "--decoder", "ctc", "--coverage_weight", "0.3"], "no attention decoder"),
    (["--ctc", "True", "--decoder", "ctc", "--coverage_report", "True"], "no attention decoder"),
    (["--ctc", "True", "--keywords", "k.txt", "--overattend_weight", "0.3"], "no attention decoder"),
    (["--ctc", "True", "--align_text", "t.txt", "--coverage_report", "True"], "no attention decoder")])
def test_flag_refusals_before_anything_is_built(argv, msg):
    from las import cli
    args, parser = _parse(["--synthetic", "True"] + argv)
    with pytest.raises(ValueError, match=msg):
        cli.check_flags(args, parser)


def test_rescore_attention_takes_the_flags_and_the_constructor_refuses_too():
    from las import cli
    from las.beam_search import BeamSearch
    args, parser = _parse(["--synthetic", "True", "--ctc", "True", "--decoder", "ctc", "--rescore", "attention", "--beam_size", "4",
                           "--coverage_weight", "0.3"])
    assert cli.check_flags(args, parser).ctc_only

    class _Las(object):
        listener = speller = None
    tok = {"<SOS>": 1, "<EOS>": 2}
    with pytest.raises(ValueError, match="coverage weight"):
        BeamSearch(make_args(coverage_weight=-1.0), _Las(), tok, None)
    with pytest.raises(ValueError, match="over-attention threshold"):
        BeamSearch(make_args(coverage_report=True, overattend_threshold=0.4), _Las(), tok, None)
    bs = BeamSearch(make_args(overattend_weight=0.7), _Las(), tok, None)
    assert bs.coverage.w_o == 0.7 and bs.coverage.kappa == 1.5
    bs.set_coverage(0.0, 0.0, 0.5, 1.5, False)
    assert bs.coverage is None
    bs.set_coverage(0.0, 0.0, 0.25, 1.0, True)
    assert bs.coverage.report and bs.coverage.tau == 0.25
    with pytest.raises(ValueError):
        bs.set_coverage(0.1, 0.1, 1.0, 1.0, False)


# ---- 3. JSON --------------------------------------------------------------------------------------------------------------------------
def test_json_records_carry_the_two_shares():
    import test_transcript_host as TH
    from las import transcript as T

    def state(text, lp, cov):
        s = TH.State(text, lp)
        s.coverage = cov
        return s
    hi, ab = state("HI YO", -0.5, (30, 3, 40)), state("AB", -1.25, (10, 0, 40))
    args = make_args(timestamps=False, coverage_report=True)
    rec = lambda r: T.record(args, TH.ID, TH.FRAME_S, *r, 0.37)
    (r,) = T.choose(args, TH.StubSearch(), None, TH.Results([[ab, hi]]), TH.ID)
    assert json.dumps(rec(r)) == '{"text": "HI YO", "score": -0.5, "coverage": 0.75, "overattended": 0.075}'
    # a segment's record; the N-best entries; the consensus carries none; without the scorer nothing changes
    seg = T.record(args, TH.ID, TH.FRAME_S, *r, 0.37, (1.0, 1.37))
    assert list(seg) == ["start", "end", "text", "score", "coverage", "overattended"]
    nb = [(hi.token_ids[1:], -0.5, 0.625), (ab.token_ids[1:], -1.25, 0.375)]
    ann = TH.StubAnnotator([[TH.note(hi, 0.625, nbest=nb)]], nbest=2)
    (r,) = T.choose(make_args(timestamps=False), TH.StubSearch(), ann, TH.Results([[ab, hi]]), TH.ID)
    d = rec(r)
    assert (d["coverage"], d["overattended"]) == (0.75, 0.075)
    assert [(e["coverage"], e["overattended"]) for e in d["nbest"]] == [(0.75, 0.075), (0.25, 0.0)]
    cons = dict(words=["HI"], conf=[0.75], tokens=[], text="HI")
    ann = TH.StubAnnotator([[TH.note(hi, 0.625, network=[], consensus=cons)]], cn=True, cn_decode=True)
    (r,) = T.choose(make_args(timestamps=False), TH.StubSearch(), ann, TH.Results([[ab, hi]]), TH.ID)
    assert "coverage" not in rec(r) and "overattended" not in rec(r)
    (r,) = T.choose(make_args(timestamps=False), TH.StubSearch(), None, TH.Results([[TH.AB, TH.HI]]), TH.ID)
    assert rec(r) == {"text": "HI YO"}
    from las import coverage
    assert coverage.fields((0, 0, 0)) == {"coverage": 0.0, "overattended": 0.0} and coverage.fields(None) == {}


# ---- 4. header, binding, version ------------------------------------------------------------------------------------------------------
def test_header_binding_and_version_stay_in_step():
    import ctypes
    from las import _hip
    hdr = open(os.path.join(ROOT, "include", "las_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    version = int(re.search(r"#define LAS_HIP_ABI_VERSION (\d+)", hdr).group(1))
    assert version == _hip.ABI_VERSION >= 608                          # (608: the version that added the two entry points)
    ctype = {"const float*": ctypes.c_void_p, "float*": ctypes.c_void_p, "const int*": ctypes.c_void_p, "int*": ctypes.c_void_p,
             "void*": ctypes.c_void_p, "int": ctypes.c_int, "float": ctypes.c_float}
    for name in ("las_coverage_step", "las_coverage_rows"):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, code)
        assert m, "include/las_hip.h does not declare %s" % name
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        want = [ctype[p.rsplit(" ", 1)[0]] for p in params]
        res, got = _hip._SIGS[name]
        assert res is ctypes.c_int and got == want, (name, params)
        src = open(os.path.join(PKG, "csrc", "coverage.hip")).read()
        d = re.search(r'extern "C" int %s\s*\(([^)]*)\)' % name, src)
        assert d and [" ".join(p.split()) for p in d.group(1).split(",")] == params          # the definition, word for word
    # the scorer hands the entry point what the header lists: (head) + state_in, state_out, state_width + the loop words
    step = [" ".join(p.split()).rsplit(" ", 1)[1] for p in re.search(r"\bint\s+las_coverage_step\s*\(([^)]*)\)", code).group(1).split(",")]
    assert step[-10:] == ["state_in", "state_out", "state_width", "token", "step", "nlive", "done", "dec_step", "Umax", "stream"]
