"""Speaker diarization on the host: the numpy restatement tests/diarize_ref.py against a two-pass LAPACK evaluation, its peak,
tie and stopping rules on hand-made inputs, the synthetic two-voice recording of the CLI test through the float64 front end and the VAD
restatement (every decision keeps a margin of 100 from zero, so a drifting recipe shows here), and transcribe.py's flags and output."""
import json

import numpy as np
import pytest

import helpers  # noqa: F401
import diarize_ref as R
import frontend_ref as FR
import vad_ref as VR

FLOOR = 1e-4


def _two_pass(x, floor):
    """log det of the floored covariance of the rows of x, centred first: the textbook two-pass form, through LAPACK"""
    x = x.astype(np.float64)
    c = x - x.mean(0)
    return np.linalg.slogdet(c.T @ c / len(x) + floor * np.eye(x.shape[1]))[1]


def _two_pass_bic(x, y, lam, floor):
    n1, n2, D = len(x), len(y), x.shape[1]
    n = n1 + n2
    return 0.5 * (n * _two_pass(np.concatenate([x, y]), floor) - n1 * _two_pass(x, floor) - n2 * _two_pass(y, floor)) \
        - lam * 0.5 * (D + D * (D + 1) / 2) * np.log(n)


def test_one_pass_delta_bic_is_the_two_pass_one():
    rng = np.random.RandomState(0)
    for D, n1, n2 in ((1, 5, 9), (13, 40, 100), (20, 60, 61)):
        x, y = rng.randn(n1, D).astype(np.float32), (1.5 * rng.randn(n2, D) + 0.5).astype(np.float32)
        x[:, 0] -= 300.0                                                  # a column with mean -300 and unit variance
        y[:, 0] -= 300.0
        got = float(R.delta_bic(R.stats(x, None, 0, n1, D), R.stats(y, None, 0, n2, D), 1.0, FLOOR))
        want = _two_pass_bic(x, y, 1.0, FLOOR)
        assert abs(got - want) <= 1e-7 * (1 + abs(want)), (D, got, want)
    # the batched window statistics are the loop's, bit for bit; a masked frame does not count
    feat = rng.randn(50, 5).astype(np.float32)
    mask = (rng.rand(50) < 0.7).astype(np.uint8)
    n, S1, S2 = R.window_stats(feat, mask, [3, 17], 20, 4)
    for k, s in enumerate((3, 17)):
        a = R.stats(feat, mask, s, s + 20, 4)
        assert a[0] == n[k] == mask[s:s + 20].sum() and np.array_equal(a[1], S1[k]) and np.array_equal(a[2], S2[k])
    # constant frames: the floor alone keeps the matrix regular
    const = np.ones((30, 3), np.float32)
    assert float(R.logdet(R.stats(const, None, 0, 30, 3), FLOOR)) == pytest.approx(3 * np.log(FLOOR), rel=1e-12)


def test_peak_rule_on_hand_made_curves():
    inf = float("inf")
    P = lambda v, R_: R.peaks(np.asarray(v, float), R_).tolist()
    assert P([1, 3, 2], 1) == [0, 1, 0]
    assert P([-1, -3, -2], 1) == [0, 0, 0]                                # a peak is positive
    assert P([0.0, 0.0], 1) == [0, 0]
    assert P([2, 5, 5, 5, 1], 1) == [0, 1, 0, 0, 0]                       # a plateau: the first of equal maxima
    assert P([5, 1, 5], 1) == [1, 0, 1] and P([5, 1, 5], 2) == [1, 0, 0]  # equal maxima inside one window
    assert P([5, -inf, 4], 1) == [1, 0, 1] and P([5, -inf, 4], 2) == [1, 0, 0]   # a gap of -inf separates nothing by itself
    assert P([-inf, -inf, 3, -inf], 2) == [0, 0, 1, 0]
    assert P([7], 3) == [1] and P([], 3) == []                            # the ends of the curve: only existing neighbours count
    assert P([4, 3, 2, 1], 2) == [1, 0, 0, 0] and P([1, 2, 3, 4], 2) == [0, 0, 0, 1]
    # two peaks are more than R candidates apart
    rng = np.random.RandomState(1)
    for R_ in (1, 3, 10):
        at = np.flatnonzero(R.peaks(rng.randn(500), R_))
        assert len(at) > 3 and (np.diff(at) > R_).all()
    assert R.candidates(39, 20, 7) == 0 and R.candidates(40, 20, 7) == 1 and R.candidates(46, 20, 7) == 1 and R.candidates(47, 20, 7) == 2


def _six_units():
    rng = np.random.RandomState(3)
    D = 13
    voices = {}
    for name in "abc":
        voices[name] = (rng.randn(D) * 1.5, rng.randn(D, D) * 0.3 + np.eye(D))
    feats = [(rng.randn(n, D) @ voices[v][1].T + voices[v][0]).astype(np.float32) for v, n in zip("abacba", (300, 200, 150, 400, 250, 180))]
    return [R.stats(f, None, 0, len(f), D) for f in feats]


def test_clustering_three_speakers():
    units = _six_units()
    cl = R.cluster(units, 0, 1.0, FLOOR)
    assert R.groups(cl.label) == [[0, 2, 5], [1, 4], [3]] and cl.n_clusters == 3 and cl.label == [0, 1, 0, 2, 1, 0]
    assert len(cl.merges) == 3 and max(cl.merge_val) < -100 and cl.stop_val > 100, (cl.merge_val, cl.stop_val)
    same = [(0, 2), (0, 5), (2, 5), (1, 4)]
    cross = [cl.dist[i, j] for i in range(6) for j in range(i + 1, 6) if (i, j) not in same]
    assert min(cross) > 100 and max(cl.dist[i, j] for i, j in same) < -100
    # --num_speakers: forced down to K whatever the sign, never below; numbering by first appearance
    assert R.cluster(units, 3, 1.0, FLOOR).label == cl.label
    two = R.cluster(units, 2, 1.0, FLOOR)
    assert two.n_clusters == 2 and two.merge_val[-1] > 0 and two.label[0] == 0 and sorted(set(two.label)) == [0, 1]
    assert R.cluster(units, 1, 1.0, FLOOR).label == [0] * 6 and R.cluster(units, 6, 1.0, FLOOR).label == list(range(6))
    assert R.cluster(units, 9, 1.0, FLOOR).label == list(range(6))       # more speakers than units: nothing to merge
    assert R.cluster(units[:1], 0, 1.0, FLOOR).label == [0]
    order = R.cluster([units[3], units[0], units[1], units[2]], 0, 1.0, FLOOR)          # c a b a
    assert order.label == [0, 1, 2, 1]


def test_identical_units_merge_in_index_order():
    rng = np.random.RandomState(4)
    f = rng.randn(40, 5).astype(np.float32)
    u = R.stats(f, None, 0, 40, 5)
    cl = R.cluster([u, u, u], 0, 1.0, FLOOR)
    assert cl.dist[0, 1] == cl.dist[0, 2] == cl.dist[1, 2] < 0
    assert cl.merges == [(0, 1), (0, 2)] and cl.label == [0, 0, 0]


# ---- the synthetic recording of tests/test_gpu_diarize_cli.py --------------------------------------------------------------------------------
FL, STEP, W, HOP, D = 400, 160, 100, 10, 13


def test_two_voice_recording_keeps_its_margins():
    """measured here: the change peak at frame 300 +208, every candidate more than w from it at most -166 (this restatement: -172), the
    same-voice distances -235 and -221, the cross-voice ones at least +747.  Every one keeps 100 from zero."""
    wave = R.two_voices()
    e, emax, runs = VR.vad(wave, FL, STEP, 1e-4, FL * 1e-7, 20, 10)      # the flags' defaults: 40 dB, -70 dB, 200 ms, 100 ms
    assert len(runs) == 3 and runs[0][0] == 0
    speech = (e >= max(emax * 1e-4, FL * 1e-7)) & (e > 0)                # 40 dB under the peak
    a = FR.fe_args(feat_dim=39, cmvn=False)
    units, far = [], []
    for ra, rb in runs:
        f = FR.ref64(wave[ra * STEP:(rb - 1) * STEP + FL], a)
        assert f.shape == (rb - ra - 1, 39)
        m = speech[ra:ra + len(f)]
        v = R.change_curve(f, m, 0, len(f), D, W, HOP, max(D + 1, W // 2), 1.0, FLOOR)
        pk = np.flatnonzero(R.peaks(v, W // HOP))
        if ra == 0:
            assert len(pk) == 1 and abs(W + pk[0] * HOP - 300) <= 1 and v[pk[0]] > 100, (pk, v[pk])
        else:
            assert len(pk) == 0
        far += [v[c] for c in range(len(v)) if all(abs(c - p) * HOP > W for p in pk)]
        for ua, ub in R.split_at((ra, rb), R.peaks(v, W // HOP), W, HOP):
            units.append((R.stats(f, m, ua - ra, min(ub - ra, len(f)), D), R.stats(f, None, ua - ra, min(ub - ra, len(f)), D)))
    assert max(far) < -100, max(far)
    cl = R.cluster([u[0] for u in units], 0, 1.0, FLOOR)
    assert cl.label == [0, 1, 0, 1] and cl.merges == [(0, 2), (1, 3)] and max(cl.merge_val) < -100
    assert min(cl.dist[i, j] for i, j in ((0, 1), (0, 3), (1, 2), (2, 3))) > 100
    # without the speech mask the padded silence splits voice A in two
    assert R.cluster([u[1] for u in units], 0, 1.0, FLOOR).dist[0, 2] > 100


# ---- transcribe.py: flags, records, RTTM -------------------------------------------------------------------------------------------------
REFUSALS = [
    (["--diarize", "True", "a.wav"], "--diarize labels the segments of --segment True: give both"),
    (["--diarize", "True", "--segment", "True", "--ctc", "True", "--keywords", "k.txt", "a.wav"],
     "--diarize labels the segments a search transcribes, --keywords prints keyword hits and runs no search: use one of them"),
    (["--diarize", "True", "--ctc", "True", "--keywords", "k.txt", "a.wav"],
     "--diarize labels the segments a search transcribes, --keywords prints keyword hits and runs no search: use one of them"),
    (["--diarize", "True", "--segment", "True", "--ctc", "True", "--align_text", "refs.txt", "a.wav"],
     "--diarize labels the segments a search transcribes, --align_text aligns one transcript per whole file: use one of them"),
    (["--diarize", "True", "--ctc", "True", "--align_text", "refs.txt", "a.wav"],
     "--diarize labels the segments a search transcribes, --align_text aligns one transcript per whole file: use one of them"),
    (["--diarize", "True", "--segment", "True", "--num_speakers", "-1", "a.wav"], "--num_speakers -1: 0 (decide by BIC) to 1024"),
    (["--diarize", "True", "--segment", "True", "--diar_hop_ms", "0", "a.wav"],
     "--diar_window_ms 1000.0, --diar_hop_ms 0.0: positive numbers of milliseconds"),
    (["--diarize", "True", "--segment", "True", "--diar_cluster_lambda", "nan", "a.wav"],
     "--diar_change_lambda 1.0, --diar_cluster_lambda nan: finite penalty weights"),
    (["--segment", "True", "--rttm", "out.rttm", "a.wav"], "--rttm writes the speakers of --diarize True: give both")]


@pytest.mark.parametrize("argv,message", REFUSALS, ids=[" ".join(a) for a, _ in REFUSALS])
def test_refusals_come_before_any_audio_is_read(argv, message):
    import transcribe
    with pytest.raises(ValueError) as e:                                  # (a.wav does not exist: reading it would be another error)
        transcribe.main(argv)
    assert str(e.value) == message


def test_diarize_switches_to_json_lines_and_is_imported_on_demand():
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import transcribe\n"
            "from las import cli, vad\n"
            "def mode(argv):\n"
            "    p = transcribe.build_parser(); cli.add_flags(p); vad.add_flags(p, cli.str2bool); cli.add_diarize_flags(p)\n"
            "    return cli.check_flags(p.parse_args(argv), p)\n"
            "assert mode(['--segment', 'True', 'a.wav']).json is False and 'las.diarize' not in sys.modules\n"
            "assert mode(['--segment', 'True', '--diarize', 'True', 'a.wav']) == cli.Mode('search', False, False, True)\n"
            "assert 'las.diarize' in sys.modules\n") % helpers.PKG
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


def test_flags_window_geometry_and_rttm():
    import argparse
    from las import cli
    from las import diarize as DZ
    p = argparse.ArgumentParser()
    DZ.add_flags(p, cli.str2bool)
    a = p.parse_args([])
    assert (a.diarize, a.num_speakers, a.diar_window_ms, a.diar_hop_ms, a.diar_change_lambda, a.diar_cluster_lambda, a.rttm) == \
        (False, 0, 1000.0, 100.0, 1.0, 1.0, "")
    assert DZ.rttm_line("meeting", 3.0049999, 2.5, 2) == "SPEAKER meeting 1 3.005 2.500 <NA> <NA> S2 <NA> <NA>"
    assert DZ.split_run((100, 700), np.array([0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1], np.uint8), 100, 10) == [(100, 220), (220, 350), (350, 700)]
    assert DZ.split_run((5, 50), np.zeros(0, np.uint8), 100, 10) == [(5, 50)] == R.split_at((5, 50), np.zeros(0, np.uint8), 100, 10)


def test_file_lines_carry_speakers(capsys):
    import argparse
    from las import transcript as T
    ids = {3: "H", 4: "I", 1: " "}
    args = argparse.Namespace(unit="char", timestamps=False, diarize=True)
    files = T.FileAssembler(lambda *a: T.record(args, ids, 0.08, *a), True)
    files.add_file([(0, 8000), (8000, 20000)], 8000, speakers=([1, 2], 2))
    files.add_file([], 8000, speakers=([], 0))
    files.take([3, 4], -1.0, None, {})
    files.take([4], -0.5, [(0, 1)], {})
    files.emit_finished()
    lines = [json.loads(x) for x in capsys.readouterr().out.splitlines()]
    assert lines[0] == {"text": "HI I", "score": -1.5, "speakers": 2, "segments": [
        {"start": 0.0, "end": 1.0, "text": "HI", "score": -1.0, "speaker": 1},
        {"start": 1.0, "end": 2.5, "text": "I", "score": -0.5, "words": [{"word": "I", "start": 1.0, "end": 1.16, "speaker": 2}], "speaker": 2}]}
    assert lines[1] == {"text": "", "score": 0.0, "speakers": 0, "segments": []}
    # without speakers the records are what they were
    files.add_file([(0, 8000)], 8000)
    files.take([3], -1.0, None, {})
    assert json.loads(capsys.readouterr().out) == {"text": "H", "score": -1.0, "segments": [{"start": 0.0, "end": 1.0, "text": "H", "score": -1.0}]}
