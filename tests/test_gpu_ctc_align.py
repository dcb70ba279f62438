"""las_ctc_align (include/las_hip.h K10d, csrc/ctc_align.hip) against the float64 restatement tests/ctc_align_ref.py.  The contract fixes
the arithmetic (one fp64 addition per frame, in frame order) and the tie rule, so score, first, last and frame_state are compared for
EQUALITY: that is the bound the contract derives, not a measured one."""
import numpy as np
import pytest
import torch

import ctc_align_ref as R
import helpers  # noqa: F401

pytestmark = pytest.mark.gpu
SENTINEL = -77


def _launch(lp, lens, token_lists, U=None, want_states=True, ws_short=0):
    """-> rc, score [n] f64, first / last [n, U] (SENTINEL where nothing was written), states [n, Tp] or None"""
    from las import _hip
    lp = np.ascontiguousarray(lp, np.float32)
    n, Vc, Tp = lp.shape
    U = max(1, max(len(t) for t in token_lists)) if U is None else U
    y = np.zeros((n, U), np.int32)
    for u, t in enumerate(token_lists):
        y[u, :len(t)] = t
    i32 = dict(dtype=torch.int32, device="cuda")
    d_lp = torch.tensor(lp, device="cuda")
    d_len, d_y, d_yl = torch.tensor(lens, **i32), torch.tensor(y, **i32), torch.tensor([len(t) for t in token_lists], **i32)
    first, last = torch.full((n, U), SENTINEL, **i32), torch.full((n, U), SENTINEL, **i32)
    states = torch.full((n, Tp), SENTINEL, **i32) if want_states else None
    score = torch.full((n,), 123.0, dtype=torch.float64, device="cuda")
    lib = _hip.lib()
    nbytes = lib.las_ctc_align_workspace_bytes(n, Tp, U)
    ws = torch.zeros(max(nbytes, 256), dtype=torch.uint8, device="cuda")
    rc = lib.las_ctc_align(_hip.p(d_lp), Vc, Tp, _hip.p(d_len), n, _hip.p(d_y), U, _hip.p(d_yl), U, _hip.p(first), _hip.p(last),
                           _hip.p(states), _hip.p(score), _hip.p(ws), nbytes - ws_short, _hip.stream())
    torch.cuda.synchronize()
    return rc, score.cpu().numpy(), first.cpu().numpy(), last.cpu().numpy(), None if states is None else states.cpu().numpy()


def _check_rows(lp, lens, token_lists, out):
    rc, score, first, last, states = out
    assert rc == 0
    n, Vc, Tp = lp.shape
    n_bad = 0
    for u, labels in enumerate(token_lists):
        T, L = min(max(int(lens[u]), 1), Tp), len(labels)
        ref = R.align(lp[u], labels, T)
        assert score[u] == ref.score, (u, score[u], ref.score)                    # equal bits (both float64)
        assert np.array_equal(first[u, :L], ref.first) and np.array_equal(last[u, :L], ref.last), (u, first[u, :L], ref.first)
        assert np.all(first[u, L:] == SENTINEL) and np.all(last[u, L:] == SENTINEL)      # entries j >= y_len[u] are not written
        if states is not None:
            assert np.all(states[u, T:] == -1)
            if ref.states is None:
                assert np.all(states[u] == -1)
            else:
                assert np.array_equal(states[u, :T], ref.states), (u, states[u, :T], ref.states)
                assert R.check_path(lp[u], labels, T, states[u]) == score[u]
        n_bad += ref.states is None
    return n_bad


def _lp(rng, n, Vc, Tp, scale=2.0):
    return torch.log_softmax(torch.tensor(rng.randn(n, Tp, Vc) * scale, dtype=torch.float32), -1).transpose(1, 2).contiguous().numpy()


def _labels(rng, L, Vc, repeats=False):
    """L labels in [0, Vc - 2]; without `repeats` no two neighbours are equal (so L labels need only L frames)"""
    out = []
    for j in range(L):
        c = int(rng.randint(0, Vc - 1))
        if repeats and j % 3 == 1:
            c = out[-1]
        while not repeats and out and c == out[-1]:
            c = int(rng.randint(0, Vc - 1))
        out.append(c)
    return out


@pytest.mark.parametrize("Vc", [31, 5001])
@pytest.mark.parametrize("Tp", [1, 2, 7, 65, 160])
def test_matches_restatement(Tp, Vc):
    """three utterances of different enc_len per launch; label counts 0 (all blanks), 1, 3, 33 (S = 67: more than one wave), the most
    that fits the row (L = T_u), and rows with adjacent repeats; counts that do not fit a short row are unalignable there and must say so"""
    rng = np.random.RandomState(Tp * 7 + Vc)
    lens = [Tp, max(1, Tp - 3), max(1, Tp // 2)]
    lp = _lp(rng, 3, Vc, Tp)
    for counts, repeats in (((0, 1, 3), (False, False, True)), ((33, lens[1], 3), (False, False, False)),
                            ((lens[0], 33, lens[2]), (False, True, False)), ((1, 0, 33), (False, False, True))):
        toks = [_labels(rng, L, Vc, rep) for L, rep in zip(counts, repeats)]
        out = _launch(lp, lens, toks)
        _check_rows(lp, lens, toks, out)
        again = _launch(lp, lens, toks)
        for a, b in zip(out[1:], again[1:]):                                        # two runs: the same bits
            assert np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if b.dtype == np.float64 else b)
    # frame_state is optional
    out = _launch(lp, lens, toks, want_states=False)
    _check_rows(lp, lens, toks, out)


def test_largest_state_count_and_long_rows():
    """U = 511 (S = 1023 states, every lane of the 1024-thread workgroup but one) at T' = 1100: 69 back-pointer rows of 1024 words, staged
    into LDS eight rows at a time by the back-trace; a second row is shorter in both directions"""
    rng = np.random.RandomState(5)
    Vc, Tp = 31, 1100
    lens = [Tp, 777]
    lp = _lp(rng, 2, Vc, Tp, scale=1.0)
    toks = [_labels(rng, 511, Vc, repeats=True), _labels(rng, 200, Vc, repeats=True)]
    assert _check_rows(lp, lens, toks, _launch(lp, lens, toks)) == 0


def test_ties_follow_the_rule():
    """a uniform lp (every path ties) and an lp that is constant along t: exactly the restatement's path"""
    rng = np.random.RandomState(9)
    Vc, Tp = 6, 40
    lens = [40, 23, 9]
    toks = [[0, 1, 1, 2, 0], [3, 3], [4, 0, 4, 0, 4, 0, 4]]
    uniform = np.full((3, Vc, Tp), np.float32(np.log(1.0 / Vc)), np.float32)
    assert _check_rows(uniform, lens, toks, _launch(uniform, lens, toks)) == 0
    rc, _, _, _, states = _launch(uniform, [6], [[0, 1]])
    assert rc == 0 and list(states[0, :6]) == [1, 3, 4, 4, 4, 4]                    # (the case worked by hand in test_ctc_align_host.py)
    const_t = np.repeat(_lp(rng, 3, Vc, 1), Tp, axis=2)
    assert _check_rows(const_t, lens, toks, _launch(const_t, lens, toks)) == 0


def test_planted_alignment_is_recovered():
    """lp peaky around a chosen alignment, every other class at least 5 nats below the planted one in every frame: any other path loses
    5 nats per frame it deviates in, so first / last are the planted ranges"""
    rng = np.random.RandomState(2)
    Vc, Tp = 31, 90
    lens, toks, want = [90, 61], [_labels(rng, 12, Vc, repeats=True), _labels(rng, 20, Vc, repeats=True)], []
    logits = rng.uniform(0, 1, size=(2, Vc, Tp)).astype(np.float32)
    for u, labels in enumerate(toks):
        T, L = lens[u], len(labels)
        # L label runs and L + 1 blank runs (the inner blanks at least one frame long) that fill the T frames
        runs = np.ones(2 * L + 1, np.int64)
        runs[0] = runs[-1] = 0
        for _ in range(T - int(runs.sum())):
            runs[rng.randint(0, 2 * L + 1)] += 1
        t, first, last = 0, [], []
        for s, r in enumerate(runs):
            c = labels[s >> 1] if s & 1 else Vc - 1
            logits[u, c, t:t + r] += 6.0
            if s & 1:
                first.append(t)
                last.append(t + r - 1)
            t += r
        assert t == T
        want.append((first, last))
    lp = torch.log_softmax(torch.tensor(logits), 1).numpy()
    out = _launch(lp, lens, toks)
    assert _check_rows(lp, lens, toks, out) == 0
    for u, (first, last) in enumerate(want):
        assert list(out[2][u, :len(first)]) == first and list(out[3][u, :len(last)]) == last


def test_unalignable_rows_leave_their_neighbours_alone():
    """more labels than frames; repeats that need more blanks than there are frames; a label equal to the blank class; a negative label:
    -inf and -1s for the row, the restatement's result for the rows beside it, return code 0"""
    rng = np.random.RandomState(4)
    Vc, Tp = 31, 12
    lens = [12, 5, 12, 6, 12, 12, 9]
    toks = [_labels(rng, 4, Vc), _labels(rng, 6, Vc), _labels(rng, 5, Vc, repeats=True), [7, 7, 7, 7],       # row 1: 6 > 5; row 3: 4 + 3 > 6
            [1, Vc - 1, 2], [3, -1], _labels(rng, 9, Vc)]
    lp = _lp(rng, len(toks), Vc, Tp)
    out = _launch(lp, lens, toks)
    assert _check_rows(lp, lens, toks, out) == 4
    rc, score, first, last, states = out
    for u in (1, 3, 4, 5):
        L = len(toks[u])
        assert score[u] == -np.inf and np.all(first[u, :L] == -1) and np.all(last[u, :L] == -1) and np.all(states[u] == -1)
    for u in (0, 2, 6):
        assert np.isfinite(score[u])


def test_refusals():
    """U = 512, T' = 2049 and a short workspace: a nonzero return, a las_last_error text, and nothing launched (the outputs keep what the
    test put there)"""
    from las import _hip
    lib = _hip.lib()
    lp = np.zeros((1, 4, 8), np.float32)
    for kw, toks, text, shape in ((dict(U=512), [[0, 1]], b"U=512", lp), (dict(), [[0, 1]], b"T' <= 2048", np.zeros((1, 4, 2049), np.float32)),
                                  (dict(ws_short=1), [[0, 1]], b"workspace too small", lp)):
        rc, score, first, last, states = _launch(shape, [8], toks, **kw)
        assert rc != 0 and text in lib.las_last_error(), (rc, lib.las_last_error())
        assert score[0] == 123.0 and np.all(first == SENTINEL) and np.all(last == SENTINEL) and np.all(states == SENTINEL)
    assert lib.las_ctc_align_workspace_bytes(1, 8, 2) > 0
