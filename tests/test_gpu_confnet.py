"""las_nbest_network (include/las_hip.h K10h, csrc/nbest.hip) against the numpy restatement tests/confnet_ref.py.  Every decision of the
contract is an integer one and the masses are fp32 sums in a fixed order, so EVERY output is compared for EQUALITY (post by its bits):
the bound the contract derives, as in test_gpu_nbest.py.  Outputs are pre-filled with a sentinel; padding symbols, absent slots' symbols
and lengths hold garbage, absent slots' weights NaN."""
import numpy as np
import pytest
import torch

import helpers  # noqa: F401
import confnet_ref as C

pytestmark = pytest.mark.gpu
SENT_I, SENT_F, SENT_B = -77, 123.0, 55
U_CEILING, BINS_CEILING = 1024, 2048                                   # include/las_hip.h K10h


def _launch(utts, weights, K=None, U=None, max_bins=None, ws_short=0, seed=0):
    """utts[u] = the live hypotheses of utterance u (best first), weights[u] their fp32 weights -> dict of the return code and host arrays"""
    from las import _hip
    rng = np.random.RandomState(2000 + seed)
    n = len(utts)
    K = max(1, max(len(h) for h in utts)) if K is None else K
    U = max(1, max((len(t) for h in utts for t in h), default=1)) if U is None else U
    if max_bins is None:
        max_bins = min(BINS_CEILING, max(1, max(sum(len(t) for t in h) for h in utts)))
    sym = rng.randint(-5, 6000, size=(n, K, U)).astype(np.int32)        # garbage wherever nothing lives
    ln = rng.randint(0, U + 1, size=(n, K)).astype(np.int32)
    w = np.full((n, K), np.nan, np.float32)
    nh = np.zeros(n, np.int32)
    for u, hyps in enumerate(utts):
        nh[u] = len(hyps)
        w[u, :len(hyps)] = np.asarray(weights[u], np.float32)
        for k, t in enumerate(hyps):
            ln[u, k] = len(t)
            sym[u, k, :len(t)] = t
    d = lambda x: torch.as_tensor(x).cuda()
    d_sym, d_len, d_nh, d_w = d(sym), d(ln), d(nh), d(w)
    i32 = dict(dtype=torch.int32, device="cuda")
    cols = torch.full((n, K, max(max_bins, 1)), SENT_I, **i32)
    nbins = torch.full((n,), SENT_I, **i32)
    merged = torch.full((n, K), SENT_B, dtype=torch.int8, device="cuda")
    best = torch.full((n, max(max_bins, 1)), SENT_I, **i32)
    post = torch.full((n, max(max_bins, 1)), SENT_F, device="cuda")
    lib = _hip.lib()
    nbytes = lib.las_nbest_network_workspace_bytes(n, K, U, max_bins)
    ws = torch.full((max(nbytes, 256),), 0xA5, dtype=torch.uint8, device="cuda")
    rc = lib.las_nbest_network(_hip.p(d_sym), _hip.p(d_len), _hip.p(d_nh), _hip.p(d_w), n, K, U, max_bins, _hip.p(cols), _hip.p(nbins),
                               _hip.p(merged), _hip.p(best), _hip.p(post), _hip.p(ws), max(nbytes - ws_short, 0), _hip.stream())
    torch.cuda.synchronize()
    return dict(rc=rc, n=n, K=K, U=U, max_bins=max_bins, cols=cols.cpu().numpy(), nbins=nbins.cpu().numpy(), merged=merged.cpu().numpy(),
                best=best.cpu().numpy(), post=post.cpu().numpy())


def _bits(x):
    return np.asarray(x, np.float32).view(np.int32)


_REF = {}


def _ref(hyps, w, max_bins):
    """the restatement's network of one utterance, computed once per distinct input"""
    key = (tuple(map(tuple, hyps)), _bits(w).tobytes(), max_bins)
    if key not in _REF:
        _REF[key] = C.network(hyps, w, max_bins, "f32")
    return _REF[key]


def _check(utts, weights, out):
    assert out["rc"] == 0
    for u, hyps in enumerate(utts):
        nh = len(hyps)
        ref = _ref(hyps, weights[u], out["max_bins"])
        B = ref["nbins"]
        assert out["nbins"][u] == B, (u, out["nbins"][u], B)
        assert np.array_equal(out["merged"][u, :nh], ref["merged"]), (u, out["merged"][u, :nh], ref["merged"])
        assert np.all(out["merged"][u, nh:] == SENT_B)
        for k in range(nh):
            if ref["merged"][k]:
                assert np.array_equal(out["cols"][u, k, :B], ref["cols"][k]), (u, k, out["cols"][u, k, :B], ref["cols"][k])
                row = out["cols"][u, k, :B]
                assert [int(s) for s in row[row != C.EPS]] == [max(int(t), 0) for t in hyps[k]]      # the invariant
                assert np.all(out["cols"][u, k, B:] == SENT_I)
            else:
                assert np.all(out["cols"][u, k] == SENT_I)
        assert np.all(out["cols"][u, nh:] == SENT_I)                    # absent slots: nothing written
        assert np.array_equal(out["best"][u, :B], ref["best"]), (u, out["best"][u, :B], ref["best"])
        assert np.array_equal(_bits(out["post"][u, :B]), _bits(ref["post"])), (u, out["post"][u, :B], ref["post"])
        assert np.all(out["best"][u, B:] == SENT_I) and np.all(out["post"][u, B:] == SENT_F)


def _weights(rng, utts):
    out = []
    for hyps in utts:
        w = rng.uniform(0.01, 1.0, size=len(hyps))
        out.append((w / max(w.sum(), 1e-9)).astype(np.float32))
    return out


LENGTHS = [0, 1, 2, 15, 16, 17, 63, 64, 65, 130]


@pytest.mark.parametrize("vocab", [2, 3, 5000])
def test_length_edges(vocab):
    """hypotheses of the lengths {0, 1, 2, 15, 16, 17, 63, 64, 65, 130} in one utterance, in four orders (rising, falling, two drawn): the
    edges of the 64-column chunks, of the 16-bin direction words, the empty hypothesis first and last.  An alphabet of 2 or 3 makes zero-cost
    moves and ties everywhere, one of 5000 nearly none.  K = 16 slots, 10 live"""
    rng = np.random.RandomState(vocab)
    hyps = [list(rng.randint(0, vocab, size=L)) for L in LENGTHS]
    utts = [hyps, hyps[::-1], [hyps[i] for i in rng.permutation(10)], [hyps[i] for i in rng.permutation(10)]]
    weights = _weights(rng, utts)
    _check(utts, weights, _launch(utts, weights, K=16))


@pytest.mark.parametrize("vocab", [3, 5000])
def test_networks_growing_across_the_block_edges(vocab):
    """prefixes of one string of the lengths 15, 16, 17, 31, 32, 33, 63, 64, 65, 130, shortest first: the network has exactly that many
    bins after each merge, so tables of 15, 16, 17, 32, 33, 64, 65 rows are run and the in-place rebuild appends at each of these sizes;
    a second utterance takes them with a noisy token in each so that bins are inserted inside, not only appended"""
    rng = np.random.RandomState(7 + vocab)
    s = list(rng.randint(0, vocab, size=130))
    sizes = [15, 16, 17, 31, 32, 33, 63, 64, 65, 130]
    a = [s[:L] for L in sizes]
    b = []
    for L in sizes:
        h = s[:L]
        h.insert(int(rng.randint(0, L)), int(rng.randint(0, vocab)))
        b.append(h)
    utts = [a, b]
    weights = _weights(rng, utts)
    out = _launch(utts, weights, K=16)
    _check(utts, weights, out)
    assert _ref(a, weights[0], out["max_bins"])["sizes"] == [0] + sizes
    assert out["nbins"][1] > 65


@pytest.mark.parametrize("K", [1, 2, 3, 16, 64])
def test_slot_counts(K):
    """K = 1, 2, 3, 16 (the search's beam), 64 (the ceiling: every lane of the rebuild is a slot); utterances with nhyp = K, K - 1, K // 2,
    1 and 0 in one batch"""
    rng = np.random.RandomState(K)
    utts = [[list(rng.randint(0, 4, size=rng.randint(0, 12))) for _ in range(nh)] for nh in (K, K - 1, K // 2, 1, 0)]
    weights = _weights(rng, utts)
    out = _launch(utts, weights, K=K)
    _check(utts, weights, out)
    assert out["nbins"][4] == 0 and np.all(out["cols"][4] == SENT_I) and np.all(out["merged"][4] == SENT_B)


def test_hand_made_cases_and_a_negative_symbol():
    """a b c / a c / a x c under two weightings; a b c d / a x c y / e b c y; and negative symbols, which are read as 0"""
    a, b, c, x, y, e, d = 1, 2, 3, 4, 5, 6, 7
    utts = [[[a, b, c], [a, c], [a, x, c]], [[a, b, c], [a, c], [a, x, c]], [[a, b, c, d], [a, x, c, y], [e, b, c, y]],
            [[a, -3, c], [a, 0, c], [-1]]]
    weights = [np.asarray(w, np.float32) for w in ([0.4, 0.35, 0.25], [0.3, 0.45, 0.25], [0.4, 0.3, 0.3], [0.5, 0.3, 0.2])]
    out = _launch(utts, weights)
    _check(utts, weights, out)
    assert out["nbins"][0] == 3 and list(out["cols"][0, :3, 1]) == [b, C.EPS, x]
    assert list(out["best"][0, :3]) == [a, b, c] and list(out["best"][1, :3]) == [a, C.EPS, c]
    assert list(out["best"][2, :4]) == [a, b, c, y]                     # the consensus no hypothesis holds
    assert out["nbins"][3] == 3 and list(out["cols"][3, 0, :3]) == [a, 0, c] and list(out["best"][3, :3]) == [a, 0, c]
    # ... and [-1] is [0]: all three agree on bin 1, the mass is the three weights added in slot order
    assert list(out["cols"][3, 2, :3]) == [C.EPS, 0, C.EPS]
    assert out["post"][3, 1] == np.float32(np.float32(np.float32(0.5) + np.float32(0.3)) + np.float32(0.2))


def test_overflow():
    """max_bins = 4: hypothesis 0 (5 tokens) does not fit and is not merged, 1 and 2 are, 3 would need two more bins and is left out, 4
    (a match everywhere) is merged again"""
    utts = [[[1, 2, 3, 4, 5], [1, 2, 3], [1, 9, 3, 4], [7, 7, 1, 2, 3, 4], [1, 2, 3, 4]], [[1, 2], [1, 2, 3, 4], [5, 6, 7, 8, 9]]]
    weights = [np.asarray([0.3, 0.25, 0.2, 0.15, 0.1], np.float32), np.asarray([0.5, 0.3, 0.2], np.float32)]
    out = _launch(utts, weights, max_bins=4)
    _check(utts, weights, out)
    assert list(out["merged"][0, :5]) == [0, 1, 1, 0, 1] and out["nbins"][0] == 4
    assert list(out["merged"][1, :3]) == [1, 1, 0] and out["nbins"][1] == 4


def test_at_the_ceiling():
    """U = 1024, max_bins = 2048, K = 3: 16 column chunks, a table of more than 1024 rows, the walk staging two row blocks at a time"""
    rng = np.random.RandomState(8)
    a = list(rng.randint(0, 4, size=U_CEILING))
    b = list(a)
    for _ in range(150):                                               # a noisy copy: deletions, insertions, substitutions
        p = rng.randint(0, len(b))
        op = rng.randint(0, 3)
        if op == 0 and len(b) > 1:
            del b[p]
        elif op == 1 and len(b) < U_CEILING:
            b.insert(p, int(rng.randint(0, 4)))
        else:
            b[p] = int(rng.randint(0, 4))
    c = list(rng.randint(0, 4, size=U_CEILING - 7))
    utts = [[a, b, c]]
    weights = [np.asarray([0.5, 0.3, 0.2], np.float32)]
    out = _launch(utts, weights, max_bins=BINS_CEILING)
    assert out["U"] == U_CEILING and out["K"] == 3
    _check(utts, weights, out)
    assert out["nbins"][0] > U_CEILING


def test_refusals():
    """K = 65, U = 1025, max_bins = 0 and 2049, a workspace short by one byte: a negative status, a las_last_error text, untouched outputs"""
    from las import _hip
    lib = _hip.lib()
    utts, weights = [[[1, 2], [1]]], [np.asarray([0.5, 0.5], np.float32)]
    for kw, text in ((dict(U=U_CEILING + 1), b"U=1025"), (dict(K=65), b"K <= 64"), (dict(max_bins=BINS_CEILING + 1), b"max_bins=2049"),
                     (dict(max_bins=0), b"max_bins=0"), (dict(ws_short=1), b"workspace too small")):
        out = _launch(utts, weights, **kw)
        assert out["rc"] < 0 and text in lib.las_last_error(), (out["rc"], lib.las_last_error())
        assert np.all(out["cols"] == SENT_I) and np.all(out["nbins"] == SENT_I) and np.all(out["merged"] == SENT_B)
        assert np.all(out["best"] == SENT_I) and np.all(out["post"] == SENT_F)
    assert lib.las_nbest_network_workspace_bytes(1, 2, 2, 4) > 0 and lib.las_nbest_network_workspace_bytes(0, 2, 2, 4) == 0


def test_same_bits_twice_permuted_and_alone():
    """one batch launched twice, with its utterances in another order (another place in the grid, other garbage around them), and one of its
    utterances as a batch of its own"""
    rng = np.random.RandomState(10)
    utts = [[list(rng.randint(0, 3, size=rng.randint(0, 90))) for _ in range(rng.randint(1, 7))] for _ in range(9)]
    weights = _weights(rng, utts)
    K, U, mb = 6, 90, 200
    a = _launch(utts, weights, K=K, U=U, max_bins=mb, seed=1)
    b = _launch(utts, weights, K=K, U=U, max_bins=mb, seed=1)
    _check(utts, weights, a)
    for key in ("cols", "nbins", "merged", "best"):
        assert np.array_equal(a[key], b[key])
    assert np.array_equal(_bits(a["post"]), _bits(b["post"]))
    perm = rng.permutation(len(utts))
    c = _launch([utts[i] for i in perm], [weights[i] for i in perm], K=K, U=U, max_bins=mb, seed=2)
    alone = _launch([utts[4]], [weights[4]], K=K, U=U, max_bins=mb, seed=3)
    for o, v, u in [(c, v, u) for v, u in enumerate(perm)] + [(alone, 0, 4)]:
        nh, B = len(utts[u]), a["nbins"][u]
        assert o["nbins"][v] == B and np.array_equal(a["merged"][u, :nh], o["merged"][v, :nh])
        assert np.array_equal(a["cols"][u, :nh, :B], o["cols"][v, :nh, :B]) and np.array_equal(a["best"][u, :B], o["best"][v, :B])
        assert np.array_equal(_bits(a["post"][u, :B]), _bits(o["post"][v, :B]))
