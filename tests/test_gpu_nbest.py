"""las_nbest_risk / las_nbest_confidence (include/las_hip.h K10g, csrc/nbest.hip) against the numpy restatement tests/nbest_ref.py.  The
contract fixes the arithmetic (integer tables, one back-trace rule, one fp32 product and one fp32 sum per slot in slot order), so EVERY
output is compared for EQUALITY: that is the bound the contract derives, not a measured one (the argument of test_gpu_ctc_align.py).
Outputs are pre-filled with a sentinel; padding tokens, absent slots' tokens and weights hold garbage (NaN weights)."""
import itertools

import numpy as np
import pytest
import torch

import helpers  # noqa: F401
import nbest_ref as R

pytestmark = pytest.mark.gpu
SENT_I, SENT_F, SENT_B = -77, 123.0, 55
U_CEILING = 1024                                                       # include/las_hip.h K10g


def _launch(utts, weights, K=None, U=None, pivot=None, ws_short=0, seed=0, chain=False):
    """utts[u] = the live hypotheses of utterance u, weights[u] their fp32 weights.  pivot None: las_nbest_risk alone; a list:
    las_nbest_confidence alone; chain: both, pick handed over on the device.  -> dict of return codes and host arrays"""
    from las import _hip
    rng = np.random.RandomState(1000 + seed)
    n = len(utts)
    K = max(1, max(len(h) for h in utts)) if K is None else K
    U = max(1, max((len(t) for h in utts for t in h), default=1)) if U is None else U
    tok = rng.randint(-5, 6000, size=(n, K, U)).astype(np.int32)        # garbage wherever nothing lives
    ln = rng.randint(0, U + 1, size=(n, K)).astype(np.int32)
    w = np.full((n, K), np.nan, np.float32)
    nh = np.zeros(n, np.int32)
    for u, hyps in enumerate(utts):
        nh[u] = len(hyps)
        w[u, :len(hyps)] = np.asarray(weights[u], np.float32)
        for k, t in enumerate(hyps):
            ln[u, k] = len(t)
            tok[u, k, :len(t)] = t
    d = lambda x: torch.as_tensor(x).cuda()
    d_tok, d_len, d_nh, d_w = d(tok), d(ln), d(nh), d(w)
    i32 = dict(dtype=torch.int32, device="cuda")
    dist, risk, pick = torch.full((n, K, K), SENT_I, **i32), torch.full((n, K), SENT_F, device="cuda"), torch.full((n,), SENT_I, **i32)
    match = torch.full((n, K, U), SENT_B, dtype=torch.int8, device="cuda")
    conf = torch.full((n, U), SENT_F, device="cuda")
    lib = _hip.lib()
    out = dict(n=n, K=K, U=U)
    if pivot is None or chain:
        out["rc_risk"] = lib.las_nbest_risk(_hip.p(d_tok), _hip.p(d_len), _hip.p(d_nh), _hip.p(d_w), n, K, U, _hip.p(dist), _hip.p(risk),
                                            _hip.p(pick), _hip.stream())
    if pivot is not None or chain:
        d_pv = pick if chain else torch.tensor(pivot, **i32)
        nbytes = lib.las_nbest_workspace_bytes(n, K, U)
        ws = torch.zeros(max(nbytes, 256), dtype=torch.uint8, device="cuda")
        out["rc_conf"] = lib.las_nbest_confidence(_hip.p(d_tok), _hip.p(d_len), _hip.p(d_nh), _hip.p(d_w), _hip.p(d_pv), n, K, U,
                                                  _hip.p(match), _hip.p(conf), _hip.p(ws), nbytes - ws_short, _hip.stream())
    torch.cuda.synchronize()
    out.update(dist=dist.cpu().numpy(), risk=risk.cpu().numpy(), pick=pick.cpu().numpy(), match=match.cpu().numpy(), conf=conf.cpu().numpy())
    return out


def _bits(x):
    return np.asarray(x, np.float32).view(np.int32)


_REF = {}


def _ref_risk(hyps, w):
    """the restatement's (dist, risk, pick) of one utterance, computed once per distinct input"""
    key = (tuple(map(tuple, hyps)), _bits(w).tobytes())
    if key not in _REF:
        _REF[key] = R.risk(hyps, w)
    return _REF[key]


def _check_risk(utts, weights, out):
    assert out["rc_risk"] == 0
    for u, hyps in enumerate(utts):
        nh = len(hyps)
        dist, risk, pick = _ref_risk(hyps, weights[u])
        assert np.array_equal(out["dist"][u, :nh, :nh], dist), (u, out["dist"][u, :nh, :nh], dist)
        assert np.array_equal(_bits(out["risk"][u, :nh]), _bits(risk)), (u, out["risk"][u, :nh], risk)
        assert out["pick"][u] == pick, (u, out["pick"][u], pick)
        # absent slots: nothing written
        assert np.all(out["dist"][u, nh:, :] == SENT_I) and np.all(out["dist"][u, :, nh:] == SENT_I)
        assert np.all(out["risk"][u, nh:] == SENT_F)


def _check_conf(utts, weights, pivot, out):
    assert out["rc_conf"] == 0
    for u, hyps in enumerate(utts):
        nh = len(hyps)
        match, conf = R.confidence(hyps, weights[u], int(pivot[u]))
        if match is None:
            assert np.all(out["match"][u] == SENT_B) and np.all(out["conf"][u] == SENT_F)
            continue
        La = len(hyps[int(pivot[u])])
        assert np.array_equal(out["match"][u, :nh, :La], match), (u, out["match"][u, :nh, :La], match)
        assert np.all(out["match"][u, int(pivot[u]), :La] == 1)
        assert np.array_equal(_bits(out["conf"][u, :La]), _bits(conf)), (u, out["conf"][u, :La], conf)
        assert np.all(out["match"][u, :, La:] == SENT_B) and np.all(out["match"][u, nh:] == SENT_B) and np.all(out["conf"][u, La:] == SENT_F)


def _weights(rng, utts):
    out = []
    for hyps in utts:
        w = rng.uniform(0.01, 1.0, size=len(hyps))
        out.append((w / max(w.sum(), 1e-9)).astype(np.float32))
    return out


def _binary_strings(max_len=4):
    return [list(s) for L in range(max_len + 1) for s in itertools.product((0, 1), repeat=L)]


def test_every_pair_of_binary_strings():
    """all 31 x 31 pairs of the strings over {0, 1} up to length 4: one utterance of K = 31 gives every distance; 31 more utterances,
    each with another string as the pivot, give every alignment -- every tie of the back-trace rule"""
    strs = _binary_strings()
    assert len(strs) == 31
    rng = np.random.RandomState(1)
    utts = [strs] * 31
    weights = _weights(rng, utts)
    _check_risk(utts[:1], weights[:1], _launch(utts[:1], weights[:1]))
    pivot = list(range(31))
    _check_conf(utts, weights, pivot, _launch(utts, weights, pivot=pivot))


@pytest.mark.parametrize("vocab", [3, 5000])
def test_chunk_and_carry_edges(vocab):
    """lengths {0, 1, 63, 64, 65, 127, 128, 129} in all combinations (0 vs 0 and 1 vs 129 among them): the edges of the 64-column chunks
    and of the boundary column carried between them, and of the 16-row direction words; vocabulary 3 makes dense ties, 5000 none.  Two
    hypotheses of every length in one utterance of K = 16 give all length pairs; every slot is the pivot once"""
    rng = np.random.RandomState(vocab)
    lens = [0, 1, 63, 64, 65, 127, 128, 129]
    hyps = [list(rng.randint(0, vocab, size=L)) for L in lens + lens]
    utts = [hyps] * 16
    weights = _weights(rng, utts)
    _check_risk(utts[:1], weights[:1], _launch(utts[:1], weights[:1]))
    pivot = list(range(16))
    _check_conf(utts, weights, pivot, _launch(utts, weights, pivot=pivot))


def test_repeats_identical_and_disjoint():
    a, b = 7, 9
    utts = [[[a, a, a, a], [a, a]], [[a, b, a, b], [b, a, b, a]], [[a, a], [a, a, a, a]],
            [[3, 4, 5, 6, 7]] * 4, [[1, 2, 3], [4, 5, 6], [7, 8, 9, 10]], [[5] * 70, [5] * 3, [5] * 64]]
    rng = np.random.RandomState(3)
    weights = _weights(rng, utts)
    out = _launch(utts, weights)
    _check_risk(utts, weights, out)
    assert out["dist"][0, 0, 1] == 2 and out["dist"][1, 0, 1] == 2 and np.all(out["dist"][3, :4, :4] == 0) and out["dist"][4, 0, 2] == 4
    for pv in (0, 1):
        pivot = [pv] * len(utts)
        o = _launch(utts, weights, pivot=pivot)
        _check_conf(utts, weights, pivot, o)
    # aaaa against aa: the rule walks the diagonal first, so the LAST two a's are the matched ones
    o = _launch(utts, weights, pivot=[0] * len(utts))
    assert list(o["match"][0, 1, :4]) == [0, 0, 1, 1]
    assert np.all(o["match"][3, :4, :5] == 1) and np.all(o["match"][4, 1:3, :3] == 0)


@pytest.mark.parametrize("K", [1, 2, 16, 64])
def test_slot_counts(K):
    """K = 1 (no pair at all), 2, 16 (the search's beam), 64 (every lane of the risk kernel); three utterances with nhyp = K, K // 2, 1"""
    rng = np.random.RandomState(K)
    utts = [[list(rng.randint(0, 4, size=rng.randint(0, 12))) for _ in range(nh)] for nh in (K, max(1, K // 2), 1)]
    weights = _weights(rng, utts)
    out = _launch(utts, weights, K=K, chain=True)
    _check_risk(utts, weights, out)
    _check_conf(utts, weights, out["pick"], out)


def test_mixed_nhyp_and_no_pivot():
    """nhyp = 0, 1, K across the utterances of one batch: pick = -1 and nothing written for nhyp = 0; pivot = -1 (and a pivot that points at
    an absent slot) writes nothing"""
    rng = np.random.RandomState(6)
    K = 5
    utts = [[], [[4, 5, 6]], [list(rng.randint(0, 3, size=L)) for L in (3, 0, 7, 7, 2)], [], [[], []]]
    weights = _weights(rng, utts)
    out = _launch(utts, weights, K=K, chain=True)
    _check_risk(utts, weights, out)
    assert out["pick"][0] == -1 and out["pick"][3] == -1 and out["pick"][1] == 0
    assert np.all(out["dist"][0] == SENT_I) and np.all(out["risk"][0] == SENT_F)
    _check_conf(utts, weights, out["pick"], out)
    pivot = [-1, -1, 1, 0, 2]                                           # utterance 2: the empty hypothesis as the pivot; 3, 4: absent slots
    o = _launch(utts, weights, K=K, pivot=pivot)
    _check_conf(utts, weights, pivot, o)
    assert np.all(o["match"][[0, 1, 3, 4]] == SENT_B) and np.all(o["conf"] == SENT_F)


def test_risk_ties_follow_the_rule():
    """equal weights over a symmetric set: [a], [b], [c] are all at distance 1 from each other -> equal risks, the lowest index wins;
    with a larger weight on slot 2 the risks of 0 and 1 tie below 2's ... and so on, as worked out in the comments"""
    q = np.float32(0.25)
    utts = [[[1], [2], [3], [4]],                                      # risks all 0.75: pick 0
            [[1], [2], [3], [4]],                                      # w = (.2, .2, .4, .2): risk 0.8, 0.8, 0.6, 0.8: pick 2
            [[1, 2], [1, 3], [1, 2], [1, 3]],                          # w = (.2, .3, .2, .3): risk 0.6, 0.4, 0.6, 0.4: 1 and 3 tie entirely: pick 1
            [[1, 2], [1, 3], [1, 2], [1, 3]],                          # w = (.25, .25, .25, .25): all 0.5: pick 0
            [[9], [8], [9], [8]]]                                      # w = (.1, .4, .4, .1): risk .5 each: the larger w: 1 and 2 tie: pick 1
    weights = [[q] * 4, [0.2, 0.2, 0.4, 0.2], [0.2, 0.3, 0.2, 0.3], [q] * 4, [0.1, 0.4, 0.4, 0.1]]
    weights = [np.asarray(w, np.float32) for w in weights]
    out = _launch(utts, weights)
    _check_risk(utts, weights, out)
    assert list(out["pick"][[0, 1, 3]]) == [0, 2, 0]
    r = out["risk"][4, :4]
    assert r[0] == r[1] == r[2] == r[3] and out["pick"][4] == 1
    r = out["risk"][2, :4]
    assert r[1] == r[3] and out["pick"][2] == 1


def test_one_pair_at_the_ceiling():
    """U = 1024: 16 column chunks, 64 direction row blocks, the back-trace staging two blocks at a time"""
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
    utts = [[a, b]]
    weights = [np.asarray([0.6, 0.4], np.float32)]
    out = _launch(utts, weights, chain=True)
    assert out["U"] == U_CEILING
    _check_risk(utts, weights, out)
    _check_conf(utts, weights, out["pick"], out)
    o = _launch(utts, weights, pivot=[1])
    _check_conf(utts, weights, [1], o)


def test_refusals():
    """U = 1025, K = 65 and a workspace short by one byte: a non-zero status, a las_last_error text, untouched outputs"""
    from las import _hip
    lib = _hip.lib()
    utts, weights = [[[1, 2], [1]]], [np.asarray([0.5, 0.5], np.float32)]
    for kw, text in ((dict(U=U_CEILING + 1), b"U=1025"), (dict(K=65), b"K <= 64"), (dict(ws_short=1), b"workspace too small")):
        out = _launch(utts, weights, chain=True, **kw)
        assert out["rc_conf"] != 0 and text in lib.las_last_error(), (out["rc_conf"], lib.las_last_error())
        assert np.all(out["match"] == SENT_B) and np.all(out["conf"] == SENT_F)
        if "ws_short" not in kw:
            assert out["rc_risk"] != 0
            assert np.all(out["dist"] == SENT_I) and np.all(out["risk"] == SENT_F) and np.all(out["pick"] == SENT_I)
    assert lib.las_nbest_workspace_bytes(1, 2, 2) > 0 and lib.las_nbest_workspace_bytes(0, 2, 2) == 0


def test_same_bits_twice_and_permuted():
    """one batch launched twice, and with its utterances in another order (another place in the grid, other garbage around them)"""
    rng = np.random.RandomState(10)
    utts = [[list(rng.randint(0, 3, size=rng.randint(0, 90))) for _ in range(rng.randint(1, 7))] for _ in range(9)]
    weights = _weights(rng, utts)
    K, U = 6, 90
    a = _launch(utts, weights, K=K, U=U, chain=True, seed=1)
    b = _launch(utts, weights, K=K, U=U, chain=True, seed=1)
    _check_risk(utts, weights, a)
    _check_conf(utts, weights, a["pick"], a)
    for key in ("dist", "pick", "match"):
        assert np.array_equal(a[key], b[key])
    for key in ("risk", "conf"):
        assert np.array_equal(_bits(a[key]), _bits(b[key]))
    perm = rng.permutation(len(utts))
    c = _launch([utts[i] for i in perm], [weights[i] for i in perm], K=K, U=U, chain=True, seed=2)
    for v, u in enumerate(perm):
        nh = len(utts[u])
        La = len(utts[u][a["pick"][u]])
        assert np.array_equal(a["dist"][u, :nh, :nh], c["dist"][v, :nh, :nh]) and a["pick"][u] == c["pick"][v]
        assert np.array_equal(_bits(a["risk"][u, :nh]), _bits(c["risk"][v, :nh]))
        assert np.array_equal(a["match"][u, :nh, :La], c["match"][v, :nh, :La]) and np.array_equal(_bits(a["conf"][u, :La]), _bits(c["conf"][v, :La]))


def test_python_layer_on_a_real_nbest_list():
    """las.nbest on the N-best lists of one small synthetic decode_batch (3 utterances, beam 4) equals the restatement; pick handed over
    on the device gives what pick read back and uploaded again gives"""
    import test_gpu_ctc_decode as D
    from las import nbest as NB
    args, p0, bs = D._model("pblstm", "lstm", enc_units=16, ctc=False, ctc_decode_weight=0.0)
    results = bs.decode_batch(None, D._utts(args))
    token_lists, scores, lens = NB.hypotheses(results, 2)
    assert any(len(t) > 1 for t in token_lists)
    for r, tl, sc in zip(results, token_lists, scores):
        assert len(tl) == len(r) and sc == [float(b.log_prob) for b in reversed(r)]
        assert all(2 not in t for t in tl)
    weights = [NB.posteriors(s, l) for s, l in zip(scores, lens)]
    for w in weights:
        assert w.dtype == np.float32 and (len(w) == 0 or int(np.argmax(w)) == 0)    # best first = the search's last-ranked
    dist, risk, pick = NB.consensus(token_lists, weights)
    for u, hyps in enumerate(token_lists):
        d, r, p = R.risk(hyps, weights[u])
        assert np.array_equal(dist[u], d) and np.array_equal(_bits(risk[u]), _bits(r)) and pick[u] == p
    conf, match = NB.token_confidence(token_lists, weights, pick)
    for u, hyps in enumerate(token_lists):
        m, c = R.confidence(hyps, weights[u], pick[u])
        if m is None:
            assert conf[u] is None and match[u] is None
            continue
        assert np.array_equal(match[u], m) and np.array_equal(_bits(conf[u]), _bits(c))
    d2, r2, p2, c2, m2 = NB.consensus_confidence(token_lists, weights)
    assert p2 == pick
    for u in range(len(token_lists)):
        assert np.array_equal(d2[u], dist[u]) and np.array_equal(_bits(r2[u]), _bits(risk[u]))
        if conf[u] is None:
            assert c2[u] is None
        else:
            assert np.array_equal(_bits(c2[u]), _bits(conf[u])) and np.array_equal(m2[u], match[u])
