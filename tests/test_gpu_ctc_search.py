"""CTC-only decoding: las_ctc_frame_topk, las_ctc_greedy and las_ctc_beam_search through the C ABI against the numpy
restatement (tests/ctc_search_ref.py).  Integer results (argmax, candidate lists, greedy tokens, beam token lists, their order, nhyp)
are EQUAL; log-probabilities and scores are within 4x the largest difference between the restatement in float32 with the kernel's
operation order and in float64, measured on the CPU over the case list (ctc_search_ref.measured_tolerance) -- the factor covers the
device's expf / logf / log1pf against numpy's, a few ulp per logaddexp over at most 160 frames.  Every output buffer is filled with
sentinels (NaN in the float ones): what lies beyond T'_u, a length or nhyp[u] must keep them."""
import numpy as np
import pytest
import torch

import ctc_search_ref as R

pytestmark = pytest.mark.gpu
SENT = -7


def _tables(lm, w, corrupt=None):
    t = {k: np.array(v, copy=True) for k, v in lm.tables(w).items()}
    if corrupt is not None:
        corrupt(t)
    pad = lambda a: a if a.size else np.zeros(1, a.dtype)
    return t, {k: torch.as_tensor(np.ascontiguousarray(pad(a))).cuda() for k, a in t.items()}


def _run(z, lens, K, C, eos, lm=None, w=0.0, beta=0.0, tab=None, ws_bytes=None, expect_fail=None):
    """the three kernels over logits z [n, Tp, Vc] -> dict of numpy arrays (sentinels where nothing was written)"""
    from las import _hip
    lib = _hip.lib()
    n, Tp, Vc = z.shape
    V = Vc - 1
    dz = torch.as_tensor(np.ascontiguousarray(z, np.float32)).cuda()
    dl = torch.as_tensor(np.asarray(lens, np.int32)).cuda()
    i32 = dict(dtype=torch.int32, device="cuda")
    nanf = lambda *s: torch.full(s, float("nan"), device="cuda")
    o = dict(cand_tok=torch.full((n, Tp, C), SENT, **i32), cand_lp=nanf(n, Tp, C), blank_lp=nanf(n, Tp), best=torch.full((n, Tp), SENT, **i32),
             best_lp=nanf(n, Tp), g_tok=torch.full((n, Tp), SENT, **i32), g_len=torch.full((n,), SENT, **i32),
             g_score=torch.full((n,), float("nan"), dtype=torch.float64, device="cuda"), tokens=torch.full((n, K, Tp), SENT, **i32),
             lens=torch.full((n, K), SENT, **i32), totals=nanf(n, K), nhyp=torch.full((n,), SENT, **i32))
    p = _hip.p
    _hip.check(lib.las_ctc_frame_topk(p(dz), p(dl), n, Tp, Vc, C, p(o["cand_tok"]), p(o["cand_lp"]), p(o["blank_lp"]), p(o["best"]),
                                      p(o["best_lp"]), _hip.stream()), "las_ctc_frame_topk")
    _hip.check(lib.las_ctc_greedy(p(o["best"]), p(o["best_lp"]), p(dl), n, Tp, V, p(o["g_tok"]), p(o["g_len"]), p(o["g_score"]),
                                  _hip.stream()), "las_ctc_greedy")
    M = E = order = start = 0
    t = lambda k: None
    if lm is not None:
        if tab is None:
            tab = _tables(lm, w)[1]
        M, E, order, start = lm.num_nodes, lm.num_entries, lm.order, lm.step(0, R.SOS)
        t = lambda k: p(tab[k])
    need = lib.las_ctc_beam_workspace_bytes(n, Tp, K, C)
    ws = torch.zeros(max(need if ws_bytes is None else ws_bytes, 8), dtype=torch.uint8, device="cuda")
    rc = lib.las_ctc_beam_search(p(o["cand_tok"]), p(o["cand_lp"]), p(o["blank_lp"]), p(dl), n, Tp, V, K, C, eos, beta, t("child_off"),
                                 t("child_tok"), t("child_lp"), t("child_next"), t("bow"), t("bo"), t("uni_lp"), t("uni_next"), M, E, order,
                                 start, p(o["tokens"]), p(o["lens"]), p(o["totals"]), p(o["nhyp"]), p(ws),
                                 need if ws_bytes is None else ws_bytes, _hip.stream())
    if expect_fail is not None:
        assert rc < 0 and expect_fail in lib.las_last_error(), (rc, lib.las_last_error())
        return None
    _hip.check(rc, "las_ctc_beam_search")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _bits(out):
    return {k: v.tobytes() for k, v in out.items()}


def _check(out, u, T, want, K, lp_tol, sc_tol, what):
    """utterance u of a launch against the restatement's (summary, greedy, hyps, margin)"""
    s, (g_tok, g_score), hyps, _ = want
    assert np.array_equal(out["best"][u, :T], s["best"]), what
    assert np.array_equal(out["cand_tok"][u, :T], s["cand_tok"]), what
    for k in ("best_lp", "blank_lp", "cand_lp"):
        got, ref = out[k][u, :T].astype(np.float64), np.asarray(s[k], np.float64)
        fin = np.isfinite(ref) & (ref > R.LOGZERO)
        d = float(np.abs(got[fin] - ref[fin]).max()) if fin.any() else 0.0
        print(what, k, "max |device - float64|", d, "allowed", lp_tol)
        assert d <= lp_tol, (what, k, d, lp_tol)
        assert np.all(got[~fin] <= R.LOGZERO), (what, k)                 # (no mass is no mass on the device too)
    # what lies beyond T'_u keeps its sentinel
    assert np.all(out["best"][u, T:] == SENT) and np.all(out["cand_tok"][u, T:] == SENT)
    assert np.all(np.isnan(out["best_lp"][u, T:])) and np.all(np.isnan(out["blank_lp"][u, T:])) and np.all(np.isnan(out["cand_lp"][u, T:]))
    # greedy
    assert out["g_len"][u] == len(g_tok) and out["g_tok"][u, :len(g_tok)].tolist() == g_tok, what
    assert np.all(out["g_tok"][u, len(g_tok):] == SENT)
    if np.isfinite(g_score):
        print(what, "greedy score", out["g_score"][u], g_score, "allowed", sc_tol)
        assert abs(out["g_score"][u] - g_score) <= sc_tol, what
    # the beam: token lists, their order, nhyp; totals
    nh = int(out["nhyp"][u])
    got = [out["tokens"][u, k, :out["lens"][u, k]].tolist() for k in range(min(nh, K))]
    assert nh == len(hyps) and got == [h[0] for h in hyps], (what, nh, got[:4], [h[0] for h in hyps][:4])
    d = max([abs(float(out["totals"][u, k]) - hyps[k][1]) for k in range(nh)] + [0.0])
    print(what, "max |total - float64|", d, "allowed", sc_tol)
    assert d <= sc_tol, (what, d, sc_tol)
    for k in range(nh):
        assert np.all(out["tokens"][u, k, out["lens"][u, k]:] == SENT)
    assert np.all(out["tokens"][u, nh:] == SENT) and np.all(out["lens"][u, nh:] == SENT) and np.all(np.isnan(out["totals"][u, nh:]))


@pytest.mark.parametrize("name", [c["name"] for c in R.CASES])
def test_case_matches_restatement(name):
    """every case of the list: summary, greedy and beam against the float64 restatement; two launches give the same bits; a permuted
    batch gives permuted results"""
    from las.ngram import NgramLM
    case = next(c for c in R.CASES if c["name"] == name)
    lp_diff, sc_diff = R.measured_tolerance()
    lp_tol, sc_tol = 4.0 * lp_diff, 4.0 * sc_diff
    z, lens, V = R.case_logits(case), case["lens"], case["Vc"] - 1
    model = R.case_model(case)
    lm = NgramLM(model[0], model[1], V, R.SOS, R.EOS, 0) if model else None
    kw = dict(K=case["K"], C=case["C"], eos=R.eos_of(V), lm=lm, w=R.LM_WEIGHT, beta=case["beta"])
    out = _run(z, lens, **kw)
    want = R.run_case(name)
    for u, T in enumerate(lens):
        assert want[u][3] >= R.MARGIN
        _check(out, u, T, want[u], case["K"], lp_tol, sc_tol, "%s[%d]" % (name, u))
    assert _bits(_run(z, lens, **kw)) == _bits(out)
    perm = list(range(len(lens)))[::-1]
    pout = _run(z[perm], [lens[i] for i in perm], **kw)
    for i, u in enumerate(perm):
        for k in out:
            assert pout[k][i].tobytes() == out[k][u].tobytes(), (name, k, u)


def test_arranged_ties_at_the_cut_and_for_the_argmax():
    """equal logits where the candidate list is cut and for the frame's maximum (also -0 against +0, and across the lanes' register /
    memory split at class 5120): the lower id wins, the list stays in ascending id"""
    rng = np.random.RandomState(5)
    for Vc, C in ((3, 1), (3, 2), (31, 2), (31, 30), (5001, 32), (5001, 1), (300, 64), (6001, 32), (10241, 3)):
        V, T = Vc - 1, 6
        z = rng.randn(1, T, Vc).astype(np.float32)
        hi = np.float32(z.max() + 1.0)
        ids = np.unique(rng.randint(V, size=min(V, 2 * C + 3)))
        z[0, 0, ids] = hi                                               # more ties than the list holds: the lowest ids enter
        z[0, 1, :] = np.float32(0.25)                                   # everything ties, the blank too: argmax = class 0
        z[0, 2, [V - 1, V]] = hi                                        # the last token against the blank: the token wins
        z[0, 3, :] = np.float32(-1.0)
        z[0, 3, V - 1], z[0, 3, 0] = np.float32(0.0), np.float32(-0.0)  # -0 == +0: the lower id
        z[0, 4, V // 2:] = hi                                           # ties on both sides of the register / memory split
        z[0, 5, :] = -np.inf
        z[0, 5, V] = np.float32(1.0)                                    # only the blank has mass: the candidates tie at -inf
        out = _run(z, [T], K=2, C=C, eos=R.eos_of(V))
        s = R.frame_summary(z[0], T, C)
        assert np.array_equal(out["best"][0], s["best"]), (Vc, C, out["best"][0], s["best"])
        assert np.array_equal(out["cand_tok"][0], s["cand_tok"]), (Vc, C)
        assert s["best"][1] == 0 and s["best"][2] == V - 1 and s["best"][3] == 0 and s["best"][5] == V
        assert np.all(np.diff(out["cand_tok"][0], axis=1) > 0)


def _assert_beam(out, u, K, hyps, sc_tol, what):
    nh = int(out["nhyp"][u])
    got = [out["tokens"][u, k, :out["lens"][u, k]].tolist() for k in range(min(nh, K))]
    assert nh == len(hyps) and got == [h[0] for h in hyps], (what, nh, got, hyps)
    for k in range(nh):
        assert abs(float(out["totals"][u, k]) - hyps[k][1]) <= sc_tol, (what, k)
    assert np.all(out["tokens"][u, nh:] == SENT) and np.all(np.isnan(out["totals"][u, nh:]))


def test_reentry_keeps_one_node_per_prefix():
    """the hand-made re-entry case (tests/test_ctc_search_host.py shows what it is): a prefix leaves the beam and comes back while its
    descendant stays.  A search that made a second node for it would list the descendant's prefix twice"""
    z, K, C, eos = R.reentry_case()
    sc_tol = 4.0 * R.measured_tolerance()[1]
    out = _run(z[None], [z.shape[0]], K=K, C=C, eos=eos)
    hyps, margin = R.beam_search(R.frame_summary(z, z.shape[0], C), K, eos)
    assert margin >= R.MARGIN
    _assert_beam(out, 0, K, hyps, sc_tol, "re-entry")
    got = [tuple(out["tokens"][0, k, :out["lens"][0, k]]) for k in range(int(out["nhyp"][0]))]
    assert len(set(got)) == len(got)


def test_closed_prefixes_no_mass_columns_and_a_short_beam():
    """EOS closes a prefix (nothing follows it in any hypothesis); -inf and LOGZERO columns carry no mass; a beam that ends with fewer
    than K live entries reports them alone"""
    sc_tol = 4.0 * R.measured_tolerance()[1]
    rng = np.random.RandomState(11)                                     # (chosen on the CPU: every utterance keeps the margin, asserted below)
    V, T, K, C = 5, 9, 16, 5
    eos = R.EOS
    z = rng.randn(3, T, V + 1).astype(np.float32)
    z[0, 0:3, 3] += 3.0                                                 # utterance 0: a token, then EOS, then frames that still offer
    z[0, 3:5, eos] += 6.0                                               # every token: the closed prefixes take none of them
    z[0, 5:, V] += 2.0
    z[1, :, 0] = -np.inf                                                # utterance 1: a -inf column, a LOGZERO column (lse > 0: the
    z[1, :, 1] = np.float32(R.LOGZERO)                                  # float32 difference is at or below LOGZERO as well), and
    z[1, :, 4] += 3.0
    z[1, 5, :V] = -np.inf                                               # a frame where only the blank has mass
    z[2, :, :V] = -np.inf                                               # utterance 2: nothing but blank: the empty hypothesis alone
    z[2, :, V] = 1.0
    out = _run(z, [T, T, T], K=K, C=C, eos=eos)
    for u in range(3):
        hyps, margin = R.beam_search(R.frame_summary(z[u], T, C), K, eos)
        assert margin >= R.MARGIN
        _assert_beam(out, u, K, hyps, sc_tol, "utterance %d" % u)
        for toks, _ in hyps:
            assert eos not in toks[:-1]
            if u == 1:
                assert 0 not in toks and 1 not in toks
    assert any(h[0] and h[0][-1] == eos for h in R.beam_search(R.frame_summary(z[0], T, C), K, eos)[0])
    assert out["nhyp"][2] == 1 and out["lens"][2, 0] == 0 and out["totals"][2, 0] == pytest.approx(0.0, abs=1e-5)
    print("nhyp", out["nhyp"])


@pytest.mark.parametrize("order", [1, 3])
def test_ngram_tables_with_out_of_range_entries_are_clamped(order):
    """a node table whose child ranges, next and back-off entries point outside their tables: the walk is clamped as in
    las_ngram_step (csrc/ngram_trie.h), restated from the TABLES by ctc_search_ref.TableGain; the search equals the restatement"""
    import ngram_ref as G
    from las.ngram import NgramLM
    sc_tol = 4.0 * R.measured_tolerance()[1]
    rng = np.random.RandomState(40 + order)
    V, T, K, C = 30, 24, 8, 12
    lm = NgramLM(G.random_model(rng, V, order), order, V, R.SOS, R.EOS, 0)
    M, E = lm.num_nodes, lm.num_entries

    def corrupt(t):
        t["uni_next"][3], t["uni_next"][4] = M + 5, -2
        if E:
            t["child_next"][::3] = 2 ** 30
            t["child_next"][1::7] = -1
            t["bo"][2::4] = M
            t["bo"][5::9] = -3
            t["child_off"][M // 2] = -4
            t["child_off"][M // 3 + 1] = E + 100
    host, dev = _tables(lm, R.LM_WEIGHT, corrupt)
    z = (rng.randn(2, T, V + 1) * 2.0).astype(np.float32)
    out = _run(z, [T, T - 5], K=K, C=C, eos=R.EOS, lm=lm, w=R.LM_WEIGHT, tab=dev, beta=0.125)
    worst = np.inf
    for u, Tu in enumerate((T, T - 5)):
        gain = R.TableGain(host, M, E, order, lm.step(0, R.SOS))
        hyps, margin = R.beam_search(R.frame_summary(z[u], Tu, C), K, R.EOS, gain, 0.125)
        worst = min(worst, margin)
        assert margin >= R.MARGIN
        _assert_beam(out, u, K, hyps, sc_tol, "order %d utterance %d" % (order, u))
    plain = _run(z, [T, T - 5], K=K, C=C, eos=R.EOS, beta=0.125)
    assert _bits(plain)["tokens"] != _bits(out)["tokens"] or _bits(plain)["totals"] != _bits(out)["totals"]   # the LM was read


def test_refusals():
    """K = 65, C = 65, C > V, a short workspace, n-gram limits: refused on the host before any launch"""
    from las import _hip
    from las.ngram import NgramLM
    import ngram_ref as G
    lib = _hip.lib()
    z = np.zeros((1, 4, 101), np.float32)
    _run(z, [4], K=65, C=2, eos=2, expect_fail=b"K <=")
    _run(z, [4], K=1, C=2, eos=2, ws_bytes=8, expect_fail=b"workspace")
    need = lib.las_ctc_beam_workspace_bytes(1, 4, 4, 2)
    assert need > 0
    _run(z, [4], K=4, C=2, eos=2, ws_bytes=need - 1, expect_fail=b"workspace")
    zi = torch.zeros(4096, dtype=torch.int32, device="cuda")
    zf = torch.zeros(4096, device="cuda")
    p = _hip.p

    def topk(C, Vc=101):
        return lib.las_ctc_frame_topk(p(zf), p(zi), 1, 4, Vc, C, p(zi), p(zf), p(zf), p(zi), p(zf), _hip.stream())

    def beam(K=4, C=2, V=100, M=0, order=0, tab=None, ws=None):
        t = (lambda k: p(tab[k])) if tab is not None else (lambda k: None)
        w = torch.zeros(1 << 22, dtype=torch.uint8, device="cuda") if ws is None else ws
        return lib.las_ctc_beam_search(p(zi), p(zf), p(zf), p(zi), 1, 4, V, K, C, 2, 0.0, t("child_off"), t("child_tok"), t("child_lp"),
                                       t("child_next"), t("bow"), t("bo"), t("uni_lp"), t("uni_next"), M, 0, order, 0, p(zi), p(zi), p(zf),
                                       p(zi), p(w), w.numel(), _hip.stream())
    assert topk(65) < 0 and b"C <=" in lib.las_last_error()
    assert topk(3, Vc=3) < 0 and b"C <=" in lib.las_last_error()
    assert topk(-1) < 0
    assert beam(C=65) < 0 and b"C <=" in lib.las_last_error()
    assert beam(K=0) < 0 and b"K <=" in lib.las_last_error()
    assert beam(C=3, V=2) < 0 and b"C <=" in lib.las_last_error()
    lm = NgramLM(G.random_model(np.random.RandomState(0), 30, 2), 2, 30)
    tab = _tables(lm, 1.0)[1]
    assert beam(V=30, M=lm.num_nodes, order=7, tab=tab) < 0 and b"order" in lib.las_last_error()
    assert beam(V=30, M=(1 << 22) + 1, order=2, tab=tab) < 0 and b"nodes" in lib.las_last_error()
    assert beam(V=16385, M=lm.num_nodes, order=2, tab=tab) < 0 and b"V <=" in lib.las_last_error()
    assert beam(V=30, M=lm.num_nodes, order=2, tab=None) < 0 and b"null pointer" in lib.las_last_error()
    assert beam() == 0 and topk(2) == 0
    torch.cuda.synchronize()


def test_host_functions_match_the_c_abi():
    """las.ctc_search.frame_topk / greedy / beam_search (one upload, the launches, one read-back) give what the C ABI gave"""
    from las import ctc_search as CS
    from las.ngram import NgramLM
    case = next(c for c in R.CASES if c["name"] == "v30-k16-tri")
    z, lens, V = R.case_logits(case), case["lens"], case["Vc"] - 1
    model = R.case_model(case)
    lm = NgramLM(model[0], model[1], V, R.SOS, R.EOS, 0)
    out = _run(z, lens, K=case["K"], C=case["C"], eos=R.EOS, lm=lm, w=R.LM_WEIGHT, beta=case["beta"])
    dz = torch.as_tensor(z).cuda()
    summ = CS.frame_topk(dz, lens, case["C"])
    gr = CS.greedy(dz, lens)
    hy = CS.beam_search(dz, lens, case["K"], case["C"], R.EOS, lm, R.LM_WEIGHT, case["beta"], R.SOS)
    for u, T in enumerate(lens):
        for k in ("best", "best_lp", "blank_lp", "cand_tok", "cand_lp"):
            assert summ[u][k].tobytes() == out[k][u, :T].tobytes(), k
        assert gr[u][0] == out["g_tok"][u, :out["g_len"][u]].tolist() and gr[u][1] == out["g_score"][u]
        nh = int(out["nhyp"][u])
        assert [h[0] for h in hy[u]] == [out["tokens"][u, k, :out["lens"][u, k]].tolist() for k in range(nh)]
        assert [np.float32(h[1]) for h in hy[u]] == [out["totals"][u, k] for k in range(nh)]
    for bad in (dict(K=65), dict(C=65), dict(K=0)):
        with pytest.raises(ValueError):
            CS.beam_search(dz, lens, **dict(dict(K=4, C=4, eos_id=R.EOS), **bad))
