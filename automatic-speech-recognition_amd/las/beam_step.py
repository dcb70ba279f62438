"""las.beam_step -- the parts of one step of BeamSearch.decode_batch: loop state, state-row registry, and the launches of a step in their
order (Speller, LM, scorers, pruning).  Every part has a `name` (its key in last_timing["parts_us"]) and a `launch()` with the same
arguments every step: all of them read the DEVICE step counter, so a step can be captured into a HIP graph and replayed."""
import collections
import ctypes

import numpy as np
import torch

from las import _hip

# the sizes of one search: n utterances x beam = N hypothesis rows, Tp encoder frames (the longest utterance's), Umax steps, and the model's
Geometry = collections.namedtuple("Geometry", "dev n beam N Tp Hd Umax V A NL D E lstm prec")


class StateRows(object):
    """The tensors whose rows follow their hypotheses through the gather of las_beam_loop_step.  Slot order of a search: per decoder layer h
    (then c for an LSTM), the alignment, the LM's state, CTC, hotwords, n-gram, coverage."""

    def __init__(self):
        self.pairs = []

    def add(self, src, dst):                # dst[row] = src[src_row[row]]: what the step wrote -> what the next step reads; returns the slot
        self.pairs.append((src, dst))
        return len(self.pairs) - 1

    def write(self, ba):
        if len(self.pairs) > 16:
            raise ValueError("decode_batch: %d state tensors follow the hypotheses (decoder and LM state, alignment, CTC, hotword and "
                             "n-gram LM state); las_beam_loop_step gathers at most 16" % len(self.pairs))
        ba.ntens = len(self.pairs)
        for k, (src, dst) in enumerate(self.pairs):
            ba.state_in[k], ba.state_out[k], ba.state_width[k] = src.data_ptr(), dst.data_ptr(), src.shape[-1]


class LoopState(object):
    """The device-resident loop tensors of one search and the las_beam_loop_args `ba` that holds their addresses (whoever uses `ba` holds
    this object).  Its launch is the pruning: files alphas_cur under the device step counter, prunes, gathers, advances the counter."""
    name = "beam"
    POINTERS = ("score", "length", "nlive", "nsel", "done", "dec_step", "step", "hist_parent", "hist_token", "hist_slot", "hist_score",
                "hist_n", "sel_t", "sel_j", "src_row", "next_token")

    def __init__(self, g, dec_steps, start_id, end_id, topn):
        dev, n, beam, N, Tp, Umax = g.dev, g.n, g.beam, g.N, g.Tp, g.Umax
        i32 = dict(dtype=torch.int32, device=dev)
        self.g, self.selcap = g, 3 * beam
        self.score, self.length = torch.zeros(n, beam, device=dev), torch.zeros(n, beam, **i32)
        self.nlive, self.nsel, self.done = torch.full((n,), beam, **i32), torch.zeros(n, **i32), torch.zeros(n, **i32)
        self.dec_step = torch.tensor(dec_steps, **i32)
        self.step = torch.zeros(1, **i32)                           # the device step counter
        self.hist_parent, self.hist_token, self.hist_slot = (torch.zeros(Umax, n, beam, **i32) for _ in range(3))
        self.hist_score, self.hist_n = torch.zeros(Umax, n, beam, device=dev), torch.zeros(Umax, n, **i32)
        self.sel_t, self.sel_j = torch.zeros(n, self.selcap, **i32), torch.zeros(n, self.selcap, **i32)
        self.src_row = torch.zeros(n, beam, **i32)
        self.next_token = torch.full((N,), start_id, **i32)
        self.alphas_hist = torch.zeros(Umax + 1, N, Tp, device=dev)      # [Umax] stays zero: item 0 of every hypothesis' att
        self.align_prev = torch.zeros(N, Tp, device=dev)
        self.alphas_cur = torch.zeros(N, Tp, device=dev)                 # the step's alignments, filed under the DEVICE step counter
        ba = self.ba = _hip.BeamLoopArgs()
        for name in self.POINTERS:
            setattr(ba, name, getattr(self, name).data_ptr())
        ba.nutt, ba.beam, ba.V, ba.Umax, ba.selcap, ba.topn, ba.start_id, ba.end_id = n, beam, g.V, Umax, self.selcap, topn, start_id, end_id
        ba.file_in, ba.file_out, ba.file_width = self.alphas_cur.data_ptr(), self.alphas_hist.data_ptr(), Tp

    def words(self):                        # of a scorer's launch: the tokens entering the step, the step counter, liveness, the step bounds
        return _hip.p(self.next_token), _hip.p(self.step), _hip.p(self.nlive), _hip.p(self.done), _hip.p(self.dec_step), self.g.Umax, _hip.stream()

    def launch(self):
        _hip.check(_hip.lib().las_beam_loop_step(ctypes.byref(self.ba), _hip.stream()), "las_beam_loop_step")


class SpellerStep(object):
    """The fused Speller step for all rows (las_speller_fwd, U = 1): slot 0 of hs / cs = state entering the step, slot 1 = state leaving
    it.  Long form: the call ends with its own logits.  Short form (speed mode, one LSTM layer, no scorer): the call stops after its cell
    (LAS_SPELLER_NO_LOGITS: attention rows + ONE cell launch) and the vocabulary projection -- the Speller's output layer and, concatenated
    along K, the LM's softmax layer -- happens inside las_beam_loop_step: 5 launches per step instead of 8."""
    name = "speller"

    def __init__(self, search, g, loop, rows, enc_u, keys_u, enc_lens, lm, ng, ctx, lam):
        from las.las import _alloc_bufs, _fill_fwd_args
        sp, a, dev = search.speller, search.args, g.dev
        N, Tp, Hd, A, D, NL, V_, E_, beam = g.N, g.Tp, g.Hd, g.A, g.D, g.NL, g.V, g.E, g.beam
        self.g, self.loop, self.enc_u, self.keys_u, self._tiled = g, loop, enc_u, keys_u, None
        P = sp._params()
        Pd = {k: (v.detach() if torch.is_tensor(v) else [t.detach() for t in v]) for k, v in P.items()}
        self.enc_len = torch.tensor(np.repeat(np.asarray(enc_lens, np.float64), beam)).to(torch.int32).to(dev)
        dims = sp._dims(N, Tp, 1)
        bufs = self.bufs = _alloc_bufs(dims, dev)
        bufs["hs"].zero_()
        if g.lstm:
            bufs["cs"].zero_()
        self.tokens_out = torch.zeros(1, N, dtype=torch.int32, device=dev)
        fa = self.fa = _hip.SpellerFwdArgs()
        self._keep = _fill_fwd_args(fa, dims, Pd, enc_u, keys_u, self.enc_len, loop.next_token, self.tokens_out, bufs, True, 0, keep_state0=True,
                                    align0=loop.align_prev)
        ws = _hip.workspace(dev, _hip.lib().las_speller_workspace_bytes(N, Tp, Hd, A, D, NL, E_, V_, 1, dims["cell"]), "speller")
        fa.ws, fa.ws_bytes = ws.data_ptr(), ws.numel()
        fa.alphas = loop.alphas_cur.data_ptr()
        # rows u beam .. (u + 1) beam - 1 are the hypotheses of utterance u (same enc / keys): the row launches keep them on one XCD
        fa.row_group = beam if search.xcd_local_rows else 0
        self.logits = bufs["logits"][0]                                                 # [N, V]
        self.register(rows, bufs, NL, g.lstm, loop)
        # (no short form with a scorer that adds to the logits: they are placed between the materialised logits and the pruning launch; the
    #  coverage scorer adds to the rows' running sums instead and is not considered here)
        self.fused = (ng is None and ctx is None and lam == 0 and g.prec == _hip.PREC_BF16 and g.lstm and NL == 1 and search.fuse_projection and
                      D % 32 == 0 and (E_ + Hd + D) % 32 == 0 and ((beam + 15) // 16) * ((V_ + 15) // 16) <= 8 and
                      (lm is None or (lm.lm.hidden_size % 32 == 0 and "packs" in lm.plan)))
        # ONE operand block per utterance (frames past T'_u are masked) where the reference feeds np.tile(h), a copy per hypothesis
        # (las/beam_search.py:216; 54 MB per step at 256 rows, r5_decode_pmc.json): the short form's row kernels take the utterance's block
        # (LAS_SPELLER_SHARED_OPERANDS); the tiled copies are made for kernel families that index per row.
        shared = self.fused and search.shared_operands and search.xcd_local_rows
        if not shared:
            fa.enc, fa.keys = (t.data_ptr() for t in self.tiled())
        if self.fused:
            Wcat, bcat = Pd["Wv"].contiguous(), Pd["bv"].clone()
            if lm is not None:
                Wcat = lm.append_softmax(Wcat, bcat)
            Wcat = Wcat.contiguous()
            self._proj = (_hip.skinny_pack(Wcat, Wcat.shape[0], V_), bcat.contiguous())
            fa.flags |= _hip.SPELLER_NO_LOGITS
            if shared:
                fa.flags |= _hip.SPELLER_SHARED_OPERANDS     # enc / keys: one block per utterance (fa.row_group = beam rows share it)
            if search.share_rows_from and N >= search.share_rows_from and beam % 4 == 0 and a.mode == "add":
                fa.flags |= _hip.SPELLER_ROWS_SHARE4         # rows 4g .. 4g+3 are hypotheses of ONE utterance: same enc / keys / length
            ba = loop.ba
            ba.proj_w, ba.proj_b = self._proj[0].data_ptr(), self._proj[1].data_ptr()
            ba.proj_h0, ba.proj_k0 = bufs["hs"][NL - 1, 1].data_ptr(), D
            ba.proj_h1, ba.proj_k1 = None, (lm.lm.hidden_size if lm is not None else 0)

    @staticmethod
    def register(rows, bufs, NL, lstm, loop):
        for l in range(NL):
            rows.add(bufs["hs"][l, 1], bufs["hs"][l, 0])
            if lstm:
                rows.add(bufs["cs"][l, 1], bufs["cs"][l, 0])
        rows.add(loop.alphas_cur, loop.align_prev)

    def tiled(self):                        # the per-row copies [N, Tp, .] of the encoder rows and keys (made once, on demand)
        if self._tiled is None:
            self._tiled = tuple(t.repeat_interleave(self.g.beam, 0) for t in (self.enc_u, self.keys_u))
        return self._tiled

    def launch(self):
        fa, lib = self.fa, _hip.lib()
        rc = lib.las_speller_fwd(ctypes.byref(fa), _hip.stream())
        if rc < 0 and self.fused and not (fa.flags & _hip.SPELLER_REUSE_PREP):
            # the library refuses the short form for this geometry (it needs its prefetching row kernels): the long form it is
            self.fused = False
            fa.flags &= ~(_hip.SPELLER_NO_LOGITS | _hip.SPELLER_ROWS_SHARE4 | _hip.SPELLER_SHARED_OPERANDS)
            fa.enc, fa.keys = (t.data_ptr() for t in self.tiled())       # (the long form's kernel families index enc / keys per row)
            fa.companion = None
            self.loop.ba.proj_w = None
            rc = lib.las_speller_fwd(ctypes.byref(fa), _hip.stream())
        _hip.check(rc, "las_speller_fwd")
        fa.flags |= _hip.SPELLER_REUSE_PREP      # enc / keys / weights are fixed for the search: their bf16 copies are made once


class LmFusion(object):
    """Shallow fusion of the char RNNLM: its recurrent state, the cells of a step and its softmax layer -- a product on top of the logits
    in the long form, rows of the pruning launch's concatenated projection in the short form.  Evident intent of the (syntactically broken) branch at las/beam_search.py:109-116,
    131-135: LM ids = LAS ids - 2, SOS (-> -1) fed as id 0; logits[:, 2:] += lm_weight * lm_logits."""
    name = "lm"

    def __init__(self, lm, weight, g, loop, state_copies):
        self.lm, self.g, self.loop = lm, g, loop
        self.plan = lm.fusion_plan(np.float32(weight))
        N, Hl, dev = g.N, lm.hidden_size, g.dev
        self.c = [torch.zeros(N, Hl, device=dev) for _ in range(lm.num_layers)]
        self.h = [torch.zeros(N, Hl, device=dev) for _ in range(lm.num_layers)]
        # bf16 copies of the recurrent state: from 384 rows on the cells read them -- and the layer below's copy -- instead of converting the
        # fp32 rows while staging them (half the bytes through a CU that is bound by its ingest); the copies follow their hypotheses as rows of
        # H / 2 floats INSTEAD of the fp32 h rows, which nobody reads then.  Bit-identical: the copy is the staging's own rounding.
        twins = state_copies and g.prec == _hip.PREC_BF16 and lm.twins_ok(self.plan, N)
        self.hb = [torch.zeros(N, Hl, dtype=torch.bfloat16, device=dev) for _ in range(lm.num_layers)] if twins else None
        self.layer0 = self.layer0_hb = self.held = self.speller = None

    def register(self, rows):               # (the inputs of these slots are re-pointed every step: the cells write fresh tensors)
        if self.hb is not None:
            self.k_c = [rows.add(c, c) for c in self.c]
            self.k_h = [rows.add(hb.view(torch.float32), hb.view(torch.float32)) for hb in self.hb]
        else:
            slots = [(rows.add(c, c), rows.add(h, h)) for c, h in zip(self.c, self.h)]
            self.k_c, self.k_h = [s[0] for s in slots], [s[1] for s in slots]

    def append_softmax(self, Wcat, bcat):   # the short form's projection: the pre-scaled softmax kernel under the Speller's, at its token columns
        Wl = torch.zeros(self.lm.hidden_size, self.g.V, device=self.g.dev)
        Wl[:, 2:2 + self.lm.vocab_size] = self.plan["sw"]
        bcat[2:2 + self.lm.vocab_size] += self.plan["sb"]
        return torch.cat([Wcat, Wl], 0)

    def attach(self, rows, speller):
        """short form: the first layer depends on the tokens only and rides with the Speller's cell as the second problem of one grid"""
        self.register(rows)
        self.speller = speller
        if not speller.fused:
            return
        N, Hl, dev = self.g.N, self.lm.hidden_size, self.g.dev
        lm0 = (torch.empty(N, Hl, device=dev), torch.empty(N, Hl, device=dev))
        lm0_hb = torch.empty(N, Hl, dtype=torch.bfloat16, device=dev) if self.hb is not None else None
        self._lm0_args = self.lm.first_cell_args(self.plan, self.loop.next_token, 2, self.c[0], self.h[0], lm0[0], lm0[1],
                                                 hb_prev=self.hb[0] if self.hb is not None else None, hb_out=lm0_hb)
        if self._lm0_args is not None:
            speller.fa.companion = ctypes.pointer(self._lm0_args)
            self.layer0, self.layer0_hb = lm0, lm0_hb

    def launch(self):
        lm, ba, sp = self.lm, self.loop.ba, self.speller
        layer0 = self.layer0 if sp.fused else None
        tw = {"prev": self.hb, "layer0": self.layer0_hb if layer0 is not None else None} if self.hb is not None else None
        cs_new, hs_new = lm.step_fused(self.plan, self.loop.next_token, self.c, self.h, sp.logits, 2, id_shift=2, project=False, layer0=layer0, twins=tw)
        follow = tw["new"] if tw is not None else hs_new
        for l in range(lm.num_layers):
            ba.state_in[self.k_c[l]], ba.state_in[self.k_h[l]] = cs_new[l].data_ptr(), follow[l].data_ptr()
        if sp.fused:
            ba.proj_h1 = hs_new[-1].data_ptr()
        else:
            lm.project_fused(self.plan, hs_new[-1], sp.logits, 2)
        self.held = (cs_new, hs_new, follow)                                  # alive until the gather has been enqueued


class Scorer(object):
    """A per-step scorer: ONE launch that reads the device step counter, advances every live row's state from its gathered parent `par`
    into `cur` and adds its term to the scores the pruning ranks; `cur` follows its hypotheses through the gather like the recurrent
    state.  Launch order coverage -> n-gram -> CTC -> hotwords: the n-gram adds to the logits in front of the CTC bank cut, the hotwords to
    what the pruning ranks, the coverage scorer to the rows' running sums.  A subclass names the C entry point and gives the arguments in front of (par, cur, width, the loop words)."""
    name = entry = None

    def __init__(self, g, loop, rows, width, *head):
        self.loop, self.width, self.head = loop, width, head
        self.par, self.cur = torch.zeros(g.N, width, device=g.dev), torch.zeros(g.N, width, device=g.dev)
        rows.add(self.cur, self.par)

    def launch(self):
        _hip.check(getattr(_hip.lib(), self.entry)(*self.head, _hip.p(self.par), _hip.p(self.cur), self.width, *self.loop.words()), self.entry)


class CtcScorer(Scorer):
    """Joint CTC-attention: las_ctc_prefix_step advances every live row's CTC state (r^n, r^b, psi, last label) and writes the
    joint scores of the row's candidates into `joint`, which the pruning ranks instead of the logits."""
    name, entry = "ctc", "las_ctc_prefix_step"

    def __init__(self, g, loop, rows, ctc_lp, enc_lens, logits, lam, end_id):
        assert ctc_lp is not None and ctc_lp.shape == (g.n, g.V + 1, g.Tp), "decode_batch: the encoder stage made no CTC log-probabilities"
        self.joint = torch.zeros(g.N, g.V, device=g.dev)
        self.keep = (ctc_lp, torch.tensor([int(x) for x in enc_lens], dtype=torch.int32, device=g.dev), logits)
        Scorer.__init__(self, g, loop, rows, 4 * ((2 * g.Tp + 2 + 3) // 4), _hip.p(ctc_lp), _hip.p(self.keep[1]), g.n, g.beam, g.Tp, g.V, end_id,
                        _hip.p(logits), _hip.p(self.joint), lam)


class BiasScorer(Scorer):
    """Contextual biasing: las_bias_step advances every live row's trie node and adds the candidates' gains to `scores` (the
    logits, or the CTC scorer's `joint`), in place.  Rows of 4 floats (the node is the first): a row of one float would take every state
    tensor of the gather off its 16-byte path."""
    name, entry = "bias", "las_bias_step"

    def __init__(self, g, loop, rows, ctx, scores):
        tab = self.keep = ctx.to(g.dev)
        Scorer.__init__(self, g, loop, rows, 4, _hip.p(tab["child_off"]), _hip.p(tab["child_tok"]), _hip.p(tab["child_next"]), _hip.p(tab["gdef"]),
                        _hip.p(tab["groot"]), float(ctx.beta), ctx.num_nodes, int(ctx.child_tok.size), _hip.p(scores), g.n, g.beam, g.V)


class NgramScorer(Scorer):
    """N-gram LM shallow fusion: las_ngram_step advances every live row's trie node and adds the candidates' weighted
    log-probabilities to the logits, in place (state rows of 4 floats, as the hotword state)."""
    name, entry = "ngram", "las_ngram_step"

    def __init__(self, g, loop, rows, ng, weight, logits):
        tab = self.keep = ng.to(g.dev, weight)
        Scorer.__init__(self, g, loop, rows, 4, _hip.p(tab["child_off"]), _hip.p(tab["child_tok"]), _hip.p(tab["child_lp"]), _hip.p(tab["child_next"]),
                        _hip.p(tab["bow"]), _hip.p(tab["bo"]), _hip.p(tab["uni_lp"]), _hip.p(tab["uni_next"]), ng.num_nodes, ng.num_entries, ng.order,
                        _hip.p(logits), g.n, g.beam, g.V)


class CoverageScorer(Scorer):
    """Attention coverage: las_coverage_step adds the step's alignments (LoopState.alphas_cur) to every live row's
    accumulated attention, counts the frames above the two thresholds and adds the gain to the row's running sum (LoopState.score) --
    a per-row constant, so no [rows, V] tensor is needed and SpellerStep's short form stays on.  `hist` [Umax, N, 2] keeps every
    step's counts: a finished hypothesis reads its own at its last step and row (BeamSearch._decode_tail)."""
    name, entry = "coverage", "las_coverage_step"

    def __init__(self, g, loop, rows, enc_len_rows, setting):
        self.setting, self.enc_len_rows = setting, enc_len_rows
        self.hist = torch.zeros(g.Umax, g.N, 2, device=g.dev)
        Scorer.__init__(self, g, loop, rows, 4 * ((g.Tp + 2 + 3) // 4), _hip.p(loop.alphas_cur), _hip.p(enc_len_rows), g.n, g.beam, g.Tp,
                        _hip.p(loop.score), setting.w_c, setting.w_o, setting.tau, setting.kappa, _hip.p(self.hist))


def make_scorers(g, loop, rows, logits, end_id, ctc_lp=None, enc_lens=None, lam=0.0, ctx=None, ng=None, ng_weight=0.0, coverage=None,
                 enc_len_rows=None):
    """The active scorers of a search, registered in slot order (CTC, hotwords, n-gram, coverage) -> (the scorers in LAUNCH order, the
    scores the pruning ranks: the CTC scorer's `joint` when it is on, else the logits).  The coverage scorer (a las.coverage.Setting;
    enc_len_rows: T'_u per row, int32 on the device) launches first: it needs the Speller's alignments only."""
    ctc = CtcScorer(g, loop, rows, ctc_lp, enc_lens, logits, lam, end_id) if lam > 0 else None
    ranked = ctc.joint if ctc is not None else logits
    bias = BiasScorer(g, loop, rows, ctx, ranked) if ctx is not None else None
    ngram = NgramScorer(g, loop, rows, ng, ng_weight, logits) if ng is not None else None
    cover = CoverageScorer(g, loop, rows, enc_len_rows, coverage) if coverage is not None else None
    return [s for s in (cover, ngram, ctc, bias) if s is not None], ranked
