"""las.beam_search -- BeamState / BeamSearch with the reference's API (reference las/beam_search.py)
on the MI355X engine.

What changed underneath: the reference issues 1 encode + U decode `sess.run`s per
utterance, re-uploading `np.tile(h)` and re-projecting the keys at every step.  Here the encoder output and
its key projection are computed once and stay resident; each step is one fused Speller step for all live
hypotheses (`Speller.decode`, las_speller_fwd with U=1) followed by the K10 pruning kernel
(`las_beam_loop_step`): expansion, SOS skip, length-normalised ranking, top-`beam` selection, EOS retirement,
termination and the gather of the survivors' recurrent state -- all on the device, for several utterances at once.
The host replays the launches and rebuilds the reference's `BeamState` objects from back-pointer records after the
last step.

Scores are RAW logits summed in float32 and ranked by sum/len, as the reference does."""
import collections.abc
import ctypes
import os
import time

import numpy as np
import torch

from las import _hip
from las import beam_step as S
from las import layers as L

NORM = True


class BeamState(object):
    """hypothesis record (reference las/beam_search.py:7-30)."""

    def __init__(self, token_ids, log_prob, att, dec_state, lm_state):
        self._token_ids = token_ids             # a list, or (round 5, decode_batch's results) a (start id, numpy row) pair turned into the list on first use
        self.log_prob = log_prob               # the search's score: the sum of the RANKED per-token scores -- with a hotword context
        #                                        (las.bias) it includes the hypothesis' biasing bonus, with an n-gram LM
        #                                        (las.ngram) the weighted log-probability of every token
        self.att = att
        self.coverage = None                   # (covered, over, frames) when the coverage scorer ran, and then log_prob
        #                                        includes the hypothesis' coverage gains
        self.dec_state = dec_state
        self.lm_state = lm_state

    @property
    def token_ids(self):
        if isinstance(self._token_ids, tuple):
            self._token_ids = [self._token_ids[0]] + self._token_ids[1].tolist()
        return self._token_ids

    @token_ids.setter
    def token_ids(self, v):
        self._token_ids = v

    def update(self, token_id, log_prob, att, dec_state, lm_state):
        """new state extended by one token; log_prob accumulates (float32 once a float32 logit is added)."""
        return BeamState(self.token_ids + [token_id], self.log_prob + log_prob, self.att + [att], dec_state, lm_state)


class _AttRows(collections.abc.Sequence):
    """`BeamState.att` of a hypothesis returned by decode_batch: item i is the alignment that produced token i (item 0 = zeros,
    las/beam_search.py:88), all items views of ONE [len, T'] tensor gathered from the device-side history in a single
    indexing operation -- building a Python list of 200 slices per hypothesis was a third of the decode time."""

    def __init__(self, rows, lo=None, n=None, width=None):
        # (round 5) lazily sliced: `rows` may be the gathered tensor of ALL hypotheses of a batch, this hypothesis being rows
        # [lo, lo + n) x [0, width) -- a torch slice per hypothesis was most of the 4 ms the host spent after a 64-utterance search
        self._all, self._lo, self._n, self._w = rows, lo, n, width
        self._cut = rows if lo is None else None

    @property
    def _rows(self):
        if self._cut is None:
            self._cut = self._all[self._lo:self._lo + self._n, :self._w]
        return self._cut

    def __len__(self):
        return self._rows.shape[0] if self._lo is None else self._n

    def __getitem__(self, i):
        if isinstance(i, slice):
            return list(self._rows[i].unbind(0))
        return self._rows[i]

    def __add__(self, other):
        return list(self) + list(other)


class AlignInputs(object):
    """what BeamSearch.align needs of a searched batch (kept on request, BeamSearch.retain_align): the encoder outputs, or -- when the
    search computed them -- the CTC head's log-probabilities, which are then not computed a second time"""

    def __init__(self, encs, enc_lens, h_one, ctc_lp):
        self.encs, self.enc_lens, self.h_one, self.ctc_lp = encs, enc_lens, h_one, ctc_lp


# what _run_encoders makes of a batch: encs [per utterance: [1, T'_u, Hd] views], enc_lens, dec_steps, h_one (the encoder output of all
# utterances when they form one group, else None), ctc_lp (class-major CTC log-probabilities [n, V + 1, max T'_u], or None)
EncodedBatch = collections.namedtuple("EncodedBatch", "encs enc_lens dec_steps h_one ctc_lp")


class _Results(list):
    """decode_batch's result list; `align_inputs` is the batch's AlignInputs when BeamSearch.retain_align was set, else None"""
    align_inputs = None


class BeamSearch(object):
    """reference las/beam_search.py:32-312."""

    TOPN = 64   # las/beam_search.py:123

    def __init__(self, args, las, token_to_id, language_model):
        self.args = args
        self.listener = las.listener
        self.speller = las.speller
        self.beam_size = args.beam_size
        self.token_to_id = token_to_id
        self.start_id = token_to_id['<SOS>']
        self.end_id = token_to_id['<EOS>']
        if args.unit.lower() != "char" and args.unit.lower() != "subword":
            raise ValueError('Other units are currently not support!')
        if args.apply_lm:
            self.lm = language_model
        # joint CTC-attention decoding: a candidate scores logit + ctc_weight * (psi(h.c) - psi(h)); 0 = attention (+ LM) only,
        # and then none of the CTC code runs
        self.ctc_weight = float(getattr(args, "ctc_decode_weight", 0.0) or 0.0)
        if self.ctc_weight < 0:
            raise ValueError("--ctc_decode_weight must be >= 0 (got %g)" % self.ctc_weight)
        if self.ctc_weight > 0 and not getattr(args, "ctc", False):
            raise ValueError("--ctc_decode_weight %g needs the CTC head: decode with --ctc True (a model trained with --ctc)" % self.ctc_weight)
        self._las = las
        # contextual biasing: --hotwords FILE --hotword_weight W; no file or weight 0 = off, and then none of its code runs.
        # A weight > 0 without a file and a missing file are refused here, before anything is launched
        self.context = None
        if (getattr(args, "hotwords", "") or "") or float(getattr(args, "hotword_weight", 0.0) or 0.0) != 0.0:
            from las import bias
            self.set_context(bias.from_args(args))
        # n-gram LM shallow fusion: --ngram_lm FILE --ngram_weight W; no file or weight 0 = off, and then none of its code
        # runs.  A weight > 0 without a file, a missing file and a negative or non-finite weight are refused here
        self.ngram, self.ngram_weight = None, 0.0
        if (getattr(args, "ngram_lm", "") or "") or float(getattr(args, "ngram_weight", 0.0) or 0.0) != 0.0:
            from las import ngram
            self.set_ngram(ngram.from_args(args), float(args.ngram_weight))
        # attention coverage: --coverage_weight / --overattend_weight / --coverage_threshold / --overattend_threshold /
        # --coverage_report; weights 0 and no report = off, and then none of its code runs.  Bad values are refused here
        from las import coverage
        self.coverage = coverage.from_args(args)
        # decode_batch / decode_batches keep what align() needs of every batch in its results' `align_inputs` (off: nothing is retained --
        # the CTC log-probabilities are 410 MB at 64 utterances and V = 5000)
        self.retain_align = False
        self._head_absent = None            # restore_las: (checkpoint path, the CTC head's variables it lacks)
        self.use_graph = os.environ.get("LAS_NO_DECODE_GRAPH") != "1"     # decode_batch replays one captured step
        self.fuse_projection = os.environ.get("LAS_NO_DECODE_FUSED_PROJ") != "1"   # decode_batch: cell in one launch, projection inside the beam kernel
        # decode_batch (round 5): the attention rows of FOUR hypotheses of an utterance in one workgroup (LAS_SPELLER_ROWS_SHARE4: Ws, keys and
        # encoder rows read once for the four) from this many hypothesis rows on (0 = never); bit-identical to one row per workgroup
        self.share_rows_from = int(os.environ.get("LAS_DECODE_SHARE_ROWS_FROM", "512"))
        self.xcd_local_rows = os.environ.get("LAS_NO_XCD_LOCAL_ROWS") != "1"       # decode_batch (round 6): an utterance's hypothesis rows on one XCD
        self.shared_operands = os.environ.get("LAS_NO_SHARED_OPERANDS") != "1"    # ... and ONE copy of its keys / encoder rows for all of them (not np.tile's 16)
        self.lm_state_copies = os.environ.get("LAS_NO_LM_STATE_COPIES") != "1"      # decode_batch (round 5): bf16 copies of the LM's state from 384 rows on
        self.steps_per_graph = int(os.environ.get("LAS_DECODE_STEPS_PER_GRAPH", "8"))   # search steps per captured HIP graph (one replay = that many steps)
        self.ragged_encoder = os.environ.get("LAS_NO_RAGGED_ENCODER") != "1"        # decode_batch: one encoder pass over rows of different lengths
        self.parallel_encoders = os.environ.get("LAS_NO_PARALLEL_ENCODERS") != "1"   # decode_batch: encoders of different lengths on several streams
        self._enc_streams = None
        self.measure = os.environ.get("LAS_DECODE_TIMING") == "1"         # decode_batch leaves its phase / per-part timing in last_timing
        self.last_timing = None
        self._capture_stream = None
        self._tail_stream = None            # decode_batches: a batch's back-tracking and read-back run here, beside the next batch's search

    def set_context(self, graph):
        """the hotword context (las.bias.ContextGraph) of the searches that follow, or None: swapped between batches"""
        if graph is not None and graph.child_tok.size and int(graph.child_tok.max()) >= self.args.vocab_size:
            raise ValueError("set_context: the context holds token %d, the vocabulary has %d" % (int(graph.child_tok.max()), self.args.vocab_size))
        if graph is not None and self.args.vocab_size > 16384:
            raise ValueError("set_context: las_bias_step handles vocabularies up to 16384 tokens (got %d)" % self.args.vocab_size)
        self.context = graph

    def set_ngram(self, lm, weight=0.0):
        """the n-gram LM (las.ngram.NgramLM) and its weight for the searches that follow, or (None, 0): swapped between batches.  A model
        with weight 0 is kept and stays off."""
        w = float(weight)
        if not np.isfinite(w) or w < 0:
            raise ValueError("set_ngram: the weight must be finite and >= 0 (got %r)" % (weight,))
        if lm is not None and lm.vocab_size != self.args.vocab_size:
            raise ValueError("set_ngram: the LM is over %d tokens, the vocabulary has %d" % (lm.vocab_size, self.args.vocab_size))
        if lm is not None and w > 0:
            lm.tables(w)                    # (a weight that takes a table value out of float32 is refused here)
        self.ngram, self.ngram_weight = lm, (w if lm is not None else 0.0)

    def set_coverage(self, w_c=0.0, w_o=0.0, tau=0.5, kappa=1.5, report=False):
        """the coverage setting of the searches that follow: swapped between batches.  Weights 0 without a report: off"""
        from las import coverage
        self.coverage = coverage.make(w_c, w_o, tau, kappa, report)

    # -- model calls (the reference's sess.run wrappers, las/beam_search.py:203-246) -------------------
    def _get_encode(self, sess, audio, audiolen):
        dev = self._las._device()
        with torch.no_grad():
            if torch.is_tensor(audio):       # a device-resident cube (las.frontend): no host round trip
                a = audio.to(device=dev, dtype=torch.float32).contiguous()
            else:
                a = torch.as_tensor(np.asarray(audio), dtype=torch.float32, device=dev)
            h, _, enc_len = self.listener(a, np.asarray(audiolen), encoder=self.args.enc_type.lower(), is_training=False)
        return h, enc_len

    # -- the search ----------------------------------------------------------------------------------------
    def decode(self, sess, xs):
        """xs = (audio [1,T,feat_dim,3], audiolen [1]) -> list of BeamState, ascending (best last),
        exactly the reference's contract (las/beam_search.py:61-158; decode.py:136 reads [-1])."""
        audio, audiolen = xs
        if len(audio) != 1:
            raise ValueError('batch size must be 1 while performing beam search.')
        return self.decode_batch(sess, [xs])[0]

    def decode_batches(self, sess, batches, sync_every=32):
        """decode_batch over a SEQUENCE of batches (decode.py's loop over a test set), as a generator of its results -- with the encoders
        of batch k+1 on a second stream UNDER the search of batch k.  An encoder pass is four latency-bound sweeps on 8-72 of the 256 CUs and
        a search step is three small launches, so the two fit side by side; one after the other the encoders are a fifth of a 64-utterance
        batch (7 of 35 ms).  The results are those of decode_batch, batch by batch (the same kernels on the same inputs; only the
        stream differs)."""
        dev = self._las._device()
        main = torch.cuda.current_stream(dev)
        # the device's `comm` auxiliary stream (idle outside training) -- it owns a hardware queue (_hip.aux_streams); a fresh stream would
        # share one of the four queues with the launch stream or an auxiliary stream and its kernels would run in line with theirs
        es = _hip.aux_streams(dev)["comm"]

        first_launch = [True]

        def launch(xs_list):
            if first_launch[0]:              # (everything queued so far: a caller's weight update.  Later launches must NOT wait for the launch
                es.wait_stream(main)         #  stream -- they are issued while the current batch's search steps are queued on it)
                first_launch[0] = False
            with torch.cuda.stream(es):
                if callable(xs_list):        # a deferred batch (transcribe.py: the front end's extraction): made here, on the encoders' stream
                    xs_list = xs_list()
                pre = self._run_encoders(sess, xs_list)
            ev = torch.cuda.Event()
            ev.record(es)
            seen = set()
            for h in pre.encs:               # allocated on `es`, read by the search on `main`
                if h.untyped_storage().data_ptr() not in seen:
                    seen.add(h.untyped_storage().data_ptr())
                    h.record_stream(main)
            if pre.ctc_lp is not None:       # (the CTC log-probabilities, likewise)
                pre.ctc_lp.record_stream(main)
            return xs_list, pre, ev

        it = iter(batches)
        first = next(it, None)
        cur = launch(first) if first is not None else None
        try:
            yield from self._decode_batches_loop(sess, it, cur, launch, main, sync_every)
        finally:
            # a consumer that stops early, or a batch that raises, must not leave the next batch's encoders running into tensors
            # nobody holds: the launch stream waits for everything that was put on the encoder stream
            main.wait_stream(es)

    def _decode_batches_loop(self, sess, it, cur, launch, main, sync_every):
        pending = None
        while cur is not None:
            box, out = [], []

            def between(pending=pending):
                # runs inside decode_batch, behind the launches of its first `sync_every` search steps, i.e. while the device is searching:
                # the host's part of the NEXT batch (stacking the utterances, the copy to the device, the encoder launches on `es`) and
                # everything behind the PREVIOUS batch's search (on the tail stream)
                nxt_xs = next(it, None)
                box.append(launch(nxt_xs) if nxt_xs is not None else None)
                if pending is not None:
                    out.append(pending())
            main.wait_event(cur[2])
            pending = self.decode_batch(sess, cur[0], sync_every, _pre=cur[1], _after_launch=between, _defer=True)
            if out:
                yield out[0]
            if not callable(pending):        # (LAS_DECODE_TIMING: decode_batch measured its phases and returned the results)
                yield pending
                pending = None
            cur = box[0]
        if pending is not None:
            yield pending()

    def _run_encoders(self, sess, xs_list):
        """The encoders of a batch of utterances on the CURRENT stream, without waiting for the device (the encoded lengths are host
        values): -> EncodedBatch (encs, enc_lens, dec_steps, h_one, ctc_lp).  ctc_lp: the CTC head's class-major log-probabilities when
        ctc_decode_weight > 0, else None.  decode_batch's first phase; decode_batches runs it
        for the NEXT batch on a second stream under the search of the current one.
        An utterance's audio is a host array or a device tensor (FeatureExtractor's cube rows); device tensors are stacked and padded
        on the device, with the values the host path would upload."""
        a = self.args
        dev = self._las._device()
        n = len(xs_list)
        sp = self.speller
        prec = L._prec()
        encs, enc_lens, dec_steps = [None] * n, [None] * n, []
        groups = {}
        for u, (audio, audiolen) in enumerate(xs_list):
            if len(audio) != 1:
                raise ValueError('every entry of xs_list is one utterance: audio [1,T,feat_dim,3]')
            al = np.asarray(audiolen).reshape(-1)
            groups.setdefault((tuple(np.shape(audio)[1:]), float(al[0])), []).append(u)
            dec_steps.append(int(al[0] * a.convert_rate))                                       # las/beam_search.py:78
        on_dev = [torch.is_tensor(x[0]) for x in xs_list]
        if any(on_dev) and not all(on_dev):
            raise ValueError('the utterances of one batch are all host arrays or all device tensors')
        on_dev = all(on_dev)

        def encode_group(us):
            # utterances of the SAME shape and length share one encoder launch: every row of the encoder is computed
            # independently of the other rows, so this is exactly the one-at-a-time result (unlike padding, see above)
            if on_dev:
                audio = xs_list[us[0]][0] if len(us) == 1 else torch.cat([xs_list[u][0] for u in us], 0)
            else:
                audio = np.concatenate([np.asarray(xs_list[u][0]) for u in us], 0)
            audiolen = np.concatenate([np.asarray(xs_list[u][1]).reshape(-1)[:1] for u in us], 0)
            h, enc_len = self._get_encode(sess, audio, audiolen)
            el = torch.as_tensor(enc_len).reshape(-1).cpu().tolist()       # (one read-back, not one per utterance)
            for i, u in enumerate(us):
                encs[u] = h[i:i + 1]
                enc_lens[u] = float(el[i])
            return h

        glist = list(groups.values())
        h_one = None                         # the encoder output of all utterances when they form one group
        cellid = L._cellid(sp.cell)
        H_enc = a.enc_units
        ragged = (len(glist) > 1 and self.ragged_encoder and prec == _hip.PREC_BF16 and a.enc_type.lower() == "pblstm" and
                  len({np.shape(x[0])[2:] for x in xs_list}) == 1 and
                  _hip.rnn_seq_io_dtype(cellid, prec, H_enc) == torch.bfloat16 and _hip.rnn_seq_fwd_rows_ok(cellid, prec, n, H_enc))
        if ragged:
            # ONE encoder pass over all utterances although their lengths differ (the reference feeds them one at a time, unpadded):
            # the forward sweeps take the rows' frame counts (las_rnn_seq_args' row_T: a row's state and outputs are zero behind its last
            # frame, so its backward direction starts from the zero state at ITS last frame and an odd length pairs with a zero frame,
            # exactly as alone); the products in between are row-wise.  Every real frame equals the one-at-a-time result.
            lens = [int(np.shape(x[0])[1]) for x in xs_list]
            Tmax = max(lens)
            if on_dev:
                audio = torch.zeros((n, Tmax) + tuple(np.shape(xs_list[0][0])[2:]), dtype=torch.float32, device=dev)
                for u, x in enumerate(xs_list):
                    audio[u, :lens[u]] = x[0][0]
            else:
                audio = np.zeros((n, Tmax) + tuple(np.shape(xs_list[0][0])[2:]), np.float32)
                for u, x in enumerate(xs_list):
                    audio[u, :lens[u]] = np.asarray(x[0])[0]
            audiolen = np.concatenate([np.asarray(x[1]).reshape(-1)[:1] for x in xs_list], 0)
            L.ROW_T[0] = torch.tensor(lens, dtype=torch.int32, device=dev)
            try:
                h, enc_len = self._get_encode(sess, audio, audiolen)
            finally:
                L.ROW_T[0] = None
            el = torch.as_tensor(enc_len).reshape(-1).cpu().tolist()
            for u in range(n):
                tp = lens[u]
                for _ in range(a.num_enc_layers):
                    tp = (tp + 1) // 2
                encs[u] = h[u:u + 1, :tp]
                enc_lens[u] = float(el[u])
            glist = []
        else:
            h_one = encode_group(glist[0])
            if len(glist) > 1:
                h_one = None
        if ragged:
            pass
        elif len(glist) > 1 and self.parallel_encoders:
            # Groups of DIFFERENT lengths (a real test set: every utterance its own) run side by side on a few streams: an encoder is
            # four latency-bound sweeps that occupy 8-16 of the 256 CUs each, one after the other they are the bulk of a search
            # (16 x 4 ms against 15 ms of search).  The first group ran on this stream (it also builds the weights' bf16 shadows once);
            # the others start behind it.  The chunked x-projection hand-over shares one side stream and one ring of flag words:
            # it is off for these launches (whole products in front of the sweeps -- they overlap across the streams anyway).
            cur = torch.cuda.current_stream()
            ready = torch.cuda.Event()
            ready.record()
            if self._enc_streams is None:
                self._enc_streams = [torch.cuda.Stream() for _ in range(8)]
            with L.schedule(XPROJ_CHUNK_STEPS=0):
                for i, us in enumerate(glist[1:]):
                    s_ = self._enc_streams[i % len(self._enc_streams)]
                    s_.wait_event(ready)
                    with torch.cuda.stream(s_):
                        encode_group(us).record_stream(cur)
            for s_ in self._enc_streams:
                cur.wait_stream(s_)
        else:
            for us in glist[1:]:
                encode_group(us)
        ctc_lp = self._ctc_log_probs(encs, h_one) if self.ctc_weight > 0 else None
        return EncodedBatch(encs, enc_lens, dec_steps, h_one, ctc_lp)

    def _stack_encs(self, encs, h_one):
        """the encoder outputs of a batch as ONE block [n, max T'_u, Hd], zero behind an utterance's last frame (h_one when the utterances
        form one encoder group: equal lengths, nothing to pad)"""
        n = len(encs)
        if h_one is not None and h_one.shape[0] == n:
            return h_one.contiguous()
        enc = torch.zeros(n, max(h.shape[1] for h in encs), encs[0].shape[2], device=self._las._device())
        for u, h in enumerate(encs):
            enc[u, :h.shape[1]] = h[0]
        return enc

    def _ctc_log_probs(self, encs, h_one):
        """The CTC head over the encoder frames of a batch (las/las.py:75-77, the product of _CTCHead.forward through las_gemm), then
        las_ctc_log_softmax: class-major log-probabilities [n, V + 1, T'] (frames past T'_u hold values nobody reads)."""
        return self._ctc_class_major(self._ctc_logits(encs, h_one))

    def _ctc_logits(self, encs, h_one):
        """the head product alone: frame-major logits [n, T', V + 1] (what the CTC-only search reads, las.ctc_search)"""
        dev = self._las._device()
        P = self.speller._params(head=True)
        Wc, bc = P["Wc"].detach(), P["bc"].detach()
        enc = self._stack_encs(encs, h_one)
        (n, Tp, Hd), Vc = enc.shape, Wc.shape[1]
        z = torch.empty(n, Tp, Vc, device=dev)
        _hip.gemm(L._prec(), enc, Wc, z, False, False, n * Tp, Vc, Hd, Hd, Vc, Vc, bias=bc)
        return z

    def _ctc_class_major(self, z):
        n, Tp, Vc = z.shape
        lp = torch.empty(n, Vc, Tp, device=z.device)
        _hip.check(_hip.lib().las_ctc_log_softmax(_hip.p(z), n, Tp, Vc, _hip.p(lp), _hip.stream()), "las_ctc_log_softmax")
        return lp

    def need_ctc_head(self, what):
        """the ValueError of the --ctc_decode_weight checks for anything else that reads the CTC head"""
        if not getattr(self.args, "ctc", False):
            raise ValueError("%s needs the CTC head: decode with --ctc True (a model trained with --ctc)" % what)
        if self._head_absent is not None:
            raise ValueError("%s: checkpoint %s holds no CTC head (%s); it was not trained with --ctc True"
                             % (what, self._head_absent[0], ", ".join(self._head_absent[1])))

    def align(self, encs, enc_lens, token_lists, h_one=None, ctc_lp=None):
        """CTC Viterbi alignment (las.align.ctc_align) of token_lists[u] to the encoder frames of utterance u: -> (scores,
        spans), spans[u][j] = (first, last) frame of token j.  encs / enc_lens / h_one: _run_encoders' (or a retained AlignInputs');
        the head runs here whether or not ctc_decode_weight is set -- unless the caller hands in the `ctc_lp` a search already computed."""
        from las.align import ctc_align
        self.need_ctc_head("BeamSearch.align")
        with torch.no_grad():
            if ctc_lp is None:
                ctc_lp = self._ctc_log_probs(encs, h_one)
            return ctc_align(ctc_lp, [int(x) for x in enc_lens], token_lists)

    def align_results(self, results, token_lists=None):
        """align() on the AlignInputs a search retained in `results` (retain_align); token_lists defaults to every utterance's best
        hypothesis without its <SOS> (an utterance without a hypothesis aligns the empty sequence)"""
        k = getattr(results, "align_inputs", None)
        if k is None:
            raise ValueError("BeamSearch.align_results: the search retained nothing -- set retain_align = True before decoding")
        if token_lists is None:
            token_lists = [list(r[-1].token_ids[1:]) if r else [] for r in results]
        return self.align(k.encs, k.enc_lens, token_lists, h_one=k.h_one, ctc_lp=k.ctc_lp)

    def keyword_search(self, encs, enc_lens, keywords, h_one=None, ctc_lp=None, threshold_per_token=-1.0, max_hits=4, series=False):
        """Keyword search on the CTC head (las.kws.keyword_search): every phrase of `keywords` (a las.kws.KeywordList) in
        every utterance -> a KeywordResult.  encs / enc_lens / h_one: _run_encoders'; as in align(), the head runs here whether or not
        ctc_decode_weight is set, unless the caller hands in the `ctc_lp` a search already computed."""
        from las.kws import keyword_search
        self.need_ctc_head("BeamSearch.keyword_search")
        with torch.no_grad():
            if ctc_lp is None:
                ctc_lp = self._ctc_log_probs(encs, h_one)
            return keyword_search(ctc_lp, [int(x) for x in enc_lens], keywords, threshold_per_token, max_hits=max_hits, series=series)

    def ctc_decode_batch(self, sess, xs_list):
        """`--decoder ctc`: the transcripts of a batch from the CTC head alone -- encoders, head product, greedy collapse
        (beam_size 1) or CTC prefix beam search with the n-gram of set_ngram (las.ctc_search) -- as decode_batch's result lists.  No
        Speller step runs."""
        from las import ctc_search
        return ctc_search.decode_batch(self, sess, xs_list)

    def score_hypotheses(self, encs, enc_lens, token_lists, rows=64, return_steps=False):
        """The attention decoder's log-likelihood of given transcripts: encs / enc_lens as _run_encoders returns them,
        token_lists[u] = token lists of utterance u (no <SOS>) -> scores[u][k]: the teacher-forced Speller over chunks of `rows`
        hypotheses and las_rescore_score on its logits.  A list is scored through its first EOS, or with one appended."""
        from las import rescore
        return rescore.attention_scores(self, encs, enc_lens, token_lists, rows, return_steps)

    def ctc_decode_batches(self, sess, batches):
        from las import ctc_search
        return ctc_search.decode_batches(self, sess, batches)

    def decode_batch(self, sess, xs_list, sync_every=32, _pre=None, _after_launch=None, _defer=False):
        """Beam search for several utterances at once (what decode.py's loop over utterances, decode.py:131-149, becomes on
        one GPU): xs_list = [(audio [1,T_u,feat_dim,3], audiolen [1]), ...] -> [list of BeamState (ascending), ...].

        Every utterance is ENCODED on its own, at its own length (the reference's encoder has no sequence mask, so its
        output depends on the padded length -- SURVEY fact 4 -- and decode.py feeds unpadded utterances); the search then
        runs all utterances x beam hypotheses as ONE batch of rows per step: fused Speller step (las_speller_fwd, U = 1)
        [+ LM step + shallow fusion] [+ n-gram, CTC prefix, hotword scores] + las_beam_loop_step (pruning, EOS retirement, termination,
        state gather -- all on the device; the parts of a step: las/beam_step.py).  The host replays the launches without waiting and
        reads the back-pointer records once at the end (plus one `done` poll every `sync_every` steps to stop early)."""
        a, dev, prec, tm = self.args, self._las._device(), L._prec(), {}
        def mark(name):                                  # wall-clock marks (with a device sync) only when asked for
            if self.measure:
                torch.cuda.synchronize(dev)
                tm[name] = time.perf_counter()
        mark("start")
        # ---- encoders (one per utterance) and the hoisted key projection
        if _pre is None:
            _pre = self._run_encoders(sess, xs_list)
        encs, enc_lens, dec_steps, h_one, ctc_lp = _pre
        kept = AlignInputs(encs, enc_lens, h_one, ctc_lp) if self.retain_align else None
        Tps = [h.shape[1] for h in encs]
        n, Tp, Hd, A = len(xs_list), max(Tps), encs[0].shape[2], a.attention_size
        Wh = self.speller._params()["Wh"].detach()
        enc_u = self._stack_encs(encs, h_one)
        if h_one is not None and h_one.shape[0] == n:
            keys_u = torch.empty(n, Tp, A, device=dev)                 # every utterance in ONE encoder group: the projection as one product
            _hip.gemm(prec, enc_u, Wh, keys_u, False, False, n * Tp, A, Hd, Hd, A, A)
        else:
            keys_u = torch.zeros(n, Tp, A, device=dev)
            for u, h in enumerate(encs):
                k = torch.empty(1, Tps[u], A, device=dev)
                _hip.gemm(prec, h.contiguous(), Wh, k, False, False, Tps[u], A, Hd, Hd, A, A)
                keys_u[u, :Tps[u]] = k[0]
        # ---- the parts of a step
        g = S.Geometry(dev, n, self.beam_size, n * self.beam_size, Tp, Hd, max(max(dec_steps), 1), a.vocab_size, A, a.num_dec_layers, a.dec_units,
                       a.embedding_size, self.speller.cell == "lstm", prec)
        loop, rows = S.LoopState(g, dec_steps, self.start_id, self.end_id, self.TOPN), S.StateRows()
        lam = self.ctc_weight
        ctx = self.context if (self.context is not None and self.context.active) else None
        ng = self.ngram if (self.ngram is not None and self.ngram_weight > 0) else None
        lm = S.LmFusion(self.lm, a.lm_weight, g, loop, self.lm_state_copies) if a.apply_lm else None
        speller = S.SpellerStep(self, g, loop, rows, enc_u, keys_u, enc_lens, lm, ng, ctx, lam)
        if lm is not None:
            lm.attach(rows, speller)
        scorers, ranked = S.make_scorers(g, loop, rows, speller.logits, self.end_id, ctc_lp, enc_lens, lam, ctx, ng, self.ngram_weight,
                                         self.coverage, speller.enc_len)
        cover = scorers[0] if self.coverage is not None else None
        loop.ba.logits = ranked.data_ptr()
        rows.write(loop.ba)
        mark("encoded")
        # One step = Speller, LM, the active scorers, the pruning: five launches in the short form (rows | cell + LM 1 | LM 2 | pruning | gather).
        # tried: three dependent launches -- LM 1 as extra workgroups of the row launch, LM 2 beside the Speller's cell, the gather inside the
        # pruning launch.  result: 73-80 us of kernel time per replayed step against 59 us for the five (14.3 + 12.7 + 11.2 + 15.9 + 4.8):
        # every kernel of the step fills the machine by itself (256 rows = 256 workgroups of 16 waves), so rows + LM 1 ran one after the other
        # inside their launch (22-26 us), and dependent launches cost ~0 us in a replayed graph (profiles/r5_decode_three_launches.txt).
        # tried: the LM's cells (they depend only on the tokens) as a parallel branch on a second stream beside the Speller step.
        # result: 111 against 99.5 us per captured step -- the cross-queue joins cost more than the overlap gives.
        parts = [speller] + ([lm] if lm is not None else []) + scorers + [loop]
        one_step = lambda: [part.launch() for part in parts]
        steps_run, graph_used = self._run_steps(one_step, loop, sync_every, _after_launch)
        mark("searched")
        if _defer and not self.measure:
            # decode_batches: everything behind the search -- back-tracking, the alignment gather, the read-back, the host objects -- as a closure
            # (it holds the loop state) that runs on a side stream behind THIS point of the launch stream: the caller launches the next batch's
            # search first and calls it while the device is busy with that (the read-back waits for the side stream only).
            ev = torch.cuda.Event()
            ev.record()
            if self._tail_stream is None:
                self._tail_stream = torch.cuda.Stream()

            def finish():
                self._tail_stream.wait_event(ev)
                with torch.cuda.stream(self._tail_stream):
                    return self._decode_tail(loop, Tps, mark, kept, cover)
            return finish
        results = self._decode_tail(loop, Tps, mark, kept, cover)
        mark("done")
        if tm:
            live_steps, parts_us = self._time_parts(parts, loop)
            ks = list(tm)
            self.last_timing = {ks[i + 1]: round(tm[ks[i + 1]] - tm[ks[i]], 4) for i in range(len(ks) - 1)}
            self.last_timing.update(steps=steps_run, live_steps=live_steps, rows=g.N, frames=Tp, graph=graph_used, short_form=bool(speller.fused), parts_us=parts_us)
            if a.verbose > 0:
                print("decode_batch timing (s):", self.last_timing)
        return results

    def _run_steps(self, one_step, loop, sync_every, _after_launch):
        """The steps of a search: step 0 eagerly, then -- captured once, at step 1 -- replays of a HIP graph of `steps_per_graph` steps (the
        loop is bound by the host's launch rate otherwise: 5-8 launches and their Python glue per step).  `_after_launch` (decode_batches: the
        next batch's host work and encoder launches) is called once, at the first `done` poll.  -> (steps run, whether the graph was used)"""
        dev, Umax, steps_run, graph = loop.g.dev, loop.g.Umax, 0, None
        use_graph = self.use_graph and Umax > 2
        # One hipGraphLaunch costs the host more than a 3-launch step costs the device (r5 probe: 75-85 us per replayed step whatever the
        # step's kernels added up to -- 55-62 us): the captured graph holds K consecutive steps.  Every launch of a step reads the DEVICE
        # step counter, and a step at t >= Umax does nothing that is kept (las_beam_loop_step returns before it files or records), so
        # the last replay may run past the bound.
        K = max(1, int(self.steps_per_graph))
        with torch.no_grad():
            t, next_check = 0, sync_every * (2 if _after_launch is not None else 1)     # (the host work done at the first check wants ~6 ms of queued steps)
            while t < Umax:
                if graph is not None:
                    graph.replay()
                    t += K
                elif use_graph and t == 1:
                    try:
                        # (capture_begin / capture_end by hand: the torch.cuda.graph context synchronises the device and EMPTIES the
                        #  caching allocator on entry -- a millisecond per search, and every buffer of the next search a fresh hipMalloc)
                        g = torch.cuda.CUDAGraph()
                        if self._capture_stream is None:
                            self._capture_stream = torch.cuda.Stream()
                        cs_ = self._capture_stream
                        cs_.wait_stream(torch.cuda.current_stream())
                        with torch.cuda.stream(cs_):
                            g.capture_begin()
                            try:
                                for _ in range(K):
                                    one_step()
                            finally:
                                g.capture_end()
                        torch.cuda.current_stream().wait_stream(cs_)
                        graph = g                      # (capturing does not execute: the captured steps run as the replay)
                        graph.replay()
                        t += K
                    except Exception as e:             # capture refused (e.g. an op that allocates host memory): stay eager
                        use_graph = False
                        torch.cuda.synchronize(dev)
                        if self.args.verbose > 0:
                            print("decode_batch: graph capture failed, running eagerly: %s" % e)
                        one_step()
                        t += 1
                else:
                    one_step()
                    t += 1
                steps_run = min(t, Umax)
                if t >= next_check:                                                     # the only host wait inside the loop
                    next_check += sync_every
                    if _after_launch is not None:                                       # (while the device runs the steps enqueued so far)
                        _after_launch(); _after_launch = None
                    if bool(loop.done.all()):
                        break
        if _after_launch is not None:
            _after_launch()
        return steps_run, graph is not None

    def _time_parts(self, parts, loop):
        """LAS_DECODE_TIMING: device time of the parts of a decode step (HIP events, 50 eager repetitions each, after the search)
        -> (live_steps, {part name: us})"""
        dev, beam, done, nlive, step = loop.g.dev, loop.g.beam, loop.done, loop.nlive, loop.step
        live_steps = int((loop.hist_n.sum(1) > 0).sum())              # steps in which some utterance still had a live hypothesis
        step.zero_()
        parts_us = {}
        for part in parts:
            forced = isinstance(part, S.Scorer)
            if forced:
                # every row live at a step > 0 (after the search every utterance is done and the kernel would return at once); the
                # loop words are put back before the pruning part is timed
                saved = (done.clone(), nlive.clone())
                done.zero_(); nlive.fill_(beam); step[0] = 1
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.no_grad():
                part.launch(); e0.record()
                for _ in range(50):
                    part.launch()
                    if part is loop:
                        step.zero_()
                e1.record()
            torch.cuda.synchronize(dev)
            parts_us[part.name] = round(e0.elapsed_time(e1) / 50 * 1e3, 2)
            if forced:
                done.copy_(saved[0]); nlive.copy_(saved[1]); step.zero_()
        return live_steps, parts_us

    def _decode_tail(self, loop, Tps, mark, kept=None, cover=None):
        """What follows a search (decode_batch; on the current stream): the back pointers are walked on the device (las_beam_backtrack), one
        read-back, then the reference's host-side objects (las/beam_search.py:136-158, :297-312)."""
        ba, selcap, alphas_hist, lib, dev, n, Umax = loop.ba, loop.selcap, loop.alphas_hist, _hip.lib(), loop.g.dev, loop.g.n, loop.g.Umax
        i32 = dict(dtype=torch.int32, device=dev)
        # ---- the back pointers are walked on the device (las_beam_backtrack); one read-back, then the reference's host-side objects
        W = n * selcap
        w_ids = torch.zeros(W, Umax, **i32)
        w_rows = torch.zeros(W, Umax, **i32)
        w_len = torch.zeros(W, **i32)
        w_score = torch.zeros(W, device=dev)
        _hip.check(lib.las_beam_backtrack(ctypes.byref(ba), _hip.p(w_ids), _hip.p(w_rows), _hip.p(w_len), _hip.p(w_score), _hip.stream()),
                   "las_beam_backtrack")
        # every hypothesis' alignments in ONE gather: item 0 of a hypothesis is the all-zero slab [Umax], item 1 + p the row it occupied at step p
        pos = torch.arange(Umax + 1, device=dev)
        item = (pos.unsqueeze(0) <= w_len.unsqueeze(1)) & (w_len > 0).unsqueeze(1)                 # [W, Umax + 1]
        t_idx = torch.cat([torch.full((1,), Umax, device=dev, dtype=torch.int64), pos[:-1]]).expand(W, -1)[item]
        r_idx = torch.cat([torch.zeros(W, 1, **i32), w_rows], 1)[item].long()
        g_att = alphas_hist[t_idx, r_idx]
        cov_h = frames = None
        if cover is not None:
            # a hypothesis' counts: the coverage scorer's record of its LAST step, at the row it occupied there
            last = (w_len - 1).clamp(min=0).long()
            cov_h = cover.hist[last, w_rows.gather(1, last.unsqueeze(1))[:, 0].long()].cpu().numpy().astype(np.int64)
            frames = cover.enc_len_rows[::loop.g.beam].clamp(0, loop.g.Tp).cpu().tolist()
        lens, ids_h, sc_h = w_len.cpu().numpy(), w_ids.cpu().numpy(), w_score.cpu().numpy()
        _hip.check_status(dev)
        mark("read back")
        # The reference's final ranking (_select_best_k: stable argsort of log_prob [/ (len - 1)], the last beam_size) on the read-back
        # arrays; host objects are built for the SELECTED hypotheses only (round 5: one BeamState + one tensor slice for each of the
        # <= 2 x beam candidates of every utterance was 4.2 ms behind a 64-utterance search, a tenth of the batch)
        nz = np.nonzero(lens)[0]
        offs = np.concatenate(([0], np.cumsum(lens[nz] + 1)))[:-1] if nz.size else np.zeros(0, np.int64)
        results = _Results([] for _ in range(n))
        results.align_inputs = kept
        first = np.searchsorted(nz, np.arange(n + 1) * selcap)
        for u in range(n):
            ws, of = nz[first[u]:first[u + 1]], offs[first[u]:first[u + 1]]
            if ws.size == 0:
                continue
            sc = sc_h[ws].astype(np.float32)
            key = sc / lens[ws].astype(np.float32) if NORM else sc
            for i in np.argsort(key, kind="stable")[-self.beam_size:].tolist():
                w, ln_ = int(ws[i]), int(lens[ws[i]])
                results[u].append(BeamState((self.start_id, ids_h[w, :ln_]), np.float32(sc_h[w]),
                                            _AttRows(g_att, int(of[i]), ln_ + 1, Tps[u]), None, None))
                if cov_h is not None:
                    results[u][-1].coverage = (int(cov_h[w, 0]), int(cov_h[w, 1]), int(frames[u]))
        return results

    def restore_las(self, sess, save_path, restore_epoch):
        """Restore LAS weights (reference las/beam_search.py:272-281; the TF name remapping of
        :252-270 is unnecessary: train and decode share one variable store)."""
        from las import checkpoint
        missing = []
        path = checkpoint.restore(save_path, restore_epoch, missing=missing)
        absent = [nm for nm in checkpoint.CTC_HEAD if nm in missing]
        self._head_absent = (path, absent) if path is not None and absent else None
        if path is not None and self.ctc_weight > 0 and absent:
            # the head would keep its initial values: the prefix scores would be noise
            raise ValueError("--ctc_decode_weight %g: checkpoint %s holds no CTC head (%s); it was not trained with --ctc True"
                             % (self.ctc_weight, path, ", ".join(absent)))
        return path
