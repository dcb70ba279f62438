"""The registry of the state rows that follow their hypotheses through the gather of a search step (las.beam_step.StateRows), on the host:
the slot order the parts of a step register in, the widths written into las_beam_loop_args, and the refusal of a 17th tensor."""
import types

import pytest
import torch

from las import _hip
from las import beam_step as S

N, D, HL, TP, V, BEAM = 8, 32, 64, 11, 30, 4


def _registered(twins, scorers):
    """an LSTM decoder layer, a two-layer LM (with / without bf16 twins) [+ CTC, hotwords, n-gram], registered as decode_batch does"""
    from las.bias import ContextGraph
    g = S.Geometry("cpu", N // BEAM, BEAM, N, TP, 16, 5, V, 8, 1, D, 16, True, _hip.PREC_BF16)
    loop = types.SimpleNamespace(alphas_cur=torch.zeros(N, TP), align_prev=torch.zeros(N, TP), words=lambda: ())
    bufs = {"hs": torch.zeros(1, 2, N, D), "cs": torch.zeros(1, 2, N, D)}
    rows = S.StateRows()
    S.SpellerStep.register(rows, bufs, 1, True, loop)
    lm = object.__new__(S.LmFusion)
    lm.c, lm.h = [torch.zeros(N, HL) for _ in range(2)], [torch.zeros(N, HL) for _ in range(2)]
    lm.hb = [torch.zeros(N, HL, dtype=torch.bfloat16) for _ in range(2)] if twins else None
    lm.register(rows)
    want = [(bufs["hs"][0, 1], bufs["hs"][0, 0], D), (bufs["cs"][0, 1], bufs["cs"][0, 0], D), (loop.alphas_cur, loop.align_prev, TP)]
    if twins:
        want += [(c, c, HL) for c in lm.c] + [(hb, hb, HL // 2) for hb in lm.hb]
        assert lm.k_c == [3, 4] and lm.k_h == [5, 6]
    else:
        want += [(t, t, HL) for pair in zip(lm.c, lm.h) for t in pair]
        assert lm.k_c == [3, 5] and lm.k_h == [4, 6]
    if scorers:
        logits = torch.zeros(N, V)
        ctx = ContextGraph([[4, 7, 4]], 2.0, vocab_size=V)
        launch, ranked = S.make_scorers(g, loop, rows, logits, 2, ctc_lp=torch.zeros(N // BEAM, V + 1, TP), enc_lens=[TP, TP - 2], lam=0.3, ctx=ctx,
                                        ng=_Tables(), ng_weight=1.0)
        assert [s.name for s in launch] == ["ngram", "ctc", "bias"]                   # launch order; slots: CTC, hotwords, n-gram
        by = {s.name: s for s in launch}
        assert ranked is by["ctc"].joint
        want += [(by[k].cur, by[k].par, w) for k, w in (("ctc", 4 * ((2 * TP + 2 + 3) // 4)), ("bias", 4), ("ngram", 4))]
    return rows, want


class _Tables(object):
    """what NgramScorer reads of an NgramLM"""
    num_nodes, num_entries, order = 1, 0, 1

    def to(self, dev, weight):
        return {k: torch.zeros(1) for k in ("child_off", "child_tok", "child_lp", "child_next", "bow", "bo", "uni_lp", "uni_next")}


@pytest.mark.parametrize("twins,scorers", [(True, False), (False, False), (True, True)])
def test_slot_order_and_widths(twins, scorers):
    rows, want = _registered(twins, scorers)
    ba = _hip.BeamLoopArgs()
    rows.write(ba)
    assert ba.ntens == len(want) == (7 if not scorers else 10)
    for k, (src, dst, width) in enumerate(want):
        assert (ba.state_in[k], ba.state_out[k], ba.state_width[k]) == (src.data_ptr(), dst.data_ptr(), width), k
    assert all(ba.state_in[k] is None and ba.state_width[k] == 0 for k in range(len(want), 16))


def test_a_seventeenth_tensor_is_refused():
    rows = S.StateRows()
    t = torch.zeros(N, 4)
    assert [rows.add(t, t) for _ in range(16)] == list(range(16))
    rows.write(_hip.BeamLoopArgs())
    assert rows.add(t, t) == 16
    with pytest.raises(ValueError) as e:
        rows.write(_hip.BeamLoopArgs())
    assert str(e.value) == ("decode_batch: 17 state tensors follow the hypotheses (decoder and LM state, alignment, CTC, hotword and "
                            "n-gram LM state); las_beam_loop_step gathers at most 16")
