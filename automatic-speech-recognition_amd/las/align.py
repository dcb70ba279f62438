"""las.align -- token and word times from the CTC head: the Viterbi alignment of a token sequence to the encoder frames
(las_ctc_align, csrc/ctc_align.hip) and the host-side bookkeeping that turns frame ranges into seconds and words.

An attention decoder has no monotone alignment to read times from; a model trained with --ctc True carries a head that does.  The
reference has no counterpart."""
import numpy as np
import torch

from las import _hip


def ctc_align(lp, enc_lens, token_lists):
    """Align token_lists[u] to the frames of utterance u.  lp: the device's class-major log-probabilities [n, V + 1, T'] (fp32,
    BeamSearch._ctc_log_probs); enc_lens [n]: frames per utterance.  -> (scores, spans): scores[u] the log-probability of the
    best path (-inf: the utterance cannot be aligned), spans[u] = [(first, last), ...] the inclusive frame range of every token
    ((-1, -1) when unalignable).
    One upload (lengths and padded tokens in one buffer), one call for the batch, one read-back."""
    _hip.require_gpu(lp)
    if lp.dim() != 3 or lp.dtype != torch.float32 or not lp.is_contiguous():
        raise ValueError("ctc_align: lp must be a contiguous fp32 [n, V + 1, T'] tensor")
    n, Vc, Tp = lp.shape
    if len(token_lists) != n or len(enc_lens) != n:
        raise ValueError("ctc_align: %d utterances, %d token lists, %d lengths" % (n, len(token_lists), len(enc_lens)))
    dev = lp.device
    U = max(1, max(len(t) for t in token_lists))
    host = np.zeros(n * (2 + U), np.int32)                    # [enc_len (n) | y_len (n) | y (n, U)]
    host[:n] = [int(x) for x in enc_lens]
    host[n:2 * n] = [len(t) for t in token_lists]
    y = host[2 * n:].reshape(n, U)
    for u, t in enumerate(token_lists):
        y[u, :len(t)] = np.asarray(t, np.int64)
    meta = torch.from_numpy(host).to(dev)
    span = torch.empty(2, n, U, dtype=torch.int32, device=dev)
    score = torch.empty(n, dtype=torch.float64, device=dev)
    lib = _hip.lib()
    ws = _hip.workspace(dev, lib.las_ctc_align_workspace_bytes(n, Tp, U), "ctc_align")
    _hip.check(lib.las_ctc_align(_hip.p(lp), Vc, Tp, _hip.p(meta[:n]), n, _hip.p(meta[2 * n:]), U, _hip.p(meta[n:2 * n]), U,
                                 _hip.p(span[0]), _hip.p(span[1]), None, _hip.p(score), _hip.p(ws), ws.numel(), _hip.stream()),
               "las_ctc_align")
    sp, sc = span.cpu().numpy(), score.cpu().numpy()
    scores = [float(x) for x in sc]
    spans = [[(int(sp[0, u, j]), int(sp[1, u, j])) for j in range(len(t))] for u, t in enumerate(token_lists)]
    return scores, spans


def time_reduction(args, enc_type):
    """input frames per encoder frame: both listeners halve the frame count with (len + len % 2) / 2 -- the pBLSTM listener once per
    pyramid layer, the CNN listener in its two stride-2 convolutions (Listener.output_length)"""
    enc_type = str(enc_type).lower()
    if enc_type not in ("pblstm", "cnn"):
        raise NotImplementedError(enc_type)
    halvings = int(args.num_enc_layers) if enc_type == "pblstm" else 2
    return 2 ** halvings


def frame_seconds(args, enc_type):
    """seconds of input per encoder frame: --frame_step (ms) times the listener's time reduction"""
    return args.frame_step / 1000.0 * time_reduction(args, enc_type)


def words(tokens, spans, id_to_token, unit, frame_s, duration_s):
    """[{"word", "start", "end"}] of one utterance.  The words are those of las.utils.convert_idx_to_string: char unit -- split at
    <SPACE>; subword unit -- a word ends at a token ending in </w>; <EOS> and everything behind it make no word.  start = first frame of
    the word's first token * frame_s, end = min((last frame of its last token + 1) * frame_s, duration_s); both None when the utterance
    could not be aligned (spans of -1)."""
    out, text, lo, hi = [], "", None, None

    def flush():
        nonlocal text, lo, hi
        if text:
            ok = lo is not None and lo >= 0 and hi >= 0
            out.append({"word": text, "start": lo * frame_s if ok else None,
                        "end": min((hi + 1) * frame_s, duration_s) if ok else None})
        text, lo, hi = "", None, None

    for tok, (first, last) in zip(tokens, spans):
        piece = id_to_token[int(tok)]
        if piece == "<EOS>":
            break
        ends = False
        if unit == "char":
            if piece == "<SPACE>":
                flush()
                continue
        elif unit == "subword" and piece.endswith("</w>"):
            piece, ends = piece[:-len("</w>")], True
        if piece.strip():
            text += piece.strip() if unit == "subword" else piece
            if lo is None:
                lo = first
            hi = last
        if ends:
            flush()
    flush()
    return out
