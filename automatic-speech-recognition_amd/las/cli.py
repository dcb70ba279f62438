"""las.cli -- decode.py and transcribe.py before the first utterance: transcribe.py's flags and their one check (`add_flags`, `check_flags`
-> `Mode`), the model set-up (`build_search`, `load_lm`, `restore_lm`), the listener-only loop of the search-less modes (`encoded_batches`)."""
import collections
import json
import logging
import os

import numpy as np

from las.arguments import check_confusion_flags, str2bool

Mode = collections.namedtuple("Mode", "kind ctc_only annotate json")


def add_flags(parser):
    """the flags of transcribe.py alone (las.arguments keeps the reference's table; the --segment flags: las.vad.add_flags)"""
    parser.add_argument("audio", nargs="*", help=".wav / .npy files to transcribe")
    parser.add_argument("--timestamps", type=str2bool, default=False, help="One JSON object per line with word times (needs --ctc True).")
    parser.add_argument("--align_text", type=str, default=None, metavar="FILE",
                        help="Forced alignment: one transcript per audio file, in order; skips the search, implies --timestamps True.")
    parser.add_argument("--keywords", type=str, default=None, metavar="FILE", help="Keyword search: one phrase per line ('#' comments); skips "
                        "the search and prints, per audio file, one JSON object with the places the CTC head hears a phrase (needs --ctc True).")
    parser.add_argument("--keyword_threshold", type=float, default=-1.0, help="A hit needs a score of at least this many nats per token of "
                        "its phrase (the score is the phrase's log-likelihood ratio against the head's frame-wise best path: <= 0).  The "
                        "default of -1.0 is a guess: nobody has measured it on a trained model.")
    parser.add_argument("--keyword_max_hits", type=int, default=4, help="Hits kept per file and phrase, the strongest (1 to 8).")


def add_diarize_flags(parser):
    """the --diarize flags (las.diarize.add_flags; kept here so that a run without --diarize never imports las.diarize)"""
    parser.add_argument("--diarize", type=str2bool, default=False, help="Label every segment with its speaker (needs --segment True; JSON "
                        "lines): BIC change points inside the speech runs and BIC clustering of the pieces, no trained model.")
    parser.add_argument("--num_speakers", type=int, default=0, help="Cluster down to this many speakers; 0 = stop when no merge lowers the BIC.")
    parser.add_argument("--diar_window_ms", type=float, default=1000.0, help="Each of the two adjacent windows of the change-point curve.")
    parser.add_argument("--diar_hop_ms", type=float, default=100.0, help="Distance between change-point candidates.")
    parser.add_argument("--diar_change_lambda", type=float, default=1.0, help="BIC penalty weight of the change points (larger: fewer).")
    parser.add_argument("--diar_cluster_lambda", type=float, default=1.0, help="BIC penalty weight of the clustering (larger: fewer speakers).")
    parser.add_argument("--rttm", type=str, default="", metavar="FILE", help="Also write the labelled segments in RTTM, one line each.")


BEAMFORM_DEFAULTS = dict(bf_window_ms=500.0, bf_max_delay_ms=10.0, bf_jump_penalty=0.01, bf_ref=0)
# the flags of --bf_method mvdr; --mvdr_floor_db: None = as --vad_floor_db
MVDR_DEFAULTS = dict(mvdr_frame_ms=32.0, mvdr_block_ms=2000.0, mvdr_top_db=25.0, mvdr_floor_db=None, mvdr_pad_ms=100.0, mvdr_loading=1e-3)
DELAYSUM_ONLY = ("bf_window_ms", "bf_max_delay_ms", "bf_jump_penalty")


def add_beamform_flags(parser):
    """the --beamform flags (kept here so that a run without --beamform never imports las.beamform).  The --bf_*
    values default to None here -- check_flags refuses one given without --beamform True and fills in BEAMFORM_DEFAULTS with it."""
    parser.add_argument("--beamform", type=str2bool, default=False, help="Accept multi-channel recordings (microphone arrays): GCC-PHAT delays "
                        "against --bf_ref per window, tracked over the windows, then delay-and-sum to one channel; no trained model.")
    parser.add_argument("--bf_window_ms", type=float, default=None, help="The analysis window, every half window (default 500).")
    parser.add_argument("--bf_max_delay_ms", type=float, default=None, help="The largest delay searched, either way (default 10).")
    parser.add_argument("--bf_jump_penalty", type=float, default=None, help="Viterbi penalty per sample of lag change per window (default 0.01).")
    parser.add_argument("--bf_ref", type=int, default=None, help="The reference channel (default 0).")
    parser.add_argument("--beamform_wav", type=str, default="", metavar="DIR", help="Also write every beamformed file as DIR/<stem>.wav (16-bit).")
    parser.add_argument("--bf_method", type=str, default="delaysum", choices=("delaysum", "mvdr"), help="delaysum: the tracked delays, whole-"
                        "sample shifts and a sum.  mvdr: a mask-driven MVDR beamformer in the STFT domain (noise covariance from the frames an "
                        "energy rule calls non-speech, speech covariance per block), which also cancels directional disturbances.")
    parser.add_argument("--mvdr_frame_ms", type=float, default=None, help="mvdr: the frame is the next power of two samples at or above this (default 32).")
    parser.add_argument("--mvdr_block_ms", type=float, default=None, help="mvdr: the weights are recomputed per block of this length (default 2000).")
    parser.add_argument("--mvdr_top_db", type=float, default=None, help="mvdr: speech = frames within this many dB of the loudest frame of "
                        "--bf_ref (default 25); everything else trains the noise covariance.")
    parser.add_argument("--mvdr_floor_db", type=float, default=None, help="mvdr: absolute floor of the mask rule (default: --vad_floor_db).")
    parser.add_argument("--mvdr_pad_ms", type=float, default=None, help="mvdr: the speech frames are widened by this much either way (default 100).")
    parser.add_argument("--mvdr_loading", type=float, default=None, help="mvdr: diagonal loading of the noise covariance, relative to its mean "
                        "diagonal (default 1e-3).")


def check_beamform_flags(args):
    """--beamform and its values: refusals before any audio is read; the defaults filled in (--bf_ref against a file's channels: at load time)"""
    given = [k for k in BEAMFORM_DEFAULTS if getattr(args, k, None) is not None]
    mvdr = [k for k in MVDR_DEFAULTS if getattr(args, k, None) is not None]
    method = getattr(args, "bf_method", None) or "delaysum"
    if method not in ("delaysum", "mvdr"):
        raise ValueError("--bf_method %r: delaysum or mvdr" % (method,))
    if not getattr(args, "beamform", False):
        if given or getattr(args, "beamform_wav", ""):
            raise ValueError("--%s sets the beamformer of --beamform True: give both" % (given[0] if given else "beamform_wav"))
        if method == "mvdr":
            raise ValueError("--bf_method mvdr chooses the beamformer of --beamform True: give both")
        if mvdr:
            raise ValueError("--%s sets the beamformer of --beamform True --bf_method mvdr: give all three" % mvdr[0])
        return False
    if method != "mvdr" and mvdr:
        raise ValueError("--%s sets the beamformer of --bf_method mvdr: give both" % mvdr[0])
    if method == "mvdr":
        idle = [k for k in DELAYSUM_ONLY if getattr(args, k, None) is not None]
        if idle:
            raise ValueError("--%s sets the delay tracker of --bf_method delaysum and would do nothing with --bf_method mvdr: use one of them" % idle[0])
    for k, v in BEAMFORM_DEFAULTS.items():
        if getattr(args, k, None) is None:
            setattr(args, k, v)
    from las import beamform as BF                                     # (las.beamform is imported only when the flag is given)
    BF.check_values(args.bf_window_ms, args.bf_max_delay_ms, args.bf_jump_penalty, args.bf_ref)
    if method == "mvdr":
        for k, v in MVDR_DEFAULTS.items():
            if getattr(args, k, None) is None:
                setattr(args, k, v)
        if args.mvdr_floor_db is None:
            floor_db = getattr(args, "vad_floor_db", None)
            args.mvdr_floor_db = -70.0 if floor_db is None else floor_db      # (las.vad.DEFAULTS["vad_floor_db"])
        BF.check_mvdr_values(args.mvdr_frame_ms, args.mvdr_block_ms, args.mvdr_top_db, args.mvdr_floor_db, args.mvdr_pad_ms, args.mvdr_loading)
    return True


def refuse(rows, message):
    for flag, on, why in rows:
        if on:
            raise ValueError(message % (flag, why))


def check_flags(args, parser):
    """every refusal of transcribe.py's flags, before anything is built, in the order that decides which one a combination gets; ->
    Mode(kind: keywords | align | search; ctc_only; annotate: an Annotator is needed; json: JSON lines).  Sets what a mode implies.
    The tables, per search-less mode: (flag, is on, what it does that the mode cannot go with)"""
    network = check_confusion_flags(args)
    consensus = bool(args.nbest or args.confidence or args.mbr or network)
    kind = "keywords" if args.keywords is not None else "align" if args.align_text is not None else "search"
    check_beamform_flags(args)
    diarize = bool(getattr(args, "diarize", False))
    if diarize:                                                        # (las.diarize is imported only when the flag is given)
        refuse((("--keywords", kind == "keywords", "prints keyword hits and runs no search"),
                ("--align_text", args.align_text is not None, "aligns one transcript per whole file")),
               "--diarize labels the segments a search transcribes, %s %s: use one of them")
        if not args.segment:
            raise ValueError("--diarize labels the segments of --segment True: give both")
        from las import diarize as DZ
        DZ.check_values(args.num_speakers, args.diar_window_ms, args.diar_hop_ms, args.diar_change_lambda, args.diar_cluster_lambda)
    elif getattr(args, "rttm", ""):
        raise ValueError("--rttm writes the speakers of --diarize True: give both")
    keywords = (("--align_text", args.align_text is not None, "aligns a given transcript"),
                ("--segment", args.segment, "cuts the recordings first; searching the segments is not built"),
                ("--timestamps", args.timestamps, "times the search's hypothesis"),
                ("--nbest", args.nbest, "reads the search's N-best list"),
                ("--confidence", args.confidence, "reads the search's N-best list"),
                ("--mbr", args.mbr, "reads the search's N-best list"))
    align = (("--segment", kind == "align" and args.segment, "cuts the recordings, --align_text aligns one transcript per whole file"),
             ("--nbest / --confidence / --mbr%s" % (" / --confusion_network" if network else ""), kind == "align" and consensus,
              "read the search's N-best list, --align_text skips the search"))
    if kind == "keywords":
        if not args.ctc:
            raise ValueError("--keywords needs the CTC head: decode with --ctc True (a model trained with --ctc)")
        refuse(keywords, "--keywords skips the search and prints keyword hits only, %s %s: use one of them")
        if not 1 <= args.keyword_max_hits <= 8:
            raise ValueError("--keyword_max_hits must be in [1, 8] (got %d)" % args.keyword_max_hits)
        if np.isnan(args.keyword_threshold):
            raise ValueError("--keyword_threshold is not a number")
    refuse(align[:1], "%s %s: use one of them")
    from las import coverage
    cover = coverage.from_args(args)                                   # (bad weights and thresholds are refused here)
    if kind != "search":
        coverage.refuse_without_attention(args, "--keywords" if kind == "keywords" else "--align_text")
        args.timestamps = args.timestamps or kind == "align"
        args.hotwords, args.hotword_weight = "", 0.0                  # (no search: nothing to bias)
        args.ngram_lm, args.ngram_weight = "", 0.0                    # (... and nothing to fuse an LM into)
    ctc_only = False
    if args.decoder != "attention" or args.rescore != "none":          # (las.ctc_search is imported only when one of the flags is given)
        from las import ctc_search
        ctc_only = ctc_search.check_args(args) and args.align_text is None
    if args.timestamps and not args.ctc:
        raise ValueError("--timestamps needs the CTC head: decode with --ctc True (a model trained with --ctc)")
    refuse(align[1:], "%s %s: use one of them")                        # (behind the head's refusals, which win over this row)
    if not args.synthetic and not args.audio:
        parser.error("no audio files (or --synthetic True)")
    if not args.cmvn:
        raise ValueError("the Listener takes the CMVN'd cube [T, feat_dim, 3]: transcribe with --cmvn True")
    report = cover is not None and cover.report                        # (--coverage_report prints the counts: JSON lines)
    return Mode(kind, ctc_only, consensus, kind != "search" or bool(args.timestamps) or consensus or report or diarize)


def load_lm(init_dir, store=None):
    """reference decode.py:27-39: build the inference CharRNN from `result.json` (hyper-parameters written by
    train_lm.py:270-272) and `vocab.json` of the LM output directory."""
    from lang.char_rnn_model import CharRNN
    with open(os.path.join(init_dir, 'result.json'), 'r') as f:
        result = json.load(f)
    params = dict(result['params'])
    with open(os.path.join(init_dir, 'vocab.json'), 'r') as f:
        vocab_index_dict = json.load(f)
    params.update(vocab_size=len(vocab_index_dict), num_unrollings=1, batch_size=1)
    logging.info('Creating rnnlm graph')
    lm = CharRNN(is_training=False, use_batch=True, store=store, **params)
    return lm, result


def restore_lm(lm, save_path):
    """reference decode.py:41-53: restore the LM's variables (this build: a torch-saved {name: array} dictionary written
    by train_lm.py; the names are the reference's TF variable names under the `lm` scope)."""
    import torch
    sd = torch.load(save_path, map_location="cpu", weights_only=True)
    lm.params()                                     # create the variables, then overwrite them
    lm.store.load({k: v for k, v in sd["params"].items() if k.startswith(lm.scope + "/")})
    logging.info("Rnnlm restored: {}".format(save_path))


def make_tokenizer(args):
    """the tokenizer of --unit; sets args.vocab_size"""
    from utils.tokenizer import CharEncoder, SubwordEncoder
    tokenizer = CharEncoder() if args.unit.lower() == "char" else SubwordEncoder(args.subword_dir)
    args.vocab_size = tokenizer.get_vocab_size()
    return tokenizer


def build_search(args, dev, ctc_only, restore_las, restore_lm_weights, log_lm=False, need_head=(), tokenizer=None):
    """the model of decode.py and transcribe.py on the current device dev: cell and precision, a fresh variable store, LAS, the RNN LM of
    --apply_lm (--synthetic without an LM directory: the shipped shape, random weights), BeamSearch, the checkpoint.  -> (tokenizer,
    BeamSearch, the restored checkpoint's path or None, the search of --decoder).  Where the entry points differ: restore_las, restore_lm_weights
    (those result.json names, when load_lm read one), log_lm, need_head (flags that read the CTC head: refused once a checkpoint lacks it)"""
    from las import layers, variables
    from las.beam_search import BeamSearch
    from las.las import LAS, Listener, Speller
    tokenizer = make_tokenizer(args) if tokenizer is None else tokenizer
    layers.set_cell(args.cell)
    layers.set_precision(args.dtype)
    variables.reset_default_store(device=dev, seed=args.seed)
    las = LAS(args, Listener, Speller, tokenizer.token_to_id)
    lm = result = ckpt = None
    if args.apply_lm:                                              # decode.py:68-75
        if log_lm:
            logging.info("Apply RNNLM...")
        st = variables.default_store()
        if args.synthetic and not os.path.exists(os.path.join(args.lm_dir, "result.json")):
            from lang.char_rnn_model import CharRNN
            lm = CharRNN(False, 1, 1, 28, 512, embedding_size=0, num_layers=2, store=st)
        else:
            lm, result = load_lm(args.lm_dir, st)
        lm.params()
    las.build_variables()
    bs = BeamSearch(args, las, tokenizer.token_to_id, lm)
    if restore_las:
        ckpt = bs.restore_las(None, args.save_dir, args.restore_epoch)
        logging.info("LAS restored: {}".format(ckpt))
    if restore_lm_weights and result is not None:
        restore_lm(lm, result['best_model'])
    for flag in need_head:
        bs.need_ctc_head(flag)
    return tokenizer, bs, ckpt, bs.ctc_decode_batches if ctc_only else bs.decode_batches


def encoded_batches(bs, batches):
    """the modes that skip the search: the listener and the CTC head of every batch -> (encs, enc_lens, h_one, ctc_lp)"""
    import torch
    for make in batches:
        with torch.no_grad():
            encs, enc_lens, _, h_one, ctc_lp = bs._run_encoders(None, make())
        yield encs, enc_lens, h_one, ctc_lp
