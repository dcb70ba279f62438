"""las.arguments -- the single flag namespace shared by train.py / test.py / decode.py.

Flag names, types and defaults are the drop-in contract (reference las/arguments.py:12-232; pinned by
golden G2).  They are declared as one table instead of fifty add_argument blocks; the MI355X build adds
a few flags of its own at the end (cell type, arithmetic mode, data-parallel bucket options)."""
import argparse


def str2bool(v):
    """'yes/true/t/y/1' -> True, 'no/false/f/n/0' -> False (case-insensitive), else ArgumentTypeError
    (reference las/arguments.py:4-10)."""
    s = v.lower()
    if s in ("yes", "true", "t", "y", "1"):
        return True
    if s in ("no", "false", "f", "n", "0"):
        return False
    raise argparse.ArgumentTypeError("Boolean value expected.")


# (flags, type, default, help)
_FLAGS = [
    # features
    (("--dataset",), str, "LibriSpeech", "Dataset: LibriSpeech or TEDLIUM."),
    (("--unit",), str, "subword", "Encoding unit for texts processing."),
    (("--sample_rate",), int, 16000, "Sample rate."),
    (("--feat_dim",), int, 39, "The feature dimension."),
    (("--frame_length",), int, 25, "Frame length in ms."),
    (("--frame_step",), int, 10, "Frame step in ms."),
    (("--feat_type",), str, "mfcc", "mfcc"),
    (("--cmvn",), str2bool, True, "Apply cmvn or not."),
    (("--augmentation",), str2bool, False, "Apply data augmentation or not."),
    (("--split",), str, "dev", "Split used for evaluation."),
    # training
    (("--verbose", "-vb"), int, 0, "Verbosity."),
    (("--batch_size", "-bs"), int, 32, "The training batch size."),
    (("--lr",), float, 1e-3, "The training learning rate."),
    (("--grad_clip",), float, 5, "Apply gradient clipping."),
    (("--dropout_rate",), float, 0.5, "The probability of drop out."),
    (("--epoch",), int, 10, "The number of training epochs."),
    (("--restore_epoch",), int, -1, "The epoch you want to restore."),
    (("--label_smoothing",), str2bool, True, "Apply label smoothing."),
    (("--apply_bn",), str2bool, False, "Apply batch normalization."),
    (("--add_vn",), str2bool, False, "Apply variational noise to weights."),
    (("--ctc",), str2bool, False, "Apply ctc."),
    (("--ctc_weight",), float, 0.2, "Weighting of ctc."),
    # Listener
    (("--enc_type",), str, "cnn", "Listener type: cnn or pblstm."),
    (("--enc_units",), int, 64, "The hidden dimension of the BLSTMs in Listener."),
    (("--num_enc_channels",), int, 32, "The number of channels in CNN layers of Listener."),
    (("--num_enc_layers",), int, 2, "The number of layers of BLSTMs in Listener."),
    # Attention
    (("--attention_size",), int, 128, "Attention size."),
    (("--loc_kernel_size",), int, 201, "Kernel size in location-aware attention."),
    (("--loc_num_channels",), int, 10, "Number of channels in location-aware attention"),
    (("--mode",), str, "add", "Additive attention or loction-aware attention."),
    # Speller
    (("--dec_units",), int, 128, "The hidden dimension of the LSTM in Speller."),
    (("--num_dec_layers",), int, 2, "The number of layers of LSTM in Speller."),
    (("--embedding_size",), int, 128, "The dimension of the embedding matrix is: [vocab_size, embedding_size]."),
    (("--scheduled_sampling",), str2bool, True, "Apply schduled sampling."),
    (("--warmup_step",), int, 100000, "Steps of pure teacher forcing before scheduled sampling starts."),
    (("--max_step",), int, 500000, "Max step in scheduled sampling."),
    (("--min_rate",), float, 0.4, "Minimum teacher-forcing rate in scheduled sampling."),
    # beam search
    (("--convert_rate",), float, 0.166, "Convert the length of audio to estimate the required decoding steps."),
    (("--beam_size",), int, 10, "Size for beam search."),
    (("--apply_lm",), str2bool, False, "Apply language model."),
    (("--lm_weight",), float, 0.5, "Weighting of recoring with language model."),
    # directories
    (("--train_100hr_corpus_dir",), str, "data/LibriSpeech/LibriSpeech_train/train-clean-100", ""),
    (("--train_360hr_corpus_dir",), str, "data/LibriSpeech/LibriSpeech_train/train-clean-360", ""),
    (("--train_500hr_corpus_dir",), str, "data/LibriSpeech/LibriSpeech_train/train-other-500", ""),
    (("--dev_data_dir",), str, "data/LibriSpeech-100/LibriSpeech_dev/dev-clean", ""),
    (("--test_data_dir",), str, "data/LibriSpeech-100/LibriSpeech_test/test-clean", ""),
    (("--feat_dir",), str, "data/LibriSpeech/features", "Path to save features."),
    (("--subword_dir",), str, "subword/", "Path to vocab files of BPE subword unit."),
    (("--log_dir",), str, "log/", "Save log file.."),
    (("--save_dir",), str, "model/las/", "Save trained model."),
    (("--summary_dir",), str, "summary/", "Save summary."),
]

# additions of the MI355X build (not in the reference; defaults keep reference behaviour)
_EXTRA = [
    (("--cell",), str, "rnn", "Recurrent cell: 'rnn' = BasicRNNCell as the reference builds, 'lstm' = BasicLSTMCell."),
    (("--dtype",), str, "f32", "Contraction arithmetic: f32 (parity) or bf16 (MFMA speed mode)."),
    (("--seed",), int, 0, "Initialiser seed."),
    (("--synthetic",), str2bool, False, "Train on synthetic [B,T,feat_dim,3] batches (no TFRecords needed)."),
    (("--max_steps",), int, -1, "Stop after this many steps (-1: run all epochs)."),
    (("--tfrecord_dir",), str, "", "Directory holding train-*.tfrecord / dev-1.tfrecord (default data/tfrecord_<feat>_bpe_5k)."),
    (("--stack",), int, 1, "Bucket batches per train step on one GPU (the reference's 48 / 96 rows times this; 1 = the reference). k batches in one "
                           "step are the update of k data-parallel ranks; the latency-bound recurrent sweeps make k = 2 / 4 cost 1.4 / 2.0 steps."),
    (("--decode_batch",), int, 64, "Utterances per device-resident beam-search batch in decode.py (rows of a search step = this x beam_size; "
                                  "64 x 16 rows decode 1.8x the utterances/s of 16 x 16)."),
    (("--ctc_decode_weight",), float, 0.0, "Weight of the CTC prefix scores in joint CTC-attention beam search (needs --ctc True; 0: attention "
                                           "(+ LM) scores only).  A candidate scores logit + weight * (CTC prefix score gain)."),
    (("--hotwords",), str, "", "Contextual biasing (las.bias): a file with one phrase per line ('#' lines are comments) whose tokens the beam "
                               "search boosts; needs --hotword_weight > 0."),
    (("--hotword_weight",), float, 0.0, "Bonus per matched token of a --hotwords phrase, taken back when the match breaks (0: off)."),
    (("--ngram_lm",), str, "", "N-gram LM shallow fusion (las.ngram): a back-off model over the model's own tokens in the ARPA text format "
                               "(train_ngram.py writes one); needs --ngram_weight > 0."),
    (("--ngram_weight",), float, 0.0, "Weight of the n-gram LM's natural-log probabilities in the beam search (0: off)."),
    # attention coverage in the beam search (las.coverage, csrc/coverage.hip): all off by default
    (("--coverage_weight",), float, 0.0, "Added to a hypothesis' score for every encoder frame whose accumulated attention rises above "
                                         "--coverage_threshold (against skipped audio; 0: off)."),
    (("--coverage_threshold",), float, 0.5, "A frame is covered once its accumulated attention exceeds this (Chorowski & Jaitly's 0.5)."),
    (("--overattend_weight",), float, 0.0, "Taken from a hypothesis' score for every encoder frame whose accumulated attention rises "
                                           "above --overattend_threshold (against loops; 0: off)."),
    (("--overattend_threshold",), float, 1.5, "A frame is over-attended once its accumulated attention exceeds this (a guess: no WER "
                                              "has been measured for any of these values)."),
    (("--coverage_report",), str2bool, False, "Count covered and over-attended frames whatever the weights; transcribe.py prints JSON lines "
                                              "with \"coverage\" and \"overattended\", the shares of the utterance's encoder frames."),
    # CTC-only decoding (las.ctc_search, csrc/ctc_search.hip): the default is the Speller's search
    (("--decoder",), str, "attention", "Search of transcribe.py / decode.py: attention = the Speller's beam search; ctc = the CTC head alone "
                                       "(needs --ctc True): --beam_size 1 is the greedy collapse, > 1 the prefix beam search, with "
                                       "--ngram_lm fused."),
    (("--ctc_cand",), int, 32, "--decoder ctc: classes of largest logit a frame offers the prefix beam search (at most 64)."),
    (("--ctc_len_bonus",), float, 0.0, "--decoder ctc: added to the score of every token the prefix beam search appends."),
    # two-pass decoding (las.rescore, csrc/rescore.hip): off by default
    (("--rescore",), str, "none", "--decoder ctc: none, or attention = the Speller scores the prefix beam search's hypotheses under teacher "
                                  "forcing and the list is re-ranked (needs --beam_size > 1)."),
    (("--rescore_ctc_weight",), float, 0.5, "--rescore attention: a hypothesis ranks by (1 - w) x attention log-likelihood + w x CTC search "
                                            "score, w inside [0, 1]."),
    (("--rescore_rows",), int, 64, "--rescore attention: hypotheses per teacher-forced Speller call (1 to 1024)."),
    # N-best consensus (las.nbest, csrc/nbest.hip): all off by default
    (("--nbest",), int, 0, "transcribe.py: every JSON line lists the K best hypotheses with their posteriors (K <= --beam_size; 0: off)."),
    (("--confidence",), str2bool, False, "transcribe.py: every JSON line carries the printed hypothesis' posterior and a confidence per word."),
    (("--mbr",), str2bool, False, "Print the minimum-Bayes-risk hypothesis of the N-best list (least expected token edit distance under the "
                                  "posteriors) instead of the top-scoring one."),
    (("--nbest_scale",), float, 1.0, "Scale of the search's ranking key in the softmax that gives the N-best posteriors."),
    # N-best confusion network (las.nbest, las_nbest_network): all off by default
    (("--confusion_network",), str2bool, False, "transcribe.py: every JSON line carries \"network\", the word alternatives per position "
                                                "(the N-best list merged into a confusion network) with their posterior masses."),
    (("--cn_decode",), str2bool, False, "Print the consensus of the confusion network (the most probable word at every position) instead "
                                        "of the top-scoring hypothesis."),
    (("--cn_alternatives",), int, 3, "--confusion_network: alternatives listed per position (1 to 8)."),
    (("--cn_unit",), str, "word", "Symbols of the confusion network: word (a word is its printed text) or token."),
    (("--lm_dir",), str, "lang/output/", "Output directory of train_lm.py (result.json, vocab.json, models) for --apply_lm."),
    (("--frontend",), str, "cpu", "Feature extraction of preprocess.py: cpu = the float64 numpy restatement, gpu = the HIP front end "
                                  "(las.frontend.FeatureExtractor, fp32)."),
    # SpecAugment in training (las.specaug, csrc/specaug.hip): off by default
    (("--spec_augment",), str2bool, False, "Warp and mask the feature cube of every train step on the device (SpecAugment)."),
    (("--specaug_time_warp",), int, 80, "SpecAugment: maximum time warp distance W in frames (0: no warp)."),
    (("--specaug_freq_masks",), int, 2, "SpecAugment: number of frequency masks."),
    (("--specaug_freq_width",), int, -1, "SpecAugment: maximum frequency mask width in bins (-1: max(1, feat_dim // 3), the paper's 27 of 80)."),
    (("--specaug_time_masks",), int, 2, "SpecAugment: number of time masks."),
    (("--specaug_time_width",), int, 100, "SpecAugment: maximum time mask width in frames."),
    (("--specaug_time_ratio",), float, 1.0, "SpecAugment: a time mask covers at most this share of the utterance's frames."),
    # multi-condition data (las.augment, csrc/wave_aug.hip): room reverberation and additive noise; all off by default
    (("--rir_dir",), str, "", "Directory of room impulse responses (.wav / .npy, resampled to --sample_rate) for --noisy_copies."),
    (("--noise_dir",), str, "", "Directory of background noise recordings (.wav / .npy, resampled to --sample_rate) for --noisy_copies."),
    (("--rir_synthetic",), int, 0, "Add N synthetic room responses (seeded Gaussian tails, preprocess.synthetic_rir) to the response bank."),
    (("--rt60",), str, "0.2,0.8", "lo,hi: the reverberation times in seconds of the --rir_synthetic responses are drawn from this range."),
    (("--snr_range",), str, "5,20", "lo,hi: the signal-to-noise ratio in dB of every noisy utterance is drawn from this range."),
    (("--reverb_prob",), float, 0.5, "Share of the utterances of a noisy copy that are reverberated."),
    (("--noisy_copies",), int, 0, "preprocess.py --augmentation True: additionally write K reverberated / noisy copies of every train "
                                  "split (noisy_<k>-feats.pkl, noisy_<k>-featlen.npy) beside the speed_* dumps (0: none)."),
    (("--noise_file",), str, "", "transcribe.py: mix this recording into every file at --snr_db before it is transcribed."),
    (("--snr_db",), float, 10.0, "transcribe.py: the signal-to-noise ratio in dB of --noise_file."),
    (("--rir_file",), str, "", "transcribe.py: convolve every file with this room impulse response before it is transcribed."),
    # minimum word error rate training (las.mwer, csrc/mwer.hip): off by default
    (("--mwer",), str2bool, False, "Train on the expected number of word errors over K hypotheses per utterance (MWER) plus a weighted "
                                   "cross entropy on the reference, instead of the cross entropy alone."),
    (("--mwer_hyps",), int, 4, "--mwer: hypotheses K per utterance (1 to 63), drawn inside the Speller loop unless LAS.train gets hyps=."),
    (("--mwer_ce_weight",), float, 0.01, "--mwer: weight of the reference's cross entropy beside the expected word errors."),
    (("--mwer_unit",), str, "word", "--mwer: errors are counted in words (one device-to-host read-back per step for the word mapping) or "
                                    "in tokens (none)."),
    (("--mwer_norm",), str, "", "--mwer: sample = every hypothesis weighs 1 / K (the default for drawn hypotheses: duplicates would be "
                                "counted twice under nbest), nbest = the model's posterior renormalised over the list (the default "
                                "with hyps=)."),
    (("--mwer_extra_steps",), int, 4, "--mwer: drawn hypotheses may be this many steps longer than the reference."),
]


def build_parser(extra=True):
    parser = argparse.ArgumentParser(
        description="Listen, Attend and Spell (LAS) end-to-end speech recognition on MI355X")
    for flags, typ, default, helptext in _FLAGS + (_EXTRA if extra else []):
        parser.add_argument(*flags, type=typ, default=default, help=helptext)
    return parser


def parse_args(argv=None):
    """reference las/arguments.py:12 (argv=None -> sys.argv[1:])."""
    return build_parser().parse_args(argv)


def check_confusion_flags(args):
    """--confusion_network / --cn_decode against the flags they cannot go with: a ValueError before anything is built.  Reads every flag
    with a default, so a namespace from before these flags (or without transcribe.py's own) passes.  -> True when one of the two is on"""
    cn, dec = bool(getattr(args, "confusion_network", False)), bool(getattr(args, "cn_decode", False))
    if not (cn or dec):
        return False
    top, unit = int(getattr(args, "cn_alternatives", 3)), str(getattr(args, "cn_unit", "word"))
    if not 1 <= top <= 8:
        raise ValueError("--cn_alternatives must be in [1, 8] (got %d)" % top)
    if unit not in ("word", "token"):
        raise ValueError("--cn_unit %s: word or token" % unit)
    if getattr(args, "keywords", None) is not None:
        raise ValueError("--keywords skips the search and prints keyword hits only, --confusion_network / --cn_decode read the search's "
                         "N-best list: use one of them")
    if dec and getattr(args, "mbr", False):
        raise ValueError("--cn_decode prints the network's consensus, --mbr the listed hypothesis of least risk: use one of them")
    if dec and (getattr(args, "timestamps", False) or getattr(args, "align_text", None) is not None):
        raise ValueError("--cn_decode prints a hypothesis no search produced; aligning it (--timestamps / --align_text) is not built")
    return True


def reference_flag_names():
    return [f[0][0].lstrip("-") for f in _FLAGS]
