"""decode.py -- beam-search evaluation entry point (counterpart of the reference's decode.py: utterances
sorted by token length, one BeamSearch.decode per utterance, per-utterance and corpus WER, same log lines).
--mbr True scores the minimum-Bayes-risk hypothesis of every N-best list (las.nbest; posteriors at --nbest_scale) instead of the
top-scoring one: the effect on the corpus WER is read from the same log lines.  --cn_decode True scores the consensus of every list's
confusion network (las_nbest_network) in the same way; the two cannot be combined.  With --coverage_weight /
--overattend_weight / --coverage_report (las.coverage) a last line logs the scored hypotheses' mean shares of covered and
over-attended encoder frames."""
import logging
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from las.arguments import check_confusion_flags, parse_args       # noqa: E402
from las.cli import build_search, load_lm, restore_lm              # noqa: E402,F401
from las.utils import convert_idx_to_string, edit_distance        # noqa: E402


def main():
    import torch
    args = parse_args()
    check_confusion_flags(args)
    logging.basicConfig(stream=sys.stdout, format='%(asctime)s %(levelname)s:%(message)s', level=logging.INFO, datefmt='%I:%M:%S')
    # replicas only: under torch.distributed.run every rank decodes its round-robin share of the
    # length-sorted utterance list and the (errors, words) counts are all-reduced at the end
    from las import parallel
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dp = parallel.init_from_env(dev)
    rank, world = (dp.rank, dp.world) if dp is not None else (0, 1)
    ctc_only = False
    if args.decoder != "attention" or args.rescore != "none":      # (las.ctc_search is imported only when one of the flags is given)
        from las import ctc_search
        ctc_only = ctc_search.check_args(args)
    tokenizer, bs, _, search = build_search(args, dev, ctc_only, restore_las=True, restore_lm_weights=True, log_lm=True)
    id_to_token = tokenizer.id_to_token
    if args.synthetic:
        from data import SyntheticBatches
        (audio, audiolen), (y, tokenlen) = next(SyntheticBatches(args.feat_dim, args.vocab_size, seed=args.seed + 2, batch_scale=0.1, max_frames=700))
        dev_feats = [audio[i, :audiolen[i]] for i in range(len(audio))]
        dev_tokens = list(y)
    elif os.path.exists(os.path.join(args.feat_dir, "{}-feats.pkl".format(args.split))):
        import joblib                                              # decode.py:80-85: the preprocess.py dumps
        dev_feats = joblib.load(args.feat_dir + "/{}-feats.pkl".format(args.split))
        dev_tokens = np.load(args.feat_dir + "/{}-{}s.npy".format(args.split, args.unit), allow_pickle=True)
        tokenlen = np.load(args.feat_dir + "/{}-{}len.npy".format(args.split, args.unit), allow_pickle=True)
    else:
        # same utterances from the packed split (create_tfrecord.py writes {split}-1.tfrecord)
        from tfrecord_data_loader import data_parser, tf_record_iterator
        path = os.path.join(args.tfrecord_dir or "data/tfrecord_{}_bpe_5k".format(args.feat_type), "{}-1.tfrecord".format(args.split))
        if not os.path.exists(path):
            raise Exception("Run preprocess.py first")
        recs = [data_parser(r) for r in tf_record_iterator(path)]
        dev_feats = [r[0][0] for r in recs]
        dev_tokens = [r[1][0] for r in recs]
        tokenlen = np.asarray([r[1][1] for r in recs])
    order = np.argsort(tokenlen)                                   # decode.py:122-124
    error, N, count = 0, 0, 0
    cov_sum, cov_n = np.zeros(2), 0                                # --coverage_*: the chosen hypotheses' covered / over-attended shares
    logging.info("Decoding...")
    limit = args.max_steps if args.max_steps >= 0 else (8 if args.synthetic else len(order))
    todo = parallel.shard(list(order[:limit]), rank, world)
    nb = max(1, int(args.decode_batch))
    chunks = [todo[c0:c0 + nb] for c0 in range(0, len(todo), nb)]  # decode.py:131-149, `decode_batch` utterances per call

    def batches():
        for chunk in chunks:
            xs_list = []
            for i in chunk:
                audio = np.asarray(dev_feats[i], np.float32)
                xs_list.append((audio[None], np.asarray([audio.shape[0]], np.int32)))
            yield xs_list

    ann = None
    if args.mbr or args.cn_decode:                                 # (las.nbest is imported only when one of the flags is given)
        from las import nbest as NB
        args.nbest, args.confidence, args.confusion_network = 0, False, False      # (transcribe.py's: nothing here prints them)
        ann = NB.Annotator(args, bs.end_id, id_to_token)
    # the model's objects live as long as the process: out of the cyclic collector's way (a full collection walks them all, 30-60 ms --
    # a batch and a half -- every few batches otherwise)
    import gc
    gc.collect()
    gc.freeze()
    # decode_batches: the encoders of the next chunk run under the search of this one (--decoder ctc: the CTC head's search)
    for chunk, results in zip(chunks, search(None, batches())):
        notes = ann.annotate(results) if ann is not None else [None] * len(results)
        chosen = [r[-1] for r in results] if ann is None else [a["state"] if a["state"] is not None else r[-1]
                                                               for a, r in zip(notes, results)]
        for i, state, a in zip(chunk, chosen, notes):
            if a is not None and "consensus" in a:                 # --cn_decode: the network's consensus, a text no search produced
                hyp = a["consensus"]["text"]
            else:
                hyp = convert_idx_to_string(state.token_ids[1:], id_to_token, args.unit)
                if getattr(state, "coverage", None) is not None:
                    covered, over, frames = state.coverage
                    cov_sum += np.array([covered, over]) / max(frames, 1)
                    cov_n += 1
            ref = convert_idx_to_string(dev_tokens[i], id_to_token, args.unit)
            dist, n = edit_distance(ref.split(" "), hyp.split(" "))
            error += dist
            N += n
            logging.info("Utt {}/{}, WER: {}".format(count, len(order), dist / n))
            count += 1
            if args.verbose > 0:
                logging.info("REF | {}".format(ref))
                logging.info("HYP | {}\n".format(hyp))
    error, N = parallel.reduce_error_counts(dp, error, N, dev)
    if cov_n:                                                      # (this rank's share of the utterances)
        logging.info("Coverage: {:.4f} of the encoder frames attended, {:.4f} over-attended ({} utterances)".format(
            cov_sum[0] / cov_n, cov_sum[1] / cov_n, cov_n))
    if rank == 0:
        logging.info("Dev WER: {}".format(error / N))


if __name__ == "__main__":
    main()
