"""train_ngram.py -- estimate a back-off n-gram LM over the model's own tokens from transcripts and write it as an ARPA file for
`decode.py` / `transcribe.py --ngram_lm lm.arpa --ngram_weight W` (las.ngram).  Host only: numpy and Python.

    python train_ngram.py --data_file transcripts.txt --order 3 --unit subword --subword_dir subword/ --output lm.arpa

One transcript per line; a line is upper-cased like the transcripts, encoded with the tokenizer (with_eos=True) and gets <s> in front.
Interpolated Witten-Bell smoothing, written in back-off form.  With c(.) the counts, T(h) the number of distinct tokens seen after h
and h' = h without its first token:
    seen (h, v):   p(v | h) = (c(hv) + T(h) p(v | h')) / (c(h) + T(h))          bow(h) = T(h) / (c(h) + T(h))
    unigrams:      p(v) = (c(v) + T() / (V - 2)) / (c() + T())                   for every token v other than PAD and SOS
so every token has a unigram and every context's distribution sums to 1 over the V - 2 tokens.  <s> is never predicted: it gets -99
(the ARPA convention) and keeps its back-off weight."""
import argparse
import collections
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def estimate(sentences, order, vocab_size, sos_id=1, eos_id=2, pad_id=0):
    """sentences: token-id lists, each starting with SOS and ending with EOS -> {token tuple: (log10 p, log10 bow)}"""
    from las.ngram import MAX_ORDER, UNSEEN
    n, V = int(order), int(vocab_size)
    if not 1 <= n <= MAX_ORDER:
        raise ValueError("train_ngram: the order must be in [1, %d] (got %d)" % (MAX_ORDER, n))
    if V < 3:
        raise ValueError("train_ngram: a vocabulary of %d tokens has none besides PAD and SOS" % V)
    counts = [collections.Counter() for _ in range(n)]
    for s in sentences:
        s = [int(t) for t in s]
        for t in s:
            if not 0 <= t < V:
                raise ValueError("train_ngram: token %d outside [0, %d)" % (t, V))
        for i in range(len(s)):
            for k in range(1, min(n, len(s) - i) + 1):
                counts[k - 1][tuple(s[i:i + k])] += 1
    # <s> and PAD are never predicted: an n-gram that holds PAD, or <s> anywhere but in front, is dropped (with everything it is a prefix
    # of, so the set stays prefix-closed) -- a PAD inside a transcript cuts the context there
    for k in range(n):
        for key in [key for key in counts[k] if pad_id in key or sos_id in key[1:]]:
            del counts[k][key]
    ctx_c, ctx_t = collections.Counter(), collections.Counter()      # c(h), T(h) by context, the empty one included
    for k in range(n):
        for key, c in counts[k].items():
            if k == 0 and key[0] == sos_id:
                continue
            ctx_c[key[:-1]] += c
            ctx_t[key[:-1]] += 1
    prob = {}
    c0, t0 = ctx_c[()], ctx_t[()]
    for v in range(V):
        if v in (sos_id, pad_id):
            continue
        prob[(v,)] = (counts[0][(v,)] + t0 / (V - 2.0)) / (c0 + t0) if c0 else 1.0 / (V - 2.0)
    for k in range(1, n):
        for key in sorted(counts[k]):
            h = key[:-1]
            prob[key] = (counts[k][key] + ctx_t[h] * prob[key[1:]]) / (ctx_c[h] + ctx_t[h])
    grams = {}
    bow = lambda key: math.log10(ctx_t[key] / float(ctx_c[key] + ctx_t[key])) if (len(key) < n and ctx_c[key]) else 0.0
    for key, p in prob.items():
        grams[key] = (math.log10(p), bow(key))
    grams[(sos_id,)] = (UNSEEN, bow((sos_id,)))
    return grams


def encode_lines(lines, tokenizer, sos_id):
    out = []
    for ln, line in enumerate(lines, 1):
        text = " ".join(line.upper().split())
        if not text:
            continue
        try:
            ids = list(tokenizer.encode(text, with_eos=True))
        except KeyError as e:                                # the char unit: a character outside its 30 symbols
            raise ValueError("train_ngram: line %d: character %s is not in the vocabulary (%r)" % (ln, e, text))
        out.append([sos_id] + ids)
    return out


def train(lines, tokenizer, order, output):
    from las.ngram import write_arpa
    t2i = tokenizer.token_to_id
    sos, eos, pad = t2i["<SOS>"], t2i["<EOS>"], t2i.get("<PAD>", 0)
    V = tokenizer.get_vocab_size()
    grams = estimate(encode_lines(lines, tokenizer, sos), order, V, sos, eos, pad)
    write_arpa(output, grams, order, tokenizer.id_to_token, sos, eos)
    return grams


def main(argv=None):
    ap = argparse.ArgumentParser(description="estimate a Witten-Bell back-off n-gram LM over the model's tokens (ARPA output)")
    ap.add_argument("--data_file", type=str, required=True, help="one transcript per line")
    ap.add_argument("--order", type=int, default=3)
    ap.add_argument("--unit", type=str, default="subword", help="char or subword")
    ap.add_argument("--subword_dir", type=str, default="subword/")
    ap.add_argument("--output", type=str, default="lm.arpa")
    o = ap.parse_args(argv)
    from utils.tokenizer import CharEncoder, SubwordEncoder
    tokenizer = CharEncoder() if o.unit.lower() == "char" else SubwordEncoder(o.subword_dir)
    with open(o.data_file, encoding="utf-8") as f:
        grams = train(f, tokenizer, o.order, o.output)
    by = collections.Counter(len(k) for k in grams)
    print("train_ngram: %s  (%s)" % (o.output, ", ".join("%d %d-grams" % (by[k], k) for k in sorted(by))))


if __name__ == "__main__":
    main()
