"""las.ngram -- a back-off n-gram language model over the model's own tokens, fused into the beam search: the host side.

Model.  Order n, 1 <= n <= MAX_ORDER, over token ids [0, V).  grams = {token tuple: (log10 p, log10 back-off weight)}; the back-off
weight of a highest-order n-gram is ignored, an absent one is 0.  Textbook scoring: log p(v | h) = logp(h, v) when (h, v) is stored,
else bow(h) + log p(v | h[1:]) with bow(h) = 0 for an h that is not stored; the recursion ends at the unigrams, which are dense (a
missing one takes the <unk> entry's value, PAD and SOS take -99, anything else is a ValueError).  The set must be prefix-closed.

Trie.  Node 0 is the root (the empty context); every stored n-gram of order 1 .. n-1 is a node, highest-order n-grams are entries only.
bo(s) = the node of the longest proper suffix of s that is a node; an entry's next = the longest suffix of (context . token) that is a
node.  A hypothesis carries the node of the longest suffix of its token string (SOS first) that is a node.  Transition on token c from
node p: descend p, bo(p), ... to the first node that has c as a child (the root always has it) and take that entry's next; a token
outside [0, V) goes to the root.

Tables (numpy; las_ngram_step, csrc/ngram.hip, header section K10f, walks them):
  child_off int32 [M + 1] (the root's list is empty: the unigrams are dense); child_tok int32 [E], ascending inside a node;
  child_lp float32 [E]; child_next int32 [E]; bow float32 [M]; bo int32 [M]; uni_lp float32 [V]; uni_next int32 [V].
.tables(w) are the copies the device gets: every log10 value times w ln 10, computed in float64 and rounded ONCE to float32.
Scores of a row whose node is s, over the chain s0 = s, s1 = bo(s0), ..., root, acc0 = 0: every child v of s_i that no deeper level
held gets score[v] = fl32(score[v] + fl32(acc_i + wlp(s_i, v))); acc_{i+1} = fl32(acc_i + wbow(s_i)); at the root the unigram table.

Limits, checked here before anything is launched (they are the kernel's): order <= 6, at most MAX_NODES = 2^22 nodes (a node travels
through the search as a float32), V <= MAX_V = 16384 (the kernel's mark table in LDS)."""
import math
import os

import numpy as np

MAX_NODES = 1 << 22
MAX_V = 16384
MAX_ORDER = 6
LN10 = math.log(10.0)
UNSEEN = -99.0                      # the ARPA convention for <s>: a token the model never predicts


def _check_weight(w, what):
    w = float(w)
    if not np.isfinite(w) or w < 0:
        raise ValueError("%s must be finite and >= 0 (got %r)" % (what, w))
    return w


class NgramLM(object):
    def __init__(self, grams, order, vocab_size, sos_id=1, eos_id=2, pad_id=0, unk_logp=None):
        n, V = int(order), int(vocab_size)
        if not 1 <= n <= MAX_ORDER:
            raise ValueError("NgramLM: the order must be in [1, %d] (got %d)" % (MAX_ORDER, n))
        if V < 2 or V > MAX_V:
            raise ValueError("NgramLM: vocab_size must be in [2, %d] (got %d)" % (MAX_V, V))
        self.order, self.vocab_size = n, V
        self.sos_id, self.eos_id, self.pad_id = int(sos_id), int(eos_id), int(pad_id)
        g = {}
        for key, val in grams.items():
            key = tuple(int(t) for t in key)
            if not 1 <= len(key) <= n:
                raise ValueError("NgramLM: n-gram %r has %d tokens, the order is %d" % (key, len(key), n))
            for t in key:
                if not 0 <= t < V:
                    raise ValueError("NgramLM: n-gram %r holds token %d outside [0, %d)" % (key, t, V))
            lp, bw = float(val[0]), float(val[1])
            if not np.isfinite(lp) or not np.isfinite(bw):
                raise ValueError("NgramLM: n-gram %r holds a value that is not finite" % (key,))
            if lp > 0:
                raise ValueError("NgramLM: n-gram %r has the positive log-probability %r" % (key, lp))
            g[key] = (lp, bw)
        for v in range(V):                                   # the unigrams are dense
            if (v,) not in g:
                if unk_logp is not None:
                    g[(v,)] = (float(unk_logp), 0.0)
                elif v in (self.pad_id, self.sos_id):
                    g[(v,)] = (UNSEEN, 0.0)
                else:
                    raise ValueError("NgramLM: token %d has no unigram and the model has no <unk>" % v)
        for key in sorted(g, key=lambda k: (len(k), k)):
            if len(key) > 1 and key[:-1] not in g:
                raise ValueError("NgramLM: n-gram %r is stored, its prefix %r is not" % (key, key[:-1]))
        self.grams = g
        # ---- nodes: the root, then the stored n-grams of order 1 .. n - 1 by (length, tokens); the unigram (v,) is node 1 + v
        nodes = [()] + sorted((k for k in g if len(k) < n), key=lambda k: (len(k), k))
        M = len(nodes)
        if M > MAX_NODES:
            raise ValueError("NgramLM: %d nodes; a node travels as a float32 value, at most %d" % (M, MAX_NODES))
        idx = {k: i for i, k in enumerate(nodes)}
        self._node_of, self.nodes = idx, nodes

        def longest(seq):                                    # the node of the longest suffix of seq that is a node
            seq = tuple(seq)[-(n - 1):] if n > 1 else ()
            for k in range(len(seq), 0, -1):
                s = idx.get(seq[-k:])
                if s is not None:
                    return s
            return 0
        self.num_nodes = M
        self.bo = np.asarray([0] + [longest(k[1:]) for k in nodes[1:]], np.int32)
        self._bow64 = np.asarray([0.0] + [g[k][1] for k in nodes[1:]], np.float64)
        kids = [[] for _ in range(M)]
        for key in g:
            if len(key) > 1:
                kids[idx[key[:-1]]].append(key[-1])
        off = np.zeros(M + 1, np.int32)
        tok, lp, nxt = [], [], []
        for s in range(M):
            for t in sorted(kids[s]):
                key = nodes[s] + (t,)
                tok.append(t); lp.append(g[key][0]); nxt.append(longest(key))
            off[s + 1] = len(tok)
        self.child_off = off
        self.child_tok = np.asarray(tok, np.int32).reshape(-1)
        self.child_next = np.asarray(nxt, np.int32).reshape(-1)
        self._lp64 = np.asarray(lp, np.float64).reshape(-1)
        self._uni64 = np.asarray([g[(v,)][0] for v in range(V)], np.float64)
        self.uni_next = np.asarray([longest((v,)) for v in range(V)], np.int32)
        self.child_lp = self._lp64.astype(np.float32)
        self.bow = self._bow64.astype(np.float32)
        self.uni_lp = self._uni64.astype(np.float32)
        self._scaled, self._dev = {}, {}

    @property
    def num_entries(self):
        return int(self.child_tok.size)

    # ---- the ARPA text format
    @classmethod
    def from_arpa(cls, path, token_to_id, vocab_size):
        """\\data\\, `ngram k=N`, \\k-grams:, lines `logp<ws>w1 ... wk[<ws>bow]`, \\end\\.  <s> -> <SOS>, </s> -> <EOS>, <unk> fills the
        missing unigrams (higher-order n-grams that hold it are skipped), every other name through token_to_id."""
        if not path or not os.path.isfile(path):
            raise ValueError("ngram LM: no such file %r" % (path,))
        V = int(vocab_size)
        if V > MAX_V:
            raise ValueError("ngram LM %s: vocab_size %d; las_ngram_step handles at most %d tokens" % (path, V, MAX_V))
        sos, eos, pad = token_to_id["<SOS>"], token_to_id["<EOS>"], token_to_id.get("<PAD>", 0)
        where = lambda ln: "ngram LM %s, line %d" % (path, ln)
        header, grams, seen = {}, {}, {}
        unk, k, state, ended = None, 0, "start", False
        with open(path, encoding="utf-8") as f:
            for ln, line in enumerate(f, 1):
                text = line.strip()
                if not text:
                    continue
                if state == "start":
                    if text == "\\data\\":
                        state = "data"
                    continue                                 # (free text in front of \data\)
                if text == "\\end\\":
                    ended = True
                    break
                if text.startswith("\\"):
                    if not text.endswith("-grams:") or not text[1:-7].isdigit():
                        raise ValueError("%s: unknown section %r" % (where(ln), text))
                    k = int(text[1:-7])
                    if k > MAX_ORDER:
                        raise ValueError("%s: order %d; at most %d" % (where(ln), k, MAX_ORDER))
                    if k not in header or k in seen:
                        raise ValueError("%s: section %r has no `ngram %d=` line or comes twice" % (where(ln), text, k))
                    seen[k] = [0, ln]
                    state = "grams"
                    continue
                if state == "data":
                    if not text.startswith("ngram ") or "=" not in text:
                        raise ValueError("%s: expected `ngram k=N`, got %r" % (where(ln), text))
                    a, b = text[6:].split("=", 1)
                    try:
                        ka, nb = int(a), int(b)
                    except ValueError:
                        raise ValueError("%s: expected `ngram k=N`, got %r" % (where(ln), text))
                    if ka > MAX_ORDER:
                        raise ValueError("%s: order %d; at most %d" % (where(ln), ka, MAX_ORDER))
                    if ka < 1 or nb < 0 or ka in header:
                        raise ValueError("%s: bad or repeated `ngram %d=%d`" % (where(ln), ka, nb))
                    header[ka] = nb
                    continue
                fields = text.split()
                if len(fields) not in (k + 1, k + 2):
                    raise ValueError("%s: a %d-gram line has %d or %d fields (got %d)" % (where(ln), k, k + 1, k + 2, len(fields)))
                try:
                    lp = float(fields[0])
                    bw = float(fields[k + 1]) if len(fields) == k + 2 else 0.0
                except ValueError:
                    raise ValueError("%s: %r holds no number where one belongs" % (where(ln), text))
                if not np.isfinite(lp) or not np.isfinite(bw):
                    raise ValueError("%s: a value that is not finite (%r)" % (where(ln), text))
                if lp > 0:
                    raise ValueError("%s: the positive log-probability %r" % (where(ln), lp))
                seen[k][0] += 1
                names = fields[1:k + 1]
                if "<unk>" in names:
                    if k == 1:
                        if unk is not None:
                            raise ValueError("%s: duplicate n-gram %r" % (where(ln), " ".join(names)))
                        unk = lp
                    continue
                key = []
                for nm in names:
                    t = sos if nm == "<s>" else eos if nm == "</s>" else token_to_id.get(nm)
                    if t is None:
                        raise ValueError("%s: unknown token %r" % (where(ln), nm))
                    if not 0 <= int(t) < V:
                        raise ValueError("%s: token %r has id %d outside [0, %d)" % (where(ln), nm, int(t), V))
                    key.append(int(t))
                key = tuple(key)
                if key in grams:
                    raise ValueError("%s: duplicate n-gram %r" % (where(ln), " ".join(names)))
                if k > 1 and key[:-1] not in grams:
                    raise ValueError("%s: n-gram %r is stored, its prefix %r is not" % (where(ln), " ".join(names), " ".join(names[:-1])))
                grams[key] = (lp, bw)
        if state == "start" or not ended:
            raise ValueError("ngram LM %s: no \\data\\ ... \\end\\ (not an ARPA file, or cut short)" % path)
        for ka in sorted(header):
            got, ln = seen.get(ka, [0, 0])
            if got != header[ka]:
                raise ValueError("%s: %d %d-grams, the header says %d" % (where(ln) if ln else "ngram LM %s" % path, got, ka, header[ka]))
        order = max([ka for ka in header if header[ka] > 0] or [1])
        try:
            return cls(grams, order, V, sos, eos, pad, unk_logp=unk)
        except ValueError as e:
            raise ValueError("ngram LM %s: %s" % (path, e))

    # ---- the device's tables
    def tables(self, weight):
        """the pre-scaled tables of weight w: w ln10 x (log10 value) in float64, rounded once to float32"""
        w = _check_weight(weight, "NgramLM.tables: the weight")
        if w not in self._scaled:
            c = np.float64(w) * np.float64(LN10)
            t = {"child_off": self.child_off, "child_tok": self.child_tok, "child_next": self.child_next, "bo": self.bo,
                 "uni_next": self.uni_next, "child_lp": (c * self._lp64).astype(np.float32), "bow": (c * self._bow64).astype(np.float32),
                 "uni_lp": (c * self._uni64).astype(np.float32)}
            if not all(np.all(np.isfinite(t[k])) for k in ("child_lp", "bow", "uni_lp")):
                raise ValueError("NgramLM.tables: the weight %r takes a table value out of float32" % w)
            self._scaled[w] = t
        return self._scaled[w]

    def to(self, device, weight):
        """the pre-scaled tables on `device`, uploaded once per (device, weight): a dict of tensors"""
        import torch
        key = (str(torch.device(device)), float(weight))
        if key not in self._dev:
            t = self.tables(weight)
            pad = lambda a: a if a.size else np.zeros(1, a.dtype)     # (order 1: valid addresses nobody reads)
            self._dev[key] = {k: torch.as_tensor(np.ascontiguousarray(pad(a))).to(device) for k, a in t.items()}
        return self._dev[key]

    # ---- the tables walked on the host (what the kernel does, for tests and tools)
    def _find(self, s, v):
        lo, hi = int(self.child_off[s]), int(self.child_off[s + 1])
        k = lo + int(np.searchsorted(self.child_tok[lo:hi], v))
        return k if k < hi and self.child_tok[k] == v else -1

    def step(self, node, token):
        """-> the node after `token` entered a hypothesis whose node was `node`"""
        v = int(token)
        if not 0 <= v < self.vocab_size:
            return 0
        q = int(node)
        for _ in range(self.order):
            if q == 0:
                break
            k = self._find(q, v)
            if k >= 0:
                return int(self.child_next[k])
            q = int(self.bo[q])
        return int(self.uni_next[v])

    def row_gains(self, node, weight):
        """float32 [V]: what the kernel adds to the scores of a row whose (advanced) node is `node`"""
        t = self.tables(weight)
        V = self.vocab_size
        g = np.zeros(V, np.float32)
        mark = np.zeros(V, bool)
        acc, q = np.float32(0.0), int(node)
        for _ in range(self.order):
            if q == 0:
                break
            lo, hi = int(self.child_off[q]), int(self.child_off[q + 1])
            vs = t["child_tok"][lo:hi]
            new = ~mark[vs]
            g[vs[new]] = (acc + t["child_lp"][lo:hi][new]).astype(np.float32)
            mark[vs] = True
            acc = np.float32(acc + t["bow"][q])
            q = int(self.bo[q])
        rest = ~mark
        g[rest] = (acc + t["uni_lp"][rest]).astype(np.float32)
        return g


def write_arpa(path, grams, order, id_to_token, sos_id=1, eos_id=2):
    """grams {token tuple: (log10 p, log10 bow)} as an ARPA file; numbers with repr's digits, so that reading gives the same floats.
    <SOS> / <EOS> are written <s> / </s>; a back-off weight of 0 is left out."""
    name = lambda t: "<s>" if t == sos_id else "</s>" if t == eos_id else id_to_token[t]
    by = [sorted(k for k in grams if len(k) == n) for n in range(1, order + 1)]
    with open(path, "w", encoding="utf-8") as f:
        f.write("\\data\\\n")
        for n, keys in enumerate(by, 1):
            f.write("ngram %d=%d\n" % (n, len(keys)))
        for n, keys in enumerate(by, 1):
            f.write("\n\\%d-grams:\n" % n)
            for k in keys:
                lp, bw = grams[k]
                f.write("%r\t%s" % (float(lp), " ".join(name(t) for t in k)))
                f.write("\t%r\n" % float(bw) if (n < order and float(bw) != 0.0) else "\n")
        f.write("\n\\end\\\n")


def from_args(args, tokenizer=None):
    """the model --ngram_lm / --ngram_weight ask for, or None (no file or weight 0).  A weight > 0 without a file, a negative or
    non-finite weight and a missing file are ValueErrors."""
    path = getattr(args, "ngram_lm", "") or ""
    w = float(getattr(args, "ngram_weight", 0.0) or 0.0)
    if not np.isfinite(w) or w < 0:
        raise ValueError("--ngram_weight must be finite and >= 0 (got %g)" % w)
    if w > 0 and not path:
        raise ValueError("--ngram_weight %g needs a model: --ngram_lm FILE" % w)
    if not path:
        return None
    if not os.path.isfile(path):
        raise ValueError("--ngram_lm: no such file %r" % path)
    if w == 0:
        return None
    if tokenizer is None:
        from utils.tokenizer import CharEncoder, SubwordEncoder
        tokenizer = CharEncoder() if args.unit.lower() == "char" else SubwordEncoder(args.subword_dir)
    return NgramLM.from_arpa(path, tokenizer.token_to_id, args.vocab_size)
