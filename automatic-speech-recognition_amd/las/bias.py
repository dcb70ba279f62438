"""las.bias -- contextual biasing (hotword boosting) of the beam search by shallow fusion: the host side.

A context is a set of phrases, each a non-empty list of token ids (never SOS or PAD), with one per-token weight beta > 0 held as
float32.  ContextGraph compiles them into the flat token trie las_bias_step (csrc/bias.hip, include/las_hip.h K10e) walks; node 0 is
the root.  For a node s: depth(s); base(s) = depth of the deepest phrase-end node on the path root .. s (s included, 0 if none);
pend(s) = fl32(beta) * fl32(depth(s) - base(s)), the bonus paid out for a match that is not complete yet.

Transition on token v from node s:
  1. v is a child of s:                              t = child(s, v),    gain beta
  2. else, s is not the root and v is a root child:  t = child(root, v), gain fl32(beta - pend(s))   (pay back, start anew at v)
  3. else:                                           t = root,           gain -pend(s)               (nothing from the root)
  4. a t that ends a phrase and has no children becomes the root; the bonus is kept.  A phrase end WITH children stays where it is
     (pend = 0), so NEW YORK CITY can still extend NEW YORK.
EOS is an ordinary token.  There are no Aho-Corasick fail links: an occurrence that starts inside a failed partial match, other than
at the failing token, is not seen -- the device tables are one child list per node plus the root's.

Tables (numpy, uploaded once by .to(device)):
  child_off int32 [M + 1]; child_tok int32 [E], ascending inside a node; child_next int32 [E], rule 4 applied;
  gdef float32 [M] = -pend; groot float32 [M] = fl32(beta - pend); beta float32.
Limits, checked here before anything is launched (they are the kernel's): at most MAX_NODES = 2^22 nodes (a node travels through the
search as a float32, exact below 2^24), vocabulary and root fan-out at most MAX_V = MAX_ROOT_FANOUT = 16384 (the kernel's token-class
table in LDS)."""
import numpy as np

MAX_NODES = 1 << 22
MAX_V = 16384
MAX_ROOT_FANOUT = 16384


class ContextGraph(object):
    def __init__(self, phrases, weight, vocab_size=None, sos_id=1, pad_id=0):
        w = float(weight)
        if not np.isfinite(w) or w < 0:
            raise ValueError("ContextGraph: the weight must be finite and >= 0 (got %r)" % (weight,))
        if w > float(np.finfo(np.float32).max):
            raise ValueError("ContextGraph: the weight %r is not finite in float32" % (weight,))
        V = MAX_V if vocab_size is None else int(vocab_size)
        if V < 2 or V > MAX_V:
            raise ValueError("ContextGraph: vocab_size must be in [2, %d] (got %d)" % (MAX_V, V))
        self.vocab_size = V
        self.beta = np.float32(w)
        children = [{}]                     # node -> {token: node}
        depth, is_end = [0], [False]
        self.phrases = []
        seen = set()
        for k, ph in enumerate(phrases):
            name = "phrase %d %r" % (k, list(ph) if not isinstance(ph, str) else ph)
            if isinstance(ph, str):
                raise ValueError("ContextGraph: %s is text; phrases are lists of token ids (ContextGraph.from_file encodes text)" % name)
            ph = list(ph)
            if len(ph) == 0:
                raise ValueError("ContextGraph: %s is empty" % name)
            for t in ph:
                if int(t) != t:
                    raise ValueError("ContextGraph: %s holds %r, not a token id" % (name, t))
                if not 0 <= int(t) < V:
                    raise ValueError("ContextGraph: %s holds token %d outside [0, %d)" % (name, int(t), V))
                if int(t) in (sos_id, pad_id):
                    raise ValueError("ContextGraph: %s holds <SOS> / <PAD> (token %d)" % (name, int(t)))
            ph = tuple(int(t) for t in ph)
            if ph in seen:                  # duplicates collapse
                continue
            seen.add(ph)
            self.phrases.append(list(ph))
            s = 0
            for t in ph:
                nx = children[s].get(t)
                if nx is None:
                    nx = len(children)
                    if nx >= MAX_NODES:
                        raise ValueError("ContextGraph: %s takes the trie past %d nodes" % (name, MAX_NODES))
                    children.append({})
                    depth.append(depth[s] + 1)
                    is_end.append(False)
                    children[s][t] = nx
                s = nx
            is_end[s] = True
            if len(children[0]) > MAX_ROOT_FANOUT:
                raise ValueError("ContextGraph: %s is phrase-initial token number %d; at most %d" % (name, len(children[0]), MAX_ROOT_FANOUT))
        M = len(children)
        base = [0] * M
        off = np.zeros(M + 1, np.int32)
        tok, nxt = [], []
        for s in range(M):                  # (a parent's number is smaller than its children's: base[] is ready when it is read)
            for t in sorted(children[s]):
                c = children[s][t]
                base[c] = depth[c] if is_end[c] else base[s]
                tok.append(t)
                nxt.append(0 if (is_end[c] and not children[c]) else c)          # rule 4
            off[s + 1] = len(tok)
        self.num_nodes = M
        self.child_off = off
        self.child_tok = np.asarray(tok, np.int32).reshape(-1)
        self.child_next = np.asarray(nxt, np.int32).reshape(-1)
        pend = self.beta * (np.asarray(depth, np.float32) - np.asarray(base, np.float32))      # one float32 product per node
        self.gdef = (-pend).astype(np.float32)
        self.groot = (self.beta - pend).astype(np.float32)
        self._dev = {}

    @property
    def active(self):
        """a context that changes a search: positive weight and at least one phrase"""
        return bool(self.beta > 0) and self.num_nodes > 1

    @classmethod
    def from_file(cls, path, tokenizer, weight, vocab_size):
        """one phrase per line; blank lines and lines starting with '#' are skipped; a line is upper-cased like the transcripts and
        encoded with tokenizer.encode(line, with_eos=False)"""
        import os
        if not path or not os.path.isfile(path):
            raise ValueError("hotwords: no such file %r" % (path,))
        phrases = []
        with open(path, encoding="utf-8") as f:
            for ln, line in enumerate(f, 1):
                text = line.strip()
                if not text or text.startswith("#"):
                    continue
                text = " ".join(text.upper().split())
                try:
                    ids = list(tokenizer.encode(text, with_eos=False))
                except KeyError as e:       # the char unit: a character outside its 30 symbols
                    raise ValueError("hotwords %s, line %d: character %s is not in the vocabulary (%r)" % (path, ln, e, text))
                if not ids:
                    raise ValueError("hotwords %s, line %d: %r encodes to no token" % (path, ln, text))
                try:
                    cls([ids], weight, vocab_size)
                except ValueError as e:
                    raise ValueError("hotwords %s, line %d (%r): %s" % (path, ln, text, e))
                phrases.append(ids)
        return cls(phrases, weight, vocab_size)

    def to(self, device):
        """the tables on `device` (uploaded once per device): a dict of tensors"""
        import torch
        key = str(torch.device(device))
        if key not in self._dev:
            up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(device)
            pad = lambda a: a if a.size else np.zeros(1, a.dtype)     # (an empty context: valid addresses nobody reads)
            self._dev[key] = {"child_off": up(self.child_off), "child_tok": up(pad(self.child_tok)), "child_next": up(pad(self.child_next)),
                              "gdef": up(self.gdef), "groot": up(self.groot)}
        return self._dev[key]

    # ---- the tables walked on the host (what the kernel does, for tests and tools)
    def step(self, s, v):
        """-> (next node, gain as float32); a gain of 0 means no add"""
        def find(node):
            lo, hi = int(self.child_off[node]), int(self.child_off[node + 1])
            k = lo + int(np.searchsorted(self.child_tok[lo:hi], v))
            return k if k < hi and self.child_tok[k] == v else -1
        k = find(s)
        if k >= 0:
            return int(self.child_next[k]), self.beta
        if s != 0:
            k = find(0)
            if k >= 0:
                return int(self.child_next[k]), self.groot[s]
            return 0, self.gdef[s]
        return 0, np.float32(0.0)


def from_args(args, tokenizer=None):
    """the context --hotwords / --hotword_weight ask for, or None (no file or weight 0).  A weight > 0 without a file, a negative
    weight and a missing file are ValueErrors."""
    path = getattr(args, "hotwords", "") or ""
    w = float(getattr(args, "hotword_weight", 0.0) or 0.0)
    if not np.isfinite(w) or w < 0:
        raise ValueError("--hotword_weight must be finite and >= 0 (got %g)" % w)
    if w > 0 and not path:
        raise ValueError("--hotword_weight %g needs a phrase list: --hotwords FILE" % w)
    if not path:
        return None
    import os
    if not os.path.isfile(path):
        raise ValueError("--hotwords: no such file %r" % path)
    if w == 0:
        return None
    if tokenizer is None:
        from utils.tokenizer import CharEncoder, SubwordEncoder
        tokenizer = CharEncoder() if args.unit.lower() == "char" else SubwordEncoder(args.subword_dir)
    return ContextGraph.from_file(path, tokenizer, w, args.vocab_size)
