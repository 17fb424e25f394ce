"""A back-off n-gram language model over a recogniser's class ids, compiled into the flat automaton that pero_ctc_beam_lm walks
(include/pero_hip.h).  Host side only: numpy in f64, the tables in f32 / int32.  (The reference has no language
model: an extension, like the recogniser itself.)"""
import math
import os

import numpy as np

BOS, EOS = -1, -2   # the tokens <s> and </s> inside n-gram tuples; class ids are >= 0
MAX_ORDER = 16      # PERO_CTC_LM_MAX_ORDER: the back-off steps of one look-up the kernel follows
_LN10 = math.log(10.0)


def _f32(v):
    return float(np.float32(v))


class NGramLM:
    """The automaton.  States 0 .. M-1, state 0 = the empty context, `start` = the state of the context <s> (0 for a model without <s>).
    Per state: backoff_state (int32, -1 for state 0), backoff_weight (f32, natural log), final (f32, ln p(</s> | state) with the back-off
    resolved; zeros for a model without </s>).  Arcs in CSR form: arc_begin (M + 1), arc_label (ascending inside a state), arc_logp (f32, ln),
    arc_next (the state of the longest suffix of context + label that is a state).  The blank is no symbol; a class without an arc in state 0
    is forbidden to the decoder.

        lookup(s, c): acc = 0; while c is no arc of s: acc += backoff_weight[s], s = backoff_state[s]; lm = acc + arc_logp, next = arc_next

    in f32, in this order (`lookup`), which is what the kernel computes; `score` is the same walk in f64 over the f32 tables.

    `fit` estimates the model with ABSOLUTE DISCOUNTING AND BACK-OFF: unigrams add-one over the C - 1 labels and, with eos, </s>:
    p(w) = (c(w) + 1) / (n + V); above that, for a context h that was seen c(h.) times in front of N(h) different symbols,
    p(w | h) = (c(hw) - D) / c(h.) for a seen hw and p(w | h) = bow(h) p(w | h') otherwise, h' = h without its first token,
    bow(h) = D N(h) / c(h.) / (1 - sum of p(w | h') over the seen w), so that every context's distribution sums to 1.  (A context seen in front
    of every symbol has no unseen one to back off to: its discounted mass is spread over the symbols in proportion to p(w | h').)  Lines
    start in the context <s> (orders >= 2); every value is rounded to f32 once, before anything is derived from it.

    contexts (optional, needed by to_arpa): per state the tuple of tokens it stands for (class ids, BOS)."""

    def __init__(self, num_classes, blank, order, start, backoff_state, backoff_weight, final, arc_begin, arc_label, arc_logp, arc_next,
                 contexts=None):
        self.num_classes, self.blank, self.order, self.start = int(num_classes), int(blank), int(order), int(start)
        self.backoff_state = np.ascontiguousarray(backoff_state, dtype=np.int32)
        self.backoff_weight = np.ascontiguousarray(backoff_weight, dtype=np.float32)
        self.final = np.ascontiguousarray(final, dtype=np.float32)
        self.arc_begin = np.ascontiguousarray(arc_begin, dtype=np.int32)
        self.arc_label = np.ascontiguousarray(arc_label, dtype=np.int32)
        self.arc_logp = np.ascontiguousarray(arc_logp, dtype=np.float32)
        self.arc_next = np.ascontiguousarray(arc_next, dtype=np.int32)
        self.contexts = None if contexts is None else [tuple(c) for c in contexts]
        self._device = {}
        self._validate()

    # ------------------------------------------------------------------------------------------ what the kernel relies on
    def _validate(self):
        C, M, A = self.num_classes, self.backoff_state.size, self.arc_label.size
        if C < 2 or not 0 <= self.blank < C:
            raise ValueError(f"NGramLM: blank {self.blank} outside [0, {C}) or fewer than 2 classes")
        if not 1 <= self.order <= MAX_ORDER:
            raise ValueError(f"NGramLM: order {self.order} outside [1, {MAX_ORDER}]")
        if M < 1 or self.backoff_weight.size != M or self.final.size != M or self.arc_begin.size != M + 1:
            raise ValueError("NGramLM: the per-state arrays must hold M entries and arc_begin M + 1")
        if self.arc_logp.size != A or self.arc_next.size != A:
            raise ValueError("NGramLM: the per-arc arrays differ in length")
        if not 0 <= self.start < M:
            raise ValueError(f"NGramLM: start {self.start} outside [0, {M})")
        begin = self.arc_begin.astype(np.int64)
        if begin[0] != 0 or begin[-1] != A or bool((np.diff(begin) < 0).any()):
            raise ValueError("NGramLM: arc_begin must rise from 0 to the number of arcs")
        for what, v in (("backoff_weight", self.backoff_weight), ("final", self.final), ("arc_logp", self.arc_logp)):
            if not bool(np.isfinite(v).all()):
                raise ValueError(f"NGramLM: {what} holds a value that is not finite")
        if A and (int(self.arc_label.min()) < 0 or int(self.arc_label.max()) >= C):
            raise ValueError(f"NGramLM: an arc label outside [0, {C})")
        if bool((self.arc_label == self.blank).any()):
            raise ValueError("NGramLM: an arc is labelled with the blank")
        if A and (int(self.arc_next.min()) < 0 or int(self.arc_next.max()) >= M):
            raise ValueError(f"NGramLM: arc_next outside [0, {M})")
        inside = np.ones(A, dtype=bool)
        inside[begin[:-1][begin[:-1] < A]] = False   # the first arc of a state has no neighbour in front
        if A > 1 and bool(((np.diff(self.arc_label.astype(np.int64)) <= 0) & inside[1:]).any()):
            raise ValueError("NGramLM: the labels of a state's arcs must ascend strictly")
        if self.backoff_state[0] != -1:
            raise ValueError("NGramLM: backoff_state[0] must be -1")
        for s in range(1, M):   # every chain ends in state 0 within MAX_ORDER steps
            k, hops = s, 0
            while k != 0:
                k = int(self.backoff_state[k])
                hops += 1
                if not 0 <= k < M or hops > MAX_ORDER:
                    raise ValueError(f"NGramLM: the back-off chain of state {s} does not end in state 0 within {MAX_ORDER} steps")
        if self.contexts is not None and len(self.contexts) != M:
            raise ValueError("NGramLM: contexts must name every state")

    @property
    def num_states(self):
        return int(self.backoff_state.size)

    @property
    def num_arcs(self):
        return int(self.arc_label.size)

    def arrays(self):
        return {k: getattr(self, k) for k in ("backoff_state", "backoff_weight", "final", "arc_begin", "arc_label", "arc_logp", "arc_next")}

    def to(self, device):
        """The arrays as device tensors (cached per device)."""
        import torch
        device = torch.device(device)
        if device not in self._device:
            self._device[device] = {k: torch.from_numpy(v).to(device) for k, v in self.arrays().items()}
        return self._device[device]

    # ------------------------------------------------------------------------------------------ the walk
    def _arc(self, s, c):
        lo, hi = int(self.arc_begin[s]), int(self.arc_begin[s + 1])
        k = lo + int(np.searchsorted(self.arc_label[lo:hi], c))
        return k if k < hi and self.arc_label[k] == c else -1

    def lookup(self, state, label):
        """(lm as numpy f32, next state) by the f32 walk of the class docstring; None for a label without an arc in state 0."""
        acc, s = np.float32(0), int(state)
        while True:
            k = self._arc(s, label)
            if k >= 0:
                return np.float32(acc + self.arc_logp[k]), int(self.arc_next[k])
            if s == 0:
                return None
            acc = np.float32(acc + self.backoff_weight[s])
            s = int(self.backoff_state[s])

    def score(self, labels, eos=True):
        """ln p(labels) (with eos: and of the end symbol behind them) from `start`: the same walk, the f32 tables added in f64.  -inf for a
        string with a forbidden label."""
        total, s = 0.0, self.start
        for c in labels:
            while True:
                k = self._arc(s, int(c))
                if k >= 0:
                    break
                if s == 0:
                    return -math.inf
                total += float(self.backoff_weight[s])
                s = int(self.backoff_state[s])
            total += float(self.arc_logp[k])
            s = int(self.arc_next[k])
        return total + (float(self.final[s]) if eos else 0.0)

    # ------------------------------------------------------------------------------------------ compilation from n-gram tables
    @classmethod
    def _compile(cls, probs, bows, order, num_classes, blank):
        """probs {n-gram tuple: ln p of its last token given the others}, bows {n-gram tuple: ln back-off weight}; tokens are class ids, BOS (first
        place only) and EOS (last place only)."""
        probs = {g: _f32(v) for g, v in probs.items()}
        bows = {g: _f32(v) for g, v in bows.items()}
        for g in list(probs) + list(bows):
            if not 1 <= len(g) <= order or BOS in g[1:] or EOS in g[:-1]:
                raise ValueError(f"NGramLM: {g} is no n-gram of a model of order {order}")
        states = {()}   # the context of every n-gram, every n-gram that can be a context of the next order, and all their suffixes
        for g in list(probs) + list(bows):
            for h in (g[:-1], g):
                if len(h) < order and EOS not in h:
                    states.update(h[k:] for k in range(len(h) + 1))
        contexts = sorted(states, key=lambda h: (len(h), h))
        index = {h: k for k, h in enumerate(contexts)}
        has_eos = any(g[-1] == EOS for g in probs)

        def suffix_state(g):
            g = g[-(order - 1):] if order > 1 else ()
            while g not in index:
                g = g[1:]
            return index[g]

        def final_of(h):
            acc = 0.0
            while True:
                if h + (EOS,) in probs:
                    return acc + probs[h + (EOS,)]
                if not h:
                    raise ValueError("NGramLM: n-grams end in </s> but </s> has no unigram")
                acc += bows.get(h, 0.0)
                h = h[1:]

        arcs = {h: [] for h in contexts}
        for g, v in probs.items():
            if g[-1] not in (EOS, BOS) and g[:-1] in arcs:
                arcs[g[:-1]].append((g[-1], v, suffix_state(g)))
        begin, label, logp, nxt = [0], [], [], []
        for h in contexts:
            for c, v, k in sorted(arcs[h]):
                label.append(c)
                logp.append(v)
                nxt.append(k)
            begin.append(len(label))
        return cls(num_classes, blank, order, index.get((BOS,), 0), [index[h[1:]] if h else -1 for h in contexts],
                   [bows.get(h, 0.0) if h else 0.0 for h in contexts], [final_of(h) if has_eos else 0.0 for h in contexts], begin, label, logp, nxt,
                   contexts=contexts)

    @classmethod
    def fit(cls, sequences, num_classes, blank, order=3, discount=0.75, eos=True):
        """Estimate the model of the class docstring from lists of label ids, in f64."""
        if not 1 <= order <= MAX_ORDER or not 0.0 < discount < 1.0:
            raise ValueError(f"NGramLM.fit: order in [1, {MAX_ORDER}] and discount in (0, 1)")
        symbols = [c for c in range(num_classes) if c != blank] + ([EOS] if eos else [])
        counts = [dict() for _ in range(order + 1)]   # counts[n][n-gram]
        for seq in sequences:
            seq = [int(c) for c in seq]
            if any(not 0 <= c < num_classes or c == blank for c in seq):
                raise ValueError("NGramLM.fit: a label outside the classes, or the blank")
            toks = ([BOS] if order > 1 else []) + seq + ([EOS] if eos else [])
            for i, w in enumerate(toks):
                if w == BOS:
                    continue
                for n in range(1, order + 1):
                    if i - n + 1 < 0:
                        break
                    g = tuple(toks[i - n + 1:i + 1])
                    counts[n][g] = counts[n].get(g, 0) + 1
        total = sum(counts[1].values())
        probs = {(w,): math.log((counts[1].get((w,), 0) + 1) / (total + len(symbols))) for w in symbols}
        bows = {}

        def p_full(h, w):   # the model so far: p(w | h) through the back-off chain
            acc = 0.0
            while h + (w,) not in probs:
                acc += bows.get(h, 0.0)
                h = h[1:]
            return acc + probs[h + (w,)]

        for n in range(2, order + 1):
            by_context = {}
            for g, c in counts[n].items():
                by_context.setdefault(g[:-1], {})[g[-1]] = c
            for h in sorted(by_context):
                seen = by_context[h]
                ch = sum(seen.values())
                lower = {w: math.exp(p_full(h[1:], w)) for w in seen}
                left, free = discount * len(seen) / ch, 1.0 - sum(lower.values())
                if len(seen) == len(symbols) or free < 1e-9:
                    for w, c in seen.items():
                        probs[h + (w,)] = math.log((c - discount) / ch + left * lower[w] / sum(lower.values()))
                    bows[h] = 0.0
                else:
                    for w, c in seen.items():
                        probs[h + (w,)] = math.log((c - discount) / ch)
                    bows[h] = math.log(left / free)
        return cls._compile(probs, bows, order, num_classes, blank)

    # ------------------------------------------------------------------------------------------ ARPA
    @classmethod
    def from_arpa(cls, path_or_text, symbols, num_classes=None, blank=0):
        """Read the ARPA text format (a path, or the text itself).  symbols {token: class id}; log10 values become natural logs; <s> and </s>
        are the start context and the end symbol; <unk> and n-grams with a token that symbols does not hold are dropped; a missing back-off
        weight is 0.  num_classes defaults to the largest id in symbols (and the blank) + 1."""
        if isinstance(path_or_text, str) and "\\data\\" in path_or_text:
            text = path_or_text
        else:
            with open(os.fspath(path_or_text)) as f:
                text = f.read()
        if num_classes is None:
            num_classes = max(list(symbols.values()) + [blank]) + 1
        probs, bows, order, n = {}, {}, 0, 0
        for line in text.splitlines():
            line = line.strip()
            if not line or line == "\\data\\":
                continue
            if line == "\\end\\":
                break
            if line.startswith("ngram "):
                order = max(order, int(line[len("ngram "):].split("=")[0]))
                continue
            if line.startswith("\\") and line.endswith("-grams:"):
                n = int(line[1:-len("-grams:")])
                continue
            if n == 0:
                continue
            parts = line.split()
            if len(parts) not in (n + 1, n + 2):
                raise ValueError(f"NGramLM.from_arpa: not a {n}-gram line: {line!r}")
            toks = []
            for tok in parts[1:n + 1]:
                toks.append(BOS if tok == "<s>" else EOS if tok == "</s>" else symbols.get(tok) if tok != "<unk>" else None)
            if any(t is None for t in toks) or BOS in toks[1:] or EOS in toks[:-1]:
                continue
            g = tuple(int(t) for t in toks)
            if g[-1] != BOS:
                probs[g] = float(parts[0]) * _LN10
            if len(parts) == n + 2 and g[-1] != EOS:
                bows[g] = float(parts[n + 1]) * _LN10
            elif g == (BOS,):
                bows.setdefault(g, 0.0)
        if order < 1:
            raise ValueError("NGramLM.from_arpa: no \\data\\ section with n-gram counts")
        return cls._compile(probs, bows, order, num_classes, blank)

    def to_arpa(self, symbols=None):
        """The model as ARPA text (log10, 17 significant digits: reading it back gives the same f32 tables).  symbols {token: class id} names the
        classes (default: the id as a decimal number).  Every state's end probability is written as an explicit n-gram."""
        if self.contexts is None:
            raise ValueError("NGramLM.to_arpa: built from bare arrays without contexts")
        names = {c: str(c) for c in range(self.num_classes)} if symbols is None else {c: tok for tok, c in symbols.items()}
        names.update({BOS: "<s>", EOS: "</s>"})
        index = {h: k for k, h in enumerate(self.contexts)}
        has_eos = bool(self.final.any())
        grams = [[] for _ in range(self.order + 1)]
        if (BOS,) in index:
            grams[1].append(((BOS,), -99.0, float(self.backoff_weight[index[(BOS,)]]) / _LN10))
        for s, h in enumerate(self.contexts):
            for k in range(int(self.arc_begin[s]), int(self.arc_begin[s + 1])):
                g = h + (int(self.arc_label[k]),)
                grams[len(g)].append((g, float(self.arc_logp[k]) / _LN10, float(self.backoff_weight[index[g]]) / _LN10 if g in index else None))
            if has_eos:
                grams[len(h) + 1].append((h + (EOS,), float(self.final[s]) / _LN10, None))
        lines = ["\\data\\"] + [f"ngram {n}={len(grams[n])}" for n in range(1, self.order + 1)] + [""]
        for n in range(1, self.order + 1):
            lines.append(f"\\{n}-grams:")
            for g, v, bow in sorted(grams[n], key=lambda e: e[0]):
                lines.append("\t".join([f"{v:.17g}", " ".join(names[t] for t in g)] + ([] if bow is None else [f"{bow:.17g}"])))
            lines.append("")
        return "\n".join(lines + ["\\end\\", ""])
