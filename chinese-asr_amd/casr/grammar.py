"""Grammar-constrained decoding: a finite-state grammar whose sentences are the only answers the beam
search may give (include/casr.h casr_grammar_*, casr_beam_grammar).  Grammar holds a deterministic
acceptor over token ids, the object the library builds from it on the host (csrc/grammar_plan.h) and, per
device, its copy there.

The builders compose small non-deterministic automata (phrase chains, concatenation, repetition, union)
and all go through one routine, ``_compile``, which determinises by the subset construction and trims
the states that reach no final state, as casr_grammar_create requires."""
import ctypes
import os

import numpy as np

from . import lib as _lib

EOS = 2  # the recogniser's end-of-sentence id (casr.config.CasrConfig.eos)


class _Nfa:
    """States 0 .. n - 1 with token arcs and epsilon arcs; fragments are (entry, exit) state pairs."""

    def __init__(self):
        self.arcs = []  # per state {token: set(next)}
        self.eps = []   # per state set(next)

    def state(self):
        self.arcs.append({})
        self.eps.append(set())
        return len(self.arcs) - 1

    def arc(self, s, tok, d):
        self.arcs[s].setdefault(tok, set()).add(d)

    def chain(self, ids):
        a = s = self.state()
        for t in ids:
            d = self.state()
            self.arc(s, t, d)
            s = d
        return a, s

    def alt(self, frags):
        a, z = self.state(), self.state()
        for fa, fz in frags:
            self.eps[a].add(fa)
            self.eps[fz].add(z)
        return a, z

    def cat(self, frags):
        a = z = self.state()
        for fa, fz in frags:
            self.eps[z].add(fa)
            z = fz
        return a, z

    def closure(self, states):
        out, todo = set(states), list(states)
        while todo:
            for d in self.eps[todo.pop()]:
                if d not in out:
                    out.add(d)
                    todo.append(d)
        return frozenset(out)


def _compile(nfa, starts, finals):
    """Determinise (subset construction from every start set, sharing states) and trim.  Returns (arcs,
    finals, start ids): arcs a list per state of (token, next) pairs ascending in token.  The first start
    becomes state 0.  A start whose language is empty raises ValueError."""
    index, subsets, arcs = {}, [], []

    def state_of(sub):
        if sub not in index:
            index[sub] = len(subsets)
            subsets.append(sub)
            arcs.append(None)
        return index[sub]

    start_ids = [state_of(nfa.closure(s)) for s in starts]
    done = 0
    while done < len(subsets):
        move = {}
        for q in subsets[done]:
            for t, ds in nfa.arcs[q].items():
                move.setdefault(t, set()).update(ds)
        arcs[done] = [(t, state_of(nfa.closure(ds))) for t, ds in sorted(move.items())]
        done += 1
    fin = [bool(sub & finals) for sub in subsets]
    # trim: keep the states that reach a final state
    back = [[] for _ in subsets]
    for s, row in enumerate(arcs):
        for _, d in row:
            back[d].append(s)
    keep, todo = set(), [s for s, f in enumerate(fin) if f]
    keep.update(todo)
    while todo:
        for s in back[todo.pop()]:
            if s not in keep:
                keep.add(s)
                todo.append(s)
    for i, s in enumerate(start_ids):
        if s not in keep:
            raise ValueError(f"Grammar: the language of start {i} is empty")
    order = sorted(keep, key=lambda s: (s != start_ids[0], s))  # the first start is state 0
    new = {s: i for i, s in enumerate(order)}
    out = [[(t, new[d]) for t, d in arcs[s] if d in keep] for s in order]
    return out, [i for i, s in enumerate(order) if fin[s]], [new[s] for s in start_ids]


def _ids(phrase, word2int, vocab, eos):
    ids = []
    for w in phrase:
        t = int(w) if isinstance(w, (int, np.integer)) else (word2int or {}).get(w, -1)
        if not 0 <= t < vocab or t == eos:
            raise ValueError(f"Grammar: {w!r} of phrase {phrase!r} is not in the vocabulary")
        ids.append(t)
    return ids


def read_phrases(path):
    """A text file with one phrase per line; empty lines and lines starting with # are skipped."""
    with open(path, encoding="utf-8") as f:
        lines = [ln.strip() for ln in f]
    return [ln for ln in lines if ln and not ln.startswith("#")]


class Grammar:
    """Grammar(arcs, finals, vocab, eos=2): ``arcs`` one list per state of (token, next state) pairs,
    ``finals`` the final states.  Sentences start in state 0.  The arcs of a state must have distinct tokens
    in [0, vocab) other than ``eos``, and every state must reach a final one (the builders below see to
    both); the library refuses anything else (casr.lib.CasrError naming the state or arc)."""

    def __init__(self, arcs, finals, vocab, eos=EOS):
        self.vocab, self.eos = int(vocab), int(eos)
        self.arcs = [sorted((int(t), int(d)) for t, d in row) for row in arcs]
        self.finals = sorted(set(int(s) for s in finals))
        self.n_states = len(self.arcs)
        self._lib = _lib.load()
        self._host = None
        self._device = {}  # (library, device index) -> casr_grammar*
        self._host = self._create(self._lib, -1)
        n = ctypes.c_int32()
        a = ctypes.c_int64()
        self.dist = np.zeros(self.n_states, np.int32)
        _lib.check(self._lib.casr_grammar_info(self._host, ctypes.byref(n), ctypes.byref(a), _p(self.dist)),
                   lib=self._lib)
        self.n_arcs = int(a.value)
        self.mask_words = int(self._lib.casr_grammar_mask_words(self.vocab))

    # ------------------------------------------------------------------ builders
    @classmethod
    def _from_nfa(cls, nfa, frag, vocab, eos):
        arcs, finals, _ = _compile(nfa, [[frag[0]]], {frag[1]})
        return cls(arcs, finals, vocab, eos)

    @classmethod
    def from_phrases(cls, phrases, word2int, vocab, eos=EOS):
        """Exactly one of the phrases (strings, one token per character, or lists of ids or words)."""
        nfa = _Nfa()
        frag = nfa.alt([nfa.chain(_ids(p, word2int, vocab, eos)) for p in phrases])
        return cls._from_nfa(nfa, frag, vocab, eos)

    @classmethod
    def from_file(cls, path, word2int, vocab, eos=EOS):
        """from_phrases of read_phrases' file format: one phrase per line."""
        return cls.from_phrases(read_phrases(path), word2int, vocab, eos)

    @classmethod
    def sequence(cls, slots, word2int, vocab, eos=EOS, optional=()):
        """One phrase of every slot in order; a slot is a list of alternative phrases.  The slots whose
        index is in ``optional``, and those that list an empty phrase, may be skipped."""
        nfa = _Nfa()
        frags = []
        for i, slot in enumerate(slots):
            alts = [nfa.chain(_ids(p, word2int, vocab, eos)) for p in slot]
            if i in optional:
                alts.append(nfa.chain([]))
            frags.append(nfa.alt(alts))
        return cls._from_nfa(nfa, nfa.cat(frags), vocab, eos)

    @classmethod
    def repeat(cls, phrases, lo, hi, word2int, vocab, eos=EOS):
        """Between ``lo`` and ``hi`` phrases of the list in a row, e.g. 3 to 11 digits."""
        if not 0 <= lo <= hi:
            raise ValueError(f"Grammar.repeat: need 0 <= lo <= hi, got {lo}, {hi}")
        nfa = _Nfa()
        ids = [_ids(p, word2int, vocab, eos) for p in phrases]
        frags = []
        for n in range(hi):
            alts = [nfa.chain(p) for p in ids]
            frags.append(nfa.alt(alts))
        a, z = nfa.cat(frags)
        # leaving after n >= lo copies: from the entry of copy n + 1 (or the end) straight to the exit
        entries = [f[0] for f in frags] + [z]
        for n in range(lo, hi):
            nfa.eps[entries[n]].add(z)
        return cls._from_nfa(nfa, (a, z), vocab, eos)

    @classmethod
    def union(cls, grammars):
        """One grammar holding every member's states, and one start state per member: the object for
        per-utterance grammars (``start`` of Engine.beam_grammar).  Sentences walked from state 0 are the
        first member's.  Returns (grammar, starts)."""
        grammars = list(grammars)
        if not grammars:
            raise ValueError("Grammar.union: no grammars")
        vocab, eos = grammars[0].vocab, grammars[0].eos
        nfa, starts, finals = _Nfa(), [], set()
        for g in grammars:
            if (g.vocab, g.eos) != (vocab, eos):
                raise ValueError("Grammar.union: the members' vocab and eos differ")
            base = len(nfa.arcs)
            for _ in range(g.n_states):
                nfa.state()
            for s, row in enumerate(g.arcs):
                for t, d in row:
                    nfa.arc(base + s, t, base + d)
            starts.append([base])
            finals.update(base + s for s in g.finals)
        arcs, fin, start_ids = _compile(nfa, starts, finals)
        return cls(arcs, fin, vocab, eos), start_ids

    @classmethod
    def universal(cls, vocab, eos=EOS):
        """Every sentence over the vocabulary: the grammar that constrains nothing."""
        return cls([[(v, 0) for v in range(vocab) if v != eos]], [0], vocab, eos)

    # ------------------------------------------------------------------ the library objects
    def _create(self, lib, device):
        off = np.zeros(self.n_states + 1, np.int64)
        off[1:] = np.cumsum([len(r) for r in self.arcs])
        tok = np.array([t for r in self.arcs for t, _ in r], np.int32)
        nxt = np.array([d for r in self.arcs for _, d in r], np.int32)
        fin = np.zeros(max(self.n_states, 1), np.uint8)
        if any(not 0 <= s < self.n_states for s in self.finals):
            raise ValueError(f"Grammar: a final state outside [0, {self.n_states})")
        fin[np.array(self.finals, np.intp)] = 1
        out = ctypes.c_void_p()
        # (empty arrays still pass a pointer: NULL is the library's refusal)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        rc = lib.casr_grammar_create(int(device), self.vocab, self.eos, self.n_states, vp(off), vp(tok), vp(nxt),
                                     vp(fin), ctypes.byref(out))
        _lib.check(rc, lib=lib)
        return out

    def close(self):
        if getattr(self, "_host", None):
            self._lib.casr_grammar_destroy(self._host)
            self._host = None
        for (lib, _), p in list(getattr(self, "_device", {}).items()):
            lib.casr_grammar_destroy(p)
        self._device = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def on(self, engine):
        """The device object for an Engine's device (uploaded once per device and library)."""
        key = (engine.lib, engine.device.index)
        if key not in self._device:
            self._device[key] = self._create(engine.lib, engine.device.index)
        return self._device[key]

    # ------------------------------------------------------------------ host queries
    def walk(self, tokens, lens):
        """(consumed, state, accepted) [n] of the rows tokens [n, L] with lens [n], on the host
        (casr_grammar_accept_host)."""
        tokens = np.ascontiguousarray(tokens, np.int32)
        lens = np.ascontiguousarray(lens, np.int32)
        if tokens.ndim != 2 or lens.shape != (tokens.shape[0],):
            raise ValueError("walk: tokens must be [n, L] and lens [n]")
        n, L = tokens.shape
        consumed, state, ok = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint8)
        rc = self._lib.casr_grammar_accept_host(self._host, _p(tokens), _p(lens), n, L, _p(consumed), _p(state),
                                                _p(ok))
        _lib.check(rc, lib=self._lib)
        return consumed, state, ok

    def accepts(self, sentence, word2int=None):
        """Is one sentence (a string, or a list of ids or words) in the language?  A character outside
        the vocabulary is in no sentence."""
        ids = [int(w) if isinstance(w, (int, np.integer)) else (word2int or {}).get(w, -1) for w in sentence]
        tok = np.array([ids + [0]], np.int32)
        return bool(self.walk(tok, [len(ids)])[2][0])

    def rows(self, state, budget):
        """mask uint32 [n, mask_words] of states [n] under budgets [n] on the host
        (casr_grammar_rows_host): bit v of a row says whether token v is a candidate."""
        state = np.ascontiguousarray(state, np.int32).reshape(-1)
        budget = np.ascontiguousarray(np.broadcast_to(np.asarray(budget, np.int32), state.shape))
        mask = np.zeros((state.size, self.mask_words), np.uint32)
        rc = self._lib.casr_grammar_rows_host(self._host, _p(state), _p(budget), state.size, _p(mask))
        _lib.check(rc, lib=self._lib)
        return mask

    @staticmethod
    def coerce(grammar, word2int, vocab, eos=EOS):
        """None, a Grammar, a file name or a list of phrases -> None or a Grammar."""
        if grammar is None or isinstance(grammar, Grammar):
            return grammar
        if isinstance(grammar, (str, os.PathLike)):
            return Grammar.from_file(grammar, word2int, vocab, eos)
        return Grammar.from_phrases(grammar, word2int, vocab, eos)


def mask_bits(mask, vocab):
    """bool [n, vocab] of mask rows uint32 [n, mask_words]."""
    mask = np.ascontiguousarray(mask, np.uint32)
    bits = np.unpackbits(mask.view(np.uint8), axis=1, bitorder="little")
    return bits[:, :vocab].astype(bool)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None
