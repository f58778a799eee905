"""Hotword (contextual) biasing: a list of phrases the beam search should favour while it searches
(include/casr.h casr_bias_*, casr_beam_bias).  PhraseBias holds the phrase automaton the library builds
(csrc/bias_plan.h) on the host and, per device, its copy there."""
import ctypes
import os

import numpy as np

from . import lib as _lib

UNIT = 256        # a boost is an integer count of 1/256 nat per token
MAX_BOOST = 4096  # 16 nats per token
MAX_LEN = _lib.BIAS_MAX_LEN


def read_hotwords(path):
    """A text file with one phrase per line and an optional boost in nats per token after it, separated
    by whitespace; empty lines and lines starting with # are skipped.  Returns (phrases, boosts) with
    None where a line gives no boost."""
    phrases, boosts = [], []
    with open(path, encoding="utf-8") as f:
        for line in f:
            parts = line.split()
            if not parts or parts[0].startswith("#"):
                continue
            if len(parts) > 2:
                raise ValueError(f"{path}: expected 'phrase [boost]', got {line.strip()!r}")
            phrases.append(parts[0])
            boosts.append(float(parts[1]) if len(parts) == 2 else None)
    return phrases, boosts


class PhraseBias:
    """PhraseBias(phrases, word2int, vocab, boost=1.0): ``phrases`` strings (one token per character, as
    the recogniser's vocabulary is) or lists of token ids or words; ``word2int`` the ASR vocabulary
    (word -> id in [0, vocab)); ``boost`` one value for all or one per phrase, in nats per token, each
    quantised to 1/256 (at least 1/256, at most 16).  A phrase with a character outside the vocabulary
    raises ValueError naming it: such a phrase could never match.  Every occurrence of every phrase
    counts, so listing both a phrase and a longer one that contains it boosts the longer one by both."""

    def __init__(self, phrases, word2int, vocab, boost=1.0):
        self.vocab = V = int(vocab)
        phrases = list(phrases)
        boosts = [boost] * len(phrases) if np.isscalar(boost) else list(boost)
        if len(boosts) != len(phrases):
            raise ValueError(f"PhraseBias: {len(phrases)} phrases but {len(boosts)} boosts")
        self.phrases, self.boost_q = [], []
        for ph, bo in zip(phrases, boosts):
            ids = []
            for w in ph:
                t = int(w) if isinstance(w, (int, np.integer)) else word2int.get(w, -1)
                if not 0 <= t < V:
                    raise ValueError(f"PhraseBias: {w!r} of phrase {ph!r} is not in the vocabulary")
                ids.append(t)
            if not 1 <= len(ids) <= MAX_LEN:
                raise ValueError(f"PhraseBias: phrase {ph!r} has {len(ids)} tokens, not 1..{MAX_LEN}")
            q = int(round(float(bo) * UNIT))
            if not 1 <= q <= MAX_BOOST:
                raise ValueError(f"PhraseBias: boost {bo!r} of phrase {ph!r} is outside [1/256, 16] nats per token")
            self.phrases.append(ids)
            self.boost_q.append(q)
        self._lib = _lib.load()
        self._host = self._create(self._lib, -1)
        self._device = {}  # (library, device index) -> casr_bias*

    @classmethod
    def from_file(cls, path, word2int, vocab, boost=1.0):
        """From read_hotwords' file format; ``boost`` serves the lines that give none."""
        phrases, boosts = read_hotwords(path)
        return cls(phrases, word2int, vocab, [boost if b is None else b for b in boosts])

    @classmethod
    def coerce(cls, hotwords, word2int, vocab, boost=1.0):
        """None, a PhraseBias, a file name or a list of phrases -> None or a PhraseBias."""
        if hotwords is None or isinstance(hotwords, cls):
            return hotwords
        if isinstance(hotwords, (str, os.PathLike)):
            return cls.from_file(hotwords, word2int, vocab, boost)
        return cls(hotwords, word2int, vocab, boost)

    def _create(self, lib, device):
        toks = np.array([t for p in self.phrases for t in p], np.int32)
        lens = np.array([len(p) for p in self.phrases], np.int32)
        boost = np.array(self.boost_q, np.int32)
        out = ctypes.c_void_p()
        rc = lib.casr_bias_create(int(device), self.vocab, len(self.phrases), _p(toks), _p(lens), _p(boost),
                                  ctypes.byref(out))
        _lib.check(rc, lib=lib)
        return out

    def close(self):
        if getattr(self, "_host", None):
            self._lib.casr_bias_destroy(self._host)
            self._host = None
        for (lib, _), p in list(getattr(self, "_device", {}).items()):
            lib.casr_bias_destroy(p)
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

    # ------------------------------------------------------------------ host scoring
    def score_ids(self, tokens, lens):
        """(full, tail, state) int32 [n] of the rows tokens [n, L] with lens [n], on the host
        (casr_bias_score_host); bias_open = (full + tail) / 256, bias_closed = full / 256."""
        tokens = np.ascontiguousarray(tokens, np.int32)
        lens = np.ascontiguousarray(lens, np.int32)
        if tokens.ndim != 2 or lens.shape != (tokens.shape[0],):
            raise ValueError("score_ids: tokens must be [n, L] and lens [n]")
        n, L = tokens.shape
        full, tail, state = (np.zeros(n, np.int32) for _ in range(3))
        rc = self._lib.casr_bias_score_host(self._host, _p(tokens), _p(lens), n, L, _p(full), _p(tail), _p(state))
        _lib.check(rc, lib=self._lib)
        return full, tail, state

    def rows(self, state, next=False):
        """gain int32 [n, V] of automaton states [n] on the host (casr_bias_rows_host), and with ``next``
        the successor states [n, V]."""
        state = np.ascontiguousarray(state, np.int32).reshape(-1)
        gain = np.zeros((state.size, self.vocab), np.int32)
        nx = np.zeros((state.size, self.vocab), np.int32) if next else None
        rc = self._lib.casr_bias_rows_host(self._host, _p(state), state.size, _p(gain), _p(nx))
        _lib.check(rc, lib=self._lib)
        return (gain, nx) if next else gain


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None
