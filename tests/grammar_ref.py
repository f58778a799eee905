"""Yardstick of grammar-constrained decoding (include/casr.h casr_grammar_*, casr_beam_grammar): a numpy
restatement from the definition.  It shares no code with the product and keeps no automaton of the
product's kind: a language is an enumerated set of sentences (SetLanguage) or a rule stated directly
(LoopLanguage), and an acceptor given as arcs is walked as a set of (state, token, next) triples with its
distances found by relaxation, not by a breadth-first search.

The constrained beam is fusion_ref.fused_beam's form on the oracle's decoder_step:

    am  = (x_v / T - lse_r) + a_r          lse over the whole row
    lm  = l == 0 ? term : g_r + term       (with an LM)
    val = (am + lm_weight lm) + len_l      (without an LM: am + len_l)

Candidates of row r with tokens y_r at step l, L = max_len: v != eos where some sentence of the language
of at most L - 1 tokens starts with y_r . v (this is the horizon rule: the state after y_r . v has a final
state within L - 2 - l tokens exactly when such a sentence exists), and eos where y_r is a sentence.  Dead
rows offer nothing.  The top 2k of the candidates (ties to the lower flat index); records are the eos
candidates among the first k ranks; active rows the non-eos candidates in rank order, at most k; the
other slots are dead.  An utterance is finished for the early stop when rank 0 is eos or its list is empty.
The best is the first maximum of the combined score over the records, or over the live rows of the last
step without one; without either the answer is empty.

With-LM comparisons: the gaps of the with-LM variants are asserted where they hold
(tests/test_grammar_host.py WIDTHS_LM); where one falls below 1e-2 the width is left to the invariants of
tests/test_gpu_grammar.py, as tests/bias_ref.py does for its k = 4."""
import functools

import numpy as np

import fusion_ref as FR
import ngram_ref as R
from golden_util import fbank_for
from oracle import casr_oracle as O

F = np.float32


# ---------------------------------------------------------------------------- languages
class SetLanguage:
    """A finite language given as its sentences (token tuples)."""

    def __init__(self, sentences):
        self.sentences = set(tuple(int(t) for t in s) for s in sentences)
        self.short = {}  # prefix -> the length of the shortest sentence it starts
        for s in self.sentences:
            for n in range(len(s) + 1):
                self.short[s[:n]] = min(self.short.get(s[:n], len(s)), len(s))

    def member(self, y):
        return tuple(y) in self.sentences

    def extends(self, y, v, longest):
        """Does some sentence of at most ``longest`` tokens start with y . v?"""
        return self.short.get(tuple(y) + (v,), longest + 1) <= longest

    def tokens_after(self, y):
        n = len(y)
        return sorted({s[n] for s in self.sentences if len(s) > n and s[:n] == tuple(y)})


class LoopLanguage:
    """Every sequence over ``tokens``, the empty one included (a digit loop)."""

    def __init__(self, tokens):
        self.tokens = sorted(int(t) for t in tokens)

    def member(self, y):
        return all(t in self.tokens for t in y)

    def extends(self, y, v, longest):
        return self.member(y) and v in self.tokens and len(y) + 1 <= longest

    def tokens_after(self, y):
        return self.tokens if self.member(y) else []


# ---------------------------------------------------------------------------- acceptors as triples
class TripleAcceptor:
    """An acceptor as a plain set of (state, token, next) triples and a set of final states, simulated as
    a non-deterministic automaton would be (a set of current states)."""

    def __init__(self, triples, finals, n_states):
        self.triples, self.finals, self.S = set(triples), set(finals), n_states

    def walk(self, y, V):
        """(consumed, states after them)"""
        cur = {0}
        for j, t in enumerate(y):
            nxt = {d for (s, v, d) in self.triples if s in cur and v == t and 0 <= t < V}
            if not nxt:
                return j, cur
            cur = nxt
        return len(y), cur

    def accepts(self, y, V):
        n, cur = self.walk(y, V)
        return n == len(y) and bool(cur & self.finals)

    def dist(self):
        """Fewest tokens to a final state by relaxation to a fixed point (inf: none reachable)."""
        d = [0 if s in self.finals else np.inf for s in range(self.S)]
        changed = True
        while changed:
            changed = False
            for s, _, t in self.triples:
                if d[t] + 1 < d[s]:
                    d[s] = d[t] + 1
                    changed = True
        return d

    def row(self, s, budget, V, eos):
        bits = np.zeros(V, bool)
        if not 0 <= s < self.S:
            return bits
        d = self.dist()
        for a, v, t in self.triples:
            if a == s and d[t] <= budget:
                bits[v] = True
        bits[eos] = s in self.finals
        return bits

    def language(self, longest):
        """Every accepted sentence of at most ``longest`` tokens, by enumeration from state 0."""
        out, level = set(), {((), 0)}
        for n in range(longest + 1):
            out.update(y for y, s in level if s in self.finals)
            if n == longest:
                break
            level = {(y + (v,), t) for y, s in level for (a, v, t) in self.triples if a == s}
        return out


def seeded_acceptor(seed, V=12, eos=2):
    """A small random deterministic acceptor in which every state reaches a final one: (arcs per state as
    (token, next) lists, finals, sentences to walk)."""
    rs = np.random.RandomState(seed)
    S = int(rs.randint(1, 9))
    toks = [v for v in range(V) if v != eos]
    arcs = []
    for s in range(S):
        n = int(rs.choice([0, 1, 2, 3, len(toks)]))
        ts = sorted(rs.choice(toks, size=n, replace=False).tolist())
        arcs.append([(int(t), int(rs.randint(S))) for t in ts])
    finals = {int(s) for s in range(S) if rs.rand() < 0.4} or {int(rs.randint(S))}
    # repair: a state that reaches no final state becomes final itself (the refusal has its own test)
    acc = TripleAcceptor({(s, v, d) for s, row in enumerate(arcs) for v, d in row}, finals, S)
    finals |= {s for s, d in enumerate(acc.dist()) if d == np.inf}
    sents = []
    for _ in range(12):
        y, s = [], 0
        for _ in range(int(rs.randint(0, 8))):
            if arcs[s] and rs.rand() < 0.85:
                v, s2 = arcs[s][rs.randint(len(arcs[s]))]
                y.append(v)
                s = s2
            else:
                y.append(int(rs.choice([rs.randint(V), eos, V, -1])))
                break
        sents.append(y)
    return arcs, sorted(finals), sents


# ---------------------------------------------------------------------------- the constrained beam
def constrained_beam(encoded, dec_sd, k, langs, ref_lm=None, lm_weight=0.0, length_weight=0.0, sos=1, eos=2, pad=0,
                     max_len=40, temperature=1.0):
    """``langs``: one language for all utterances or a list of one per utterance.  Returns dict(tokens,
    score (the choice's am), lm, complete, records {b: [(tokens, am, lm, step)]} in (step, rank) order,
    steps, gap [B]: per utterance the smallest distance between vals adjacent in rank among its best 2k + 1
    candidates, over all steps (inf where no step had two candidates))."""
    enc, h, c, mask, keys = encoded
    B = enc.shape[1]
    V = dec_sd["proj_linear.weight"].shape[0]
    langs = list(langs) if isinstance(langs, (list, tuple)) else [langs] * B
    rows = FR.TermRows(ref_lm, eos) if ref_lm is not None else None
    w = F(lm_weight)
    rep = np.repeat(np.arange(B), k)
    enc_t, mask_t, keys_t = enc[:, rep], mask[:, rep], keys[:, rep]
    h, c = h[rep], c[rep]
    ctx = np.zeros((B * k, enc.shape[2]), F)
    hist = np.full((max_len + 1, B * k), pad, np.int64)
    hist[0] = sos
    a_buf, g_buf = np.zeros(B * k, F), np.zeros(B * k, F)
    alive = np.ones(B * k, bool)
    records = {b: [] for b in range(B)}
    top_fin = np.zeros(B, bool)
    gap = np.full(B, np.inf)
    len_of = lambda l: F(float(F(length_weight)) * float(l + 1))  # noqa: E731

    def comb(am, lm, l):
        r = F(am)
        if ref_lm is not None:
            r = F(r + F(w * F(lm)))
        return F(r + len_of(l))

    l = 0
    for l in range(max_len):
        logit, h, c, ctx, _ = O.decoder_step(enc_t, mask_t, keys_t, hist[l], h, c, ctx, dec_sd)
        logit = (logit / F(temperature)).astype(F)
        am = (O._log_softmax(logit) + a_buf[:, None]).astype(F)
        if ref_lm is not None:
            term = np.stack([rows([ref_lm.lm_id(ref_lm.bos)] + [ref_lm.lm_id(int(t)) for t in hist[1:l + 1, r]])
                             for r in range(B * k)])
            lm = term if l == 0 else (g_buf[:, None] + term).astype(F)
            val = ((am + (w * lm).astype(F)).astype(F) + len_of(l)).astype(F)
        else:
            lm = np.zeros_like(am)
            val = (am + len_of(l)).astype(F)
        nh, nc, nctx = h.copy(), c.copy(), ctx.copy()
        nhist = hist.copy()
        na, ng, nalive = np.zeros(B * k, F), np.zeros(B * k, F), np.zeros(B * k, bool)
        for b in range(B):
            cands = []  # (val, flat index)
            for j in range(1 if l == 0 else k):
                r = b * k + j
                if not alive[r]:
                    continue
                y = hist[1:l + 1, r].tolist()
                for v in langs[b].tokens_after(y):
                    if v != eos and langs[b].extends(y, v, max_len - 1):
                        cands.append((val[r, v], j * V + v))
                if langs[b].member(y):
                    cands.append((val[r, eos], j * V + eos))
            cands.sort(key=lambda e: (-e[0], e[1]))
            best = cands[:2 * k + 1]
            for x, y_ in zip(best[:-1], best[1:]):
                gap[b] = min(gap[b], float(x[0]) - float(y_[0]))
            ranked = cands[:2 * k]
            for rank, (_, ix) in enumerate(ranked[:k]):
                j, v = divmod(ix, V)
                if v == eos:
                    r = b * k + j
                    records[b].append((hist[1:l + 1, r].tolist(), am[r, eos], lm[r, eos], l))
            if not ranked or ranked[0][1] % V == eos:
                top_fin[b] = True
            slot = 0
            for _, ix in ranked:
                j, v = divmod(ix, V)
                if v == eos or slot >= k:
                    continue
                r, d = b * k + j, b * k + slot
                nh[d], nc[d], nctx[d] = h[r], c[r], ctx[r]
                nhist[:, d] = hist[:, r]
                nhist[l + 1, d] = v
                na[d], ng[d], nalive[d] = am[r, v], lm[r, v], True
                slot += 1
            for s in range(slot, k):  # dead rows: the token eos from row b k, nothing carried
                d = b * k + s
                nh[d], nc[d], nctx[d] = h[b * k], c[b * k], ctx[b * k]
                nhist[:, d] = hist[:, b * k]
                nhist[l + 1, d] = eos
        h, c, ctx, hist, a_buf, g_buf, alive = nh, nc, nctx, nhist, na, ng, nalive
        if top_fin.all():
            break
    toks, score, lms, complete = [], [], [], []
    for b in range(B):
        live = [j for j in range(k) if alive[b * k + j]]  # (the rows the last executed step left)
        if records[b]:
            i = int(np.argmax([comb(a, q, rl) for _, a, q, rl in records[b]]))
            t, a, q, _ = records[b][i]
        elif live:
            j = live[int(np.argmax([comb(a_buf[b * k + j], g_buf[b * k + j], l) for j in live]))]
            t, a, q = hist[1:l + 2, b * k + j].tolist(), a_buf[b * k + j], g_buf[b * k + j]
        else:
            t, a, q = [], F(0), F(0)
        toks.append(t)
        score.append(F(a))
        lms.append(F(q))
        complete.append(bool(records[b]))
    return dict(tokens=toks, score=np.array(score, F), lm=np.array(lms, F), complete=np.array(complete),
                records=records, steps=l + 1, gap=gap)


# ---------------------------------------------------------------------------- shared inputs
B, T = FR.B, FR.T
UTTS = FR.UTTS
EOS_BIASES = (18.0, 28.5)
GPU_K = (2, 4)  # the widths compared with constrained_beam on the device, without an LM (gaps checked on the CPU)
WEIGHTS = (1.5, 1.5)
LM_SEED = 700


@functools.lru_cache(maxsize=None)
def grammar_case(eos_bias):
    """Synthetic peaked weights with the given eos bias, the six utterances fusion_ref.UTTS of T = 101 frames,
    the oracle's plain beam at k = 4, and the record language: every record of that beam, of all
    utterances, except each utterance's own best.  Returns dict(cfg, enc_sd, dec_sd, feats, lens, encoded,
    plain, sentences, lang, grams)."""
    from casr.config import CasrConfig
    from casr.weights import synthetic_state_dicts
    cfg = CasrConfig()
    enc_sd, dec_sd = synthetic_state_dicts(cfg, peaked=True, eos_bias=eos_bias)
    feats = [O.features_from_fbank(fbank_for(b, T)) for b in UTTS]
    lens = [f.shape[0] for f in feats]
    plain = O.beam_decode(feats, lens, enc_sd, dec_sd, 4)
    best = {tuple(t) for t in plain["tokens"]}
    sentences = sorted({tuple(t) for v in plain["records"].values() for t, _ in v} - best)
    grams = FR.lm_grams_from_records(plain["records"], cfg.vocab, LM_SEED)
    return dict(cfg=cfg, enc_sd=enc_sd, dec_sd=dec_sd, feats=feats, lens=lens,
                encoded=FR.encode(feats, lens, enc_sd, dec_sd), plain=plain, sentences=sentences,
                lang=SetLanguage(sentences), grams=grams)


LOOP_TOKENS = tuple(range(10, 20))  # the horizon tests' ten-token loop
HORIZON_EOS_BIAS, HORIZON_B, HORIZON_T = -60.0, 2, 48


def chain_tokens(n):
    """The one sentence of the horizon tests' chain grammar of n tokens."""
    return [100 + (7 * i) % 53 for i in range(n)]


@functools.lru_cache(maxsize=None)
def horizon_case():
    """An eos that can never win on its own: eos_bias -60, B = 2 utterances of T = 48 frames."""
    from casr.config import CasrConfig
    from casr.weights import synthetic_state_dicts
    cfg = CasrConfig()
    enc_sd, dec_sd = synthetic_state_dicts(cfg, peaked=True, eos_bias=HORIZON_EOS_BIAS)
    feats = [O.features_from_fbank(fbank_for(b, HORIZON_T)) for b in range(HORIZON_B)]
    lens = [f.shape[0] for f in feats]
    return dict(cfg=cfg, enc_sd=enc_sd, dec_sd=dec_sd, feats=feats, lens=lens,
                encoded=FR.encode(feats, lens, enc_sd, dec_sd))


@functools.lru_cache(maxsize=None)
def constrained_case(eos_bias, k, with_lm=False):
    case = grammar_case(eos_bias)
    ref = R.RefLM(4, case["cfg"].vocab, case["grams"]) if with_lm else None
    lw, nw = WEIGHTS if with_lm else (0.0, 0.0)
    return constrained_beam(case["encoded"], case["dec_sd"], k, case["lang"], ref, lw, nw)
