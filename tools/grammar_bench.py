#!/usr/bin/env python
"""Time the grammar-constrained beam search (casr_beam_grammar), without and with the n-gram LM, against
the plain beam (casr_beam), the fused beam (casr_beam_lm) and the biased beam (casr_beam_bias), in one
process and on one encode: B = 256, T = 800, the EOS-bias weights, lm_weight = length_weight = 1.5, k = 8
and k = 16, fusion_bench's synthetic 4-gram model, and three grammars:

  universal  every token everywhere (one state, V - 1 arcs): what the constraint's machinery costs
  trie       about 1,000 phrases taken from the batch's own records
  digits     a loop over ten tokens, 3 to 11 of them

  (a) the calls alternated in one loop, so that drift of the shared machine falls on all alike;
  (b) per kernel class (dec_lstm, attention, proj, select) the time of each, from the library's own
      event pairs (a separate pass: the events serialise the launches);
  (c) casr_grammar_rows alone on 2,048 states of the trie, beside casr_bias_rows on 2,048 automaton
      states: a mask row is V / 8 bytes where a gain row is 4 V.

Device calls are timed with HIP events.  Prints one JSON line; --out also writes it to a file (default
profiles/grammar/grammar_bench.json)."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "chinese-asr_amd"), REPO, os.path.dirname(os.path.abspath(__file__))]

from bias_bench import phrases_from  # noqa: E402
from rescore_bench import I2W, V, build_model, stats  # noqa: E402

DECODE = ["dec_lstm", "attention", "proj", "select"]


def sentences_from(rt, rv, n, seed):
    """About n distinct records (token lists) of the batch."""
    seen = sorted({tuple(rt[b, l, c, :l].tolist()) for b, l, c in zip(*np.nonzero(rv)) if l > 0})
    pick = np.random.RandomState(seed).permutation(len(seen))[:n]
    return [list(seen[i]) for i in sorted(pick)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=800)
    ap.add_argument("--beams", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--ngrams", type=int, default=2000000)
    ap.add_argument("--phrases", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "grammar", "grammar_bench.json"))
    args = ap.parse_args()

    import torch
    from casr.bias import PhraseBias
    from casr.config import CasrConfig
    from casr.engine import Engine
    from casr.grammar import Grammar
    from casr.ngram import NgramLM
    from casr.weights import synthetic_state_dicts

    cfg = CasrConfig()
    B, T = args.batch, args.frames
    eng = Engine(cfg, *synthetic_state_dicts(cfg, peaked=True))  # the EOS-bias recipe: hypotheses finish
    fb = torch.from_numpy(np.random.RandomState(B).standard_normal((B, T, cfg.n_mels)).astype(np.float32)).to(eng.device)
    eng.encode_fbank(fb, torch.full((B,), T, dtype=torch.int32, device=eng.device))

    def span(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        return a, b

    def events(fns, steps=args.steps, warmup=args.warmup):
        """{name: stats} of the calls, alternated: one of each per round."""
        for _ in range(warmup):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        spans = {n: [] for n in fns}
        for _ in range(steps):
            for n, fn in fns.items():
                spans[n].append(span(fn))
        torch.cuda.synchronize()
        return {n: stats([a.elapsed_time(b) for a, b in v]) for n, v in spans.items()}

    def classes(fn, n=3):
        fn()
        eng.profile(DECODE)
        for _ in range(n):
            fn()
        out = {c: {"launches": v[0] // n, "ms": round(v[1] / n, 4)} for c, v in eng.profile_read().items()}
        eng.profile([])
        return out

    note = lambda what: print(f"grammar_bench: {what}", file=sys.stderr, flush=True)  # noqa: E731
    res = {"metric": "grammar_over_beam", "B": B, "T": T, "precision": eng.precision(), "lm_weight": 1.5,
           "length_weight": 1.5, "steps": args.steps, "warmup": args.warmup, "k": {}}
    eng.beam(16, 1.5, 1.5)
    rt, rs, rv = (x.cpu().numpy() for x in eng.beam_records())
    sents = sentences_from(rt, rv, args.phrases, 11)
    digits = list(range(10, 20))
    grammars = {"universal": Grammar.universal(V, cfg.eos), "trie": Grammar.from_phrases(sents, {}, V, cfg.eos),
                "digits": Grammar.repeat([[d] for d in digits], 3, 11, None, V, cfg.eos)}
    res["grammars"] = {n: {"states": g.n_states, "arcs": g.n_arcs, "dist_start": int(g.dist[0])}
                       for n, g in grammars.items()}
    res["grammars"]["trie"]["sentences"] = len(sents)
    ph, boost = phrases_from(rt, rv, args.phrases, 11)
    bias = PhraseBias(ph, {}, V, boost)
    note(f"{int(np.count_nonzero(rv))} records, {len(sents)} sentences, {len(ph)} phrases; building the LM")
    ids, prob, back, own = build_model(rt, rv, args.ngrams, 5)
    lm = NgramLM.from_ids(ids, prob, back, {w: i for i, w in I2W.items()}, V)
    res["lm"] = {"order": 4, "ngrams": [int(len(a)) for a in ids], "from_records": own}
    # the rows kernels alone: 2,048 states of the trie (mask rows) and of the phrase automaton (gain rows)
    n = 2048
    trie = grammars["trie"]
    gst = torch.from_numpy(np.random.RandomState(n).randint(0, trie.n_states, size=n).astype(np.int32)).to(eng.device)
    bst = torch.zeros(n, dtype=torch.int32, device=eng.device)
    rows = events({"grammar_rows": lambda: eng.grammar_rows(trie, gst, 20), "bias_rows": lambda: eng.bias_rows(bias, bst)})
    rows["grammar_rows"]["bytes_written"] = n * trie.mask_words * 4
    rows["bias_rows"]["bytes_written"] = n * V * 4
    rows["bias_over_grammar_rows"] = round(rows["bias_rows"]["median_ms"] / rows["grammar_rows"]["median_ms"], 2)
    res["rows_2048"] = rows
    for k in args.beams:
        note(f"k = {k}")
        calls = {"beam": lambda: eng.beam(k, 1.5, 1.5),
                 "beam_lm": lambda: eng.beam_lm(lm, k, 1.5, 1.5),
                 "beam_bias": lambda: eng.beam_bias(bias, k, 1.0, None, 1.5, 1.5),
                 "beam_bias_lm": lambda: eng.beam_bias(bias, k, 1.0, lm, 1.5, 1.5)}
        for name, g in grammars.items():
            calls["grammar_" + name] = lambda g=g: eng.beam_grammar(g, k, None, 0.0, 1.5)
            calls["grammar_" + name + "_lm"] = lambda g=g: eng.beam_grammar(g, k, lm, 1.5, 1.5)
        r = {"R": B * k, "mask_row_bytes_per_step": B * k * trie.mask_words * 4, "gain_row_bytes_per_step": B * k * V * 4}
        r.update(events(calls))
        for name in ("beam", "beam_bias", "grammar_universal", "grammar_trie", "grammar_universal_lm"):
            r["classes_" + name] = classes(calls[name])
        out = {name: fn() for name, fn in calls.items()}
        r["decode_steps"] = {name: int(v["steps"][0]) for name, v in out.items()}
        r["complete"] = {name: int(v["complete"].sum()) for name, v in out.items() if "complete" in v}
        med = lambda name: r[name]["median_ms"]  # noqa: E731
        r["ratios"] = {"universal_over_beam": round(med("grammar_universal") / med("beam"), 4),
                       "universal_lm_over_beam_lm": round(med("grammar_universal_lm") / med("beam_lm"), 4),
                       "universal_over_bias": round(med("grammar_universal") / med("beam_bias"), 4),
                       "universal_lm_over_bias_lm": round(med("grammar_universal_lm") / med("beam_bias_lm"), 4),
                       "trie_over_beam": round(med("grammar_trie") / med("beam"), 4),
                       "digits_over_beam": round(med("grammar_digits") / med("beam"), 4)}
        res["k"][str(k)] = r
    res["flags"] = eng.device_flags()
    eng.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if res["flags"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
