#!/usr/bin/env python
"""Time the beam search with the hotword bias in its first pass (casr_beam_bias), without and with the
n-gram LM, against the plain beam (casr_beam) and the fused beam (casr_beam_lm), in one process and on
one encode: B = 256, T = 800, the EOS-bias weights, lm_weight = length_weight = 1.5, bias_weight = 1,
k = 8 and k = 16, about 1,000 phrases (1..4-grams of the batch's own records, so that they match) and
fusion_bench's synthetic 4-gram model.

  (a) casr_beam, casr_beam_lm, casr_beam_bias and casr_beam_bias with the LM, alternated in one loop so
      that drift of the shared machine falls on all four alike;
  (b) per kernel class (dec_lstm, attention, proj, select) the time of each, from the library's own
      event pairs (a separate pass: the events serialise the launches);
  (c) casr_bias_rows alone on 2,048 and 4,096 automaton states taken from the records' own prefixes;
  (d) how many choices differ from the unbiased beam's.

Device calls are timed with HIP events.  Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "chinese-asr_amd"), REPO, os.path.dirname(os.path.abspath(__file__))]

from rescore_bench import I2W, V, build_model, stats  # noqa: E402

DECODE = ["dec_lstm", "attention", "proj", "select"]


def phrases_from(rt, rv, n, seed):
    """About n distinct 1..4-grams of the records' token rows, boosts of 0.5 .. 2 nats per token."""
    rs = np.random.RandomState(seed)
    seen = set()
    for b, l, c in zip(*np.nonzero(rv)):
        t = rt[b, l, c, :l].tolist()
        for m in (1, 2, 3, 4):
            seen.update(tuple(t[i:i + m]) for i in range(len(t) - m + 1))
    seen = sorted(seen)
    pick = rs.permutation(len(seen))[:n]
    ph = [list(seen[i]) for i in sorted(pick)]
    return ph, rs.choice([0.5, 1.0, 1.5, 2.0], size=len(ph)).tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=800)
    ap.add_argument("--beams", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--ngrams", type=int, default=2000000)
    ap.add_argument("--phrases", type=int, default=1000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from casr.bias import PhraseBias
    from casr.config import CasrConfig
    from casr.engine import Engine
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

    def classes(fn, n=5):
        fn()
        eng.profile(DECODE)
        for _ in range(n):
            fn()
        out = {c: {"launches": v[0] // n, "ms": round(v[1] / n, 4)} for c, v in eng.profile_read().items()}
        eng.profile([])
        return out

    note = lambda what: print(f"bias_bench: {what}", file=sys.stderr, flush=True)
    res = {"metric": "bias_over_beam", "B": B, "T": T, "precision": eng.precision(), "lm_weight": 1.5,
           "length_weight": 1.5, "bias_weight": 1.0, "steps": args.steps, "warmup": args.warmup, "k": {}}
    eng.beam(16, 1.5, 1.5)
    rt, rs, rv = (x.cpu().numpy() for x in eng.beam_records())
    ph, boost = phrases_from(rt, rv, args.phrases, 11)
    bias = PhraseBias(ph, {}, V, boost)
    res["phrases"] = {"count": len(ph), "tokens": int(sum(map(len, ph))),
                      "by_length": [int(sum(len(p) == m for p in ph)) for m in (1, 2, 3, 4)]}
    note(f"{int(np.count_nonzero(rv))} records, {len(ph)} phrases; building the LM")
    ids, prob, back, own = build_model(rt, rv, args.ngrams, 5)
    lm = NgramLM.from_ids(ids, prob, back, {w: i for i, w in I2W.items()}, V)
    res["lm"] = {"order": 4, "ngrams": [int(len(a)) for a in ids], "from_records": own}
    # the rows kernel alone, on the states the records' own prefixes reach
    where = np.nonzero(rv)
    rows = np.stack([rt[b, l, c] for b, l, c in zip(*where)]).astype(np.int32)
    rows[rows < 0] = 0
    lens = np.random.RandomState(12).randint(0, where[1] + 1).astype(np.int32)
    states = bias.score_ids(rows, lens)[2]
    res["states"] = {"distinct": int(len(set(states.tolist()))), "at_root": float((states == 0).mean())}
    for n in (2048, 4096):
        st = torch.from_numpy(states[np.random.RandomState(n).randint(0, len(states), size=n)]).to(eng.device)
        res[f"bias_rows_{n}"] = events({"rows": lambda: eng.bias_rows(bias, st)})["rows"]
        res[f"bias_rows_{n}"]["bytes_written"] = n * V * 4
    for k in args.beams:
        note(f"k = {k}")
        calls = {"beam": lambda: eng.beam(k, 1.5, 1.5),
                 "beam_lm": lambda: eng.beam_lm(lm, k, 1.5, 1.5),
                 "beam_bias": lambda: eng.beam_bias(bias, k, 1.0, None, 1.5, 1.5),
                 "beam_bias_lm": lambda: eng.beam_bias(bias, k, 1.0, lm, 1.5, 1.5)}
        r = {"R": B * k, "gain_row_bytes_per_step": B * k * V * 4}
        r.update(events(calls))
        for n, fn in calls.items():
            r["classes_" + n] = classes(fn)
        out = {n: fn() for n, fn in calls.items()}
        tok = lambda x: x["tokens"].cpu().numpy()
        r["decode_steps"] = {n: int(v["steps"][0]) for n, v in out.items()}
        r["choices_differ_bias_from_beam"] = int((tok(out["beam_bias"]) != tok(out["beam"])).any(axis=1).sum())
        r["choices_differ_bias_lm_from_beam_lm"] = int((tok(out["beam_bias_lm"]) != tok(out["beam_lm"])).any(axis=1).sum())
        r["choices_with_bias"] = int((out["beam_bias"]["bias"].cpu().numpy() > 0).sum())
        med = lambda n: r[n]["median_ms"]
        r["bias_over_beam"] = round(med("beam_bias") / med("beam"), 4)
        r["bias_lm_over_beam_lm"] = round(med("beam_bias_lm") / med("beam_lm"), 4)
        r["bias_over_beam_lm"] = round(med("beam_bias") / med("beam_lm"), 4)
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
