#!/usr/bin/env python
"""Time the beam search with the n-gram LM fused into its first pass (casr_beam_lm) against the plain
beam and the plain beam followed by the device second pass, in one process and on one encode:
B = 256, T = 800, the EOS-bias weights, lm_weight = length_weight = 1.5, k = 8 and k = 16, with a
synthetic 4-gram model of rescore_bench's size (about 2 million n-grams, seeded with the n-grams of
the batch's own records so that high orders hit).

  (a) casr_beam_lm;
  (b) casr_beam (whose code the fusion does not touch: the figure to report is (a) / (b));
  (c) casr_beam followed by casr_beam_rescore;
  (d) per kernel class (dec_lstm, attention, proj, select) the time of (a) and of (b), from the
      library's own event pairs (a separate pass: the events serialise the launches);
  (e) casr_lm_terms alone on 2,048 and 4,096 contexts taken from the decode's own records.

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


def contexts_from(rt, rv, n, seed):
    """n contexts [n, 3] (nearest first) and their lengths: positions inside the records' own token
    sequences (<s> before the first token), cycled up to n."""
    rs = np.random.RandomState(seed)
    ctx, nc = [], []
    for b, l, c in zip(*np.nonzero(rv)):
        ids = [V] + rt[b, l, c, :l].tolist()
        for p in range(1, len(ids) + 1):
            h = ids[max(0, p - 3):p][::-1]
            ctx.append(h + [0] * (3 - len(h)))
            nc.append(len(h))
    pick = rs.randint(0, len(nc), size=n)
    return np.array(ctx, np.int32)[pick], np.array(nc, np.int32)[pick]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=800)
    ap.add_argument("--beams", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--ngrams", type=int, default=2000000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from casr.config import CasrConfig
    from casr.engine import Engine
    from casr.ngram import NgramLM
    from casr.weights import synthetic_state_dicts

    cfg = CasrConfig()
    B, T = args.batch, args.frames
    eng = Engine(cfg, *synthetic_state_dicts(cfg, peaked=True))  # the EOS-bias recipe: hypotheses finish
    fb = torch.from_numpy(np.random.RandomState(B).standard_normal((B, T, cfg.n_mels)).astype(np.float32)).to(eng.device)
    eng.encode_fbank(fb, torch.full((B,), T, dtype=torch.int32, device=eng.device))

    def events(fn, steps=args.steps, warmup=args.warmup):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        spans = []
        for _ in range(steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            spans.append((a, b))
        torch.cuda.synchronize()
        return stats([a.elapsed_time(b) for a, b in spans])

    def classes(fn, n=5):
        fn()
        eng.profile(DECODE)
        for _ in range(n):
            fn()
        out = {c: {"launches": v[0] // n, "ms": round(v[1] / n, 4)} for c, v in eng.profile_read().items()}
        eng.profile([])
        return out

    note = lambda what: print(f"fusion_bench: {what}", file=sys.stderr, flush=True)
    res = {"metric": "fused_over_beam", "B": B, "T": T, "precision": eng.precision(), "lm_weight": 1.5,
           "length_weight": 1.5, "steps": args.steps, "warmup": args.warmup, "k": {}}
    eng.beam(16, 1.5, 1.5)
    rt, rs, rv = (x.cpu().numpy() for x in eng.beam_records())
    note(f"{int(np.count_nonzero(rv))} records; building the LM")
    ids, prob, back, own = build_model(rt, rv, args.ngrams, 5)
    lm = NgramLM.from_ids(ids, prob, back, {w: i for i, w in I2W.items()}, V)
    res["lm"] = {"order": 4, "ngrams": [int(len(a)) for a in ids], "from_records": own}
    for n in (2048, 4096):
        ctx, nc = contexts_from(rt, rv, n, n)
        ctx, nc = torch.from_numpy(ctx).to(eng.device), torch.from_numpy(nc).to(eng.device)
        res[f"lm_terms_{n}"] = events(lambda: eng.lm_terms(lm, ctx, nc, cfg.eos))
        res[f"lm_terms_{n}"]["bytes_written"] = n * V * 4
    for k in args.beams:
        note(f"k = {k}")
        r = {"R": B * k}
        r["beam"] = events(lambda: eng.beam(k, 1.5, 1.5))
        r["beam_lm"] = events(lambda: eng.beam_lm(lm, k, 1.5, 1.5))

        def two_pass():
            eng.beam(k, 1.5, 1.5)
            eng.beam_rescore(lm, 1.5, 1.5)

        r["beam_then_rescore"] = events(two_pass)
        r["beam_again"] = events(lambda: eng.beam(k, 1.5, 1.5))  # drift check: same code as "beam"
        r["classes_beam"] = classes(lambda: eng.beam(k, 1.5, 1.5))
        r["classes_beam_lm"] = classes(lambda: eng.beam_lm(lm, k, 1.5, 1.5))
        plain = eng.beam(k, 1.5, 1.5)
        second = eng.beam_rescore(lm, 1.5, 1.5)
        fused = eng.beam_lm(lm, k, 1.5, 1.5)
        tok = lambda x: x["tokens"].cpu().numpy()
        r["decode_steps"] = {"beam": int(plain["steps"][0]), "beam_lm": int(fused["steps"][0])}
        r["choices_differ_from_beam"] = int((tok(fused) != tok(plain)).any(axis=1).sum())
        r["choices_differ_from_second_pass"] = int((tok(fused) != tok(second)).any(axis=1).sum())
        r["fused_over_beam"] = round(r["beam_lm"]["median_ms"] / r["beam"]["median_ms"], 4)
        r["fused_over_two_pass"] = round(r["beam_lm"]["median_ms"] / r["beam_then_rescore"]["median_ms"], 4)
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
