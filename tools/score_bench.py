#!/usr/bin/env python
"""Time teacher-forced scoring (Engine.score, L = 40) against greedy decoding on one encode, in one
process, at (B, T, F) = (256, 800, 80) and B = 32: score, greedy with CASR_OPT_DEC_FOLD = 0 (the
three-launch step score reuses) and greedy with the default fold.  HIP events around each call,
bench.py's warm-up and step counts (3 and 20); then one instrumented call of each for the
per-class breakdown (casr_profile_read).  Prints one JSON line.

The batched projection's algorithmic work is 2 R 1024 V flop (R = L B rows); its fraction of the
s16x3 ceiling uses VERDICT.md's 833 TF/s."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "chinese-asr_amd"), REPO]

from casr.config import CasrConfig  # noqa: E402
from casr.engine import Engine  # noqa: E402
from casr.weights import synthetic_state_dicts  # noqa: E402

S16X3_CEILING_TFLOPS = 833.0
DEC = ["dec_lstm", "attention", "proj", "select"]


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def timed(fn, steps, warmup):
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
    ms = [a.elapsed_time(b) for a, b in spans]
    return {"median_ms": round(median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def classes(eng, fn):
    eng.profile(DEC)
    fn()
    torch.cuda.synchronize()
    out = {k: {"launches": n, "ms": round(ms, 4)} for k, (n, ms) in eng.profile_read().items()}
    eng.profile([])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=800)
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 32])
    ap.add_argument("--precision", default="s16x3", choices=["s16x3", "f32"])
    args = ap.parse_args()
    cfg = CasrConfig()
    L, V = cfg.max_len, cfg.vocab
    eng = Engine(cfg, *synthetic_state_dicts(cfg, peaked=False))
    eng.set_precision(args.precision)
    res = {"metric": "score_vs_greedy_ms", "precision": eng.precision(), "L": L, "frames": args.frames,
           "steps": args.steps, "warmup": args.warmup, "shapes": {}}
    for B in args.batches:
        rs = np.random.RandomState(B)
        fb = torch.from_numpy(rs.standard_normal((B, args.frames, cfg.n_mels)).astype(np.float32)).to(eng.device)
        frames = torch.full((B,), args.frames, dtype=torch.int32, device=eng.device)
        targets = torch.from_numpy(rs.randint(3, V, size=(B, L)).astype(np.int32)).to(eng.device)
        n = torch.full((B,), L, dtype=torch.int32, device=eng.device)
        eng.encode_fbank(fb, frames)
        r = {}
        r["score"] = timed(lambda: eng.score(targets, n), args.steps, args.warmup)
        r["score_all_outputs"] = timed(lambda: eng.score(targets, n, alignment=True, best=True, mean=True),
                                       args.steps, args.warmup)
        r["score_classes"] = classes(eng, lambda: eng.score(targets, n))
        eng.set_option("DEC_FOLD", 0)
        r["greedy_fold0"] = timed(eng.greedy, args.steps, args.warmup)
        r["greedy_fold0_classes"] = classes(eng, eng.greedy)
        eng.set_option("DEC_FOLD", 1)
        r["greedy_fold1"] = timed(eng.greedy, args.steps, args.warmup)
        r["greedy_fold1_classes"] = classes(eng, eng.greedy)
        r["flags"] = eng.device_flags()
        R = L * B
        flop = 2.0 * R * 1024 * V
        pms = r["score_classes"].get("proj", {}).get("ms")
        if pms:
            tf = flop / (pms * 1e-3) / 1e12
            r["batched_proj"] = {"rows": R, "gflop": round(flop / 1e9, 2), "ms": pms, "tflops": round(tf, 1),
                                 "fraction_of_s16x3_ceiling": round(tf / S16X3_CEILING_TFLOPS, 4)}
        r["score_over_greedy_fold0"] = round(r["score"]["median_ms"] / r["greedy_fold0"]["median_ms"], 4)
        res["shapes"][f"B{B}"] = r
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
