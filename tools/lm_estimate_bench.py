#!/usr/bin/env python
"""Time the Kneser-Ney estimate (casr_lm_estimate) on a seeded corpus: a Zipf(1.1) law over V = 5,000
ids, --tokens of them (default 10 M) in sentences of 5..40, at orders 3 and 4.

  device         the whole call (tokens already on the device; it ends with the dense result on the
                 host), a host clock around it since the call is synchronous: warm, then --steps
                 repetitions, median / min / max
  stages         the call's own HIP-event split of the median repetition: count, extend, stats, prob,
                 compact, copy (casr_lm_estimate_timing)
  no_combining   the same with the count kernel's LDS combining off (casr_lm_estimate_combine(0)),
                 the repetitions alternating with the combining ones
  host           casr_lm_estimate_host on one thread, --host-steps times
  lm_create      NgramLM.from_ids on the result (the query tables and successor lists; with upload)

The device's and the host's results must agree bit for bit.  Prints one JSON line; --out also writes it."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "chinese-asr_amd"), REPO, os.path.join(REPO, "tools")]

from rescore_bench import stats  # noqa: E402

STAGES = ("count", "extend", "stats", "prob", "compact", "copy")


def corpus(tokens, V, seed):
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, V + 1) ** 1.1
    ids = rng.choice(V, size=tokens, p=w / w.sum()).astype(np.int32)
    cum = np.cumsum(rng.integers(5, 41, size=tokens // 5 + 1))
    offsets = np.concatenate([[0], cum[cum < tokens], [tokens]])  # (the last sentence takes what is left)
    return ids, offsets.astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-steps", type=int, default=1)
    ap.add_argument("--orders", default="3,4")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from casr import ngram
    from casr.config import CasrConfig
    from casr.engine import Engine

    V = 5000
    cfg = CasrConfig(max_num_words=V - 4)
    eng = Engine(cfg)
    ids, offsets = corpus(args.tokens, V, 1)
    d_ids, d_off = torch.from_numpy(ids).to(eng.device), torch.from_numpy(offsets).to(eng.device)
    res = {"metric": "lm_estimate_ms", "V": V, "tokens": int(args.tokens), "sentences": len(offsets) - 1,
           "positions": int(args.tokens + len(offsets) - 1), "steps": args.steps, "warmup": args.warmup, "orders": {}}
    ok = True
    for order in [int(x) for x in args.orders.split(",")]:
        def call(combine):
            eng.lib.casr_lm_estimate_combine(combine)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            est = eng.lm_estimate(d_ids, d_off, order)
            return (time.perf_counter() - t0) * 1e3, est

        for _ in range(args.warmup):
            call(1), call(0)
        runs = {1: [], 0: []}
        for _ in range(args.steps):
            for c in (1, 0):
                ms, est = call(c)
                runs[c].append((ms, est.timing_ms.copy()))
        eng.lib.casr_lm_estimate_combine(1)
        out = {"workspace_bytes": ngram.workspace_bytes(order, res["positions"])}
        for c, name in ((1, "device"), (0, "no_combining")):
            mid = sorted(runs[c], key=lambda r: r[0])[len(runs[c]) // 2]
            out[name] = dict(stats([r[0] for r in runs[c]]), kernels_ms=round(float(mid[1][7]), 4),
                             stages_ms={s: round(float(mid[1][i]), 4) for i, s in enumerate(STAGES)})
        out["count_combining_speedup"] = round(out["no_combining"]["stages_ms"]["count"] /
                                               max(out["device"]["stages_ms"]["count"], 1e-9), 4)
        dev = eng.lm_estimate(d_ids, d_off, order).sorted()
        out["ngrams"] = [len(a) for a in dev.ids]
        out["fallback"] = [bool(x) for x in dev.fallback]
        hs = []
        for _ in range(args.host_steps):
            t0 = time.perf_counter()
            host = ngram.estimate_host(ids, offsets, order, V)
            hs.append((time.perf_counter() - t0) * 1e3)
        out["host"] = stats(hs)
        out["host_over_device"] = round(out["host"]["median_ms"] / out["device"]["median_ms"], 3)
        same = all(np.array_equal(a, b) for x, y in ((dev.ids, host.ids), (dev.raw, host.raw), (dev.adjusted, host.adjusted))
                   for a, b in zip(x, y))
        same = same and all(np.array_equal(a.view(np.uint64), b.view(np.uint64))
                            for x, y in ((dev.p, host.p), (dev.gamma, host.gamma)) for a, b in zip(x, y))
        same = same and np.array_equal(dev.discounts.view(np.uint64), host.discounts.view(np.uint64))
        out["results_agree"] = bool(same)
        ok = ok and same
        t0 = time.perf_counter()
        lm = ngram.NgramLM.from_ids(dev.ids, dev.prob, dev.backoff, {}, V)
        t1 = time.perf_counter()
        lm.on(eng)
        torch.cuda.synchronize()
        out["lm_create"] = {"host_ms": round((t1 - t0) * 1e3, 3), "device_ms": round((time.perf_counter() - t1) * 1e3, 3)}
        lm.close()
        res["orders"][str(order)] = out
    res["flags"] = eng.device_flags()
    eng.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok and res["flags"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
