#!/usr/bin/env python
"""Measure relative-entropy pruning (casr_lm_prune) on the estimate bench's seeded corpus: a Zipf(1.1)
law over V = 5,000 ids, --tokens of them (default 10 M) in sentences of 5..40.  The first nine tenths of
the sentences train an order-3 and an order-4 Kneser-Ney model on the device; each is pruned at theta
in {1e-8, 1e-7, 1e-6}.

  kept           the n-grams per order before and after
  device         the whole call (the model already on the device; it ends with the result on the host),
                 a host clock around it since the call is synchronous: warm, then --steps repetitions
  stages         the call's own HIP-event split of the median repetition: linearise, decide, renew,
                 compact, copy (casr_lm_prune_timing)
  host           casr_lm_prune_host on one thread, --host-steps times; its result must equal the
                 device's bit for bit
  perplexity     of the held-out tenth through casr_lm_score, with the full and the pruned model
  terms          casr_lm_terms on 2,048 contexts of the held-out text, with the full and the pruned model

Nothing is claimed in advance: the numbers are written down as measured, also where the device loses.
Prints one JSON line; --out also writes it (profiles/lm_prune/lm_prune_bench.json)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "chinese-asr_amd"), REPO, os.path.join(REPO, "tools")]

from lm_estimate_bench import corpus  # noqa: E402
from rescore_bench import stats  # noqa: E402

STAGES = ("linearise", "decide", "renew", "compact", "copy")
THETAS = (1e-8, 1e-7, 1e-6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=3)
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
    eng = Engine(CasrConfig(max_num_words=V - 4))
    ids, offsets = corpus(args.tokens, V, 1)
    n_sent = len(offsets) - 1
    n_train = n_sent - n_sent // 10
    train_ids, train_off = ids[:offsets[n_train]], offsets[:n_train + 1]
    lens = np.diff(offsets[n_train:]).astype(np.int32)
    L = int(lens.max())
    held = np.zeros((len(lens), L), np.int32)
    for i in range(len(lens)):
        held[i, :lens[i]] = ids[offsets[n_train + i]:offsets[n_train + i + 1]]
    d_held, d_lens = torch.from_numpy(held).to(eng.device), torch.from_numpy(lens).to(eng.device)
    words = float(lens.sum() + len(lens))  # (every sentence's </s> is predicted too)
    rng = np.random.default_rng(2)
    rows = rng.integers(0, len(lens), size=2048)
    res = {"metric": "lm_prune_ms", "V": V, "tokens": int(args.tokens), "train_sentences": int(n_train),
           "held_out_sentences": int(len(lens)), "steps": args.steps, "warmup": args.warmup, "orders": {}}
    ok = True

    def perplexity(lm):
        q = eng.lm_score(lm, d_held, d_lens).double().sum().item()
        return round(10.0 ** (-q / words), 4)

    def terms_ms(lm, order):
        ctx = np.zeros((2048, 3), np.int32)
        nc = np.zeros(2048, np.int32)
        for i, r in enumerate(rows):  # the last order - 1 tokens of a held-out sentence, nearest first
            t = held[r, :lens[r]][::-1][:order - 1]
            ctx[i, :len(t)] = t
            nc[i] = len(t)
        d_ctx, d_nc = torch.from_numpy(ctx).to(eng.device), torch.from_numpy(nc).to(eng.device)
        ms = []
        for i in range(args.warmup + max(args.steps, 5)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.lm_terms(lm, d_ctx, d_nc)
            torch.cuda.synchronize()
            if i >= args.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        return stats(ms)

    for order in [int(x) for x in args.orders.split(",")]:
        est = eng.lm_estimate(torch.from_numpy(train_ids).to(eng.device), torch.from_numpy(train_off).to(eng.device),
                              order).sorted()
        full = ngram.NgramLM.from_ids(est.ids, est.prob, est.backoff, {}, V)
        out = {"ngrams": [len(a) for a in est.ids], "workspace_bytes": full.prune_workspace_bytes(),
               "perplexity_full": perplexity(full), "terms_full": terms_ms(full, order), "thetas": {}}
        for theta in THETAS:
            runs = []
            for i in range(args.warmup + args.steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                dev = eng.lm_prune(full, theta)
                if i >= args.warmup:
                    runs.append(((time.perf_counter() - t0) * 1e3, dev.timing_ms.copy()))
            mid = sorted(runs, key=lambda r: r[0])[len(runs) // 2]
            one = {"kept": [int(c) for c in dev.count_out], "protected": [int(c) for c in dev.n_protected],
                   "degenerate": int(dev.n_degenerate),
                   "device": dict(stats([r[0] for r in runs]), kernels_ms=round(float(mid[1][7]), 4),
                                  stages_ms={s: round(float(mid[1][i]), 4) for i, s in enumerate(STAGES)})}
            dev.sorted()
            hs = []
            for _ in range(args.host_steps):
                p = ctypes.c_void_p()
                t0 = time.perf_counter()
                rc = eng.lib.casr_lm_prune_host(full._host, ctypes.c_double(theta), ctypes.byref(p))
                hs.append((time.perf_counter() - t0) * 1e3)
                assert rc == 0
                host = ngram.LmPruned(eng.lib, p, order)
            pruned = ngram.NgramLM.from_ids(host.ids, host.prob, host.backoff, {}, V)
            one["host"] = stats(hs)
            one["host_over_device"] = round(one["host"]["median_ms"] / one["device"]["median_ms"], 3)
            same = all(np.array_equal(a, b) for x, y in ((dev.ids, host.ids), (dev.kept, host.kept)) for a, b in zip(x, y))
            same = same and all(np.array_equal(a.view(np.uint64), b.view(np.uint64))
                                for x, y in ((dev.delta, host.delta), (dev.backoff_f64, host.backoff_f64))
                                for a, b in zip(x, y))
            same = same and all(np.array_equal(a.view(np.uint32), b.view(np.uint32))
                                for x, y in ((dev.prob, host.prob), (dev.backoff, host.backoff)) for a, b in zip(x, y))
            one["results_agree"] = bool(same)
            ok = ok and same
            one["perplexity"] = perplexity(pruned)
            one["terms"] = terms_ms(pruned, order)
            pruned.close()
            out["thetas"]["%g" % theta] = one
            print("order %d theta %g: kept %s" % (order, theta, one["kept"]), file=sys.stderr, flush=True)
        full.close()
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
