#!/usr/bin/env python
"""Time the N-best list and the confusion network over a beam's records, in one process.

After casr_beam at B = 256, T = 800 with the EOS-bias weights of tools/rescore_bench.py, at k = 8 and
k = 16: casr_beam alone, casr_beam_nbest (N = 8) alone, casr_beam_confusion (M = 4) alone, and the host path
they replace: casr_beam_records, its copy to the host, then casr_nbest_host, casr_posterior_units_host and
casr_confusion_host.  The device's and the host's results must agree (units within 1).

Device calls are timed with HIP events (medians of --steps), host stages with a host clock around work
that ends synchronised.  Per kernel: run the tool once with --kernels-only under a kernel trace
(rocprofv3 --kernel-trace --output-format csv -- python tools/confusion_bench.py --kernels-only) and hand
the trace to the timed run with --kernel-trace: the medians of the cn_* kernels per beam width go into
the result.  Prints one JSON line; --out also writes it to a file."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "chinese-asr_amd"), REPO, os.path.join(REPO, "tools")]

from rescore_bench import median, stats  # noqa: E402

KERNELS = ("cn_prepare_kernel", "cn_align_kernel", "cn_reduce_kernel")


def kernel_medians(path, beams, per_beam):
    """ms per cn_* kernel from a kernel trace of --kernels-only: its dispatches come in the order of
    ``beams``, ``per_beam`` calls each (the first of each beam, a warm-up, is dropped)."""
    spans = {n: [] for n in KERNELS}
    with open(path) as f:
        for r in csv.DictReader(f):
            for n in KERNELS:
                if n in r["Kernel_Name"]:
                    spans[n].append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
    out = {}
    for n, v in spans.items():
        v = [d for _, d in sorted(v)]
        if len(v) != per_beam * len(beams):
            raise SystemExit(f"confusion_bench: {len(v)} dispatches of {n} in {path}, expected {per_beam * len(beams)}")
        for i, k in enumerate(beams):
            out.setdefault(f"k{k}", {})[n] = round(median(v[i * per_beam + 1:(i + 1) * per_beam]), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=800)
    ap.add_argument("--beams", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--nbest", type=int, default=8)
    ap.add_argument("--entries", type=int, default=4)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--kernels-only", action="store_true", help="only --steps + 1 confusion calls per beam width")
    ap.add_argument("--kernel-trace", default=None, help="kernel trace CSV of a --kernels-only run with the same --steps")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "confusion", "confusion_bench.json"))
    args = ap.parse_args()

    import torch
    from casr import lib as L
    from casr.config import CasrConfig
    from casr.engine import Engine
    from casr.weights import synthetic_state_dicts

    cfg = CasrConfig()
    B, T, N, M = args.batch, args.frames, args.nbest, args.entries
    eng = Engine(cfg, *synthetic_state_dicts(cfg, peaked=True))  # the EOS-bias recipe: hypotheses finish
    note = lambda what: print(f"confusion_bench: {what}", file=sys.stderr, flush=True)  # noqa: E731
    fb = torch.from_numpy(np.random.RandomState(B).standard_normal((B, T, cfg.n_mels)).astype(np.float32)).to(eng.device)
    eng.encode_fbank(fb, torch.full((B,), T, dtype=torch.int32, device=eng.device))

    if args.kernels_only:
        for k in args.beams:
            eng.beam(k, 1.5, 1.5)
            for _ in range(args.steps + 1):
                eng.beam_confusion(M, args.scale, length_weight=1.5)
            torch.cuda.synchronize()
        flags = eng.device_flags()
        eng.close()
        return 0 if flags == 0 else 1

    def events(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        spans = []
        for _ in range(args.steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            spans.append((a, b))
        torch.cuda.synchronize()
        return stats([a.elapsed_time(b) for a, b in spans])

    def host(fn, steps):
        out, ms = None, []
        for _ in range(steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return stats(ms), out

    res = {"metric": "confusion_ms", "B": B, "T": T, "N": N, "M": M, "scale": args.scale, "precision": eng.precision(),
           "steps": args.steps, "warmup": args.warmup, "max_len": cfg.max_len, "vocab": cfg.vocab}
    ok = True
    per_kernel = kernel_medians(args.kernel_trace, args.beams, args.steps + 1) if args.kernel_trace else {}
    for k in args.beams:
        row = {"k": k}
        row["beam"] = events(lambda: eng.beam(k, 1.5, 1.5))
        eng.beam(k, 1.5, 1.5)
        row["nbest"] = events(lambda: eng.beam_nbest(N, length_weight=1.5))
        row["confusion"] = events(lambda: eng.beam_confusion(M, args.scale, length_weight=1.5))
        if f"k{k}" in per_kernel:
            row["confusion_kernels_ms"] = per_kernel[f"k{k}"]
        nb = {n: v.cpu().numpy() for n, v in eng.beam_nbest(N, length_weight=1.5).items() if v is not None}
        cn = {n: v.cpu().numpy() for n, v in eng.beam_confusion(M, args.scale, length_weight=1.5, units=True).items()
              if v is not None}

        def host_path():
            rt, rs, rv = (x.cpu().numpy() for x in eng.beam_records())
            hn = L.nbest_host(rt, rs, rv, N, length_weight=1.5)
            unit, _ = L.posterior_units_host(rs, rv, args.scale, length_weight=1.5)
            return rt, rv, hn, unit, L.confusion_host(rt, rv, unit, hn["index"][:, 0], cfg.vocab, M)

        row["host_path"], (rt, rv, hn, unit, hc) = host(host_path, 3)
        row["host_copy_only"], _ = host(lambda: [x.cpu().numpy() for x in eng.beam_records()], 3)
        cnt = rv.reshape(B, -1).sum(axis=1).astype(np.int64)
        row["records"] = int(cnt.sum())
        row["records_max_per_utterance"] = int(cnt.max())
        row["slots"] = int(cn["n_slots"].sum())
        row["nbest_equal_host"] = bool(all(np.array_equal(nb[n], hn[n]) for n in ("index", "tokens", "length")) and
                                       np.array_equal(nb["comb"].view(np.int64), hn["comb"].view(np.int64)))
        row["unit_max_diff"] = int(np.abs(cn["rec_unit"] - unit).max())
        mine = L.confusion_host(rt, rv, cn["rec_unit"], hn["index"][:, 0], cfg.vocab, M)  # on the device's units
        row["confusion_equal_host"] = bool(all(np.array_equal(cn[n], mine[n]) for n in mine))
        ok = ok and row["nbest_equal_host"] and row["confusion_equal_host"] and row["unit_max_diff"] <= 1
        row["nbest_over_beam"] = round(row["nbest"]["median_ms"] / row["beam"]["median_ms"], 5)
        row["confusion_over_beam"] = round(row["confusion"]["median_ms"] / row["beam"]["median_ms"], 5)
        row["host_over_device"] = round(row["host_path"]["median_ms"] /
                                        (row["nbest"]["median_ms"] + row["confusion"]["median_ms"]), 2)
        ok = ok and row["host_over_device"] > 1.0  # the point of the feature
        res[f"k{k}"] = row
        note(f"k={k} done: {row['records']} records, {row['slots']} slots")
    res["flags"] = eng.device_flags()
    res["results_agree"] = bool(ok)
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
