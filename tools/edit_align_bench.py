#!/usr/bin/env python
"""Time casr_edit_align (Engine.edit_align's entry, outputs preallocated) and main.align_long.

  (a) The edit script of long pairs with HIP events: 1 pair of 16,384 x 16,384, 4 pairs of 3,000 x 3,000
      and 1 pair at the limit, 32,768 x 32,768; b random over 3,000 symbols, a its copy with one edit per
      ten symbols.  Beside them casr_edit_align_host on the same pairs (a host clock, one run), whose
      results the device's must equal.  Per case also the launches, the direction-bit bytes and what
      the times say per launch and per byte.
  (b) main.align_long on the synthetic 60 min recording of tools/segment_bench.py (the 35 s signal of
      tests/segment_ref.py repeated) with synthetic weights, the text its own transcription with one
      edit per twenty characters; beside it main.transcribe on the same recording in the same process,
      alternating (transcribe's code path is the one of the commit before align_long existed).  Host
      clock around work that ends synchronised.

--only CASE runs one case of (a) ``--steps`` times and writes nothing: the target of a
``rocprofv3 --kernel-trace --stats`` run of its own.  --kernel-stats CASE=FILE ... reads the kernel_stats
CSV such a run wrote and adds the split over fill, sweep and backtrace to the case.  Prints one JSON line
and writes it to profiles/edit/edit_align_bench.json (--out)."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "chinese-asr_amd"), REPO, os.path.join(REPO, "tests")]

from casr import lib as L  # noqa: E402
from casr.config import CasrConfig  # noqa: E402
from casr.engine import Engine, _ptr, _stream  # noqa: E402

CASES = {"16k": (1, 16384), "4x3k": (4, 3000), "limit": (1, 32768)}
ALPHABET = 3000


def stats(ms):
    v = sorted(ms)
    med = v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])
    return {"median_ms": round(med, 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4), "n": len(v)}


def make_pairs(n, length, seed):
    """b random, a its copy with length / 10 edits, both cut to ``length``: (a, a_len, b, b_len)."""
    rs = np.random.RandomState(seed)
    a = np.zeros((n, length), np.int32)
    b = rs.randint(0, ALPHABET, size=(n, length)).astype(np.int32)
    al = np.zeros(n, np.int32)
    for k in range(n):
        row = b[k].tolist()
        for _ in range(length // 10):
            op, at = rs.randint(3), rs.randint(len(row))
            if op == 0:
                row[at] = int(rs.randint(ALPHABET))
            elif op == 1:
                del row[at]
            else:
                row.insert(at, int(rs.randint(ALPHABET)))
        row = row[:length]
        a[k, :len(row)], al[k] = row, len(row)
    return a, al, b, np.full(n, length, np.int32)


def device_call(eng, a, al, b, bl):
    dev = eng.device
    t = [torch.from_numpy(x).to(dev) for x in (a, al, b, bl)]
    n, La, Lb = a.shape[0], a.shape[1], b.shape[1]
    out = dict(dist=torch.empty(n, dtype=torch.int32, device=dev), ops=torch.empty(n, 3, dtype=torch.int32, device=dev),
               b_of_a=torch.empty(n, La, dtype=torch.int32, device=dev),
               a_of_b=torch.empty(n, Lb, dtype=torch.int32, device=dev))

    def call():
        L.check(eng.lib.casr_edit_align(eng.handle, _ptr(t[0]), _ptr(t[1]), La, _ptr(t[2]), _ptr(t[3]), Lb, n,
                                        _ptr(out["dist"]), _ptr(out["ops"]), _ptr(out["b_of_a"]), _ptr(out["a_of_b"]),
                                        _stream()), eng.handle)
    return call, out


def events(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    spans = []
    for _ in range(steps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        spans.append((s, e))
    torch.cuda.synchronize()
    return stats([s.elapsed_time(e) for s, e in spans])


def read_kernel_stats(path):
    """rocprofv3's kernel_stats CSV -> {fill, sweep, backtrace: {calls, total_ms}} of the ea_* kernels."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            for key in ("fill", "sweep", "backtrace"):
                if f"ea_{key}_kernel" in name:
                    cur = out.setdefault(key, {"calls": 0, "total_ms": 0.0})
                    cur["calls"] += int(row["Calls"])
                    cur["total_ms"] = round(cur["total_ms"] + float(row["TotalDurationNs"]) * 1e-6, 4)
    return out


def pair_case(eng, name, steps, warmup, host=True):
    n, length = CASES[name]
    a, al, b, bl = make_pairs(n, length, 100 + length)
    plan = L.edit_align_plan(length, length, n)
    call, out = device_call(eng, a, al, b, bl)
    r = {"case": name, "pairs": n, "La": length, "Lb": length, "cells": int(n) * length * length,
         "launches": plan["launches"] + 2, "bits_bytes": plan["bits_bytes"], "workspace_bytes": plan["bytes"]}
    r["device"] = events(call, steps, warmup)
    ms = r["device"]["median_ms"]
    r["us_per_launch"] = round(ms * 1e3 / r["launches"], 3)
    r["bits_gbytes_per_s"] = round(plan["bits_bytes"] / (ms * 1e-3) / 1e9, 2)
    r["gcells_per_s"] = round(r["cells"] / (ms * 1e-3) / 1e9, 2)
    r["flags"] = eng.device_flags()
    if host:
        t0 = time.perf_counter()
        want = L.edit_align_host(a, al, b, bl)
        r["host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        r["equals_host"] = all(np.array_equal(out[k].cpu().numpy(), want[k]) for k in want)
        r["dist"] = want["dist"].tolist()
    return r


def long_case(minutes, repeats):
    import main as MN
    import model as M
    import segment_ref as R
    from casr.weights import synthetic_state_dicts
    cfg = CasrConfig()
    m = M.Model()
    m.load_state_dicts(*synthetic_state_dicts(cfg, peaked=True))
    import types
    i2w = {i: chr(0x4E00 + i) for i in range(cfg.vocab)}
    ab = types.SimpleNamespace(int2word=i2w, word2int={w: i for i, w in i2w.items()})
    n = minutes * 60 * 16000
    x = R.synthetic_recording(7)
    wav = np.tile(x, n // len(x) + 1)[:n]
    segs = MN.transcribe([wav], m, ab)[0]  # (also the warm-up of every shape)
    own = ''.join(s.text for s in segs)
    rs = np.random.RandomState(1)
    text = list(own)
    for at in sorted(rs.choice(len(text), size=len(text) // 20, replace=False).tolist(), reverse=True):
        op = rs.randint(3)
        if op == 0:
            text[at] = i2w[int(rs.randint(10, 3000))]
        elif op == 1:
            del text[at]
        else:
            text.insert(at, i2w[int(rs.randint(10, 3000))])
    text = ''.join(text)
    got = MN.align_long([wav], [text], m, ab)[0]  # warm-up
    t_tr, t_al = [], []
    for _ in range(repeats):
        for fn, sink in ((lambda: MN.transcribe([wav], m, ab), t_tr), (lambda: MN.align_long([wav], [text], m, ab), t_al)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            sink.append((time.perf_counter() - t0) * 1e3)
    r = {"minutes": minutes, "segments": len(segs), "hyp_chars": len(own), "text_chars": len(text),
         "dist": got.dist, "ops": list(got.ops), "interpolated": sum(s.interpolated for s in got),
         "text_restored": ''.join(s.text for s in got) == text,
         "transcribe": stats(t_tr), "align_long": stats(t_al)}
    r["added_ms"] = round(r["align_long"]["median_ms"] - r["transcribe"]["median_ms"], 1)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=sorted(CASES), default=None)
    ap.add_argument("--kernel-stats", nargs="*", default=[], metavar="CASE=FILE")
    ap.add_argument("--minutes", type=int, default=60)
    ap.add_argument("--long-repeats", type=int, default=3)
    ap.add_argument("--no-long", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "edit", "edit_align_bench.json"))
    args = ap.parse_args()
    eng = Engine(CasrConfig())
    if args.only:
        pair_case(eng, args.only, args.steps, args.warmup, host=False)
        eng.close()
        return
    res = {"metric": "edit_align_ms", "device": torch.cuda.get_device_name(eng.device), "steps": args.steps,
           "warmup": args.warmup, "tile": list(L.EDIT_ALIGN_TILE), "cases": []}
    for name in ("16k", "4x3k", "limit"):
        res["cases"].append(pair_case(eng, name, args.steps, args.warmup))
    eng.close()
    for item in args.kernel_stats:
        name, path = item.split("=", 1)
        case = next(c for c in res["cases"] if c["case"] == name)
        case["kernels"] = read_kernel_stats(path)
        case["kernels"]["runs"] = case["kernels"].get("fill", {}).get("calls", 0)  # calls of the profiled run
    if not args.no_long:
        res["align_long"] = long_case(args.minutes, args.long_repeats)
    line = json.dumps(res, ensure_ascii=False)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(json.dumps(res, indent=1, ensure_ascii=False) + "\n")
    print(line)


if __name__ == "__main__":
    main()
