#!/usr/bin/env python
"""Time casr_segment and casr_gather_segments (Engine.segment / gather_segments, the default
parameters) with HIP events on long recordings: B = 4 recordings of 10 minutes (T = 60,000 frames
each) and B = 1 of 60 minutes, of the 35 s synthetic signal of tests/segment_ref.py repeated to that
length.  Beside them: casr_log_mel on the same batch (it reads the samples of the same number of
frames; the ratio to it is the number to report) and the numpy restatement of the formulas on the
host (tests/segment_ref.py, one run).

Per case: the median call times, the segment counts, the bytes each call has to move (from the
shapes) over its time, and that the device's segments equal the restatement's.  Output buffers are
allocated once, outside the timed window (ctypes calls on preallocated tensors).  Prints one JSON
line and writes it to profiles/segment/segment_bench.json (--out)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "chinese-asr_amd"), REPO, os.path.join(REPO, "tests")]

import segment_ref as R  # noqa: E402
from casr import lib as L  # noqa: E402
from casr.config import CasrConfig  # noqa: E402
from casr.engine import Engine, _ptr, _stream  # noqa: E402
from casr.segment import SegmentParams, segment_bound  # noqa: E402

CASES = [(4, 10), (1, 60)]  # (recordings, minutes each)


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


def one(eng, B, minutes, steps, warmup):
    n = minutes * 60 * 16000
    base = [R.synthetic_recording(7 + b) for b in range(B)]
    wav_h = np.stack([np.tile(x, n // len(x) + 1)[:n] for x in base])
    wav = torch.from_numpy(wav_h).to(eng.device)
    ns = torch.full((B,), n, dtype=torch.int32, device=eng.device)
    T = L.log_mel_frames(n)
    fbank = torch.empty(B, T, 80, device=eng.device)
    frames = torch.empty(B, dtype=torch.int32, device=eng.device)

    def log_mel():
        L.check(eng.lib.casr_log_mel(eng.handle, _ptr(wav), _ptr(ns), B, n, T, ctypes.c_float(0.97), _ptr(fbank),
                                     _ptr(frames), _stream()), eng.handle)

    params = SegmentParams()
    c = params.struct()
    s_max = segment_bound(T, params)
    start = torch.full((B, s_max), -1, dtype=torch.int32, device=eng.device)
    length = torch.full((B, s_max), -1, dtype=torch.int32, device=eng.device)
    n_seg = torch.empty(B, dtype=torch.int32, device=eng.device)
    thr = torch.empty(B, dtype=torch.int32, device=eng.device)

    def segment():
        L.check(eng.lib.casr_segment(eng.handle, _ptr(fbank), _ptr(frames), B, T, ctypes.byref(c), s_max, _ptr(start),
                                     _ptr(length), _ptr(n_seg), _ptr(thr), _stream()), eng.handle)

    r = {"B": B, "minutes": minutes, "T": T, "s_max": s_max}
    r["log_mel"] = timed(log_mel, steps, warmup)
    r["segment"] = timed(segment, steps, warmup)
    counts = n_seg.cpu().tolist()
    src = torch.tensor([b for b, k in enumerate(counts) for _ in range(k)], dtype=torch.int64, device=eng.device)
    slot = torch.tensor([i for k in counts for i in range(k)], dtype=torch.int64, device=eng.device)
    src32, st, ln = src.to(torch.int32), start[src, slot].contiguous(), length[src, slot].contiguous()
    S, t_seg = int(src.numel()), int(ln.max())
    out = torch.empty(S, t_seg, 80, device=eng.device)
    frames_out = torch.empty(S, dtype=torch.int32, device=eng.device)

    def gather():
        L.check(eng.lib.casr_gather_segments(eng.handle, _ptr(fbank), B, T, _ptr(src32), _ptr(st), _ptr(ln), S, t_seg,
                                             _ptr(out), _ptr(frames_out), _stream()), eng.handle)

    r["gather"] = timed(gather, steps, warmup)
    r["segments"] = counts
    r["t_seg"] = t_seg
    r["flags"] = eng.device_flags()
    # the numpy restatement on the host, on the device's own fbank: one run, and the same segments
    fb_h = fbank.cpu().numpy()
    t0 = time.perf_counter()
    ref = [R.segment_fbank(fb_h[b], T, R.P()) for b in range(B)]
    r["numpy_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    sh, lh, th = start.cpu().numpy(), length.cpu().numpy(), thr.cpu().numpy()
    r["equals_numpy"] = all(int(th[b]) == ref[b][0] and
                            list(zip(sh[b, :counts[b]].tolist(), lh[b, :counts[b]].tolist())) == ref[b][1] for b in range(B))
    seg_bytes = B * T * (80 * 4 + 2 * 2)  # fbank read once, q written and read
    gat_bytes = 4.0 * 80 * (int(ln.sum()) + S * t_seg)  # rows read + the padded batch written
    r["segment_gbytes_per_s"] = round(seg_bytes / (r["segment"]["median_ms"] * 1e-3) / 1e9, 1)
    r["gather_gbytes_per_s"] = round(gat_bytes / (r["gather"]["median_ms"] * 1e-3) / 1e9, 1)
    r["segment_over_log_mel"] = round(r["segment"]["median_ms"] / r["log_mel"]["median_ms"], 4)
    r["gather_over_log_mel"] = round(r["gather"]["median_ms"] / r["log_mel"]["median_ms"], 4)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "segment", "segment_bench.json"))
    args = ap.parse_args()
    eng = Engine(CasrConfig())
    res = {"metric": "segment_ms", "device": torch.cuda.get_device_name(eng.device), "steps": args.steps,
           "warmup": args.warmup, "params": "defaults", "cases": []}
    for B, minutes in CASES:
        res["cases"].append(one(eng, B, minutes, args.steps, args.warmup))
    eng.close()
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
