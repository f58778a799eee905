#!/usr/bin/env python
"""Time casr_convert_audio (Engine.convert_audio: s16 quantisation on, -1 dB normalisation, the
load_audio defaults) with HIP events, at B = 256 utterances of 8 s and at B = 1, for 8, 44.1 and
48 kHz mono and 48 kHz stereo input, next to casr_log_mel on the batch the conversion produced.

Per case: the median call time, the bytes the operation has to move (input + output, from the
shapes) over that time and as a fraction of the 6.29 TB/s a float4 copy reaches on an MI355X, the
multiply-adds of the FIR (outputs x 2K taps) per second, and the log-mel time.  Output buffers are
allocated once, outside the timed window (ctypes calls on preallocated tensors).  Prints one JSON
line and writes it to profiles/convert/convert_bench.json (--out)."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "chinese-asr_amd"), REPO]

from casr import lib as L  # noqa: E402
from casr.config import CasrConfig  # noqa: E402
from casr.engine import Engine, _ptr, _stream  # noqa: E402

HBM_COPY_TBS = 6.29  # measured float4 copy
CASES = [(8000, 1), (44100, 1), (48000, 1), (48000, 2)]


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


def one(eng, B, seconds, rate, ch, steps, warmup):
    n = int(seconds * rate)
    gen = torch.Generator(device=eng.device).manual_seed(rate + ch + B)
    pcm = 0.2 * torch.randn(B, n, ch, device=eng.device, generator=gen)
    n_in = torch.full((B,), n, dtype=torch.int32, device=eng.device)
    m = L.resample_frames(n, rate)
    wav = torch.empty(B, m, device=eng.device)
    n_out = torch.empty(B, dtype=torch.int32, device=eng.device)
    gain = torch.empty(B, device=eng.device)

    def convert():
        L.check(eng.lib.casr_convert_audio(eng.handle, _ptr(pcm), _ptr(n_in), B, n, ch, rate, m, 1, ctypes.c_float(-1.0),
                                           _ptr(wav), _ptr(n_out), _ptr(gain), _stream()), eng.handle)

    t_max = L.log_mel_frames(m)
    fbank = torch.empty(B, t_max, 80, device=eng.device)
    frames = torch.empty(B, dtype=torch.int32, device=eng.device)

    def log_mel():
        L.check(eng.lib.casr_log_mel(eng.handle, _ptr(wav), _ptr(n_out), B, m, t_max, ctypes.c_float(0.97), _ptr(fbank),
                                     _ptr(frames), _stream()), eng.handle)

    r = {"B": B, "seconds": seconds, "rate": rate, "channels": ch}
    r["convert"] = timed(convert, steps, warmup)
    r["log_mel"] = timed(log_mel, steps, warmup)
    _, _, taps = L.resample_plan(rate)
    nbytes = 4.0 * B * (n * ch + m)
    sec = r["convert"]["median_ms"] * 1e-3
    r["bytes"] = int(nbytes)
    r["tbytes_per_s"] = round(nbytes / sec / 1e12, 4)
    r["fraction_of_hbm_copy"] = round(nbytes / sec / 1e12 / HBM_COPY_TBS, 4)
    r["taps"] = taps
    r["tmac_per_s"] = round(B * m * taps / sec / 1e12, 3)
    r["convert_over_log_mel"] = round(r["convert"]["median_ms"] / r["log_mel"]["median_ms"], 3)
    r["flags"] = eng.device_flags()
    assert int(n_out[0]) == m and int(frames[0]) == t_max
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=8.0)
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 1])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "convert", "convert_bench.json"))
    args = ap.parse_args()
    eng = Engine(CasrConfig())
    res = {"metric": "convert_audio_ms", "device": torch.cuda.get_device_name(eng.device), "steps": args.steps,
           "warmup": args.warmup, "quantize": 1, "norm_db": -1.0, "hbm_copy_tbytes_per_s": HBM_COPY_TBS, "cases": []}
    for B in args.batches:
        for rate, ch in CASES:
            res["cases"].append(one(eng, B, args.seconds, rate, ch, args.steps, args.warmup))
    eng.close()
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
