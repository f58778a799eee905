#!/usr/bin/env python
"""Time the second pass of BASELINE config 5's shard shape (B = 256, k = 16, T = 800, the EOS-bias
weights, lm_weight = length_weight = 1.5) with one n-gram LM, in one process:

  (a) the host path as it stands: the casr_beam_records expansion and its copy into pinned host
      memory; casr.rescore.ParallelRescorer with 12 worker processes; casr.results.second_pass_arrays
      in this process, all with the same NgramLM;
  (b) casr_beam_rescore on the device;
  (c) casr_beam alone, for scale.

The LM is a synthetic 4-gram model of about 2 million n-grams (its tables are far larger than an
XCD's 4 MiB L2, as a real model's are), seeded with the n-grams of the batch's own records so that
high orders hit.  Device calls are timed with HIP events, host stages with a host clock around work
that ends synchronised.  The choices of (a) and (b) must be equal.  Prints one JSON line; --out also
writes it to a file."""
import argparse
import functools
import json
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "chinese-asr_amd"), REPO]

V = 5004
I2W = {i: chr(0xE000 + i) for i in range(V)}


class FileLM:
    """The LM of an .npz of id arrays, loaded at the first score() (a worker process starts before
    the file exists: the pool must be up before this process initialises the GPU)."""

    def __init__(self, path):
        self.path, self.lm = path, None

    def score(self, s, bos=True):
        if self.lm is None:
            self.lm = load_lm(self.path)
        return self.lm.score(s, bos=bos)


def load_lm(path):
    from casr.ngram import NgramLM
    z = np.load(path)
    order = int(z["order"])
    return NgramLM.from_ids([z[f"ids{n}"] for n in range(1, order + 1)], [z[f"prob{n}"] for n in range(1, order + 1)],
                            [z[f"back{n}"] for n in range(1, order + 1)], {w: i for i, w in I2W.items()}, V)


def build_model(rt, rv, total, seed):
    """Id arrays of a 4-gram model: unigrams for every id, and per higher order the n-grams of the
    records of the first 32 utterances (<s> and </s> included) plus random ones up to `total`."""
    rs = np.random.RandomState(seed)
    share = {2: 0.2, 3: 0.3, 4: 0.5}
    own = {n: set() for n in share}
    for b, l, c in zip(*np.nonzero(rv[:32])):
        ids = [V] + rt[b, l, c, :l].tolist() + [V + 1]
        for n in share:
            own[n].update(tuple(ids[i:i + n]) for i in range(len(ids) - n + 1))
    ids = [np.arange(V + 3, dtype=np.int32).reshape(-1, 1)]
    for n in (2, 3, 4):
        rnd = rs.randint(0, V, size=(int(total * share[n]), n)).astype(np.int32)
        a = np.concatenate([np.array(sorted(own[n]), np.int32).reshape(-1, n), rnd])
        key = np.zeros(len(a), np.uint64)
        for e in range(n):
            key = key * np.uint64(65536) + a[:, e].astype(np.uint64)
        _, first = np.unique(key, return_index=True)
        ids.append(np.ascontiguousarray(a[np.sort(first)]))
    prob = [(-4.0 + 3.9 * rs.rand(len(a))).astype(np.float32) for a in ids]
    back = [(-1.0 * rs.rand(len(a))).astype(np.float32) for a in ids]
    return ids, prob, back, {n: len(own[n]) for n in own}


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def stats(ms):
    return {"median_ms": round(median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=800)
    ap.add_argument("--beam", type=int, default=16)
    ap.add_argument("--ngrams", type=int, default=2000000)
    ap.add_argument("--workers", type=int, default=12)
    ap.add_argument("--host-steps", type=int, default=3, help="repetitions of each host stage")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from casr.rescore import ParallelRescorer
    npz = os.path.join(tempfile.mkdtemp(), "lm.npz")
    pool = ParallelRescorer(functools.partial(FileLM, npz), I2W, V, workers=args.workers)  # before the GPU

    import torch
    from casr.config import CasrConfig
    from casr.engine import Engine
    from casr.results import second_pass_arrays
    from casr.ngram import NgramLM
    from casr.weights import synthetic_state_dicts

    cfg = CasrConfig()
    B, T, k = args.batch, args.frames, args.beam
    eng = Engine(cfg, *synthetic_state_dicts(cfg, peaked=True))  # the EOS-bias recipe: hypotheses finish
    fb = torch.from_numpy(np.random.RandomState(B).standard_normal((B, T, cfg.n_mels)).astype(np.float32)).to(eng.device)
    eng.encode_fbank(fb, torch.full((B,), T, dtype=torch.int32, device=eng.device))

    def events(fn, steps, warmup):
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

    def host(fn, steps, warmup=1):
        out = None
        for _ in range(warmup):
            out = fn()
        ms = []
        for _ in range(steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return stats(ms), out

    res = {"metric": "second_pass_ms", "B": B, "T": T, "k": k, "precision": eng.precision(),
           "lm_weight": 1.5, "length_weight": 1.5, "steps": args.steps, "warmup": args.warmup}
    note = lambda what: print(f"rescore_bench: {what}", file=sys.stderr, flush=True)
    res["beam"] = events(lambda: eng.beam(k, 1.5, 1.5), args.steps, args.warmup)  # (c)
    pinned = [torch.empty(x.shape, dtype=x.dtype, pin_memory=True) for x in eng.beam_records()]

    def records_to_host():
        for h, x in zip(pinned, eng.beam_records()):
            h.copy_(x, non_blocking=True)
        torch.cuda.synchronize()
        return [h.numpy() for h in pinned]

    res["records_expand_and_copy"], (rt, rs, rv) = host(records_to_host, args.steps, args.warmup)  # (a) 1
    res["records_kernel_only"] = events(eng.beam_records, args.steps, args.warmup)
    res["records_bytes"] = int(sum(h.numel() * h.element_size() for h in pinned))
    res["records"] = int(np.count_nonzero(rv))
    res["utterances_with_records"] = int(np.count_nonzero(rv.reshape(B, -1).any(axis=1)))

    note(f"{res['records']} records on the host; building the LM")
    ids, prob, back, own = build_model(rt, rv, args.ngrams, 5)
    np.savez(npz, order=4, **{f"ids{n}": a for n, a in enumerate(ids, 1)},
             **{f"prob{n}": a for n, a in enumerate(prob, 1)}, **{f"back{n}": a for n, a in enumerate(back, 1)})
    lm = NgramLM.from_ids(ids, prob, back, {w: i for i, w in I2W.items()}, V)
    res["lm"] = {"order": 4, "ngrams": [int(len(a)) for a in ids], "from_records": own,
                 "table_bytes": int(sum(16 * (1 << int(np.ceil(np.log2(2 * len(a))))) for a in ids[1:]))}

    note("host stages")
    res["host_parallel_rescorer"], sel_pool = host(lambda: pool.select(rt, rs, rv, 1.5, 1.5), args.host_steps)  # (a) 2
    res["host_parallel_rescorer"]["workers"] = args.workers
    res["host_second_pass_arrays"], sel_host = host(lambda: second_pass_arrays(rt, rs, rv, I2W, lm, 1.5, 1.5),
                                                    max(1, args.host_steps - 1), 0)  # (a) 3
    note("device rescore")
    res["device_rescore"] = events(lambda: eng.beam_rescore(lm, 1.5, 1.5), args.steps, args.warmup)  # (b)
    res["device_rescore_with_rec_lm"] = events(lambda: eng.beam_rescore(lm, 1.5, 1.5, records=True), args.steps,
                                               args.warmup)
    r = {n: v.cpu().numpy() for n, v in eng.beam_rescore(lm, 1.5, 1.5).items() if v is not None}
    same = sel_pool == sel_host
    for b, (t, s) in sel_host.items():
        same = same and r["tokens"][b, :r["length"][b]].tolist() == t and float(r["score"][b]) == s
    res["choices_equal"] = bool(same)
    first = eng.beam(k, 1.5, 1.5)
    res["choices_changed_by_lm"] = int((first["length"].cpu().numpy() != r["length"]).sum())
    res["flags"] = eng.device_flags()
    res["rescore_over_beam"] = round(res["device_rescore"]["median_ms"] / res["beam"]["median_ms"], 5)
    pool.close()
    eng.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if same and res["flags"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
