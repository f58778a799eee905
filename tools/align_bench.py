#!/usr/bin/env python
"""Time the monotone attention path (casr_align_path) and what character timestamps add to a decode,
in one process, at B = 256, max_len = 40, T = 800 log-mel frames (Tp = 266) on the attention of a real
greedy decode (synthetic weights, the EOS-bias recipe of tools/rescore_bench.py: hypotheses finish).

  kernel         casr_align_path alone, under the plan's choice and under every CASR_OPT_ALIGN_GROUP
                 (utterances per workgroup), the calls alternating
  timestamps     casr_score + casr_align_path on the decoded tokens (what ``timestamps=True`` adds to a
                 decode), next to casr_greedy's own time
  host_path      what the kernel replaces: the [L][Tp][B] alignment copied to the host, then
                 casr_align_path_host; and separately casr.results.token_times on the copy
  hbm_fraction   the bytes the kernel reads once (4 n_b T_b per utterance: every cell of its rows) over
                 its time, as a fraction of the HBM rates in MI355X_MICROARCH.md (8.0 TB/s spec, 6.29
                 TB/s measured copy)

Device calls are timed with HIP events, host stages with a host clock around work that ends
synchronised.  The device's and the host's results must agree.  Prints one JSON line; --out also writes
it to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "chinese-asr_amd"), REPO, os.path.join(REPO, "tools")]

from rescore_bench import stats  # noqa: E402

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12  # bytes/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=800)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from casr import lib as L
    from casr.config import CasrConfig
    from casr.engine import Engine
    from casr.results import token_times
    from casr.weights import synthetic_state_dicts

    cfg = CasrConfig()
    B, T, Lx = args.batch, args.frames, cfg.max_len
    eng = Engine(cfg, *synthetic_state_dicts(cfg, peaked=True))
    dev = eng.device

    def events(fns, steps, warmup):
        """the calls of fns alternating; per call its own event pair"""
        for _ in range(warmup):
            for fn in fns:
                fn()
        torch.cuda.synchronize()
        spans = [[] for _ in fns]
        for _ in range(steps):
            for i, fn in enumerate(fns):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                spans[i].append((a, b))
        torch.cuda.synchronize()
        return [stats([a.elapsed_time(b) for a, b in s]) for s in spans]

    def host(fn, steps):
        ms, out = [], None
        for _ in range(steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return stats(ms), out

    rs = np.random.RandomState(B)
    frames = rs.randint(T // 2, T + 1, size=B).astype(np.int32)  # utterances of 4 to 8 s
    frames[0] = T
    fb = torch.from_numpy(rs.standard_normal((B, T, cfg.n_mels)).astype(np.float32)).to(dev)
    enc_len = eng.encode_fbank(fb, torch.from_numpy(frames).to(dev))
    g = eng.greedy(alignment=True)
    n = g["out_len"]
    pos = torch.arange(Lx, device=dev, dtype=torch.int32)[None, :]
    tgt = torch.where(pos == n[:, None], torch.full_like(g["tokens"], cfg.eos), g["tokens"])
    tgt_len = torch.clamp(n + 1, max=Lx)
    align = g["alignment"]
    Tp = int(align.shape[1])
    res = {"metric": "align_ms", "B": B, "T": T, "Tp": Tp, "L": Lx, "precision": eng.precision(), "steps": args.steps,
           "warmup": args.warmup, "tokens_mean": float(tgt_len.float().mean()), "enc_len_mean": float(enc_len.float().mean())}

    # ------------------------------------------------------------------ the kernel, every group size
    groups = (0, 16, 8, 4, 2, 1)

    def with_group(gsz):
        def run():
            eng.set_option("ALIGN_GROUP", gsz)
            return eng.align_path(align, enc_len, tgt_len)
        return run

    timed = events([with_group(gsz) for gsz in groups], args.steps, args.warmup)
    eng.set_option("ALIGN_GROUP", 0)
    res["kernel"] = {("default" if gsz == 0 else f"group_{gsz}"): t for gsz, t in zip(groups, timed)}
    cells = int((enc_len.to(torch.int64) * tgt_len.to(torch.int64)).sum())
    res["bytes_read_once"] = 4 * cells
    sec = res["kernel"]["default"]["median_ms"] * 1e-3
    res["hbm_fraction"] = {"of_spec_8.0TBps": round(4 * cells / sec / HBM_SPEC, 5),
                           "of_measured_copy_6.29TBps": round(4 * cells / sec / HBM_COPY, 5)}

    # ------------------------------------------------------------------ what timestamps add to a decode
    def score_and_path():
        sc = eng.score(tgt, tgt_len, alignment=True)
        return eng.align_path(sc["alignment"], enc_len, tgt_len)

    t_greedy, t_add, t_score = events([lambda: eng.greedy(alignment=True), score_and_path,
                                       lambda: eng.score(tgt, tgt_len, alignment=True)], max(args.steps // 5, 5), 2)
    res["timestamps"] = {"greedy": t_greedy, "score_plus_align_path": t_add, "score_alone": t_score,
                         "added_over_greedy": round(t_add["median_ms"] / t_greedy["median_ms"], 4)}

    # ------------------------------------------------------------------ the path it replaces
    d = {k: v.cpu().numpy() for k, v in eng.align_path(align, enc_len, tgt_len).items()}
    enc_h, tgt_h = enc_len.cpu().numpy(), tgt_len.cpu().numpy()
    t_copy, a_h = host(lambda: align.cpu().numpy(), args.host_steps)
    t_host, h = host(lambda: L.align_path_host(a_h, enc_h, tgt_h), args.host_steps)
    t_times, _ = host(lambda: token_times(a_h, enc_h, tgt_h), args.host_steps)
    res["host_path"] = {"copy_to_host": t_copy, "align_path_host": t_host, "token_times": t_times,
                        "copy_bytes": int(a_h.nbytes)}
    ok = all(np.array_equal(d[k], h[k]) for k in ("first", "last", "peak", "path_score"))
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
