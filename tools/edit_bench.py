#!/usr/bin/env python
"""Time the edit distance of an evaluation and the MBR choice over a beam's records, in one process.

  (a) WER: 256 (prediction, reference) pairs of 15-40 symbols with 0-5 edits each, and 256 pairs at 512
      symbols: casr.results.wer_batch on the device (its host-to-device and device-to-host copies
      included), the host entry (casr_edit_distance_host through wer_batch), and the Python loop
      [get_wer(p, r) ...] they replace; each with distances only and with the operation counts.
  (b) MBR: after casr_beam at B = 256, T = 800 with the EOS-bias weights of tools/rescore_bench.py, at
      k = 16 and k = 8: casr_beam alone, casr_beam_mbr alone under both mappings of CASR_OPT_MBR_MAP,
      and casr_mbr_host on the copied records; the record and pair counts, and how many choices differ
      from the first pass's and from the second pass's (casr_beam_rescore with a synthetic 4-gram LM).

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

from rescore_bench import I2W, V, build_model, stats  # noqa: E402

CHARS = [chr(0x4E00 + i) for i in range(3000)]


def make_pairs(n, lo, hi, edits, seed):
    rs = np.random.RandomState(seed)
    preds, refs = [], []
    for _ in range(n):
        ref = [CHARS[i] for i in rs.randint(0, len(CHARS), size=rs.randint(lo, hi + 1))]
        pred = list(ref)
        for _ in range(rs.randint(0, edits + 1)):
            op = rs.randint(3)
            at = rs.randint(len(pred))
            if op == 0:
                pred[at] = CHARS[rs.randint(len(CHARS))]
            elif op == 1 and len(pred) > 1:
                del pred[at]
            else:
                pred.insert(at, CHARS[rs.randint(len(CHARS))])
        preds.append("".join(pred[:hi]))
        refs.append("".join(ref))
    return preds, refs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=800)
    ap.add_argument("--beams", type=int, nargs="+", default=[16, 8])
    ap.add_argument("--ngrams", type=int, default=200000)
    ap.add_argument("--scale", type=float, default=0.5)
    ap.add_argument("--python-steps", type=int, default=3, help="repetitions of the Python loops")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from casr import lib as L
    from casr.config import CasrConfig
    from casr.engine import Engine
    from casr.ngram import NgramLM
    from casr.results import _symbol_rows, get_wer, wer_batch
    from casr.weights import synthetic_state_dicts

    cfg = CasrConfig()
    B, T = args.batch, args.frames
    eng = Engine(cfg, *synthetic_state_dicts(cfg, peaked=True))  # the EOS-bias recipe: hypotheses finish
    note = lambda what: print(f"edit_bench: {what}", file=sys.stderr, flush=True)  # noqa: E731

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

    res = {"metric": "edit_ms", "B": B, "T": T, "precision": eng.precision(), "steps": args.steps,
           "warmup": args.warmup, "scale": args.scale}
    ok = True

    # ------------------------------------------------------------------ (a) WER
    res["wer"] = {}
    for name, (lo, hi, edits) in {"pairs_15_40": (15, 40, 5), "pairs_512": (512, 512, 40)}.items():
        preds, refs = make_pairs(256, lo, hi, edits, 17)
        row = {"pairs": len(preds)}
        for tup in (False, True):
            tag = "ops" if tup else "dist"
            py_steps = args.python_steps if hi <= 40 else 1
            if hi > 40 and tup:
                want = None  # (edit_ops at 512 x 512 takes minutes in Python: not timed)
            else:
                row[f"python_{tag}"], want = host(lambda: [get_wer(p, r, True, tup) for p, r in zip(preds, refs)],
                                                  py_steps, 0)
            row[f"host_{tag}"], got_h = host(lambda: wer_batch(preds, refs, True, tup), args.steps)
            row[f"device_{tag}"], got_d = host(lambda: wer_batch(preds, refs, True, tup, engine=eng), args.steps,
                                               args.warmup)
            ok = ok and got_h == got_d and (want is None or want == got_h)
        a, al, b, bl = (torch.as_tensor(x).to(eng.device) for x in _symbol_rows(preds) + _symbol_rows(refs))
        row["device_kernel_dist"] = events(lambda: eng.edit_distance(a, al, b, bl), args.steps, args.warmup)
        row["device_kernel_ops"] = events(lambda: eng.edit_distance(a, al, b, bl, ops=True), args.steps, args.warmup)
        res["wer"][name] = row
        note(f"wer {name} done")

    # ------------------------------------------------------------------ (b) MBR
    fb = torch.from_numpy(np.random.RandomState(B).standard_normal((B, T, cfg.n_mels)).astype(np.float32)).to(eng.device)
    eng.encode_fbank(fb, torch.full((B,), T, dtype=torch.int32, device=eng.device))
    res["mbr"] = {}
    for k in args.beams:
        row = {"k": k}
        row["beam"] = events(lambda: eng.beam(k, 1.5, 1.5), args.steps, args.warmup)
        first = {n: v.cpu().numpy() for n, v in eng.beam(k, 1.5, 1.5).items()}
        rt, rs, rv = (x.cpu().numpy() for x in eng.beam_records())
        cnt = rv.reshape(B, -1).sum(axis=1).astype(np.int64)
        row["records"] = int(cnt.sum())
        row["records_max_per_utterance"] = int(cnt.max())
        row["pairs"] = int((cnt * (cnt - 1) // 2).sum())
        row["utterances_with_records"] = int((cnt > 0).sum())
        for mp, tag in ((1, "wave_per_pair"), (2, "lane_per_pair")):
            eng.set_option("MBR_MAP", mp)
            row[f"mbr_{tag}"] = events(lambda: eng.beam_mbr(args.scale, length_weight=1.5), args.steps, args.warmup)
        eng.set_option("MBR_MAP", 0)
        row["mbr_default"] = events(lambda: eng.beam_mbr(args.scale, length_weight=1.5), args.steps, args.warmup)
        r = {n: v.cpu().numpy() for n, v in eng.beam_mbr(args.scale, length_weight=1.5, records=True).items()
             if v is not None}
        row["mbr_host"], (best, risk) = host(lambda: L.mbr_host(rt, rs, rv, args.scale, length_weight=1.5, risk=True), 1, 0)
        valid = rv.astype(bool)
        row["choices_equal_host"] = int((r["index"] == best).sum())
        row["risk_max_rel_diff"] = float(np.max(np.abs(r["rec_risk"][valid] - risk[valid]) /
                                                np.maximum(np.abs(risk[valid]), 1e-300))) if valid.any() else 0.0
        ok = ok and row["choices_equal_host"] >= B - B // 100 and row["risk_max_rel_diff"] <= 1e-12
        top = np.array([int(np.argmax(np.where(valid[b].reshape(-1), rs[b].reshape(-1), -np.inf))) if cnt[b] else -1
                        for b in range(B)])
        row["choices_differ_from_first_pass"] = int((r["index"] != top).sum())
        ids, prob, back, _ = build_model(rt, rv, args.ngrams, 5)
        lm = NgramLM.from_ids(ids, prob, back, {w: i for i, w in I2W.items()}, V)
        second = {n: v.cpu().numpy() for n, v in eng.beam_rescore(lm, 1.5, 1.5).items() if v is not None}
        row["choices_differ_from_second_pass"] = int(sum(
            r["tokens"][b, :r["length"][b]].tolist() != second["tokens"][b, :second["length"][b]].tolist()
            for b in range(B)))
        row["mbr_with_lm"] = events(lambda: eng.beam_mbr(args.scale, lm, 1.5, 1.5), args.steps, args.warmup)
        lm.close()
        row["mbr_over_beam"] = round(row["mbr_default"]["median_ms"] / row["beam"]["median_ms"], 5)
        res["mbr"][f"k{k}"] = row
        note(f"mbr k={k} done: {row['records']} records, {row['pairs']} pairs")
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
