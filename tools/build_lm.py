#!/usr/bin/env python
"""Estimate an n-gram LM from text and write it as ARPA.

  tools/build_lm.py corpus.txt out.arpa --order 3 [--prune THETA] [--host] [--vocab vocab.json]

corpus.txt holds one sentence per line (UTF-8); every character that is not white space is a token,
looked up in the ASR vocabulary (the committed vocab.json, or --vocab); a character outside it counts as
<unk>.  The model is the interpolated modified-Kneser-Ney estimate of include/casr.h
(casr_lm_estimate): on the GPU by default, with --host through casr_lm_estimate_host (no GPU needed; the
same model bit for bit before the ARPA's 7 significant digits).  --prune THETA then removes the n-grams
whose relative entropy is below the threshold (casr_lm_prune, the same place and the same bits).  The
file is what ``lm_path=`` of main.ASR and casr.ngram.NgramLM read."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "chinese-asr_amd"), REPO]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("corpus")
    ap.add_argument("out")
    ap.add_argument("--order", type=int, default=3)
    ap.add_argument("--prune", type=float, default=None, metavar="THETA",
                    help="relative-entropy pruning threshold (e.g. 1e-7); default: keep every n-gram")
    ap.add_argument("--host", action="store_true", help="estimate (and prune) on the host (no GPU)")
    ap.add_argument("--vocab", default=None, help="vocab.json or dict.pkl (default: the committed vocab.json)")
    args = ap.parse_args()

    from casr import ngram
    from casr.config import CasrConfig
    from casr.vocab import load_vocab

    word2int, int2word = load_vocab(args.vocab)
    cfg = CasrConfig()
    V = cfg.vocab
    with open(args.corpus, "r", encoding="utf-8") as f:
        sentences = [line.rstrip("\n") for line in f]
    engine = None
    if not args.host:
        from casr.engine import Engine
        engine = Engine(cfg)
    t0 = time.perf_counter()
    lm = ngram.estimate(sentences, args.order, V, word2int=word2int, engine=engine)
    est = lm.estimate
    kept = None
    if args.prune is not None:
        full, lm = lm, lm.prune(args.prune, engine=engine)
        full.close()
        kept = [int(c) for c in lm.pruned.count_out]
    dt = time.perf_counter() - t0
    flags = engine.device_flags() if engine is not None else 0
    lm.write_arpa(args.out, int2word)
    print(json.dumps({"sentences": len(sentences), "positions": est.positions, "order": args.order,
                      "ngrams": [len(a) for a in est.ids], "prune": args.prune, "kept": kept, "types": est.n_types,
                      "discounts": [[round(float(x), 6) for x in d] for d in est.discounts],
                      "fallback": [bool(x) for x in est.fallback], "where": "host" if args.host else "device",
                      "seconds": round(dt, 3), "flags": flags, "out": args.out}, ensure_ascii=False))
    lm.close()
    if engine is not None:
        engine.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
