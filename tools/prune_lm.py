#!/usr/bin/env python
"""Make an ARPA n-gram LM smaller by relative-entropy pruning.

  tools/prune_lm.py in.arpa out.arpa --theta 1e-7 [--host] [--vocab vocab.json]

in.arpa is any backoff model of order 1..4 (an estimate of tools/build_lm.py or a third party's); its
words are looked up in the ASR vocabulary (the committed vocab.json, or --vocab), and an n-gram with a
word outside it is dropped as casr.ngram.NgramLM drops it.  An n-gram is removed where removing it
changes the model's relative entropy by less than theta (include/casr.h casr_lm_prune has the
definition; Stolcke 1998), prefixes of kept n-grams stay, and the backoffs of the kept contexts are
renewed: on the GPU by default, with --host through casr_lm_prune_host (no GPU needed; the same model bit
for bit).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "chinese-asr_amd"), REPO]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("arpa")
    ap.add_argument("out")
    ap.add_argument("--theta", type=float, required=True, help="the threshold (SRILM's -prune), e.g. 1e-7")
    ap.add_argument("--host", action="store_true", help="prune on the host (no GPU)")
    ap.add_argument("--vocab", default=None, help="vocab.json or dict.pkl (default: the committed vocab.json)")
    args = ap.parse_args()

    from casr import ngram
    from casr.config import CasrConfig
    from casr.vocab import load_vocab

    word2int, int2word = load_vocab(args.vocab)
    cfg = CasrConfig()
    lm = ngram.NgramLM(args.arpa, word2int, cfg.vocab)
    engine = None
    if not args.host:
        from casr.engine import Engine
        engine = Engine(cfg)
    t0 = time.perf_counter()
    out = lm.prune(args.theta, engine=engine)
    dt = time.perf_counter() - t0
    flags = engine.device_flags() if engine is not None else 0
    out.write_arpa(args.out, int2word)
    r = out.pruned
    print(json.dumps({"order": lm.order, "theta": args.theta, "tau": r.tau, "ngrams": [int(c) for c in r.count_in],
                      "kept": [int(c) for c in r.count_out], "protected": [int(c) for c in r.n_protected],
                      "degenerate": int(r.n_degenerate), "where": "host" if args.host else "device",
                      "seconds": round(dt, 3), "flags": flags, "out": args.out}, ensure_ascii=False))
    out.close()
    lm.close()
    if engine is not None:
        engine.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
