#!/usr/bin/env python
"""Capture beam_tree_len320.npz: the CPU oracle's beam (oracle/casr_oracle.py beam_decode) at the
smallest shape whose plain finalize takes the thread-per-utterance form, max_len = 320 at k = 16, on
two utterances of T = 101 frames (golden_util.fbank_for(b, 101)) with synthetic peaked weights whose
eos cannot win (eos_bias -60): no record, all 320 steps executed.  tests/test_gpu_beam_tree.py compares
the device's beam with it; the oracle takes several seconds here, which a GPU test should not.  Needs
nothing but this repository.  Stored: tokens [2, 320] int32, score [2] float32."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(REPO, "chinese-asr_amd"), REPO, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

from casr.config import CasrConfig  # noqa: E402
from casr.weights import synthetic_state_dicts  # noqa: E402
from golden_util import fbank_for  # noqa: E402
from oracle import casr_oracle as O  # noqa: E402

MAX_LEN, K, FRAMES, EOS_BIAS = 320, 16, [101, 101], -60.0


def main():
    cfg = CasrConfig(max_len=MAX_LEN)
    enc_sd, dec_sd = synthetic_state_dicts(cfg, peaked=True, eos_bias=EOS_BIAS)
    feats = [O.features_from_fbank(fbank_for(b, t)) for b, t in enumerate(FRAMES)]
    ref = O.beam_decode(feats, [f.shape[0] for f in feats], enc_sd, dec_sd, K, max_len=MAX_LEN)
    assert [len(t) for t in ref["tokens"]] == [MAX_LEN] * len(FRAMES)
    np.savez_compressed(os.path.join(HERE, "beam_tree_len320.npz"), tokens=np.asarray(ref["tokens"], np.int32),
                        score=np.asarray(ref["score"], np.float32))
    print("score", ref["score"])


if __name__ == "__main__":
    main()
