#!/usr/bin/env python
"""Capture the teacher-forced scoring fixture (score_golden.npz) from the REFERENCE implementation.

Runs only where the reference checkout exists, like make_golden.py, whose stubs, legacy-torch
shims and reference imports it reuses by importing it (nothing is written under the reference).
It is never imported by the tests; its output is.

What is driven: ``RNNDecoder.forward`` (decoder.py:94-137) teacher-forced with
``compute_logit=False`` for 40 steps, then ONE ``proj_linear`` over every step's [h || attn] rows
(the training-time forward the reference keeps commented out, model.py:405-469), and
``util.label_smoothing`` (util.py:265-279) on those logits.

Inputs: the first 8 golden utterances (golden.json "frames"), plain and peaked synthetic weights.
Targets: each utterance's golden greedy tokens, plus eos where the golden run finished (fewer than
40 tokens in a 40-step run).  Steps past an utterance's targets feed eos; nothing of them is stored.

Stored per weight set (name = plain | peaked), arrays [8, 40] with 0 past tgt_len:
  {name}_targets, {name}_tgt_len, {name}_finished
  {name}_token_logp   log_softmax(logits)[target]
  {name}_mean_logp    mean(logits) - logsumexp(logits)
  {name}_ls0, {name}_ls01   util.label_smoothing(logits, targets, ls) at ls = 0 and 0.1
  {name}_align_sum    [40, 8] each step's alignment summed over time (float64)
  {name}_align_expect [40, 8] sum_t t alpha_t (float64)
"""
import json
import os

import numpy as np
import torch

import make_golden as MG

HERE = os.path.dirname(os.path.abspath(__file__))
CFG = MG.CFG
NUTT, L = 8, CFG.max_len


def score_suite(name, peaked, frames, gold, out):
    enc_sd, dec_sd = MG.synthetic_state_dicts(CFG, peaked=peaked)
    m = MG.build_ref_model(enc_sd, dec_sd)
    feats = [MG.ref_features(MG.fbank_for(b, T))[1] for b, T in enumerate(frames)]
    lens = torch.tensor([f.shape[0] for f in feats])
    toks = gold["tokens"][:NUTT]
    assert gold["steps"] == L
    fin = np.array([len(t) < L for t in toks])
    n = np.array([len(t) + int(f) for t, f in zip(toks, fin)], np.int32)
    targets = np.zeros((NUTT, L), np.int64)
    for b, t in enumerate(toks):
        targets[b, :len(t)] = t
        if fin[b]:
            targets[b, len(t)] = CFG.eos
    with torch.no_grad():
        enc_out, enc_len, state = m.encoder(feats, lens)
        mask = MG.ref_model.get_mask_for_softmax(enc_len)
        cell_state = m.decoder.get_initial_state(NUTT, state)
        keys, values = m.attn_mechanism.compute_key_value(enc_out)
        attn = None
        rows, aligns = [], []
        for l in range(L):
            if l == 0:
                feed = torch.full((NUTT,), CFG.sos, dtype=torch.long)
            else:
                feed = torch.from_numpy(np.where(l - 1 < n, targets[:, l - 1], CFG.eos))
            d = m.decoder(enc_out, mask, keys, values, feed, cell_state, attn, compute_logit=False)
            assert d.logit is None
            attn, cell_state = d.attn_hidden_state, d.cell_state
            rows.append(torch.cat((cell_state[-1][0], attn), -1))
            aligns.append(d.alignment)
        logits = m.decoder.proj_linear(torch.cat(rows, 0))           # [L * B, V], row l * B + b
        tgt = torch.from_numpy(targets.T.reshape(-1))               # the same row order
        logp = torch.log_softmax(logits, 1).gather(1, tgt[:, None])[:, 0]
        mean = logits.mean(1) - torch.logsumexp(logits, 1)
        ls0 = MG.ref_util.label_smoothing(logits, tgt, 0.0)
        ls01 = MG.ref_util.label_smoothing(logits, tgt, 0.1)
    keep = (np.arange(L)[None, :] < n[:, None])

    def bl(x):  # [L * B] -> [B, L], 0 past tgt_len
        return np.where(keep, x.numpy().reshape(L, NUTT).T, 0).astype(np.float32)

    out[f"{name}_targets"] = targets.astype(np.int32)
    out[f"{name}_tgt_len"] = n
    out[f"{name}_finished"] = fin
    out[f"{name}_token_logp"] = bl(logp)
    out[f"{name}_mean_logp"] = bl(mean)
    out[f"{name}_ls0"] = bl(ls0)
    out[f"{name}_ls01"] = bl(ls01)
    out[f"{name}_align_sum"] = np.stack([a.double().sum(0).numpy() for a in aligns])
    t = torch.arange(aligns[0].shape[0], dtype=torch.float64)[:, None]
    out[f"{name}_align_expect"] = np.stack([(a.double() * t).sum(0).numpy() for a in aligns])
    return n


def main():
    with open(os.path.join(HERE, "golden.json"), encoding="utf-8") as f:
        meta = json.load(f)
    frames = [int(x) for x in meta["frames"]][:NUTT]
    out = {}
    for name, peaked in (("plain", False), ("peaked", True)):
        n = score_suite(name, peaked, frames, meta[name]["greedy"], out)
        tot = out[f"{name}_token_logp"].sum(1)
        print(name, "tgt_len", n.tolist(), "total", np.round(tot, 4).tolist())
    np.savez_compressed(os.path.join(HERE, "score_golden.npz"), **out)


if __name__ == "__main__":
    main()
