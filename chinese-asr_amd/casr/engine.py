"""Device-side engine: one casr handle per GPU, torch tensors as caller-owned buffers.

PyTorch supplies device memory, the current HIP stream and (for multi-GPU) RCCL; every
compute step is a call into the HIP C-ABI library.  There is no CPU or torch-op fallback:
without a GPU or the library, construction raises.
"""
import atexit
import ctypes
import os
import weakref

import numpy as np
import torch

from . import lib as _lib
from .config import CasrConfig

# casr_device_flags guard bits (include/casr.h) that invalidate results
FLAG_REC_TIMEOUT = 32   # a persistent-recurrence hand-off wait expired: that encode is invalid
FLAG_F16_RANGE = 128    # s16x3 / s16x1: an activation beyond the f16 range, the split images are wrong


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# Every live Engine, closed at interpreter exit before module teardown: a handle's device work is
# drained and its buffers freed while the HIP runtime (and a profiler attached to it) is still
# fully up, not from __del__ during finalisation in whatever order the garbage collector picks.
_LIVE = weakref.WeakSet()


@atexit.register
def _close_all():
    for e in list(_LIVE):
        try:
            e.close()
        except Exception:
            pass


class Engine:
    """casr handle bound to packed weights on one device.

    arithmetic: "s16x3" (default, the shipped library) or "s16x1", the opt-in perf arithmetic of
    the libcasr_hip_s16x1.so build (include/casr.h CASR_PREC_S16X1: one f16 MFMA per split
    product; token ids not identical to the reference's).  Either can run "f32" by set_precision."""

    def __init__(self, cfg: CasrConfig, enc_sd=None, dec_sd=None, device=None, packed=None, arithmetic="s16x3"):
        if not torch.cuda.is_available():
            raise _lib.CasrError("casr Engine needs an MI355X GPU (torch.cuda.is_available() is False)")
        self.cfg = cfg
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else
                                   torch.device(device).index or 0)
        self.lib = _lib.load(variant=_lib.VARIANT_OF[arithmetic])
        self.handle = ctypes.c_void_p()
        c = _lib.config_struct(cfg)
        _lib.check(self.lib.casr_create(ctypes.byref(c), self.device.index, ctypes.byref(self.handle)), lib=self.lib)
        _lib.register_handle(self.handle, self.lib)
        _LIVE.add(self)
        self.packed = None
        if packed is None and enc_sd is not None:
            packed = _lib.pack_weights(cfg, enc_sd, dec_sd)
        if packed is not None:  # no weights: front-end only (log_mel / features)
            self.bind(packed)
        self._B = self._Tp = None
        self.requested = arithmetic
        # A/B tooling hook (tools/probes): CASR_OPTS="REC_SLEEP=2,REC_POLL_GAP=3" sets tuning
        # options on every new handle; the library itself reads no environment
        for item in filter(None, os.environ.get("CASR_OPTS", "").split(",")):
            name, val = item.split("=")
            self.set_option(name.strip(), int(val))

    def bind(self, packed):
        """packed: host numpy blob or a device tensor (e.g. received by RCCL broadcast)."""
        if isinstance(packed, np.ndarray):
            packed = torch.from_numpy(packed).to(self.device)
        if packed.device != self.device or packed.dtype != torch.float32:
            raise ValueError("packed weights must be a float32 tensor on the engine device")
        want = _lib.packed_floats(self.cfg)
        if packed.numel() != want:
            # a blob packed by another build (e.g. broadcast from a rank running a different
            # library version) would be read past its end by the kernels
            raise ValueError(f"packed weights hold {packed.numel()} floats; this build's layout has {want}")
        self.packed = packed.contiguous()
        _lib.check(self.lib.casr_bind_weights(self.handle, _ptr(self.packed)), self.handle)

    def close(self):
        """Destroy the handle (casr_destroy drains the device first).  Idempotent."""
        if self.handle:
            _lib.unregister_handle(self.handle)
            self.lib.casr_destroy(self.handle)
            self.handle = ctypes.c_void_p()
        _LIVE.discard(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ features
    def convert_audio(self, pcm, n_in, rate, channels=None, quantize=True, norm_db=-1.0, m_max=None):
        """pcm [B, n_max_in, channels] (or [B, n_max_in] mono) float32, n_in [B] frames per utterance,
        one integer rate -> (wav [B, m_max] 16 kHz mono float32, zero past n_out; n_out [B] int32;
        gain [B]).  casr_convert_audio (include/casr.h): downmix, polyphase Kaiser-sinc resampling,
        s16 quantisation (quantize) and peak normalisation to norm_db dBFS (>= 0: off); the
        reference's convert_audio (main.py:19-24) without ffmpeg or sox.  Returns after enqueueing:
        wav and n_out feed log_mel directly."""
        pcm = torch.as_tensor(pcm).to(self.device, torch.float32)
        if pcm.dim() == 2:
            pcm = pcm.unsqueeze(-1)
        if pcm.dim() != 3 or (channels is not None and pcm.shape[2] != int(channels)):
            raise ValueError(f"convert_audio: pcm must be [B, n_max_in, channels={channels}], got {tuple(pcm.shape)}")
        pcm = pcm.contiguous()
        B, n_max_in, ch = pcm.shape
        ns = torch.as_tensor(n_in).to(self.device, torch.int32).contiguous()
        if ns.shape != (B,):
            raise ValueError(f"convert_audio: n_in must be [B={B}]")
        need = int(self.lib.casr_resample_frames(int(n_max_in), int(rate)))  # -1: the call below says why
        m_max = max(need, 1) if m_max is None else int(m_max)
        wav = torch.empty(B, m_max, device=self.device, dtype=torch.float32)
        n_out = torch.empty(B, device=self.device, dtype=torch.int32)
        gain = torch.empty(B, device=self.device, dtype=torch.float32)
        _lib.check(self.lib.casr_convert_audio(self.handle, _ptr(pcm), _ptr(ns), B, n_max_in, ch, int(rate), m_max,
                                               int(bool(quantize)), ctypes.c_float(norm_db), _ptr(wav), _ptr(n_out),
                                               _ptr(gain), _stream()), self.handle)
        self._keep_convert = (pcm, ns)  # read by the enqueued kernels
        return wav, n_out, gain

    def log_mel(self, wav, n_samples, t_max=None, preemphasis=0.97):
        """wav [B, n_max] float32 (device), n_samples [B] int (device or host) ->
        (fbank [B, t_max, 80] log-mel, frames [B] int32).  get_log_mel data.py:167-224."""
        wav = wav.to(self.device, torch.float32).contiguous()
        B, n_max = wav.shape
        ns = torch.as_tensor(n_samples).to(self.device, torch.int32).contiguous()
        t_max = _lib.log_mel_frames(n_max) if t_max is None else int(t_max)
        fbank = torch.empty(B, max(t_max, 1), self.cfg.n_mels, device=self.device, dtype=torch.float32)
        frames = torch.empty(B, device=self.device, dtype=torch.int32)
        _lib.check(self.lib.casr_log_mel(self.handle, _ptr(wav), _ptr(ns), B, n_max, max(t_max, 1),
                                         ctypes.c_float(preemphasis), _ptr(fbank), _ptr(frames), _stream()),
                   self.handle)
        return fbank, frames

    def features(self, fbank, frames, eps=1e-6):
        """fbank [B, T, n_mels] float32 (device), frames [B] int32 (device) ->
        (feat [B, T//3, feat_dim], feat_len [B] int32).  eps < 0: no CMVN."""
        fbank = fbank.contiguous()
        B, T, _ = fbank.shape
        feat = torch.empty(B, T // 3, self.cfg.feat_dim, device=self.device, dtype=torch.float32)
        flen = torch.empty(B, device=self.device, dtype=torch.int32)
        _lib.check(self.lib.casr_features(self.handle, _ptr(fbank), _ptr(frames.to(torch.int32).contiguous()),
                                          B, T, ctypes.c_float(eps), _ptr(feat), _ptr(flen), _stream()),
                   self.handle)
        return feat, flen

    def segment(self, fbank, frames, params=None, s_max=None):
        """Cut long recordings at their pauses (casr_segment, include/casr.h): fbank [B, T, n_mels]
        float32 and frames [B] int32 on the device, as log_mel returns them -> device tensors
        (seg_start [B, s_max], seg_len [B, s_max], n_seg [B], thr [B]), all int32.  n_seg[b] is the
        true count even above s_max; entries past it are -1.  s_max defaults to the bound
        (casr.segment.segment_bound).  Returns after enqueueing."""
        from .segment import SegmentParams, segment_bound
        params = (params or SegmentParams()).validate()
        fbank = fbank.to(self.device, torch.float32).contiguous()
        B, T, _ = fbank.shape
        frames = torch.as_tensor(frames).to(self.device, torch.int32).contiguous()
        if frames.shape != (B,):
            raise ValueError(f"segment: frames must be [B={B}]")
        s_max = segment_bound(T, params) if s_max is None else int(s_max)
        start = torch.full((B, s_max), -1, device=self.device, dtype=torch.int32)
        length = torch.full((B, s_max), -1, device=self.device, dtype=torch.int32)
        n_seg = torch.empty(B, device=self.device, dtype=torch.int32)
        thr = torch.empty(B, device=self.device, dtype=torch.int32)
        c = params.struct()
        _lib.check(self.lib.casr_segment(self.handle, _ptr(fbank), _ptr(frames), B, T, ctypes.byref(c), s_max,
                                         _ptr(start), _ptr(length), _ptr(n_seg), _ptr(thr), _stream()), self.handle)
        self._keep_segment = (fbank, frames)  # read by the enqueued kernels
        return start, length, n_seg, thr

    def gather_segments(self, fbank, src, start, length, t_seg=None):
        """Copy S segments of fbank [B, T, n_mels] into a padded batch (casr_gather_segments): src, start,
        length [S] int (recording, first frame, frames) -> (out [S, t_seg, n_mels], zero past each
        length; frames_out [S] int32), what features and encode_fbank take.  t_seg defaults to the
        longest length (one host read when they are device tensors)."""
        fbank = fbank.to(self.device, torch.float32).contiguous()
        B, T, n_mels = fbank.shape
        src, start, length = (torch.as_tensor(x).to(self.device, torch.int32).contiguous() for x in (src, start, length))
        S = int(src.shape[0])
        if src.shape != (S,) or start.shape != (S,) or length.shape != (S,):
            raise ValueError("gather_segments: src, start and length must be [S]")
        if t_seg is None:
            t_seg = max(int(length.max()), 1) if S else 1
        out = torch.empty(S, int(t_seg), n_mels, device=self.device, dtype=torch.float32)
        frames_out = torch.empty(S, device=self.device, dtype=torch.int32)
        if S:
            _lib.check(self.lib.casr_gather_segments(self.handle, _ptr(fbank), B, T, _ptr(src), _ptr(start), _ptr(length),
                                                     S, int(t_seg), _ptr(out), _ptr(frames_out), _stream()), self.handle)
        self._keep_gather_seg = (fbank, src, start, length)
        return out, frames_out

    def gather(self, utts, lens, Tp=None):
        """list of B device tensors [T_b, feat_dim] -> padded [B, Tp, feat_dim]."""
        B = len(utts)
        utts = [u.contiguous().to(self.device, torch.float32) for u in utts]
        Tp = int(max(int(u.shape[0]) for u in utts)) if Tp is None else Tp
        # the pointer array goes up from pinned memory, stream-ordered: a copy from pageable memory would
        # make the host wait for everything already enqueued on the caller's stream
        ptrs = torch.tensor([u.data_ptr() for u in utts], dtype=torch.int64).pin_memory()
        ptrs = ptrs.to(self.device, non_blocking=True)
        lens_d = lens.to(self.device, torch.int32).contiguous()
        feat = torch.empty(B, Tp, self.cfg.feat_dim, device=self.device, dtype=torch.float32)
        _lib.check(self.lib.casr_gather_utterances(self.handle, _ptr(ptrs), _ptr(lens_d), B, Tp, _ptr(feat),
                                                   _stream()), self.handle)
        self._keep = (utts, ptrs)
        return feat, lens_d

    # ------------------------------------------------------------------ encoder
    def encode(self, feat, lens):
        feat = feat.contiguous()
        B, Tp, _ = feat.shape
        lens = lens.to(self.device, torch.int32).contiguous()
        _lib.check(self.lib.casr_encode(self.handle, _ptr(feat), _ptr(lens), B, Tp, _stream()), self.handle)
        self._B, self._Tp = B, Tp
        self._lens = lens

    def encode_fbank(self, fbank, frames, eps=1e-6):
        """features + encode in one call (casr_encode_fbank): fbank [B, T, n_mels] float32 and
        frames [B] int32 on the device; the features stay inside the handle (s16x3: written
        straight as the layer-0 split-f16 image).  Returns feat_len [B] int32 (= frames // 3)."""
        fbank = fbank.contiguous()
        B, T, _ = fbank.shape
        flen = torch.empty(B, device=self.device, dtype=torch.int32)
        _lib.check(self.lib.casr_encode_fbank(self.handle, _ptr(fbank), _ptr(frames.to(torch.int32).contiguous()),
                                              B, T, ctypes.c_float(eps), _ptr(flen), _stream()), self.handle)
        self._B, self._Tp = B, T // 3
        self._lens = flen
        return flen

    def encoder_results(self):
        B, Tp, Cz = self._B, self._Tp, 2 * self.cfg.enc_hidden
        enc = torch.empty(B, Tp, Cz, device=self.device)
        h = torch.empty(B, Cz, device=self.device)
        c = torch.empty(B, Cz, device=self.device)
        keys = torch.empty(B, self.cfg.attn_size, Tp, device=self.device)
        _lib.check(self.lib.casr_encoder_results(self.handle, _ptr(enc), _ptr(h), _ptr(c), _ptr(keys),
                                                 _stream()), self.handle)
        return enc, h, c, keys

    # ------------------------------------------------------------------ decode
    def greedy(self, alignment=False):
        B, L = self._B, self.cfg.max_len
        dev = self.device
        tokens = torch.empty(B, L, dtype=torch.int32, device=dev)
        out_len = torch.empty(B, dtype=torch.int32, device=dev)
        fin = torch.empty(B, dtype=torch.uint8, device=dev)
        accum = torch.empty(B, dtype=torch.float32, device=dev)
        align = torch.zeros(L, self._Tp, B, device=dev) if alignment else None
        _lib.check(self.lib.casr_greedy(self.handle, _ptr(tokens), _ptr(out_len), _ptr(fin), _ptr(accum),
                                        _ptr(align), _stream()), self.handle)
        return dict(tokens=tokens, out_len=out_len, finished=fin, accum=accum, alignment=align)

    def beam(self, k, lm_weight=0.0, length_weight=0.0):
        B, L = self._B, self.cfg.max_len
        dev = self.device
        toks = torch.empty(B, L, dtype=torch.int32, device=dev)
        blen = torch.empty(B, dtype=torch.int32, device=dev)
        score = torch.empty(B, dtype=torch.float32, device=dev)
        steps = torch.empty(1, dtype=torch.int32, device=dev)
        _lib.check(self.lib.casr_beam(self.handle, int(k), ctypes.c_float(lm_weight), ctypes.c_float(length_weight),
                                      _ptr(toks), _ptr(blen), _ptr(score), _ptr(steps), _stream()), self.handle)
        self._k = k
        return dict(tokens=toks, length=blen, score=score, steps=steps)

    def beam_records(self):
        B, L, k = self._B, self.cfg.max_len, self._k
        dev = self.device
        rt = torch.empty(B, L, k, L, dtype=torch.int32, device=dev)
        rs = torch.empty(B, L, k, dtype=torch.float32, device=dev)
        rv = torch.empty(B, L, k, dtype=torch.uint8, device=dev)
        _lib.check(self.lib.casr_beam_records(self.handle, _ptr(rt), _ptr(rs), _ptr(rv), _stream()), self.handle)
        return rt, rs, rv

    def lm_score(self, lm, tokens, lens, bos=True):
        """Sentence scores of an n-gram LM on the device (casr_lm_score): lm a casr.ngram.NgramLM,
        tokens [n, L] LM ids, lens [n] -> q [n] float32, the bits NgramLM.score_ids gives on the host."""
        dev = self.device
        tokens = torch.as_tensor(tokens).to(dev, torch.int32).contiguous()
        lens = torch.as_tensor(lens).to(dev, torch.int32).contiguous()
        if tokens.dim() != 2 or lens.shape != (tokens.shape[0],):
            raise ValueError("lm_score: tokens must be [n, L] and lens [n]")
        n, L = tokens.shape
        q = torch.empty(n, dtype=torch.float32, device=dev)
        _lib.check(self.lib.casr_lm_score(self.handle, lm.on(self), _ptr(tokens), _ptr(lens), n, L, int(bool(bos)),
                                          _ptr(q), _stream()), self.handle)
        self._keep_lm = (lm, tokens, lens)  # read by the enqueued kernel
        return q

    def lm_estimate(self, tokens, offsets, order):
        """An interpolated modified-Kneser-Ney n-gram model of the flat corpus on the device
        (casr_lm_estimate; include/casr.h has the definition): tokens [total] LM ids, offsets [n + 1]
        ascending from 0 -> casr.ngram.LmEstimate, whose counts and float64 p and gamma are the host
        entry's bit for bit (the order within an order is unspecified: ``.sorted()``).  A bad id is
        counted as <unk> and a descending offset clamped, both raising guard bit 1.  Needs no weights
        and no encode; synchronous."""
        from .ngram import LmEstimate
        dev = self.device
        tokens = torch.as_tensor(tokens).to(dev, torch.int32).contiguous().reshape(-1)
        offsets = torch.as_tensor(offsets).to(dev, torch.int64).contiguous().reshape(-1)
        if tokens.numel() == 0:
            tokens = torch.zeros(1, dtype=torch.int32, device=dev)  # (a pointer to pass; never read)
        out = ctypes.c_void_p()
        _lib.check(self.lib.casr_lm_estimate(self.handle, int(order), _ptr(tokens), _ptr(offsets),
                                             offsets.numel() - 1, _stream(), ctypes.byref(out)), self.handle)
        return LmEstimate(self.lib, out, order)

    def lm_prune(self, lm, theta):
        """Relative-entropy pruning of a casr.ngram.NgramLM on the device (casr_lm_prune; include/casr.h
        has the definition) -> casr.ngram.LmPruned, whose decisions, float64 backoffs and stored
        values are the host entry's bit for bit (the order within an order is unspecified:
        ``.sorted()``).  Needs no weights and no encode; synchronous.  NgramLM.prune(theta, engine)
        builds the pruned model from it."""
        from .ngram import LmPruned
        out = ctypes.c_void_p()
        _lib.check(self.lib.casr_lm_prune(self.handle, lm.on(self), ctypes.c_double(theta), _stream(),
                                          ctypes.byref(out)), self.handle)
        return LmPruned(self.lib, out, lm.order)

    def beam_rescore(self, lm, lm_weight, length_weight, records=False):
        """The second pass (model.py:749-763) over the last beam()'s finished hypotheses on the device
        (casr_beam_rescore): lm a casr.ngram.NgramLM.  Returns tokens [B, max_len] (-1 past the
        length), length [B], score [B] (the chosen record's first-pass score), lm [B] (its LM score;
        0 where the utterance had no record and keeps beam()'s fallback), and with ``records`` rec_lm
        [B, max_len, k], the LM score of every valid record."""
        B, L, k = self._B, self.cfg.max_len, self._k
        dev = self.device
        toks = torch.empty(B, L, dtype=torch.int32, device=dev)
        blen = torch.empty(B, dtype=torch.int32, device=dev)
        score = torch.empty(B, dtype=torch.float32, device=dev)
        best_lm = torch.empty(B, dtype=torch.float32, device=dev)
        rec_lm = torch.empty(B, L, k, dtype=torch.float32, device=dev) if records else None
        _lib.check(self.lib.casr_beam_rescore(self.handle, lm.on(self), ctypes.c_double(lm_weight),
                                              ctypes.c_double(length_weight), _ptr(toks), _ptr(blen), _ptr(score),
                                              _ptr(best_lm), _ptr(rec_lm), _stream()), self.handle)
        self._keep_lm = (lm,)
        return dict(tokens=toks, length=blen, score=score, lm=best_lm, rec_lm=rec_lm)

    def lm_terms(self, lm, ctx, nc, eos=None):
        """Term rows of an n-gram LM on the device (casr_lm_terms): ctx [n, 3] LM ids (nearest
        predecessor first), nc [n] -> terms [n, V] float32, the bits NgramLM.terms gives on the host."""
        dev = self.device
        ctx = torch.as_tensor(ctx).to(dev, torch.int32).contiguous()
        nc = torch.as_tensor(nc).to(dev, torch.int32).contiguous()
        if ctx.dim() != 2 or ctx.shape[1] != 3 or nc.shape != (ctx.shape[0],):
            raise ValueError("lm_terms: ctx must be [n, 3] and nc [n]")
        n = ctx.shape[0]
        terms = torch.empty(n, self.cfg.vocab, dtype=torch.float32, device=dev)
        _lib.check(self.lib.casr_lm_terms(self.handle, lm.on(self), _ptr(ctx), _ptr(nc), n,
                                          -1 if eos is None else int(eos), _ptr(terms), _stream()), self.handle)
        self._keep_lm = (lm, ctx, nc)  # read by the enqueued kernel
        return terms

    def beam_lm(self, lm, k, lm_weight, length_weight):
        """Beam search with the n-gram LM fused into the first pass (casr_beam_lm): lm a
        casr.ngram.NgramLM.  Returns tokens [B, max_len] (-1 past the length), length [B], score [B]
        (the choice's acoustic log-probability), lm [B] (its LM score) and steps [1]."""
        B, L = self._B, self.cfg.max_len
        dev = self.device
        toks = torch.empty(B, L, dtype=torch.int32, device=dev)
        blen = torch.empty(B, dtype=torch.int32, device=dev)
        score = torch.empty(B, dtype=torch.float32, device=dev)
        best_lm = torch.empty(B, dtype=torch.float32, device=dev)
        steps = torch.empty(1, dtype=torch.int32, device=dev)
        _lib.check(self.lib.casr_beam_lm(self.handle, lm.on(self), int(k), ctypes.c_float(lm_weight),
                                         ctypes.c_float(length_weight), _ptr(toks), _ptr(blen), _ptr(score),
                                         _ptr(best_lm), _ptr(steps), _stream()), self.handle)
        self._k = k
        self._keep_lm = (lm,)
        return dict(tokens=toks, length=blen, score=score, lm=best_lm, steps=steps)

    def beam_record_lm(self):
        """rec_lm [B, max_len, k]: the LM score of every valid record of the last beam_lm() (0
        elsewhere), beside beam_records()' tokens and acoustic scores."""
        B, L, k = self._B, self.cfg.max_len, self._k
        rec_lm = torch.empty(B, L, k, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.casr_beam_record_lm(self.handle, _ptr(rec_lm), _stream()), self.handle)
        return rec_lm

    def bias_score(self, bias, tokens, lens):
        """(full, tail, state) int32 [n] of the rows tokens [n, L] (1 <= L <= 512) with lens [n] under a
        casr.bias.PhraseBias, on the device (casr_bias_score): PhraseBias.score_ids' values."""
        dev = self.device
        tokens = torch.as_tensor(tokens).to(dev, torch.int32).contiguous()
        lens = torch.as_tensor(lens).to(dev, torch.int32).contiguous()
        if tokens.dim() != 2 or lens.shape != (tokens.shape[0],):
            raise ValueError("bias_score: tokens must be [n, L] and lens [n]")
        n, L = tokens.shape
        full, tail, state = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
        _lib.check(self.lib.casr_bias_score(self.handle, bias.on(self), _ptr(tokens), _ptr(lens), n, L, _ptr(full),
                                            _ptr(tail), _ptr(state), _stream()), self.handle)
        self._keep_bias = (bias, tokens, lens)  # read by the enqueued kernel
        return full, tail, state

    def bias_rows(self, bias, state, next=False):
        """gain int32 [n, V] of automaton states [n] on the device (casr_bias_rows), and with ``next``
        the successor states [n, V]: PhraseBias.rows' values."""
        dev = self.device
        state = torch.as_tensor(state).to(dev, torch.int32).contiguous().reshape(-1)
        n = state.shape[0]
        gain = torch.empty(n, self.cfg.vocab, dtype=torch.int32, device=dev)
        nx = torch.empty(n, self.cfg.vocab, dtype=torch.int32, device=dev) if next else None
        _lib.check(self.lib.casr_bias_rows(self.handle, bias.on(self), _ptr(state), n, _ptr(gain), _ptr(nx),
                                           _stream()), self.handle)
        self._keep_bias = (bias, state)  # read by the enqueued kernel
        return (gain, nx) if next else gain

    def beam_bias(self, bias, k, bias_weight=1.0, lm=None, lm_weight=0.0, length_weight=0.0):
        """Beam search with the phrase bias (a casr.bias.PhraseBias) and, with ``lm`` (a
        casr.ngram.NgramLM), the n-gram LM in the first pass (casr_beam_bias).  Returns tokens [B,
        max_len] (-1 past the length), length [B], score [B] (the choice's acoustic log-probability),
        lm [B] (its LM score; None without an LM), bias [B] (its bias in nats) and steps [1]."""
        B, L = self._B, self.cfg.max_len
        dev = self.device
        toks = torch.empty(B, L, dtype=torch.int32, device=dev)
        blen = torch.empty(B, dtype=torch.int32, device=dev)
        score = torch.empty(B, dtype=torch.float32, device=dev)
        best_lm = torch.empty(B, dtype=torch.float32, device=dev) if lm is not None else None
        best_bias = torch.empty(B, dtype=torch.float32, device=dev)
        steps = torch.empty(1, dtype=torch.int32, device=dev)
        _lib.check(self.lib.casr_beam_bias(self.handle, bias.on(self), lm.on(self) if lm is not None else None, int(k),
                                           ctypes.c_float(bias_weight), ctypes.c_float(lm_weight),
                                           ctypes.c_float(length_weight), _ptr(toks), _ptr(blen), _ptr(score),
                                           _ptr(best_lm), _ptr(best_bias), _ptr(steps), _stream()), self.handle)
        self._k = k
        self._keep_lm = (lm, bias)
        return dict(tokens=toks, length=blen, score=score, lm=best_lm, bias=best_bias, steps=steps)

    def beam_record_bias(self):
        """rec_bias [B, max_len, k]: bias_closed (nats) of every valid record of the last beam_bias() (0
        elsewhere), beside beam_records()' tokens and acoustic scores."""
        B, L, k = self._B, self.cfg.max_len, self._k
        rec_bias = torch.empty(B, L, k, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.casr_beam_record_bias(self.handle, _ptr(rec_bias), _stream()), self.handle)
        return rec_bias

    def grammar_accept(self, grammar, tokens, lens):
        """(consumed, state, accepted) [n] of the rows tokens [n, L] (1 <= L <= 512) with lens [n] under a
        casr.grammar.Grammar, on the device (casr_grammar_accept): Grammar.walk's values."""
        dev = self.device
        tokens = torch.as_tensor(tokens).to(dev, torch.int32).contiguous()
        lens = torch.as_tensor(lens).to(dev, torch.int32).contiguous()
        if tokens.dim() != 2 or lens.shape != (tokens.shape[0],):
            raise ValueError("grammar_accept: tokens must be [n, L] and lens [n]")
        n, L = tokens.shape
        consumed, state = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
        ok = torch.empty(n, dtype=torch.uint8, device=dev)
        _lib.check(self.lib.casr_grammar_accept(self.handle, grammar.on(self), _ptr(tokens), _ptr(lens), n, L,
                                                _ptr(consumed), _ptr(state), _ptr(ok), _stream()), self.handle)
        self._keep_grammar = (grammar, tokens, lens)  # read by the enqueued kernel
        return consumed, state, ok

    def grammar_rows(self, grammar, state, budget):
        """mask int32 [n, mask_words] (the uint32 words' bits) of grammar states [n] under budgets [n] on
        the device (casr_grammar_rows): Grammar.rows' values."""
        dev = self.device
        state = torch.as_tensor(state).to(dev, torch.int32).contiguous().reshape(-1)
        n = state.shape[0]
        budget = torch.as_tensor(budget).to(dev, torch.int32).broadcast_to(state.shape).contiguous()
        mask = torch.empty(n, grammar.mask_words, dtype=torch.int32, device=dev)
        _lib.check(self.lib.casr_grammar_rows(self.handle, grammar.on(self), _ptr(state), _ptr(budget), n,
                                              _ptr(mask), _stream()), self.handle)
        self._keep_grammar = (grammar, state, budget)  # read by the enqueued kernel
        return mask

    def beam_grammar(self, grammar, k, lm=None, lm_weight=0.0, length_weight=0.0, start=None):
        """Beam search over the sentences of a casr.grammar.Grammar and, with ``lm`` (a
        casr.ngram.NgramLM), the n-gram LM in the first pass (casr_beam_grammar).  ``start`` [B]: the
        grammar state each utterance starts in (None: state 0; Grammar.union gives the states).  Returns
        tokens [B, max_len] (-1 past the length), length [B], score [B] (the choice's acoustic
        log-probability), lm [B] (its LM score; None without an LM), complete [B] (1 where the choice is
        a finished sentence of the grammar) and steps [1]."""
        B, L = self._B, self.cfg.max_len
        dev = self.device
        if start is not None:
            start = torch.as_tensor(start).to(dev, torch.int32).contiguous().reshape(-1)
            if start.shape[0] != B:
                raise ValueError(f"beam_grammar: start must be [{B}]")
        toks = torch.empty(B, L, dtype=torch.int32, device=dev)
        blen = torch.empty(B, dtype=torch.int32, device=dev)
        score = torch.empty(B, dtype=torch.float32, device=dev)
        best_lm = torch.empty(B, dtype=torch.float32, device=dev) if lm is not None else None
        complete = torch.empty(B, dtype=torch.uint8, device=dev)
        steps = torch.empty(1, dtype=torch.int32, device=dev)
        _lib.check(self.lib.casr_beam_grammar(self.handle, grammar.on(self), lm.on(self) if lm is not None else None,
                                              _ptr(start), int(k), ctypes.c_float(lm_weight),
                                              ctypes.c_float(length_weight), _ptr(toks), _ptr(blen), _ptr(score),
                                              _ptr(best_lm), _ptr(complete), _ptr(steps), _stream()), self.handle)
        self._k = k
        self._keep_lm = (lm, grammar, start)
        return dict(tokens=toks, length=blen, score=score, lm=best_lm, complete=complete, steps=steps)

    def edit_distance(self, a, a_len, b, b_len, ops=False):
        """Edit distances of n pairs on the device (casr_edit_distance): a [n, La], b [n, Lb] int32
        symbols (1 <= La, Lb <= casr.lib.EDIT_MAX_LEN), a_len and b_len [n] -> dist [n] int32, and with
        ``ops`` the (insert, delete, replace) counts [n, 3] of the script turning a into b; the values
        casr.lib.edit_distance_host gives.  Needs no weights and no encode; returns after enqueueing."""
        dev = self.device
        a = torch.as_tensor(a).to(dev, torch.int32).contiguous()
        b = torch.as_tensor(b).to(dev, torch.int32).contiguous()
        if a.dim() != 2 or b.dim() != 2 or a.shape[0] != b.shape[0]:
            raise ValueError("edit_distance: a must be [n, La] and b [n, Lb]")
        n = a.shape[0]
        a_len = torch.as_tensor(a_len).to(dev, torch.int32).contiguous()
        b_len = torch.as_tensor(b_len).to(dev, torch.int32).contiguous()
        if a_len.shape != (n,) or b_len.shape != (n,):
            raise ValueError(f"edit_distance: a_len and b_len must be [n={n}]")
        dist = torch.empty(n, dtype=torch.int32, device=dev)
        counts = torch.empty(n, 3, dtype=torch.int32, device=dev) if ops else None
        _lib.check(self.lib.casr_edit_distance(self.handle, _ptr(a), _ptr(a_len), int(a.shape[1]), _ptr(b), _ptr(b_len),
                                               int(b.shape[1]), n, _ptr(dist), _ptr(counts), _stream()), self.handle)
        self._keep_edit = (a, a_len, b, b_len)  # read by the enqueued kernel
        return (dist, counts) if ops else dist

    def edit_align(self, a, a_len, b, b_len, ops=True, maps=True):
        """The edit script of n long pairs on the device (casr_edit_align): a [n, La], b [n, Lb] int32
        symbols (1 <= La, Lb <= casr.lib.EDIT_ALIGN_MAX_LEN), a_len and b_len [n] -> dict of dist [n],
        and with ``ops`` the counts ops [n, 3], with ``maps`` b_of_a [n, La] and a_of_b [n, Lb] (-1: no
        partner); the values casr.lib.edit_align_host gives.  Needs no weights and no encode, leaves
        the last encode and beam as they are; returns after enqueueing."""
        dev = self.device
        a = torch.as_tensor(a).to(dev, torch.int32).contiguous()
        b = torch.as_tensor(b).to(dev, torch.int32).contiguous()
        if a.dim() != 2 or b.dim() != 2 or a.shape[0] != b.shape[0]:
            raise ValueError("edit_align: a must be [n, La] and b [n, Lb]")
        n = a.shape[0]
        a_len = torch.as_tensor(a_len).to(dev, torch.int32).contiguous()
        b_len = torch.as_tensor(b_len).to(dev, torch.int32).contiguous()
        if a_len.shape != (n,) or b_len.shape != (n,):
            raise ValueError(f"edit_align: a_len and b_len must be [n={n}]")
        dist = torch.empty(n, dtype=torch.int32, device=dev)
        counts = torch.empty(n, 3, dtype=torch.int32, device=dev) if ops else None
        b_of_a = torch.empty(a.shape, dtype=torch.int32, device=dev) if maps else None
        a_of_b = torch.empty(b.shape, dtype=torch.int32, device=dev) if maps else None
        _lib.check(self.lib.casr_edit_align(self.handle, _ptr(a), _ptr(a_len), int(a.shape[1]), _ptr(b), _ptr(b_len),
                                            int(b.shape[1]), n, _ptr(dist), _ptr(counts), _ptr(b_of_a), _ptr(a_of_b),
                                            _stream()), self.handle)
        self._keep_edit_align = (a, a_len, b, b_len)  # read by the enqueued kernels
        return dict(dist=dist, ops=counts, b_of_a=b_of_a, a_of_b=a_of_b)

    def edit_align_workspace_bytes(self):
        """Bytes of casr_edit_align's workspace this engine's handle holds now."""
        return int(self.lib.casr_edit_align_workspace_bytes(self.handle))

    def beam_mbr(self, scale, lm=None, lm_weight=0.0, length_weight=0.0, records=False):
        """The minimum-Bayes-risk choice over the last beam()'s finished hypotheses on the device
        (casr_beam_mbr): per utterance the record with the lowest expected edit distance to the
        others under the posterior exp(scale (c - c_max)), c the second pass's combined score.  With
        ``lm`` (a casr.ngram.NgramLM) the rescore runs first for the records' LM scores.  Returns
        tokens [B, max_len] (-1 past the length), length [B], score [B] (the choice's first-pass
        score), index [B] (step k + rank, -1 where the utterance had no record and keeps beam()'s
        fallback), risk [B] float64, and with ``records`` rec_risk [B, max_len, k]."""
        B, L, k = self._B, self.cfg.max_len, self._k
        dev = self.device
        rec_lm = None
        if lm is not None:
            rec_lm = self.beam_rescore(lm, lm_weight, length_weight, records=True)["rec_lm"]
        toks = torch.empty(B, L, dtype=torch.int32, device=dev)
        blen = torch.empty(B, dtype=torch.int32, device=dev)
        score = torch.empty(B, dtype=torch.float32, device=dev)
        index = torch.empty(B, dtype=torch.int32, device=dev)
        risk = torch.empty(B, dtype=torch.float64, device=dev)
        rec_risk = torch.empty(B, L, k, dtype=torch.float64, device=dev) if records else None
        _lib.check(self.lib.casr_beam_mbr(self.handle, float(scale), _ptr(rec_lm), float(lm_weight if lm is not None else 0.0),
                                          float(length_weight), _ptr(toks), _ptr(blen), _ptr(score), _ptr(index),
                                          _ptr(risk), _ptr(rec_risk), _stream()), self.handle)
        self._keep_mbr = (rec_lm,)  # read by the enqueued kernels
        return dict(tokens=toks, length=blen, score=score, index=index, risk=risk, rec_risk=rec_risk, rec_lm=rec_lm)

    def beam_mbr_distances(self):
        """The distances of the last beam_mbr() (casr_beam_mbr_distances): dist [B, max_len k, max_len k]
        uint8 over each utterance's valid records in (step, rank) order, and their counts [B]."""
        B, LK = self._B, self.cfg.max_len * self._k
        dist = torch.empty(B, LK, LK, dtype=torch.uint8, device=self.device)
        n_rec = torch.empty(B, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.casr_beam_mbr_distances(self.handle, _ptr(dist), _ptr(n_rec), _stream()), self.handle)
        return dist, n_rec

    def beam_nbest(self, N, lm=None, lm_weight=0.0, length_weight=0.0, rec_lm=None):
        """The N best finished hypotheses of the last beam() by the second pass's combined score c, on the
        device (casr_beam_nbest).  With ``lm`` (a casr.ngram.NgramLM) the rescore runs first for the records'
        LM scores; ``rec_lm`` hands in the array an earlier rescore returned instead.  Returns index [B, N]
        (step k + rank, -1 past the record count), tokens [B, N, max_len] (-1 past each length), length
        [B, N] and comb [B, N] float64."""
        B, L = self._B, self.cfg.max_len
        dev = self.device
        if lm is not None and rec_lm is None:
            rec_lm = self.beam_rescore(lm, lm_weight, length_weight, records=True)["rec_lm"]
        N = int(N)
        index = torch.empty(B, max(N, 0), dtype=torch.int32, device=dev)
        toks = torch.empty(B, max(N, 0), L, dtype=torch.int32, device=dev)
        ln = torch.empty(B, max(N, 0), dtype=torch.int32, device=dev)
        comb = torch.empty(B, max(N, 0), dtype=torch.float64, device=dev)
        _lib.check(self.lib.casr_beam_nbest(self.handle, N, _ptr(rec_lm), float(lm_weight if rec_lm is not None else 0.0),
                                            float(length_weight), _ptr(index), _ptr(toks), _ptr(ln), _ptr(comb),
                                            _stream()), self.handle)
        self._keep_nbest = (rec_lm,)  # read by the enqueued kernel
        return dict(index=index, tokens=toks, length=ln, comb=comb, rec_lm=rec_lm)

    def beam_confusion(self, M=4, scale=1.0, lm=None, lm_weight=0.0, length_weight=0.0, pivot=None, rec_lm=None,
                       units=False):
        """The confusion network of the last beam()'s finished hypotheses around a pivot, on the device
        (casr_beam_confusion): per slot of the pivot (odd: its characters, even: the gaps) the M tokens with
        the largest posterior mass under exp(scale (c - c_max)) in units of 2^-32.  ``pivot`` [B] flat
        indices step k + rank (None: the record with the largest c; -1: none).  LM arguments as
        beam_nbest.  Returns n_slots [B], slot_token [B, 2 max_len + 1, M] (casr.lib.CN_EPS = -1 nothing,
        CN_NONE = -2 unused), slot_mass of the same shape int64, pivot_mass [B, max_len] int64, total [B]
        int64, and with ``units`` rec_unit [B, max_len, k] int64."""
        B, L, k = self._B, self.cfg.max_len, self._k
        dev = self.device
        if lm is not None and rec_lm is None:
            rec_lm = self.beam_rescore(lm, lm_weight, length_weight, records=True)["rec_lm"]
        if pivot is not None:
            pivot = torch.as_tensor(pivot).to(dev, torch.int32).contiguous()
            if pivot.shape != (B,):
                raise ValueError(f"beam_confusion: pivot must be [B={B}]")
        M = int(M)
        n_slots = torch.empty(B, dtype=torch.int32, device=dev)
        st = torch.empty(B, 2 * L + 1, max(M, 0), dtype=torch.int32, device=dev)
        sm = torch.empty(B, 2 * L + 1, max(M, 0), dtype=torch.int64, device=dev)
        pm = torch.empty(B, L, dtype=torch.int64, device=dev)
        total = torch.empty(B, dtype=torch.int64, device=dev)
        ru = torch.empty(B, L, k, dtype=torch.int64, device=dev) if units else None
        _lib.check(self.lib.casr_beam_confusion(self.handle, M, float(scale), _ptr(rec_lm),
                                                float(lm_weight if rec_lm is not None else 0.0), float(length_weight),
                                                _ptr(pivot), _ptr(n_slots), _ptr(st), _ptr(sm), _ptr(pm), _ptr(total),
                                                _ptr(ru), _stream()), self.handle)
        self._keep_cn = (rec_lm, pivot)  # read by the enqueued kernels
        return dict(n_slots=n_slots, slot_token=st, slot_mass=sm, pivot_mass=pm, total=total, rec_unit=ru,
                    rec_lm=rec_lm)

    def confusion(self, rec_tokens, rec_valid, rec_unit, pivot, vocab, M=4):
        """casr.lib.confusion_host's operation on the device (casr_confusion): rec_tokens [B, L, k, L]
        int32, rec_valid [B, L, k], rec_unit [B, L, k] int64, pivot [B] -> the same dict, of device tensors,
        value for value.  L <= 255, k <= 16.  Needs no weights and no encode; returns after enqueueing."""
        dev = self.device
        rt = torch.as_tensor(rec_tokens).to(dev, torch.int32).contiguous()
        if rt.dim() != 4 or rt.shape[1] != rt.shape[3]:
            raise ValueError("confusion: rec_tokens must be [B, L, k, L]")
        B, L, k = rt.shape[:3]
        rv = torch.as_tensor(rec_valid).to(dev, torch.uint8).contiguous()
        ru = torch.as_tensor(rec_unit).to(dev, torch.int64).contiguous()
        pv = torch.as_tensor(pivot).to(dev, torch.int32).contiguous()
        if rv.shape != (B, L, k) or ru.shape != (B, L, k) or pv.shape != (B,):
            raise ValueError("confusion: rec_valid and rec_unit must be [B, L, k] and pivot [B]")
        M = int(M)
        n_slots = torch.empty(B, dtype=torch.int32, device=dev)
        st = torch.empty(B, 2 * L + 1, max(M, 0), dtype=torch.int32, device=dev)
        sm = torch.empty(B, 2 * L + 1, max(M, 0), dtype=torch.int64, device=dev)
        pm = torch.empty(B, L, dtype=torch.int64, device=dev)
        total = torch.empty(B, dtype=torch.int64, device=dev)
        _lib.check(self.lib.casr_confusion(self.handle, _ptr(rt), _ptr(rv), _ptr(ru), _ptr(pv), B, L, k, int(vocab), M,
                                           _ptr(n_slots), _ptr(st), _ptr(sm), _ptr(pm), _ptr(total), _stream()),
                   self.handle)
        self._keep_cn = (rt, rv, ru, pv)  # read by the enqueued kernels
        return dict(n_slots=n_slots, slot_token=st, slot_mass=sm, pivot_mass=pm, total=total)

    def score(self, targets, tgt_len, alignment=False, best=False, mean=False):
        """Teacher-forced pass over the last encode (casr_score): targets [B, L] int (1 <= L <=
        max_len), tgt_len [B] scored positions per utterance.  Returns token_logp [B, L] (0 past
        tgt_len), total_logp [B], and on request best_token / best_logp [B, L], mean_logp [B, L]
        (the label-smoothing term) and alignment [L, Tp, B].  Like greedy / beam it is the decode
        half of run_checked (flag 32 raises, flag 128 re-runs at f32)."""
        dev = self.device
        targets = torch.as_tensor(targets).to(dev, torch.int32).contiguous()
        tgt_len = torch.as_tensor(tgt_len).to(dev, torch.int32).contiguous()
        if targets.dim() != 2 or targets.shape[0] != self._B or tgt_len.shape != (self._B,):
            raise ValueError(f"score: targets must be [B={self._B}, L] and tgt_len [B]")
        B, L = targets.shape
        token_logp = torch.empty(B, L, dtype=torch.float32, device=dev)
        total = torch.empty(B, dtype=torch.float32, device=dev)
        best_token = torch.empty(B, L, dtype=torch.int32, device=dev) if best else None
        best_logp = torch.empty(B, L, dtype=torch.float32, device=dev) if best else None
        mean_logp = torch.empty(B, L, dtype=torch.float32, device=dev) if mean else None
        align = torch.zeros(L, self._Tp, B, device=dev) if alignment else None
        _lib.check(self.lib.casr_score(self.handle, _ptr(targets), _ptr(tgt_len), int(L), _ptr(token_logp), _ptr(total),
                                       _ptr(best_token), _ptr(best_logp), _ptr(mean_logp), _ptr(align), _stream()),
                   self.handle)
        self._keep_score = (targets, tgt_len)  # read by the enqueued kernels
        return dict(token_logp=token_logp, total_logp=total, best_token=best_token, best_logp=best_logp,
                    mean_logp=mean_logp, alignment=align, tgt_len=tgt_len)

    def align_path(self, align, enc_len, tgt_len):
        """The best monotone path through attention weights on the device (casr_align_path): align
        [L, Tp, B] float32 as greedy(alignment=True) and score(alignment=True) return it (Tp at most
        casr.lib.ALIGN_MAX_TP), enc_len [B] encoder frames and tgt_len [B] scored positions -> dict of
        device tensors first, last, peak [B, L] int32 (-1 past tgt_len) and path_score [B] int32: the
        values casr.lib.align_path_host gives.  Needs no weights and no encode; returns after enqueueing."""
        dev = self.device
        align = torch.as_tensor(align).to(dev, torch.float32).contiguous()
        if align.dim() != 3:
            raise ValueError("align_path: align must be [L, Tp, B]")
        L, Tp, B = align.shape
        enc_len = torch.as_tensor(enc_len).to(dev, torch.int32).contiguous()
        tgt_len = torch.as_tensor(tgt_len).to(dev, torch.int32).contiguous()
        if enc_len.shape != (B,) or tgt_len.shape != (B,):
            raise ValueError(f"align_path: enc_len and tgt_len must be [B={B}]")
        first, last, peak = (torch.empty(B, L, dtype=torch.int32, device=dev) for _ in range(3))
        score = torch.empty(B, dtype=torch.int32, device=dev)
        _lib.check(self.lib.casr_align_path(self.handle, _ptr(align), _ptr(enc_len), _ptr(tgt_len), B, Tp, L,
                                            _ptr(first), _ptr(last), _ptr(peak), _ptr(score), _stream()), self.handle)
        self._keep_align = (align, enc_len, tgt_len)  # read by the enqueued kernel
        return dict(first=first, last=last, peak=peak, path_score=score)

    def device_flags(self):
        """Guard bits raised since the previous read (read and clear: every encode / decode in
        between is covered; 0 = clean); synchronises the stream."""
        f = ctypes.c_int32()
        _lib.check(self.lib.casr_device_flags(self.handle, ctypes.byref(f), _stream()), self.handle)
        return f.value

    def set_graphs(self, enable):
        """hipGraph replay of the launch-bound loops: True = decode loop and per-step recurrence
        fallback, False = both eager, or an int mode (include/casr.h CASR_GRAPHS_*; default 2:
        decode eager, recurrence fallback replayed)."""
        mode = (3 if enable else 0) if isinstance(enable, bool) else int(enable)
        _lib.check(self.lib.casr_set_graphs(self.handle, mode), self.handle)

    def set_persistent(self, enable):
        """Persistent per-layer recurrence (default on where its grid fits); off = per-step."""
        _lib.check(self.lib.casr_set_persistent(self.handle, int(bool(enable))), self.handle)

    def set_precision(self, precision):
        """'s16x3' (default: split-f16 MFMA, f32 accumulate) or 'f32' (exact-f32 MFMA); an
        Engine(arithmetic='s16x1') takes 's16x1' or 'f32'."""
        _lib.check(self.lib.casr_set_precision(self.handle, _lib.PRECISIONS[precision]), self.handle)
        self.requested = precision

    def check_flags(self):
        """Guard bits raised since the previous read (read and clear, casr_device_flags: every
        encode / decode since then is covered; synchronises).  Raises CasrError when a recurrence
        hand-off timed out (bit 32: those encoder results are invalid); returns the bits
        otherwise, so a caller can re-run at f32 on bit 128 (FLAG_F16_RANGE)."""
        f = self.device_flags()
        if f & FLAG_REC_TIMEOUT:
            raise _lib.CasrError("persistent recurrence hand-off wait expired (device flag 32): "
                                 "the encoder results of this batch are invalid")
        return f

    def run_checked(self, encode, decode):
        """encode(); out = decode(); then the guard bits.  Bit 32 raises; bit 128 (an s16x3
        operand beyond the f16 range) re-runs encode + decode on the exact-f32 path, so no
        result rests on a wrong split image.  Bits left by earlier unchecked calls are read and
        discarded first, so only this batch's bits decide."""
        self.device_flags()
        encode()
        out = decode()
        f = self.check_flags()
        if f & FLAG_F16_RANGE and self.precision() in ("s16x3", "s16x1"):
            req = self.requested
            self.set_precision("f32")
            try:
                encode()
                out = decode()
                f = self.check_flags()
            finally:
                self.set_precision(req)
        return out, f

    def set_option(self, name, value):
        """Tuning option (include/casr.h CASR_OPT_*, lib.OPTIONS): speed only, same bits, except the
        numerics variants ATTN_DIRECT, DEC_FOLD and DEC_KSPLIT (same tokens, results within tolerance)."""
        _lib.check(self.lib.casr_set_option(self.handle, _lib.OPTIONS[name], int(value)), self.handle)

    def get_option(self, name):
        v = ctypes.c_int32()
        _lib.check(self.lib.casr_get_option(self.handle, _lib.OPTIONS[name], ctypes.byref(v)), self.handle)
        return v.value

    def precision(self):
        """Effective arithmetic of the MFMA contractions ('s16x3', 's16x1' or 'f32')."""
        p = int(self.lib.casr_get_precision(self.handle))
        return {v: k for k, v in _lib.PRECISIONS.items()}[p]

    def recurrence_mode(self, B):
        """1 if casr_encode would run the persistent recurrence for batch B, else 0."""
        return int(self.lib.casr_recurrence_mode(self.handle, int(B)))

    # ------------------------------------------------------------------ launch timing
    def profile(self, classes):
        """Enable HIP-event timing for the named kernel classes (lib.KERNEL_CLASSES)."""
        mask = 0
        for c in classes:
            mask |= 1 << _lib.KERNEL_CLASSES.index(c)
        _lib.check(self.lib.casr_profile_enable(self.handle, mask), self.handle)

    def profile_read(self):
        """{class: (launches, total_ms)} for the enabled classes since profile()."""
        out = {}
        for i, name in enumerate(_lib.KERNEL_CLASSES):
            n = ctypes.c_int32()
            ms = ctypes.c_double()
            _lib.check(self.lib.casr_profile_read(self.handle, i, ctypes.byref(n), ctypes.byref(ms)), self.handle)
            if n.value:
                out[name] = (n.value, ms.value)
        return out
