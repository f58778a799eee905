"""ctypes binding of the casr C ABI (include/casr.h).

There is no fallback: if ``libcasr_hip.so`` is missing or fails to load, every entry point
raises.  ``torch`` is imported first so the HIP runtime it ships (soname
libamdhip64.so.7) is the one the library binds to."""
import ctypes
import os

import numpy as np

from . import build as _build

CASR_MAX_LAYERS = 8
STATUS = {0: "CASR_OK", 1: "CASR_ERR_ARG", 2: "CASR_ERR_HIP", 3: "CASR_ERR_STATE",
          4: "CASR_ERR_UNSUPPORTED"}

# every symbol include/casr.h declares (tests check the library exports all of them)
EXPORTS = [
    "casr_api_version", "casr_packed_weights_floats", "casr_pack_weights", "casr_create",
    "casr_bind_weights", "casr_destroy", "casr_last_error", "casr_features",
    "casr_gather_utterances", "casr_encode", "casr_encode_fbank", "casr_encoder_results", "casr_greedy", "casr_beam",
    "casr_beam_records", "casr_profile_enable", "casr_profile_read", "casr_set_graphs",
    "casr_device_flags", "casr_set_persistent", "casr_recurrence_mode", "casr_log_mel",
    "casr_log_mel_frames", "casr_mel_filterbank", "casr_set_precision", "casr_get_precision",
    "casr_set_option", "casr_get_option", "casr_score",
    "casr_convert_audio", "casr_resample_plan", "casr_resample_filter", "casr_resample_frames",
    "casr_lm_create", "casr_lm_destroy", "casr_lm_score_host", "casr_lm_score", "casr_beam_rescore",
    "casr_lm_terms_host", "casr_lm_terms", "casr_beam_lm", "casr_beam_record_lm",
    "casr_segment_default_params", "casr_segment_bound", "casr_segment_host", "casr_segment",
    "casr_gather_segments",
    "casr_edit_align_host", "casr_edit_align_tiles_host", "casr_edit_align", "casr_edit_align_plan",
    "casr_edit_align_workspace_bytes",
    "casr_edit_distance_host", "casr_edit_distance", "casr_mbr_host", "casr_beam_mbr", "casr_beam_mbr_distances",
    "casr_bias_create", "casr_bias_destroy", "casr_bias_score_host", "casr_bias_score", "casr_bias_rows_host",
    "casr_bias_rows", "casr_beam_bias", "casr_beam_record_bias",
    "casr_grammar_create", "casr_grammar_destroy", "casr_grammar_info", "casr_grammar_mask_words",
    "casr_grammar_accept_host", "casr_grammar_accept", "casr_grammar_rows_host", "casr_grammar_rows",
    "casr_beam_grammar",
    "casr_align_path_host", "casr_align_path",
    "casr_posterior_units_host", "casr_nbest_host", "casr_confusion_host", "casr_confusion", "casr_beam_nbest",
    "casr_beam_confusion",
    "casr_lm_estimate_host", "casr_lm_estimate", "casr_lm_estimate_combine", "casr_lm_estimate_info",
    "casr_lm_estimate_arrays", "casr_lm_estimate_counts", "casr_lm_estimate_timing", "casr_lm_estimate_destroy",
    "casr_lm_estimate_workspace_bytes",
    "casr_lm_prune_host", "casr_lm_prune", "casr_lm_prune_info", "casr_lm_prune_arrays", "casr_lm_prune_decisions",
    "casr_lm_prune_timing", "casr_lm_prune_destroy", "casr_lm_prune_workspace_bytes",
]

# arithmetic of the MFMA contractions (casr_set_precision); s16x1 is the opt-in perf arithmetic of
# the libcasr_hip_s16x1.so build (build.py variant "s16x1"), which Engine(arithmetic="s16x1") loads
PRECISIONS = {"f32": 0, "s16x3": 1, "s16x1": 2}
VARIANT_OF = {"s16x3": None, "s16x1": "s16x1"}

# tuning options (include/casr.h CASR_OPT_*): speed only, every value gives the same bits, except
# ATTN_DIRECT (the direct tanh(k + q) attention scores) and DEC_FOLD (the folded decode step: two
# launches per step, greedy always, beam at R >= 1024 rows with the one-accumulator fused GEMM; the
# same arithmetic regrouped): numerics variants within tolerance, the same token ids.
# REC_COOP_REFUSE is for tests: layer n - 1's cooperative launch is treated as refused
OPTIONS = {"FUSE_SELECT": 0, "REC_LAYOUT": 1, "REC_STORE_PLAIN": 2, "REC_SLEEP": 3, "REC_POLL_GAP": 4,
           "REC_COOP": 5, "GEMM16_PERSIST": 6, "GEMM16_TAIL": 7, "ATTN_KPB": 8, "ATTN_DIRECT": 9,
           "DEC_FOLD": 10, "REC_COOP_REFUSE": 11, "DIAG_COLD": 12,
           "LOGMEL_Q16": 13, "KEYS_ROWS": 14, "X16_KM": 15, "DEC_KSPLIT": 16, "GEMM16_LEAN": 17,
           "ATTN_SPLIT": 18, "MBR_MAP": 19, "ALIGN_GROUP": 20}

# kernel classes of casr_profile_enable / casr_profile_read (include/casr.h)
KERNEL_CLASSES = ["features", "input_proj", "rec_step", "keys", "dec_lstm", "attention", "proj", "select"]


class CasrConfigC(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        "n_mels", "feat_dim", "enc_hidden", "enc_layers", "residual", "dec_hidden", "embed_dim",
        "attn_size", "vocab", "max_len", "sos", "eos")] + [("temperature", ctypes.c_float)]


_FP = ctypes.POINTER(ctypes.c_float)


class CasrWeightsHostC(ctypes.Structure):
    _fields_ = [
        ("enc_w_ih", (_FP * 2) * CASR_MAX_LAYERS),
        ("enc_w_hh", (_FP * 2) * CASR_MAX_LAYERS),
        ("enc_b_ih", (_FP * 2) * CASR_MAX_LAYERS),
        ("enc_b_hh", (_FP * 2) * CASR_MAX_LAYERS),
        ("embedding", _FP), ("dec_w_ih", _FP), ("dec_w_hh", _FP), ("dec_b_ih", _FP),
        ("dec_b_hh", _FP), ("proj_w", _FP), ("proj_b", _FP), ("attn_w_enc", _FP),
        ("attn_b", _FP), ("attn_w_hidden", _FP), ("attn_v", _FP),
    ]


class CasrError(RuntimeError):
    pass


_LIBS = {}     # variant -> loaded library
_HANDLES = {}  # casr handle address -> the library that created it (check() reads its error text)


def load(path=None, variant=None):
    """Load (building first if stale and a compiler is present) the HIP library: the shipped
    build, or variant "s16x1" (the opt-in perf arithmetic)."""
    key = path or variant
    if key in _LIBS:
        return _LIBS[key]
    import torch  # noqa: F401  (HIP runtime first)
    path = path or _build.lib_path(variant)
    if not os.path.exists(path) or _build.is_stale(variant):
        if os.path.exists(_build.HIPCC):
            _build.build(variant=variant)
        if not os.path.exists(path):
            raise CasrError(f"casr HIP library not found at {path}; run __graft_entry__.build()")
    lib = ctypes.CDLL(path)
    vp, i32, f32, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    sig = {
        "casr_api_version": (i32, []),
        "casr_packed_weights_floats": (sz, [ctypes.POINTER(CasrConfigC)]),
        "casr_pack_weights": (i32, [ctypes.POINTER(CasrConfigC), ctypes.POINTER(CasrWeightsHostC), vp]),
        "casr_create": (i32, [ctypes.POINTER(CasrConfigC), i32, ctypes.POINTER(vp)]),
        "casr_bind_weights": (i32, [vp, vp]),
        "casr_destroy": (None, [vp]),
        "casr_last_error": (ctypes.c_char_p, [vp]),
        "casr_features": (i32, [vp, vp, vp, i32, i32, f32, vp, vp, vp]),
        "casr_gather_utterances": (i32, [vp, vp, vp, i32, i32, vp, vp]),
        "casr_encode": (i32, [vp, vp, vp, i32, i32, vp]),
        "casr_encode_fbank": (i32, [vp, vp, vp, i32, i32, f32, vp, vp]),
        "casr_encoder_results": (i32, [vp, vp, vp, vp, vp, vp]),
        "casr_greedy": (i32, [vp, vp, vp, vp, vp, vp, vp]),
        "casr_beam": (i32, [vp, i32, f32, f32, vp, vp, vp, vp, vp]),
        "casr_beam_records": (i32, [vp, vp, vp, vp, vp]),
        "casr_score": (i32, [vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]),
        "casr_profile_enable": (i32, [vp, ctypes.c_uint32]),
        "casr_set_graphs": (i32, [vp, i32]),
        "casr_device_flags": (i32, [vp, ctypes.POINTER(ctypes.c_int32), vp]),
        "casr_set_persistent": (i32, [vp, i32]),
        "casr_recurrence_mode": (i32, [vp, i32]),
        "casr_set_precision": (i32, [vp, i32]),
        "casr_get_precision": (i32, [vp]),
        "casr_log_mel": (i32, [vp, vp, vp, i32, i32, i32, f32, vp, vp, vp]),
        "casr_log_mel_frames": (i32, [i32]),
        "casr_mel_filterbank": (i32, [i32, f32, f32, i32, vp]),
        "casr_profile_read": (i32, [vp, i32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)]),
        "casr_set_option": (i32, [vp, i32, i32]),
        "casr_get_option": (i32, [vp, i32, ctypes.POINTER(ctypes.c_int32)]),
        "casr_convert_audio": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, f32, vp, vp, vp, vp]),
        "casr_resample_plan": (i32, [i32] + [ctypes.POINTER(ctypes.c_int32)] * 3),
        "casr_resample_filter": (i32, [i32, vp]),
        "casr_resample_frames": (i32, [i32, i32]),
        "casr_lm_create": (i32, [i32, i32, i32, vp, vp, vp, vp, ctypes.POINTER(vp)]),
        "casr_lm_destroy": (None, [vp]),
        "casr_lm_score_host": (i32, [vp, vp, vp, i32, i32, i32, vp]),
        "casr_lm_score": (i32, [vp, vp, vp, vp, i32, i32, i32, vp, vp]),
        "casr_beam_rescore": (i32, [vp, vp, ctypes.c_double, ctypes.c_double, vp, vp, vp, vp, vp, vp]),
        "casr_lm_terms_host": (i32, [vp, vp, vp, i32, i32, vp]),
        "casr_lm_terms": (i32, [vp, vp, vp, vp, i32, i32, vp, vp]),
        "casr_beam_lm": (i32, [vp, vp, i32, ctypes.c_float, ctypes.c_float, vp, vp, vp, vp, vp, vp]),
        "casr_beam_record_lm": (i32, [vp, vp, vp]),
        "casr_segment_default_params": (i32, [vp]),
        "casr_segment_bound": (i32, [i32, vp]),
        "casr_segment_host": (i32, [vp, vp, i32, i32, i32, vp, i32, vp, vp, vp, vp]),
        "casr_segment": (i32, [vp, vp, vp, i32, i32, vp, i32, vp, vp, vp, vp, vp]),
        "casr_gather_segments": (i32, [vp, vp, i32, i32, vp, vp, vp, i32, i32, vp, vp, vp]),
        "casr_edit_distance_host": (i32, [vp, vp, i32, vp, vp, i32, i32, vp, vp]),
        "casr_edit_distance": (i32, [vp, vp, vp, i32, vp, vp, i32, i32, vp, vp, vp]),
        "casr_edit_align_host": (i32, [vp, vp, i32, vp, vp, i32, i32, vp, vp, vp, vp]),
        "casr_edit_align_tiles_host": (i32, [vp, vp, i32, vp, vp, i32, i32, vp, vp, vp, vp]),
        "casr_edit_align": (i32, [vp, vp, vp, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp]),
        "casr_edit_align_plan": (i32, [i32, i32, i32, i32, vp, vp]),
        "casr_edit_align_workspace_bytes": (ctypes.c_int64, [vp]),
        "casr_mbr_host": (i32, [vp, vp, vp, vp, i32, i32, i32] + [ctypes.c_double] * 3 + [vp, vp]),
        "casr_beam_mbr": (i32, [vp, ctypes.c_double, vp, ctypes.c_double, ctypes.c_double, vp, vp, vp, vp, vp, vp, vp]),
        "casr_beam_mbr_distances": (i32, [vp, vp, vp, vp]),
        "casr_bias_create": (i32, [i32, i32, i32, vp, vp, vp, ctypes.POINTER(vp)]),
        "casr_bias_destroy": (None, [vp]),
        "casr_bias_score_host": (i32, [vp, vp, vp, i32, i32, vp, vp, vp]),
        "casr_bias_score": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, vp, vp]),
        "casr_bias_rows_host": (i32, [vp, vp, i32, vp, vp]),
        "casr_bias_rows": (i32, [vp, vp, vp, i32, vp, vp, vp]),
        "casr_beam_bias": (i32, [vp, vp, vp, i32, f32, f32, f32, vp, vp, vp, vp, vp, vp, vp]),
        "casr_beam_record_bias": (i32, [vp, vp, vp]),
        "casr_grammar_create": (i32, [i32, i32, i32, i32, vp, vp, vp, vp, ctypes.POINTER(vp)]),
        "casr_grammar_destroy": (None, [vp]),
        "casr_grammar_info": (i32, [vp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64), vp]),
        "casr_grammar_mask_words": (i32, [i32]),
        "casr_grammar_accept_host": (i32, [vp, vp, vp, i32, i32, vp, vp, vp]),
        "casr_grammar_accept": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, vp, vp]),
        "casr_grammar_rows_host": (i32, [vp, vp, vp, i32, vp]),
        "casr_grammar_rows": (i32, [vp, vp, vp, vp, i32, vp, vp]),
        "casr_beam_grammar": (i32, [vp, vp, vp, vp, i32, f32, f32, vp, vp, vp, vp, vp, vp, vp]),
        "casr_align_path_host": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp, vp]),
        "casr_align_path": (i32, [vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp]),
        "casr_posterior_units_host": (i32, [vp, vp, vp, i32, i32, i32] + [ctypes.c_double] * 3 + [vp, vp]),
        "casr_nbest_host": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, ctypes.c_double, ctypes.c_double, vp, vp, vp, vp]),
        "casr_confusion_host": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp]),
        "casr_confusion": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp]),
        "casr_beam_nbest": (i32, [vp, i32, vp, ctypes.c_double, ctypes.c_double, vp, vp, vp, vp, vp]),
        "casr_beam_confusion": (i32, [vp, i32, ctypes.c_double, vp, ctypes.c_double, ctypes.c_double, vp, vp, vp, vp, vp,
                                      vp, vp, vp]),
        "casr_lm_estimate_host": (i32, [i32, i32, vp, vp, ctypes.c_int64, ctypes.POINTER(vp)]),
        "casr_lm_estimate": (i32, [vp, i32, vp, vp, ctypes.c_int64, vp, ctypes.POINTER(vp)]),
        "casr_lm_estimate_combine": (i32, [i32]),
        "casr_lm_estimate_info": (i32, [vp, vp, vp, vp, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
        "casr_lm_estimate_arrays": (i32, [vp, i32, vp, vp, vp, vp, vp, vp]),
        "casr_lm_estimate_counts": (i32, [vp, i32, vp]),
        "casr_lm_estimate_timing": (i32, [vp, vp]),
        "casr_lm_estimate_destroy": (None, [vp]),
        "casr_lm_estimate_workspace_bytes": (ctypes.c_int64, [i32, ctypes.c_int64]),
        "casr_lm_prune_host": (i32, [vp, ctypes.c_double, ctypes.POINTER(vp)]),
        "casr_lm_prune": (i32, [vp, vp, ctypes.c_double, vp, ctypes.POINTER(vp)]),
        "casr_lm_prune_info": (i32, [vp, vp, vp, vp, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)]),
        "casr_lm_prune_arrays": (i32, [vp, i32, vp, vp, vp, vp]),
        "casr_lm_prune_decisions": (i32, [vp, i32, vp, vp, vp]),
        "casr_lm_prune_timing": (i32, [vp, vp]),
        "casr_lm_prune_destroy": (None, [vp]),
        "casr_lm_prune_workspace_bytes": (ctypes.c_int64, [vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.casr_api_version() != 3:
        raise CasrError("casr library API version mismatch")
    _LIBS[key] = lib
    return lib


def register_handle(handle, lib):
    _HANDLES[handle.value] = lib


def unregister_handle(handle):
    _HANDLES.pop(handle.value, None)


def check(rc, handle=None, lib=None):
    if rc != 0:
        lib = lib or (_HANDLES.get(handle.value) if handle is not None and handle.value else None) or load()
        msg = lib.casr_last_error(handle)
        raise CasrError(f"{STATUS.get(rc, rc)}: {msg.decode(errors='replace') if msg else ''}")


def mel_filterbank(n_stft=257, f_min=80.0, f_max=7600.0, n_mels=80):
    """The filterbank casr_log_mel uses (create_fb_matrix, data.py:21-57), computed by the
    library on the host: float32 [n_stft, n_mels]."""
    lib = load()
    out = np.empty((n_stft, n_mels), np.float32)
    check(lib.casr_mel_filterbank(n_stft, ctypes.c_float(f_min), ctypes.c_float(f_max), n_mels,
                                  out.ctypes.data_as(ctypes.c_void_p)))
    return out


def log_mel_frames(n_samples):
    """Frames of log-mel an utterance of n_samples produces (0 below 513 samples)."""
    return int(load().casr_log_mel_frames(int(n_samples)))


def resample_plan(rate):
    """(L, M, taps) of casr_convert_audio's resampler for an input rate (include/casr.h): 16000 / g,
    rate / g and the 2K taps of every phase.  Raises CasrError on a rate the library refuses."""
    lib = load()
    L, M, taps = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    check(lib.casr_resample_plan(int(rate), ctypes.byref(L), ctypes.byref(M), ctypes.byref(taps)), lib=lib)
    return L.value, M.value, taps.value


def resample_filter(rate):
    """The f32 polyphase table [L, taps] casr_convert_audio applies at an input rate."""
    lib = load()
    L, _, taps = resample_plan(rate)
    out = np.empty((L, taps), np.float32)
    check(lib.casr_resample_filter(int(rate), out.ctypes.data_as(ctypes.c_void_p)), lib=lib)
    return out


def resample_frames(n_in, rate):
    """16 kHz samples casr_convert_audio produces from n_in frames at a rate: ceil(n_in L / M)."""
    n = int(load().casr_resample_frames(int(n_in), int(rate)))
    if n < 0:
        raise CasrError(f"casr_resample_frames({n_in}, {rate}): unsupported rate, or the count does not fit an int")
    return n


def config_struct(cfg):
    return CasrConfigC(cfg.n_mels, cfg.feat_dim, cfg.enc_hidden, cfg.enc_layers, int(cfg.residual),
                       cfg.dec_hidden, cfg.embed_dim, cfg.attn_size, cfg.vocab, cfg.max_len,
                       cfg.sos, cfg.eos, float(cfg.temperature))


def packed_floats(cfg):
    """Floats in this build's packed weight layout (casr_packed_weights_floats)."""
    c = config_struct(cfg)
    n = int(load().casr_packed_weights_floats(ctypes.byref(c)))
    if n == 0:
        check(4)
    return n


def pack_weights(cfg, enc_sd, dec_sd):
    """Pack reference state dicts (numpy float32) into the kernel blob (host numpy array)."""
    lib = load()
    c = config_struct(cfg)
    n = lib.casr_packed_weights_floats(ctypes.byref(c))
    if n == 0:
        check(4)
    keep = []

    def ptr(a):
        a = np.ascontiguousarray(a, dtype=np.float32)
        keep.append(a)
        return a.ctypes.data_as(_FP)

    w = CasrWeightsHostC()
    for l in range(cfg.enc_layers):
        for d, suf in enumerate(("", "_reverse")):
            p = f"rnn.rnn.{l}."
            w.enc_w_ih[l][d] = ptr(enc_sd[p + "weight_ih_l0" + suf])
            w.enc_w_hh[l][d] = ptr(enc_sd[p + "weight_hh_l0" + suf])
            w.enc_b_ih[l][d] = ptr(enc_sd[p + "bias_ih_l0" + suf])
            w.enc_b_hh[l][d] = ptr(enc_sd[p + "bias_hh_l0" + suf])
    w.embedding = ptr(dec_sd["embedding.weight"])
    w.dec_w_ih = ptr(dec_sd["cell.cell.0.weight_ih"])
    w.dec_w_hh = ptr(dec_sd["cell.cell.0.weight_hh"])
    w.dec_b_ih = ptr(dec_sd["cell.cell.0.bias_ih"])
    w.dec_b_hh = ptr(dec_sd["cell.cell.0.bias_hh"])
    w.proj_w = ptr(dec_sd["proj_linear.weight"])
    w.proj_b = ptr(dec_sd["proj_linear.bias"])
    w.attn_w_enc = ptr(dec_sd["attn_mechanism.W_enc"])
    w.attn_b = ptr(dec_sd["attn_mechanism.b_attn"])
    w.attn_w_hidden = ptr(dec_sd["attn_mechanism.W_hidden"])
    w.attn_v = ptr(dec_sd["attn_mechanism.v"])
    out = np.empty(n, np.float32)
    check(lib.casr_pack_weights(ctypes.byref(c), ctypes.byref(w), out.ctypes.data_as(ctypes.c_void_p)))
    return out


EDIT_MAX_LEN = 512  # include/casr.h CASR_EDIT_MAX_LEN: the longest row of the device entry
EDIT_ALIGN_MAX_LEN = 32768  # include/casr.h CASR_EDIT_ALIGN_MAX_LEN: the longest row of casr_edit_align
EDIT_ALIGN_TILE = (128, 64)  # csrc/edit_align_plan.h EA_TR, EA_TC: rows and columns of a tile
BIAS_MAX_LEN = 16   # include/casr.h CASR_BIAS_MAX_LEN: the longest phrase
ALIGN_MAX_TP = 1024  # include/casr.h CASR_ALIGN_MAX_TP: the longest row of casr_align_path
CN_EPS, CN_NONE = -1, -2  # include/casr.h CASR_CN_EPS, CASR_CN_NONE: "nothing here", an unused entry
CN_MAX_M, NBEST_MAX_N = 8, 64  # include/casr.h CASR_CN_MAX_M, CASR_NBEST_MAX_N


def _i32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.int32)
    if shape is not None and a.shape != shape:
        raise ValueError(f"expected an int32 array of shape {shape}, got {a.shape}")
    return a


def edit_distance_host(a, a_len, b, b_len, ops=False):
    """casr_edit_distance_host: a [n, La], b [n, Lb] int32 symbols with their lengths -> dist [n] int32,
    and with ``ops`` the (insert, delete, replace) counts [n, 3] of the script turning a into b
    (casr.results.edit_distance / edit_ops, value for value).  Host only, no GPU."""
    lib = load()
    a, b = np.ascontiguousarray(a, dtype=np.int32), np.ascontiguousarray(b, dtype=np.int32)
    if a.ndim != 2 or b.ndim != 2 or a.shape[0] != b.shape[0]:
        raise ValueError("edit_distance_host: a must be [n, La] and b [n, Lb]")
    n = a.shape[0]
    a_len, b_len = _i32(a_len, (n,)), _i32(b_len, (n,))
    dist = np.zeros(n, np.int32)
    counts = np.zeros((n, 3), np.int32) if ops else None
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None and x.size else None  # noqa: E731
    check(lib.casr_edit_distance_host(p(a), p(a_len), a.shape[1], p(b), p(b_len), b.shape[1], n, p(dist), p(counts)),
          lib=lib)
    return (dist, counts) if ops else dist


def edit_align_host(a, a_len, b, b_len, tiles=False):
    """casr_edit_align_host: a [n, La], b [n, Lb] int32 symbols with their lengths -> dict of dist [n],
    ops [n, 3] (insert, delete, replace), b_of_a [n, La] and a_of_b [n, Lb] int32: where the backtrace
    takes a diagonal step through cell (i, j), b_of_a[i] = j and a_of_b[j] = i; -1 for a deleted or
    inserted symbol and past a length.  ``tiles``: computed in the device's tile order
    (casr_edit_align_tiles_host), the same values.  Host only, no GPU."""
    lib = load()
    a, b = np.ascontiguousarray(a, dtype=np.int32), np.ascontiguousarray(b, dtype=np.int32)
    if a.ndim != 2 or b.ndim != 2 or a.shape[0] != b.shape[0]:
        raise ValueError("edit_align_host: a must be [n, La] and b [n, Lb]")
    n = a.shape[0]
    a_len, b_len = _i32(a_len, (n,)), _i32(b_len, (n,))
    dist = np.zeros(n, np.int32)
    counts = np.zeros((n, 3), np.int32)
    b_of_a = np.full(a.shape, -1, np.int32)
    a_of_b = np.full(b.shape, -1, np.int32)
    fn = lib.casr_edit_align_tiles_host if tiles else lib.casr_edit_align_host
    check(fn(_p(a), _p(a_len), a.shape[1], _p(b), _p(b_len), b.shape[1], n, _p(dist), _p(counts), _p(b_of_a),
             _p(a_of_b)), lib=lib)
    return dict(dist=dist, ops=counts, b_of_a=b_of_a, a_of_b=a_of_b)


def edit_align_plan(La, Lb, n=1, bits=True):
    """casr_edit_align_plan: what casr_edit_align does with n pairs of [La] x [Lb] -> dict of ok,
    tiles_r, tiles_c, launches, bits_bytes, bytes (the workspace) and grid (workgroups per launch)."""
    lib = load()
    out = np.zeros(6, np.int64)
    check(lib.casr_edit_align_plan(int(La), int(Lb), int(n), int(bool(bits)), _p(out), None), lib=lib)
    grid = np.zeros(int(out[3]), np.int64)
    check(lib.casr_edit_align_plan(int(La), int(Lb), int(n), int(bool(bits)), _p(out), _p(grid)), lib=lib)
    return dict(ok=bool(out[0]), tiles_r=int(out[1]), tiles_c=int(out[2]), launches=int(out[3]),
                bits_bytes=int(out[4]), bytes=int(out[5]), grid=grid.tolist())


def mbr_host(rec_tokens, rec_score, rec_valid, scale, rec_lm=None, lm_weight=0.0, length_weight=0.0, risk=False):
    """casr_mbr_host on the arrays casr_beam_records writes: rec_tokens [B, L, k, L], rec_score and
    rec_valid [B, L, k], rec_lm None or [B, L, k] -> best_index [B] (step k + rank, -1 without a
    record), and with ``risk`` rec_risk [B, L, k] float64.  Host only, no GPU."""
    lib = load()
    rt = np.ascontiguousarray(rec_tokens, dtype=np.int32)
    B, L, k = rt.shape[:3]
    if rt.shape != (B, L, k, L):
        raise ValueError("mbr_host: rec_tokens must be [B, L, k, L]")
    rs = np.ascontiguousarray(rec_score, dtype=np.float32)
    rv = np.ascontiguousarray(rec_valid, dtype=np.uint8)
    rl = None if rec_lm is None else np.ascontiguousarray(rec_lm, dtype=np.float32)
    for x in (rs, rv) + ((rl,) if rl is not None else ()):
        if x.shape != (B, L, k):
            raise ValueError("mbr_host: rec_score, rec_valid and rec_lm must be [B, L, k]")
    best = np.full(B, -1, np.int32)
    rr = np.zeros((B, L, k), np.float64) if risk else None
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None and x.size else None  # noqa: E731
    check(lib.casr_mbr_host(p(rt), p(rs), p(rv), p(rl), B, L, k, float(scale), float(lm_weight), float(length_weight),
                            p(best), p(rr)), lib=lib)
    return (best, rr) if risk else best


def align_path_host(align, enc_len, tgt_len):
    """casr_align_path_host: the best monotone path through attention weights align [L, Tp, B] float32
    (the layout Engine.greedy and Engine.score write), enc_len [B] encoder frames and tgt_len [B] scored
    positions per utterance -> dict of first, last, peak [B, L] int32 (-1 past tgt_len) and path_score
    [B] int32 (include/casr.h has the formulas).  Host only, no GPU."""
    lib = load()
    align = np.ascontiguousarray(align, dtype=np.float32)
    if align.ndim != 3:
        raise ValueError("align_path_host: align must be [L, Tp, B]")
    L, Tp, B = align.shape
    enc_len, tgt_len = _i32(enc_len, (B,)), _i32(tgt_len, (B,))
    first, last, peak = (np.full((B, L), -1, np.int32) for _ in range(3))
    score = np.zeros(B, np.int32)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x.size else None  # noqa: E731
    check(lib.casr_align_path_host(p(align), p(enc_len), p(tgt_len), B, Tp, L, p(first), p(last), p(peak), p(score)),
          lib=lib)
    return dict(first=first, last=last, peak=peak, path_score=score)


def _records(who, rec_tokens, rec_valid, *others):
    """rec_tokens [B, L, k, L] int32, rec_valid and every other given array [B, L, k]."""
    rt = np.ascontiguousarray(rec_tokens, dtype=np.int32)
    B, L, k = rt.shape[:3]
    if rt.shape != (B, L, k, L):
        raise ValueError(f"{who}: rec_tokens must be [B, L, k, L]")
    out = [rt, np.ascontiguousarray(rec_valid, dtype=np.uint8)]
    out += [None if x is None else np.ascontiguousarray(x, dtype=dt) for x, dt in others]
    for x in out[1:]:
        if x is not None and x.shape != (B, L, k):
            raise ValueError(f"{who}: rec_valid and the other record arrays must be [B, L, k]")
    return (B, L, k), out


def _p(x):
    return x.ctypes.data_as(ctypes.c_void_p) if x is not None and x.size else None


def posterior_units_host(rec_score, rec_valid, scale, rec_lm=None, lm_weight=0.0, length_weight=0.0):
    """casr_posterior_units_host on the arrays casr_beam_records writes: rec_score, rec_valid and rec_lm
    (or None) [B, L, k] -> (rec_unit [B, L, k] int64 = floor(exp(scale (c - c_max)) 2^32), 0 where there is
    no record, total [B] int64).  Host only, no GPU."""
    lib = load()
    rs = np.ascontiguousarray(rec_score, dtype=np.float32)
    rv = np.ascontiguousarray(rec_valid, dtype=np.uint8)
    rl = None if rec_lm is None else np.ascontiguousarray(rec_lm, dtype=np.float32)
    if rs.ndim != 3 or rv.shape != rs.shape or (rl is not None and rl.shape != rs.shape):
        raise ValueError("posterior_units_host: rec_score, rec_valid and rec_lm must be [B, L, k]")
    B, L, k = rs.shape
    unit = np.zeros((B, L, k), np.int64)
    total = np.zeros(B, np.int64)
    check(lib.casr_posterior_units_host(_p(rs), _p(rv), _p(rl), B, L, k, float(scale), float(lm_weight),
                                        float(length_weight), _p(unit), _p(total)), lib=lib)
    return unit, total


def nbest_host(rec_tokens, rec_score, rec_valid, N, rec_lm=None, lm_weight=0.0, length_weight=0.0):
    """casr_nbest_host: the N records with the largest c per utterance -> dict of index [B, N] (step k +
    rank, -1 past the record count), tokens [B, N, L] (-1 past each length), length [B, N] and comb
    [B, N] float64.  Host only, no GPU."""
    lib = load()
    (B, L, k), (rt, rv, rs, rl) = _records("nbest_host", rec_tokens, rec_valid, (rec_score, np.float32),
                                           (rec_lm, np.float32))
    N = int(N)
    index = np.full((B, N), -1, np.int32)
    toks = np.full((B, N, L), -1, np.int32)
    ln = np.zeros((B, N), np.int32)
    comb = np.zeros((B, N), np.float64)
    check(lib.casr_nbest_host(_p(rt), _p(rs), _p(rv), _p(rl), B, L, k, N, float(lm_weight), float(length_weight),
                              _p(index), _p(toks), _p(ln), _p(comb)), lib=lib)
    return dict(index=index, tokens=toks, length=ln, comb=comb)


def confusion_host(rec_tokens, rec_valid, rec_unit, pivot, vocab, M=4):
    """casr_confusion_host: the confusion network of every utterance's records around its pivot (a flat
    index step k + rank, [B]) under the given units rec_unit [B, L, k] int64 -> dict of n_slots [B],
    slot_token [B, 2 L + 1, M] int32 (CN_EPS = -1: nothing, CN_NONE = -2: unused), slot_mass of the same
    shape int64, pivot_mass [B, L] int64 and total [B] int64.  Host only, no GPU."""
    lib = load()
    (B, L, k), (rt, rv, ru) = _records("confusion_host", rec_tokens, rec_valid, (rec_unit, np.int64))
    pv = _i32(pivot, (B,))
    M = int(M)
    n_slots = np.zeros(B, np.int32)
    st = np.full((B, 2 * L + 1, max(M, 0)), CN_NONE, np.int32)
    sm = np.zeros((B, 2 * L + 1, max(M, 0)), np.int64)
    pm = np.zeros((B, L), np.int64)
    total = np.zeros(B, np.int64)
    check(lib.casr_confusion_host(_p(rt), _p(rv), _p(ru), _p(pv), B, L, k, int(vocab), M, _p(n_slots), _p(st), _p(sm),
                                  _p(pm), _p(total)), lib=lib)
    return dict(n_slots=n_slots, slot_token=st, slot_mass=sm, pivot_mass=pm, total=total)
