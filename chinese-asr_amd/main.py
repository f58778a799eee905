#!/usr/bin/env python
"""Drop-in for the reference's ``main.py`` (main.py:19-102) on the MI355X path.

``parse(path, model, audio_base, lm_model, bw)`` and ``ASR(lm_path=None, bw=None)(path)`` keep
the reference signatures and results; ``align(path, text, model, audio_base)`` is this path's own
addition (forced alignment of a given transcript), and so are ``transcribe(paths, model, audio_base)``
(recordings of any length, cut at their pauses on the device: casr_segment), ``parse_timed`` and
``ASR.subtitles`` (a start, an end and a confidence per decoded character: casr_align_path), and
``align_long`` / ``ASR.align`` (a long recording timed against the text known to be spoken in it:
casr_edit_align, casr.longalign).  The chain wav ->
log-mel -> delta/stack -> CMVN (eps 1e-6, main.py:37) -> encoder -> greedy / beam (+ second pass with a KenLM-like
``lm_model.score(s, bos=True)``) runs on the GPU through the casr C ABI.  Format conversion
(``convert_audio``: ffmpeg + sox, main.py:19-24) uses the external tools where both are present;
without them a WAV input of any rate and channel count is converted on the device
(``data.load_audio``: casr_convert_audio), and only a non-WAV container is refused.
"""
import os
import shutil
import subprocess
import sys
import tempfile
from time import time

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from gpd import gpd  # noqa: E402
from data import AudioBase, fast_read, load_audio, log_mel_batch  # noqa: E402
from model import Model  # noqa: E402


def convert_audio(path):
    """main.py:19-24: ffmpeg -> 16 kHz mono s16, sox --norm=-1.  Without the tools, a WAV input is
    returned as it is (read_audio then converts it on the device)."""
    if shutil.which("ffmpeg") and shutil.which("sox"):
        td = tempfile.mkdtemp()
        tmp, norm = os.path.join(td, "tmp.wav"), os.path.join(td, "a.wav")
        subprocess.run(["ffmpeg", "-loglevel", "quiet", "-i", path, "-sample_fmt", "s16", "-ar", "16000",
                        "-ac", "1", tmp], check=True)
        subprocess.run(["sox", "--norm=-1", tmp, norm], check=True)
        return norm
    if not path.lower().endswith(".wav"):
        raise RuntimeError(f"{path}: ffmpeg/sox are not available to convert it; pass a 16 kHz mono WAV")
    return path


def have_tools():
    return bool(shutil.which("ffmpeg") and shutil.which("sox"))


def read_audio(paths):
    """Paths (or sample arrays, passed through) -> 16 kHz mono float32 sample arrays.  With ffmpeg and
    sox present: the reference's chain, file by file.  Without them: WAV files of any rate and
    channel count through data.load_audio as one batch (a non-WAV path raises, as convert_audio does)."""
    out = list(paths)
    files = [i for i, p in enumerate(out) if isinstance(p, (str, os.PathLike))]
    if have_tools():
        for i in files:
            out[i] = fast_read(convert_audio(out[i]))
    elif files:
        for i, a in zip(files, load_audio([convert_audio(os.fspath(out[i])) for i in files])):
            out[i] = a
    return out


def features_for(audios):
    """Samples -> CMVN'd encoder inputs (data.py:167-253 + main.py:37), batched on the GPU.
    Returns the list-of-tensors form Model.eval_one_batch_* takes, plus lengths."""
    feat, flen = log_mel_batch(audios, cmvn_eps=1e-6)
    lens = flen.cpu()
    return [feat[b, :int(lens[b])] for b in range(len(audios))], lens


def parse(path, model, audio_base, lm_model, bw, fusion=False, bias=None, bias_weight=1.0, grammar=None):
    """main.py:27-65: one file -> predicted text.  ``fusion``, ``bias`` (a casr.bias.PhraseBias),
    ``bias_weight`` and ``grammar`` (a casr.grammar.Grammar: the answer is one of its sentences):
    Model.eval_one_batch_with_beam's; with a bias or a grammar an LM takes part only when fused."""
    data, lens = features_for(read_audio([path]))
    text = None
    if bw is not None:
        if gpd['verbose']:
            print(f"[INFO] Beam Decode [bw={bw}]...")
        res = model.eval_one_batch_with_beam(model.device, bw, data, lens, text, audio_base.int2word,
                                             **_beam_args(lm_model, fusion, bias, bias_weight, grammar))
    else:
        res = model.eval_one_batch_with_greedy(model.device, data, lens, audio_base.int2word, text)
    return res.pred_text[0]


def parse_timed(path, model, audio_base, lm_model=None, bw=None, fusion=False, bias=None, bias_weight=1.0):
    """parse with times: one file -> [(char, start_s, end_s, confidence)], one tuple per character of
    the text parse returns (Model.eval_one_batch_*'s ``timestamps``; casr.results.token_spans says what
    the times mean)."""
    data, lens = features_for(read_audio([path]))
    if bw is not None:
        res = model.eval_one_batch_with_beam(model.device, bw, data, lens, None, audio_base.int2word, timestamps=True,
                                             **_beam_args(lm_model, fusion, bias, bias_weight))
    else:
        res = model.eval_one_batch_with_greedy(model.device, data, lens, audio_base.int2word, None, timestamps=True)
    return [(ch, t[0], t[1], t[3]) for ch, t in zip(res.pred_text[0], res.timing[0])]


def _beam_args(lm_model, fusion, bias, bias_weight, grammar=None):
    """The beam's keyword arguments; with a bias or a grammar the LM enters only fused, and no second pass
    runs.  The grammar keyword is passed only when one is given."""
    if (bias is not None or grammar is not None) and not fusion:
        lm_model = None
    kw = dict(second_pass=lm_model is not None, lm_model=lm_model, lm_weight=1.5, length_weight=1.5,
              fusion=fusion and lm_model is not None, bias=bias, bias_weight=bias_weight)
    if grammar is not None:
        kw["grammar"] = grammar
    return kw


def align(path, text, model, audio_base):
    """Forced alignment of a known transcript: one file and its text -> [(char, start_s, logp)],
    the attention's argmax frame of each character in seconds and its teacher-forced
    log-probability (Model.score_one_batch; the closing eos is scored but not listed)."""
    data, lens = features_for(read_audio([path]))
    res = model.score_one_batch(model.device, data, lens, [text], audio_base.word2int, audio_base.int2word)
    start = res.times['frame_s'][0]
    return [(ch, float(start[i]), float(res.token_logp[0][i])) for i, ch in enumerate(text)]


def parse_batch(paths, model, audio_base, lm_model=None, bw=None, fusion=False, bias=None, bias_weight=1.0,
                grammar=None):
    """Batched form of parse (the reference's __init__.py names it but never defines it): all
    files go through the GPU path as one batch."""
    data, lens = features_for(read_audio(paths))
    if bw is not None:
        res = model.eval_one_batch_with_beam(model.device, bw, data, lens, None, audio_base.int2word,
                                             **_beam_args(lm_model, fusion, bias, bias_weight, grammar))
    else:
        res = model.eval_one_batch_with_greedy(model.device, data, lens, audio_base.int2word, None)
    return list(res.pred_text)


MIN_SEGMENT_FRAMES = 9  # the delta filters' 9 taps: a shorter segment is returned with empty text


def transcribe(paths, model, audio_base, lm_model=None, bw=None, params=None, batch_size=256, fusion=False,
               bias=None, bias_weight=1.0, timestamps=False):
    """Recordings of any length -> per recording a list of casr.segment.Segment (start_s, end_s, text,
    score, truncated), this path's own addition: the log-mel of every recording is cut at its pauses
    on the device (casr_segment, include/casr.h; ``params`` a casr.segment.SegmentParams) and the
    segments are decoded as parse decodes an utterance, ``batch_size`` at a time in (recording, time)
    order.  ``truncated`` marks a segment whose decode used all max_len steps without an EOS (lower
    ``params.max_frames`` then).  A recording with no speech returns [].  With ``timestamps`` every
    decoded segment's ``chars`` holds [(char, start_s, end_s, confidence)], one per character of its
    text, in the recording's time (parse_timed's tuples, offset by the segment's start)."""
    return _transcribe(paths, model, audio_base, lm_model, bw, params, batch_size, fusion, bias, bias_weight,
                       timestamps)[0]


def _transcribe(paths, model, audio_base, lm_model, bw, params, batch_size, fusion, bias, bias_weight, timestamps):
    """transcribe's work -> (its result, what a second pass over the same segments needs: None without a
    segment, else a dict of the log-mel ``fb``, the segments' ``src``, ``starts``, ``lens`` on the device,
    ``src_h`` and ``lens_h`` on the host, all ``segs`` in (recording, time) order and ``todo``, the
    indices of those long enough to decode)."""
    import numpy as np
    import torch
    from data import _engine
    from casr.segment import Segment, SegmentParams, frame_time

    params = (params or SegmentParams()).validate()
    audios = read_audio(paths)
    eng = _engine()
    n = [int(len(a)) for a in audios]
    if min(n) < 513:  # as log_mel_batch: torch.stft raises on a signal shorter than n_fft (data.py:204)
        raise RuntimeError(f"audio of {min(n)} samples is shorter than n_fft + 1 = 513")
    wav = np.zeros((len(audios), max(n)), np.float32)
    for b, a in enumerate(audios):
        wav[b, :n[b]] = a
    fb, frames = eng.log_mel(torch.from_numpy(wav).to(eng.device), torch.tensor(n, dtype=torch.int32),
                             preemphasis=float(gpd['preemphasis']))
    start, length, n_seg, _ = eng.segment(fb, frames, params)
    counts = n_seg.cpu().tolist()  # the one read the decode's shape depends on
    out = [[] for _ in audios]
    if sum(counts) == 0:
        return out, None
    src = torch.tensor([b for b, c in enumerate(counts) for _ in range(c)], dtype=torch.int64, device=eng.device)
    slot = torch.tensor([i for c in counts for i in range(c)], dtype=torch.int64, device=eng.device)
    starts, lens = start[src, slot], length[src, slot]  # (recording, time) order, no sorting
    src_h, starts_h, lens_h = src.cpu().tolist(), starts.cpu().tolist(), lens.cpu().tolist()
    segs = [Segment(frame_time(s), frame_time(s + l), '', 0.0, False) for s, l in zip(starts_h, lens_h)]
    todo = [i for i, l in enumerate(lens_h) if l >= MIN_SEGMENT_FRAMES]
    for c0 in range(0, len(todo), int(batch_size)):
        idx = todo[c0:c0 + int(batch_size)]
        sel = torch.tensor(idx, dtype=torch.int64, device=eng.device)
        seg_fb, seg_frames = eng.gather_segments(fb, src[sel], starts[sel], lens[sel], t_seg=max(lens_h[i] for i in idx))
        feat, flen = eng.features(seg_fb, seg_frames, eps=1e-6)
        flen = flen.cpu()
        data = [feat[i, :int(flen[i])] for i in range(len(idx))]
        if bw is not None:
            res = model.eval_one_batch_with_beam(model.device, bw, data, flen, None, audio_base.int2word,
                                                 timestamps=timestamps,
                                                 **_beam_args(lm_model, fusion, bias, bias_weight))
            # no finished hypothesis: the fallback ran to max_len (with timestamps the model took the
            # flags before its scoring pass reused the beam's workspace)
            cut = (model.beam_unfinished if timestamps else
                   ~model.engine.beam_records()[2].flatten(1).bool().any(1)).cpu().tolist()
        else:
            res = model.eval_one_batch_with_greedy(model.device, data, flen, audio_base.int2word, None,
                                                   timestamps=timestamps)
            cut = (res.text_len >= model.cfg.max_len).cpu().tolist()
        for j, i in enumerate(idx):
            segs[i].text, segs[i].score, segs[i].truncated = res.pred_text[j], float(res.score[j]), bool(cut[j])
            if timestamps:
                t0 = segs[i].start_s
                segs[i].chars = [(ch, t0 + t[0], t0 + t[1], t[3]) for ch, t in zip(res.pred_text[j], res.timing[j])]
    for b, s in zip(src_h, segs):
        out[b].append(s)
    return out, dict(fb=fb, src=src, starts=starts, lens=lens, src_h=src_h, lens_h=lens_h, segs=segs, todo=todo)


def align_long(paths, texts, model, audio_base, params=None, batch_size=256, bw=None, lm_model=None, fusion=False,
               bias=None, bias_weight=1.0):
    """Recordings of any length and the text known to be spoken in each -> per recording a
    casr.longalign.AlignedRecording: the list of casr.segment.Segment whose ``text`` is the part of the
    transcript spoken in the segment and whose ``chars`` hold [(char, start_s, end_s, confidence)] for
    every character of it in recording time, plus the recording's ``dist`` and ``ops`` (the character
    errors of the decode against the transcript: how far the alignment can be trusted).
    casr.longalign states the policy.  The steps: transcribe's own segmentation and decode (greedy, or a
    beam with ``bw`` and transcribe's other arguments); ONE casr_edit_align call for all recordings,
    decoded ids against transcript ids; a span of the transcript per segment (assign_spans); a second
    pass over the segments, ``batch_size`` at a time in the same order, gathered and encoded as the
    first, that scores every span teacher-forced with its closing eos (a span of exactly max_len tokens
    without it, as transcribe times a decode that ran to max_len) and runs the monotone path through its
    attention (casr_score, casr_align_path).  ``confidence`` is exp of the character's teacher-forced
    log-probability, as transcribe(timestamps=True) reports it; None for a character outside the
    vocabulary and in an ``interpolated`` segment."""
    import numpy as np
    import torch
    from data import _engine
    from casr import lib as _lib
    from casr import longalign as LA

    paths, texts = list(paths), list(texts)
    if len(paths) != len(texts):
        raise ValueError(f"align_long: {len(paths)} recordings but {len(texts)} texts")
    w2i, i2w = audio_base.word2int, audio_base.int2word
    out, st = _transcribe(paths, model, audio_base, lm_model, bw, params, batch_size, fusion, bias, bias_weight, False)
    ref = [LA.text_ids(t, w2i) for t in texts]
    hyp = [[i for s in segs for i in LA.hyp_ids(s.text, w2i)] for segs in out]
    n = len(paths)
    eng = _engine()
    a = np.zeros((n, max([1] + [len(h) for h in hyp])), np.int32)
    b = np.zeros((n, max([1] + [len(r[0]) for r in ref])), np.int32)
    for k in range(n):
        a[k, :len(hyp[k])] = hyp[k]
        b[k, :len(ref[k][0])] = ref[k][0]
    a_len, b_len = [len(h) for h in hyp], [len(x[0]) for x in ref]
    if _lib.edit_align_plan(a.shape[1], b.shape[1], n)["ok"]:
        r = eng.edit_align(a, a_len, b, b_len)
        dist, ops, a_of_b = (r[key].cpu().numpy() for key in ("dist", "ops", "a_of_b"))
    else:  # past the device entry's limits (include/casr.h): the host entry, the same values
        r = _lib.edit_align_host(a, a_len, b, b_len)
        dist, ops, a_of_b = r["dist"], r["ops"], r["a_of_b"]
    result, spans = [], []
    for k in range(n):
        ids, pos = ref[k]
        if not out[k] and ids:
            raise RuntimeError(f"align_long: recording {k} has no speech segment to hold its transcript")
        sp = LA.assign_spans([len(s.text) for s in out[k]], a_of_b[k, :len(ids)])
        for s, txt in zip(out[k], LA.span_text(texts[k], pos, sp)):
            s.text, s.score, s.truncated, s.chars, s.interpolated = txt, 0.0, False, [], False
        spans += [(k, lo, hi) for lo, hi in sp]
        result.append(LA.AlignedRecording(out[k], dist[k], ops[k], len(hyp[k]), len(ids)))
    if st is None:
        return result
    segs, L = st['segs'], model.cfg.max_len
    timed = [None] * len(segs)  # per segment [(start_s, end_s, confidence)] of its span's characters
    scored = set()
    for c0 in range(0, len(st['todo']), int(batch_size)):
        idx = st['todo'][c0:c0 + int(batch_size)]
        sel = torch.tensor(idx, dtype=torch.int64, device=eng.device)
        seg_fb, seg_frames = eng.gather_segments(st['fb'], st['src'][sel], st['starts'][sel], st['lens'][sel],
                                                 t_seg=max(st['lens_h'][i] for i in idx))
        feat, flen = eng.features(seg_fb, seg_frames, eps=1e-6)
        flen = flen.cpu()
        data = [feat[i, :int(flen[i])] for i in range(len(idx))]
        toks = []
        for i in idx:
            k, lo, hi = spans[i]
            toks.append(ref[k][0][lo:hi] if hi - lo <= L else [])  # (L tokens: scored without the eos)
        if not any(toks):
            continue
        tgt = np.zeros((len(idx), L), np.int32)
        for j, t in enumerate(toks):
            tgt[j, :len(t)] = t
        _, _, td = model._run(data, flen, lambda: model._timed(tgt, [len(t) for t in toks]))
        for j, (i, sp) in enumerate(zip(idx, model._spans(td, toks, i2w))):
            if toks[j]:
                t0 = segs[i].start_s
                timed[i] = [(t0 + x[0], t0 + x[1], x[3]) for x in sp]
                scored.add(i)
    for i, s in enumerate(segs):
        k, lo, hi = spans[i]
        if hi > lo and i not in scored:
            s.interpolated = True
            timed[i] = LA.interpolate(hi - lo, s.start_s, s.end_s)
        s.chars = LA.span_chars(texts[k], ref[k][1], lo, hi, timed[i], s.start_s)
        conf = [c[3] for c in s.chars if c[3] is not None]
        s.score = float(np.mean(np.log(conf))) if conf and min(conf) > 0 else 0.0
    return result


class ASR:
    """main.py:68-102."""

    def __init__(self, lm_path=None, bw=None, ckpt='./pretrain-0.06328.ckpt', lm_backend="kenlm", fusion=False,
                 hotwords=None, hotword_boost=1.0, bias_weight=1.0, grammar=None):
        """lm_backend "kenlm" (default: the reference's import) or "casr": the library's own ARPA
        n-gram LM (casr.ngram.NgramLM), rescored on the device; with ``fusion`` (the "casr" backend
        only) fused into the beam's first pass instead (Model.eval_one_batch_with_beam).
        ``hotwords``: a list of phrases, or a text file with one phrase per line and an optional boost
        in nats per token after it (casr.bias.read_hotwords; ``hotword_boost`` serves the others): the
        beam search favours them (needs ``bw``).
        ``grammar``: a casr.grammar.Grammar, a list of phrases, or a text file with one phrase per line:
        every answer of __call__ is then one of its sentences (needs ``bw``; not together with hotwords)."""
        self.fusion = bool(fusion)
        if lm_backend not in ("kenlm", "casr"):
            raise ValueError(f"lm_backend must be 'kenlm' or 'casr', got {lm_backend!r}")
        want_lm = lm_path is not None and bw is not None and bw > 1
        if want_lm and lm_backend == "kenlm":
            import kenlm  # third-party (model.py:13); absent here -> ImportError like the reference
            print('loading language model...')
            ts = time()
            lm_model = kenlm.LanguageModel(lm_path)
            print('loading cost %.3fs' % (time() - ts))
        else:
            lm_model = None
        model = Model()
        model.load(ckpt)
        model.model.eval()
        self.audio_base = AudioBase()
        if want_lm and lm_backend == "casr":
            from casr.ngram import NgramLM
            print('loading language model...')
            ts = time()
            lm_model = NgramLM(lm_path, self.audio_base.word2int, model.cfg.vocab)
            print('loading cost %.3fs' % (time() - ts))
        self.lm_model = lm_model
        self.model = model
        self.bw = bw
        self.bias, self.bias_weight = None, float(bias_weight)
        if hotwords is not None:
            from casr.bias import PhraseBias
            if bw is None:
                raise ValueError("hotwords need a beam search: pass bw")
            self.bias = PhraseBias.coerce(hotwords, self.audio_base.word2int, model.cfg.vocab, hotword_boost)
        self.grammar = None
        if grammar is not None:
            from casr.grammar import Grammar
            if bw is None:
                raise ValueError("a grammar needs a beam search: pass bw")
            if hotwords is not None:
                raise ValueError("grammar and hotwords exclude each other")
            self.grammar = Grammar.coerce(grammar, self.audio_base.word2int, model.cfg.vocab, model.cfg.eos)

    def __call__(self, path):
        return parse(path, self.model, self.audio_base, self.lm_model, self.bw, fusion=self.fusion, bias=self.bias,
                     bias_weight=self.bias_weight, grammar=self.grammar)

    def transcribe(self, path, params=None):
        """A recording of any length -> its text: the segments' texts of transcribe(), joined."""
        segs = transcribe([path], self.model, self.audio_base, self.lm_model, self.bw, params=params,
                          fusion=self.fusion, bias=self.bias, bias_weight=self.bias_weight)[0]
        return ''.join(s.text for s in segs)

    def align(self, path, text, params=None):
        """A recording of any length and the text spoken in it -> align_long's result for it: the
        segments with the transcript's characters timed, and the decode's character errors."""
        return align_long([path], [text], self.model, self.audio_base, params=params, bw=self.bw,
                          lm_model=self.lm_model, fusion=self.fusion, bias=self.bias, bias_weight=self.bias_weight)[0]

    def subtitles(self, path, fmt="srt", params=None, text=None):
        """A recording of any length -> its subtitles as SubRip ("srt") or WebVTT ("vtt") text: the
        segments of transcribe(timestamps=True), one cue each, split between characters while a cue
        is too long (casr.subtitles.cues).  With ``text``, the transcript known to be spoken, the cues
        carry that text, timed by align()."""
        from casr import subtitles
        if fmt not in ("srt", "vtt"):
            raise ValueError(f"fmt must be 'srt' or 'vtt', got {fmt!r}")
        if text is not None:
            cue_list = subtitles.cues(self.align(path, text, params=params))
            return subtitles.to_srt(cue_list) if fmt == "srt" else subtitles.to_vtt(cue_list)
        segs = transcribe([path], self.model, self.audio_base, self.lm_model, self.bw, params=params,
                          fusion=self.fusion, bias=self.bias, bias_weight=self.bias_weight, timestamps=True)[0]
        cue_list = subtitles.cues(segs)
        return subtitles.to_srt(cue_list) if fmt == "srt" else subtitles.to_vtt(cue_list)


if __name__ == '__main__':
    gpd['verbose'] = False
    gpd['temperature'] = 1
    asr = ASR(bw=int(sys.argv[2]) if len(sys.argv) > 2 else None,
              ckpt=os.environ.get('CASR_CKPT', './pretrain-0.06328.ckpt'))
    print(asr(sys.argv[1]))
