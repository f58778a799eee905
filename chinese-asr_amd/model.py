"""Drop-in for the reference ``Model`` (model.py:18-987) on the MI355X path.

Same constructor, ``load``/``save``, ``eval_one_batch_with_greedy`` and
``eval_one_batch_with_beam`` signatures and ``EvalOutput`` results; the encoder, attention,
decoder and the decode loops run as HIP kernels behind the casr C-ABI (include/casr.h).
The reference builds nn.Modules; here ``model.model`` only provides ``eval()`` (main.py:90)
and ``model.decoder.real_vcb_sz`` (model.py:623) for callers that read them.
"""
import numpy as np
import torch

from gpd import gpd
from casr.config import config_from_gpd
from casr.engine import Engine
from casr.lib import pack_weights
from casr.ngram import NgramLM
from casr.results import (BeamEvalOutput, EvalOutput, ScoreOutput, confusion_slots, encode_targets, get_wer,
                          greedy_outputs, greedy_steps, label_smoothed_loss, score_outputs, second_pass_arrays,
                          token_spans, token_times, wer_batch)
from casr.vocab import load_vocab
from casr.weights import check_state_dicts, load_checkpoint, save_checkpoint, synthetic_state_dicts


class _ModuleList(object):
    """Stands in for ``nn.ModuleList([encoder, decoder])`` (model.py:78-81): inference only."""

    def eval(self):
        return self

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("the MI355X casr path is inference-only")
        return self


class _DecoderInfo(object):
    def __init__(self, cfg):
        self.vocab_size = cfg.max_num_words
        self.real_vcb_sz = cfg.vocab
        self.hidden_size = cfg.dec_hidden
        self.embed_dim = cfg.embed_dim


class _EncoderInfo(object):
    def __init__(self, cfg):
        self.enc_size = cfg.enc_size
        self.num_directions = 2


class Model(object):
    def __init__(self):
        self.cfg = config_from_gpd(gpd)
        if not torch.cuda.is_available():
            raise RuntimeError("casr Model runs on an MI355X GPU; none is visible")
        self.device = torch.device('cuda', torch.cuda.current_device())
        # the reference starts from random init (init_rnn, util.py:90-114); this path starts
        # from the deterministic synthetic recipe until load() replaces it
        self.enc_sd, self.dec_sd = synthetic_state_dicts(self.cfg, peaked=False)
        self.engine = Engine(self.cfg, self.enc_sd, self.dec_sd, device=self.device)
        self.encoder = _EncoderInfo(self.cfg)
        self.decoder = _DecoderInfo(self.cfg)
        self.model = _ModuleList()
        self.optimizer = None
        # eval_one_batch_with_beam(timestamps=True): [B] bool, the utterances whose beam finished no
        # hypothesis (the handle's beam state cannot be asked afterwards); None after any other decode
        self.beam_unfinished = None
        self._default_int2word = None

    # ------------------------------------------------------------------ weights
    def load_state_dicts(self, enc_sd, dec_sd):
        check_state_dicts(self.cfg, enc_sd, dec_sd)
        self.enc_sd, self.dec_sd = enc_sd, dec_sd
        self.engine.bind(pack_weights(self.cfg, enc_sd, dec_sd))

    def load(self, path):
        """model.py:357-370."""
        if gpd['verbose']:
            print(f'[INFO] Loading weights from {path}...', end='')
        enc_sd, dec_sd, args = load_checkpoint(path)
        self.load_state_dicts(enc_sd, dec_sd)
        if gpd['verbose']:
            print(' Loading done.')
        return args

    def save(self, args, path):
        """model.py:347-355."""
        save_checkpoint(path, self.enc_sd, self.dec_sd, args)

    # ------------------------------------------------------------------ helpers
    def _int2word(self, int2word):
        if int2word is not None:
            return int2word
        if self._default_int2word is None:
            self._default_int2word = load_vocab()[1]
        return self._default_int2word

    def _gather(self, data, lens):
        lens = torch.as_tensor(lens)
        if isinstance(data, (list, tuple)):
            feat, lens_d = self.engine.gather(list(data), lens)
        else:  # already padded [B, Tp, feat_dim]
            feat, lens_d = data.to(self.device, torch.float32), lens.to(self.device, torch.int32)
        return feat, lens_d, lens

    def _run(self, data, lens, decode):
        """encode + decode with the device guard bits checked (Engine.run_checked): a hand-off
        timeout raises, an s16x3 range overflow re-runs the batch on the exact-f32 path."""
        feat, lens_d, lens = self._gather(data, lens)
        out, _ = self.engine.run_checked(lambda: self.engine.encode(feat, lens_d), decode)
        return feat.shape[0], lens, out

    # ------------------------------------------------------------------ character timestamps
    def _timed(self, tokens, length):
        """Times of a decode's chosen tokens, on the encode the handle still holds: the tokens
        [B, max_len] with their lengths [B] are scored teacher-forced (casr_score; an eos appended
        where length < max_len, so the path has a row for the trailing quiet) and the monotone path
        runs through that pass's attention (casr_align_path).  Device tensors; nothing is read back."""
        L, dev = self.cfg.max_len, self.engine.device
        tokens = torch.as_tensor(tokens).to(dev, torch.int32)
        n = torch.as_tensor(length).to(dev, torch.int32)
        pos = torch.arange(L, device=dev, dtype=torch.int32)[None, :]
        tgt = torch.where(pos == n[:, None], torch.full_like(tokens, self.cfg.eos), tokens)
        tgt_len = torch.clamp(n + 1, max=L)
        sc = self.engine.score(tgt, tgt_len, alignment=True)
        ap = self.engine.align_path(sc['alignment'], self.engine._lens, tgt_len)
        return dict(ap, token_logp=sc['token_logp'], tgt_len=tgt_len, n_tokens=n)

    def _with_timing(self, r, timestamps):
        """r (a decode's dict with tokens and length / out_len) plus, when asked, its 'timing'.  The
        scoring pass reuses the decode workspace, so a beam's state is spent after it (beam_records,
        a rescore or an MBR choice would read a cleared step count): what main.transcribe wants from
        it, which utterances finished no hypothesis, is taken first ('unfinished', [B] bool)."""
        if not timestamps:
            return r
        if 'length' in r:
            r = dict(r, unfinished=~self.engine.beam_records()[2].flatten(1).bool().any(1))
        return dict(r, timing=self._timed(r['tokens'], r['length'] if 'length' in r else r['out_len']))

    def _spans(self, timed, toks, i2w):
        """_timed's tensors -> per utterance one token_spans tuple per character of the predicted text
        (a token whose word has several characters lends each of them its span)."""
        if timed is None:
            return None
        h = {k: v.cpu().numpy() for k, v in timed.items()}
        spans = token_spans(h['first'], h['last'], h['peak'], h['token_logp'], h['tgt_len'],
                            gpd.get('sample_rate', 16000), n_tokens=h['n_tokens'])
        return [[sp for e, sp in zip(t, row) for _ in i2w[e]] for t, row in zip(toks, spans)]

    # ------------------------------------------------------------------ decode
    @torch.no_grad()
    def eval_one_batch_with_greedy(self, device, data, lens, int2word=None, text=None, timestamps=False):
        """model.py:503-602.  ``timestamps`` (this path's own addition, default off: nothing else is
        launched): the result's ``timing`` holds per utterance one (start_s, end_s, peak_s, confidence)
        per character of pred_text (casr.results.token_spans), from the monotone path through the
        attention of a teacher-forced pass over the decoded tokens."""
        self.model.eval()
        bsz, lens, out = self._run(data, lens,
                                   lambda: self._with_timing(self.engine.greedy(alignment=True), timestamps))
        tokens = out['tokens'].cpu().numpy()
        out_len = out['out_len'].cpu().numpy()
        fin = out['finished'].cpu().numpy().astype(bool)
        accum = out['accum'].cpu().numpy()
        toks, score = greedy_outputs(tokens, out_len, fin, accum)
        steps = greedy_steps(out_len, fin, self.cfg.max_len)
        alignments = [out['alignment'][l] for l in range(steps)]
        i2w = self._int2word(int2word)
        pred_text = ['' if len(t) == 0 else ''.join([i2w[e] for e in t]) for t in toks]
        wer = None
        if text is not None:
            text = [''.join([i2w[e] for e in ele]) for ele in text]
            wer = np.mean(wer_batch(pred_text, text, engine=self.engine))
        return EvalOutput(pred_text=pred_text, score=score, text=text, wer=wer, n=bsz, alignment=alignments,
                          audio_feat_len=lens, text_len=out['out_len'], timing=self._spans(out.get('timing'), toks, i2w))

    @torch.no_grad()
    def eval_one_batch_with_beam(self, device, bmsz, data, lens, text, int2word,
                                 second_pass=gpd['second_pass'], lm_model=None,
                                 lm_weight=gpd['lm_weight'], length_weight=gpd['length_weight'], fusion=False,
                                 mbr=None, bias=None, bias_weight=1.0, timestamps=False, nbest=None, alternatives=None,
                                 posterior_scale=1.0, grammar=None, grammar_start=None):
        """model.py:604-987.  ``fusion`` (this path's own addition, default off): with an NgramLM as
        ``lm_model`` the LM is fused into the first pass on the device (casr_beam_lm: every candidate
        ranked by logp + lm_weight lm + length_weight (l + 1), the ranking model.py:843-857 was designed
        for) and no second pass runs; ``score`` is the choice's acoustic log-probability.  A duck-typed
        host scorer cannot be fused: TypeError.
        ``mbr`` (this path's own addition, default None: off): a scale >= 0.  The result is the finished
        hypothesis with the lowest expected edit distance to the others under the posterior
        exp(mbr (c - c_max)) (casr_beam_mbr), c the second pass's combined score: with an NgramLM and
        ``second_pass`` the LM enters c, without either c = logp + length_weight len.  ``score`` is the
        choice's first-pass score.  Any other ``lm_model`` cannot be read on the device: TypeError;
        together with ``fusion``: ValueError.
        ``bias`` (this path's own addition, default None: off): a casr.bias.PhraseBias, the hotwords the
        search favours while it searches (casr_beam_bias: a candidate's rank gains bias_weight times the
        boost of the phrases it completes or continues); ``score`` is the choice's acoustic
        log-probability.  With ``fusion`` and an NgramLM the LM is fused as well; otherwise no LM takes
        part in the first pass.  Together with ``mbr``, or with a host second pass (``second_pass`` and
        an ``lm_model`` that is not fused): ValueError.  Both read the records of a plain beam through
        its scores alone (casr_beam_mbr's and the second pass's fallback assume them), so a biased
        search under them would be ranked by one expression and chosen by another.
        ``timestamps`` (this path's own addition, default off: nothing else is launched): ``timing`` as
        eval_one_batch_with_greedy fills it, for the hypothesis that was chosen, whatever chose it.  The
        device-only modes score it inside the guarded decode; after a host second pass the scoring runs
        once the host has chosen, on the encode the handle still holds, and the guard bits are read again.
        ``nbest`` (this path's own addition, default None: off): N in 1..64, the N best finished
        hypotheses per utterance by the combined score c (casr_beam_nbest).  ``alternatives`` (default
        None: off): M in 1..8, per character of the answer, and per gap where something else was likely,
        the M most probable competitors under the posterior exp(posterior_scale (c - c_max)) over the
        finished hypotheses (casr_beam_confusion, a confusion network around the answer).  With either the
        result is a casr.results.BeamEvalOutput: the same nine fields and the attributes ``nbest`` and
        ``alternatives``.  c is what chose the answer: logp alone after a plain first pass, the second pass's
        combined score with an NgramLM and ``second_pass``, ``mbr``'s c with ``mbr`` (the pivot is then the
        MBR choice).  An lm_model that is no NgramLM cannot be read on the device: TypeError; together with
        ``fusion`` or ``bias``: ValueError (both read the records of a plain beam through its scores).  As
        with ``mbr``, no host second pass runs under either keyword: ``second_pass`` with ``lm_model`` None
        keeps the first pass's choice and does not raise the reference's AttributeError.
        ``grammar`` (this path's own addition, default None: off): a casr.grammar.Grammar; every answer is
        then a sentence of it (casr_beam_grammar: only the grammar's continuations are ranked, and every
        hypothesis can still finish before max_len), ``score`` the choice's acoustic log-probability.
        ``grammar_start``: one grammar state per utterance to start in (Grammar.union's), default state 0.
        With ``fusion`` and an NgramLM the LM is fused as well; otherwise no LM takes part.  ``timestamps``
        works as elsewhere.  Together with ``bias``, ``mbr``, ``nbest``, ``alternatives`` or a second pass
        over an ``lm_model`` that is not fused: ValueError (those read a plain beam's tree and scores)."""
        self.model.eval()
        if grammar is not None:
            for name, on in (("bias", bias is not None), ("mbr", mbr is not None), ("nbest", nbest is not None),
                             ("alternatives", alternatives is not None)):
                if on:
                    raise ValueError(f"grammar and {name} exclude each other: {name} reads or ranks a plain beam")
            if second_pass and lm_model is not None and not fusion:
                raise ValueError("grammar with a second pass: fuse the LM (fusion=True with a casr.ngram.NgramLM) "
                                 "or drop it; the second pass rescores a plain beam")
            if fusion and not isinstance(lm_model, NgramLM):
                raise TypeError(f"fusion=True needs a casr.ngram.NgramLM as lm_model, got {type(lm_model).__name__}")
            lm = lm_model if fusion else None
            bsz, _, r = self._run(data, lens, lambda: self._with_timing(
                self.engine.beam_grammar(grammar, bmsz, lm, lm_weight if fusion else 0.0, length_weight,
                                         start=grammar_start), timestamps))
            return self._first_pass_output(bsz, r, text, int2word)
        extras = nbest is not None or alternatives is not None
        if extras:
            if bias is not None or fusion:
                raise ValueError("nbest and alternatives exclude bias and fusion: they read the records of a plain beam")
            if lm_model is not None and not isinstance(lm_model, NgramLM):
                raise TypeError("nbest and alternatives need a casr.ngram.NgramLM as lm_model (or None), got "
                                f"{type(lm_model).__name__}")
        if bias is not None:
            if mbr is not None:
                raise ValueError("bias and mbr exclude each other: the MBR choice reads the records of a plain beam")
            if second_pass and lm_model is not None and not fusion:
                raise ValueError("bias with a second pass: fuse the LM (fusion=True with a casr.ngram.NgramLM) "
                                 "or drop it; the second pass rescores a plain beam")
            if fusion and not isinstance(lm_model, NgramLM):
                raise TypeError(f"fusion=True needs a casr.ngram.NgramLM as lm_model, got {type(lm_model).__name__}")
            lm = lm_model if fusion else None
            bsz, _, r = self._run(data, lens, lambda: self._with_timing(
                self.engine.beam_bias(bias, bmsz, bias_weight, lm, lm_weight, length_weight), timestamps))
            return self._first_pass_output(bsz, r, text, int2word)
        if mbr is not None:
            if fusion:
                raise ValueError("mbr and fusion exclude each other: the MBR choice reads the records of a plain beam")
            if lm_model is not None and not isinstance(lm_model, NgramLM):
                raise TypeError(f"mbr needs a casr.ngram.NgramLM as lm_model (or None), got {type(lm_model).__name__}")
        if fusion:
            if not isinstance(lm_model, NgramLM):
                raise TypeError(f"fusion=True needs a casr.ngram.NgramLM as lm_model, got {type(lm_model).__name__}")
            bsz, _, r = self._run(data, lens, lambda: self._with_timing(
                self.engine.beam_lm(lm_model, bmsz, lm_weight, length_weight), timestamps))
            return self._first_pass_output(bsz, r, text, int2word)
        # an NgramLM (casr/ngram.py) is rescored on the device from the beam tree: no record copy and
        # no host pass; any other lm_model keeps the host second pass below
        on_device = bool(second_pass) and isinstance(lm_model, NgramLM)
        host_pass = bool(second_pass) and not on_device and mbr is None and not extras

        def decode():
            r = self.engine.beam(bmsz, lm_weight, length_weight)
            if mbr is not None:
                r = self.engine.beam_mbr(mbr, lm_model if on_device else None, lm_weight, length_weight)
            elif on_device:
                r = self.engine.beam_rescore(lm_model, lm_weight, length_weight, records=extras)
            if extras:
                # c as the answer was chosen by it: mbr's and the rescore's comb, else the first pass's score
                weighted = mbr is not None or on_device
                kw = dict(rec_lm=r.get('rec_lm'), lm_weight=lm_weight if weighted else 0.0,
                          length_weight=length_weight if weighted else 0.0)
                if nbest is not None:
                    r['nbest'] = self.engine.beam_nbest(nbest, **kw)
                if alternatives is not None:
                    r['confusion'] = self.engine.beam_confusion(alternatives, posterior_scale,
                                                                pivot=r['index'] if mbr is not None else None, **kw)
            return self._with_timing(r, timestamps and not host_pass)

        bsz, _, r = self._run(data, lens, decode)
        self.beam_unfinished = r.get('unfinished')
        second_pass = host_pass
        toks = r['tokens'].cpu().numpy()
        blen = r['length'].cpu().numpy()
        bscore = r['score'].cpu().numpy()
        best = {b: (toks[b, :blen[b]].tolist(), float(bscore[b])) for b in range(bsz)}
        i2w = self._int2word(int2word)
        if second_pass:
            rt, rs, rv = (x.cpu().numpy() for x in self.engine.beam_records())
            if lm_model is None and bool((np.bincount(np.nonzero(rv)[0], minlength=bsz) > 1).any()):
                # the reference calls lm_model.score here (model.py:755) and fails
                raise AttributeError("second_pass=True needs lm_model ('NoneType' object has no attribute 'score')")
            best.update(second_pass_arrays(rt, rs, rv, i2w, lm_model, lm_weight, length_weight))
        pred_text = [''.join([i2w[idx] for idx in best[b][0]]) for b in range(bsz)]
        score = [best[b][1] for b in range(bsz)]
        timed = r.get('timing')
        if timestamps and host_pass:
            rows = np.full((bsz, self.cfg.max_len), -1, np.int32)
            for b in range(bsz):
                rows[b, :len(best[b][0])] = best[b][0]
            self.beam_unfinished = torch.from_numpy(~rv.reshape(bsz, -1).astype(bool).any(axis=1))
            timed = self._timed(torch.from_numpy(rows), torch.tensor([len(best[b][0]) for b in range(bsz)]))
            self.engine.check_flags()
        timing = self._spans(timed, [best[b][0] for b in range(bsz)], i2w)
        if text is not None:
            text = [''.join([i2w[idx] for idx in ele]) for ele in text]
        wer = None
        if text is not None:
            wer = np.mean(wer_batch(pred_text, text, engine=self.engine))
        out = EvalOutput(pred_text=pred_text, score=score, text=text, wer=wer, n=bsz, alignment=None,
                         audio_feat_len=None, text_len=None, timing=timing)
        if not extras:
            return out
        lists = slots = None
        if nbest is not None:
            nb = {n: r['nbest'][n].cpu().numpy() for n in ('index', 'tokens', 'length', 'comb')}
            lists = [[(''.join(i2w[t] for t in nb['tokens'][b, j, :nb['length'][b, j]].tolist()), float(nb['comb'][b, j]))
                      for j in range(nb['index'].shape[1]) if nb['index'][b, j] >= 0] for b in range(bsz)]
        if alternatives is not None:
            cn = {n: r['confusion'][n].cpu().numpy() for n in ('slot_token', 'slot_mass', 'n_slots', 'total')}
            slots = confusion_slots(cn['slot_token'], cn['slot_mass'], cn['n_slots'], cn['total'], i2w)
        return BeamEvalOutput(*out, nbest=lists, alternatives=slots)

    def _first_pass_output(self, bsz, r, text, int2word):
        """The EvalOutput of a beam whose first pass made the choice (beam_lm, beam_bias, beam_grammar)."""
        toks, blen, bscore = (r[n].cpu().numpy() for n in ('tokens', 'length', 'score'))
        self.beam_unfinished = r.get('unfinished')
        i2w = self._int2word(int2word)
        pred_text = [''.join([i2w[idx] for idx in toks[b, :blen[b]].tolist()]) for b in range(bsz)]
        timing = self._spans(r.get('timing'), [toks[b, :blen[b]].tolist() for b in range(bsz)], i2w)
        wer = None
        if text is not None:
            text = [''.join([i2w[idx] for idx in ele]) for ele in text]
            wer = np.mean(wer_batch(pred_text, text, engine=self.engine))
        return EvalOutput(pred_text=pred_text, score=[float(s) for s in bscore], text=text, wer=wer, n=bsz,
                          alignment=None, audio_feat_len=None, text_len=None, timing=timing)

    @torch.no_grad()
    def score_one_batch(self, device, data, lens, text, word2int=None, int2word=None, eos=True):
        """Teacher-forced scoring of given transcripts (the reference's training-time forward,
        model.py:405-469, and its label-smoothed criterion, util.py:265-279, as an evaluation):
        ``text`` one transcript per utterance (a string or a list of words; or lists of ids when
        ``word2int`` is False).  With ``eos`` every transcript is scored with its closing eos.
        Returns a ScoreOutput: token_logp (one list per utterance), score (sum / scored tokens, the
        form greedy reports), loss (label-smoothed with gpd['label_smooth'] if present, else 0: the
        mean over all scored tokens), best_text (the per-step argmax), times (token_times)."""
        self.model.eval()
        if word2int is False:
            w2i = {i: i for i in range(self.cfg.vocab)}
        else:
            w2i = word2int if word2int is not None else load_vocab()[0]
        unk = gpd.get('unk', 3)
        ids, n = encode_targets(text, w2i, self.cfg.eos if eos else None, unk, V=self.cfg.vocab,
                                max_len=self.cfg.max_len)
        bsz, lens, out = self._run(data, lens, lambda: self.engine.score(ids, n, alignment=True, best=True, mean=True))
        lp = out['token_logp'].cpu().numpy()
        fin = np.full(bsz, 1 if eos else 0)
        _, score = score_outputs(lp, n, fin)
        V, ls = self.cfg.vocab, float(gpd.get('label_smooth', 0.0))
        tok_loss = label_smoothed_loss(lp, out['mean_logp'].cpu().numpy(), n, V, ls)
        loss = float(tok_loss.sum(dtype=np.float64) / max(int(n.sum()), 1))
        i2w = self._int2word(int2word)
        bt = out['best_token'].cpu().numpy()
        best_text = [''.join(i2w[int(e)] for e in bt[b, :n[b] - (1 if eos else 0)]) for b in range(bsz)]
        times = token_times(out['alignment'].cpu().numpy(), np.asarray(lens), n, gpd.get('sample_rate', 16000))
        return ScoreOutput(token_logp=[lp[b, :n[b]].tolist() for b in range(bsz)], score=score, loss=loss,
                           best_text=best_text, times=times, token_loss=tok_loss, ids=ids, tgt_len=n)
