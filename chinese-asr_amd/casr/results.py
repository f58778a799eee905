"""Host-side result assembly with the reference's exact finalize rules.

The device returns integer token arrays and float32 scores; this module turns them into the
reference's Python results: greedy (model.py:582-602), beam first-max / second-pass
selection (parse_finished_tensors, model.py:708-765) and the unfinished fallback
(model.py:961-972).  Also the reference's record types (util.py:2403-2406)."""
from collections import namedtuple

import numpy as np

# timing (this path's own addition, None unless a decode is asked for timestamps): per utterance one
# (start_s, end_s, peak_s, confidence) per character of pred_text (token_spans)
EvalOutput = namedtuple('EvalOutput', ('pred_text', 'score', 'text', 'wer', 'n', 'alignment',
                                       'audio_feat_len', 'text_len', 'timing'), defaults=(None,))
EncoderOutput = namedtuple('EncoderOutput', ('out', 'out_lens', 'state'))


class BeamEvalOutput(EvalOutput):
    """An EvalOutput (the same nine fields, unpacking the same) of eval_one_batch_with_beam called with
    ``nbest`` or ``alternatives``, carrying two attributes more: ``nbest``, per utterance [(text, comb)]
    best first, and ``alternatives``, per utterance confusion_slots' list of slots (each None when it was
    not asked for).  An utterance that finished no hypothesis has [] in both.  Built like an EvalOutput,
    the two attributes by keyword; pickle, copy and _replace keep them."""
    nbest = None
    alternatives = None

    def __new__(cls, *fields, nbest=None, alternatives=None, **named):
        self = super().__new__(cls, *fields, **named)
        self.nbest = nbest
        self.alternatives = alternatives
        return self

    def __reduce__(self):
        return _beam_eval_output, (tuple(self), self.nbest, self.alternatives)

    def _replace(self, **kwds):
        nbest = kwds.pop('nbest', self.nbest)
        alternatives = kwds.pop('alternatives', self.alternatives)
        return type(self)(*EvalOutput._replace(EvalOutput._make(self), **kwds), nbest=nbest, alternatives=alternatives)


def _beam_eval_output(fields, nbest, alternatives):
    return BeamEvalOutput(*fields, nbest=nbest, alternatives=alternatives)


DecoderOutput = namedtuple('DecoderOutput', ('logit', 'attn_hidden_state', 'alignment', 'cell_state'))
# Model.score_one_batch (teacher-forced scoring; no reference counterpart)
ScoreOutput = namedtuple('ScoreOutput', ('token_logp', 'score', 'loss', 'best_text', 'times', 'token_loss', 'ids',
                                         'tgt_len'))


def edit_distance(a, b):
    """Levenshtein distance (the reference calls python-Levenshtein, util.py:237-262)."""
    m, n = len(a), len(b)
    if m == 0:
        return n
    if n == 0:
        return m
    prev = list(range(n + 1))
    for i in range(1, m + 1):
        cur = [i] + [0] * n
        ai = a[i - 1]
        for j in range(1, n + 1):
            cur[j] = prev[j - 1] if ai == b[j - 1] else 1 + min(prev[j - 1], prev[j], cur[j - 1])
        prev = cur
    return prev[n]


def edit_ops(pred, ref):
    """(insert, delete, replace) counts of one minimal edit script turning ``pred`` into ``ref``
    (python-Levenshtein ``editops(pred, ref)`` semantics, util.py:250-256).  The total always equals
    the distance; how it splits into the three kinds depends on the backtrace's tie order, which
    here prefers replace, then delete, then insert.  python-Levenshtein is absent (no fixture):
    the split is parity-unpinned, the total is exact."""
    m, n = len(pred), len(ref)
    d = np.zeros((m + 1, n + 1), np.int64)
    d[:, 0] = np.arange(m + 1)
    d[0, :] = np.arange(n + 1)
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            d[i, j] = d[i - 1, j - 1] if pred[i - 1] == ref[j - 1] else \
                1 + min(d[i - 1, j - 1], d[i - 1, j], d[i, j - 1])
    i, j, ins, dele, rep = m, n, 0, 0, 0
    while i > 0 or j > 0:
        if i > 0 and j > 0 and pred[i - 1] == ref[j - 1] and d[i, j] == d[i - 1, j - 1]:
            i, j = i - 1, j - 1
        elif i > 0 and j > 0 and d[i, j] == d[i - 1, j - 1] + 1:
            rep += 1
            i, j = i - 1, j - 1
        elif i > 0 and d[i, j] == d[i - 1, j] + 1:
            dele += 1
            i -= 1
        else:
            ins += 1
            j -= 1
    return ins, dele, rep


def get_wer(pred, ref, normalize=True, return_tuple=False):
    """util.py:237-262: distance(pred, ref) [/ len(ref)]; return_tuple: (all, insert, delete,
    replace) [/ len(ref)] from the edit script (edit_ops)."""
    n = len(ref) * 1.
    if not return_tuple:
        r = edit_distance(pred, ref)
        return r / n if normalize else r
    ins, dele, rep = edit_ops(pred, ref)
    r = (ins + dele + rep, ins, dele, rep)
    return tuple(e / n for e in r) if normalize else r


def _symbol_rows(seqs):
    """Sequences -> (rows [n, L] int32 padded with 0, L at least 1; lens [n] int32).  A string becomes
    its UTF-32 code points; anything else is taken as a list of int32 ids."""
    rows = [np.frombuffer(s.encode('utf-32-le', 'surrogatepass'), dtype='<i4') if isinstance(s, str)
            else np.asarray(s, dtype=np.int32).reshape(-1) for s in seqs]
    lens = np.array([len(r) for r in rows], np.int32)
    out = np.zeros((len(rows), max([1] + lens.tolist())), np.int32)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out, lens


def wer_batch(preds, refs, normalize=True, return_tuple=False, engine=None):
    """``[get_wer(p, r, normalize, return_tuple) for p, r in zip(preds, refs)]`` in one call of the HIP
    library: the same Python values (the same integer over the same ``len(ref) * 1.``, the same
    ZeroDivisionError for an empty reference under ``normalize``).  Strings are compared by code
    point, id lists by id.  With an ``engine`` (casr.engine.Engine) and every row within
    casr.lib.EDIT_MAX_LEN symbols the pairs go to the device (casr_edit_distance), else to the host
    entry (casr_edit_distance_host)."""
    from . import lib as _lib
    preds, refs = list(preds), list(refs)
    n = min(len(preds), len(refs))  # (zip's rule)
    a, a_len = _symbol_rows(preds[:n])
    b, b_len = _symbol_rows(refs[:n])
    if engine is not None and n and max(a.shape[1], b.shape[1]) <= _lib.EDIT_MAX_LEN:
        r = engine.edit_distance(a, a_len, b, b_len, ops=return_tuple)
        dist, ops = (r[0].cpu().numpy(), r[1].cpu().numpy()) if return_tuple else (r.cpu().numpy(), None)
    else:
        r = _lib.edit_distance_host(a, a_len, b, b_len, ops=return_tuple)
        dist, ops = r if return_tuple else (r, None)
    out = []
    for i, d in enumerate(dist.tolist()):
        m = int(b_len[i]) * 1.
        if not return_tuple:
            out.append(d / m if normalize else d)
            continue
        ins, dele, rep = ops[i].tolist()
        t = (ins + dele + rep, ins, dele, rep)
        out.append(tuple(e / m for e in t) if normalize else t)
    return out


def wer_long(hyps, refs, engine=None):
    """(distance, insert, delete, replace) of every (hyp, ref) pair, as integers, for texts of any
    length up to casr.lib.EDIT_ALIGN_MAX_LEN symbols: ``wer_batch(.., normalize=False,
    return_tuple=True)`` without its limit of casr.lib.EDIT_MAX_LEN on the device.  With an ``engine``
    the pairs go to the device in one call (casr_edit_align without its maps), else, or past the
    device's limits, to the host entry (casr_edit_align_host)."""
    from . import lib as _lib
    hyps, refs = list(hyps), list(refs)
    n = min(len(hyps), len(refs))
    a, a_len = _symbol_rows(hyps[:n])
    b, b_len = _symbol_rows(refs[:n])
    if engine is not None and n and _lib.edit_align_plan(a.shape[1], b.shape[1], n)["ok"]:
        r = engine.edit_align(a, a_len, b, b_len, ops=True, maps=False)
        dist, ops = r["dist"].cpu().numpy(), r["ops"].cpu().numpy()
    else:
        r = _lib.edit_align_host(a, a_len, b, b_len)
        dist, ops = r["dist"], r["ops"]
    return [(int(d),) + tuple(int(x) for x in o) for d, o in zip(dist.tolist(), ops.tolist())]


def greedy_outputs(tokens, out_len, finished, accum):
    """model.py:582-593.  Host numpy inputs.  Returns (token lists, scores)."""
    toks = [tokens[b, :out_len[b]].tolist() for b in range(tokens.shape[0])]
    score = []
    for b, t in enumerate(toks):
        if len(t) == 0:
            score.append(0.0)
        else:
            score.append(float(accum[b]) / (int(out_len[b]) + int(finished[b])))
    return toks, score


def greedy_steps(out_len, finished, max_len):
    """Iterations the reference loop runs (model.py:578 breaks once all are finished)."""
    if len(finished) and bool(np.all(finished)):
        return int(np.max(out_len)) + 1
    return max_len


def records_by_utterance(rec_tokens, rec_score, rec_valid):
    """Finished hypotheses per utterance in the reference's list order (step, then rank):
    b -> [(tokens, score)] (model.py:715-733)."""
    bs, ls, cs = np.nonzero(rec_valid)  # row-major: already in (utterance, step, rank) order
    scores = rec_score[bs, ls, cs].tolist()
    # token lists converted per step, only the l tokens a step-l record holds
    toks = [None] * len(bs)
    for l in np.unique(ls).tolist():
        sel = np.nonzero(ls == l)[0]
        rows = rec_tokens[bs[sel], l, cs[sel], :l].tolist()
        for i, t in zip(sel.tolist(), rows):
            toks[i] = t
    res = {}
    for b, t, s in zip(bs.tolist(), toks, scores):
        res.setdefault(b, []).append((t, s))
    return res


def second_pass_select(records, int2word, lm_model, lm_weight, length_weight):
    """parse_finished_tensors with second_pass (model.py:749-763): for > 1 finished
    hypotheses pick argmax(logp + lm_w * LM(' '.join(words), bos=True) + len_w * len);
    returns the original (tokens, logp)."""
    out = {}
    for b, v in records.items():
        if len(v) == 1:
            out[b] = v[0]
            continue
        word = int2word.__getitem__
        lm = [lm_model.score(' '.join(map(word, t)), bos=True) for t, _ in v]
        comb = [s + lm_weight * q + length_weight * len(t) for (t, s), q in zip(v, lm)]
        out[b] = v[int(np.argmax(comb))]
    return out


def _word_array(int2word, n):
    """int2word as an object array over ids 0 .. n - 1 (the word strings themselves, not copies),
    or None when the mapping does not cover that range."""
    try:
        return np.array([int2word[i] for i in range(n)] + [None], dtype=object)[:n]
    except (KeyError, IndexError, TypeError):
        return None


def second_pass_arrays(rec_tokens, rec_score, rec_valid, int2word, lm_model, lm_weight, length_weight):
    """second_pass_select(records_by_utterance(rec_tokens, rec_score, rec_valid), ...) from the record
    arrays directly: the same choice per utterance with records (model.py:749-763) and the same
    returned (tokens, logp), the LM called with the same sentences in the same order, but without
    a Python token list per record (the words come from one object-array gather, and only the
    chosen records become lists).  Falls back to the list form when int2word does not cover the
    token ids."""
    bs, ls, cs = np.nonzero(rec_valid)
    if len(bs) == 0:
        return {}
    full = rec_tokens[bs, ls, cs]  # [n][L]: the records' token rows, in (utterance, step, rank) order
    used = full[np.arange(full.shape[1])[None, :] < ls[:, None]]  # the l tokens of each step-l record
    warr = _word_array(int2word, int(used.max()) + 1) if used.size else np.array([], dtype=object)
    if warr is None or (used.size and int(used.min()) < 0):
        return second_pass_select(records_by_utterance(rec_tokens, rec_score, rec_valid), int2word, lm_model,
                                  lm_weight, length_weight)
    full = np.where(np.arange(full.shape[1])[None, :] < ls[:, None], full, 0)  # (slots past l unused)
    scores = rec_score[bs, ls, cs].tolist()
    lens = ls.tolist()
    starts = np.flatnonzero(np.r_[True, bs[1:] != bs[:-1]]).tolist() + [len(bs)]
    words = None
    out = {}
    for a, z in zip(starts[:-1], starts[1:]):
        b = int(bs[a])
        if z - a == 1:
            out[b] = (full[a, :lens[a]].tolist(), scores[a])
            continue
        if words is None:
            words = warr[full] if len(warr) else np.empty(full.shape, dtype=object)
        rows = words[a:z].tolist()
        lm = [lm_model.score(' '.join(row[:l]), bos=True) for row, l in zip(rows, lens[a:z])]
        comb = [sc + lm_weight * q + length_weight * l for sc, q, l in zip(scores[a:z], lm, lens[a:z])]
        i = a + int(np.argmax(comb))
        out[b] = (full[i, :lens[i]].tolist(), scores[i])
    return out


# ------------------------------------------------------------------ teacher-forced scoring (Engine.score)
def encode_targets(texts, word2int, eos, unk, V=None, max_len=None):
    """Transcripts (strings or lists of words) -> (ids [B, L] int32 padded with 0, lens [B] int32).
    Unknown words become ``unk``; ``eos`` (None: nothing) is appended to every transcript, so it is
    scored as the reference's targets are (data.py:192-193).  L is the longest row (at least 1).
    An id outside [0, V) raises ValueError here, on the host, instead of the device's clamp and
    guard bit (V defaults to one past the largest id of word2int); so does a row longer than
    ``max_len``."""
    V = (max(word2int.values()) + 1 if word2int else 0) if V is None else int(V)
    rows = []
    for t in texts:
        ids = [word2int.get(w, unk) for w in t]
        if eos is not None:
            ids.append(eos)
        rows.append(ids)
    for b, ids in enumerate(rows):
        bad = [i for i in ids if not (isinstance(i, (int, np.integer)) and 0 <= i < V)]
        if bad:
            raise ValueError(f"transcript {b}: token id {bad[0]} outside [0, {V})")
        if max_len is not None and len(ids) > max_len:
            raise ValueError(f"transcript {b}: {len(ids)} tokens > max_len {max_len}")
    L = max([len(r) for r in rows] + [1])
    out = np.zeros((len(rows), L), np.int32)
    for b, ids in enumerate(rows):
        out[b, :len(ids)] = ids
    return out, np.array([len(r) for r in rows], np.int32)


def score_outputs(token_logp, tgt_len, finished):
    """Per-utterance totals of a teacher-forced pass, and the score in the form greedy decoding
    reports (model.py:593): sum / (len + finished), where tgt_len = len + finished counts the
    scored eos of a finished hypothesis, and 0.0 for an empty transcript (len == 0), as
    greedy_outputs.  Host numpy inputs; returns (totals float32 [B], scores list[float])."""
    token_logp = np.asarray(token_logp, np.float32)
    tgt_len = np.asarray(tgt_len).astype(np.int64)
    fin = np.asarray(finished).astype(np.int64)
    totals = np.zeros(token_logp.shape[0], np.float32)
    score = []
    for b in range(token_logp.shape[0]):
        acc = np.float32(0.0)
        for l in range(int(tgt_len[b])):  # ascending, f32: the device's total_logp
            acc = np.float32(acc + token_logp[b, l])
        totals[b] = acc
        n = int(tgt_len[b]) - int(fin[b])
        score.append(0.0 if n <= 0 else float(acc) / (n + int(fin[b])))
    return totals, score


def label_smoothed_loss(token_logp, mean_logp, tgt_len, V, ls):
    """util.py:265-279 per scored token, from the two log-probability terms the device returns:
    with lp_t = logit_t - lse and mean_logp = sum(logits) / V - lse,
        loss = -[(1 - ls) lp_t + ls / (V - 1) (V mean_logp - lp_t)]
    (the reference's (1 - ls) logit_t + ls / (V - 1) (sum(logits) - logit_t) - lse, negated).
    Returns float32 [B, L], 0 past tgt_len; the reference's criterion then takes the mean over the
    scored tokens."""
    lp = np.asarray(token_logp, np.float64)
    mp = np.asarray(mean_logp, np.float64)
    loss = -((1.0 - ls) * lp + (ls / (V - 1)) * (V * mp - lp))
    mask = np.arange(lp.shape[1])[None, :] < np.asarray(tgt_len).reshape(-1, 1)
    return np.where(mask, loss, 0.0).astype(np.float32)


def token_times(align, enc_lens, tgt_len, sample_rate=16000):
    """Where each scored token sits in the audio, from the attention weights of a teacher-forced
    pass: align [L, Tp, B] (Engine.score(alignment=True)), enc_lens [B] encoder frames per
    utterance, tgt_len [B].  Per scored token: ``frame`` the attention's argmax frame (the first of
    equal maxima) and ``expect`` the expectation sum_t t alpha_t, both over the utterance's own
    frames; ``frame_s`` / ``expect_s`` the same in seconds (one encoder frame = 3 stacked frames x
    160 samples = 30 ms at 16 kHz).  Arrays [B, L]; positions past tgt_len hold -1 / 0."""
    align = np.asarray(align)
    L, _, B = align.shape
    frame = np.full((B, L), -1, np.int64)
    expect = np.zeros((B, L), np.float64)
    for b in range(B):
        n, T = min(int(tgt_len[b]), L), int(enc_lens[b])
        if n == 0 or T == 0:
            continue
        a = align[:n, :T, b].astype(np.float64)
        frame[b, :n] = a.argmax(axis=1)
        expect[b, :n] = a @ np.arange(T, dtype=np.float64)
    sec = 3 * 160 / float(sample_rate)
    return dict(frame=frame, expect=expect, frame_s=np.where(frame >= 0, frame * sec, 0.0), expect_s=expect * sec)


def token_spans(first, last, peak, token_logp, tgt_len, sample_rate=16000, n_tokens=None):
    """Per-token times and confidences from the monotone attention path (Engine.align_path /
    casr.lib.align_path_host: first, last, peak [B, L] encoder frames) and the teacher-forced
    log-probabilities of the same pass (token_logp [B, L]); tgt_len [B] the scored positions.  Per
    utterance a list of (start_s, end_s, peak_s, confidence): start_s = first x 0.03, end_s = (last + 1)
    x 0.03, peak_s = peak x 0.03 (one encoder frame = 3 stacked frames x 160 samples = 30 ms at 16 kHz),
    confidence = exp(token_logp).  ``n_tokens`` [B] (default tgt_len) is how many positions are listed:
    a closing eos is scored and takes part in the path, where it absorbs the trailing quiet, but is not
    listed.  The spans tile the utterance, so token 0's span absorbs the leading quiet the same way:
    start_s / end_s say which stretch of audio a token owns, peak_s (the frame of its span the
    attention weighs most) is the robust instant of the token itself."""
    first, last, peak = (np.asarray(x) for x in (first, last, peak))
    token_logp = np.asarray(token_logp, np.float64)
    sec = 3 * 160 / float(sample_rate)
    n_tokens = tgt_len if n_tokens is None else n_tokens
    out = []
    for b in range(first.shape[0]):
        n = min(int(n_tokens[b]), int(tgt_len[b]), first.shape[1])
        out.append([(float(first[b, l] * sec), float((last[b, l] + 1) * sec), float(peak[b, l] * sec),
                     float(np.exp(token_logp[b, l]))) for l in range(n) if first[b, l] >= 0])
    return out


def confusion_slots(slot_token, slot_mass, n_slots, total, int2word, min_gap=0.05):
    """The confusion network of Engine.beam_confusion / casr.lib.confusion_host (host numpy arrays) as
    lists: per utterance a list of slots in the pivot's order, each slot [(char, prob)] by falling
    posterior, prob = mass / U and '' for "nothing here" (EPS).  Every slot of a pivot character is kept;
    a gap slot only where the mass of its tokens other than EPS is at least ``min_gap`` U.  That mass is
    exact where EPS is among the M listed entries or fewer than M are listed.  Else EPS weighs at most the
    last listed entry, and the larger of the listed sum and U less that entry stands for it, a lower bound:
    such a gap (M or more distinct inserts, each outweighing EPS) can be dropped though its tokens together
    reach ``min_gap`` U; a larger M lists EPS.  An utterance without a pivot gives []."""
    out = []
    for b in range(len(n_slots)):
        U = int(total[b])
        slots = []
        for s in range(int(n_slots[b])):
            ent = [(int(t), int(w)) for t, w in zip(slot_token[b, s], slot_mass[b, s]) if t != -2 and w > 0]
            if s % 2 == 0:
                eps = [w for t, w in ent if t == -1]
                other = U - eps[0] if eps else max(sum(w for _, w in ent), U - ent[-1][1]) if ent else 0
                if not ent or other <= 0 or other < min_gap * U:
                    continue
            slots.append([('' if t == -1 else int2word[t], w / U) for t, w in ent])
        out.append(slots)
    return out
