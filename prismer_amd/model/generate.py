"""Beam-search and sampled decoding for the caption / VQA heads.

Reference: `self.text_decoder.generate(input_ids=..., encoder_hidden_states=..., num_beams=3, max_length=..., min_length=...,
length_penalty=...)` at model/prismer_caption.py:45-50 and model/prismer_vqa.py:52-58, i.e. transformers' (4.26.1)
beam search: BeamSearchScorer.process / finalize, BeamHypotheses.add / is_done, MinLengthLogitsProcessor.  The reference re-runs
the FULL prefix every step (prepare_inputs_for_generation, roberta.py:401-406, passes no cache).

Here:
  * the decoder runs KV-cached (DecoderProgram.decode_begin / decode / decode_reorder): cross-attention K/V projected once,
    self-attention K/V cached per layer and re-ordered with the beams on the device;
  * with `share_image` the `num_beams` hypotheses of an image share the image's cross-attention K/V (projected for B images, not
    B * num_beams) and the prompt runs once per image: at the first step every beam but the first starts at -1e9 anyway;
  * the beam step runs on the device: `beam_search_device` is `step_fn -> ops.beam_topk -> ops.beam_advance -> reorder_fn`, two library
    calls on device-resident state, no stock torch reduction / sort / top-k / boolean-mask indexing and no host read inside the loop
    but the "all items done?" check every fourth step;
  * `beam_search_from_logits` is the algorithm alone, as tensor ops (any callable that maps the current ids to next-token logits): the
    SPECIFICATION of the device step.  It runs on CPU tensors, which is how tests/test_generate_cpu.py checks it against the loop-form
    oracle (oracle/beam_oracle.py).  On a GPU its boolean-mask indexing synchronises with the device several times per step.

Ties.  `torch.topk` leaves the order of equal candidates undefined, and with bf16 logits exact ties among a row's leaders are common.
The library's rule (ph_beam_topk) is: score descending, then flat index beam * V + token ascending -- `stable_topk` below; pass it
as `topk_fn` to run the specification under that rule.

Semantics kept from transformers 4.26.1 (num_return_sequences = 1, early_stopping = False, do_sample = False):
  - scores of the first step come from beam 0 only (the other beams start at -1e9);
  - EOS is banned while cur_len < min_length; cur_len counts the decoder prompt;
  - per step the best 2*num_beams (beam, token) candidates are visited in score order until num_beams continuing beams are
    found; an EOS candidate becomes a finished hypothesis only if its rank is < num_beams, with score
    sum_logprobs / cur_len ** length_penalty (cur_len = length before the EOS); a batch item keeps its num_beams best hypotheses;
  - an item is done when it holds num_beams hypotheses and the worst of them is at least best_running / cur_len ** length_penalty;
    done items are frozen (padding beams);
  - at max_length the running beams of unfinished items are added as hypotheses; the best hypothesis wins.

Sampling (generate(do_sample=True), the second half of this file): `sample_from_logits` is the specification as tensor ops -- transformers'
MinLengthLogitsProcessor -> TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper -> multinomial and the bookkeeping of _sample,
with three things DEFINED that transformers leaves to its sort: top-p keeps whole classes of equal logit (the boundary tie class stays,
so the kept set is a threshold set; transformers cuts inside it), the draw walks the kept tokens class descending / token id ascending,
and the uniform of (seed, row, position) is a Philox word.  `sample_device` runs the step in the library (ops.sample_step, one launch per
position); `sample` drives the decoder, the n rows of an image sharing its K/V and prompt as the beams do, with no re-ordering after
the prompt's cache rows are handed out.

repetition_penalty / no_repeat_ngram_size (both modes): `decode_edits` is transformers' RepetitionPenaltyLogitsProcessor and
NoRepeatNGramLogitsProcessor as tensor ops, applied where transformers applies them -- to the log-probabilities before the beam score is
added, to the raw logits before the sampling warpers.  On the device the step stays one library call (ph_beam_topk_edit,
ph_sample_step_edit); with both options off every function here does exactly what it did without them.
"""
import torch

NEG = -1e9


EDIT_MAX_CUR = 512                                                 # PH_EDIT_MAX_CUR: history length of ph_beam_topk_edit / ph_sample_step_edit


def check_edit_args(repetition_penalty=1.0, no_repeat_ngram_size=0):
    """transformers' conditions: RepetitionPenaltyLogitsProcessor wants a strictly positive float (finite here: inf and nan have no
    meaning as a divisor), NoRepeatNGramLogitsProcessor an integer (0 = off)"""
    t, n = repetition_penalty, no_repeat_ngram_size
    if isinstance(t, bool) or not isinstance(t, (int, float)) or not (t > 0 and t < float('inf')):
        raise ValueError(f'repetition_penalty must be a finite float > 0, got {t}')
    if isinstance(n, bool) or not isinstance(n, (int, float)) or int(n) != n or n < 0:
        raise ValueError(f'no_repeat_ngram_size must be an integer >= 0, got {n}')


def _edits_on(repetition_penalty, no_repeat_ngram_size):
    check_edit_args(repetition_penalty, no_repeat_ngram_size)
    return float(repetition_penalty) != 1.0 or int(no_repeat_ngram_size) > 0


def decode_edits(ids, x, repetition_penalty=1.0, no_repeat_ngram_size=0):
    """transformers' RepetitionPenaltyLogitsProcessor and NoRepeatNGramLogitsProcessor as tensor ops: the SPECIFICATION of
    ph_beam_topk_edit / ph_sample_step_edit.  ids int64 [R, cur]: the whole row as transformers sees it (prompt and pad tokens count, no
    attention mask is consulted); x [R, V] scores.  Returns (y [R, V], banned bool [R, V]); y is fp32 (float64 for a float64 x).
      penalty  for every column t that occurs in ids[r]: y = x * theta if x < 0 else x / theta (IEEE division); theta = 1: the identity;
      n-gram   n > 0 and cur >= n: for every i in [0, cur - n] with ids[r, i : i+n-1] == ids[r, cur-n+1 : cur], column ids[r, i+n-1] is banned
               (n = 1: every token seen).
    A banned column wins over a penalised one (the caller removes it); history tokens outside [0, V) are ignored by both rules."""
    check_edit_args(repetition_penalty, no_repeat_ngram_size)
    n = int(no_repeat_ngram_size)
    x = x if x.dtype == torch.float64 else x.float()
    R, V = x.shape
    cur = ids.shape[1]
    inside = (ids >= 0) & (ids < V)
    row = torch.arange(R, device=x.device)[:, None].expand(R, cur)
    seen = torch.zeros(R, V, dtype=torch.bool, device=x.device)
    seen[row[inside], ids[inside]] = True
    theta = torch.tensor(float(repetition_penalty), dtype=x.dtype, device=x.device)      # a tensor: tensor / tensor is a true division everywhere
    y = torch.where(seen, torch.where(x < 0, x * theta, x / theta), x)
    banned = torch.zeros(R, V, dtype=torch.bool, device=x.device)
    if n > 0 and cur >= n:
        win = ids.unfold(1, n, 1)                                                         # [R, cur - n + 1, n]
        match = (win[:, :, :n - 1] == ids[:, cur - n + 1:][:, None, :]).all(dim=-1)       # n = 1: no prefix to compare, every window matches
        tok = win[:, :, n - 1]
        hit = match & (tok >= 0) & (tok < V)
        banned[row[:, :tok.shape[1]][hit], tok[hit]] = True
    return y, banned


def stable_topk(cand, k):
    """(values, indices) of the k best entries of every row of cand [B, N], best first, equal values in ascending index order: the
    tie rule of ph_beam_topk as tensor ops"""
    s, i = torch.sort(cand, dim=1, descending=True, stable=True)
    return s[:, :k], i[:, :k]


@torch.no_grad()
def beam_search_from_logits(step_fn, input_ids, num_beams=3, max_length=20, min_length=8, eos_token_id=2, pad_token_id=1,
                            length_penalty=1.0, reorder_fn=None, topk_fn=None, repetition_penalty=1.0, no_repeat_ngram_size=0):
    """step_fn(ids [B*nb, T]) -> next-token logits [B*nb, V] (any float dtype) for the LAST position of every row.
    reorder_fn(rows int64 [B*nb]) is called after each step with the source row of every continuing beam (cache re-ordering).
    topk_fn(cand [B, nb*V], k) -> (values, indices), best first; None = `cand.topk(k, dim=1)`, whose order among equal candidates is
    torch's; `stable_topk` is the library's rule.
    Returns a list of B 1-D LongTensors (prompt + generated tokens, EOS included when the hypothesis ended with one).
    All tensor ops, on the device of input_ids -- but not free of host round trips there: every boolean-mask index below is a
    `nonzero`, which waits for the device.
    repetition_penalty / no_repeat_ngram_size: `decode_edits` on the log-probabilities (fp32) with ids[:, :cur] as history, before the beam
    score is added, as transformers applies its processors: a penalised score is theta * logp, a banned column is no candidate, and the
    beam scores accumulate the processed values."""
    edit = _edits_on(repetition_penalty, no_repeat_ngram_size)
    B, T0 = input_ids.shape
    dev = input_ids.device
    nb = num_beams
    Tmax = max_length
    ids = torch.full((B * nb, Tmax), pad_token_id, dtype=torch.long, device=dev)
    ids[:, :T0] = input_ids.repeat_interleave(nb, dim=0)
    beam_scores = torch.zeros(B, nb, device=dev)
    beam_scores[:, 1:] = NEG
    hyp_score = torch.full((B, nb), -float('inf'), device=dev)            # finished hypotheses (BeamHypotheses): score,
    hyp_tok = torch.full((B, nb, Tmax), pad_token_id, dtype=torch.long, device=dev)      # tokens,
    hyp_len = torch.zeros(B, nb, dtype=torch.long, device=dev)            # length (EOS included)
    n_hyp = torch.zeros(B, dtype=torch.long, device=dev)
    done = torch.zeros(B, dtype=torch.bool, device=dev)
    ar_b = torch.arange(B, device=dev)
    cur = T0

    def add_hyp(sel, score, tokens, length):
        """BeamHypotheses.add for the batch items in `sel` (bool [B]): append while fewer than nb, else replace the worst if better"""
        worst, worst_i = hyp_score.min(dim=1)
        slot = torch.where(n_hyp < nb, n_hyp.clamp(max=nb - 1), worst_i)
        ok = sel & ((n_hyp < nb) | (score > worst))
        b = ar_b[ok]
        s = slot[ok]
        hyp_score[b, s] = score[ok]
        hyp_tok[b, s] = tokens[ok]
        hyp_len[b, s] = length[ok]
        n_hyp[ok & (n_hyp < nb)] += 1

    T_start = cur
    while cur < Tmax:
        logits = step_fn(ids[:, :cur])
        logp = torch.log_softmax(logits.float(), dim=-1)
        V = logp.shape[-1]
        if edit:
            logp, banned = decode_edits(ids[:, :cur], logp, repetition_penalty, no_repeat_ngram_size)
            logp[banned] = -float('inf')
        if cur < min_length:
            logp[:, eos_token_id] = -float('inf')
        cand = (beam_scores.view(-1, 1) + logp).view(B, nb * V)
        top_s, top_i = cand.topk(2 * nb, dim=1) if topk_fn is None else topk_fn(cand, 2 * nb)      # sorted, best first
        top_beam, top_tok = top_i // V, top_i % V
        n_next = torch.zeros(B, dtype=torch.long, device=dev)
        nxt_score = torch.zeros(B, nb, device=dev)
        nxt_row = (ar_b * nb)[:, None].repeat(1, nb)                     # padding beams of done items: (score 0, pad, first row)
        nxt_tok = torch.full((B, nb), pad_token_id, dtype=torch.long, device=dev)
        cur_ids = ids.view(B, nb, Tmax)
        for r in range(2 * nb):
            s, bm, tk = top_s[:, r], top_beam[:, r], top_tok[:, r]
            live = ~done & (n_next < nb)                                 # the reference loop breaks once nb beams are collected
            is_eos = tk == eos_token_id
            if r < nb:                                                   # EOS ranked inside the top nb: a finished hypothesis
                e = live & is_eos
                tokens = cur_ids[ar_b, bm].clone()
                tokens[:, cur] = eos_token_id
                add_hyp(e, s / (cur ** length_penalty), tokens, torch.full((B,), cur + 1, dtype=torch.long, device=dev))
            c = live & ~is_eos
            b = ar_b[c]
            k = n_next[c]
            nxt_score[b, k] = s[c]
            nxt_row[b, k] = (b * nb + bm[c])
            nxt_tok[b, k] = tk[c]
            n_next[c] += 1
        # is_done (4.26.1): num_beams hypotheses held and the worst one beats what the best running beam could still score
        best_running = top_s[:, 0] / (cur ** length_penalty)
        done = done | ((n_hyp >= nb) & (hyp_score.min(dim=1).values >= best_running))
        rows = nxt_row.reshape(-1)
        ids = ids.index_select(0, rows)
        ids[:, cur] = nxt_tok.reshape(-1)
        beam_scores = nxt_score
        if reorder_fn is not None:
            reorder_fn(rows)
        cur += 1
        # transformers breaks out once every item is done (beam_scorer.is_done); one small device->host sync every 4 steps here
        if (cur - T_start) % 4 == 0 and bool(done.all()):
            break
    # finalize: running beams of unfinished items become hypotheses (score / cur_len ** lp)
    cur_ids = ids.view(B, nb, Tmax)
    for k in range(nb):
        add_hyp(~done, beam_scores[:, k] / (cur ** length_penalty), cur_ids[:, k], torch.full((B,), cur, dtype=torch.long, device=dev))
    best = hyp_score.argmax(dim=1)
    out_tok = hyp_tok[ar_b, best].cpu()
    out_len = hyp_len[ar_b, best].cpu()
    return [out_tok[b, :int(out_len[b])].to(dev) for b in range(B)]


@torch.no_grad()
def beam_search_device(step_fn, input_ids, num_beams=3, max_length=20, min_length=8, eos_token_id=2, pad_token_id=1,
                       length_penalty=1.0, reorder_fn=None, rows_rep=1, repetition_penalty=1.0, no_repeat_ngram_size=0):
    """beam_search_from_logits with the beam step in the library (ops.beam_topk, ops.beam_advance) and the search state in device
    buffers allocated once: same arguments, same return value, ties by the library's rule.
    step_fn(ids [B*nb, T]) -> bf16 logits on the GPU, [B*nb, V], or [B, V] when one row stands for all beams of its item (the first
    step after a per-image prefill).  reorder_fn(rows int32 [rows_rep * B*nb]) gets, for l < rows_rep, l * B*nb + the source row of
    every continuing beam AMONG THE ROWS step_fn RETURNED (rows_rep > 1: the gather index of a stack of caches).
    With repetition_penalty != 1 or no_repeat_ngram_size > 0 the step is ph_beam_topk_edit on the token rows of the search state (at most
    EDIT_MAX_CUR tokens of history: max_length <= EDIT_MAX_CUR + 1); with both off it is ph_beam_topk, launch for launch what it was."""
    from .. import ops
    edit = _edits_on(repetition_penalty, no_repeat_ngram_size)
    B, T0 = input_ids.shape
    dev = input_ids.device
    nb, Tmax = num_beams, max_length
    i32 = torch.int32
    ids = [torch.full((B * nb, Tmax), pad_token_id, dtype=torch.long, device=dev) for _ in range(2)]      # ping-pong
    ids[0][:, :T0] = input_ids.repeat_interleave(nb, dim=0)
    which = 0
    beam_scores = torch.zeros(B, nb, device=dev)
    beam_scores[:, 1:] = NEG
    first_scores = torch.zeros(B, device=dev)                             # one row per item: that row is beam 0
    hyp_score = torch.full((B, nb), -float('inf'), device=dev)
    hyp_tok = torch.full((B, nb, Tmax), pad_token_id, dtype=torch.long, device=dev)
    hyp_len = torch.zeros(B, nb, dtype=i32, device=dev)
    n_hyp = torch.zeros(B, dtype=i32, device=dev)
    done = torch.zeros(B, dtype=i32, device=dev)
    rows = torch.empty(rows_rep * B * nb, dtype=i32, device=dev)
    top = (torch.empty(B, 2 * nb, device=dev), torch.empty(B, 2 * nb, dtype=i32, device=dev), torch.empty(B, 2 * nb, dtype=i32, device=dev))
    ws = None
    cur = T_start = T0
    while cur < Tmax:
        logits = step_fn(ids[which][:, :cur])
        if ws is None:
            ws = ops.beam_topk_workspace(B, nb, logits.shape[1], dev)
        nb_in = logits.shape[0] // B
        ops.beam_topk(logits, beam_scores if nb_in == nb else first_scores, B, nb, eos_token_id, cur < min_length, workspace=ws, out=top,
                      edits=(ids[which], cur, repetition_penalty, no_repeat_ngram_size) if edit else None)
        ops.beam_advance(top, ids[which], ids[which ^ 1], beam_scores, hyp_score, hyp_tok, hyp_len, n_hyp, done, rows, nb_in, cur,
                         eos_token_id, pad_token_id, float(cur) ** length_penalty)
        which ^= 1
        if reorder_fn is not None:
            reorder_fn(rows)
        cur += 1
        if (cur - T_start) % 4 == 0 and bool(done.cpu().all()):           # the one host read: B flags, every fourth step
            break
    # finalize, once per call, on the host (the state is B * nb token rows): running beams of unfinished items become hypotheses
    # (score / cur_len ** lp, BeamHypotheses.add as above), the best hypothesis wins
    cur_ids = ids[which].view(B, nb, Tmax).cpu()
    beam_scores, hyp_score, hyp_tok, hyp_len, n_hyp = (t.cpu() for t in (beam_scores.view(B, nb), hyp_score, hyp_tok, hyp_len, n_hyp))
    live = done.cpu() == 0
    for k in range(nb):
        score = beam_scores[:, k] / (cur ** length_penalty)
        worst, worst_i = hyp_score.min(dim=1)
        slot = torch.where(n_hyp < nb, n_hyp.clamp(max=nb - 1).long(), worst_i)
        ok = live & ((n_hyp < nb) | (score > worst))
        sel = ok[:, None] & (torch.arange(nb)[None, :] == slot[:, None])                 # [B, nb]: the slot that takes the beam
        hyp_score = torch.where(sel, score[:, None], hyp_score)
        hyp_tok = torch.where(sel[:, :, None], cur_ids[:, k][:, None, :], hyp_tok)
        hyp_len = torch.where(sel, torch.full_like(hyp_len, cur), hyp_len)
        n_hyp = n_hyp + (ok & (n_hyp < nb)).to(i32)
    best = hyp_score.argmax(dim=1)
    ar_b = torch.arange(B)
    out_tok, out_len = hyp_tok[ar_b, best], hyp_len[ar_b, best]
    return [out_tok[b, :int(out_len[b])].to(dev) for b in range(B)]


def _device_beams_ok(device_beams, dev, nb, edit=False, max_length=0):
    if device_beams is False:
        return False
    ok = dev.type == 'cuda' and 1 <= nb <= 8 and not (edit and max_length - 1 > EDIT_MAX_CUR)
    if device_beams and not ok:
        raise ValueError(f'device_beams=True needs logits on the GPU, 1 <= num_beams <= 8 and, with repetition_penalty / no_repeat_ngram_size, '
                         f'max_length <= {EDIT_MAX_CUR + 1}')
    return ok


@torch.no_grad()
def beam_search(decoder, input_ids, attention_mask, enc, num_beams=3, max_length=20, min_length=8, eos_token_id=2, pad_token_id=1,
                length_penalty=1.0, use_cache=True, device_beams=None, share_image=True, repetition_penalty=1.0, no_repeat_ngram_size=0):
    """decoder: prismer_amd RobertaForCausalLMModified (eval mode); enc: [B, S, Hv] encoder states (one row per image).
    use_cache=False re-runs the full prefix every step like the reference (kept for the equivalence test).
    device_beams: None = the device beam step (beam_search_device) when the logits are bf16 on the GPU and num_beams <= 8, else the
    tensor form; False forces the tensor form (beam_search_from_logits).  Cached and recomputing decoding take the same beam step.
    repetition_penalty / no_repeat_ngram_size: see `decode_edits`; the history is the whole row, prompt and pads included.  With them on,
    a max_length beyond EDIT_MAX_CUR + 1 takes the tensor form.
    share_image: the beams of an image share its cross-attention K/V and the prompt runs once per image; False tiles every image
    num_beams times before anything runs (the earlier layout, kept for A/B measurements)."""
    B, T0 = input_ids.shape
    nb = num_beams
    edit = _edits_on(repetition_penalty, no_repeat_ngram_size)
    on_device = _device_beams_ok(device_beams, input_ids.device, nb, edit, max_length)
    kw = dict(num_beams=nb, max_length=max_length, min_length=min_length, eos_token_id=eos_token_id, pad_token_id=pad_token_id,
              length_penalty=length_penalty)
    if edit:
        kw.update(repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size)
    search = beam_search_device if on_device else beam_search_from_logits
    att_b = torch.cat([attention_mask.repeat_interleave(nb, dim=0), attention_mask.new_ones(B * nb, max(max_length - T0, 0))], dim=1)

    def mask_for(T):                                               # generated positions are real tokens
        return att_b[:, :T]
    if not use_cache:
        enc_b = enc.repeat_interleave(nb, dim=0).contiguous()

        def step(ids):
            out = decoder(ids, attention_mask=mask_for(ids.shape[1]), encoder_hidden_states=enc_b, return_dict=True)
            return out.logits[:, -1, :]
        return search(step, input_ids, **kw)
    if not share_image:
        prog, enc_bf = decoder.decoding_program(enc.repeat_interleave(nb, dim=0).contiguous())
        st = prog.decode_begin(enc_bf, max_length)

        def step(ids):
            T = ids.shape[1]
            return prog.decode(st, ids, mask_for(T), 0 if T == T0 else T - 1)
        return search(step, input_ids, reorder_fn=lambda rows: prog.decode_reorder(st, rows), **kw)
    prog, enc_bf = decoder.decoding_program(enc)
    st = prog.decode_begin(enc_bf, max_length, beams=nb)
    nl = st['cache'][0].shape[0]

    def step(ids):
        T = ids.shape[1]
        if T == T0:                                                # the prompt once per image: the beams of an item are identical here
            return prog.decode(st, ids[::nb], attention_mask, 0)
        return prog.decode(st, ids, mask_for(T), T - 1)
    if on_device:                                                  # ph_beam_advance writes the gather index of the whole cache stack
        return beam_search_device(step, input_ids, reorder_fn=lambda rows: prog.decode_reorder(st, rows), rows_rep=nl, **kw)
    first = [True]

    def step_tiled(ids):                                           # the tensor form wants one logit row per beam
        lg = step(ids)
        return lg.repeat_interleave(nb, dim=0) if lg.shape[0] == B else lg

    def reorder(rows):                                             # ... and names source rows among B * nb: after the prefill they are B
        prog.decode_reorder(st, rows // nb if first[0] else rows)
        first[0] = False
    return beam_search_from_logits(step_tiled, input_ids, reorder_fn=reorder, **kw)


# ------------------------------------------------------------------------------------------------ sampled decoding
PHILOX_ROUNDS = 7                                                  # PH_PHILOX_ROUNDS of csrc/common.h
SAMPLE_MAX_V = 65535                                               # ph_sample_step: 16-bit class counts
SAMPLE_MAX_GROUP = 8                                               # rows of one image the grouped decode step is used with (as the beams)


def philox_word0(c0, c1, c2, c3, seed):
    """word 0 of philox4x32(counter = (c0, c1, c2, c3), key = seed) of csrc/common.h, on python ints"""
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(PHILOX_ROUNDS):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & 0xFFFFFFFF, p1 & 0xFFFFFFFF, ((p0 >> 32) ^ c3 ^ k1) & 0xFFFFFFFF, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0


def sample_uniforms(rows, cur, seed):
    """fp32 [rows]: the uniform of every row at position cur, u = (w >> 8) * 2^-24 in [0, 1), a function of (seed, row, position) alone"""
    return torch.tensor([(philox_word0(r, cur, 0, 0x5a3b1e, seed) >> 8) / 16777216.0 for r in range(rows)], dtype=torch.float32)


def check_sampling_args(temperature=1.0, top_k=50, top_p=1.0, num_return_sequences=1):
    if not (temperature > 0 and temperature < float('inf')):
        raise ValueError(f'temperature must be a positive finite number, got {temperature}')
    if not (0 < top_p <= 1):
        raise ValueError(f'top_p must lie in (0, 1], got {top_p}')
    if int(top_k) != top_k or top_k < 0:
        raise ValueError(f'top_k must be an integer >= 0 (0 = off), got {top_k}')
    if int(num_return_sequences) != num_return_sequences or num_return_sequences < 1:
        raise ValueError(f'num_return_sequences must be an integer >= 1, got {num_return_sequences}')


def sample_filter(x, temperature=1.0, top_k=50, top_p=1.0, banned_col=None, banned=None):
    """The kept set of every row of x (fp32 [R, V]: bf16 logits read as fp32) as (keep bool [R, V], z float64 [R, V] = x / temperature).
    Candidates are the finite columns (a NaN is never one; -inf is what transformers' own filters write for a removed token; +inf has
    no distribution) but `banned_col` and the columns of the optional mask `banned` (bool [R, V]).  Top-k keeps z >= the k-th largest z, ties included.  Top-p works on classes of equal logit over
    what top-k kept: a class stays iff the mass of the strictly higher classes is < top_p, so the top class always stays and the kept set is
    a threshold set -- TopPLogitsWarper's rule but inside the boundary class, which transformers cuts by sort position."""
    x = x.float()
    cand = torch.isfinite(x)
    if banned_col is not None:
        cand[:, banned_col] = False
    if banned is not None:
        cand = cand & ~banned
    z = x.double() / float(temperature)
    ninf = torch.full_like(z, -float('inf'))
    keep = cand
    if top_k > 0:
        zc = torch.where(cand, z, ninf)
        kth = zc.topk(min(int(top_k), x.shape[1]), dim=1).values[:, -1:]
        keep = cand & (zc >= kth)
    if top_p < 1:
        s, idx = torch.sort(torch.where(keep, z, ninf), dim=1, descending=True, stable=True)
        live = torch.isfinite(s)
        p = torch.where(live, torch.exp(s - s[:, :1]), torch.zeros_like(s))
        p = p / p.sum(dim=1, keepdim=True).clamp_min(1e-300)
        above = torch.cumsum(p, dim=1) - p                                        # mass before each sorted position ...
        start = torch.ones_like(live)
        start[:, 1:] = s[:, 1:] != s[:, :-1]
        above = torch.where(start, above, torch.full_like(above, -1.0)).cummax(dim=1).values       # ... before the position's class
        keep = torch.zeros_like(keep).scatter(1, idx, live & (above < top_p))
    return keep, z


def sample_draw(keep, z, u):
    """token int64 [R] (-1 for a row that keeps nothing): inverse CDF over the kept tokens in the defined order -- class (logit)
    descending, token id ascending inside a class -- the first token whose cumulative kept mass exceeds u * Z_kept; float64 masses."""
    s, idx = torch.sort(torch.where(keep, z, torch.full_like(z, -float('inf'))), dim=1, descending=True, stable=True)
    live = torch.isfinite(s)
    mass = torch.where(live, torch.exp(s - s[:, :1]), torch.zeros_like(s))
    C = torch.cumsum(mass, dim=1)
    n_live = live.sum(dim=1)
    hit = C > (u.double()[:, None] * C[:, -1:])
    pos = torch.where(hit.any(dim=1), hit.int().argmax(dim=1), (n_live - 1).clamp_min(0))
    tok = idx.gather(1, pos[:, None])[:, 0]
    return torch.where(n_live > 0, tok, torch.full_like(tok, -1))


def _trim_sampled(ids, T0, cur, eos_token_id):
    """ids[:, :L], L = the longest row (EOS included) among positions < cur: what a loop that stops the moment every row is done returns"""
    gen = ids[:, T0:cur].cpu() == eos_token_id
    if gen.shape[1] == 0:
        return ids[:, :cur]
    first = torch.where(gen.any(dim=1), gen.int().argmax(dim=1) + 1, torch.full((gen.shape[0],), gen.shape[1]))
    return ids[:, :T0 + int(first.max())]


@torch.no_grad()
def sample_from_logits(step_fn, input_ids, num_return_sequences=1, max_length=20, min_length=0, temperature=1.0, top_k=50, top_p=1.0,
                       eos_token_id=2, pad_token_id=1, seed=0, uniforms=None, reorder_fn=None, repetition_penalty=1.0, no_repeat_ngram_size=0):
    """Sampled decoding as tensor ops: the SPECIFICATION of ph_sample_step / sample_device (transformers' generate(do_sample=True):
    MinLengthLogitsProcessor -> TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper -> multinomial, bookkeeping of _sample).
    step_fn(ids [B*n, T]) -> next-token logits for the last position, [B*n, V], or [B, V] when one row stands for the n rows of its
    image (the first step after a per-image prefill); reorder_fn(rows int64 [B*n]) is then called once after that step with the
    source row r // n of every row.  Row r = image * n + j.  Per step, on the logits rounded to bf16 and read as fp32:
    `sample_filter` (EOS banned while cur < min_length), `sample_draw` with u = uniforms[r, cur] or `sample_uniforms`; a finished row
    emits pad, a row that draws EOS is finished, a row without candidates emits EOS and is finished (its log-probability stays).
    Returns (ids [B*n, L] padded with pad_token_id, L = the longest row, EOS included; seq_logprob fp32 [B*n] = the sum of
    log_softmax(raw fp32 row)[token] over the drawn tokens: temperature 1, no filter, no ban).
    repetition_penalty / no_repeat_ngram_size: `decode_edits` on the row (bf16 read as fp32) with ids[r, :cur] as history; the result is
    rounded back to bf16 (nearest even) -- again a row of bf16 logits, the one deviation from transformers: relative 2^-9 on penalised
    logits -- and everything downstream runs on it with the banned columns joined to the non-candidates; the log-probability stays the RAW
    row's."""
    check_sampling_args(temperature, top_k, top_p, num_return_sequences)
    edit = _edits_on(repetition_penalty, no_repeat_ngram_size)
    B, T0 = input_ids.shape
    dev = input_ids.device
    n, Tmax = int(num_return_sequences), max_length
    R = B * n
    ids = torch.full((R, max(Tmax, T0)), pad_token_id, dtype=torch.long, device=dev)
    ids[:, :T0] = input_ids.repeat_interleave(n, dim=0)
    done = torch.zeros(R, dtype=torch.bool, device=dev)
    logprob = torch.zeros(R, dtype=torch.float32, device=dev)
    cur = T0
    while cur < Tmax and not bool(done.all()):
        logits = step_fn(ids[:, :cur])
        shared = logits.shape[0] != R
        x = logits.bfloat16().float()
        if shared:
            x = x.repeat_interleave(n, dim=0)
        xe, banned = x, None
        if edit:
            y, banned = decode_edits(ids[:, :cur], x, repetition_penalty, no_repeat_ngram_size)
            xe = y.bfloat16().float()
        keep, z = sample_filter(xe, temperature, top_k, top_p, eos_token_id if cur < min_length else None, banned=banned)
        u = (sample_uniforms(R, cur, seed) if uniforms is None else uniforms[:, cur].float().cpu()).to(dev)
        tok = sample_draw(keep, z, u)
        empty = tok < 0
        tok = torch.where(empty, torch.full_like(tok, eos_token_id), tok)
        lp = torch.log_softmax(x, dim=-1).gather(1, tok[:, None])[:, 0]
        logprob = torch.where(done | empty, logprob, logprob + lp)
        ids[:, cur] = torch.where(done, torch.full_like(tok, pad_token_id), tok)
        done = done | (tok == eos_token_id)
        if shared and reorder_fn is not None:
            reorder_fn(torch.arange(R, device=dev) // n)
        cur += 1
    return _trim_sampled(ids, T0, cur, eos_token_id), logprob


@torch.no_grad()
def sample_device(step_fn, input_ids, num_return_sequences=1, max_length=20, min_length=0, temperature=1.0, top_k=50, top_p=1.0,
                  eos_token_id=2, pad_token_id=1, seed=0, reorder_fn=None, rows_rep=1, repetition_penalty=1.0, no_repeat_ngram_size=0):
    """sample_from_logits with the step in the library (ops.sample_step: one launch per position for all rows) on state allocated once:
    same arguments (no `uniforms`), same return value.  step_fn -> bf16 logits on the GPU; reorder_fn(rows int32 [rows_rep * B*n]) gets,
    once, after a step whose logits had one row per image, l * B*n + r // n for l < rows_rep.  The one host read is the "all rows
    done?" check every fourth step.  With repetition_penalty != 1 or no_repeat_ngram_size > 0 the step is ph_sample_step_edit (max_length <=
    EDIT_MAX_CUR + 1); with both off it is ph_sample_step."""
    from .. import ops
    check_sampling_args(temperature, top_k, top_p, num_return_sequences)
    edits = (repetition_penalty, no_repeat_ngram_size) if _edits_on(repetition_penalty, no_repeat_ngram_size) else None
    B, T0 = input_ids.shape
    dev = input_ids.device
    n, Tmax = int(num_return_sequences), max_length
    R = B * n
    ids = torch.full((R, max(Tmax, T0)), pad_token_id, dtype=torch.long, device=dev)
    ids[:, :T0] = input_ids.repeat_interleave(n, dim=0)
    done = torch.zeros(R, dtype=torch.int32, device=dev)
    logprob = torch.zeros(R, dtype=torch.float32, device=dev)
    cur = T_start = T0
    while cur < Tmax:
        logits = step_fn(ids[:, :cur])
        ops.sample_step(logits, ids, done, logprob, cur, temperature, top_k, top_p, eos_token_id, pad_token_id, cur < min_length, seed, edits=edits)
        if logits.shape[0] != R and reorder_fn is not None:
            i32 = torch.int32
            rows = torch.arange(R, device=dev, dtype=i32) // n
            reorder_fn((torch.arange(rows_rep, device=dev, dtype=i32)[:, None] * R + rows[None, :]).reshape(-1) if rows_rep > 1 else rows)
        cur += 1
        if (cur - T_start) % 4 == 0 and bool(done.cpu().all()):           # the one host read: R flags, every fourth step
            break
    return _trim_sampled(ids, T0, cur, eos_token_id), logprob


def _device_sample_ok(device_sample, dev, V, edit=False, max_length=0):
    if device_sample is False:
        return False
    ok = dev.type == 'cuda' and 8 <= V <= SAMPLE_MAX_V and not (edit and max_length - 1 > EDIT_MAX_CUR)
    if device_sample and not ok:
        raise ValueError(f'device_sample=True needs logits on the GPU, 8 <= vocabulary <= {SAMPLE_MAX_V} and, with repetition_penalty / '
                         f'no_repeat_ngram_size, max_length <= {EDIT_MAX_CUR + 1}')
    return ok


@torch.no_grad()
def sample(decoder, input_ids, attention_mask, enc, num_return_sequences=1, max_length=20, min_length=0, temperature=1.0, top_k=50,
           top_p=1.0, eos_token_id=2, pad_token_id=1, seed=0, use_cache=True, device_sample=None, share_image=True, repetition_penalty=1.0,
           no_repeat_ngram_size=0):
    """Sampled decoding with the decoder, the counterpart of `beam_search`: n = num_return_sequences rows per image, row image * n + j.
    Returns (ids [B*n, L], seq_logprob [B*n]) as `sample_from_logits` does.
    device_sample: None = the device step (sample_device) when the logits are bf16 on the GPU and the vocabulary fits ph_sample_step,
    else the tensor form; False forces the tensor form.
    share_image: the n rows of an image share its cross-attention K/V (decode_begin(beams=n)), the prompt runs once per image and one
    decode_reorder (source row r // n) hands the prompt's cache rows out; nothing is re-ordered afterwards.  n = 1 needs neither.  The
    grouped decode step is used with up to SAMPLE_MAX_GROUP rows per image (what the beam search exercises); a larger n, or
    share_image=False, tiles every image n times before anything runs.
    repetition_penalty / no_repeat_ngram_size: see `sample_from_logits`; with them on, a max_length beyond EDIT_MAX_CUR + 1 takes the tensor form."""
    check_sampling_args(temperature, top_k, top_p, num_return_sequences)
    B, T0 = input_ids.shape
    n = int(num_return_sequences)
    edit = _edits_on(repetition_penalty, no_repeat_ngram_size)
    on_device = _device_sample_ok(device_sample, input_ids.device, decoder.config.vocab_size, edit, max_length)
    kw = dict(num_return_sequences=n, max_length=max_length, min_length=min_length, temperature=temperature, top_k=top_k, top_p=top_p,
              eos_token_id=eos_token_id, pad_token_id=pad_token_id, seed=seed)
    if edit:
        kw.update(repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size)
    search = sample_device if on_device else sample_from_logits
    att_b = torch.cat([attention_mask.repeat_interleave(n, dim=0), attention_mask.new_ones(B * n, max(max_length - T0, 0))], dim=1)
    if not use_cache:
        enc_b = enc.repeat_interleave(n, dim=0).contiguous()

        def step(ids):
            out = decoder(ids, attention_mask=att_b[:, :ids.shape[1]], encoder_hidden_states=enc_b, return_dict=True)
            return out.logits[:, -1, :]
        return search(step, input_ids, **kw)
    if not share_image or n == 1 or n > SAMPLE_MAX_GROUP:
        prog, enc_bf = decoder.decoding_program(enc.repeat_interleave(n, dim=0).contiguous() if n > 1 else enc)
        st = prog.decode_begin(enc_bf, max_length)

        def step(ids):
            T = ids.shape[1]
            return prog.decode(st, ids, att_b[:, :T], 0 if T == T0 else T - 1)
        return search(step, input_ids, **kw)
    prog, enc_bf = decoder.decoding_program(enc)
    st = prog.decode_begin(enc_bf, max_length, beams=n)

    def step(ids):
        T = ids.shape[1]
        if T == T0:                                                # the prompt once per image: the n rows of an image are identical here
            return prog.decode(st, ids[::n], attention_mask, 0)
        return prog.decode(st, ids, att_b[:, :T], T - 1)
    kw['reorder_fn'] = lambda rows: prog.decode_reorder(st, rows)
    if on_device:
        kw['rows_rep'] = st['cache'][0].shape[0]
    return search(step, input_ids, **kw)
