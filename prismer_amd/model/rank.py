"""`inference='rank'` of the caption and VQA heads (reference: model/prismer_caption.py:59-112, model/prismer_vqa.py:64-113).

The reference scores k candidate answers per image by running the decoder on [prompt || answer] for all B*k pairs: every image's
encoder states are tiled k times (and their cross-attention K/V projected k times) and the prompt runs through every layer once
per candidate, although causal attention makes its hidden states the same for all k.  Here the prompt runs ONCE per image, KV-cached
(DecoderProgram.decode_begin + the prefill decode), and only the continuations run per candidate (DecoderProgram.score_continuations):

  continuation row r = b*k + j:  [q[b, Tq-1], answer topk(b, j)]  (Tc = Ta + 1 tokens)
    - self-attention: the cached prefix positions 0 .. Tp-1 (Tp = Tq - 1) of image b under its question mask, then its own tokens
      causally under [q_att[b, Tq-1], a_att];
    - cross-attention: image b's K/V, projected once;
    - positions: pad + (number of non-pad tokens of q[b, :Tp]) + cumsum(id != pad) for real tokens, pad for pads;
    - labels: [-100, answer with pad -> -100]: the question's last token is recomputed per candidate, so the existing loss kernel
      scores the first answer token from its logits exactly as the reference does (from the last question position, a pad for a
      shorter question of a ragged batch).
  Score = -loss / #targets; nothing is approximated.

The shared path needs head dim 64, Tc = Ta + 1 <= 32 and Tp = Tq - 1 <= 288 (ph_attention_prefix_fwd); every reference configuration
is inside.  Outside those limits the tiled path (the reference's own layout) runs.
"""
import torch

PREFIX_MAX = 288          # ph_attention_prefix_fwd: prefix keys
CONT_MAX = 32             # ph_attention_prefix_fwd: continuation tokens (answer + the question's last token)


def _first_token_probs(logits_last, first_ids):
    """softmax(logits, dim=1).index_select(1, first token of every candidate answer) (prismer_caption.py:70, prismer_vqa.py:51) through the
    library's kernel (ph_softmax_gather_bf16: no stock torch softmax on the rank path, round 6); logits_last: [B, V] view of the decoder's logits"""
    from .. import ops
    x = logits_last
    if x.dtype != torch.bfloat16 or x.stride(-1) != 1 or (x.stride(0) % 8) != 0 or (x.data_ptr() % 16) != 0:
        x = x.to(torch.bfloat16).contiguous()
        if x.shape[1] % 8:                                      # (row stride must be a multiple of 8 elements)
            x = torch.nn.functional.pad(x, (0, 8 - x.shape[1] % 8))[:, :logits_last.shape[1]]
    return ops.softmax_gather(x, first_ids.to(torch.int64))


def _candidates(prob_first, a_ids, a_att, k_test):
    """top-k answers per image and their rows, item-major (reference tile(): rows b*k .. b*k+k-1 belong to image b), in ONE gather"""
    _, topk_ids = prob_first.topk(k_test, dim=1)
    flat = topk_ids.reshape(-1)
    return topk_ids, a_ids.index_select(0, flat), a_att.index_select(0, flat)


def shared_ok(decoder, Tq, Ta):
    c = decoder.config
    return c.hidden_size // c.num_attention_heads == 64 and 1 <= Tq <= PREFIX_MAX + 1 and Ta + 1 <= CONT_MAX


def continuation_layout(q_ids, q_att, ans_ids, ans_att, k_test, pad):
    """continuation rows r = b*k + j = [q[b, Tq-1], ans[r]] of the shared path: (ids [R, Tc] int64, attention mask [R, Tc], labels [R, Tc]
    with -100 for unscored tokens, position base int32 [R] = number of non-pad tokens of q[b, :Tq-1])"""
    Tp = q_ids.shape[1] - 1
    q_ids = q_ids.long()
    cont_ids = torch.cat([q_ids[:, Tp:].repeat_interleave(k_test, dim=0), ans_ids.long()], dim=1)
    cont_att = torch.cat([q_att[:, Tp:].repeat_interleave(k_test, dim=0), ans_att.to(q_att.dtype)], dim=1)
    labels = cont_ids.masked_fill(cont_ids == pad, -100)
    labels[:, 0] = -100
    pos_base = (q_ids[:, :Tp] != pad).sum(1).to(torch.int32).repeat_interleave(k_test)
    return cont_ids, cont_att, labels, pos_base


def _rank_tiled(decoder, enc, q_ids, q_att, a_ids, a_att, k_test, pad):
    """the reference's layout: [prompt || answer] for all B*k pairs, encoder states tiled k times"""
    start = decoder(q_ids, attention_mask=q_att, encoder_hidden_states=enc, return_dict=True)
    prob_first = _first_token_probs(start.logits[:, -1, :], a_ids[:, 0])
    topk_ids, ans_ids, ans_att = _candidates(prob_first, a_ids, a_att, k_test)
    input_ids = torch.cat([q_ids.repeat_interleave(k_test, dim=0), ans_ids], dim=1).long()
    att = torch.cat([q_att.repeat_interleave(k_test, dim=0), ans_att], dim=1)
    targets = input_ids.masked_fill(input_ids == pad, -100)
    targets[:, :-a_ids.shape[1]] = -100
    out = decoder(input_ids, attention_mask=att, encoder_hidden_states=enc.repeat_interleave(k_test, dim=0), labels=targets, return_dict=True)
    lp = (-out.loss / torch.sum(targets != -100, dim=-1)).view(-1, k_test)
    return topk_ids, lp


def _rank_shared(decoder, enc, q_ids, q_att, a_ids, a_att, k_test, pad):
    """prompt once per image (KV-cached), then the B*k continuations against the cached prefix (module docstring)"""
    prog, enc = decoder.decoding_program(enc)
    B, Tq = q_ids.shape
    Tp = Tq - 1
    q_ids = q_ids.long()
    st = prog.decode_begin(enc, Tq)
    last = prog.decode(st, q_ids, q_att, 0)                                      # logits of the last prompt position [B, V]
    prob_first = _first_token_probs(last, a_ids[:, 0])
    topk_ids, ans_ids, ans_att = _candidates(prob_first, a_ids, a_att, k_test)
    cont_ids, cont_att, labels, pos_base = continuation_layout(q_ids, q_att, ans_ids, ans_att, k_test, pad)
    loss = prog.score_continuations(st, cont_ids, cont_att, labels, pos_base, Tp, k_test)
    lp = (-loss / torch.sum(labels != -100, dim=-1)).view(-1, k_test)
    return topk_ids, lp


def rank_answers(decoder, enc, q_ids, q_att, a_ids, a_att, k_test, pad):
    """enc: [B, S, D] encoder states; q_ids / q_att: [B, Tq] prompt (right-padded); a_ids / a_att: [n, Ta] candidate answers.
    Returns (topk_ids [B, k], length-normalised log-probabilities [B, k]) of the reference's rank inference."""
    if shared_ok(decoder, q_ids.shape[1], a_ids.shape[1]):
        return _rank_shared(decoder, enc, q_ids, q_att, a_ids, a_att, k_test, pad)
    return _rank_tiled(decoder, enc, q_ids, q_att, a_ids, a_att, k_test, pad)
