"""VQA head (reference: model/prismer_vqa.py:15-122): question ‖ answer training loss with per-sample weights."""
import torch

from .prismer import Prismer
from .rank import rank_answers
from ..trainer import check_text_rows


class PrismerVQA(Prismer):
    def _ids(self, text, device, **kw):
        if isinstance(text, dict):
            return text['input_ids'].to(device), text['attention_mask'].to(device)
        if isinstance(text, (tuple, list)) and len(text) == 2 and torch.is_tensor(text[0]):
            return text[0].to(device), text[1].to(device)
        t = self._tokenize(text, return_tensors='pt', **kw).to(device)
        return t.input_ids, t.attention_mask

    def forward(self, experts, question, answer=None, weights=None, train=True, inference='rank', k_test=128, return_scores=False, sample=None,
                generate_args=None, texts_per_image=1):
        """texts_per_image=n (training): `question`, `answer` and `weights` hold n entries per image, image-major (entries b*n .. b*n+n-1 belong
        to image b).  The encoder runs once per image and the decoder's cross-attention shares an image's K/V among its n rows; the loss is the
        mean of weights * loss over the B*n rows.
        sample: None = the reference's fixed beam search; a dict of sampling arguments of `text_decoder.generate` (top_p, top_k, temperature,
        num_return_sequences, seed) routes inference='generate' through sampled decoding: B * num_return_sequences answers, image-major.
        generate_args: None, or a dict of further arguments of `text_decoder.generate` for the beam search (repetition_penalty,
        no_repeat_ngram_size); the `sample` dict carries them for sampled decoding."""
        device = experts['rgb'].device
        pad = self.text_decoder.config.pad_token_id
        if isinstance(question, (list, tuple)) and question and isinstance(question[0], str):
            question = ['<s>' + q.capitalize() for q in question]
            q_ids, q_att = self._ids(question, device, padding='longest', truncation=True, max_length=35, add_special_tokens=False)
        else:
            q_ids, q_att = self._ids(question, device)
        if train:
            enc = self.expert_encoder(experts).permute(1, 0, 2)
            if isinstance(answer, (list, tuple)) and answer and isinstance(answer[0], str):
                answer = [' ' + a.capitalize() + '</s>' for a in answer]
                a_ids, a_att = self._ids(answer, device, padding='longest', add_special_tokens=False)
            else:
                a_ids, a_att = self._ids(answer, device)
            input_ids = torch.cat([q_ids, a_ids], dim=1).long()
            attention_mask = torch.cat([q_att, a_att], dim=1)
            targets = input_ids.masked_fill(input_ids == pad, -100)
            targets[:, :-a_ids.shape[1]] = -100                                           # prismer_vqa.py:32-33
            check_text_rows(enc.shape[0], input_ids.shape[0], texts_per_image, 'PrismerVQA.forward')
            out = self.text_decoder(input_ids, attention_mask=attention_mask, encoder_hidden_states=enc, labels=targets, return_dict=True)
            return (weights.to(out.loss.dtype) * out.loss).mean()                           # prismer_vqa.py:40-41
        with torch.no_grad():
            enc = self.expert_encoder(experts).permute(1, 0, 2)
            if inference == 'generate':
                if sample is None:
                    out = self.text_decoder.generate(input_ids=q_ids, encoder_hidden_states=enc, attention_mask=q_att,
                                                     max_length=q_ids.shape[1] + 10, min_length=q_ids.shape[1] + 2, num_beams=3,
                                                     length_penalty=-1, **(generate_args or {}))         # prismer_vqa.py:52-58
                else:
                    out = self.text_decoder.generate(input_ids=q_ids, encoder_hidden_states=enc, attention_mask=q_att, do_sample=True,
                                                     max_length=q_ids.shape[1] + 10, min_length=q_ids.shape[1] + 2, **sample)
                if self.tokenizer is None:
                    return out[:, q_ids.shape[1]:]
                return [self.tokenizer.decode(o[q_ids.shape[1]:], skip_special_tokens=True).lower().strip() for o in out]
            a_ids, a_att = self._ids(answer, device) if not (isinstance(answer, (list, tuple)) and isinstance(answer[0], str)) else \
                self._ids([' ' + a.capitalize() + '</s>' for a in answer], device, padding='longest', add_special_tokens=False)
            topk_ids, lp = rank_answers(self.text_decoder, enc, q_ids, q_att, a_ids, a_att, k_test, pad)
            best = lp.argmax(dim=1)
            if return_scores:                                   # (extension for the parity tests: the candidates and their scores)
                return topk_ids[best >= 0, best], topk_ids, lp
            return topk_ids[best >= 0, best]
