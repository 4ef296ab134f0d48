"""Caption head (reference: model/prismer_caption.py:14-121): training loss, answer ranking, generation."""
import torch

from .prismer import Prismer
from .rank import rank_answers
from ..trainer import check_text_rows


def tile(x, dim, n_tile):
    """prismer_caption.py:115-121: repeat each slice n_tile times consecutively."""
    return x.repeat_interleave(n_tile, dim=dim)


class PrismerCaption(Prismer):
    prompt_length = 4          # len(tokenizer('A picture of').input_ids) - 1 (prismer_caption.py:24-25) when ids are passed directly

    def _ids(self, text, device, **kw):
        """strings -> tokenizer (reference behaviour); dict/tuple of tensors -> used as given (offline path)."""
        if isinstance(text, dict):
            return text['input_ids'].to(device), text['attention_mask'].to(device)
        if isinstance(text, (tuple, list)) and len(text) == 2 and torch.is_tensor(text[0]):
            return text[0].to(device), text[1].to(device)
        t = self._tokenize(text, return_tensors='pt', **kw).to(device)
        return t.input_ids, t.attention_mask

    def forward(self, experts, caption=None, answer=None, train=True, prefix='', inference='generate', k_test=32, return_scores=False, sample=None,
                generate_args=None, texts_per_image=1):
        """texts_per_image=n (training): `caption` holds n captions per image, image-major (captions b*n .. b*n+n-1 describe image b: the order
        generate(num_return_sequences=n) returns).  The encoder runs once per image; the decoder's cross-attention shares an image's K/V among
        its n rows instead of reading an n-fold tiled encoder output.  The loss is the mean over the B*n rows.
        sample: None = the reference's fixed beam search; a dict of sampling arguments of `text_decoder.generate` (top_p, top_k, temperature,
        num_return_sequences, seed) routes inference='generate' through sampled decoding: B * num_return_sequences captions, image-major.
        generate_args: None, or a dict of further arguments of `text_decoder.generate` for the beam search (repetition_penalty,
        no_repeat_ngram_size); the `sample` dict carries them for sampled decoding."""
        device = experts['rgb'].device
        pad = self.text_decoder.config.pad_token_id
        if train:
            experts_train = self.expert_encoder(experts).permute(1, 0, 2)              # 'l b d -> b l d'
            input_ids, attention_mask = self._ids(caption, device, padding='longest', truncation=True, max_length=30)
            answer_targets = input_ids.masked_fill(input_ids == pad, -100)
            if isinstance(prefix, int):
                answer_targets[:, :prefix] = -100
            elif len(prefix) > 0:
                plen = len(self._tokenize(prefix).input_ids) - 1 if self.tokenizer is not None else self.prompt_length
                answer_targets[:, :plen] = -100
            check_text_rows(experts_train.shape[0], input_ids.shape[0], texts_per_image, 'PrismerCaption.forward')
            out = self.text_decoder(input_ids, attention_mask=attention_mask, encoder_hidden_states=experts_train, labels=answer_targets,
                                    return_dict=True)
            return out.loss.mean()
        with torch.no_grad():
            experts_train = self.expert_encoder(experts).permute(1, 0, 2)
            B = experts['rgb'].size(0)
            if inference == 'generate':
                if isinstance(prefix, str):
                    ids, att = self._ids([prefix] * B, device, padding='longest')
                else:
                    ids, att = self._ids(prefix, device)
                ids, att = ids[:, :-1], att[:, :-1]                                        # drop </s>
                if sample is None:
                    outputs = self.text_decoder.generate(input_ids=ids, encoder_hidden_states=experts_train, attention_mask=att, num_beams=3,
                                                         max_length=20, min_length=8, **(generate_args or {}))       # prismer_caption.py:45-50
                else:
                    outputs = self.text_decoder.generate(input_ids=ids, encoder_hidden_states=experts_train, attention_mask=att, do_sample=True,
                                                         max_length=20, min_length=8, **sample)
                if self.tokenizer is None:
                    return outputs
                captions = []
                for o in outputs:
                    cap = self.tokenizer.decode(o, skip_special_tokens=True)
                    captions.append(cap[len(prefix) + (1 if len(prefix) > 0 else 0):])
                return captions
            # inference == 'rank' (prismer_caption.py:59-112)
            if isinstance(answer, (list, tuple)) and answer and isinstance(answer[0], str):
                answer = [' ' + a.lower() + '</s>' for a in answer]
                a_ids, a_att = self._ids(answer, device, padding='longest', add_special_tokens=False)
            else:
                a_ids, a_att = self._ids(answer, device)
            if isinstance(prefix, str):
                s_ids, s_att = self._ids([prefix] * B, device, padding='longest')
            else:
                s_ids, s_att = self._ids(prefix, device)
            s_ids, s_att = s_ids[:, :-1], s_att[:, :-1]
            topk_ids, lp = rank_answers(self.text_decoder, experts_train, s_ids, s_att, a_ids, a_att, k_test, pad)
            best = lp.argmax(dim=1)
            if return_scores:                                   # (extension for the parity tests: the candidates and their scores)
                return topk_ids[best >= 0, best], topk_ids, lp
            return topk_ids[best >= 0, best]
