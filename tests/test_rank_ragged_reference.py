"""CPU: O.rank_answers (the oracle of inference='rank') against the reference's OWN rank code (model/prismer_vqa.py:64-113,
model/prismer_caption.py:59-112) on right-padded questions of DIFFERENT lengths -- the case where the last question position of a
shorter question is a pad and still scores the first answer token -- and on the empty caption prompt (`prefix=''`: the prompt is <s>
alone).  tests/test_oracle_golden.py pins all-ones question masks only."""
import random

import pytest
import torch

from oracle import prismer_oracle as O
from oracle import ref_harness as RH
from tests.golden import cases as C


class _Batch:
    def __init__(self, ids, att):
        self.input_ids, self.attention_mask = ids, att

    def to(self, device):
        return self


class _Tokenizer:
    """every string the reference head builds is looked up in a table of pre-tokenised rows (already padded to the longest)"""
    pad_token_id = 1

    def __init__(self, table):
        self.table = table

    def __call__(self, texts, padding=None, return_tensors=None, add_special_tokens=True, **kw):
        rows = [self.table[t] for t in texts]
        return _Batch(torch.stack([r[0] for r in rows]), torch.stack([r[1] for r in rows]))


@pytest.mark.skipif(not RH.available(), reason='reference not mounted')
@pytest.mark.parametrize('head', ['vqa_ragged', 'caption_empty_prefix'])
def test_oracle_rank_matches_reference_on_ragged_prompts(head):
    import torch.nn as nn
    RH._import_reference()
    import model.prismer_caption as RC
    import model.prismer_vqa as RV
    case = C.Case('tiny_vqa')
    d = case.dims
    esd, dsd = case.weights()
    x, _, _, _, _ = case.inputs()
    enc, dec = RH.build_reference(d, esd, dsd)
    B = x['rgb'].shape[0]
    g = torch.Generator().manual_seed(23)
    n_ans, Ta, k = 12, 5, 6
    a_ids = torch.randint(3, d.vocab_size, (n_ans, Ta), generator=g)
    a_att = torch.ones(n_ans, Ta, dtype=torch.long)
    for i in range(n_ans):                                              # ragged answers ending in </s>
        L = 2 + i % (Ta - 1)
        a_ids[i, L - 1] = d.eos_token_id
        a_ids[i, L:] = d.pad_token_id; a_att[i, L:] = 0
    answers = [f'answer {i}' for i in range(n_ans)]
    table = {}
    if head == 'vqa_ragged':
        Tq = 8
        lens = [Tq, 3, 5, 2][:B]
        assert len(set(lens)) == B and min(lens) < Tq
        start_ids = torch.randint(3, d.vocab_size, (B, Tq), generator=g); start_ids[:, 0] = d.bos_token_id
        start_att = torch.ones(B, Tq, dtype=torch.long)
        for b, L in enumerate(lens):
            start_ids[b, L:] = d.pad_token_id; start_att[b, L:] = 0        # right-padded: the last position is a pad for all but one
        questions = [f'question {b}' for b in range(B)]
        for b, q in enumerate(questions):
            table['<s>' + q.capitalize()] = (start_ids[b], start_att[b])   # prismer_vqa.py:18-20
        for i, a in enumerate(answers):
            table[' ' + a.capitalize() + '</s>'] = (a_ids[i], a_att[i])    # prismer_vqa.py:68
        cls = RV.PrismerVQA
    else:
        table[''] = (torch.tensor([d.bos_token_id, d.eos_token_id]), torch.ones(2, dtype=torch.long))
        for i, a in enumerate(answers):
            table[' ' + a.lower() + '</s>'] = (a_ids[i], a_att[i])        # prismer_caption.py:64
        start_ids, start_att = torch.full((B, 1), d.bos_token_id), torch.ones(B, 1, dtype=torch.long)
        cls = RC.PrismerCaption
    m = cls.__new__(cls)
    nn.Module.__init__(m)
    m.expert_encoder, m.text_decoder, m.tokenizer = enc, dec, _Tokenizer(table)
    random.seed(C.INSTANCE_SEED)
    with torch.no_grad():
        if head == 'vqa_ragged':
            want = m(x, questions, answer=answers, train=False, inference='rank', k_test=k)
        else:
            want = m(x, answer=answers, train=False, prefix='', inference='rank', k_test=k)
        tab = case.instance_table(x)
        eo = O.vision_encoder(esd, x, d.patch_size, d.vit_heads, False, tab)
        best, topk, lp = O.rank_answers(dsd, eo.transpose(0, 1), start_ids, start_att, a_ids, a_att, k, d.num_attention_heads,
                                        pad=d.pad_token_id)
    assert best.tolist() == want.tolist(), (best, want, lp)
