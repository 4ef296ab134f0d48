"""CPU: the continuation layout of shared-prefix rank inference (prismer_amd/model/rank.py) against the reference's tiled layout
(model/prismer_vqa.py:64-113, model/prismer_caption.py:59-112): for ragged, right-padded questions and answers, every scored token has the
same position id, label and visible key set in both, and every row the same number of targets."""
import pytest
import torch

from prismer_amd.model.rank import continuation_layout

PAD = 1


def _ragged(g, n, T, lens, lo=3, hi=500):
    ids = torch.randint(lo, hi, (n, T), generator=g)
    att = torch.ones(n, T, dtype=torch.long)
    for i, L in enumerate(lens):
        ids[i, L:] = PAD
        att[i, L:] = 0
    return ids, att


def _position_ids(ids):
    """create_position_ids_from_input_ids (roberta.py:38-45)"""
    m = (ids != PAD).long()
    return torch.cumsum(m, 1) * m + PAD


@pytest.mark.parametrize('Tq,q_lens', [(7, [7, 3, 5, 1]), (1, [1, 1, 1, 1]), (2, [1, 2, 2, 1])])
def test_continuation_layout_reproduces_tiled_tokens(Tq, q_lens):
    g = torch.Generator().manual_seed(5)
    B, k, n_ans, Ta = len(q_lens), 3, 6, 5
    q_ids, q_att = _ragged(g, B, Tq, q_lens)
    q_ids[:, 0] = 0                                                    # <s>
    a_ids, a_att = _ragged(g, n_ans, Ta, [1 + i % Ta for i in range(n_ans)])
    topk = torch.stack([torch.randperm(n_ans, generator=g)[:k] for _ in range(B)])
    flat = topk.reshape(-1)
    ans_ids, ans_att = a_ids[flat], a_att[flat]
    # the reference's tiled rows
    rep = torch.arange(B).repeat_interleave(k)
    t_ids = torch.cat([q_ids[rep], ans_ids], 1)
    t_att = torch.cat([q_att[rep], ans_att], 1)
    t_tgt = t_ids.masked_fill(t_ids == PAD, -100)
    t_tgt[:, :-Ta] = -100
    t_pos = _position_ids(t_ids)
    # the continuation rows
    c_ids, c_att, c_lab, base = continuation_layout(q_ids, q_att, ans_ids, ans_att, k, PAD)
    Tp, Tc = Tq - 1, Ta + 1
    assert c_ids.shape == (B * k, Tc) and base.dtype == torch.int32
    c_pos = torch.where(c_ids != PAD, PAD + base[:, None].long() + torch.cumsum((c_ids != PAD).long(), 1), torch.full_like(c_ids, PAD))
    # the tokens the shared path drops are never scored: they precede the continuation and carry no target
    assert (t_tgt[:, :Tp] == -100).all()
    assert torch.equal((t_tgt != -100).sum(1), (c_lab != -100).sum(1))                 # #targets
    for r in range(B * k):
        b = r // k
        for c in range(Tc):
            p = Tp + c                                                  # tiled position of continuation token c
            assert int(c_ids[r, c]) == int(t_ids[r, p])
            assert int(c_pos[r, c]) == int(t_pos[r, p]), (r, c)
            assert int(c_lab[r, c]) == int(t_tgt[r, p]), (r, c)         # shifted CE: logits at c score label c + 1 in both layouts
            tiled_keys = {j for j in range(p + 1) if t_att[r, j]}
            shared_keys = {j for j in range(Tp) if q_att[b, j]} | {Tp + j for j in range(c + 1) if c_att[r, j]}
            assert tiled_keys == shared_keys, (r, c)
    # the first answer token is scored from the last question position, also where that position is a pad
    assert (c_lab[:, 1] == torch.where(ans_ids[:, 0] == PAD, -100, ans_ids[:, 0])).all()
