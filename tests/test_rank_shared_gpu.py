"""GPU: shared-prefix rank inference (prismer_amd/model/rank.py).  ph_attention_prefix_fwd and ph_embed_fwd_offset against torch
references; the caption and VQA heads on ragged questions against the oracle (O.rank_answers) and against the tiled layout in the same
process; the memory the rank call adds, shared against tiled."""
import functools

import pytest
import torch

from oracle import prismer_oracle as O
from prismer_amd import ops
from prismer_amd._lib import PrismerHipError
from prismer_amd.model import rank as RK
from prismer_amd.model.prismer import _Cfg
from prismer_amd.modules.roberta import RobertaForCausalLMModified
from prismer_amd.modules.vit import VisionTransformer
from tests.golden import cases as C
from tests.util import rel_fro

pytestmark = pytest.mark.gpu
DH = 64


# ------------------------------------------------------------------------------------------------------------ kernel
def _prefix_case(g, nP, group, Tp, Tc, H, Tmax_extra=3):
    """prefix K | V in a decode-cache layout [nP, Tmax, 2*H*dh]; continuation q | k | v in a QKV GEMM layout [R*Tc, 3*H*dh]"""
    R, W = nP * group, H * DH
    Tmax = Tp + Tmax_extra
    gd = torch.Generator(device='cuda').manual_seed(int(torch.randint(0, 1 << 30, (1,), generator=g)))
    cache = torch.randn(nP, Tmax, 2 * W, generator=gd, device='cuda').to(torch.bfloat16)
    qkv = torch.randn(R * Tc, 3 * W, generator=gd, device='cuda').to(torch.bfloat16)
    pm = (torch.rand(nP, Tmax, generator=g) > 0.3).to(torch.uint8)
    pm[:, 0] = 1
    if Tp > 0:
        pm[0, Tp - 1] = 0                                                       # a masked last prefix position
    cm = torch.ones(R, Tc, dtype=torch.uint8)
    for r in range(R):                                                          # ragged continuation masks (right-padded answers)
        n = 1 + (r * 7) % Tc
        cm[r, n:] = 0
        if r % 3 == 1:
            cm[r, 0] = 0                                                        # the question's last token is a pad
    return cache, qkv, pm.cuda(), cm.cuda(), Tmax


def _prefix_reference(cache, qkv, pm, cm, nP, group, Tp, Tc, H):
    """fp32 torch: ph_attention_fwd semantics on the concatenated keys [prefix, continuation], queries at positions Tp .. Tp+Tc-1"""
    R, W = nP * group, H * DH
    src = torch.arange(R, device=cache.device) // group
    pk = cache[:, :Tp, :W].float()[src]
    pv = cache[:, :Tp, W:].float()[src]
    x = qkv.float().view(R, Tc, 3 * W)
    q, ck, cv = x[..., :W], x[..., W:2 * W], x[..., 2 * W:]
    k = torch.cat([pk, ck], 1).view(R, Tp + Tc, H, DH).transpose(1, 2)
    v = torch.cat([pv, cv], 1).view(R, Tp + Tc, H, DH).transpose(1, 2)
    q = q.view(R, Tc, H, DH).transpose(1, 2)
    s = q @ k.transpose(-1, -2) * DH ** -0.5                                    # [R, H, Tc, Tp+Tc]
    live = torch.cat([pm[src, :Tp].bool(), cm.bool()], 1)[:, None, None, :]
    causal = torch.ones(Tc, Tc, dtype=torch.bool, device=s.device).tril()
    vis = torch.cat([torch.ones(Tc, Tp, dtype=torch.bool, device=s.device), causal], 1)[None, None]
    s = s.masked_fill(~(live & vis), torch.finfo(torch.float32).min)
    o = torch.softmax(s, -1) @ v
    return o.transpose(1, 2).reshape(R * Tc, W)


def _run_prefix(cache, qkv, pm, cm, nP, group, Tp, Tc, H, Tmax):
    W = H * DH
    cs, qs = (Tmax * 2 * W, 2 * W), (Tc * 3 * W, 3 * W)
    return ops.attention_prefix_fwd(qkv[:, :W], cache[:, :, :W], cache[:, :, W:], qkv[:, W:2 * W], qkv[:, 2 * W:], nP * group, H, Tc, Tp,
                                    group, DH, q_strides=qs, pk_strides=cs, pv_strides=cs, ck_strides=qs, cv_strides=qs, prefix_mask=pm,
                                    pm_stride=pm.stride(0), cont_mask=cm, cm_stride=Tc)


@pytest.mark.parametrize('group', [1, 5, 128])
@pytest.mark.parametrize('Tp', [0, 1, 7, 31, 33, 288])
def test_attention_prefix_matches_concatenated_reference(group, Tp):
    g = torch.Generator().manual_seed(1000 * group + Tp)
    nP = 3 if group < 128 else 2
    for Tc in (1, 2, 9, 32):
        for H in (12, 16):
            cache, qkv, pm, cm, Tmax = _prefix_case(g, nP, group, Tp, Tc, H)
            got = _run_prefix(cache, qkv, pm, cm, nP, group, Tp, Tc, H, Tmax)
            want = _prefix_reference(cache, qkv, pm, cm, nP, group, Tp, Tc, H)
            err = rel_fro(got.float(), want)
            assert err < 8e-3, (group, Tp, Tc, H, err)


def test_attention_prefix_rejects_out_of_range_arguments():
    g = torch.Generator().manual_seed(3)
    cache, qkv, pm, cm, Tmax = _prefix_case(g, 1, 1, 8, 4, 12)
    W = 12 * DH
    base = dict(q_strides=(4 * 3 * W, 3 * W), pk_strides=(Tmax * 2 * W, 2 * W), pv_strides=(Tmax * 2 * W, 2 * W), ck_strides=(4 * 3 * W, 3 * W),
                cv_strides=(4 * 3 * W, 3 * W), out=torch.empty(64 * W, dtype=torch.bfloat16, device='cuda').view(-1, W))
    args = (qkv[:, :W], cache[:, :, :W], cache[:, :, W:], qkv[:, W:2 * W], qkv[:, 2 * W:])
    with pytest.raises(PrismerHipError, match='Tc = 33'):
        ops.attention_prefix_fwd(*args, 1, 12, 33, 8, 1, DH, **base)
    with pytest.raises(PrismerHipError, match='Tp = 289'):
        ops.attention_prefix_fwd(*args, 1, 12, 4, 289, 1, DH, **base)
    with pytest.raises(PrismerHipError, match='head dim 96'):
        ops.attention_prefix_fwd(*args, 1, 8, 4, 8, 1, 96, **base)


def test_embed_offset_matches_torch_with_reference_position_ids():
    g = torch.Generator().manual_seed(11)
    R, T, H, V, P, pad = 37, 9, 768, 1000, 514, 1
    ids = torch.randint(3, V, (R, T), generator=g)
    for r in range(R):
        ids[r, 1 + r % T:] = pad
        if r % 4 == 0:
            ids[r, 0] = pad                                                     # a pad before real tokens (the question's last position)
    base = torch.randint(0, 40, (R,), generator=g, dtype=torch.int32)
    word, pos = torch.randn(V, H, generator=g) * 0.5, torch.randn(P, H, generator=g) * 0.5
    typ, gamma, beta = torch.randn(1, H, generator=g) * 0.5, 1 + 0.1 * torch.randn(H, generator=g), 0.1 * torch.randn(H, generator=g)
    dev = [t.cuda() for t in (ids, word, pos, typ, gamma, beta, base)]
    h, _, _, hf = ops.embed_fwd(dev[0], *dev[1:6], 1e-5, pad, None, want_f32=True, pos_base=dev[6])
    real = (ids != pad).long()
    pid = torch.where(ids != pad, pad + base[:, None].long() + torch.cumsum(real, 1), torch.full_like(ids, pad))   # roberta.py:38-45, shifted
    want = torch.nn.functional.layer_norm(word[ids] + typ[0] + pos[pid], (H,), gamma, beta, 1e-5).view(R * T, H)
    assert rel_fro(hf, want) < 1e-4 and rel_fro(h.float(), want) < 8e-3
    h0, _, _ = ops.embed_fwd(dev[0], *dev[1:6], 1e-5, pad, None, pos_base=torch.zeros(R, dtype=torch.int32, device='cuda'))
    h1, _, _ = ops.embed_fwd(dev[0], *dev[1:6], 1e-5, pad, None)
    assert torch.equal(h0, h1)                                                  # base 0 = ph_embed_fwd


# ------------------------------------------------------------------------------------------------------------ heads
@functools.lru_cache(maxsize=None)
def _model(name):
    case = C.Case(name)
    d = case.dims
    enc = VisionTransformer(d.image_resolution, d.patch_size, d.width, d.vit_layers, d.vit_heads, dict(d.experts))
    dec = RobertaForCausalLMModified(_Cfg(d.roberta_config_dict()))
    esd, dsd = case.weights()
    enc.load_state_dict(esd, strict=True)
    dec.load_state_dict(dsd, strict=True)
    enc.cuda().eval(); dec.cuda().eval()
    return case, enc, dec, esd, dsd


def _head(cls, enc, dec):
    m = cls.__new__(cls)
    torch.nn.Module.__init__(m)
    m.tokenizer = None
    m.expert_encoder, m.text_decoder = enc, dec
    return m


def _inputs(case, head, B):
    d = case.dims
    x, _, _, _, _ = case.inputs()
    B = min(B, x['rgb'].shape[0])
    x = {k: ({kk: vv[:B] for kk, vv in v.items()} if isinstance(v, dict) else v[:B]) for k, v in x.items()}
    g = torch.Generator().manual_seed(29)
    n_ans, Ta = 12, 5
    a_ids = torch.randint(3, d.vocab_size, (n_ans, Ta), generator=g)
    a_att = torch.ones(n_ans, Ta, dtype=torch.long)
    for i in range(n_ans):                                              # ragged answers ending in </s>, padded to the longest
        L = 2 + i % (Ta - 1)
        a_ids[i, L - 1] = d.eos_token_id
        a_ids[i, L:] = d.pad_token_id; a_att[i, L:] = 0
    if head == 'caption':
        q_ids = torch.tensor([[0, 83 % d.vocab_size, 2170 % d.vocab_size, 9]] * B)
        q_att = torch.ones(B, 4, dtype=torch.long)
    else:
        Tq = 9
        q_ids = torch.randint(3, d.vocab_size, (B, Tq), generator=g); q_ids[:, 0] = d.bos_token_id
        q_att = torch.ones(B, Tq, dtype=torch.long)
        for b in range(B):                                              # ragged, right-padded questions
            L = Tq - (b * 3) % (Tq - 1)
            q_ids[b, L:] = d.pad_token_id; q_att[b, L:] = 0
    return x, q_ids, q_att, a_ids, a_att


def _encode(m, case, x):
    tab = case.instance_table(x)
    m.expert_encoder.instance_table = None if tab is None else torch.tensor(tab, dtype=torch.int32).cuda()
    xs = {k: ({kk: vv.cuda() for kk, vv in v.items()} if isinstance(v, dict) else v.cuda()) for k, v in x.items()}
    return xs, tab


def _check_scores(B, k, topk, lp, want_topk, want_lp, want_best, best):
    agree = 0
    for b in range(B):
        score = {int(i): float(s) for i, s in zip(topk[b], lp[b])}
        wscore = {int(i): float(s) for i, s in zip(want_topk[b], want_lp[b])}
        common = sorted(set(score) & set(wscore))
        assert len(common) >= k - 1, (b, topk[b].tolist(), want_topk[b].tolist())
        for i in common:
            assert abs(score[i] - wscore[i]) < 2e-2 * abs(wscore[i]) + 2e-2, (b, i, score[i], wscore[i])
        srt = sorted(wscore.values(), reverse=True)
        if srt[0] - srt[1] > 5e-2:
            assert int(best[b]) == int(want_best[b]), (b, score, wscore)
        agree += int(best[b]) == int(want_best[b])
    assert agree >= B - 1


@pytest.mark.parametrize('name,head', [('tiny_vqa', 'caption'), ('tiny_vqa', 'vqa'), ('base_b8', 'caption'), ('base_b8', 'vqa')])
def test_rank_shared_matches_oracle_and_tiled_on_ragged_questions(name, head):
    from prismer_amd.model.prismer_caption import PrismerCaption
    from prismer_amd.model.prismer_vqa import PrismerVQA
    case, enc, dec, esd, dsd = _model(name)
    d = case.dims
    m = _head(PrismerCaption if head == 'caption' else PrismerVQA, enc, dec)
    x, q_ids, q_att, a_ids, a_att = _inputs(case, head, 4)
    B, k = q_ids.shape[0], 5
    assert RK.shared_ok(dec, q_ids.shape[1], a_ids.shape[1])
    xs, tab = _encode(m, case, x)
    if head == 'caption':                                               # the head drops the prompt's </s> (prismer_caption.py:70-71)
        prefix = (torch.cat([q_ids, torch.full((B, 1), d.eos_token_id)], 1), torch.cat([q_att, torch.ones(B, 1, dtype=torch.long)], 1))
        got = m(xs, answer=(a_ids, a_att), train=False, prefix=prefix, inference='rank', k_test=k, return_scores=True)
    else:
        got = m(xs, (q_ids, q_att), answer=(a_ids, a_att), train=False, inference='rank', k_test=k, return_scores=True)
    best, topk, lp = [t.cpu() for t in got]
    with torch.no_grad():
        eo = O.vision_encoder(esd, x, d.patch_size, d.vit_heads, False, tab)
        want_best, want_topk, want_lp = O.rank_answers(dsd, eo.transpose(0, 1), q_ids, q_att, a_ids, a_att, k, d.num_attention_heads,
                                                       pad=d.pad_token_id)
    print(name, head, 'best', best.tolist(), want_best.tolist())
    _check_scores(B, k, topk, lp, want_topk, want_lp, want_best, best)
    # the private tiled path on the same encoder states, same bars
    with torch.no_grad():
        e = enc(xs).permute(1, 0, 2)
        tq, tl = RK._rank_tiled(dec, e, q_ids.cuda(), q_att.cuda(), a_ids.cuda(), a_att.cuda(), k, d.pad_token_id)
        sq, sl = RK._rank_shared(dec, e, q_ids.cuda(), q_att.cuda(), a_ids.cuda(), a_att.cuda(), k, d.pad_token_id)
    tq, tl, sq, sl = tq.cpu(), tl.cpu(), sq.cpu(), sl.cpu()
    _check_scores(B, k, sq, sl, tq, tl, tq[torch.arange(B), tl.argmax(1)], sq[torch.arange(B), sl.argmax(1)])


def test_rank_memory_shared_against_tiled():
    """BASE decoder, S = 260 image tokens, B = 4 images, k = 64 candidates of <= 8 tokens: the shared path adds <= 1 GiB; the tiled path's merged
    cross-attention K/V buffer alone is 4*64*260*18432*2 B = 2.45 GB, and its peak is at least twice the shared one"""
    case, enc, dec, _, _ = _model('base_b8')
    d = case.dims
    B, S, k, n_ans, Ta, Tq = 4, 260, 64, 200, 8, 12
    g = torch.Generator().manual_seed(41)
    e = (torch.randn(B, S, d.vision_hidden_size, generator=g) * 0.5).to(torch.bfloat16).cuda()
    q_ids = torch.randint(3, d.vocab_size, (B, Tq), generator=g); q_ids[:, 0] = d.bos_token_id
    q_att = torch.ones(B, Tq, dtype=torch.long)
    q_ids[1, 7:] = d.pad_token_id; q_att[1, 7:] = 0
    a_ids = torch.randint(3, d.vocab_size, (n_ans, Ta), generator=g)
    a_att = torch.ones(n_ans, Ta, dtype=torch.long)
    for i in range(n_ans):
        L = 1 + i % Ta
        a_ids[i, L:] = d.pad_token_id; a_att[i, L:] = 0
    args = [t.cuda() for t in (q_ids, q_att, a_ids, a_att)]

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        with torch.no_grad():
            out = fn(dec, e, *args, k, d.pad_token_id)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, [t.cpu() for t in out]
    peak(RK._rank_shared)                                               # warm-up (library workspaces, first launches)
    shared, (sq, sl) = peak(RK._rank_shared)
    tiled, (tq, tl) = peak(RK._rank_tiled)
    print('rank peak bytes: shared', shared, 'tiled', tiled)
    assert shared <= 1 << 30, shared
    assert tiled >= 2 * shared, (tiled, shared)
    _check_scores(B, k, sq, sl, tq, tl, tq[torch.arange(B), tl.argmax(1)], sq[torch.arange(B), sl.argmax(1)])
