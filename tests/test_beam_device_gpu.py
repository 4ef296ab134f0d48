"""GPU: the device beam step (ph_beam_topk, ph_beam_advance, beam_search_device) and `generate` with one image's K/V shared by its beams.
  1. ph_beam_topk against float64 (identical (beam, token) at every rank, scores within 4x torch's own fp32 deviation);
  2. the tie rule (flat index ascending, bit-equal scores);  3. argument validation;
  4. beam_search_device == beam_search_from_logits(topk_fn=stable sort) token for token, reorder rows at every step;
  5. the heads: shared against tiled against the fp32 CPU oracle;  6. structure and memory of the shared layout.
Ties and near-ties: see tests/beam_util.py -- every case first checks its REFERENCE run for the 1e-4 separation and fails loudly without it.

Measured on the MI355X (test 1, largest deviation from float64 per case, printed by the test): torch's fp32 log_softmax + add 1.7e-8 ..
1.09e-6, ph_beam_topk 1.7e-8 .. 1.04e-6; at the eval shape (B = 32, 3 beams, V = 50 265) torch 8.3e-7 / kernel 1.04e-6 with one row per beam,
torch 1.09e-6 / kernel 9.3e-7 with one row per item; largest ratio kernel / torch 5.2 (4.0e-7 against 7.6e-8 at B = 1, 8 beams: under the
floor of 4 fp32 ulps = 1.9e-6 at |score| = 4 .. 8).  Bar: 4x torch's deviation, at least 4 fp32 ulps of the score."""
import numpy as np
import pytest
import torch

from tests import beam_util as U

pytestmark = pytest.mark.gpu
NEG = -1e9


# ------------------------------------------------------------------------------------------------------------ 1: top-k against float64
# (B, nb, nb_in, V, ld, seed): the seed of each shape is one whose REFERENCE satisfies the separation precondition with and without the
# EOS ban (found on the CPU by counting up from 1; `topk_reference` checks it again on every run)
TOPK_SHAPES = [(1, 1, 1, 23, 24, 1), (4, 3, 3, 23, 24, 1), (4, 8, 8, 23, 24, 1), (4, 3, 1, 1003, 1008, 1), (4, 3, 3, 1003, 1008, 1),
               (4, 8, 1, 1003, 1008, 1), (32, 3, 3, 50265, 50304, 1), (32, 3, 1, 50265, 50304, 1), (1, 8, 8, 50265, 50304, 1),
               (4, 1, 1, 50265, 50304, 1)]
EOS = 2


def topk_case(B, nb, nb_in, V, ld, seed):
    """bf16 logits [B*nb_in, ld] (columns >= V hold 1e4: a kernel that reads them as logits cannot pass) and fp32 beam scores; item 0 of a
    per-beam layout carries the start pattern (0, -1e9, ...), item 0 of a per-item layout the score 0"""
    g = torch.Generator().manual_seed(seed)
    R = B * nb_in
    buf = torch.full((R, ld), 1e4).bfloat16()
    buf[:, :V] = (torch.randn(R, V, generator=g) * 2.0).bfloat16()
    scores = -(torch.rand(B, nb_in, generator=g) * 6.0)
    scores[0] = 0.0
    if nb_in > 1:
        scores[0, 1:] = NEG
    return buf, scores.reshape(-1).contiguous()


def topk_reference(buf, scores, B, nb, nb_in, V, ban):
    """float64 log_softmax of the bf16 values + scores, stable descending sort.  Returns (score f64 [B, 2nb], beam, tok, problems)."""
    lp = torch.log_softmax(buf[:, :V].double(), dim=-1)
    if ban:
        lp[:, EOS] = -float('inf')
    cand = (scores.double().view(-1, 1) + lp).view(B, nb_in * V)
    s, i = torch.sort(cand, dim=1, descending=True, stable=True)
    K = 2 * nb
    problems = []
    for b in range(B):
        for r in range(K):
            a, c = float(s[b, r]), float(s[b, r + 1])
            if not ((a == c and int(i[b, r]) // V == int(i[b, r + 1]) // V) or a - c >= U.GAP):
                problems.append((b, r, a, c))
    return s[:, :K], i[:, :K] // V, i[:, :K] % V, problems


@pytest.mark.parametrize('ban', [False, True])
@pytest.mark.parametrize('B,nb,nb_in,V,ld,seed', TOPK_SHAPES)
def test_beam_topk_matches_float64(B, nb, nb_in, V, ld, seed, ban):
    from prismer_amd import ops
    buf, scores = topk_case(B, nb, nb_in, V, ld, seed)
    want_s, want_b, want_t, problems = topk_reference(buf, scores, B, nb, nb_in, V, ban)
    assert not problems, f'reference precondition violated (item, rank, score, next): {problems[:3]} -- choose another seed'
    dbuf, dscores = buf.cuda(), scores.cuda()
    top_s, top_b, top_t = ops.beam_topk(dbuf[:, :V], dscores, B, nb, EOS, ban)
    assert top_b.cpu().tolist() == want_b.tolist() and top_t.cpu().tolist() == want_t.tolist()
    # how far torch's own fp32 log_softmax + add lands from float64 on the same candidates
    t32 = (dscores.view(-1, 1) + torch.log_softmax(dbuf[:, :V].float(), dim=-1)).view(B, nb_in * V).cpu()
    t32 = t32.gather(1, (want_b * V + want_t))
    dev_torch = float((t32.double() - want_s).abs().max())
    err = (top_s.cpu().double() - want_s).abs()
    ulp = torch.from_numpy(np.spacing(want_s.abs().float().numpy())).double()
    print(f'beam_topk B={B} nb={nb} nb_in={nb_in} V={V} ban={ban}: max |fp32 - f64| torch {dev_torch:.3e} kernel {float(err.max()):.3e}')
    bar = torch.maximum(torch.full_like(err, 4 * dev_torch), 4 * ulp)
    assert bool((err <= bar).all()), (float(err.max()), dev_torch)


# ------------------------------------------------------------------------------------------------------------ 2: the tie rule
@pytest.mark.parametrize('V,ld,toks', [(1003, 1008, (7, 500, 1002)), (50265, 50304, (5, 20000, 50264))])
@pytest.mark.parametrize('nb', [3, 8])
def test_beam_topk_tie_rule(V, ld, toks, nb):
    from prismer_amd import ops
    B = 2
    g = torch.Generator().manual_seed(5)
    row = (torch.randn(B, 1, V, generator=g)).bfloat16()
    top = row.float().amax(dim=-1, keepdim=True) + 1.0
    for t in toks:
        row[:, :, t] = top[:, :, 0].bfloat16()
    buf = torch.zeros(B * nb, ld, dtype=torch.bfloat16)
    buf[:, :V] = row.expand(B, nb, V).reshape(B * nb, V)
    scores = torch.full((B * nb,), -1.5)
    top_s, top_b, top_t = [t.cpu() for t in ops.beam_topk(buf.cuda()[:, :V], scores.cuda(), B, nb, EOS, True)]
    want = [(bm, t) for bm in range(nb) for t in toks][:2 * nb]
    for b in range(B):
        got = list(zip(top_b[b].tolist(), top_t[b].tolist()))
        n = min(len(want), 3 * nb)
        assert got[:n] == want[:n], (b, got, want)
        assert len(set(top_s[b, :n].view(torch.int32).tolist())) == 1                          # bit-equal scores


# ------------------------------------------------------------------------------------------------------------ 3: argument validation
def test_beam_topk_rejects_bad_arguments():
    from prismer_amd import ops
    from prismer_amd._lib import PrismerHipError
    x = torch.zeros(36, 1008, dtype=torch.bfloat16, device='cuda')
    s = torch.zeros(36, device='cuda')
    with pytest.raises(PrismerHipError, match='num_beams 9 outside 1..8'):
        ops.beam_topk(x[:, :1003], s, 4, 9, EOS, False)
    with pytest.raises(PrismerHipError, match=r'vocabulary 6 below 2 \* num_beams \+ 1 = 7'):
        ops.beam_topk(x[:12, :6], s[:12], 4, 3, EOS, False)
    y = torch.zeros(12, 1003, dtype=torch.bfloat16, device='cuda')                             # row stride 1003: rows not 16-byte aligned
    with pytest.raises(PrismerHipError, match='16-byte aligned'):
        ops.beam_topk(y, s[:12], 4, 3, EOS, False)
    with pytest.raises(PrismerHipError, match='16-byte aligned'):
        ops.beam_topk(x[:12, 1:1004], s[:12], 4, 3, EOS, False)


# ------------------------------------------------------------------------------------------------------------ 4: the search
@pytest.mark.parametrize('lp,eos_boost', U.PAIRS)
@pytest.mark.parametrize('V,nb,seeds', U.CASES)
def test_beam_search_device_equals_specification(V, nb, seeds, lp, eos_boost):
    from prismer_amd.model.generate import beam_search_device, beam_search_from_logits
    ld = (V + 7) // 8 * 8
    for seed in seeds:
        prompt, lm = U.toy_case(V, seed, eos_boost)
        problems, want_rows, got_rows = [], [], []
        want = beam_search_from_logits(lm, prompt, nb, U.TMAX, U.TMIN, U.EOS, U.PAD, lp, topk_fn=U.checked_topk(nb, V, problems),
                                       reorder_fn=lambda r: want_rows.append(r.tolist()))
        assert not problems, f'precondition violated: {problems[:3]}'

        def step(ids):                                                      # the same bf16 logits, in the padded layout _lm_head writes
            buf = torch.full((ids.shape[0], ld), 1e4, dtype=torch.bfloat16)
            buf[:, :V] = lm(ids.cpu())
            return buf.cuda()[:, :V]
        got = beam_search_device(step, prompt.cuda(), nb, U.TMAX, U.TMIN, U.EOS, U.PAD, lp, reorder_fn=lambda r: got_rows.append(r.cpu().tolist()))
        assert got_rows == want_rows, (seed, got_rows, want_rows)
        assert [g.tolist() for g in got] == [w.tolist() for w in want], seed
        assert all(g.is_cuda and g.dtype == torch.long for g in got)


def test_beam_search_device_one_row_per_item_first_step():
    """a step function that answers the first step with one row per item (the per-image prefill): same tokens, source rows among B"""
    from prismer_amd.model.generate import beam_search_device
    V, nb, seed, lp, boost = 1003, 3, 2, 1.0, 2.5
    prompt, lm = U.toy_case(V, seed, boost)
    ld = 1008

    def run(per_item):
        rows = []

        def step(ids):
            if per_item and ids.shape[1] == prompt.shape[1]:
                ids = ids[::nb]
            buf = torch.full((ids.shape[0], ld), 1e4, dtype=torch.bfloat16)
            buf[:, :V] = lm(ids.cpu())
            return buf.cuda()[:, :V]
        out = beam_search_device(step, prompt.cuda(), nb, U.TMAX, U.TMIN, U.EOS, U.PAD, lp, reorder_fn=lambda r: rows.append(r.cpu().tolist()),
                                 rows_rep=2 if per_item else 1)
        return [o.tolist() for o in out], rows
    a, ra = run(False)
    b, rb = run(True)
    assert a == b
    Bb = U.B * nb
    assert [r // nb for r in ra[0]] == rb[0][:Bb] and rb[0][Bb:] == [Bb + r for r in rb[0][:Bb]]
    assert all(x == y[:Bb] and [Bb + r for r in x] == y[Bb:] for x, y in zip(ra[1:], rb[1:]))


# ------------------------------------------------------------------------------------------------------------ 5: the heads
def _states(name, B=None):
    from tests.test_rank_shared_gpu import _model
    case, enc, dec, esd, dsd = _model(name)
    x = case.inputs()[0]
    if B is not None:
        x = {k: ({kk: vv[:B] for kk, vv in v.items()} if isinstance(v, dict) else v[:B]) for k, v in x.items()}
    tab = case.instance_table(x)
    enc.instance_table = None if tab is None else torch.tensor(tab, dtype=torch.int32).cuda()
    xs = {k: ({kk: vv.cuda() for kk, vv in v.items()} if isinstance(v, dict) else v.cuda()) for k, v in x.items()}
    with torch.no_grad():
        e = enc(xs).permute(1, 0, 2).contiguous()
    return case, dec, dsd, e


@pytest.mark.parametrize('name,lp', [('tiny_caption', 1.0), ('tiny_vqa', -1.0), ('base_b8', 1.0)])
def test_generate_shared_equals_tiled_and_oracle(name, lp):
    from oracle import prismer_oracle as O
    from oracle.beam_oracle import beam_search_loops
    from prismer_amd.model.generate import beam_search
    case, dec, dsd, e = _states(name, B=4 if name == 'base_b8' else None)
    d = case.dims
    B, nb = e.shape[0], 3
    prompt = torch.tensor([[0, 83 % d.vocab_size, 170 % d.vocab_size, 9]] * B)
    att = torch.ones_like(prompt)
    if name == 'tiny_vqa' and B > 1:
        att[1, 2] = 0; prompt[1, 2] = d.pad_token_id            # a pad inside one question (VQA questions are padded to the longest)
    kw = dict(num_beams=nb, max_length=14, min_length=8, eos_token_id=d.eos_token_id, pad_token_id=d.pad_token_id, length_penalty=lp)
    with torch.no_grad():
        shared = beam_search(dec, prompt.cuda(), att.cuda(), e, share_image=True, **kw)
        tiled = beam_search(dec, prompt.cuda(), att.cuda(), e, share_image=False, **kw)
    shared, tiled = [s.tolist() for s in shared], [t.tolist() for t in tiled]
    if name == 'base_b8':
        # random-init BASE weights give near-uniform next-token distributions over 50 265 words: bf16 noise between two decoders can swap a
        # near-tied continuation, so identity is required for all but one item (the allowance of tests/test_generate_gpu.py)
        assert sum(s == t for s, t in zip(shared, tiled)) >= B - 1, (shared, tiled)
    else:
        assert shared == tiled
    enc_cpu = e.float().cpu()
    att_l = att.tolist()

    def mask(rows, owner):                                              # the prompt's mask, generated positions are real tokens
        T = len(rows[0])
        return torch.tensor([att_l[o] + [1] * (T - len(att_l[o])) for o in owner])

    def step_list(rows):
        ids = torch.tensor(rows)
        owner = [r // nb for r in range(len(rows))]
        with torch.no_grad():
            lg, _ = O.text_decoder(dsd, ids, mask(rows, owner), enc_cpu.repeat_interleave(nb, 0), d.num_attention_heads)
        return torch.log_softmax(lg[:, -1].double(), -1).tolist()
    want = beam_search_loops(step_list, prompt.tolist(), nb, 14, 8, d.eos_token_id, d.pad_token_id, lp)
    same = sum(s == w for s, w in zip(shared, want))
    print(name, 'hypotheses identical to the fp32 oracle:', same, 'of', B, shared, want)

    def score(tokens, b):                                               # the hypothesis under the ORACLE's model
        ids = torch.tensor([tokens])
        with torch.no_grad():
            lg, _ = O.text_decoder(dsd, ids, mask([tokens], [b]), enc_cpu[[b]], d.num_attention_heads)
        lp_ = torch.log_softmax(lg[0].double(), -1)
        s = sum(float(lp_[t - 1, tokens[t]]) for t in range(prompt.shape[1], len(tokens)))
        n = len(tokens) - (1 if tokens[-1] == d.eos_token_id else 0)
        return s / (n ** lp)
    for b, (s, w) in enumerate(zip(shared, want)):
        if s != w:
            assert abs(score(s, b) - score(w, b)) < 0.05 * abs(score(w, b)) + 0.05, (s, w)
    assert same >= 1


# ------------------------------------------------------------------------------------------------------------ 6: structure and memory
def test_generate_shares_image_kv_structure_and_memory():
    """BASE decoder, B = 8 images of S = 260 tokens, 3 beams.  The K/V of every cross-attention layer hold B*S rows, and one generate call adds
    less than B*nb*S*2H*L*2 bytes = 8*3*260*18432*2 = 230 MB -- the size of the tiled layout's K/V buffer alone -- while the tiled layout in the
    same process exceeds it.  Both bounds are arithmetic on shapes."""
    from prismer_amd.model.generate import beam_search
    from tests.test_rank_shared_gpu import _model
    case, _, dec, _, _ = _model('base_b8')
    d = case.dims
    B, S, nb, Tmax = 8, 260, 3, 20
    H, L = d.hidden_size, d.num_hidden_layers
    bound = B * nb * S * 2 * H * L * 2
    assert bound == 8 * 3 * 260 * 18432 * 2
    g = torch.Generator().manual_seed(43)
    e = (torch.randn(B, S, d.vision_hidden_size, generator=g) * 0.5).to(torch.bfloat16).cuda()
    prompt = torch.tensor([[0, 83, 2170, 9]] * B).cuda()
    att = torch.ones_like(prompt)
    prog, enc_bf = dec.decoding_program(e)
    st = prog.decode_begin(enc_bf, Tmax, beams=nb)
    assert len(st['kvs']) == L and all(kv.shape[0] == B * S for kv in st['kvs'])
    assert st['cache'][0].shape[1] == B * nb
    del st

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        with torch.no_grad():
            out = fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, out
    gen = lambda: dec.generate(input_ids=prompt, encoder_hidden_states=e, attention_mask=att, num_beams=nb, max_length=Tmax, min_length=8,
                               length_penalty=1.0)
    kw = dict(num_beams=nb, max_length=Tmax, min_length=8, eos_token_id=d.eos_token_id, pad_token_id=d.pad_token_id, length_penalty=1.0)
    peak(gen)                                                           # warm-up (library workspaces, first launches)
    shared, out = peak(gen)
    tiled, _ = peak(lambda: beam_search(dec, prompt, att, e, share_image=False, **kw))
    print('generate peak bytes added: shared', shared, 'tiled', tiled, 'bound', bound)
    assert out.shape[0] == B and out.shape[1] <= Tmax
    assert shared < bound, (shared, bound)
    assert tiled > bound, (tiled, bound)
