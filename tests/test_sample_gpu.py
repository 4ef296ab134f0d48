"""GPU: the sampled decoding step of the library (ph_sample_step through ops.sample_step), the device loop (sample_device) and the public
surface (decoder.generate(do_sample=True), the caption head's `sample=`) against the float64 row model of tests/sample_util.py, which
follows the specification prismer_amd/model/generate.py::sample_from_logits.

EPS.  The kernel sums class masses in fp32 in a fixed order: at most 64 bin terms inside a thread, a 6-step scan inside a wave, 16 wave
totals -- a relative error of about (64 + 6 + 16) * 2^-24 = 5e-6 -- and takes exp with v_exp_f32 on an fp32 argument of magnitude <= 20
wherever the term matters (2.4e-6).  Bound 8e-6; EPS = 1e-4 of probability mass is 12x that."""
import numpy as np
import pytest
import torch

from tests import sample_util as S
from tests.sample_util import SETTINGS, RowModel

pytestmark = pytest.mark.gpu

EPS = 1e-4
EOS, PAD = 2, 1
_rows_cache = {}


def rows_of(kind):
    """(bf16 rows [R, V], exact): exact = the boundary margin is asserted and the kept set must equal the specification's"""
    if kind not in _rows_cache:
        small = S.bf16_rows(S.SMALL_SEED, S.SMALL_SCALE, 1, S.V_SMALL)
        _rows_cache[kind] = {
            'big8_1': lambda: (S.bf16_rows(11, 8.0, 3, S.V_BIG)[:1], True),
            'big8_3': lambda: (S.bf16_rows(11, 8.0, 3, S.V_BIG), True),
            'big2_3': lambda: (S.bf16_rows(12, 2.0, 3, S.V_BIG), False),
            'small_96': lambda: (small.repeat(96, 1), True),
            'small_3': lambda: (small.repeat(3, 1), True),
            'tiny_5': lambda: (S.bf16_rows(13, 2.0, 5, 8), False),
        }[kind]()
    return _rows_cache[kind]


_models = {}


def model_of(x, setting, banned):
    """the RowModel of a row, computed once and shared among the cases that use the row"""
    key = (x.tobytes(), setting, banned)
    if key not in _models:
        _models[key] = RowModel(x, *setting, banned=banned)
    return _models[key]


def launch(xdev, R, Tmax, cur, setting, ban, done0, lp0, seed):
    from prismer_amd import ops
    T, k, p = setting
    dev = xdev.device
    ids = torch.full((R, Tmax), 7, dtype=torch.long, device=dev)
    done = done0.clone().to(dev)
    lp = lp0.clone().to(dev)
    diag = (torch.empty(R, device=dev), torch.empty(R, device=dev), torch.empty(R, dtype=torch.int32, device=dev), torch.empty(R, device=dev))
    ops.sample_step(xdev, ids, done, lp, cur, T, k, p, EOS, PAD, ban, seed, diag=diag)
    torch.cuda.synchronize()
    return [t.cpu() for t in (ids, done, lp) + diag]


def kept_models(m, setting):
    """the kept sets the tolerance form admits: n highest classes with mass(kept) >= top_p - EPS and mass(kept minus its lowest class) <
    top_p + EPS; for top_p = 1 everything that survived top-k"""
    p = setting[2]
    if p >= 1:
        return [len(m.vals)]
    cum = np.cumsum(m.mass)
    return [n for n in range(1, len(m.vals) + 1) if cum[n - 1] >= p - EPS and (cum[n - 2] if n > 1 else 0.0) < p + EPS]


def token_ok(m, setting, tok, u):
    keep_n = m.n_keep_classes
    try:
        for n in kept_models(m, setting):
            m.set_classes(n)
            if m.interval_ok(tok, u, EPS):
                return True
        return False
    finally:
        m.set_classes(keep_n)


CASES = [  # kind, ld, view offset columns, cur, ban, done rows
    ('big8_1', 50304, 0, 3, False, ()),
    ('big8_3', 50304, 0, 3, False, ()),
    ('big2_3', 50304, 0, 5, False, ()),
    ('small_96', 1008, 0, 0, False, ()),
    ('tiny_5', 8, 0, 2, False, ()),
    ('small_3', 1024, 8, 4, False, ()),              # a strided view: ld > V + 8, rows start 16 bytes into the buffer's rows
    ('big8_3', 50304, 0, 2, True, ()),               # cur < min_length: EOS, the row's best logit, is banned
    ('small_96', 1008, 0, 6, False, (0, 5, 95)),     # some rows already done
]


@pytest.mark.parametrize('setting', SETTINGS)
@pytest.mark.parametrize('kind,ld,off,cur,ban,done_rows', CASES)
def test_sample_step_against_float64(kind, ld, off, cur, ban, done_rows, setting):
    x, exact = rows_of(kind)
    x = x.clone()
    R, V = x.shape
    if ban:
        x[:, EOS] = x.float().max(dim=1).values.bfloat16() + 1
    Tmax, seed = 9, 0xABCDEF0123 + cur
    buf = torch.full((R, ld), 1e4, dtype=torch.bfloat16)
    buf[:, off:off + V] = x
    xdev = buf.cuda()[:, off:off + V]
    done0 = torch.zeros(R, dtype=torch.int32)
    done0[list(done_rows)] = 1
    lp0 = torch.linspace(-3, -1, R)
    out = launch(xdev, R, Tmax, cur, setting, ban, done0, lp0, seed)
    again = launch(xdev, R, Tmax, cur, setting, ban, done0, lp0, seed)
    for a, b in zip(out, again):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), \
            'two launches on the same inputs differ'
    ids, done, lp, u, thr, kcnt, kmass = out
    want_u = S.uniforms_mirror(R, cur, seed)
    assert torch.equal(u.view(torch.int32), want_u.view(torch.int32)), 'u_out is not the Philox mirror'
    other = torch.ones(Tmax, dtype=torch.bool)
    other[cur] = False
    assert bool((ids[:, other] == 7).all()), 'a column other than `cur` was written'
    xf = x.float().numpy()
    p = setting[2]
    for r in range(R):
        tok = int(ids[r, cur])
        if r in done_rows:
            assert tok == PAD and int(done[r]) == 1 and float(lp[r]) == float(lp0[r])
            continue
        m = model_of(xf[r], setting, EOS if ban else None)
        kept = m.cand & (m.x >= float(thr[r]))
        assert int(kept.sum()) == int(kcnt[r]), (r, int(kept.sum()), int(kcnt[r]))
        if exact:
            assert m.margin() > S.MARGIN, f'row {r}: a class boundary within {S.MARGIN} of top_p, the case is not clean'
            assert np.array_equal(kept, m.keep), (r, int(kept.sum()), int(m.keep.sum()))
        n = int((m.vals >= float(thr[r])).sum())
        assert n in kept_models(m, setting) and np.array_equal(kept, m.elig & (m.x >= m.vals[n - 1])), (r, n, kept_models(m, setting))
        assert abs(float(kmass[r]) - float(np.cumsum(m.mass)[n - 1])) <= EPS
        keep_n = m.n_keep_classes
        m.set_classes(n)
        ok = m.interval_ok(tok, float(u[r]), EPS)
        m.set_classes(keep_n)
        assert ok, (r, tok, float(u[r]))
        assert abs((float(lp[r]) - float(lp0[r])) - m.logprob(tok)) <= 1e-4
        assert int(done[r]) == int(tok == EOS)
        assert not (ban and tok == EOS)


def test_sample_step_rejects_bad_arguments():
    from prismer_amd import ops
    from prismer_amd._lib import PrismerHipError
    dev = 'cuda'
    st = lambda R, Tmax: (torch.zeros(R, Tmax, dtype=torch.long, device=dev), torch.zeros(R, dtype=torch.int32, device=dev), torch.zeros(R, device=dev))
    big = torch.zeros(1, 65536, dtype=torch.bfloat16, device=dev)
    ok = torch.zeros(2, 1008, dtype=torch.bfloat16, device=dev)
    with pytest.raises(PrismerHipError, match='vocabulary'):
        ops.sample_step(big, *st(1, 4), 1, 1.0, 0, 1.0, EOS, PAD, False, 0)
    with pytest.raises(PrismerHipError, match='aligned'):
        ops.sample_step(torch.zeros(2, 1004, dtype=torch.bfloat16, device=dev)[:, :1003], *st(2, 4), 1, 1.0, 0, 1.0, EOS, PAD, False, 0)
    with pytest.raises(PrismerHipError, match='aligned'):
        ops.sample_step(ok[:, 1:1004], *st(2, 4), 1, 1.0, 0, 1.0, EOS, PAD, False, 0)
    with pytest.raises(PrismerHipError, match='position'):
        ops.sample_step(ok[:, :1003], *st(2, 4), 4, 1.0, 0, 1.0, EOS, PAD, False, 0)
    with pytest.raises(PrismerHipError, match='temperature'):
        ops.sample_step(ok[:, :1003], *st(2, 4), 1, 0.0, 0, 1.0, EOS, PAD, False, 0)
    ids, done, lp = st(2, 4)
    ops.sample_step(ok[:, :1003], ids, done, lp, 1, 1.0, 0, 1.0, EOS, PAD, False, 0)          # ... and the valid call goes through
    torch.cuda.synchronize()
    assert bool((ids[:, 1] >= 0).all()) and bool((ids[:, 1] < 1003).all())


def _check_rows(ids, prompt_rows, T0, Tmin):
    """the bookkeeping rules on final rows [R, L]: the prompt, no EOS before min_length, only pad after the first EOS"""
    assert torch.equal(ids[:, :T0], prompt_rows)
    for row in ids.tolist():
        gen = row[T0:]
        if EOS in gen:
            e = gen.index(EOS)
            assert T0 + e >= Tmin and all(t == PAD for t in gen[e + 1:]), row


@pytest.mark.parametrize('per_image', [False, True])
def test_sample_device_loop_against_specification(per_image):
    from prismer_amd.model.generate import sample_device, sample_from_logits
    V, ld, B, n, T0, Tmax, Tmin, seed = 1003, 1008, 3, 2, 2, 10, 4, 99
    setting = (1.0, 0, 0.9)
    R = B * n
    rec, reorders = {}, []

    def logits_at(T):                                                       # a function of the position alone: both forms see the same rows
        if T not in rec:
            x = S.bf16_rows(700 + T, 3.0, R, V)
            x[:, EOS] += 6                                                  # EOS likely once it is allowed
            x[:, PAD] = float('-inf')
            if per_image and T == T0:
                x = x[::n].repeat_interleave(n, dim=0)
            rec[T] = x
        return rec[T]

    def step(ids):
        T = ids.shape[1]
        x = logits_at(T)
        if per_image and T == T0:
            x = x[::n]
        buf = torch.full((x.shape[0], ld), 1e4, dtype=torch.bfloat16)
        buf[:, :V] = x
        return buf.cuda()[:, :V]
    prompt = torch.tensor([[0, 5], [0, 6], [0, 9]])
    kw = dict(num_return_sequences=n, max_length=Tmax, min_length=Tmin, temperature=setting[0], top_k=setting[1], top_p=setting[2],
              eos_token_id=EOS, pad_token_id=PAD, seed=seed)
    got, got_lp = sample_device(step, prompt.cuda(), reorder_fn=lambda rows: reorders.append(rows.cpu().tolist()), rows_rep=2, **kw)
    assert got.is_cuda and got.dtype == torch.long
    got, got_lp = got.cpu(), got_lp.cpu()
    assert reorders == ([[r // n for r in range(R)] + [R + r // n for r in range(R)]] if per_image else [])
    _check_rows(got, prompt.repeat_interleave(n, dim=0), T0, Tmin)
    want, want_lp = sample_from_logits(lambda ids: logits_at(ids.shape[1]), prompt, **kw)
    L = got.shape[1]
    ref_lp = np.zeros(R)
    for r in range(R):
        same = True                                                         # the two forms agree on the row so far
        for t in range(T0, L):
            m = RowModel(rec[t][r].float().numpy(), *setting, banned=EOS if t < Tmin else None)
            u = float(S.uniforms_mirror(R, t, seed)[r])
            tok = int(got[r, t])
            assert token_ok(m, setting, tok, u), (r, t, tok, u)
            ref_lp[r] += m.logprob(tok)
            if same and int(want[r, t]) != tok:                             # they part only where the interval admits both tokens
                assert token_ok(m, setting, int(want[r, t]), u), (r, t, tok, int(want[r, t]))
                same = False
            if tok == EOS:
                break
    assert np.abs(got_lp.double().numpy() - ref_lp).max() <= 1e-4 * (L - T0)


@pytest.fixture(scope='module')
def tiny():
    from tests.test_rank_shared_gpu import _model
    case, enc, dec, esd, dsd = _model('tiny_caption')
    x = case.inputs()[0]
    tab = case.instance_table(x)
    enc.instance_table = None if tab is None else torch.tensor(tab, dtype=torch.int32).cuda()
    xs = {k: ({kk: vv.cuda() for kk, vv in v.items()} if isinstance(v, dict) else v.cuda()) for k, v in x.items()}
    with torch.no_grad():
        e2 = enc(xs).permute(1, 0, 2).contiguous()
    e = torch.cat([e2, e2[:1].flip(1)], dim=0).contiguous()                 # a third image: the case holds two
    d = case.dims
    B = 3
    prompt = torch.tensor([[0, 83 % d.vocab_size, 170 % d.vocab_size, 9]] * B)
    prompt[1, 1] = 11
    return dict(case=case, enc=enc, dec=dec, xs=xs, e=e, e2=e2, prompt=prompt.cuda(), att=torch.ones_like(prompt).cuda(), B=B)


def _rules(ids, prompt, n, T0, Tmin, eos, pad):
    assert torch.equal(ids[:, :T0].cpu(), prompt.cpu().repeat_interleave(n, dim=0))
    for row in ids.tolist():
        gen = row[T0:]
        if eos in gen:
            e = gen.index(eos)
            assert T0 + e >= Tmin and all(t == pad for t in gen[e + 1:]), row


@pytest.mark.parametrize('n', [1, 4])
def test_generate_do_sample(tiny, n):
    from prismer_amd.model.generate import sample
    dec, e, prompt, att, B = tiny['dec'], tiny['e'], tiny['prompt'], tiny['att'], tiny['B']
    d = tiny['case'].dims
    kw = dict(input_ids=prompt, encoder_hidden_states=e, attention_mask=att, do_sample=True, top_p=0.9, num_return_sequences=n, max_length=14,
              min_length=8)
    a = dec.generate(seed=7, **kw)
    assert a.shape[0] == B * n and 4 < a.shape[1] <= 14 and a.dtype == torch.long
    _rules(a, prompt, n, 4, 8, d.eos_token_id, d.pad_token_id)
    b, lp = dec.generate(seed=7, return_logprobs=True, **kw)
    assert torch.equal(a, b) and lp.shape == (B * n,) and bool((lp < 0).all())
    c = dec.generate(seed=8, **kw)
    assert c.shape != a.shape or not torch.equal(a, c)
    if n > 1:
        rows = a.view(B, n, -1)
        assert all(not bool((rows[i] == rows[i, :1]).all()) for i in range(B)), 'the n samples of an image are all the same'
    t, _ = sample(dec, prompt, att, e, num_return_sequences=n, max_length=14, min_length=8, top_p=0.9, eos_token_id=d.eos_token_id,
                  pad_token_id=d.pad_token_id, seed=7, share_image=False)
    assert t.shape[0] == B * n
    _rules(t, prompt, n, 4, 8, d.eos_token_id, d.pad_token_id)
    torch.manual_seed(5)
    dec._sample_calls = 0
    s1, s2 = dec.generate(**kw), dec.generate(**kw)
    dec._sample_calls = 0
    assert torch.equal(s1, dec.generate(**kw)) and (s1.shape != s2.shape or not torch.equal(s1, s2))


def test_generate_without_sampling_is_the_beam_search(tiny):
    from prismer_amd.model.generate import beam_search
    dec, e, prompt, att, B = tiny['dec'], tiny['e'], tiny['prompt'], tiny['att'], tiny['B']
    d = tiny['case'].dims
    got = dec.generate(input_ids=prompt, encoder_hidden_states=e, attention_mask=att, num_beams=3, max_length=14, min_length=8, do_sample=False,
                       some_unknown_keyword=1)
    outs = beam_search(dec, prompt, att, e, num_beams=3, max_length=14, min_length=8, eos_token_id=d.eos_token_id, pad_token_id=d.pad_token_id)
    L = max(o.numel() for o in outs)
    assert got.shape == (B, L)
    for i, o in enumerate(outs):
        assert got[i, :o.numel()].tolist() == o.tolist() and bool((got[i, o.numel():] == d.pad_token_id).all())


def test_caption_head_sample_argument(tiny):
    from prismer_amd.model.prismer_caption import PrismerCaption
    from tests.test_rank_shared_gpu import _head
    dec, B = tiny['dec'], tiny['e2'].shape[0]                               # the head runs the encoder: the case's own images
    d = tiny['case'].dims
    m = _head(PrismerCaption, tiny['enc'], dec)
    prompt = tiny['prompt'][:B]
    ids = torch.cat([prompt.cpu(), torch.full((B, 1), d.eos_token_id)], dim=1)
    prefix = (ids, torch.ones_like(ids))
    out = m(tiny['xs'], train=False, prefix=prefix, inference='generate', sample=dict(top_p=0.9, temperature=1.0, top_k=0, num_return_sequences=5, seed=1))
    assert out.shape[0] == B * 5 and out.shape[1] <= 20
    _rules(out, prompt, 5, 4, 8, d.eos_token_id, d.pad_token_id)
    ref = dec.generate(input_ids=prompt, encoder_hidden_states=tiny['e2'], attention_mask=tiny['att'][:B], num_beams=3, max_length=20, min_length=8)
    assert torch.equal(m(tiny['xs'], train=False, prefix=prefix, inference='generate', sample=None), ref)
    assert torch.equal(m(tiny['xs'], train=False, prefix=prefix, inference='generate'), ref)
