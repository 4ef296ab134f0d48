"""CPU: repetition_penalty and no_repeat_ngram_size of `generate` -- the specification prismer_amd/model/generate.py::decode_edits against the
installed transformers processors (bit for bit), the beam search with them against both loop-form oracle readings, the sampling filter,
argument validation, the ABI of the two new entry points (host-side rejection, no GPU needed), and "options off changes nothing"."""
import ctypes as C

import pytest
import torch

from prismer_amd.model import generate as G
from tests import edits_util as E
from tests import sample_util as S

transformers = pytest.importorskip('transformers')
COVER = {'banned': 0, 'penalised': 0}
COVER5 = {'banned': 0, 'penalised': 0}


# ------------------------------------------------------------------------------------------------ 1: decode_edits == transformers
def _edit_case(V, seed, cur):
    g = torch.Generator().manual_seed(seed)
    R = 4
    x = (torch.randn(R, V, generator=g) * 3.0).bfloat16().float()
    ids = torch.randint(3, 9, (R, cur), generator=g)                    # a 6-token alphabet: repeats and n-gram matches occur
    x[0, int(ids[0, 0])] = 0.0                                          # a zero logit in the history
    x[1, int(ids[1, -1])] = -float('inf')                               # a -inf column in the history
    x[2, int(ids[2, 0])] = 2.0 ** -130                                  # a subnormal one (a product / quotient that rounds)
    return ids, x


@pytest.mark.parametrize('n', range(5))
@pytest.mark.parametrize('theta', [1, 1.2, 0.8, 2.5])
@pytest.mark.parametrize('V', [12, 50, 1003])
def test_decode_edits_equals_transformers_processors(V, theta, n):
    for seed, cur in enumerate([1, 2, 3, 5, 9, 14]):                    # cur < n included
        ids, x = _edit_case(V, 100 * V + seed, cur)
        y, banned = G.decode_edits(ids, x, theta, n)
        assert y.dtype == torch.float32 and banned.dtype == torch.bool
        got = torch.where(banned, torch.full_like(y, -float('inf')), y)
        want = E.hf_edit(ids, x, theta, n)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (V, theta, n, cur)
        assert torch.equal(got.bfloat16().view(torch.int16), want.bfloat16().view(torch.int16))
        if n == 0 or cur < n:
            assert not bool(banned.any())
        if n == 1:
            assert int(banned.sum()) == sum(len(set(r)) for r in ids.tolist())


def test_decode_edits_ignores_tokens_outside_the_vocabulary():
    V = 12
    x = torch.linspace(-3, 3, V).repeat(2, 1)
    ids = torch.tensor([[3, V + 5, 4, V + 5, -1], [V, V, V, V, V]])
    y, banned = G.decode_edits(ids, x, 2.0, 2)
    assert not bool(banned[1].any()) and torch.equal(y[1], x[1])
    touched = (y[0] != x[0]).nonzero().flatten().tolist()
    assert touched == [3, 4] and not bool(banned[0].any())
    y, banned = G.decode_edits(torch.tensor([[3, V + 5, 4, 7, V + 5]]), x[:1], 1.0, 2)
    assert banned[0].nonzero().flatten().tolist() == [4]               # the out-of-range token still takes part in the MATCH; it is never banned itself
    y64, _ = G.decode_edits(ids, x.double(), 2.0, 2)
    assert y64.dtype == torch.float64


# ------------------------------------------------------------------------------------------------ 2: beam search, both oracle readings
@pytest.mark.parametrize('eos_boost', [0.0, 3.0])
@pytest.mark.parametrize('theta,n', E.BEAM_EDITS)
@pytest.mark.parametrize('seed', range(3))
def test_beam_search_with_edits_matches_loop_oracle(seed, theta, n, eos_boost):
    from oracle.beam_oracle import beam_search_loops
    V, B, nb, T0, Tmax, Tmin = 23, 4, 3, 3, 12, 6
    lm = E.repeat_lm(V, seed, eos_boost)
    g = torch.Generator().manual_seed(1000 + seed)
    prompt = torch.randint(3, V, (B, T0), generator=g)
    prompt[:, 0] = 0
    got = G.beam_search_from_logits(lm, prompt, nb, Tmax, Tmin, E.EOS, E.PAD, 1.0, repetition_penalty=theta, no_repeat_ngram_size=n)
    step_list = lambda rows: torch.log_softmax(lm(torch.tensor(rows)).float(), -1).tolist()
    want = beam_search_loops(E.wrap_list_step(step_list, theta, n, COVER), prompt.tolist(), nb, Tmax, Tmin, E.EOS, E.PAD, 1.0)
    assert [o.tolist() for o in got] == want
    if theta != 1:
        COVER['penalised'] += E.count_repeats(want, T0, E.EOS, E.PAD)
    if n > 0:
        for row in want:
            grams = [tuple(row[i:i + n]) for i in range(len(row) - n + 1)]
            assert len(grams) == len(set(grams)), (n, row)


@pytest.mark.parametrize('eos_bias', [0.0, 3.0])
@pytest.mark.parametrize('theta,n', E.BEAM_EDITS)
@pytest.mark.parametrize('seed', range(3))
def test_v5_loops_with_processors_reproduce_installed_generate(seed, theta, n, eos_bias):
    from oracle.beam_oracle import beam_search_loops_v5
    from tests.test_oracle_beam_vs_transformers import _tiny_lm
    vocab, nb, lp = 12, 3, 1.0
    m = _tiny_lm(seed, vocab, eos_bias)
    g = torch.Generator().manual_seed(100 + seed)
    B, plen, Tmax, Tmin = 3, 3, 11, 5
    prompt = torch.randint(3, vocab, (B, plen), generator=g)
    with torch.no_grad():
        out = m.generate(input_ids=prompt, attention_mask=torch.ones_like(prompt), num_beams=nb, max_length=Tmax, min_length=Tmin,
                         length_penalty=lp, early_stopping=False, do_sample=False, eos_token_id=1, pad_token_id=2, use_cache=True,
                         repetition_penalty=float(theta), no_repeat_ngram_size=n)

    def step(rows):
        with torch.no_grad():
            logits = m(input_ids=torch.tensor(rows)).logits[:, -1].float()
        return torch.log_softmax(logits, -1).tolist()
    want = beam_search_loops_v5(E.wrap_list_step(step, theta, n, COVER5), prompt.tolist(), nb, Tmax, Tmin, 1, 2, lp)
    if theta != 1:
        COVER5['penalised'] += E.count_repeats(want, plen, 1, 2)
    for b in range(B):
        got = out[b].tolist()
        while len(got) > len(want[b]) and got[-1] == 2:
            got.pop()
        assert got == want[b], (b, got, want[b])


def test_the_beam_cases_above_ban_and_penalise():
    """(runs after the parametrised cases) the n-gram rule removed candidates and penalised tokens were chosen all the same"""
    assert COVER['banned'] >= 1 and COVER['penalised'] >= 1, COVER
    assert COVER5['banned'] >= 1 and COVER5['penalised'] >= 1, COVER5


# ------------------------------------------------------------------------------------------------ 3: sampling
@pytest.mark.parametrize('theta,n', E.GPU_EDITS)
@pytest.mark.parametrize('setting', S.SETTINGS)
def test_sample_kept_set_is_processors_then_bf16_then_filter(setting, theta, n):
    V, R, cur = S.V_SMALL, 4, 9
    x = S.bf16_rows(31, 4.0, R, V).float()
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(3, 9, (R, cur), generator=g)
    top = x.topk(4, dim=1).indices
    ids[:, 0], ids[:, 4] = top[:, 0], top[:, 2]                         # leaders of the row are in the history
    y, banned = G.decode_edits(ids, x, theta, n)
    keep, z = G.sample_filter(y.bfloat16().float(), *setting, banned=banned)
    ref = E.hf_edit(ids, x, theta, n).bfloat16().float()
    keep_ref, z_ref = G.sample_filter(ref, *setting)
    assert torch.equal(keep, keep_ref) and bool(keep.any(dim=1).all())
    assert torch.equal(z[keep], z_ref[keep])
    keep_eos, _ = G.sample_filter(y.bfloat16().float(), *setting, banned_col=E.EOS, banned=banned)
    assert not bool(keep_eos[:, E.EOS].any()) and not bool((keep_eos & banned).any())


def test_sampling_with_unigram_blocking_never_repeats_a_token():
    V, B, n_seq, T0, Tmax = 23, 3, 2, 2, 12
    lm = E.repeat_lm(V, 3, 0.0)
    prompt = torch.tensor([[0, 5], [0, 6], [0, 9]])
    g = torch.Generator().manual_seed(1)
    u = torch.rand(B * n_seq, Tmax, generator=g)
    kw = dict(num_return_sequences=n_seq, max_length=Tmax, min_length=4, top_k=0, top_p=0.95, eos_token_id=E.EOS, pad_token_id=E.PAD, uniforms=u)
    plain, _ = G.sample_from_logits(lm, prompt, **kw)
    assert E.count_repeats(plain.tolist(), T0, E.EOS, E.PAD) > 0, 'the case does not repeat without the rule'
    ids, lp = G.sample_from_logits(lm, prompt, no_repeat_ngram_size=1, **kw)
    for row in ids.tolist():
        body = row[:row.index(E.EOS)] if E.EOS in row[T0:] else row
        body = [t for t in body if t != E.PAD]
        assert len(body) == len(set(body)), row
    assert bool(torch.isfinite(lp).all())


# ------------------------------------------------------------------------------------------------ 4: validation and ABI
@pytest.mark.parametrize('bad', [dict(repetition_penalty=0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float('nan')),
                                 dict(repetition_penalty=float('inf')), dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=1.5)])
def test_edit_argument_validation(bad):
    with pytest.raises(ValueError):
        G.check_edit_args(**bad)
    lm = E.repeat_lm(23, 1, 0.0)
    prompt = torch.tensor([[0, 5]])
    with pytest.raises(ValueError):
        G.beam_search_from_logits(lm, prompt, 2, 6, 0, E.EOS, E.PAD, **bad)
    with pytest.raises(ValueError):
        G.sample_from_logits(lm, prompt, max_length=6, **bad)
    with pytest.raises(ValueError):
        G.decode_edits(prompt, torch.zeros(1, 23), **bad)
    G.check_edit_args(1.0, 0)
    G.check_edit_args(1, 3)
    G.check_edit_args(2.5, 2.0)


def test_generate_validates_the_edit_arguments_in_both_modes():
    from prismer_amd.modules.roberta import RobertaForCausalLMModified as M
    ids = torch.tensor([[0, 5]])
    for mode in (dict(num_beams=3), dict(do_sample=True)):
        for bad in (dict(repetition_penalty=0.0), dict(no_repeat_ngram_size=-1)):
            with pytest.raises(ValueError, match='repetition_penalty|no_repeat_ngram_size'):
                M.generate(object(), input_ids=ids, encoder_hidden_states=None, **mode, **bad)


def test_edit_entry_points_abi_without_gpu():
    """both symbols resolve, the revision stays 106, and out-of-range edit arguments are rejected on the host before any launch"""
    from prismer_amd import _lib
    lib = _lib.lib
    assert lib.ph_version() == 106 and _lib.EDIT_MAX_CUR == 512 == G.EDIT_MAX_CUR
    assert 'ph_beam_topk_edit' in _lib.EXPORTS and 'ph_sample_step_edit' in _lib.EXPORTS
    assert callable(lib.ph_beam_topk_edit) and callable(lib.ph_sample_step_edit)

    def topk(ids=64, ids_ld=600, cur=5, theta=1.3, n=2):
        a = _lib.BeamTopkArgs()
        a.logits = a.beam_scores = a.workspace = a.top_score = a.top_beam = a.top_tok = 64
        a.ld, a.V, a.B, a.nb, a.nb_in, a.eos_token_id, a.workspace_bytes = 1008, 1003, 2, 3, 3, 2, 1 << 30
        return lib.ph_beam_topk_edit(C.byref(a), ids, ids_ld, cur, theta, n, None), lib.ph_last_error()

    def step(cur=5, Tmax=600, theta=1.3, n=2):
        a = _lib.SampleStepArgs()
        a.logits = a.ids = a.done = a.seq_logprob = 64
        a.ld, a.V, a.R, a.rows_per_logit, a.Tmax, a.cur, a.temperature, a.top_p = 1008, 1003, 2, 1, Tmax, cur, 1.0, 1.0
        return lib.ph_sample_step_edit(C.byref(a), theta, n, None), lib.ph_last_error()
    for kw, msg in [(dict(cur=0), b'history length'), (dict(cur=513), b'history length'), (dict(theta=0.0), b'repetition_penalty'),
                    (dict(theta=float('nan')), b'repetition_penalty'), (dict(theta=float('inf')), b'repetition_penalty'),
                    (dict(n=-1), b'no_repeat_ngram_size')]:
        for fn in (topk, step):
            rc, err = fn(**kw)
            assert rc == -1 and msg in err, (fn.__name__, kw, rc, err)
    rc, err = topk(ids=None)
    assert rc == -1 and b'null ids' in err
    rc, err = topk(ids_ld=4)
    assert rc == -1 and b'history length' in err
    rc, err = step(cur=5, Tmax=5)                                       # ... and the limits of the plain entry point still hold
    assert rc == -1 and b'position' in err


# ------------------------------------------------------------------------------------------------ 5: options off
def test_options_off_change_nothing():
    V = 23
    lm = E.repeat_lm(V, 2, 2.5)
    prompt = torch.tensor([[0, 5, 7], [0, 6, 6]])
    x = S.bf16_rows(3, 3.0, 2, V).float()
    y, banned = G.decode_edits(prompt, x, 1.0, 0)
    assert torch.equal(y.view(torch.int32), x.view(torch.int32)) and not bool(banned.any())
    a = G.beam_search_from_logits(lm, prompt, 3, 12, 6, E.EOS, E.PAD, 1.0, topk_fn=G.stable_topk)
    b = G.beam_search_from_logits(lm, prompt, 3, 12, 6, E.EOS, E.PAD, 1.0, topk_fn=G.stable_topk, repetition_penalty=1.0, no_repeat_ngram_size=0)
    assert [t.tolist() for t in a] == [t.tolist() for t in b]
    kw = dict(num_return_sequences=2, max_length=12, min_length=4, top_p=0.9, eos_token_id=E.EOS, pad_token_id=E.PAD, seed=11)
    (ia, la), (ib, lb) = G.sample_from_logits(lm, prompt, **kw), G.sample_from_logits(lm, prompt, repetition_penalty=1.0, no_repeat_ngram_size=0, **kw)
    assert torch.equal(ia, ib) and torch.equal(la.view(torch.int32), lb.view(torch.int32))
    for setting in S.SETTINGS:
        (ka, za), (kb, zb) = G.sample_filter(x, *setting, banned_col=E.EOS), G.sample_filter(x, *setting, banned_col=E.EOS, banned=None)
        assert torch.equal(ka, kb) and torch.equal(za, zb)
