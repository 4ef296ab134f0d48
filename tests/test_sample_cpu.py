"""CPU: the specification of sampled decoding, prismer_amd/model/generate.py::sample_from_logits -- its filter against transformers'
TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper, its draw against a float64 cumulative sum in the defined order, its
generator against the Philox mirror of tests/util.py, the bookkeeping of transformers' _sample, and the argument checks."""
import types

import numpy as np
import pytest
import torch

from prismer_amd.model.generate import sample, sample_filter, sample_from_logits, sample_uniforms
from tests.sample_util import SETTINGS, SMALL_SCALE, SMALL_SEED, V_BIG, V_SMALL, RowModel, bf16_rows, uniforms_mirror
from tests.test_generate_cpu import make_lm

ROWS = {'flat': lambda: bf16_rows(21, 2.0, 1, V_BIG), 'peaked': lambda: bf16_rows(22, 8.0, 1, V_BIG),
        'small': lambda: bf16_rows(SMALL_SEED, SMALL_SCALE, 1, V_SMALL)}


@pytest.mark.parametrize('setting', SETTINGS)
@pytest.mark.parametrize('row', sorted(ROWS))
def test_filter_against_transformers_warpers(row, setting):
    """transformers' kept set is a subset of ours, and every extra token of ours has exactly the logit of transformers' lowest kept token:
    the one defined difference (the boundary tie class stays whole)"""
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    T, k, p = setting
    x = ROWS[row]().float()
    scores = TemperatureLogitsWarper(float(T))(None, x.clone())
    if k > 0:
        scores = TopKLogitsWarper(top_k=k)(None, scores)
    if p < 1:
        scores = TopPLogitsWarper(top_p=p)(None, scores)
    theirs = torch.isfinite(scores)[0]
    ours = sample_filter(x, T, k, p)[0][0]
    assert bool(theirs.any()) and bool((ours | ~theirs).all()), 'transformers keeps a token the specification drops'
    extra = ours & ~theirs
    assert bool((x[0][extra] == x[0][theirs].min()).all()), 'an extra token lies outside transformers\' boundary tie class'
    m = RowModel(x[0].numpy(), T, k, p)                            # ... and the tensor code is the rule of the float64 row model
    assert np.array_equal(ours.numpy(), m.keep)


def _one_step(x, uniforms, **kw):
    """sample_from_logits for a single position over fixed logit rows x [R, V]"""
    R = x.shape[0]
    prompt = torch.zeros(R, 1, dtype=torch.long)
    U = torch.zeros(R, 2)
    U[:, 1] = uniforms
    ids, lp = sample_from_logits(lambda ids: x, prompt, max_length=2, uniforms=U, eos_token_id=V_SMALL + 7, **kw)
    return ids[:, 1], lp


@pytest.mark.parametrize('setting', SETTINGS)
def test_draw_is_the_inverse_cdf_in_the_defined_order(setting):
    T, k, p = setting
    us = torch.tensor([0.0, 1e-7, 0.1, 0.3, 0.5, 0.77, 0.9, 0.999, 1 - 2.0 ** -24])
    x = bf16_rows(SMALL_SEED, SMALL_SCALE, 1, V_SMALL)
    x[0, 17] = x[0, 400] = x[0, 3] = x.max()                           # a tie class at the top: ids 3 < 17 < 400 (and the arg-max itself)
    m = RowModel(x[0].float().numpy(), T, k, p)
    tok, lp = _one_step(x.repeat(len(us), 1), us, temperature=T, top_k=k, top_p=p)
    assert tok.tolist() == [m.draw(float(u)) for u in us]
    assert int(tok[0]) == int(np.nonzero(m.x == m.x.max())[0][0]), 'u = 0: the arg-max with the lowest id among ties'
    ref = torch.tensor([m.logprob(int(t)) for t in tok])
    assert float((lp.double() - ref.double()).abs().max()) <= 1e-5


def test_generator_is_the_philox_mirror_bitwise():
    seed = 0x1234_5678_9ABC_DEF1
    for cur in (0, 3, 19):
        a, b = sample_uniforms(7, cur, seed), uniforms_mirror(7, cur, seed)
        assert a.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert float(a.min()) >= 0 and float(a.max()) < 1
    lm, prompt = _toy()
    kw = dict(num_return_sequences=2, max_length=9, min_length=4, top_k=0, top_p=0.9, seed=seed)
    R = prompt.shape[0] * 2
    U = torch.stack([uniforms_mirror(R, c, seed) for c in range(9)], dim=1)
    got, want = sample_from_logits(lm, prompt, **kw), sample_from_logits(lm, prompt, uniforms=U, **kw)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    other = sample_from_logits(lm, prompt, **dict(kw, seed=seed + 1))
    assert other[0].shape != got[0].shape or not torch.equal(other[0], got[0])


def _toy(V=23, seed=3, eos_boost=3.0):
    lm = make_lm(V, seed, 2, eos_boost)
    g = torch.Generator().manual_seed(50 + seed)
    prompt = torch.randint(3, V, (3, 3), generator=g)

    def logits(ids):
        x = lm(ids).bfloat16()
        x[:, 1] = float('-inf')                                             # the pad id is no token of the toy language
        return x
    return logits, prompt


@pytest.mark.parametrize('seed', range(4))
def test_bookkeeping(seed):
    """no EOS before min_length, only pad after the first EOS, model log-probability of the drawn tokens from the RAW logits"""
    lm, prompt = _toy(seed=seed)
    rec = []

    def step(ids):
        rec.append(lm(ids))
        return rec[-1]
    n, T0, Tmax, Tmin = 4, 3, 12, 6
    ids, lp = sample_from_logits(step, prompt, num_return_sequences=n, max_length=Tmax, min_length=Tmin, temperature=1.3, top_k=0, top_p=0.95,
                                 seed=seed)
    R, L = ids.shape
    assert R == 3 * n and T0 < L <= Tmax and torch.equal(ids[:, :T0], prompt.repeat_interleave(n, dim=0))
    assert len(rec) == L - T0, 'the loop stops once every row is done'
    ref = np.zeros(R)
    for r in range(R):
        row = ids[r].tolist()
        ended = False
        for t in range(T0, L):
            if ended:
                assert row[t] == 1
                continue
            assert row[t] != 1 and not (row[t] == 2 and t < Tmin)
            ref[r] += RowModel(rec[t - T0][r].float().numpy(), 1.0, 0, 1.0).logprob(row[t])
            ended = row[t] == 2
    assert L == Tmax or bool((ids == 2).any(dim=1).all())
    assert np.abs(lp.double().numpy() - ref).max() <= 1e-5
    assert bool((ids == 2).any()), 'the toy model never drew EOS: the case checks nothing'


def test_row_without_candidates_emits_eos_and_the_loop_stops():
    V = 16
    calls = []

    def step(ids):
        calls.append(ids.shape[1])
        x = torch.zeros(ids.shape[0], V)
        x[0] = float('nan')                                                 # nothing to draw from
        x[1, :] = float('-inf')
        x[1, 2] = 0.0                                                       # EOS is the only finite column, and banned while cur < min_length
        x[2, 2] = 60.0                                                      # EOS as good as certain once allowed
        return x.bfloat16()
    ids, lp = sample_from_logits(step, torch.zeros(3, 2, dtype=torch.long), max_length=10, min_length=4, top_k=0, seed=5)
    assert ids[0].tolist() == [0, 0, 2, 1, 1] and ids[1].tolist() == [0, 0, 2, 1, 1]
    assert ids[2, 4] == 2 and not bool((ids[2, :4] == 2).any())
    assert calls == [2, 3, 4] and float(lp[0]) == 0.0 and float(lp[1]) == 0.0


def test_argument_validation():
    dec = types.SimpleNamespace(config=types.SimpleNamespace(vocab_size=23, pad_token_id=1, eos_token_id=2))
    ids, att, enc = torch.zeros(2, 3, dtype=torch.long), torch.ones(2, 3, dtype=torch.long), torch.zeros(2, 4, 8)
    for bad in (dict(temperature=0.0), dict(temperature=-1.0), dict(top_p=0.0), dict(top_p=1.5), dict(top_k=-1), dict(num_return_sequences=0)):
        with pytest.raises(ValueError):
            sample(dec, ids, att, enc, **bad)
        with pytest.raises(ValueError):
            sample_from_logits(lambda i: None, ids, **bad)
    from prismer_amd.modules.roberta import RobertaForCausalLMModified
    gen = RobertaForCausalLMModified.generate
    with pytest.raises(ValueError, match='beam sampling'):
        gen(dec, input_ids=ids, encoder_hidden_states=enc, do_sample=True, num_beams=3)
    with pytest.raises(ValueError, match='do_sample'):
        gen(dec, input_ids=ids, encoder_hidden_states=enc, num_return_sequences=2)
    with pytest.raises(ValueError):
        gen(dec, input_ids=ids, encoder_hidden_states=enc, do_sample=True, top_p=0.0)


def test_sample_step_abi_without_gpu():
    """the ctypes mirror has the C layout of ph_sample_step_args, and out-of-range arguments are rejected on the host before any launch"""
    import ctypes as C
    import os
    import subprocess
    import tempfile
    from prismer_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "prismer_hip.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(ph_sample_step_args), ' \
           'offsetof(ph_sample_step_args, seed), offsetof(ph_sample_step_args, kept_mass_out)); return 0; }\n'
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, 't.c'), os.path.join(td, 't')
        open(src, 'w').write(prog)
        subprocess.check_call(['gcc', '-I', os.path.join(root, 'include'), src, '-o', exe])
        out = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    A = _lib.SampleStepArgs
    assert out == [C.sizeof(A), A.seed.offset, A.kept_mass_out.offset]

    def call(**kw):
        a = A()
        a.logits = a.ids = a.done = a.seq_logprob = 64
        a.ld, a.V, a.R, a.rows_per_logit, a.Tmax, a.cur, a.temperature, a.top_p = 1008, 1003, 2, 1, 4, 1, 1.0, 1.0
        for k, v in kw.items():
            setattr(a, k, v)
        rc = _lib.lib.ph_sample_step(C.byref(a), None)
        return rc, _lib.lib.ph_last_error()
    for kw, msg in [(dict(V=65536, ld=65536), b'vocabulary'), (dict(V=7), b'vocabulary'), (dict(ld=1004), b'aligned'), (dict(ld=1000), b'aligned'),
                    (dict(logits=72), b'aligned'), (dict(cur=4), b'position'), (dict(cur=-1), b'position'), (dict(R=0), b'row count'),
                    (dict(rows_per_logit=3), b'row count'), (dict(temperature=0.0), b'temperature'), (dict(top_p=0.0), b'top_p'),
                    (dict(top_k=-1), b'top_k'), (dict(ban_eos=1, eos_token_id=1003), b'eos_token_id'), (dict(ids=0), b'null pointer')]:
        rc, err = call(**kw)
        assert rc == -1 and msg in err, (kw, rc, err)
