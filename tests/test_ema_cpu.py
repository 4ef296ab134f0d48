"""Trainer(ema_decay=, ema_warmup=) without a device: the specification (prismer_amd.trainer.ema_decay_at / ema_update_spec) against torch.lerp --
the call torch.optim.swa_utils.get_ema_multi_avg_fn and timm's ModelEma make -- and against float64, the decay schedule, the closed form of K folded
updates, and the validation of the constructor options.

Error bar (used by the GPU tests too): against e + w (p - e) evaluated in float64 every element satisfies |err| <= 2^-21 max(|e|, |p|) -- three
fp32 roundings (difference, product, sum; two with an fma), each <= 2^-24 of a quantity <= 2 max(|e|, |p|), for every w in [0, 1]."""
import pytest
import torch

from prismer_amd.trainer import Trainer, check_ema_options, ema_decay_at, ema_update_spec

BAR = 2.0 ** -21


def ema_err(got, e, p, w):
    """worst |got - (e + w32 (p - e))| / max(|e|, |p|) over the elements, the reference evaluated in float64 with the fp32 word of w"""
    w32 = torch.tensor(float(w), dtype=torch.float64).to(torch.float32).double()
    e, p = e.double().cpu(), p.double().cpu()
    scale = torch.maximum(e.abs(), p.abs()).clamp_min(1e-30)
    return float(((got.double().cpu() - (e + w32 * (p - e))).abs() / scale).max())


def _pair(n, seed):
    g = torch.Generator().manual_seed(seed)
    e = torch.randn(n, generator=g)
    return e, e + 1e-2 * torch.randn(n, generator=g)


@pytest.mark.parametrize('w', [1e-4, 1.0 - 0.999, 0.1, 0.3, 0.49])
def test_spec_is_torch_lerp_bit_for_bit_below_one_half(w):
    assert w < 0.5
    for n in (1, 15, 1000, 100003):                           # (torch's vector body and its scalar tail)
        e, p = _pair(n, n)
        w32 = float(torch.tensor(w, dtype=torch.float64).to(torch.float32))
        got = ema_update_spec(e, p, w)
        assert got.dtype == torch.float32
        assert torch.equal(got.view(torch.int32), torch.lerp(e, p, w32).view(torch.int32)), (w, n)
        assert ema_err(got, e, p, w) <= BAR


@pytest.mark.parametrize('w', [1e-4, 0.5, 0.9])
def test_spec_holds_the_bar_against_float64(w):
    e, p = _pair(100003, 7)
    err = ema_err(ema_update_spec(e, p, w), e, p, w)
    plain = ema_err(e + torch.tensor(w, dtype=torch.float64).to(torch.float32) * (p - e), e, p, w)      # the uncontracted fp32 expression
    print(f'w = {w}: worst error / max(|e|, |p|): spec {err:.3e}, uncontracted fp32 expression {plain:.3e}, bar {BAR:.3e}')
    assert err <= BAR and plain <= BAR


def test_decay_schedule():
    d = 0.9999
    assert ema_decay_at(0, d, True) == 0.1 and ema_decay_at(1, d, True) == 2.0 / 11.0 and ema_decay_at(10 ** 9, d, True) == d
    for u in (0, 1, 10 ** 9):
        assert ema_decay_at(u, d, False) == d and ema_decay_at(u, d) == d
    assert ema_decay_at(5, 0.3, True) == 0.3                    # a decay under the ramp is never raised
    ramp = [ema_decay_at(u, d, True) for u in range(200)]
    assert all(a < b for a, b in zip(ramp, ramp[1:])) and ramp[-1] < d


def test_folded_updates_follow_the_closed_form():
    K, d = 5, 0.9
    g = torch.Generator().manual_seed(3)
    e0 = torch.randn(4099, generator=g)
    ps = [e0 + 1e-2 * (j + 1) * torch.randn(4099, generator=g) for j in range(K)]
    e = e0.clone()
    for p in ps:
        e = ema_update_spec(e, p, 1.0 - d)
    w32 = torch.tensor(1.0 - d, dtype=torch.float64).to(torch.float32).double()
    d64 = 1.0 - w32                                             # the decay the fp32 word stands for
    want = d64 ** K * e0.double() + sum(w32 * d64 ** (K - 1 - j) * ps[j].double() for j in range(K))
    scale = torch.stack([e0.abs()] + [p.abs() for p in ps]).max(0).values.double()
    err = float(((e.double() - want).abs() / scale).max())
    print(f'K = {K} folded updates against the closed form: worst error / max {err:.3e}, bar {K * BAR:.3e}')
    assert err <= K * BAR


def test_option_validation_runs_before_anything_is_built():
    assert check_ema_options() == (None, False)
    assert check_ema_options(0.999, True) == (0.999, True) and check_ema_options(0.5) == (0.5, False)
    for bad in (0.0, 1.0, -0.1, 1.5, float('nan'), float('inf'), 1, 0, True, '0.9'):
        with pytest.raises(ValueError, match='ema_decay must be a float'):
            check_ema_options(bad)
        with pytest.raises(ValueError, match='ema_decay must be a float'):
            Trainer(None, ema_decay=bad)
    with pytest.raises(ValueError, match='ema_warmup=True needs ema_decay'):
        Trainer(None, ema_warmup=True)
    for kw in (dict(shard_optimizer=True), dict(shard_optimizer='rs_ag')):
        with pytest.raises(ValueError, match='ema_decay with shard_optimizer is not supported'):
            Trainer(None, ema_decay=0.99, **kw)
    with pytest.raises(ValueError, match='ema_decay with the eager micro_batches experiment'):
        Trainer(None, ema_decay=0.99, side_stream=True, micro_batches=2, use_graph=False)


def test_prologue_ships_the_weight_in_front_of_the_hyper_words():
    """the word of the update at schedule position u = it - 1 rides the one ph_store_words launch; without ema_decay the words are today's"""
    import types
    from prismer_amd import trainer as T
    stored = []
    orig = T.ops.store_words
    T.ops.store_words = lambda dst, vals, *a: stored.append((dst, tuple(vals)))
    try:
        for kw in (dict(), dict(ema_decay=0.999, ema_warmup=True, _step_words='words'), dict(ema_decay=0.75, ema_warmup=False, _step_words='words', guard=True)):
            fake = types.SimpleNamespace(accum=1, _micro=0, it=0, betas=(0.9, 0.999), lr_schedule=lambda it: 1e-3,
                                         enc=types.SimpleNamespace(experts=['depth']), hyper='hyper', table=None, **kw)
            Trainer._host_prologue(fake); Trainer._host_prologue(fake)
    finally:
        T.ops.store_words = orig
    assert stored[0:2] == [('hyper', (1e-3, 1.0 - 0.9, 1.0 - 0.999)), ('hyper', (1e-3, 1.0 - 0.9 ** 2, 1.0 - 0.999 ** 2))]
    assert stored[2:4] == [('words', (1.0 - 0.1, 1e-3, 1.0 - 0.9, 1.0 - 0.999)), ('words', (1.0 - 2.0 / 11.0, 1e-3, 1.0 - 0.9 ** 2, 1.0 - 0.999 ** 2))]
    assert stored[4:6] == [('words', (0.25, 1e-3)), ('words', (0.25, 1e-3))]
