"""ph_adamw_ema (AdamW with the moving average of the weights updated in the same launch) and ph_swap_f32 on the device: the AdamW side bit for bit
against ph_adamw_keep / ph_adamw_ctl on cloned inputs, the average against prismer_amd.trainer.ema_update_spec applied to the kernel's own new
masters under the derived bar of tests/test_ema_cpu.py (2^-21 max(|e|, |p|) against float64), the skipped update, the weight read from device
memory at every launch, and the exchange kernel with its host-side argument checks."""
import ctypes

import pytest
import torch

from tests.test_ema_cpu import BAR, ema_err

pytestmark = pytest.mark.gpu
F32 = torch.float32

# n: a single element | tail only | one whole vector, no tail | one chunk plus a tail | three chunks plus a tail | many blocks | past the 2048-block
# cap with an uneven last chunk
SIZES = [1, 3, 4, 1025, 3 * 1024 + 2, 256 * 1024 + 7, 2_200_003]
HYPER = (1e-3, 1 - 0.9 ** 3, 1 - 0.999 ** 3)


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


_STATE = {}


def _state(n):
    """(p, g, m, v, shadow, keep bitmap with alternating bits, ema) for n parameters: generated once per n, handed out as clones"""
    if n not in _STATE:
        g = torch.Generator(device='cuda').manual_seed(n)
        p, gr = torch.randn(n, generator=g, device='cuda', dtype=F32), torch.randn(n, generator=g, device='cuda', dtype=F32) * 3.0
        m, v = torch.randn(n, generator=g, device='cuda', dtype=F32) * 0.1, torch.rand(n, generator=g, device='cuda', dtype=F32)
        pb = torch.full((n,), 1.5, device='cuda', dtype=torch.bfloat16)
        keep = torch.full((((n + 1023) // 1024 + 31) // 32,), -1431655766, dtype=torch.int32, device='cuda')          # 0xAAAAAAAA: odd chunks kept
        ema = p + 0.05 * torch.randn(n, generator=g, device='cuda', dtype=F32)
        _STATE[n] = (p, gr, m, v, pb, keep, ema)
    return [t.clone() for t in _STATE[n]]


def _ctl(coef, apply):
    from prismer_amd import ops
    c = ops.ClipCtl('cuda')
    c.coef.fill_(coef); c.apply.fill_(apply)
    return c


def _check_ema(got, e0, p_new, w, what):
    from prismer_amd.trainer import ema_update_spec
    err_spec = ema_err(ema_update_spec(e0, p_new, w), e0, p_new, w)
    err = ema_err(got, e0, p_new, w)
    print(f'{what}: ema worst error / max(|e|, |p|) {err:.3e} (the fp32 spec itself {err_spec:.3e}; bar {BAR:.3e})')
    assert err <= BAR, (what, err)


@pytest.mark.parametrize('shadow', [True, False])
@pytest.mark.parametrize('n', SIZES)
def test_adamw_ema_is_adamw_plus_the_average(n, shadow):
    from prismer_amd import ops
    hyper = torch.tensor(HYPER, dtype=F32, device='cuda')
    w = 1.0 - 0.999
    ema_w = torch.tensor([w], dtype=F32, device='cuda')
    for zero_grad in (False, True):
        for use_keep in (False, True):
            ref, a = _state(n), _state(n)
            e0 = a[6].clone()
            ops.adamw(*ref[:4], ref[4] if shadow else None, n, hyper, grad_scale=0.5, zero_grad=zero_grad, keep=ref[5] if use_keep else None)
            ops.adamw_ema(*a[:4], a[4] if shadow else None, n, hyper, a[6], ema_w, grad_scale=0.5, zero_grad=zero_grad, keep=a[5] if use_keep else None)
            for name, x, y in zip(('p', 'g', 'm', 'v', 'shadow'), a[:5], ref[:5]):
                assert torch.equal(_bits(x), _bits(y)), (name, n, shadow, zero_grad, use_keep)
            if not shadow:
                assert bool((a[4] == 1.5).all())
            assert not torch.equal(a[0], _STATE[n][0]) and not torch.equal(a[6], e0)
            _check_ema(a[6], e0, a[0], w, f'n={n} shadow={shadow} zero_grad={zero_grad} keep={use_keep}')


@pytest.mark.parametrize('n', SIZES)
def test_adamw_ema_under_a_control_block(n):
    from prismer_amd import ops
    hyper = torch.tensor(HYPER, dtype=F32, device='cuda')
    w = 0.1
    ema_w = torch.tensor([w], dtype=F32, device='cuda')
    for zero_grad, use_keep in ((True, True), (True, False), (False, False)):
        kw = dict(grad_scale=0.5, zero_grad=zero_grad)
        # apply = 1, coef = 0.5: ph_adamw_ctl bit for bit, the average moves by the spec
        ref, a = _state(n), _state(n)
        e0 = a[6].clone()
        ops.adamw_ctl(*ref[:5], n, hyper, _ctl(0.5, 1), keep=ref[5] if use_keep else None, **kw)
        ops.adamw_ema(*a[:5], n, hyper, a[6], ema_w, _ctl(0.5, 1), keep=a[5] if use_keep else None, **kw)
        for name, x, y in zip(('p', 'g', 'm', 'v', 'shadow'), a[:5], ref[:5]):
            assert torch.equal(_bits(x), _bits(y)), (name, n, zero_grad, use_keep)
        _check_ema(a[6], e0, a[0], w, f'ctl apply=1 n={n} zero_grad={zero_grad} keep={use_keep}')
        # apply = 0: ema, p, m, v and the shadow keep their bits; the gradients are cleaned as ph_adamw_ctl cleans them
        ref, s = _state(n), _state(n)
        ops.adamw_ctl(*ref[:5], n, hyper, _ctl(float('nan'), 0), keep=ref[5] if use_keep else None, **kw)
        ops.adamw_ema(*s[:5], n, hyper, s[6], ema_w, _ctl(float('nan'), 0), keep=s[5] if use_keep else None, **kw)
        for k, name in ((0, 'p'), (2, 'm'), (3, 'v'), (4, 'shadow'), (6, 'ema')):
            assert torch.equal(_bits(s[k]), _bits(_STATE[n][k])), (name, n, zero_grad, use_keep)
        assert torch.equal(_bits(s[1]), _bits(ref[1]))
        if zero_grad and not use_keep:
            assert not bool(s[1].any())
        if not zero_grad:
            assert torch.equal(s[1], _STATE[n][1])


def test_the_weight_is_read_from_device_memory_at_every_launch():
    """two launches, two values written into the SAME device word (what a replayed graph does): two different, correct results"""
    from prismer_amd import ops
    n = 3 * 1024 + 2
    hyper = torch.tensor(HYPER, dtype=F32, device='cuda')
    ema_w = torch.zeros(1, dtype=F32, device='cuda')
    outs = []
    for w in (0.9, 1e-4):
        a = _state(n)
        e0 = a[6].clone()
        ops.store_words(ema_w, (w,))
        ops.adamw_ema(*a[:5], n, hyper, a[6], ema_w)
        _check_ema(a[6], e0, a[0], w, f'w={w} through the device word')
        outs.append(a[6])
    assert not torch.equal(outs[0], outs[1])


@pytest.mark.parametrize('n', [1, 5, 1024, 1_000_003])
def test_swap_is_an_exact_exchange(n):
    from prismer_amd import ops
    g = torch.Generator(device='cuda').manual_seed(n)
    a0 = torch.randn(n + 4, generator=g, device='cuda', dtype=F32)
    b0 = torch.randn(n + 4, generator=g, device='cuda', dtype=F32)
    a0[n // 2] = float('nan'); b0[0] = float('inf')            # (bit patterns, not values, are exchanged)
    a, b = a0.clone(), b0.clone()
    ops.swap_f32(a[:n], b[:n])
    assert torch.equal(_bits(a[:n]), _bits(b0[:n])) and torch.equal(_bits(b[:n]), _bits(a0[:n]))
    assert torch.equal(_bits(a[n:]), _bits(a0[n:])) and torch.equal(_bits(b[n:]), _bits(b0[n:]))          # nothing past the ranges
    ops.swap_f32(a[:n], b[:n])
    assert torch.equal(_bits(a), _bits(a0)) and torch.equal(_bits(b), _bits(b0))


def test_bad_arguments_are_refused_on_the_host():
    from prismer_amd import _lib
    lib = _lib.lib
    buf = torch.arange(64, device='cuda', dtype=F32)
    keep = buf.clone()
    base = buf.data_ptr()
    assert lib.ph_swap_f32(base, base + 16, 8, None) == _lib.PH_OK - 1 and b'overlap' in lib.ph_last_error()          # PH_ERR_BAD_ARG
    assert lib.ph_swap_f32(base + 16, base, 8, None) == -1 and b'overlap' in lib.ph_last_error()
    assert lib.ph_swap_f32(base, base, 8, None) == -1
    assert lib.ph_swap_f32(base + 4, base + 128, 8, None) == -1 and b'aligned' in lib.ph_last_error()
    assert lib.ph_swap_f32(base, base + 132, 8, None) == -1
    assert lib.ph_swap_f32(None, base, 8, None) == -1 and lib.ph_swap_f32(base, base + 128, 0, None) == -1
    args = [base] * 4 + [None, ctypes.c_int64(8), base, 0.9, 0.999, 1e-8, 0.05, 1.0, 0, None, None]
    assert lib.ph_adamw_ema(*args, None, base, None) == -1 and b'ph_adamw_ema' in lib.ph_last_error()                # no average
    assert lib.ph_adamw_ema(*args, base, None, None) == -1                                                          # no weight
    assert lib.ph_adamw_ema(*args, base + 4, base, None) == -1 and b'misaligned' in lib.ph_last_error()
    torch.cuda.synchronize()
    assert torch.equal(buf, keep)                               # nothing was launched
    assert lib.ph_swap_f32(base, base + 32, 8, None) == _lib.PH_OK                    # adjacent ranges are disjoint
    torch.cuda.synchronize()
    assert torch.equal(buf[:8], keep[8:16]) and torch.equal(buf[8:16], keep[:8]) and torch.equal(buf[16:], keep[16:])
