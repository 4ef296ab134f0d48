"""GPU: the kernels of the guarded update -- ph_grad_sqnorm + ph_clip_finalize against the fp64 norm of the same fp32 buffer (yardstick: the
error of torch's own fp32 vector_norm, twice that allowed), replay determinism, the non-finite cases, the bias-correction words, and ph_adamw_ctl
against ph_adamw_keep (bitwise with coef = 1 / apply = 1; nothing but the gradient clean-up with apply = 0)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
F32 = torch.float32
BASE_RANGES = (24_963_075, 217_084_929)          # about Prismer-BASE's two trainable ranges under freeze_vision (n_train ~ 242 M), both with n & 3 != 0


def _measure(ranges, pre_scale=1.0, max_norm=None, skip=True, ctl=None, hyper=None, ws=None):
    from prismer_amd import ops
    ctl = ctl or ops.ClipCtl(ranges[0].device)
    hyper = hyper if hyper is not None else torch.zeros(3, dtype=F32, device='cuda')
    ws = ops.grad_sqnorm(ranges, ws)
    ops.clip_finalize(ws, ctl, hyper, pre_scale, max_norm, skip, 0.9, 0.999)
    return ctl, hyper, ws


def _torch_total(ranges):
    """clip_grad_norm_'s total norm in fp32: the norm of the per-tensor norms"""
    return torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(t, 2) for t in ranges]), 2)


@pytest.mark.parametrize('sizes', [(1,), (3,), (5,), (1023,), (4099,), (8193,), (100_003,), ((1 << 20) + 1,), (7, 8192 * 3 + 2, 13), (1 << 23, 5, 77, 1 << 21), BASE_RANGES])
def test_norm_against_fp64_with_torch_fp32_as_yardstick(sizes):
    g = torch.Generator(device='cuda').manual_seed(sum(sizes))
    ranges = [torch.randn(n, generator=g, device='cuda', dtype=F32) * (0.5 + r) for r, n in enumerate(sizes)]
    want = float(torch.sqrt(sum(t.double().pow(2).sum() for t in ranges)))
    ctl, _, ws = _measure(ranges)
    got, yard = float(ctl.norm.item()), float(_torch_total(ranges).item())
    e_got, e_yard = abs(got - want) / want, abs(yard - want) / want
    print(f'sizes {sizes}: blocks {ws.numel()}  fp64 norm {want!r}  kernel {got!r} (rel. error {e_got:.3e})  torch fp32 vector_norm {yard!r} (rel. error {e_yard:.3e})  '
          f'fp64 sumsq word rel. error {abs(float(ctl.sumsq.item()) - want * want) / (want * want):.3e}')
    assert e_got <= 2.0 * e_yard, (sizes, e_got, e_yard)
    assert int(ctl.apply.item()) == 1 and int(ctl.finite.item()) == 1 and float(ctl.coef.item()) == 1.0
    assert (int(ctl.applied.item()), int(ctl.skipped.item())) == (1, 0)


def test_pre_scale_and_clip_coefficient_are_torchs():
    ranges = [torch.full((4099,), 2.0, device='cuda', dtype=F32), torch.full((5,), -1.0, device='cuda', dtype=F32)]
    total = (4099 * 4.0 + 5.0) ** 0.5
    for pre, mx in [(1.0, 10.0), (0.125, 10.0), (0.5, 1e9), (1.0, float('inf')), (1.0, None)]:
        ctl, _, _ = _measure(ranges, pre_scale=pre, max_norm=mx)
        n32 = np.float32(total * pre)
        assert np.float32(ctl.norm.item()) == n32
        want = np.float32(1.0) if mx is None else min(np.float32(1.0), np.float32(mx) / (n32 + np.float32(1e-6)))
        assert np.float32(ctl.coef.item()) == want, (pre, mx, ctl.coef.item(), want)


def test_two_launches_on_one_buffer_give_identical_bits():
    from prismer_amd import ops
    g = torch.Generator(device='cuda').manual_seed(5)
    ranges = [torch.randn(n, generator=g, device='cuda', dtype=F32) for n in (3_000_001, 12_345_679)]
    ws1, ws2 = ops.grad_norm_workspace([t.numel() for t in ranges], 'cuda'), ops.grad_norm_workspace([t.numel() for t in ranges], 'cuda')
    ws1.fill_(float('nan')); ws2.fill_(123.0)                              # the workspace needs no zeroing: every partial read was written by the launch
    c1, _, _ = _measure(ranges, ws=ws1)
    c2, _, _ = _measure(ranges, ws=ws2)
    assert torch.equal(ws1.view(torch.int64), ws2.view(torch.int64))
    assert torch.equal(c1.words[:3], c2.words[:3]) and bool(torch.isfinite(ws1).all())


@pytest.mark.parametrize('bad', [float('nan'), float('inf'), -float('inf'), 1e30])
@pytest.mark.parametrize('n,where', [(5, 4), (8193 * 4 + 3, 8193 * 4 + 2), (3_000_001, 1_234_567)])
def test_non_finite_sum_of_squares_is_not_applied(bad, n, where):
    """a single NaN, a single inf, and a value whose SQUARE overflows fp32 (1e30: torch's fp32 norm is inf): apply == 0 under skip_nonfinite, and
    the skipped counter moves instead of the applied one; without skip_nonfinite the update is applied (torch's clip: garbage propagates)"""
    from prismer_amd import ops
    x = torch.ones(n, device='cuda', dtype=F32)
    x[where] = bad
    ctl = ops.ClipCtl('cuda')
    ctl.applied.fill_(7)
    hyper = torch.zeros(3, dtype=F32, device='cuda')
    _measure([x], max_norm=1.0, skip=True, ctl=ctl, hyper=hyper)
    assert int(ctl.apply.item()) == 0 and int(ctl.finite.item()) == 0
    assert (int(ctl.applied.item()), int(ctl.skipped.item())) == (7, 1)
    assert np.float32(hyper[1].item()) == np.float32(1 - 0.9 ** 7)         # t did not move
    assert not np.isfinite(np.float32(_torch_total([x]).item()))           # torch's fp32 norm of the same buffer is not finite either
    _measure([x], max_norm=1.0, skip=False, ctl=ctl, hyper=hyper)
    assert int(ctl.apply.item()) == 1 and int(ctl.finite.item()) == 0 and (int(ctl.applied.item()), int(ctl.skipped.item())) == (8, 1)
    c = float(ctl.coef.item())
    assert np.isnan(c) if bad != bad else c == 0.0                        # 1 / (nan + eps) stays NaN through the clamp; 1 / (inf + eps) = 0


def test_bias_corrections_follow_the_applied_count():
    """hyper[1], hyper[2] within one fp32 ulp of 1 - b ** t for t = 1 .. 50 (t = the count of applied updates, advanced by the kernel); hyper[0],
    the learning rate, is the host's and is left alone"""
    from prismer_amd import ops
    x = torch.ones(1000, device='cuda', dtype=F32)
    ctl, hyper = ops.ClipCtl('cuda'), torch.tensor([0.125, 0.0, 0.0], dtype=F32, device='cuda')
    ws = None
    rows = []
    for t in range(1, 51):
        _, _, ws = _measure([x], ctl=ctl, hyper=hyper, ws=ws)
        rows.append(hyper.cpu().numpy().copy())
    assert int(ctl.applied.item()) == 50
    worst = 0.0
    for t, h in enumerate(rows, 1):
        assert h[0] == np.float32(0.125)
        for got, b in ((h[1], 0.9), (h[2], 0.999)):
            want = 1.0 - b ** t
            ulp = float(np.spacing(np.float32(want)))
            worst = max(worst, abs(float(got) - want) / ulp)
            assert abs(float(got) - want) <= ulp, (t, b, got, want)
    print('bias corrections t = 1..50: worst error in fp32 ulps', worst)


def _adamw_state(n, seed=0):
    g = torch.Generator(device='cuda').manual_seed(seed)
    p, gr = torch.randn(n, generator=g, device='cuda', dtype=F32), torch.randn(n, generator=g, device='cuda', dtype=F32) * 3.0
    m, v = torch.randn(n, generator=g, device='cuda', dtype=F32) * 0.1, torch.rand(n, generator=g, device='cuda', dtype=F32)
    pb = torch.zeros(n, device='cuda', dtype=torch.bfloat16)
    nchunks = (n + 1023) // 1024
    keep = torch.zeros((nchunks + 31) // 32, dtype=torch.int32, device='cuda')
    bits = torch.randint(0, 2, (keep.numel() * 32,), generator=g, device='cuda')
    keep.copy_((bits.view(-1, 32) << torch.arange(32, device='cuda')).sum(1).to(torch.int32))
    return p, gr, m, v, pb, keep


def _ctl(coef, apply):
    from prismer_amd import ops
    c = ops.ClipCtl('cuda')
    c.coef.fill_(coef); c.apply.fill_(apply)
    return c


@pytest.mark.parametrize('n', [3, 1024 * 37 + 3, 1 << 22, (1 << 22) + 1025])
@pytest.mark.parametrize('zero_grad,use_keep', [(True, True), (True, False), (False, False)])
def test_adamw_ctl_against_adamw_keep(n, zero_grad, use_keep):
    from prismer_amd import ops
    hyper = torch.tensor([1e-3, 1 - 0.9 ** 3, 1 - 0.999 ** 3], dtype=F32, device='cuda')
    ref = _adamw_state(n)
    before = [t.clone() for t in ref]
    ops.adamw(*ref[:5], n, hyper, grad_scale=0.5, zero_grad=zero_grad, keep=ref[5] if use_keep else None)
    # coef = 1, apply = 1: ph_adamw_keep bit for bit -- tail elements (n & 3) and keep bitmap included
    a = _adamw_state(n)
    ops.adamw_ctl(*a[:5], n, hyper, _ctl(1.0, 1), grad_scale=0.5, zero_grad=zero_grad, keep=a[5] if use_keep else None)
    for x, y in zip(a[:5], ref[:5]):
        assert torch.equal(x.view(torch.int32 if x.dtype == F32 else torch.int16), y.view(torch.int32 if y.dtype == F32 else torch.int16))
    # ctl == NULL through the new entry point: the same kernel as ph_adamw_keep
    z = _adamw_state(n)
    ops.adamw_ctl(*z[:5], n, hyper, None, grad_scale=0.5, zero_grad=zero_grad, keep=z[5] if use_keep else None)
    for x, y in zip(z[:5], ref[:5]):
        assert torch.equal(x, y)
    # coef = 0.25: the gradient scale is grad_scale * coef
    b, r2 = _adamw_state(n), _adamw_state(n)
    ops.adamw_ctl(*b[:5], n, hyper, _ctl(0.25, 1), grad_scale=0.5, zero_grad=zero_grad, keep=b[5] if use_keep else None)
    ops.adamw(*r2[:5], n, hyper, grad_scale=0.125, zero_grad=zero_grad, keep=r2[5] if use_keep else None)
    for x, y in zip(b[:5], r2[:5]):
        assert torch.equal(x, y)
    # apply = 0: p, m, v and the shadow keep their bits; the gradients are what the applied launch left
    s = _adamw_state(n)
    s[4].fill_(1.5)
    ops.adamw_ctl(*s[:5], n, hyper, _ctl(float('nan'), 0), grad_scale=0.5, zero_grad=zero_grad, keep=s[5] if use_keep else None)
    for k in (0, 2, 3):
        assert torch.equal(s[k].view(torch.int32), before[k].view(torch.int32)), k
    assert bool((s[4] == 1.5).all())
    assert torch.equal(s[1].view(torch.int32), ref[1].view(torch.int32))
    if zero_grad and not use_keep:
        assert not bool(ref[1].any())
    if zero_grad and use_keep and n >= 1 << 22:
        assert bool(ref[1].any()) and int((ref[1] == 0).sum()) > n // 8          # kept chunks hold their gradients, the others are zeroed
    if not zero_grad:
        assert torch.equal(ref[1], before[1])
