"""CPU: the device-side guard of the optimizer state (Trainer(max_grad_norm=, skip_nonfinite=)) -- the ABI of ph_grad_sqnorm / ph_clip_finalize /
ph_adamw_ctl / PH_WS_GRAD_NORM without a device, the specification (guarded_update_spec / guarded_step_spec) against torch.nn.utils.clip_grad_norm_
+ torch.optim.AdamW + a manual skip, the constructor's refusals, and the fixture's own conditions."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_clip_symbols_resolve_and_ctl_layout_matches_header():
    from prismer_amd import _lib
    for name in ('ph_grad_sqnorm', 'ph_clip_finalize', 'ph_adamw_ctl'):
        assert name in _lib.EXPORTS and getattr(_lib.lib, name) is not None
    assert _lib.lib.ph_version() == 106                                    # (these additions did not move the revision; 106 is ph_gemm_route)
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "prismer_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d %d\n", sizeof(ph_clip_ctl), offsetof(ph_clip_ctl, coef), offsetof(ph_clip_ctl, apply), offsetof(ph_clip_ctl, norm),
         offsetof(ph_clip_ctl, finite), offsetof(ph_clip_ctl, sumsq), offsetof(ph_clip_ctl, applied), offsetof(ph_clip_ctl, skipped), PH_WS_GRAD_NORM,
         PH_SQNORM_RANGES_MAX, PH_SQNORM_BLOCKS_MAX);
  return 0;
}'''
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, 't.c'); exe = os.path.join(td, 't')
        open(src, 'w').write(prog)
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), src, '-o', exe])
        out = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    T = _lib.ClipCtl
    assert out == [C.sizeof(T), T.coef.offset, T.apply.offset, T.norm.offset, T.finite.offset, T.sumsq.offset, T.applied.offset, T.skipped.offset,
                   _lib.WS_GRAD_NORM, _lib.SQNORM_RANGES_MAX, _lib.SQNORM_BLOCKS_MAX]
    assert C.sizeof(T) == 40 and _lib.WS_GRAD_NORM == 5


def test_grad_norm_workspace_query_matches_its_documentation():
    """8 * sum_r min(ceil(n_r / 8192), max(1, floor(PH_SQNORM_BLOCKS_MAX * n_r / sum n))) bytes for 1 .. PH_SQNORM_RANGES_MAX range lengths: the
    grid of at most PH_SQNORM_BLOCKS_MAX (+ one per tiny range) blocks is shared out by length"""
    from prismer_amd import _lib
    q = lambda *d: _lib.lib.ph_query_workspace(_lib.WS_GRAD_NORM, (C.c_int64 * max(len(d), 1))(*d), len(d))
    blocks = lambda n, tot: min((n + 8191) // 8192, max(1, _lib.SQNORM_BLOCKS_MAX * n // tot))
    for d in [(1,), (3,), (8192,), (8193,), (1 << 23,), ((1 << 23) + 1,), (242_000_003,), (25_000_000, 217_000_000), (5, 7, 9), (1, 1, 1, 1), (1 << 33,), (1 << 33, 3, 1 << 20)]:
        assert q(*d) == 8 * sum(blocks(n, sum(d)) for n in d), d
    assert q(242_000_003) == 8 * 2048 and q(25_000_000, 217_000_000) == 8 * (211 + 1836) and q(1 << 30, 1, 1, 1) == 8 * (2047 + 3)
    assert q() == -1 and q(1, 1, 1, 1, 1) == -1 and q(0) == -1 and q(5, -1) == -1
    assert _lib.lib.ph_query_workspace(9, (C.c_int64 * 1)(1), 1) == -1


def test_clip_argument_validation_without_gpu():
    """every refusal comes back as PH_ERR_BAD_ARG before any launch (no device is touched: the pointers are small fake addresses)"""
    from prismer_amd import _lib
    L = _lib.lib
    err = lambda: L.ph_last_error()

    def sqnorm(ranges=(32,), n=(100,), k=None, ws=64, ws_bytes=1 << 20):
        k = len(ranges) if k is None else k
        return L.ph_grad_sqnorm((C.c_void_p * max(len(ranges), 1))(*ranges), (C.c_int64 * max(len(n), 1))(*n), k, ws, ws_bytes, None)
    assert sqnorm(k=0) == -1 and b'1..4 ranges' in err()
    assert sqnorm(ranges=(32,) * 5, n=(1,) * 5) == -1 and b'1..4 ranges' in err()
    assert sqnorm(ws=None) == -1
    assert sqnorm(ranges=(None,)) == -1 and b'range 0' in err()
    assert sqnorm(ranges=(36,)) == -1 and b'16-byte aligned' in err()
    assert sqnorm(n=(0,)) == -1 and b'range 0' in err()
    assert sqnorm(ranges=(32, 64), n=(10, -3)) == -1 and b'range 1' in err()
    assert sqnorm(n=(8193,), ws_bytes=8) == -1 and b'16 needed' in err()
    assert sqnorm(ws=68) == -1 and b'workspace' in err()
    assert L.ph_grad_sqnorm(None, None, 1, 64, 64, None) == -1

    def fin(partials=64, np_=4, pre=1.0, mx=1.0, skip=1, b1=0.9, b2=0.999, hyper=64, ctl=64):
        return L.ph_clip_finalize(partials, np_, pre, mx, skip, b1, b2, hyper, ctl, None)
    assert fin(partials=None) == -1 and fin(hyper=None) == -1 and fin(ctl=None) == -1
    assert fin(np_=0) == -1 and b'partials' in err()
    assert fin(np_=2048 + 4 + 1) == -1 and fin(np_=2048 + 4, mx=0.0) == -1 and b'max_norm' in err()
    assert fin(ctl=68) == -1 and b'8-byte aligned' in err()
    assert fin(mx=0.0) == -1 and b'max_norm' in err()
    assert fin(mx=float('nan')) == -1 and b'max_norm' in err()
    assert fin(pre=0.0) == -1 and fin(pre=float('nan')) == -1 and b'pre_scale' in err()
    assert fin(b1=1.0) == -1 and fin(b2=-0.1) == -1

    def adamw(p=64, g=64, m=64, v=64, pb=64, n=10, hyper=64, keep=None, ctl=64):
        return L.ph_adamw_ctl(p, g, m, v, pb, n, hyper, 0.9, 0.999, 1e-8, 0.05, 1.0, 1, keep, ctl, None)
    assert adamw(p=None) == -1 and adamw(hyper=None) == -1 and adamw(n=0) == -1 and b'bad args' in err()
    assert adamw(g=68) == -1 and b'misaligned' in err()
    assert adamw(ctl=68) == -1 and b'control block' in err()


# ---------------------------------------------------------------------------------------------------------------- the specification
def _toy(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g, dtype=torch.float64) for s in [(7, 5), (13,), (3, 4, 2), (1,)]]


@pytest.mark.parametrize('max_norm,skip', [(0.5, True), (1e9, True), (None, True), (0.5, False), (float('inf'), True)])
def test_specification_matches_torch_clip_adamw_and_manual_skip(max_norm, skip):
    """six iterations on a toy parameter set in fp64, iteration 3 poisoned (one NaN), iteration 5 with an inf: the specification against
    clip_grad_norm_ + torch.optim.AdamW + `if isfinite(total): step()`, equal to fp64 rounding.  skip=False: garbage propagates in both alike."""
    from prismer_amd.trainer import guarded_step_spec, guarded_update_spec
    lr0, wd, betas, eps = 1e-2, 0.05, (0.9, 0.999), 1e-8
    ref = [torch.nn.Parameter(t.clone()) for t in _toy()]
    opt = torch.optim.AdamW(ref, lr=lr0, weight_decay=wd, betas=betas, eps=eps)
    p = [t.clone() for t in _toy()]
    m, v = [torch.zeros_like(t) for t in p], [torch.zeros_like(t) for t in p]
    applied, n_skipped = 0, 0
    for i in range(6):
        lr = lr0 * (1.0 - 0.1 * i)                              # the schedule counts iterations, skipped ones included
        grads = [3.0 * t for t in _toy(100 + i)]
        if i == 2:
            grads[1][4] = float('nan')
        if i == 4:
            grads[2][1, 2, 0] = float('inf')
        for gp in opt.param_groups:
            gp['lr'] = lr
        for q, g in zip(ref, grads):
            q.grad = g.clone()
        pre = [g.clone() for g in grads]
        total_ref = torch.nn.utils.clip_grad_norm_(ref, max_norm if max_norm is not None else float('inf'))
        if (not skip) or bool(torch.isfinite(total_ref)):
            opt.step()
        total, coef, apply = guarded_update_spec(pre, max_norm, skip)
        total2, apply2, applied_new = guarded_step_spec(p, pre, m, v, applied, lr, betas, eps, wd, max_norm, skip)
        assert apply == apply2 == ((not skip) or i not in (2, 4))
        assert applied_new == applied + int(apply)
        applied, n_skipped = applied_new, n_skipped + int(not apply)
        assert torch.equal(total, total2) or (bool(torch.isnan(total)) and bool(torch.isnan(total2)))
        assert torch.equal(torch.isfinite(total), torch.isfinite(total_ref))
        if bool(torch.isfinite(total_ref)):
            assert abs(float(total) - float(total_ref)) <= 1e-14 * float(total_ref)
            if max_norm is not None:                            # torch scaled q.grad in place by ITS coefficient
                for q, g in zip(ref, pre):
                    assert torch.allclose(q.grad, g * coef, rtol=1e-14, atol=0.0)
        for q, t in zip(ref, p):
            assert torch.allclose(q.detach(), t, rtol=1e-12, atol=1e-15, equal_nan=True), (i, (q.detach() - t).abs().max())
    assert (applied, n_skipped) == ((4, 2) if skip else (6, 0))
    if skip:
        assert all(int(opt.state[q]['step']) == 4 for q in ref) and all(bool(torch.isfinite(t).all()) for t in p)
    else:
        assert not all(bool(torch.isfinite(t).all()) for t in p)        # torch's clip lets the garbage through, and so does the specification


def test_specification_coefficient_is_torchs():
    from prismer_amd.trainer import guarded_update_spec
    g = [torch.full((4,), 3.0, dtype=torch.float64)]                                       # norm 6
    total, coef, apply = guarded_update_spec(g, 3.0, True)
    assert float(total) == 6.0 and float(coef) == 3.0 / (6.0 + 1e-6) and apply
    assert float(guarded_update_spec(g, 12.0, True)[1]) == 1.0                            # clamp(max=1.0)
    assert float(guarded_update_spec(g, None, False)[1]) == 1.0
    big = [torch.tensor([1e30, 1.0], dtype=torch.float32)]                                 # the square overflows fp32: torch's fp32 norm is inf
    total, coef, apply = guarded_update_spec(big, 1.0, True)
    assert math.isinf(float(total)) and not apply and float(coef) == 0.0
    assert guarded_update_spec(big, 1.0, False)[2]


def test_constructor_refusals():
    from prismer_amd.trainer import Trainer
    for bad in (0.0, -1.0, float('nan')):
        with pytest.raises(ValueError, match='max_grad_norm'):
            Trainer(None, max_grad_norm=bad)
    for shard in (True, 'rs_ag'):
        with pytest.raises(ValueError, match='shard_optimizer'):
            Trainer(None, max_grad_norm=1.0, shard_optimizer=shard)
        with pytest.raises(ValueError, match='shard_optimizer'):
            Trainer(None, skip_nonfinite=True, shard_optimizer=shard)
    with pytest.raises(ValueError, match='micro_batches'):
        Trainer(None, skip_nonfinite=True, side_stream=True, micro_batches=2, use_graph=False)


def test_fixture_conditions():
    """what the minting script asserts, read back from the committed fixture: the clip is active with a factor of two to spare on every clean
    iteration, the poisoned iteration is the one skipped, in the fp32 loop and in the autocast yardstick alike"""
    from tests.golden import cases as GC
    from tests.golden.make_clip_golden import CLIP_ITERS, FIXTURE, MAX_NORM, POISON_ITER
    g = GC.load(FIXTURE)
    assert (int(g['iters']), int(g['poison_iter']), float(g['max_norm'])) == (CLIP_ITERS, POISON_ITER, MAX_NORM) == (3, 1, 50.0)
    for pre in ('', 'ac_'):
        totals, applied, losses = g[pre + 'totals'], g[pre + 'applied'], g[pre + 'losses']
        assert applied.tolist() == [1, 0, 1]
        for i in range(CLIP_ITERS):
            if i == POISON_ITER:
                assert not np.isfinite(totals[i]) and not np.isfinite(losses[i])
            else:
                assert totals[i] >= 2.0 * MAX_NORM and np.isfinite(losses[i])
    trainable = str(g['requires_grad']).split('\n')
    total0 = math.sqrt(sum(float(g['gnorm.' + n]) ** 2 for n in trainable))
    assert abs(total0 - float(g['totals'][0])) < 1e-4 * total0             # the stored per-tensor norms are those of the PRE-CLIP gradient
    for key in g:
        if key.startswith('bn.'):
            assert np.isfinite(np.asarray(g[key], dtype=np.float64)).all(), key     # the NaN never reached a BatchNorm buffer


def test_fixture_minting_conditions_hold_against_the_reference():
    """when the reference is mounted: the poisoned batch differs from the clean one in exactly one rgb value, and the script's constants are
    the ones the issue fixes"""
    from oracle import ref_harness as RH
    if not RH.available():
        pytest.skip('reference not mounted')
    from tests.golden import cases as GC
    from tests.golden.make_clip_golden import CLIP_CASE, MAX_NORM, poison
    x = GC.Case(CLIP_CASE).inputs()[0]
    y = poison(x)
    assert int(torch.isnan(y['rgb']).sum()) == 1 and int(torch.isnan(x['rgb']).sum()) == 0
    for k in x:
        if k != 'rgb':
            a, b = x[k], y[k]
            for kk in (a if isinstance(a, dict) else [None]):
                assert torch.equal(a[kk] if kk is not None else a, b[kk] if kk is not None else b)
    assert MAX_NORM == 50.0
