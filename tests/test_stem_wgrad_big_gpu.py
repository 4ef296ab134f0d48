"""GPU: the stems' 3x3-conv weight gradients on the persistent k-balanced 256x128 LDS-DMA kernel -- B is the im2col VIEW of the NHWC
activation (k-row = output pixel, column = (tap, channel)), gathered by the DMA source address; padding taps and columns beyond 9 C / N
read the zero page.  Every case first asks ph_gemm_route and asserts the class, so that none can pass on the register-staged kernel.
Bars: those of test_kernels_gpu.py::test_implicit_gemm_conv_forward_stats_and_wgrad for the same quantity -- rel-Frobenius < 2e-4 against
the explicit-im2col route (same bf16 products, another summation order), < 3e-4 against fp32 F.conv2d autograd on the bf16-rounded
operands, columns >= 9 C exactly zero."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests.util import rel_fro

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
WS_BYTES = 64 << 20

# geometries (B, H = W, C, Cout, stride), 3x3 pad 1
ODD_S2 = (48, 15, 16, 264, 2)          # M, N, K = 264, 144, 3072: odd image with stride 2 (right / bottom border taps), ragged second row and column tile, 64 pixels per image
STRADDLE = (16, 14, 200, 264, 1)       # 264, 1800, 3136: 196 pixels per image (k-tiles straddle images), N no multiple of 128, C no multiple of 64
LONG = (32, 14, 24, 512, 1)            # 512, 216, 6272
TINY = (8, 16, 8, 16, 1)               # 16, 72, 2048: C = 8 (every chunk its own tap), M far below a tile
MID = (16, 14, 96, 192, 1)             # 192, 864, 3136
WIDE = (32, 14, 16, 264, 1)            # 264, 144, 6272

# name -> (geometries, workspace, extra zero columns, expected (units, cut) or None where only the relation is pinned)
GROUPS = {
    'odd_stride2': ([ODD_S2], True, 0),
    'straddle_images': ([STRADDLE], True, 0),
    'three_reductions': ([ODD_S2, STRADDLE, LONG], True, 0),
    'uncut_no_workspace': ([TINY, MID, WIDE], False, 0),
    'padded_columns': ([ODD_S2], True, 8),            # N = 9 C + 8: the last chunk of every row lies beyond 9 C
}


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator(device='cpu').manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(BF).cuda()


@pytest.fixture(scope='module')
def ops():
    from prismer_amd import ops as o
    return o


@pytest.fixture(scope='module')
def ws():
    return torch.empty(WS_BYTES // 4, dtype=torch.float32, device='cuda')


_CACHE = {}


def problem(ops, geo, pad):
    """operands and both references of one geometry, computed once and shared (never modified)"""
    key = geo + (pad,)
    if key not in _CACHE:
        B, H, Cc, Cout, stride = geo
        Ho = ops.conv_out_size(H, 3, stride)
        K, N = B * Ho * Ho, 9 * Cc + pad
        x = rnd(B, H, H, Cc, scale=0.7, seed=31)
        dy = rnd(K, Cout, scale=0.3, seed=33)
        col = ops.im2col(x, B, H, H, Cc, 3, stride, N)
        via_col = ops.gemm(dy, col, trans_a=True, trans_b=True, out_f32=True, M=Cout, N=N, K=K)
        w = torch.zeros(Cout, Cc, 3, 3, device='cuda', requires_grad=True)
        F.conv2d(x.float().permute(0, 3, 1, 2), w, stride=stride, padding=1).backward(dy.float().view(B, Ho, Ho, Cout).permute(0, 3, 1, 2))
        torch.cuda.synchronize()
        _CACHE[key] = dict(geo=geo, M=Cout, N=N, K=K, C=Cc, x=x, dy=dy, via_col=via_col,
                           dw=w.grad.permute(0, 2, 3, 1).reshape(Cout, 9 * Cc).contiguous(), conv=(B, H, H, Cc, 3, stride))
    return _CACHE[key]


def group(ops, name):
    geos, use_ws, pad = GROUPS[name]
    return [problem(ops, g, pad) for g in geos], use_ws


def group_args(probs, outs, ws, accumulate=0):
    from prismer_amd import _lib
    arr, keep = (_lib.GemmArgs * len(probs))(), []
    for g, p, out in zip(arr, probs, outs):
        g.A, g.B, g.C = p['dy'].data_ptr(), p['x'].data_ptr(), out.data_ptr()
        g.M, g.N, g.K = p['M'], p['N'], p['K']
        g.lda, g.ldb, g.ldc = p['dy'].stride(0), p['N'], out.stride(0)
        g.trans_a, g.trans_b, g.out_f32, g.accumulate, g.alpha = 1, 1, 1, accumulate, 1.0
        cg = _lib.ConvGather(*p['conv'])
        keep.append(cg)
        g.conv = C.pointer(cg)
        if ws is not None:
            g.workspace, g.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    return arr, keep


def route(arr):
    from prismer_amd import _lib
    info = _lib.GemmRouteInfo()
    _lib.check(_lib.lib.ph_gemm_route(arr, len(arr), 1, 0, C.byref(info)), 'ph_gemm_route')
    return info.part[0]


def assert_persistent(arr, probs, cut):
    """the group takes the persistent 256x128 kernel; cut: tiles are cut over K and folded inside the launch / the group runs whole"""
    from prismer_amd import _lib
    r = route(arr)
    tiles = sum(((p['M'] + 255) // 256) * ((p['N'] + 127) // 128) for p in probs)
    assert r.cls == _lib.GEMM_CLS_BIG_GROUPED and (r.bm, r.bn) == (256, 128), (r.cls, r.bm, r.bn)
    if cut:
        assert r.max_split > 1 and r.units > tiles and r.fold == _lib.GEMM_FOLD_IN_LAUNCH and r.ws_bytes > 0, (r.units, r.max_split, r.fold, r.ws_bytes)
    else:
        assert r.max_split == 1 and r.units == tiles and r.fold == _lib.GEMM_FOLD_NONE and r.ws_bytes == 0, (r.units, r.max_split, r.fold, r.ws_bytes)
    return r


def run(arr):
    from prismer_amd import _lib
    _lib.check(_lib.lib.ph_gemm_grouped_bf16(arr, len(arr), torch.cuda.current_stream().cuda_stream), 'ph_gemm_grouped_bf16')


def check_outputs(name, probs, outs, base=None):
    for i, (p, out) in enumerate(zip(probs, outs)):
        got = out if base is None else out - base[i]
        e_col, e_ref = rel_fro(got, p['via_col']), rel_fro(got[:, :9 * p['C']], p['dw'])
        print(name, p['geo'], 'vs im2col route', e_col, 'vs conv2d autograd', e_ref)
        assert e_col < 2e-4, (p['geo'], e_col)
        assert e_ref < 3e-4, (p['geo'], e_ref)
        if base is None:
            assert float(got[:, 9 * p['C']:].abs().sum()) == 0.0


@pytest.mark.parametrize('name', list(GROUPS))
def test_gathered_wgrad_matches_im2col_and_autograd(ops, ws, name):
    """one launch of the persistent kernel, no fold pass; the same launch twice is bit-identical (the in-launch fold is order-fixed)"""
    from prismer_amd import _lib
    probs, use_ws = group(ops, name)
    outs = [torch.full((p['M'], p['N']), float('nan'), device='cuda') for p in probs]
    arr, keep = group_args(probs, outs, ws if use_ws else None)
    r = assert_persistent(arr, probs, cut=use_ws)
    print(name, 'units', r.units, 'max_split', r.max_split, 'ws_bytes', r.ws_bytes)
    if name == 'odd_stride2':
        assert (r.units, r.max_split) == (8, 2), (r.units, r.max_split)
    if name == 'straddle_images':
        assert r.max_split == 2, r.max_split
    if name == 'three_reductions':
        assert r.units == 84 and r.max_split <= 4, (r.units, r.max_split)
    if name == 'uncut_no_workspace':
        assert r.units == 12, r.units
    cnt = (C.c_int64 * 16)()
    _lib.lib.ph_gemm_dispatch_counts(cnt, 16, 1)
    run(arr)
    torch.cuda.synchronize()
    _lib.lib.ph_gemm_dispatch_counts(cnt, 16, 0)
    assert cnt[4] == 1 and cnt[6] == 0 and sum(cnt[:7]) == 1, list(cnt)[:7]      # one big_grouped launch, no splitk_reduce
    check_outputs(name, probs, outs)
    first = [o.clone() for o in outs]
    for o in outs:
        o.fill_(float('nan'))
    run(arr)
    torch.cuda.synchronize()
    for a, b in zip(first, outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize('name', ['three_reductions', 'uncut_no_workspace'])
def test_accumulate_into_nonzero_output(ops, ws, name):
    probs, use_ws = group(ops, name)
    base = [torch.randn(p['M'], p['N'], device='cuda', generator=torch.Generator(device='cuda').manual_seed(900 + i)) for i, p in enumerate(probs)]
    outs = [b.clone() for b in base]
    arr, keep = group_args(probs, outs, ws if use_ws else None, accumulate=1)
    assert_persistent(arr, probs, cut=use_ws)
    run(arr)
    torch.cuda.synchronize()
    # (out - base) carries the rounding of base + dW in fp32: |base| ~ 1 against |dW| ~ several, far inside the bars)
    check_outputs(name + '+acc', probs, outs, base)


def test_graph_replay_bitwise(ops, ws):
    """captured once, replayed three times: equal results every time (the arrival counters are re-zeroed by a kernel inside the graph)"""
    probs, _ = group(ops, 'three_reductions')
    outs = [torch.empty(p['M'], p['N'], device='cuda') for p in probs]
    arr, keep = group_args(probs, outs, ws)
    assert_persistent(arr, probs, cut=True)
    run(arr)
    torch.cuda.synchronize()
    eager = [o.clone() for o in outs]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            run(arr)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(3):
        for o in outs:
            o.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, outs):
            assert torch.equal(a, b)
    check_outputs('replay', probs, outs)
