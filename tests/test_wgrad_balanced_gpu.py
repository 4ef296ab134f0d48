"""GPU: the k-balanced persistent weight-gradient kernel (units = (problem, tile, k-range), partial tiles folded inside the launch by the
unit that arrives last) and the bias-gradient column sums fused into the weight-gradient GEMMs (ph_gemm_args.a_colsum), against fp32
PyTorch products.  Bars are those of test_kernels_gpu.py::test_wgrad_queue_grouped_launch: rel-Frobenius < 3e-4 for dW (fp32 output of
a bf16 contraction), < 1e-4 for the column sums (exact bf16 values summed in fp32)."""
import ctypes as C

import pytest
import torch

from tests.util import rel_fro

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
ALPHA = 0.75
WS_BYTES = 64 << 20

# [K][M] x [K][N] groups that the plan cuts over K: ragged against the 256x128 tile (2 x 2 tiles per problem), 32 / 65 / 130 k-tiles -> the
# problems differ in split count, the shortest stays whole; and a single problem of 2 tiles
GROUPS = {
    'three_ragged': [(264, 136, 2048), (264, 136, 4160), (264, 136, 8320)],
    'one_two_tiles': [(512, 128, 8320)],
}


@pytest.fixture(scope='module')
def ops():
    from prismer_amd import ops as o
    return o


def rnd(*shape, scale=1.0, seed=0, dtype=BF):
    g = torch.Generator(device='cpu').manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(dtype).cuda()


_CACHE = {}


def problems(name):
    """operands and fp32 references of a group, computed once and shared (never modified)"""
    if name not in _CACHE:
        out = []
        for i, (M, N, K) in enumerate(GROUPS[name]):
            dy, x = rnd(K, M, scale=0.3, seed=300 + i), rnd(K, N, scale=0.3, seed=400 + i)
            gw0 = torch.randn(M, N, device='cuda', generator=torch.Generator(device='cuda').manual_seed(500 + i))
            gb0 = torch.randn(M, device='cuda', generator=torch.Generator(device='cuda').manual_seed(600 + i))
            out.append(dict(M=M, N=N, K=K, dy=dy, x=x, gw0=gw0, gb0=gb0, ref=dy.float().t() @ x.float(), cref=dy.float().sum(0)))
        _CACHE[name] = out
    return _CACHE[name]


def group_args(probs, gws, gbs, ws, accumulate):
    from prismer_amd import _lib
    arr = (_lib.GemmArgs * len(probs))()
    for g, p, gw, gb in zip(arr, probs, gws, gbs):
        g.A, g.B, g.C = p['dy'].data_ptr(), p['x'].data_ptr(), gw.data_ptr()
        g.M, g.N, g.K = p['M'], p['N'], p['K']
        g.lda, g.ldb, g.ldc = p['dy'].stride(0), p['x'].stride(0), gw.stride(0)
        g.trans_a, g.trans_b, g.out_f32, g.accumulate, g.alpha = 1, 1, 1, int(accumulate), ALPHA
        g.a_colsum = gb.data_ptr() if gb is not None else None
        if ws is not None:
            g.workspace, g.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    return arr


def plan_of(arr):
    """(units, max_split) of the group on the persistent 256x128 weight-gradient kernel, (0, 0) when it does not take that kernel"""
    from prismer_amd import _lib
    info = _lib.GemmRouteInfo()
    _lib.check(_lib.lib.ph_gemm_route(arr, len(arr), 1, 0, C.byref(info)), 'ph_gemm_route')
    part = info.part[0]
    return (part.units, part.max_split) if part.cls == _lib.GEMM_CLS_BIG_GROUPED else (0, 0)


def run(arr):
    from prismer_amd import _lib
    _lib.check(_lib.lib.ph_gemm_grouped_bf16(arr, len(arr), torch.cuda.current_stream().cuda_stream), 'ph_gemm_grouped_bf16')


@pytest.fixture(scope='module')
def ws():
    return torch.empty(WS_BYTES // 4, dtype=torch.float32, device='cuda')


@pytest.mark.parametrize('with_colsum', [False, True])
@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('name', list(GROUPS))
def test_split_path(ops, ws, name, accumulate, with_colsum):
    """the persistent kernel with tiles cut over K: overwrite and accumulate onto a random dW, alpha != 1, with and without fused column sums"""
    probs = problems(name)
    gws = [p['gw0'].clone() for p in probs]
    gbs = [p['gb0'].clone() if with_colsum else None for p in probs]
    arr = group_args(probs, gws, gbs, ws, accumulate)
    units, max_split = plan_of(arr)
    tiles = sum(((p['M'] + 255) // 256) * ((p['N'] + 127) // 128) for p in probs)
    assert max_split > 1 and units > tiles, (units, max_split)
    from prismer_amd import _lib
    cnt = (C.c_int64 * 16)()
    _lib.lib.ph_gemm_dispatch_counts(cnt, 16, 1)
    run(arr)
    torch.cuda.synchronize()
    _lib.lib.ph_gemm_dispatch_counts(cnt, 16, 0)
    assert cnt[4] == 1 and sum(cnt[:7]) == 1, list(cnt)[:7]           # one launch of the persistent 256x128 class, no fold pass
    for p, gw, gb in zip(probs, gws, gbs):
        got = gw - p['gw0'] if accumulate else gw
        e = rel_fro(got, ALPHA * p['ref'])
        print(name, accumulate, with_colsum, p['K'], 'dW', e)
        assert e < 3e-4, (p['K'], e)
        if gb is not None:
            ec = rel_fro(gb - p['gb0'], p['cref'])
            print(name, p['K'], 'colsum', ec)
            assert ec < 1e-4, (p['K'], ec)


def test_plan_without_workspace_is_unsplit(ops):
    """no workspace: the group runs whole, exactly as before"""
    probs = problems('three_ragged')
    gws = [p['gw0'].clone() for p in probs]
    arr = group_args(probs, gws, [None] * len(probs), None, False)
    units, max_split = plan_of(arr)
    assert max_split == 1 and units == 12, (units, max_split)
    run(arr)
    torch.cuda.synchronize()
    for p, gw in zip(probs, gws):
        assert rel_fro(gw, ALPHA * p['ref']) < 3e-4


@pytest.mark.parametrize('name', list(GROUPS))
def test_repeat_and_replay_bitwise(ops, ws, name):
    """the same split call twice back to back, then captured and replayed three times: dW bit-identical every time (slabs folded in split
    order whoever arrives last; counters re-zeroed by the memset ahead of every launch), the column sums grow by one sum per run"""
    probs = problems(name)
    gws = [torch.empty_like(p['gw0']) for p in probs]
    gbs = [p['gb0'].clone() for p in probs]
    arr = group_args(probs, gws, gbs, ws, False)
    assert plan_of(arr)[1] > 1
    runs = 0
    seen = []

    def check():
        torch.cuda.synchronize()
        seen.append([gw.clone() for gw in gws])
        for gw in gws:
            gw.fill_(float('nan'))
        for p, gb in zip(probs, gbs):
            ec = rel_fro((gb - p['gb0']) / runs, p['cref'])
            print(name, 'runs', runs, 'colsum', ec)
            assert ec < 1e-4, (runs, ec)

    run(arr); runs += 1; check()
    run(arr); runs += 1; check()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            run(arr)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(3):
        graph.replay(); runs += 1; check()
    for p, first in zip(probs, seen[0]):
        assert rel_fro(first, ALPHA * p['ref']) < 3e-4
    for later in seen[1:]:
        for a, b in zip(seen[0], later):
            assert torch.equal(a, b)


@pytest.mark.parametrize('shapes', [
    [(768, 768, 960), (2304, 768, 960), (384, 768, 960), (768, 3072, 960), (3072, 768, 960)],      # 128x128 register-staged tiles
    [(384, 768, 1984), (768, 384, 1984), (100, 200, 1984)],               # 64x64 tiles, ragged edge
    [(64, 72, 130)],                                                      # K tail (K % 64 != 0): rows past K add nothing
])
def test_register_staged_colsum(ops, shapes):
    from prismer_amd import _lib
    probs = []
    for i, (M, N, K) in enumerate(shapes):
        Mp, Np = (M + 7) // 8 * 8, (N + 7) // 8 * 8
        dy = torch.zeros(K, Mp, dtype=BF, device='cuda'); dy[:, :M] = rnd(K, M, scale=0.3, seed=100 + i)
        x = torch.zeros(K, Np, dtype=BF, device='cuda'); x[:, :N] = rnd(K, N, scale=0.3, seed=200 + i)
        probs.append(dict(M=M, N=N, K=K, dy=dy, x=x, gw0=torch.randn(M, N, device='cuda'), gb0=torch.randn(M, device='cuda')))
    gws = [p['gw0'].clone() for p in probs]
    gbs = [p['gb0'].clone() for p in probs]
    arr = group_args(probs, gws, gbs, None, True)
    assert plan_of(arr) == (0, 0)                                         # not the persistent kernel
    cnt = (C.c_int64 * 16)()
    _lib.lib.ph_gemm_dispatch_counts(cnt, 16, 1)
    run(arr)
    torch.cuda.synchronize()
    _lib.lib.ph_gemm_dispatch_counts(cnt, 16, 0)
    assert cnt[5] == 1, list(cnt)[:7]
    for p, gw, gb in zip(probs, gws, gbs):
        M, N = p['M'], p['N']
        assert rel_fro(gw - p['gw0'], ALPHA * (p['dy'][:, :M].float().t() @ p['x'][:, :N].float())) < 3e-4
        ec = rel_fro(gb - p['gb0'], p['dy'][:, :M].float().sum(0))
        print(shapes[0], M, 'colsum', ec)
        assert ec < 1e-4, (M, N, p['K'], ec)


def test_single_call_colsum(ops):
    """ph_gemm_bf16 with a_colsum is served as a group of one"""
    from prismer_amd import _lib
    p = problems('one_two_tiles')[0]
    gw, gb = torch.empty_like(p['gw0']), p['gb0'].clone()
    arr = group_args([p], [gw], [gb], None, False)
    _lib.check(_lib.lib.ph_gemm_bf16(C.byref(arr[0]), torch.cuda.current_stream().cuda_stream), 'ph_gemm_bf16')
    torch.cuda.synchronize()
    assert rel_fro(gw, ALPHA * p['ref']) < 3e-4
    assert rel_fro(gb - p['gb0'], p['cref']) < 1e-4
    arr[0].trans_a = 0                                                    # only the weight-gradient layout has the fused sums
    assert _lib.lib.ph_gemm_bf16(C.byref(arr[0]), torch.cuda.current_stream().cuda_stream) != 0


class _CountingLib:
    """the library with ph_colsum_grouped_bf16 counted"""

    def __init__(self, lib):
        self._lib, self.colsum_calls = lib, 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != 'ph_colsum_grouped_bf16':
            return fn

        def counted(*a):
            self.colsum_calls += 1
            return fn(*a)
        return counted


def test_queue_pairing(ops, monkeypatch):
    counting = _CountingLib(ops.lib)
    monkeypatch.setattr(ops, 'lib', counting)
    M, N, K = 384, 256, 1984
    dy, x, x2 = rnd(K, M, scale=0.3, seed=1), rnd(K, N, scale=0.3, seed=2), rnd(K, N, scale=0.3, seed=3)
    lone = rnd(K, 200, scale=0.3, seed=4)
    cref = dy.float().sum(0)
    # (a) a paired queue: the sum rides with the GEMM, no colsum launch
    q = ops.WgradQueue()
    gw, gb = torch.zeros(M, N, device='cuda'), torch.zeros(M, device='cuda')
    q.add_gemm(dy, x, gw, M, N, K); q.add_colsum(dy, gb, M)
    assert q.cols
    q.flush(); torch.cuda.synchronize()
    assert counting.colsum_calls == 0 and not q.cols and not q.gemms
    assert rel_fro(gw, dy.float().t() @ x.float()) < 3e-4 and rel_fro(gb, cref) < 1e-4
    # (b) two GEMMs on one dy, one cols entry: summed once
    gw1, gw2, gb = torch.zeros(M, N, device='cuda'), torch.zeros(M, N, device='cuda'), torch.zeros(M, device='cuda')
    q.add_gemm(dy, x, gw1, M, N, K); q.add_gemm(dy, x2, gw2, M, N, K); q.add_colsum(dy, gb, M)
    q.flush(); torch.cuda.synchronize()
    assert counting.colsum_calls == 0
    assert rel_fro(gb, cref) < 1e-4
    assert rel_fro(gw1, dy.float().t() @ x.float()) < 3e-4 and rel_fro(gw2, dy.float().t() @ x2.float()) < 3e-4
    # (c) an entry without a partner (another tensor; and a dy whose row count differs from the GEMM's K) still gets its sum
    gw, gb, gl, gh = torch.zeros(M, N, device='cuda'), torch.zeros(M, device='cuda'), torch.zeros(200, device='cuda'), torch.zeros(M, device='cuda')
    half = dy[:K // 2]
    q.add_gemm(dy, x, gw, M, N, K); q.add_colsum(dy, gb, M); q.add_colsum(lone, gl, 200); q.add_colsum(half, gh, M)
    q.flush(); torch.cuda.synchronize()
    assert counting.colsum_calls == 1
    assert rel_fro(gb, cref) < 1e-4 and rel_fro(gl, lone.float().sum(0)) < 1e-4 and rel_fro(gh, half.float().sum(0)) < 1e-4
    # (d) the queue switched off keeps its immediate path
    q.enabled = False
    gb = torch.zeros(M, device='cuda')
    q.add_colsum(dy, gb, M); torch.cuda.synchronize()
    assert rel_fro(gb, cref) < 1e-4
