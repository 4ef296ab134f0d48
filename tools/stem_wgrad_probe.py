"""The stems' conv weight gradients in isolation: per-k-tile constant of the persistent 256x128 kernel with a gathered B against the plain
kernel (two reduction lengths of an uncut group of 324 tiles = two units on the longest block: slope = (t2 - t1) / extra k-tiles), and the headline's
per-layer groups as ONE gathered launch against the per-expert deferred split-K calls they replace.

    python tools/stem_wgrad_probe.py [OUT.txt]

Times are device events around 20 back-to-back repetitions after 5 warm-up launches (us per repetition)."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from prismer_amd import _lib, ops

BF = torch.bfloat16
# base_b32 stems, weight gradients of layers 4..1: (Cout, conv geometry (B, H, W, C, ks, stride)) x experts
LAYERS = {
    'layer4': [(768, (32, 28, 28, 384, 3, 2))] * 3 + [(768, (32, 14, 14, 384, 3, 1))] * 3,
    'layer3': [(384, (32, 56, 56, 192, 3, 2))] * 3 + [(384, (32, 14, 14, 192, 3, 1))] * 3,
    'layer2': [(192, (32, 112, 112, 96, 3, 2))] * 3 + [(192, (32, 28, 28, 96, 3, 2))] * 3,
    'layer1_label': [(96, (32, 56, 56, 64, 3, 2))] * 3,
}


def timed(fn, reps=20, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def item(Cout, conv, seed):
    B, H, W, Cc, ks, stride = conv
    Ho = ops.conv_out_size(H, ks, stride)
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = (torch.randn(B * H * W, Cc, device='cuda', generator=g) * 0.7).to(BF)
    dy = (torch.randn(B * Ho * Ho, Cout, device='cuda', generator=g) * 0.3).to(BF)
    return (dy, x, Cout, 9 * Cc, B * Ho * Ho, conv)


def route_of(items, ws):
    arr, *keep = ops.wgrad_group_args(items, ws)
    info = _lib.GemmRouteInfo()
    _lib.check(_lib.lib.ph_gemm_route(arr, len(items), 1, 0, C.byref(info)), 'ph_gemm_route')
    r = info.part[0]
    return f'cls {_lib.GEMM_CLS[r.cls]} {r.bm}x{r.bn} units {r.units} cut {r.max_split} fold {r.fold} ws {r.ws_bytes}'


def grouped_launch(items, ws):
    arr, *keep = ops.wgrad_group_args(items, ws)
    stream = torch.cuda.current_stream().cuda_stream
    return lambda: _lib.check(_lib.lib.ph_gemm_grouped_bf16(arr, len(items), stream), 'ph_gemm_grouped_bf16'), keep


def main():
    out = open(sys.argv[1], 'w') if len(sys.argv) > 1 else None

    def say(*a):
        line = ' '.join(str(x) for x in a)
        print(line, flush=True)
        if out:
            out.write(line + '\n')

    ws = torch.empty(ops.WS_BYTES // 4, dtype=torch.float32, device='cuda')
    # ---- per-k-tile constant: 4 x (768, 3456, K) uncut = 324 units, the longest block walks two; K = 98 and 196 k-tiles
    say('per-k-tile constant, uncut group of 4 x (768 x 3456) = 324 tiles (two units on the longest block), 14x14x384 stride 1:')
    t = {}
    for B in (32, 64):
        it = item(768, (B, 14, 14, 384, 3, 1), 1)
        col = ops.im2col(it[1].view(B, 14, 14, 384), B, 14, 14, 384, 3, 1, 3456)
        for kind, items in (('gathered', [it] * 4), ('plain', [(it[0], col, 768, 3456, it[4], None)] * 4)):
            fn, keep = grouped_launch(items, None)
            t[kind, B] = timed(fn)
            say(f'  {kind:9s} K = {it[4]:6d} ({it[4] // 64} k-tiles): {t[kind, B]:7.1f} us   [{route_of(items, None)}]')
        del col
    for kind in ('gathered', 'plain'):
        slope = (t[kind, 64] - t[kind, 32]) / 196.0
        say(f'  {kind:9s} per k-tile {slope:.3f} us, fixed part per unit {(t[kind, 32] - 196 * slope) / 2:.1f} us')
    # ---- the headline's layers: one gathered launch against the per-expert calls
    say('base_b32 layers, one persistent launch (gathered B) against the per-expert deferred split-K calls + their grouped fold pass:')
    for name, spec in LAYERS.items():
        items = [item(co, cv, 10 + i) for i, (co, cv) in enumerate(spec)]
        flops = sum(2.0 * it[2] * it[3] * it[4] for it in items)
        fn, keep = grouped_launch(items, ws)
        tg = timed(fn)

        def old():
            for dy, x, M, N, K, conv in items:
                ops.gemm(dy, x, trans_a=True, trans_b=True, out_f32=True, M=M, N=N, K=K, conv=conv, defer_reduce=True)
            ops.gemm_flush_deferred()
        to = timed(old)
        say(f'  {name:13s} grouped {tg:7.1f} us ({flops / tg / 1e6:6.1f} TFLOP/s)   per-expert {to:7.1f} us ({flops / to / 1e6:6.1f} TFLOP/s)   [{route_of(items, ws)}]')
    if out:
        out.close()


if __name__ == '__main__':
    main()
