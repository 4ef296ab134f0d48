"""n texts per image (Trainer(texts_per_image=n), ph_attention_group_fwd / _bwd) on one device: what the grouped cross-attention kernels cost
against the routes they replace, and what a step on n texts per image costs against the step on the image-tiled batch.  ONE process, the arms
alternating inside every round (box / clock drift cannot pass for a difference); hipGraph replay everywhere.

    python tools/group_probe.py --parent-tree DIR       # DIR/prismer_amd = the PARENT commit's python package (e.g. `git archive <parent> prismer_amd |
                                                        #   tar -x -C DIR`), run on the same library build
    python tools/group_probe.py                         # without a parent: the tiled arm is this tree's Trainer(texts_per_image=1)
    python tools/group_probe.py --only layer            # part (a) alone; --only step: part (b) alone

(a) ONE cross-attention layer, forward + backward, Bi = 32 images, n = 5, T = 30, S = 260, H = 12 (dh = 64), dropout 0.1, K / V and dK / dV as
    column slices of a 12-layer buffer.  Arms: the grouped kernels, twice (the difference of identical arms is the spread the probe itself
    measures); the same entry points routed to the small-query kernels on tiled K / V + the fold (ph_attention_group_tuning(0)); the backward
    alone on either route; the streaming kernels on the [Bi, n*T] query view (one ungrouped launch per direction, other dropout words).
(b) a Prismer-BASE step, 224^2, T = 30, freeze_vision: texts_per_image = 5 on 32 images against the parent's step on the same 160 texts with the
    images tiled (batch 160), each twice, and texts_per_image = 1 at batch 32 against the parent: ms per step, texts/s, device memory the arm holds
    once captured and its peak up to there (allocated bytes), library calls of an eager step.
Output: plain text (profiles/group_probe.txt is one run of it)."""
import argparse
import gc
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                 # noqa: E402
import prismer_amd                                           # noqa: E402
from prismer_amd import _lib, ops                            # noqa: E402

BF = torch.bfloat16


def _timed_rounds(arms, rounds, reps):
    """arms: [(name, graph)]; every round replays each arm `reps` times between two events, arms in order"""
    ms = {name: [] for name, _ in arms}
    for _ in range(rounds):
        for name, g in arms:
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                g.replay()
            e1.record(); torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / reps)
    return ms


def layer_probe(Bi=32, n=5, T=30, S=260, H=12, L=12, rounds=7, reps=200):
    dh = 64
    D, R = H * dh, Bi * n
    dev = torch.device('cuda')
    gen = torch.Generator(device=dev).manual_seed(0)
    q = torch.randn(R * T, D, generator=gen, device=dev).to(BF)
    kva = torch.randn(Bi * S, 2 * D * L, generator=gen, device=dev).to(BF)
    d_o = torch.randn(R * T, D, generator=gen, device=dev).to(BF)
    kv = kva[:, 2 * D * 5:2 * D * 6]
    dkva = torch.zeros_like(kva)
    dkv = dkva[:, 2 * D * 5:2 * D * 6]
    k, v = kv[:, :D], kv[:, D:]
    seed = torch.tensor([4242], dtype=torch.int64, device=dev)
    drop = ops.Dropout(0.1, seed, 11)
    qs, ks = (T * D, D), (S * kv.stride(0), kv.stride(0))
    dq = torch.empty_like(q)
    gkw = dict(q_strides=qs, k_strides=ks, v_strides=ks, drop=drop)
    bkw = dict(dq=dq, dk=dkv[:, :D], dv=dkv[:, D:], dq_strides=qs, dk_strides=ks, dv_strides=ks, **gkw)
    o_ref, lse_ref = ops.attention_group_fwd(q, k, v, R, n, H, T, S, dh, **gkw)

    def grouped(fwd=True, bwd=True):
        def run():
            o, lse = ops.attention_group_fwd(q, k, v, R, n, H, T, S, dh, **gkw) if fwd else (o_ref, lse_ref)
            if bwd:
                ops.attention_group_bwd(d_o, q, k, v, o, lse, R, n, H, T, S, dh, **bkw)
        return run

    def streaming():
        qv = ((n * T) * D, D)
        o, lse = ops.attention_fwd(q, k, v, Bi, H, n * T, S, dh, q_strides=qv, k_strides=ks, v_strides=ks, drop=drop)
        ops.attention_bwd(d_o, q, k, v, o, lse, Bi, H, n * T, S, dh, q_strides=qv, k_strides=ks, v_strides=ks, dq=dq, dk=dkv[:, :D], dv=dkv[:, D:],
                          dq_strides=qv, dk_strides=ks, dv_strides=ks, drop=drop)

    def capture(fn, route):
        old = _lib.lib.ph_attention_group_tuning(route)
        try:
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                fn()
        finally:
            _lib.lib.ph_attention_group_tuning(old)
        return g
    arms = [('grouped kernels (1)', capture(grouped(), 3)), ('tiled small-query + fold', capture(grouped(), 0)), ('grouped kernels (2)', capture(grouped(), 3)),
            ('streaming, [Bi, n*T] view', capture(streaming, 3)), ('backward alone: grouped', capture(grouped(fwd=False), 3)),
            ('backward alone: tiled + fold', capture(grouped(fwd=False), 0)), ('forward alone: grouped', capture(grouped(bwd=False), 3)),
            ('forward alone: tiled', capture(grouped(bwd=False), 0))]
    # the two routes compute the same thing
    _lib.lib.ph_attention_group_tuning(3); grouped()(); a = (dq.clone(), dkv.clone())
    _lib.lib.ph_attention_group_tuning(0); grouped()(); b = (dq.clone(), dkv.clone())
    _lib.lib.ph_attention_group_tuning(3)
    rel = lambda x, y: float((x.float() - y.float()).norm() / y.float().norm())
    ms = _timed_rounds(arms, rounds, reps)
    print(f'\n== (a) one cross-attention layer, forward + backward: Bi = {Bi}, n = {n} (R = {R} text rows), T = {T}, S = {S}, H = {H}, dh = {dh}, dropout 0.1; '
          f'{rounds} rounds x {reps} graph replays, arms alternating')
    for name, _ in arms:
        t = ms[name]
        print(f'{name:30s} us per pass: best {min(t) * 1e3:8.1f} median {statistics.median(t) * 1e3:8.1f} spread {(max(t) - min(t)) * 1e3:6.1f} | rounds '
              f'{" ".join(f"{x * 1e3:.1f}" for x in t)}', flush=True)
    med = {name: statistics.median(t) * 1e3 for name, t in ms.items()}
    twin = abs(med['grouped kernels (1)'] - med['grouped kernels (2)'])
    g_med = 0.5 * (med['grouped kernels (1)'] + med['grouped kernels (2)'])
    print(f'spread between the two identical grouped arms (medians): {twin:.1f} us; grouped - tiled: {g_med - med["tiled small-query + fold"]:+.1f} us '
          f'({g_med / med["tiled small-query + fold"]:.3f} x); grouped - streaming view: {g_med - med["streaming, [Bi, n*T] view"]:+.1f} us; '
          f'backward alone grouped - tiled: {med["backward alone: grouped"] - med["backward alone: tiled + fold"]:+.1f} us; forward alone grouped - tiled: '
          f'{med["forward alone: grouped"] - med["forward alone: tiled"]:+.1f} us')
    print(f'grouped against the tiled route on the same inputs: dq {"bit-equal" if torch.equal(a[0], b[0]) else rel(a[0], b[0])}, dk | dv rel. difference '
          f'{rel(a[1], b[1]):.2e} (one rounding of the fp32 member sum against the fold of bf16 per-row results)')


def step_probe(parent, Bi=32, n=5, rounds=5, steps=20):
    import bench
    from clip_probe import library_calls
    import importlib
    import random

    def build(pkg, images, texts, kw, tile):
        pcfg = importlib.import_module(pkg.__name__ + '.config')
        PrismerCaption = importlib.import_module(pkg.__name__ + '.model.prismer_caption').PrismerCaption
        Trainer = importlib.import_module(pkg.__name__ + '.trainer').Trainer
        torch.manual_seed(0)
        random.seed(0)
        dims = pcfg.prismer_base()
        model = PrismerCaption({'experts': pcfg.CAPTION_EXPERTS, 'image_resolution': 224, 'prismer_model': 'prismer_base', 'freeze': 'freeze_vision'}).cuda()
        tr = Trainer(model, lr=5e-5, weight_decay=0.05, total_steps=10000, task='caption', use_graph=True, **kw)
        dev = torch.device('cuda')
        x, _, _, _ = bench.make_inputs(dims, images, 30, 1234, dev, False)
        _, ids, mask, labels = bench.make_inputs(dims, texts, 30, 1234, dev, False)
        if tile > 1:
            x = {k: ({a: b.repeat_interleave(tile, 0) for a, b in v.items()} if isinstance(v, dict) else v.repeat_interleave(tile, 0)) for k, v in x.items()}
        tr.set_batch(x, ids, mask, labels, None)
        return tr
    base_pkg = parent or prismer_amd
    bname = 'parent' if parent else 'texts_per_image=1'
    R = Bi * n
    arms = [(f'{bname}, images tiled to {R} (1)', base_pkg, Bi, R, {}, n, R), (f'texts_per_image={n}, {Bi} images (1)', prismer_amd, Bi, R, dict(texts_per_image=n), 1, R),
            (f'{bname}, images tiled to {R} (2)', base_pkg, Bi, R, {}, n, R), (f'texts_per_image={n}, {Bi} images (2)', prismer_amd, Bi, R, dict(texts_per_image=n), 1, R),
            (f'{bname}, batch {Bi} (1)', base_pkg, Bi, Bi, {}, 1, Bi), (f'this tree, batch {Bi} (1)', prismer_amd, Bi, Bi, {}, 1, Bi),
            (f'{bname}, batch {Bi} (2)', base_pkg, Bi, Bi, {}, 1, Bi), (f'this tree, batch {Bi} (2)', prismer_amd, Bi, Bi, {}, 1, Bi)]
    built = []
    for name, pkg, images, texts, kw, tile, rows in arms:
        gc.collect(); torch.cuda.synchronize()
        held0 = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        tr = build(pkg, images, texts, kw, tile)
        for _ in range(3):
            loss = tr.step()
        torch.cuda.synchronize()
        # what the arm holds once captured (weights, optimizer state, static inputs, the graph's activation pool) and the peak on the way there
        held, peak = torch.cuda.memory_allocated() - held0, torch.cuda.max_memory_allocated() - held0
        built.append(dict(name=name, tr=tr, rows=rows, calls=library_calls(tr), ms=[], first=float(loss.item()), held=held, peak=peak))
    for _ in range(rounds):
        for arm in built:
            tr = arm['tr']
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                loss = tr.step()
            e1.record(); torch.cuda.synchronize()
            arm['ms'].append(e0.elapsed_time(e1) / steps)
            arm['loss'] = float(loss.item())
    print(f'\n== (b) Prismer-BASE 224^2, T = 30, freeze_vision, hipGraph replay; {rounds} rounds x {steps} steps per arm, arms alternating')
    for arm in built:
        t = arm['ms']
        m = statistics.median(t)
        print(f'{arm["name"]:40s} ms/step best {min(t):8.3f} median {m:8.3f} spread {max(t) - min(t):6.3f} | {arm["rows"] / m * 1e3:8.1f} texts/s | library calls per '
              f'step (eager pass) {arm["calls"]} | holds {arm["held"] / 2 ** 20:.0f} MiB, peak {arm["peak"] / 2 ** 20:.0f} MiB | rounds {" ".join(f"{x:.3f}" for x in t)} | '
              f'loss {arm["first"]:.4f} -> {arm["loss"]:.4f}', flush=True)
    med = [statistics.median(a['ms']) for a in built]
    tiled, grp = 0.5 * (med[0] + med[2]), 0.5 * (med[1] + med[3])
    print(f'{R} texts per step: tiled batch {tiled:.3f} ms = {R / tiled * 1e3:.1f} texts/s, texts_per_image={n} {grp:.3f} ms = {R / grp * 1e3:.1f} texts/s '
          f'({tiled / grp:.2f} x); spread between identical arms (medians): tiled {abs(med[0] - med[2]):.3f} ms, texts_per_image={n} {abs(med[1] - med[3]):.3f} ms')
    print(f'n = 1 at batch {Bi}: this tree - {bname} (means of the two arms each): {0.5 * (med[5] + med[7]) - 0.5 * (med[4] + med[6]):+.3f} ms; spread between '
          f'identical arms: {bname} {abs(med[4] - med[6]):.3f} ms, this tree {abs(med[5] - med[7]):.3f} ms; library calls {built[5]["calls"]} vs {built[4]["calls"]}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--only', default=None, choices=[None, 'layer', 'step'])
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=20, help='steps timed per arm and round in part (b)')
    args = ap.parse_args()
    print(f'group_probe: {torch.cuda.get_device_name(0)}')
    if args.only in (None, 'layer'):
        layer_probe()
    if args.only in (None, 'step'):
        from clip_probe import load_parent
        step_probe(load_parent(args.parent_tree) if args.parent_tree else None, rounds=args.rounds, steps=args.steps)


if __name__ == '__main__':
    main()
