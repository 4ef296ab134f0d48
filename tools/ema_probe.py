"""Weight average fused into the AdamW launch (Trainer(ema_decay=)) on one device: what it costs, and that the default (no average) is the step it
was.  ONE process, the arms alternating inside every round (A, B, C, D, A, B, ...: box / clock drift cannot pass for a difference).

    python tools/ema_probe.py --parent-tree DIR         # DIR/prismer_amd = the PARENT commit's python package (e.g. `git archive <parent> prismer_amd |
                                                        #   tar -x -C DIR`), run on the same library build.  Arms: parent, ema off, parent, ema off (the
                                                        #   difference of identical arms is the spread the probe itself measures), ema on
    python tools/ema_probe.py                           # without a parent: off, off again, on
    python tools/ema_probe.py --configs base224,base480 --rounds 7

Sizes: Prismer-BASE 224^2 / B = 32 (bench.py's configuration) and, on request, 480^2 / B = 4; T = 30, freeze_vision, hipGraph replay.
(a) ema off against the parent: ms per step (best / median / spread over the rounds) and LIBRARY CALLS per step (entry-point calls of an
    instrumented eager pass, ph_prof_collect: equal between arms that run the same launch list).
(b) ema on (ema_decay = 0.9999, ema_warmup): added milliseconds and calls per step, and the device memory the arm holds beyond an ema-off arm
    (allocated bytes after build + capture, and the peak of one replayed step) against 4 B per trainable parameter.
(c) ph_adamw_ema (38 B/parameter) against ph_adamw_keep (30 B/parameter) alone, event-timed, ALTERNATING launches over the same buffers of the
    configuration's n_train: us and TB/s (medians), the added time, and what a separate 12 B/parameter pass would take at ph_adamw_keep's rate.
Output: plain text, one block per configuration."""
import argparse
import gc
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                 # noqa: E402
import prismer_amd                                           # noqa: E402
from prismer_amd import ops                                  # noqa: E402
from clip_probe import CONFIGS, build, library_calls, load_parent      # noqa: E402


def kernel_rates(lengths, reps=20):
    """ph_adamw_keep and ph_adamw_ema alone over the same buffers of these lengths, alternating: (us, GB/s) each, median of `reps` event-timed calls"""
    dev = torch.device('cuda')
    bufs = [[torch.randn(n, device=dev) * s for s in (1.0, 1e-3, 1e-3, 1e-6)] + [torch.zeros(n, device=dev, dtype=torch.bfloat16), torch.randn(n, device=dev)]
            for n in lengths]
    for b in bufs:
        b[3].abs_()
    hyper = torch.tensor([5e-5, 0.1, 0.001], device=dev)
    ema_w = torch.tensor([1e-4], device=dev)
    t_keep, t_ema = [], []
    for _ in range(reps + 3):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        for b in bufs:
            ops.adamw(b[0], b[1], b[2], b[3], b[4], b[0].numel(), hyper)
        e[1].record()
        for b in bufs:
            ops.adamw_ema(b[0], b[1], b[2], b[3], b[4], b[0].numel(), hyper, b[5], ema_w)
        e[2].record()
        torch.cuda.synchronize()
        t_keep.append(e[0].elapsed_time(e[1])); t_ema.append(e[1].elapsed_time(e[2]))
    n = sum(lengths)
    tk, te = statistics.median(t_keep[3:]), statistics.median(t_ema[3:])
    return dict(n=n, keep_us=tk * 1e3, keep_tb_s=30.0 * n / tk / 1e9, keep_spread_us=(max(t_keep[3:]) - min(t_keep[3:])) * 1e3,
                ema_us=te * 1e3, ema_tb_s=38.0 * n / te / 1e9, ema_spread_us=(max(t_ema[3:]) - min(t_ema[3:])) * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='base224')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=40, help='steps timed per arm and round')
    ap.add_argument('--parent-tree', default=None)
    args = ap.parse_args()
    parent = load_parent(args.parent_tree) if args.parent_tree else None
    print(f'ema_probe: {torch.cuda.get_device_name(0)}, rounds {args.rounds}, {args.steps} steps per arm and round, arms alternate inside every round')
    for cname in args.configs.split(','):
        cfg = CONFIGS[cname]
        base_pkg, base_name = (parent, 'parent') if parent else (prismer_amd, 'ema off')
        if parent:
            arms = [('parent (1)', parent, {}), ('ema off (1)', prismer_amd, {}), ('parent (2)', parent, {}), ('ema off (2)', prismer_amd, {})]
        else:
            arms = [(base_name + ' (1)', base_pkg, {}), (base_name + ' (2)', base_pkg, {})]
        arms.append(('ema_decay=0.9999 + warmup', prismer_amd, dict(ema_decay=0.9999, ema_warmup=True)))
        built = []
        for name, pkg, kw in arms:
            gc.collect(); torch.cuda.synchronize()
            held0 = torch.cuda.memory_allocated()
            tr = build(pkg, cfg, kw)
            for _ in range(3):
                loss = tr.step()
            torch.cuda.synchronize()
            held = torch.cuda.memory_allocated() - held0
            torch.cuda.reset_peak_memory_stats()
            base_alloc = torch.cuda.memory_allocated()
            tr.step()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base_alloc
            built.append(dict(name=name, tr=tr, calls=library_calls(tr), ms=[], first=float(loss.item()), held=held, step_peak=peak))
        for r in range(args.rounds):
            for arm in built:
                tr = arm['tr']
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.steps):
                    loss = tr.step()
                e1.record(); torch.cuda.synchronize()
                arm['ms'].append(e0.elapsed_time(e1) / args.steps)
                arm['loss'] = float(loss.item())
        print(f'\n== {cname}: Prismer-BASE {cfg["res"]}^2, batch {cfg["batch"]}, T = 30, freeze_vision, hipGraph replay')
        for arm in built:
            t = arm['ms']
            print(f'{arm["name"]:26s} ms/step best {min(t):8.3f} median {statistics.median(t):8.3f} spread {max(t) - min(t):6.3f} | library calls per step (eager pass) '
                  f'{arm["calls"]} | held {arm["held"] / 2 ** 20:9.1f} MiB, step peak +{arm["step_peak"] / 2 ** 20:.1f} MiB | rounds {" ".join(f"{x:.3f}" for x in t)} | '
                  f'loss {arm["first"]:.4f} -> {arm["loss"]:.4f}', flush=True)
        med = {arm['name']: statistics.median(arm['ms']) for arm in built}
        calls = {arm['name']: arm['calls'] for arm in built}
        held = {arm['name']: arm['held'] for arm in built}
        twin = abs(med[base_name + ' (1)'] - med[base_name + ' (2)'])
        off = 'ema off (1)'
        on = built[-1]
        med_off = 0.5 * (med['ema off (1)'] + med['ema off (2)'])
        print(f'(a) spread between the two identical {base_name!r} arms (medians): {twin:.3f} ms' +
              (f'; between the two identical ema-off arms: {abs(med["ema off (1)"] - med["ema off (2)"]):.3f} ms; ema off - parent (means of the two): '
               f'{med_off - 0.5 * (med["parent (1)"] + med["parent (2)"]):+.3f} ms; library calls {calls[off]} vs {calls["parent (1)"]}' if parent else ''))
        tr_on = on['tr']
        lengths = [st.n_train for st in tr_on.stores if st.n_train]
        n = sum(lengths)
        print(f'(b) ema on - ema off: {med[on["name"]] - med_off:+.3f} ms per step, {calls[on["name"]] - calls[off]:+d} library calls per step; memory held '
              f'{(held[on["name"]] - held[off]) / 2 ** 20:+.1f} MiB against ema off (1), {(held[on["name"]] - held["ema off (2)"]) / 2 ** 20:+.1f} MiB against ema off (2) '
              f'(4 B x {n} trainable parameters = {4 * n / 2 ** 20:.1f} MiB); step peak {(on["step_peak"] - built[1 if parent else 0]["step_peak"]) / 2 ** 20:+.1f} MiB; '
              f'it {tr_on.it}, w = {tr_on._ema_w.item():.6g}, |ema - master| / |master| = '
              f'{[round(float((e[:st.n_train] - st.master[:st.n_train]).norm() / st.master[:st.n_train].norm()), 6) for st, e in zip(tr_on.stores, tr_on.ema)]}')
        for arm in built:
            arm['tr'] = None
        del built, tr, tr_on, on
        gc.collect(); torch.cuda.empty_cache()
        k = kernel_rates(lengths)
        sep_us = 12.0 * k['n'] / (k['keep_tb_s'] * 1e12) * 1e6
        print(f'(c) kernels alone at n_train = {k["n"]} ({lengths}), alternating launches: ph_adamw_keep {k["keep_us"]:.1f} us = {k["keep_tb_s"]:.2f} TB/s (30 B/parameter; '
              f'spread {k["keep_spread_us"]:.1f} us) | ph_adamw_ema {k["ema_us"]:.1f} us = {k["ema_tb_s"]:.2f} TB/s (38 B/parameter; spread {k["ema_spread_us"]:.1f} us) | '
              f'fused average adds {k["ema_us"] - k["keep_us"]:+.1f} us; a separate 12 B/parameter pass at ph_adamw_keep\'s rate would take {sep_us:.1f} us (+ a launch)', flush=True)


if __name__ == '__main__':
    main()
