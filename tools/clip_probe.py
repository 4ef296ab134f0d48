"""Device-side gradient clipping / non-finite update skip (Trainer(max_grad_norm=, skip_nonfinite=)) on one device: what the guard costs, and that
the unguarded default is the step it was.  ONE process, the arms alternating inside every round (A, B, C, D, A, B, ...: box / clock drift cannot
pass for a difference).

    python tools/clip_probe.py --parent-tree DIR        # DIR/prismer_amd = the PARENT commit's python package (e.g. `git archive <parent> prismer_amd |
                                                        #   tar -x -C DIR`), run on the same library build.  Arms: parent, options off, parent, options off (the
                                                        #   difference of identical arms is the spread the probe itself measures), options on
    python tools/clip_probe.py                          # without a parent: off, off again, on
    python tools/clip_probe.py --configs base224 --rounds 7

Sizes: Prismer-BASE 224^2 / B = 32 and 480^2 / B = 4, T = 30, freeze_vision, hipGraph replay (bench.py's Trainer).
(a) options off against the parent: ms per step (best / median / spread over the rounds) and LIBRARY CALLS per step (entry-point calls of an
    instrumented eager pass, ph_prof_collect: equal between arms that run the same launch list; every entry point launches a fixed number of
    kernels, so equal calls = equal kernels).
(b) options on (max_grad_norm = 1, skip_nonfinite: the clip is active in every step): added milliseconds and added calls per step, and -- timed
    alone with events (one event pair per entry point, so each figure carries one launch), back to back over buffers of the configuration's
    n_train -- ph_grad_sqnorm's achieved read rate (4 B per parameter), ph_clip_finalize's time, and ph_adamw's achieved byte rate (16 B read + 14 B written per parameter).
Output: plain text, one block per configuration."""
import argparse
import ctypes
import gc
import importlib
import importlib.util
import os
import random
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                 # noqa: E402
import bench                                                 # noqa: E402
import prismer_amd                                           # noqa: E402
from prismer_amd import _lib, ops                            # noqa: E402

CONFIGS = {'base224': dict(res=224, batch=32), 'base480': dict(res=480, batch=4)}
FAMILIES = len(bench.FAMILIES)


def load_parent(tree):
    """the parent commit's python package under another name (its intra-package imports are relative), bound to the library already loaded"""
    os.environ['PRISMER_HIP_LIB'] = _lib.LIB_PATH
    root = os.path.join(tree, 'prismer_amd')
    spec = importlib.util.spec_from_file_location('prismer_amd_parent', os.path.join(root, '__init__.py'), submodule_search_locations=[root])
    mod = importlib.util.module_from_spec(spec)
    sys.modules['prismer_amd_parent'] = mod
    spec.loader.exec_module(mod)
    return mod


def build(pkg, cfg, kw):
    """bench.build_trainer's Prismer-BASE caption Trainer from package `pkg` (this tree's or the parent's)"""
    pcfg = importlib.import_module(pkg.__name__ + '.config')
    PrismerCaption = importlib.import_module(pkg.__name__ + '.model.prismer_caption').PrismerCaption
    Trainer = importlib.import_module(pkg.__name__ + '.trainer').Trainer
    torch.manual_seed(0)
    random.seed(0)
    dims = pcfg.prismer_base(image_resolution=cfg['res']) if cfg['res'] != 224 else pcfg.prismer_base()
    model = PrismerCaption({'experts': pcfg.CAPTION_EXPERTS, 'image_resolution': cfg['res'], 'prismer_model': 'prismer_base', 'freeze': 'freeze_vision'}).cuda()
    tr = Trainer(model, lr=5e-5, weight_decay=0.05, total_steps=10000, task='caption', use_graph=True, **kw)
    x, ids, mask, labels = bench.make_inputs(dims, cfg['batch'], 30, 1234, torch.device('cuda'), False)
    tr.set_batch(x, ids, mask, labels, None)
    return tr


def library_calls(tr):
    """entry-point calls of one eager step"""
    buf = (ctypes.c_double * (FAMILIES * 4))()
    graphs, tr.use_graph = tr.use_graph, False
    try:
        torch.cuda.synchronize()
        _lib.lib.ph_prof_enable(1)
        _lib.lib.ph_prof_collect(buf)
        tr.step()
        _lib.lib.ph_prof_collect(buf)
    finally:
        _lib.lib.ph_prof_enable(0)
        tr.use_graph = graphs
    return int(sum(buf[4 * i + 3] for i in range(FAMILIES)))


def kernel_rates(lengths, reps=20):
    """ph_grad_sqnorm + ph_clip_finalize and ph_adamw alone, over fresh buffers of these lengths: (us, GB/s) each, median of `reps` event-timed calls"""
    dev = torch.device('cuda')
    bufs = [[torch.randn(n, device=dev) * s for s in (1.0, 1e-3, 1e-3, 1e-6)] + [torch.zeros(n, device=dev, dtype=torch.bfloat16)] for n in lengths]
    for b in bufs:
        b[3].abs_()
    hyper = torch.tensor([5e-5, 0.1, 0.001], device=dev)
    ctl, ws = ops.ClipCtl(dev), ops.grad_norm_workspace(lengths, dev)
    t_norm, t_fin, t_adam = [], [], []
    for _ in range(reps + 3):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        ops.grad_sqnorm([b[1] for b in bufs], ws)
        e[1].record()
        ops.clip_finalize(ws, ctl, hyper, 1.0, 1.0, True)
        e[2].record()
        for b in bufs:
            ops.adamw(b[0], b[1], b[2], b[3], b[4], b[0].numel(), hyper)
        e[3].record()
        torch.cuda.synchronize()
        t_norm.append(e[0].elapsed_time(e[1])); t_fin.append(e[1].elapsed_time(e[2])); t_adam.append(e[2].elapsed_time(e[3]))
    n = sum(lengths)
    tn, ta = statistics.median(t_norm[3:]), statistics.median(t_adam[3:])
    return dict(n=n, norm_us=tn * 1e3, norm_gb_s=4.0 * n / tn / 1e6, norm_spread_us=(max(t_norm[3:]) - min(t_norm[3:])) * 1e3, fin_us=statistics.median(t_fin[3:]) * 1e3,
                adamw_us=ta * 1e3, adamw_gb_s=30.0 * n / ta / 1e6, adamw_spread_us=(max(t_adam[3:]) - min(t_adam[3:])) * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='base224,base480')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=40, help='steps timed per arm and round')
    ap.add_argument('--parent-tree', default=None)
    args = ap.parse_args()
    parent = load_parent(args.parent_tree) if args.parent_tree else None
    print(f'clip_probe: {torch.cuda.get_device_name(0)}, rounds {args.rounds}, {args.steps} steps per arm and round, arms alternate inside every round')
    for cname in args.configs.split(','):
        cfg = CONFIGS[cname]
        base_pkg, base_name = (parent, 'parent') if parent else (prismer_amd, 'options off')
        # (identical arms are built and timed interleaved: parent, off, parent, off -- an arm's place in the build order, i.e. where the allocator put
        # its buffers, shows up as a few hundredths of a millisecond, and must not pass for a difference between the packages)
        if parent:
            arms = [('parent (1)', parent, {}), ('options off (1)', prismer_amd, {}), ('parent (2)', parent, {}), ('options off (2)', prismer_amd, {})]
        else:
            arms = [(base_name + ' (1)', base_pkg, {}), (base_name + ' (2)', base_pkg, {})]
        arms.append(('max_grad_norm=1 + skip', prismer_amd, dict(max_grad_norm=1.0, skip_nonfinite=True)))
        built = []
        for name, pkg, kw in arms:
            tr = build(pkg, cfg, kw)
            for _ in range(3):
                loss = tr.step()
            torch.cuda.synchronize()
            built.append(dict(name=name, tr=tr, calls=library_calls(tr), ms=[], first=float(loss.item())))
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
            print(f'{arm["name"]:24s} ms/step best {min(t):8.3f} median {statistics.median(t):8.3f} spread {max(t) - min(t):6.3f} | library calls per step (eager pass) '
                  f'{arm["calls"]} | rounds {" ".join(f"{x:.3f}" for x in t)} | loss {arm["first"]:.4f} -> {arm["loss"]:.4f}', flush=True)
        med = {arm['name']: statistics.median(arm['ms']) for arm in built}
        calls = {arm['name']: arm['calls'] for arm in built}
        twin = abs(med[base_name + ' (1)'] - med[base_name + ' (2)'])
        off = 'options off (1)'
        on = built[-1]
        med_off = 0.5 * (med['options off (1)'] + med['options off (2)'])
        print(f'(a) spread between the two identical {base_name!r} arms (medians): {twin:.3f} ms' +
              (f'; between the two identical options-off arms: {abs(med["options off (1)"] - med["options off (2)"]):.3f} ms; options off - parent (means of the two): '
               f'{med_off - 0.5 * (med["parent (1)"] + med["parent (2)"]):+.3f} ms; library calls {calls[off]} vs {calls["parent (1)"]}' if parent else ''))
        tr_on = on['tr']
        print(f'(b) options on - options off: {med[on["name"]] - med_off:+.3f} ms per step, {calls[on["name"]] - calls[off]:+d} library calls per step; '
              f'grad_norm {tr_on.grad_norm.item():.4f}, coef {tr_on.ctl.coef.item():.6f}, applied / skipped {tr_on.applied_updates} / {tr_on.skipped_updates}')
        lengths = [st.n_train for st in tr_on.stores if st.n_train]
        for arm in built:
            arm['tr'] = None
        del built, tr, tr_on, on
        gc.collect(); torch.cuda.empty_cache()
        k = kernel_rates(lengths)
        print(f'    kernels alone at n_train = {k["n"]} ({lengths}): ph_grad_sqnorm {k["norm_us"]:.1f} us = {k["norm_gb_s"]:.0f} GB/s read (4 B/parameter; spread '
              f'{k["norm_spread_us"]:.1f} us) + ph_clip_finalize {k["fin_us"]:.1f} us | ph_adamw {k["adamw_us"]:.1f} us = {k["adamw_gb_s"]:.0f} GB/s (30 B/parameter; spread {k["adamw_spread_us"]:.1f} us)', flush=True)


if __name__ == '__main__':
    main()
