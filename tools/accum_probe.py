"""Gradient accumulation (Trainer(accum_steps=k)) on one device: what a micro-step and an update cost, in ONE process with the arms alternating
(A, B, C, A, B, C, ...: box / clock drift cannot pass for a difference).

    python tools/accum_probe.py                                   # Prismer-BASE 224^2 / B = 32 and 480^2 / B = 4, accum_steps in {1, 8, 64}
    python tools/accum_probe.py --parent-tree DIR                 # + an arm running the PARENT commit's python package (DIR/prismer_amd, e.g. from
                                                                  #   `git archive <parent> prismer_amd | tar -x -C DIR`) on the same library build:
                                                                  #   accum_steps = 1 must sit inside the spread of that arm's own repeated rounds
    python tools/accum_probe.py --configs base224 --accum 1,8 --rounds 7

Per arm: ms per micro-step (best / median over the rounds), ms per update, images/s, peak memory (allocator: reserved bytes while this arm was
built, captured and first run), LIBRARY CALLS per micro-step by kind (entry-point calls of an instrumented EAGER pass: ph_prof_collect -- some
entry points launch two kernels, so this is NOT the kernel count of a trace; it is equal between arms that run the same launch list).
Every arm owns its model, weights and graphs; all start from the same seed.  Output: plain text, one block per configuration.

KERNELS per micro-step come from a kernel trace of the replayed graphs, one arm per traced process:
    rocprofv3 --kernel-trace -d OUT -o kt -- python tools/accum_probe.py --trace-arm 8 [--configs base224] [--parent-tree DIR with --trace-arm parent]
    python tools/accum_probe.py --count-trace OUT 8        # dispatches between the once-per-micro-step ce_fwd_kernel launches, whole groups only"""
import argparse
import ctypes
import importlib.util
import os
import random
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                 # noqa: E402
import bench                                                 # noqa: E402
import prismer_amd                                           # noqa: E402
from prismer_amd import _lib                                 # noqa: E402

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


def build(pkg, cfg, accum):
    """bench.build_trainer's Prismer-BASE caption Trainer from package `pkg` (this tree's or the parent's)"""
    import importlib
    pcfg = importlib.import_module(pkg.__name__ + '.config')
    PrismerCaption = importlib.import_module(pkg.__name__ + '.model.prismer_caption').PrismerCaption
    Trainer = importlib.import_module(pkg.__name__ + '.trainer').Trainer
    torch.manual_seed(0)
    random.seed(0)
    dims = pcfg.prismer_base(image_resolution=cfg['res']) if cfg['res'] != 224 else pcfg.prismer_base()
    model = PrismerCaption({'experts': pcfg.CAPTION_EXPERTS, 'image_resolution': cfg['res'], 'prismer_model': 'prismer_base', 'freeze': 'freeze_vision'}).cuda()
    kw = {} if accum is None else dict(accum_steps=accum)
    tr = Trainer(model, lr=5e-5, weight_decay=0.05, total_steps=10000, task='caption', use_graph=True, **kw)
    x, ids, mask, labels = bench.make_inputs(dims, cfg['batch'], 30, 1234, torch.device('cuda'), False)
    tr.set_batch(x, ids, mask, labels, None)
    return tr


def launches_by_kind(tr, k):
    """library entry-point calls of one eager micro-step of every kind (open / middle / close, or the whole step)"""
    out = {}
    buf = (ctypes.c_double * (FAMILIES * 4))()
    graphs, tr.use_graph = tr.use_graph, False
    try:
        for j in sorted({0, min(1, k - 1), k - 1}):
            while getattr(tr, 'micro_index', 0) != j:
                tr.step()
            torch.cuda.synchronize()
            _lib.lib.ph_prof_enable(1)
            _lib.lib.ph_prof_collect(buf)
            tr.step()
            _lib.lib.ph_prof_collect(buf)
            _lib.lib.ph_prof_enable(0)
            kind = 'whole' if k == 1 else 'open' if j == 0 else 'close' if j == k - 1 else 'middle'
            out[kind] = int(sum(buf[4 * i + 3] for i in range(FAMILIES)))
        while getattr(tr, 'micro_index', 0) != 0:
            tr.step()
        torch.cuda.synchronize()
    finally:
        _lib.lib.ph_prof_enable(0)
        tr.use_graph = graphs
    return out


def trace_arm(args):
    """one arm, for a kernel trace: capture, then 4 whole groups (at least 16 micro-steps) of replays"""
    cfg = CONFIGS[args.configs.split(',')[0]]
    if args.trace_arm == 'parent':
        tr, k = build(load_parent(args.parent_tree), cfg, None), 1
    else:
        k = int(args.trace_arm)
        tr = build(prismer_amd, cfg, k)
    for _ in range(max(4, -(-16 // k)) * k):
        tr.step()
    torch.cuda.synchronize()
    print('traced arm', args.trace_arm, 'micro_index', getattr(tr, 'micro_index', 0))


def count_trace(out_dir, k):
    """kernels per micro-step from the rocpd database(s) under out_dir: the last 2 k micro-steps' worth of dispatches, delimited by ce_fwd_kernel (one per forward)"""
    import glob
    import sqlite3
    for db in sorted(glob.glob(os.path.join(out_dir, '**', '*.db'), recursive=True)):
        cur = sqlite3.connect(db).cursor()
        ce = [r[0] for r in cur.execute("select start from kernels where name like '%ce_fwd_kernel%' order by start")]
        n = 2 * k if k > 1 else 8
        if len(ce) <= n:
            print(db, 'too few steps in the trace:', len(ce))
            continue
        t0, t1 = ce[-1 - n], ce[-1]
        cnt, busy = cur.execute(f'select count(*), sum(end - start) from kernels where start >= {t0} and start < {t1}').fetchone()
        print(f'{db}: accum_steps={k}: {cnt / n:.1f} kernels per micro-step over the last {n} micro-steps ({len(ce)} forwards traced), '
              f'{busy / n / 1e6:.3f} ms of kernel time, {(t1 - t0) / n / 1e6:.3f} ms wall per micro-step')


def main():
    if len(sys.argv) > 1 and sys.argv[1] == '--count-trace':
        return count_trace(sys.argv[2], int(sys.argv[3]))
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='base224,base480')
    ap.add_argument('--accum', default='1,8,64')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--micro-steps', type=int, default=64, help='micro-steps timed per arm and round (rounded up to whole groups)')
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--no-launch-count', action='store_true')
    ap.add_argument('--trace-arm', default=None, help="'parent' or an accum_steps value: run that one arm only (under rocprofv3 --kernel-trace)")
    args = ap.parse_args()
    if args.trace_arm:
        return trace_arm(args)
    parent = load_parent(args.parent_tree) if args.parent_tree else None
    print(f'accum_probe: {torch.cuda.get_device_name(0)}, rounds {args.rounds}, >= {args.micro_steps} micro-steps per arm and round, arms alternate inside every round')
    for cname in args.configs.split(','):
        cfg = CONFIGS[cname]
        arms = ([('parent (accum n/a)', parent, None, 1)] if parent else []) + [(f'accum_steps={k}', prismer_amd, int(k), int(k)) for k in args.accum.split(',')]
        built = []
        for name, pkg, accum, k in arms:
            torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_reserved()
            tr = build(pkg, cfg, accum)
            for _ in range(2 * k):
                loss = tr.step()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_reserved() - base
            counts = {} if args.no_launch_count else launches_by_kind(tr, k)
            built.append(dict(name=name, tr=tr, k=k, peak=peak, counts=counts, ms=[], first=float(loss.item())))
        for r in range(args.rounds):
            for arm in built:
                tr, k = arm['tr'], arm['k']
                n = -(-args.micro_steps // k) * k
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n):
                    loss = tr.step()
                e1.record(); torch.cuda.synchronize()
                arm['ms'].append(e0.elapsed_time(e1) / n)
                arm['loss'] = float(loss.item())
        print(f'\n== {cname}: Prismer-BASE {cfg["res"]}^2, micro-batch {cfg["batch"]}, T = 30, freeze_vision, hipGraph replay')
        for arm in built:
            t, k, B = arm['ms'], arm['k'], cfg['batch']
            best, med = min(t), statistics.median(t)
            print(f'{arm["name"]:20s} ms/micro-step best {best:8.3f} median {med:8.3f} spread {max(t) - min(t):6.3f} | ms/update {med * k:9.2f} | images/s {B / med * 1e3:8.1f} '
                  f'| effective batch {B * k:5d} | peak reserved {arm["peak"] / 2 ** 30:6.2f} GiB | library calls (eager pass) {arm["counts"]} | rounds {" ".join(f"{x:.3f}" for x in t)} '
                  f'| loss {arm["first"]:.3f} -> {arm["loss"]:.3f}', flush=True)
        for arm in built:
            arm['tr'] = None
        del built, tr
        import gc
        gc.collect(); torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
