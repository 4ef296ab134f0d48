"""The GEMM route table (tests/golden/gemm_routes.json): rows = (description of a call of ph_gemm_bf16 / ph_gemm_grouped_bf16 /
ph_gemm_grouped_capped_bf16, the ph_gemm_route_info the library answers for it).  tests/test_gemm_route_cpu.py asserts the table
field for field on a machine without a device, so a changed dispatch threshold is a diff of that file.

  python tools/gemm_routes.py harvest OUT.json [case ...]   GPU: one eager step (two, the first-writer bookkeeping differs) of each case
                                                            with the three entry points wrapped where prismer_amd/ops.py calls them
  python tools/gemm_routes.py record STEP.json              CPU: the hand-written threshold rows (hand_rows below) + the step rows, each with what
                                                            ph_gemm_route answers, written to the table
  python tools/gemm_routes.py drive OUT.pt                  GPU: issue every row of the table once on seeded operands (run it under
                                                            rocprofv3 --kernel-trace to list the launches); saves every output to OUT.pt
  python tools/gemm_routes.py compare A.pt B.pt             CPU: outputs of two drive runs -- bit-identical, float-atomic rows at a tolerance
  python tools/gemm_routes.py step CASE                     GPU: two eager training steps of a case (for the same trace)
  python tools/gemm_routes.py launches TRACE.db OUT.txt     the GEMM-family launches of a rocprofv3 kernel trace in order: kernel name with
                                                            template arguments, grid, workgroup, LDS bytes
  python tools/gemm_routes.py difflaunch A.txt B.txt        compares two such lists

A problem is described by the ph_gemm_args fields that differ from zero (alpha: from 1); pointers are stored as present / absent
(true / false), the workspace as its byte count, the conv gather as its twelve integers.  A row may carry `tuning`: the (big_mode,
big_min_tiles) of ph_gemm_tuning it is routed and run under (default: the library's)."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
TABLE = os.path.join(ROOT, 'tests', 'golden', 'gemm_routes.json')

INTS = ('M', 'N', 'K', 'lda', 'ldb', 'ldc', 'trans_a', 'trans_b', 'act', 'ld_act', 'ldr', 'drop_stream', 'out_f32', 'accumulate', 'split_k',
        'residual_f32', 'pre_grad', 'rowmap_wo', 'rowmap_mul', 'rowmap_sub', 'rowmap_add', 'defer_reduce')
FLOATS = ('drop_p',)
PTRS = ('bias', 'pre_out', 'act_in', 'residual', 'drop_seed', 'col_stats', 'a_colsum')
CONV = ('B', 'H', 'W', 'C', 'ks', 'stride', 'kh', 'kw', 'off_y', 'off_x', 'Ho', 'Wo')
INFO = ('cls', 'bm', 'bn', 'variant', 'units', 'max_split', 'fold', 'fold_lanes', 'ws_bytes')
CASES = ('base_b32', 'zbase_b32', 'large_vqa_b16')


def describe(g):
    """ph_gemm_args (ctypes) -> row problem"""
    d = {k: int(getattr(g, k)) for k in INTS if getattr(g, k)}
    d.update({k: float(getattr(g, k)) for k in FLOATS if getattr(g, k)})
    d.update({k: True for k in PTRS if getattr(g, k)})
    if g.alpha != 1.0:
        d['alpha'] = float(g.alpha)
    if g.workspace:
        d['workspace'] = int(g.workspace_bytes)
    if g.conv:
        d['conv'] = [int(getattr(g.conv.contents, k)) for k in CONV]
    return d


def args_of(row, ptr=lambda prob, name, i: 4096):
    """row -> (ph_gemm_args array, keep-alive list).  `ptr(problem, field, index)` supplies the address of a present pointer (the route looks
    at presence, alignment and at whether the workspaces of a group are one buffer only: the default hands every one the same address)."""
    from prismer_amd import _lib
    probs = row['problems']
    arr, keep = (_lib.GemmArgs * len(probs))(), []
    for i, (g, d) in enumerate(zip(arr, probs)):
        for k in INTS + FLOATS:
            setattr(g, k, d.get(k, 0))
        g.alpha = d.get('alpha', 1.0)
        for k in ('A', 'B', 'C') + PTRS:
            if k in 'ABC' or d.get(k):
                setattr(g, k, ptr(d, k, i))
        if d.get('workspace'):
            g.workspace, g.workspace_bytes = ptr(d, 'workspace', i), d['workspace']
        if 'conv' in d:
            cg = _lib.ConvGather(*d['conv'])
            keep.append(cg)
            g.conv = C.pointer(cg)
    return arr, keep


class tuned:
    """the row's ph_gemm_tuning for the duration of a with block"""

    def __init__(self, row):
        self.t = row.get('tuning')

    def __enter__(self):
        from prismer_amd import _lib
        if self.t:
            _lib.lib.ph_gemm_tuning(*self.t)

    def __exit__(self, *exc):
        from prismer_amd import _lib
        if self.t:
            _lib.lib.ph_gemm_tuning(*_lib.GEMM_BIG_DEFAULT)


def route_of(row):
    """the library's answer for a row, as the dict the table stores: the call's parts (two for a tail-split ph_gemm_bf16) with every field"""
    from prismer_amd import _lib
    arr, keep = args_of(row)
    info = _lib.GemmRouteInfo()
    with tuned(row):
        _lib.check(_lib.lib.ph_gemm_route(arr, len(arr), int(row['entry'] != 'single'), row.get('max_blocks', 0), C.byref(info)), 'ph_gemm_route')
    return {'parts': info.parts, 'tail_m': info.tail_m, 'part': [{k: int(getattr(info.part[p], k)) for k in INFO} for p in range(info.parts)]}


def prob(M, N, K, layout='NN', **kw):
    """a dense problem with tight leading dimensions (rows padded to 8 elements)"""
    ta, tb = int(layout[0] == 'T'), int(layout[1] == 'T')
    pad = lambda v: (v + 7) // 8 * 8
    d = dict(M=M, N=N, K=K, lda=pad(M) if ta else K, ldb=pad(N) if tb else K, ldc=N)
    if ta: d['trans_a'] = 1
    if tb: d['trans_b'] = 1
    d.update(kw)
    return d


def wgrad(M, N, K, ws=64 << 20, **kw):
    """[K][M] x [K][N] -> fp32, the weight-gradient call of prismer_amd/ops.py"""
    kw = dict(dict(out_f32=1, accumulate=1), **kw)
    if ws:
        kw['workspace'] = ws
    return prob(M, N, K, 'TT', **kw)


def conv_nn(H, W, C=64, N=128):
    """3x3 stride-1 forward gather of one H x W image: M = H * W rows, K = 9 C"""
    return dict(prob(H * W, N, 9 * C), conv=[1, H, W, C, 3, 1, 0, 0, 0, 0, 0, 0])


def hand_rows():
    """both sides of every threshold of the dispatch (prismer_amd/csrc/gemm.hip route_single / route_grouped); `note` says which"""
    S = lambda note, p, **kw: dict(dict(entry='single', problems=[p], note=note), **kw)
    Gr = lambda note, ps, **kw: dict(dict(entry='grouped', problems=ps, note=note), **kw)
    ragged = [(264, 136, 2048), (264, 136, 4160), (264, 136, 8320)]
    rows = [
        S('tail split: 1560 tiles = 3 rounds + 24 -> rows 8192 + 128', prob(8320, 3072, 768)),
        S('tail split off: 390 tiles fit one round', prob(8320, 768, 768)),
        S('tail split: overshoot 61 tiles <= 12 % of 512', prob(65664, 7808, 128)),
        S('tail split off: overshoot 62 tiles > 12 % of 512', prob(65792, 3968, 128)),
        S('256x128: 191 tiles, 12 k-tiles -> not', prob(191 * 256, 128, 768)),
        S('256x128: 192 tiles, 12 k-tiles', prob(192 * 256, 128, 768)),
        S('256x128: 191 tiles, 31 k-tiles -> not', prob(191 * 256, 128, 1984)),
        S('256x128: 191 tiles, 32 k-tiles', prob(191 * 256, 128, 2048)),
        S('cost tie (2 rounds of 256x128 = pair + lone round of 128x128), [N,K] B: 256x128', prob(10496, 1024, 768)),
        S('cost tie, [K,N] B: 128x128', prob(10496, 1024, 768, 'NT')),
        S('256x128 weight-gradient layout, 136 tiles, 32 k-tiles', wgrad(4352, 1024, 2048, ws=0)),
        S('256x128 TT, cost model bypassed: 64 tiles, 32 k-tiles', wgrad(2048, 1024, 2048, ws=0), tuning=[7, 1]),
        S('256x128 TT, cost model bypassed: 64 tiles, 31 k-tiles -> not', wgrad(2048, 1024, 1984, ws=0), tuning=[7, 1]),
        S('256x128 TT, cost model bypassed: 63 tiles -> not', wgrad(1792, 1152, 2048, ws=0), tuning=[7, 1]),
        S('big_mode 0: off', prob(8320, 768, 768), tuning=[0, 128]),
        S('big_mode 1: plain main loop', prob(8320, 768, 768), tuning=[1, 128]),
        S('big_mode 5: lean', prob(8320, 768, 768), tuning=[5, 128]),
        S('big_mode 6: lean', prob(8320, 768, 768), tuning=[6, 128]),
        S('ks2: 512 tiles of 64x64, 8 k-tiles', prob(2048, 1024, 512)),
        S('ks2 off: 513 tiles', prob(1728, 1216, 512)),
        S('ks2 off: 7 k-tiles', prob(2048, 1024, 448)),
        S('128x64 tiles: N = 192', prob(100352, 192, 864)),
        S('128x128 tiles: N = 320', prob(100352, 320, 864)),
        S('fold: 32 splits, 16384 vectors -> 16 lanes', wgrad(128, 512, 4096, split_k=32)),
        S('fold: 31 splits -> 1 lane', wgrad(128, 512, 3968, split_k=31)),
        S('fold: 32 splits, 16388 vectors -> 1 lane', wgrad(68, 964, 4096, split_k=32)),
        S('fold deferred', wgrad(128, 512, 4096, split_k=32, defer_reduce=1)),
        S('split without a workspace: fp32 atomics, no fold', wgrad(128, 512, 4096, ws=0, split_k=4)),
        S('auto split-K of a weight gradient with 2 tiles', wgrad(96, 32, 401408, accumulate=0)),
        Gr('grouped tile: 192 tiles of 128x128', [prob(2048, 1536, 768)]),
        Gr('grouped tile: 191 tiles -> 64x64', [prob(24448, 128, 768)]),
        Gr('grouped tile: 64 tiles, 32 k-tiles -> 128x128', [prob(1024, 1024, 2048)]),
        Gr('grouped tile: 64 tiles, 31 k-tiles -> 64x64', [prob(1024, 1024, 1984)]),
        Gr('grouped tile: 63 tiles, 32 k-tiles -> 64x64', [prob(896, 1152, 2048)]),
        Gr('grouped tile: a thin problem (M = 64) -> 64x64', [prob(2048, 1536, 768), prob(64, 1536, 768)]),
        Gr('grouped, K % 64 != 0: no prefetch ring', [prob(2048, 1536, 776)]),
        Gr('persistent plan: 32 k-tiles', [wgrad(1536, 768, 2048, ws=0)] * 4),
        Gr('persistent plan off: 31 k-tiles', [wgrad(1536, 768, 1984, ws=0)] * 4),
        Gr('persistent plan: tiles a multiple of 256 stay whole', [wgrad(1024, 2048, 4096)] * 16),
        Gr('persistent plan: workspace too small for any cut', [wgrad(*s, ws=1 << 20) for s in ragged]),
        Gr('persistent plan (40, 6)', [wgrad(*s) for s in ragged]),
        Gr('persistent plan without a workspace (12, 1)', [wgrad(*s, ws=0) for s in ragged]),
        Gr('persistent plan (12, 6)', [wgrad(512, 128, 8320)]),
        Gr('persistent plan (432, 3)', [wgrad(768, 384, 8320)] * 16),
        Gr('persistent plan (144, 1)', [wgrad(1536, 768, 4096)] * 4),
        Gr('register-staged split: 2 x 512 tiles = 1024 slots', [wgrad(512, 256, 1024)] * 16),
        Gr('register-staged split off: 2 x 513 tiles', [wgrad(512, 256, 1024)] * 15 + [wgrad(704, 192, 1024)]),
        Gr('capped launch stays on the register-staged kernel', [wgrad(1536, 768, 4096)] * 4, max_blocks=64),
        S('conv NN, M = 256: LDS-DMA gather', conv_nn(16, 16)),
        S('conv NN, M = 255: register gather', conv_nn(15, 17)),
        S('conv NN, big_mode 1: register gather', conv_nn(16, 16), tuning=[1, 128]),
        Gr('conv NN group', [conv_nn(32, 32), conv_nn(16, 16)]),
        Gr('conv TT (weight gradient, gathered B)', [dict(wgrad(128, 576, 256, ws=0), conv=[1, 16, 16, 64, 3, 1, 0, 0, 0, 0, 0, 0])]),
        S('conv TT, single call', dict(wgrad(128, 576, 256, ws=0), conv=[1, 16, 16, 64, 3, 1, 0, 0, 0, 0, 0, 0])),
        S('a_colsum: served as a group of one', wgrad(512, 128, 8320, ws=0, a_colsum=True)),
    ]
    return rows


def _key(row):
    return json.dumps({k: row[k] for k in ('entry', 'max_blocks', 'tuning', 'problems') if k in row}, sort_keys=True)


class _Harvest:
    """prismer_amd.ops.lib with the three GEMM entry points recorded"""

    def __init__(self, lib):
        self._lib, self.rows = lib, {}

    def _note(self, entry, arr, n, max_blocks, case):
        row = {'entry': entry, 'problems': [describe(arr[i]) for i in range(n)]}
        if max_blocks:
            row['max_blocks'] = int(max_blocks)
        self.rows.setdefault(_key(row), dict(row, cases=[]))
        if case not in self.rows[_key(row)]['cases']:
            self.rows[_key(row)]['cases'].append(case)

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name == 'ph_gemm_bf16':
            def single(a, s):
                self._note('single', [a._obj], 1, 0, self.case)
                return fn(a, s)
            return single
        if name == 'ph_gemm_grouped_bf16':
            def grouped(arr, n, s):
                self._note('grouped', arr, n, 0, self.case)
                return fn(arr, n, s)
            return grouped
        if name == 'ph_gemm_grouped_capped_bf16':
            def capped(arr, n, mb, s):
                self._note('grouped', arr, n, mb, self.case)
                return fn(arr, n, mb, s)
            return capped
        return fn


def harvest(out, cases):
    import torch
    from prismer_amd import ops
    from tests import test_parity_gpu as P
    from tests.golden import cases as G
    h = _Harvest(ops.lib)
    ops.lib = h
    for name in cases:
        h.case = name
        tr, _ = P._pinned_trainer(G.Case(name), use_graph=False)
        for _ in range(2):
            tr.step()
        torch.cuda.synchronize()
        print(name, 'distinct calls so far:', len(h.rows), flush=True)
        del tr
        torch.cuda.empty_cache()
    json.dump(list(h.rows.values()), open(out, 'w'))


def record(step_json):
    rows, seen = [], set()
    for src in (hand_rows(), json.load(open(step_json))):
        for row in src:
            if _key(row) in seen:
                continue
            seen.add(_key(row))
            row.pop('expect', None)
            row['expect'] = route_of(row)
            rows.append(row)
    with open(TABLE, 'w') as f:
        f.write('[\n' + ',\n'.join(json.dumps(r, sort_keys=True, separators=(',', ':')) for r in rows) + '\n]\n')
    print(len(rows), 'rows,', os.path.getsize(TABLE), 'bytes')


def _rows_needed(d):
    """elements of A, B and rows of C a problem touches"""
    M, N, K = d['M'], d['N'], d['K']
    if 'conv' in d:
        cv = dict(zip(CONV, d['conv']))
        gathered = cv['B'] * cv['H'] * cv['W'] * cv['C']
    a = (K if d.get('trans_a') else M) * d['lda']
    b = (K if d.get('trans_b') else N) * d['ldb']
    if 'conv' in d and not d.get('trans_a'):
        a = gathered
    if 'conv' in d and d.get('trans_a'):
        b = gathered
    crows = M
    if d.get('rowmap_wo'):
        m = M - 1
        crows = m * d.get('rowmap_mul', 0) + d.get('rowmap_add', 0) + 1          # (rowmap_sub >= 0: the last row is an upper bound)
    return a, b, crows


def _atomic(row):
    """rows whose result depends on the order of float atomics: fused column sums, BatchNorm statistics, a k split without a workspace"""
    return any(p.get('a_colsum') or p.get('col_stats') for p in row['problems']) or \
        any(p['max_split'] > 1 and p['fold'] == 0 and p['cls'] in (0, 1) for p in row['expect']['part'])


def drive(out):
    """every row once; operands from a seeded generator (the same at every build), outputs kept for `compare`"""
    import torch
    from prismer_amd import _lib
    rows = json.load(open(TABLE))
    stream = torch.cuda.current_stream().cuda_stream
    ws = torch.empty(max([p.get('workspace', 0) for r in rows for p in r['problems']] + [4]) // 4, dtype=torch.float32, device='cuda')
    seed = torch.zeros(2, dtype=torch.int64, device='cuda')
    gen = torch.Generator(device='cuda')
    saved = []
    for ri, row in enumerate(rows):
        gen.manual_seed(1234 + ri)
        bufs = []

        def rnd(n, dtype, scale):
            t = (torch.randn(max(int(n), 8), device='cuda', generator=gen) * scale).to(dtype)
            bufs.append(t)
            return t

        outs = []
        per = []
        for d in row['problems']:
            a, b, crows = _rows_needed(d)
            f32 = bool(d.get('out_f32'))
            t = {'A': rnd(a, torch.bfloat16, 0.3), 'B': rnd(b, torch.bfloat16, 0.3),
                 'C': rnd(crows * d['ldc'], torch.float32 if f32 else torch.bfloat16, 1.0)}
            if d.get('bias'): t['bias'] = rnd(d['N'], torch.float32, 0.5)
            if d.get('pre_out'): t['pre_out'] = rnd(d['M'] * d['ldc'], torch.bfloat16, 1.0)
            if d.get('act_in'): t['act_in'] = rnd(d['M'] * d['ld_act'], torch.bfloat16, 1.0)
            if d.get('residual'): t['residual'] = rnd(d['M'] * d['ldr'], torch.float32 if d.get('residual_f32') else torch.bfloat16, 1.0)
            if d.get('col_stats'): t['col_stats'] = torch.zeros(8 * 2 * d['N'], dtype=torch.float64, device='cuda')
            if d.get('a_colsum'): t['a_colsum'] = torch.zeros(d['M'], dtype=torch.float32, device='cuda')
            t['drop_seed'], t['workspace'] = seed, ws
            per.append(t)
            outs += [t['C']] + [t[k] for k in ('pre_out', 'col_stats', 'a_colsum') if k in t]
        arr, keep = args_of(row, lambda d, k, i: per[i][k].data_ptr())
        with tuned(row):
            if row['entry'] == 'single':
                rc = _lib.lib.ph_gemm_bf16(C.byref(arr[0]), stream)
            else:
                rc = _lib.lib.ph_gemm_grouped_capped_bf16(arr, len(arr), row.get('max_blocks', 0), stream)
            rc2 = _lib.lib.ph_gemm_flush_deferred(stream)
        torch.cuda.synchronize()
        if rc or rc2:                # (kept and compared like an output: a rejected row must be rejected by both builds)
            print('row', ri, 'rejected:', rc, rc2, _lib.lib.ph_last_error().decode(), flush=True)
        # a digest per output (sum and sum of |x| in fp64, plus a strided sample) keeps the file small; `compare` wants them bit-equal
        saved.append([(float(rc), float(rc2), torch.zeros(1))] + [(o.double().sum().item(), o.double().abs().sum().item(), o.flatten()[::max(1, o.numel() // 4096)].cpu().clone()) for o in outs])
        atomic = _atomic(row)
        print('row', ri, row['entry'], len(row['problems']), 'problems', 'atomic' if atomic else '', flush=True)
    torch.save({'rows': [_key(r) for r in rows], 'atomic': [_key(r) for r in rows if _atomic(r)], 'out': saved}, out)


def compare(pa, pb):
    import torch
    a, b = torch.load(pa), torch.load(pb)
    assert a['rows'] == b['rows'], 'the two runs drove different tables'
    exact = loose = 0
    same = lambda u, v: u == v or (u != u and v != v)
    bits = lambda u, v: u.dtype == v.dtype and torch.equal(u.contiguous().view(torch.uint8), v.contiguous().view(torch.uint8))
    for key, ra, rb in zip(a['rows'], a['out'], b['out']):
        atomic = key in a['atomic']
        for (s0, s1, x), (t0, t1, y) in zip(ra, rb):
            if atomic and not (same(s0, t0) and same(s1, t1) and bits(x, y)):
                # float atomics: order-dependent rounding, held to the tighter bar of tests/test_wgrad_balanced_gpu.py (column sums 1e-4; dW 3e-4)
                e = ((x.double() - y.double()).norm() / (y.double().norm() + 1e-30)).item()
                assert e < 1e-4 and abs(s1 - t1) <= 1e-4 * abs(t1), (key, e)
                loose += 1
            else:
                assert same(s0, t0) and same(s1, t1) and bits(x, y), key
                exact += 1
    print(f'{len(a["rows"])} rows: {exact} outputs bit-identical, {loose} float-atomic outputs within 1e-4')


def step(case):
    import torch
    from tests import test_parity_gpu as P
    from tests.golden import cases as G
    tr, _ = P._pinned_trainer(G.Case(case), use_graph=False)
    for _ in range(2):
        tr.step()
    torch.cuda.synchronize()


def launches(db, out):
    import sqlite3
    cur = sqlite3.connect(db).cursor()
    cols = [d[0] for d in cur.execute('select * from kernels limit 1').description]
    lds = [c for c in cols if 'lds' in c.lower() or 'group_segment' in c.lower()]
    stream = [c for c in cols if c.lower() in ('stream_id', 'queue_id', 'stream', 'queue')][:1]
    dims = [c for c in ('grid_x', 'grid_y', 'grid_z', 'workgroup_x', 'workgroup_y', 'workgroup_z') if c in cols]
    q = f"select name, {', '.join(dims + lds + stream)} from kernels where name like '%gemm%' or name like '%splitk_reduce%' or name like '%zero_counters%' order by start"
    with open(out, 'w') as f:
        f.write('# columns: name | ' + ' '.join(dims + lds) + (' | ' + stream[0] if stream else '') + '\n')
        for r in cur.execute(q):
            body = ' '.join(str(v) for v in r[1:1 + len(dims) + len(lds)])
            f.write(f'{r[0]} | {body}' + (f' | {r[-1]}' if stream else '') + '\n')


def difflaunch(pa, pb):
    """identical in trace order; if kernels of different streams overlap the trace order is not the issue order: then per stream, and as a multiset"""
    import collections
    a, b = ([l.rstrip('\n') for l in open(p) if not l.startswith('#')] for p in (pa, pb))
    strip = lambda ls: [l.rsplit(' | ', 1)[0] if l.count(' | ') == 2 else l for l in ls]
    by_stream = lambda ls: {k: [x for x in strip([l for l in ls if l.rsplit(' | ', 1)[-1] == k])] for k in {l.rsplit(' | ', 1)[-1] for l in ls}} \
        if ls and ls[0].count(' | ') == 2 else {}
    sa, sb = by_stream(a), by_stream(b)
    print(f'{os.path.basename(pa)}: {len(a)} launches; {os.path.basename(pb)}: {len(b)} launches')
    print('identical in trace order:', strip(a) == strip(b))
    print('identical per stream (streams matched by their launch lists):', sorted(sa.values()) == sorted(sb.values()))
    ca, cb = collections.Counter(strip(a)), collections.Counter(strip(b))
    print('identical as a multiset:', ca == cb)
    for k in sorted((ca - cb) + (cb - ca)):
        print('  differs:', k, ca[k], cb[k])
    return strip(a) == strip(b) or (ca == cb and sorted(sa.values()) == sorted(sb.values()))


if __name__ == '__main__':
    cmd = sys.argv[1]
    if cmd == 'harvest':
        harvest(sys.argv[2], sys.argv[3:] or CASES)
    elif cmd == 'record':
        record(sys.argv[2])
    elif cmd == 'drive':
        drive(sys.argv[2])
    elif cmd == 'compare':
        compare(sys.argv[2], sys.argv[3])
    elif cmd == 'step':
        step(sys.argv[2])
    elif cmd == 'launches':
        launches(sys.argv[2], sys.argv[3])
    elif cmd == 'difflaunch':
        raise SystemExit(0 if difflaunch(sys.argv[2], sys.argv[3]) else 1)
    else:
        raise SystemExit(__doc__)
