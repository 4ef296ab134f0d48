"""The call layer's pin (tests/golden/ops_calls.json): what prismer_amd/ops.py hands the library for a fixed list of scenarios, recorded
on a machine without a device.  ops.lib is replaced by a recorder that answers 0 (ph_gemm_route, ph_query_workspace and
ph_layernorm_bwd_blocks are host-only and pass through), ops._stream and ops._workspace are patched, the operands are CPU tensors that
nothing reads.  tests/test_ops_calls_cpu.py asserts `check`, so a lost leading-dimension rule or pointer offset is a diff of that file.

  python tools/ops_calls.py record      write the table from this tree
  python tools/ops_calls.py check       compare this tree against the table (exit status 1 and the first differences when they differ)

A call = [entry point, arguments].  A structure is written with every field; an array of structures as the list of its items (= the item
count); a pointer as [scenario tensor, byte offset] -- 'ws0' / 'ws1' / 'ws2' are the workspace roles, 'ret<i>' the i-th tensor the
scenario returned, 'ln_arena' the queue's LayerNorm arena, '?' memory the op allocated and did not return -- or null; the stream as 'stream'."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
TABLE = os.path.join(ROOT, 'tests', 'golden', 'ops_calls.json')
STREAM = 0x5EA0
HOST_ONLY = ('ph_gemm_route', 'ph_query_workspace', 'ph_layernorm_bwd_blocks', 'ph_last_error')


class _Ptr(int):
    """an address waiting for the scenario's tensor registry"""


def _dump(v, ctype=None):
    """a ctypes value -> plain data, addresses as _Ptr"""
    if isinstance(v, C.Structure):
        return {name: _dump(getattr(v, name), t) for name, t in v._fields_}
    if isinstance(v, C.Array):
        return [_dump(x, v._type_) for x in v]
    if isinstance(v, C._Pointer):
        return _dump(v.contents) if v else None
    if ctype is C.c_void_p:
        return None if v is None else _Ptr(v)
    return v


class Recorder:
    """stands in for ops.lib: notes every call and answers 0"""

    def __init__(self, lib, sigs):
        self._lib, self._sigs, self.calls = lib, sigs, []

    def __getattr__(self, name):
        if name in HOST_ONLY:
            return getattr(self._lib, name)
        argtypes = self._sigs[name][1]

        def call(*args):
            assert len(args) == len(argtypes), name
            out = []
            for i, (a, t) in enumerate(zip(args, argtypes)):
                if i == len(args) - 1 and a == STREAM:
                    out.append('stream')
                elif isinstance(a, C.Array) and i + 1 < len(args) and isinstance(args[i + 1], int) and issubclass(a._type_, C.Structure):
                    out.append([_dump(a[j]) for j in range(args[i + 1])])                 # grouped entry point: the first n items
                elif hasattr(a, '_obj'):
                    out.append(_dump(a._obj))                                             # byref(struct)
                else:
                    out.append(_dump(a, t))
            self.calls.append([name, out])
            return 0
        return call


class Scene:
    """the tensors of one scenario by name; views of them resolve to (name, byte offset)"""

    def __init__(self):
        self.t = {}

    def new(self, name, *shape, dtype=None):
        import torch
        t = torch.empty(shape, dtype=dtype or torch.bfloat16)
        self.t[name] = t
        return t

    def f32(self, name, *shape):
        import torch
        return self.new(name, *shape, dtype=torch.float32)

    def resolve(self, v):
        if isinstance(v, _Ptr):
            for name, t in self.t.items():
                st = t.untyped_storage()
                if st.data_ptr() <= v < st.data_ptr() + max(st.nbytes(), 1):
                    return [name, int(v) - st.data_ptr()]
            return ['?', 0]
        if isinstance(v, dict):
            return {k: self.resolve(x) for k, x in v.items()}
        if isinstance(v, (list, tuple)):
            return [self.resolve(x) for x in v]
        return v


# ------------------------------------------------------------------------------------------------------------ scenarios
# each: fn(S, ops) -> the tensors ops returned (a list, entries may be None), or None.  Every tensor an op returns is in that list: memory freed
# inside a scenario could come back as a later tensor and be taken for it.

def _drops(S, ops):
    import torch
    seed = S.new('seed', 1, dtype=torch.int64)
    return {'none': None, 'p0': ops.Dropout(0.0, seed, 3), 'p': ops.Dropout(0.1, seed, 3)}


def gemm_epilogue(which):
    def run(S, ops):
        from prismer_amd._lib import ACT_GELU
        M, N, K = 24, 40, 32                                    # operands are column slices of wider buffers: every leading dimension != its width
        a, b, out = S.new('a', M, 64)[:, 8:8 + K], S.new('b', N, 72)[:, 16:16 + K], S.new('out', M, 56)[:, 8:8 + N]
        pre, res = S.new('pre', M, 56)[:, 8:8 + N], S.f32('res', M, 48)[:, :N]
        ops.gemm(a, b, out, bias=S.f32('bias', N), act=ACT_GELU, pre_out=pre, pre_grad=True, residual=res, drop=_drops(S, ops)[which], M=M, N=N, K=K)
    return run


def gemm_dgrad(S, ops):
    from prismer_amd._lib import ACT_SAVED_GRAD
    M, N, K = 24, 48, 40                                        # dx[M, N] = dy[M, K] . W[K, N], times the saved act' from a strided view
    return [ops.gemm(S.new('dy', M, K), S.new('w', K, N), trans_b=True, N=N, K=K, act=ACT_SAVED_GRAD, act_in=S.new('pre', M, 64)[:, 8:8 + N])]


def gemm_split(S, ops):
    return [ops.gemm(S.new('a', 16, 256), S.new('b', 24, 256), split_k=4, alpha=0.5)]


def gemm_conv(stride):
    def run(S, ops):
        B, H, Ci, Co = 2, 8, 16, 32                             # 3x3 on an 8x8x16 image: K = 144
        Ho = ops.conv_out_size(H, 3, stride)
        x, w, conv = S.new('x', B, H, H, Ci), S.new('w', Co, 9 * Ci), (B, H, H, Ci, 3, stride)
        y = S.new('y', B * Ho * Ho, Co)
        ops.gemm(x.view(-1, Ci), w, out=y, conv=conv, col_stats=S.new('sums', 8, 2, Co, dtype=__import__('torch').float64), M=B * Ho * Ho, N=Co, K=9 * Ci)
        return [ops.gemm(S.new('dy', B * Ho * Ho, Co), x.view(-1, Ci), trans_a=True, trans_b=True, out_f32=True, M=Co, N=9 * Ci, K=B * Ho * Ho,
                         conv=conv, defer_reduce=True)]
    return run


def _route_fold(ops, M, N, K, n):
    """does ph_gemm_route fold n queued (M, N, K) weight gradients inside the launch?"""
    from prismer_amd import _lib
    arr = (_lib.GemmArgs * n)()
    for g in arr:
        g.A = g.B = g.C = g.workspace = 4096
        g.M, g.N, g.K, g.lda, g.ldb, g.ldc, g.workspace_bytes = M, N, K, M, N, N, ops.WS_BYTES
        g.trans_a, g.trans_b, g.out_f32, g.accumulate, g.alpha = 1, 1, 1, 1, 1.0
    info = _lib.GemmRouteInfo()
    assert _lib.lib.ph_gemm_route(arr, n, 1, 0, C.byref(info)) == 0
    return info.part[0].fold == _lib.GEMM_FOLD_IN_LAUNCH


def wgrad_queue(S, ops):
    q = ops.WQ
    # 18 x (64, 32, 128): two launches (16 + 2) the route leaves whole -> issued without the workspace
    assert not _route_fold(ops, 64, 32, 128, 16) and not _route_fold(ops, 64, 32, 128, 2)
    gw = [S.f32(f'gw{i}', 64, 32) for i in range(18)]
    dy = [S.new(f'dy{i}', 128, 64) for i in range(18)]
    for i in range(18):
        q.add_gemm(dy[i], S.new(f'x{i}', 128, 32), gw[i], 64, 32, 128)
    q.exclusive = {gw[3].data_ptr()}                            # a single-writer output: overwritten, not accumulated
    # a second reduction length; two writers of one output never share a launch
    g2 = S.f32('g2', 64, 32)
    for i in range(2):
        q.add_gemm(S.new(f'ey{i}', 256, 64), S.new(f'ex{i}', 256, 32), g2, 64, 32, 256)
    # (512, 128, 8320) alone: cut and folded inside the launch -> keeps the workspace
    assert _route_fold(ops, 512, 128, 8320, 1)
    q.add_gemm(S.new('fy', 8320, 512), S.new('fx', 8320, 128), S.f32('fg', 512, 128), 512, 128, 8320)
    q.add_colsum(dy[0], S.f32('gb0', 64), 64)                   # rides with the first GEMM (a_colsum)
    q.add_colsum(S.new('lone', 50, 24), S.f32('gb1', 24), 24)   # no partner: ph_colsum_grouped_bf16
    q.add_conv_fold(S.f32('ds', 32, 144), S.f32('dw', 32, 16, 3, 3), 32, 16, 3, 144)
    q.flush()
    q.exclusive = None


def queue_lists(S, ops):
    """item lists one longer than their group maximum"""
    import torch
    q = ops.WQ
    M, D = 8, 16
    for i in range(17):
        ops.layernorm_bwd(S.new(f'dy{i}', M, D), S.new(f'x{i}', M, D), S.f32(f'mean{i}', M), S.f32(f'rstd{i}', M), S.f32(f'gamma{i}', D),
                          dgamma=S.f32(f'dgamma{i}', D), dbeta=S.f32(f'dbeta{i}', D), dx=S.new(f'dx{i}', M, D))
        q.add_colsum(S.new(f'c{i}', 10 + i, 24), S.f32(f'cb{i}', 24), 24)
    S.t['ln_arena'] = q.ln_arena
    q.flush()
    lay = [(S.f32(f'w{i}', 8, 4, 3, 3), S.new(f's{i}', 8, 40), 8, 4, 3, 40) for i in range(33)]
    ops.conv_layout_grouped(lay, True)
    ops.conv_layout_grouped([(S.f32(f'ds{i}', 8, 40), w, 8, 4, 3, 40) for i, (w, *_) in enumerate(lay)], False)
    ops.conv_dgrad_shadows([(w, S.new(f'wd{i}', 4, 72), 8, 4, 1 + i % 2) for i, (w, *_) in enumerate(lay)])
    bn = [dict(y=S.new(f'y{i}', 6, 8), a=S.new(f'a{i}', 6, 8), gamma=S.f32(f'g{i}', 8), beta=S.f32(f'b{i}', 8), running_mean=S.f32(f'rm{i}', 8),
               running_var=S.f32(f'rv{i}', 8), stats=S.f32(f'st{i}', 4, 8), sums=S.new(f'sm{i}', 8, 2, 8, dtype=torch.float64)) for i in range(9)]
    ops.bn_apply_relu_grouped(bn, True, 0.1, 1e-5)
    ops.bn_relu_bwd_grouped([dict(y=d['y'], a=d['a'], dy=S.new(f'bdy{i}', 6, 8), gamma=d['gamma'], beta=d['beta'], stats=d['stats'],
                                  sums=S.f32(f'bs{i}', 2, 8), dgamma=S.f32(f'dg{i}', 8), dbeta=(S.f32(f'db{i}', 8) if i % 2 else None))
                             for i, d in enumerate(bn)])


def conv_fwd_grouped(S, ops):
    import torch
    items = []
    for i in range(17):
        stride = 1 + i % 2
        Ho = ops.conv_out_size(8, 3, stride)
        items.append((S.new(f'x{i}', 2, 8, 8, 16), (2, 8, 8, 16, 3, stride), S.new(f'w{i}', 32, 144), S.new(f'y{i}', 2 * Ho * Ho, 32),
                      S.new(f'sums{i}', 8, 2, 32, dtype=torch.float64) if i % 3 else None))
    ops.conv_fwd_grouped(items)


def gemm_grouped_tb(S, ops):
    ops.gemm_grouped([(S.new(f'a{i}', 8 + i, 24), S.new(f'b{i}', 24, 16), S.new(f'o{i}', 8 + i, 16), 8 + i, 16, 24) for i in range(17)], trans_b=True)


def conv_dgrad(S, ops):
    B, H, Ci, Co = 2, 8, 16, 32
    items = []
    for i, stride in enumerate((1, 2)):
        Ho = H // stride
        items.append((S.new(f'dy{i}', B * Ho * Ho, Co), S.new(f'wd{i}', Ci, 9 * Co), S.new(f'dx{i}', B * H * H, Ci), (B, H, H, Ci, Co, stride)))
    ops.conv_dgrad_grouped(items)


def wgrad_split(S, ops):
    items = []
    for i in range(4):                                          # conv and plain items interleaved: the returned order is the items'
        Co = 32 + 8 * i
        if i % 2 == 0:
            items.append((S.new(f'dy{i}', 2 * 64, Co), S.new(f'x{i}', 2 * 64, 16), Co, 144, 2 * 64, (2, 8, 8, 16, 3, 1)))
        else:
            items.append((S.new(f'dy{i}', 96, Co), S.new(f'x{i}', 96, 40), Co, 40, 96, None))
    return ops.wgrad_split_grouped(items)


def _stem_items(S, ops, spec):
    """spec as tests/test_stem_wgrad_route_cpu.py: [(Cout, (B, H, W, C, ks, stride))]; the tensors are never touched, only their addresses"""
    items = []
    for i, (Co, cv) in enumerate(spec):
        B, H, W, Cc, ks, stride = cv
        K = B * ops.conv_out_size(H, ks, stride) ** 2
        items.append((S.new(f'dy{i}', K, Co), S.new(f'x{i}', B * H * W, Cc), Co, ks * ks * Cc, K, cv))
    return items


def wgrad_persistent_taken(S, ops):
    # layer 3 of the headline's stems: cut and folded in the launch
    return ops.conv_wgrad_persistent(_stem_items(S, ops, [(384, (32, 56, 56, 192, 3, 2))] * 3 + [(384, (32, 14, 14, 192, 3, 1))] * 3))


def wgrad_persistent_refused(S, ops):
    # first label layer: stays on the register-staged split; and a reduction that is no multiple of 64 pixels
    a = ops.conv_wgrad_persistent(_stem_items(S, ops, [(96, (32, 56, 56, 64, 3, 2))] * 3))
    b = ops.conv_wgrad_persistent(_stem_items(S, ops, [(768, (32, 28, 28, 384, 3, 2))] * 2 + [(768, (31, 14, 14, 384, 3, 1))]))
    return [a, b]


def attention(which):
    def run(S, ops):
        B, H, Sq, Sk, dh = 2, 2, 5, 7, 8
        W = H * dh
        q, kv = S.new('q', B * Sq, W), S.new('kv', B * Sk, 2 * W)
        mask = S.new('mask', B, Sk, dtype=__import__('torch').uint8)
        st = dict(q_strides=(Sq * W, W), k_strides=(Sk * 2 * W, 2 * W), v_strides=(Sk * 2 * W, 2 * W))
        drop = _drops(S, ops)[which]
        o, lse = ops.attention_fwd(q, kv[:, :W], kv[:, W:], B, H, Sq, Sk, dh, key_mask=mask, causal=True, drop=drop, **st)
        S.t['o'], S.t['lse'] = o, lse
        dq, dkv = S.new('dq', B * Sq, W), S.new('dkv', B * Sk, 2 * W)
        ops.attention_bwd(S.new('do', B * Sq, W), q, kv[:, :W], kv[:, W:], o, lse, B, H, Sq, Sk, dh, dq=dq, dk=dkv[:, :W], dv=dkv[:, W:],
                          dq_strides=st['q_strides'], dk_strides=st['k_strides'], dv_strides=st['v_strides'], key_mask=mask, causal=True, drop=drop, **st)
    return run


def layernorm_bwd(which):
    def run(S, ops):
        M, D = 8, 16
        ops.WQ.enabled = False                                  # the reduction inside the call: the per-call workspace
        try:
            return list(ops.layernorm_bwd(S.new('dy', M, D), S.f32('x', M, D), S.f32('mean', M), S.f32('rstd', M), S.f32('gamma', D),
                                          dskip=S.new('dskip', M, D), dgamma=S.f32('dgamma', D), dbeta=S.f32('dbeta', D), drop=_drops(S, ops)[which]))
        finally:
            ops.WQ.enabled = True
    return run


def embed(which):
    def run(S, ops):
        import torch
        B, T, H, V = 2, 6, 16, 50
        ids = S.new('ids', B, T, dtype=torch.int64)
        word, pos, typ, gamma, beta = S.f32('word', V, H), S.f32('pos', 32, H), S.f32('typ', 1, H), S.f32('gamma', H), S.f32('beta', H)
        drop = _drops(S, ops)[which]
        out, xhat, rstd, o32 = ops.embed_fwd(ids, word, pos, typ, gamma, beta, 1e-5, 1, drop=drop, want_f32=True)
        second = ops.embed_fwd(ids, word, pos, typ, gamma, beta, 1e-5, 1, drop=drop, pos_base=S.new('pos_base', B, dtype=torch.int32))
        ops.embed_bwd(S.new('dout', B * T, H), ids, word, pos, typ, gamma, beta, 1e-5, 1, xhat, rstd, drop, S.f32('dword', V, H), S.f32('dpos', 32, H),
                      None, S.f32('dgamma', H), S.f32('dbeta', H))
        return [out, xhat, rstd, o32, *second]
    return run


def scenarios():
    sc = [(f'gemm epilogue, drop {w}', gemm_epilogue(w)) for w in ('none', 'p0', 'p')]
    sc += [('gemm dgrad', gemm_dgrad), ('gemm split_k', gemm_split), ('gemm conv stride 1', gemm_conv(1)), ('gemm conv stride 2', gemm_conv(2)),
           ('weight-gradient queue', wgrad_queue), ('lists one longer than the group maximum', queue_lists), ('conv_fwd_grouped', conv_fwd_grouped),
           ('gemm_grouped trans_b', gemm_grouped_tb), ('conv_dgrad_grouped', conv_dgrad), ('wgrad_split_grouped', wgrad_split),
           ('conv_wgrad_persistent taken', wgrad_persistent_taken), ('conv_wgrad_persistent refused', wgrad_persistent_refused)]
    for w in ('none', 'p'):
        sc += [(f'attention, drop {w}', attention(w)), (f'layernorm_bwd, drop {w}', layernorm_bwd(w)), (f'embed, drop {w}', embed(w))]
    return sc


def run_all():
    """-> {scenario: {'calls': [...], 'returns': [...]}} from this tree's prismer_amd.ops"""
    import torch
    from prismer_amd import _lib, ops
    saved = ops.lib, ops._stream, ops._workspace, ops.WQ
    ws = {}

    def workspace(device, which=0):
        if which not in ws:
            ws[which] = torch.empty(ops.WS_BYTES // 4, dtype=torch.float32)                 # (never touched: no page is committed)
        return ws[which]
    out = {}
    try:
        ops._stream, ops._workspace = (lambda: STREAM), workspace
        for name, fn in scenarios():
            rec = ops.lib = Recorder(_lib.lib, _lib._SIGS)
            ops.WQ = ops.WgradQueue()
            S = Scene()
            ret = fn(S, ops)
            for i, t in enumerate(ret or []):
                if t is not None:
                    S.t[f'ret{i}'] = t
            S.t.update({f'ws{k}': t for k, t in ws.items()})
            out[name] = {'calls': S.resolve(rec.calls),
                         'returns': None if ret is None else [None if t is None else [str(t.dtype).split('.')[-1]] + list(t.shape) for t in ret]}
    finally:
        ops.lib, ops._stream, ops._workspace, ops.WQ = saved
    return out


def _plain(x):
    return json.loads(json.dumps(x))


def record():
    got = _plain(run_all())
    with open(TABLE, 'w') as f:
        f.write('{\n' + ',\n'.join(json.dumps(k) + ':' + json.dumps(v, sort_keys=True, separators=(',', ':')) for k, v in got.items()) + '\n}\n')
    print(len(got), 'scenarios,', sum(len(v['calls']) for v in got.values()), 'calls,', os.path.getsize(TABLE), 'bytes')


def _diff(a, b, path, out):
    if len(out) >= 20:
        return
    if isinstance(a, dict) and isinstance(b, dict):
        for k in sorted(set(a) | set(b)):
            _diff(a.get(k, '<absent>'), b.get(k, '<absent>'), f'{path}.{k}', out)
    elif isinstance(a, list) and isinstance(b, list) and len(a) == len(b):
        for i, (x, y) in enumerate(zip(a, b)):
            _diff(x, y, f'{path}[{i}]', out)
    elif a != b:
        out.append(f'{path}: table {json.dumps(a)[:200]} != tree {json.dumps(b)[:200]}')


def check():
    """-> list of differences between the table and this tree (empty: the same calls)"""
    want, got, out = json.load(open(TABLE)), _plain(run_all()), []
    _diff(want, got, '', out)
    return out


if __name__ == '__main__':
    cmd = sys.argv[1] if len(sys.argv) > 1 else ''
    if cmd == 'record':
        record()
    elif cmd == 'check':
        d = check()
        print('\n'.join(d) if d else 'ops calls: identical to the table')
        raise SystemExit(1 if d else 0)
    else:
        raise SystemExit(__doc__)
