"""Tensor-level wrappers over the C ABI (prismer_amd/_lib.py).  torch supplies device memory and the current
HIP stream; every arithmetic step runs in libprismer_hip.so.  No fallbacks: a missing library fails at import.
"""
import ctypes as C
import os
import struct

import torch

from . import _lib
from ._lib import (ACT_GELU, ACT_NONE, ACT_QUICKGELU, ACT_RELU, ACT_RELU2, ACT_SAVED_GRAD, IDENT, RowMap, check, lib, ptr)

BF16 = torch.bfloat16
F32 = torch.float32


_raw_stream, _cur_device = torch._C._cuda_getCurrentRawStream, torch._C._cuda_getDevice


def _stream():
    """the current HIP stream's handle (what torch.cuda.current_stream().cuda_stream returns, without building the Stream object: the
    eager drop-in step asks ~2000 times and is bound by host time, not by the GPU)"""
    return _raw_stream(_cur_device())


class Dropout:
    """Dropout descriptor: probability, device seed tensor (uint64 viewed as int64[1]) and a per-call-site stream id."""
    __slots__ = ('p', 'seed', 'stream')

    def __init__(self, p, seed, stream):
        self.p, self.seed, self.stream = float(p), seed, int(stream)


NO_DROP = None

_WS = {}
WS_BYTES = 256 << 20


# roles of the three fp32 scratch buffers a (device, stream) owns
WS_CALL, WS_DEFERRED, WS_STEM_WGRAD = 0, 1, 2


def _workspace(device, role=WS_CALL):
    """per-(device, stream, role) fp32 scratch, allocated once and reused by every launch on that stream.  Kernels on one stream are serialised,
    so a buffer is race-free as long as nothing parks data in it across launches; the roles keep apart what does:
      WS_CALL        split-K partial tiles / LayerNorm partials of a single call (gemm, layernorm_bwd): written and folded inside the call, so the
                     next call on the stream may reuse it
      WS_DEFERRED    partial sums that OUTLIVE their call: gemm(defer_reduce=True) parks them until gemm_flush_deferred(); also the grouped
                     launches of the weight-gradient queue and of wgrad_split_grouped, which fold inside the launch or in a pass issued right
                     behind it and park nothing -- on the main stream they may share the buffer with deferred folds only because no caller puts
                     one between a deferred call and its flush (the stems flush per layer); the queue normally runs on the side stream, i.e. on
                     that stream's own buffer
      WS_STEM_WGRAD  counters and slabs of the stems' persistent launch (conv_wgrad_persistent): issued on the main stream while the deferred
                     split-K calls of the same layer (first dense layer) have partial sums parked in this stream's WS_DEFERRED and whatever
                     split-K / LayerNorm call comes next takes WS_CALL.  Consecutive layers share it: launches on one stream run one after the
                     other and the counters are zeroed on the stream ahead of every launch"""
    key = (device, _raw_stream(device.index if device.index is not None else _cur_device()), role)
    ws = _WS.get(key)
    if ws is None:
        ws = torch.empty(WS_BYTES // 4, dtype=F32, device=device)
        _WS[key] = ws
    return ws


def _set_drop(s, drop):
    """the dropout triple of an argument structure (zero-initialised = no dropout); True when dropout is on"""
    if drop is None or drop.p <= 0.0:
        return False
    s.drop_p, s.drop_seed, s.drop_stream = drop.p, drop.seed.data_ptr(), drop.stream
    return True


def launch_grouped(entry, array_type, items, fill, group_max=_lib.GEMM_GROUP_MAX, what='', cut=None):
    """items in launches of at most group_max: per launch one ctypes array, fill(arr, j, item) writes element j (what it returns stays referenced
    until the launch is issued), entry(arr, n, stream) issues it.  cut(i0, i1) -> the end (<= i1) of the launch that starts at item i0, for a
    grouping rule beyond the maximum."""
    i0 = 0
    while i0 < len(items):
        i1 = min(i0 + group_max, len(items))
        if cut is not None:
            i1 = cut(i0, i1)
        arr = (array_type * (i1 - i0))()
        keep = [fill(arr, j, items[i]) for j, i in enumerate(range(i0, i1))]     # noqa: F841 -- alive across the call below
        check(entry(arr, i1 - i0, _stream()), what)
        i0 = i1


class SideStream:
    """Second HIP stream for work that is OFF the critical path of the backward pass (weight-gradient GEMMs, bias column
    sums): the dgrad chain keeps the main stream, the side stream fills the CUs its short / narrow launches leave idle.
    Under hipGraph capture the fork/join events become graph edges, i.e. parallel branches.  Tensors touched on the side
    stream are kept referenced until join() so the caching allocator cannot recycle them under the side stream's feet."""

    def __init__(self, device):
        self.stream = torch.cuda.Stream(device=device)
        self.keep = []
        self.dirty = False

    def run(self, fn, *tensors):
        main = torch.cuda.current_stream()
        ev = torch.cuda.Event()
        ev.record(main)
        self.stream.wait_event(ev)
        with torch.cuda.stream(self.stream):
            out = fn()
        self.keep.append(tensors)
        if out is not None:
            self.keep.append(out)
        self.dirty = True
        return out

    def wait(self):
        """current stream waits for everything queued on the side stream so far; keeps the tensor references (used inside
        micro-batch branches, where another branch's side work may still be pending)."""
        torch.cuda.current_stream().wait_stream(self.stream)

    def join(self):
        if self.dirty:
            torch.cuda.current_stream().wait_stream(self.stream)
            self.dirty = False
        self.keep.clear()


class BranchPool:
    """N extra HIP streams for INDEPENDENT sub-graphs (the six expert stems): each branch forks from the current stream,
    runs on its own stream (parallel branches of the hipGraph) and join() makes the current stream wait for all of them.
    Tensors created inside a branch must stay referenced until join() (the callers keep them in their saved state)."""

    def __init__(self, device, n):
        self.streams = [torch.cuda.Stream(device=device) for _ in range(n)]
        self.used = set()

    def branch(self, i):
        s = self.streams[i % len(self.streams)]
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        s.wait_event(ev)
        self.used.add(s)
        return torch.cuda.stream(s)

    def join(self):
        cur = torch.cuda.current_stream()
        for s in self.used:
            cur.wait_stream(s)
        self.used.clear()


class _NoPool:
    def branch(self, i):
        import contextlib
        return contextlib.nullcontext()

    def join(self):
        pass


POOL = _NoPool()     # set by the Trainer (native path)
MICRO = _NoPool()    # set by the Trainer: one stream per micro-batch (independent halves of the batch as parallel branches)
SIDE = None          # set by the Trainer (native path); None = everything on the current stream


def off_critical_path(fn, *tensors):
    """run fn() on the side stream when one is active, else inline."""
    if SIDE is None:
        return fn()
    return SIDE.run(fn, *tensors)


class WgradQueue:
    """Deferred weight gradients.  Nothing inside a step reads dW / db before the optimizer, so the wgrad GEMMs
    (dW += dY^T X: outputs of 18..144 tiles, alone they fill a fraction of the chip and need split-K + a reduce pass) and
    the bias column sums are queued and issued per reduction length K as ONE grouped launch each
    (ph_gemm_grouped_bf16 / ph_colsum_grouped_bf16).  At flush() a queued column sum whose dy is the [K][M] operand of a queued GEMM rides
    with that GEMM (ph_gemm_args.a_colsum: the sums are taken from the fragments the GEMM holds, dy is not read a second time); only the
    entries without a partner go through ph_colsum_grouped_bf16.  join_side() flushes, so every existing synchronisation point of the
    programs still sees complete gradients.  Operand tensors stay referenced until their launch."""

    def __init__(self):
        self.enabled = True
        self.gemms = {}          # K -> [(dy, x, gw, M, N, K)] (flush() appends the paired bias gradient, or None, as a 7th element)
        self.cols = []           # [(dy, gb, M, N)]
        self.folds = []          # [(dshadow, dw, Cout, Cin, ks, Kp)]  conv weight gradients: shadow layout -> parameter layout
        self.lns = []            # [(partials, blocks, D, dgamma, dbeta)]  LayerNorm gamma / beta partial sums
        self.ln_arena = None     # fp32 scratch the deferred LayerNorm backwards write their per-block partials into
        self.ln_off = 0
        self.ln_stream = None
        # first-writer bookkeeping of a native training step (Trainer._wq_scope): `counts` (while not None) tallies the writes per
        # output address of one whole step; `exclusive` = addresses written exactly once per step -> their GEMM overwrites
        self.counts = None
        self.exclusive = None

    def add_gemm(self, dy, x, gw, M, N, K):
        """gw[M, N] (fp32) += dy[K, M]^T . x[K, N]"""
        if self.counts is not None:
            key = gw.data_ptr()
            c = self.counts.get(key, (0, 0, True))
            self.counts[key] = (c[0] + 1, M * N, c[2] and gw.is_contiguous() and self.enabled)
        if not self.enabled:
            gemm(dy, x, out=gw, trans_a=True, trans_b=True, out_f32=True, accumulate=True, M=M, N=N, K=K)
            return
        self.gemms.setdefault(K, []).append((dy, x, gw, M, N, K))  # (two writers of one output never share a launch: _flush_gemms)

    def add_colsum(self, dy, gb, N):
        if not self.enabled:
            colsum(dy, gb, N=N)
            return
        self.cols.append((dy, gb, dy.shape[0], N))

    def add_conv_fold(self, ds, dw, Cout, Cin, ks, Kp):
        """dw[Cout, Cin, ks, ks] += ds[Cout, Kp] (im2col column order): queued behind the GEMM that produces ds on the
        side stream; all layers of a step fold in one launch"""
        if not self.enabled:
            conv_grad_from_shadow(ds, dw, Cout, Cin, ks, Kp)
            return
        self.folds.append((ds, dw, Cout, Cin, ks, Kp))

    LN_ARENA_FLOATS = 48 << 20          # 192 MB: one pass of the decoder (~80 MB) or the encoder (~110 MB) at bs32

    def ln_slot(self, blocks, D, dgamma, dbeta):
        """partials buffer [blocks, 2, D] for one LayerNorm backward whose gamma / beta reduction is deferred; None = do not
        defer (queue off, arena full, or a stream other than the one the pending partials were written on)"""
        if not self.enabled:
            return None
        cur = _stream()
        if self.lns and self.ln_stream != cur:
            return None
        n = blocks * 2 * D
        if self.ln_arena is None:
            self.ln_arena = torch.empty(self.LN_ARENA_FLOATS, dtype=F32, device=dgamma.device if dgamma is not None else dbeta.device)
        if self.ln_off + n > self.ln_arena.numel():
            self._flush_lns()           # same stream as the writers: the fold finishes before the arena is reused
        if n > self.ln_arena.numel():
            return None
        self.ln_stream = cur
        slot = self.ln_arena[self.ln_off:self.ln_off + n]
        self.ln_off += n
        self.lns.append((slot, blocks, D, dgamma, dbeta))
        return slot

    def _flush_lns(self):
        q, self.lns, self.ln_off = self.lns, [], 0

        def fill(arr, j, e):
            it, (ws, blocks, D, dg, db) = arr[j], e
            it.ws, it.blocks, it.D, it.dgamma, it.dbeta = ws.data_ptr(), blocks, D, ptr(dg), ptr(db)
        launch_grouped(lib.ph_ln_param_reduce_grouped, _lib.LnReduceItem, q, fill, what='ph_ln_param_reduce_grouped')

    def _flush_gemms(self, K):
        allq = self.gemms.pop(K, [])
        if not allq:
            return
        excl = self.exclusive

        def cut(i0, i1):                             # no output twice in one launch
            seen = set()
            for i in range(i0, i1):
                if allq[i][2].data_ptr() in seen:
                    return i
                seen.add(allq[i][2].data_ptr())
            return i1

        def entry(arr, n, stream):
            # the workspace is for the persistent kernel's k-balanced plan only (partial tiles folded inside the launch); a group
            # that plan leaves whole is issued without one, as before
            info = _lib.GemmRouteInfo()
            if lib.ph_gemm_route(arr, n, 1, 0, C.byref(info)) != 0 or info.part[0].fold != _lib.GEMM_FOLD_IN_LAUNCH:
                gemm_args_drop_workspace(arr)
            return lib.ph_gemm_grouped_capped_bf16(arr, n, 0, stream)

        def work():
            ws = _workspace(allq[0][0].device, WS_DEFERRED)

            def fill(arr, j, e):
                dy, x, gw, M, N, Kk, *gb = e
                # single-writer outputs of the native step are OVERWRITTEN (no read of the zeroed buffer, and AdamW does not
                # have to zero it): self.exclusive is set by the Trainer for the duration of its own step only
                gemm_args(dy, x, gw, M, N, Kk, trans_a=True, trans_b=True, out_f32=True, a_colsum=gb[0] if gb else None,
                          accumulate=excl is None or gw.data_ptr() not in excl, workspace=ws, into=arr[j])
            launch_grouped(entry, _lib.GemmArgs, allq, fill, what='ph_gemm_grouped_capped_bf16', cut=cut)
        off_critical_path(work, *[t for e in allq for t in e[:3]], *[e[6] for e in allq if len(e) > 6 and e[6] is not None])

    def _pair_cols(self):
        """column sums that can ride with a queued GEMM: same dy (address, row stride), rows = the GEMM's K, columns = its M.  Each cols entry
        goes to ONE GEMM (the first free one that reads its dy), so a dy shared by two GEMMs is still summed once."""
        if not self.cols or not self.gemms:
            return
        free = {}
        for K, q in self.gemms.items():
            for i, e in enumerate(q):
                if len(e) == 6:
                    free.setdefault((e[0].data_ptr(), e[0].stride(0), K, e[3]), []).append((K, i))
        rest = []
        for dy, gb, rows, N in self.cols:
            slot = free.get((dy.data_ptr(), dy.stride(0), rows, N))
            if slot and dy.dtype == BF16 and gb.dtype == F32 and gb.is_contiguous():
                K, i = slot.pop(0)
                self.gemms[K][i] = self.gemms[K][i] + (gb,)
            else:
                rest.append((dy, gb, rows, N))
        self.cols = rest

    def _flush_cols(self):
        allq, self.cols = self.cols, []
        if not allq:
            return

        def fill(arr, j, e):
            it, (dy, gb, M, N) = arr[j], e
            it.x, it.out, it.M, it.N, it.ld = dy.data_ptr(), gb.data_ptr(), M, N, dy.stride(0)

        def work():
            launch_grouped(lib.ph_colsum_grouped_bf16, _lib.ColsumItem, allq, fill, what='ph_colsum_grouped_bf16')
        off_critical_path(work, *[t for e in allq for t in e[:2]])

    def flush(self):
        self._pair_cols()
        for K in list(self.gemms):
            self._flush_gemms(K)
        self._flush_cols()
        if self.lns:
            self._flush_lns()
        if self.folds:
            q, self.folds = self.folds, []
            off_critical_path(lambda: conv_layout_grouped(q, False), *[t for e in q for t in e[:2]])


WQ = WgradQueue()


def join_side():
    WQ.flush()
    if SIDE is not None:
        SIDE.join()


def wait_side():
    if SIDE is not None:
        SIDE.wait()


def gemm_args(a, b, out, M, N, K, *, trans_a=False, trans_b=False, bias=None, act=ACT_NONE, pre_out=None, pre_grad=False, act_in=None,
              residual=None, drop=None, out_f32=False, accumulate=False, alpha=1.0, split_k=0, conv=None, col_stats=None, a_colsum=None,
              b_offset=0, rowmap=None, workspace=None, defer_reduce=False, into=None):
    """The ph_gemm_args of out[M,N] = epi(alpha * opA . opB^T), a: [M,K] (or [K,M] if trans_a), b: [N,K] (or [K,N] if trans_b) -- the one place
    that writes the structure; launches nothing.  Returns (args, keep-alive: what the structure points to besides the tensors passed in).
    conv: the ConvGather integers, (B, H, W, C, ks, stride) or all twelve -- the A (forward, dgrad) / B (wgrad: trans_a) operand is an im2col
          view of an NHWC activation; the gathered side's leading dimension is the width of that view
    b_offset: bytes added to b's address (a tap range of the dgrad shadow);  rowmap: (wo, mul, sub, add) output-row scatter of a dgrad class
    workspace: fp32 tensor for split-K partial tiles / the k-balanced plan, or None
    into: a zero-initialised element of a group's array to fill instead of a fresh structure
    Only the fields that differ from the zero-initialised structure are written (the eager step is bound by host time)."""
    g = _lib.GemmArgs() if into is None else into
    g.A, g.B, g.C = a.data_ptr(), b.data_ptr() + b_offset, out.data_ptr()
    g.M, g.N, g.K = M, N, K
    g.lda, g.ldb, g.ldc = a.stride(0), b.stride(0), out.stride(0)
    g.alpha = alpha
    if trans_a:
        g.trans_a = 1
    if trans_b:
        g.trans_b = 1
    cg = None
    if conv is not None:
        cg = _lib.ConvGather(*conv)
        g.conv = C.pointer(cg)
        if trans_a:
            g.ldb = N
        else:
            g.lda = K
    if col_stats is not None:
        g.col_stats = col_stats.data_ptr()
    if a_colsum is not None:
        g.a_colsum = a_colsum.data_ptr()
    if bias is not None:
        g.bias = bias.data_ptr()
    if act:
        g.act = act
    if pre_out is not None:
        g.pre_out = pre_out.data_ptr()
    if pre_grad:
        g.pre_grad = 1
    if act_in is not None:
        g.act_in, g.ld_act = act_in.data_ptr(), act_in.stride(0)
    if residual is not None:
        g.residual, g.ldr, g.residual_f32 = residual.data_ptr(), residual.stride(0), int(residual.dtype == F32)
    if drop is not None:
        _set_drop(g, drop)
    if out_f32:
        g.out_f32 = 1
    if accumulate:
        g.accumulate = 1
    if split_k:
        g.split_k = split_k
    if rowmap is not None:
        g.rowmap_wo, g.rowmap_mul, g.rowmap_sub, g.rowmap_add = rowmap
    if workspace is not None:
        g.workspace, g.workspace_bytes = workspace.data_ptr(), workspace.numel() * 4
    if defer_reduce:
        g.defer_reduce = 1
    return g, cg


def gemm_args_drop_workspace(arr):
    """gemm_args' one companion: a built group is issued without its workspace after all (the route can only be asked about built arguments)"""
    for g in arr:
        g.workspace, g.workspace_bytes = None, 0


def gemm(a, b, out=None, *, trans_a=False, trans_b=False, out_f32=False, M=None, N=None, K=None, defer_reduce=False, **epilogue):
    """out[M,N] = epi(alpha * opA . opB^T).  a: [M,K] (or [K,M] if trans_a), b: [N,K] (or [K,N] if trans_b); epilogue: gemm_args' keywords.
    defer_reduce: a split-K call leaves its fold pass to gemm_flush_deferred() (one grouped launch for up to 16 of them); the partial sums of
    the queued calls are parked in WS_DEFERRED."""
    if M is None:
        M = a.shape[1] if trans_a else a.shape[0]
    if K is None:
        K = a.shape[0] if trans_a else a.shape[1]
    if N is None:
        N = b.shape[1] if trans_b else b.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=F32 if out_f32 else BF16, device=a.device)
    g, keep = gemm_args(a, b, out, M, N, K, trans_a=trans_a, trans_b=trans_b, out_f32=out_f32, defer_reduce=defer_reduce,
                        workspace=_workspace(a.device, WS_DEFERRED if defer_reduce else WS_CALL), **epilogue)
    check(lib.ph_gemm_bf16(C.byref(g), _stream()), 'ph_gemm_bf16')
    return out


def gemm_flush_deferred():
    check(lib.ph_gemm_flush_deferred(_stream()), 'ph_gemm_flush_deferred')


def layernorm_fwd(x, gamma, beta, eps=1e-5, out=None, out_map=IDENT, out2=None, out2_map=IDENT, save_stats=True, out_f32=None):
    """x: bf16 or fp32 [M, D]; out: bf16; out_f32: optional fp32 [M, D] copy of the output (fp32 residual stream)."""
    M, D = x.shape
    if out is None:
        out = torch.empty((M, D), dtype=BF16, device=x.device)
    mean = rstd = None
    if save_stats:
        stats = torch.empty((2, M), dtype=F32, device=x.device)
        mean, rstd = stats[0], stats[1]
    a = _lib.LayerNormFwdArgs(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), out_map, ptr(out2), out2_map,
                              ptr(mean), ptr(rstd), M, D, eps, int(x.dtype == F32), ptr(out_f32))
    check(lib.ph_layernorm_fwd(C.byref(a), _stream()), 'ph_layernorm_fwd')
    return out, mean, rstd


def layernorm_bwd(dy, x, mean, rstd, gamma, *, dy_map=IDENT, dy2=None, dy2_map=IDENT, dskip=None, dgamma=None, dbeta=None,
                  drop=None, dx=None, dx_drop=None):
    M, D = x.shape
    if dx is None:
        dx = torch.empty((M, D), dtype=BF16, device=x.device)
    a = _lib.LayerNormBwdArgs()
    a.x_f32 = int(x.dtype == F32)
    a.dy, a.dy_map, a.dy2, a.dy2_map = dy.data_ptr(), dy_map, ptr(dy2), dy2_map
    a.x, a.mean, a.rstd, a.gamma = x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr()
    a.dskip, a.dx = ptr(dskip), dx.data_ptr()
    if _set_drop(a, drop):
        if dx_drop is None:
            dx_drop = torch.empty((M, D), dtype=BF16, device=x.device)
        a.dx_drop = dx_drop.data_ptr()
    else:
        dx_drop = None
    a.dgamma, a.dbeta, a.M, a.D = ptr(dgamma), ptr(dbeta), M, D
    slot = None
    if dgamma is not None or dbeta is not None:
        slot = WQ.ln_slot(lib.ph_layernorm_bwd_blocks(M), D, dgamma, dbeta)     # gamma / beta reduction deferred and grouped
    if slot is not None:
        a.partial_ws, a.partial_ws_bytes, a.defer_reduce = slot.data_ptr(), slot.numel() * 4, 1
    else:
        ws = _workspace(x.device)
        a.partial_ws, a.partial_ws_bytes, a.defer_reduce = ws.data_ptr(), WS_BYTES, 0
    check(lib.ph_layernorm_bwd(C.byref(a), _stream()), 'ph_layernorm_bwd')
    return dx, (dx_drop if dx_drop is not None else dx)


def _attn_args(q, k, v, o, B, H, Sq, Sk, dh, strides, scale, key_mask, causal, drop, lse):
    f = _lib.AttnFwdArgs()
    f.q, f.k, f.v, f.o = q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr()
    (f.q_bs, f.q_ts), (f.k_bs, f.k_ts), (f.v_bs, f.v_ts), (f.o_bs, f.o_ts) = strides
    f.B, f.H, f.Sq, f.Sk, f.dh = B, H, Sq, Sk, dh
    f.scale = scale
    f.key_mask = ptr(key_mask)
    f.causal = int(causal)
    _set_drop(f, drop)
    f.lse = ptr(lse)
    return f


def attention_fwd(q, k, v, B, H, Sq, Sk, dh, *, q_strides, k_strides, v_strides, key_mask=None, causal=False, drop=None,
                  out=None):
    """q/k/v: any tensors whose (batch, token) strides (in elements) are given; heads contiguous (h*dh + c).
    Returns (o [B*Sq, H*dh] bf16, lse [B*H*Sq] fp32)."""
    if out is None:
        out = torch.empty((B * Sq, H * dh), dtype=BF16, device=q.device)
    lse = torch.empty((B * H * Sq,), dtype=F32, device=q.device)
    o_strides = (Sq * H * dh, H * dh)
    f = _attn_args(q, k, v, out, B, H, Sq, Sk, dh, (q_strides, k_strides, v_strides, o_strides), dh ** -0.5, key_mask,
                   causal, drop, lse)
    check(lib.ph_attention_fwd(C.byref(f), _stream()), 'ph_attention_fwd')
    return out, lse


def attention_bwd(d_o, q, k, v, o, lse, B, H, Sq, Sk, dh, *, q_strides, k_strides, v_strides, dq, dk, dv, dq_strides,
                  dk_strides, dv_strides, key_mask=None, causal=False, drop=None):
    a = _lib.AttnBwdArgs()
    o_strides = (Sq * H * dh, H * dh)
    a.f = _attn_args(q, k, v, o, B, H, Sq, Sk, dh, (q_strides, k_strides, v_strides, o_strides), dh ** -0.5, key_mask,
                     causal, drop, lse)
    a.d_o = d_o.data_ptr()
    a.do_bs, a.do_ts = o_strides
    a.dq, a.dk, a.dv = dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    (a.dq_bs, a.dq_ts), (a.dk_bs, a.dk_ts), (a.dv_bs, a.dv_ts) = dq_strides, dk_strides, dv_strides
    delta = torch.empty((B * H * Sq,), dtype=F32, device=q.device)
    a.delta = delta.data_ptr()
    check(lib.ph_attention_bwd(C.byref(a), _stream()), 'ph_attention_bwd')


def _group_ws(g, f, group, backward, device):
    """workspace of a grouped launch outside the grouped kernels (tiled K / V, per-row dK / dV); None on the grouped kernels"""
    nbytes = lib.ph_attention_group_ws_bytes(C.byref(f), group, int(backward))
    if nbytes <= 0:
        return None
    ws = torch.empty(nbytes // 2, dtype=BF16, device=device)
    g.ws, g.ws_bytes = ws.data_ptr(), nbytes
    return ws


def attention_group_fwd(q, k, v, R, group, H, Sq, Sk, dh, *, q_strides, k_strides, v_strides, drop=None, out=None):
    """cross-attention of R query rows, `group` consecutive rows per K/V batch row (ph_attention_group_fwd): q [R][Sq], k / v [R // group][Sk],
    strides as attention_fwd.  Returns (o [R*Sq, H*dh] bf16, lse [R*H*Sq] fp32): what attention_fwd gives on K/V tiled to R rows."""
    if out is None:
        out = torch.empty((R * Sq, H * dh), dtype=BF16, device=q.device)
    lse = torch.empty((R * H * Sq,), dtype=F32, device=q.device)
    o_strides = (Sq * H * dh, H * dh)
    g = _lib.AttnGroupFwdArgs()
    g.f = _attn_args(q, k, v, out, R, H, Sq, Sk, dh, (q_strides, k_strides, v_strides, o_strides), dh ** -0.5, None, False, drop, lse)
    g.group = group
    ws = _group_ws(g, g.f, group, False, q.device)
    check(lib.ph_attention_group_fwd(C.byref(g), _stream()), 'ph_attention_group_fwd')
    del ws
    return out, lse


def attention_group_bwd(d_o, q, k, v, o, lse, R, group, H, Sq, Sk, dh, *, q_strides, k_strides, v_strides, dq, dk, dv, dq_strides,
                        dk_strides, dv_strides, drop=None):
    """backward of attention_group_fwd: dq [R][Sq]; dk / dv [R // group][Sk] = the sum over a K/V row's `group` query rows"""
    g = _lib.AttnGroupBwdArgs()
    a = g.b
    o_strides = (Sq * H * dh, H * dh)
    a.f = _attn_args(q, k, v, o, R, H, Sq, Sk, dh, (q_strides, k_strides, v_strides, o_strides), dh ** -0.5, None, False, drop, lse)
    a.d_o = d_o.data_ptr()
    a.do_bs, a.do_ts = o_strides
    a.dq, a.dk, a.dv = dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    (a.dq_bs, a.dq_ts), (a.dk_bs, a.dk_ts), (a.dv_bs, a.dv_ts) = dq_strides, dk_strides, dv_strides
    delta = torch.empty((R * H * Sq,), dtype=F32, device=q.device)
    a.delta = delta.data_ptr()
    g.group = group
    ws = _group_ws(g, a.f, group, True, q.device)
    check(lib.ph_attention_group_bwd(C.byref(g), _stream()), 'ph_attention_group_bwd')
    del ws


def attention_prefix_fwd(q, pk, pv, ck, cv, R, H, Tc, Tp, group, dh, *, q_strides, pk_strides, pv_strides, ck_strides, cv_strides,
                         prefix_mask=None, pm_stride=0, cont_mask=None, cm_stride=0, out=None):
    """shared-prefix attention (ph_attention_prefix_fwd): continuation row r (queries / keys q, ck, cv: [R][Tc]) against the Tp
    prefix keys of prefix row r // group (pk, pv: [R / group][Tp]) and, causally, its own keys.  Masks: uint8, (batch stride, token
    stride 1).  Returns o [R*Tc, H*dh] bf16."""
    if out is None:
        out = torch.empty((R * Tc, H * dh), dtype=BF16, device=q.device)
    a = _lib.AttnPrefixFwdArgs()
    a.q, a.ck, a.cv, a.o = q.data_ptr(), ck.data_ptr(), cv.data_ptr(), out.data_ptr()
    a.pk, a.pv = (pk.data_ptr(), pv.data_ptr()) if Tp > 0 else (None, None)
    (a.q_bs, a.q_ts), (a.pk_bs, a.pk_ts), (a.pv_bs, a.pv_ts) = q_strides, pk_strides, pv_strides
    (a.ck_bs, a.ck_ts), (a.cv_bs, a.cv_ts), (a.o_bs, a.o_ts) = ck_strides, cv_strides, (Tc * H * dh, H * dh)
    a.prefix_mask, a.pm_bs = ptr(prefix_mask), pm_stride
    a.cont_mask, a.cm_bs = ptr(cont_mask), cm_stride
    a.R, a.group, a.H, a.Tc, a.Tp, a.dh = R, group, H, Tc, Tp, dh
    a.scale = dh ** -0.5
    check(lib.ph_attention_prefix_fwd(C.byref(a), _stream()), 'ph_attention_prefix_fwd')
    return out


# ---------------------------------------------------------------------------------------------- front end

def patchify(img, p, Kp):
    B, Cc, R, _ = img.shape
    g = R // p
    col = torch.empty((B * g * g, Kp), dtype=BF16, device=img.device)
    check(lib.ph_patchify(img.data_ptr(), col.data_ptr(), B, Cc, R, p, Kp, _stream()), 'ph_patchify')
    return col


def resize_to_nhwc(x, Hout, Wout):
    B, Cc, Hin, Win = x.shape
    y = torch.empty((B, Hout, Wout, Cc), dtype=BF16, device=x.device)
    check(lib.ph_resize_bilinear_nchw_to_nhwc(x.data_ptr(), y.data_ptr(), B, Cc, Hin, Win, Hout, Wout, _stream()),
          'ph_resize_bilinear_nchw_to_nhwc')
    return y


REMAP_PARTS = 16


def remap_resize_to_nhwc(raw, Hout, Wout):
    """raw: fp32 [B, C, H, W] dense expert map BEFORE post_label_process (depth / normal / edge).  Returns the stem input [B, Hout, Wout, C] bf16 =
    bilinear(2 * (x - min) / (max - min + 1e-6) - 1) with the min / max of each sample's whole map (dataset/utils.py:120-121 + vit.py:88-90)."""
    B, Cc, Hin, Win = raw.shape
    raw = raw.contiguous().float()
    part = torch.empty((B, REMAP_PARTS, 2), dtype=F32, device=raw.device)
    check(lib.ph_dense_minmax_partial(raw.data_ptr(), part.data_ptr(), B, Cc * Hin * Win, REMAP_PARTS, _stream()), 'ph_dense_minmax_partial')
    y = torch.empty((B, Hout, Wout, Cc), dtype=BF16, device=raw.device)
    check(lib.ph_resize_remap_nchw_to_nhwc(raw.data_ptr(), part.data_ptr(), REMAP_PARTS, y.data_ptr(), B, Cc, Hin, Win, Hout, Wout, _stream()),
          'ph_resize_remap_nchw_to_nhwc')
    return y


def inpaint_resize(label_map, table, Hout, Wout):
    """label_map: uint8 [B, H, W] (or [B, 1, H, W]); table: fp32 [256, C] (shared) or [B, 256, C] (per image).
    Returns the stem input [B, Hout, Wout, C] bf16 = bilinear(post_label_process(label_map)) (dataset/utils.py:117-160 + vit.py:88-90)."""
    if label_map.dim() == 4:
        label_map = label_map[:, 0]
    assert label_map.dtype == torch.uint8 and table.dtype == F32 and table.shape[-2] == 256
    label_map, table = label_map.contiguous(), table.contiguous()
    B, Hin, Win = label_map.shape
    Cc = table.shape[-1]
    stride = 256 * Cc if table.dim() == 3 else 0
    assert table.dim() == 2 or table.shape[0] == B
    y = torch.empty((B, Hout, Wout, Cc), dtype=BF16, device=label_map.device)
    check(lib.ph_inpaint_resize_nhwc(label_map.data_ptr(), table.data_ptr(), stride, y.data_ptr(), B, Cc, Hin, Win, Hout, Wout, _stream()),
          'ph_inpaint_resize_nhwc')
    return y


def conv_fwd_grouped(items):
    """items: [(x, geo, w_shadow, y, col_stats)] -- the same-layer convolutions of several expert stems in ONE launch per
    PH_GEMM_GROUP_MAX problems (vit.py:88-120: the stems are independent until their tokens are concatenated).  Each is an implicit GEMM
    y[B*Ho*Wo, Cout] = im2col(x) . w_shadow[Cout, Kp]^T with x the NHWC bf16 activation and geo = (B, H, W, C, ks, stride)."""
    def fill(arr, j, it):
        x, (B, H, W, Cc, ks, stride), w_shadow, y, col_stats = it
        return gemm_args(x, w_shadow, y, B * conv_out_size(H, ks, stride) * conv_out_size(W, ks, stride), w_shadow.shape[0], w_shadow.shape[1],
                         conv=it[1], col_stats=col_stats, into=arr[j])
    launch_grouped(lib.ph_gemm_grouped_bf16, _lib.GemmArgs, items, fill, what='ph_gemm_grouped_bf16 (conv)')


def _wgrad_problem(item, ws):
    """one item of wgrad_split_grouped -> (ph_gemm_args, its fresh fp32 output, keep-alive)"""
    dy, x, M, N, K, conv = item
    out = torch.empty((M, N), dtype=F32, device=dy.device)
    g, keep = gemm_args(dy, x, out, M, N, K, trans_a=True, trans_b=True, out_f32=True, conv=conv, workspace=ws)
    return g, out, keep


def wgrad_split_grouped(items):
    """Weight gradients with few output tiles and very long reductions -- the same conv layer of several expert stems -- in ONE grouped
    launch that is also split over K, plus one grouped fold pass (include/prismer_hip.h: ph_gemm_grouped_bf16 with a workspace).
    items: [(dy [K, M] bf16, x, M, N, K, conv)]: out[M, N] (fp32, returned) = dy^T . x with x = [K, N] bf16 (conv None) or the im2col
    view of the NHWC activation x (conv = (B, H, W, C, ks, stride): the gathered operand sits on the reduction side).
    Implicit and plain problems cannot share a launch, so they are grouped separately."""
    outs = [None] * len(items)

    def fill(arr, j, i):
        arr[j], outs[i], keep = _wgrad_problem(items[i], _workspace(items[i][0].device, WS_DEFERRED))
        return keep
    for want_conv in (True, False):
        launch_grouped(lib.ph_gemm_grouped_bf16, _lib.GemmArgs, [i for i, it in enumerate(items) if (it[5] is not None) == want_conv], fill,
                       what='ph_gemm_grouped_bf16 (split wgrad)')
    return outs


def wgrad_group_args(items, ws):
    """ph_gemm_args of ONE group of wgrad_split_grouped items sharing the workspace ws (or None) -> (array, fresh fp32 outputs, keep-alives)"""
    arr, outs, keep = (_lib.GemmArgs * len(items))(), [], []
    for j, it in enumerate(items):
        arr[j], out, k = _wgrad_problem(it, ws)
        outs.append(out)
        keep.append(k)
    return arr, outs, keep


def conv_wgrad_persistent(items, ws=None):
    """The conv weight gradients of ONE layer of several expert stems (items as in wgrad_split_grouped, all with a conv gather) in one launch
    of the persistent 256x128 kernel: units of (problem, tile, k-range) fill its blocks evenly, cut tiles are folded inside the launch.
    Returns the fp32 outputs, or None -- nothing launched -- when the library would not take that kernel for the group (ph_gemm_route: a
    reduction that is no multiple of 64 or shorter than 32 k-tiles, ...): the caller then keeps its per-expert calls.
    ws: fp32 scratch for counters and slabs, or None for this stream's WS_STEM_WGRAD (see _workspace)."""
    if not items or len(items) > _lib.GEMM_GROUP_MAX:
        return None
    if ws is None:
        ws = _workspace(items[0][0].device, WS_STEM_WGRAD)
    arr, outs, keep = wgrad_group_args(items, ws)
    info = _lib.GemmRouteInfo()
    if lib.ph_gemm_route(arr, len(items), 1, 0, C.byref(info)) != 0 or info.part[0].cls != _lib.GEMM_CLS_BIG_GROUPED:
        return None
    check(lib.ph_gemm_grouped_bf16(arr, len(items), _stream()), 'ph_gemm_grouped_bf16 (stem conv wgrad)')
    return outs


def conv_out_size(H, ks, stride):
    pad = ks // 2
    return (H + 2 * pad - ks) // stride + 1


def im2col(x, B, H, W, Cc, ks, stride, Kp, bn_scale=None, bn_shift=None):
    Ho, Wo = conv_out_size(H, ks, stride), conv_out_size(W, ks, stride)
    col = torch.empty((B * Ho * Wo, Kp), dtype=BF16, device=x.device)
    check(lib.ph_im2col_nhwc(x.data_ptr(), col.data_ptr(), B, H, W, Cc, ks, stride, Kp, ptr(bn_scale), ptr(bn_shift), _stream()),
          'ph_im2col_nhwc')
    return col


def col2im(dcol, B, H, W, Cc, ks, stride, Kp):
    dx = torch.empty((B * H * W, Cc), dtype=BF16, device=dcol.device)
    check(lib.ph_col2im_nhwc(dcol.data_ptr(), dx.data_ptr(), B, H, W, Cc, ks, stride, Kp, _stream()), 'ph_col2im_nhwc')
    return dx


def bn_stats(y, gamma, beta, running_mean, running_var, training, momentum=0.1, eps=1e-5, out=None):
    """returns stats [4, C] fp32 = (mean, rstd, scale, shift); y: bf16 [M, C] conv output.
    out: optional ZEROED [4, C] slice of a per-step arena (saves the per-layer memset launch)."""
    M, Cc = y.shape
    st = out if out is not None else torch.empty((4, Cc), dtype=F32, device=y.device)
    check(lib.ph_bn_stats(y.data_ptr(), M, Cc, gamma.data_ptr(), beta.data_ptr(), running_mean.data_ptr(), running_var.data_ptr(),
                          momentum, eps, int(training), st[0].data_ptr(), st[1].data_ptr(), st[2].data_ptr(), st[3].data_ptr(),
                          int(out is not None), _stream()), 'ph_bn_stats')
    return st


def bn_relu_bwd(da, y, gamma, beta, stats, dgamma, dbeta, sums=None):
    """sums: optional ZEROED fp32 [2C] slice of a per-step arena (saves the per-layer memset launch)."""
    M, Cc = y.shape
    dy = torch.empty_like(y)
    pre = sums is not None
    if sums is None:
        sums = torch.empty((2 * Cc,), dtype=F32, device=y.device)
    check(lib.ph_bn_relu_bwd(da.data_ptr(), y.data_ptr(), dy.data_ptr(), M, Cc, gamma.data_ptr(), beta.data_ptr(), stats[0].data_ptr(),
                             stats[1].data_ptr(), ptr(dgamma), ptr(dbeta), sums.data_ptr(), int(pre), _stream()), 'ph_bn_relu_bwd')
    return dy


def _bn_fill(arr, j, d):
    it = arr[j]
    it.y, it.a, it.dy = d['y'].data_ptr(), d['a'].data_ptr(), ptr(d.get('dy'))
    it.M, it.C = d['y'].shape[0], d['y'].shape[1]
    it.gamma, it.beta = d['gamma'].data_ptr(), d['beta'].data_ptr()
    it.running_mean, it.running_var = ptr(d.get('running_mean')), ptr(d.get('running_var'))
    it.stats, it.sums = d['stats'].data_ptr(), d['sums'].data_ptr()
    it.dgamma, it.dbeta = ptr(d.get('dgamma')), ptr(d.get('dbeta'))


def bn_apply_relu_grouped(items, training, momentum=0.1, eps=1e-5):
    """items: dicts y [M,C] bf16 (conv output), a [M,C] bf16 (out: relu(bn(y))), gamma, beta, running_mean, running_var,
    stats [4,C] fp32 (out), sums [PH_COLSTAT_SLABS = 8][2][C] fp64 (column sums / sums of squares from the conv GEMM epilogue,
    ph_gemm_args.col_stats; unused in eval mode)"""
    launch_grouped(lambda arr, n, stream: lib.ph_bn_apply_relu_grouped(arr, n, momentum, eps, int(training), stream), _lib.BnItem, items, _bn_fill,
                   _lib.BN_GROUP_MAX, 'ph_bn_apply_relu_grouped')


def bn_relu_bwd_grouped(items):
    """items: dicts y, a (= dA, gradient w.r.t. relu(bn(y))), dy (out), gamma, beta, stats [4,C], sums [2,C] ZEROED, dgamma, dbeta"""
    launch_grouped(lib.ph_bn_relu_bwd_grouped, _lib.BnItem, items, _bn_fill, _lib.BN_GROUP_MAX, 'ph_bn_relu_bwd_grouped')


def gemm_grouped(problems, trans_a=False, trans_b=False):
    """problems: [(a, b, out, M, N, K)] plain bf16 GEMMs of one layout in grouped launches (out bf16, no epilogue)"""
    def fill(arr, j, p):
        gemm_args(*p, trans_a=trans_a, trans_b=trans_b, into=arr[j])
    launch_grouped(lib.ph_gemm_grouped_bf16, _lib.GemmArgs, problems, fill, what='ph_gemm_grouped_bf16')


def tokens_finalize(feat, pos, tokens, B, G, D, tok_per_batch, tok_off, inst=None, E=0, g=0, table=None, inst_emb=None):
    check(lib.ph_tokens_finalize(feat.data_ptr(), pos.data_ptr(), tokens.data_ptr(), B, G, D, tok_per_batch, tok_off, ptr(inst), E, g,
                                 ptr(table), ptr(inst_emb), _stream()), 'ph_tokens_finalize')


def tokens_finalize_bwd(dtokens, dfeat, dpos, B, G, D, tok_per_batch, tok_off, inst=None, E=0, g=0, table=None, dinst_emb=None):
    check(lib.ph_tokens_finalize_bwd(dtokens.data_ptr(), ptr(dfeat), ptr(dpos), B, G, D, tok_per_batch, tok_off, ptr(inst), E, g,
                                     ptr(table), ptr(dinst_emb), _stream()), 'ph_tokens_finalize_bwd')


def gather_taps(inp, idx, w, n_out, taps, D):
    out = torch.empty((n_out, D), dtype=F32, device=inp.device)
    check(lib.ph_gather_taps(inp.data_ptr(), out.data_ptr(), idx.data_ptr(), w.data_ptr(), n_out, taps, D, _stream()), 'ph_gather_taps')
    return out


def scatter_taps(dout, din, idx, w, n_out, taps, D):
    check(lib.ph_scatter_taps(dout.data_ptr(), din.data_ptr(), idx.data_ptr(), w.data_ptr(), n_out, taps, D, _stream()), 'ph_scatter_taps')


# ---------------------------------------------------------------------------------------------- decoder ends

def embed_args(ids, word, pos, typ, gamma, beta, eps, pad_id, out, xhat, rstd, drop, out_f32=None):
    B, T = ids.shape
    a = _lib.EmbedFwdArgs()
    a.ids, a.B, a.T, a.H, a.pad_id = ids.data_ptr(), B, T, word.shape[1], pad_id
    a.word, a.pos, a.type = word.data_ptr(), pos.data_ptr(), typ.data_ptr()
    a.gamma, a.beta, a.eps = gamma.data_ptr(), beta.data_ptr(), eps
    a.out, a.xhat, a.rstd = out.data_ptr(), ptr(xhat), ptr(rstd)
    _set_drop(a, drop)
    a.out_f32 = ptr(out_f32)
    return a


def embed_fwd(ids, word, pos, typ, gamma, beta, eps, pad_id, drop=None, want_f32=False, pos_base=None):
    """pos_base: int32 [B] device tensor or None -- the offset form (ph_embed_fwd_offset): real tokens of row b take position
    pad + pos_base[b] + cumsum(ids != pad)"""
    B, T = ids.shape
    H = word.shape[1]
    out = torch.empty((B * T, H), dtype=BF16, device=ids.device)
    xhat = torch.empty((B * T, H), dtype=BF16, device=ids.device)
    rstd = torch.empty((B * T,), dtype=F32, device=ids.device)
    out_f32 = torch.empty((B * T, H), dtype=F32, device=ids.device) if want_f32 else None
    a = embed_args(ids, word, pos, typ, gamma, beta, eps, pad_id, out, xhat, rstd, drop, out_f32)
    if pos_base is None:
        check(lib.ph_embed_fwd(C.byref(a), _stream()), 'ph_embed_fwd')
    else:
        assert pos_base.dtype == torch.int32 and pos_base.numel() == B and pos_base.is_contiguous()
        check(lib.ph_embed_fwd_offset(C.byref(a), pos_base.data_ptr(), _stream()), 'ph_embed_fwd_offset')
    if want_f32:
        return out, xhat, rstd, out_f32
    return out, xhat, rstd


def embed_bwd(dout, ids, word, pos, typ, gamma, beta, eps, pad_id, xhat, rstd, drop, dword, dpos, dtype, dgamma, dbeta):
    a = _lib.EmbedBwdArgs()
    a.f = embed_args(ids, word, pos, typ, gamma, beta, eps, pad_id, dout, xhat, rstd, drop)
    a.dout = dout.data_ptr()
    a.dword, a.dpos, a.dtype, a.dgamma, a.dbeta = ptr(dword), ptr(dpos), ptr(dtype), ptr(dgamma), ptr(dbeta)
    check(lib.ph_embed_bwd(C.byref(a), _stream()), 'ph_embed_bwd')


def ce_fwd(logits, labels, B, T, V, eps):
    loss = torch.empty((B,), dtype=F32, device=logits.device)
    row_lse = torch.empty((2, B * T), dtype=F32, device=logits.device)           # [0]: log-sum-exp per token (kept for the backward), [1]: per-token loss scratch
    check(lib.ph_ce_fwd(logits.data_ptr(), logits.stride(0), labels.data_ptr(), B, T, V, eps, loss.data_ptr(), row_lse[0].data_ptr(),
                        row_lse[1].data_ptr(), _stream()), 'ph_ce_fwd')
    row_lse = row_lse[0]
    return loss, row_lse


def softmax_gather(logits, ids):
    """softmax(logits, dim=1).index_select(1, ids) for bf16 logit rows [R, V] (a strided view of the decoder's padded logits buffer is fine:
    the row stride must be a multiple of 8 elements, the rows 16-B aligned); fp32 [R, len(ids)] out -- prismer_caption.py:70 / prismer_vqa.py:51"""
    assert logits.dim() == 2 and logits.dtype == BF16 and logits.stride(1) == 1 and ids.dtype == torch.int64
    R, V = logits.shape
    ids = ids.contiguous()
    out = torch.empty((R, ids.numel()), dtype=F32, device=logits.device)
    check(lib.ph_softmax_gather_bf16(logits.data_ptr(), logits.stride(0), R, V, ids.data_ptr(), ids.numel(), out.data_ptr(), _stream()), 'ph_softmax_gather_bf16')
    return out


def beam_topk_workspace(B, nb, V, device):
    """the caller-owned scratch of beam_topk for B items x nb beams over V columns (either row layout), sized by ph_query_workspace"""
    n = lib.ph_query_workspace(_lib.WS_BEAM_TOPK, (C.c_int64 * 3)(B, nb, V), 3)
    if n < 0:
        raise _lib.PrismerHipError(f'ph_query_workspace(PH_WS_BEAM_TOPK, {B}, {nb}, {V}): dimensions outside the limits of ph_beam_topk')
    return torch.empty(n // 4, dtype=F32, device=device)


def beam_topk(logits, beam_scores, B, nb, eos_token_id, ban_eos, workspace=None, out=None, edits=None):
    """The best 2*nb candidates of every item, best first: (top_score fp32, top_beam int32, top_tok int32), each [B, 2*nb], of
    beam_scores[row] + log_softmax(logits[row]) over bf16 logit rows [B*nb or B, V] (a strided view is fine: row stride a multiple of 8
    elements, rows 16-B aligned).  B rows = one row per item (all its beams share it, beam 0 is reported).  Ties: flat index ascending.
    edits: None, or (ids int64 [B*nb, >= cur], cur, repetition_penalty, no_repeat_ngram_size): ph_beam_topk_edit, the two processors on the
    log-probabilities with ids[:, :cur] as every beam's history."""
    assert logits.dim() == 2 and logits.dtype == BF16 and logits.stride(1) == 1 and beam_scores.dtype == F32 and beam_scores.is_contiguous()
    R, V = logits.shape
    assert R in (B, B * nb) and beam_scores.numel() == R, 'beam_topk: one logit row and one score per beam, or one per item'
    if workspace is None:
        workspace = beam_topk_workspace(B, nb, V, logits.device) if 1 <= nb <= 8 and V >= 2 * nb + 1 else torch.empty(1, dtype=F32, device=logits.device)
    if out is None:
        out = (torch.empty((B, 2 * nb), dtype=F32, device=logits.device), torch.empty((B, 2 * nb), dtype=torch.int32, device=logits.device),
               torch.empty((B, 2 * nb), dtype=torch.int32, device=logits.device))
    a = _lib.BeamTopkArgs(logits.data_ptr(), logits.stride(0), V, B, nb, R // B, beam_scores.data_ptr(), int(eos_token_id), int(bool(ban_eos)),
                          workspace.data_ptr(), workspace.numel() * workspace.element_size(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr())
    if edits is None:
        check(lib.ph_beam_topk(C.byref(a), _stream()), 'ph_beam_topk')
        return out
    ids, cur, penalty, ngram = edits
    assert ids.dtype == torch.int64 and ids.dim() == 2 and ids.shape[0] == B * nb and ids.stride(1) == 1 and ids.device == logits.device, \
        'beam_topk: ids int64 [B*nb, T] on the device of the logits'
    check(lib.ph_beam_topk_edit(C.byref(a), ids.data_ptr(), ids.stride(0), int(cur), float(penalty), int(ngram), _stream()), 'ph_beam_topk_edit')
    return out


def beam_advance(top, ids_in, ids_out, beam_scores, hyp_score, hyp_tok, hyp_len, n_hyp, done, rows_out, nb_in, cur, eos_token_id, pad_token_id,
                 len_div):
    """One step of the device-resident beam-search state from beam_topk's output `top` (see ph_beam_advance): ids_in -> ids_out with the new
    token at `cur`, next beam_scores, finished hypotheses, done flags, and into rows_out (int32 [rep * B*nb]) the source row of every beam."""
    top_score, top_beam, top_tok = top
    B, nb = hyp_score.shape
    Bb, Tmax = ids_in.shape
    assert Bb == B * nb and ids_out.shape == ids_in.shape and ids_in.dtype == ids_out.dtype == hyp_tok.dtype == torch.int64
    assert ids_in.is_contiguous() and ids_out.is_contiguous() and hyp_tok.is_contiguous() and hyp_tok.shape == (B, nb, Tmax)
    assert top_score.shape == (B, 2 * nb) and beam_scores.numel() == Bb and beam_scores.dtype == hyp_score.dtype == F32
    assert hyp_len.dtype == n_hyp.dtype == done.dtype == rows_out.dtype == top_beam.dtype == top_tok.dtype == torch.int32
    assert hyp_len.numel() == Bb and n_hyp.numel() == B and done.numel() == B and rows_out.numel() % Bb == 0
    a = _lib.BeamAdvanceArgs(top_score.data_ptr(), top_beam.data_ptr(), top_tok.data_ptr(), ids_in.data_ptr(), ids_out.data_ptr(), beam_scores.data_ptr(),
                             hyp_score.data_ptr(), hyp_tok.data_ptr(), hyp_len.data_ptr(), n_hyp.data_ptr(), done.data_ptr(), rows_out.data_ptr(),
                             B, nb, nb_in, Tmax, cur, int(eos_token_id), int(pad_token_id), rows_out.numel() // Bb, float(len_div))
    check(lib.ph_beam_advance(C.byref(a), _stream()), 'ph_beam_advance')


def sample_step(logits, ids, done, seq_logprob, cur, temperature, top_k, top_p, eos_token_id, pad_token_id, ban_eos, seed, diag=None, edits=None):
    """One sampled decoding step for every row (see ph_sample_step): over bf16 logit rows [R, V], or [R / n, V] when n consecutive rows share
    one (a strided view is fine: row stride a multiple of 8 elements, rows 16-B aligned), it writes ids[:, cur] (int64 [R, Tmax]), done (int32 [R]) and seq_logprob (fp32 [R]) in place.
    The draw of row r is a function of (seed, r, cur) alone.  diag: None or (u fp32, thr fp32, kept_count int32, kept_mass fp32), [R] each,
    any of them None.  edits: None, or (repetition_penalty, no_repeat_ngram_size): ph_sample_step_edit, the two processors on the row first,
    with ids[r, :cur] as row r's history."""
    assert logits.dim() == 2 and logits.dtype == BF16 and logits.stride(1) == 1
    Rl, V = logits.shape
    R = ids.shape[0]
    assert ids.dtype == torch.int64 and ids.dim() == 2 and R % Rl == 0 and ids.is_contiguous(), 'sample_step: ids int64 [R, Tmax], R a multiple of the logit rows'
    assert done.dtype == torch.int32 and done.numel() == R and done.is_contiguous() and seq_logprob.dtype == F32 and seq_logprob.numel() == R \
        and seq_logprob.is_contiguous()
    d = [None] * 4 if diag is None else list(diag)
    for t, dt in zip(d, (F32, F32, torch.int32, F32)):
        assert t is None or (t.dtype == dt and t.numel() == R and t.is_contiguous())
    a = _lib.SampleStepArgs(logits.data_ptr(), logits.stride(0), V, R, R // Rl, ids.shape[1], int(cur), ids.data_ptr(), done.data_ptr(), seq_logprob.data_ptr(),
                            float(temperature), float(top_p), int(top_k), int(eos_token_id), int(pad_token_id), int(bool(ban_eos)),
                            int(seed) & 0xFFFFFFFFFFFFFFFF, *(None if t is None else t.data_ptr() for t in d))
    if edits is None:
        check(lib.ph_sample_step(C.byref(a), _stream()), 'ph_sample_step')
    else:
        check(lib.ph_sample_step_edit(C.byref(a), float(edits[0]), int(edits[1]), _stream()), 'ph_sample_step_edit')


def ce_bwd(logits, labels, B, T, V, eps, row_lse, dloss):
    check(lib.ph_ce_bwd(logits.data_ptr(), logits.stride(0), labels.data_ptr(), B, T, V, logits.shape[1], eps, row_lse.data_ptr(),
                        dloss.data_ptr(), _stream()), 'ph_ce_bwd')
    return logits


# ---------------------------------------------------------------------------------------------- utilities

def adamw(p, g, m, v, p_bf16, n, hyper, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.05, grad_scale=1.0, zero_grad=False, keep=None):
    """keep: optional int32 tensor, bit c = gradients [1024 c, 1024 c + 1024) keep their values (see ph_adamw_keep)"""
    assert keep is None or keep.numel() * 32 * 1024 >= n
    check(lib.ph_adamw_keep(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), ptr(p_bf16), n, hyper.data_ptr(), beta1, beta2, eps,
                            weight_decay, grad_scale, int(zero_grad), ptr(keep), _stream()), 'ph_adamw')


class ClipCtl:
    """the device control block of the guarded update (ph_clip_ctl) and typed views of its words: coef / norm fp32 [1], apply / finite int32 [1],
    sumsq fp64 [1], applied / skipped int64 [1].  Allocated zeroed: no update applied or skipped yet."""

    def __init__(self, device):
        self.words = torch.zeros(5, dtype=torch.int64, device=device)
        f, i = self.words.view(F32), self.words.view(torch.int32)
        self.coef, self.norm, self.apply, self.finite = f[0:1], f[2:3], i[1:2], i[3:4]
        self.sumsq = self.words.view(torch.float64)[2:3]
        self.applied, self.skipped = self.words[3:4], self.words[4:5]

    def data_ptr(self):
        return self.words.data_ptr()


def grad_norm_workspace(lengths, device):
    """the caller-owned partials of grad_sqnorm for ranges of these lengths (fp64, one per block), sized by ph_query_workspace"""
    n = lib.ph_query_workspace(_lib.WS_GRAD_NORM, (C.c_int64 * len(lengths))(*lengths), len(lengths))
    if n < 0:
        raise _lib.PrismerHipError(f'ph_query_workspace(PH_WS_GRAD_NORM, {list(lengths)}): need 1..{_lib.SQNORM_RANGES_MAX} ranges of >= 1 element')
    return torch.empty(n // 8, dtype=torch.float64, device=device)


def grad_sqnorm(ranges, workspace=None):
    """one fp64 partial sum of squares per block over the flat fp32 tensors `ranges` (ph_grad_sqnorm); returns the workspace, every element of
    which this launch wrote.  Feed it to clip_finalize."""
    assert all(t.dtype == F32 and t.is_contiguous() for t in ranges)
    lengths = [t.numel() for t in ranges]
    if workspace is None:
        workspace = grad_norm_workspace(lengths, ranges[0].device)
    k = len(ranges)
    check(lib.ph_grad_sqnorm((C.c_void_p * k)(*[t.data_ptr() for t in ranges]), (C.c_int64 * k)(*lengths), k, workspace.data_ptr(),
                             workspace.numel() * 8, _stream()), 'ph_grad_sqnorm')
    return workspace


def clip_finalize(partials, ctl, hyper, pre_scale=1.0, max_norm=None, skip_nonfinite=False, beta1=0.9, beta2=0.999):
    """partials -> ctl (norm, clip coefficient, apply flag, applied / skipped counters) and Adam's bias corrections hyper[1:3] from the applied
    count (ph_clip_finalize).  max_norm None: no clipping."""
    assert partials.dtype == torch.float64 and hyper.dtype == F32 and hyper.numel() >= 3
    check(lib.ph_clip_finalize(partials.data_ptr(), partials.numel(), float(pre_scale), -1.0 if max_norm is None else float(max_norm),
                               int(bool(skip_nonfinite)), float(beta1), float(beta2), hyper.data_ptr(), ctl.data_ptr(), _stream()), 'ph_clip_finalize')


def adamw_ctl(p, g, m, v, p_bf16, n, hyper, ctl, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.05, grad_scale=1.0, zero_grad=False, keep=None):
    """adamw under a control block (ph_adamw_ctl): gradients scaled by grad_scale * ctl.coef; ctl.apply == 0 leaves p, m, v and the shadow alone"""
    assert keep is None or keep.numel() * 32 * 1024 >= n
    check(lib.ph_adamw_ctl(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), ptr(p_bf16), n, hyper.data_ptr(), beta1, beta2, eps,
                           weight_decay, grad_scale, int(zero_grad), ptr(keep), ptr(ctl), _stream()), 'ph_adamw_ctl')


def adamw_ema(p, g, m, v, p_bf16, n, hyper, ema, ema_w, ctl=None, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.05, grad_scale=1.0, zero_grad=False,
              keep=None):
    """adamw / adamw_ctl (ctl given) with the moving average of the weights updated in the same launch (ph_adamw_ema): ema += ema_w[0] * (p' - ema),
    ema fp32 [>= n], ema_w one fp32 on the device (1 - decay of this update); a skipped update (ctl.apply == 0) leaves ema alone"""
    assert keep is None or keep.numel() * 32 * 1024 >= n
    assert ema.dtype == F32 and ema.is_contiguous() and ema.numel() >= n and ema_w.dtype == F32 and ema_w.numel() >= 1 and ema_w.device == ema.device
    check(lib.ph_adamw_ema(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), ptr(p_bf16), n, hyper.data_ptr(), beta1, beta2, eps,
                           weight_decay, grad_scale, int(zero_grad), ptr(keep), ptr(ctl), ema.data_ptr(), ema_w.data_ptr(), _stream()), 'ph_adamw_ema')


def swap_f32(a, b):
    """a <-> b for two contiguous, disjoint, 16-B aligned fp32 tensors of one length (ph_swap_f32): exact, no temporary"""
    assert a.dtype == F32 and b.dtype == F32 and a.is_contiguous() and b.is_contiguous() and a.numel() == b.numel()
    check(lib.ph_swap_f32(a.data_ptr(), b.data_ptr(), a.numel(), _stream()), 'ph_swap_f32')


def cast_to_bf16(x, out=None, scale=1.0):
    if out is None:
        out = torch.empty(x.shape, dtype=BF16, device=x.device)
    if scale == 1.0:
        check(lib.ph_cast_f32_to_bf16(x.data_ptr(), out.data_ptr(), x.numel(), _stream()), 'ph_cast_f32_to_bf16')
    else:
        check(lib.ph_scale_cast_f32_to_bf16(x.data_ptr(), out.data_ptr(), x.numel(), float(scale), _stream()), 'ph_scale_cast_f32_to_bf16')
    return out


def cast_to_f32(x, out=None):
    if out is None:
        out = torch.empty(x.shape, dtype=F32, device=x.device)
    check(lib.ph_cast_bf16_to_f32(x.data_ptr(), out.data_ptr(), x.numel(), _stream()), 'ph_cast_bf16_to_f32')
    return out


def colsum(x, out, M=None, N=None):
    """out[N] (fp32) += column sums of bf16 x[M, N]."""
    M = x.shape[0] if M is None else M
    N = x.shape[1] if N is None else N
    check(lib.ph_colsum_bf16(x.data_ptr(), M, N, x.stride(0), out.data_ptr(), _stream()), 'ph_colsum_bf16')


def add(a, b, out=None):
    if out is None:
        out = torch.empty_like(a)
    check(lib.ph_add_bf16(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), _stream()), 'ph_add_bf16')
    return out


def act_bwd(dy, pre, act, out=None):
    if out is None:
        out = torch.empty_like(dy)
    check(lib.ph_act_bwd_bf16(dy.data_ptr(), pre.data_ptr(), out.data_ptr(), dy.numel(), act, _stream()), 'ph_act_bwd_bf16')
    return out


def copy_rows(src, dst, rows, cols, src_map=IDENT, dst_map=IDENT, accumulate=False, src_ld=None, dst_ld=None):
    check(lib.ph_copy_rows_bf16(src.data_ptr(), src_ld or src.stride(0), src_map, dst.data_ptr(), dst_ld or dst.stride(0), dst_map,
                                rows, cols, int(accumulate), _stream()), 'ph_copy_rows_bf16')


def gather_rows(src, idx, dst, cols=None):
    """dst[r, :cols] = src[idx[r], :cols]; src / dst: 2-D bf16 views (row stride = stride(0)), idx: int32 device tensor"""
    assert src.dtype == BF16 and dst.dtype == BF16 and idx.dtype == torch.int32 and idx.is_cuda
    cols = src.shape[1] if cols is None else cols
    check(lib.ph_gather_rows_bf16(src.data_ptr(), src.stride(0), idx.data_ptr(), dst.data_ptr(), dst.stride(0), idx.numel(), cols, _stream()),
          'ph_gather_rows_bf16')
    return dst


def conv_weight_to_shadow(w, shadow, Cout, Cin, ks, Kp):
    check(lib.ph_conv_weight_to_shadow(w.data_ptr(), shadow.data_ptr(), Cout, Cin, ks, Kp, _stream()), 'ph_conv_weight_to_shadow')


def conv_grad_from_shadow(dshadow, dw, Cout, Cin, ks, Kp):
    check(lib.ph_conv_grad_from_shadow(dshadow.data_ptr(), dw.data_ptr(), Cout, Cin, ks, Kp, _stream()), 'ph_conv_grad_from_shadow')


def conv_layout_grouped(items, to_shadow):
    """items: [(src, dst, Cout, Cin, ks, Kp)]; one launch per PH_CONV_GROUP_MAX layers."""
    def fill(arr, j, e):
        it, (src, dst, Co, Ci, ks, Kp) = arr[j], e
        it.src, it.dst, it.Cout, it.Cin, it.ks, it.Kp = src.data_ptr(), dst.data_ptr(), Co, Ci, ks, Kp
    launch_grouped(lib.ph_conv_weight_to_shadow_grouped if to_shadow else lib.ph_conv_grad_from_shadow_grouped, _lib.ConvLayoutItem, items, fill,
                   _lib.CONV_GROUP_MAX, 'ph_conv_layout_grouped')


def conv_dgrad_shadows(items):
    """items: [(w fp32 [Cout,Cin,3,3], dst bf16 [Cin, 9*Cout], Cout, Cin, stride)]: weight operands of the implicit data gradients,
    one launch per PH_CONV_GROUP_MAX layers (include/prismer_hip.h: ph_conv_dgrad_shadow_grouped)"""
    def fill(arr, j, e):
        it, (w, dst, Co, Ci, stride) = arr[j], e
        it.w, it.dst, it.Cout, it.Cin, it.stride = w.data_ptr(), dst.data_ptr(), Co, Ci, stride
    launch_grouped(lib.ph_conv_dgrad_shadow_grouped, _lib.ConvDgradItem, items, fill, _lib.CONV_GROUP_MAX, 'ph_conv_dgrad_shadow_grouped')


# parity classes of the input pixel of a stride-2, 3x3, pad-1 convolution: (py, px) -> (first tap, taps) in the dgrad shadow
DGRAD_CLASSES = (((0, 0), 0, 1), ((0, 1), 1, 2), ((1, 0), 3, 2), ((1, 1), 5, 4))


def conv_dgrad_grouped(items):
    """Implicit data gradients of 3x3 (pad 1) convolutions, the same layer of several stems in grouped launches (round 3; replaces
    dcol = dY . W followed by the col2im gather: 9 x the output in transient traffic and, for stride 2, 4 x the useful FLOPs).
    items: [(dy [B*Ho*Wo, Cout] bf16, wd [Cin, 9*Cout] dgrad shadow, dx [B*H*W, Cin] bf16 out, (B, H, W, Cin, Cout, stride))].
    stride 1: dX = conv3x3(dY) with flipped taps, one problem.  stride 2: one problem per parity class of the input pixel: the
    A operand gathers a (1+py) x (1+px) window of dY, the output rows are scattered to the class's pixels (GemmArgs.rowmap_*)."""
    probs = []
    for dy, wd, dx, (B, H, W, Ci, Co, stride) in items:
        Ho, Wo = (H, W) if stride == 1 else (H // 2, W // 2)
        if stride == 1:
            classes = (((0, 0), 0, 9),)
        else:
            assert H % 2 == 0 and W % 2 == 0 and stride == 2
            classes = DGRAD_CLASSES
        for (py, px), t0, nt in classes:
            if stride == 1:
                conv, rowmap = (B, Ho, Wo, Co, 3, 1, 3, 3, -1, -1, Ho, Wo), None
            else:
                conv, rowmap = (B, Ho, Wo, Co, 3, 1, 1 + py, 1 + px, 0, 0, Ho, Wo), (Wo, 4, 2, py * W + px)
            # the class's taps are nt * Cout consecutive columns of the shadow's rows, from tap t0 on (bf16: 2 bytes)
            probs.append(gemm_args(dy, wd, dx, B * Ho * Wo, Ci, nt * Co, conv=conv, rowmap=rowmap, b_offset=2 * t0 * Co))

    def fill(arr, j, p):
        arr[j] = p[0]
    launch_grouped(lib.ph_gemm_grouped_bf16, _lib.GemmArgs, probs, fill, what='ph_gemm_grouped_bf16 (conv dgrad)')


def add_i64(x, value=1):
    """x (int64, contiguous) += value -- BatchNorm's num_batches_tracked counters, all layers in one launch"""
    check(lib.ph_add_i64(x.data_ptr(), x.numel(), int(value), _stream()), 'ph_add_i64')


def weighted_sum(x, weights, scale, out=None):
    """out[0] = scale * sum(x * weights) (weights None: plain sum): the batch loss"""
    if out is None:
        out = torch.empty(1, dtype=F32, device=x.device)
    check(lib.ph_weighted_sum_f32(x.data_ptr(), ptr(weights), x.numel(), float(scale), out.data_ptr(), _stream()), 'ph_weighted_sum_f32')
    return out


_ELEM_SIZE = {}


def zeros(shape, dtype, device):
    """torch.zeros through the library: an empty tensor + ONE ph_fill_zero launch (no stock torch kernel, no memset node in a captured step)."""
    if isinstance(shape, int):
        shape = (shape,)
    n = 1
    for v in shape:
        n *= int(v)
    esz = _ELEM_SIZE.get(dtype)
    if esz is None:
        esz = _ELEM_SIZE[dtype] = (torch.finfo(dtype).bits if dtype.is_floating_point else (8 if dtype == torch.bool else torch.iinfo(dtype).bits)) // 8
    nbytes = n * esz
    dev = device if isinstance(device, torch.device) else torch.device(device)
    # the fill runs on the calling thread's current stream: that stream must belong to `device` (round-5 advisor finding)
    assert dev.type != 'cuda' or dev.index is None or dev.index == torch.cuda.current_device(), 'ops.zeros: `device` is not the current device'
    pad = (nbytes + 15) // 16 * 16
    buf = torch.empty(pad, dtype=torch.uint8, device=device)              # (the caching allocator aligns to 512 B)
    check(lib.ph_fill_zero(buf.data_ptr(), pad, _stream()), 'ph_fill_zero')
    return buf[:nbytes].view(dtype).reshape(shape)


def fill_zero(t):
    """t[:] = 0 for a contiguous, 16-B aligned tensor of a multiple of 16 bytes (the flat gradient buffers): ONE ph_fill_zero launch, what a
    captured segment uses instead of Tensor.zero_() (a memset node)"""
    nbytes = t.numel() * t.element_size()
    assert t.is_contiguous() and nbytes % 16 == 0 and t.data_ptr() % 16 == 0, 'ops.fill_zero: need a contiguous 16-B aligned buffer of a multiple of 16 bytes'
    check(lib.ph_fill_zero(t.data_ptr(), nbytes, _stream()), 'ph_fill_zero')
    return t


def copy_flat(dst, src):
    """dst[:] = src for contiguous 1-D tensors of one dtype: ph_copy_bytes for the 16-B aligned body, Tensor.copy_ for a ragged tail / head"""
    assert dst.dtype == src.dtype and dst.numel() == src.numel() and dst.is_contiguous() and src.is_contiguous()
    nbytes = dst.numel() * dst.element_size()
    if nbytes == 0:
        return dst
    if (dst.data_ptr() | src.data_ptr()) & 15 or nbytes < 16:
        dst.copy_(src)
        return dst
    body = nbytes // 16 * 16
    check(lib.ph_copy_bytes(dst.data_ptr(), src.data_ptr(), body, _stream()), 'ph_copy_bytes')
    if body < nbytes:
        k = body // dst.element_size()
        dst.reshape(-1)[k:].copy_(src.reshape(-1)[k:])
    return dst


STORE_WORDS_MAX = 320


def store_words(dst0, vals0, dst1=None, vals1=()):
    """dst0[:len(vals0)] (fp32 tensor) <- floats, dst1[:len(vals1)] (int32 tensor) <- ints, carried in the arguments of one tiny kernel
    (no host-to-device copy: see ph_store_words)"""
    n0, n1 = len(vals0), len(vals1)
    assert dst0.dtype == F32 and dst0.numel() >= n0 and (n1 == 0 or (dst1.dtype == torch.int32 and dst1.numel() >= n1))
    words = struct.pack(f'{n0}f{n1}i', *vals0, *vals1)
    buf = (C.c_uint32 * (n0 + n1)).from_buffer_copy(words)
    check(lib.ph_store_words(dst0.data_ptr(), n0, ptr(dst1) if n1 else None, n1, buf, _stream()), 'ph_store_words')


def advance_seed(seed):
    check(lib.ph_advance_seed(seed.data_ptr(), _stream()), 'ph_advance_seed')


def probe_layouts(inp):
    out = torch.empty((512 + 1024,), dtype=F32, device=inp.device)
    check(lib.ph_probe_layouts(inp.data_ptr(), out.data_ptr(), _stream()), 'ph_probe_layouts')
    return out
