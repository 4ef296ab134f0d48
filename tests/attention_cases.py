"""The case table and the inputs shared by test_attention_emulation_cpu.py and test_attention_rows_gpu.py.

Inputs are drawn on the CPU (one generator per case) and live where production keeps them: q, k and v are the column slices [:, W:2W],
[:, 2W:3W] and [:, 3W:4W] (W = H * dh) of one [B * S + 8, 5W] bf16 buffer, token stride 5W, batch stride S * 5W; when Sq != Sk the queries
have such a buffer of their own.  The 8 spare rows and the two outer column blocks are what a stray write would land in.
"""
import torch

from tests.util import attn_emulated, attn_live, attn_ref64, dropout_keep_attention, lse_floor32, row_err

BF = torch.bfloat16
SEED, STREAM = 4242, 11
SPARE_ROWS = 8

ROW_CASES = [  # B, H, Sq, Sk, dh, causal, masked, drop
    (1, 2, 520, 136, 64, False, False, 0.0),     # dQ kernel with 32 queries per wave (Sq >= 512); 520 = 4 * 128 + 8: the last block has one wave with 8 live rows
    (1, 2, 136, 530, 64, False, False, 0.0),     # dK/dV kernel with 32 keys per wave (Sk >= 512), ragged last block
    (1, 1, 520, 530, 32, False, False, 0.0),     # both 32-per-wave kernels at head dim 32
    (2, 2, 70, 130, 96, True, True, 0.1),        # masked streaming kernels, head dim 96
    (2, 2, 70, 130, 32, True, True, 0.1),        # masked streaming kernels, head dim 32
    (2, 2, 70, 130, 128, True, True, 0.1),       # masked streaming kernels, head dim 128, with the causal cut
    (1, 11, 130, 70, 32, False, False, 0.0),     # block_xy(): 8 re-mapped heads + 3 in plain order, 3 query blocks per head
    (1, 11, 130, 70, 64, False, False, 0.0),     # the same through the head-resident (default) and the streaming kernels
    (3, 4, 30, 30, 64, True, True, 0.1),         # decoder self-attention as trained (small-query backward, streaming forward)
    (2, 12, 30, 260, 64, False, False, 0.1),     # decoder cross-attention at BASE geometry
    (2, 4, 40, 40, 64, True, True, 0.1),         # VQA length: streaming kernels on both sides
    (2, 3, 260, 260, 64, False, False, 0.0),     # ViT, head-resident
    (1, 3, 100, 272, 64, False, False, 0.0),     # the longest head-resident key sequence
    (2, 3, 280, 150, 64, False, False, 0.0),     # plain streaming, ragged on both sides
    (2, 8, 64, 300, 160, False, False, 0.0),     # HUGE resampler head dim
    (2, 2, 17, 320, 64, False, True, 0.2),       # the largest small-query key image
]

TENSORS = ('o', 'dq', 'dk', 'dv')


def case_id(case):
    B, H, Sq, Sk, dh, causal, masked, p = case
    return f'{B}x{H}x{Sq}x{Sk}x{dh}' + ('-causal' if causal else '') + ('-mask' if masked else '') + (f'-p{p}' if p > 0 else '')


def routes(Sq, Sk, dh, plain):
    """ph_attention_tuning() arguments a shape is run with: None = default, 0 = streaming kernels where the default takes the small-query
    kernels, 2 = streaming kernels where the default takes the head-resident ones (the dispatch of csrc/attention.hip)"""
    r = [None]
    if dh == 64 and Sq <= 32 and Sk <= 320:
        r.append(0)
    if dh == 64 and plain and 32 < Sq <= 272 and Sk <= 272:
        r.append(2)
    return r


def default_key_mask(B, Sk):
    """right padding of another length per batch entry (the mask of test_attention)"""
    km = torch.ones(B, Sk, dtype=torch.uint8)
    for b in range(B):
        km[b, Sk - 3 - 2 * b:] = 0
    return km


class Inputs:
    """CPU tensors of one case.  qbuf / kvbuf: the packed bf16 buffers (the same object when Sq == Sk); d_o: [B * Sq, W] bf16."""

    def __init__(self, B, H, Sq, Sk, dh, seed=0):
        self.B, self.H, self.Sq, self.Sk, self.dh = B, H, Sq, Sk, dh
        self.W = W = H * dh
        g = torch.Generator(device='cpu').manual_seed(1000 + seed + B + 3 * H + 5 * Sq + 7 * Sk + 11 * dh)
        self.kvbuf = torch.randn(B * Sk + SPARE_ROWS, 5 * W, generator=g).to(BF)
        self.qbuf = self.kvbuf if Sq == Sk else torch.randn(B * Sq + SPARE_ROWS, 5 * W, generator=g).to(BF)
        self.d_o = torch.randn(B * Sq, W, generator=g).to(BF)

    def heads(self, device='cpu'):
        """q, k, v, d_o as [B, H, S, dh] float64 on `device` (the values the kernels read)"""
        B, H, Sq, Sk, dh, W = self.B, self.H, self.Sq, self.Sk, self.dh, self.W
        q = to_heads(self.qbuf[:B * Sq, W:2 * W], B, H, Sq, dh, device)
        k = to_heads(self.kvbuf[:B * Sk, 2 * W:3 * W], B, H, Sk, dh, device)
        v = to_heads(self.kvbuf[:B * Sk, 3 * W:4 * W], B, H, Sk, dh, device)
        return q, k, v, to_heads(self.d_o, B, H, Sq, dh, device)


def to_heads(x2d, B, H, S, dh, device='cpu'):
    """[B * S, H * dh] -> [B, H, S, dh] float64"""
    return x2d.to(device).double().reshape(B, S, H, dh).transpose(1, 2).contiguous()


def token_rows(x):
    """[B, H, S, dh] -> [B * S, H * dh]: the 2-D layout of the buffers, whose rows row_err() judges"""
    B, H, S, dh = x.shape
    return x.transpose(1, 2).reshape(B * S, H * dh)


def keep_mask(B, H, Sq, Sk, p):
    return dropout_keep_attention(B * H, Sq, Sk, SEED, STREAM, p).reshape(B, H, Sq, Sk) if p > 0 else None


class Reference:
    """attn_ref64, attn_emulated and what the bounds are made of, computed once per case on `device`"""

    def __init__(self, case, device='cpu', key_mask=None, backward=True, inputs=None):
        B, H, Sq, Sk, dh, causal, masked, p = case
        self.case, self.device = case, device
        self.inp = inputs if inputs is not None else Inputs(B, H, Sq, Sk, dh)
        self.key_mask = key_mask if key_mask is not None else (default_key_mask(B, Sk) if masked else None)
        self.scale = dh ** -0.5
        self.q, self.k, self.v, d_o = self.inp.heads(device)
        self.d_o = d_o if backward else None
        keep = keep_mask(B, H, Sq, Sk, p)
        self.keep = keep.to(device) if keep is not None else None
        self.p = p
        self.live = attn_live(B, H, Sq, Sk, self.key_mask, causal, device)
        self.ref = attn_ref64(self.q, self.k, self.v, self.d_o, self.scale, keep=self.keep, p=p, live=self.live)
        self.emu = attn_emulated(self.q, self.k, self.v, self.d_o, self.scale, keep=self.keep, p=p, live=self.live)
        self.lse_floor = lse_floor32(self.q, self.k, self.scale, self.live)

    def floor(self, name, sel=None):
        """row_err(emulated, ref64) of one tensor; sel = batch entries to judge (None = all)"""
        e, r = self.emu[name], self.ref[name]
        if sel is not None:
            e, r = e[sel], r[sel]
        return row_err(token_rows(e), token_rows(r))
