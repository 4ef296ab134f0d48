"""CPU: n texts per image -- ABI of the grouped cross-attention entry points, their argument validation without a GPU, and the host logic
of the option (row / image validation, refusals, the d(total)/d(loss) scale, the statement of the semantics in torch)."""
import ctypes as C
import os
import subprocess
import tempfile
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1


def _lib():
    from prismer_amd import build
    build.build(verbose=False)
    from prismer_amd import _lib as L
    return L


def test_entry_points_are_declared_and_bound():
    import re
    L = _lib()
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'prismer_hip.h')).read(), flags=re.S)
    for s in ('ph_attention_group_fwd', 'ph_attention_group_bwd', 'ph_attention_group_ws_bytes'):
        assert re.search(r'\b%s\s*\(' % s, src), f'{s} not declared in prismer_hip.h'
        assert s in L.EXPORTS and hasattr(L.lib, s)
    assert 'ph_attn_group_fwd_args' in src and 'ph_attn_group_bwd_args' in src
    assert L.lib.ph_version() == L.ABI_VERSION == 106              # additive: the revision and the existing structs stay


def test_group_structs_match_header():
    L = _lib()
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "prismer_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(ph_attn_group_fwd_args), sizeof(ph_attn_group_bwd_args), offsetof(ph_attn_group_fwd_args, group),
         offsetof(ph_attn_group_fwd_args, ws), offsetof(ph_attn_group_fwd_args, ws_bytes), offsetof(ph_attn_group_bwd_args, group),
         offsetof(ph_attn_group_bwd_args, ws), offsetof(ph_attn_group_bwd_args, ws_bytes));
  return 0;
}'''
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, 't.c'), os.path.join(td, 't')
        open(src, 'w').write(prog)
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), src, '-o', exe])
        out = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    F, B = L.AttnGroupFwdArgs, L.AttnGroupBwdArgs
    assert out == [C.sizeof(F), C.sizeof(B), F.group.offset, F.ws.offset, F.ws_bytes.offset, B.group.offset, B.ws.offset, B.ws_bytes.offset]
    assert F.f.offset == 0 and B.b.offset == 0 and C.sizeof(L.AttnFwdArgs) == F.group.offset and C.sizeof(L.AttnBwdArgs) == B.group.offset


def _good_fwd(L, R=6, group=3):
    g = L.AttnGroupFwdArgs()
    f = g.f
    f.q = f.k = f.v = f.o = 16
    f.B, f.H, f.Sq, f.Sk, f.dh = R, 2, 30, 260, 64
    f.q_ts = f.k_ts = f.v_ts = f.o_ts = 128
    f.q_bs = f.o_bs = 30 * 128
    f.k_bs = f.v_bs = 260 * 128
    f.scale = 0.125
    f.lse = 16
    g.group = group
    return g


def _good_bwd(L, R=6, group=3):
    g = L.AttnGroupBwdArgs()
    g.b.f = _good_fwd(L, R, group).f
    b = g.b
    b.d_o = b.dq = b.dk = b.dv = 16
    b.do_ts = b.dq_ts = b.dk_ts = b.dv_ts = 128
    b.do_bs = b.dq_bs = 30 * 128
    b.dk_bs = b.dv_bs = 260 * 128
    g.group = group
    return g


@pytest.mark.parametrize('which', ['fwd', 'bwd'])
def test_argument_validation_without_gpu(which):
    """every bad argument is PH_ERR_BAD_ARG with a message, before any launch (there is no GPU here: a launch would fail differently)"""
    L = _lib()
    make = _good_fwd if which == 'fwd' else _good_bwd
    entry = L.lib.ph_attention_group_fwd if which == 'fwd' else L.lib.ph_attention_group_bwd
    fwd_of = (lambda g: g.f) if which == 'fwd' else (lambda g: g.b.f)

    def rejected(g, text):
        rc = entry(C.byref(g), None)
        assert rc == BAD_ARG and text in L.lib.ph_last_error(), (rc, L.lib.ph_last_error())
    assert entry(None, None) == BAD_ARG
    g = make(L); g.group = 0
    rejected(g, b'group = 0')
    g = make(L); g.group = -2
    rejected(g, b'group = -2')
    g = make(L, R=7, group=3)
    rejected(g, b'not a multiple of group')
    g = make(L); fwd_of(g).causal = 1
    rejected(g, b'no causal cut and no key mask')
    g = make(L); fwd_of(g).key_mask = 16
    rejected(g, b'no causal cut and no key mask')
    for name in ('q', 'k', 'v', 'o'):
        g = make(L); setattr(fwd_of(g), name, 24)
        rejected(g, b'16-B aligned')
    g = make(L); fwd_of(g).k_bs = 260 * 128 + 4
    rejected(g, b'multiples of 8')
    g = make(L); fwd_of(g).dh = 48
    rejected(g, b'head dim 48')
    if which == 'bwd':
        for name in ('d_o', 'dq', 'dk', 'dv'):
            g = make(L); setattr(g.b, name, 24)
            rejected(g, b'16-B aligned')
        g = make(L); g.b.dk = None
        rejected(g, b'null pointer')
        g = make(L); g.b.dk_bs = 260 * 128 + 4
        rejected(g, b'multiples of 8')
    # outside the grouped kernels the tiled route needs its workspace: refused before anything is launched
    g = make(L); fwd_of(g).Sq = 40
    f = fwd_of(g)
    assert L.lib.ph_attention_group_ws_bytes(C.byref(f), 3, int(which == 'bwd')) == (4 if which == 'bwd' else 2) * 6 * 260 * 128 * 2
    rejected(g, b'workspace')
    assert L.lib.ph_attention_group_ws_bytes(C.byref(make(L).f if which == 'fwd' else make(L).b.f), 3, 1) == 0
    assert L.lib.ph_attention_group_ws_bytes(C.byref(make(L).f if which == 'fwd' else make(L).b.f), 17, 1) > 0      # group > 16


def test_decoder_program_refuses_rows_that_are_no_multiple_of_the_images():
    from prismer_amd.programs.decoder import DecoderProgram
    assert DecoderProgram.texts_per_image(8, 2) == 4 and DecoderProgram.texts_per_image(3, 3) == 1
    with pytest.raises(ValueError, match='8 text rows'):
        DecoderProgram.texts_per_image(8, 3)
    prog = object.__new__(DecoderProgram)
    prog.d = types.SimpleNamespace(hidden_size=64, num_attention_heads=1)
    ids = torch.zeros(8, 5, dtype=torch.long)
    with pytest.raises(ValueError, match='8 text rows'):
        prog.forward(ids, torch.ones_like(ids), torch.zeros(3, 7, 64), None, None, False)
    with pytest.raises(ValueError):
        prog.forward(ids, torch.ones_like(ids), torch.zeros(16, 7, 64), None, None, False)


def test_module_forward_refuses_a_row_image_mismatch():
    from prismer_amd import config
    from prismer_amd.model.prismer import _Cfg
    from prismer_amd.modules.roberta import RobertaForCausalLMModified
    d = config.prismer_tiny()
    dec = RobertaForCausalLMModified(_Cfg(d.roberta_config_dict()))
    ids = torch.zeros(8, 5, dtype=torch.long)
    with pytest.raises(ValueError, match='8 text rows'):
        dec(input_ids=ids, attention_mask=torch.ones_like(ids), encoder_hidden_states=torch.zeros(3, 4, d.vision_hidden_size), labels=ids)
    with pytest.raises(RuntimeError, match='HIP path'):           # a valid n = 4 gets as far as the device check
        dec(input_ids=ids, attention_mask=torch.ones_like(ids), encoder_hidden_states=torch.zeros(2, 4, d.vision_hidden_size), labels=ids)


def test_trainer_option_validation():
    from prismer_amd import trainer as T
    assert T.check_texts_per_image(1) == 1 and T.check_texts_per_image(5) == 5
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match='texts_per_image'):
            T.check_texts_per_image(bad)
    with pytest.raises(ValueError, match='micro_batches'):
        T.check_texts_per_image(2, side_stream=True, micro_batches=2)
    assert T.check_texts_per_image(1, side_stream=True, micro_batches=2) == 1
    with pytest.raises(ValueError, match='micro_batches'):       # the constructor refuses before it touches the model
        T.Trainer(None, side_stream=True, micro_batches=2, texts_per_image=2)
    with pytest.raises(ValueError, match='texts_per_image'):
        T.Trainer(None, texts_per_image=0)


def test_set_batch_validates_image_rows_against_text_rows():
    from prismer_amd import trainer as T
    tr = object.__new__(T.Trainer)
    tr.texts_per_image = 4
    tr.static, tr._staged = {}, False                          # (prefetch_batch: a first batch is bound, nothing staged)
    ids = torch.zeros(8, 5, dtype=torch.long)
    experts = {'rgb': torch.zeros(3, 3, 8, 8), 'depth': torch.zeros(3, 1, 8, 8)}
    with pytest.raises(ValueError, match='8 text rows for 3 images with texts_per_image = 4'):
        tr.set_batch(experts, ids, ids, ids)
    with pytest.raises(ValueError, match='prefetch_batch: 8 text rows for 3 images'):
        tr.prefetch_batch(experts, ids, ids, ids)
    tr.texts_per_image = 1
    with pytest.raises(ValueError, match='8 text rows for 3 images with texts_per_image = 1'):
        tr.set_batch(experts, ids, ids, ids)
    T.check_text_rows(2, 8, 4)
    assert T._image_rows({'seg_coco': {'label_map': torch.zeros(5, 1, 4, 4)}}) == 5


def test_dloss_scale():
    from prismer_amd import trainer as T
    d = T.dloss_rows(2, 4)
    assert d.shape == (8,) and d.dtype == torch.float32 and bool((d == torch.tensor(1.0 / 8)).all())
    w = torch.tensor([1.0, 0.5, 0.0, 2.0, 1.0, 1.0, 0.25, 3.0])
    assert torch.equal(T.dloss_rows(2, 4, w), w / 8)
    assert torch.equal(T.dloss_rows(8, 1), torch.full((8,), 1.0 / 8))          # n = 1: what it was
    # d(mean(w * loss)) / d(loss_r) in autograd
    loss = torch.randn(8, requires_grad=True)
    (w * loss).mean().backward()
    assert torch.allclose(loss.grad, T.dloss_rows(2, 4, w))


def test_semantics_tiled_encoder_output_gives_the_member_sum():
    """The definition of the feature in torch: the decoder runs on the encoder output tiled n times (repeat_interleave, image-major); autograd
    through the tiling gives d(enc) of an image = the sum over its n rows of the per-row gradients."""
    torch.manual_seed(0)
    Bi, n, S, Hv, T = 3, 4, 5, 8, 6
    enc = torch.randn(Bi, S, Hv, requires_grad=True)
    q = torch.randn(Bi * n, T, Hv)
    wv = torch.randn(Hv, Hv)

    def rows_loss(e):                                            # a cross-attention-shaped function of [R, S, Hv] -> [R]
        p = torch.softmax(q @ e.transpose(1, 2) / Hv ** 0.5, -1)
        return ((p @ (e @ wv)) ** 2).mean((1, 2))
    tiled = enc.repeat_interleave(n, 0)
    assert torch.equal(tiled[5], enc[1]) and torch.equal(tiled[4], enc[1]) and torch.equal(tiled[3], enc[0])     # row r reads image r // n
    w = torch.rand(Bi * n)
    (w * rows_loss(tiled)).mean().backward()
    g_shared = enc.grad.clone()
    t2 = enc.detach().repeat_interleave(n, 0).requires_grad_(True)
    (w * rows_loss(t2)).mean().backward()
    assert torch.allclose(g_shared, t2.grad.reshape(Bi, n, S, Hv).sum(1), rtol=1e-5, atol=1e-7)
