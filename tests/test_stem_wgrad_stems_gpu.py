"""GPU: the expert stems' backward with the conv weight gradients of a layer as ONE launch of the persistent k-balanced kernel
(encoder.STEM_WGRAD_GROUPED, the default) against one deferred split-K call per expert (the switch off), through the nn.Module shell and
autograd.  Geometry: BASE stems (width 768) of one dense and one label expert at batch 16 -- the smallest at which the reductions of
layers 2..4 are multiples of 64 pixels (16 x 14 x 14 = 3136) with >= 32 k-tiles AND the library's cost model puts groups of two experts on
the persistent kernel; one ViT block.

Bar: rel-Frobenius < 3e-4 between the two paths' conv weight gradients, the bar of
test_kernels_gpu.py::test_wgrad_groups_split_over_k_match_single_launches (same bf16 products, fp32 sums in another order).  That bar
is for two paths fed the SAME operands, and two runs of stems_bwd do not feed them the same: the chain above a weight gradient (BatchNorm
backward sums by float atomics, then bf16 re-rounding layer after layer) is not reproducible from run to run.  Measured on the MI355X at
this geometry, the per-expert path against ITSELF in a second run: 5e-6 (layer 4), 6e-5 (layer 3), 2.4e-4 / 2.7e-4 (layer 2),
5.8e-4 / 8.1e-4 (layer 1, which the switch does not touch); grouped against per-expert: the same figures (6e-6, 6e-5, 2.3e-4 / 2.7e-4,
5.6e-4 / 8.5e-4).  So:
  (a) inside the switched-on run every group the persistent kernel takes is ALSO computed by the per-expert calls from the very same dy
      and activations, and the two must agree within 3e-4 -- the bar applied to what it was made for;
  (b) the final gradients of the switched-on and the switched-off run must agree within 3e-4 plus the run-to-run difference of the
      per-expert path against itself (a third run), layer by layer."""
import pytest
import torch

from tests.util import rel_fro

pytestmark = pytest.mark.gpu


def _grads(grouped, monkeypatch):
    from prismer_amd import config, ops, synth
    from prismer_amd.modules.vit import VisionTransformer
    from prismer_amd.programs import encoder as E
    monkeypatch.setattr(E, 'STEM_WGRAD_GROUPED', grouped)
    taken, same_operands = [], []
    orig = ops.conv_wgrad_persistent

    def checked(items, ws=None):
        outs = orig(items, ws)
        taken.append((len(items), outs is not None))
        if outs is not None:                                      # the per-expert calls on the same operands
            ref = [ops.gemm(dy, x, trans_a=True, trans_b=True, out_f32=True, M=M, N=N, K=K, conv=conv, defer_reduce=True) for dy, x, M, N, K, conv in items]
            ops.gemm_flush_deferred()
            same_operands.extend(((it[2], it[3], it[4]), rel_fro(o, r)) for it, o, r in zip(items, outs, ref))
        return outs
    monkeypatch.setattr(ops, 'conv_wgrad_persistent', checked)
    d = config.prismer_base(experts=['depth', 'seg_coco'])
    d.vit_layers = 1
    enc = VisionTransformer(d.image_resolution, d.patch_size, d.width, d.vit_layers, d.vit_heads, dict(d.experts))
    enc.load_state_dict(synth.synth_encoder_state(d, 3))
    enc.cuda().train()
    for n, p in enc.named_parameters():
        p.requires_grad = n.startswith('conv1.') and 'rgb' not in n
    x = synth.synth_experts(d, 16, seed=21)
    x = {k: ({a: b.cuda() for a, b in v.items()} if isinstance(v, dict) else v.cuda()) for k, v in x.items()}
    out = enc(x)
    w = torch.randn(out.shape, device='cuda', generator=torch.Generator(device='cuda').manual_seed(5))
    (out.float() * w).sum().backward()
    torch.cuda.synchronize()
    g = {n: p.grad.detach().float().clone() for n, p in enc.named_parameters() if p.requires_grad and p.grad is not None and p.dim() == 4 and p.shape[-1] == 3}
    return g, taken, same_operands


def test_stems_bwd_grouped_matches_per_expert(monkeypatch):
    on, taken_on, same_operands = _grads(True, monkeypatch)
    off, taken_off, _ = _grads(False, monkeypatch)
    off2, _, _ = _grads(False, monkeypatch)
    print('grouped path: (experts in the group, persistent launch taken) per layer', taken_on)
    assert not taken_off                                          # the switch off never asks
    assert sum(1 for n, ok in taken_on if ok and n == 2) >= 3, taken_on      # layers 4, 3, 2 of both experts ran as one persistent launch each
    for shape, e in same_operands:
        print('same operands, (M, N, K) =', shape, 'grouped vs per-expert', e)
    assert len(same_operands) >= 6
    for shape, e in same_operands:
        assert e < 3e-4, (shape, e)
    names = sorted(on)
    assert len(names) == 8 and sorted(off) == names, names        # 2 experts x 4 conv layers
    errs = {n: (rel_fro(on[n], off[n]), rel_fro(off2[n], off[n])) for n in names}
    for n in names:
        print(n, tuple(on[n].shape), 'grouped vs per-expert', errs[n][0], '| per-expert vs per-expert again', errs[n][1])
    for n in names:
        assert errs[n][0] < 3e-4 + errs[n][1], (n, errs[n])
