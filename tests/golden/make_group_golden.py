"""Mint the n-texts-per-image fixture by running the REFERENCE module classes on CPU fp32 (build container only):

    python -m tests.golden.make_group_golden            # writes tests/golden/base_b8_group4*.npz

The definition of Trainer(texts_per_image=n): the reference encoder runs ONCE on the Bi images, its output is tiled n times along the batch
(repeat_interleave: image-major), the reference decoder runs on the R = Bi*n text rows, the total is the mean of the R row losses.

Case('base_b8'): the experts of its first GROUP_IMAGES = 2 samples and ALL 8 text rows (n = 4: rows 0-3 belong to image 0, rows 4-7 to image
1), 'freeze_vision', train mode (BatchNorm batch statistics of the 2 images, one running-statistics update), dropout 0.1 under the library's
masks (tests/util.LibraryDropout with C.DROP_SEED: the masks of an ordinary batch of 8 rows), random.seed(C.INSTANCE_SEED) before the encoder
call.  Weights and inputs are not stored (prismer_amd.synth regenerates them).  Keys:

  loss, row_losses [8]                                     the total and the per-row losses
  gnorm.* gsamp.* gproj.* (gfull.* for C.FULL_GRAD_KEYS)   the gradient per trainable tensor (encoder: summed over an image's rows by autograd)
  ac_loss, ac_samp.* ac_norm.* ac_rel.*                    the same computation under PyTorch's bf16 autocast (yardstick), same masks
  bn.*                                                     BatchNorm running statistics / counters after the one forward
  requires_grad                                            names joined by '\\n';  n, images
"""
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle import ref_harness as RH                     # noqa: E402
from tests.golden import cases as C                      # noqa: E402
from tests.golden.make_accum_golden import rows          # noqa: E402

GROUP_CASE, GROUP_IMAGES = 'base_b8', 2
FIXTURE = GROUP_CASE + '_group4'


def group_inputs(case, images=GROUP_IMAGES):
    """(experts of the first `images` samples, ids, mask, labels of ALL rows, n)"""
    x, ids, mask, labels, weights = case.inputs()
    assert weights is None and ids.shape[0] % images == 0
    return rows(x, 0, images), ids, mask, labels, ids.shape[0] // images


def run(name=GROUP_CASE):
    from tests.util import LibraryDropout
    case = C.Case(name)
    d = case.dims
    d.hidden_dropout_prob = d.attention_probs_dropout_prob = 0.1
    x, ids, mask, labels, n = group_inputs(case)
    out = {}

    def once(autocast):
        esd, dsd = case.weights()
        enc, dec = RH.build_reference(d, esd, dsd)
        holder = RH.reference_freeze(enc, dec, 'freeze_vision')
        enc.train()
        drop = LibraryDropout(C.DROP_SEED, d.hidden_dropout_prob, d.attention_probs_dropout_prob)
        RH.patch_dropout(dec, lambda site, t: drop(site, t))
        params = [(nm, p) for nm, p in holder.named_parameters() if p.requires_grad]
        random.seed(C.INSTANCE_SEED)
        with (torch.autocast('cpu', dtype=torch.bfloat16) if autocast else torch.autocast('cpu', enabled=False)):
            e = enc(x)                                                             # [S, Bi, Hv]: ONE encoder pass
            tiled = e.permute(1, 0, 2).repeat_interleave(n, 0)                     # [Bi*n, S, Hv], image-major
            o = dec(ids, attention_mask=mask, encoder_hidden_states=tiled, labels=labels, return_dict=True)
            row_losses = o.loss.float()
            loss = row_losses.mean()
        loss.backward()
        print(f'{FIXTURE} autocast={autocast}: loss {float(loss):.6f}', flush=True)
        return float(loss.detach()), row_losses.detach(), {nm: p.grad.detach().clone() for nm, p in params}, enc

    loss, row_losses, grads, enc = once(False)
    out['loss'], out['row_losses'] = np.float64(loss), row_losses.numpy().astype(np.float64)
    out['n'], out['images'] = np.int64(n), np.int64(GROUP_IMAGES)
    for key, v in enc.state_dict().items():
        if 'running_' in key or 'num_batches' in key:
            out['bn.' + key] = v.numpy().copy()
    for nm, g in grads.items():
        out['gnorm.' + nm] = np.float64(g.double().norm().item())
        out['gsamp.' + nm] = g.flatten()[C.sample_idx(nm, g.numel())].numpy()
        out['gproj.' + nm] = C.grad_projections(nm, g)
        if nm in C.FULL_GRAD_KEYS:
            out['gfull.' + nm] = g.numpy()
    out['requires_grad'] = np.array('\n'.join(grads))
    ac_loss, _, ac_grads, _ = once(True)
    out['ac_loss'] = np.float64(ac_loss)
    for nm, g in ac_grads.items():
        gn = float(out['gnorm.' + nm])
        sm = g.flatten()[C.sample_idx(nm, g.numel())].float().numpy()
        out['ac_samp.' + nm] = np.float64(np.linalg.norm(sm - out['gsamp.' + nm]) / (np.linalg.norm(out['gsamp.' + nm]) + 1e-30))
        out['ac_norm.' + nm] = np.float64(abs(g.double().norm().item() - gn) / (gn + 1e-30))
        out['ac_rel.' + nm] = np.float64((g.double() - grads[nm].double()).norm().item() / (gn + 1e-30))
    paths = C.save(FIXTURE, out)
    print(f'{FIXTURE}: wrote {paths} ({sum(os.path.getsize(p) for p in paths) / 1e6:.2f} MB)  loss={loss}  autocast loss={ac_loss}')


if __name__ == '__main__':
    assert RH.available(), 'reference not mounted'
    torch.set_num_threads(int(os.environ.get('GOLDEN_THREADS', os.cpu_count())))
    run()
