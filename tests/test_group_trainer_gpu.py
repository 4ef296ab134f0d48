"""n texts per image end to end (Trainer(texts_per_image=n), the drop-in heads' texts_per_image=n): one encoder pass, grouped cross-attention.

Against the REFERENCE classes on the tiled encoder output (tests/golden/base_b8_group4*.npz, minted by tests/golden/make_group_golden.py), against
this library on the tiled batch, eager against hipGraph replay, n = 1 against the plain Trainer, the heads against the Trainer, and composed with
accum_steps / max_grad_norm.  Bars are those of tests/test_parity_gpu.py and tests/test_accum_gpu.py."""
import gc
import random

import numpy as np
import pytest
import torch

from tests.golden import cases as C
from tests.golden.make_group_golden import FIXTURE, GROUP_CASE, GROUP_IMAGES, group_inputs
from tests.test_accum_gpu import _named_grads, _pin_tables, _set_seed, _store_grads
from tests.test_parity_gpu import (PROJ_SLACK, TOL_GRAD, TOL_LOSS, _check_grads_against_golden, _head, _Holder, build, math_close, set_freeze,
                                   to_dev)
from tests.util import rel_fro

pytestmark = pytest.mark.gpu


def _trainer(enc, dec, batch, tabs, n, use_graph=True, **kw):
    """Trainer(texts_per_image=n) bound to batch = (experts of Bi images, ids, mask, labels of Bi*n rows, weights); tabs: the pinned instance
    table per micro-step (one entry: every step)"""
    from prismer_amd.trainer import Trainer
    set_freeze(enc, dec)
    m = _Holder(); m.expert_encoder, m.text_decoder = enc, dec
    kw.setdefault('keep_grads', True)
    kw.setdefault('weight_decay', 0.05)
    kw.setdefault('total_steps', 10)
    if n is not None:
        kw['texts_per_image'] = n
    tr = Trainer(m, use_graph=use_graph, **kw)
    _bind(tr, batch)
    _pin_tables(tr, tabs, select=(lambda: 0) if len(tabs) == 1 else None)
    return tr, m


def _bind(tr, batch):
    x, ids, mask, labels, weights = batch
    tr.set_batch(to_dev(x), ids, mask, labels, None if weights is None else weights.cuda())


def _bn_state(enc):
    return {k: v.detach().clone() for k, v in enc.state_dict().items() if 'running_' in k or 'num_batches' in k}


# ----------------------------------------------------------------------------------------------------------------- Prismer-BASE, built once
@pytest.fixture(scope='module')
def base():
    case = C.Case(GROUP_CASE)
    enc, dec, esd, dsd = build(case, p_drop=0.1)

    def reset():
        gc.collect()
        enc.load_state_dict(esd, strict=True); dec.load_state_dict(dsd, strict=True)
        for mod in (enc, dec):
            if getattr(mod, '_store', None) is not None and mod._store.attached:
                mod._store.refresh()
        return enc, dec
    return case, reset, esd


@pytest.fixture(scope='module')
def group_step(base):
    """ONE replayed step of Trainer(texts_per_image=4) on the fixture's batch (2 images, 8 text rows), lr = 0: loss, gradients, BatchNorm buffers
    and the pixel count of every BatchNorm batch -- shared by the tests below"""
    from prismer_amd import ops
    case, reset, _ = base
    enc, dec = reset()
    x2, ids, mask, labels, n = group_inputs(case)
    assert n == 4 and GROUP_IMAGES == 2
    pixels = {}
    orig = ops.bn_apply_relu_grouped

    def spy(items, *a, **kw):
        for it in items:
            if it.get('running_var') is not None:
                pixels[it['running_var'].data_ptr()] = it['y'].shape[0]
        return orig(items, *a, **kw)
    ops.bn_apply_relu_grouped = spy
    try:
        tr, m = _trainer(enc, dec, (x2, ids, mask, labels, None), [case.instance_table(x2)], n, lr=0.0)
        _set_seed(tr, C.DROP_SEED)
        loss = tr.step()
        torch.cuda.synchronize()
    finally:
        ops.bn_apply_relu_grouped = orig
    assert tr.use_graph and tr.graphs is not None and tr.it == 1
    res = dict(loss=loss.item(), grads={k: v.clone() for k, v in _named_grads(tr).items()}, bn=_bn_state(enc),
               pixels={k: pixels[v.data_ptr()] for k, v in enc.state_dict(keep_vars=True).items() if 'running_var' in k and v.data_ptr() in pixels})
    del tr, m
    return res


def test_group_step_matches_reference_fixture(group_step):
    """hipGraph replay of Trainer(texts_per_image=4) against the reference classes on the encoder output tiled 4 times, dropout 0.1 under the same
    masks: loss, every trainable gradient (the checks of the single-step fixture tests), BatchNorm running statistics and counters after ONE
    forward on the 2 images"""
    g = C.load(FIXTURE)
    assert int(g['n']) == 4 and int(g['images']) == 2
    ref, ac = float(g['loss']), float(g['ac_loss'])
    bar = max(TOL_LOSS, 3.0 * abs(ac - ref) / ref)
    print(FIXTURE, 'loss', group_step['loss'], 'reference', ref, 'autocast yardstick', ac, 'bar', bar)
    assert math_close(group_step['loss'], ref, bar), (group_step['loss'], ref)
    _check_grads_against_golden(g, group_step['grads'], FIXTURE)
    for k, v in group_step['bn'].items():
        if 'running_' in k:
            assert rel_fro(v, torch.from_numpy(g['bn.' + k])) < 5e-3, k
        if 'num_batches' in k:
            assert int(v) == int(g['bn.' + k]) == 1


def test_group_step_equals_the_tiled_batch(base, group_step):
    """The same library on the batch of 8 with every image repeated 4 times (texts_per_image = 1), same seed, same pinned instance table: the
    same function.  Loss to TOL_LOSS; every trainable gradient through the projection check (full-tensor error estimate from C.N_PROJ
    projections against PROJ_SLACK x max(TOL_GRAD, 2 x the fixture's autocast error; stems 1.5 x), as _check_grads_against_golden); running
    means equal; running variances differ by the unbiased-count factor only: a BatchNorm batch of M pixels tiled 4 times has the same mean and
    the same biased variance v, and the running update takes v * M / (M - 1) against v * 4M / (4M - 1), so
        (rv_tiled - 0.9 rv0) / (rv_group - 0.9 rv0) = 4 (M - 1) / (4 M - 1)        (momentum 0.1, rv0 = the value before the step)."""
    case, reset, esd = base
    g = C.load(FIXTURE)
    enc, dec = reset()
    x2, ids, mask, labels, n = group_inputs(case)
    x8 = {k: ({a: b.repeat_interleave(n, 0) for a, b in v.items()} if isinstance(v, dict) else v.repeat_interleave(n, 0)) for k, v in x2.items()}
    tr, m = _trainer(enc, dec, (x8, ids, mask, labels, None), [case.instance_table(x2)], None, lr=0.0)
    _set_seed(tr, C.DROP_SEED)
    loss = tr.step().item()
    torch.cuda.synchronize()
    assert tr.texts_per_image == 1 and tr.graphs is not None
    print('tiled batch loss', loss, 'texts_per_image=4 loss', group_step['loss'])
    assert math_close(group_step['loss'], loss, TOL_LOSS)
    tiled, worst = _named_grads(tr), []
    assert sorted(tiled) == sorted(group_step['grads'])
    for name, gt in tiled.items():
        gn = gt.double().norm().item()
        if float(g['gnorm.' + name]) < 1e-4:
            continue
        e = C.projected_error(C.grad_projections(name, group_step['grads'][name]), C.grad_projections(name, gt)) / gn
        bar = PROJ_SLACK * max(TOL_GRAD, (1.5 if '.conv1.' in name else 2.0) * float(g['ac_rel.' + name]))
        worst.append((e / bar, e, name))
    worst.sort(reverse=True)
    print('texts_per_image=4 against the tiled batch: worst (err/bar, full-tensor error estimate, name)', worst[:3], 'median',
          float(np.median([w[1] for w in worst])))
    assert worst[0][0] < 1.0, worst[:4]
    bn_t, checked = _bn_state(enc), 0
    for k, v in group_step['bn'].items():
        if 'running_mean' in k:
            assert rel_fro(bn_t[k], v) < 1e-5, (k, float(rel_fro(bn_t[k], v)))
        if 'running_var' in k:
            M = group_step['pixels'].get(k)
            if M is None:
                continue
            rv0 = esd[k].cuda().float()
            want = 4.0 * (M - 1) / (4.0 * M - 1)
            ratio = ((bn_t[k] - 0.9 * rv0).double().sum() / (v - 0.9 * rv0).double().sum()).item()
            # within a tenth of the factor's distance from 1 (fp32 storage of the running value: ~1e-6 on the ratio)
            assert abs(ratio - want) < 0.1 * (1.0 - want) + 2e-6, (k, M, ratio, want)
            checked += 1
        if 'num_batches' in k:
            assert int(bn_t[k]) == int(v) == 1
    assert checked >= 6
    del tr, m


# ----------------------------------------------------------------------------------------------------------------- tiny geometry
def _tiny_group_batches(n, count=2):
    """`count` batches of 2 images and 2n text rows at the tiny case's geometry: the case's images (then image 1 twice), and as text the case's two
    rows and their row-swapped copy, alternating, image-major"""
    case = C.Case('tiny_caption')
    x, ids, mask, labels, _ = case.inputs()
    sw = torch.tensor([1, 0])
    order = torch.cat([torch.arange(2), sw] * n)[:2 * n]
    out = []
    for j in range(count):
        pick = torch.tensor([0, 1]) if j == 0 else torch.tensor([1, 1])
        xj = {k: ({a: b[pick] for a, b in v.items()} if isinstance(v, dict) else v[pick]) for k, v in x.items()}
        oj = order if j == 0 else order.flip(0)
        out.append((xj, ids[oj], mask[oj], labels[oj], None))
    return case, out


def _tiny(case, batch_list, n, p_drop=0.0, **kw):
    enc, dec, _, _ = build(case, p_drop=p_drop)
    return _trainer(enc, dec, batch_list[0], [case.instance_table(b[0]) for b in batch_list], n, **kw)


def test_group_graph_equals_eager():
    """n = 4, Bi = 2, dropout on: the first replayed step and the first eager step give the same loss, gradients, parameters, Adam moments and
    seed (the rule of test_accum_graph_equals_eager_first_group)"""
    case, bl = _tiny_group_batches(4, 1)
    res = []
    for use_graph in (False, True):
        tr, m = _tiny(case, bl, 4, p_drop=None, use_graph=use_graph, lr=1e-3)
        _set_seed(tr, 1234567)
        random.seed(99)
        loss = tr.step().item()
        torch.cuda.synchronize()
        assert (tr.graphs is not None) == use_graph and tr.it == 1
        res.append(dict(loss=loss, seed=int(tr.seed.item()), p=[st.master.clone() for st in tr.stores], g=_store_grads(tr), m=[t.clone() for t in tr.m]))
        del tr, m
    a, b = res
    assert math_close(a['loss'], b['loss'], 1e-5) and a['seed'] == b['seed'], (a['loss'], b['loss'])
    for ta, tb in zip(a['p'] + a['m'] + a['g'], b['p'] + b['m'] + b['g']):
        assert rel_fro(tb, ta) < 5e-3


class _CallSpy:
    """stands in front of ops.lib: the entry points called, in order"""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if not callable(f):
            return f

        def call(*args):
            self.names.append(name)
            return f(*args)
        return call


def test_one_text_per_image_is_the_plain_trainer():
    """Trainer(texts_per_image=1) against Trainer(): the same loss bits and the same list of library calls in an eager step"""
    from prismer_amd import ops
    case = C.Case('tiny_caption')
    batch = case.inputs()
    res = []
    for n in (None, 1):
        tr, m = _tiny(case, [batch], n, p_drop=None, use_graph=False, lr=1e-3)
        _set_seed(tr, 424242)
        spy = _CallSpy(ops.lib)
        ops.lib = spy
        try:
            loss = tr.step()
            torch.cuda.synchronize()
        finally:
            ops.lib = spy._lib
        res.append((loss.clone(), spy.names))
        del tr, m
    (la, ca), (lb, cb) = res
    assert torch.equal(la, lb), (la.item(), lb.item())
    assert len(ca) > 100 and ca == cb
    assert 'ph_attention_group_fwd' not in ca and 'ph_attention_group_bwd' not in ca


def test_caption_head_with_texts_per_image_matches_the_trainer():
    """drop-in path: PrismerCaption(experts of 2 images, 8 captions, texts_per_image=4).backward() against Trainer(texts_per_image=4) on the same
    batch (dropout off, encoder in train mode): loss and every gradient, the bars of
    test_autograd_path_dropout_masks_match_between_forward_and_backward; d(enc) reaches the encoder with 2 rows"""
    from prismer_amd import ops
    from prismer_amd.model.prismer_caption import PrismerCaption
    case, bl = _tiny_group_batches(4, 1)
    x, ids, mask, labels, _ = bl[0]
    tr, m = _tiny(case, bl, 4, use_graph=False, lr=0.0, weight_decay=0.0)
    l_nat = tr.step().item()
    g_nat = torch.cat([torch.cat([st.g(n).flatten() for n in st.names if st.is_trainable(n)]) for st in tr.stores])
    called = []
    orig = ops.attention_group_bwd
    ops.attention_group_bwd = lambda *a, **kw: (called.append(1), orig(*a, **kw))[1]
    try:
        cap = _head(PrismerCaption, case)
        loss = cap(to_dev(x), caption=(ids, mask), prefix=4, train=True, texts_per_image=4)
        loss.backward()
    finally:
        ops.attention_group_bwd = orig
    assert called, 'the autograd backward did not run the grouped cross-attention'
    assert math_close(loss.item(), l_nat, 1e-4), (loss.item(), l_nat)
    g_auto = torch.cat([torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).flatten().float()
                                   for n, p in sorted(((n, p) for n, p in mod.named_parameters() if p.requires_grad),
                                                      key=lambda t: mod._store.offset[t[0]])])
                        for mod in (cap.expert_encoder, cap.text_decoder)])
    assert g_auto.shape == g_nat.shape
    assert rel_fro(g_auto, g_nat) < 2e-3, float(rel_fro(g_auto, g_nat))
    with pytest.raises(ValueError, match='8 text rows for 2 images with texts_per_image = 2'):
        cap(to_dev(x), caption=(ids, mask), prefix=4, train=True, texts_per_image=2)
    del tr, m


def test_vqa_head_with_texts_per_image_and_row_weights_matches_the_tiled_call():
    """PrismerVQA at n = 2 with per-row weights on the tiny VQA geometry (3 images, 6 question / answer rows) against the same head on the
    images repeated twice (texts_per_image = 1): the same function (BatchNorm statistics of a batch tiled twice are those of the batch).
    Loss to TOL_LOSS, gradients to 5e-3 (the bar of the same-result comparisons of the accumulation tests)."""
    from prismer_amd.model.prismer_vqa import PrismerVQA
    case = C.Case('tiny_vqa_head')
    x = case.inputs()[0]
    q_ids, q_att, a_ids, a_att, w = case.vqa_parts()
    B, n = q_ids.shape[0], 2
    order = torch.stack([torch.arange(B), torch.arange(B).flip(0)], 1).reshape(-1)         # image b: its own row, then the mirrored row
    q2, qa2, a2, aa2 = q_ids[order], q_att[order], a_ids[order], a_att[order]
    w2 = (w[order] * torch.linspace(0.5, 1.5, B * n)).cuda()
    res = []
    for tiled in (False, True):
        vqa = _head(PrismerVQA, case)
        xx = to_dev(x)
        if tiled:
            xx = {k: ({a: b.repeat_interleave(n, 0) for a, b in v.items()} if isinstance(v, dict) else v.repeat_interleave(n, 0)) for k, v in xx.items()}
        loss = vqa(xx, (q2, qa2), (a2, aa2), weights=w2, train=True, texts_per_image=1 if tiled else n)
        loss.backward()
        res.append((loss.item(), {k: p.grad.clone() for k, p in vqa.named_parameters() if p.requires_grad and p.grad is not None}))
    (la, ga), (lb, gb) = res
    assert math_close(la, lb, TOL_LOSS), (la, lb)
    assert sorted(ga) == sorted(gb)
    flat = lambda d: torch.cat([d[k].flatten().float() for k in sorted(d)])
    assert rel_fro(flat(ga), flat(gb)) < 5e-3, float(rel_fro(flat(ga), flat(gb)))


def test_accumulation_and_guard_compose_with_texts_per_image():
    """accum_steps = 2 with texts_per_image = 2 (lr = 0, dropout off): the accumulated buffers hold the sum of the two micro-steps' gradients,
    i.e. twice their mean, to the 1e-3 floor of test_accumulation_equals_the_sum_of_its_parts; then one guarded step (max_grad_norm,
    skip_nonfinite) at n = 2 runs under graph replay and reports a finite norm"""
    case, bl = _tiny_group_batches(2, 2)
    parts = []
    for b in bl:                                                 # each micro-batch alone, accum_steps = 1
        trj, mj = _tiny(case, [b], 2, use_graph=False, lr=0.0)
        trj.step()
        parts.append(_store_grads(trj))
        del trj, mj
    tr, m = _tiny(case, bl, 2, lr=0.0, accum_steps=2)
    losses = []
    for b in bl:
        _bind(tr, b)
        losses.append(tr.step().item())
    torch.cuda.synchronize()
    assert tr.graphs is not None and sorted(tr.graphs) == ['close', 'open'] and tr.it == 1 and tr.texts_per_image == 2
    for i, st in enumerate(tr.stores):
        want = parts[0][i] + parts[1][i]
        err = rel_fro(st.grad[:st.n_train], want)
        print('store', i, 'accumulated vs sum of the two micro-steps', float(err), 'one part against the sum', float(rel_fro(parts[0][i], want)))
        assert err < 1e-3, (i, float(err))
        assert rel_fro(parts[0][i], want) > 0.1
    assert math_close(tr.group_loss.item(), float(np.mean(losses)), 1e-6)
    del tr, m
    tr, m = _tiny(case, bl[:1], 2, lr=1e-3, max_grad_norm=1.0, skip_nonfinite=True, keep_grads=False)
    loss = tr.step()
    torch.cuda.synchronize()
    assert tr.graphs is not None and np.isfinite(loss.item())
    norm = float(tr.grad_norm.item())
    assert np.isfinite(norm) and norm > 0.0 and tr.applied_updates == 1 and tr.skipped_updates == 0
