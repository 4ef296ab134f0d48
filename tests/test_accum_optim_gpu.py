"""Gradient accumulation in the REFERENCE-style loop on the drop-in modules:
    for j in 1..k: (model(experts_j, caption_j, prefix=...) / k).backward();  optimizer.step();  optimizer.zero_grad()
Every backward hands autograd views of a FRESH flat gradient buffer; the first one becomes Parameter.grad, autograd adds the later ones into it
tensor by tensor, in place -- so the gradients keep aliasing one flat buffer in layout order and prismer_amd.optim.AdamW stays on its fused path
(one launch per store).  Pinned here, together with the update torch.optim.AdamW gives."""
import pytest
import torch

from tests.golden import cases as C
from tests.test_parity_gpu import _head, to_dev

pytestmark = pytest.mark.gpu

K = 2


def _model():
    from prismer_amd.model.prismer_caption import PrismerCaption
    case = C.Case('tiny_caption')
    m = _head(PrismerCaption, case)
    x, ids, mask, _, _ = case.inputs()
    x = to_dev(x)

    def pick(t, idx):
        if isinstance(t, dict):
            return {k: pick(v, idx) for k, v in t.items()}
        return t[idx]
    mbs = [(pick(x, torch.tensor(idx).cuda()), (ids[idx], mask[idx])) for idx in ([0, 1], [1, 1])]
    return m, mbs


def _accum_update(m, opt, mbs):
    losses = []
    for x, cap in mbs:
        loss = m(x, caption=cap, prefix=4, train=True)
        (loss / K).backward()
        losses.append(loss.item())
    return losses


def test_accumulated_reference_loop_stays_fused_and_equals_torch_adamw_on_the_same_gradients():
    """two accumulated updates; a twin set of plain tensors takes torch.optim.AdamW steps on COPIES of the very same accumulated gradients
    (isolates the optimizer from the backward's atomics noise, as tests/test_optim_gpu.py does)"""
    from prismer_amd.optim import AdamW
    m, mbs = _model()
    params = [p for p in m.parameters() if p.requires_grad]
    twin = [torch.nn.Parameter(p.detach().clone()) for p in params]
    opt, ref = AdamW(params, lr=1e-4, weight_decay=0.05), torch.optim.AdamW(twin, lr=1e-4, weight_decay=0.05)
    for u in range(2):
        opt.zero_grad()
        _accum_update(m, opt, mbs)
        for st in (m.expert_encoder._store, m.text_decoder._store):
            names = [n for n in st.names if n in st.trainable]
            assert AdamW._aliased_flat_grad(st, names) is not None            # the k backwards left ONE flat buffer per store behind the .grad views
        for p, q in zip(params, twin):
            q.grad = p.grad.detach().clone()
        opt.step(); ref.step()
        assert opt.fused_launches == 2 and opt.plain_updates == 0, (u, opt.fused_launches, opt.plain_updates)
        for p, q in zip(params, twin):
            assert (p - q).abs().max().item() <= 2e-6 + 1e-6 * q.abs().max().item(), (u, (p - q).abs().max().item())
    for st in (m.expert_encoder._store, m.text_decoder._store):
        assert torch.equal(st.shadow[:st.n_train], st.master[:st.n_train].bfloat16())


def test_accumulated_reference_loop_tracks_torch_adamw():
    """the same loop on two models, one per optimizer: first micro losses equal, the loss curve inside 2e-3 (the bar of tests/test_optim_gpu.py),
    and the accumulated gradient is the mean of the parts (one backward per micro-batch alone, on a third model)"""
    from prismer_amd.optim import AdamW
    ma, mbs = _model()
    mb_, _ = _model()
    oa = torch.optim.AdamW([p for p in ma.parameters() if p.requires_grad], lr=1e-4, weight_decay=0.05)
    ob = AdamW([p for p in mb_.parameters() if p.requires_grad], lr=1e-4, weight_decay=0.05)
    la, lb = [], []
    for u in range(3):
        oa.zero_grad(); ob.zero_grad()
        la += _accum_update(ma, oa, mbs); lb += _accum_update(mb_, ob, mbs)
        if u == 0:
            mc, _ = _model()
            parts = []
            for x, cap in mbs:
                mc.zero_grad()
                mc(x, caption=cap, prefix=4, train=True).backward()
                parts.append([p.grad.detach().clone() for p in mc.parameters() if p.requires_grad])
            num = den = 0.0
            for p, g0, g1 in zip([p for p in mb_.parameters() if p.requires_grad], *parts):
                num += float(((g0 + g1) / K - p.grad).double().pow(2).sum()); den += float(p.grad.double().pow(2).sum())
            assert (num / den) ** 0.5 < 1e-3, (num / den) ** 0.5
        oa.step(); ob.step()
        assert ob.fused_launches == 2 and ob.plain_updates == 0
    assert la[:K] == lb[:K]
    for a, b in zip(la, lb):
        assert abs(a - b) <= 2e-3 * abs(a), (la, lb)
    assert la[-1] < la[1] and la[-2] < la[0]
