"""Gradient accumulation in the native Trainer (Trainer(accum_steps=k)): k consecutive step() calls form one group, each a forward + backward on
its own micro-batch (own BatchNorm batch statistics, dropout masks, instance draws), the k-th ending in ONE AdamW update with the group's mean
gradient -- against the REFERENCE classes running the same loop (tests/golden/base_b8_accum*.npz, minted by tests/golden/make_accum_golden.py),
against the k = 1 path, eager against hipGraph replay, across an interrupted group, and in peak memory.  Bars are those of tests/test_parity_gpu.py."""
import gc
import random

import numpy as np
import pytest
import torch

from tests.golden import cases as C
from tests.golden.make_accum_golden import ACCUM_CASE, ACCUM_K, ACCUM_UPDATES, FIXTURE, micro_batches
from tests.test_parity_gpu import PROJ_SLACK, TOL_LOSS, _check_grads_against_golden, _Holder, build, math_close, set_freeze, to_dev
from tests.util import rel_fro

pytestmark = pytest.mark.gpu


def _pin_tables(tr, tabs, select=None):
    """the instance table of micro-step j (or of batch select()) pinned the way test_parity_gpu._pinned_trainer pins the batch's"""
    orig = tr._host_prologue

    def prologue():
        j = tr.micro_index if select is None else select()
        orig()
        if tabs[j] is not None:
            tr.table.copy_(torch.tensor(tabs[j], dtype=torch.int32))
    tr._host_prologue = prologue


def _bind(tr, mb):
    x, ids, mask, labels, weights = mb
    tr.set_batch(to_dev(x), ids, mask, labels, None if weights is None else weights.cuda())


def _trainer(case, enc, dec, mbs, k, use_graph=True, select=None, **kw):
    """Trainer(accum_steps=k) over the micro-batches `mbs` (micro-step j binds mbs[j] and its own pinned instance table)"""
    from prismer_amd.trainer import Trainer
    set_freeze(enc, dec)
    m = _Holder(); m.expert_encoder, m.text_decoder = enc, dec
    kw.setdefault('keep_grads', True)
    kw.setdefault('weight_decay', 0.05)
    kw.setdefault('total_steps', 10)
    tr = Trainer(m, use_graph=use_graph, accum_steps=k, **kw)
    _bind(tr, mbs[0])
    _pin_tables(tr, [case.instance_table(mb[0]) for mb in mbs], select)
    return tr, m


def _group(tr, mbs):
    losses = []
    for mb in mbs:
        _bind(tr, mb)
        losses.append(tr.step())
    return losses


def _named_grads(tr):
    named = {}
    for pref, st in (('expert_encoder.', tr.stores[0]), ('text_decoder.', tr.stores[1])):
        for nm in st.names:
            if st.is_trainable(nm):
                named[pref + nm] = st.g(nm).detach()
    return named


def _set_seed(tr, seed):
    tr.seed.copy_(torch.tensor([seed - (1 << 64) if seed >= (1 << 63) else seed], dtype=torch.int64))


# ----------------------------------------------------------------------------------------------------------------- Prismer-BASE, built once
@pytest.fixture(scope='module')
def base():
    case = C.Case(ACCUM_CASE)
    enc, dec, esd, dsd = build(case, p_drop=0.1)

    def reset():
        gc.collect()
        enc.load_state_dict(esd, strict=True); dec.load_state_dict(dsd, strict=True)
        for mod in (enc, dec):
            if getattr(mod, '_store', None) is not None and mod._store.attached:
                mod._store.refresh()
        return enc, dec
    return case, reset


def test_accumulated_gradient_matches_reference_loop(base):
    """update 1 of the fixture under hipGraph replay (accum_steps = 2, opening + closing graph): the two micro losses, and the gradient buffers
    after micro-step 2 -- the plain fp32 SUM over the group, divided by k here -- against sum_j g_j / k of the reference loop, per tensor, through
    the checks of the single-step fixture tests (norm, sampled entries, 16 projections, full tensors; autocast yardsticks from the fixture)"""
    case, reset = base
    g = C.load(FIXTURE)
    k = int(g['k'])
    assert (k, int(g['updates'])) == (ACCUM_K, ACCUM_UPDATES) == (2, 2)
    enc, dec = reset()
    mbs = micro_batches(case, k)
    tr, m = _trainer(case, enc, dec, mbs, k, lr=C.TRAJ_LR, keep_grads=True)
    _set_seed(tr, C.DROP_SEED)
    losses = [l.item() for l in _group(tr, mbs)]
    torch.cuda.synchronize()
    assert tr.use_graph and tr.graphs is not None and sorted(tr.graphs) == ['close', 'open'] and tr.it == 1 and tr.micro_index == 0
    ref, ac = g['losses'], g['ac_losses']
    print(FIXTURE, 'micro losses', losses, 'reference', ref[:k].tolist(), 'autocast yardstick', ac[:k].tolist(), 'group loss', tr.group_loss.item())
    for j in range(k):
        bar = max(TOL_LOSS, 3.0 * abs(ac[j] - ref[j]) / ref[j])
        assert math_close(losses[j], float(ref[j]), bar), (j, losses[j], float(ref[j]))
    assert math_close(tr.group_loss.item(), float(np.mean(losses)), 1e-6)
    _check_grads_against_golden(g, {n: t / k for n, t in _named_grads(tr).items()}, FIXTURE + ' update 1')
    del tr, m


def test_accumulated_trajectory_matches_reference_loop(base):
    """all U k micro-steps of the fixture under hipGraph replay, keep_grads=False (the bench's gradient handling: AdamW re-zeroes, the opening
    micro-step overwrites the single-writer outputs): loss curve, displacement p_U - p_0 of every trainable tensor under the bars of
    test_trainer_hipgraph_trajectory_matches_reference_loop, BatchNorm running statistics after U k forwards, counters == U k, it == U"""
    case, reset = base
    g = C.load(FIXTURE)
    k, U = int(g['k']), int(g['updates'])
    enc, dec = reset()
    mbs = micro_batches(case, k)
    tr, m = _trainer(case, enc, dec, mbs, k, lr=C.TRAJ_LR, keep_grads=False)
    assert (C.TRAJ_LR, C.TRAJ_MIN_LR, C.TRAJ_WD, C.TRAJ_TOTAL) == (5e-5, 0.0, 0.05, 10) and tr.total_steps == C.TRAJ_TOTAL and tr.wd == C.TRAJ_WD
    _set_seed(tr, C.DROP_SEED)
    p0 = [st.master.clone() for st in tr.stores]
    losses = []
    for u in range(U):
        for mb in mbs:
            _bind(tr, mb)
            losses.append(tr.step().item())
        assert tr.it == u + 1 and tr.micro_index == 0
    torch.cuda.synchronize()
    assert tr.use_graph and tr.graphs is not None and tr._exclusive is not None and len(tr._exclusive) > 50
    ref, ac = g['losses'], g['ac_losses']
    print(FIXTURE, 'micro losses', losses, 'reference', ref.tolist(), 'autocast yardstick', ac.tolist(), 'group loss', tr.group_loss.item())
    for i in range(U * k):
        bar = max(TOL_LOSS, 3.0 * abs(ac[i] - ref[i]) / ref[i])
        assert math_close(losses[i], float(ref[i]), bar), (i, losses[i], float(ref[i]))
    gl_ref, gl_ac = float(np.mean(ref[-k:])), float(np.mean(ac[-k:]))
    assert math_close(tr.group_loss.item(), gl_ref, max(TOL_LOSS, 3.0 * abs(gl_ac - gl_ref) / gl_ref))
    trainable = str(g['requires_grad']).split('\n')
    rws = []
    for pref, st, before in (('expert_encoder.', tr.stores[0], p0[0]), ('text_decoder.', tr.stores[1], p0[1])):
        for nm in st.names:
            if not st.is_trainable(nm):
                continue
            n = pref + nm
            assert n in trainable
            dn = float(g['dnorm.' + n])
            if dn < 1e-6:
                continue
            o = st.offset[nm]
            delta = st.master[o:o + st.numel[nm]] - before[o:o + st.numel[nm]]
            e = C.projected_error(C.grad_projections(n, delta), g['dproj.' + n]) / dn
            bar = PROJ_SLACK * max(0.15, 2.0 * float(g['ac_drel.' + n]))
            rws.append((e / bar, e, float(g['ac_drel.' + n]), abs(delta.double().norm().item() - dn) / dn, n))
    rws.sort(reverse=True)
    med = float(np.median([r[1] for r in rws]))
    print(FIXTURE, 'displacement after', U, 'updates: worst (err/bar, full-tensor error estimate, autocast error, norm error, name)', rws[:3], 'median', med,
          'autocast median', float(np.median([r[2] for r in rws])))
    assert rws[0][0] < 1.0, rws[:4]
    worst_n = max(rws, key=lambda r: r[3] / max(0.1, 2.0 * r[2]))
    assert med < 0.15 and worst_n[3] < max(0.1, 2.0 * worst_n[2]), worst_n
    for key, v in m.expert_encoder.state_dict().items():
        if 'running_' in key:
            assert rel_fro(v, torch.from_numpy(g['bn.' + key])) < 1e-2, key
        if 'num_batches' in key:
            assert int(v) == int(g['bn.' + key]) == U * k
    del tr, m


def test_shared_pool_keeps_peak_memory_of_the_plain_step(base):
    """a condition, not a measurement: with P = bytes of masters + shadows + gradients + moments,
    peak(accum_steps = 4) - P <= 1.25 x (peak(accum_steps = 1) - P) at base_b8: the three graphs of an accumulating Trainer share ONE pool
    (private pools would hold the activation set two or three times; 25 % is head-room for allocator rounding).  Peaks are the allocator's
    RESERVED bytes (what the process holds, graph pools included), both taken here, k = 1 first."""
    case, reset = base
    mb = tuple(t for t in case.inputs())
    peaks = {}
    for k in (1, 4):
        enc, dec = reset()
        gc.collect(); torch.cuda.synchronize(); torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        tr, m = _trainer(case, enc, dec, [mb] * k, k, lr=1e-4, keep_grads=False)
        for _ in range(2 * k):
            tr.step()
        torch.cuda.synchronize()
        assert tr.graphs is not None and len(tr.graphs) == (1 if k == 1 else 3)
        P = sum(4 * st.master.numel() + 2 * st.shadow.numel() + 4 * st.grad.numel() for st in tr.stores) + sum(4 * t.numel() for t in tr.m + tr.v)
        peaks[k] = (torch.cuda.max_memory_reserved(), torch.cuda.max_memory_allocated(), P)
        del tr, m
    (r1, a1, P1), (r4, a4, P4) = peaks[1], peaks[4]
    print('peak reserved / allocated / P in MB: accum_steps=1', r1 >> 20, a1 >> 20, P1 >> 20, ' accum_steps=4', r4 >> 20, a4 >> 20, P4 >> 20)
    assert P1 == P4
    assert r4 - P4 <= 1.25 * (r1 - P1), (r4 - P4, r1 - P1)
    assert a4 - P4 <= 1.25 * (a1 - P1), (a4 - P4, a1 - P1)


# ----------------------------------------------------------------------------------------------------------------- tiny geometry
def _tiny_mbs(n=3):
    """n different micro-batches of the tiny case's size: its batch, then one of its rows repeated"""
    case = C.Case('tiny_caption')
    full = case.inputs()
    picks = [torch.tensor([0, 1]), torch.tensor([0, 0]), torch.tensor([1, 1])][:n]

    def pick(t, idx):
        if isinstance(t, dict):
            return {kk: pick(v, idx) for kk, v in t.items()}
        return None if t is None else t[idx]
    return case, [tuple(pick(t, idx) for t in full) for idx in picks]


def _tiny(case, mbs, k, p_drop=0.0, **kw):
    enc, dec, _, _ = build(case, p_drop=p_drop)
    return _trainer(case, enc, dec, mbs, k, **kw)


def _store_grads(tr):
    return [st.grad[:st.n_train].clone() for st in tr.stores]


def test_accumulation_equals_the_sum_of_its_parts():
    """dropout 0, lr = 0 (the weights stay put), k = 3 with three different micro-batches: the accumulated buffers equal the sum of the three
    gradients the k = 1 path produces for each micro-batch alone, per store, to max(2 x noise, 1e-3) -- noise = two identical k = 1 runs"""
    case, mbs = _tiny_mbs(3)
    sums, singles = [], []
    for rep in range(2):
        cur = [0]
        tr, m = _tiny(case, mbs, 1, lr=0.0, select=lambda: cur[0])            # (k = 1: the table of the bound batch)
        parts = []
        for cur[0], mb in enumerate(mbs):
            _bind(tr, mb)
            tr.step()
            parts.append(_store_grads(tr))
        torch.cuda.synchronize()
        assert tr.graphs is not None and tr.it == 3
        sums.append([sum(p[i] for p in parts) for i in range(2)])
        singles.append(parts)
        del tr, m
    tr, m = _tiny(case, mbs, 3, lr=0.0)
    p0 = [st.master.clone() for st in tr.stores]
    losses = [l.item() for l in _group(tr, mbs)]
    torch.cuda.synchronize()
    assert tr.graphs is not None and sorted(tr.graphs) == ['close', 'middle', 'open'] and tr.it == 1
    assert tr._exclusive is not None and len(tr._exclusive) > 10
    for i, st in enumerate(tr.stores):
        noise = rel_fro(sums[1][i], sums[0][i])
        err = rel_fro(st.grad[:st.n_train], sums[0][i])
        print('store', i, 'accumulated vs sum of parts', err, 'noise of two k=1 runs', noise, 'a single part against the sum', rel_fro(singles[0][0][i], sums[0][i]))
        assert err < max(2.0 * noise, 1e-3), (i, err, noise)
        assert rel_fro(singles[0][0][i], sums[0][i]) > 0.1                      # (the parts matter: one micro-batch alone is far from the sum)
        assert torch.equal(st.master, p0[i])
    assert math_close(tr.group_loss.item(), float(np.mean(losses)), 1e-6)


@pytest.mark.parametrize('keep_grads', [True, False])
def test_accum_graph_equals_eager_first_group(keep_grads):
    """capture warm-up (one micro-step of every kind, twice) must not leak into the training state: the first replayed group and the first eager
    group give the same losses, gradients, parameters, Adam moments, BatchNorm buffers, iteration counter and seed (dropout ON: k seed advances)"""
    from tests.util import splitmix64
    case, mbs = _tiny_mbs(3)
    res = []
    for use_graph in (False, True):
        tr, m = _tiny(case, mbs, 3, p_drop=None, use_graph=use_graph, lr=1e-3, keep_grads=keep_grads)
        _set_seed(tr, 1234567)
        random.seed(99)
        losses = [l.item() for l in _group(tr, mbs)]
        assert tr.micro_index == 0
        grads = _store_grads(tr)                                # (keep_grads: the group's sum, read before anything else runs)
        with pytest.raises(RuntimeError, match='inside an open accumulation group'):
            _bind(tr, mbs[0]); tr.step(); tr.state_dict()
        tr.abort_group()
        sd = tr.state_dict()
        torch.cuda.synchronize()
        res.append(dict(losses=losses, it=tr.it, sd_it=sd['it'], seed=int(tr.seed.item()) & 0xFFFFFFFFFFFFFFFF, p=[st.master.clone() for st in tr.stores],
                        g=grads, m=[t.clone() for t in tr.m], gl=tr.group_loss.item()))
        del tr, m
    a, b = res
    want_seed = 1234567
    for _ in range(4):                                          # three micro-steps of the group + the aborted one
        want_seed = splitmix64(want_seed)
    assert a['it'] == b['it'] == a['sd_it'] == 1 and a['seed'] == b['seed'] == want_seed
    for la, lb in zip(a['losses'], b['losses']):
        assert math_close(la, lb, 1e-5), (a['losses'], b['losses'])
    assert math_close(a['gl'], b['gl'], 1e-5) and math_close(a['gl'], float(np.mean(a['losses'])), 1e-6)
    # (moments and, with keep_grads, the summed gradients carry the check; the masters move by far less than 5e-3 of their norm in one update)
    for ta, tb in zip(a['p'] + a['m'] + (a['g'] if keep_grads else []), b['p'] + b['m'] + (b['g'] if keep_grads else [])):
        assert rel_fro(tb, ta) < 5e-3


def test_opening_micro_step_overwrites_single_writer_outputs():
    """keep_grads=False, lr = 0: AdamW leaves the kept chunks of the single-writer outputs un-zeroed and the OPENING micro-step overwrites them
    (the later ones accumulate): garbage written into those ranges between two groups changes nothing"""
    case, mbs = _tiny_mbs(3)
    res = []
    for garbage in (False, False, True):
        tr, m = _tiny(case, mbs, 3, lr=0.0, keep_grads=False)
        _group(tr, mbs)
        torch.cuda.synchronize()
        assert tr._exclusive and sum(len(r) for r in tr._excl_ranges) > 10 and all(int(km.abs().sum()) > 0 for km in tr._keep_maps)
        if garbage:
            for st, rs in zip(tr.stores, tr._excl_ranges):
                for off, numel in rs:
                    st.grad[off:off + numel].fill_(1.0e3)
        _group(tr, mbs)
        torch.cuda.synchronize()
        assert tr.it == 2
        res.append([t.clone() for t in tr.m])
        del tr, m
    for ta, tn, tb in zip(*res):
        noise = rel_fro(tn, ta)
        assert rel_fro(tb, ta) < max(2.0 * noise, 1e-3), (rel_fro(tb, ta), noise)


@pytest.mark.parametrize('keep_grads', [True, False])
def test_captured_micro_steps_issue_no_stock_fill_or_copy(keep_grads, monkeypatch):
    """behaviour, not source text: while the three micro-step graphs are being captured no Tensor.zero_ / fill_ runs at all (they would become
    memset nodes: _seg_forward's own fill must stay switched off, the opening graph fills through ops.fill_zero) and no Tensor.copy_ touches a
    buffer the Trainer owns (gradients, loss words, seed, hyper-parameters)"""
    calls = []

    def spy(name):
        orig = getattr(torch.Tensor, name)

        def wrapped(self, *a, **kw):
            if self.is_cuda and torch.cuda.is_current_stream_capturing():
                calls.append((name, self.data_ptr(), self.numel()))
            return orig(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, wrapped)
    for name in ('zero_', 'fill_', 'copy_'):
        spy(name)
    case, mbs = _tiny_mbs(3)
    tr, m = _tiny(case, mbs, 3, lr=1e-3, keep_grads=keep_grads)
    _group(tr, mbs)
    torch.cuda.synchronize()
    assert tr.graphs is not None and sorted(tr.graphs) == ['close', 'middle', 'open']
    owned = [(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for t in [st.grad for st in tr.stores] + [tr._loss_acc, tr._group_loss, tr.seed, tr.hyper]]
    fills = [c for c in calls if c[0] != 'copy_']
    copies = [c for c in calls if c[0] == 'copy_' and any(lo <= c[1] < hi for lo, hi in owned)]
    print('stock in-place calls seen during capture:', len(calls), 'fills', fills[:4], 'copies into Trainer buffers', copies[:4])
    assert not fills and not copies, (fills[:4], copies[:4])


def test_interrupted_group_restarts_from_clean_buffers():
    """an exception between micro-step 1 and 2 (a raising host hook) ends the group; the fresh group that follows gives the update of an
    undisturbed Trainer: the partial sums of the interrupted group never reach AdamW"""
    case, mbs = _tiny_mbs(2)
    res = []
    for interrupt in (False, True):
        tr, m = _tiny(case, mbs, 2, lr=1e-3, keep_grads=False)
        if interrupt:
            _bind(tr, mbs[0]); tr.step()
            assert tr.micro_index == 1
            pinned = tr._host_prologue

            def hook():
                raise OSError('injected between two micro-steps')
            tr._host_prologue = hook
            with pytest.raises(OSError, match='injected'):
                _bind(tr, mbs[1]); tr.step()
            tr._host_prologue = pinned
            assert tr.micro_index == 0 and tr.it == 0
        _group(tr, mbs)
        torch.cuda.synchronize()
        assert tr.it == 1 and tr.micro_index == 0 and tr.graphs is not None
        res.append((([st.master[:st.n_train].clone() for st in tr.stores]), [t.clone() for t in tr.m]))
        del tr, m
    (pa, ma), (pb, mb_) = res
    # (the Adam moments carry this check; one lr = 1e-3 update moves the masters by far less than 5e-3 of their norm, they only show that nothing blew up)
    for ta, tb in zip(pa + ma, pb + mb_):
        assert rel_fro(tb, ta) < 5e-3, rel_fro(tb, ta)       # (twice the first micro-batch's gradient in the sum would move the moments by ~50 %)
