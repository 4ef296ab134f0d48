"""Trainer(max_grad_norm=, skip_nonfinite=) under hipGraph replay: gradient-norm clipping and the non-finite update skip decided on the device --
against the REFERENCE classes running clip_grad_norm_ + `if isfinite(total): optimizer.step()` (tests/golden/base_b8_clip*.npz, minted by
tests/golden/make_clip_golden.py; bars: those of tests/test_accum_gpu.py / tests/test_parity_gpu.py for the same quantities), against the
unguarded path, under accumulation, across a checkpoint, during capture, and on two ranks."""
import gc
import os
import socket

import numpy as np
import pytest
import torch

from tests.golden import cases as C
from tests.golden.make_clip_golden import CLIP_CASE, CLIP_ITERS, FIXTURE, MAX_NORM, POISON_ITER, poison
from tests.test_accum_gpu import _bind, _set_seed, _tiny, _tiny_mbs, _trainer
from tests.test_parity_gpu import PROJ_SLACK, TOL_GRAD, TOL_LOSS, build, math_close
from tests.util import rel_fro

pytestmark = pytest.mark.gpu


def _poisoned(mb):
    return (poison(mb[0]),) + tuple(mb[1:])


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _state(tr):
    """everything a skipped update must leave alone, as bit patterns"""
    return [_bits(st.master).clone() for st in tr.stores] + [_bits(t).clone() for t in tr.m + tr.v] + [_bits(st.shadow).clone() for st in tr.stores]


# ----------------------------------------------------------------------------------------------------------------- Prismer-BASE, built once
@pytest.fixture(scope='module')
def base():
    case = C.Case(CLIP_CASE)
    enc, dec, esd, dsd = build(case, p_drop=0.1)

    def reset():
        gc.collect()
        enc.load_state_dict(esd, strict=True); dec.load_state_dict(dsd, strict=True)
        for mod in (enc, dec):
            if getattr(mod, '_store', None) is not None and mod._store.attached:
                mod._store.refresh()
        return enc, dec
    return case, reset


def test_clipped_and_skipped_trajectory_matches_reference_loop(base):
    """the fixture's three iterations under hipGraph replay with the bench's gradient handling (keep_grads=False): iteration 2 runs on the batch
    with one NaN rgb value.  grad_norm per iteration against the reference's pre-clip total norms (bar: max(TOL_GRAD, 2 x the autocast loop's
    error), the norm bar of _check_grads_against_golden), applied / skipped = 2 / 1, master weights, moments and shadows bitwise untouched by the
    poisoned iteration, and the displacement p_3 - p_0 under the bars of test_accumulated_trajectory_matches_reference_loop -- which holds only
    if update 1 was clipped by torch's coefficient, the skipped iteration cleaned the gradient buffers, and update 3 ran with Adam's t = 2 at
    the schedule position of iteration 3."""
    case, reset = base
    g = C.load(FIXTURE)
    assert (int(g['iters']), int(g['poison_iter']), float(g['max_norm'])) == (CLIP_ITERS, POISON_ITER, MAX_NORM)
    enc, dec = reset()
    clean = tuple(case.inputs())
    mbs = [_poisoned(clean) if i == POISON_ITER else clean for i in range(CLIP_ITERS)]
    tr, m = _trainer(case, enc, dec, [clean], 1, lr=C.TRAJ_LR, keep_grads=False, max_grad_norm=MAX_NORM, skip_nonfinite=True)
    assert tr.total_steps == C.TRAJ_TOTAL and tr.wd == C.TRAJ_WD
    _set_seed(tr, C.DROP_SEED)
    p0 = [st.master.clone() for st in tr.stores]
    losses, norms, counts = [], [], []
    for i, mb in enumerate(mbs):
        before = _state(tr)
        _bind(tr, mb)
        losses.append(tr.step().item())
        norms.append(tr.grad_norm.item())
        counts.append((tr.applied_updates, tr.skipped_updates, tr.it))
        same = all(torch.equal(a, b) for a, b in zip(before, _state(tr)))
        assert same == (i == POISON_ITER), (i, same)
    torch.cuda.synchronize()
    assert tr.use_graph and tr.graphs is not None and len(tr.graphs) == 1
    ref, ac, tot, ac_tot = g['losses'], g['ac_losses'], g['totals'], g['ac_totals']
    print(FIXTURE, 'losses', losses, 'reference', ref.tolist(), '| grad_norm', norms, 'reference', tot.tolist(), 'autocast yardstick', ac_tot.tolist(), '| counts', counts)
    assert counts == [(1, 0, 1), (1, 1, 2), (2, 1, 3)]
    for i in range(CLIP_ITERS):
        if i == POISON_ITER:
            assert not np.isfinite(norms[i]) and not np.isfinite(losses[i])
            continue
        assert math_close(losses[i], float(ref[i]), max(TOL_LOSS, 3.0 * abs(ac[i] - ref[i]) / ref[i])), (i, losses[i], float(ref[i]))
        bar_n = max(TOL_GRAD, 2.0 * abs(ac_tot[i] - tot[i]) / tot[i])
        assert abs(norms[i] - tot[i]) / tot[i] < bar_n, (i, norms[i], float(tot[i]), bar_n)
        assert norms[i] > MAX_NORM                              # the clip was active here as it was in the reference
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
            assert bool(torch.isfinite(delta).all()), n
            e = C.projected_error(C.grad_projections(n, delta), g['dproj.' + n]) / dn
            bar = PROJ_SLACK * max(0.15, 2.0 * float(g['ac_drel.' + n]))
            rws.append((e / bar, e, float(g['ac_drel.' + n]), abs(delta.double().norm().item() - dn) / dn, n))
    rws.sort(reverse=True)
    med = float(np.median([r[1] for r in rws]))
    print(FIXTURE, 'displacement after', CLIP_ITERS, 'iterations: worst (err/bar, full-tensor error estimate, autocast error, norm error, name)', rws[:3], 'median', med,
          'autocast median', float(np.median([r[2] for r in rws])))
    assert rws[0][0] < 1.0, rws[:4]
    worst_n = max(rws, key=lambda r: r[3] / max(0.1, 2.0 * r[2]))
    assert med < 0.15 and worst_n[3] < max(0.1, 2.0 * worst_n[2]), worst_n
    for key, v in m.expert_encoder.state_dict().items():
        if 'running_' in key:
            assert rel_fro(v, torch.from_numpy(g['bn.' + key])) < 1e-2, key           # the NaN never reached a BatchNorm buffer
        if 'num_batches' in key:
            assert int(v) == int(g['bn.' + key]) == CLIP_ITERS
    del tr, m


# ----------------------------------------------------------------------------------------------------------------- tiny geometry
def _calls_of_one_eager_step(tr):
    """entry-point calls of one eager step (ph_prof_collect: the count tools/clip_probe.py reports per arm)"""
    import ctypes
    from prismer_amd import _lib
    buf = (ctypes.c_double * (64 * 4))()
    graphs, tr.use_graph = tr.use_graph, False
    try:
        torch.cuda.synchronize()
        _lib.lib.ph_prof_enable(1); _lib.lib.ph_prof_collect(buf)
        tr.step()
        _lib.lib.ph_prof_collect(buf)
    finally:
        _lib.lib.ph_prof_enable(0)
        tr.use_graph = graphs
    return int(sum(buf[4 * i + 3] for i in range(8)))


def test_defaults_are_the_unguarded_path(monkeypatch):
    """both options off: none of the new entry points is ever called (capture warm-up, capture, replay, eager), no control block or workspace
    exists, the host writes all three hyper words, and a step is exactly two entry-point calls shorter than a guarded step (ph_grad_sqnorm,
    ph_clip_finalize; ph_adamw_ctl stands where ph_adamw_keep stood).  That the unguarded step is the parent commit's -- same call count, same
    step time -- is the parent arm of tools/clip_probe.py (profiles/clip_probe.txt); bitwise equality of two unguarded RUNS does not exist
    to be asserted: the backward reduces bias gradients with atomics, two runs of one build differ in the last bits."""
    from prismer_amd import ops
    called = []
    for name in ('adamw_ctl', 'grad_sqnorm', 'clip_finalize'):
        orig = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _o=orig, _n=name, **kw: (called.append(_n), _o(*a, **kw))[1])
    case, mbs = _tiny_mbs(1)
    calls = {}
    for tag, kw in (('off', {}), ('on', dict(max_grad_norm=float('inf'), skip_nonfinite=True))):
        n0 = len(called)
        tr, m = _tiny(case, [mbs[0]], 1, p_drop=None, lr=C.TRAJ_LR, keep_grads=False, **kw)
        for _ in range(3):
            tr.step()
        torch.cuda.synchronize()
        assert tr.graphs is not None and tr.it == 3 and tr.guard == (tag == 'on')
        assert np.float32(tr.hyper[1].item()) == np.float32(1 - 0.9 ** 3) and np.float32(tr.hyper[2].item()) == np.float32(1 - 0.999 ** 3)
        calls[tag] = _calls_of_one_eager_step(tr)
        if tag == 'off':
            assert len(called) == n0 and tr.ctl is None and tr._norm_ws is None and tr.grad_norm is None
            assert (tr.applied_updates, tr.skipped_updates) == (4, 0)
        else:
            assert set(called[n0:]) == {'adamw_ctl', 'grad_sqnorm', 'clip_finalize'} and (tr.applied_updates, tr.skipped_updates) == (4, 0)
        del tr, m
    print('entry-point calls per step (tiny_caption, eager pass): options off', calls['off'], 'options on', calls['on'])
    assert calls['on'] == calls['off'] + 2


@pytest.mark.parametrize('use_graph', [True, False])
def test_a_guard_that_never_triggers_is_bitwise_the_unguarded_update(use_graph):
    """deterministic form of "guard on, never triggering, equals guard off": Trainer(max_grad_norm=inf, skip_nonfinite=True, keep_grads=True) walks
    three steps; after each, the UNGUARDED kernel (ops.adamw: ph_adamw_keep, the launch of a guard-off step) is run on the pre-step masters /
    moments with the very gradients the step consumed (keep_grads leaves them in the buffers) and the three hyper words the HOST would have
    written (lr, 1 - b1^it, 1 - b2^it).  Masters, both moments and the bf16 shadows must agree bit for bit: coef = 1 exactly, the device's fp64
    bias corrections round to the host's fp32 words, nothing else differs.  (Two separate Trainers cannot be compared bitwise: the backward's
    atomics make two runs of ONE configuration differ, which is why this test feeds identical gradients.)"""
    from prismer_amd import ops
    case, mbs = _tiny_mbs(1)
    tr, m = _tiny(case, [mbs[0]], 1, p_drop=None, use_graph=use_graph, lr=1e-3, keep_grads=True, max_grad_norm=float('inf'), skip_nonfinite=True)
    _set_seed(tr, 1234567)
    for it in range(1, 4):
        before = [(st.master.clone(), tr.m[i].clone(), tr.v[i].clone(), st.shadow.clone()) for i, st in enumerate(tr.stores)]
        tr.step()
        torch.cuda.synchronize()
        assert tr.it == it and (tr.applied_updates, tr.skipped_updates) == (it, 0) and float(tr.ctl.coef.item()) == 1.0
        hyper = torch.tensor([tr.lr_schedule(it - 1), 1.0 - tr.betas[0] ** it, 1.0 - tr.betas[1] ** it], dtype=torch.float32, device='cuda')
        assert torch.equal(hyper.view(torch.int32), tr.hyper.view(torch.int32)), (it, hyper, tr.hyper)
        for i, st in enumerate(tr.stores):
            p, mm, vv, sh = before[i]
            g = st.grad.clone()
            ops.adamw(p, g, mm, vv, sh, st.n_train, hyper, tr.betas[0], tr.betas[1], tr.eps, tr.wd, tr._post_scale(), zero_grad=False)
            for name, a, b in (('master', st.master, p), ('m', tr.m[i], mm), ('v', tr.v[i], vv), ('shadow', st.shadow, sh)):
                assert torch.equal(_bits(a)[:st.n_train], _bits(b)[:st.n_train]), (it, i, name)
    assert (tr.graphs is not None) == use_graph


def test_accumulation_measures_the_group_mean_and_skips_the_whole_group():
    """accum_steps = 2, keep_grads=True (the buffers hold the group's SUM after the closing micro-step): grad_norm is the norm of the group MEAN
    (sum / 2) -- only the closing micro-step measures, it holds the previous value until then; a poisoned OPENING micro-step skips the whole
    group: state bitwise untouched, `it` moves, Adam's t does not; the next clean group applies update 2"""
    case, mbs = _tiny_mbs(2)
    tr, m = _tiny(case, mbs, 2, lr=1e-3, keep_grads=True, max_grad_norm=1e-3, skip_nonfinite=True)
    _bind(tr, mbs[0]); tr.step()
    assert tr.micro_index == 1 and (tr.applied_updates, tr.skipped_updates) == (0, 0) and tr.grad_norm.item() == 0.0
    _bind(tr, mbs[1]); tr.step()
    torch.cuda.synchronize()
    assert sorted(tr.graphs) == ['close', 'open'] and (tr.applied_updates, tr.skipped_updates, tr.it) == (1, 0, 1)
    want = float(torch.sqrt(sum((st.grad[:st.n_train].double() / 2).pow(2).sum() for st in tr.stores)))
    got = tr.grad_norm.item()
    print('accum_steps=2: grad_norm', got, 'norm of the buffers / 2 in fp64', want, 'coef', tr.ctl.coef.item())
    assert abs(got - want) <= 2e-7 * want
    assert np.float32(tr.ctl.coef.item()) == np.float32(1e-3) / (np.float32(got) + np.float32(1e-6)) and got > 1e-2
    before = _state(tr)
    _bind(tr, _poisoned(mbs[0])); tr.step()
    assert all(torch.equal(a, b) for a, b in zip(before, _state(tr))) and (tr.applied_updates, tr.skipped_updates) == (1, 0)
    _bind(tr, mbs[1]); tr.step()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, _state(tr)))
    assert (tr.applied_updates, tr.skipped_updates, tr.it, tr.micro_index) == (1, 1, 2, 0) and not np.isfinite(tr.grad_norm.item())
    for mb in mbs:
        _bind(tr, mb); tr.step()
    torch.cuda.synchronize()
    assert (tr.applied_updates, tr.skipped_updates, tr.it) == (2, 1, 3) and np.isfinite(tr.grad_norm.item()) and tr.grad_norm.item() > 0.0
    assert not all(torch.equal(a, b) for a, b in zip(before, _state(tr)))
    assert all(bool(torch.isfinite(st.master).all()) for st in tr.stores) and all(bool(torch.isfinite(t).all()) for t in tr.m + tr.v)
    assert np.float32(tr.hyper[1].item()) == np.float32(1 - 0.9 ** 2)


def test_state_dict_round_trip_after_a_skip():
    """clean, poisoned, save, load into a fresh guarded Trainer, one more clean step in both: same applied / skipped counts, the same bias
    corrections (t = 2 at it = 3), parameters equal to the noise of the step; a checkpoint without the key loads with applied = it"""
    case, mbs = _tiny_mbs(1)
    kw = dict(lr=1e-3, keep_grads=False, max_grad_norm=0.05, skip_nonfinite=True)
    tr, m = _tiny(case, mbs, 1, **kw)
    tr.step()
    _bind(tr, _poisoned(mbs[0])); tr.step()
    sd = tr.state_dict()
    assert (sd['it'], sd['applied'], sd['skipped']) == (2, 1, 1)
    tr2, m2 = _tiny(case, mbs, 1, **kw)
    tr2.load_state_dict(sd)
    assert (tr2.it, tr2.applied_updates, tr2.skipped_updates) == (2, 1, 1)
    for t in (tr, tr2):
        _bind(t, mbs[0]); t.step()
    torch.cuda.synchronize()
    for t in (tr, tr2):
        assert (t.it, t.applied_updates, t.skipped_updates) == (3, 2, 1)
        assert np.float32(t.hyper[1].item()) == np.float32(1 - 0.9 ** 2) and np.float32(t.hyper[2].item()) == np.float32(1 - 0.999 ** 2)
    for a, b in zip([st.master[:st.n_train] for st in tr.stores] + tr.m, [st.master[:st.n_train] for st in tr2.stores] + tr2.m):
        assert rel_fro(b, a) < 5e-3
    old = {k: v for k, v in sd.items() if k not in ('applied', 'skipped')}
    tr2.load_state_dict(old)
    assert (tr2.it, tr2.applied_updates, tr2.skipped_updates) == (2, 2, 0)
    tr3, m3 = _tiny(case, mbs, 1, lr=1e-3, keep_grads=False)              # an unguarded Trainer reads and writes the same checkpoints
    tr3.load_state_dict(sd)
    assert tr3.it == 2 and tr3.state_dict()['applied'] == 2


@pytest.mark.parametrize('accum', [1, 2])
def test_guarded_capture_issues_no_stock_fill_or_copy(accum, monkeypatch):
    """the spy of tests/test_accum_gpu.py with the guard on: no Tensor.zero_ / fill_ while a graph is being captured, no Tensor.copy_ into a
    buffer the Trainer owns -- control block, partials and hyper words included"""
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
    case, mbs = _tiny_mbs(accum)
    tr, m = _tiny(case, mbs, accum, lr=1e-3, keep_grads=False, max_grad_norm=0.05, skip_nonfinite=True)
    for mb in mbs:
        _bind(tr, mb); tr.step()
    torch.cuda.synchronize()
    assert tr.graphs is not None and (tr.applied_updates, tr.skipped_updates, tr.it) == (1, 0, 1)          # (the capture warm-up's updates were rolled back)
    owned = [(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size())
             for t in [st.grad for st in tr.stores] + [tr._loss_acc, tr._group_loss, tr.seed, tr.hyper, tr.ctl.words, tr._norm_ws]]
    fills = [c for c in calls if c[0] != 'copy_']
    copies = [c for c in calls if c[0] == 'copy_' and any(lo <= c[1] < hi for lo, hi in owned)]
    print('stock in-place calls seen during capture:', len(calls), 'fills', fills[:4], 'copies into Trainer buffers', copies[:4])
    assert not fills and not copies, (fills[:4], copies[:4])


def test_failed_capture_restores_the_counters(monkeypatch):
    """a capture that fails after its warm-up passes (two real updates) leaves no trace of them: allow_eager_fallback continues eagerly from
    applied = skipped = 0, and the first step is update 1"""
    case, mbs = _tiny_mbs(1)
    tr, m = _tiny(case, mbs, 1, lr=1e-3, keep_grads=False, max_grad_norm=0.05, skip_nonfinite=True, allow_eager_fallback=True)
    p0 = [st.master.clone() for st in tr.stores]

    def broken(*a, **kw):
        raise RuntimeError('injected: no graphs today')
    monkeypatch.setattr(torch.cuda, 'CUDAGraph', broken)
    tr.step()
    torch.cuda.synchronize()
    assert not tr.use_graph and tr.graphs is None
    assert (tr.applied_updates, tr.skipped_updates, tr.it) == (1, 0, 1) and np.float32(tr.hyper[1].item()) == np.float32(1 - 0.9)
    assert all(not torch.equal(a, st.master) for a, st in zip(p0, tr.stores))
    _bind(tr, _poisoned(mbs[0])); tr.step()                     # the eager step is guarded like the replayed one
    assert (tr.applied_updates, tr.skipped_updates, tr.it) == (1, 1, 2)


# ----------------------------------------------------------------------------------------------------------------- two ranks on one device
def _free_port():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); p = s.getsockname()[1]; s.close(); return p


def _dp_worker(rank, world, port, out, payload, issue):
    import sys
    import torch.distributed as dist
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    os.environ['MASTER_ADDR'] = '127.0.0.1'; os.environ['MASTER_PORT'] = str(port)
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from prismer_amd.trainer import Trainer
    from tests.test_parity_gpu import _Holder, set_freeze, to_dev
    case = C.Case('tiny_caption')
    x, ids, mask, labels, _ = case.inputs()
    if rank == 1:                                   # a different local batch on rank 1: sample 0 twice
        pick = torch.tensor([0, 0])
        x = {k: ({kk: vv[pick] for kk, vv in v.items()} if isinstance(v, dict) else v[pick]) for k, v in x.items()}
        ids, mask, labels = ids[pick], mask[pick], labels[pick]
    enc, dec, _, _ = build(case, p_drop=0.0)
    set_freeze(enc, dec)
    m = _Holder(); m.expert_encoder, m.text_decoder = enc, dec
    tab = case.instance_table(x)
    tr = Trainer(m, lr=1e-3, total_steps=10, use_graph=True, keep_grads=False, grad_payload=payload, dec_backward_stages=2, exchange_issue=issue,
                 max_grad_norm=0.05, skip_nonfinite=True)
    tr.set_batch(to_dev(x), ids, mask, labels)
    orig = tr._host_prologue

    def prologue():
        orig()
        tr.table.copy_(torch.tensor(tab, dtype=torch.int32))
    tr._host_prologue = prologue
    steps = []
    for i in range(3):
        xb = poison(x) if (i == 1 and rank == 1) else x          # the NaN enters on ONE rank: the all-reduce carries it to both
        tr.set_batch(to_dev(xb), ids, mask, labels)
        loss = tr.step()
        torch.cuda.synchronize()
        steps.append(dict(loss=float(loss), norm=tr.grad_norm.clone().cpu(), coef=float(tr.ctl.coef.item()), apply=int(tr.ctl.apply.item()),
                          applied=tr.applied_updates, skipped=tr.skipped_updates, it=tr.it,
                          params=[st.master[:st.n_train].clone().cpu() for st in tr.stores], m=[t.clone().cpu() for t in tr.m],
                          shadow=[st.shadow[:st.n_train].float().cpu() for st in tr.stores]))
    out[rank] = dict(steps=steps, trace=list(tr.trace), graphs=len(tr.graphs))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize('payload,issue', [('fp32', 'device'), ('bf16', 'host')])
def test_two_ranks_take_the_same_decision(payload, issue):
    """world_size 2 on one device over gloo (tests/test_dp_gpu.py's arrangement), hipGraph replay: a clipped update, an update whose NaN enters on
    rank 1 only, a clipped update.  The norm is taken after the last range has been reduced: both ranks report the same norm bits, take the same
    decision, and their parameters stay bitwise equal across the skipped and the clipped updates"""
    import torch.multiprocessing as mp
    world = 2
    mgr = mp.Manager(); out = mgr.dict()
    mp.spawn(_dp_worker, args=(world, _free_port(), out, payload, issue), nprocs=world, join=True)
    a, b = out[0]['steps'], out[1]['steps']
    print(payload, issue, 'rank 0 (norm, coef, apply, applied, skipped):', [(float(s['norm']), s['coef'], s['apply'], s['applied'], s['skipped']) for s in a])
    for i, (sa, sb) in enumerate(zip(a, b)):
        assert torch.equal(sa['norm'].view(torch.int32), sb['norm'].view(torch.int32)), (i, sa['norm'], sb['norm'])
        assert (sa['apply'], sa['applied'], sa['skipped'], sa['it']) == (sb['apply'], sb['applied'], sb['skipped'], sb['it']) == \
            ((1, 1, 0, 1), (0, 1, 1, 2), (1, 2, 1, 3))[i]
        for ta, tb in zip(sa['params'] + sa['m'] + sa['shadow'], sb['params'] + sb['m'] + sb['shadow']):
            assert torch.equal(ta, tb), i
        if i != 1:
            assert 0.0 < sa['coef'] < 1.0 and sa['coef'] == sb['coef']                     # the clip was active
    assert np.isfinite(a[0]['loss']) and np.isfinite(a[1]['loss']) and not np.isfinite(b[1]['loss'])        # rank 0's own batch was clean
    for ta, tb in zip(a[0]['params'] + a[0]['m'] + a[0]['shadow'], a[1]['params'] + a[1]['m'] + a[1]['shadow']):
        assert torch.equal(ta, tb)                              # the skipped update left everything alone
    assert any(not torch.equal(ta, tb) for ta, tb in zip(a[1]['params'], a[2]['params']))
    assert all(bool(torch.isfinite(t).all()) for t in a[2]['params'] + a[2]['m'])
    # the decoder's AdamW no longer runs beside the encoder backward: the optimizer tail is the last segment, after the last hand-off
    assert out[0]['trace'][-2:] == [('issue', 'front'), ('seg', 4)] and out[0]['graphs'] == 5
