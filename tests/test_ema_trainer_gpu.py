"""Trainer(ema_decay=, ema_warmup=) on the device (tiny_caption): the weight average kept by the AdamW launch of the captured step -- off by default
and then the step it was, the trajectory against prismer_amd.trainer.ema_update_spec / ema_decay_at under the derived bar of
tests/test_ema_cpu.py, the AdamW side bitwise untouched, the guard's skipped update, accumulation, a checkpoint, the ema_weights() scope, two ranks."""
import os

import numpy as np
import pytest
import torch

from tests.golden import cases as C
from tests.golden.make_clip_golden import poison
from tests.test_accum_gpu import _bind, _set_seed, _tiny, _tiny_mbs
from tests.test_clip_trainer_gpu import _bits, _calls_of_one_eager_step, _free_port
from tests.test_ema_cpu import BAR, ema_err
from tests.test_parity_gpu import build

pytestmark = pytest.mark.gpu


def _masters(tr):
    return [st.master[:st.n_train].clone() for st in tr.stores]


def _emas(tr):
    return [e[:st.n_train].clone() for st, e in zip(tr.stores, tr.ema)]


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _moved_by_the_spec(tr, before, u, what):
    """the average after an update at schedule position u, against the spec applied to the average before it and the masters after it"""
    from prismer_amd.trainer import ema_decay_at
    w = 1.0 - ema_decay_at(u, tr.ema_decay, tr.ema_warmup)
    assert np.float32(tr._ema_w.item()) == np.float32(w), (what, tr._ema_w.item(), w)
    for i, (e0, p, e) in enumerate(zip(before, _masters(tr), _emas(tr))):
        err = ema_err(e, e0, p, w)
        print(f'{what}, store {i}: w = {w:.6g}, ema worst error / max(|e|, |p|) {err:.3e} (bar {BAR:.3e})')
        assert err <= BAR, (what, i, err)
        assert not torch.equal(e, e0), (what, i)


def test_defaults_are_todays_path(monkeypatch):
    """ema_decay=None: neither new entry point is ever called (capture warm-up, capture, replay, eager), no buffer exists, the hyper words are
    the three they were; ema_decay set: the average rides the AdamW launches, an eager step makes exactly as many entry-point calls"""
    from prismer_amd import ops
    called = []
    for name in ('adamw_ema', 'swap_f32'):
        orig = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _o=orig, _n=name, **kw: (called.append(_n), _o(*a, **kw))[1])
    case, mbs = _tiny_mbs(1)
    calls = {}
    for tag, kw in (('off', {}), ('on', dict(ema_decay=0.999))):
        n0 = len(called)
        tr, m = _tiny(case, [mbs[0]], 1, p_drop=None, lr=C.TRAJ_LR, keep_grads=False, **kw)
        for _ in range(3):
            tr.step()
        torch.cuda.synchronize()
        assert tr.graphs is not None and tr.it == 3 and tr.hyper.numel() == 3
        assert np.float32(tr.hyper[1].item()) == np.float32(1 - 0.9 ** 3) and np.float32(tr.hyper[2].item()) == np.float32(1 - 0.999 ** 3)
        calls[tag] = _calls_of_one_eager_step(tr)
        if tag == 'off':
            assert len(called) == n0 and tr.ema is None and tr._ema_w is None and tr._step_words is None and tr.ema_decay is None
            assert tr.hyper.storage_offset() == 0 and 'ema' not in tr.state_dict()
            with pytest.raises(RuntimeError, match='ema_decay'):
                tr.ema_state_dict()
        else:
            assert set(called[n0:]) == {'adamw_ema'} and len(tr.ema) == 2
        del tr, m
    print('entry-point calls per step (tiny_caption, eager pass): ema off', calls['off'], 'ema on', calls['on'])
    assert calls['on'] == calls['off']


@pytest.mark.parametrize('use_graph', [True, False])
def test_trajectory_follows_the_spec_with_warmup(use_graph):
    """4 steps with the warm-up ramp (d = 0.1, 2/11, 3/12, 4/13): after each, the average is one spec update from the average before it and the
    masters after it.  The first step() holds warm-up passes + capture + replay: the average is ONE update from the initial masters, with
    d = 0.1 -- a leak of the capture warm-up or a weight frozen into the graph fails here"""
    case, mbs = _tiny_mbs(1)
    tr, m = _tiny(case, [mbs[0]], 1, use_graph=use_graph, lr=1e-3, keep_grads=False, ema_decay=0.999, ema_warmup=True)
    assert _same(_emas(tr), _masters(tr))
    for it in range(1, 5):
        before = _emas(tr)                                      # (step 1: the initial masters)
        tr.step()
        torch.cuda.synchronize()
        assert tr.it == it
        _moved_by_the_spec(tr, before, it - 1, f'use_graph={use_graph} step {it}')
        assert np.float32(tr._ema_w.item()) == np.float32((1 - 0.1, 1 - 2 / 11, 1 - 3 / 12, 1 - 4 / 13)[it - 1])
    assert (tr.graphs is not None) == use_graph


@pytest.mark.parametrize('use_graph', [True, False])
def test_the_average_only_observes_the_update(use_graph):
    """keep_grads=True: after each of 3 steps the UNFUSED kernel (ops.adamw: ph_adamw_keep) runs on the pre-step masters / moments with the gradients
    the step consumed and the host's hyper words: masters, both moments and shadows agree bit for bit with the step's"""
    from prismer_amd import ops
    case, mbs = _tiny_mbs(1)
    tr, m = _tiny(case, [mbs[0]], 1, p_drop=None, use_graph=use_graph, lr=1e-3, keep_grads=True, ema_decay=0.99)
    _set_seed(tr, 1234567)
    for it in range(1, 4):
        before = [(st.master.clone(), tr.m[i].clone(), tr.v[i].clone(), st.shadow.clone()) for i, st in enumerate(tr.stores)]
        tr.step()
        torch.cuda.synchronize()
        hyper = torch.tensor([tr.lr_schedule(it - 1), 1.0 - tr.betas[0] ** it, 1.0 - tr.betas[1] ** it], dtype=torch.float32, device='cuda')
        assert torch.equal(hyper.view(torch.int32), tr.hyper.view(torch.int32)), (it, hyper, tr.hyper)
        for i, st in enumerate(tr.stores):
            p, mm, vv, sh = before[i]
            g = st.grad.clone()
            ops.adamw(p, g, mm, vv, sh, st.n_train, hyper, tr.betas[0], tr.betas[1], tr.eps, tr.wd, tr._post_scale(), zero_grad=False)
            for name, a, b in (('master', st.master, p), ('m', tr.m[i], mm), ('v', tr.v[i], vv), ('shadow', st.shadow, sh)):
                assert torch.equal(_bits(a)[:st.n_train], _bits(b)[:st.n_train]), (it, i, name)
    assert (tr.graphs is not None) == use_graph


def test_a_skipped_update_leaves_the_average_alone():
    case, mbs = _tiny_mbs(1)
    tr, m = _tiny(case, [mbs[0]], 1, lr=1e-3, keep_grads=False, ema_decay=0.99, max_grad_norm=float('inf'), skip_nonfinite=True)
    bad = (poison(mbs[0][0]),) + tuple(mbs[0][1:])
    for i in range(3):
        before, p_before = _emas(tr), _masters(tr)
        _bind(tr, bad if i == 1 else mbs[0])
        tr.step()
        torch.cuda.synchronize()
        assert (tr.it, tr.skipped_updates) == (i + 1, 1 if i >= 1 else 0)
        if i == 1:
            assert _same(_emas(tr), before) and _same(_masters(tr), p_before)
        else:
            _moved_by_the_spec(tr, before, i, f'guarded step {i + 1}')
    assert tr.graphs is not None and all(bool(torch.isfinite(e).all()) for e in tr.ema)


def test_accumulation_moves_the_average_with_the_closing_micro_step():
    case, mbs = _tiny_mbs(3)
    tr, m = _tiny(case, mbs, 3, lr=1e-3, keep_grads=False, ema_decay=0.9)
    start = _emas(tr)
    for j, mb in enumerate(mbs):
        _bind(tr, mb)
        tr.step()
        torch.cuda.synchronize()
        if j < 2:
            assert _same(_emas(tr), start) and tr.it == 0, j
    assert tr.it == 1 and sorted(tr.graphs) == ['close', 'middle', 'open']
    _moved_by_the_spec(tr, start, 0, 'accum_steps=3, closing micro-step')
    _bind(tr, mbs[0]); tr.step()                                # opens the next group
    with pytest.raises(RuntimeError, match='open accumulation group'):
        with tr.ema_weights():
            pass
    tr.abort_group()


def test_checkpoint_round_trip():
    """2 steps, state_dict() into a fresh Trainer: the average is restored bitwise.  One more step on both: each average is one spec update, within
    the bar, from the restored bits and its own new masters, and the two averages agree with each other within the bare bar,
    |ema - ema2| <= 2^-21 max(|e|, |p|) -- not bitwise: the backward reduces bias gradients with atomics, so the new masters of two runs of one step
    differ, and Adam's normalisation amplifies that.  The test runs where the bar can be met as written and can be missed by a wrong restore:
    lr = 1e-4 and ema_decay = 0.9999, so the step's own noise reaches the averages scaled by w = 1e-4 (measured figures: printed below and
    quoted in profiles/README.md), while masters, moments, `it` or an average restored wrongly move them by far more.  A checkpoint
    without `ema` starts the average from the loaded masters; a Trainer without an average ignores the checkpoint's; another decay warns."""
    case, mbs = _tiny_mbs(1)
    kw = dict(lr=1e-4, keep_grads=False, ema_decay=0.9999)
    tr, m = _tiny(case, mbs, 1, **kw)
    for _ in range(2):
        tr.step()
    sd = tr.state_dict()
    assert sd['ema_decay'] == 0.9999 and len(sd['ema']) == 2 and all(a.data_ptr() != b.data_ptr() for a, b in zip(sd['ema'], tr.ema))
    tr2, m2 = _tiny(case, mbs, 1, **kw)
    tr2.load_state_dict(sd)
    assert _same(_emas(tr2), _emas(tr)) and _same(_masters(tr2), _masters(tr)) and tr2.it == 2
    start = _emas(tr)
    assert not _same(start, _masters(tr))
    for t in (tr, tr2):
        _bind(t, mbs[0]); t.step()
        torch.cuda.synchronize()
        _moved_by_the_spec(t, start, 2, 'step 3 after the checkpoint')
    for i, (a, b, pa, pb) in enumerate(zip(_emas(tr), _emas(tr2), _masters(tr), _masters(tr2))):
        scale = torch.maximum(start[i].abs(), pa.abs()).double().clamp_min(1e-30)
        err = float(((a.double() - b.double()).abs() / scale).max())
        dp = float(((pa.double() - pb.double()).abs() / scale).max())
        print(f'one more step on both, store {i}: worst |ema - ema2| / max(|e|, |p|) {err:.3e} (bar {BAR:.3e}); the new masters of the two runs differ by {dp:.3e}')
        assert err <= BAR, (i, err, dp)
    tr2.load_state_dict({k: v for k, v in sd.items() if k not in ('ema', 'ema_decay')})
    assert _same(_emas(tr2), _masters(tr2)) and not _same(_emas(tr2), start)
    tr3, m3 = _tiny(case, mbs, 1, lr=1e-4, keep_grads=False)
    tr3.load_state_dict(sd)
    assert tr3.ema is None and tr3.it == 2 and 'ema' not in tr3.state_dict()
    tr4, m4 = _tiny(case, mbs, 1, lr=1e-4, keep_grads=False, ema_decay=0.99)      # the decay is a constructor option: the average loads, with a warning
    with pytest.warns(UserWarning, match='ema_decay=0.9999'):
        tr4.load_state_dict(sd)
    assert tr4.ema_decay == 0.99 and _same(_emas(tr4), [e[:st.n_train] for st, e in zip(tr4.stores, sd['ema'])])


def test_scope_swaps_the_average_in_and_back_out():
    case, mbs = _tiny_mbs(1)
    tr, m = _tiny(case, mbs, 1, lr=1e-3, keep_grads=False, ema_decay=0.9)
    for _ in range(2):
        tr.step()
    torch.cuda.synchronize()
    n_graphs = len(tr.graphs)
    masters, emas = [st.master.clone() for st in tr.stores], _emas(tr)
    shadows = [st.shadow.clone() for st in tr.stores]
    derived = [{k: v[0].clone() for k, v in st.derived.items()} for st in tr.stores]
    convs = [k for k, (t, fn, meta) in tr.stores[0].derived.items() if meta is not None and meta[0] != 'dgrad' and tr.stores[0].is_trainable(meta[0])]
    assert convs, 'no trainable stem conv shadow among the derived buffers'
    live = {k: v.detach().clone() for k, v in m.state_dict().items()}
    outside = tr.ema_state_dict()
    assert set(outside) == set(live)
    moved = [k for k in live if not torch.equal(outside[k], live[k])]
    assert moved and all(outside[k].data_ptr() != v.data_ptr() for k, v in m.state_dict().items())
    with tr.ema_weights():
        torch.cuda.synchronize()
        inside = {k: v.detach().clone() for k, v in m.state_dict().items()}
        for k in live:
            assert inside[k].dtype == outside[k].dtype and torch.equal(inside[k], outside[k]), k
        again = tr.ema_state_dict()
        assert all(torch.equal(again[k], outside[k]) for k in live)
        for st, e, sh in zip(tr.stores, emas, shadows):
            assert torch.equal(_bits(st.master[:st.n_train]), _bits(e))
            assert torch.equal(_bits(st.shadow[:st.n_train]), _bits(e.to(torch.bfloat16)))
            assert torch.equal(_bits(st.shadow[st.n_train:]), _bits(sh[st.n_train:]))              # frozen parameters: untouched
        assert not torch.equal(tr.stores[0].derived[convs[0]][0], derived[0][convs[0]])
        for what, fn in (('step', tr.step), ('state_dict', tr.state_dict), ('load_state_dict', lambda: tr.load_state_dict({}))):
            with pytest.raises(RuntimeError, match='inside `with ema_weights'):
                fn()
        with pytest.raises(RuntimeError, match='inside `with ema_weights'):
            with tr.ema_weights():
                pass
    torch.cuda.synchronize()
    for st, p, sh, dv, e in zip(tr.stores, masters, shadows, derived, emas):
        assert torch.equal(_bits(st.master), _bits(p)) and torch.equal(_bits(st.shadow), _bits(sh))
        assert all(torch.equal(_bits(st.derived[k][0]), _bits(t)) for k, t in dv.items())
    assert _same(_emas(tr), emas) and len(tr.graphs) == n_graphs
    before = _emas(tr)
    tr.step()
    torch.cuda.synchronize()
    assert tr.it == 3 and len(tr.graphs) == n_graphs
    _moved_by_the_spec(tr, before, 2, 'the step after the scope')


# ----------------------------------------------------------------------------------------------------------------- two ranks on one device
def _dp_worker(rank, world, port, out):
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
    if rank == 1:                                   # rank 1 starts from other weights: the rank-0 broadcast of the construction must win
        with torch.no_grad():
            for mod in (enc, dec):
                for p in mod.parameters():
                    if p.requires_grad:
                        p.add_(0.01)
    m = _Holder(); m.expert_encoder, m.text_decoder = enc, dec
    pre = {k: v.detach().clone().cpu() for k, v in m.state_dict().items()}
    tab = case.instance_table(x)
    tr = Trainer(m, lr=1e-3, total_steps=10, use_graph=True, keep_grads=False, dec_backward_stages=2, ema_decay=0.9)
    init_equal = all(torch.equal(e[:st.n_train], st.master[:st.n_train]) for st, e in zip(tr.stores, tr.ema))
    tr.set_batch(to_dev(x), ids, mask, labels)
    orig = tr._host_prologue

    def prologue():
        orig()
        tr.table.copy_(torch.tensor(tab, dtype=torch.int32))
    tr._host_prologue = prologue
    for i in range(2):
        tr.step()
        torch.cuda.synchronize()
    esd = {k: v.cpu() for k, v in tr.ema_state_dict().items()}
    trainable = [k for k, v in m.state_dict().items()
                 if any(st.master.data_ptr() <= v.data_ptr() < st.master.data_ptr() + 4 * st.n_train for st in tr.stores)]
    out[rank] = dict(ema=[e[:st.n_train].clone().cpu() for st, e in zip(tr.stores, tr.ema)], master=[st.master[:st.n_train].clone().cpu() for st in tr.stores],
                     init_equal=init_equal, it=tr.it, graphs=len(tr.graphs),
                     differs_from_pre=[k for k in trainable if not torch.equal(esd[k], pre[k])], trainable=trainable)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_hold_the_same_average():
    """world_size 2 on one device over gloo (the arrangement of tests/test_clip_trainer_gpu.py): rank 1 is built on perturbed weights and a
    different batch; the construction broadcasts rank 0's weights and re-initialises the average, every rank applies the same reduced gradient:
    after 2 steps the averages are bitwise equal across the ranks and are not rank 1's own initial weights"""
    import torch.multiprocessing as mp
    world = 2
    mgr = mp.Manager(); out = mgr.dict()
    mp.spawn(_dp_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    a, b = out[0], out[1]
    assert a['init_equal'] and b['init_equal'] and a['it'] == b['it'] == 2
    for ea, eb, pa, pb in zip(a['ema'], b['ema'], a['master'], b['master']):
        assert torch.equal(ea.view(torch.int32), eb.view(torch.int32)) and torch.equal(pa.view(torch.int32), pb.view(torch.int32))
        assert not torch.equal(ea, pa)                          # the average trails the masters
    assert b['trainable'] and b['differs_from_pre'] == b['trainable']
