"""GPU, world_size 2 on ONE device over gloo (the harness of tests/test_dp_gpu.py) x Trainer(accum_steps=2): non-closing micro-steps run as
one segment and exchange nothing (DDP's no_sync), the closing micro-step runs the staged schedule and exchanges the group's accumulated sum once
per UPDATE; 1 / (world k) is applied by AdamW (fp32 payload) or as the bf16 pre-scale.  Reference for the reduced buffers: world 1 x
accum_steps=4 over the same four micro-batches, in this process."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_dp_gpu import _free_port

pytestmark = pytest.mark.gpu

WORLD, K = 2, 2


def _four_micro_batches():
    from tests.golden import cases as C
    case = C.Case('tiny_caption')
    full = case.inputs()

    def pick(t, idx):
        if isinstance(t, dict):
            return {kk: pick(v, idx) for kk, v in t.items()}
        return None if t is None else t[idx]
    return case, [tuple(pick(t, torch.tensor(idx)) for t in full) for idx in ([0, 1], [0, 0], [1, 1], [1, 0])]


def _worker(rank, world, port, out, payload, lr, n_groups, issue, use_graph, keep_grads=True):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    os.environ['MASTER_ADDR'] = '127.0.0.1'; os.environ['MASTER_PORT'] = str(port)
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    import tests.test_accum_gpu as A
    case, mbs = _four_micro_batches()
    mine = [mbs[K * rank + j] for j in range(K)]              # rank r accumulates micro-batches 2 r, 2 r + 1
    enc, dec, _, _ = A.build(case, p_drop=0.0)
    tr, m = A._trainer(case, enc, dec, mine, K, use_graph=use_graph, lr=lr, keep_grads=keep_grads, grad_payload=payload, dec_backward_stages=2, exchange_issue=issue)
    assert tr.world == world and tr.dec_cuts == [2, 1, 0]
    traces, logs = [], []
    for _ in range(n_groups):
        for mb in mine:
            A._bind(tr, mb)
            loss = tr.step()
            traces.append(list(tr.trace))
            logs.append(list(tr.exchange.log))
    torch.cuda.synchronize()
    out[rank] = dict(loss=float(loss), grads=[st.grad[:st.n_train].float().cpu() for st in tr.stores], params=[st.master[:st.n_train].float().cpu() for st in tr.stores],
                     m=[t.float().cpu() for t in tr.m], traces=traces, logs=logs, post_scale=tr._post_scale(), pre_scale=tr.exchange.pre_scale,
                     n_train=[st.n_train for st in tr.stores], it=tr.it, graphs=None if tr.graphs is None else {kk: len(v) for kk, v in tr.graphs.items()},
                     desc=tr.exchange_desc() if tr.exchange.log_last else None)
    dist.barrier()
    dist.destroy_process_group()


def _spawn(payload='fp32', lr=0.0, n_groups=2, issue='device', use_graph=True, keep_grads=True):
    mgr = mp.Manager(); out = mgr.dict()
    mp.spawn(_worker, args=(WORLD, _free_port(), out, payload, lr, n_groups, issue, use_graph, keep_grads), nprocs=WORLD, join=True)
    return out[0], out[1]


def _world1_accum4(lr, keep_grads=True, n_groups=1):
    import tests.test_accum_gpu as A
    case, mbs = _four_micro_batches()
    enc, dec, _, _ = A.build(case, p_drop=0.0)
    tr, m = A._trainer(case, enc, dec, mbs, WORLD * K, lr=lr, keep_grads=keep_grads)
    for _ in range(n_groups):
        A._group(tr, mbs)
    torch.cuda.synchronize()
    assert tr.it == n_groups and tr.graphs is not None
    return [st.grad[:st.n_train].float().cpu() for st in tr.stores], [t.float().cpu() for t in tr.m]


@pytest.mark.parametrize('issue', ['device', 'host'])
def test_two_ranks_accumulate_and_exchange_once_per_update(issue):
    from tests.util import rel_fro
    a, b = _spawn('fp32', 0.0, 2, issue)
    assert a['it'] == b['it'] == 2 and a['graphs'] == dict(open=1, close=5)
    for ga, gb in zip(a['grads'], b['grads']):                 # after the all-reduce both ranks hold the same summed gradient, bit for bit
        assert torch.equal(ga, gb) and ga.abs().sum() > 0
    for pa, pb in zip(a['params'], b['params']):
        assert torch.equal(pa, pb)
    assert a['loss'] != b['loss']                              # the ranks closed on different micro-batches
    assert a['post_scale'] == 1.0 / (WORLD * K)
    # host enqueue order: a non-closing micro-step is ONE segment and hands nothing to the exchange; the closing one is the staged schedule
    for r in (a, b):
        assert r['traces'][0] == r['traces'][2] == [('seg', 0)], r['traces'][0]
        tc = r['traces'][3]
        assert [t for t in tc if t[0] == 'issue'] == [('issue', s) for s in ('dec0', 'dec1', 'trunk', 'front')], tc
        assert [t for t in tc if t[0] == 'seg'] == [('seg', i) for i in range(5)], tc
        if issue == 'device':
            assert tc == [('seg', 0), ('issue', 'dec0'), ('seg', 1), ('issue', 'dec1'), ('seg', 2), ('issue', 'trunk'), ('seg', 3), ('issue', 'front'), ('seg', 4)], tc
    # the exchange log is per UPDATE: untouched by the opening micro-step of the second group, and every range in it exactly once
    assert a['logs'][1] == a['logs'][2] and a['logs'][3] == a['logs'][1]
    cover, seen = {0: 0, 1: 0}, set()
    for tag, lo, hi, n in a['logs'][3]:
        assert n >= 1 and hi > lo and (tag, lo) not in seen
        seen.add((tag, lo))
        cover[int(tag.split(':')[1])] += hi - lo
    assert [cover[0], cover[1]] == a['n_train'], (cover, a['n_train'])
    # lr = 0: the reduced buffers are the accumulated sum of world 1 x accum_steps = 4 over the same four micro-batches
    (g1, _), (g1b, _) = _world1_accum4(0.0), _world1_accum4(0.0)
    for i in range(2):
        noise = rel_fro(g1b[i], g1[i])
        err = rel_fro(a['grads'][i], g1[i])
        print('store', i, 'world 2 x accum 2 against world 1 x accum 4:', err, 'noise of two world-1 runs', noise)
        assert err < max(2.0 * noise, 1e-3), (i, err, noise)


def test_two_ranks_accum_bf16_payload_close_to_fp32_and_update_matches_one_rank():
    """bf16 payload: every rank pre-scales its accumulated sum by 1 / (world k) before the cast, AdamW's scale is 1; fp32: the SUM travels and
    AdamW applies 1 / (world k).  Same mean gradient either way, and the same first Adam moment as one rank accumulating all four micro-batches."""
    from tests.util import rel_fro
    res = {p: _spawn(p, 1e-3, 1, 'device', False) for p in ('fp32', 'bf16')}
    f, h = res['fp32'][0], res['bf16'][0]
    assert f['post_scale'] == 0.25 and h['post_scale'] == 1.0 and h['pre_scale'] == 0.25
    for g32, g16 in zip(f['grads'], h['grads']):
        assert ((g16 * WORLD * K - g32).norm() / g32.norm()).item() < 1e-2
    for p in ('fp32', 'bf16'):
        for pa, pb in zip(res[p][0]['params'], res[p][1]['params']):
            assert torch.equal(pa, pb)
    _, m1 = _world1_accum4(1e-3)
    for i in range(2):
        assert rel_fro(f['m'][i], m1[i]) < 5e-3 and rel_fro(h['m'][i], m1[i]) < 1e-2, i


def test_two_ranks_accumulate_without_kept_gradients():
    """keep_grads=False (the bench's gradient handling) under the staged closing schedule: the graphs carry no fill, the second group relies on
    the first one's AdamW launches for clean buffers and on the opening micro-step overwriting the kept single-writer chunks.  lr = 0, two
    groups: both ranks bit-identical, and the Adam moments equal one rank x accum_steps = 4 over the same micro-batches (to the noise of two such runs)"""
    from tests.util import rel_fro
    a, b = _spawn('fp32', 0.0, 2, 'device', True, False)
    assert a['it'] == b['it'] == 2 and a['graphs'] == dict(open=1, close=5)
    for ta, tb in zip(a['params'] + a['m'], b['params'] + b['m']):
        assert torch.equal(ta, tb)
    (_, m1), (_, m1b) = _world1_accum4(0.0, False, 2), _world1_accum4(0.0, False, 2)
    for i in range(2):
        noise = rel_fro(m1b[i], m1[i])
        err = rel_fro(a['m'][i], m1[i])
        print('store', i, 'moments, world 2 x accum 2 against world 1 x accum 4, keep_grads=False:', err, 'noise', noise)
        assert err < max(2.0 * noise, 1e-3), (i, err, noise)


def test_refused_combinations_raise():
    import tests.test_accum_gpu as A
    from prismer_amd.trainer import Trainer
    case, mbs = _four_micro_batches()
    enc, dec, _, _ = A.build(case, p_drop=0.0)
    A.set_freeze(enc, dec)
    m = A._Holder(); m.expert_encoder, m.text_decoder = enc, dec
    for kw in (dict(shard_optimizer=True), dict(shard_optimizer='rs_ag'), dict(side_stream=True, micro_batches=2, use_graph=False)):
        with pytest.raises(ValueError, match='accum_steps > 1'):
            Trainer(m, accum_steps=2, **kw)
    Trainer(m, accum_steps=1, shard_optimizer=True)            # (k = 1: every existing mode stays available)
