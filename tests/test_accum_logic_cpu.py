"""Host-side bookkeeping of gradient accumulation (Trainer(accum_steps=k)) that needs no GPU: which captured program runs at micro-step j,
whether it exchanges, the AdamW scale, the seed / LR / bias-correction indices; the single-writer configuration key; the checkpoint rule;
and that the code the accumulating micro-steps capture holds no stock torch fill / copy (they become memset / memcpy nodes)."""
import inspect
import re
import types

import pytest

from prismer_amd import trainer as T
from prismer_amd.dist import GradExchange
from prismer_amd.trainer import Trainer, accum_plan


@pytest.mark.parametrize('k', [1, 2, 5])
def test_group_bookkeeping(k):
    want = {1: ['whole'], 2: ['open', 'close'], 5: ['open', 'middle', 'middle', 'middle', 'close']}[k]
    for u in range(3):
        for j in range(k):
            for world in (1, 2):
                p = accum_plan(k, j, u, world)
                assert p['graph'] == want[j]
                assert p['overwrite'] == (j == 0)                       # single-writer outputs overwritten in the first micro-step only
                assert p['update'] == (j == k - 1)
                assert p['exchanges'] == (world > 1 and j == k - 1)     # DDP's no_sync before the closing micro-step
                assert p['avg_scale'] == 1.0 / (world * k)
                assert p['seed_index'] == u * k + j                     # the dropout seed advances per MICRO-step
                assert p['lr_index'] == u and p['bias_step'] == u + 1   # schedule and Adam's t count UPDATES
    fake = types.SimpleNamespace(accum=k, _micro=0)
    assert Trainer._kinds(fake) == sorted(set(want), key=['whole', 'open', 'middle', 'close'].index)      # at most three captured programs
    with pytest.raises(AssertionError):
        accum_plan(k, k)


def test_scales_fold_the_group_size_in_fp32():
    for k in (1, 2, 5):
        assert Trainer._post_scale(types.SimpleNamespace(accum=k, exchange=None)) == 1.0 / k
        for world in (2, 8):
            fp32 = GradExchange(world, lambda t: None, payload='fp32', accum=k)
            bf16 = GradExchange(world, lambda t: None, payload='bf16', accum=k)
            assert fp32.post_scale == 1.0 / (world * k)                 # fp32 SUM: everything is left to AdamW's grad_scale
            assert bf16.post_scale == 1.0 and bf16.pre_scale == 1.0 / (world * k)
            assert Trainer._post_scale(types.SimpleNamespace(accum=k, exchange=fp32)) == 1.0 / (world * k)
    assert GradExchange(4, lambda t: None).post_scale == 0.25 and GradExchange(4, lambda t: None, payload='bf16').pre_scale == 0.25


def test_wq_config_changes_with_accum_steps():
    st = types.SimpleNamespace(n_train=4096)
    a = Trainer._wq_config(types.SimpleNamespace(micro=1, keep_grads=False, stores=[st], accum=1))
    b = Trainer._wq_config(types.SimpleNamespace(micro=1, keep_grads=False, stores=[st], accum=4))
    assert a != b and a[:-1] == b[:-1]


def test_prologue_moves_update_state_with_the_closing_micro_step_only():
    calls = []
    fake = types.SimpleNamespace(accum=3, _micro=0, it=0, betas=(0.9, 0.999), lr_schedule=lambda it: calls.append(it) or 1e-3,
                                 enc=types.SimpleNamespace(experts=['depth']), hyper=None, table=None)
    stored = []
    orig = T.ops.store_words
    T.ops.store_words = lambda dst, vals, *a: stored.append(tuple(vals))
    try:
        for j in range(6):
            fake._micro = j % 3
            Trainer._host_prologue(fake)
    finally:
        T.ops.store_words = orig
    assert fake.it == 2 and calls == [0, 1]
    assert stored == [(1e-3, 1.0 - 0.9, 1.0 - 0.999), (1e-3, 1.0 - 0.9 ** 2, 1.0 - 0.999 ** 2)]


def test_state_dict_inside_a_group_raises_and_abort_reopens():
    fake = types.SimpleNamespace(_micro=2, accum=4, _grads_clean=True)
    with pytest.raises(RuntimeError, match='inside an open accumulation group'):
        Trainer.state_dict(fake)
    Trainer.abort_group(fake)
    assert fake._micro == 0 and fake._grads_clean is False


def test_refused_combinations_raise_before_anything_is_built():
    for kw in (dict(shard_optimizer=True), dict(shard_optimizer='rs_ag'), dict(side_stream=True, micro_batches=2, use_graph=False)):
        with pytest.raises(ValueError, match='accum_steps > 1'):
            Trainer(None, accum_steps=2, **kw)
    with pytest.raises(ValueError, match='accum_steps'):
        Trainer(None, accum_steps=0)


def test_accumulating_micro_steps_capture_no_stock_fill_or_copy():
    """what the new Trainer code puts INTO a captured segment: library launches only (ops.fill_zero / ops.weighted_sum / ops.advance_seed); a
    Tensor.zero_() / fill_() / copy_() / torch.zeros there would be a memset / memcpy node or a stock kernel (tests/test_abi.py checks the library)"""
    for fn in (Trainer._seg_micro, Trainer._seg_close_first, Trainer._micro_begin, Trainer._micro_loss, Trainer._zero_grads):
        code = re.sub(r'#[^\n]*', '', inspect.getsource(fn))
        code = re.sub(r'""".*?"""', '', code, flags=re.S)
        assert not re.search(r'\.(zero_|fill_|copy_|add_|mul_|div_|sum|stack|clone)\s*\(|torch\.(zeros|empty|ones|full|stack|add|div)\b', code), fn.__name__


@pytest.mark.parametrize('k', [1, 3])
def test_failed_capture_with_eager_fallback_leaves_the_training_state_as_it_was(k, monkeypatch):
    """the capture warm-up runs real steps and (accum_steps > 1) walks the group position; when it or the capture raises and
    allow_eager_fallback continues eagerly, position, iteration counter and model state are those from before the attempt"""
    import torch
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **kw: None)
    state = dict(micro=0, it=4, master=1.0)
    fake = types.SimpleNamespace(use_graph=True, graphs=None, static={}, allow_eager_fallback=True, accum=k, _micro=0, it=4, master=1.0,
                                 _graph_no_fill=False, _grads_clean=True)
    fake._snapshot = lambda: dict(micro=fake._micro, it=fake.it, master=fake.master)

    def restore(snap):
        fake._micro, fake.it, fake.master = snap['micro'], snap['it'], snap['master']
    fake._restore = restore

    def capture_from(snap):
        fake._micro, fake.it, fake.master, fake._graph_no_fill = k - 1, 6, 2.0, True      # what two warm-up passes leave behind
        raise RuntimeError('capture refused')
    fake._capture_from = capture_from
    fake._capture = lambda: Trainer._capture(fake)
    fake._step_body = lambda: (fake._micro, fake.it, fake.master)
    assert Trainer.step(fake) == (state['micro'], state['it'], state['master'])
    assert fake.use_graph is False and fake.graphs is None and fake._graph_no_fill is False
    fake.use_graph, fake.allow_eager_fallback = True, False
    with pytest.raises(RuntimeError, match='hipGraph capture of the training step failed'):
        Trainer.step(fake)
    assert (fake._micro, fake.it, fake.master) == (0, 4, 1.0)
