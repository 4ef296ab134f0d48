"""CPU: the float64 reference, the bf16 emulation and the per-row metric that test_attention_rows_gpu.py judges the attention kernels with.

1. Floor: for every case of the table row_err(emulated, ref64) is finite and below 2.5e-2 on every tensor, so the GPU bound (twice that)
   stays below 5e-2.
2. Planted defects, applied to the EMULATED result (never to a kernel): each must exceed 2 x row_err(emulated, ref64) on a tensor it
   touches, and the first must at the same time pass the whole-tensor bounds of test_attention (rel_fro 8e-3 for o, 1.5e-2 for the
   gradients) -- which is what the per-row metric adds.
3. An lse wrong by log 2 on one row fails the lse bound (8 x the float32 logsumexp floor).
"""
import math

import pytest
import torch

from tests.attention_cases import ROW_CASES, TENSORS, Reference, case_id, default_key_mask, token_rows
from tests.util import attn_emulated, attn_live, lse_err, rel_fro, row_err

FLOOR_CAP = 2.5e-2
OLD_BOUND = {'o': 8e-3, 'dq': 1.5e-2, 'dk': 1.5e-2, 'dv': 1.5e-2}

_refs = {}


def reference(case):
    if case not in _refs:
        _refs[case] = Reference(case)
    return _refs[case]


def emulate(R, live=None, d_o=None):
    return attn_emulated(R.q, R.k, R.v, R.d_o if d_o is None else d_o, R.scale, keep=R.keep, p=R.p, live=R.live if live is None else live)


def errs(R, got):
    return {n: row_err(token_rows(got[n]), token_rows(R.ref[n])) for n in TENSORS}


@pytest.mark.parametrize('case', ROW_CASES, ids=case_id)
def test_emulation_floor(case):
    R = reference(case)
    floors = {n: R.floor(n) for n in TENSORS}
    print(case_id(case), ' '.join(f'{n} {e:.2e}' for n, e in floors.items()), f'lse fp32 floor {R.lse_floor:.2e}')
    for n, e in floors.items():
        assert math.isfinite(e) and e < FLOOR_CAP, (n, e)
    assert lse_err(R.emu['lse'], R.ref['lse']) <= 8 * R.lse_floor


@pytest.mark.parametrize('case', [(3, 4, 30, 30, 64, True, True, 0.1), (2, 2, 17, 320, 64, False, True, 0.2), (1, 2, 136, 530, 64, False, False, 0.0)],
                         ids=case_id)
def test_ref64_is_attn_ref_in_float64(case):
    """the closed-form gradients of attn_ref64 against autograd through attn_ref (the reference of test_attention) on float64 tensors"""
    from tests.test_kernels_gpu import attn_ref
    R = reference(case)
    q, k, v = (t.clone().requires_grad_(True) for t in (R.q, R.k, R.v))
    o = attn_ref(q, k, v, R.scale, R.key_mask, case[5], R.keep, R.p)
    o.backward(R.d_o)
    for n, t in (('o', o), ('dq', q.grad), ('dk', k.grad), ('dv', v.grad)):
        assert rel_fro(R.ref[n], t) < 1e-12, (n, rel_fro(R.ref[n], t))


def test_ref64_row_with_no_live_key_is_the_uniform_mean():
    case = (2, 2, 20, 40, 64, False, True, 0.0)
    km = default_key_mask(2, 40)
    km[1] = 0
    R = Reference(case, key_mask=km)
    mean = R.v[1].mean(dim=1, keepdim=True).expand(2, 20, 64)
    assert rel_fro(R.ref['o'][1], mean) < 1e-12 and rel_fro(R.emu['o'][1], mean) < 4e-3
    assert all(bool(torch.isfinite(R.ref[n]).all()) and bool(torch.isfinite(R.emu[n]).all()) for n in TENSORS)
    assert R.floor('o') < FLOOR_CAP and all(R.floor(n, slice(0, 1)) < FLOOR_CAP for n in ('dq', 'dk', 'dv'))


def test_row_err_zero_median_demands_equality():
    ref = torch.zeros(5, 8)
    assert row_err(ref.clone(), ref) == 0.0
    got = ref.clone(); got[3, 2] = 1e-30
    assert row_err(got, ref) == float('inf')
    ref2 = torch.zeros(5, 8); ref2[:3] = 1.0                       # median row norm > 0: the zero rows are judged against it
    got2 = ref2.clone(); got2[4, 0] = 0.5
    assert abs(row_err(got2, ref2) - 0.5 / 8 ** 0.5) < 1e-12


@pytest.mark.parametrize('case', [(2, 3, 260, 260, 64, False, False, 0.0), (2, 2, 17, 320, 64, False, True, 0.2)], ids=case_id)
def test_defect_a_last_row_drops_its_last_live_key(case):
    """(a) passes every whole-tensor bound of test_attention and fails the per-row bound"""
    R = reference(case)
    live = R.live.clone()
    last = int(live[-1, -1, -1].nonzero().max())
    live[-1, -1, -1, last] = False
    bad = emulate(R, live=live)
    e = errs(R, bad)
    whole = {n: rel_fro(token_rows(bad[n]), token_rows(R.ref[n])) for n in TENSORS}
    print(case_id(case), 'per row', e, 'bounds', {n: 2 * R.floor(n) for n in TENSORS}, 'whole tensor', whole)
    for n in TENSORS:
        assert whole[n] < OLD_BOUND[n], ('the whole-tensor bound sees it', n, whole[n])
    assert e['o'] > 2 * R.floor('o') and e['dq'] > 2 * R.floor('dq'), e


def test_defect_b_next_entrys_key_mask_length():
    R = reference((3, 4, 30, 30, 64, True, True, 0.1))
    km = R.key_mask.clone()
    km[0] = R.key_mask[1]
    bad = emulate(R, live=attn_live(3, 4, 30, 30, km, True))
    e = errs(R, bad)
    print('per row', e, 'bounds', {n: 2 * R.floor(n) for n in TENSORS})
    for n in TENSORS:
        assert e[n] > 2 * R.floor(n), (n, e[n], R.floor(n))


def test_defect_c_causal_cut_off_by_one_in_one_subtile():
    R = reference((2, 2, 70, 130, 32, True, True, 0.1))
    live = R.live.clone()
    for qi in range(16, 32):
        live[1, 0, qi, qi] = False                                 # ki >= qi cut in the second 16-row sub-tile of one head
    bad = emulate(R, live=live)
    e = errs(R, bad)
    print('per row', e, 'bounds', {n: 2 * R.floor(n) for n in TENSORS})
    for n in TENSORS:
        assert e[n] > 2 * R.floor(n), (n, e[n], R.floor(n))


def test_defect_d_last_key_tile_sees_only_the_first_query_tile():
    """dK / dV are sums over the queries; with dO = 0 for the queries from 64 on those contribute exactly nothing"""
    R = reference((2, 3, 280, 150, 64, False, False, 0.0))
    d_o = R.d_o.clone()
    d_o[:, :, 64:] = 0
    part = emulate(R, d_o=d_o)
    bad = {n: R.emu[n].clone() for n in TENSORS}
    for n in ('dk', 'dv'):
        bad[n][:, :, 128:] = part[n][:, :, 128:]                   # the ragged key tile 128..149
    e = errs(R, bad)
    print('per row', e, 'bounds', {n: 2 * R.floor(n) for n in TENSORS})
    assert e['dk'] > 2 * R.floor('dk') and e['dv'] > 2 * R.floor('dv'), e
    assert e['o'] <= 2 * R.floor('o') and e['dq'] <= 2 * R.floor('dq')     # untouched tensors stay inside: the bound is not trivially failed


def test_lse_wrong_by_log2_on_one_row_fails_the_bound():
    R = reference((2, 2, 70, 130, 32, True, True, 0.1))
    rows = R.live.any(-1)
    good = R.ref['lse'].float()
    assert lse_err(good, R.ref['lse'], rows) <= 8 * R.lse_floor
    bad = good.clone()
    bad[1, 1, 40] += math.log(2.0)
    assert lse_err(bad, R.ref['lse'], rows) > 8 * R.lse_floor
    assert rel_fro(bad, good) < 5e-2                               # ... while a whole-tensor figure hardly moves
