"""Grouped cross-attention (ph_attention_group_fwd / _bwd): `group` consecutive query rows read the K / V of one image.

Reference 1: fp32 torch (attn_ref of test_kernels_gpu) on K / V tiled with repeat_interleave, dropout masks of an ordinary launch on
R = Bi * group batch rows (generator row (r*H + h)*Sq + i) -- the bars of test_attention.
Reference 2: the ungrouped ops of the tree on materialised tiled K / V.
"""
import pytest
import torch

from tests.test_kernels_gpu import BF, attn_ref, rnd, seed_tensor
from tests.util import dropout_keep_attention, rel_fro

pytestmark = pytest.mark.gpu

BI, DH, LAYERS, SEED, STREAM = 2, 64, 2, 4242, 11
SENTINEL = -7.0


@pytest.fixture(scope='module')
def ops():
    from prismer_amd import ops as o
    return o


def _run(ops, group, H, Sq, Sk, p, tuning=None):
    """One grouped forward + backward on the layer-1 column slice of a [images * Sk, 2 * D * LAYERS] K/V buffer of BI + 1 images (the launch covers
    the first BI), and the same through the ungrouped ops on tiled K / V.  Returns a dict of everything the checks read."""
    from prismer_amd import _lib
    D, R = H * DH, BI * group
    W = 2 * D * LAYERS
    q = rnd(R * Sq, D, seed=40)
    kv_all = rnd((BI + 1) * Sk, W, seed=41)
    kv = kv_all[:, 2 * D:4 * D]                                  # what kv_all hands layer 1: K | V as a column slice
    k, v = kv[:, :D], kv[:, D:]
    d_o = rnd(R * Sq, D, seed=42)
    drop = ops.Dropout(p, seed_tensor(SEED), STREAM) if p > 0 else None
    qs, ks = (Sq * D, D), (Sk * W, W)
    dkv_all = torch.full_like(kv_all, SENTINEL)
    dkv = dkv_all[:, 2 * D:4 * D]
    dq = torch.empty_like(q)
    kw = dict(q_strides=qs, k_strides=ks, v_strides=ks)
    bkw = dict(dq_strides=qs, dk_strides=ks, dv_strides=ks, drop=drop, **kw)
    if tuning is not None:
        assert _lib.lib.ph_attention_tuning(tuning) == 1
    try:
        o, lse = ops.attention_group_fwd(q, k, v, R, group, H, Sq, Sk, DH, drop=drop, **kw)
        ops.attention_group_bwd(d_o, q, k, v, o, lse, R, group, H, Sq, Sk, DH, dq=dq, dk=dkv[:, :D], dv=dkv[:, D:], **bkw)
        dkv_again = torch.full_like(kv_all, SENTINEL)
        dq_again = torch.empty_like(q)
        ops.attention_group_bwd(d_o, q, k, v, o, lse, R, group, H, Sq, Sk, DH, dq=dq_again, dk=dkv_again[:, 2 * D:3 * D],
                                dv=dkv_again[:, 3 * D:4 * D], **bkw)
    finally:
        if tuning is not None:
            _lib.lib.ph_attention_tuning(1)
    # the ungrouped ops of the tree on K / V tiled to one copy per query row (contiguous [R * Sk, 2D])
    kvt = kv[:BI * Sk].reshape(BI, Sk, 2 * D).repeat_interleave(group, 0).reshape(R * Sk, 2 * D).contiguous()
    kts = (Sk * 2 * D, 2 * D)
    if tuning is not None:
        _lib.lib.ph_attention_tuning(tuning)
    try:
        o_t, lse_t = ops.attention_fwd(q, kvt[:, :D], kvt[:, D:], R, H, Sq, Sk, DH, q_strides=qs, k_strides=kts, v_strides=kts, drop=drop)
        dq_t, dkv_t = torch.empty_like(q), torch.empty_like(kvt)
        # (on the grouped launch's o / lse: the backward under test and this one then start from the same bits)
        ops.attention_bwd(d_o, q, kvt[:, :D], kvt[:, D:], o, lse, R, H, Sq, Sk, DH, q_strides=qs, k_strides=kts, v_strides=kts, dq=dq_t,
                          dk=dkv_t[:, :D], dv=dkv_t[:, D:], dq_strides=qs, dk_strides=kts, dv_strides=kts, drop=drop)
    finally:
        if tuning is not None:
            _lib.lib.ph_attention_tuning(1)
    fold = dkv_t.float().reshape(BI, group, Sk, 2 * D).sum(1).reshape(BI * Sk, 2 * D)       # fp32 fold of the per-row results
    return dict(D=D, R=R, q=q, kv=kv, kvt=kvt, d_o=d_o, o=o, lse=lse, dq=dq, dkv_all=dkv_all, dkv=dkv, dkv_again=dkv_again, dq_again=dq_again,
                o_t=o_t, lse_t=lse_t, dq_t=dq_t, fold=fold)


def _check(ops, group, H, Sq, Sk, p, tuning=None, same_family_fwd=None):
    c = _run(ops, group, H, Sq, Sk, p, tuning)
    D, R = c['D'], c['R']
    n_img = BI * Sk
    # ---- 1. fp32 torch on tiled K / V
    qf = c['q'].float().reshape(R, Sq, H, DH).transpose(1, 2).requires_grad_(True)
    kvf = c['kv'][:n_img].float().reshape(BI, Sk, 2, H, DH).requires_grad_(True)            # per image: the gradient folds over the members
    kf = kvf[:, :, 0].transpose(1, 2).repeat_interleave(group, 0)
    vf = kvf[:, :, 1].transpose(1, 2).repeat_interleave(group, 0)
    keep = dropout_keep_attention(R * H, Sq, Sk, SEED, STREAM, p).reshape(R, H, Sq, Sk).cuda() if p > 0 else None
    ref = attn_ref(qf, kf, vf, DH ** -0.5, None, False, keep, p)
    e_o = rel_fro(c['o'], ref.transpose(1, 2).reshape(R * Sq, D))
    ref.backward(c['d_o'].float().reshape(R, Sq, H, DH).transpose(1, 2))
    gq = qf.grad.transpose(1, 2).reshape(R * Sq, D)
    gkv = kvf.grad.reshape(n_img, 2 * D)
    e_dq, e_dk, e_dv = rel_fro(c['dq'], gq), rel_fro(c['dkv'][:n_img, :D], gkv[:, :D]), rel_fro(c['dkv'][:n_img, D:], gkv[:, D:])
    print(f'group {group} H {H} Sq {Sq} Sk {Sk} p {p}: vs fp32 o {e_o:.2e} dq {e_dq:.2e} dk {e_dk:.2e} dv {e_dv:.2e}')
    assert e_o < 8e-3, ('o', e_o)
    assert e_dq < 1.5e-2 and e_dk < 1.5e-2 and e_dv < 1.5e-2, ('dq dk dv', e_dq, e_dk, e_dv)
    # ---- 2. the ungrouped ops on materialised tiled K / V
    if same_family_fwd is None:
        # The grouped forward is the small-query forward for every Sk <= 320.  The ungrouped forward of the tree runs that kernel for Sk > 64
        # only and the streaming kernel below (one or two key units: ph_attention_fwd keeps them there), i.e. another summation order over
        # the keys: bit equality is asserted where both sides run one kernel family, the family-to-family bars of test_attention elsewhere.
        same_family_fwd = Sk > 64
    if same_family_fwd:
        assert torch.equal(c['o'], c['o_t']) and torch.equal(c['lse'], c['lse_t']), (rel_fro(c['o'], c['o_t']), rel_fro(c['lse'], c['lse_t']))
    else:
        assert rel_fro(c['o'], c['o_t']) < 4e-3 and rel_fro(c['lse'], c['lse_t']) < 1e-5, (rel_fro(c['o'], c['o_t']), rel_fro(c['lse'], c['lse_t']))
    assert torch.equal(c['dq'], c['dq_t']), ('dq', rel_fro(c['dq'], c['dq_t']))
    e_fk, e_fv = rel_fro(c['dkv'][:n_img, :D], c['fold'][:, :D]), rel_fro(c['dkv'][:n_img, D:], c['fold'][:, D:])
    print(f'   vs fp32 fold of the ungrouped per-row results: dk {e_fk:.2e} dv {e_fv:.2e}')
    assert e_fk < 6e-3 and e_fv < 6e-3, ('dk dv vs fold', e_fk, e_fv)
    # ---- 3. reproducibility: a second backward gives the same bits
    assert torch.equal(c['dkv'], c['dkv_again'][:, 2 * D:4 * D]) and torch.equal(c['dq'], c['dq_again'])
    # ---- 4. untouched memory: the image outside the launch and the columns outside the slice keep the sentinel
    dall = c['dkv_all']
    assert bool((dall[n_img:] == SENTINEL).all()), 'rows of an image outside the launch were written'
    assert bool((dall[:, :2 * D] == SENTINEL).all()) and bool((dall[:, 4 * D:] == SENTINEL).all()), 'columns outside the slice were written'
    assert not bool((c['dkv'][:n_img] == SENTINEL).all())


@pytest.mark.parametrize('p', [0.0, 0.1])
@pytest.mark.parametrize('Sq,Sk', [(1, 23), (12, 33), (30, 260), (32, 320), (17, 31)])
@pytest.mark.parametrize('H', [2, 12])
@pytest.mark.parametrize('group', [1, 2, 3, 5, 16])
def test_grouped_kernels(ops, group, H, Sq, Sk, p):
    _check(ops, group, H, Sq, Sk, p)


@pytest.mark.parametrize('p', [0.0, 0.1])
@pytest.mark.parametrize('group,Sq,Sk', [(3, 40, 260), (3, 30, 330), (17, 30, 260)])
def test_outside_the_grouped_kernels(ops, group, Sq, Sk, p):
    """Sq > 32, Sk > 320, group > 16: the same entry points run the ungrouped kernels on K / V tiled into the workspace and fold dK / dV --
    forward and dQ are then the ungrouped launch itself (same kernels on both sides)."""
    _check(ops, group, 2, Sq, Sk, p, same_family_fwd=True)


@pytest.mark.parametrize('Sq,Sk', [(30, 260), (12, 33)])
def test_tuning_zero_forces_the_tiled_route(ops, Sq, Sk):
    """ph_attention_tuning(0): a shape of the grouped kernels takes the tiled route (streaming kernels on both sides of the comparison)"""
    _check(ops, 3, 2, Sq, Sk, 0.1, tuning=0, same_family_fwd=True)


def test_workspace_is_demanded_only_outside_the_grouped_kernels(ops):
    import ctypes as C
    from prismer_amd import _lib
    f = _lib.AttnFwdArgs()
    f.B, f.H, f.Sq, f.Sk, f.dh = 10, 12, 30, 260, 64
    assert _lib.lib.ph_attention_group_ws_bytes(C.byref(f), 5, 1) == 0
    f.Sq = 40
    assert _lib.lib.ph_attention_group_ws_bytes(C.byref(f), 5, 0) == 2 * 10 * 260 * 768 * 2
    assert _lib.lib.ph_attention_group_ws_bytes(C.byref(f), 5, 1) == 4 * 10 * 260 * 768 * 2
    g = _lib.AttnGroupFwdArgs()
    q = torch.zeros(10 * 40, 768, dtype=BF, device='cuda')
    kv = torch.zeros(2 * 260, 1536, dtype=BF, device='cuda')
    o = torch.empty_like(q)
    lse = torch.empty(10 * 12 * 40, device='cuda')
    g.f = ops._attn_args(q, kv[:, :768], kv[:, 768:], o, 10, 12, 40, 260, 64, ((40 * 768, 768), (260 * 1536, 1536), (260 * 1536, 1536), (40 * 768, 768)),
                         0.125, None, False, None, lse)
    g.group = 5
    assert _lib.lib.ph_attention_group_fwd(C.byref(g), None) == -1          # no workspace: refused before any launch
