"""Test helpers: error metrics and a numpy Philox4x32-7 mirror of csrc/common.h (dropout masks)."""
import numpy as np
import torch


def rel_fro(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def max_abs(a, b):
    return (a.detach().double().cpu() - b.detach().double().cpu()).abs().max().item()


def bf16_round(x):
    return x.to(torch.bfloat16).to(torch.float32)


def _mulhilo(a, b):
    p = a.astype(np.uint64) * np.uint64(b)
    return (p >> np.uint64(32)).astype(np.uint32), (p & np.uint64(0xFFFFFFFF)).astype(np.uint32)


PHILOX_ROUNDS = 7


def philox4x32(c0, c1, c2, c3, k0, k1):
    """vectorised Philox4x32 with PHILOX_ROUNDS rounds (= PH_PHILOX_ROUNDS of csrc/common.h); counters are numpy uint32 arrays, keys python ints.
    Returns 4 uint32 arrays."""
    c0 = c0.astype(np.uint32); c1 = np.broadcast_to(np.uint32(c1), c0.shape).copy() if np.isscalar(c1) else c1.astype(np.uint32)
    c2 = np.broadcast_to(np.uint32(c2), c0.shape).copy() if np.isscalar(c2) else c2.astype(np.uint32)
    c3 = np.broadcast_to(np.uint32(c3), c0.shape).copy() if np.isscalar(c3) else c3.astype(np.uint32)
    k0 = np.uint32(k0 & 0xFFFFFFFF); k1 = np.uint32(k1 & 0xFFFFFFFF)
    for _ in range(PHILOX_ROUNDS):
        hi0, lo0 = _mulhilo(c0, 0xD2511F53)
        hi1, lo1 = _mulhilo(c2, 0xCD9E8D57)
        n0 = hi1 ^ c1 ^ k0; n1 = lo1; n2 = hi0 ^ c3 ^ k1; n3 = lo0
        c0, c1, c2, c3 = n0, n1, n2, n3
        k0 = np.uint32((int(k0) + 0x9E3779B9) & 0xFFFFFFFF); k1 = np.uint32((int(k1) + 0xBB67AE85) & 0xFFFFFFFF)
    return c0, c1, c2, c3


def dropout_keep_linear(n_elems, seed, stream, p):
    """keep mask (bool [n_elems]) for the GEMM-epilogue / LayerNorm / embedding dropout: element i uses word i%4 of
    philox(counter=(i/4 lo, i/4 hi, stream, 0x5eed), key=seed)."""
    assert n_elems % 4 == 0
    idx4 = np.arange(n_elems // 4, dtype=np.uint64)
    r = philox4x32((idx4 & 0xFFFFFFFF).astype(np.uint32), (idx4 >> 32).astype(np.uint32), stream, 0x5eed,
                   seed & 0xFFFFFFFF, seed >> 32)
    r = np.stack(r, axis=1).reshape(-1)
    thr = np.uint32(int(np.float32(p) * np.float32(16777216.0)))
    return torch.from_numpy((r >> np.uint32(8)) >= thr)


def dropout_keep_attention(BH, Sq, Sk, seed, stream, p):
    """keep mask [BH, Sq, Sk] for attention-probability dropout: philox(counter=(key/4, row id, stream, 0xa77e))."""
    k4 = (Sk + 3) // 4
    rows = np.arange(BH * Sq, dtype=np.uint32)
    c0 = np.tile(np.arange(k4, dtype=np.uint32), BH * Sq)
    c1 = np.repeat(rows, k4)
    r = philox4x32(c0, c1, stream, 0xa77e, seed & 0xFFFFFFFF, seed >> 32)
    r = np.stack(r, axis=1).reshape(BH * Sq, k4 * 4)[:, :Sk]
    thr = np.uint32(int(np.float32(p) * np.float32(16777216.0)))
    return torch.from_numpy((r >> np.uint32(8)) >= thr).reshape(BH, Sq, Sk)


SITE_STREAM = {'self_probs': 1, 'self_out': 2, 'cross_probs': 3, 'cross_out': 4, 'mlp_out': 5}     # programs/decoder.py: li * 16 + k; embeddings: 9000


class LibraryDropout:
    """`drop(site, x)` for oracle.text_decoder / the patched reference modules with EXACTLY the masks libprismer_hip draws for `seed`:
    hidden-state sites use the linear scheme (element i of the [B*T, H] matrix -> word i % 4 of philox(i / 4, stream)), attention-probability
    sites the (row = (b * heads + h) * Sq + q, key / 4) scheme; stream = layer * 16 + k (programs/decoder.py), 9000 for the embeddings.
    Scaling 1 / (1 - p) with p rounded like the kernels do (threshold = int(p * 2^24))."""

    def __init__(self, seed, p_hidden, p_attn, site_base=0):
        self.seed, self.p_hidden, self.p_attn, self.site_base = int(seed) & 0xFFFFFFFFFFFFFFFF, float(p_hidden), float(p_attn), site_base
        self.calls = []

    def __call__(self, site, x):
        self.calls.append(site)
        if site == ('emb',):
            stream, p, attn = 9000, self.p_hidden, False
        else:
            layer, kind = site
            stream, attn = layer * 16 + SITE_STREAM[kind], kind.endswith('_probs')
            p = self.p_attn if attn else self.p_hidden
        if p <= 0.0:
            return x
        stream += self.site_base
        if attn:
            B, H, Sq, Sk = x.shape
            keep = dropout_keep_attention(B * H, Sq, Sk, self.seed, stream, p).reshape(B, H, Sq, Sk)
        else:
            keep = dropout_keep_linear(x.numel(), self.seed, stream, p).reshape(x.shape)
        return x * keep.to(x.dtype) / (1.0 - p)


def splitmix64(z):
    """csrc/optim.hip advance_seed_kernel: the dropout seed of step k+1 from the seed of step k"""
    m = 0xFFFFFFFFFFFFFFFF
    z = (z + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


# ---------------------------------------------------------------------------------------------- attention: per-row checks
# A float64 reference, a float64 emulation that rounds where the bf16 kernels round, and a per-row metric.  Plain torch, any device.
# Layout of every tensor: [B, H, S, dh]; every result is float64 (lse: [B, H, Sq]).
def bf16_round64(x):
    return x.to(torch.bfloat16).to(torch.float64)


def attn_live(B, H, Sq, Sk, key_mask=None, causal=False, device='cpu'):
    """bool [B, H, Sq, Sk]: the keys a query may see (attn_ref of test_kernels_gpu: tril for the causal cut, & key mask)"""
    m = torch.ones(Sq, Sk, dtype=torch.bool, device=device)
    if causal:
        m = torch.tril(m)
    m = m[None, None].expand(B, H, Sq, Sk).clone()
    if key_mask is not None:
        m &= key_mask.to(device).bool()[:, None, None, :]
    return m


def _attn_scores(q, k, scale, live):
    s = q.double() @ k.double().transpose(-1, -2) * scale
    return s.masked_fill(~live, torch.finfo(torch.float32).min)      # a row with no live key: uniform over the Sk keys, like attn_ref


def _keep_scale(keep, p, like):
    if keep is None:
        return None
    return keep.to(like.device).reshape(like.shape).double() / (1.0 - p)


def attn_ref64(q, k, v, d_o, scale, key_mask=None, causal=False, keep=None, p=0.0, live=None):
    """attn_ref in float64 on the values handed in (bf16-rounded by the caller), gradients in closed form.  `live` overrides the mask built
    from key_mask / causal.  Returns dict(o, lse, dq, dk, dv); d_o = None leaves the gradients out.  Like autograd through masked_fill,
    no gradient reaches an excluded score."""
    B, H, Sq, _ = q.shape
    Sk = k.shape[2]
    if live is None:
        live = attn_live(B, H, Sq, Sk, key_mask, causal, q.device)
    s = _attn_scores(q, k, scale, live)
    lse = torch.logsumexp(s, dim=-1)
    pr = torch.softmax(s, dim=-1)                                    # (not exp(s - lse): lse of a row with no live key saturates at finfo.min)
    ks = _keep_scale(keep, p, pr)
    prd = pr if ks is None else pr * ks
    out = dict(o=prd @ v.double(), lse=lse)
    if d_o is None:
        return out
    d_o = d_o.double()
    dp = d_o @ v.double().transpose(-1, -2)
    if ks is not None:
        dp = dp * ks
    ds = pr * (dp - (pr * dp).sum(-1, keepdim=True)) * live
    out.update(dq=ds @ k.double() * scale, dk=ds.transpose(-1, -2) @ q.double() * scale, dv=prd.transpose(-1, -2) @ d_o)
    return out


def attn_emulated(q, k, v, d_o, scale, key_mask=None, causal=False, keep=None, p=0.0, live=None):
    """The operation of attn_ref64 in float64 with the roundings of a bf16 flash-attention kernel put in: P (after dropout) to bf16 before P V and
    before P^T dO, o to bf16, delta = rowsum(dO * o) from the rounded o, lse to fp32 (the backward recomputes P from it), dS to bf16 before
    dS K and dS^T Q, every output to bf16.  It says how far a correct kernel may be from attn_ref64 and never sees a kernel."""
    B, H, Sq, _ = q.shape
    Sk = k.shape[2]
    if live is None:
        live = attn_live(B, H, Sq, Sk, key_mask, causal, q.device)
    s = _attn_scores(q, k, scale, live)
    mx = s.max(-1, keepdim=True).values
    pu = torch.exp(s - mx)                                           # unnormalised, <= 1: what goes into the P V product
    lsum = pu.sum(-1, keepdim=True)
    ks = _keep_scale(keep, p, pu)
    o = bf16_round64((bf16_round64(pu if ks is None else pu * ks) @ v.double()) / lsum)
    lse = (mx[..., 0] + torch.log(lsum[..., 0])).float().double()
    out = dict(o=o, lse=lse)
    if d_o is None:
        return out
    d_o = d_o.double()
    pr = torch.exp(s - lse[..., None])
    dv = bf16_round64(bf16_round64(pr if ks is None else pr * ks).transpose(-1, -2) @ d_o)
    dp = d_o @ v.double().transpose(-1, -2)
    if ks is not None:
        dp = dp * ks
    delta = (d_o * o).sum(-1, keepdim=True)
    ds = bf16_round64(pr * (dp - delta) * live)
    out.update(dq=bf16_round64(ds @ k.double() * scale), dk=bf16_round64(ds.transpose(-1, -2) @ q.double() * scale), dv=dv)
    return out


def row_err(got, ref):
    """max over rows r of |got_r - ref_r| / max(|ref_r|, median_r |ref_r|) for 2-D [rows, n] tensors.  The median floor: some rows are zero or
    nearly zero in the reference (dq of the first causal query rows) and their error scales with the other rows' size.  A zero median
    (Sq = 1 under a causal cut: every dq row is zero) demands equality: 0.0 if equal, else inf."""
    assert got.dim() == 2 and got.shape == ref.shape, (got.shape, ref.shape)
    got, ref = got.detach().double(), ref.detach().double()
    n = ref.norm(dim=1)
    med = n.median()
    if med.item() == 0.0:
        return 0.0 if torch.equal(got, ref) else float('inf')
    return ((got - ref).norm(dim=1) / torch.maximum(n, med)).max().item()


def lse_err(lse, lse_ref, live_rows=None):
    """max |lse - lse_ref| over the rows with at least one live key (bool mask of the shape of lse; None = all rows)"""
    d = (lse.detach().double() - lse_ref.detach().double()).abs()
    if live_rows is not None:
        d = d[live_rows.to(d.device)]
    return d.max().item()


def lse_floor32(q, k, scale, live):
    """lse_err of torch.logsumexp in float32 on the same masked scores: the float32 floor the lse bound is a multiple of"""
    s = _attn_scores(q, k, scale, live)
    rows = live.any(-1)
    return lse_err(torch.logsumexp(s.float(), dim=-1), torch.logsumexp(s, dim=-1), rows)
