"""Golden-case definitions shared by make_golden.py (runs the REFERENCE, build container only) and the tests
(which regenerate the identical weights / inputs from prismer_amd.synth and compare against the stored
reference outputs)."""
import io
import os
import random
from collections import OrderedDict

import numpy as np
import torch

from prismer_amd import config, synth

INSTANCE_SEED = 7     # random.seed before every encoder call: vit.py:145-147 draws from Python's `random`

GOLD = os.path.dirname(os.path.abspath(__file__))
PART_BYTES = 960 * 1024      # every committed file stays below 1 MiB: a fixture is stored as <name>.npz or as parts <name>.<i>.npz


def _zsize(arrays):
    b = io.BytesIO()
    np.savez_compressed(b, **arrays)
    return b.tell()


def save(name, arrays):
    """Writes the fixture `name` as compressed parts below PART_BYTES each: one <name>.npz when it fits, otherwise <name>.0.npz,
    <name>.1.npz, ...; an array too large for one part is cut along axis 0 into entries '<key>@<j>'.  load() reassembles it exactly."""
    for p in [os.path.join(GOLD, name + '.npz')] + [os.path.join(GOLD, f'{name}.{i}.npz') for i in range(1000)]:
        if os.path.isfile(p):
            os.remove(p)
    items = []                                             # (key, array, compressed size on its own)
    for k, v in arrays.items():
        v = np.asarray(v)
        z = _zsize({k: v})
        n = -(-z // (PART_BYTES // 2))
        if n == 1:
            items.append((k, v, z))
        else:
            assert v.ndim >= 1 and v.shape[0] >= n, (name, k, v.shape)
            items += [(f'{k}@{j}', c, _zsize({k: c})) for j, c in enumerate(np.array_split(v, n))]
    parts, cur, used = [], {}, 0
    for k, v, z in items:
        if cur and used + z > PART_BYTES:
            parts.append(cur)
            cur, used = {}, 0
        cur[k] = v
        used += z
    parts.append(cur)
    paths = [os.path.join(GOLD, name + '.npz')] if len(parts) == 1 else [os.path.join(GOLD, f'{name}.{i}.npz') for i in range(len(parts))]
    for p, part in zip(paths, parts):
        np.savez_compressed(p, **part)
        assert os.path.getsize(p) < 1 << 20, p
    return paths


def load(name):
    """{key: array} of the fixture `name` (see save())."""
    p = os.path.join(GOLD, name + '.npz')
    paths = [p] if os.path.isfile(p) else []
    while not os.path.isfile(p) and os.path.isfile(os.path.join(GOLD, f'{name}.{len(paths)}.npz')):
        paths.append(os.path.join(GOLD, f'{name}.{len(paths)}.npz'))
    if not paths:
        raise FileNotFoundError(f'no fixture {name} under {GOLD}')
    out, chunks = {}, {}
    for path in paths:
        with np.load(path) as z:
            for k in z.files:
                base, sep, j = k.rpartition('@')
                if sep:
                    chunks.setdefault(base, []).append((int(j), z[k]))
                    out.setdefault(base, None)
                else:
                    out[k] = z[k]
    for k, cs in chunks.items():
        out[k] = np.concatenate([c for _, c in sorted(cs, key=lambda t: t[0])])
    return out


def _dims(name):
    if name in ('tiny_caption', 'tiny_vqa', 'tiny_vqa_head'):
        return config.prismer_tiny()
    if name == 'tiny_bicubic':            # rgb grid 6x6 vs expert grid 4x4 -> bicubic pos-embed path (utils.py:34-44)
        return config.prismer_tiny(image_resolution=96, expert_resolution=64)
    if name == 'tiny_z':                  # PrismerZ: rgb only, no resampler (vit.py:125,128)
        return config.prismer_tiny(experts=[])
    if name in ('base_caption', 'base_b8', 'base_b32'):
        return config.prismer_base()
    if name in ('zbase_b4', 'zbase_b32'):  # BASELINE config 2 geometry: PrismerZ-BASE, full depth
        return config.prismerz_base()
    if name == 'huge_b1':                 # configs/prismer.json:50-73 + ViT-H/14 (vit.py:211-214): width 1280, 32 + 24 layers, resampler head dim 160
        return config.prismer_huge()
    if name in ('large_vqa_b1', 'large_vqa_b4', 'large_vqa_b16'):            # BASELINE config 5 geometry: Prismer-LARGE VQA, 480^2, full depth (24 + 24 layers)
        return config.prismer_large()
    raise KeyError(name)


CASES = OrderedDict([
    # name            : (batch, T, ragged)
    ('tiny_caption', (2, 12, True)),
    ('tiny_vqa', (3, 14, True)),
    ('tiny_bicubic', (2, 10, False)),
    ('tiny_z', (2, 12, True)),
    ('base_caption', (1, 30, False)),
    # round 2: the sizes bench.py runs (full depth, batch > 1); train-mode + gradients are what the Trainer tests compare
    ('base_b8', (8, 30, True)),
    ('zbase_b4', (4, 30, True)),
    ('large_vqa_b1', (1, 40, False)),
    # question ‖ answer exactly as PrismerVQA.forward concatenates them (prismer_vqa.py:22-33): each part padded to ITS longest,
    # so pads sit in the middle of a row
    ('tiny_vqa_head', (3, 9 + 5, True)),
    # round 3: EXACTLY the configuration bench.py times (BASELINE config 3: Prismer-BASE, bs32, T=30) -- at this batch the GEMM dispatch
    # selects the 256x128 ping-pong kernel and the grouped persistent weight-gradient kernel, which B=8 never reaches
    ('base_b32', (32, 30, True)),
    # round 4: config 5 at a batch where the dispatch picks the 256x128 / grouped kernels UNFORCED (B=1 had to force them); ragged rows
    ('large_vqa_b4', (4, 40, True)),
    # round 5: Prismer-HUGE geometry (the pre-train recipe's largest model): one sample, full depth
    ('huge_b1', (1, 30, False)),
    # round 6: every benchmarked leg at ITS benchmarked batch (the GEMM dispatch -- tile choice, split-K, tail split -- depends on M = B * S):
    # config 2 at bs32, config 5 at bs16
    ('zbase_b32', (32, 30, True)),
    ('large_vqa_b16', (16, 40, True)),
])

LOGIT_STRIDE = {'base_caption': 97, 'base_b8': 97, 'zbase_b4': 97, 'large_vqa_b1': 97, 'base_b32': 97, 'large_vqa_b4': 97, 'huge_b1': 97, 'zbase_b32': 97, 'large_vqa_b16': 97}    # every 97th vocab column for the big cases
ENC_STRIDE = {'base_b8': 16, 'zbase_b4': 8, 'large_vqa_b1': 16, 'base_b32': 16, 'large_vqa_b4': 16, 'huge_b1': 16, 'zbase_b32': 16, 'large_vqa_b16': 32}                             # every n-th feature of the encoder output
VQA_CASES = ('tiny_vqa', 'large_vqa_b1', 'large_vqa_b4', 'large_vqa_b16')
VQA_HEAD_TQ, VQA_HEAD_TA = 9, 5
DROP_CASES = ('tiny_caption', 'base_b8', 'base_b32')     # (base_b32: round 6, the headline's exact arithmetic) <case>_drop.npz: reference outputs in full training mode under the library's dropout masks (round 5)
TRAJ_CASES = ('base_b8',)                   # <case>_traj.npz: TRAJ_STEPS AdamW steps of the reference loop (train_caption.py:111-112,126-135) under the library's masks (round 6)
TRAJ_STEPS, TRAJ_TOTAL = 4, 10              # cosine schedule over TRAJ_TOTAL iterations, init_lr / min_lr / weight_decay of configs/caption.yaml:12-14
TRAJ_LR, TRAJ_MIN_LR, TRAJ_WD = 5e-5, 0.0, 0.05
DROP_SEED = 0x5EED0123456789AB              # device dropout seed of step 1; step 2 uses splitmix64 of it (csrc/optim.hip advance_seed_kernel)


class Case:
    def __init__(self, name):
        self.name = name
        self.dims = _dims(name)
        self.batch, self.T, self.ragged = CASES[name]
        self.seed = 0

    def weights(self):
        return synth.synth_encoder_state(self.dims, self.seed), synth.synth_decoder_state(self.dims, self.seed)

    def inputs(self):
        d = self.dims
        x = synth.synth_experts(d, self.batch, seed=1234)
        prompt = 4
        if self.name == 'tiny_vqa_head':
            q_ids, q_att, a_ids, a_att, weights = self.vqa_parts()
            ids, mask = torch.cat([q_ids, a_ids], 1), torch.cat([q_att, a_att], 1)
            labels = ids.masked_fill(ids == d.pad_token_id, -100)
            labels[:, :-a_ids.shape[1]] = -100
            return x, ids, mask, labels, weights
        if self.name in VQA_CASES:        # prismer_vqa.py:32-33: everything but the answer span is -100
            ids, mask, labels = synth.synth_text(d, self.batch, self.T, seed=1234, ragged=self.ragged, prompt_length=1)
            ans = 4 if self.name == 'tiny_vqa' else 5
            for b in range(self.batch):
                L = int(mask[b].sum())
                labels[b, :max(0, L - ans)] = -100
            weights = 0.6 + 0.4 * synth.uniform_pm1('in.vqa_w', (self.batch,), 1234)
            return x, ids, mask, labels, weights
        ids, mask, labels = synth.synth_text(d, self.batch, self.T, seed=1234, ragged=self.ragged, prompt_length=prompt)
        return x, ids, mask, labels, None

    def vqa_parts(self):
        """what the tokenizer calls of prismer_vqa.py:22-30 return: '<s>Question' ids (no </s>, ragged, padded to longest) and
        ' Answer</s>' ids (ragged, padded to longest), with their attention masks, plus the per-sample loss weights"""
        d = self.dims
        Tq, Ta = VQA_HEAD_TQ, VQA_HEAD_TA
        q = synth.randint('in.vqa_q', (self.batch, Tq), 3, d.vocab_size, 1234)
        a = synth.randint('in.vqa_a', (self.batch, Ta), 3, d.vocab_size, 1234)
        q[:, 0] = d.bos_token_id
        qa, aa = torch.ones_like(q), torch.ones_like(a)
        for b in range(self.batch):
            lq, la = Tq - (2 * b) % (Tq - 2), Ta - b % (Ta - 1)
            q[b, lq:] = d.pad_token_id; qa[b, lq:] = 0
            a[b, la - 1] = d.eos_token_id
            a[b, la:] = d.pad_token_id; aa[b, la:] = 0
        weights = 0.6 + 0.4 * synth.uniform_pm1('in.vqa_w', (self.batch,), 1234)
        return q, qa, a, aa, weights

    def instance_table(self, x):
        """The table the reference's per-label random.randint draws produce after random.seed(INSTANCE_SEED)."""
        if 'obj_detection' not in x:
            return None
        rng = random.Random(INSTANCE_SEED)
        table = [0] * 256
        for l in x['obj_detection']['instance'].unique().tolist():
            table[int(l)] = rng.randint(0, 127)
        return table


# parameters whose FULL gradient is stored (the rest: L2 norm + 16 sampled entries)
FULL_GRAD_KEYS = (
    'expert_encoder.resampler.latents',
    'expert_encoder.ln_pre.weight',
    'expert_encoder.conv1.depth.2.weight',
    'expert_encoder.transformer.resblocks.0.1.adaptor.down_proj.bias',
    'text_decoder.lm_head.dense.bias',
    'text_decoder.roberta.encoder.layer.0.1.self.key.bias',
    'text_decoder.roberta.embeddings.LayerNorm.weight',
)


def sample_idx(key, numel, n=16):
    return synth.randint('gidx.' + key, (n,), 0, numel, 0)


# ---------------------------------------------------------------------------------------------------------------------------
# Random projections of every gradient tensor (round 3).  16 sampled entries + the L2 norm cannot see a gradient that has the
# right norm and the wrong direction; N_PROJ fixed pseudo-random directions r_j (entries U(-1,1), integer-hash generated so
# that the CPU fixture script and the GPU test build the SAME vectors, on whichever device the gradient lives) can:
# for an error tensor e,  <e, r_j> ~ N(0, |e|^2 / 3), so  sqrt(3 * mean_j <e, r_j>^2)  estimates the FULL-tensor Frobenius error.
N_PROJ = 16


def _mix32(x):
    """32-bit integer hash (xorshift-multiply), evaluated in int64 with explicit masks: exact on CPU and GPU alike."""
    m = 0xFFFFFFFF
    x = x & m
    x = ((x ^ (x >> 16)) * 0x7FEB352D) & m
    x = ((x ^ (x >> 15)) * 0x846CA68B) & m
    return x ^ (x >> 16)


def proj_direction(key, numel, j, device='cpu', lo=0, hi=None):
    """entries [lo, hi) of direction j for the gradient called `key`: float64 in [-1, 1), 24 random bits each"""
    import zlib
    hi = numel if hi is None else hi
    k0 = (zlib.crc32(('gproj.' + key).encode()) * 0x9E3779B1 + 0x85EBCA6B * (j + 1)) & 0xFFFFFFFF
    i = torch.arange(lo, hi, dtype=torch.int64, device=device)
    h = _mix32(_mix32(i + k0) + (i >> 32) + 0x27D4EB2F * (j + 1))
    return (h >> 8).double() / float(1 << 23) - 1.0


def grad_projections(key, g, chunk=1 << 24):
    """[N_PROJ] float64: <g, r_j>, accumulated in fp64 on g's device"""
    flat = g.detach().reshape(-1)
    out = torch.zeros(N_PROJ, dtype=torch.float64, device=flat.device)
    for lo in range(0, flat.numel(), chunk):
        hi = min(flat.numel(), lo + chunk)
        part = flat[lo:hi].double()
        for j in range(N_PROJ):
            out[j] += torch.dot(part, proj_direction(key, flat.numel(), j, flat.device, lo, hi))
    return out.cpu().numpy()


def projected_error(p_got, p_ref):
    """estimate of |g_got - g_ref|_F from the two projection vectors"""
    import numpy as np
    d = np.asarray(p_got, dtype=np.float64) - np.asarray(p_ref, dtype=np.float64)
    return float(np.sqrt(3.0 * np.mean(d * d)))
