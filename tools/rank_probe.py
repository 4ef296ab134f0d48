"""inference='rank' at the reference's eval configurations: the shared-prefix path (prismer_amd/model/rank.py) against the tiled one, in one process,
alternating.  Per leg: device-synchronised ms per rank call after warm-up (the decoder part: both paths get the same encoder states, whose
forward is identical in both), the peak memory the call adds (torch.cuda.max_memory_allocated), and whether the chosen answers agree.
Prismer-BASE decoder with synthetic weights, random encoder states of the leg's length (S = (res / 16)^2 + 64 resampler latents).
    python tools/rank_probe.py [--reps N] [--out FILE]          all legs
    python tools/rank_probe.py --profile                        one warm-up + one shared call of the first leg (for rocprofv3 --kernel-trace --stats)"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from prismer_amd import config, synth
from prismer_amd.model import rank as RK
from prismer_amd.model.prismer import _Cfg
from prismer_amd.modules.roberta import RobertaForCausalLMModified

# (name, resolution, images B, candidates n, k, question tokens Tq (padded), answer tokens Ta (padded))
LEGS = [('vqa 480^2 B=32 k=16', 480, 32, 3128, 16, 25, 8),                # configs/vqa.yaml: k_test 16, batch_size_test 32
        ('vqa 480^2 B=32 k=128', 480, 32, 3128, 128, 25, 8),              # PrismerVQA.forward's default k_test
        ('classification 384^2 B=8 n=1000 k=32', 384, 8, 1000, 32, 5, 8)]   # 1-shot ImageNet: 1000 class names, prompt 'A picture of a'


def inputs(d, B, n, Tq, Ta, res, seed):
    g = torch.Generator().manual_seed(seed)
    S = (res // 16) ** 2 + 64
    enc = (torch.randn(B, S, d.vision_hidden_size, generator=g) * 0.5).to(torch.bfloat16).cuda()
    q = torch.randint(3, d.vocab_size, (B, Tq), generator=g); q[:, 0] = d.bos_token_id
    qa = torch.ones(B, Tq, dtype=torch.long)
    for b in range(B):                                                  # ragged questions, right-padded to Tq
        L = Tq - (b * 5) % max(Tq - 3, 1)
        q[b, L:] = d.pad_token_id; qa[b, L:] = 0
    a = torch.randint(3, d.vocab_size, (n, Ta), generator=g)
    aa = torch.ones(n, Ta, dtype=torch.long)
    for i in range(n):                                                  # ragged answers ending in </s>
        L = 2 + i % (Ta - 1)
        a[i, L - 1] = d.eos_token_id
        a[i, L:] = d.pad_token_id; aa[i, L:] = 0
    return enc, [t.cuda() for t in (q, qa, a, aa)]


def tiled_footprint(d, B, S, k, Tq, Ta):
    """bytes of the tiled path's largest transient buffers: merged cross-attention K/V, tiled encoder states, logits"""
    R, L, H = B * k, d.num_hidden_layers, d.hidden_size
    vpad = (d.vocab_size + 63) // 64 * 64
    return R * S * 2 * H * L * 2 + R * S * d.vision_hidden_size * 2 + R * (Tq + Ta) * vpad * 2


def call(fn, dec, enc, args, k, pad):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    with torch.no_grad():
        topk, lp = fn(dec, enc, *args, k, pad)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    return ms, torch.cuda.max_memory_allocated() - before, topk, lp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--profile', action='store_true')
    args = ap.parse_args()
    d = config.prismer_base()
    dec = RobertaForCausalLMModified(_Cfg(d.roberta_config_dict()))
    dec.load_state_dict(synth.synth_decoder_state(d, 0))
    dec.cuda().eval()
    pad = d.pad_token_id
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    if args.profile:
        name, res, B, n, k, Tq, Ta = LEGS[0]
        enc, a = inputs(d, B, n, Tq, Ta, res, 0)
        call(RK._rank_shared, dec, enc, a, k, pad)
        ms, _, _, _ = call(RK._rank_shared, dec, enc, a, k, pad)
        print(f'profile: one shared rank call, {name}: {ms:.2f} ms')
        return
    props = torch.cuda.get_device_properties(0)
    say(f'device: {props.name}, {props.total_memory / 2**30:.0f} GiB; Prismer-BASE decoder (synthetic weights), random encoder states')
    say(f'{"leg":40s} {"path":7s} {"ms/call (min / median)":>24s} {"peak added":>12s}  chosen answers')
    for li, (name, res, B, n, k, Tq, Ta) in enumerate(LEGS):
        S = (res // 16) ** 2 + 64
        enc, a = inputs(d, B, n, Tq, Ta, res, li)
        foot = tiled_footprint(d, B, S, k, Tq, Ta)
        free, _ = torch.cuda.mem_get_info()
        run_tiled = foot < 0.5 * free
        paths = [('shared', RK._rank_shared)] + ([('tiled', RK._rank_tiled)] if run_tiled else [])
        res_ = {p: call(fn, dec, enc, a, k, pad) for p, fn in paths}          # warm-up
        times = {p: [] for p, _ in paths}
        for _ in range(args.reps):                                      # alternating
            for p, fn in paths:
                ms, peak, topk, lp = call(fn, dec, enc, a, k, pad)
                times[p].append(ms)
                res_[p] = (ms, peak, topk, lp)
        chosen = {p: r[2][torch.arange(B, device=r[2].device), r[3].argmax(1)] for p, r in res_.items()}
        for p, _ in paths:
            t = sorted(times[p])
            agree = ''
            if p == 'tiled':
                same = chosen['tiled'] == chosen['shared']
                lp = res_['tiled'][3].float()
                top2 = lp.topk(2, dim=1).values
                gap = (top2[:, 0] - top2[:, 1])[~same]
                agree = f'{int(same.sum())}/{B} agree with shared' + (f' (tiled margins where not: {[round(float(x), 4) for x in gap]})' if (~same).any() else '')
            say(f'{name:40s} {p:7s} {t[0]:10.2f} / {t[len(t) // 2]:10.2f} {res_[p][1] / 2**30:10.2f} GiB  {agree}')
        if not run_tiled:
            say(f'{name:40s} tiled   not run: computed footprint {foot / 1e9:.1f} GB (K/V + tiled encoder states + logits) against {free / 1e9:.1f} GB free')
        else:
            say(f'{name:40s} tiled   computed footprint {foot / 1e9:.1f} GB; speed-up shared over tiled {sorted(times["tiled"])[len(times["tiled"]) // 2] / sorted(times["shared"])[len(times["shared"]) // 2]:.2f}x (medians)')
        del enc, a, res_
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
