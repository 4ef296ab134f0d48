"""inference='generate' at the reference's eval configurations (3 beams): the parent layout -- every image tiled num_beams times, beam step as
stock tensor ops (beam_search(device_beams=False, share_image=False)) -- against the new path -- one image's K/V shared by its beams, prompt once
per image, beam step in the library (ph_beam_topk, ph_beam_advance) -- in one process, alternating, device-synchronised, after a warm-up of both.
Per arm: ms per generate call (median over all calls, and the medians of the two halves of the calls: their distance is the spread a
difference between the arms has to exceed), the peak memory the call adds (torch.cuda.max_memory_allocated), kernels per decode step, and whether
the returned token lists agree (reported, not asserted: at random-init BASE weights near-ties flip).
Kernels per step: one extra call per arm under torch.profiler; every device kernel event is counted, those whose name carries `at::` (ATen's
namespaces) or is a copy / fill of the runtime as torch's, the rest as the library's; divided by the decode steps of the call (prefill included).
ph_prof_collect's count of library ENTRY-POINT calls is printed beside it (some entry points launch two kernels).
Prismer-BASE decoder with synthetic weights, random encoder states of the leg's length (S = (res / 16)^2 + 64 resampler latents).
    python tools/generate_probe.py [--reps N] [--out FILE]        all legs
    python tools/generate_probe.py --profile [--arm new|parent]   one warm-up + one call of the first leg (for rocprofv3 --kernel-trace --stats)
    python tools/generate_probe.py --sample [--reps N] [--out FILE]   sampled decoding (top_p 0.9, n = 1 and 5 per image, caption 480^2 B=32): the
        tensor form (sample(device_sample=False)) against the device step (ph_sample_step), medians of alternating calls
    python tools/generate_probe.py --edits [--reps N] [--out FILE]    repetition_penalty / no_repeat_ngram_size on the device step: the beam and the
        sampled (n = 5) leg of caption 480^2 B=32 with (theta, n) = (1, 0) -- the plain entry points -- against (1.2, 3) -- ph_beam_topk_edit /
        ph_sample_step_edit --, alternating in one process; run it on the parent commit too (there the options are swallowed: both arms are
        "off") to compare the off arm across commits"""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from prismer_amd import _lib, config, synth
from prismer_amd.model.generate import beam_search, sample
from prismer_amd.model.prismer import _Cfg
from prismer_amd.modules.roberta import RobertaForCausalLMModified

NB = 3
# (name, resolution, images, prompt tokens (padded), ragged prompts, max_length, min_length, length_penalty)
LEGS = [('caption 480^2 B=32', 480, 32, 4, False, 20, 8, 1.0),             # prismer_caption.py:45-50: prompt 'A picture of', max_length 20, min_length 8
        ('vqa 480^2 B=32', 480, 32, 25, True, 35, 1, -1.0),                # prismer_vqa.py:52-58: questions padded to the longest, + 10 tokens, lp -1
        ('caption 224^2 B=32', 224, 32, 4, False, 20, 8, 1.0)]
ARMS = [('parent', dict(device_beams=False, share_image=False)), ('new', dict())]


def inputs(d, B, Tq, ragged, res, seed):
    g = torch.Generator().manual_seed(seed)
    S = (res // 16) ** 2 + 64
    enc = (torch.randn(B, S, d.vision_hidden_size, generator=g) * 0.5).to(torch.bfloat16).cuda()
    q = torch.randint(3, d.vocab_size, (B, Tq), generator=g); q[:, 0] = d.bos_token_id
    qa = torch.ones(B, Tq, dtype=torch.long)
    if ragged:
        for b in range(B):                                              # ragged questions, right-padded to Tq
            L = Tq - (b * 5) % max(Tq - 3, 1)
            q[b, L:] = d.pad_token_id; qa[b, L:] = 0
    return enc, q.cuda(), qa.cuda(), S


def call(dec, d, enc, q, qa, leg, kw):
    _, _, _, _, _, Tmax, Tmin, lp = leg
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    with torch.no_grad():
        out = beam_search(dec, q, qa, enc, num_beams=NB, max_length=Tmax, min_length=Tmin, eos_token_id=d.eos_token_id, pad_token_id=d.pad_token_id,
                          length_penalty=lp, **kw)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    return ms, torch.cuda.max_memory_allocated() - before, [o.tolist() for o in out]


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def kernels_per_step(dec, d, enc, q, qa, leg, kw):
    """(torch kernels, library kernels, library entry-point calls) per decode step of one call"""
    from torch.profiler import ProfilerActivity, profile
    steps = leg[5] - leg[3]
    _lib.lib.ph_prof_enable(1)
    buf = (C.c_double * 32)()
    _lib.lib.ph_prof_collect(buf)                                          # reset
    call(dec, d, enc, q, qa, leg, kw)
    _lib.lib.ph_prof_collect(buf)
    _lib.lib.ph_prof_enable(0)
    entry = sum(buf[4 * f + 3] for f in range(8))
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        call(dec, d, enc, q, qa, leg, kw)
    n_torch = n_lib = 0
    for ev in prof.key_averages():
        if str(getattr(ev, 'device_type', '')).endswith('CUDA') or getattr(ev, 'is_legacy', False):
            name = ev.key
            if 'at::' in name or 'Memcpy' in name or 'Memset' in name or 'memcpy' in name or 'fillBuffer' in name or 'copyBuffer' in name:
                n_torch += ev.count
            else:
                n_lib += ev.count
    return n_torch / steps, n_lib / steps, entry / steps


def sample_arm(dec, d, reps, say):
    """ms per sampled generate call, tensor form against device step, n = 1 and n = 5 rows per image"""
    name, res, B, Tq, ragged, Tmax, Tmin, _ = LEGS[0]
    enc, q, qa, S = inputs(d, B, Tq, ragged, res, 0)
    say(f'sampled decoding, {name}, top_p 0.9, top_k 0, temperature 1: tensor = sample(device_sample=False), device = ph_sample_step')
    say(f'{"n":>3s} {"arm":7s} {"ms/call median":>15s} {"half medians":>19s} {"steps":>6s}')
    for n in (1, 5):
        def run(kw, seed):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.no_grad():
                ids, _ = sample(dec, q, qa, enc, num_return_sequences=n, max_length=Tmax, min_length=Tmin, top_k=0, top_p=0.9,
                                eos_token_id=d.eos_token_id, pad_token_id=d.pad_token_id, seed=seed, **kw)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, ids.shape[1] - Tq
        arms = [('tensor', dict(device_sample=False)), ('device', dict())]
        for _, kw in arms:
            run(kw, 0)                                                         # warm-up of both
        times, steps = {a: [] for a, _ in arms}, {}
        for i in range(reps):                                                  # alternating, the same seed for both arms of a round
            for a, kw in arms:
                ms, steps[a] = run(kw, 1 + i)
                times[a].append(ms)
        for a, _ in arms:
            t = times[a]
            say(f'{n:3d} {a:7s} {median(t):15.2f} {median(t[:len(t) // 2]):9.2f} {median(t[len(t) // 2:]):9.2f} {steps[a]:6d}')
        say(f'{n:3d} tensor / device = {median(times["tensor"]) / median(times["device"]):.2f}x (medians)')


def edits_arm(dec, d, reps, say):
    """ms per call with the two options off (1, 0) and on (1.2, 3): beam search (3 beams) and sampled decoding (n = 5), device step"""
    leg = LEGS[0]
    name, res, B, Tq, ragged, Tmax, Tmin, lp = leg
    enc, q, qa, S = inputs(d, B, Tq, ragged, res, 0)
    arms = [('off', dict(repetition_penalty=1.0, no_repeat_ngram_size=0)), ('on', dict(repetition_penalty=1.2, no_repeat_ngram_size=3))]
    import inspect
    if 'repetition_penalty' not in inspect.signature(beam_search).parameters:     # a commit before the options: both arms are the plain step
        arms = [(a, {}) for a, _ in arms]
        say('this commit has no repetition_penalty / no_repeat_ngram_size: both arms run the plain entry points')
    say(f'{name}: off = (repetition_penalty 1, no_repeat_ngram_size 0): ph_beam_topk / ph_sample_step;  on = (1.2, 3): ph_beam_topk_edit / ph_sample_step_edit')
    say(f'{"leg":14s} {"arm":4s} {"ms/call median":>15s} {"half medians":>19s} {"spread":>8s} {"steps":>6s}')

    def beam(kw, seed):
        ms, _, out = call(dec, d, enc, q, qa, leg, kw)
        return ms, max(len(o) for o in out) - Tq

    def sampled(kw, seed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            ids, _ = sample(dec, q, qa, enc, num_return_sequences=5, max_length=Tmax, min_length=Tmin, top_k=0, top_p=0.9,
                            eos_token_id=d.eos_token_id, pad_token_id=d.pad_token_id, seed=seed, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, ids.shape[1] - Tq
    for lname, run in (('beam 3', beam), ('sampled n=5', sampled)):
        for _, kw in arms:
            run(kw, 0)                                                             # warm-up of both
        times, steps = {a: [] for a, _ in arms}, {}
        for i in range(reps):                                                      # alternating, the same seed for both arms of a round
            for a, kw in arms:
                ms, steps[a] = run(kw, 1 + i)
                times[a].append(ms)
        spread = 0.0
        for a, _ in arms:
            t = times[a]
            h0, h1 = median(t[:len(t) // 2]), median(t[len(t) // 2:])
            spread = max(spread, abs(h0 - h1))
            say(f'{lname:14s} {a:4s} {median(t):15.2f} {h0:9.2f} {h1:9.2f} {abs(h0 - h1):8.2f} {steps[a]:6d}')
        diff = median(times['on']) - median(times['off'])
        say(f'{lname:14s} on - off = {diff:+.2f} ms per call = {diff / max(steps["on"], 1) * 1e3:+.1f} us per decode step (medians; spread of the half medians {spread:.2f} ms)')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sample', action='store_true')
    ap.add_argument('--edits', action='store_true')
    ap.add_argument('--reps', type=int, default=12)
    ap.add_argument('--out', default=None)
    ap.add_argument('--profile', action='store_true')
    ap.add_argument('--arm', default='new', choices=['new', 'parent'])
    ap.add_argument('--no-kernel-count', action='store_true')
    args = ap.parse_args()
    d = config.prismer_base()
    dec = RobertaForCausalLMModified(_Cfg(d.roberta_config_dict()))
    dec.load_state_dict(synth.synth_decoder_state(d, 0))
    dec.cuda().eval()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    if args.profile:
        leg = LEGS[0]
        enc, q, qa, _ = inputs(d, leg[2], leg[3], leg[4], leg[1], 0)
        kw = dict(ARMS)[args.arm]
        call(dec, d, enc, q, qa, leg, kw)
        ms, _, _ = call(dec, d, enc, q, qa, leg, kw)
        print(f'profile: one {args.arm} generate call, {leg[0]}: {ms:.2f} ms')
        return
    reps = max(args.reps, 10)
    props = torch.cuda.get_device_properties(0)
    if args.sample or args.edits:
        say(f'device: {props.name}, {props.total_memory / 2**30:.0f} GiB; Prismer-BASE decoder (synthetic weights), random encoder states')
        (edits_arm if args.edits else sample_arm)(dec, d, reps, say)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
        return
    say(f'device: {props.name}, {props.total_memory / 2**30:.0f} GiB; Prismer-BASE decoder (synthetic weights), random encoder states, {NB} beams')
    say(f'parent = beam_search(device_beams=False, share_image=False): images tiled {NB}x, tensor-op beam step;  new = shared image K/V, device beam step')
    say(f'{"leg":20s} {"arm":7s} {"ms/call median":>15s} {"half medians":>19s} {"spread":>8s} {"peak added":>11s} {"kernels/step torch | library (entry calls)":>44s}')
    for li, leg in enumerate(LEGS):
        name, res, B, Tq, ragged = leg[:5]
        enc, q, qa, S = inputs(d, B, Tq, ragged, res, li)
        res_ = {a: call(dec, d, enc, q, qa, leg, kw) for a, kw in ARMS}            # warm-up of both
        times = {a: [] for a, _ in ARMS}
        for _ in range(reps):                                              # alternating
            for a, kw in ARMS:
                r = call(dec, d, enc, q, qa, leg, kw)
                times[a].append(r[0])
                res_[a] = r
        spread = {}
        for a, kw in ARMS:
            t = times[a]
            h0, h1 = median(t[:len(t) // 2]), median(t[len(t) // 2:])
            spread[a] = abs(h0 - h1)
            if args.no_kernel_count:
                kc = 'not counted'
            else:
                try:
                    kt, kl, ke = kernels_per_step(dec, d, enc, q, qa, leg, kw)
                    kc = f'{kt:7.1f} | {kl:7.1f} ({ke:6.1f})'
                except Exception as e:                                     # the profiler is a measuring aid, not a product path
                    kc = f'profiler unavailable: {type(e).__name__}: {e}'[:60]
            say(f'{name:20s} {a:7s} {median(t):15.2f} {h0:9.2f} {h1:9.2f} {spread[a]:8.2f} {res_[a][1] / 2**20:7.0f} MiB {kc:>44s}')
        same = sum(x == y for x, y in zip(res_['parent'][2], res_['new'][2]))
        mp, mn = median(times['parent']), median(times['new'])
        Hh, L = d.hidden_size, d.num_hidden_layers
        say(f'{name:20s} S = {S}: cross-attention K/V {B * NB * S * 2 * Hh * L * 2 / 2**20:.0f} MiB tiled, {B * S * 2 * Hh * L * 2 / 2**20:.0f} MiB shared; '
            f'parent / new = {mp / mn:.2f}x (medians; difference {mp - mn:.2f} ms against a spread of {max(spread.values()):.2f} ms); '
            f'token lists agree for {same}/{B} items')
        del enc, q, qa, res_
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
