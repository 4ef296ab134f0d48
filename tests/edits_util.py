"""Shared by tests/test_decode_edits_cpu.py and tests/test_decode_edits_gpu.py: the (repetition_penalty, no_repeat_ngram_size) settings, the
installed transformers processors as a reference for prismer_amd/model/generate.py::decode_edits, wrappers that apply them to the
log-probabilities a loop-form oracle asks for, a toy language model that likes to repeat itself, and planted histories."""
import torch

from tests.test_generate_cpu import make_lm

GPU_EDITS = [(1.3, 0), (1.0, 2), (0.8, 3), (2.5, 1)]                   # (theta, n) of the kernel tests
BEAM_EDITS = [(1.3, 0), (1.0, 2), (1.3, 2), (0.7, 3)]                  # (theta, n) of the beam-search tests
EOS, PAD = 2, 1


def hf_edit(ids, scores, theta, n):
    """transformers' RepetitionPenaltyLogitsProcessor then NoRepeatNGramLogitsProcessor (the order of generate's processor list) on
    scores [R, V] with history ids [R, cur]; banned columns come back as -inf"""
    from transformers import NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor
    s = scores.clone()
    if float(theta) != 1.0:
        s = RepetitionPenaltyLogitsProcessor(float(theta))(ids, s)
    if n > 0:
        s = NoRepeatNGramLogitsProcessor(int(n))(ids, s.clone())
    return s


def wrap_list_step(step_list, theta, n, cover):
    """step_list(rows) -> log-probabilities as lists (the interface of oracle/beam_oracle.py) with transformers' processors applied to
    them in fp32; cover['banned'] counts the columns the n-gram rule removed"""
    def step(rows):
        lp = torch.tensor(step_list(rows), dtype=torch.float32)
        out = hf_edit(torch.tensor(rows), lp, theta, n)
        cover['banned'] += int((torch.isinf(out) & ~torch.isinf(lp)).sum())
        return out.tolist()
    return step


def count_repeats(rows, T0, eos=None, pad=None):
    """generated tokens (position >= T0, EOS / pad excluded) that already stood earlier in their row: each was a penalised candidate when
    it was chosen"""
    n = 0
    for row in rows:
        for t in range(T0, len(row)):
            if row[t] not in (eos, pad) and row[t] in row[:t]:
                n += 1
    return n


def repeat_lm(V, seed, eos_boost, boost=3.0):
    """make_lm's table model with `boost` added to the logit of the last-but-one token: a repeat tendency.  Logits rounded to bf16."""
    lm = make_lm(V, seed, EOS, eos_boost)

    def logits(ids):
        z = lm(ids)
        if ids.shape[1] > 1:
            z[torch.arange(ids.shape[0]), ids[:, -2]] += boost
        return z.bfloat16()
    return logits


def planted_history(V, cur, R, seed, n):
    """int64 [R, cur]: tokens the kernels' boundaries care about -- columns 0 and V - 1, one in the last partial 8-vector, block and vector
    boundaries 1023 / 1024 / 8191 / 8192 where V allows, EOS, pad, a duplicate, an id >= V (and a negative one) -- in a row-dependent
    order, filled up from a nine-token alphabet (at most 14 distinct tokens inside any vocabulary: a row of 23 keeps candidates), then for
    cur >= 4 an n-gram repeat at the suffix: the last n - 1 tokens also stand earlier in the row, followed by a token that the rule must ban"""
    pool = [0, V - 1, V - 3, EOS, PAD, 5, 5, V + 7, -4] + [c for c in (1023, 1024, 8191, 8192) if c < V - 3]
    g = torch.Generator().manual_seed(seed)
    out = torch.empty(R, cur, dtype=torch.long)
    for r in range(R):
        perm = torch.randperm(len(pool), generator=g).tolist()
        row = [pool[i] for i in perm]
        while len(row) < cur:
            row.append(int(torch.randint(3, 12, (1,), generator=g)))
        row = row[:cur]
        m = max(n - 1, 1)
        if cur >= 2 * m + 2:                                               # ... suffix s, earlier "s followed by w": w is banned for n = m + 1
            row[1:1 + m] = row[cur - m:]
        out[r] = torch.tensor(row)
    return out
