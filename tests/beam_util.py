"""Shared by tests/test_beam_abi_cpu.py and tests/test_beam_device_gpu.py: the toy language models of the beam-search tests with their
logits rounded to bf16, the library's tie rule as a `topk_fn` that also checks each case's precondition, and the chosen cases.

Ties and near-ties.  The reference side always orders by the library's rule: score descending, flat index beam * V + token ascending
(a stable descending sort).  Exact ties inside one row are harmless: the kernel gives equal bf16 logits of a row bit-equal scores
and breaks them alike.  What could differ is a pair the reference separates by less than the kernel's log-sum-exp rounding (fp32, of
order 1e-6 at |lse| = 10 .. 30).  So a case is only valid if, in the REFERENCE run, every adjacent pair among the first 2*nb + 1
candidates of a live item is exactly equal and from the same beam, or at least 1e-4 apart.  A case that violates this fails loudly."""
import torch

from prismer_amd.model.generate import stable_topk
from tests.test_generate_cpu import make_lm

GAP = 1e-4
PAIRS = [(1.0, 0.0), (1.0, 2.5), (-1.0, 1.0), (0.5, 4.0)]              # (length_penalty, eos_boost)
# (V, nb, seeds): every seed is clean (precondition above) for all four PAIRS under the stable sort -- found by running
# `first_gap_violation` over seeds 1 .. 12 on the CPU
CASES = [(23, 3, (1, 2, 3)), (1003, 3, (1, 2, 3)), (23, 5, (4, 5)), (1003, 5, (4, 7))]
B, T0, TMAX, TMIN, EOS, PAD = 4, 3, 12, 6, 2, 1


def toy_case(V, seed, eos_boost):
    """(prompt [B, T0], lm) with lm(ids) = bf16 logits [rows, V]: make_lm's table model, rounded once"""
    lm = make_lm(V, seed, EOS, eos_boost)
    g = torch.Generator().manual_seed(1000 + seed)
    prompt = torch.randint(3, V, (B, T0), generator=g)
    prompt[:, 0] = 0
    return prompt, (lambda ids: lm(ids).bfloat16())


def checked_topk(nb, V, problems):
    """stable_topk that appends to `problems` every violation of the precondition among the first 2*nb + 1 candidates of a live item.
    A finished item is recognised by its padding beams: all nb rows of the item identical (score 0, same tokens)."""
    def fn(cand, k):
        s, i = torch.sort(cand, dim=1, descending=True, stable=True)
        rows = cand.view(cand.shape[0], nb, V)
        for b in range(cand.shape[0]):
            if nb > 1 and bool((rows[b] == rows[b, :1]).all()):
                continue
            for r in range(2 * nb):
                a, c = float(s[b, r]), float(s[b, r + 1])
                same_beam = int(i[b, r]) // V == int(i[b, r + 1]) // V
                if not ((a == c and same_beam) or a - c >= GAP):
                    problems.append((b, r, a, c, int(i[b, r]), int(i[b, r + 1])))
        return s[:, :k], i[:, :k]
    return fn


def first_gap_violation(V, nb, seed, lp, eos_boost):
    from prismer_amd.model.generate import beam_search_from_logits
    prompt, lm = toy_case(V, seed, eos_boost)
    problems = []
    beam_search_from_logits(lm, prompt, nb, TMAX, TMIN, EOS, PAD, lp, topk_fn=checked_topk(nb, V, problems))
    return problems[0] if problems else None


__all__ = ['stable_topk', 'toy_case', 'checked_topk', 'first_gap_violation', 'CASES', 'PAIRS', 'GAP']
