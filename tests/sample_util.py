"""Shared by tests/test_sample_cpu.py and tests/test_sample_gpu.py: the logit rows and (temperature, top_k, top_p) settings of the sampling
tests, and a float64 numpy model of one row -- classes of equal logit, their masses, the kept set under the rule of
prismer_amd/model/generate.py::sample_filter and the cumulative mass of the kept tokens in the defined draw order (class descending,
token id ascending).  The numpy model is written independently of the tensor code it checks."""
import numpy as np
import torch

from tests.util import philox4x32

SETTINGS = [(1.0, 0, 0.9), (0.7, 50, 1.0), (1.3, 50, 0.9), (1.0, 0, 0.5), (1.0, 1, 1.0)]           # (temperature, top_k, top_p)
V_BIG, V_SMALL = 50265, 1003
# the V = 1003 row: chosen (among seeds 1 .. 12 of randn * 4) so that no class boundary lies within MARGIN of top_p at any of SETTINGS;
# test_sample_gpu.py asserts it
SMALL_SEED, SMALL_SCALE = 8, 4.0
MARGIN = 1e-3


def bf16_rows(seed, scale, R, V):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(R, V, generator=g) * scale).bfloat16()


def uniforms_mirror(rows, cur, seed):
    """fp32 [rows]: u = (w >> 8) * 2^-24, w = word 0 of philox4x32(counter = (row, cur, 0, 0x5a3b1e), key = seed) -- tests/util.py's mirror"""
    w = philox4x32(np.arange(rows, dtype=np.uint32), cur, 0, 0x5a3b1e, seed & 0xFFFFFFFF, seed >> 32)[0]
    return torch.from_numpy(((w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)))


class RowModel:
    """one row under one setting, in float64.  x: fp32 numpy [V] (bf16 values).  Attributes: cand (bool [V]), vals / cnt / mass (classes
    that survive top-k, highest first; mass normalised over them), above (mass of the strictly higher classes), n_keep_classes, keep
    (bool [V]), order (kept tokens in draw order), C (their cumulative UNNORMALISED mass, relative to the top class), Z = C[-1]"""

    def __init__(self, x, T, k, p, banned=None):
        x = np.asarray(x, dtype=np.float64)
        self.x = x
        cand = np.isfinite(x)
        if banned is not None:
            cand[banned] = False
        self.cand = cand
        z = x / T
        zc = np.where(cand, z, -np.inf)
        if k > 0 and cand.sum() > k:
            kth = np.sort(zc)[::-1][k - 1]
            elig = cand & (zc >= kth)
        else:
            elig = cand
        self.elig = elig
        vals, cnt = np.unique(x[elig], return_counts=True)
        self.vals, self.cnt = vals[::-1], cnt[::-1]
        w = self.cnt * np.exp(self.vals / T - self.vals[0] / T) if len(vals) else np.zeros(0)
        self.w = w
        self.mass = w / w.sum() if len(vals) else w
        self.above = np.concatenate([[0.0], np.cumsum(self.mass)[:-1]]) if len(vals) else w
        self.T, self.p = T, p
        self.set_classes(int((self.above < p).sum()) if p < 1 else len(self.vals))

    def set_classes(self, n):
        """keep the n highest classes"""
        self.n_keep_classes = n
        self.keep = self.elig & (self.x >= self.vals[n - 1]) if n else np.zeros_like(self.elig)
        tok = np.nonzero(self.keep)[0]
        self.order = tok[np.lexsort((tok, -self.x[tok]))]
        e = np.exp(self.x[self.order] / self.T - (self.vals[0] / self.T if n else 0.0))
        self.C = np.cumsum(e)
        self.Z = self.C[-1] if n else 0.0

    def margin(self):
        """distance of top_p from the nearest class boundary (mass above a class), over all classes"""
        return float(np.abs(self.above - self.p).min()) if self.p < 1 else 1.0

    def draw(self, u):
        """the token of the first cumulative mass above u * Z"""
        i = int(np.searchsorted(self.C, np.float64(u) * self.Z, side='right'))
        return int(self.order[min(i, len(self.order) - 1)])

    def interval_ok(self, tok, u, eps):
        """tok is kept and C(before tok) - eps * Z <= u * Z <= C(tok) + eps * Z"""
        pos = np.nonzero(self.order == tok)[0]
        if len(pos) == 0:
            return False
        i = int(pos[0])
        lo = self.C[i - 1] if i else 0.0
        t = np.float64(u) * self.Z
        return lo - eps * self.Z <= t <= self.C[i] + eps * self.Z

    def logprob(self, tok):
        """log_softmax of the raw row (every finite or -inf column, temperature 1) at tok"""
        m = self.x.max()
        return float(self.x[tok] - m - np.log(np.exp(self.x - m).sum()))
