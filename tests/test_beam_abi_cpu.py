"""CPU: the ABI of the device beam step (ph_beam_topk, ph_beam_advance, PH_WS_BEAM_TOPK) -- struct layouts, workspace sizing, argument
validation without a device -- and the specification (beam_search_from_logits) under the library's tie rule against the loop oracle."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest
import torch

from oracle.beam_oracle import beam_search_loops
from tests import beam_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_beam_struct_sizes_match_header():
    from prismer_amd import _lib
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "prismer_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %d\n", sizeof(ph_beam_topk_args), sizeof(ph_beam_advance_args), offsetof(ph_beam_topk_args, workspace_bytes),
         offsetof(ph_beam_topk_args, top_tok), offsetof(ph_beam_advance_args, rows_out), offsetof(ph_beam_advance_args, len_div), PH_WS_BEAM_TOPK);
  return 0;
}'''
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, 't.c'); exe = os.path.join(td, 't')
        open(src, 'w').write(prog)
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), src, '-o', exe])
        out = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    T, A = _lib.BeamTopkArgs, _lib.BeamAdvanceArgs
    assert out == [C.sizeof(T), C.sizeof(A), T.workspace_bytes.offset, T.top_tok.offset, A.rows_out.offset, A.len_div.offset, _lib.WS_BEAM_TOPK]
    assert _lib.WS_BEAM_TOPK == 4


def _split(rows, V):
    cdiv = lambda a, b: (a + b - 1) // b
    return max(cdiv(V, 8192), min(16, cdiv(512, rows), cdiv(V, 1024)))


def test_beam_workspace_query():
    from prismer_amd import _lib
    q = lambda *d: _lib.lib.ph_query_workspace(_lib.WS_BEAM_TOPK, (C.c_int64 * len(d))(*d), len(d))
    for B, nb, V in [(1, 1, 23), (4, 3, 23), (4, 3, 1003), (32, 3, 50265), (1, 8, 50265), (32, 8, 50265), (2, 5, 300000)]:
        want = max(B * _split(B, V), B * nb * _split(B * nb, V)) * 34 * 4
        assert q(B, nb, V) == want, (B, nb, V)
    assert q(32, 3, 50265) == max(32 * 16, 96 * 7) * 136                                        # the eval shape: 7 blocks per beam row
    assert q(4, 9, 1003) == -1 and q(4, 0, 1003) == -1                                          # num_beams outside 1..8
    assert q(4, 3, 6) == -1                                                                      # V < 2 * nb + 1
    assert q(0, 3, 1003) == -1 and q(4, 3) == -1 and q(4, 3, 1003, 1) == -1
    assert q(4, 3, 64 * 8192 + 1) == -1
    assert _lib.lib.ph_query_workspace(9, (C.c_int64 * 1)(1), 1) == -1                          # op 9 stays invalid


def test_beam_argument_validation_without_gpu():
    from prismer_amd import _lib
    L = _lib.lib
    err = lambda: L.ph_last_error()

    def topk(**kw):
        a = _lib.BeamTopkArgs(logits=32, ld=1008, V=1003, B=4, nb=3, nb_in=3, beam_scores=16, eos_token_id=2, ban_eos=1, workspace=16,
                              workspace_bytes=1 << 20, top_score=16, top_beam=16, top_tok=16)
        for k, v in kw.items():
            setattr(a, k, v)
        return L.ph_beam_topk(C.byref(a), None)
    assert topk(logits=None) == -1 and b'null pointer' in err()
    assert topk(top_tok=None) == -1 and b'null pointer' in err()
    assert topk(nb=9, nb_in=9) == -1 and b'num_beams 9 outside 1..8' in err()
    assert topk(nb_in=2) == -1 and b'nb_in 2' in err()
    assert topk(V=6, ld=8) == -1 and b'below 2 * num_beams + 1' in err()
    assert topk(ld=1003) == -1 and b'16-byte aligned' in err()
    assert topk(ld=1000) == -1 and b'16-byte aligned' in err()
    assert topk(logits=34) == -1 and b'16-byte aligned' in err()
    assert topk(eos_token_id=1003) == -1 and b'eos_token_id' in err()
    assert topk(workspace_bytes=64) == -1 and b'workspace' in err()
    assert topk(B=0) == -1

    def adv(**kw):
        a = _lib.BeamAdvanceArgs(top_score=16, top_beam=16, top_tok=16, ids_in=16, ids_out=32, beam_scores=16, hyp_score=16, hyp_tok=16,
                                 hyp_len=16, n_hyp=16, done=16, rows_out=16, B=4, nb=3, nb_in=3, Tmax=12, cur=3, eos_token_id=2,
                                 pad_token_id=1, rows_rep=1, len_div=3.0)
        for k, v in kw.items():
            setattr(a, k, v)
        return L.ph_beam_advance(C.byref(a), None)
    assert adv(done=None) == -1 and b'null pointer' in err()
    assert adv(ids_out=16) == -1 and b'different buffers' in err()
    assert adv(nb=9, nb_in=9) == -1 and b'outside 1..8' in err()
    assert adv(nb_in=2) == -1 and b'nb_in' in err()
    assert adv(cur=12) == -1 and b'position 12' in err()
    assert adv(cur=0) == -1 and b'position 0' in err()
    assert adv(rows_rep=0) == -1
    assert adv(len_div=0.0) == -1 and b'len_div' in err()


def test_stable_topk_is_the_flat_index_rule():
    cand = torch.tensor([[1.0, 3.0, 3.0, 0.5, 3.0, 1.0], [2.0, 2.0, 2.0, 2.0, 2.0, 2.0]])
    s, i = U.stable_topk(cand, 4)
    assert i.tolist() == [[1, 2, 4, 0], [0, 1, 2, 3]] and s.tolist() == [[3.0, 3.0, 3.0, 1.0], [2.0, 2.0, 2.0, 2.0]]


@pytest.mark.parametrize('lp,eos_boost', U.PAIRS)
@pytest.mark.parametrize('V,nb,seeds', U.CASES)
def test_specification_under_the_library_tie_rule_matches_loop_oracle(V, nb, seeds, lp, eos_boost):
    """beam_search_from_logits(topk_fn=stable sort) on the chosen toy cases (bf16-rounded logits): the precondition of the device tests
    holds, and the result is the loop oracle's.  The oracle breaks ties its own way, which the precondition makes irrelevant except for
    exact ties inside one row, where both take the lower token first."""
    from prismer_amd.model.generate import beam_search_from_logits
    for seed in seeds:
        prompt, lm = U.toy_case(V, seed, eos_boost)
        problems = []
        got = beam_search_from_logits(lm, prompt, nb, U.TMAX, U.TMIN, U.EOS, U.PAD, lp, topk_fn=U.checked_topk(nb, V, problems))
        assert not problems, f'precondition violated (item, rank, score, next score, flat indices): {problems[:3]}'

        def step_list(rows):
            return torch.log_softmax(lm(torch.tensor(rows)).float(), -1).tolist()
        want = beam_search_loops(step_list, prompt.tolist(), nb, U.TMAX, U.TMIN, U.EOS, U.PAD, lp)
        assert [g.tolist() for g in got] == want, (seed, [g.tolist() for g in got], want)
        plain = beam_search_from_logits(lm, prompt, nb, U.TMAX, U.TMIN, U.EOS, U.PAD, lp)        # default topk_fn: nothing else moved
        assert [g.tolist() for g in plain] == want
