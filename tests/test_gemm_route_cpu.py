"""CPU: the GEMM dispatch as a table.  tests/golden/gemm_routes.json holds, for every distinct ph_gemm_bf16 / ph_gemm_grouped(_capped)_bf16
call of one training step of base_b32, zbase_b32 and large_vqa_b16 and for both sides of every threshold of the dispatch (tools/gemm_routes.py
hand_rows), the route the library takes: kernel class, tile, main-loop variant, blocks / units, k split, fold pass, workspace bytes, tail split.
ph_gemm_route answers without a device; every field must equal the table, so a changed threshold or constant is a diff of that file
(`python tools/gemm_routes.py record` rewrites it; the launches behind the recorded routes: profiles/gemm_route_equivalence.txt)."""
import ctypes as C
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import gemm_routes as R  # noqa: E402

ROWS = json.load(open(R.TABLE))


def test_table_covers_step_and_thresholds():
    assert len(ROWS) == len({R._key(r) for r in ROWS})                                  # de-duplicated
    for case in R.CASES:
        assert sum(case in r.get('cases', ()) for r in ROWS) >= 40, case
    assert [r['note'] for r in ROWS if 'note' in r] == [r['note'] for r in R.hand_rows()]
    assert [R._key(r) for r in ROWS if 'note' in r] == [R._key(r) for r in R.hand_rows()]
    assert os.path.getsize(R.TABLE) < 512 << 10


def test_every_row_routes_as_recorded():
    bad = []
    for i, row in enumerate(ROWS):
        got = R.route_of(row)
        if got != row['expect']:
            bad.append((i, row.get('note') or row.get('cases'), got, row['expect']))
    assert not bad, bad[:5]


def test_persistent_plans_of_the_k_balanced_kernel():
    """(units, max_split) the plan query gave before ph_gemm_route replaced it: 64 MB workspace, fp32 accumulate, [K][M] x [K][N]"""
    from prismer_amd import _lib
    ragged = [(264, 136, 2048), (264, 136, 4160), (264, 136, 8320)]
    for shapes, ws, want in ((ragged, 64 << 20, (40, 6)), ([(512, 128, 8320)], 64 << 20, (12, 6)), ([(768, 384, 8320)] * 16, 64 << 20, (432, 3)),
                             ([(1536, 768, 4096)] * 4, 64 << 20, (144, 1)), (ragged, 0, (12, 1))):
        part = R.route_of(dict(entry='grouped', problems=[R.wgrad(*s, ws=ws) for s in shapes]))['part'][0]
        assert part['cls'] == _lib.GEMM_CLS_BIG_GROUPED and (part['units'], part['max_split']) == want, (shapes[0], part)
        assert part['fold'] == (_lib.GEMM_FOLD_IN_LAUNCH if want[1] > 1 else _lib.GEMM_FOLD_NONE)


def test_tail_split_reports_both_parts():
    from prismer_amd import _lib
    e = R.route_of(dict(entry='single', problems=[R.prob(8320, 3072, 768)]))
    assert e['parts'] == 2 and e['tail_m'] == 8192
    assert [p['cls'] for p in e['part']] == [_lib.GEMM_CLS.index('big'), _lib.GEMM_CLS.index('ks2')]
    assert R.route_of(dict(entry='single', problems=[R.prob(8320, 768, 768)]))['parts'] == 1


def test_big_mode_is_decoded_once():
    """0 off, 1 plain, 2..6 lean, >= 7 spread -- the same for a single launch, a persistent group and a conv group"""
    from prismer_amd import _lib
    single = [R.prob(8320, 768, 768)]
    group = [R.wgrad(1536, 768, 4096, ws=0)] * 4
    conv = [R.conv_nn(16, 16)]
    for mode, want in ((1, 1), (2, 2), (5, 2), (6, 2), (7, 3), (9, 3), (12, 3)):
        t = [mode, 128]
        assert R.route_of(dict(entry='single', problems=single, tuning=t))['part'][0]['variant'] == want, mode
        # the grouped forms have no plain loop: plain runs as lean; the conv gather takes the 256x128 kernel from mode 2 on
        assert R.route_of(dict(entry='grouped', problems=group, tuning=t))['part'][0]['variant'] == max(want, 2), mode
        c = R.route_of(dict(entry='grouped', problems=conv, tuning=t))['part'][0]
        assert (c['cls'], c['variant']) == ((_lib.GEMM_CLS_BIG_GROUPED, want) if mode > 1 else (_lib.GEMM_CLS.index('grouped'), 0)), mode
    for rows in (single, group, conv):
        p = R.route_of(dict(entry='single' if rows is single else 'grouped', problems=rows, tuning=[0, 128]))['part'][0]
        assert p['variant'] == 0 and p['cls'] not in (_lib.GEMM_CLS.index('big'), _lib.GEMM_CLS_BIG_GROUPED)


def test_route_rejects_bad_arguments():
    from prismer_amd import _lib
    info = _lib.GemmRouteInfo()
    arr, _ = R.args_of(dict(entry='grouped', problems=[R.prob(64, 64, 64), R.prob(64, 64, 64, 'TT')]))
    assert _lib.lib.ph_gemm_route(arr, 2, 1, 0, C.byref(info)) == -1 and b'mixed layouts' in _lib.lib.ph_last_error()
    assert _lib.lib.ph_gemm_route(arr, 2, 0, 0, C.byref(info)) == -1                      # ph_gemm_bf16 takes one problem
    arr[0].K = 0
    assert _lib.lib.ph_gemm_route(arr, 1, 1, 0, C.byref(info)) == -1 and b'bad dims' in _lib.lib.ph_last_error()
    assert _lib.lib.ph_gemm_route(arr, 1, 1, 0, None) == -1


def test_struct_layout_matches_header():
    import subprocess
    import tempfile
    from prismer_amd import _lib
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include <stdint.h>
#include "prismer_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %d %d\n", sizeof(ph_gemm_route_part), sizeof(ph_gemm_route_info), offsetof(ph_gemm_route_part, ws_bytes),
         offsetof(ph_gemm_route_info, part), PH_GEMM_CLS_COUNT, PH_GEMM_FOLD_IN_LAUNCH);
  return 0;
}'''
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, 't.c'), os.path.join(td, 't')
        open(src, 'w').write(prog)
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), src, '-o', exe])
        out = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    assert out == [C.sizeof(_lib.GemmRoutePart), C.sizeof(_lib.GemmRouteInfo), _lib.GemmRoutePart.ws_bytes.offset, _lib.GemmRouteInfo.part.offset,
                   len(_lib.GEMM_CLS), _lib.GEMM_FOLD_IN_LAUNCH]


if __name__ == '__main__':
    raise SystemExit(pytest.main([__file__, '-q']))
