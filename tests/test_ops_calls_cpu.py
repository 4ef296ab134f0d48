"""CPU: prismer_amd/ops.py hands the library the calls tests/golden/ops_calls.json lists -- every ph_gemm_args field, pointers as (tensor, byte
offset), the dropout triple of every structure that has one, the workspace role, the cut of every item list into launches -- for the
scenarios of tools/ops_calls.py.  The table was recorded from the hand-rolled call sites the argument builder (ops.gemm_args) and the group
launcher (ops.launch_grouped) replaced; a deliberate change of the call layer re-records it (`python tools/ops_calls.py record`)."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import ops_calls  # noqa: E402


def test_the_table_holds_every_scenario():
    table = json.load(open(ops_calls.TABLE))
    assert list(table) == [name for name, _ in ops_calls.scenarios()]
    assert table['conv_wgrad_persistent refused'] == {'calls': [], 'returns': [None, None]}
    assert os.path.getsize(ops_calls.TABLE) < 1 << 20


def test_ops_issues_the_recorded_calls():
    diff = ops_calls.check()
    assert not diff, '\n'.join(diff)
