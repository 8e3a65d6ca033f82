"""Every case of tests/window_forms.py -- the row window (phase B of csrc/sdp_colfull_kernel.h) on units of 63 to 683
rows: 8, 4, 2 and 1 chunks of the control lattice, idle waves, a second trip of the item loop, a ragged last group,
chunks that are empty, boxes no multiple of SDP_COL_UNROLL_U, a window narrower than the controls need, both table
builds, both real types -- at every geometry of the case, on every input of the table, through the checks of
tests/test_gpu_percontrol_forms.py: three chained sweeps against the direct kernel on all nodes, the first and the third
against the numpy oracle on the sample (the rows around every unit boundary, the whole last column), policy evaluation
and the relative form on the random input.  Bit for bit; on the 'flat' input most controls of a node -- hence its chunks --
tie exactly, and the lowest index must win the merge.

The trailing axes are sized from the compute units of the chip the test runs on, and groups, chunks and trips of the
units the launch code then cuts are asserted from the restated split rule: where the claimed shape is not reached the
test fails, nothing skips."""
import pytest

import window_forms as wf
from test_gpu_percontrol_forms import cus, run_case, _ids   # noqa: F401  (cus: the fixture)

pytestmark = pytest.mark.gpu


def _bounds(col, plan, cus, case, geometry):
    assert plan['unit'].form == 'row window' and plan['col_seg_nodes'] == case.seg_nodes, plan['unit']
    bounds = wf.sweep_bounds(col, cus, case.seg_nodes)
    shapes = {hi - lo: wf.phase_b(hi - lo) for lo, hi in bounds}
    assert shapes == case.units[geometry], (
        '{} at {} on {} compute units: units of {{rows: (groups, chunks, second trip)}} {}, claimed {}'.format(
            case, geometry, cus, shapes, case.units[geometry]))
    return bounds


@pytest.mark.timeout(120)
@pytest.mark.parametrize('case,geometry,vname', wf.RUNS, ids=_ids(wf.RUNS))
def test_window_form_against_the_direct_kernel_and_the_oracle(gpu, cus, case, geometry, vname):
    run_case(case, geometry, vname, cus, lambda col, plan, cus: _bounds(col, plan, cus, case, geometry), 'row_window')
