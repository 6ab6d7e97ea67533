"""SharedEngine({ resident: true, tnsMode, pnsMode }) under Node with a stub addon (no GPU): a decoder whose modes equal the engine's
takes the resident route, the pipeline is created with the matching `stages` word, other modes are refused as on the parsing route,
carryWindowShape and int16 PCM still take the parsing route.  The GPU half is in tests/test_resident_stages_gpu.py."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")


@pytest.mark.skipif(NODE is None, reason="node not present on this machine")
def test_spec_modes_take_the_resident_route_with_a_stub_addon():
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "test_resident_stages.js")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "resident stages cpu tests ok" in r.stdout, r.stdout + r.stderr


def test_a_plan_made_for_the_stages_has_one_route(engine_lib):
    """aacg_pick_route through aacg_debug_route (no device): the plan flag set at creation gives aacg_imdct_run_quant_ex_rv serial or
    pipelined, with or without a filter, a noise band, long chains or wide frames in the batch — and nothing else changes its route"""
    import aacgpu
    for extra in (0, aacgpu.ROUTE_PLAN_TNS, aacgpu.ROUTE_PLAN_PNS, aacgpu.ROUTE_PLAN_TNS | aacgpu.ROUTE_PLAN_PNS, aacgpu.ROUTE_PLAN_LONG_CHAINS,
                  aacgpu.ROUTE_PLAN_FULL_LATER_RUNS, aacgpu.ROUTE_PLAN_WIDE_FRAMES):
        for pipelined in (False, True):
            assert aacgpu.debug_route(aacgpu.INPUT_QUANT_I16, aacgpu.OUTPUT_F32, aacgpu.ROUTE_PLAN_STAGES | extra, pipelined) == "aacg_imdct_run_quant_ex_rv"
    # without the flag a batch without optional stages keeps the plain kernels
    assert aacgpu.debug_route(aacgpu.INPUT_QUANT_I16, aacgpu.OUTPUT_F32, 0, True) == "aacg_imdct_run_quant_rv"
    assert aacgpu.debug_route(aacgpu.INPUT_QUANT_I16, aacgpu.OUTPUT_F32, 0, False) == "aacg_imdct_run_quant"
