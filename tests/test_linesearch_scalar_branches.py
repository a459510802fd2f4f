"""The HagerZhang state machine of the headline kernel branches on the scalar unit (the inline-asm rule).

An inline-asm statement whose output is constrained to a VGPR makes that value -- and every condition computed from it --
divergent for the compiler: Solver::wolfe once laundered its three constants that way, and the line search's `state`, its
continuation, the iteration counters and the loop's exit then lived in VGPRs behind s_and_saveexec_b64 / s_cbranch_execz,
with the phi-copies of all the machine's points at every merge.  That build of the headline instantiation's map kernel held
98 s_and_saveexec_b64; with the constants laundered through SGPRs it holds 25, each of them a lane-dependent condition
(thread 0, lane 0 of a wave, the validity mask of an element loop, the poll of a flag).  The bound is half the old count.

Compiles the instantiation alone to assembly (hipcc cross-compiles without a GPU), as tools/inspect_one.sh does."""
import importlib.util
import os
import shutil
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = "FunnelModel<1>, PlaceResident<512, 10, true>"

pytestmark = pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc not available")


def _regs():
    spec = importlib.util.spec_from_file_location("regs", os.path.join(ROOT, "tools", "regs.py"))
    regs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(regs)
    return regs


def test_headline_map_kernel_masks_lanes_only_where_lanes_differ():
    regs = _regs()
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "headline.s")
        regs.compile_one(HEADLINE, out)
        n = regs.exec_masks(out, "map_score")
        (short, vgpr, vspill, sspill, scratch), = regs.report(out)
    print(f"{HEADLINE}: {n} s_and_saveexec_b64, vgpr {vgpr} vspill {vspill} sspill {sspill} scratch {scratch}")
    assert n < 49, n
    assert vspill == 0 and scratch == 0, (vspill, scratch)


def test_register_budget_of_the_hot_kernels_holds():
    assert _regs().check() == []
