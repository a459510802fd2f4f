"""Register budget of the kernels behind MUSE_IMPLICIT_PL_JACOBI (csrc/kernels.hpp: JacobiPlace; csrc/solver.hpp: jacobi_cg), in the
manner of tests/test_kernel_resources.py: no scratch beyond the product's bound, no spilled vector register beyond the twin's -- the
implicit kernel of the same model and placement without the preconditioned loop.  No GPU: hipcc cross-compiles."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _regs():
    spec = importlib.util.spec_from_file_location("regs", os.path.join(ROOT, "tools", "regs.py"))
    regs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(regs)
    return regs


def _twins(rows):
    """{jacobi row: twin row} of a library report: ...JacobiPlaceI<placement>E...ELb1EE against ...<placement>...ELb1EE."""
    by_name = {r[0]: r for r in rows}
    out = {}
    for name, r in by_name.items():
        if "11JacobiPlaceI" in name:
            twin = name.replace("NS_11JacobiPlaceINS_14PlaceStreaming", "NS_14PlaceStreaming").replace("EEEEELb1EE", "EEELb1EE")
            assert twin in by_name, (name, twin)
            out[name] = (r, by_name[twin])
    return out


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="llvm-readelf not available")
def test_built_libraries_hold_the_preconditioned_kernels_within_their_twins_budget():
    """The product library (funnel at 1, 2, 4, 8 components and in the big tier, noise: two placements each) and the libraries of
    models/cubic.h and models/offset_noise.h (three tiers, two placements): every preconditioned kernel at most 256 B of scratch per
    lane, no call, and no more spilled vector registers than its twin (measured: 0 and 0; 203-236 VGPRs)."""
    import museinference_jl_amd as M
    regs = _regs()
    libs = {"main": (M.build.build_extension(), 12)}
    for name in ("cubic", "offset_noise"):
        libs[name] = (M.ElementwiseModel.packaged(name).library(), 6)
    for what, (lib, count) in libs.items():
        pairs = _twins(regs.library_report(lib))
        assert len(pairs) == count, (what, sorted(pairs))
        for name, (r, twin) in pairs.items():
            assert not r[5] and r[4] <= regs.LIBRARY_SCRATCH_LIMIT, (what, r)
            assert r[2] <= twin[2], (what, r, twin)           # vgpr_spill_count
            print(f"{what:12s} {name:90s} vgpr {r[1]:3d} (twin {twin[1]:3d}) vspill {r[2]} sspill {r[3]:3d} (twin {twin[3]:3d}) scratch {r[4]}")


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc not available")
@pytest.mark.parametrize("inst", ["FunnelModel<4>, JacobiPlace<PlaceStreaming<512, false, 4>>, true",
                                  "NoiseModel, JacobiPlace<PlaceStreaming<256, true, 4>>, true"])
def test_a_single_instantiation_spills_nothing(inst, tmp_path):
    regs = _regs()
    out = str(tmp_path / "one.s")
    regs.compile_one(inst, out)
    (short, vgpr, vspill, sspill, scratch), = regs.report(out)
    print(f"{inst}: vgpr {vgpr} vspill {vspill} sspill {sspill} scratch {scratch}")
    assert vspill == 0 and scratch == 0
