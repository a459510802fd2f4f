"""muse_lbfgs_normals (include/muse_lbfgs.h: the engine's normal stream for all rows of a map in one launch) without a GPU: the export
in the library, the header and the ctypes table; the refusal of every bad argument before any launch; the kernel's resources; the new
argument of BatchedTorchMuseProblem."""
import inspect
import os
import subprocess
import sys

import numpy as np

from museinference_jl_amd import _capi, simple
from museinference_jl_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_point_is_exported_declared_and_in_the_ctypes_table():
    path = B.build_lbfgs_library()
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert "muse_lbfgs_normals" in exported
    assert "muse_lbfgs_normals" in B.lbfgs_declared_symbols()
    assert "muse_lbfgs_normals" in _capi.LBFGS_SIGNATURES
    for f in (os.path.join(B.LBFGS_DIR, "normals_kernels.hpp"), os.path.join(B.CSRC, "rng.hpp")):
        assert os.path.exists(f) and f in B._LBFGS_DEPS, f


def test_bad_arguments_are_refused_before_any_launch():
    """(a non-null pointer is never followed: these are host addresses)"""
    lib = _capi.load_lbfgs_library()
    buf = np.zeros(64)
    p = buf.ctypes.data
    assert lib.muse_lbfgs_normals(None, 1, 4, 7, p, 0, None) == -1          # out
    assert lib.muse_lbfgs_normals(p, 1, 4, 7, None, 0, None) == -1          # sims
    assert lib.muse_lbfgs_normals(p, 0, 4, 7, p, 0, None) == -1             # nrows < 1
    assert lib.muse_lbfgs_normals(p, -3, 4, 7, p, 0, None) == -1
    assert lib.muse_lbfgs_normals(p, 1, 0, 7, p, 0, None) == -1             # count < 1
    assert lib.muse_lbfgs_normals(p, 1, -1, 7, p, 0, None) == -1
    assert lib.muse_lbfgs_normals(p, 1, 4, 7, p, -1, None) == -1            # pair_offset < 0
    # what the flat grid and the 63-bit counter cannot hold
    assert lib.muse_lbfgs_normals(p, 1 << 31, 1, 7, p, 0, None) == -1
    assert lib.muse_lbfgs_normals(p, 1 << 20, 1 << 23, 7, p, 0, None) == -1
    assert lib.muse_lbfgs_normals(p, 1, 4, 7, p, (1 << 63) - 2, None) == -1


def test_the_normals_kernel_resources():
    """Exactly one normals kernel; its name holds neither substring the L-BFGS and CG resource tests count by; no kernel of the
    library spills, uses scratch or has a dynamic stack."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import regs
    rows = regs.library_report(B.build_lbfgs_library())
    for name, vgpr, vspill, sspill, scratch, dyn in rows:
        assert vspill == 0 and scratch == 0 and not dyn, (name, vgpr, vspill, scratch, dyn)
    normals = [r for r in rows if "normals" in r[0]]
    assert len(normals) == 1, rows
    name, vgpr, vspill, sspill, scratch, dyn = normals[0]
    print(name, "vgpr", vgpr, "vspill", vspill, "sspill", sspill, "scratch", scratch)
    assert "advance_kernel" not in name and "cg_" not in name
    assert vspill == 0 and sspill == 0 and scratch == 0 and not dyn
    assert vgpr <= 128       # 256 threads: four workgroups per compute unit and more


def test_the_problem_accepts_a_batched_sampler():
    sig = inspect.signature(simple.BatchedTorchMuseProblem.__init__)
    assert "sample_x_z_batched" in sig.parameters and sig.parameters["sample_x_z_batched"].default is None
    assert list(sig.parameters)[:8] == ["self", "x", "sample_x_z", "logLike", "logPrior", "device", "dtype", "logLike_batched"]
    import museinference_jl_amd as M
    assert M.EngineNormals is simple.EngineNormals and "EngineNormals" in M.__all__
