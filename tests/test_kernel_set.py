"""The kernels of the BUILT libmuse_hip.so are exactly the committed list (tests/golden/libmuse_hip_kernels.txt, one mangled name per
line, written from tools/code_hash.py's listing): a dispatch that instantiates a kernel nobody launches -- a generic visitor compiled
for a tier it never takes does that -- or that loses one fails here.  A change that adds or drops a kernel on purpose regenerates the
list:  python tools/code_hash.py museinference.jl_amd/libmuse_hip.so | cut -d' ' -f1 > tests/golden/libmuse_hip_kernels.txt"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"   # (tools/code_hash.py's disassembler)


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="llvm-objdump not available")
def test_library_holds_exactly_the_listed_kernels():
    import museinference_jl_amd as M
    lib = M.build.build_extension() if hasattr(M, "build") else os.path.join(ROOT, "museinference.jl_amd", "libmuse_hip.so")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "code_hash.py"), lib], capture_output=True, text=True, check=True)
    built = sorted(line.split()[0] for line in r.stdout.splitlines() if line.strip())
    listed = sorted(open(os.path.join(ROOT, "tests", "golden", "libmuse_hip_kernels.txt")).read().split())
    assert len(listed) == len(set(listed)) == 195
    assert sorted(set(built) - set(listed)) == [], "kernels the library holds that the list does not"
    assert sorted(set(listed) - set(built)) == [], "kernels of the list that the library lost"
    assert built == listed
