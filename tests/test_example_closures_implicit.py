"""examples/closures_implicit.py (get_H! by implicit differentiation for a closure problem, next to the finite-difference get_H!), run as
a user would run it: the script itself asserts that its two H agree to its stated bound."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_closures_implicit_example_runs(gpu):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "closures_implicit.py")], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    print(p.stdout)
    Hi = float(re.search(r"H by implicit differentiation\s+(\S+)", p.stdout).group(1))
    Hf = float(re.search(r"H by finite differences\s+(\S+)", p.stdout).group(1))
    assert abs(Hi - Hf) <= 0.05 * abs(Hf) and "rounds" in p.stdout
