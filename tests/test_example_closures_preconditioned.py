"""examples/closures_preconditioned.py (get_H! by implicit differentiation for a closure problem with badly scaled latents, with and
without implicit_diff_cg_kwargs' Pl = "jacobi"), run as a user would run it: the script itself asserts that its two H agree to its
stated bound and that the preconditioned counts are the smaller ones."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_closures_preconditioned_example_runs(gpu):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "closures_preconditioned.py")], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    print(p.stdout)
    Hp = float(re.search(r"H with plain\s+CG\s+(\S+)", p.stdout).group(1))
    Hj = float(re.search(r"H with jacobi\s+CG\s+(\S+)", p.stdout).group(1))
    rounds = [int(r) for r in re.findall(r"(\d+) rounds", p.stdout)]
    assert abs(Hp - Hj) <= 1e-6 * abs(Hp) and len(rounds) == 2 and rounds[1] < rounds[0]
