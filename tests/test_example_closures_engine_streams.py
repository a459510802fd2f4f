"""examples/closures_engine_streams.py (the funnel as closures on the engine's streams next to HipMuseProblem(model="funnel") with the
same seed), run as a user would run it: the script itself asserts that the two θ trajectories agree to its stated bound."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_closures_engine_streams_example_runs(gpu):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "closures_engine_streams.py")], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    print(p.stdout)
    m = re.search(r"iterations (\d+) and (\d+); max \|difference of theta\| over the trajectory (\S+)", p.stdout)
    assert m and m.group(1) == m.group(2) and int(m.group(1)) >= 2
    assert float(m.group(3)) <= 1e-6
