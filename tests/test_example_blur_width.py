"""examples/blur_width.py (the stencil model with run-time weights), run as a user would run it."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_blur_width_example_runs(gpu):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "blur_width.py")], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert "narrow" in p.stdout and "wide" in p.stdout and "theta" in p.stdout
    print(p.stdout)
