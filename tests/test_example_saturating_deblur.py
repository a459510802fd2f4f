"""examples/saturating_deblur.py (the stencil model behind a response stated in a header, with a noise map and a mask; get_H! by
finite differences and by implicit differentiation), run as a user would run it."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_saturating_deblur_example_runs(gpu):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "saturating_deblur.py")], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert "theta[0]" in p.stdout and "theta[1]" in p.stdout and "host root" in p.stdout and "CG iterations" in p.stdout
    print(p.stdout)
