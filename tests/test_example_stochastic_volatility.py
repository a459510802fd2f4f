"""examples/stochastic_volatility.py (the model from its terms, muse() with the covariance, and the closure restatement on the
engine's streams), run as a user would run it: the script itself asserts that the scores of one map agree to its stated rtol.

Measured on an MI355X: from zero both solvers end on the unchanged-value rule at gradient norms of 1e-8 to 1e-7 and their scores
differ by 3.45e-9; after the example's warm restarts (gradient norms below 1e-9, three each) by 3.2e-11.  muse() in the same run: mu -0.4835 +-
0.0190, tau +0.3637 +- 0.0397 (truth -0.5, 0.4: 0.87 and 0.92 sigma)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_example_model_library_is_built(M):
    """(not gpu) The library the example loads: compiled here, cached in-tree, so that the GPU run finds it."""
    lib = M._capi.load_library(M.ElementwiseModel.packaged("stochastic_volatility").library())
    assert lib.muse_model_name(M._capi.MODEL_USER) == b"stochastic_volatility" and lib.muse_model_has_second() == 1


@pytest.mark.gpu
def test_stochastic_volatility_example_runs(gpu):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "stochastic_volatility.py")], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    print(p.stdout)
    assert p.stdout.count("muse_model_exp(") == 1                      # the generated gradient: one exponential
    m = re.search(r"max relative difference of the scores (\S+)", p.stdout)
    assert m and float(m.group(1)) <= 1e-9
    sig = [float(v) for v in re.findall(r"\(truth \S+ (\S+) sigma\)", p.stdout)]
    assert len(sig) == 2 and max(sig) < 4.0
