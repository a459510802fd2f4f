"""-m gpu: the implicit-differentiation get_H! gives the bits recorded in tests/golden/implicit_bits.npz -- H as raw float64 and the
returned CG iteration counts, array_equal on both -- for every case of tests/golden/make_implicit_bits.py: the elementwise branch
(funnel, noise, the cubic header) with and without the preconditioned loop, the pair family (offset_noise), the stencil branch
(smooth as built, with run-time weights, with noise and a mask) and the response branch (saturating_response at the defaults, at a
loose tolerance and at one iteration), each with one column per workgroup and with all columns in one, in clusters and in the big tier.

The file was recorded before the implicit section of csrc/solver.hpp was folded into shared members (plain_cg, the stencil passes,
the epilogue), so this holds that section to "the same operands in the same order": a moved barrier, a vector left out of a pass's
written list or a changed reduction order shows at N = 1001 (the pad element), N = 65536 (clusters) or 9 components (the big tier)."""
import os

import numpy as np
import pytest

from golden.make_implicit_bits import CASES, PATH, run_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    return np.load(PATH)


def test_every_case_is_recorded(recorded):
    assert sorted(recorded.files) == sorted(k + s for k, _ in CASES for s in ("_H", "_it"))
    assert os.path.getsize(PATH) < 100 * 1024


@pytest.mark.parametrize("key,case", CASES, ids=[k for k, _ in CASES])
def test_implicit_H_gives_the_recorded_bits(gpu, M, recorded, key, case):
    H, its = run_case(M, case)
    want_H, want_it = recorded[key + "_H"], recorded[key + "_it"]
    assert H.dtype == want_H.dtype == np.float64 and H.shape == want_H.shape
    print(key, "CG iterations", its.tolist(), "recorded", want_it.tolist(), "max |H - recorded|", float(np.abs(H - want_H).max()))
    assert np.array_equal(its, want_it)
    assert np.array_equal(H, want_H)
