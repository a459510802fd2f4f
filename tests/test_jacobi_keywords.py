"""No GPU: the keyword Pl = "jacobi" of implicit_diff_cg_kwargs on its way to the flag bit MUSE_IMPLICIT_PL_JACOBI, the value of that
bit in the three places that state it, and the claim the feature rests on -- for a diagonal Hessian, CG preconditioned by the diagonal
ends after ONE iteration whatever the spectrum, where plain CG needs many -- in the longdouble restatement tests/jacobi_reference.py."""
import os
import re

import numpy as np
import pytest

import hp_reference as R
import jacobi_reference as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_ld = pytest.mark.skipif(not R.HAVE_LD, reason=R.SKIP_REASON)


def test_pl_jacobi_becomes_the_flag(M):
    from museinference_jl_amd.muse import _cg_keywords
    from museinference_jl_amd.problem import HipMuseProblem
    assert _cg_keywords({"Pl": "jacobi"}) == {"cg_maxiter": 100, "cg_Pl": "jacobi"}
    assert _cg_keywords({"Pl": "jacobi", "maxiter": 5, "reltol": 1e-4}) == {"cg_maxiter": 5, "cg_reltol": 1e-4, "cg_Pl": "jacobi"}
    # the identity and None behave as they did: the keyword does not reach the problem at all
    assert _cg_keywords({"Pl": np.eye(3)}) == {"cg_maxiter": 100}
    assert _cg_keywords({"Pl": None}) == {"cg_maxiter": 100}
    assert _cg_keywords(None) == {"cg_maxiter": 100}
    # ... and the problem turns it into the bit, beside H1-is-zero
    sq = float(np.sqrt(np.finfo(np.float64).eps))
    assert HipMuseProblem._cg_options(None, 0.0, False, "jacobi") == (sq, 0.0, M._capi.IMPLICIT_PL_JACOBI)
    assert HipMuseProblem._cg_options(None, 0.0, True, "jacobi") == (sq, 0.0, M._capi.IMPLICIT_PL_JACOBI | M._capi.IMPLICIT_H1_IS_ZERO)
    assert HipMuseProblem._cg_options(1e-3, 1e-9, False, None) == (1e-3, 1e-9, 0)
    assert HipMuseProblem._cg_options(None, 0.0, False) == (sq, 0.0, 0)
    with pytest.raises(ValueError, match="cg_Pl"):
        HipMuseProblem._cg_options(None, 0.0, False, "ilu")


def test_any_other_pl_is_refused_with_a_text_that_names_jacobi(M):
    from museinference_jl_amd.muse import _cg_keywords
    for bad in ("ilu", 2 * np.eye(2), np.ones((2, 2)), lambda v: v):
        with pytest.raises(ValueError) as e:
            _cg_keywords({"Pl": bad})
        assert '"jacobi"' in str(e.value) and "not supported" not in str(e.value), str(e.value)
        with pytest.raises(ValueError, match="jacobi"):
            M.get_H_(None, None, implicit_diff=True, implicit_diff_cg_kwargs={"Pl": bad})


def test_the_three_statements_of_the_bit_agree(M):
    """include/muse_hip.h, the ctypes table and the Julia shim: MUSE_IMPLICIT_PL_JACOBI == 2 (and H1-is-zero == 1) in each."""
    header = open(os.path.join(ROOT, "include", "muse_hip.h")).read()
    capi = open(os.path.join(ROOT, "museinference.jl_amd", "_capi.py")).read()
    julia = open(os.path.join(ROOT, "julia", "HipMuseInference.jl")).read()
    for name, value in (("IMPLICIT_PL_JACOBI", 2), ("IMPLICIT_H1_IS_ZERO", 1)):
        h = re.search(r"^#define MUSE_%s (\d+)\s*$" % name, header, flags=re.M)
        p = re.search(r"^%s = (\d+)\b" % name, capi, flags=re.M)
        j = re.search(r"^const MUSE_%s = (\d+)\s*$" % name, julia, flags=re.M)
        assert h and p and j, name
        assert int(h.group(1)) == int(p.group(1)) == int(j.group(1)) == value == getattr(M._capi, name)
    # the shim's two _ex entries pass the flags word it builds from both keywords
    assert julia.count("implicit_flags(H1_is_zero, Pl)") == 3     # its definition and the two ccalls


def spread_diagonal(n=1000, decades=6, seed=0):
    rng = np.random.default_rng(seed)
    d = -(10.0 ** rng.uniform(-decades / 2, decades / 2, n))
    assert np.unique(d).size == n and d.max() / d.min() < 10.0 ** -(decades - 1)
    return d, rng.standard_normal(n)


@needs_ld
def test_one_iteration_with_the_diagonal_many_without():
    """A random negative diagonal with 1000 distinct entries over six decades: PCG takes exactly 1 iteration and lands on b / d; plain
    CG (the same module, Pl off) takes more than 20 -- and with maxiter = 100 has not converged at all."""
    d, b = spread_diagonal()
    x, exact, it = J.solve(d, b, jacobi=True)
    assert it == 1
    assert float(np.max(np.abs(x - exact) / np.abs(exact))) < 1e-17
    xp, _, itp = J.solve(d, b, jacobi=False, maxiter=100)
    assert itp > 20, itp
    # the recurrence with Pl off IS plain CG: on a diagonal with 5 distinct values it ends in 5 iterations
    d5 = -np.repeat([1.0, 2.0, 3.5, 7.0, 11.0], 40)
    x5, e5, it5 = J.solve(d5, b[:200], jacobi=False)
    assert it5 == 5 and float(np.max(np.abs(x5 - e5))) < 1e-12
    # keywords: maxiter = 0 leaves x = 0; an abstol above |b| stops at once; a zero right-hand side takes no iteration
    assert J.solve(d, b, maxiter=0)[2] == 0 and not J.solve(d, b, maxiter=0)[0].any()
    assert J.solve(d, b, abstol=1e9)[2] == 0
    assert J.solve(d, np.zeros_like(b))[2] == 0


@needs_ld
def test_a_zero_on_the_diagonal_is_a_phantom_slot():
    """d_i = 0 (a header that says ozz = 0 on a real element; the pad element): c_i = 0 there, never inf or nan.  With b_i = 0 at
    that slot -- a phantom -- the solve is untouched: one iteration, the exact result, 0 at the slot."""
    d, b = spread_diagonal(n=101, seed=3)
    d[7], b[7] = 0.0, 0.0
    x, exact, it = J.solve(d, b)
    assert it == 1 and np.isfinite(x.astype(np.float64)).all() and x[7] == 0 and exact[7] == 0
    keep = np.arange(101) != 7
    assert float(np.max(np.abs(x[keep] - exact[keep]) / np.abs(exact[keep]))) < 1e-17
    # b_i != 0 there: that component is never updated (c_i = 0), nothing overflows, and the residual cannot fall below |b_i|
    b[7] = 0.5
    x, _, it = J.solve(d, b, maxiter=3)
    assert it == 3 and np.isfinite(x.astype(np.float64)).all() and x[7] == 0
