"""CPU: the longdouble reference of the stencil model with a response as callables (tests/response_reference.py) against
tests/link_reference.py, against itself, and against an fp64 restatement of what the kernels compute; the header family's Python
(ResponseModel, the generator, check_model_consistency), the engine's host evaluation of the two packaged libraries, get_H!'s
handling of a stopped CG, and the packaged libraries' kernel sets and resources.  No GPU anywhere; the libraries are build()'s."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import hp_reference as R
import link_cases as C
import link_reference as L
import response_cases as RC
import response_reference as RR
import stencil_reference as S
from test_gpu_noise_weights import STENCILS, noise_of, theta_of

pytestmark = pytest.mark.skipif(not R.HAVE_LD, reason=R.SKIP_REASON)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

NO_SECOND = '''#define MUSE_MODEL_RESPONSE 1
#include "muse_model.h"
#define MUSE_MODEL_NAME "softsign_first_only"
MUSE_MODEL_FN void muse_model_response(double u, const double* p, double* phi, double* dphi) {
    const double a = sqrt(p[0] * p[0] * (u * u));     /* |p0 u| */
    const double d = 1.0 + a;
    const double g = 1.0 - p[1];                      /* a gain with a pole at p1 = 1: 0 / 0 at u = 0 there */
    *phi = u / (d * g);
    *dphi = 1.0 / ((d * d) * g);
}
'''
BAD_AT_ZERO = '''#define MUSE_MODEL_RESPONSE 1
#include "muse_model.h"
#define MUSE_MODEL_NAME "cusp_at_zero"
MUSE_MODEL_FN void muse_model_response(double u, const double* p, double* phi, double* dphi) {
    (void)p;
    const double a = sqrt(u * u);
    *phi = u / sqrt(a);                                /* sign(u) sqrt|u|: 0 / 0 at u = 0, which the contract forbids */
    *dphi = 0.5 / sqrt(a);
}
'''


def no_second_model(M):
    """A response header that states no phi'' (built by build(), so that no test compiles a library)."""
    return M.ResponseModel.from_source("softsign_first_only", NO_SECOND)


def bad_at_zero_model(M):
    """A response header that is not finite at u = 0: the engine refuses a context of it (built by build())."""
    return M.ResponseModel.from_source("cusp_at_zero", BAD_AT_ZERO)


def _eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ 1. the cubic IS link_reference
@pytest.mark.parametrize("link", [C.LINK, C.HARD_LINK, None])
@pytest.mark.parametrize("w", STENCILS)
def test_cubic_callables_give_link_reference(link, w):
    N, nth = 301, 2
    theta = np.array([-0.3, 0.2]) if link == C.HARD_LINK else theta_of(nth)
    wr = S.BUILTIN if w is None else w
    sd, mask, _ = noise_of(N, nth)
    om, s = RR.weights(N, sd, mask)
    resp = RR.cubic(link)
    a, b = RR.sample_x_z(N, 5, 1, theta, wr, s, resp), L.sample_x_z(N, 5, 1, theta, wr, s, link)
    assert all(_eq(u, v) for u, v in zip(a, b))
    x = a[0].astype(np.float64)
    zz = (0.7 * a[1] + 0.1).astype(np.float64)
    for u, v in zip(RR.objective(x, zz, theta, wr, om, resp), L.objective(x, zz, theta, wr, om, link)):
        assert _eq(u, v)
    assert _eq(RR.curvature(x, zz, wr, om, resp), L.curvature(x, zz, wr, om, link))
    assert _eq(RR.hessian(x, zz, theta, wr, om, resp), L.hessian(x, zz, theta, wr, om, link))
    assert RR.hessian_floor(x, zz, theta, wr, om, resp) == L.hessian_floor(x, zz, theta, wr, om, link)
    for dense in (True, False):
        assert _eq(RR.exact_map(x, theta, wr, om, resp, dense=dense), L.exact_map(x, theta, wr, om, link, dense=dense))
    for u, v in zip(RR.score_at_exact_map(x, theta, wr, om, resp), L.score_at_exact_map(x, theta, wr, om, link)):
        assert _eq(u, v)
    assert _eq(RR.rounding(np.arange(4.0), resp), L.rounding(np.arange(4.0)))


# ------------------------------------------------------------------------------------------------ 2. the saturating cases' own conditions
@pytest.mark.parametrize("w", STENCILS)
@pytest.mark.parametrize("N,nth", [(301, 1), (7001, 4), (70001, 4), (1500, 12)])
def test_saturating_cases_satisfy_their_conditions(N, nth, w):
    theta = theta_of(nth)
    wr = S.BUILTIN if w is None else w
    resp = RR.saturating(RC.P0)
    sd, mask, _ = noise_of(N, nth)
    om, s = RR.weights(N, sd, mask)
    lo = 1.0
    sims = (3, 4) if N < 70001 else (3,)
    for sim in sims:
        x, z, _ = RR.sample_x_z(N, 42, sim, theta, wr, s, resp)
        lo = min(lo, float(resp.dphi(S.stencil(z, wr)).min()))
    print("phi' over the draws: min", lo)
    assert lo <= 0.7
    x = RR.sample_x_z(N, 42, 3, theta, wr, s, resp)[0].astype(np.float64)
    zs = RR.exact_map(x, theta, wr, om, resp)
    lam = RR.hessian_floor(x, zs, theta, wr, om, resp)
    assert lam > 0, lam
    dz = 2 * RC.ATOL / lam
    sg = np.where(zs >= 0, 1.0, -1.0)
    for away in (zs + dz * sg, zs - dz * sg):
        assert RR.hessian_floor(x, away, theta, wr, om, resp) > 0
    print("hessian floor", lam, "of", float(np.exp(-theta.max())))
    # the fp64 restatement stays inside the stated bounds
    fns = RR.numpy_response("saturating_response", RC.SAT)
    zz = (0.7 * RR.sample_x_z(N, 42, 3, theta, wr, s, resp)[1] + 0.1).astype(np.float64)
    f, g = RR.numpy_objective(x, zz, theta, wr, om, fns)
    fh, gh, cf, cg = RR.objective(x, zz, theta, wr, om, resp)
    rf = abs(f - float(fh)) / float(RR.rounding(cf, resp))
    rg = float((np.abs(g - gh).astype(np.float64) / RR.rounding(cg, resp)).max())
    print("fp64 restatement: error / bound: f", rf, "g", rg)
    assert rf <= 1.0 and rg <= 1.0


def test_theta_zero_case_is_harder_than_its_noise_twin_for_the_host_solver(M):
    import torch
    from museinference_jl_amd import optim
    case = RC.HARD
    N, theta = case["N"], case["theta"]
    x, sd, mask, om, s, wr = RC.hard_data(case)

    def fg_of(p, total):
        fns = RR.numpy_response("saturating_response", p)

        def fg(zt):
            f, g = RR.numpy_objective(x, zt.numpy(), theta, wr, om, fns, total)
            return f, torch.from_numpy(g)
        return fg
    zo, io = optim.lbfgs(fg_of(case["p"], C.ORDERS["exact"]), torch.zeros(N, dtype=torch.float64), RC.ATOL)
    _, iq = optim.lbfgs(fg_of((0.0, 0.0), C.ORDERS["exact"]), torch.zeros(N, dtype=torch.float64), RC.ATOL)
    print("host lbfgs: saturating", io["iterations"], io["f_calls"], "noise twin", iq["iterations"], iq["f_calls"])
    assert io["status"] == 0 and iq["status"] == 0 and io["f_calls"] >= iq["f_calls"] + 5
    # ... and the solve's path does not depend on the order of the objective's sum, nor on a few ulps of f (the kernels' order -- a
    # thread's fma chain, then a tree -- is none of the listed ones)
    fgs = {name: fg_of(case["p"], total) for name, total in C.ORDERS.items()}
    for j in range(C.JITTERS):
        fgs["jitter%d" % j] = C._jittered(fgs["exact"], j)
    for name, fg in fgs.items():
        _, i2 = optim.lbfgs(fg, torch.zeros(N, dtype=torch.float64), RC.ATOL)
        assert (i2["status"], i2["iterations"], i2["f_calls"]) == (0, io["iterations"], io["f_calls"]), (name, i2)
    ev = np.linalg.eigvalsh(RR.hessian(x, zo.numpy(), theta, wr, om, RR.saturating(case["p"][0])).astype(np.float64)).min()
    assert ev > 0.5


# ------------------------------------------------------------------------------------------------ 3. the rounding constant
def test_rounding_constant_of_the_saturating_header_is_its_operation_count():
    u = 3                           # fma(w1, zl + zr, w0 z0)
    s = u + 1                       # p0 u
    q = 2 * s + 1                   # fma(s, s, 1): relative 2 * 4 U s^2 / q + U
    rt = (q + 1) // 2 + 1           # sqrt: half the operand's, and its own
    phi = u + rt + 1                # u / sqrt(q)
    r = phi + 1
    qw = r + 1
    assert qw + r + 1 == 24         # the objective's term
    slope = q + rt + 1 + 1          # 1 / (q sqrt(q))
    rho = qw + slope + 1
    grad = rho + 3 + 1 + 1
    assert (phi, slope, rho, grad) == (10, 17, 30, 35)
    assert RR.C_SAT == grad + 5 and RR.saturating(1.0).c_round == RR.C_SAT and RR.cubic(C.LINK).c_round == L.C_LINK


# ------------------------------------------------------------------------------------------------ 4. / 5. the implicit H
@pytest.mark.parametrize("name,p", [("poly_response", C.LINK), ("saturating_response", RC.SAT)])
@pytest.mark.parametrize("N,nth", [(301, 1), (1500, 3)])
def test_fp64_conjugate_gradients_meet_the_implicit_H_bound(N, nth, name, p):
    theta = theta_of(nth)
    wr = S.BUILTIN
    resp = RR.cubic(p) if name == "poly_response" else RR.saturating(p[0])
    fns = RR.numpy_response(name, p)
    sd, mask, _ = noise_of(N, nth)
    om, s = RR.weights(N, sd, mask)
    x, zt, _ = RR.sample_x_z(N, 9, 3, theta, wr, s, resp)
    x, zt = x.astype(np.float64), zt.astype(np.float64)
    k, iv = R.blocks(N, nth), np.exp(-theta)
    for reltol in (RC.CG_RELTOL, 1e-12):
        Href, bound, lam = RR.implicit_H_bound(N, 9, 3, theta, wr, om, s, resp, RC.ATOL_H, reltol)
        zh = RR.exact_map(x, theta, wr, om, resp).astype(np.float64)
        H = np.zeros((nth, nth))
        for j in range(nth):
            v, it = RR.numpy_cg(x, zh, zt, theta, wr, om, fns, j, reltol=reltol, maxiter=400)
            assert it > 0
            for i in range(nth):
                H[i, j] = -np.sum((iv[i] * zh * v)[k == i])
        ratio = float((np.abs(H - Href).astype(np.float64) / bound).max())
        print(name, N, "reltol", reltol, "fp64 CG: largest error / bound", ratio, "lambda", lam)
        assert ratio <= 0.5                                 # with room


def test_fp64_conjugate_gradients_flag_an_indefinite_matrix():
    N, nth = 301, 1
    theta = theta_of(nth)
    wr = S.BUILTIN
    resp = RR.saturating(RC.P0)
    fns = RR.numpy_response("saturating_response", RC.SAT)
    sd, mask, _ = noise_of(N, nth)
    om, s = RR.weights(N, sd, mask)
    x, zt, _ = RR.sample_x_z(N, 9, 3, theta, wr, s, resp)
    x, zt = x.astype(np.float64), zt.astype(np.float64)
    zh = RR.exact_map(x, theta, wr, om, resp).astype(np.float64)
    _, ok = RR.numpy_cg(x, zh, zt, theta, wr, om, fns, 0)
    assert ok > 0
    _, it = RR.numpy_cg(x, zh, zt, theta, wr, om, fns, 0, d=np.full(N, -1e4))      # A' diag(d) A + e^-theta: indefinite at once
    assert it == -1
    d = np.zeros(N)
    d[::7] = -4e2                                                                   # ... and one CG meets only later
    _, it2 = RR.numpy_cg(x, zh, zt, theta, wr, om, fns, 0, d=d)
    assert it2 < 0 and -1 - it2 >= 0
    _, bad = RR.numpy_cg(x, zh, zt, theta, wr, om, fns, 0, d=np.full(N, np.nan))
    assert bad == -1


# ------------------------------------------------------------------------------------------------ 6. get_H! and a stopped CG
class _Stub:
    """A problem whose implicit_H_batch seam reports a stopped column on simulation 1."""
    def __init__(self, counts):
        self.counts = counts

    def standardize_theta(self, t):
        return np.atleast_1d(np.asarray(t, float))

    def implicit_H_batch(self, rng, sim_begin, sim_end, theta0, *, atol=1e-1, cg_maxiter=100):
        n, nt = sim_end - sim_begin, np.size(theta0)
        return np.stack([np.eye(nt) * (1 + e) for e in range(n)]), np.array(self.counts[:n], dtype=np.int32).reshape(n, nt)

    def hess_logPrior_theta(self, theta, space=None):
        return np.zeros((np.size(theta), np.size(theta)))


def test_get_H_raises_on_a_negative_count_and_skips_with_skip_errors(M):
    theta = np.array([0.1, 0.2])
    prob = _Stub([[7, 9], [5, -4], [8, 8]])
    res = M.MuseResult()
    res.theta = theta.copy()
    with pytest.raises(M.MuseError) as e:
        M.get_H_(res, prob, theta, rng=1, nsims=3, implicit_diff=True)
    assert "simulation 1" in str(e.value) and "grad_z_logLike_atol" in str(e.value) and "finite-difference" in str(e.value)
    assert len(res.Hs) == 0
    res = M.MuseResult()
    res.theta = theta.copy()
    with warnings.catch_warnings(record=True) as wlist:
        warnings.simplefilter("always")
        M.get_H_(res, prob, theta, rng=1, nsims=3, implicit_diff=True, skip_errors=True)
    assert any("simulation 1 skipped" in str(w.message) for w in wlist)
    assert len(res.Hs) == 2 and np.array_equal(res.Hs[0], np.eye(2)) and np.array_equal(res.Hs[1], 3 * np.eye(2))
    assert np.array_equal(np.asarray(res.metadata["implicit_diff_cg_hists"]), [[7, 9], [8, 8]])
    ok = M.MuseResult()
    ok.theta = theta.copy()
    M.get_H_(ok, _Stub([[7, 9], [5, 4], [8, 8]]), theta, rng=1, nsims=3, implicit_diff=True)
    assert len(ok.Hs) == 3


# ------------------------------------------------------------------------------------------------ 7. headers
def _cc(path, *flags):
    return subprocess.run(["cc", "-std=c99", "-fsyntax-only", "-Wall", "-Werror", "-I", INCLUDE, "-x", "c", *flags, path], capture_output=True, text=True)


def test_generated_header_compiles_and_refusals_write_nothing(M, tmp_path):
    from museinference_jl_amd.symbolic import response_header_from_expression
    good = tmp_path / "good"
    m = M.ResponseModel.from_expression("softclip", phi="u/sqrt(1 + (p0*u)**2)", directory=str(good))
    assert m.response and not m.pair
    r = _cc(m.header)
    assert r.returncode == 0, r.stderr
    text = open(m.header).read()
    assert "pow(" not in text and "exp(" not in text and "#define MUSE_MODEL_RESPONSE_SECOND 1" in text
    bad = tmp_path / "bad"
    bad.mkdir()
    src = response_header_from_expression("softclip", "u/sqrt(1 + (p0*u)**2)")
    for macro in ("MUSE_MODEL_PAIR", "MUSE_MODEL_NCONST"):
        both = f"#define {macro} 1\n" + src
        with pytest.raises(ValueError) as e:
            M.ResponseModel.from_source("both", both, directory=str(bad))
        assert macro in str(e.value)
        f = tmp_path / (macro + ".h")                      # ... and the header itself says so, with the reason
        f.write_text(both)
        r = _cc(str(f))
        assert r.returncode != 0 and "MUSE_MODEL_RESPONSE cannot be combined with " + macro in r.stderr
    with pytest.raises(ValueError):
        M.ResponseModel.from_source("plain", '#include "muse_model.h"\n', directory=str(bad))
    with pytest.raises(ValueError):
        M.ResponseModel.from_source("consts", src, directory=str(bad), runtime_constants=["P"])
    for phi in ("exp(u)", "u**p0", "1/u", "u*k"):
        with pytest.raises(ValueError):
            M.ResponseModel.from_expression("refused", phi=phi, directory=str(bad))
    assert os.listdir(str(bad)) == []


def _ulps(a, b):
    return abs(a - b) / np.spacing(max(abs(a), abs(b), np.finfo(float).tiny))


@pytest.mark.parametrize("name,p", [("poly_response", C.LINK), ("poly_response", C.HARD_LINK), ("saturating_response", RC.SAT),
                                    ("saturating_response", (RC.P0_HARD, 0.0))])
def test_packaged_libraries_evaluate_the_callables(M, name, p):
    model = M.ResponseModel.packaged(name)
    lib = M._capi.load_library(model.library())
    assert lib.muse_model_name(M._capi.MODEL_USER) == name.encode() and lib.muse_model_has_second() == 1
    resp = RR.cubic(p) if name == "poly_response" else RR.saturating(p[0])
    # 4 ulp OF THE VALUE at every probe -- except where the cubic's terms cancel: phi, phi' or phi'' is there a difference of terms
    # of opposite sign (u < 0 with a2, a3 > 0), and an fp64 evaluation of ANY expression for it errs by ulps of the terms, not of
    # their much smaller sum.  A probe counts as cancelling when the value is below a quarter of the terms' absolute sum (the
    # reference's condition number: |u| dpa, dpa, ddpa); only there the 4 ulp are measured against that sum.  For LINK no probe of
    # phi or phi' cancels; which ones do is listed in the printed line and asserted to be few and on the negative axis.
    worst, cancelling = 0.0, []
    for u in np.concatenate([np.linspace(-3.0, 3.0, 41), [0.0, 1e-300, -1e-8, 37.5]]):
        got = model.eval(u, p)
        want = [float(f(R.LD(np.float64(u)))) for f in (resp.phi, resp.dphi, resp.ddphi)]
        t = R.LD(abs(u))
        terms = [float(t * resp.dpa(t)), float(resp.dpa(t)), float(resp.ddpa(t))]
        for what, g, v, sc in zip(("phi", "phi'", "phi''"), got, want, terms):
            if name == "poly_response" and abs(v) < 0.25 * sc:
                cancelling.append((what, round(float(u), 3)))
                assert u < 0
            else:
                sc = abs(v)
            worst = max(worst, abs(g - v) / np.spacing(max(sc, np.finfo(float).tiny)))
    print(name, p, "largest error in ulp", worst, "cancelling probes (ulp of the terms' sum there):", cancelling)
    assert worst <= 4.0
    assert len(cancelling) <= 0.1 * 3 * 45 and (p != C.LINK or all(what == "phi''" for what, _ in cancelling))   # (a tenth of the 135 values at most)
    out = M.check_model_consistency(model, link=p)
    print("check_model_consistency", out)
    assert out["response"] <= 2e-5
    # p = 0: the identity, exactly
    for u in (-2.5, 0.0, 0.3):
        assert model.eval(u, (0.0, 0.0))[:2] == (u, 1.0) and model.eval(u, (0.0, 0.0))[2] == 0.0


def test_a_header_without_second_derivatives(M):
    model = no_second_model(M)
    assert not model.has_second
    lib = M._capi.load_library(model.library())
    assert lib.muse_model_name(M._capi.MODEL_USER) == b"softsign_first_only"
    assert lib.muse_model_has_second() == 0          # (the refusal of the implicit entries: tests/test_gpu_response.py)
    phi, dphi, d2 = model.eval(0.5, (2.0, 0.0))
    assert phi == 0.25 and dphi == 0.25 and np.isnan(d2)
    assert M.check_model_consistency(model, link=(2.0, 0.0), n_probe=5)["response"] <= 2e-5   # (probes avoid the kink at u = 0)


def test_a_header_that_is_not_finite_at_zero_is_refused_when_a_context_is_created(M):
    import ctypes
    model = bad_at_zero_model(M)
    lib = M._capi.load_library(model.library())
    assert lib.muse_model_name(M._capi.MODEL_USER) == b"cusp_at_zero"
    assert np.isnan(model.eval(0.0)[0]) and model.eval(4.0)[0] == 2.0
    ctx = ctypes.c_void_p()
    rc = lib.muse_ctx_create(M._capi.MODEL_USER, 64, 2, 0, ctypes.byref(ctx))        # (refused before any device is looked for)
    assert rc != 0 and not ctx.value
    msg = lib.muse_last_error().decode()
    assert "cusp_at_zero" in msg and "must be finite at u = 0" in msg


# ------------------------------------------------------------------------------------------------ 8. kernel sets and resources
def test_packaged_libraries_hold_the_expected_kernels_within_their_resources(M):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import regs
    twin = {r[0].replace("15SmoothLinkModel", "17UserResponseModel"): r for r in regs.library_report(M._capi.library_path()) if "SmoothLinkModel" in r[0]}
    assert len(twin) == 16
    for name in ("poly_response", "saturating_response"):
        path = M.ResponseModel.packaged(name).library()
        rows = regs.library_report(path)
        maps = [r for r in rows if r[0].endswith("Lb0EE")]
        imps = [r for r in rows if r[0].endswith("Lb1EE")]
        # S256, S512, C256 with s in LDS and without, in the tiers of 2, 4, 8 and 64 components; S512 and C256 for the implicit branch
        assert len(rows) == 24 and len(maps) == 16 and len(imps) == 8, [r[0] for r in rows]
        assert all("UserResponseModel" in r[0] and "PlaceStreaming" in r[0] for r in rows)
        for short, vgpr, vspill, sspill, scratch, dyn in sorted(rows):
            print(f"{name:20s} {short:78s} vgpr {vgpr:3d} vspill {vspill:3d} sspill {sspill:3d} scratch {scratch:4d}")
            assert not dyn and scratch <= regs.LIBRARY_SCRATCH_LIMIT and vgpr <= 256, short
        assert regs.check_library(path) == []
        if name == "poly_response":
            for r in maps:
                assert r[2] <= twin[r[0]][2], (r, twin[r[0]])
        kernels = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "code_hash.py"), path], capture_output=True, text=True, check=True).stdout.split("\n")
        others = sorted(k.split()[0] for k in kernels if k.strip() and "map_score" not in k)
        assert len(others) == 6 and sum("loglike_kernel" in k for k in others) == 2 and sum("smooth_finish_link_kernel" in k for k in others) == 1, others
