"""Exponentials in a user's model terms (include/muse_model.h, EXPONENTIALS): the generator accepts `exp` and prints it as
muse_model_exp; the two shipped models whose per-element functions call it -- models/stochastic_volatility.h (two-parameter family:
z_i ~ N(mu, e^tau), x_i ~ N(0, e^z_i)) and models/lognormal_obs.h (one-parameter family: x_i ~ N(2 (e^(z_i/2) - 1), 1)) -- and their
generated twins on the CPU checker, which compiles the same text with its own restatement of the fixed-sequence exponential; and
the resources of the two model libraries' kernels (tools/regs.py) with the engine's fence for what is beyond the bound.

not gpu: everything here.  The GPU side is tests/test_gpu_model_exp.py, which finds the libraries this file builds."""
import importlib.util
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MODELS = os.path.join(ROOT, "museinference.jl_amd", "models")
SV, LN = os.path.join(MODELS, "stochastic_volatility.h"), os.path.join(MODELS, "lognormal_obs.h")
PROBE = os.path.join(HERE, "models", "exp_probe.h")
PROFILE = os.path.join(ROOT, "profiles", "r18_model_exp_resources.txt")

SV_TERMS = dict(coefs=["a", "exp(b/2)", "exp(-b)", "1"], C="b", o="x**2*exp(-z) + c3*z + c2*(z - c0)**2", z="c0 + c1*n1", x="exp(z/2)*n2")
LN_TERMS = dict(A="(x - 2*(exp(z/2) - 1))**2", B="z**2", z="sd*n1", x="2*(exp(z/2) - 1) + n2")


def generated_sv(M, directory=None):
    return M.ElementwiseModel.from_pair_expressions("sv_gen", directory=directory, **SV_TERMS)


def generated_ln(M, directory=None):
    return M.ElementwiseModel.from_expressions("lognormal_gen", directory=directory, **LN_TERMS)


def _code(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _body(code, fn):
    return code.split(fn + "(")[1].split("\n}")[0]


# ------------------------------------------------------------------------------------------------ the generator
def test_the_generator_accepts_exp_in_the_terms(M, tmp_path):
    """`exp` in A, B, z, x of from_expressions and in o, z, x of from_pair_expressions (a ValueError before): printed as
    muse_model_exp(...), nothing of libm left, ONE exponential per function body -- the gradient, its objective term and the second
    derivatives share it -- and every other function still refused with the message tests/test_symbolic_model.py matches."""
    sv, ln = generated_sv(M, str(tmp_path)), generated_ln(M, str(tmp_path))
    for m, fns in ((sv, ("muse_model_sample", "muse_model_grad", "muse_model_pair_second", "muse_model_pair_dx")),
                   (ln, ("muse_model_sample", "muse_model_grad", "muse_model_second", "muse_model_dx_dsd"))):
        code = _code(open(m.header).read())
        assert "muse_model_exp(" in code
        assert not re.search(r"(?<![A-Za-z0-9_])(exp|pow|expm1|log)\(", code), m.header
        for fn in fns:
            assert _body(code, fn).count("muse_model_exp(") == 1, (m.name, fn)
    assert sv.pair and not ln.pair
    assert _body(_code(open(sv.header).read()), "muse_model_coefs").count("muse_model_exp(") == 2
    f = lambda **kw: M.ElementwiseModel.from_expressions("bad", directory=str(tmp_path / "bad"), **{**LN_TERMS, **kw})
    g = lambda **kw: M.ElementwiseModel.from_pair_expressions("bad", directory=str(tmp_path / "bad"), **{**SV_TERMS, **kw})
    for bad in ("log(1 + z**2)", "sin(z)"):
        with pytest.raises(ValueError, match="not allowed in a model header"):
            f(A=f"(x - {bad})**2", x=f"{bad} + n2")
        with pytest.raises(ValueError, match="not allowed in a model header"):
            g(o=SV_TERMS["o"] + f" + z*{bad}")
    with pytest.raises(ValueError, match="vanish at x = z = 0"):        # the pad-element checks see through the exponential
        f(A="(x - exp(z/2))**2", x="exp(z/2) + n2")
    with pytest.raises(ValueError, match="vanish at x = z = 0 with zero coefficients"):
        g(o="x**2*exp(-z) + z + c2*(z - c0)**2")                         # (the z term without c3: 1/2 at the pad element's gradient)
    assert os.listdir(str(tmp_path / "bad")) == [] if os.path.isdir(str(tmp_path / "bad")) else True
    # a response header takes no exponential (ResponseModel.from_expression is as it was)
    with pytest.raises(ValueError, match="not allowed in a model header"):
        M.ResponseModel.from_expression("bad_response", "2*(exp(u/2) - 1)", directory=str(tmp_path / "bad"))


def test_exponentials_with_commensurate_arguments_share_one_call(M, tmp_path):
    """e^z beside e^(z/2) in one body -- what differentiating (e^(z/2))^2 leaves -- is the square of ONE exponential."""
    m = M.ElementwiseModel.from_expressions("expsq", directory=str(tmp_path), A="(x - (exp(z) - 1) - 2*(exp(z/2) - 1))**2", B="z**2", z="sd*n1",
                                            x="exp(z) - 1 + 2*(exp(z/2) - 1) + n2")
    code = _code(open(m.header).read())
    for fn in ("muse_model_sample", "muse_model_grad", "muse_model_second"):
        assert _body(code, fn).count("muse_model_exp(") == 1, fn


# ------------------------------------------------------------------------------------------------ the models on the checker
def sv_blocks(theta, N):
    K = len(theta) // 2
    k = (np.arange(N) * K) // N
    th = np.asarray(theta, dtype=np.float64)
    return th[k], th[K + k]


def sv_logLike(x, z, theta):
    mu, tau = sv_blocks(theta, x.size)
    return -0.5 * np.sum(x * x * np.exp(-z) + z + np.exp(-tau) * (z - mu) ** 2) - 0.5 * np.sum(tau)


def sv_grad(x, z, theta):
    mu, tau = sv_blocks(theta, x.size)
    return -(0.5 * (1.0 - x * x * np.exp(-z)) + np.exp(-tau) * (z - mu))


_HOST_WRAPPER = '''
#include <math.h>
#define MUSE_MODEL_FN static inline
#include "%s"
void ev_coefs(double a, double b, double* c) { (void)muse_model_coefs(a, b, c); }
void ev_second(const double* c, long n, const double* x, const double* z, double* out) {
    for (long i = 0; i < n; ++i) muse_model_pair_second(c, x[i], z[i], out + 6 * i, out + 6 * i + 1, out + 6 * i + 2, out + 6 * i + 3, out + 6 * i + 4, out + 6 * i + 5, i);
}
void ev_dx(const double* c, long n, const double* n1, const double* n2, double* out) {
    for (long i = 0; i < n; ++i) muse_model_pair_dx(c, n1[i], n2[i], out + 2 * i, out + 2 * i + 1, i);
}
'''
_host = {}


def pair_host_functions(header):
    """The second-derivative functions of a header of the two-parameter family (muse_model_pair_second, muse_model_pair_dx) and its
    coefficients, evaluated on the host: the header compiled by gcc as the plain C it is (muse_model_exp is libm's exp there,
    include/muse_model.h; no contraction), a few seconds, no engine library.  Returns second(a, b, x, z) -> [n, 6] (ozz, ozx, gza, gzb,
    sxa, sxb) and dx(a, b, n1, n2) -> [n, 2] (xa, xb) for ONE block's parameters."""
    if header in _host:
        return _host[header]
    import ctypes
    import subprocess
    import tempfile
    d = tempfile.mkdtemp()
    src, lib = os.path.join(d, "w.c"), os.path.join(d, "w.so")
    with open(src, "w") as f:
        f.write(_HOST_WRAPPER % header)
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), src, "-o", lib, "-lm"])
    L = ctypes.CDLL(lib)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def coefs(a, b):
        c = np.zeros(4)
        L.ev_coefs(ctypes.c_double(a), ctypes.c_double(b), P(c))
        return c

    def second(a, b, x, z):
        x, z = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(z, np.float64)
        out, c = np.empty((x.size, 6)), coefs(a, b)
        L.ev_second(P(c), ctypes.c_long(x.size), P(x), P(z), P(out))
        return out

    def dx(a, b, n1, n2):
        n1, n2 = np.ascontiguousarray(n1, np.float64), np.ascontiguousarray(n2, np.float64)
        out, c = np.empty((n1.size, 2)), coefs(a, b)
        L.ev_dx(P(c), ctypes.c_long(n1.size), P(n1), P(n2), P(out))
        return out
    _host[header] = (second, dx)
    return _host[header]


def sv_operands(theta, x, z, n1, n2, header=None):
    """(ozz, ozx, gza, gzb, sxa, sxb) [N, 6] and (xa, xb) [N, 2] of the stochastic-volatility model at (x, z) and the normals: from the
    HEADER's own functions (header given: pair_host_functions) or from the closed forms in numpy."""
    theta = np.asarray(theta, dtype=np.float64)
    N, K = x.size, theta.size // 2
    k = (np.arange(N) * K) // N
    sec, dxs = np.empty((N, 6)), np.empty((N, 2))
    for kb in range(K):
        m = k == kb
        mu, tau = theta[kb], theta[K + kb]
        if header is not None:
            second, dx = pair_host_functions(header)
            sec[m], dxs[m] = second(mu, tau, x[m], z[m]), dx(mu, tau, n1[m], n2[m])
        else:
            sd, iv, e = np.exp(0.5 * tau), np.exp(-tau), np.exp(-z[m])
            hx = 0.5 * np.exp(0.5 * (mu + sd * n1[m])) * n2[m]
            zero = np.zeros(int(m.sum()))
            sec[m] = np.stack([0.5 * x[m] * x[m] * e + iv, -x[m] * e, zero - iv, -iv * (z[m] - mu), zero, zero], axis=1)
            dxs[m] = np.stack([hx, hx * 0.5 * sd * n1[m]], axis=1)
    return sec, dxs


def sv_implicit_H(O, N, seed, sim, theta, zhat, header=None):
    """get_H! by implicit differentiation for a header of the two-parameter family, restated from include/muse_model.h
    (MUSE_MODEL_PAIR_SECOND) at the MAP `zhat` of simulation (seed, sim) -- inside `with O.user_model(...)`: x and the normals are the
    checker's; the per-element operands are the HEADER's muse_model_pair_second / muse_model_pair_dx (header given) or the closed forms
    of the stochastic-volatility model.  The Hessian in z is diagonal, so the solve is exact: column q of block kb,
    H[p, q] = sum sxp xq + sum gzp (ozx xq / ozz) over the block, p the block's two parameters."""
    theta = np.asarray(theta, dtype=np.float64)
    K = theta.size // 2
    x, _ = O.sample_x_z("user", N, seed, sim, theta)
    n1, n2 = O.normals(seed, sim, N)
    k = (np.arange(N) * K) // N
    sec, dxs = sv_operands(theta, x, zhat, n1, n2, header)
    ozz, ozx, gz, sx = sec[:, 0], sec[:, 1], (sec[:, 2], sec[:, 3]), (sec[:, 4], sec[:, 5])
    H = np.zeros((2 * K, 2 * K))
    for col in range(2 * K):
        kb, kind = col % K, col // K
        m = k == kb
        xq = dxs[m, kind]
        v = ozx[m] * xq / ozz[m]
        for pk in range(2):
            H[pk * K + kb, col] = np.sum(sx[pk][m] * xq) + np.sum(gz[pk][m] * v)
    return H


def polish(O, x, z0, theta, atol, max_restarts=40):
    """The checker's MAP of x from z0 with its gradient norm below atol: L-BFGS restarted warm from its own result while it ended
    on another rule than the gradient's (Optim's "the value did not change twice", status 2: a value of ~N/2 stops changing in its last
    bit well before a gradient of 1e-8 does, and an exactly repeated value ends the solve; a restart drops the history and goes on).
    Inside `with O.user_model(...)`.  Returns (zhat, the last solve's record, restarts, iterations of all solves)."""
    zh, info = O.zhat_at_theta("user", x, z0, theta, atol)
    restarts, its = 0, info["iterations"]
    while info["status"] != 0 and restarts < max_restarts:
        zh, info = O.zhat_at_theta("user", x, zh, theta, atol)
        restarts += 1
        its += info["iterations"]
    return zh, info, restarts, its


def fd_H(O, N, seed, sim, theta0, h, zfid):
    """get_H! by central differences (src/muse.jl:407-446) from the checker's operators: column j = (s(+h) - s(-h)) / 2 h with
    s(d) the score AT theta0 of the MAP (at theta0, polished to 1e-12 from the fiducial MAP) of the simulation drawn at theta0 + d e_j."""
    theta0 = np.asarray(theta0, dtype=np.float64)
    H = np.empty((theta0.size, theta0.size))
    for j in range(theta0.size):
        s = []
        for sign in (1.0, -1.0):
            th = theta0.copy()
            th[j] += sign * h
            x, _ = O.sample_x_z("user", N, seed, sim, th)
            zh, info, _, _ = polish(O, x, zfid, theta0, 1e-12)
            assert info["status"] == 0 and info["gnorm"] <= 1e-12, info
            s.append(O.grad_theta("user", x, zh, theta0))
        H[:, j] = (s[0] - s[1]) / (2 * h)
    return H


def ln_h(z):
    return 2.0 * np.expm1(0.5 * z)


def ln_blocks(theta, N):
    return np.asarray(theta, dtype=np.float64)[(np.arange(N) * len(theta)) // N]


def ln_logLike(x, z, theta):
    th = ln_blocks(theta, x.size)
    return -0.5 * np.sum((x - ln_h(z)) ** 2 + np.exp(-th) * z * z) - 0.5 * np.sum(th)


def ln_grad(x, z, theta):
    return (x - ln_h(z)) * np.exp(0.5 * z) - np.exp(-ln_blocks(theta, x.size)) * z


CASES = {"sv": dict(theta=[0.3, -0.2, -0.5, 0.4], N=301, logLike=sv_logLike, grad=sv_grad, Hn=2000, Hth=[0.3, -0.5]),
         "ln": dict(theta=[0.4, -0.3, -0.6], N=301, logLike=ln_logLike, grad=ln_grad, Hn=2000, Hth=[-0.2, -0.5])}
_seen = {}


def quantities(O, kind, header, name):
    """Everything the tests below look at, once per header: the draw, value / gradient / score off the draw, the MAP at 1e-8 and
    polished to 1e-13, the implicit-differentiation H and its finite-difference counterpart."""
    if header in _seen:
        return _seen[header]
    c = CASES[kind]
    theta, N = c["theta"], c["N"]
    with O.user_model(header, name):
        q = {}
        q["x"], q["z"] = O.sample_x_z("user", N, 17, 3, theta)
        q["n"] = O.normals(17, 3, N)
        q["zz"] = 0.6 * q["z"] + 0.05
        q["f"], q["g"] = O.logLike_and_grad_z("user", q["x"], q["zz"], theta)
        q["s"] = O.grad_theta("user", q["x"], q["zz"], theta)
        q["s_fd"] = np.empty(len(theta))
        for j in range(len(theta)):
            tp, tm = np.array(theta), np.array(theta)
            tp[j] += 1e-5
            tm[j] -= 1e-5
            q["s_fd"][j] = (O.logLike_and_grad_z("user", q["x"], q["zz"], tp)[0] - O.logLike_and_grad_z("user", q["x"], q["zz"], tm)[0]) / 2e-5
        q["zh"], q["info"], q["restarts"], q["map_its"] = polish(O, q["x"], np.zeros(N), theta, 1e-8)
        q["g_map"] = O.logLike_and_grad_z("user", q["x"], q["zh"], theta)[1]
        q["zh13"], q["info13"], _, _ = polish(O, q["x"], q["zh"], theta, 1e-13)      # the MAP itself, for the twins' comparison
        xf, _ = O.sample_x_z("user", c["Hn"], 5, 0, c["Hth"])
        zfid, q["info_fid"], _, _ = polish(O, xf, np.zeros(c["Hn"]), c["Hth"], 1e-12)
        if kind == "sv":   # (the checker has no implicit-differentiation H of the two-parameter family: the restatement above, from the
            #                 HEADER's muse_model_pair_second / muse_model_pair_dx evaluated on the host, at the checker's MAP)
            q["H"], q["its"] = sv_implicit_H(O, c["Hn"], 5, 0, c["Hth"], zfid, header), np.zeros(len(c["Hth"]), dtype=np.int32)
            n1, n2 = O.normals(5, 0, c["Hn"])
            q["operands"] = sv_operands(c["Hth"], xf, zfid, n1, n2, header)
            q["operands_closed"] = sv_operands(c["Hth"], xf, zfid, n1, n2, None)
        else:
            q["H"], q["its"] = O.implicit_H("user", c["Hn"], 5, 0, c["Hth"], atol=1e-12)
        q["Hfd"] = fd_H(O, c["Hn"], 5, 0, c["Hth"], 1e-4, zfid)
        q["exp"] = np.vectorize(O.exp_fixed)
    _seen[header] = q
    return q


def check_model(O, kind, header, name):
    c = CASES[kind]
    theta, N = c["theta"], c["N"]
    q = quantities(O, kind, header, name)
    x, z, zz, (n1, n2) = q["x"], q["z"], q["zz"], q["n"]
    # the draw against the closed form -- in the checker's own exponential (bit for bit in z, to rounding in x), and in numpy's
    if kind == "sv":
        mu, tau = sv_blocks(theta, N)
        zc = mu + q["exp"](0.5 * tau) * n1
        xc, xn = q["exp"](0.5 * z) * n2, np.exp(0.5 * z) * n2
    else:
        zc = q["exp"](0.5 * ln_blocks(theta, N)) * n1
        xc, xn = 2.0 * q["exp"](0.5 * z) + (n2 - 2.0), ln_h(z) + n2
    # (the header rounds mu + sd n1 once, in an fma, numpy twice: a few ulps of the larger term)
    assert np.abs(z - zc).max() <= 4e-15 * max(1.0, np.abs(z).max())
    assert np.abs(x - xc).max() <= 4e-15 * max(1.0, np.abs(x).max())
    np.testing.assert_allclose(x, xn, rtol=1e-14, atol=1e-14)
    # value and gradient against the closed forms, the gradient against central differences of the value
    np.testing.assert_allclose(q["f"], c["logLike"](x, zz, theta), rtol=1e-13)
    np.testing.assert_allclose(q["g"], c["grad"](x, zz, theta), rtol=1e-12, atol=1e-13)
    for i in (0, N // 2, N - 1):
        e = np.zeros(N)
        e[i] = 1e-5
        fd = (c["logLike"](x, zz + e, theta) - c["logLike"](x, zz - e, theta)) / 2e-5
        np.testing.assert_allclose(q["g"][i], fd, rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(q["s"], q["s_fd"], rtol=1e-7, atol=1e-8)          # the score: d logLike / d theta
    # the MAP at atol = 1e-8: converged on the gradient's rule (status 0; polish() restarts a solve that ended on the unchanged value),
    # stationary by the checker's gradient and by the closed form, not a one-step problem
    info = q["info"]
    assert info["status"] == 0 and info["gnorm"] <= 1e-8 and q["map_its"] > 3, (info, q["restarts"])
    assert np.abs(q["g_map"]).max() <= 1e-8 and np.abs(c["grad"](x, q["zh"], theta)).max() <= 1e-8 + 1e-12, info
    assert q["info13"]["status"] == 0 and q["info13"]["gnorm"] <= 1e-13 and q["info_fid"]["status"] == 0, (q["info13"], q["info_fid"])
    # get_H! by implicit differentiation through the header's second derivatives against central differences of polished maps, to the
    # tolerance of the cubic model's test (tests/test_user_model.py)
    assert np.all(q["its"] >= 1) or kind == "sv"
    np.testing.assert_allclose(q["H"], q["Hfd"], rtol=1e-7, atol=1e-6)
    if kind == "sv":   # the header's second derivatives and draw derivatives against the closed forms (libm's exp on both sides)
        for got, want in zip(q["operands"], q["operands_closed"]):
            np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-15)
    print(kind, name, "MAP iterations", q["map_its"], "warm restarts", q["restarts"], "CG iterations", q["its"])
    return q


def check_consistency(M, O, header, name, nth, theta):
    from oracle_problem import OracleMuseProblem
    with O.user_model(header, name):
        res = M.check_model_consistency(OracleMuseProblem(None, model="user", ntheta=nth, N=2001), theta, rng=5)
    assert res["grad_z"] <= 2e-5 + res["noise_floor"] and res["grad_theta"] <= 2e-5 + res["noise_floor"] and res["noise_floor"] < 1e-4, res


def assert_twins_agree(a, b):
    """The hand-written and the generated header: another order of the same operations -- rtol 1e-12 on everything."""
    for key in ("x", "z", "f", "g", "s", "H", "zh13"):      # (zh13: the MAP, each header's own solve polished to a gradient of 1e-13)
        np.testing.assert_allclose(b[key], a[key], rtol=1e-12, err_msg=key)
    assert np.array_equal(a["its"], b["its"])
    # ... and each header's MAP at 1e-8 is the MAP to what that tolerance means: |grad| / min curvature
    for q in (a, b):
        assert np.abs(q["zh"] - a["zh13"]).max() <= 1e-8 / 0.5


def test_stochastic_volatility_on_the_checker(M, O):
    check_model(O, "sv", SV, "stochastic_volatility")
    check_consistency(M, O, SV, "stochastic_volatility", 4, CASES["sv"]["theta"])


def test_generated_stochastic_volatility_on_the_checker(M, O):
    m = generated_sv(M)
    b = check_model(O, "sv", m.header, m.library_name)
    check_consistency(M, O, m.header, m.library_name, 4, CASES["sv"]["theta"])
    assert_twins_agree(quantities(O, "sv", SV, "stochastic_volatility"), b)


def test_lognormal_obs_on_the_checker(M, O):
    check_model(O, "ln", LN, "lognormal_obs")
    check_consistency(M, O, LN, "lognormal_obs", 3, CASES["ln"]["theta"])


def test_generated_lognormal_obs_on_the_checker(M, O):
    m = generated_ln(M)
    b = check_model(O, "ln", m.header, m.library_name)
    check_consistency(M, O, m.header, m.library_name, 3, CASES["ln"]["theta"])
    assert_twins_agree(quantities(O, "ln", LN, "lognormal_obs"), b)


# ------------------------------------------------------------------------------------------------ the libraries' kernels
def _regs():
    spec = importlib.util.spec_from_file_location("regs", os.path.join(ROOT, "tools", "regs.py"))
    regs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(regs)
    return regs


def _rows_of(section):
    """{kernel: (vgpr, vspill, sspill, scratch)} of one `== <section>` block of profiles/r18_model_exp_resources.txt."""
    text = open(PROFILE).read().split("== " + section + "\n")[1].split("\n== ")[0]
    rows = {}
    for line in text.splitlines():
        m = re.match(r"(\S+)\s+vgpr\s+(\d+)\s+vspill\s+(\d+)\s+sspill\s+(\d+)\s+scratch\s+(\d+)", line)
        if m:
            rows[m.group(1)] = tuple(int(v) for v in m.groups()[1:])
    return rows


RESIDENT_10 = "PlaceResidentILi512ELi10ELb1ELb0EE"      # PlaceResident<512, 10, true>: x and g in LDS, ten element pairs per thread


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="llvm-readelf not available")
def test_kernel_resources_of_the_libraries_with_an_exponential(M):
    """Builds the libraries the GPU tests load (the two models and tests/models/exp_probe.h) and reads their code objects.
    lognormal_obs: no kernel calls a device function or keeps more than 256 bytes of scratch per lane (regs.check_library == []).
    stochastic_volatility: the same for every kernel the engine launches -- what is beyond the bound (recorded in
    profiles/r18_model_exp_resources.txt: the four- and eight-parameter kernels of PlaceResident<512, 10>, 328 / 296 bytes for the map
    kernels against 944 / 976 with the branchy exponential inlined, 348 / 428 against 1036 / 1068 for their loop kernels) is what the engine fences: the map
    kernels by map_unfit_mask (muse_engine.cpp: the shape streams), the loop kernels by loop_usable (the host loop runs).  The fence
    can never trigger for the libraries that existed before: their resident map kernels are within the bound; and cubic's rows are
    those of the parent commit (the profile file's `cubic before`)."""
    regs = _regs()
    libs = {name: M.ElementwiseModel.packaged(name).library() for name in ("lognormal_obs", "stochastic_volatility", "cubic", "normal_mean_var")}
    M.ElementwiseModel("exp_probe", PROBE).library()
    assert regs.check_library(libs["lognormal_obs"]) == []
    beyond = regs.check_library(libs["stochastic_volatility"])
    assert not any(r[5] for r in beyond), beyond                                         # no calls anywhere
    for r in beyond:                                                                      # ... and only fenced kernels beyond the bound
        assert RESIDENT_10 in r[0] and ("UserModelILi4E" in r[0] or "UserModelILi8E" in r[0]), r
    assert all(r[4] <= regs.LIBRARY_SCRATCH_LIMIT for r in regs.library_report(libs["stochastic_volatility"]) if "UserModelILi2E" in r[0])
    recorded = _rows_of("stochastic_volatility after")
    for r in beyond:
        assert r[0] in recorded, r[0]
    for name in ("cubic", "normal_mean_var"):     # the never-triggering condition: map kernels of the resident placements within the bound
        rows = regs.library_report(libs[name])
        resident = [r for r in rows if "PlaceResident" in r[0] and not r[0].startswith("loop:")]
        assert len(resident) >= 6 and all(r[4] <= regs.LIBRARY_SCRATCH_LIMIT and not r[5] for r in resident), (name, resident)
    now = {r[0]: tuple(r[1:5]) for r in regs.library_report(libs["cubic"])}
    assert now == _rows_of("cubic before") == _rows_of("cubic after")
