"""An instrument whose blur is not the built-in one: the coupled `smooth` model with the operator's weights as state of the problem.

    z_i ~ N(0, e^theta),   x = A z + n,   (A z)_i = w1 (z_{i-1} + z_{i+1}) + w0 z_i  (periodic),   n_i ~ N(0, 1)

Data are drawn with a narrow and with a wide stencil, muse() runs on each with the weights it was drawn with -- on the HIP path,
the operator read by the kernels at run time (HipMuseProblem(..., stencil=(w0, w1))) -- and the answer is set next to the exact
posterior: the model is jointly Gaussian and A is circulant, so the marginal likelihood is a sum over Fourier modes with
a_q = w0 + 2 w1 cos(2 pi q / N) (the variance of mode q is 1 + e^theta a_q^2)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from scipy.optimize import brentq

import museinference_jl_amd as M

N, truth, nsims, prior_sigma = 8192, 1.0, 128, 3.0


def exact_posterior(x, w):
    a2 = (w[0] + 2 * w[1] * np.cos(2 * np.pi * np.arange(x.size) / x.size)) ** 2
    p = np.abs(np.fft.fft(x)) ** 2 / x.size
    dlogp = lambda t: 0.5 * np.sum(np.exp(t) * a2 * (p - (1 + np.exp(t) * a2)) / (1 + np.exp(t) * a2) ** 2) - t / prior_sigma ** 2
    mode = brentq(dlogp, -8.0, 8.0, xtol=1e-13)
    u = np.exp(mode) * a2 / (1 + np.exp(mode) * a2)
    return mode, 1.0 / np.sqrt(0.5 * np.sum(u ** 2) + 1.0 / prior_sigma ** 2)


for name, w in (("narrow", (0.8, 0.1)), ("wide", (0.4, 0.3))):
    draw = M.HipMuseProblem(None, model="smooth", ntheta=1, N=N, stencil=w)
    x, _ = draw.sample_x_z(M.SimRng(2024, M.DATA_SIM), [truth])
    draw.close()
    prob = M.HipMuseProblem(x, model="smooth", ntheta=1, prior=M.GaussianPrior(0.0, prior_sigma), stencil=w)
    res = M.muse(prob, [0.0], rng=1, nsims=nsims, maxsteps=40, theta_rtol=1e-5, grad_z_logLike_atol=1e-6, get_covariance=True)
    mode, sigma = exact_posterior(x, w)
    got = float(np.sqrt(np.atleast_2d(res.Sigma)[0, 0]))
    print(f"{name:6s} stencil {w}: muse theta = {res.theta[0]:+.4f} +- {got:.4f}   exact posterior {mode:+.4f} +- {sigma:.4f}"
          f"   (truth {truth:+.1f}; Monte-Carlo error of the mode {sigma / np.sqrt(nsims):.4f})")
    assert abs(res.theta[0] - mode) < 5 * sigma / np.sqrt(nsims) and abs(got / sigma - 1) < 0.3
    prob.close()
