"""SimpleMuseProblem (src/simple.jl:4-12, 79-95): a problem given as CLOSURES, differentiated by AD.

    prob = TorchMuseProblem(x, sample_x_z, logLike, logPrior=None, device="cuda")
        sample_x_z(generator, theta) -> (x, z)      torch tensors on `device`, drawn with the torch.Generator it is given
        logLike(x, z, theta)         -> 0-d tensor  log P(x, z | theta), differentiable in z and theta (theta: a float64 tensor)
        logPrior(theta)              -> 0-d tensor  (default: flat)

grad_z and grad_theta come from torch.autograd -- the reference uses ForwardDiff / Zygote (src/simple.jl:84-85) -- and the MAP from
the interface's default `ẑ_at_θ` (src/interface.jl:140-166; optim.py: L-BFGS + HagerZhang on the device's tensors).  This is the
GENERAL front-end: any logLike, any coupling between the elements, any number of parameters -- at the price of one autograd pass and
a dozen small torch kernels per evaluation, simulation after simulation.  A model of the elementwise families belongs in a header
(models.ElementwiseModel: hand-written, or generated from its terms by symbolic.py) behind HipMuseProblem, where a whole batch of
simulations is ONE launch of the HIP solver; this class is what runs the models those families do not hold.  Nothing routes from
one to the other: which one runs is the caller's choice of class.

Everything of the host driver applies (muse, get_J_, get_H_ by finite differences, transforms, checkpoints): the driver sees an
AbstractMuseProblem.
"""
import numpy as np

from .problem import AbstractMuseProblem, SimRng, UnTransformedθ
from . import optim


class TorchMuseProblem(AbstractMuseProblem):
    def __init__(self, x, sample_x_z, logLike, logPrior=None, device=None, dtype=None, hess_diag=None):
        import torch
        self._torch = torch
        self.device = torch.device(device) if device is not None else (x.device if torch.is_tensor(x) else torch.device("cpu"))
        self.dtype = dtype or torch.float64
        self.x = None if x is None else self._t(x)
        self._sample, self._logLike, self._logPrior = sample_x_z, logLike, logPrior
        self._hess_diag = self._checked_hess_diag(hess_diag)

    # -- what implicit_diff_cg_kwargs' Pl = "jacobi" means for a closure: the diagonal of -∂²logLike/∂z² at a fiducial MAP
    def _checked_hess_diag(self, hess_diag):
        """hess_diag: None; a callable (x [B, ...], z [B, ...], θ [B, nθ]) -> [B, ...], the diagonal itself; "elementwise" (one all-ones
        probe: exact for uncoupled latents); or a tensor of probes [k, *zshape] with 0 / 1 entries that partition the latent elements --
        the diagonal is then Σ_c v_c ⊙ (M v_c), k Hessian-vector products, exact when no two coupled elements share a probe (a
        colouring, for stencil-like couplings).  The diagonal only preconditions conjugate gradients: any positive one gives the same
        H to the tolerance and only the counts move, so an inexact probing costs iterations, never correctness; a diagonal that is
        not positive is reported through a negative count."""
        torch = self._torch
        if hess_diag is None or callable(hess_diag) or (isinstance(hess_diag, str) and hess_diag == "elementwise"):
            return hess_diag
        if isinstance(hess_diag, str) or not torch.is_tensor(hess_diag):
            raise ValueError(f'hess_diag must be None, a callable, "elementwise" or a tensor of probes [k, *zshape]; got {hess_diag!r}')
        probes = hess_diag.detach().to(self.device, self.dtype)
        if probes.dim() < 2 or probes.shape[0] < 1:
            raise ValueError("hess_diag: a tensor of probes has shape [k, *zshape] with k >= 1")
        if not bool(((probes == 0) | (probes == 1)).all()) or not bool((probes.sum(dim=0) == 1).all()):
            raise ValueError("hess_diag: the probes must partition the latent elements (entries 0 or 1, every element in exactly one probe)")
        return probes

    @staticmethod
    def _checked_cg_Pl(cg_Pl, hess_diag):
        if cg_Pl is None:
            return False
        if not (isinstance(cg_Pl, str) and cg_Pl == "jacobi"):
            raise ValueError(f'implicit_H_batch: cg_Pl must be None (the identity) or "jacobi"; got {cg_Pl!r}')
        if hess_diag is None:
            raise ValueError('implicit_H_batch: cg_Pl="jacobi" needs the diagonal of the closure\'s Hessian in z: construct the problem with '
                             'hess_diag (a callable, a tensor of probes or "elementwise")')
        return True

    def _hess_diagonal(self, X, Z, TH, hvp):
        """The diagonal [S, N] of M = -∂²logLike/∂z² for S simulations at Z [S, *zshape]; hvp(V [S, *zshape]) -> M V [S, *zshape]."""
        torch = self._torch
        S, zshape = Z.shape[0], tuple(Z.shape[1:])
        hd = self._hess_diag
        if callable(hd):
            with torch.no_grad():
                d = hd(X, Z, TH)
            if not torch.is_tensor(d) or d.numel() != Z.numel():
                raise ValueError(f"hess_diag(x, z, θ) must return a tensor of z's shape {tuple(Z.shape)}")
            return d.detach().to(self.device, self.dtype).reshape(S, -1).contiguous()
        probes = torch.ones((1,) + zshape, dtype=self.dtype, device=self.device) if isinstance(hd, str) else hd
        if tuple(probes.shape[1:]) != zshape:
            raise ValueError(f"hess_diag: probes of shape {tuple(probes.shape)} do not match the latent shape {zshape}")
        d = torch.zeros((S,) + zshape, dtype=self.dtype, device=self.device)
        for c in range(probes.shape[0]):
            V = probes[c].expand((S,) + zshape).contiguous()
            d = d + V * hvp(V).detach().reshape(V.shape)
        return d.reshape(S, -1).contiguous()

    # -- tensors in, numpy for theta-sized results out (the driver's algebra is numpy)
    def _t(self, v):
        torch = self._torch
        return v.to(self.device, self.dtype) if torch.is_tensor(v) else torch.as_tensor(np.asarray(v, dtype=np.float64), device=self.device).to(self.dtype)

    def _theta(self, theta, grad=False):
        t = self._torch.as_tensor(np.atleast_1d(np.asarray(theta, dtype=np.float64)), device=self.device).to(self.dtype)
        return t.requires_grad_(True) if grad else t

    def sample_x_z(self, rng, theta):
        """A stream per (master seed, simulation index), never advanced by the caller (src/util.jl:87-92): the generator handed to the
        closure is seeded from the pair, so a simulation's draw depends on nothing else."""
        torch = self._torch
        gen = torch.Generator(device=self.device)
        gen.manual_seed(self._stream(rng if isinstance(rng, SimRng) else SimRng(int(rng), 0)))
        with torch.no_grad():
            x, z = self._sample(gen, self._theta(theta))
        return self._t(x), self._t(z)

    def logLike_and_grad_z_logLike(self, x, z, theta):
        torch = self._torch
        zt = self._t(z).detach().clone().requires_grad_(True)
        with torch.enable_grad():
            f = self._logLike(self._t(x), zt, self._theta(theta))
            g, = torch.autograd.grad(f, zt)
        return float(f.detach()), g

    def grad_theta_logLike(self, x, z, theta, theta_space=UnTransformedθ):
        torch = self._torch
        th = self.inv_transform_theta(theta) if theta_space is not UnTransformedθ else theta
        tt = self._theta(th, grad=True)
        with torch.enable_grad():
            f = self._logLike(self._t(x), self._t(z).detach(), tt)
            g, = torch.autograd.grad(f, tt, allow_unused=True)
        g = np.zeros(tt.numel()) if g is None else g.detach().cpu().numpy().astype(np.float64)
        if theta_space is not UnTransformedθ:       # chain rule through the transform, by central differences (as check_self_consistency)
            g = self._jac_inv_transform(np.atleast_1d(np.asarray(theta, dtype=np.float64))).T @ g
        return g

    def _jac_inv_transform(self, theta_t, step=1e-6):
        n = theta_t.size
        J = np.zeros((n, n))
        for j in range(n):
            e = np.zeros(n)
            e[j] = step
            J[:, j] = (np.atleast_1d(self.inv_transform_theta(theta_t + e)) - np.atleast_1d(self.inv_transform_theta(theta_t - e))) / (2 * step)
        return J

    def zhat_at_theta(self, x, z0, theta, grad_z_logLike_atol=1e-2):
        """ẑ_at_θ, the interface's default (src/interface.jl:140-166): minimise -logLike over z from z0, g_tol = the tolerance."""
        torch = self._torch
        xt, tt = self._t(x), self._theta(theta)

        def fg(z):
            zt = z.detach().clone().requires_grad_(True)
            with torch.enable_grad():
                f = -self._logLike(xt, zt, tt)
                g, = torch.autograd.grad(f, zt)
            return float(f.detach()), g
        z, info = optim.lbfgs(fg, self._t(z0).reshape(-1), grad_z_logLike_atol)
        rec = np.zeros((), dtype=_info_dtype())
        for k in ("iterations", "f_calls", "status"):
            rec[k] = info[k]
        rec["f_min"], rec["gnorm"] = info["f_min"], info["gnorm"]
        return z.reshape(self._t(z0).shape), rec

    def zhat_guess_from_truth(self, x, z, theta):
        return self._torch.zeros_like(self._t(z))

    # -- get_H! by implicit differentiation (src/muse.jl:335-405), every derivative by autograd as the reference takes them by nested AD
    def implicit_H_batch(self, seed, sim_begin, sim_end, theta0, atol=1e-1, cg_maxiter=100, cg_reltol=1.4901161193847656e-08, cg_Pl=None):
        """Per simulation H = H1 - dFdθᵀ A⁻¹ dFdθ1: H1 the Jacobian of the score through the DRAW x(θ) at fixed ẑ, dFdθ = ∂θ ∇z logLike,
        dFdθ1 = ∂θ ∇z logLike(x(θ), ẑ, θ₀), A the Hessian of logLike in z applied by double backward, A⁻¹ by conjugate gradients (reltol
        sqrt(eps), maxiter 100: IterativeSolvers' defaults).  The draw is differentiated through the closure itself (the generator
        re-seeded: the same random numbers at every θ), so sample_x_z must be written with differentiable torch operations.
        cg_Pl="jacobi" preconditions the solves with the diagonal the constructor's hess_diag describes (_pcg; a ValueError, raised before
        any draw, without one): the same H to the tolerance, fewer iterations; a count is then -1 - iterations where the diagonal or
        p.Ap was not positive.  Returns (Hs [n, nθ, nθ], CG iteration counts [n, nθ])."""
        torch = self._torch
        jacobi = self._checked_cg_Pl(cg_Pl, self._hess_diag)
        th0 = self._theta(theta0)
        nt = th0.numel()
        Hs, its = [], []
        jac = torch.autograd.functional.jacobian
        for sim in range(int(sim_begin), int(sim_end)):
            rng = SimRng(int(seed), sim)
            x, z = self.sample_x_z(rng, theta0)
            zh, _ = self.zhat_at_theta(x, self.zhat_guess_from_truth(x, z, theta0), theta0, atol)
            zh = zh.detach()

            def x_of(th):          # the draw at th, the simulation's own random numbers
                gen = torch.Generator(device=self.device)
                gen.manual_seed(self._stream(rng))
                return self._sample(gen, th)[0].to(self.dtype)

            def grad_z(xx, zz, th):
                zz = zz if zz.requires_grad else zz.detach().clone().requires_grad_(True)
                return torch.autograd.grad(self._logLike(xx, zz, th), zz, create_graph=True)[0]

            def score(xx, th_eval):
                tt = th_eval.detach().clone().requires_grad_(True)
                return torch.autograd.grad(self._logLike(xx, zh, tt), tt, create_graph=True)[0]
            with torch.enable_grad():
                H1 = jac(lambda th: score(x_of(th), th0), th0).reshape(nt, nt)
                dF = jac(lambda th: grad_z(x, zh, th), th0).reshape(-1, nt)
                dF1 = jac(lambda th: grad_z(x_of(th), zh, th0), th0).reshape(-1, nt)
                zz = zh.clone().requires_grad_(True)
                g = torch.autograd.grad(self._logLike(x, zz, th0), zz, create_graph=True)[0].reshape(-1)

                def A(w):          # Hessian of logLike in z at the MAP, applied
                    return torch.autograd.grad(g, zz, w.reshape(zz.shape), retain_graph=True)[0].reshape(-1)
                if jacobi:
                    d = self._hess_diagonal(x[None], zh[None], th0[None], lambda V: -A(V[0])[None])[0]
                cols, n_it = [], []
                for j in range(nt):
                    if jacobi:
                        y, k = _pcg(lambda w: -A(w), -dF1[:, j].detach(), d, cg_maxiter, cg_reltol)
                    else:
                        y, k = _cg(lambda w: -A(w), -dF1[:, j].detach(), cg_maxiter, cg_reltol)     # (-A is positive definite at a maximum)
                    cols.append(y)
                    n_it.append(k)
            H = H1.detach() - dF.detach().T @ torch.stack(cols, dim=1)
            Hs.append(H.cpu().numpy().astype(np.float64))
            its.append(n_it)
        return np.array(Hs).reshape(-1, nt, nt), np.array(its, dtype=np.int32).reshape(-1, nt)

    @staticmethod
    def _stream(rng):
        return (int(rng.seed) * 0x9E3779B97F4A7C15 + int(rng.sim) * 0xBF58476D1CE4E5B9 + 0x94D049BB133111EB) % (1 << 63)

    # -- prior: the closure, differentiated (the reference: ForwardDiff, src/muse.jl:184,207,539)
    def logPrior_theta(self, theta, theta_space=UnTransformedθ):
        if self._logPrior is None:
            return 0.0
        th = self.inv_transform_theta(theta) if theta_space is not UnTransformedθ else theta
        return float(self._logPrior(self._theta(th)))

    def grad_logPrior_theta(self, theta, theta_space=UnTransformedθ):
        n = np.atleast_1d(np.asarray(theta)).size
        if self._logPrior is None:
            return np.zeros(n)
        if theta_space is not UnTransformedθ:
            return _fd_grad(lambda t: self.logPrior_theta(t, theta_space), np.atleast_1d(np.asarray(theta, dtype=np.float64)))
        torch = self._torch
        tt = self._theta(theta, grad=True)
        with torch.enable_grad():
            g, = torch.autograd.grad(self._logPrior(tt), tt, allow_unused=True)
        return np.zeros(n) if g is None else g.detach().cpu().numpy().astype(np.float64)

    def hess_logPrior_theta(self, theta, theta_space=UnTransformedθ):
        n = np.atleast_1d(np.asarray(theta)).size
        if self._logPrior is None:
            return np.zeros((n, n))
        t0 = np.atleast_1d(np.asarray(theta, dtype=np.float64))
        if theta_space is not UnTransformedθ:
            H = np.zeros((n, n))
            for j in range(n):
                e = np.zeros(n)
                e[j] = 1e-5
                H[:, j] = (self.grad_logPrior_theta(t0 + e, theta_space) - self.grad_logPrior_theta(t0 - e, theta_space)) / 2e-5
            return 0.5 * (H + H.T)
        torch = self._torch
        H = torch.autograd.functional.hessian(lambda t: self._logPrior(t), self._theta(t0))
        return H.detach().cpu().numpy().astype(np.float64).reshape(n, n)


class LbfgsBatch:
    """libmuse_lbfgs.so (include/muse_lbfgs.h) for one batch shape [nprob, n] on a GPU: the workspace, the evaluation points and the
    word the kernel reports into are allocated once, as torch tensors; every launch goes to torch's current stream.

        batch.begin(z0, g_tol);  repeat: f, g at batch.z_eval -> active = batch.advance(f, g)  until active == 0;  batch.result()
    """

    def __init__(self, device, nprob, n):
        import torch
        from . import _capi
        self._torch, self._capi, self._lib = torch, _capi, _capi.load_lbfgs_library()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _capi.MuseError(-3, "no HIP device available (libmuse_lbfgs has no CPU fallback)")
        self.nprob, self.n, self.m = int(nprob), int(n), _capi.LBFGS_M
        nbytes = _capi.check_lbfgs(self._lib.muse_lbfgs_workspace_bytes(self.nprob, self.n, self.m))
        self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.z_eval = torch.empty((self.nprob, self.n), dtype=torch.float64, device=self.device)
        self._active = torch.zeros(1, dtype=torch.int32).pin_memory()
        self._info = torch.empty(self.nprob * _capi.INFO_DTYPE.itemsize, dtype=torch.uint8, device=self.device)
        self.rounds = self.syncs = 0
        self._diag = None          # (diagonal, rows_per_diag) of a preconditioned solve, from begin to result
        self.timing, self.advance_ms = False, 0.0      # timing: device time of the advance launches, summed (tools/closures_bench.py)

    def _stream(self):
        return self._torch.cuda.current_stream(self.device).cuda_stream

    def _rows(self, t, shape):
        torch = self._torch
        if not (torch.is_tensor(t) and t.device == self.z_eval.device and t.dtype == torch.float64 and tuple(t.shape) == shape):
            raise ValueError(f"expected a float64 tensor of shape {shape} on {self.z_eval.device}")
        return t.contiguous()

    def begin(self, z0, g_tol, maxiter=1000):
        z0 = self._rows(z0, (self.nprob, self.n))
        with self._torch.cuda.device(self.device):
            self._capi.check_lbfgs(self._lib.muse_lbfgs_begin(self._ws.data_ptr(), self.nprob, self.n, self.m, z0.data_ptr(), float(g_tol),
                                                              int(maxiter), self.z_eval.data_ptr(), self._stream()))
        self.rounds = self.syncs = 0

    def advance(self, f, g):
        """One round: f [nprob], g [nprob, n] at z_eval.  Returns the number of problems still active (the round's ONE synchronisation)."""
        f, g = self._rows(f, (self.nprob,)), self._rows(g, (self.nprob, self.n))
        stream = self._torch.cuda.current_stream(self.device)
        if self.timing:
            e0, e1 = self._torch.cuda.Event(enable_timing=True), self._torch.cuda.Event(enable_timing=True)
            e0.record(stream)
        with self._torch.cuda.device(self.device):
            self._capi.check_lbfgs(self._lib.muse_lbfgs_advance(self._ws.data_ptr(), self.nprob, self.n, self.m, f.data_ptr(), g.data_ptr(),
                                                                self.z_eval.data_ptr(), self._active.data_ptr(), self._stream()))
        if self.timing:
            e1.record(stream)
        stream.synchronize()
        if self.timing:
            self.advance_ms += e0.elapsed_time(e1)
        self.rounds += 1
        self.syncs += 1
        return int(self._active[0])

    def result(self):
        """(ẑ [nprob, n] -- a new tensor on the device --, records [nprob] in _capi.INFO_DTYPE)"""
        z = self._torch.empty_like(self.z_eval)
        with self._torch.cuda.device(self.device):
            self._capi.check_lbfgs(self._lib.muse_lbfgs_result(self._ws.data_ptr(), self.nprob, self.n, self.m, z.data_ptr(),
                                                               self._info.data_ptr(), self._stream()))
        info = np.frombuffer(self._info.cpu().numpy().tobytes(), dtype=self._capi.INFO_DTYPE).copy()
        self.syncs += 1
        return z, info


class CgBatch:
    """libmuse_lbfgs.so's lock-step conjugate gradients (include/muse_lbfgs.h, muse_lbfgs_cg_*) for one batch shape [nrows, n] on a GPU:
    row r is one system M_r y = b_r whose operator the caller applies.  The workspace, the direction rows and the word the kernel
    reports into are allocated once, as torch tensors; every launch goes to torch's current stream.

        active = cg.begin(b, reltol, abstol, maxiter);  while active: Mp = M applied to cg.p_eval -> active = cg.advance(Mp);  cg.result()

    The direction lives in `p_eval` and nowhere else: read it, never write it.  begin(..., diag=d) preconditions the solve with
    Diagonal(d) (see there); without it every call is plain CG's.
    """

    def __init__(self, device, nrows, n):
        import torch
        from . import _capi
        self._torch, self._capi, self._lib = torch, _capi, _capi.load_lbfgs_library()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _capi.MuseError(-3, "no HIP device available (libmuse_lbfgs has no CPU fallback)")
        self.nrows, self.n = int(nrows), int(n)
        nbytes = _capi.check_lbfgs(self._lib.muse_lbfgs_cg_workspace_bytes(self.nrows, self.n))
        self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.p_eval = torch.zeros((self.nrows, self.n), dtype=torch.float64, device=self.device)
        self._active = torch.zeros(1, dtype=torch.int32).pin_memory()
        self._its = torch.empty(self.nrows, dtype=torch.int32, device=self.device)
        self._res = torch.empty(self.nrows, dtype=torch.float64, device=self.device)
        self.rounds = self.syncs = 0
        self._diag = None          # (diagonal, rows_per_diag) of a preconditioned solve, from begin to result
        self.timing, self.advance_ms = False, 0.0      # timing: device time of the advance launches, summed (tools/closures_implicit_bench.py)

    def _stream(self):
        return self._torch.cuda.current_stream(self.device).cuda_stream

    def _rows(self, t):
        torch = self._torch
        if not (torch.is_tensor(t) and t.device == self.p_eval.device and t.dtype == torch.float64 and tuple(t.shape) == (self.nrows, self.n)):
            raise ValueError(f"expected a float64 tensor of shape {(self.nrows, self.n)} on {self.p_eval.device}")
        if t.data_ptr() == self.p_eval.data_ptr():
            raise ValueError("p_eval is the solver's own: pass a tensor of the caller's")
        return t.contiguous()

    def _wait(self):
        self._torch.cuda.current_stream(self.device).synchronize()
        self.syncs += 1
        return int(self._active[0])

    def _diagonal(self, diag, rows_per_diag):
        torch, k = self._torch, int(rows_per_diag)
        if k < 1 or self.nrows % k != 0:
            raise ValueError(f"rows_per_diag must be at least 1 and divide the number of rows ({self.nrows}); got {rows_per_diag!r}")
        shape = (self.nrows // k, self.n)
        if not (torch.is_tensor(diag) and diag.device == self.p_eval.device and diag.dtype == torch.float64 and tuple(diag.shape) == shape):
            raise ValueError(f"diag: expected a float64 tensor of shape {shape} on {self.p_eval.device}")
        return diag.contiguous(), k

    def begin(self, b, reltol, abstol=0.0, maxiter=100, diag=None, rows_per_diag=1):
        """Start every row at y = 0 with right-hand side b [nrows, n]; p_eval = b.  Returns the number of active rows (one synchronisation).

        With `diag` -- a float64 tensor [nrows / rows_per_diag, n] on the device, row r reading diagonal row r // rows_per_diag -- the
        solve is preconditioned by Diagonal(diag) (muse_lbfgs_pcg_*): p_eval = b / diag, and advance() goes on with the same diagonal,
        which is held until result().  Any diagonal of positive finite entries gives the same solution to the tolerance, only the
        counts move; a row whose diagonal holds an entry that is not positive or not finite ends at once with the count -1 and y = 0."""
        b = self._rows(b)
        self._diag = None if diag is None else self._diagonal(diag, rows_per_diag)
        self.rounds = self.syncs = 0
        self.advance_ms = 0.0
        with self._torch.cuda.device(self.device):
            if self._diag is None:
                rc = self._lib.muse_lbfgs_cg_begin(self._ws.data_ptr(), self.nrows, self.n, b.data_ptr(), float(reltol), float(abstol),
                                                   int(maxiter), self.p_eval.data_ptr(), self._active.data_ptr(), self._stream())
            else:
                d, k = self._diag
                rc = self._lib.muse_lbfgs_pcg_begin(self._ws.data_ptr(), self.nrows, self.n, b.data_ptr(), d.data_ptr(), k, float(reltol),
                                                    float(abstol), int(maxiter), self.p_eval.data_ptr(), self._active.data_ptr(), self._stream())
            self._capi.check_lbfgs(rc)
        return self._wait()

    def advance(self, Mp):
        """One round: Mp [nrows, n] = M applied to p_eval.  Returns the number of rows still active (the round's ONE synchronisation)."""
        Mp = self._rows(Mp)
        stream = self._torch.cuda.current_stream(self.device)
        if self.timing:
            e0, e1 = self._torch.cuda.Event(enable_timing=True), self._torch.cuda.Event(enable_timing=True)
            e0.record(stream)
        with self._torch.cuda.device(self.device):
            if self._diag is None:
                rc = self._lib.muse_lbfgs_cg_advance(self._ws.data_ptr(), self.nrows, self.n, Mp.data_ptr(), self.p_eval.data_ptr(),
                                                     self._active.data_ptr(), self._stream())
            else:
                d, k = self._diag
                rc = self._lib.muse_lbfgs_pcg_advance(self._ws.data_ptr(), self.nrows, self.n, Mp.data_ptr(), d.data_ptr(), k,
                                                      self.p_eval.data_ptr(), self._active.data_ptr(), self._stream())
            self._capi.check_lbfgs(rc)
        if self.timing:
            e1.record(stream)
        active = self._wait()
        if self.timing:
            self.advance_ms += e0.elapsed_time(e1)
        self.rounds += 1
        return active

    def result(self):
        """(y [nrows, n] -- a new tensor on the device --, counts [nrows] int32 (negative: -1 - iterations, the guard stopped the row),
        |r| [nrows], the recurrence residual; the last two on the host)"""
        y = self._torch.empty_like(self.p_eval)
        with self._torch.cuda.device(self.device):
            self._capi.check_lbfgs(self._lib.muse_lbfgs_cg_result(self._ws.data_ptr(), self.nrows, self.n, y.data_ptr(), self._its.data_ptr(),
                                                                  self._res.data_ptr(), self._stream()))
        its, res = self._its.cpu().numpy().copy(), self._res.cpu().numpy().copy()
        self.syncs += 1
        self._diag = None
        return y, its, res


class EngineNormals:
    """The ENGINE's normal streams (csrc/rng.hpp; include/muse_lbfgs.h, muse_lbfgs_normals) for a batch of simulations: row b draws from
    stream (seed, sims[b]) -- the numbers HipMuseProblem gives that simulation's elements, and oracle.normals, bit for bit.  A stream
    as a sequence is e_2i = n1(i), e_2i+1 = n2(i); a request for k values per row returns the next k and starts at a pair boundary:
    the cursor (in pairs, the same for every row) advances by ceil(k / 2), an odd request discards its last n2.

        normals = EngineNormals(device, seed, sims);   e = normals(N, 2)        # e[b, i] = (n1(i), n2(i)) of simulation sims[b]

    Every request is ONE launch for all rows on torch's current stream.  The result is a new float64 tensor and is not differentiable
    (the numbers do not depend on θ).  A GPU only: no CPU fallback."""

    def __init__(self, device, seed, sims):
        import torch
        from . import _capi
        self._torch, self._capi, self._lib = torch, _capi, _capi.load_lbfgs_library()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _capi.MuseError(-3, "no HIP device available (libmuse_lbfgs has no CPU fallback)")
        self.seed = int(seed) % (1 << 64)
        s = sims.detach().cpu().numpy() if torch.is_tensor(sims) else np.asarray(sims)
        s = np.ascontiguousarray(np.atleast_1d(s).astype(np.int64).reshape(-1))
        if s.size < 1 or s.min() < 0:
            raise ValueError("EngineNormals: at least one simulation index, every one non-negative")
        self.sims = torch.as_tensor(s, device=self.device)
        self.B = int(s.size)
        self.cursor = 0          # in pairs

    def normals(self, *shape):
        """[B, *shape] float64: row b holds the next prod(shape) values of stream (seed, sims[b])."""
        torch = self._torch
        shape = tuple(int(k) for k in shape)
        count = int(np.prod(shape, dtype=np.int64))
        if not shape or any(k < 1 for k in shape):
            raise ValueError("EngineNormals: every dimension of a request is at least 1")
        out = torch.empty((self.B,) + shape, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            self._capi.check_lbfgs(self._lib.muse_lbfgs_normals(out.data_ptr(), self.B, count, self.seed, self.sims.data_ptr(), self.cursor,
                                                                torch.cuda.current_stream(self.device).cuda_stream))
        self.cursor += (count + 1) // 2
        return out

    __call__ = normals

    def fresh(self):
        """The same streams from their start: a new object (cursor 0) over the same device tensor of simulation indices."""
        other = object.__new__(EngineNormals)
        other.__dict__.update(self.__dict__)
        other.cursor = 0
        return other


class BatchedTorchMuseProblem(TorchMuseProblem):
    """TorchMuseProblem whose maps run ALL their elements at once: the closure is evaluated once per round for the whole batch -- by
    `logLike_batched(x [B, ...], z [B, ...], theta [B, nθ]) -> [B]` (row b: element b's own θ) or, without it, by torch.func.vmap of
    the per-simulation `logLike` -- and everything between two evaluations (L-BFGS + HagerZhang, optim.lbfgs decision for decision) is
    one launch of libmuse_lbfgs.so's kernel for all elements, one workgroup per element.  The host reads one word per round.

    The driver's batched seams (map_and_score_batch, fd_jacobian_batch, get_zhat / set_zhat, scores_in_both_spaces) follow
    HipMuseProblem's element order and slot rule; draws are the serial class's, bit for bit.  float64 on a GPU only: no CPU fallback.

    With `sample_x_z_batched(normals, theta [B, nθ]) -> (x [B, ...], z [B, ...])` the draws of a map are batched too: `normals` is an
    EngineNormals over the map's rows (`normals(*shape)` -> [B, *shape] standard normals, row b from the engine's stream of row b's
    simulation), row b uses its own θ row as in logLike_batched, and a map draws all its rows in one call -- every request one launch,
    no generator seeded per simulation.  The random numbers are then the ENGINE's: a closure restatement of a header model sees exactly
    HipMuseProblem's simulations.  A sampler must request the same shapes in the same order at every θ (a simulation then keeps its
    random numbers across θ, which the finite-difference and the implicit get_H! rely on), and must be written with differentiable
    torch operations for implicit_H_batch.  `sample_x_z` may then be None: the per-simulation seam sample_x_z(rng, θ) is the batched
    sampler with one row, so a simulation's draw is the same bits alone or in any batch."""
    supports_native_muse = False
    MAX_ROUNDS = 200000
    IMPLICIT_MAX_ELEMS = 1 << 24     # implicit_H_batch: simulations per chunk so that (rows = nsims nθ) x N stays at or below this

    def __init__(self, x, sample_x_z, logLike, logPrior=None, device=None, dtype=None, logLike_batched=None, sample_x_z_batched=None,
                 hess_diag=None):
        if sample_x_z is None and sample_x_z_batched is None:
            raise ValueError("BatchedTorchMuseProblem needs sample_x_z or sample_x_z_batched")
        super().__init__(x, sample_x_z, logLike, logPrior, device, dtype, hess_diag=hess_diag)
        from . import _capi
        if self.device.type != "cuda":
            raise _capi.MuseError(-3, "no HIP device available (BatchedTorchMuseProblem runs libmuse_lbfgs's kernels: there is no CPU fallback)")
        if self.dtype != self._torch.float64:
            raise ValueError("BatchedTorchMuseProblem is float64 only (libmuse_lbfgs's kernels)")
        _capi.load_lbfgs_library()
        self._capi = _capi
        self._batched = logLike_batched
        self._sample_batched = sample_x_z_batched
        self._vmapped = None
        self._batch = None
        self._zhat = None        # [slots, N] on the device: element e's MAP stays at slot e
        self._zshape = None
        self.last_rounds = self.last_syncs = 0
        self._cg_batch = None
        self.cg_timing = False       # implicit_H_batch: sum the device time of the CG advance launches into last_cg_advance_ms
        self.last_cg_rounds = self.last_cg_syncs = self.last_cg_chunks = 0
        self.last_cg_advance_ms = 0.0
        self.last_fiducial_info = None

    # -- the batched closure
    def _logLike_rows(self, x, z, theta):
        if self._batched is not None:
            return self._batched(x, z, theta)
        torch = self._torch
        if self._vmapped is None:
            self._vmapped = torch.func.vmap(self._logLike, in_dims=(0, 0, 0))
        try:
            return self._vmapped(x, z, theta)
        except Exception as e:
            raise ValueError("torch.func.vmap cannot trace this logLike (" + str(e).splitlines()[0] + "): pass `logLike_batched(x [B, ...], "
                             "z [B, ...], theta [B, nθ]) -> [B]` to BatchedTorchMuseProblem") from e

    def _theta_rows(self, theta, n):
        t = self._theta(theta)
        return t.reshape(1, -1).expand(n, -1).contiguous()

    def _solve(self, X, Z0, TH, atol):
        """MAPs of all rows: X [B, ...], Z0 [B, N] (flattened latents), TH [B, nθ] -> (ẑ [B, N], records [B])."""
        torch = self._torch
        B, N = Z0.shape
        if self._batch is None or (self._batch.nprob, self._batch.n) != (B, N):
            self._batch = LbfgsBatch(self.device, B, N)
        batch = self._batch
        batch.begin(Z0.contiguous(), atol)
        while True:
            z = batch.z_eval.view((B,) + self._zshape).detach().requires_grad_(True)
            with torch.enable_grad():
                f = -self._logLike_rows(X, z, TH)
                g, = torch.autograd.grad(f.sum(), z)
            if batch.advance(f.detach().reshape(B), g.reshape(B, N)) == 0:
                break
            if batch.rounds > self.MAX_ROUNDS:
                raise RuntimeError("BatchedTorchMuseProblem: the batch did not end")
        zhat, info = batch.result()
        self.last_rounds, self.last_syncs = batch.rounds, batch.syncs
        return zhat, info

    def _scores(self, X, zhat, TH):
        torch = self._torch
        th = TH.detach().clone().requires_grad_(True)
        with torch.enable_grad():
            f = self._logLike_rows(X, zhat.view((zhat.shape[0],) + self._zshape).detach(), th)
            g, = torch.autograd.grad(f.sum(), th, allow_unused=True)
        return np.zeros(tuple(th.shape)) if g is None else g.detach().cpu().numpy().astype(np.float64)

    # -- the batched sampler: all rows of a map in one call, the engine's streams
    def sample_x_z(self, rng, theta):
        """The per-simulation seam.  With sample_x_z_batched: that sampler with ONE row (the engine's stream (seed, sim)), so a
        simulation's draw is the same bits here and in any batch; without it, the serial class's."""
        if self._sample_batched is None:
            return super().sample_x_z(rng, theta)
        rng = rng if isinstance(rng, SimRng) else SimRng(int(rng), 0)
        X, Z = self._draw_rows(EngineNormals(self.device, rng.seed, [rng.sim]), self._theta(theta).reshape(1, -1))
        return X[0], Z[0]

    def _draw_rows(self, normals, TH):
        """(x [B, ...], z [B, ...]) of the batched sampler: row b is simulation normals.sims[b] at TH[b].  Differentiable in TH where TH
        requires grad (and the sampler is written so); otherwise plain tensors."""
        torch = self._torch
        with torch.set_grad_enabled(bool(TH.requires_grad)):
            x, z = self._sample_batched(normals, TH)
        B = normals.B
        if not (torch.is_tensor(x) and torch.is_tensor(z) and x.shape[:1] == (B,) and z.shape[:1] == (B,)):
            raise ValueError(f"sample_x_z_batched must return (x [B, ...], z [B, ...]) with B = {B} rows")
        x, z = x.to(self.device, self.dtype), z.to(self.device, self.dtype)
        if self._zshape is None:
            self._zshape = tuple(z.shape[1:])
        return x, z

    def _draw_sims(self, seed, sims, TH):
        """_draw_rows over fresh streams of `sims` (one per row of TH)."""
        return self._draw_rows(EngineNormals(self.device, seed, sims), TH)

    def _theta_rows_of(self, rows):
        """[R, nθ] on the device from a numpy array of θ rows"""
        return self._torch.as_tensor(np.ascontiguousarray(rows, dtype=np.float64), device=self.device).to(self.dtype)

    def _draw(self, rng, sim, theta):
        x, z = self.sample_x_z(SimRng(int(rng), int(sim)), theta)
        if self._zshape is None:
            self._zshape = tuple(z.shape)
        return x, z

    def _latent_shape(self, rng, theta):
        if self._zshape is None:
            self._draw(rng, 0, theta)
        return self._zshape

    def _slots(self, n, N):
        torch = self._torch
        if self._zhat is None or self._zhat.shape[1] != N:
            self._zhat = torch.zeros((n, N), dtype=self.dtype, device=self.device)
        elif self._zhat.shape[0] < n:
            self._zhat = torch.cat([self._zhat, torch.zeros((n - self._zhat.shape[0], N), dtype=self.dtype, device=self.device)])
        return self._zhat

    # -- the seams muse.py looks for
    def map_and_score_batch(self, rng, sim_begin, sim_end, theta, *, include_data=False, atol=1e-2, z0_mode=0):
        """All elements of one muse!/get_J! map at once.  Returns (g [n, nθ], info [n]); element order: [data], sim_begin .. sim_end-1;
        ẑ of element e stays resident (on the device) at slot e."""
        torch, capi = self._torch, self._capi
        rng = int(rng.seed) if isinstance(rng, SimRng) else int(rng)
        xs, zs = [], []
        zshape = self._latent_shape(rng, theta)
        if include_data:
            if self.x is None:
                raise ValueError("include_data needs the problem's x")
            xs.append(self.x)
            zs.append(None)
        sims = range(int(sim_begin), int(sim_end))
        if self._sample_batched is not None and len(sims) > 0:          # every simulation's draw in one call
            Xs, Zs = self._draw_sims(rng, list(sims), self._theta_rows(theta, len(sims)))
            xs.extend(Xs.unbind(0))
            zs.extend(Zs.unbind(0))
        else:
            for s in sims:
                x, z = self._draw(rng, s, theta)
                xs.append(x)
                zs.append(z)
        n, N = len(xs), int(np.prod(zshape, dtype=np.int64))
        X = torch.stack(xs)
        if z0_mode == capi.Z0_WARM:
            if self._zhat is None or self._zhat.shape[0] < n or self._zhat.shape[1] != N:
                raise ValueError("Z0_WARM needs resident MAPs for every element (an earlier map, or set_zhat)")
            Z0 = self._zhat[:n].clone()
        elif z0_mode == capi.Z0_TRUE:
            Z0 = torch.stack([torch.zeros(zshape, dtype=self.dtype, device=self.device) if z is None else z for z in zs]).reshape(n, N)
        else:
            Z0 = torch.zeros((n, N), dtype=self.dtype, device=self.device)
        TH = self._theta_rows(theta, n)
        zhat, info = self._solve(X, Z0, TH, atol)
        self._slots(n, N)[:n] = zhat
        return self._scores(X, zhat, TH), info

    def scores_in_both_spaces(self, g, theta, theta_t):
        """(g, g′): the transformed-space score by the chain rule through the transform, as grad_theta_logLike takes it."""
        J = self._jac_inv_transform(np.atleast_1d(np.asarray(theta_t, dtype=np.float64)))
        return g, g @ J

    def get_zhat(self, slot_begin, slot_end):
        if self._zhat is None or slot_end > self._zhat.shape[0]:
            raise ValueError("no resident MAP at these slots")
        return self._zhat[slot_begin:slot_end].cpu().numpy().astype(np.float64)

    def set_zhat(self, slot_begin, zs):
        zs = self._t(zs)
        zs = zs.reshape(zs.shape[0], -1) if zs.dim() > 1 else zs.reshape(1, -1)
        self._slots(slot_begin + zs.shape[0], zs.shape[1])[slot_begin:slot_begin + zs.shape[0]] = zs

    def fd_jacobian_batch(self, rng, sim_begin, sim_end, theta0, step, *, atol=1e-2, fid_mode=0, fid_sim=None):
        """get_H! by finite differences for sims [sim_begin, sim_end) (muse._fd_serial's map; include/muse_hip.h, muse_fd_jacobian_batch):
        the fiducial MAP(s) first, then all 2 nθ nsims perturbed solves as ONE batch.  Returns (Hs [nsims, nθ, nθ],
        info [nsims, nθ, 2]: last index 0 = plus, 1 = minus)."""
        torch = self._torch
        from .problem import MASTER_SIM
        rng = int(rng.seed) if isinstance(rng, SimRng) else int(rng)
        fid_sim = MASTER_SIM if fid_sim is None else int(fid_sim)
        theta0 = np.atleast_1d(np.asarray(theta0, dtype=np.float64))
        step = np.broadcast_to(np.atleast_1d(np.asarray(step, dtype=np.float64)), theta0.shape)
        nth, sims = theta0.size, list(range(int(sim_begin), int(sim_end)))
        zshape = self._latent_shape(rng, theta0)
        N = int(np.prod(zshape, dtype=np.int64))
        fids = [fid_sim] if fid_mode == 0 else sims
        if self._sample_batched is not None:
            Xf = self._draw_sims(rng, fids, self._theta_rows(theta0, len(fids)))[0]
        else:
            Xf = torch.stack([self._draw(rng, s, theta0)[0] for s in fids])
        zfid, _ = self._solve(Xf, torch.zeros((len(fids), N), dtype=self.dtype, device=self.device), self._theta_rows(theta0, len(fids)), atol)
        if self._sample_batched is not None:
            # all 2 nθ nsims perturbed draws in one call: row (k, j, sign) is simulation sims[k] at θ0 ± step_j e_j
            thp = np.tile(theta0, (len(sims), nth, 2, 1))
            for j in range(nth):
                thp[:, j, 0, j] = theta0[j] + step[j]
                thp[:, j, 1, j] = theta0[j] - step[j]
            X = self._draw_sims(rng, np.repeat(np.asarray(sims, dtype=np.int64), 2 * nth), self._theta_rows_of(thp.reshape(-1, nth)))[0]
            Z0 = (zfid[:1].expand(X.shape[0], N) if fid_mode == 0 else zfid.repeat_interleave(2 * nth, dim=0)).contiguous()
        else:
            xs, z0 = [], []
            for k, s in enumerate(sims):
                for j in range(nth):
                    for sign in (1.0, -1.0):
                        th = theta0.copy()
                        th[j] = theta0[j] + sign * step[j]
                        xs.append(self._draw(rng, s, th)[0])
                        z0.append(zfid[0 if fid_mode == 0 else k])
            X, Z0 = torch.stack(xs), torch.stack(z0)
        TH = self._theta_rows(theta0, X.shape[0])
        zhat, info = self._solve(X, Z0, TH, atol)
        g = self._scores(X, zhat, TH).reshape(len(sims), nth, 2, nth)          # [sim, column j, plus / minus, component i]
        cols = (-0.5 * g[:, :, 1, :] + 0.5 * g[:, :, 0, :]) / step[None, :, None]
        return np.ascontiguousarray(np.swapaxes(cols, 1, 2)), info.reshape(len(sims), nth, 2)

    # -- get_H! by implicit differentiation, all simulations at once
    def implicit_H_batch(self, seed, sim_begin, sim_end, theta0, atol=1e-1, cg_maxiter=100, cg_reltol=1.4901161193847656e-08, cg_abstol=0.0,
                         H1_is_zero=False, cg_Pl=None):
        """The serial class's implicit_H_batch (H = H1 - dFdθᵀ A⁻¹ dFdθ1 per simulation, see there) with every step taken for all
        simulations at once: the fiducial MAPs are one lock-step L-BFGS batch, the derivative terms one autograd pass per θ component
        over the whole batch, and the nsims nθ linear solves one lock-step conjugate-gradient batch of libmuse_lbfgs.so (CgBatch: one
        workgroup per (simulation, column), the operator one double backward of the batched closure per round, one word read per round).
        cg_abstol and H1_is_zero are IterativeSolvers' abstol and the reference's implicit_diff_H1_is_zero.  Simulations are taken in
        chunks of at most IMPLICIT_MAX_ELEMS / (nθ N); rows are independent.

        cg_Pl="jacobi" (implicit_diff_cg_kwargs' Pl) preconditions every solve with the diagonal of -∂²logLike/∂z² at its simulation's
        fiducial MAP, as the constructor's hess_diag describes it (given by a callable, or probed by Hessian-vector products over the
        simulations): one [nsims, N] diagonal shared by a simulation's nθ rows, applied inside the CG kernel.  Every round is a double
        backward pass, a launch and a synchronisation, so the number of rounds is the cost of the call and the diagonal the lever on
        it.  Correctness never rests on the diagonal's quality: any positive one gives the same H to the tolerance and only the counts
        move; one that is not positive (or not finite) gives that simulation's rows the count -1.  Without hess_diag "jacobi" is a
        ValueError, raised before any draw or launch; a general (non-diagonal) preconditioner is not supported.

        Returns (Hs [n, nθ, nθ], CG counts [n, nθ]: negative, -1 - iterations, where p.Ap was not positive -- the Hessian in z is not
        negative definite at that fiducial MAP -- or the diagonal was not usable)."""
        jacobi = self._checked_cg_Pl(cg_Pl, self._hess_diag)
        seed = int(seed.seed) if isinstance(seed, SimRng) else int(seed)
        theta0 = np.atleast_1d(np.asarray(theta0, dtype=np.float64))
        sims = list(range(int(sim_begin), int(sim_end)))
        nt = theta0.size
        N = int(np.prod(self._latent_shape(seed, theta0), dtype=np.int64))
        per = max(1, int(self.IMPLICIT_MAX_ELEMS) // max(1, nt * N))
        self.last_cg_rounds = self.last_cg_syncs = self.last_cg_chunks = 0
        self.last_cg_advance_ms = 0.0
        Hs, its, infos = [], [], []
        for c in range(0, len(sims), per):
            H, k, info = self._implicit_chunk(seed, sims[c:c + per], theta0, atol, cg_maxiter, cg_reltol, cg_abstol, H1_is_zero, jacobi)
            Hs.append(H)
            its.append(k)
            infos.append(info)
        self.last_fiducial_info = np.concatenate(infos) if infos else None
        if not Hs:
            return np.zeros((0, nt, nt)), np.zeros((0, nt), dtype=np.int32)
        return np.concatenate(Hs), np.concatenate(its)

    def _implicit_chunk(self, seed, sims, theta0, atol, cg_maxiter, cg_reltol, cg_abstol, H1_is_zero, jacobi=False):
        torch = self._torch
        S, nt = len(sims), theta0.size
        TH = self._theta_rows(theta0, S)
        if self._sample_batched is not None:
            normals = EngineNormals(self.device, seed, sims)
            X = self._draw_rows(normals, TH)[0]                          # every simulation's draw in one call
        else:
            X = torch.stack([self._draw(seed, s, theta0)[0] for s in sims])          # the serial class's draws, bit for bit
        zshape = self._zshape
        N = int(np.prod(zshape, dtype=np.int64))
        zhat, info = self._solve(X, torch.zeros((S, N), dtype=self.dtype, device=self.device), TH, atol)     # (zhat_guess_from_truth: zeros)
        zhat = zhat.detach()
        R = S * nt
        with torch.enable_grad():
            # the draws again, as functions of each simulation's own θ (the generator re-seeded: the same random numbers)
            th_draw = TH.clone().requires_grad_(True)
            xg = []
            if self._sample_batched is not None:
                Xg = self._draw_rows(normals.fresh(), th_draw)[0]       # (the streams from their start: the same numbers, in one call)
            else:
                for i, s in enumerate(sims):
                    gen = torch.Generator(device=self.device)
                    gen.manual_seed(self._stream(SimRng(seed, s)))
                    xg.append(self._sample(gen, th_draw[i])[0].to(self.dtype))
                Xg = torch.stack(xg)
            zfix = zhat.view((S,) + zshape)
            # H1[s, i, j] = ∂/∂θ_j of the score's component i through the draw: nθ backward passes, each over every simulation
            H1 = torch.zeros((S, nt, nt), dtype=self.dtype, device=self.device)
            if not H1_is_zero and Xg.requires_grad:
                th_score = TH.clone().requires_grad_(True)
                score, = torch.autograd.grad(self._logLike_rows(Xg, zfix, th_score).sum(), th_score, create_graph=True, allow_unused=True)
                if score is not None and score.requires_grad:
                    for i in range(nt):
                        row, = torch.autograd.grad(score[:, i].sum(), th_draw, retain_graph=True, allow_unused=True)
                        if row is not None:
                            H1[:, i, :] = row
            # dFdθ1 = ∂θ ∇z logLike(x(θ), ẑ, θ0), column by column in forward mode (the double-backward identity: w = Jᵀ v is linear in v,
            # so ∂(w_j)/∂v = J e_j): nθ passes over every simulation, never one per latent component
            b = torch.zeros((S, nt, N), dtype=self.dtype, device=self.device)
            if Xg.requires_grad:
                zz = zfix.clone().requires_grad_(True)
                gz, = torch.autograd.grad(self._logLike_rows(Xg, zz, TH).sum(), zz, create_graph=True)
                if gz.requires_grad:
                    v = torch.zeros_like(gz).requires_grad_(True)
                    w, = torch.autograd.grad(gz, th_draw, grad_outputs=v, create_graph=True, allow_unused=True)
                    if w is not None and w.requires_grad:
                        for j in range(nt):
                            col, = torch.autograd.grad(w[:, j].sum(), v, retain_graph=True, allow_unused=True)
                            if col is not None:
                                b[:, j, :] = -col.reshape(S, N)
            del xg, Xg
            # the R = S nθ systems (-A) y = b: row (s, j) sees simulation s's x and ẑ, so one double backward of the batched closure is
            # every row's own Hessian-vector product
            XR, THR = X.repeat_interleave(nt, dim=0), self._theta_rows(theta0, R)
            ZR = zhat.repeat_interleave(nt, dim=0).view((R,) + zshape).clone().requires_grad_(True)
            g, = torch.autograd.grad(self._logLike_rows(XR, ZR, THR).sum(), ZR, create_graph=True)
            if self._cg_batch is None or (self._cg_batch.nrows, self._cg_batch.n) != (R, N):
                self._cg_batch = CgBatch(self.device, R, N)
            cg = self._cg_batch
            cg.timing = self.cg_timing
            if jacobi:
                # the diagonal at the S fiducial MAPs, [S, N]: row (s, j) of the batch reads diagonal row s
                ZS = zfix.clone().requires_grad_(True)
                gS, = torch.autograd.grad(self._logLike_rows(X, ZS, TH).sum(), ZS, create_graph=True)
                diag = self._hess_diagonal(X, zfix, TH, lambda V: -torch.autograd.grad(gS, ZS, V, retain_graph=True)[0])
                del gS, ZS
                active = cg.begin(b.reshape(R, N), cg_reltol, cg_abstol, cg_maxiter, diag=diag, rows_per_diag=nt)
            else:
                active = cg.begin(b.reshape(R, N), cg_reltol, cg_abstol, cg_maxiter)
            while active > 0:
                Ap, = torch.autograd.grad(g, ZR, cg.p_eval.view_as(g), retain_graph=True)
                active = cg.advance(-Ap.reshape(R, N))
                if cg.rounds > max(int(cg_maxiter), 0):
                    raise RuntimeError("BatchedTorchMuseProblem: the conjugate-gradient batch did not end")
            Y, counts, _ = cg.result()
            del g
            # H2 = -dFdθᵀ Y without forming dFdθ: one backward pass with respect to every row's own θ
            thR = THR.clone().requires_grad_(True)
            z2 = ZR.detach().requires_grad_(True)
            gz2, = torch.autograd.grad(self._logLike_rows(XR, z2, thR).sum(), z2, create_graph=True)
            dth, = torch.autograd.grad((gz2.reshape(R, N) * Y).sum(), thR, allow_unused=True)
        H = H1
        if dth is not None:
            H = H1 - dth.reshape(S, nt, nt).transpose(1, 2)        # dth[(s, j), i] = (dFdθᵀ y_sj)_i = H2[s, i, j]
        self.last_cg_rounds += cg.rounds
        self.last_cg_syncs += cg.syncs
        self.last_cg_chunks += 1
        self.last_cg_advance_ms += cg.advance_ms
        return H.detach().cpu().numpy().astype(np.float64), counts.reshape(S, nt).astype(np.int32), info


def _cg(A, b, maxiter, reltol):
    """Conjugate gradients for A y = b from y = 0 (A symmetric positive definite, given as a function): (y, iterations); stops at
    |r| <= reltol |b| or after maxiter iterations."""
    y = b.new_zeros(b.shape)
    r = b.clone()
    p = r.clone()
    rs = float(r.dot(r))
    stop = (reltol ** 2) * rs
    k = 0
    while k < maxiter and rs > stop and rs > 0.0:
        Ap = A(p)
        alpha = rs / float(p.dot(Ap))
        y = y + alpha * p
        r = r - alpha * Ap
        rs_new = float(r.dot(r))
        p = r + (rs_new / rs) * p
        rs = rs_new
        k += 1
    return y, k


def _pcg(A, b, d, maxiter, reltol, abstol=0.0):
    """Conjugate gradients for A y = b from y = 0 preconditioned by Diagonal(d) (IterativeSolvers' cg with Pl; the serial statement of
    lbfgs/pcg_control.hpp, decision for decision): (y, count).  Stops at |r| <= max(reltol |b|, abstol) or after maxiter iterations; the
    count is -1 - iterations where the guard stopped the solve with y as it was -- p.Ap not positive or not finite, or (before the
    first iteration) an entry of d that is not positive or not finite.  Any positive d gives the same solution to the tolerance."""
    import math
    y = b.new_zeros(b.shape)
    r = b.clone()
    rr = float(r.dot(r))
    tol = max(reltol * math.sqrt(rr), abstol)
    if maxiter <= 0 or math.sqrt(rr) <= tol:
        return y, 0
    if not bool(((d > 0) & ~d.isinf()).all()):
        return y, -1
    p = r / d
    rho = float(p.dot(r))
    k = 0
    while True:
        Ap = A(p)
        pAp = float(p.dot(Ap))
        if not (pAp > 0.0) or math.isinf(pAp):
            return y, -1 - k
        alpha = rho / pAp
        y = y + alpha * p
        r = r - alpha * Ap
        c = r / d
        rr, rho_new = float(r.dot(r)), float(c.dot(r))
        k += 1
        if k == maxiter or math.sqrt(rr) <= tol:
            return y, k
        p = c + (rho_new / rho) * p
        rho = rho_new


def _fd_grad(f, t, step=1e-6):
    g = np.zeros(t.size)
    for j in range(t.size):
        e = np.zeros(t.size)
        e[j] = step
        g[j] = (f(t + e) - f(t - e)) / (2 * step)
    return g


def _info_dtype():
    from . import _capi
    return _capi.INFO_DTYPE
