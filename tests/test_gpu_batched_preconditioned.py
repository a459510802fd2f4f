"""BatchedTorchMuseProblem.implicit_H_batch(cg_Pl="jacobi") on the GPU -- the lock-step CG batch preconditioned by the diagonal the
constructor's hess_diag describes (CgBatch with diag, rows_per_diag = nθ) -- on the two models of tests/test_closure_preconditioner.py,
against the serial TorchMuseProblem under the same cg_Pl on the same device: equal counts, equal fiducial records, Hs within ten
times what the serial path itself moves between a CPU and a GPU run; against the unpreconditioned H at cg_reltol = 1e-12; chunking,
the engine-streams sampler, and the driver's keywords."""
import numpy as np
import pytest
import torch

from test_closure_preconditioner import HETERO, SCALED, hetero_closures, hetero_sigma, scaled_dense_closures
from test_gpu_batched_closures import same_counts

DEV = "cuda"
# The scaled dense model's seed and MAP tolerance.  The seed is the first of 0, 1, 2, ... for which the SERIAL class agrees with itself in a
# CPU run, a GPU run and a GPU run with the latents permuted (pick_dense_seed() below prints the rows per seed), in its CG counts under
# cg_Pl="jacobi" -- a count decided by |r| <= sqrt(eps) |b| in the last iteration can move by one with the order of the sums -- and in
# its fiducial MAPs' records, which the test below compares too.  On an MI355X the counts of seed 0 were [17 18 18 18] three times at
# every MAP tolerance (seeds 1 - 4 [18 18 18 18], seed 5 [17 18 18 17]).  The records, however, are no property of this model at a tight
# tolerance: with the MAPs solved to 1e-8 (28 L-BFGS iterations, about 80 evaluations on these badly scaled latents) the serial
# class's own f_calls differed between its three runs for EVERY seed 0 - 7 (seed 0: cpu 82 82 84 84, gpu 79 82 84 85, permuted
# 79 83 84 83).  At 1e-1 -- the tolerance get_H! itself solves its fiducial MAPs to (src/muse.jl:344) -- the three runs agree for each of
# the seeds 0 - 3 (seed 0: 13 37, 13 38, 12 35, 12 36 iterations and f_calls, three times); at 1e-3 for seeds 0, 2, 3.  So this file
# runs the scaled model at the driver's own tolerance.  The Hessian does not depend on z (the model is quadratic), so neither do the
# operator nor the diagonal.
DENSE_SEED, DENSE_ATOL = SCALED["seed"], 1e-1
CONSTANTS = {"hetero": HETERO, "scaled": dict(SCALED, seed=DENSE_SEED, atol=DENSE_ATOL)}
# How far the SERIAL class's Hs under cg_Pl="jacobi" move between a run on the CPU and a run on the GPU with the same (host) draws,
# max |dH|: measure_serial_H_between_devices() below, on an MI355X (the same value in two runs): hetero 1.08e-13 (|H| up to 10.8), scaled
# 1.52e-12 (|H| up to 6.0).
SERIAL_PCG_H_MOVES = {"hetero": 1.0835776720341528e-13, "scaled": 1.5196732761069143e-12}
# How far the SERIAL class's H at cg_reltol = 1e-12 moves between cg_Pl="jacobi" and plain CG, max |dH| on the CPU
# (measure_serial_H_between_preconditioners() below); the tests allow ten times that for the order of the sums.  Measured on the host
# of an MI355X: hetero 6.87e-12, scaled 3.84e-12 (the same call on the GPU: 6.85e-12 and 1.40e-12).
SERIAL_PL_H_MOVES = {"hetero": 6.8691718979607685e-12, "scaled": 3.841815754412892e-12}


def closures(M, model, device, perm=None):
    """(sample_x_z, logLike, hess_diag callable)"""
    if model == "hetero":
        return hetero_closures(HETERO["N"], device)[:3]
    return scaled_dense_closures(M, device, perm=perm)[:3]


def serial_implicit(M, model, device, perm=None, seed=None, jacobi=True, atol=None, **kw):
    sample_x_z, logLike, hd = closures(M, model, device, perm)
    c = dict(CONSTANTS[model], **({} if atol is None else {"atol": atol}))
    prob = M.TorchMuseProblem(None, sample_x_z, logLike, device=device, hess_diag=hd)
    return prob.implicit_H_batch(c["seed"] if seed is None else seed, 0, c["nsims"], c["theta0"], atol=c["atol"], cg_Pl="jacobi" if jacobi else None, **kw)


def measure_serial_H_between_devices(M, model):
    return float(np.abs(serial_implicit(M, model, "cpu")[0] - serial_implicit(M, model, DEV)[0]).max())


def measure_serial_H_between_preconditioners(M, model, device="cpu"):
    return float(np.abs(serial_implicit(M, model, device, cg_reltol=1e-12)[0] - serial_implicit(M, model, device, jacobi=False, cg_reltol=1e-12)[0]).max())


def serial_fiducial_records(M, model, device, perm=None, seed=None, atol=None):
    """The serial class's fiducial MAPs, one record per simulation"""
    sample_x_z, logLike, hd = closures(M, model, device, perm)
    c = dict(CONSTANTS[model], **({} if atol is None else {"atol": atol}))
    serial = M.TorchMuseProblem(None, sample_x_z, logLike, device=device)
    infos = []
    for s in range(c["nsims"]):
        x, z = serial.sample_x_z(M.SimRng(c["seed"] if seed is None else seed, s), c["theta0"])
        infos.append(serial.zhat_at_theta(x, torch.zeros_like(z), c["theta0"], c["atol"])[1])
    return infos


def pick_dense_seed(M, seeds=range(6), atol=None):
    """Per seed: the serial CG counts under cg_Pl="jacobi", and the serial fiducial MAPs' (iterations, f_calls), on the CPU, on the GPU and
    on the GPU with the latents permuted.  A seed qualifies when all three runs of the serial class agree in both."""
    perm = torch.as_tensor(np.random.RandomState(5).permutation(SCALED["n"]))
    for seed in seeds:
        runs = [("cpu", None), (DEV, None), (DEV, perm)]
        rows = [serial_implicit(M, "scaled", d, perm=p, seed=seed, atol=atol)[1].ravel() for d, p in runs]
        recs = [np.array([(int(i["iterations"]), int(i["f_calls"]), int(i["status"])) for i in serial_fiducial_records(M, "scaled", d, p, seed, atol)]).ravel()
                for d, p in runs]
        print("seed", seed, "cpu", rows[0], "gpu", rows[1], "gpu permuted", rows[2], "counts agree", all(np.array_equal(rows[0], r) for r in rows))
        print("seed", seed, "fiducial (iterations, f_calls, status) cpu", recs[0], "gpu", recs[1], "gpu permuted", recs[2], "records agree",
              all(np.array_equal(recs[0], r) for r in recs), flush=True)


_serial = {}


def serial_reference(M, model):
    """The serial class on the GPU under cg_Pl="jacobi", once per model: (Hs, counts)"""
    if model not in _serial:
        _serial[model] = serial_implicit(M, model, DEV)
    return _serial[model]


def batched(M, model, hess_diag="callable"):
    sample_x_z, logLike, hd = closures(M, model, DEV)
    kind = hd if hess_diag == "callable" else hess_diag
    return M.BatchedTorchMuseProblem(None, sample_x_z, logLike, device=DEV, hess_diag=kind), CONSTANTS[model]


def run(prob, c, **kw):
    return prob.implicit_H_batch(c["seed"], 0, c["nsims"], c["theta0"], atol=c["atol"], **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["hetero", "scaled"])
def test_preconditioned_implicit_H_batch_equals_the_serial_class(M, gpu, model):
    """Tolerance: ten times SERIAL_PCG_H_MOVES[model], the distance between two runs of the serial path itself."""
    prob, c = batched(M, model)
    infos = serial_fiducial_records(M, model, DEV)
    Hs, its = run(prob, c, cg_Pl="jacobi")
    rounds, syncs = prob.last_cg_rounds, prob.last_cg_syncs
    ref, ref_its = serial_reference(M, model)
    H0, its0 = run(prob, c)
    nth = c["theta0"].size
    print(model, "max |dH| batched - serial", float(np.abs(Hs - ref).max()), "|H|", float(np.abs(ref).max()), "counts", its.ravel(), "serial",
          ref_its.ravel(), "plain", its0.ravel(), "rounds", rounds, "syncs", syncs, "plain rounds", prob.last_cg_rounds)
    assert Hs.shape == (c["nsims"], nth, nth) and its.shape == (c["nsims"], nth) and its.dtype == np.int32
    same_counts(prob.last_fiducial_info, infos)
    assert np.array_equal(its, ref_its)
    assert np.all(its == 1) if model == "hetero" else (np.all(its > 0) and np.all(its < its0))
    assert rounds == its.max() and syncs == rounds + 2 and rounds < prob.last_cg_rounds
    np.testing.assert_allclose(Hs, ref, rtol=0, atol=10 * SERIAL_PCG_H_MOVES[model])


@pytest.mark.gpu
@pytest.mark.parametrize("model,hess_diag", [("hetero", "callable"), ("hetero", "elementwise"), ("scaled", "callable"), ("scaled", "probes")])
def test_preconditioned_H_equals_the_plain_H_at_a_tight_tolerance(M, gpu, model, hess_diag):
    """Any positive diagonal gives the same H to the tolerance: at cg_reltol = 1e-12 within ten times what the serial class's own two
    Hs differ by on the CPU (SERIAL_PL_H_MOVES)."""
    kind = torch.eye(SCALED["n"], dtype=torch.float64) if hess_diag == "probes" else hess_diag
    prob, c = batched(M, model, kind)
    Hj, kj = run(prob, c, cg_reltol=1e-12, cg_Pl="jacobi")
    Hp, kp = run(prob, c, cg_reltol=1e-12)
    print(model, hess_diag, "counts", kj.ravel(), "plain", kp.ravel(), "max |dH|", float(np.abs(Hj - Hp).max()), "|H|", float(np.abs(Hp).max()))
    assert np.all(kj > 0) and np.all(kj < kp)
    np.testing.assert_allclose(Hj, Hp, rtol=0, atol=10 * SERIAL_PL_H_MOVES[model])


@pytest.mark.gpu
def test_chunks_of_one_simulation_give_the_same_bits(M, gpu):
    """Rows are independent and so are the rows of the diagonal: on the elementwise model (vmap: elementwise with per-row sums) the
    chunking changes nothing."""
    for kind in ("callable", "elementwise"):
        prob, c = batched(M, "hetero", kind)
        Hs, its = run(prob, c, cg_Pl="jacobi")
        prob.IMPLICIT_MAX_ELEMS = c["N"] * c["theta0"].size
        Hc, itc = run(prob, c, cg_Pl="jacobi")
        assert prob.last_cg_chunks == c["nsims"] and prob.last_cg_syncs == prob.last_cg_rounds + 2 * prob.last_cg_chunks
        assert np.array_equal(Hs, Hc) and np.array_equal(its, itc)


@pytest.mark.gpu
def test_the_engine_streams_sampler_works_with_the_preconditioner(M, gpu):
    c, N = HETERO, HETERO["N"]
    sig = hetero_sigma(N, DEV)
    _, logLike, hd = closures(M, "hetero", DEV)

    def sample_x_z_batched(normals, theta):
        e = normals(N, 2)
        z = torch.exp(theta[:, 0:1] / 2) * e[..., 0]
        return z + sig * torch.exp(theta[:, 1:2] / 2) * e[..., 1], z
    prob = M.BatchedTorchMuseProblem(None, None, logLike, device=DEV, sample_x_z_batched=sample_x_z_batched, hess_diag="elementwise")
    Hj, kj = run(prob, c, cg_reltol=1e-12, cg_Pl="jacobi")
    Hp, kp = run(prob, c, cg_reltol=1e-12)
    print("engine streams: counts", kj.ravel(), "plain", kp.ravel(), "max |dH|", float(np.abs(Hj - Hp).max()))
    assert np.all(kj == 1) and np.all(kp > 1)
    np.testing.assert_allclose(Hj, Hp, rtol=0, atol=10 * SERIAL_PL_H_MOVES["hetero"])


@pytest.mark.gpu
def test_the_driver_reaches_the_seam_with_Pl(M, gpu):
    prob, c = batched(M, "scaled")
    nth = c["theta0"].size

    def get_H(p, **kw):
        res = M.MuseResult()
        res.theta = c["theta0"]
        M.get_H_(res, p, rng=c["seed"], nsims=c["nsims"], implicit_diff=True, **kw)
        return res
    full, its = prob.implicit_H_batch(c["seed"], 0, c["nsims"], c["theta0"], cg_Pl="jacobi")
    res = get_H(prob, implicit_diff_cg_kwargs={"Pl": "jacobi"})
    hists = np.array(res.metadata["implicit_diff_cg_hists"])
    assert hists.shape == (c["nsims"], nth) and np.array_equal(hists, its)
    np.testing.assert_array_equal(res.H, full.mean(axis=0))
    res3 = get_H(prob, implicit_diff_H1_is_zero=True, implicit_diff_cg_kwargs={"Pl": "jacobi", "maxiter": 3, "reltol": 1e-12})
    assert np.all(np.array(res3.metadata["implicit_diff_cg_hists"]) == 3)
    # a diagonal that is not positive: reported through the count, an error of the driver's
    sample_x_z, logLike, hd = closures(M, "scaled", DEV)
    bad = M.BatchedTorchMuseProblem(None, sample_x_z, logLike, device=DEV, hess_diag=lambda x, z, th: -hd(x, z, th))
    assert np.all(run(bad, c, cg_Pl="jacobi")[1] == -1) and bad.last_cg_rounds == 0
    with pytest.raises(M.MuseError):
        get_H(bad, implicit_diff_cg_kwargs={"Pl": "jacobi"})
    # a problem built without hess_diag refuses, before any draw or launch
    plain = M.BatchedTorchMuseProblem(None, sample_x_z, logLike, device=DEV)
    with pytest.raises(ValueError, match="hess_diag"):
        get_H(plain, implicit_diff_cg_kwargs={"Pl": "jacobi"})
