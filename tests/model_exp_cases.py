"""The arguments the exponentials are compared on (tests/test_model_exp_host.py, tests/test_gpu_model_exp.py): the set of
tests/test_muse_exp.py -- uniform and near-zero samples, every boundary at which k changes +- 2 ulp, both cut-offs +- 3, the
k = 1024 and k = -1022 bands, the subnormal results -- and the special arguments +-0, +-inf, NaN."""
import numpy as np

LD = np.longdouble
HI_CUT, LO_CUT = 7.09782712893383973096e+02, -7.45133219101941108420e+02     # the source's cut-offs
LN2 = np.log(LD(2))


def _neighbours(v, n=2):
    out = [np.asarray(v, np.float64)]
    for d in (-np.inf, np.inf):
        w = out[0]
        for _ in range(n):
            w = np.nextafter(w, d)
            out.append(w)
    return np.concatenate([np.atleast_1d(o) for o in out])


def arguments():
    rng = np.random.default_rng(20240)
    m = np.arange(-1076, 1026)
    edges = np.concatenate([((m + s) * LN2).astype(np.float64) for s in (LD(0.5), LD(-0.5))])     # where k changes
    return np.concatenate([
        rng.uniform(-745.2, 709.8, 50_000), rng.uniform(-2.0, 2.0, 30_000), rng.normal(0.0, 1e-3, 10_000),
        rng.uniform(-1.0, 1.0, 5_000) * 2.0 ** rng.integers(-1074, -10, 5_000).astype(np.float64),       # dense around 0, down to subnormals
        _neighbours(edges), _neighbours([HI_CUT, LO_CUT], 3),
        rng.uniform(-745.2, -708.3, 10_000),                                                             # subnormal results
        rng.uniform(709.44, HI_CUT, 2_000), _neighbours([709.5, 709.7]),                                 # k = 1024
        rng.uniform(-708.75, -708.05, 2_000), _neighbours([-708.4]),                                     # k = -1022
        _neighbours([0.0, -0.0, 1.0, -1.0, 0.5 * float(LN2), -0.5 * float(LN2)]),
        np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e300, -1e300, 5e-324, -5e-324])])


def same_bits(a, b):
    """Elementwise: equal as bit patterns, NaN comparing as NaN."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
