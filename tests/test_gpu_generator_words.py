"""-m gpu: the generator's word arithmetic (csrc/rng.hpp) at every place the engine calls it, against the oracle's draw.

The Philox round mixes its words with the three-input bitwise operation of gfx950 (rng.hpp, xor3), and the quadrant signs of
sin / cos (pi t) are an xor into the sign bit (xor_andn).  Both are integer identities, so every draw must be the oracle's
(oracle/muse_oracle.c, the independent C restatement of Philox + Box-Muller) bit for bit:

* the operands of the three-input op are the counter words (element low / high, simulation low / high) and the key words (seed
  low / high): simulations 0, 1, 2^32 - 1, 2^32, 2^40 + 7 (a nonzero high counter word) under seeds with only the low word, only
  the high word, and both, through sample_x_z at N = 1, 2, 129, 1025;
* every call site of the generator at the smallest N that reaches it: the register placements (N <= 512 and 512 < N <= 4096), the
  LDS-resident placement (N = 4098: even, so the pad pair is live, and not a multiple of the 1024 elements a trip of the
  workgroup covers), the streaming placement forced on the same sizes, the resident and the streaming clusters (an element split
  of 2; the streaming one draws the next problem in the background), the normals cache (store, then load) and normals_kernel
  (a finite-difference call after a cached map).  A map does not return its draw, so a call site is held three ways: the context's
  own sample_x_z is the oracle's bit for bit, the map's scores and solver records are the oracle's at the suite's stated
  tolerances (equal counts, scores rtol 1e-10, MAPs 1e-9: tests/test_gpu_parity.py), and placements that reduce in the same order
  (everything but the element splits) return the same bits;
* the start modes of the LDS-resident placement: its sampler stages the simulation's true z in the g area only for the start that
  reads it back (solver.hpp, begin).  Z0_ZERO and Z0_TRUE maps and an implicit-H call against the oracle, and a Z0_TRUE map directly
  after a Z0_ZERO map on the same context against a fresh context's, bit for bit, with more problems than workgroups (a workgroup
  that goes on to a second problem finds the first one's gradient in the g area).

Tolerances of the calls that are not plain maps are the suite's: finite differences rtol 1e-8 (tests/test_gpu_parity.py,
test_fd_jacobian), implicit H rtol 1e-6 (tests/test_gpu_highprec.py: CG stops at a relative residual of sqrt(eps)).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED_LO, SEED_HI = 0x85A308D3, 0x243F6A88 << 32
SEED_BOTH = SEED_HI | SEED_LO
SIMS = (0, 1, 2**32 - 1, 2**32, 2**40 + 7)
SIM0, NSIMS = 2**32 - 2, 5      # a map's simulation range: 2^32 - 2 .. 2^32 + 2 (both values of the high counter word)
THETA = [0.7]
ATOL = 1e-2

# label: (N, placement, element split)
SITES = {
    "registers_256": (511, -1, 0),
    "registers_512": (513, -1, 0),
    "lds_resident": (4098, -1, 0),
    "streaming_256": (511, 0, 0),
    "streaming_512": (513, 0, 0),
    "streaming_4098": (4098, 0, 0),
    "cluster_resident": (4098, -1, 2),
    "cluster_streaming": (4098, 0, 2),
}
# placements that must agree bit for bit (the same reduction order: tests/test_gpu_parity.py, test_resident_equals_streaming_bitwise)
SAME_BITS = [("registers_256", "streaming_256"), ("registers_512", "streaming_512"), ("lds_resident", "streaming_4098")]


def problem(M, N, placement=-1, split=0):
    prob = M.HipMuseProblem(None, model="funnel", ntheta=1, N=N)
    if placement >= 0:
        prob.set_placement(placement)
    if split:
        prob.set_element_split(split)
    return prob


@pytest.fixture(scope="module")
def oracle_maps(O):
    """The oracle's map over the shared simulation range, once per (N, start mode)."""
    cache = {}

    def get(N, z0_mode=0, nsims=NSIMS):
        key = (N, z0_mode, nsims)
        if key not in cache:
            cache[key] = O.map_and_score_batch("funnel", N, SEED_BOTH, SIM0, SIM0 + nsims, THETA, atol=ATOL, z0_mode=z0_mode, nthreads=4)
        return cache[key]
    return get


@pytest.fixture(scope="module")
def site_maps(gpu, M):
    """Every call site's map (and the context's own draw of the first simulation), once."""
    out = {}
    for label, (N, placement, split) in SITES.items():
        prob = problem(M, N, placement, split)
        g, info = prob.map_and_score_batch(SEED_BOTH, SIM0, SIM0 + NSIMS, THETA, atol=ATOL, z0_mode=M.Z0_ZERO)
        out[label] = (g, info, prob.get_zhat(0, NSIMS), prob.sample_x_z(M.SimRng(SEED_BOTH, SIM0 + 1), THETA))
        prob.close()
    return out


def assert_map_is_the_oracles(g, info, zh, ref, ctx):
    go, zo, io = ref
    for k in ("status", "iterations", "f_calls"):
        assert np.array_equal(info[k], io[k]), (ctx, k, info[k], io[k])
    np.testing.assert_allclose(g, go, rtol=1e-10, err_msg=ctx)
    np.testing.assert_allclose(zh, zo, rtol=0, atol=1e-9, err_msg=ctx)
    np.testing.assert_allclose(info["f_min"], io["f_min"], rtol=1e-11, err_msg=ctx)


@pytest.mark.parametrize("N", [1, 2, 129, 1025])
def test_counter_and_key_words(gpu, M, O, N):
    prob = problem(M, N)
    for seed in (SEED_LO, SEED_HI, SEED_BOTH):
        for sim in SIMS:
            x, z = prob.sample_x_z(M.SimRng(seed, sim), THETA)
            xo, zo = O.sample_x_z("funnel", N, seed, sim, THETA)
            assert np.array_equal(z, zo), (hex(seed), sim, "z")
            assert np.array_equal(x, xo), (hex(seed), sim, "x")
    prob.close()


@pytest.mark.parametrize("label", list(SITES))
def test_call_site(site_maps, oracle_maps, O, label):
    N = SITES[label][0]
    g, info, zh, (x, z) = site_maps[label]
    xo, zo = O.sample_x_z("funnel", N, SEED_BOTH, SIM0 + 1, THETA)
    assert np.array_equal(x, xo) and np.array_equal(z, zo), label
    assert_map_is_the_oracles(g, info, zh, oracle_maps(N), label)


@pytest.mark.parametrize("a,b", SAME_BITS)
def test_placements_return_the_same_bits(site_maps, a, b):
    for u, v, what in zip(site_maps[a][:3], site_maps[b][:3], ("scores", "records", "MAPs")):
        assert np.array_equal(u, v), (a, b, what)


def test_normals_cache_and_normals_kernel(gpu, M, O, oracle_maps):
    """The second request of a simulation range stores the normals it draws, the third loads them: both must return the first's
    bits (so the stored normals are the drawn ones).  The cache then holds the range, and a finite-difference call over it draws its
    fiducial stream with normals_kernel: the oracle's Jacobians, and the bits of a fresh context whose fiducial MAP draws for itself."""
    N = 4098
    prob = problem(M, N)
    prob.set_normals_cache(True)
    runs = []
    for _ in range(3):
        g, info = prob.map_and_score_batch(SEED_BOTH, SIM0, SIM0 + NSIMS, THETA, atol=ATOL, z0_mode=M.Z0_ZERO)
        runs.append((g.copy(), info.copy(), prob.get_zhat(0, NSIMS)))
    assert_map_is_the_oracles(*runs[0], oracle_maps(N), "first request")
    for k in (1, 2):
        for u, v, what in zip(runs[k], runs[0], ("scores", "records", "MAPs")):
            assert np.array_equal(u, v), (("stored", "loaded")[k - 1], what)
    step = np.array([0.05])
    Hs, _ = prob.fd_jacobian_batch(SEED_BOTH, SIM0, SIM0 + NSIMS, THETA, step, atol=ATOL, fid_mode=0)
    prob.close()
    _, zfid, _ = O.map_and_score_batch("funnel", N, SEED_BOTH, M.MASTER_SIM, M.MASTER_SIM + 1, THETA, atol=ATOL, z0_mode=0)
    for s in range(NSIMS):
        Ho = O.fd_jacobian("funnel", N, SEED_BOTH, SIM0 + s, THETA, step, zfid[0], atol=ATOL)
        np.testing.assert_allclose(Hs[s], Ho, rtol=1e-8, atol=1e-8 * np.abs(Ho).max(), err_msg=f"sim {s}")
    fresh = problem(M, N)
    fresh.debug_flags(1 << 21)   # the fiducial MAP draws its own normals
    Hf, _ = fresh.fd_jacobian_batch(SEED_BOTH, SIM0, SIM0 + NSIMS, THETA, step, atol=ATOL, fid_mode=0)
    fresh.close()
    assert np.array_equal(Hs, Hf)


def test_start_modes_on_the_lds_resident_placement(gpu, M, O, oracle_maps):
    N = 4098
    prob = problem(M, N)
    for mode in (M.Z0_ZERO, M.Z0_TRUE):
        g, info = prob.map_and_score_batch(SEED_BOTH, SIM0, SIM0 + NSIMS, THETA, atol=ATOL, z0_mode=mode)
        assert_map_is_the_oracles(g, info, prob.get_zhat(0, NSIMS), oracle_maps(N, mode), f"z0_mode {mode}")
    Hs, _ = prob.implicit_H_batch(SEED_BOTH, SIM0, SIM0 + 2, THETA, atol=1e-10, cg_maxiter=1000)
    for s in range(2):
        Ho, _ = O.implicit_H("funnel", N, SEED_BOTH, SIM0 + s, THETA, 1e-10, 1000)
        np.testing.assert_allclose(Hs[s], Ho, rtol=1e-6, atol=1e-6 * np.abs(Ho).max(), err_msg=f"sim {s}")
    prob.close()


@pytest.mark.parametrize("cache", [True, False])
def test_true_start_after_zero_start_reads_nothing_stale(gpu, M, cache):
    """More problems than workgroups, so that a workgroup's second problem finds the g area as the first one's solve left it; with the
    normals cache on, the Z0_TRUE map is the range's second request (it stores what it draws), without it a plain draw."""
    N, n = 4098, 300
    outs = []
    for zero_first in (True, False):
        prob = problem(M, N)
        prob.set_normals_cache(cache)
        if zero_first:
            prob.map_and_score_batch(SEED_BOTH, SIM0, SIM0 + n, THETA, atol=ATOL, z0_mode=M.Z0_ZERO)
        g, info = prob.map_and_score_batch(SEED_BOTH, SIM0, SIM0 + n, THETA, atol=ATOL, z0_mode=M.Z0_TRUE)
        outs.append((g, info, prob.get_zhat(0, n)))
        prob.close()
    assert outs[0][1]["iterations"].max() >= 1
    for u, v, what in zip(outs[0], outs[1], ("scores", "records", "MAPs")):
        assert np.array_equal(u, v), what
