"""block_allreduce (csrc/reduce.hpp) alone: the bits of every thread's result against a host restatement of the stated tree.

tests/native/allreduce_tree_driver.hip launches, per case, ONE workgroup that does nothing but block_allreduce<T, KS, KM> and writes
what every thread holds afterwards.  T in {64, 128, 256, 512, 1024} (NW = 1, 2, 4, 8, 16 waves: every branch of the cross-wave
butterfly) x (KS, KM) in {(1,0), (0,1), (3,1), (4,2), (7,1), (8,0)}, three input sets per case (one launch: the parity buffer
alternates between them):
  0  seeded random doubles of mixed sign and magnitude (2^-40 .. 2^40);
  1  -0.0, +0.0, subnormals of both signs, tiny and huge normals, and infinities -- +inf only in the even sums, -inf only in the odd
     ones (inf - inf would be an invalid operation, whose default NaN has another sign bit on the host than on the GPU: not a
     property of the tree), both infinities in the maxima, and one sum (the third, where there is one) of nothing but -0.0;
  2  set 0 with a quiet NaN in one lane of one sum and in one lane of one maximum.
The tree, restated with numpy float64: within a wave pairwise xor 1, xor 2, half-row mirror and row mirror in
rows of 16, then (r0 + r1) + (r2 + r3) over the four rows' totals; across waves lane l holds wave (l mod NW)'s total and the same
butterfly runs over the first NW lanes.  A maximum drops a NaN operand (and +0 > -0, as v_max_f64 orders them).  Every thread of the
workgroup must hold the expected 64-bit pattern -- the result is uniform; a NaN result must be a NaN in every thread (the payload is
the one input NaN's on both sides, but it is not what the tree defines).  Both forms of the row combination (reduce.hpp, ROW_BCAST:
in vector registers towards lane 63, and the v_readlane form that one entry point keeps) run on the same inputs.

The restatement itself is checked without a GPU against a straightforward sum, per row of 16 and over the workgroup, at rtol 1e-15:
on inputs whose every partial sum is exact in float64 (multiples of 2^-20 below 2^20 in magnitude, mixed in sign and size: at most
1024 of them need 51 bits), so that the order of summation cannot matter and any difference is an element counted twice or not at
all."""
import math
import os
import subprocess

import numpy as np
import pytest

from museinference_jl_amd import build as B

HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(HERE, "native", "allreduce_tree_driver.hip")
TS = (64, 128, 256, 512, 1024)
KSKM = ((1, 0), (0, 1), (3, 1), (4, 2), (7, 1), (8, 0))
NSETS = 3
FORMS = ("rows combined in vector registers", "rows read into scalars")   # block_allreduce's ROW_BCAST = true (the default), false


# ---- the tree, restated -------------------------------------------------------------------------------------------------------
def fmax_drop_nan(a, b):
    """v_max_f64 on quiet operands: a NaN operand is dropped (both NaN: NaN), +0 is larger than -0."""
    with np.errstate(invalid="ignore"):
        r = np.where(np.isnan(a), b, np.where(np.isnan(b), a, np.where(a >= b, a, b)))
    both_zero = (a == 0.0) & (b == 0.0)
    return np.where(both_zero, np.where(np.signbit(a) & np.signbit(b), -0.0, 0.0), r)


def combine(a, b, is_max):
    if is_max:
        return fmax_drop_nan(a, b)
    with np.errstate(invalid="ignore", over="ignore"):
        return a + b


_LANE = np.arange(64)
_EXCHANGES = (_LANE ^ 1, _LANE ^ 2, (_LANE & ~7) | (7 - (_LANE & 7)), (_LANE & ~15) | (15 - (_LANE & 15)))


def row_totals(v, is_max):
    """v: 64 lanes of one wave -> 64 lanes, each holding the total of its row of 16 (the four DPP exchange steps)."""
    v = np.asarray(v, dtype=np.float64)
    for partner in _EXCHANGES:
        v = combine(v, v[partner], is_max)
    return v


def wave_total(v, is_max):
    r = row_totals(v, is_max)
    return combine(combine(r[0], r[16], is_max), combine(r[32], r[48], is_max), is_max)


def workgroup_total(x, is_max):
    """x: T values, thread t's contribution -> the value every thread holds after block_allreduce."""
    nw = x.size // 64
    w = np.array([wave_total(x[64 * i:64 * (i + 1)], is_max) for i in range(nw)], dtype=np.float64)
    lanes = w[_LANE % nw]                       # lane l reads wave (l mod NW)'s total
    for step, partner in enumerate(_EXCHANGES):
        if nw >= 2 << step:
            lanes = combine(lanes, lanes[partner], is_max)
    return np.float64(lanes[0])                 # v_readfirstlane


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
_SPECIALS = np.array([-0.0, 0.0, 5e-324, -5e-324, 2.2e-308, -2.2e-308, 1e-310, -1e-310, 1e300, -1e300, 1.0, -1.0])


def case_inputs(rng, T, KS, KM):
    """(NSETS, K, T) doubles: value k < KS is a sum, the others are maxima."""
    K = KS + KM
    x = np.empty((NSETS, K, T))
    x[0] = rng.standard_normal((K, T)) * np.exp2(rng.integers(-40, 41, size=(K, T)))
    x[1] = _SPECIALS[rng.integers(0, _SPECIALS.size, size=(K, T))]
    for k in range(K):
        lanes = rng.choice(T, size=3, replace=False)
        if k < KS:
            x[1, k, lanes[:2]] = np.inf if k % 2 == 0 else -np.inf
        else:
            x[1, k, lanes[0]], x[1, k, lanes[1]] = np.inf, -np.inf
    if KS >= 3:
        x[1, 2] = -0.0
    if KM >= 2:
        x[1, KS + 1] = np.where(rng.integers(0, 2, size=T) == 0, -0.0, 0.0)   # signed zeros alone
        x[1, KS + 1, : T // 2] = -0.0
    x[2] = x[0]
    if KS:
        x[2, rng.integers(0, KS), rng.integers(0, T)] = np.nan
    if KM:
        x[2, KS + rng.integers(0, KM), rng.integers(0, T)] = np.nan
    return x


def all_inputs():
    rng = np.random.default_rng(20240607)
    return [(T, KS, KM, case_inputs(rng, T, KS, KM)) for T in TS for KS, KM in KSKM]


# ---- without a GPU: the restatement against a straightforward sum ----------------------------------------------------------------
@pytest.mark.parametrize("T", TS)
def test_restatement_matches_straightforward_sums(T):
    rng = np.random.default_rng(T)
    # multiples of 2^-20 with magnitudes from 2^-20 to 2^20, mixed in sign: every partial sum of up to 1024 is exact
    x = rng.integers(-(1 << 20), 1 << 20, size=T).astype(np.float64) * np.exp2(rng.integers(-20, 1, size=T))
    assert np.any(x > 0) and np.any(x < 0) and np.all(x * 2.0 ** 20 == np.round(x * 2.0 ** 20))
    for w in range(T // 64):
        rows = row_totals(x[64 * w:64 * (w + 1)], False)
        for r in range(4):
            want = math.fsum(x[64 * w + 16 * r:64 * w + 16 * (r + 1)])
            np.testing.assert_allclose(rows[16 * r:16 * (r + 1)], want, rtol=1e-15, atol=0)
    np.testing.assert_allclose(workgroup_total(x, False), math.fsum(x), rtol=1e-15, atol=0)
    np.testing.assert_allclose(workgroup_total(x, False), np.sum(x), rtol=1e-15, atol=0)
    # maxima: the largest element, whatever the order; a NaN is dropped, signed zeros are ordered
    assert workgroup_total(x, True) == x.max()
    y = x.copy()
    y[T // 3] = np.nan
    assert workgroup_total(y, True) == np.nanmax(y)
    z = np.full(T, -0.0)
    assert np.signbit(workgroup_total(z, True))
    z[T - 5] = 0.0
    assert not np.signbit(workgroup_total(z, True))
    assert np.isnan(workgroup_total(y, False))


# ---- on the GPU ---------------------------------------------------------------------------------------------------------------------
def driver_path():
    """The driver, built next to the product library's objects (a build directory git ignores) when missing or older than its sources."""
    out_dir = os.path.join(os.path.dirname(B.LIB_PATH), "build_allreduce_tree")
    exe = os.path.join(out_dir, "allreduce_tree_driver")
    deps = [DRIVER, os.path.join(B.CSRC, "reduce.hpp"), os.path.join(B.CSRC, "args.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        os.makedirs(out_dir, exist_ok=True)
        hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
        subprocess.check_call([hipcc] + B.COMMON_FLAGS + B._DEVICE_FLAGS + ["-I" + B.CSRC, "-x", "hip", DRIVER, "-o", exe + ".tmp"])
        os.replace(exe + ".tmp", exe)
    return exe


@pytest.fixture(scope="module")
def device_results(gpu, tmp_path_factory):
    d = tmp_path_factory.mktemp("allreduce_tree")
    cases = all_inputs()
    fin, fout = str(d / "in.f64"), str(d / "out.f64")
    np.concatenate([x.ravel() for _, _, _, x in cases]).tofile(fin)
    r = subprocess.run([driver_path(), fin, fout, str(NSETS)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = np.fromfile(fout, dtype=np.float64).reshape(len(FORMS), -1)
    got, pos = {}, 0
    for T, KS, KM, x in cases:
        got[(T, KS, KM)] = (x, [out[f, pos:pos + x.size].reshape(x.shape) for f in range(len(FORMS))])
        pos += x.size
    assert pos == out.shape[1]
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("KS,KM", KSKM)
def test_every_thread_holds_the_tree_bits(device_results, T, KS, KM):
    x, got = device_results[(T, KS, KM)]
    names = ("random", "specials", "nan")
    for s in range(NSETS):
        for k in range(KS + KM):
            want = workgroup_total(x[s, k], k >= KS)
            for form, out in zip(FORMS, got):
                g = out[s, k]
                if np.isnan(want):
                    assert np.all(np.isnan(g)), (form, names[s], k, g[:4])
                    continue
                wb, gb = np.float64(want).view(np.uint64), g.view(np.uint64)
                assert np.all(gb == wb), (form, names[s], k, hex(int(wb)), [hex(int(b)) for b in np.unique(gb)[:4]])
    # what the sets are there for: the NaN reached its sum and was dropped from its maximum
    if KS:
        assert any(np.isnan(workgroup_total(x[2, k], False)) for k in range(KS))
    for k in range(KS, KS + KM):
        assert not np.isnan(workgroup_total(x[2, k], True)) and np.isnan(x[2, KS:]).sum() == 1
