"""muse_lbfgs_normals on the GPU (include/muse_lbfgs.h: the engine's normal stream for all rows of a map in one launch) against the
oracle's restatement of the stream (oracle.normals; mo_normal_pair through ctypes at offsets too large to reach by a prefix): every
value bit for bit (compared as int64 words), nothing written outside `out`, rows independent of the batch, and EngineNormals'
cursor.  The stream of (seed, sim) as a sequence: e_2i = n1(i), e_2i+1 = n2(i); a request starts at a pair boundary."""
import ctypes as C

import numpy as np
import pytest
import torch

DEV = "cuda"
SEEDS = (7, (1 << 63) + 11)
SIMS = (0, 5, (1 << 32) - 1, (1 << 40) + 3, (1 << 62) - 1)        # DATA_SIM and MASTER_SIM among them
K, T = 4, 256                                                    # the kernel's chains per lane and workgroup size: T K pairs per workgroup
# 1, 2: one pair, with and without its n2; 7, 8: a few lanes; 511 - 513: one pair per lane of the workgroup, with the odd end on either
# side, and the first second-pair of a lane; 2 T K + 1: a second workgroup that stores one value; 2 1024 K + 1: five workgroups per row
COUNTS = (1, 2, 7, 8, 511, 512, 513, 2 * T * K + 1, 2 * 1024 * K + 1)
OFFSETS = (0, 3, (1 << 32) - 2)                                  # the last: the counter's low word carries into the high one
MAXPAIRS = (max(COUNTS) + 1) // 2


def launch(M, out, nrows, count, seed, sims, pair_offset):
    rc = M._capi.load_lbfgs_library().muse_lbfgs_normals(out.data_ptr(), nrows, count, seed, sims.data_ptr(), pair_offset,
                                                         torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc


def draw(M, seed, sims, count, pair_offset):
    s = torch.as_tensor(np.asarray(sims, dtype=np.int64), device=DEV)
    out = torch.full((len(sims), count), float("nan"), dtype=torch.float64, device=DEV)
    launch(M, out, len(sims), count, seed, s, pair_offset)
    return out.cpu().numpy()


def pairs_by_ctypes(O, seed, sim, first, npairs):
    lib = O.lib()
    n1, n2 = C.c_double(), C.c_double()
    e = np.empty(2 * npairs)
    for i in range(npairs):
        lib.mo_normal_pair(C.c_uint64(seed), C.c_uint64(sim), C.c_uint64(first + i), C.byref(n1), C.byref(n2))
        e[2 * i], e[2 * i + 1] = n1.value, n2.value
    return e


_ref = {}


def reference(O, seed, sim, pair_offset):
    """e_{2 pair_offset} .. of stream (seed, sim), MAXPAIRS pairs; computed once per stream and offset, never modified."""
    key = (seed, sim, pair_offset)
    if key not in _ref:
        if pair_offset < 1 << 16:
            n1, n2 = O.normals(seed, sim, pair_offset + MAXPAIRS)
            e = np.empty(2 * MAXPAIRS)
            e[0::2], e[1::2] = n1[pair_offset:], n2[pair_offset:]
        else:
            e = pairs_by_ctypes(O, seed, sim, pair_offset, MAXPAIRS)
        e.setflags(write=False)
        _ref[key] = e
    return _ref[key]


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def test_mo_normal_pair_is_oracle_normals(O):
    n1, n2 = O.normals(7, 5, 40)
    e = pairs_by_ctypes(O, 7, 5, 3, 37)
    assert same_bits(e[0::2], n1[3:]) and same_bits(e[1::2], n2[3:])


@pytest.mark.gpu
@pytest.mark.parametrize("pair_offset", OFFSETS)
@pytest.mark.parametrize("seed", SEEDS)
def test_every_value_is_the_oracles_bit_for_bit(M, O, gpu, seed, pair_offset):
    for count in COUNTS:
        got = draw(M, seed, SIMS, count, pair_offset)
        assert not np.isnan(got).any(), count
        for r, sim in enumerate(SIMS):
            assert same_bits(got[r], reference(O, seed, sim, pair_offset)[:count]), (seed, sim, count, pair_offset)


@pytest.mark.gpu
@pytest.mark.parametrize("count", [7, 513, 2 * T * K + 1])
def test_nothing_is_written_outside_out(M, O, gpu, count):
    """`out` starts at an odd element of a 256-byte aligned allocation -- 8-byte but not 16-byte aligned -- and count is odd, so the rows
    alternate between the two store paths; two launches into two slices of one sentinel-filled tensor."""
    seed, nrows, pad, sentinel = 7, len(SIMS), 37, -12345.678
    big = torch.full((1 + nrows * count + pad + nrows * count + pad,), sentinel, dtype=torch.float64, device=DEV)
    assert big.data_ptr() % 16 == 0
    a0, b0 = 1, 1 + nrows * count + pad
    A, Bv = big[a0:a0 + nrows * count], big[b0:b0 + nrows * count]
    assert A.data_ptr() % 16 == 8 and A.data_ptr() % 8 == 0
    sims = torch.as_tensor(np.asarray(SIMS, dtype=np.int64), device=DEV)
    launch(M, A, nrows, count, seed, sims, 0)
    launch(M, Bv, nrows, count, seed, sims, 3)
    h = big.cpu().numpy()
    assert np.all(h[:a0] == sentinel) and np.all(h[a0 + nrows * count:b0] == sentinel) and np.all(h[b0 + nrows * count:] == sentinel)
    for r, sim in enumerate(SIMS):
        assert same_bits(h[a0 + r * count:a0 + (r + 1) * count], reference(O, seed, sim, 0)[:count])
        assert same_bits(h[b0 + r * count:b0 + (r + 1) * count], reference(O, seed, sim, 3)[:count])


@pytest.mark.gpu
def test_rows_do_not_depend_on_the_batch(M, gpu):
    seed, count, off = 7, 513, 3
    batch = draw(M, seed, (3, 0, 7), count, off)
    for r, sim in enumerate((3, 0, 7)):
        assert same_bits(batch[r], draw(M, seed, (sim,), count, off)[0])
    perm = draw(M, seed, (7, 3, 0), count, off)
    assert same_bits(perm, batch[[2, 0, 1]])
    assert not same_bits(batch[0], batch[1])


@pytest.mark.gpu
def test_engine_normals_cursor(M, gpu):
    """(5) then (2, 3): three pairs (the sixth value discarded), then three more -- the kernel at pair offsets 0 and 3."""
    sims = (3, 0, 7)
    en = M.EngineNormals(DEV, 7, sims)
    assert en.B == 3 and en.device.type == "cuda" and en.sims.dtype == torch.int64 and en.cursor == 0
    a, b = en.normals(5), en.normals(2, 3)
    assert a.shape == (3, 5) and b.shape == (3, 2, 3) and a.dtype == torch.float64 and not a.requires_grad and en.cursor == 6
    assert same_bits(a.cpu().numpy(), draw(M, 7, sims, 5, 0))
    assert same_bits(b.cpu().numpy().reshape(3, 6), draw(M, 7, sims, 6, 3))
    other = M.EngineNormals(DEV, 7, torch.as_tensor(sims))
    assert torch.equal(other(5), a) and torch.equal(other(2, 3), b)
    again = en.fresh()
    assert again.cursor == 0 and torch.equal(again.normals(5), a) and en.cursor == 6
    with pytest.raises(ValueError):
        en.normals(0)


def test_engine_normals_refuses_a_cpu_device(M):
    with pytest.raises(M.MuseError) as e:
        M.EngineNormals("cpu", 7, [0])
    assert "no HIP device available (libmuse_lbfgs has no CPU fallback)" in str(e.value)
