"""CPU tests of the device-drawn random stream's specification (include/dqmc_hip.h, dqmc_rng_seed): the numpy restatement
(tests/rng_ref.py) against the published Philox4x32-10 answers, against the text the fill kernel compiles (dqmc_amd/csrc/philox.h
through libdqmc_host.so), the stream's invariants and four fixed-seed statistics, and the new entry points without a device."""
import ctypes as C
import itertools

import numpy as np
import pytest

import dqmc_amd
import rng_ref

KAT = [  # counter, key -> output
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def host():
    h = C.CDLL(dqmc_amd.HOST_LIB_PATH)
    h.dqmc_host_philox.argtypes = [C.c_void_p] * 3; h.dqmc_host_philox.restype = None
    h.dqmc_host_rng_stream.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_int] + [C.c_void_p] * 3
    h.dqmc_host_rng_stream.restype = None
    return h


@pytest.mark.parametrize("counter,key,out", KAT)
def test_philox_known_answers(counter, key, out):
    got = rng_ref.philox4x32_10(counter, key)
    assert tuple(int(x[0]) for x in got) == out
    c = np.array(counter, np.uint32); k = np.array(key, np.uint32); o = np.zeros(4, np.uint32)
    host().dqmc_host_philox(c.ctypes.data, k.ctypes.data, o.ctypes.data)          # csrc/philox.h, the kernel's own text
    assert tuple(int(x) for x in o) == out


def test_philox_is_vectorised_consistently():
    rng = np.random.default_rng(0)
    ctr = rng.integers(0, 2 ** 32, size=(4, 50), dtype=np.uint64)
    all_at_once = rng_ref.philox4x32_10(tuple(ctr), (123, 456))
    for j in range(50):
        one = rng_ref.philox4x32_10(tuple(int(x) for x in ctr[:, j]), (123, 456))
        assert all(int(one[k][0]) == int(all_at_once[k][j]) for k in range(4))


@pytest.mark.parametrize("seed,g,h,nt,n", [(0x123456789abcdef, 5, 0, 3, 4), (0xfedcba9876543210, 7, 2 ** 32 - 2, 20, 100),
                                           (2024, 0, 1, 5, 1024), (1, 2 ** 32 - 1, 2 ** 32 - 1, 2, 289)])
def test_kernel_text_matches_the_numpy_statement(seed, g, h, nt, n):
    """philox.h's rng_proposal / rng_perm_key (what rng_fill_kernel runs per thread) with std::sort on (key64, site)."""
    perm = np.empty((nt, n), np.int32); k = np.empty((nt, n), np.uint8); u = np.empty((nt, n))
    host().dqmc_host_rng_stream(seed, g, h, nt, n, perm.ctypes.data, k.ctypes.data, u.ctypes.data)
    rp, rk, ru = rng_ref.stream(seed, g, h, nt, n)
    assert (perm == rp).all() and (k == rk).all() and (u.view(np.uint64) == ru.view(np.uint64)).all()


def test_stream_invariants():
    for n, nt in [(4, 7), (100, 5), (1000, 3)]:
        perm, k, u = rng_ref.stream(0xabcdef0012345678, 3, 9, nt, n)
        assert perm.dtype == np.int32 and k.dtype == np.uint8 and u.dtype == np.float64
        assert (np.sort(perm, axis=1) == np.arange(n)[None, :]).all()
        assert k.max() <= 2
        assert u.min() >= 0.0 and u.max() < 1.0
        assert (u * 2.0 ** 53 == np.floor(u * 2.0 ** 53)).all()


def test_streams_of_different_counter_or_chain_differ():
    base = rng_ref.stream(99, 4, 10, 6, 64)
    for other in (rng_ref.stream(99, 4, 11, 6, 64), rng_ref.stream(99, 5, 10, 6, 64), rng_ref.stream(100, 4, 10, 6, 64),
                  rng_ref.stream(99 + (1 << 32), 4, 10, 6, 64)):
        for a, b in zip(base, other):
            assert (a != b).any()
        assert (base[2] != other[2]).mean() > 0.99
    again = rng_ref.stream(99, 4, 10, 6, 64)
    assert all((a == b).all() for a, b in zip(base, again))


def chi2(counts, expected):
    return float(((np.asarray(counts, np.float64) - expected) ** 2 / expected).sum())


def test_fixed_seed_statistics():
    """Deterministic, so conditions and not measurements; each bound is about the 99.9 % quantile of its chi-square distribution
    (23, 2, 63 and 7 degrees of freedom)."""
    perm, k, u = rng_ref.stream(2024, 0, 0, 24000, 4)
    code = perm[:, 0] * 64 + perm[:, 1] * 16 + perm[:, 2] * 4 + perm[:, 3]
    counts = [int((code == a * 64 + b * 16 + c * 4 + d).sum()) for a, b, c, d in itertools.permutations(range(4))]
    assert sum(counts) == 24000
    x = chi2(counts, 1000.0); print(f"chi2 over the 24 permutations of 4 sites: {x:.2f}"); assert x < 49.7
    x = chi2(np.bincount(k.ravel(), minlength=3), k.size / 3.0); print(f"chi2 of kprop: {x:.2f}"); assert x < 13.8
    x = chi2(np.bincount((u.ravel() * 64).astype(np.int64), minlength=64), u.size / 64.0); print(f"chi2 of u in 64 bins: {x:.2f}"); assert x < 103.4
    perm, _, _ = rng_ref.stream(7, 3, 11, 4000, 256)
    pos0 = np.argmax(perm == 0, axis=1)
    x = chi2(np.bincount(pos0 // 32, minlength=8), 4000 / 8.0); print(f"chi2 of site 0's position over 8 octiles: {x:.2f}"); assert x < 24.3


def test_new_entry_points_without_an_engine():
    lib = dqmc_amd.lib()
    for s in ("rng_seed", "rng_state", "rng_draw", "rng_fill_time"):
        assert s in dqmc_amd.ABI_SYMBOLS and lib.has_symbol(s)
    EINVAL = -1
    assert lib._sym("rng_seed")(None, C.c_uint64(1), C.c_uint32(0), C.c_uint32(0)) == EINVAL
    sd = C.c_uint64(0); fc = C.c_uint32(0); ct = C.c_uint32(0); on = C.c_int(0)
    assert lib._sym("rng_state")(None, C.byref(sd), C.byref(fc), C.byref(ct), C.byref(on)) == EINVAL
    perm = np.zeros(4, np.int32); k = np.zeros(4, np.uint8); u = np.zeros(4)
    assert lib._sym("rng_draw")(None, C.c_uint32(0), perm.ctypes.data_as(dqmc_amd.abi.c_int32_p), k.ctypes.data_as(dqmc_amd.abi.c_uint8_p),
                                u.ctypes.data_as(dqmc_amd.abi.c_double_p)) == EINVAL
    ms = C.c_double(0.0)
    assert lib._sym("rng_fill_time")(None, 1, C.byref(ms)) == EINVAL
    assert b"null engine" in lib._sym("last_error")()
