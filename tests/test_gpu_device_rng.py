"""GPU tests (-m gpu) of the random stream drawn on the device (dqmc_rng_seed / dqmc_rng_state / dqmc_rng_draw, rng.hip):
the stream is the one tests/rng_ref.py states, bit for bit; a sweep without arrays is the sweep with those arrays (against the
CPU oracle and against a second engine fed explicitly); a batched engine draws what single-chain engines with the same stream
ids draw; a chain resumes from (fields, seed, chain id, counter); the error paths; the driver's [simulation] device_rng key."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pt_twin
import rng_ref

import dqmc_amd
from dqmc_amd import CONFIGS, DqmcError, HubbardModel, ghq_tables

pytestmark = pytest.mark.gpu
TOL = 1e-10
SEED = 0x9e3779b97f4a7c15            # both 32-bit halves non-zero
EINVAL, ERANGE = -1, -4


def close(a, b, tol=TOL):
    """the suite's bar: tol * max(1, max|G|)"""
    a = np.asarray(a); b = np.asarray(b)
    return np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max())


def bare_engine(lib, n, nt, n_chains=None):
    """An engine that only has to draw: the kinetic matrices are never used."""
    gamma, eta = ghq_tables()
    return lib.engine(n, nt, 10, 0.5, gamma, eta, np.eye(n), np.eye(n), n_chains=n_chains)


def same_stream(got, ref):
    return (got[0] == ref[0]).all() and (got[1] == ref[1]).all() and (got[2].view(np.uint64) == ref[2].view(np.uint64)).all()


# n < 64, non-powers of two, 1000 and 1024
@pytest.mark.parametrize("L1,L2", [(2, 2), (3, 3), (4, 4), (8, 8), (9, 8), (10, 10), (16, 16), (17, 17), (24, 24), (40, 25), (32, 32)])
def test_exact_stream(hip, L1, L2):
    n = L1 * L2
    for nt in (3, 20):
        for Cn in (1, 3):
            with bare_engine(hip, n, nt, n_chains=None if Cn == 1 else Cn) as e:
                e.rng_seed(SEED, first_chain=5)
                for h in (0, 1, 2 ** 32 - 2):
                    perm, k, u = e.rng_draw(h)
                    assert perm.dtype == np.int32 and k.dtype == np.uint8 and u.dtype == np.float64
                    for c in range(Cn):
                        got = (perm, k, u) if Cn == 1 else (perm[c], k[c], u[c])
                        assert same_stream(got, rng_ref.stream(SEED, 5 + c, h, nt, n)), (n, nt, Cn, c, h)
                assert e.rng_state() == (SEED, 5, 0, True)            # drawing leaves the counter alone


REPLAY = [CONFIGS["cfg1"], CONFIGS["cfg2"], dict(L1=10, L2=10, U=4.0, beta=2.0, nt=20, n_stab=10),
          dict(L1=20, L2=16, U=4.0, beta=2.0, nt=20, n_stab=10)]        # the last: n = 320, the n > 256 path


@pytest.mark.parametrize("cfg", REPLAY, ids=lambda c: f"{c['L1']}x{c['L2']}")
def test_replay_parity(hip, orc, cfg):
    m = HubbardModel(**cfg); f = m.random_fields(31)
    e = m.engine(hip); e.set_fields(f); e.init(); e.rng_seed(SEED, first_chain=2)
    s1, s2 = e.rng_draw(0), e.rng_draw(1)
    assert same_stream(s1, rng_ref.stream(SEED, 2, 0, m.nt, m.n)) and same_stream(s2, rng_ref.stream(SEED, 2, 1, m.nt, m.n))
    e.sweep_0_to_beta(); e.sweep_beta_to_0()
    o = m.engine(orc); o.set_fields(f); o.init()
    o.sweep_0_to_beta(*s1); o.sweep_beta_to_0(*s2)
    assert (e.get_fields() == o.get_fields()).all()
    assert e.stats().n_accepted == o.stats().n_accepted
    Ge, Go = e.get_G(), o.get_G()
    print(f"{cfg['L1']}x{cfg['L2']}: max|dG| = {np.abs(Ge - Go).max():.3e}, max|G| = {np.abs(Go).max():.3e}")
    assert close(Ge, Go)
    assert e.rng_state() == (SEED, 2, 2, True)
    # explicit arrays on a seeded engine: the same chain, and the counter stays
    x = m.engine(hip); x.set_fields(f); x.init(); x.rng_seed(SEED, first_chain=2)
    x.sweep_0_to_beta(*s1); x.sweep_beta_to_0(*s2)
    assert (x.get_fields() == e.get_fields()).all()
    assert x.stats().n_accepted == e.stats().n_accepted
    assert x.rng_state() == (SEED, 2, 0, True)
    for eng in (e, o, x):
        eng.close()


def test_batch_draws_what_singles_draw(hip, orc):
    m = HubbardModel(**CONFIGS["cfg1"]); K = 4
    f = np.stack([m.random_fields(100 + c) for c in range(K)])
    b = m.engine(hip, n_chains=K); b.set_fields(f); b.init(); b.rng_seed(SEED, first_chain=8)
    draws = [b.rng_draw(h) for h in (0, 1)]
    for c in range(K):
        with m.engine(hip) as s:
            s.rng_seed(SEED, first_chain=8 + c)
            for h in (0, 1):
                assert same_stream(s.rng_draw(h), tuple(a[c] for a in draws[h])), (c, h)
    b.sweep_0_to_beta(); b.sweep_beta_to_0()
    fb, Gb, st = b.get_fields(), b.get_G(), b.stats()
    for c in range(K):
        o = m.engine(orc); o.set_fields(f[c]); o.init()
        o.sweep_0_to_beta(*(a[c] for a in draws[0])); o.sweep_beta_to_0(*(a[c] for a in draws[1]))
        assert (fb[c] == o.get_fields()).all(), c
        assert st[c].n_accepted == o.stats().n_accepted
        assert close(Gb[c], o.get_G())
        o.close()
    assert b.rng_state() == (SEED, 8, 2, True)
    b.close()


@pytest.mark.parametrize("cfg", [CONFIGS["cfg1"], dict(L1=8, L2=8, U=4.0, beta=2.0, nt=20, n_stab=10)], ids=["4x4", "8x8"])
def test_resume_from_fields_and_counter(hip, cfg):
    m = HubbardModel(**cfg); f = m.random_fields(7)

    def sweeps(e, k):
        for _ in range(k):
            e.sweep_0_to_beta(); e.sweep_beta_to_0()

    a = m.engine(hip); a.set_fields(f); a.init(); a.rng_seed(SEED, first_chain=1); sweeps(a, 3)
    b = m.engine(hip); b.set_fields(f); b.init(); b.rng_seed(SEED, first_chain=1); sweeps(b, 1)
    seed, first, counter, seeded = b.rng_state()
    assert (seed, first, counter, seeded) == (SEED, 1, 2, True)
    c = m.engine(hip); c.set_fields(b.get_fields()); c.init(); c.rng_seed(seed, first, counter); sweeps(c, 2)
    assert (a.get_fields() == c.get_fields()).all()
    assert close(c.get_G(), a.get_G())
    assert a.rng_state() == c.rng_state() == (SEED, 1, 6, True)
    for e in (a, b, c):
        e.close()


def test_errors(hip):
    m = HubbardModel(**CONFIGS["cfg1"]); f = m.random_fields(3)
    e = m.engine(hip); e.set_fields(f); e.init()
    rng = np.random.default_rng(0)
    perm, k, u = e._stream(*m.random_stream(rng), m.nt)
    P, K, U = perm.ctypes.data_as(dqmc_amd.abi.c_int32_p), k.ctypes.data_as(dqmc_amd.abi.c_uint8_p), u.ctypes.data_as(dqmc_amd.abi.c_double_p)
    fwd, bwd = hip._sym("sweep_0_to_beta"), hip._sym("sweep_beta_to_0")
    assert e.rng_state() == (0, 0, 0, False)
    for fn in (fwd, bwd):                                            # never seeded: NULL streams are refused as before
        assert fn(e._h, None, None, None) == EINVAL
    with pytest.raises(DqmcError) as ei:
        e.rng_draw(0)
    assert ei.value.code == EINVAL
    e.rng_seed(SEED)
    for fn in (fwd, bwd):                                            # some NULL, some not
        for args in ((None, K, U), (P, None, U), (P, K, None), (P, None, None), (None, None, U)):
            assert fn(e._h, *args) == EINVAL
    e.sync()
    assert (e.get_fields() == f).all() and e.rng_state() == (SEED, 0, 0, True)
    with pytest.raises(DqmcError):                                   # the slice-level call keeps requiring arrays
        e._c("local_update_slice", 0, None, None, None, None)
    # the counter's last value means "used up"
    e.rng_seed(SEED, 0, 2 ** 32 - 1)
    for fn in (fwd, bwd):
        assert fn(e._h, None, None, None) == ERANGE
    e.sync()
    assert (e.get_fields() == f).all() and e.rng_state() == (SEED, 0, 2 ** 32 - 1, True)
    e.rng_seed(SEED, 0, 2 ** 32 - 2)
    e.sweep_0_to_beta()                                              # half sweep 2^32 - 2 is drawn ...
    assert e.rng_state()[2] == 2 ** 32 - 1
    f1 = e.get_fields()
    assert bwd(e._h, None, None, None) == ERANGE                     # ... the next one is refused
    e.sync()
    assert (e.get_fields() == f1).all()
    e.sweep_beta_to_0(*m.random_stream(rng))                         # explicit arrays still work
    e.sync()
    e.close()


def test_driver_device_rng_key(hip, tmp_path):
    """dqmc_driver with [simulation] device_rng = true, seed 777, rank label 3: the bins it prints are those of a Python engine
    seeded (777, 3) on the fields the facade builds from the same seed, and the counter it reports is 2 (5 + 2 * 4)."""
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    driver = os.path.join(here, "dqmc_amd", "dqmc_driver")
    assert os.path.exists(driver), "dqmc_driver missing: run make / __graft_entry__.build()"
    ini = ("[Lattice]\nL1 = 4\nL2 = 4\n[hubbard]\nU = 4.0\nt = 1.0\nmu = -0.1\n[simulation]\nbeta = 2.0\nnt = 20\nn_therms = 5\nn_sweeps = 4\n"
           "n_bins = 2\nn_stab = 10\nsymmetric = false\nisMeasureUnequalTime = false\ndevice_rng = true\n"
           "[ParallelTempering]\nenabled = false\nsweep_steps = 20\nbetas = 2.0\n")
    (tmp_path / "parameters.in").write_text(ini)
    out = subprocess.run([driver, "parameters.in", "0", "777", "3"], cwd=tmp_path, capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, DQMC_NO_HDF5="1"))
    assert out.returncode == 0, out.stderr[-2000:]
    printed = re.findall(r"bin (\d+) \((\d+) sweeps\): density ([-\d.eE+]+)\s+doubleOcc ([-\d.eE+]+)\s+swave ([-\d.eE+]+)", out.stdout)
    assert len(printed) == 2, out.stdout
    pos = re.search(r"rank 3: rng seed (\d+) chain (\d+) counter (\d+)", out.stdout)
    assert pos, out.stdout
    assert tuple(int(x) for x in pos.groups()) == (777, 3, 2 * (5 + 8))

    h = pt_twin.load_host()
    mdl = pt_twin.host_model(h, ini, 2.0, 777 + 3, 16, 20)           # utility::random rng(seed + rank) draws the initial fields
    e = hip.engine(16, 20, 10, mdl["g"], mdl["gamma"], mdl["eta"], mdl["expK"], mdl["invexpK"])
    e.set_fields(mdl["fields"]); e.init(); e.rng_seed(777, 3)
    for _ in range(5):
        e.sweep_0_to_beta(); e.sweep_beta_to_0()
    for b in range(2):
        for _ in range(4):
            e.sweep_0_to_beta(); e.sweep_beta_to_0(); e.measure_accumulate(4, 4)
        sc, _, cnt = e.measure_fetch(4, 4)
        assert cnt == 4 and int(printed[b][1]) == 4
        for name, mine, theirs in zip(("density", "doubleOcc", "swave"), sc / cnt, printed[b][2:]):
            print(f"bin {b + 1} {name}: engine {mine:.10f} driver {theirs}")
            assert abs(mine - float(theirs)) < 1e-7
    assert e.rng_state() == (777, 3, 26, True)
    e.close()
