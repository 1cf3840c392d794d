"""GPU tests (-m gpu) of what the stabilisation keeps from one call to the next, and of the explicit Q of the panel QR.

* Every stack entry of an engine with at most 8 chains owns a slot for X = R^-1 diag(1 / max(d, 1)); a stabilisation that finds
  the slot valid skips the triangular (or LU) solve.  The slot must go stale with every write of the entry's d or R: the
  cases below change the fields under an initialised stack (set_fields + init, an in-engine replica exchange) and sweep on,
  and start a forward sweep on the product entries init leaves (no slot valid, the LU route fills them).  Each against the
  CPU oracle on the same fields and random streams: fields exact, |dG| <= 1e-10 * max(1, max|G|), the suite's bar for i.i.d.
  fields (tests/test_gpu_parity.py).
* dqmc_to_ldr with Q accumulated beside the trailing updates (qr_panel.hip), at the bounds of test_gpu_parity.py::test_to_ldr.
* The transposed copy of G a backward stabilisation leaves for the local-update walk is G^T, entry for entry."""
import numpy as np
import pytest

from dqmc_amd import CONFIGS, HubbardModel

pytestmark = pytest.mark.gpu
TOL = 1e-10


def check(tag, e, o):
    G, Go = e.get_G(), o.get_G()
    err, scale = float(np.abs(G - Go).max()), max(1.0, float(np.abs(Go).max()))
    print(f"{tag}: max|dG| = {err:.3e}, max|G| = {scale:.3e}")
    assert np.array_equal(e.get_fields(), o.get_fields()), tag
    assert err <= TOL * scale, (tag, err, scale)
    assert e.stats().n_accepted == o.stats().n_accepted, tag


def sweep_both(m, rng, e, o, forward=True, backward=True):
    for on, name in ((forward, "sweep_0_to_beta"), (backward, "sweep_beta_to_0")):
        if on:
            s = m.random_stream(rng)
            getattr(e, name)(*s); getattr(o, name)(*s)


@pytest.mark.parametrize("cfg", ["cfg2", "cfg3_short"])
def test_new_fields_and_init_leave_no_stale_slot(hip, orc, cfg):
    """sweep forward and backward (every slot of the stack is filled and reused), other fields, init, sweep again"""
    m = HubbardModel(**CONFIGS["cfg2"]) if cfg == "cfg2" else HubbardModel(16, 16, 8.0, 1.6, 40, 10)     # N = 64 | N = 256, 4 stack entries
    e, o = m.engine(hip), m.engine(orc)
    rng = np.random.default_rng(5)
    for rnd, seed in enumerate((21, 22)):
        f = m.random_fields(seed)
        e.set_fields(f); e.init(); o.set_fields(f); o.init()
        check(f"{cfg} round {rnd} init", e, o)
        sweep_both(m, rng, e, o)
        check(f"{cfg} round {rnd} sweep", e, o)
    e.close(); o.close()


def test_forward_sweep_directly_after_init_fills_the_slots_by_the_lu_route(hip, orc):
    """init leaves products in the stack (R is no single triangular factor): the first forward sweep finds no valid slot and takes
    the LU route for every X; the backward sweep behind it replaces the entries one by one and reuses none of those."""
    m = HubbardModel(**CONFIGS["cfg2"])
    e, o = m.engine(hip), m.engine(orc)
    f = m.random_fields(77)
    e.set_fields(f); e.init(); o.set_fields(f); o.init()
    rng = np.random.default_rng(6)
    sweep_both(m, rng, e, o, backward=False)
    check("forward after init", e, o)
    sweep_both(m, rng, e, o, forward=False)
    check("backward behind it", e, o)
    sweep_both(m, rng, e, o)
    check("one more sweep", e, o)
    e.close(); o.close()


def test_in_engine_replica_exchange_leaves_no_stale_slot(hip, orc):
    """4 chains of an 8x8 lattice in one engine (at most 8 chains: the stack has slots).  One sweep, then attempt 2 (pairs 0-1, 2-3)
    with u = 0 for chain 0 (accepted) and u = 1 for chain 2 (rejected): chains 0 and 1 get each other's fields and a fresh init under
    a stack whose slots the sweep filled.  Every chain then sweeps on and is compared with an oracle engine of its own that was
    given the chain's fields after the exchange."""
    betas = [2.0, 1.8, 1.6, 1.4]
    L, nt, n_stab = 8, 20, 5
    ms = [HubbardModel(L, L, 4.0, b, nt, n_stab) for b in betas]
    m0 = ms[0]
    e = hip.engine(m0.n, m0.nt, m0.n_stab, [m.g for m in ms], m0.gamma, m0.eta, np.stack([m.expK for m in ms]),
                   np.stack([m.invexpK for m in ms]), n_chains=len(betas))
    e.set_fields(np.stack([m.random_fields(50 + c) for c, m in enumerate(ms)])); e.init()
    rng = np.random.default_rng(9)

    def streams():
        st = [m0.random_stream(rng) for _ in betas]
        return st, tuple(np.stack([x[k] for x in st]) for k in range(3))
    for fn in (e.sweep_0_to_beta, e.sweep_beta_to_0):
        fn(*streams()[1])
    f_before = e.get_fields().copy()
    res = hip.exchange_batch(e, 2, [0.0, np.nan, 1.0, np.nan])
    assert [r.accepted for r in res] == [1, 1, 0, 0]
    f_after = e.get_fields().copy()
    assert np.array_equal(f_after[0], f_before[1]) and np.array_equal(f_after[1], f_before[0])
    os_ = []
    for c, m in enumerate(ms):
        o = m.engine(orc); o.set_fields(f_after[c]); o.init(); os_.append(o)
    for name in ("sweep_0_to_beta", "sweep_beta_to_0", "sweep_0_to_beta", "sweep_beta_to_0"):
        st, batched = streams()
        getattr(e, name)(*batched)
        for c, o in enumerate(os_):
            getattr(o, name)(*st[c])
        G, F = e.get_G(), e.get_fields()
        for c, o in enumerate(os_):
            Go = o.get_G()
            err, scale = float(np.abs(G[c] - Go).max()), max(1.0, float(np.abs(Go).max()))
            print(f"{name} chain {c}: max|dG| = {err:.3e}, max|G| = {scale:.3e}")
            assert np.array_equal(F[c], o.get_fields()), (name, c)
            assert err <= TOL * scale, (name, c, err, scale)
    e.close()
    for o in os_:
        o.close()


@pytest.mark.parametrize("n", [16, 64, 256, 576, 1024])
def test_to_ldr_with_q_accumulated_beside_the_updates(hip, n):
    """orthogonality of L = Q and the reconstruction, at the bounds of test_to_ldr (n = 16 is below the panel family's range and pins
    that the smallest size still factors)"""
    rng = np.random.default_rng(300 + n)
    M = rng.standard_normal((n, n)) * np.exp(rng.uniform(-6, 6, n))[None, :]
    L, d, R = hip.to_ldr(M)
    orth = float(np.abs(L.T @ L - np.eye(n)).max())
    rec = float(np.abs((L * d[None, :]) @ R - M).max())
    col = float((np.abs((L * d[None, :]) @ R - M).max(axis=0) / np.abs(M).max(axis=0)).max())
    print(f"n = {n}: |Q^T Q - I| = {orth:.3e} (bound {1e-13 * n:.1e}), |L d R - M| = {rec:.3e} (bound {1e-13 * n * np.abs(M).max():.1e}), "
          f"column-wise {col:.3e} (bound {1e-12 * n:.1e})")
    assert orth < 1e-13 * n
    assert rec < 1e-13 * n * np.abs(M).max()
    assert col < 1e-12 * n


@pytest.mark.parametrize("cfg", ["cfg2", "cfg3_short"])
def test_backward_stabilisation_leaves_the_transposed_copy_of_g(hip, cfg):
    """every stabilisation of a backward sweep but the last (which ends the sweep: no local update follows) writes GT beside G;
    dqmc_debug_gt_check compares each with an explicit transpose: exactly equal"""
    m = HubbardModel(**CONFIGS["cfg2"]) if cfg == "cfg2" else HubbardModel(16, 16, 8.0, 1.6, 40, 10)
    e = m.engine(hip)
    e.set_fields(m.random_fields(3)); e.init()
    rng = np.random.default_rng(4)
    e.debug_gt_check(True)
    e.sweep_0_to_beta(*m.random_stream(rng)); e.sweep_beta_to_0(*m.random_stream(rng))
    err, checks = e.debug_gt_check(False)
    assert checks == m.n_stack - 1
    assert err.tolist() == [0.0]
    e.sweep_0_to_beta(*m.random_stream(rng)); e.sweep_beta_to_0(*m.random_stream(rng))
    assert e.debug_gt_check(False)[1] == 0                   # switched off: no checks ran
    e.close()
