"""Replica exchange between the chains of a batched engine (dqmc_replica_exchange_batch, include/dqmc_hip.h).

GPU tests (-m gpu): cfg 4 (16x16, U = 8, Ltau = 200, 8 inverse temperatures) as the 8 chains of ONE engine, and as two
engines of 4 chains exchanging over the callback transport, against an 8-rank OracleTwin (tests/pt_twin.py restates
source/update.cpp:34-117 on CPU-oracle engines) fed with the same generators; then what moves with a swap and what stays
with a chain, and the argument errors.  The two CPU tests check the null-pointer errors without a device."""
import ctypes as C
import os
import re
import subprocess
import sys
import threading

import numpy as np
import pytest

import dqmc_amd
from dqmc_amd import CONFIGS, DqmcError, HubbardModel

from pt_twin import OracleTwin, host_model, ini_text, load_host
from test_replica import PyHub

TOL = 1e-10
CFG4_PT_BETAS = [8.0, 7.9, 7.0, 6.9, 6.0, 5.9, 5.0, 4.9]     # near pairs: probabilistic decisions; far pairs: forced rejections
SEEDS = [1000 + r for r in range(8)]


class BatchedReplicas:
    """`world` replicas of cfg 4 as `ranks` batched engines of world/ranks chains; replica r = rank * C + c holds beta[r] and
    the host generator seeded like OracleTwin's rank r."""

    def __init__(self, hip, h, betas, seeds, ranks):
        cfg = CONFIGS["cfg4"]
        self.L, self.nt, self.n_stab = cfg["L1"], cfg["nt"], cfg["n_stab"]; self.n = self.L * self.L
        self.h, self.world, self.ranks = h, len(betas), ranks
        self.C = self.world // ranks
        ini = ini_text(self.L, cfg["U"], self.nt, self.n_stab)
        mdl = [host_model(h, ini, float(b), int(s), self.n, self.nt) for b, s in zip(betas, seeds)]
        self.rng = [h.dqmc_host_rng_create(int(s)) for s in seeds]
        self.eng = []
        for k in range(ranks):
            ms = mdl[k * self.C:(k + 1) * self.C]
            e = hip.engine(self.n, self.nt, self.n_stab, [m["g"] for m in ms], ms[0]["gamma"], ms[0]["eta"],
                           np.stack([m["expK"] for m in ms]), np.stack([m["invexpK"] for m in ms]), n_chains=self.C)
            e.set_fields(np.stack([m["fields"] for m in ms])); e.init()
            self.eng.append(e)
        self.attempt = 0

    def uniforms(self, rank, attempt):
        """u[c] for the chains of `rank` that decide (lower global index of their pair), NaN elsewhere: only deciders draw."""
        u = np.full(self.C, np.nan)
        for c in range(self.C):
            g = rank * self.C + c
            if g < OracleTwin.partner_rank(g, self.world, attempt):
                u[c] = self.h.dqmc_host_rng_bernoulli_uniform(self.rng[g])
        return u

    def sweep(self):
        """One sweep of every chain with its replica's own stream, drawn as DQMC::draw_half_sweep does (OracleTwin._half_stream)."""
        n, nt = self.n, self.nt
        for forward in (True, False):
            for k, e in enumerate(self.eng):
                perm = np.empty((self.C, nt, n), np.int32); kp = np.empty((self.C, nt, n), np.uint8); u = np.empty((self.C, nt, n))
                for c in range(self.C):
                    for step in range(nt):
                        l = step if forward else nt - 1 - step
                        self.h.dqmc_host_draw_slice(self.rng[k * self.C + c], n, perm[c, l].ctypes.data, kp[c, l].ctypes.data, u[c, l].ctypes.data)
                (e.sweep_0_to_beta if forward else e.sweep_beta_to_0)(perm, kp, u)

    def state(self, g):
        e, c = self.eng[g // self.C], g % self.C
        return dict(fields=e.get_fields()[c], G=e.get_G()[c], logdet=float(e.get_logdet()[c]))

    def close(self):
        for e in self.eng:
            e.close()
        for r in self.rng:
            self.h.dqmc_host_rng_destroy(r)


def _compare(tag, res, ref, br):
    for g in range(br.world):
        a, b = res[g], ref[g]
        assert a.partner == b["partner"] and a.decider == b["decider"], (tag, g, a.partner, a.decider)
        assert bool(a.accepted) == bool(b["accepted"]), (tag, g, a.deltaS, b["deltaS"])
        for got, want in ((a.S, b["S"]), (a.S_prime, b["S_prime"]), (a.S_partner, b["S_partner"]), (a.S_prime_partner, b["S_prime_partner"])):
            assert abs(got - want) <= 1e-8 * max(1.0, abs(want)), (tag, g, got, want)
    _compare_state(tag, br)


def _compare_state(tag, br):
    for g in range(br.world):
        s, o = br.state(g), br.tw.get(g)
        assert np.array_equal(s["fields"], o["fields"]), (tag, g)
        scale = max(1.0, np.abs(o["G"]).max())
        err = np.abs(s["G"] - o["G"]).max()
        assert err <= TOL * scale, (tag, g, err, scale)
        assert abs(s["logdet"] - o["logdet"]) <= 1e-9 * max(1.0, abs(o["logdet"])), (tag, g)


def _run_cfg4(hip, orc, ranks, exchange):
    """Three rounds (odd attempt with the 0 <-> 7 wrap, even, odd), one sweep of every replica, one more round; every round and the
    sweep compared with the 8-rank oracle twin, and at the end the generators (only deciders drew)."""
    h = load_host()
    orc.set_backend("lapack")                                 # MKL dgeqp3 / dgetrf when present (what the reference links); built-in otherwise
    cfg = CONFIGS["cfg4"]
    br = BatchedReplicas(hip, h, CFG4_PT_BETAS, SEEDS, ranks)
    br.tw = OracleTwin(orc, h, ini_text(br.L, cfg["U"], br.nt, br.n_stab), CFG4_PT_BETAS, SEEDS, br.n, br.nt, br.n_stab)
    try:
        _compare_state("initial", br)
        seen = set()
        for rnd in range(4):
            if rnd == 3:
                br.sweep(); br.tw.sweeps(1)
                _compare_state("after a sweep", br)
            br.attempt += 1
            res = exchange(br, br.attempt); ref = br.tw.exchange()
            _compare(f"round {rnd}", res, ref, br)
            seen |= {bool(x["accepted"]) for x in ref}
            if rnd == 0:
                assert res[0].partner == 7 and res[7].partner == 0 and res[0].decider == 1        # the wrap pair, replica 0 decides
        assert seen == {True, False}, "both an accepted and a rejected swap must occur"
        for g in range(br.world):
            assert h.dqmc_host_rng_next(br.rng[g]) == h.dqmc_host_rng_next(br.tw.rng[g]), g
    finally:
        br.tw.close(); br.close(); orc.set_backend("builtin")


@pytest.mark.gpu
def test_cfg4_eight_betas_in_one_batched_engine(hip, orc):
    _run_cfg4(hip, orc, 1, lambda br, a: hip.exchange_batch(br.eng[0], a, br.uniforms(0, a)))


@pytest.mark.gpu
def test_cfg4_two_batched_engines_across_ranks(hip, orc):
    """Two ranks of 4 chains = two threads over the callback transport: odd attempts pair chain 3 of rank 0 with chain 0 of rank 1
    and (the wrap) chain 0 of rank 0 with chain 3 of rank 1."""
    hub = PyHub()

    def exchange(br, attempt):
        out, errs = [None] * 2, []
        us = [br.uniforms(k, attempt) for k in range(2)]

        def run(k):
            try:
                c = hip.comm_callbacks(2, k, hub.endpoint(k))
                out[k] = c.exchange_batch(br.eng[k], attempt, us[k])
                c.close()
            except Exception as e:                      # noqa: BLE001
                errs.append((k, repr(e)))
        th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
        [t.start() for t in th]; [t.join(600) for t in th]
        assert not errs, errs
        return out[0] + out[1]
    _run_cfg4(hip, orc, 2, exchange)


def _small_batch(hip, betas, sweeps=1, seed=7, L=4, nt=20, n_stab=10):
    ms = [HubbardModel(L, L, 4.0, b, nt, n_stab) for b in betas]
    m0 = ms[0]
    e = hip.engine(m0.n, m0.nt, m0.n_stab, [m.g for m in ms], m0.gamma, m0.eta, np.stack([m.expK for m in ms]),
                   np.stack([m.invexpK for m in ms]), n_chains=len(betas))
    e.set_fields(np.stack([m.random_fields(seed + c) for c, m in enumerate(ms)])); e.init()
    rng = np.random.default_rng(seed)
    for _ in range(sweeps):
        for fn in (e.sweep_0_to_beta, e.sweep_beta_to_0):
            st = [m0.random_stream(rng) for _ in betas]
            fn(*(np.stack([x[k] for x in st]) for k in range(3)))
    return ms, e


@pytest.mark.gpu
@pytest.mark.parametrize("L, nt, n_stab", [(4, 20, 10), (6, 10, 5)])
def test_fields_move_and_the_rest_stays_with_the_chain(hip, L, nt, n_stab):
    """4 chains, no communicator, attempt 2 (pairs 0-1, 2-3): chain 0 decides with u = 0 (accepted whatever deltaS is), chain 2
    with u = 1 (rejected whatever deltaS is).  Accepted chains hold the partner's fields with G = a fresh dqmc_init of them at their
    own beta; rejected chains their own fields; stats and measurement bins of every chain do not move.  A chain's configuration is
    nt * n_sites bytes: 320 at 4x4 moves 16 bytes per lane, 360 at 6x6 byte by byte (the two variants of the field kernels)."""
    betas = [2.0, 1.8, 1.6, 1.4]
    ms, e = _small_batch(hip, betas, sweeps=2, L=L, nt=nt, n_stab=n_stab)
    e.measure_accumulate(L, L)
    f0 = e.get_fields().copy(); st0 = [(s.n_accepted, s.n_proposed, s.acc_rate, s.max_err) for s in e.stats()]
    sc0, chi0, cnt0 = e.measure_fetch(L, L, reset=False)
    res = hip.exchange_batch(e, 2, [0.0, np.nan, 1.0, np.nan])
    assert [r.partner for r in res] == [1, 0, 3, 2] and [r.decider for r in res] == [1, 0, 1, 0]
    assert [r.accepted for r in res] == [1, 1, 0, 0]
    f1, G1, ld1 = e.get_fields(), e.get_G(), e.get_logdet()
    for c, p in ((0, 1), (1, 0)):
        assert np.array_equal(f1[c], f0[p])
        fresh = ms[c].engine(hip); fresh.set_fields(f0[p]); fresh.init()
        assert np.abs(G1[c] - fresh.get_G()).max() <= TOL * max(1.0, np.abs(G1[c]).max())
        assert abs(ld1[c] - fresh.get_logdet()) <= 1e-9 * max(1.0, abs(ld1[c]))
        fresh.close()
    for c in (2, 3):
        assert np.array_equal(f1[c], f0[c])
        fresh = ms[c].engine(hip); fresh.set_fields(f0[c]); fresh.init()
        assert np.abs(G1[c] - fresh.get_G()).max() <= TOL * max(1.0, np.abs(G1[c]).max())
        fresh.close()
    assert [(s.n_accepted, s.n_proposed, s.acc_rate, s.max_err) for s in e.stats()] == st0
    sc1, chi1, cnt1 = e.measure_fetch(L, L, reset=False)
    assert cnt1 == cnt0 and np.array_equal(sc1, sc0) and np.array_equal(chi1, chi0)
    # the swapped configurations keep sweeping
    for fn in (e.sweep_0_to_beta, e.sweep_beta_to_0):
        st = [ms[0].random_stream(np.random.default_rng(3)) for _ in betas]
        fn(*(np.stack([x[k] for x in st]) for k in range(3)))
    e.sync(); e.close()


@pytest.mark.gpu
def test_argument_errors_leave_the_fields_untouched(hip):
    ms, e = _small_batch(hip, [2.0, 1.8, 1.6], sweeps=0)
    f0 = e.get_fields().copy()
    with pytest.raises(DqmcError) as ei:                      # 3 replicas: W odd
        hip.exchange_batch(e, 1, np.zeros(3))
    assert ei.value.code == -1 and "even" in str(ei.value)
    res = (dqmc_amd.ExchangeResult * 3)()
    assert hip._sym("replica_exchange_batch")(e._h, None, 1, None, res) == -1          # u NULL
    assert "uniform" in hip._sym("last_error")().decode()
    assert np.array_equal(e.get_fields(), f0)
    e.close()
    one = ms[0].engine(hip, n_chains=1); one.set_fields(f0[:1]); one.init()
    with pytest.raises(DqmcError) as ei:                      # one chain, no communicator
        hip.exchange_batch(one, 1, np.zeros(1))
    assert ei.value.code == -1
    one.close()


def _ranks_refuse(hip, chains, attempt, refuse=None):
    """len(chains) ranks (threads over the callback transport), rank k a batched engine of chains[k] chains; rank `refuse` passes a
    NULL u.  Returns (error code, message) of every rank ((None, "") when the round ran) and whether every engine kept its fields.
    A rank left waiting for a message that never comes gets the hub's time-out as a callback failure, with another message."""
    R = len(chains)
    engs = [_small_batch(hip, [2.0 - 0.05 * (k * 8 + c) for c in range(ck)], sweeps=0, seed=11 + k)[1] for k, ck in enumerate(chains)]
    before = [x.get_fields().copy() for x in engs]
    hub = PyHub(); codes = [("hung", "")] * R

    def run(k):
        c = hip.comm_callbacks(R, k, hub.endpoint(k))
        try:
            if k == refuse:
                res = (dqmc_amd.ExchangeResult * engs[k].C)()
                rc = hip._sym("replica_exchange_batch")(engs[k]._h, c._h, attempt, None, res)
                codes[k] = (rc, hip._sym("last_error")().decode()) if rc else (None, "")
            else:
                c.exchange_batch(engs[k], attempt, np.zeros(engs[k].C)); codes[k] = (None, "")
        except DqmcError as ex:
            codes[k] = (ex.code, str(ex))
        c.close()
    th = [threading.Thread(target=run, args=(k,), daemon=True) for k in range(R)]
    [t.start() for t in th]; [t.join(120) for t in th]
    kept = all(np.array_equal(x.get_fields(), b) for x, b in zip(engs, before))
    for x in engs:
        x.close()
    return codes, kept


@pytest.mark.gpu
@pytest.mark.parametrize("chains, attempt", [((2, 3), 1), ((2, 3), 2), ((2, 4), 1), ((2, 4), 2), ((2, 2, 4), 1), ((2, 2, 4), 2)])
def test_ranks_with_different_chain_counts_all_refuse(hip, chains, attempt):
    """Ranks whose C differ would pair replicas differently (world = ranks * own C): every rank must return DQMC_EINVAL before any
    field moves, whatever the attempt's pairing, also a rank whose neighbours both hold its own C (ranks 0 and 1 of (2, 2, 4))."""
    codes, kept = _ranks_refuse(hip, chains, attempt)
    assert all(code == -1 and "same number of chains" in msg for code, msg in codes), codes
    assert kept


@pytest.mark.gpu
def test_a_refusing_rank_makes_every_rank_refuse(hip):
    """Rank 1 passes a NULL u: it refuses, and rank 0 (whose arguments are fine) refuses with it instead of waiting for rank 1."""
    codes, kept = _ranks_refuse(hip, (2, 2), 1, refuse=1)
    assert codes[0][0] == -1 and "refused its arguments" in codes[0][1], codes
    assert codes[1][0] == -1 and "uniform" in codes[1][1], codes
    assert kept


@pytest.mark.gpu
def test_communicator_on_another_device_is_refused(hip):
    if hip.device_count() < 2:
        pytest.skip("needs two GPUs: an RCCL communicator on device 1 next to an engine on device 0")
    ms, e = _small_batch(hip, [2.0, 1.8], sweeps=0)
    f0 = e.get_fields().copy()
    c = hip.comm_rccl(hip.comm_unique_id(), 1, 0, 1)
    with pytest.raises(DqmcError) as ei:
        c.exchange_batch(e, 1, np.zeros(2))
    assert ei.value.code == -1 and "different devices" in str(ei.value)
    assert np.array_equal(e.get_fields(), f0)
    c.close(); e.close()


def test_null_engine_or_results_is_einval_without_a_device():
    lib = dqmc_amd.lib()
    fn = lib._sym("replica_exchange_batch")
    u = np.zeros(2)
    res = (dqmc_amd.ExchangeResult * 2)()
    assert fn(None, None, 1, u.ctypes.data_as(C.POINTER(C.c_double)), res) == -1
    assert "null" in lib._sym("last_error")().decode()
    assert fn(C.c_void_p(1), None, 1, u.ctypes.data_as(C.POINTER(C.c_double)), None) == -1     # checked before the engine is touched
    assert "null" in lib._sym("last_error")().decode()


def test_batch_symbol_is_bound():
    lib = dqmc_amd.lib()
    assert "replica_exchange_batch" in dqmc_amd.ABI_SYMBOLS and lib.has_symbol("replica_exchange_batch")
    assert lib._sym("replica_exchange_batch").argtypes[3] is C.POINTER(C.c_double)


@pytest.mark.gpu
def test_pt_run_with_four_replicas_per_gpu(hip):
    """dqmc_amd/pt_run.py --replicas-per-gpu 4 as one process: one batched engine holds the four betas, no communicator.  A child
    process, because pt_run imports torch, whose wheel brings its own HIP runtime next to the one this library links (the suite keeps
    torch out of its own process, as test_gpu_replica.py does for the RCCL loopback)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(root, "dqmc_amd", "pt_run.py"), "--betas", "2.0,1.9,1.8,1.7", "--L", "4", "--U", "4.0",
                          "--nt", "20", "--n-stab", "10", "--therm", "1", "--sweeps", "6", "--sweep-steps", "2", "--replicas-per-gpu", "4"],
                         capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    m = re.search(r"PT: 4 replicas = 1 rank\(s\) x 4 chains over one engine, 6 sweeps .* \((\d+)/(\d+)\)", out.stdout)
    assert m and int(m.group(2)) == 3 and 0 <= int(m.group(1)) <= 3, out.stdout
