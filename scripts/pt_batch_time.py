"""Parallel tempering on one GPU, two ways (DESIGN.md section "Replica exchange inside a batched engine"): W inverse temperatures
at cfg-4 size (16x16, U = 8, Ltau = 200) as the W chains of ONE batched engine exchanging with dqmc_replica_exchange_batch, against
W single-chain engines driven by W host threads (HostPT: sweeps concurrently, rounds through update::replica_exchange).  Prints
aggregate replica sweeps/s and milliseconds per exchange round of each, one JSON line per measurement.

    python scripts/pt_batch_time.py [--betas 8|32] [--sweeps 4] [--rounds 6] [--mode both|batched|threads]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/pt_batch_time.py --mode batched --sweeps 0 --rounds 4
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dqmc_amd                                            # noqa: E402
from pt_twin import HostPT, host_model, ini_text, load_host   # noqa: E402

L, U, NT, NS = 16, 8.0, 200, 10
N = L * L


def betas_for(w):
    if w == 8:
        return [8.0, 7.9, 7.0, 6.9, 6.0, 5.9, 5.0, 4.9]
    return [float(b) for b in np.linspace(8.0, 2.0, w)]


def batched(lib, h, betas, seeds, sweeps, rounds):
    W = len(betas); ini = ini_text(L, U, NT, NS)
    ms = [host_model(h, ini, b, s, N, NT) for b, s in zip(betas, seeds)]
    e = lib.engine(N, NT, NS, [m["g"] for m in ms], ms[0]["gamma"], ms[0]["eta"], np.stack([m["expK"] for m in ms]),
                   np.stack([m["invexpK"] for m in ms]), n_chains=W)
    e.set_fields(np.stack([m["fields"] for m in ms]))
    t = time.perf_counter(); e.init(); t_init = time.perf_counter() - t
    rng = np.random.default_rng(5)
    out = dict(mode="batched", replicas=W, init_ms=1e3 * t_init)

    def sweep():
        for fn in (e.sweep_0_to_beta, e.sweep_beta_to_0):
            st = [rng.permutation(N) for _ in range(W * NT)]
            fn(np.stack(st).reshape(W, NT, N).astype(np.int32), rng.integers(0, 3, size=(W, NT, N), dtype=np.uint8), rng.random((W, NT, N)))
    if sweeps:
        sweep(); e.sync()
        t = time.perf_counter()
        for _ in range(sweeps):
            sweep()
        e.sync()
        dt = time.perf_counter() - t
        out.update(sweeps=sweeps, replica_sweeps_per_s=W * sweeps / dt, ms_per_sweep=1e3 * dt / sweeps)
    times, second = [], 0
    for a in range(1, rounds + 1):
        u = rng.random(W)
        t = time.perf_counter(); res = lib.exchange_batch(e, a, u); times.append(time.perf_counter() - t)
        second += int(any(not r.accepted for r in res))
    if rounds:
        out.update(rounds=rounds, ms_per_round=1e3 * float(np.mean(times)), ms_per_round_min=1e3 * float(np.min(times)),
                   rounds_with_second_init=second)
    e.close()
    return out


def threads(h, betas, seeds, sweeps, rounds):
    W = len(betas)
    pt = HostPT(h, ini_text(L, U, NT, NS), betas, seeds)
    out = dict(mode="threads", replicas=W)
    try:
        if sweeps:
            pt.sweeps(1, concurrently=True)
            t = time.perf_counter(); pt.sweeps(sweeps, concurrently=True); dt = time.perf_counter() - t
            out.update(sweeps=sweeps, replica_sweeps_per_s=W * sweeps / dt, ms_per_sweep=1e3 * dt / sweeps)
        times = []
        for _ in range(rounds):
            t = time.perf_counter(); pt.exchange(); times.append(time.perf_counter() - t)
        if rounds:
            out.update(rounds=rounds, ms_per_round=1e3 * float(np.mean(times)), ms_per_round_min=1e3 * float(np.min(times)))
    finally:
        pt.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--betas", type=int, default=8)
    ap.add_argument("--sweeps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--mode", default="both", choices=["both", "batched", "threads"])
    args = ap.parse_args()
    lib = dqmc_amd.lib(); h = load_host()
    betas = betas_for(args.betas); seeds = [1000 + r for r in range(len(betas))]
    rows = []
    if args.mode in ("both", "batched"):
        rows.append(batched(lib, h, betas, seeds, args.sweeps, args.rounds))
    if args.mode in ("both", "threads"):
        rows.append(threads(h, betas, seeds, args.sweeps, args.rounds))
    for r in rows:
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
