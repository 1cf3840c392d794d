"""What drawing the per-slice random stream costs a run, on cfg 3 with 1, 8 and 128 chains per engine:

  (a) host stream drawn inside the timed loop     -- what dqmc_amd/pt_run.py does without --device-rng
  (b) host stream drawn before the clock starts   -- what bench.py's batched figure times; run twice: its spread is the yardstick
  (c) stream drawn on the device (dqmc_rng_seed)  -- nothing drawn on the host, nothing uploaded

wall ms per sweep (both half sweeps of all chains, ending in a synchronise), and the fill kernel's own time by HIP events
(dqmc_rng_fill_time).  All cases run on ONE engine from the same thermalised fields, in the order b, a, c, b.

    python scripts/rng_time.py [--chains 1,8,128] [--sweeps 0 = 20 / 6 / 3 by chain count]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dqmc_amd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", default="1,8,128")
    ap.add_argument("--sweeps", type=int, default=0)
    args = ap.parse_args()
    lib = dqmc_amd.lib()
    if lib.device_count() == 0:
        raise SystemExit("rng_time.py needs a GPU")
    m = dqmc_amd.HubbardModel(**dqmc_amd.CONFIGS["cfg3"])
    f0 = np.load(os.path.join(ROOT, "tests", "golden", "cfg3_therm.npz"))["fields"]
    print(f"cfg 3: {m.L1}x{m.L2}, nt = {m.nt}; {13 * m.nt * m.n / 1e6:.2f} MB of stream per chain and half sweep")
    print(f"{'chains':>6s} {'sweeps':>6s} | {'(b) pre-drawn':>14s} {'(a) in loop':>12s} {'(c) device':>11s} {'(b) again':>10s}  ms per sweep | "
          f"{'(a)-(c)':>8s} {'(c)-min(b)':>10s} {'spread(b)':>9s} | fill kernel ms")
    for C in [int(x) for x in args.chains.split(",")]:
        n_sw = args.sweeps or (20 if C == 1 else 6 if C <= 8 else 3)
        e = m.engine(lib, n_chains=C); e.set_fields(np.stack([f0] * C)); e.init()
        rngs = [np.random.default_rng(1000 + c) for c in range(C)]

        def host_streams():
            s = [m.random_stream(r) for r in rngs]
            return tuple(np.stack([x[i] for x in s]) for i in range(3))

        def timed(draw_in_loop, device):
            pre = None if (draw_in_loop or device) else [(host_streams(), host_streams()) for _ in range(n_sw)]
            e.sync(); t0 = time.perf_counter()
            for k in range(n_sw):
                if device:
                    e.sweep_0_to_beta(); e.sweep_beta_to_0()
                elif draw_in_loop:
                    e.sweep_0_to_beta(*host_streams()); e.sweep_beta_to_0(*host_streams())
                else:
                    e.sweep_0_to_beta(*pre[k][0]); e.sweep_beta_to_0(*pre[k][1])
            e.sync()
            return 1e3 * (time.perf_counter() - t0) / n_sw

        e.rng_seed(2024, first_chain=0)
        e.sweep_0_to_beta(*host_streams()); e.sweep_beta_to_0(); e.sync()           # warm-up of both paths
        b1 = timed(False, False); a = timed(True, False); c = timed(False, True); b2 = timed(False, False)
        fill = e.rng_fill_time(50)
        print(f"{C:6d} {n_sw:6d} | {b1:14.2f} {a:12.2f} {c:11.2f} {b2:10.2f}               | {a - c:8.2f} {c - min(b1, b2):10.2f} {abs(b1 - b2):9.2f} | {fill:.4f}",
              flush=True)
        e.close()


if __name__ == "__main__":
    main()
