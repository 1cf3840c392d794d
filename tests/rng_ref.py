"""Numpy restatement of the random stream a seeded engine draws on the device (include/dqmc_hip.h, dqmc_rng_seed).

Philox4x32-10 with the standard constants, vectorised over counters, and ``stream(seed, g, h, nt, n)``: the (perm, kprop, u) of
half-sweep counter ``h`` for stream id ``g``, bit for bit what ``Engine.rng_draw`` returns for the chain with that id.
"""
from __future__ import annotations

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four arrays (or scalars) of 32-bit words, key: two 32-bit integers -> four uint32 arrays."""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, dtype=np.uint64)) & MASK for c in np.broadcast_arrays(*counter))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                       # 32 x 32 -> 64 bit: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c3 ^ np.uint64(k1), p0 & MASK
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def stream(seed: int, g: int, h: int, nt: int, n: int):
    """(perm int32, kprop uint8, u float64), each (nt, n), of engine seed `seed`, stream id `g`, half-sweep counter `h`."""
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    l, i = np.meshgrid(np.arange(nt, dtype=np.uint64), np.arange(n, dtype=np.uint64), indexing="ij")
    hh, gg = np.full_like(l, h), np.full_like(l, g)
    x0, x1, x2, _ = (x.reshape(nt, n).astype(np.uint64) for x in philox4x32_10((i.ravel(), l.ravel(), hh.ravel(), gg.ravel()), key))
    u = ((x0 >> np.uint64(5)) * np.uint64(1 << 26) + (x1 >> np.uint64(6))).astype(np.float64) * 2.0 ** -53
    kprop = ((x2 * np.uint64(3)) >> S32).astype(np.uint8)
    y0, y1, _, _ = (x.reshape(nt, n).astype(np.uint64)
                    for x in philox4x32_10((i.ravel(), (l | np.uint64(0x80000000)).ravel(), hh.ravel(), gg.ravel()), key))
    key64 = (y0 << S32) | y1
    sites = np.arange(n)
    perm = np.stack([np.lexsort((sites, key64[row])) for row in range(nt)]).astype(np.int32)      # ascending by (key64, site)
    return perm, kprop, u
