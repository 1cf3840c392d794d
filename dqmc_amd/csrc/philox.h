// philox.h -- the counter-based random stream of a seeded engine (dqmc_rng_seed, include/dqmc_hip.h), element by element.
//
// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) with the standard
// constants.  Plain C++ without any HIP type, so the fill kernel (rng.hip) and the host library (host_capi.cpp: the CPU
// suite checks the known answers and the draws against tests/rng_ref.py) compile the very same text.
//
// With engine seed S, chain id g = first_chain + c, half-sweep counter h, time slice l and n sites:
//   key                 (S & 0xffffffff, S >> 32)
//   proposal  idx of l  counter (idx, l, h, g) -> x0..x3:   u = ((x0 >> 5) 2^26 + (x1 >> 6)) 2^-53  in [0, 1) on a 2^-53 grid,
//                       kprop = (x2 * 3) >> 32 (64-bit product; the three values differ in probability by at most 2^-32),
//                       x3 unused
//   site      i   of l  counter (i, l | 0x80000000, h, g) -> key64 = x0 << 32 | x1;  perm[l][.] = the sites sorted
//                       ascending by (key64, i): a uniform permutation, the index breaks ties (probability ~ n^2 2^-65)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DQ_HD __host__ __device__ __forceinline__
#else
#define DQ_HD inline
#endif

namespace dq {

struct Philox4 { uint32_t x[4]; };

DQ_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += W0; k1 += W1;
    }
    return Philox4{{c0, c1, c2, c3}};
}

constexpr uint32_t RNG_PERM_BIT = 0x80000000u;

// the proposal draw of position idx in the visiting order of slice l
DQ_HD void rng_proposal(uint64_t seed, uint32_t g, uint32_t h, uint32_t l, uint32_t idx, double* u, uint8_t* kprop) {
    const Philox4 r = philox4x32_10(idx, l, h, g, (uint32_t)seed, (uint32_t)(seed >> 32));
    *u = ((double)(r.x[0] >> 5) * 67108864.0 + (double)(r.x[1] >> 6)) * (1.0 / 9007199254740992.0);
    *kprop = (uint8_t)(((uint64_t)r.x[2] * 3u) >> 32);
}

// the sort key of site i in slice l
DQ_HD uint64_t rng_perm_key(uint64_t seed, uint32_t g, uint32_t h, uint32_t l, uint32_t i) {
    const Philox4 r = philox4x32_10(i, l | RNG_PERM_BIT, h, g, (uint32_t)seed, (uint32_t)(seed >> 32));
    return ((uint64_t)r.x[0] << 32) | r.x[1];
}

}  // namespace dq
