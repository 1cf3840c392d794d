// rng.hip -- the random stream of one half sweep drawn on the device (dqmc_rng_seed, include/dqmc_hip.h).
//
// The host path (update::draw_slice_stream + Engine::upload_stream) draws perm / kprop / u of every slice with the reference's
// generator and uploads 13 bytes per proposal.  A seeded engine fills the same three buffers with ONE launch per half sweep from
// (seed, chain id, half-sweep counter): a counter-based generator (Philox4x32-10, philox.h, which also states the stream) needs no
// state in memory, so any element can be drawn by any thread and the chain's position is three integers.
//
// rng_fill_kernel<NP>: grid = (nt, chains), one workgroup per slice and chain, NP = the sites padded to a power of two (64 .. 1024)
// threads.  Thread t draws the proposal of position t (u, kprop: coalesced stores) and the sort key of site t, then the workgroup
// sorts the NP records (key64, site) ascending, lexicographically, with a bitonic network: thread t holds record t in registers
// throughout and only ever needs its partner's, t ^ j.
//   j < 64   the partner is in the same wave: three ds_bpermute shuffles, no LDS memory, no barrier
//   j >= 64  through LDS, double-buffered on the stage parity, so ONE LDS-only barrier per stage (a record written in stage s is
//            overwritten in stage s + 2 at the earliest, and every reader of stage s has passed the barrier of stage s + 1 by then)
// Padding records carry (2^64 - 1, t >= n): behind every real record under the lexicographic rule, whatever its key.  After the
// last stage thread t < n holds the site visited at position t.  n <= 64 is a single wave without any barrier.  No scratch, no
// dynamically indexed register arrays (the records are scalars); 24 KiB of LDS at NP = 1024 (scripts/kernel_regs.py).
#include "common.h"
#include "philox.h"

namespace dq {

namespace {

__device__ __forceinline__ void lds_barrier_only() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// keep the smaller (take_min) or the larger of the own record (k, i) and the partner's (pk, pi); records are distinct (i is)
__device__ __forceinline__ void keep(uint64_t& k, uint32_t& i, uint64_t pk, uint32_t pi, bool take_min) {
    const bool partner_less = pk < k || (pk == k && pi < i);
    if (partner_less == take_min) { k = pk; i = pi; }
}

template <int NP>
__global__ __launch_bounds__(NP) void rng_fill_kernel(int32_t* __restrict__ perm, uint8_t* __restrict__ kprop, double* __restrict__ u,
                                                      int n, int nt, uint64_t seed, uint32_t first_chain, uint32_t h) {
    constexpr int NX = NP > 64 ? NP : 1;                             // records that cross waves
    __shared__ uint64_t xk[2][NX];
    __shared__ uint32_t xi[2][NX];
    const uint32_t t = threadIdx.x, l = blockIdx.x, c = blockIdx.y, g = first_chain + c;
    const size_t row = ((size_t)c * nt + l) * (size_t)n;             // [c][l][.] of the three [chains][nt][n] arrays
    const bool live = t < (uint32_t)n;

    uint64_t key = ~0ull; uint32_t site = t;
    if (live) {
        double uu; uint8_t kk;
        rng_proposal(seed, g, h, l, t, &uu, &kk);
        u[row + t] = uu; kprop[row + t] = kk;
        key = rng_perm_key(seed, g, h, l, t);
    }

    int stage = 0;
#pragma unroll
    for (int k = 2; k <= NP; k <<= 1) {
        const bool ascending = (t & k) == 0;
#pragma unroll
        for (int j = k >> 1; j >= 1; j >>= 1) {
            uint64_t pk; uint32_t pi;
            if (j >= 64) {
                const int b = stage & 1; ++stage;
                xk[b][t] = key; xi[b][t] = site;
                lds_barrier_only();
                pk = xk[b][t ^ j]; pi = xi[b][t ^ j];
            } else {
                const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)key, j, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(key >> 32), j, 64);
                pk = ((uint64_t)hi << 32) | lo; pi = (uint32_t)__shfl_xor((int)site, j, 64);
            }
            keep(key, site, pk, pi, ((t & j) == 0) == ascending);
        }
    }
    if (live) perm[row + t] = (int32_t)site;
}

}  // namespace

int launch_rng_fill(int32_t* perm, uint8_t* kprop, double* u, int n, int nt, unsigned long long seed, unsigned first_chain, unsigned h,
                    int n_chains, hipStream_t s) {
    if (n < 1 || n > 1024 || nt < 1 || n_chains < 1) { set_error("rng fill: n_sites in 1 .. 1024"); return -1; }
    const dim3 grid((unsigned)nt, (unsigned)n_chains);
#define DQ_RNG_FILL(NP) hipLaunchKernelGGL(rng_fill_kernel<NP>, grid, dim3(NP), 0, s, perm, kprop, u, n, nt, (uint64_t)seed, (uint32_t)first_chain, (uint32_t)h)
    if (n <= 64) DQ_RNG_FILL(64);
    else if (n <= 128) DQ_RNG_FILL(128);
    else if (n <= 256) DQ_RNG_FILL(256);
    else if (n <= 512) DQ_RNG_FILL(512);
    else DQ_RNG_FILL(1024);
#undef DQ_RNG_FILL
    DQ_HIP(hipGetLastError());
    return 0;
}

}  // namespace dq
