// gemm_tile.h -- one 16x16 tile of the split-K GEMM (gemm.hip) as a device function.
//
// gemm_splitk_kernel is this body with (i0, j0) taken from blockIdx; the persistent slice kernel (update.hip) runs the same body in
// its flush workgroups for the B-bar product that rides on a slice launch.  One definition, so both give the same bits: the K
// partition per wave, the MFMA order, part[0] + part[1] + part[2] + part[3], then rs, then cs.
#pragma once

#include "common.h"

namespace dq {

// k per wave of the split-K GEMM at size n: a quarter of K rounded up to a multiple of 16.  The one statement of it: the launcher
// (launch_gemm_main, gemm.hip) picks its instance from it and the slice kernel's rider (update.hip) its partition.
__host__ __device__ inline int gemm_splitk_kq(int n) { return ((n + 3) / 4 + 15) / 16 * 16; }

// A 256-thread workgroup (4 waves) computes C[i0 .. i0+15][j0 .. j0+15] of chain `chain`; wave w takes k = w KQ .. w KQ + KQ - 1
// (KQ a multiple of 16, 4 KQ >= n; out-of-range k contributes zeros).  `part` is 8 KiB of LDS, [wave][reg][lane]; the caller puts a
// barrier between two tiles that use the same area.
// kq <= KQ (a multiple of 16, workgroup-uniform): the K partition of the instance <TRANSA, kq> run on this instance's registers -- the
// 16-deep blocks past kq are skipped, loads and MFMAs alike, so the MFMA sequence of every wave and with it every bit of C is that
// instance's.  For a caller that cannot afford one instance per size (the slice kernel's rider); the kernels pass kq = KQ.
template <bool TRANSA, int KQ>
__device__ __forceinline__ void gemm_splitk_tile(const GemmDesc& g, int chain, int i0, int j0, double (*part)[4][64], int kq = KQ) {
    using d4 = __attribute__((ext_vector_type(4))) double;
    const int n = g.n;
    const double* __restrict__ A = g.A.at(chain);
    const double* __restrict__ B = g.B.at(chain);
    double* __restrict__ C = g.C.at(chain);
    const double* __restrict__ ks = g.ks.p ? g.ks.at(chain) : nullptr;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, kk = lane >> 4;
    const int ia = min(i0 + r, n - 1), jb = min(j0 + r, n - 1);      // clamped: loads stay unconditional, results masked
    const bool ia_ok = i0 + r < n, jb_ok = j0 + r < n;
    const int kbeg = wave * kq;
    constexpr int NB = KQ / 16;
    double av[NB][4], bv[NB][4];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if (16 * b >= kq) break;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = kbeg + 16 * b + 4 * kk + s;
            const int kc = min(k, n - 1);
            double a = TRANSA ? A[kc + (long)n * ia] : A[ia + (long)n * kc];
            double bb = B[kc + (long)n * jb];
            if (ks) a *= ks[kc];
            const bool ok = k < n;
            av[b][s] = (ok && ia_ok) ? a : 0.0;
            bv[b][s] = (ok && jb_ok) ? bb : 0.0;
        }
    }
    d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if (16 * b >= kq) break;
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(bv[b][s], av[b][s], acc, 0, 0, 0);
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) part[wave][reg][lane] = acc[reg];
    __syncthreads();
    // wave w finishes accumulator register w: lane holds C[i0 + r][j0 + kk + 4*w]
    const double v4 = part[0][wave][lane] + part[1][wave][lane] + part[2][wave][lane] + part[3][wave][lane];
    const int j = j0 + kk + 4 * wave;
    if (ia_ok && j < n) {
        double v = v4;
        if (g.rs.p) v *= g.rs.at(chain)[i0 + r];
        if (g.cs.p) v *= g.cs.at(chain)[j];
        double* dst = C + (i0 + r) + (long)n * j;
        if (g.accumulate) v += *dst;
        *dst = v;
        if (g.CT.p) g.CT.at(chain)[j + (long)n * (i0 + r)] = v;       // transposed copy for the local-update walk (G -> GT)
    }
}

}  // namespace dq
