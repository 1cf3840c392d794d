// lu_gj.hip -- X = A^-1 B for n <= 1024 (the arma::solve(M, RHS) of
// stablelinalg::inv_I_plus_ldr_mul_ldr / inv_invldr_plus_ldr / inv_I_plus_ldr,
// source/stablelinalg.cpp:122-125,153-155,184-186) as a blocked Gauss-Jordan
// elimination with partial pivoting, two launches per panel of 32 columns and
// no substitution phase at all:
//
//   gj_panel_kernel   (n <= 64; gj_panel_mw_kernel<NW, RPL> above that: NW waves x RPL rows per lane, one LDS barrier per step, see there)
//                     ONE wave per chain.  Lane owns rows lane, lane+64, ... of the panel in
//                     registers and runs dgetf2 on the live rows (pivot search = per-lane max +
//                     32-bit DPP wave maxima + ballot, pivot row broadcast by v_readlane into
//                     SGPRs: no LDS, no barrier, no memory access in the step loop).  A is NOT
//                     modified: the kernel emits the pivot rows S of the panel, log|det| of the
//                     pivot block P11 = L11 U11, the block itself and the inverses of its four
//                     16 x 16 diagonal triangles (one column per lane).
//   gj_update_kernel  whole chip, fp64 MFMA.  Every wave forms, for its 16 columns,
//                     U12 = U11^-1 (L11^-1 A[S, cols]) by block substitution on the matrix cores (the pivot rows
//                     are read-only in this launch) and subtracts A[r, panel] U12 from every
//                     other row r -- the live rows of A and B, and the rows retired by earlier
//                     panels.  Retired rows live in pivot order in SA | X, so that after the
//                     last panel A has become the identity in that order and X holds the
//                     solution in natural row order: no row permutation, no triangular solves.
//
// The Schur complements are those of dgetrf with the same pivot choice inside a panel
// (A22 - A21 P11^-1 A12); against dgetrf + dgetrs the result differs at rounding level
// (measured on the cfg-3 stabilisation matrices, cond(M) ~ 1e3: 1e-13 .. 9e-13 on G, the same
// spread two LAPACK routes show among themselves).  For n = 256: 8 x (panel 13 us + update
// 8 us) instead of the 8 x (30 + 18 + 7) us of lu_blocked.hip plus a ~200 us substitution.
//
//   gj_step_kernel    (64 < n <= 256, the default for 128 < n <= 256) the two in ONE launch per panel: the update's grid, every workgroup of which factors the panel itself
//                     with the panel kernel's device functions and keeps the pivot block, its inverses, perm and the new rowpos in LDS; the
//                     same bits as the two launches (DQMC_GJ_FUSED=0 keeps those; tests/test_gpu_fused_gj.py).
#include "common.h"
#include "wave.h"
#include <cstdlib>
#include <type_traits>
#include <utility>

namespace dq {

namespace {
constexpr int GJ_NB = 32;
using d4 = __attribute__((ext_vector_type(4))) double;

__device__ __forceinline__ void lds_wait() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// One elimination step of the panel, J a compile-time constant so that every register index is static (a rolled
// step loop would put the panel into scratch).  No LDS and no memory traffic: the pivot search is a per-lane max
// over the lane's rows, two 32-bit DPP wave maxima (high word of |a|, then low word among the lanes that tie) and a
// ballot; the pivot row reaches the other lanes through v_readlane into SGPRs, which the FMAs take as operands.
template <int NR, int J>
__device__ __forceinline__ void gj_step(double (&a)[NR][GJ_NB], bool (&live)[NR], int (&mypos)[NR], int& myperm, bool& singular, int lane, int k0) {
    unsigned long long best = 0ULL; int bq = -1;
#pragma unroll
    for (int q = 0; q < NR; ++q) {
        const unsigned long long kq = live[q] ? ((unsigned long long)__double_as_longlong(fabs(a[q][J])) | 1ULL) : 0ULL;   // live rows have a nonzero key
        if (kq > best) { best = kq; bq = q; }             // strict: the lowest row of the lane wins a tie
    }
    const unsigned hi = (unsigned)(best >> 32), lo = (unsigned)best;
    const unsigned m1 = wave_max_u32(hi);
    const unsigned m2 = wave_max_u32(hi == m1 ? lo : 0u);
    const unsigned long long winners = __ballot(hi == m1 && lo == m2 && bq >= 0);
    const int pl = winners ? (int)__builtin_ctzll(winners) : 0;             // winners == 0 only when no live row is left (n < k0 + J + 1: excluded by the caller)
    const int pq = __builtin_amdgcn_readlane(bq, pl);
    if (lane == J) myperm = pl + 64 * pq;
    double prow[GJ_NB - J];
#pragma unroll
    for (int q = 0; q < NR; ++q) {
        if (q == pq) {                                    // wave-uniform
#pragma unroll
            for (int c = J; c < GJ_NB; ++c) prow[c - J] = readlane_f64(a[q][c], pl);
        }
    }
#pragma unroll
    for (int q = 0; q < NR; ++q)
        if (q == pq && lane == pl) { live[q] = false; mypos[q] = k0 + J; }
    const double piv = prow[0];
    singular = singular || !(fabs(piv) > 0.0);
    // reciprocal pivot (dgetf2 scales by the reciprocal as well): v_rcp_f64 + two Newton steps, no div_scale / div_fixup
    double r = __builtin_amdgcn_rcp(piv);
    r = fma(fma(-piv, r, 1.0), r, r);
    r = fma(fma(-piv, r, 1.0), r, r);
#pragma unroll
    for (int q = 0; q < NR; ++q) {
        if (live[q]) {
            const double l = a[q][J] * r;
            a[q][J] = l;
#pragma unroll
            for (int c = J + 1; c < GJ_NB; ++c) a[q][c] = fma(-l, prow[c - J], a[q][c]);
        }
    }
}
template <int NR, int J>
struct GjSteps {
    static __device__ __forceinline__ void run(double (&a)[NR][GJ_NB], bool (&live)[NR], int (&mypos)[NR], int& myperm, bool& singular, int lane, int nbw, int k0) {
        if (J < nbw) gj_step<NR, J>(a, live, mypos, myperm, singular, lane, k0);      // wave-uniform
        GjSteps<NR, J + 1>::run(a, live, mypos, myperm, singular, lane, nbw, k0);
    }
};
template <int NR>
struct GjSteps<NR, GJ_NB> {
    static __device__ __forceinline__ void run(double (&)[NR][GJ_NB], bool (&)[NR], int (&)[NR], int&, bool&, int, int, int) {}
};
}  // namespace

// tinv: per chain 2048 doubles: [0, 1024) the pivot block LU[j][c] row-major in pivot order (L11 strictly below, U11 on and
// above the diagonal), then the four 16 x 16 triangular inverses, column-major: L11[0:16,0:16]^-1, L11[16:32,16:32]^-1,
// U11[0:16,0:16]^-1, U11[16:32,16:32]^-1.  Rows / columns >= nbw are the identity.
template <int NR>
__global__ __launch_bounds__(64) void gj_panel_kernel(CMat Am, int* rowpos_p, long rowpos_stride, int* perm_p, long perm_stride, double* tinv_p,
                                                      double* logabsdet, int accumulate, int* info, int n, int k0) {
    __shared__ __attribute__((aligned(16))) double LU[GJ_NB][GJ_NB];
    const int chain = blockIdx.y;
    const double* __restrict__ A = Am.at(chain);
    int* rowpos = rowpos_p + (long)chain * rowpos_stride;
    int* perm = perm_p + (long)chain * perm_stride;
    double* tinv = tinv_p + (long)chain * 2 * GJ_NB * GJ_NB;
    const int lane = threadIdx.x;
    const int nbw = min(GJ_NB, n - k0);

    bool live[NR]; int mypos[NR];
    double a[NR][GJ_NB];
#pragma unroll
    for (int q = 0; q < NR; ++q) {
        const int r = lane + 64 * q;
        live[q] = r < n && (k0 == 0 ? true : rowpos[r] < 0);
        mypos[q] = -1;
#pragma unroll
        for (int c = 0; c < GJ_NB; ++c) a[q][c] = (live[q] && c < nbw) ? A[r + (long)n * (k0 + c)] : 0.0;
    }
    for (int e = lane; e < GJ_NB * GJ_NB; e += 64) (&LU[0][0])[e] = ((e >> 5) == (e & 31)) ? 1.0 : 0.0;   // identity padding for nbw < 32
    int myperm = 0; bool singular = false;

    GjSteps<NR, 0>::run(a, live, mypos, myperm, singular, lane, nbw, k0);

    lds_wait();                                          // the identity fill is in LDS before the pivot rows overwrite theirs
#pragma unroll
    for (int q = 0; q < NR; ++q) {
        const int r = lane + 64 * q;
        if (r < n) { if (k0 == 0) rowpos[r] = mypos[q]; else if (mypos[q] >= 0) rowpos[r] = mypos[q]; }
        if (mypos[q] >= 0) {                             // a pivot row: untouched since its step, L11[j][:j] | U11[j][j:]
            double* dst = &LU[mypos[q] - k0][0];
#pragma unroll
            for (int c = 0; c < GJ_NB; c += 2) *reinterpret_cast<double2*>(dst + c) = make_double2(a[q][c], a[q][c + 1]);
        }
    }
    if (lane < nbw) perm[k0 + lane] = myperm;
    lds_wait();
#pragma unroll
    for (int e = 0; e < GJ_NB * GJ_NB / 64; ++e) tinv[lane + 64 * e] = (&LU[0][0])[lane + 64 * e];
    {                                                    // log|det P11| and singularity check
        const double pv = lane < nbw ? fabs(LU[lane][lane]) : 1.0;
        const double ls = wave_sum(log(pv));
        if (lane == 0) {
            if (logabsdet) logabsdet[chain] = ((accumulate || k0 > 0) ? logabsdet[chain] : 0.0) + ls;
            if (info && (singular || !(ls == ls))) atomicOr(info, DQ_STATUS_PIVOT);
        }
    }
    // The four 16 x 16 triangular inverses, one column per lane (lane = 16 * block + column): unit-lower blocks by forward
    // substitution, upper blocks by the same recurrence on the index-reversed block.
    {
        const int blk = lane >> 4, c = lane & 15;
        const bool up = blk >= 2;
        const int base = (blk & 1) * 16;
        const double* T0 = &LU[0][0] + (up ? (base + 15) * 33 : base * 33);
        const int sg = up ? -1 : 1;
        const int cc = up ? 15 - c : c;                  // position of the unit vector's 1 in recurrence order
        double x[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            double s0 = (j == cc) ? 1.0 : 0.0, s1 = 0.0;
#pragma unroll
            for (int m = 0; m < j; ++m) {
                const double t = T0[sg * (j * 32 + m)];
                if (m & 1) s1 = fma(-t, x[m], s1); else s0 = fma(-t, x[m], s0);
            }
            const double s = s0 + s1;
            x[j] = up ? s / T0[sg * (j * 33)] : s;
        }
        double* out = tinv + GJ_NB * GJ_NB + 256 * blk + 16 * c;
#pragma unroll
        for (int j = 0; j < 16; ++j) out[up ? 15 - j : j] = x[j];
    }
}

// After a multi-wave panel, one wave each: log|det P11| with the singularity flag, and the four 16 x 16 triangular inverses of the pivot block
// (4 us when wave 0 did both, each upper-block step ending in an fp64 division: the sixteen reciprocals are formed once, in parallel).
__device__ __forceinline__ void gj_panel_logdet(double (&LU)[GJ_NB][GJ_NB], double* logabsdet, int accumulate, int* info, int chain, int lane, int nbw, int k0, int s_sing) {
    const double pv = lane < nbw ? fabs(LU[lane][lane]) : 1.0;
    const double ls = wave_sum(log(pv));
    if (lane == 0) {
        if (logabsdet) logabsdet[chain] = ((accumulate || k0 > 0) ? logabsdet[chain] : 0.0) + ls;
        if (info && (s_sing || !(ls == ls))) atomicOr(info, DQ_STATUS_PIVOT);
    }
}
template <int... Js>
__device__ __forceinline__ void gj_tri_steps(double (&x)[16], const double* T0, int sg, int cc, bool up, bool hi, double rd, std::integer_sequence<int, Js...>) {
    auto step = [&](auto jc) {
        constexpr int j = decltype(jc)::value;
        double s0 = (j == cc) ? 1.0 : 0.0, s1 = 0.0;
#pragma unroll
        for (int m = 0; m < j; ++m) {
            const double tt = T0[sg * (j * 32 + m)];
            if (m & 1) s1 = fma(-tt, x[m], s1); else s0 = fma(-tt, x[m], s0);
        }
        const double s = s0 + s1;
        // 1 / U[base + 15 - j][base + 15 - j] sits in lane base + 15 - j (base = 0 or 16)
        const double r0 = readlane_f64(rd, 15 - j), r1 = readlane_f64(rd, 31 - j);
        x[j] = up ? s * (hi ? r1 : r0) : s;
    };
    (step(std::integral_constant<int, Js>{}), ...);
}
// inv: 4 x (16 x 16) column-major, in global memory or in LDS
__device__ __forceinline__ void gj_panel_tri_inverses(double (&LU)[GJ_NB][GJ_NB], double* inv, int lane) {
    // one column per lane (lane = 16 * block + column): unit-lower blocks by forward substitution, upper blocks by the same recurrence on
    // the index-reversed block
    const int blk = lane >> 4, c = lane & 15;
    const bool up = blk >= 2;
    const int base = (blk & 1) * 16;
    const double* T0 = &LU[0][0] + (up ? (base + 15) * 33 : base * 33);
    const int sg = up ? -1 : 1;
    const int cc = up ? 15 - c : c;
    const double rd = 1.0 / LU[lane & 31][lane & 31];
    double x[16];
    gj_tri_steps(x, T0, sg, cc, up, (blk & 1) != 0, rd, std::make_integer_sequence<int, 16>{});
    double* out = inv + 256 * blk + 16 * c;
#pragma unroll
    for (int j = 0; j < 16; ++j) out[up ? 15 - j : j] = x[j];
}

#ifdef DQ_GJ_STAMPS
#ifndef DQ_GJ_STAMP_K0
#define DQ_GJ_STAMP_K0 0         // the panel whose clocks the stamp build prints (-DDQ_GJ_STAMP_K0=192: a compacted one at n = 256)
#endif
// diagnostic build only (scripts/gj_stamps.py): where a step's time goes; s_memtime counts 100 MHz ticks
#define GST(i) { unsigned long long t_; asm volatile("s_waitcnt lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); gst[i] += t_ - gprev; gprev = t_; }
#define GST_ARGS , unsigned long long (&gst)[8], unsigned long long& gprev
#define GST_PASS , gst, gprev
#else
#define GST(i)
#define GST_ARGS
#define GST_PASS
#endif
// ---- multi-wave panel: one row per lane, W = ceil(n / 64) waves (one per SIMD) ------------------------------------------------
// The single-wave kernel above is bound by instruction issue (one wave, ~12 k instructions).  Here every wave owns 64 rows, so a
// step costs a quarter of the FMAs per wave, at the price of one workgroup barrier per step: each wave finds its own best row,
// and its candidate lane publishes {key, lane} and the row's live part (columns >= J) into the wave's LDS slot BEFORE the global
// winner is known; after the barrier every wave reads the W keys, picks the winner (largest |a|, lowest wave on ties) and reads the
// pivot row from the winner's slot.  Slots are double-buffered on the parity of J (a wave can be at most one step ahead).
// VAL (the <4, 1> instance): the search inside a wave compares |a| without its low 9 bits as well, so that both levels apply one rule -- the
// lowest row among those with the largest truncated |a| -- and the pivot is a function of the values alone, not of which rows share a wave
// (without it two candidates of ONE wave that agree in their leading 43 mantissa bits are told apart, two of different waves are not).
template <int J, int NW, int RPL, bool VAL>
__device__ __forceinline__ void gj_step_mw(double (&a)[RPL][GJ_NB], unsigned& live, int (&mypos)[RPL], int& myperm, bool& singular, int lane, int wave, int k0,
                                           double (*slot_row)[NW][GJ_NB + 2], unsigned long long (*slot_key)[(NW + 1) & ~1] GST_ARGS) {
    constexpr int PAR = J & 1;
    constexpr int C0 = J & ~1;
    GST(0)
    // this lane's best row: strict comparisons keep the lowest slot (= the lowest row) on a tie
    // (the values pass through an empty asm: a select between a[0][J], a[1][J], ... is otherwise turned into a load at a[bs][J], and a
    // dynamically indexed array lives in scratch)
    double aj = a[0][J]; int bs = 0;
    if (RPL > 1) asm volatile("" : "+v"(aj));
    unsigned long long key = (live & 1u) ? (VAL ? ((unsigned long long)__double_as_longlong(fabs(aj)) & ~0x1FFULL) | 0x100ULL : ((unsigned long long)__double_as_longlong(fabs(aj)) | 1ULL)) : 0ULL;
    static_assert(!VAL || RPL == 1, "the truncated in-wave search is written for one row per lane");
#pragma unroll
    for (int q = 1; q < RPL; ++q) {
        double v = a[q][J];
        asm volatile("" : "+v"(v));
        const unsigned long long kq = ((live >> q) & 1u) ? ((unsigned long long)__double_as_longlong(fabs(v)) | 1ULL) : 0ULL;
        if (kq > key) { key = kq; aj = v; bs = q; }
    }
    // the reciprocal of the lane's own candidate element, off the critical path (dgetf2 scales by the reciprocal pivot as
    // well): v_rcp_f64 + two Newton steps; the winner's value travels with its row
    double rme = __builtin_amdgcn_rcp(aj);
    rme = fma(fma(-aj, rme, 1.0), rme, rme);
    rme = fma(fma(-aj, rme, 1.0), rme, rme);
    const unsigned hi = (unsigned)(key >> 32), lo = (unsigned)key;
    const unsigned m1 = wave_max_u32(hi);
    const unsigned m2 = wave_max_u32(hi == m1 ? lo : 0u);
    const unsigned long long winners = __ballot(hi == m1 && lo == m2 && key != 0ULL);
    const int cl = winners ? (int)__builtin_ctzll(winners) : 0;
    GST(1)
    if (lane == cl) {                                     // this wave's candidate
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            if (bs == q) {                                // one of the RPL store sequences runs (the row index is a register name)
#pragma unroll
                for (int c = C0; c < GJ_NB; c += 2) *reinterpret_cast<double2*>(&slot_row[PAR][wave][c]) = make_double2(a[q][c], a[q][c + 1]);
            }
        }
        slot_row[PAR][wave][GJ_NB] = rme;
        // key: |a| with its low 9 bits replaced by {non-empty marker, slot, lane}; waves compare bits 9 and up (43 mantissa bits)
        slot_key[PAR][wave] = winners ? ((((unsigned long long)m1 << 32) | m2) & ~0x1FFULL) | (unsigned long long)(cl | (bs << 6)) | 0x100ULL : 0ULL;
    }
    GST(2)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    GST(3)
    // all keys in ONE LDS round trip (slots of absent waves stay 0 = "no candidate"): reading them under `w < nw` branches
    // made each key its own dependent round trip, ~450 clk per step
    constexpr int NWK = (NW + 1) & ~1;
    ulonglong2 kp[NWK / 2];
#pragma unroll
    for (int q = 0; q < NWK / 2; ++q) kp[q] = *reinterpret_cast<const ulonglong2*>(&slot_key[PAR][2 * q]);
    unsigned long long best = kp[0].x; int pw = 0;
    if ((kp[0].y >> 9) > (best >> 9)) { best = kp[0].y; pw = 1; }
#pragma unroll
    for (int q = 1; q < NWK / 2; ++q) {                   // strict: the lowest wave wins a tie
        if ((kp[q].x >> 9) > (best >> 9)) { best = kp[q].x; pw = 2 * q; }
        if ((kp[q].y >> 9) > (best >> 9)) { best = kp[q].y; pw = 2 * q + 1; }
    }
    const int pl = (int)(best & 0x3FULL), ps = (int)((best >> 6) & 3ULL);
    GST(4)
    double prow[GJ_NB - C0];
#pragma unroll
    for (int c = C0; c < GJ_NB; c += 2) { const double2 v = *reinterpret_cast<const double2*>(&slot_row[PAR][pw][c]); prow[c - C0] = v.x; prow[c + 1 - C0] = v.y; }
    const double r = slot_row[PAR][pw][GJ_NB];
    GST(5)
    if (lane == J && wave == 0) myperm = pl + 64 * pw + 64 * NW * ps;
    const bool mine = wave == pw && lane == pl;
    singular = singular || !(fabs(prow[J - C0]) > 0.0);
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        if (mine && ps == q) { live &= ~(1u << q); mypos[q] = k0 + J; }
        // branch-free: dead rows (earlier pivots, rows >= n) run the FMAs with l = 0, so the next step's pivot search can be
        // scheduled into them
        const bool lv = (live >> q) & 1u;
        const double l = lv ? a[q][J] * r : 0.0;
        a[q][J] = lv ? l : a[q][J];
#pragma unroll
        for (int c = J + 1; c < GJ_NB; ++c) a[q][c] = fma(-l, prow[c - C0], a[q][c]);
    }
    GST(6)
}
template <int J, int NW, int RPL, bool VAL>
struct GjStepsMW {
    static __device__ __forceinline__ void run(double (&a)[RPL][GJ_NB], unsigned& live, int (&mypos)[RPL], int& myperm, bool& singular, int lane, int wave, int nbw, int k0,
                                               double (*slot_row)[NW][GJ_NB + 2], unsigned long long (*slot_key)[(NW + 1) & ~1] GST_ARGS) {
        if (J < nbw) gj_step_mw<J, NW, RPL, VAL>(a, live, mypos, myperm, singular, lane, wave, k0, slot_row, slot_key GST_PASS);      // workgroup-uniform
        GjStepsMW<J + 1, NW, RPL, VAL>::run(a, live, mypos, myperm, singular, lane, wave, nbw, k0, slot_row, slot_key GST_PASS);
    }
};
template <int NW, int RPL, bool VAL>
struct GjStepsMW<GJ_NB, NW, RPL, VAL> {
    static __device__ __forceinline__ void run(double (&)[RPL][GJ_NB], unsigned&, int (&)[RPL], int&, bool&, int, int, int, int, double (*)[NW][GJ_NB + 2],
                                               unsigned long long (*)[(NW + 1) & ~1] GST_ARGS) {}
};
// ---- compacted panel: the live rows in ONE wave -------------------------------------------------------------------------------
// A late panel of the <4, 1> instance (n - k0 <= GJ_CMAX live rows) moves its live rows into rank order (= row order) through LDS and
// wave 0 eliminates alone, C = 1 or 2 rows per lane (ranks C lane + q, so "lowest lane, lowest slot" is "lowest row"): the single-wave
// step of gj_panel_kernel -- wave maxima, ballot, the pivot row by v_readlane into scalar operands, no LDS, no barrier -- with the pivot
// rule and the arithmetic of gj_step_mw<.., VAL = true>: truncated keys, the reciprocal by v_rcp_f64 + two Newton steps of the pivot
// element, l = a r, a <- fma(-l, p, a), dead rows with l = 0.  Same pivots, same bits.  A lane carries the ORIGINAL row of each slot.
constexpr int GJ_CMAX = 128;
struct GjCompactShared {
    double rows[GJ_NB][GJ_CMAX];                         // [column][rank]: a wave's stores and loads run along the ranks
    int orow[GJ_CMAX];                                   // rank -> original row
    int pos[256];                                        // original row -> the pivot position it took in this panel, or -1
};
template <int J, int C>
__device__ __forceinline__ void gj_step_cw(double (&a)[C][GJ_NB], unsigned& live, const int (&orow)[C], int (&pos)[C], int& myperm, bool& singular, int lane, int k0) {
    unsigned long long key = 0ULL; int bq = 0;
#pragma unroll
    for (int q = 0; q < C; ++q) {
        const unsigned long long kq = ((live >> q) & 1u) ? ((unsigned long long)__double_as_longlong(fabs(a[q][J])) & ~0x1FFULL) | 0x100ULL : 0ULL;
        if (kq > key) { key = kq; bq = q; }               // strict: the lower slot (= the lower row) of the lane wins a tie
    }
    const unsigned hi = (unsigned)(key >> 32), lo = (unsigned)key;
    const unsigned m1 = wave_max_u32(hi);
    const unsigned m2 = wave_max_u32(hi == m1 ? lo : 0u);
    const unsigned long long winners = __ballot(hi == m1 && lo == m2 && key != 0ULL);
    const int pl = winners ? (int)__builtin_ctzll(winners) : 0;
    const int pq = C > 1 ? __builtin_amdgcn_readlane(bq, pl) : 0;
    double prow[GJ_NB - J]; int prw = 0;
#pragma unroll
    for (int q = 0; q < C; ++q) {
        if (q == pq) {                                    // wave-uniform
#pragma unroll
            for (int c = J; c < GJ_NB; ++c) prow[c - J] = readlane_f64(a[q][c], pl);
            prw = __builtin_amdgcn_readlane(orow[q], pl);
        }
    }
    if (lane == J) myperm = prw;
    const double piv = prow[0];
    singular = singular || !(fabs(piv) > 0.0);
    double r = __builtin_amdgcn_rcp(piv);
    r = fma(fma(-piv, r, 1.0), r, r);
    r = fma(fma(-piv, r, 1.0), r, r);
#pragma unroll
    for (int q = 0; q < C; ++q) {
        if (lane == pl && pq == q) { live &= ~(1u << q); pos[q] = k0 + J; }
        const bool lv = (live >> q) & 1u;
        const double l = lv ? a[q][J] * r : 0.0;
        a[q][J] = lv ? l : a[q][J];
#pragma unroll
        for (int c = J + 1; c < GJ_NB; ++c) a[q][c] = fma(-l, prow[c - J], a[q][c]);
    }
}
template <int J, int C>
struct GjStepsCW {
    static __device__ __forceinline__ void run(double (&a)[C][GJ_NB], unsigned& live, const int (&orow)[C], int (&pos)[C], int& myperm, bool& singular, int lane, int nbw, int k0) {
        if (J < nbw) gj_step_cw<J, C>(a, live, orow, pos, myperm, singular, lane, k0);      // wave-uniform
        GjStepsCW<J + 1, C>::run(a, live, orow, pos, myperm, singular, lane, nbw, k0);
    }
};
template <int C>
struct GjStepsCW<GJ_NB, C> {
    static __device__ __forceinline__ void run(double (&)[C][GJ_NB], unsigned&, const int (&)[C], int (&)[C], int&, bool&, int, int, int) {}
};
// wave 0, after the barrier behind the compaction: the nl live rows out of cs, the steps, then the pivot rows into LU (the identity fill
// is behind the same barrier), their positions into cs.pos[original row] and the singular flag
template <int C>
__device__ __forceinline__ void gj_chain_cw(GjCompactShared& cs, double (&LU)[GJ_NB][GJ_NB], int& s_sing, int& myperm, int nl, int lane, int nbw, int k0) {
    double a[C][GJ_NB]; int orow[C], pos[C];
    unsigned live = 0u;
#pragma unroll
    for (int q = 0; q < C; ++q) {
        const int slot = C * lane + q;
        const bool ok = slot < nl;
        const int sc = ok ? slot : 0;
#pragma unroll
        for (int c = 0; c < GJ_NB; ++c) { const double v = cs.rows[c][sc]; a[q][c] = ok ? v : 0.0; }
        orow[q] = ok ? cs.orow[sc] : 0;
        pos[q] = -1;
        live |= ok ? (1u << q) : 0u;
    }
    bool singular = false;
    GjStepsCW<0, C>::run(a, live, orow, pos, myperm, singular, lane, nbw, k0);
#pragma unroll
    for (int q = 0; q < C; ++q) {
        if (pos[q] >= 0) {
            cs.pos[orow[q]] = pos[q];
            double* dst = &LU[pos[q] - k0][0];
#pragma unroll
            for (int c = 0; c < GJ_NB; c += 2) *reinterpret_cast<double2*>(dst + c) = make_double2(a[q][c], a[q][c + 1]);
        }
    }
    if (singular && lane == 0) s_sing = 1;
}

// NW waves (the most the workgroup may have), RPL matrix rows per lane: row t + 64 NW q is slot q of thread t.  One wave per SIMD up to n = 768
// (<4, 1> n <= 256, <4, 2> <= 512, <3, 3> <= 576, <4, 3> <= 768), two beyond (<8, 2>): with one row per lane n = 576 took 9 waves, three on
// a SIMD, and a step cost what the three issue one after the other plus nine single-lane row publishes instead of three.
//
// The panel is three device functions, shared by gj_panel_mw_kernel (one workgroup per chain, results to global memory) and
// gj_step_kernel (every update workgroup factors the panel itself and keeps the results in LDS): the same code, hence the same pivots.
template <int NW, int RPL>
struct GjPanelShared {
    double LU[GJ_NB][GJ_NB];
    double slot_row[2][NW][GJ_NB + 2];                   // row | reciprocal of its pivot element
    unsigned long long slot_key[2][(NW + 1) & ~1];
    int s_sing;
};
// The live rows of the panel's columns into registers.  oldpos: the row's rowpos entry before this panel (-1 = live).  CLAMPED: every load
// has a valid, clamped address and is masked at use, so that the row loads do not wait for rowpos (the fused step, where the rows of a
// panel are read by every workgroup anyway); otherwise only live rows are loaded, behind rowpos (the panel kernel, as it always did).
template <int NW, int RPL, bool CLAMPED>
__device__ __forceinline__ void gj_panel_load(const double* __restrict__ A, const int* rowpos, int n, int k0, int nbw, int t, double (&a)[RPL][GJ_NB], unsigned& live,
                                              int (&oldpos)[RPL]) {
    live = 0u;
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = t + 64 * NW * q;
        const int rc = r < n ? r : 0;
        if (CLAMPED) {
            double v[GJ_NB];
#pragma unroll
            for (int c = 0; c < GJ_NB; ++c) v[c] = A[rc + (long)n * (k0 + (c < nbw ? c : 0))];
            oldpos[q] = k0 == 0 ? -1 : rowpos[rc];
            const bool lv = r < n && oldpos[q] < 0;
            live |= lv ? (1u << q) : 0u;
#pragma unroll
            for (int c = 0; c < GJ_NB; ++c) a[q][c] = (lv && c < nbw) ? v[c] : 0.0;
        } else {
            oldpos[q] = k0 == 0 ? -1 : rowpos[rc];
            const bool lv = r < n && oldpos[q] < 0;
            live |= lv ? (1u << q) : 0u;
#pragma unroll
            for (int c = 0; c < GJ_NB; ++c) a[q][c] = (lv && c < nbw) ? A[r + (long)n * (k0 + c)] : 0.0;
        }
    }
}
// The elimination steps, then the pivot block into sh.LU (row-major in pivot order, identity beyond nbw) and the singular flag into
// sh.s_sing: both are complete after the caller's next barrier.  mypos[q]: the pivot position row q of this thread took in this panel, or -1;
// myperm (wave 0, lane j): the row that became pivot j.
//
// CMP (the <4, 1> instance) with cs != nullptr and nl = n - k0 <= GJ_CMAX live rows: the compacted chain above.  rank: this thread's row among
// the live ones (gj_compact_rank).  mypos / myperm come out as from the four-wave chain: a thread learns the position its ORIGINAL row took
// through cs.pos, so the callers' rowpos code is one for both chains.  The live count is n - k0 by construction (every earlier panel retired
// 32 rows), so the choice is workgroup-uniform.  A wave without a live row does nothing at all.
template <int NW, int RPL, bool CMP>
__device__ __forceinline__ void gj_panel_factor(GjPanelShared<NW, RPL>& sh, double (&a)[RPL][GJ_NB], unsigned& live, int (&mypos)[RPL], int& myperm, int t, int nbw, int k0,
                                                GjCompactShared* cs, int nl, int rank
#ifdef DQ_GJ_STAMPS
                                                , unsigned long long& gstart, unsigned long long& gsteps_end
#endif
                                                ) {
    constexpr int NWK = (NW + 1) & ~1;
    static_assert(RPL <= 4, "two key bits name the slot");
    static_assert(!CMP || (NW == 4 && RPL == 1), "the compacted chain is written for one row per lane in at most four waves");
    const int lane = t & 63, wave = t >> 6;
    bool singular = false;
    myperm = 0;
#pragma unroll
    for (int q = 0; q < RPL; ++q) mypos[q] = -1;
    for (int e = t; e < GJ_NB * GJ_NB; e += blockDim.x) (&sh.LU[0][0])[e] = ((e >> 5) == (e & 31)) ? 1.0 : 0.0;   // identity padding for nbw < 32
    if (t == 0) sh.s_sing = 0;
    if (t < 2 * NWK) (&sh.slot_key[0][0])[t] = 0ULL;      // waves that do not exist never publish: their keys stay "no candidate"
    if constexpr (CMP) {
        if (cs != nullptr && nl <= GJ_CMAX) {             // workgroup-uniform
            cs->pos[t] = -1;
            if ((live & 1u) && rank < GJ_CMAX) {          // (rank < nl always: the bound keeps a corrupt rowpos inside the buffer)
#pragma unroll
                for (int c = 0; c < GJ_NB; ++c) cs->rows[c][rank] = a[0][c];
                cs->orow[rank] = t;
            }
            lds_wait();
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
#ifdef DQ_GJ_STAMPS
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(gstart) :: "memory");
#endif
            if (wave == 0) {
                if (nl <= 64) gj_chain_cw<1>(*cs, sh.LU, sh.s_sing, myperm, nl, lane, nbw, k0);
                else gj_chain_cw<2>(*cs, sh.LU, sh.s_sing, myperm, nl, lane, nbw, k0);
            }
#ifdef DQ_GJ_STAMPS
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(gsteps_end) :: "memory");
            if (t == 0 && k0 == DQ_GJ_STAMP_K0 && blockIdx.x == 0 && blockIdx.y == 0)
                printf("gj panel k0=%d grid.x=%d, compacted: %d live rows on one wave, clocks over %d steps incl. the read-back and the deposit: %llu\n", k0, (int)gridDim.x, nl, nbw, gsteps_end - gstart);
#endif
            lds_wait();
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            mypos[0] = cs->pos[t];
            return;
        }
    }
    lds_wait();
    __builtin_amdgcn_s_barrier();                        // LDS only: loads the caller has in flight stay in flight
    asm volatile("" ::: "memory");

#ifdef DQ_GJ_STAMPS
    unsigned long long gst[8] = {0, 0, 0, 0, 0, 0, 0, 0}, gprev;
    asm volatile("s_waitcnt vmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(gprev) :: "memory"); gstart = gprev;
#endif
    GjStepsMW<0, NW, RPL, CMP>::run(a, live, mypos, myperm, singular, lane, wave, nbw, k0, sh.slot_row, sh.slot_key GST_PASS);
#ifdef DQ_GJ_STAMPS
    gsteps_end = gprev;
    if (t == 0 && k0 == DQ_GJ_STAMP_K0 && blockIdx.x == 0 && blockIdx.y == 0)
        printf("gj panel k0=%d grid.x=%d, %d waves x %d rows per lane, clocks over %d steps (each segment includes one stamp, ~130): (loop) %llu | search %llu | publish %llu | barrier %llu | keys %llu | row %llu | fma %llu | total %llu\n",
               k0, (int)gridDim.x, (int)(blockDim.x >> 6), RPL, nbw, gst[0], gst[1], gst[2], gst[3], gst[4], gst[5], gst[6], gprev - gstart);
#endif

    lds_wait();
    __builtin_amdgcn_s_barrier();                        // identity fill done everywhere before the pivot rows overwrite theirs
    asm volatile("" ::: "memory");
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        if (mypos[q] >= 0) {
            double* dst = &sh.LU[mypos[q] - k0][0];
#pragma unroll
            for (int c = 0; c < GJ_NB; c += 2) *reinterpret_cast<double2*>(dst + c) = make_double2(a[q][c], a[q][c + 1]);
        }
    }
    if (singular && lane == 0) sh.s_sing = 1;
}
// the rank of this thread's row among the live rows of a panel that will be compacted (else 0) and their number nl: rowpos of this lane's row in EVERY wave, loaded in
// the round of the panel's own loads, so that the wave offsets need no exchange.  pos: this thread's own entry, n <= 256.
__device__ __forceinline__ int gj_compact_rank(const int* rowpos, int n, int t, bool compact, int& nl) {
    int rank = 0;
    nl = GJ_CMAX + 1;                                    // "not compacted"
    if (compact) {                                       // workgroup-uniform
        int tot = 0;
        const int lane = t & 63, wave = t >> 6;
        int pw[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) { const int r = lane + 64 * w; pw[w] = rowpos[r < n ? r : n - 1]; }
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const unsigned long long b = __ballot(lane + 64 * w < n && pw[w] < 0);
            rank += w < wave ? __popcll(b) : (w == wave ? __popcll(b & ((1ULL << lane) - 1ULL)) : 0);
            tot += __popcll(b);
        }
        nl = tot < GJ_CMAX ? tot : GJ_CMAX;              // counted, = n - k0: wave 0 reads no slot that nobody wrote, whatever rowpos holds
    }
    return rank;
}
#ifdef DQ_GJ_STAMPS
#define GJ_STAMP_VM(x) asm volatile("s_waitcnt vmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(x) :: "memory")
#endif

template <int NW, int RPL>
__global__ __launch_bounds__(64 * NW) void gj_panel_mw_kernel(CMat Am, int* rowpos_p, long rowpos_stride, int* perm_p, long perm_stride, double* tinv_p,
                                                          double* logabsdet, int accumulate, int* info, int n, int k0, int compact) {
    __shared__ __attribute__((aligned(16))) GjPanelShared<NW, RPL> sh;
    const int chain = blockIdx.y;
    const double* __restrict__ A = Am.at(chain);
    int* rowpos = rowpos_p + (long)chain * rowpos_stride;
    int* perm = perm_p + (long)chain * perm_stride;
    double* tinv = tinv_p + (long)chain * 2 * GJ_NB * GJ_NB;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
#ifdef DQ_GJ_STAMPS
    unsigned long long gentry, gstart, gprev;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(gentry) :: "memory");
#endif
    const int nbw = min(GJ_NB, n - k0);
    unsigned live;
    int oldpos[RPL], mypos[RPL], myperm;
    double a[RPL][GJ_NB];
    gj_panel_load<NW, RPL, false>(A, rowpos, n, k0, nbw, t, a, live, oldpos);
    constexpr bool CMP = NW == 4 && RPL == 1;              // late panels run on one wave (gj_panel_factor); the other instances name no buffer
    __shared__ __attribute__((aligned(16))) std::conditional_t<CMP, GjCompactShared, int> s_cs;
    GjCompactShared* cs = nullptr;
    if constexpr (CMP) { if (compact) cs = &s_cs; }
    int nl = GJ_CMAX + 1;
    const int rank = CMP ? gj_compact_rank(rowpos, n, t, cs != nullptr && k0 > 0 && n - k0 <= GJ_CMAX, nl) : 0;      // (k0 = 0: rowpos holds the last solve's)
#ifdef DQ_GJ_STAMPS
    gj_panel_factor<NW, RPL, CMP>(sh, a, live, mypos, myperm, t, nbw, k0, cs, nl, rank, gstart, gprev);
#else
    gj_panel_factor<NW, RPL, CMP>(sh, a, live, mypos, myperm, t, nbw, k0, cs, nl, rank);
#endif
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = t + 64 * NW * q;
        if (r < n) { if (k0 == 0) rowpos[r] = mypos[q]; else if (mypos[q] >= 0) rowpos[r] = mypos[q]; }
    }
    if (wave == 0 && lane < nbw) perm[k0 + lane] = myperm;
    __syncthreads();
    for (int e = t; e < GJ_NB * GJ_NB; e += blockDim.x) tinv[e] = (&sh.LU[0][0])[e];
#ifdef DQ_GJ_STAMPS
    unsigned long long gmid;
    GJ_STAMP_VM(gmid);
#endif
    if (wave == 0) gj_panel_tri_inverses(sh.LU, tinv + GJ_NB * GJ_NB, lane);
    else if (wave == 1) gj_panel_logdet(sh.LU, logabsdet, accumulate, info, chain, lane, nbw, k0, sh.s_sing);
#ifdef DQ_GJ_STAMPS
    unsigned long long gend;
    GJ_STAMP_VM(gend);
    if (t == 0 && k0 == DQ_GJ_STAMP_K0 && blockIdx.y == 0) printf("   prologue %llu | steps %llu | LU hand-over (+ printf) %llu | epilogue %llu\n", gstart - gentry, gprev - gstart, gmid - gprev, gend - gmid);
#endif
}

// MFMA operand convention (v_mfma_f64_16x16x4_f64, lane = (r16, kk) = (lane & 15, lane >> 4)):
//   mfma(a, b, acc): a = A[row r16][k kk], b = B[k kk][col r16], acc[reg] = D[row kk + 4 reg][col r16].
// A D tile therefore feeds the next product as its B operand directly: acc[reg] of lane (c, kk) is row k = kk + 4 reg
// of column c, and any partition of k into groups of four works as long as the A operand uses the same one.
//
// grid.x = col_tiles * row_tiles; 256 threads = 2 x 2 waves of 16 x 16.  Row tiles: [0, nA) rows of A / B (live rows
// only), [nA, nA + nS) retired rows (pivot order, SA / X), the last one writes the panel's own rows U12 into SA / X.
// Column tiles: [0, nCA) trailing columns of A, then n/32 tiles of B.
__global__ __launch_bounds__(256) void gj_update_kernel(Mat Am, Mat Bm, Mat SAm, Mat Xm, const int* rowpos_p, long rowpos_stride,
                                                        const int* perm_p, long perm_stride, const double* tinv_p, int n, int k0, int nA, int nS, int nCA) {
    const int chain = blockIdx.y;
    double* __restrict__ A = Am.at(chain);
    double* __restrict__ B = Bm.at(chain);
    double* __restrict__ SA = SAm.at(chain);
    double* __restrict__ X = Xm.at(chain);
    const int* rowpos = rowpos_p + (long)chain * rowpos_stride;
    const int* perm = perm_p + (long)chain * perm_stride;
    const double* __restrict__ LUg = tinv_p + (long)chain * 2 * GJ_NB * GJ_NB;      // pivot block, row-major
    const double* __restrict__ Tinv = LUg + GJ_NB * GJ_NB;                          // 4 x (16 x 16) triangular inverses, column-major
    const int nbw = min(GJ_NB, n - k0);
    const int row_tiles = nA + nS + 1;
    const int rt = blockIdx.x % row_tiles, ct = blockIdx.x / row_tiles;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kk = lane >> 4;
    const int wr = wave & 1, wc = wave >> 1;
    const bool colA = ct < nCA;
    const int col = (colA ? k0 + nbw + 32 * ct : 32 * (ct - nCA)) + 16 * wc + r16;      // this lane's column (B operand / D layout)
    const bool col_ok = col < n;
    const long coff = (long)n * (col_ok ? col : n - 1);
    const double* __restrict__ src12 = colA ? A : B;         // pivot rows are read from here
    double* __restrict__ dstS = colA ? SA : X;               // retired rows of this column block

    // ---- operands, all loads issued up front ----
    double a12[2][4];                                        // A12[k = 16h + 4s + kk][col]
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = 16 * h + 4 * s + kk;
            const int pr = perm[k0 + (k < nbw ? k : 0)];
            const double v = src12[pr + coff];
            a12[h][s] = (k < nbw && col_ok) ? v : 0.0;
        }
    // rows of this wave
    const bool writer = rt == nA + nS;
    const bool rowS = rt >= nA;
    const int row0 = (rowS ? 32 * (rt - nA) : 32 * rt) + 16 * wr;         // A rows: original index; S rows: pivot position
    const int rowlim = rowS ? k0 : n;
    const double* __restrict__ msrc = rowS ? SA : A;         // multipliers A[r, panel]
    double* __restrict__ dst = rowS ? dstS : (colA ? A : B);
    double mult[2][4];                                       // Mult[row0 + r16][k = 16h + kk + 4s]
    double cold[4];                                          // C[row0 + kk + 4 reg][col]
    bool st_ok[4];
    if (!writer) {
        const int mrow = min(row0 + r16, rowlim - 1);
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int k = 16 * h + kk + 4 * s;
                const double v = msrc[mrow + (long)n * (k0 + (k < nbw ? k : 0))];
                mult[h][s] = k < nbw ? v : 0.0;
            }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int r = row0 + kk + 4 * reg;
            const int rc = min(r, rowlim - 1);
            st_ok[reg] = col_ok && r < rowlim && (rowS || rowpos[rc] < 0);
            cold[reg] = dst[rc + coff];
        }
    }
    // ---- triangular operands (A operand of the MFMA: row r16, k = 4 s + kk) ----
    double lai[4], lbi[4], uai[4], ubi[4], cl[4], cu[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int k = 4 * s + kk;
        lai[s] = Tinv[0 * 256 + r16 + 16 * k]; lbi[s] = Tinv[1 * 256 + r16 + 16 * k];
        uai[s] = Tinv[2 * 256 + r16 + 16 * k]; ubi[s] = Tinv[3 * 256 + r16 + 16 * k];
        cl[s] = -LUg[(16 + r16) * 32 + k];               // -L11[16 + r16][k]
        cu[s] = -LUg[r16 * 32 + 16 + k];                 // -U11[r16][16 + k]
    }
    // ---- T1 = L11^-1 A12 by block forward substitution.  The B-operand chunking k = 4 s + kk is the D layout
    //      (row kk + 4 reg), so a12[1] seeds the accumulator of the Schur step directly. ----
    const d4 zero4 = {0.0, 0.0, 0.0, 0.0};
    d4 t1[2], u[2];
    t1[0] = zero4;
#pragma unroll
    for (int s = 0; s < 4; ++s) t1[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(lai[s], a12[0][s], t1[0], 0, 0, 0);
    d4 w = {a12[1][0], a12[1][1], a12[1][2], a12[1][3]};
#pragma unroll
    for (int s = 0; s < 4; ++s) w = __builtin_amdgcn_mfma_f64_16x16x4f64(cl[s], t1[0][s], w, 0, 0, 0);
    t1[1] = zero4;
#pragma unroll
    for (int s = 0; s < 4; ++s) t1[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(lbi[s], w[s], t1[1], 0, 0, 0);
    // ---- U12 = U11^-1 T1 by block back substitution ----
    u[1] = zero4;
#pragma unroll
    for (int s = 0; s < 4; ++s) u[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(ubi[s], t1[1][s], u[1], 0, 0, 0);
    w = t1[0];
#pragma unroll
    for (int s = 0; s < 4; ++s) w = __builtin_amdgcn_mfma_f64_16x16x4f64(cu[s], u[1][s], w, 0, 0, 0);
    u[0] = zero4;
#pragma unroll
    for (int s = 0; s < 4; ++s) u[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(uai[s], w[s], u[0], 0, 0, 0);
    if (writer) {                                            // rows k0 + 16 wr + kk + 4 reg of SA / X receive U12
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int i = 16 * wr + kk + 4 * reg;
            if (i < nbw && col_ok) dstS[k0 + i + coff] = u[wr][reg];
        }
        return;
    }
    // ---- C -= Mult U12 ----
    d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(mult[h][s], u[h][s], acc, 0, 0, 0);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg)
        if (st_ok[reg]) dst[row0 + kk + 4 * reg + coff] = cold[reg] - acc[reg];
}

// One launch per panel: gj_update_kernel's grid and tile assignment, but every workgroup first factors the panel itself (the device
// functions of gj_panel_mw_kernel: same code, same pivots) and keeps the pivot block, its triangular inverses, the panel's perm and the
// new rowpos in LDS.  Nothing is handed over between workgroups and none waits for another.  The arithmetic of the update is
// gj_update_kernel's bit for bit: operand partition k = 16h + 4s + kk, the order of the six substitution products, cold - acc.
//
// Within one launch every workgroup reads, and none writes:
//   - the panel's columns A[:, k0 .. k0+31] (the trailing tiles start at column k0 + nbw) and SA[0 .. k0, panel] of the retired rows;
//   - the pivot rows of this panel in the trailing columns of A and in B (st_ok masks them with the workgroup's own new rowpos);
//   - rowpos of the previous panel: the new one goes to the OTHER half of the buffer (halves alternate with the panel's parity), written by
//     workgroup 0 of the chain, which also performs the two read-modify-writes, logabsdet[chain] and the singular-pivot flag.
// The writer row tile writes rows k0 .. k0+31 of SA / X, disjoint from the retired rows [0, k0) the S tiles update.
// mult[][] and cold[] depend on no pivot: their loads are issued before the elimination steps, behind the panel's own in program order, so the
// counted wait in front of the first step covers the panel's loads only; they have clamped addresses and are masked at use.
template <int NW, int RPL>
__global__ __launch_bounds__(64 * NW) void gj_step_kernel(Mat Am, Mat Bm, Mat SAm, Mat Xm, const int* rowpos_old_p, int* rowpos_new_p, long rowpos_stride,
                                                          double* logabsdet, int accumulate, int* info, int n, int k0, int nA, int nS, int nCA, int compact) {
    static_assert(NW == 4, "the update's 2 x 2 waves are the panel's");
    __shared__ __attribute__((aligned(16))) GjPanelShared<NW, RPL> sh;
    __shared__ __attribute__((aligned(16))) double s_inv[4 * 256];      // the four 16 x 16 triangular inverses, column-major
    __shared__ int s_rowpos[64 * NW * RPL];
    __shared__ int s_perm[GJ_NB];
    const int chain = blockIdx.y;
    double* __restrict__ A = Am.at(chain);
    double* __restrict__ B = Bm.at(chain);
    double* __restrict__ SA = SAm.at(chain);
    double* __restrict__ X = Xm.at(chain);
    const int* rowpos_old = rowpos_old_p + (long)chain * rowpos_stride;
    int* rowpos_new = rowpos_new_p + (long)chain * rowpos_stride;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
#ifdef DQ_GJ_STAMPS
    unsigned long long gentry, gstart, gprev;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(gentry) :: "memory");
#endif
    const int nbw = min(GJ_NB, n - k0);

    // ---- the panel's rows, then the operands of the update that depend on no pivot ----
    unsigned live;
    int oldpos[RPL], mypos[RPL], myperm;
    double a[RPL][GJ_NB];
    gj_panel_load<NW, RPL, true>(A, rowpos_old, n, k0, nbw, t, a, live, oldpos);
    constexpr bool CMP = NW == 4 && RPL == 1;
    __shared__ __attribute__((aligned(16))) std::conditional_t<CMP, GjCompactShared, int> s_cs;
    GjCompactShared* cs = nullptr;
    if constexpr (CMP) { if (compact) cs = &s_cs; }
    int nl = GJ_CMAX + 1;
    const int rank = CMP ? gj_compact_rank(rowpos_old, n, t, cs != nullptr && k0 > 0 && n - k0 <= GJ_CMAX, nl) : 0;      // (k0 = 0: rowpos holds the last solve's)

    const int row_tiles = nA + nS + 1;
    const int rt = blockIdx.x % row_tiles, ct = blockIdx.x / row_tiles;
    const int r16 = lane & 15, kk = lane >> 4;
    const int wr = wave & 1, wc = wave >> 1;
    const bool colA = ct < nCA;
    const int col = (colA ? k0 + nbw + 32 * ct : 32 * (ct - nCA)) + 16 * wc + r16;      // this lane's column (B operand / D layout)
    const bool col_ok = col < n;
    const long coff = (long)n * (col_ok ? col : n - 1);
    const double* __restrict__ src12 = colA ? A : B;         // pivot rows are read from here
    double* __restrict__ dstS = colA ? SA : X;               // retired rows of this column block
    const bool writer = rt == nA + nS;
    const bool rowS = rt >= nA;
    const int row0 = (rowS ? 32 * (rt - nA) : 32 * rt) + 16 * wr;         // A rows: original index; S rows: pivot position
    const int rowlim = rowS ? k0 : n;
    const double* __restrict__ msrc = rowS ? SA : A;         // multipliers A[r, panel]
    double* __restrict__ dst = rowS ? dstS : (colA ? A : B);
    double mult[2][4];                                       // Mult[row0 + r16][k = 16h + kk + 4s]
    double cold[4];                                          // C[row0 + kk + 4 reg][col]
    {                                                        // the writer tile (rowlim = k0, possibly 0) loads too and uses nothing of it
        const int mrow = max(min(row0 + r16, rowlim - 1), 0);
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int k = 16 * h + kk + 4 * s;
                const double v = msrc[mrow + (long)n * (k0 + (k < nbw ? k : 0))];
                mult[h][s] = k < nbw ? v : 0.0;
            }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) cold[reg] = dst[max(min(row0 + kk + 4 * reg, rowlim - 1), 0) + coff];
    }

#ifdef DQ_GJ_STAMPS
    gj_panel_factor<NW, RPL, CMP>(sh, a, live, mypos, myperm, t, nbw, k0, cs, nl, rank, gstart, gprev);
#else
    gj_panel_factor<NW, RPL, CMP>(sh, a, live, mypos, myperm, t, nbw, k0, cs, nl, rank);
#endif
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = t + 64 * NW * q;
        const int np = mypos[q] >= 0 ? mypos[q] : oldpos[q];
        s_rowpos[r] = np;
        if (blockIdx.x == 0 && r < n) rowpos_new[r] = np;
    }
    if (wave == 0 && lane < GJ_NB) s_perm[lane] = lane < nbw ? myperm : 0;
    __syncthreads();
#ifdef DQ_GJ_STAMPS
    unsigned long long gmid, ginv, ggather;
    GJ_STAMP_VM(gmid);
#endif

    // ---- the pivot rows of this wave's columns: the only loads behind the chain, in flight under the triangular inverses ----
    double a12[2][4];                                        // A12[k = 16h + 4s + kk][col]
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = 16 * h + 4 * s + kk;
            const double v = src12[s_perm[k < nbw ? k : 0] + coff];
            a12[h][s] = (k < nbw && col_ok) ? v : 0.0;
        }
    bool st_ok[4];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int r = row0 + kk + 4 * reg;
        st_ok[reg] = !writer && col_ok && r < rowlim && (rowS || s_rowpos[max(min(r, rowlim - 1), 0)] < 0);
    }
    if (wave == 0) gj_panel_tri_inverses(sh.LU, s_inv, lane);
    else if (wave == 1 && blockIdx.x == 0) gj_panel_logdet(sh.LU, logabsdet, accumulate, info, chain, lane, nbw, k0, sh.s_sing);
#ifdef DQ_GJ_STAMPS
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(ginv) :: "memory");
#endif
    __syncthreads();
#ifdef DQ_GJ_STAMPS
    GJ_STAMP_VM(ggather);
#endif

    // ---- triangular operands (A operand of the MFMA: row r16, k = 4 s + kk) ----
    const double* LUs = &sh.LU[0][0];
    double lai[4], lbi[4], uai[4], ubi[4], cl[4], cu[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int k = 4 * s + kk;
        lai[s] = s_inv[0 * 256 + r16 + 16 * k]; lbi[s] = s_inv[1 * 256 + r16 + 16 * k];
        uai[s] = s_inv[2 * 256 + r16 + 16 * k]; ubi[s] = s_inv[3 * 256 + r16 + 16 * k];
        cl[s] = -LUs[(16 + r16) * 32 + k];               // -L11[16 + r16][k]
        cu[s] = -LUs[r16 * 32 + 16 + k];                 // -U11[r16][16 + k]
    }
    // ---- T1 = L11^-1 A12, U12 = U11^-1 T1: gj_update_kernel's sequence ----
    const d4 zero4 = {0.0, 0.0, 0.0, 0.0};
    d4 t1[2], u[2];
    t1[0] = zero4;
#pragma unroll
    for (int s = 0; s < 4; ++s) t1[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(lai[s], a12[0][s], t1[0], 0, 0, 0);
    d4 w = {a12[1][0], a12[1][1], a12[1][2], a12[1][3]};
#pragma unroll
    for (int s = 0; s < 4; ++s) w = __builtin_amdgcn_mfma_f64_16x16x4f64(cl[s], t1[0][s], w, 0, 0, 0);
    t1[1] = zero4;
#pragma unroll
    for (int s = 0; s < 4; ++s) t1[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(lbi[s], w[s], t1[1], 0, 0, 0);
    u[1] = zero4;
#pragma unroll
    for (int s = 0; s < 4; ++s) u[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(ubi[s], t1[1][s], u[1], 0, 0, 0);
    w = t1[0];
#pragma unroll
    for (int s = 0; s < 4; ++s) w = __builtin_amdgcn_mfma_f64_16x16x4f64(cu[s], u[1][s], w, 0, 0, 0);
    u[0] = zero4;
#pragma unroll
    for (int s = 0; s < 4; ++s) u[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(uai[s], w[s], u[0], 0, 0, 0);
    if (writer) {                                            // rows k0 + 16 wr + kk + 4 reg of SA / X receive U12
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int i = 16 * wr + kk + 4 * reg;
            if (i < nbw && col_ok) dstS[k0 + i + coff] = u[wr][reg];
        }
    } else {
        // ---- C -= Mult U12 ----
        d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(mult[h][s], u[h][s], acc, 0, 0, 0);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
            if (st_ok[reg]) dst[row0 + kk + 4 * reg + coff] = cold[reg] - acc[reg];
    }
#ifdef DQ_GJ_STAMPS
    unsigned long long gend;
    GJ_STAMP_VM(gend);
    if (t == 0 && k0 == DQ_GJ_STAMP_K0 && blockIdx.x == 0 && blockIdx.y == 0)
        printf("   fused step: prologue %llu | chain %llu | deposit (+ printf) %llu | inverses (wave 0) %llu | gather wait %llu | update %llu\n", gstart - gentry, gprev - gstart,
               gmid - gprev, ginv - gmid, ggather - ginv, gend - ggather);
#endif
}
bool gj_fused_fits(int n) { return n > 64 && n <= 256; }
// where the fused step measured faster than the two launches: with three or four waves of rows.  At n <= 128 the panel kernel
// runs two waves and its barrier is cheaper than that of the step's four (n = 72, 100: 26.1 / 26.5 us per pair against 27.5 / 28.0 us per step).
bool gj_fused_default(int n) { return n > 128 && n <= 256; }

// X = A^-1 B (n <= 1024).  A and B are destroyed; SA: n*n scratch per chain; tinv: 2048 doubles per chain;
// perm / rowpos / rowpos_alt: n ints per chain.  logabsdet (optional) receives (+)= log|det A|; *info |= DQ_STATUS_PIVOT on a zero / NaN pivot.
// fused: one gj_step_kernel per panel where an instance exists (gj_fused_fits); rowpos_alt is then the second half of rowpos.
int launch_gj_solve(Mat A, Mat B, Mat X, Mat SA, double* tinv, int* perm, long perm_stride, int* rowpos, int* rowpos_alt, long rowpos_stride,
                    double* logabsdet, int accumulate_logdet, int* info, int n, int n_chains, bool fused, bool compact, hipStream_t s) {
    if (n > 1024) { set_error("gj_solve supports n <= 1024"); return -1; }
    if (fused && rowpos_alt && gj_fused_fits(n)) {
        int p = 0;
        for (int k0 = 0; k0 < n; k0 += GJ_NB, ++p) {
            const int nbw = n - k0 < GJ_NB ? n - k0 : GJ_NB;
            const int nA = (n + 31) / 32, nS = k0 / 32;
            const int nCA = (n - k0 - nbw + 31) / 32, nCB = (n + 31) / 32;
            hipLaunchKernelGGL((gj_step_kernel<4, 1>), dim3((nA + nS + 1) * (nCA + nCB), n_chains), dim3(256), 0, s, A, B, SA, X, (const int*)((p & 1) ? rowpos_alt : rowpos),
                               (p & 1) ? rowpos : rowpos_alt, rowpos_stride, logabsdet, accumulate_logdet, info, n, k0, nA, nS, nCA, compact ? 1 : 0);
        }
        DQ_HIP(hipGetLastError());
        return 0;
    }
    for (int k0 = 0; k0 < n; k0 += GJ_NB) {
        const dim3 pg(1, n_chains);
#define DQ_GJ_PANEL(NW, RPL) hipLaunchKernelGGL((gj_panel_mw_kernel<NW, RPL>), pg, dim3(RPL == 1 ? 64 * ((n + 63) / 64) : 64 * NW), 0, s, CMat(A), rowpos, rowpos_stride, perm, perm_stride, tinv, logabsdet, accumulate_logdet, info, n, k0, compact ? 1 : 0)
        if (n > 768) DQ_GJ_PANEL(8, 2);
        else if (n > 576) DQ_GJ_PANEL(4, 3);
        else if (n > 512) DQ_GJ_PANEL(3, 3);
        else if (n > 256) DQ_GJ_PANEL(4, 2);
        else if (n > 64) DQ_GJ_PANEL(4, 1);
        else hipLaunchKernelGGL((gj_panel_kernel<1>), pg, dim3(64), 0, s, CMat(A), rowpos, rowpos_stride, perm, perm_stride, tinv, logabsdet, accumulate_logdet, info, n, k0);      // n <= 64: one wave holds every row
        const int nbw = n - k0 < GJ_NB ? n - k0 : GJ_NB;
        const int nA = (n + 31) / 32, nS = k0 / 32;
        const int nCA = (n - k0 - nbw + 31) / 32, nCB = (n + 31) / 32;
        hipLaunchKernelGGL(gj_update_kernel, dim3((nA + nS + 1) * (nCA + nCB), n_chains), dim3(256), 0, s, A, B, SA, X, (const int*)rowpos, rowpos_stride,
                           (const int*)perm, perm_stride, (const double*)tinv, n, k0, nA, nS, nCA);
    }
#undef DQ_GJ_PANEL
    DQ_HIP(hipGetLastError());
    return 0;
}

}  // namespace dq
