// qr_panel.hip -- stablelinalg::to_LDR (source/stablelinalg.cpp:35-55) as a PANEL-pivoted blocked Householder QR.
//
// The reference factorises with dgeqp3 (arma::qr(Q, R, P, M, "vector")): one global pivot decision per COLUMN, i.e. n dependent
// chip-wide steps (qr_colown.hip runs them on one CU in 3.2 us each, qr_coop.hip pays a cross-CU exchange for each).  to_LDR's
// consumers only ever use the product L diag(d) R and the grading of d, so the pivot ORDER is free as long
// as the factorisation stays rank-revealing.  Here one global decision is taken per panel of QP_B = 16 columns:
//
//   sketch     Y = Omega . A_trailing, Omega = QP_SR x m matrix of +-1 from an integer hash of the row index (fixed: the
//              factorisation is deterministic), formed on the matrix cores by the update kernel from the tiles it has just
//              updated -- the sketch is FRESH for every panel (a down-dated sketch loses the small columns of a graded DQMC
//              matrix to cancellation);
//   selection  the first 16 pivots of a column-pivoted Householder QR of the 32 x n_c sketch (one workgroup, lane <-> column, the
//              column in registers, one barrier per step) are the panel's columns, in that order;
//   panel      unpivoted Householder QR of the 16 selected full-height columns: lane <-> (column c = lane & 15, 16 rows), the
//              pivot column reaches the other 15 lanes of its DPP row by row_newbcast (v_fmac_f64_dpp), so the 15 dot products
//              and the 15 updates of a step are 16 DPP-FMAs each; ONE fused reduction per step yields the dots, the squared
//              norm of the pivot column's tail and the entries v_c^T v_j of the compact-WY factor T;
//   update     A <- (I - V T V^T)^T A on the trailing columns, 16 columns per workgroup, v_mfma_f64_16x16x4_f64;
//   form Q     Q^T = H_{n/16-1}^T ... H_0^T I is the same update applied to an n x n buffer that starts as the identity: a second range
//              of workgroups of every update launch (the Q role, on CUs the launch leaves idle) carries it along, and the 16 rows of
//              Q^T that factor k completes go straight into L as 16 columns of Q.  No launch of its own.
//
// n / 16 panels x (qp_panel_kernel, qp_update_kernel) + the explicit-Q launch of the time: 575 us at n = 256 (qr_colown + formq_blocked:
// 892), 2.0 ms at n = 576 (qr_coop: 4.26).  Where the time goes, and the forms that were measured and dropped (one persistent launch, a lane pair per
// sketch column, 24 sketch rows, look-ahead selection): DESIGN.md section 5.
//
// One launch per panel up to n = 512 (qp_step_kernel: the update launch, every workgroup of which factors the panel itself -- no hand-over,
// no reflector panels in global memory; 29.6 against 25.2 + 6.5 us per panel at n = 256); the pair of launches above that and under
// DQMC_QR_PANEL_FUSED=0.  Both forms give the same bits.
//
// Randomised panel pivoting (Duersch & Gu 2017; Martinsson, Quintana-Orti, Heavner, van de Geijn 2017).  The numpy statement
// of exactly this algorithm is oracle/panel_qr.py::qr_sketch(b = 16, p = 16, sign = True, local_pivot = False); its effect on
// G (cfg 3 thermalised sweep 3e-11 absolute, cfg 3 / cfg 5 i.i.d. <= 3e-11 relative; tournament pivoting and Gaussian sketches
// beside it) is in profiles/r04_eval_panel_qr_numpy.log; tests/test_panel_qr.py pins the numpy statements on the CPU.
// Output format = the other QRCP kernels': reflectors and R0 in place in A WITHOUT column swaps, tau, jpvt (formq_* and
// assemble_r_kernel of qr.hip finish L, d, R).
#include "common.h"
#include "wave.h"
#include <utility>

namespace dq {

namespace {

#ifdef DQ_QP_STAMPS
#define QST(i) { unsigned long long t_; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); if (threadIdx.x == 0) qst[i] = t_; }
#else
#define QST(i)
#endif

#ifdef DQ_QP_STAMPS
#ifndef DQ_QP_STAMP_K
#define DQ_QP_STAMP_K 0          // the panel whose ticks the stamp build prints (-DDQ_QP_STAMP_K=192: a compacted one at n = 256)
#endif
#define QP_QST_PARAM , unsigned long long* qst
#define QP_QST_ARG , qst
#else
#define QP_QST_PARAM
#define QP_QST_ARG
#endif

constexpr int QP_B = 16;         // panel width
constexpr int QP_SR = 32;        // sketch rows formed by the update kernel (two MFMA row tiles)
#ifndef QP_SEL_ROWS
#define QP_SEL_ROWS 32
#endif
constexpr int QP_SEL = QP_SEL_ROWS;   // ... and used by the selection (b + p, p = 16).  24 rows (p = 8) are 3 us per panel faster at n = 256 (25.2 against 28.2 us) but put the thermalised unequal-time series of cfg 3 at 1.44e-10 of its largest entry (32 rows: 6.8e-11; bound 1e-10)
typedef double d4 __attribute__((ext_vector_type(4)));

// Omega[i][r] = +-1: bit i of a 32-bit mix of the ROW index r (oracle/panel_qr.py::omega_sign is the same function)
__device__ __forceinline__ unsigned qp_row_bits(unsigned r) {
    unsigned h = r * 0x9E3779B1u + 0x85EBCA77u;
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
__device__ __forceinline__ double qp_sign(unsigned bits, int i) {
    return __hiloint2double((int)(0x3FF00000u | (((bits >> i) & 1u) << 31)), 0);
}

// lane-wise sum over the four 16-lane rows of a wave (gfx950 v_permlane16_swap / v_permlane32_swap), result in every lane
__device__ __forceinline__ double rows4_sum(double x) {
    const unsigned lo = (unsigned)__double_as_longlong(x), hi = (unsigned)(__double_as_longlong(x) >> 32);
    auto l16 = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    auto h16 = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    const double e = __hiloint2double((int)h16[0], (int)l16[0]), o = __hiloint2double((int)h16[1], (int)l16[1]);   // even row | odd row of each pair
    const double s = e + o;
    const unsigned slo = (unsigned)__double_as_longlong(s), shi = (unsigned)(__double_as_longlong(s) >> 32);
    auto l32 = __builtin_amdgcn_permlane32_swap(slo, slo, false, false);
    auto h32 = __builtin_amdgcn_permlane32_swap(shi, shi, false, false);
    return __hiloint2double((int)h32[0], (int)l32[0]) + __hiloint2double((int)h32[1], (int)l32[1]);               // lower half | upper half
}

// d += a[lane J of this 16-lane row] * a  (own value times the broadcast one, one register).  No wait state in front: the callers
// fence every register these blocks read (dpp_fence) after its last VALU write.
template <int J>
__device__ __forceinline__ void dpp_fmac_self(double& d, double a) {
    asm volatile("v_fmac_f64_dpp %0, %1, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "+v"(d) : "v"(a), "n"(J));
}
// a += a[lane J] * m
template <int J>
__device__ __forceinline__ void dpp_axpy_self(double& a, double m) {
    asm volatile("v_fmac_f64_dpp %0, %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "+v"(a) : "v"(m), "n"(J));
}
// every VALU write of a[] issued so far is complete and two wait states old: what a DPP read of these registers needs (the hazard
// recogniser does not look inside inline asm)
__device__ __forceinline__ void dpp_fence(double (&a)[16]) {
    asm volatile("s_nop 1" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]),
                             "+v"(a[8]), "+v"(a[9]), "+v"(a[10]), "+v"(a[11]), "+v"(a[12]), "+v"(a[13]), "+v"(a[14]), "+v"(a[15]));
}

__device__ __forceinline__ void dpp_fence1(double& z) { asm volatile("s_nop 1" : "+v"(z)); }
// d += z[lane T of this 16-lane row] * y
template <int T>
__device__ __forceinline__ void dpp_fmac(double& d, double z, double y) {
    asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(d) : "v"(z), "v"(y), "n"(T));
}
// tj += sum over t < J of trow[t] * z[lane t of this row]
template <int... Ts>
__device__ __forceinline__ void t_row_dot(double& tj, const double (&trow)[16], double z, std::integer_sequence<int, Ts...>) {
    (dpp_fmac<Ts>(tj, z, trow[Ts]), ...);
}

template <int NW>
struct PanelShared {
    static constexpr int NWP = NW < 2 ? 2 : NW;
    alignas(16) unsigned long long key[2][NWP];   // selection: every wave's best {norm^2 | column}, double-buffered on the step parity
    alignas(16) double cand[2][QP_SEL + 2];        // ... and the winning column's residual sketch (rows j..31) | its tail norm^2
    alignas(16) double part[2][QP_B][NWP];        // panel: per wave partial x^T a_c, [column][wave]
    alignas(16) double prow[2][QP_B];             // panel: row k + j of the panel before step j
    int sel[QP_B];
};

// dlarfg for (alpha, sum of squares below): H = I - tau v v^T, v = (1, x * scale), H (alpha, x) = (beta, 0).
// 1 / sqrt and 1 / (alpha - beta) by v_rsq_f64 / v_rcp_f64 + NEWTON Newton steps instead of the IEEE sqrt and two divisions (60
// dependent instructions on every lane, on the critical path of every step): NEWTON = 2 is good to an ulp or two -- tau, beta and
// the reflector stay consistent to working precision, which is what the orthogonality of H needs --, NEWTON = 1 (sketch: the
// selection only ranks columns) to ~1e-8.
template <int NEWTON>
__device__ __forceinline__ void householder(double alpha, double tail2, double& beta, double& tau, double& scale) {
    const double s = fma(alpha, alpha, tail2);
    double r = __builtin_amdgcn_rsq(s);
    const double h = 0.5 * s;
#pragma unroll
    for (int it = 0; it < NEWTON; ++it) r = r * fma(-h * r, r, 1.5);
    double sq = s * r;
    if (NEWTON > 1) sq = fma(0.5 * r, fma(-sq, sq, s), sq);
    const double b = -copysign(sq, alpha);
    const double d = alpha - b;                                        // |alpha| + sqrt(s): no cancellation
    double id = __builtin_amdgcn_rcp(d);
#pragma unroll
    for (int it = 0; it < NEWTON; ++it) id = id * fma(-d, id, 2.0);
    const bool none = tail2 == 0.0;                                    // H = I
    beta = none ? alpha : b;
    tau = none ? 0.0 : d * copysign(r, alpha);                         // (beta - alpha) / beta = -d / beta = d * sign(alpha) / sqrt(s)
    scale = none ? 0.0 : id;
}

// the steps exchange data through LDS only: a barrier that does not drain the vector memory queue (__syncthreads() is s_waitcnt vmcnt(0)
// lgkmcnt(0) + s_barrier: it would park every wave until its global stores / loads have completed)
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// ---- selection: step J of the column-pivoted QR of the sketch ----
// A lane owns CPL columns, col_q = t + 64 NW q (q < CPL), each as QP_SEL registers: the workgroup stays at one wave per SIMD up to
// n = 1024 (NW = 4, CPL = 4).  With one column per lane n = 576 needs 9-10 waves, three on a SIMD, and a step costs what the three
// issue one after the other (24-row selection: 44.3 us per panel against 38.3 for 3 waves x 3 columns).
template <int J, int NW, int CPL>
__device__ __forceinline__ void select_step(double (&y)[CPL][QP_SEL], unsigned& live, int t, int lane, int wave, PanelShared<NW>& sh) {
    constexpr int par = J & 1;
    unsigned long long key = 0ULL; int bq = 0; double btail = 0.0;
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
        double tl[4] = {0.0, 0.0, 0.0, 0.0};                         // four chains: a dependent fp64 FMA every ~8 clk, an independent one every 4
#pragma unroll
        for (int i = J + 1; i < QP_SEL; ++i) tl[i & 3] = fma(y[q][i], y[q][i], tl[i & 3]);
        const double tail = (tl[0] + tl[1]) + (tl[2] + tl[3]);
        const double nrm2 = fma(y[q][J], y[q][J], tail);
        // {norm^2 with its low 11 bits dropped | 1024 - column}: one maximum decides, the lowest column wins a tie
        const unsigned long long kq = ((live >> q) & 1u) ? (((unsigned long long)__double_as_longlong(nrm2) & ~0x7FFULL) | (unsigned long long)(1024 - (t + 64 * NW * q))) : 0ULL;
        if (kq > key) { key = kq; bq = q; btail = tail; }
    }
    const unsigned long long wmax = wave_max_u64(key);
    // Two barriers per step: every wave's candidate publishes its KEY, all waves pick the winner, and only the winning wave's candidate lane
    // publishes its column.  Publishing every candidate's column before the winner is known saved the second barrier but put NW columns on the
    // CU's one LDS pipeline per step (an LDS store costs the pipeline the same whether one lane is active or 64):
    // 26.7 -> 25.2 us per panel at N = 256, 40.3 -> 39.0 at N = 576.
    const bool cand_ = wmax != 0ULL && key == wmax;
    if (cand_) sh.key[par][wave] = wmax;
    if (wmax == 0ULL && lane == 0) sh.key[par][wave] = 0ULL;
    lds_barrier();
    unsigned long long best = sh.key[par][0]; int ww = 0;
#pragma unroll
    for (int q = 1; q < NW; ++q) { const unsigned long long o = sh.key[par][q]; if (o > best) { best = o; ww = q; } }
    if (cand_ && wave == ww) {
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
            if (bq == q) {
#pragma unroll
                for (int i = J & ~1; i < QP_SEL; i += 2) *reinterpret_cast<double2*>(&sh.cand[par][i]) = double2{y[q][i], y[q][i + 1]};
            }
        }
        sh.cand[par][QP_SEL] = btail;
    }
    lds_barrier();
    const int pcol = 1024 - (int)(best & 0x7FFULL);
    const double* xs = sh.cand[par];
    double x[QP_SEL];
#pragma unroll
    for (int i = J & ~1; i < QP_SEL; i += 2) { const double2 v = *reinterpret_cast<const double2*>(&xs[i]); x[i] = v.x; x[i + 1] = v.y; }
    double beta, tau, scale;
    householder<1>(x[J], xs[QP_SEL], beta, tau, scale);
    const double st = -scale * tau;
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
        double dt[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = J + 1; i < QP_SEL; ++i) dt[i & 3] = fma(x[i], y[q][i], dt[i & 3]);
        const double dot = (dt[0] + dt[1]) + (dt[2] + dt[3]);
        const double cf = st * fma(scale, dot, y[q][J]);             // y_i -= v_i * tau * (v^T y), v_i = x_i * scale
#pragma unroll
        for (int i = J + 1; i < QP_SEL; ++i) y[q][i] = fma(x[i], cf, y[q][i]);
        if (t + 64 * NW * q == pcol) live &= ~(1u << q);
    }
    if (lane == 0 && wave == 0) sh.sel[J] = pcol;
}

// ---- selection on a compacted sketch: ONE wave, no workgroup barrier in the step ----
// Late panels (<4, 1>, n - k <= QP_CMAX = 64 live columns): the live columns stand in rank order (= column order) in an LDS buffer, lane j
// of wave 0 holds the j-th of them with its ORIGINAL column index mc, and wave 0 runs the 16 steps alone: the wave maximum of the keys is
// the winner in every lane, the winner's lane puts its column into cand[] and the wave reads it back -- LDS accesses of one wave execute
// in order, s_waitcnt lgkmcnt(0) is all the exchange needs.  The other waves wait at the barrier that closes the selection.
// The bits are select_step's: norms, dots and updates are lane-local per column and written exactly as there; the key {norm^2 without
// its low 11 bits | 1024 - column} carries the original column and is unique per live column, and a maximum of distinct keys does not
// depend on which lane holds which column or on the order of the comparisons; the Householder scalars come from the same published
// numbers (the winner's column and its lane-local tail).  Hence sel[], and with it L, d, R and jpvt, are bit for bit those of the
// uncompacted selection.  (Two columns per lane for 64 < n - k <= 128 were measured and lost: DESIGN.md 5.7.)
constexpr int QP_CMAX = 64;      // live columns up to which the selection is compacted
template <int J, int NW>
__device__ __forceinline__ void select_step_cw(double (&y)[QP_SEL], bool& live, int mc, int lane, PanelShared<NW>& sh) {
    constexpr int par = J & 1;
    double tl[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = J + 1; i < QP_SEL; ++i) tl[i & 3] = fma(y[i], y[i], tl[i & 3]);
    const double tail = (tl[0] + tl[1]) + (tl[2] + tl[3]);
    const double nrm2 = fma(y[J], y[J], tail);
    const unsigned long long key = live ? (((unsigned long long)__double_as_longlong(nrm2) & ~0x7FFULL) | (unsigned long long)(1024 - mc)) : 0ULL;
    const unsigned long long best = wave_max_u64(key);
    if (best != 0ULL && key == best) {                               // one lane: keys of live columns are distinct
#pragma unroll
        for (int i = J & ~1; i < QP_SEL; i += 2) *reinterpret_cast<double2*>(&sh.cand[par][i]) = double2{y[i], y[i + 1]};
        sh.cand[par][QP_SEL] = tail;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const int pcol = 1024 - (int)(best & 0x7FFULL);
    const double* xs = sh.cand[par];
    double x[QP_SEL];
#pragma unroll
    for (int i = J & ~1; i < QP_SEL; i += 2) { const double2 v = *reinterpret_cast<const double2*>(&xs[i]); x[i] = v.x; x[i + 1] = v.y; }
    double beta, tau, scale;
    householder<1>(x[J], xs[QP_SEL], beta, tau, scale);
    const double st = -scale * tau;
    double dt[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = J + 1; i < QP_SEL; ++i) dt[i & 3] = fma(x[i], y[i], dt[i & 3]);
    const double dot = (dt[0] + dt[1]) + (dt[2] + dt[3]);
    const double cf = st * fma(scale, dot, y[J]);
#pragma unroll
    for (int i = J + 1; i < QP_SEL; ++i) y[i] = fma(x[i], cf, y[i]);
    if (mc == pcol) live = false;
    if (lane == 0) sh.sel[J] = pcol;
    asm volatile("" ::: "memory");                                   // the reads of cand[par] stay in front of the stores of step J + 2
}
// wave 0 after the compaction: lane j < nl takes the j-th live column out of cy[i][j] / ci[j] (into the registers of the column it
// loaded), then the 16 steps
template <int NW>
__device__ __forceinline__ void select_compacted(double (&y)[QP_SEL], const double* cy, const int* ci, int nl, int lane, PanelShared<NW>& sh QP_QST_PARAM) {
    bool live = lane < nl;
    const int sc = live ? lane : 0;
#pragma unroll
    for (int i = 0; i < QP_SEL; ++i) { const double v = cy[i * QP_CMAX + sc]; y[i] = live ? v : 0.0; }
    const int mc = live ? ci[sc] : -1;
    QST(1)
#define QP_CSTEP(J) select_step_cw<J, NW>(y, live, mc, lane, sh); QST(2 + J)
    QP_CSTEP(0) QP_CSTEP(1) QP_CSTEP(2) QP_CSTEP(3) QP_CSTEP(4) QP_CSTEP(5) QP_CSTEP(6) QP_CSTEP(7)
    QP_CSTEP(8) QP_CSTEP(9) QP_CSTEP(10) QP_CSTEP(11) QP_CSTEP(12) QP_CSTEP(13) QP_CSTEP(14) QP_CSTEP(15)
#undef QP_CSTEP
}

// ---- panel: Householder step J on the 16 selected columns ----
// a[b][16]: rows 64 NW b + 64 wave + 16 g + idx of column sel[c] (b < CPL: a lane owns one 16-row block in each "layer" of 64 NW rows);
// diag bit b: that block is the panel's own rows k .. k + 15; rows above the panel (r < k) hold zeros.  x = column J below row k + J:
// all sources are the registers a[][] themselves (row_newbcast:J picks lane J of the 16-lane row); the rows <= k + J of the diagonal
// block are kept out by summing them separately (dots) / by a zero factor (update).
// The reflector tails stay UNSCALED in the registers (v_c = x_c * myscale below the diagonal, myscale kept by the lanes of column c,
// applied at the write-out): no per-step scaling pass, and v_c^T v_J = myscale_c (x_c[k+J] + scale_J x_c^T x_J) comes out of the same dots.
template <int J, int NW, int CPL>
__device__ __forceinline__ void panel_step(double (&a)[CPL][16], double (&trow)[QP_B], double& myscale, unsigned diag, unsigned blk_live, int c, int g, int wave,
                                           PanelShared<NW>& sh, double* tau_out) {
    constexpr int par = J & 1;
    if (blk_live) {
        double acc = 0.0;
#pragma unroll
        for (int b = 0; b < CPL; ++b) {
            if ((blk_live >> b) & 1u) {                                // wave-uniform: blocks above the panel are skipped
                double dlo0 = 0.0, dlo1 = 0.0, dhi0 = 0.0, dhi1 = 0.0;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    if (i <= J) { if (i & 1) dpp_fmac_self<J>(dlo1, a[b][i]); else dpp_fmac_self<J>(dlo0, a[b][i]); }
                    else { if (i & 1) dpp_fmac_self<J>(dhi1, a[b][i]); else dpp_fmac_self<J>(dhi0, a[b][i]); }
                }
                acc += (dhi0 + dhi1) + (((diag >> b) & 1u) ? 0.0 : dlo0 + dlo1);
                if ((diag >> b) & 1u) sh.prow[par][c] = a[b][J];
            }
        }
        const double part = rows4_sum(acc);
        if (g == 0) sh.part[par][c][wave] = part;
    } else if (g == 0) sh.part[par][c][wave] = 0.0;
    lds_barrier();
    double s_c = sh.part[par][c][0], s_j = sh.part[par][J][0];
#pragma unroll
    for (int q = 1; q < NW; ++q) { s_c += sh.part[par][c][q]; s_j += sh.part[par][J][q]; }
    const double alpha = sh.prow[par][J], apc = sh.prow[par][c];
    double beta, tau, scale;
    householder<2>(alpha, s_j, beta, tau, scale);
    const double zc = fma(scale, s_c, apc);                           // c > J: v_J^T a_c; c < J: v_J^T x_c (x_c = the unscaled tail of v_c)
    if (c == J) myscale = scale;
    if (blk_live) {
        const double mcf = c > J ? -scale * tau * zc : 0.0;
#pragma unroll
        for (int b = 0; b < CPL; ++b) {
            if ((blk_live >> b) & 1u) {
                const bool isd = (diag >> b) & 1u;
                const double mlo = isd ? 0.0 : mcf;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    if (i <= J) dpp_axpy_self<J>(a[b][i], mlo);
                    else dpp_axpy_self<J>(a[b][i], mcf);
                }
                const double newd = c > J ? fma(-tau, zc, a[b][J]) : beta;   // row k + J: v = 1
                a[b][J] = (isd && c >= J) ? newd : a[b][J];
                dpp_fence(a[b]);
            }
        }
    }
    // compact WY: T[0:J, J] = -tau T[0:J, 0:J] (V^T v_J), T[J][J] = tau; lane c keeps row c of T
    if (wave == 0) {
        double zt = myscale * zc;                                     // (V^T v_J)_c for c < J
        double tj = 0.0;
        dpp_fence1(zt);
        t_row_dot(tj, trow, zt, std::make_integer_sequence<int, J>{});
        trow[J] = c < J ? -tau * tj : (c == J ? tau : 0.0);
        if (g == 0 && c == J) tau_out[J] = tau;
    }
}

}  // namespace

// per-chain workspace (doubles): the sketch Y [QP_SR][n], twice (the fused step reads the buffer of the panel's parity and writes the other
// one) | Qacc [n][n] | the ticket counter of the fused step (one word, 16-byte slot) | two-launch form only: the clean reflector panels
// column-major [n][n] | the T factors [QP_B][n] | the panels row-major [n][n]
__host__ __device__ __forceinline__ long qp_off_qacc(int n) { return 2L * QP_SR * n; }
__host__ __device__ __forceinline__ long qp_off_ticket(int n) { return qp_off_qacc(n) + (long)n * n; }
__host__ __device__ __forceinline__ long qp_off_vp(int n) { return qp_off_ticket(n) + 2; }
__host__ __device__ __forceinline__ long qp_off_tm(int n) { return qp_off_vp(n) + (long)n * n; }
__host__ __device__ __forceinline__ long qp_off_vtp(int n) { return qp_off_tm(n) + (long)QP_B * n; }


// The selection and the factorisation of the panel that starts at step k, by one workgroup of NW waves (64 NW CPL >= n: a lane owns CPL
// columns in the selection and CPL 16-row blocks of one column in the panel).  Reads Y, pivpos and rows >= k of the selected columns of A;
// writes nothing but tau_out[0..15] and leaves the factored panel in registers: lane (c, g) of every wave holds a[b][i] = rows
// 64 NW b + 64 wave + 16 g + i of column mycol = sel[c] (R0 / beta on and above the column's diagonal, the UNSCALED reflector tail below:
// times myscale), wave 0 holds row c of T in trow.  Every global load has landed when step 0 of the panel passes its barrier;
// pre() runs once the first round of loads (sketch, pivpos) is issued and before anything is waited for -- true: the workgroup leaves, the
// function returns false --, mid() right after step 0 of the panel.  qp_panel_kernel and qp_step_kernel both call this body, so they factor bit for bit alike.
//
// CMP (the <4, 1> instances: 128 < n <= 256) with cy != nullptr: a panel with n - k <= QP_CMAX live columns compacts them into cy / ci (LDS:
// QP_SEL x QP_CMAX doubles, QP_CMAX ints, dead before and after the selection) and wave 0 alone selects (select_step_cw: the same bits).
// The live count is n - k by construction -- every earlier panel retired 16 columns --, so the mode is workgroup-uniform and nothing is counted.
template <int NW, int CPL, bool CMP, class Pre, class Mid>
__device__ __forceinline__ bool qp_factor_panel(const double* A, const double* __restrict__ Y, const int* pivpos, int n, int k, PanelShared<NW>& sh,
                                                double* tau_out, double (&a)[CPL][16], double (&trow)[QP_B], double& myscale, unsigned& diag, int& mycol,
                                                double* cy, int* ci, Pre&& pre, Mid&& mid QP_QST_PARAM) {
    static_assert(!CMP || (NW == 4 && CPL == 1), "the compacted selection is written for one column per lane in four waves");
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const bool compact = CMP && cy != nullptr && n - k <= QP_CMAX;      // workgroup-uniform
    QST(0)
    // ---- selection ----
    {
        unsigned live = 0u;
        double y[CPL][QP_SEL]; int pp[CPL];
        int ppw[CMP ? 4 : 1];                                        // CMP: pivpos of this lane's column in EVERY wave, same round of loads: the wave offsets of the ranks need no exchange
        if (CMP) {
            if (compact) {
#pragma unroll
                for (int w = 0; w < 4; ++w) { const int col = lane + 64 * w; ppw[w] = pivpos[col < n ? col : n - 1]; }
            }
        }
#pragma unroll
        for (int q = 0; q < CPL; ++q) {                              // one round of loads: clamped addresses, masked afterwards
            const int col = t + 64 * NW * q, cc = col < n ? col : n - 1;
#pragma unroll
            for (int i = 0; i < QP_SEL; ++i) y[q][i] = Y[(long)i * n + cc];
            pp[q] = pivpos[cc];
        }
        if (pre()) return false;                                     // (workgroup-uniform)
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
            const int col = t + 64 * NW * q;
            if (col < n && pp[q] < 0) live |= 1u << q;
            if (col >= n) {
#pragma unroll
                for (int i = 0; i < QP_SEL; ++i) y[q][i] = 0.0;
            }
        }
        if (y[0][0] == 1.2345e300) live = 0u;                            // (stamps: forces the loads to have landed before the first stamp)
        bool selected = false;
        if constexpr (CMP) {
            if (compact) {
                QST(39)
                // rank of a live column among the live ones, in column order: live lanes below it in its wave + the live counts of the waves below
                int rank = 0, tot = 0;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const unsigned long long b = __ballot(lane + 64 * w < n && ppw[w] < 0);
                    rank += w < wave ? __popcll(b) : (w == wave ? __popcll(b & ((1ULL << lane) - 1ULL)) : 0);
                    tot += __popcll(b);
                }
                const int nl = tot < QP_CMAX ? tot : QP_CMAX;        // counted, = n - k: wave 0 reads no slot that nobody wrote, whatever pivpos holds
                if ((live & 1u) && rank < QP_CMAX) {                 // (rank < n - k <= QP_CMAX always: the bound keeps a corrupt pivpos inside the buffer)
#pragma unroll
                    for (int i = 0; i < QP_SEL; ++i) cy[i * QP_CMAX + rank] = y[0][i];
                    ci[rank] = t;
                }
                lds_barrier();
                if (wave == 0) select_compacted<NW>(y[0], cy, ci, nl, lane, sh QP_QST_ARG);
                selected = true;
            }
        }
        if (!selected) {
            QST(1)
#define QP_SEL_STEP(J) select_step<J, NW, CPL>(y, live, t, lane, wave, sh); QST(2 + J)
            QP_SEL_STEP(0) QP_SEL_STEP(1) QP_SEL_STEP(2) QP_SEL_STEP(3) QP_SEL_STEP(4) QP_SEL_STEP(5) QP_SEL_STEP(6) QP_SEL_STEP(7)
            QP_SEL_STEP(8) QP_SEL_STEP(9) QP_SEL_STEP(10) QP_SEL_STEP(11) QP_SEL_STEP(12) QP_SEL_STEP(13) QP_SEL_STEP(14) QP_SEL_STEP(15)
#undef QP_SEL_STEP
        }
    }
    lds_barrier();
    // ---- panel ----
    const int c = lane & 15, g = lane >> 4;
    mycol = sh.sel[c];
    myscale = 0.0; diag = 0u;
    unsigned blk_live = 0u;
#pragma unroll
    for (int b = 0; b < CPL; ++b) {
        const int r0 = 64 * NW * b + 64 * wave + 16 * g;
        if (r0 == k) diag |= 1u << b;
        if (64 * NW * b + 64 * wave + 64 > k && 64 * NW * b + 64 * wave < n) blk_live |= 1u << b;   // wave-uniform: some row of the wave's 64 is in the panel
        const double2* src = reinterpret_cast<const double2*>(A + (long)n * mycol + r0);      // 16 contiguous rows of one column: n and r0 are multiples of 16, so 16-byte pieces
        const bool rows_live = r0 >= k && r0 < n;
#pragma unroll
        for (int i = 0; i < 16; i += 2) { const double2 v = rows_live ? src[i >> 1] : double2{0.0, 0.0}; a[b][i] = v.x; a[b][i + 1] = v.y; }
        dpp_fence(a[b]);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // every wave, also one whose blocks all lie above the panel: nothing of this workgroup's is in flight past step 0
#pragma unroll
    for (int i = 0; i < QP_B; ++i) trow[i] = 0.0;
#ifdef DQ_QP_STAMPS
    if (a[0][0] == 1.2345e300) myscale = 1.0;
#endif
    QST(18)
#define QP_PAN(J) panel_step<J, NW, CPL>(a, trow, myscale, diag, blk_live, c, g, wave, sh, tau_out); QST(19 + J)
    QP_PAN(0)
    mid();
    QP_PAN(1) QP_PAN(2) QP_PAN(3) QP_PAN(4) QP_PAN(5) QP_PAN(6) QP_PAN(7)
    QP_PAN(8) QP_PAN(9) QP_PAN(10) QP_PAN(11) QP_PAN(12) QP_PAN(13) QP_PAN(14) QP_PAN(15)
#undef QP_PAN
    return true;
}

// Two-launch form, first launch: one workgroup per chain selects and factors the panel and writes it out for qp_update_kernel.
template <int NW, int CPL>
__global__ __launch_bounds__(64 * NW) void qp_panel_kernel(Mat Am, QrWork w, int n, int k) {
    __shared__ PanelShared<NW> sh;
    const int chain = blockIdx.y;
    double* __restrict__ A = Am.at(chain);
    double* __restrict__ pw = w.pw + (long)chain * w.pw_stride;
    const double* __restrict__ Y = pw;                         // [QP_SR][n]
    double* __restrict__ Vp = pw + qp_off_vp(n) + (long)n * k;                    // [n][QP_B] column-major clean copy of THIS panel's reflectors
    double* __restrict__ Tm = pw + qp_off_tm(n) + (long)QP_B * k;                 // [QP_B][QP_B] column-major, one per panel
    double* __restrict__ VTp = pw + qp_off_vtp(n) + (long)n * k;                  // the same panel row-major ([n][QP_B]): the operand of V^T A is read along its rows
    int* __restrict__ pivpos = w.pivpos + (long)chain * w.pivpos_stride;
    double* tau = w.tau + (long)chain * w.tau_stride;
    int* jpvt = w.jpvt + (long)chain * w.jpvt_stride;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int c = lane & 15, g = lane >> 4;

#ifdef DQ_QP_STAMPS
    __shared__ unsigned long long qst[40];
#endif
    double a[CPL][16], trow[QP_B], myscale;
    unsigned diag; int mycol;
    constexpr bool CMP = NW == 4 && CPL == 1;                  // late panels select on a compacted sketch (qp_factor_panel); the other instances name no buffer
    __shared__ double s_cy[CMP ? QP_SEL * QP_CMAX : 1];
    __shared__ int s_ci[CMP ? QP_CMAX : 1];
    double* cy = nullptr; int* ci = nullptr;
    if constexpr (CMP) { if (w.pw_compact) { cy = s_cy; ci = s_ci; } }
    qp_factor_panel<NW, CPL, CMP>(A, Y, pivpos, n, k, sh, tau + k, a, trow, myscale, diag, mycol, cy, ci, [] { return false; }, [] {} QP_QST_ARG);
    // ---- write-out: R0 / beta / reflectors in place, the clean reflector panel (unit diagonal, zeros above), T, jpvt, pivpos ----
#pragma unroll
    for (int b = 0; b < CPL; ++b) {
        const int r0 = 64 * NW * b + 64 * wave + 16 * g;
        if (r0 >= k && r0 < n) {
            const bool isd = (diag >> b) & 1u;
            double2* dst = reinterpret_cast<double2*>(A + (long)n * mycol + r0);
            double2* vdst = reinterpret_cast<double2*>(Vp + (long)n * c + r0);
            double v[16], vc[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const bool below = !isd || i > c;                         // strictly below the column's diagonal: the reflector tail
                v[i] = below ? a[b][i] * myscale : a[b][i];
                vc[i] = below ? v[i] : (i == c ? 1.0 : 0.0);
                VTp[(long)QP_B * (r0 + i) + c] = vc[i];
            }
#pragma unroll
            for (int i = 0; i < 16; i += 2) { dst[i >> 1] = double2{v[i], v[i + 1]}; vdst[i >> 1] = double2{vc[i], vc[i + 1]}; }
        }
    }
    if (wave == 0 && g == 0) {
#pragma unroll
        for (int i = 0; i < QP_B; ++i) Tm[c + QP_B * i] = trow[i];
        jpvt[k + c] = mycol;
        pivpos[mycol] = k + c;
    }
#ifdef DQ_QP_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    QST(35)
    __syncthreads();
    if (t == 0 && k == DQ_QP_STAMP_K && blockIdx.y == 0) {
        if (cy != nullptr && n - k <= QP_CMAX) printf("panel k=%d n=%d: compaction (ranks, LDS pass, barrier, wave 0's read-back) %llu of the load segment\n", k, n, qst[1] - qst[39]);
        printf("panel k=%d n=%d (100 MHz ticks x 24 = clk @2.4GHz): load Y %llu | sel steps", k, n, qst[1] - qst[0]);
        for (int j = 0; j < 16; ++j) printf(" %llu", qst[2 + j] - qst[1 + j]);
        printf(" | gather %llu | panel steps", qst[18] - qst[17]);
        for (int j = 0; j < 16; ++j) printf(" %llu", qst[19 + j] - qst[18 + j]);
        printf(" | write-out %llu | total %llu\n", qst[35] - qst[34], qst[35] - qst[0]);
    }
#endif
}

// grid.x = n / 16 column blocks, QP_UW waves each.  UPDATE: A[k:, cols] <- (I - V T V^T)^T A[k:, cols] for the live columns of the block, then
// the sketch of rows >= k + 16 of the result; !UPDATE (before the first panel): pivpos = -1 and the sketch of A itself.
// A wave keeps its row tiles (tile rt = wave + QP_UW ti, ti < TPW) in registers in the accumulator layout from the first load on: the same
// registers are the B operand of W = V^T A (k-step s <-> row kk + 4 s of the tile: any partition of k works as long as V is fed the same
// way), the accumulator of A - V W', and the B operand of the sketch product.
constexpr int QP_UW = 8;      // waves per workgroup of the update kernel (4: 6.7 us at n = 256 against 6.3; 16: 8.3)
constexpr int QP_YT = QP_SR / 16;

// The Q role of an update launch: column block cb of Qacc (n x n, column-major like A; it holds rows >= k of H_{k/16-1}^T ... H_0^T I, the
// identity before the first factor -- formed in registers then, nothing is cleared) gets the factor of panel k exactly as the
// trailing matrix does, without a pivot test, a sketch or an early exit.  The later factors start below row k + 16, so rows k .. k + 15
// of Q^T are final: that tile goes transposed into columns k .. k + 15 of L = Q (the 16 lanes of one (kk, r) write 128 contiguous
// bytes), the tiles below go back to Qacc for the next launch.  Loads first, as in the A role: one cold round.
template <int TPW>
__device__ __forceinline__ void qp_q_role(double (&red)[QP_UW][QP_YT * 4][64], double* __restrict__ Qacc, double* __restrict__ L,
                                          const double* __restrict__ Vp, const double* __restrict__ VTp, const double* __restrict__ Tm,
                                          int n, int k, int cb) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int r16 = lane & 15, kk = lane >> 4;
    const int col = 16 * cb + r16;
    double* __restrict__ Qc = Qacc + (long)n * col;
    const int m_tiles = (n - k) / 16;
    d4 Qt[TPW]; double v1[TPW][4], v2[TPW][4], tv[4];
#pragma unroll
    for (int ti = 0; ti < TPW; ++ti) {
        const int rt = wave + QP_UW * ti;
        Qt[ti] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < 4; ++s) { v1[ti][s] = 0.0; v2[ti][s] = 0.0; }
        if (rt < m_tiles) {
            const int r0 = k + 16 * rt;
#pragma unroll
            for (int r = 0; r < 4; ++r) Qt[ti][r] = Qc[r0 + kk + 4 * r];     // loaded at k = 0 as well (whatever the last factorisation left) and replaced below: a branch here would put a wait between the rounds of loads
#pragma unroll
            for (int s = 0; s < 4; ++s) { v1[ti][s] = VTp[(long)QP_B * (r0 + kk + 4 * s) + r16]; v2[ti][s] = Vp[(long)n * (kk + 4 * s) + (r0 + r16)]; }
        }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) tv[s] = Tm[(kk + 4 * s) + QP_B * r16];
    const bool first = k == 0;                                    // before the first factor the accumulator is the identity: a select, no branch
#pragma unroll
    for (int ti = 0; ti < TPW; ++ti)
#pragma unroll
        for (int r = 0; r < 4; ++r) Qt[ti][r] = first ? ((16 * (wave + QP_UW * ti) + kk + 4 * r == col) ? 1.0 : 0.0) : Qt[ti][r];
    d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ti = 0; ti < TPW; ++ti) {
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(v1[ti][s], Qt[ti][s], acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][r][lane] = acc[r];
    __syncthreads();
    d4 W;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        double v = red[0][r][lane];
#pragma unroll
        for (int q = 1; q < QP_UW; ++q) v += red[q][r][lane];
        W[r] = v;
    }
    d4 wp = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < 4; ++s) wp = __builtin_amdgcn_mfma_f64_16x16x4f64(tv[s], W[s], wp, 0, 0, 0);
    wp = -wp;
#pragma unroll
    for (int ti = 0; ti < TPW; ++ti) {
        const int rt = wave + QP_UW * ti;
        if (rt < m_tiles) {
            const int r0 = k + 16 * rt;
#pragma unroll
            for (int s = 0; s < 4; ++s) Qt[ti] = __builtin_amdgcn_mfma_f64_16x16x4f64(v2[ti][s], wp[s], Qt[ti], 0, 0, 0);
            if (rt == 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) L[(long)n * (k + kk + 4 * r) + col] = Qt[ti][r];     // Q[col][k + kk + 4 r] = Q^T[k + kk + 4 r][col]
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) Qc[r0 + kk + 4 * r] = Qt[ti][r];
            }
        }
    }
}

// blockIdx.x >= q_first: the workgroup has the Q role on column block blockIdx.x - q_first (uniform per workgroup)
template <bool UPDATE, int TPW>
__global__ __launch_bounds__(64 * QP_UW) void qp_update_kernel(Mat Am, QrWork w, int n, int k, Mat Lm, int q_first) {
    constexpr int YT = QP_YT;
    __shared__ double red[QP_UW][YT * 4][64];                  // per wave partial tiles (W: 4 registers, Y: 4 YT registers)
    const int chain = blockIdx.y;
    double* __restrict__ pw = w.pw + (long)chain * w.pw_stride;
    if (UPDATE && (int)blockIdx.x >= q_first) {
        qp_q_role<TPW>(red, pw + qp_off_qacc(n), Lm.at(chain), pw + qp_off_vp(n) + (long)n * k, pw + qp_off_vtp(n) + (long)n * k,
                       pw + qp_off_tm(n) + (long)QP_B * k, n, k, (int)blockIdx.x - q_first);
        return;
    }
    double* __restrict__ A = Am.at(chain);
    double* __restrict__ Y = pw;
    const double* __restrict__ Vp = pw + qp_off_vp(n) + (long)n * k;
    const double* __restrict__ Tm = pw + qp_off_tm(n) + (long)QP_B * k;
    const double* __restrict__ VTp = pw + qp_off_vtp(n) + (long)n * k;
    int* __restrict__ pivpos = w.pivpos + (long)chain * w.pivpos_stride;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int r16 = lane & 15, kk = lane >> 4;
    const int col = 16 * blockIdx.x + r16;
    double* __restrict__ Ac = A + (long)n * col;
    const int m_tiles = (n - k) / 16;
    // every global load of the launch is issued here, before the first use: the operands were written by the previous kernel (another
    // CU, mostly another XCD), so each dependent round of loads costs a cold miss (~2 us) -- one round instead of three
    int pp = -1;
    if (UPDATE) pp = pivpos[col];
    d4 At[TPW]; double v1[TPW][4], v2[TPW][4], tv[4];
#pragma unroll
    for (int ti = 0; ti < TPW; ++ti) {
        const int rt = wave + QP_UW * ti;
        At[ti] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < 4; ++s) { v1[ti][s] = 0.0; v2[ti][s] = 0.0; }
        if (rt < m_tiles) {
            const int r0 = k + 16 * rt;
#pragma unroll
            for (int r = 0; r < 4; ++r) At[ti][r] = Ac[r0 + kk + 4 * r];
            if (UPDATE) {
#pragma unroll
                for (int s = 0; s < 4; ++s) { v1[ti][s] = VTp[(long)QP_B * (r0 + kk + 4 * s) + r16]; v2[ti][s] = Vp[(long)n * (kk + 4 * s) + (r0 + r16)]; }   // both along the lanes' fast index
            }
        }
    }
    if (UPDATE) {
#pragma unroll
        for (int s = 0; s < 4; ++s) tv[s] = Tm[(kk + 4 * s) + QP_B * r16];
    }
    const bool live_col = pp < 0;
    if (UPDATE) { if (__ballot(live_col) == 0ULL) return; }   // every wave sees the same 16 columns: a uniform exit
    else if (t < 16) pivpos[col] = -1;
    d4 wp = {0.0, 0.0, 0.0, 0.0};
    if (UPDATE) {
        d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int ti = 0; ti < TPW; ++ti) {
#pragma unroll
            for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(v1[ti][s], At[ti][s], acc, 0, 0, 0);     // tiles beyond the matrix hold zeros
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave][r][lane] = acc[r];
        __syncthreads();
        d4 W;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double v = red[0][r][lane];
#pragma unroll
            for (int q = 1; q < QP_UW; ++q) v += red[q][r][lane];
            W[r] = live_col ? v : 0.0;
        }
        // W' = T^T W: a = T[i = kk + 4 s][i' = r16], b = W[kk + 4 s][c] (the accumulator registers as they are)
#pragma unroll
        for (int s = 0; s < 4; ++s) wp = __builtin_amdgcn_mfma_f64_16x16x4f64(tv[s], W[s], wp, 0, 0, 0);
        wp = -wp;                                                 // A - V W'
        __syncthreads();
    }
    d4 ya[YT];
#pragma unroll
    for (int yt = 0; yt < YT; ++yt) ya[yt] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ti = 0; ti < TPW; ++ti) {
        const int rt = wave + QP_UW * ti;
        if (rt < m_tiles) {
            const int r0 = k + 16 * rt;
            if (UPDATE) {
#pragma unroll
                for (int s = 0; s < 4; ++s) At[ti] = __builtin_amdgcn_mfma_f64_16x16x4f64(v2[ti][s], wp[s], At[ti], 0, 0, 0);
                if (live_col) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) Ac[r0 + kk + 4 * r] = At[ti][r];
                }
            }
            if (!UPDATE || rt >= 1) {                              // rows of the NEXT trailing matrix: sketch them while they are in registers
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const unsigned bits = qp_row_bits((unsigned)(r0 + kk + 4 * s));
#pragma unroll
                    for (int yt = 0; yt < YT; ++yt) ya[yt] = __builtin_amdgcn_mfma_f64_16x16x4f64(qp_sign(bits, 16 * yt + r16), At[ti][s], ya[yt], 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int yt = 0; yt < YT; ++yt)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave][4 * yt + r][lane] = ya[yt][r];
    __syncthreads();
    for (int idx = t; idx < YT * 4 * 64; idx += 64 * QP_UW) {
        const int l = idx & 63, q = idx >> 6, yt = q >> 2, r = q & 3;
        double v = red[0][q][l];
#pragma unroll
        for (int qq = 1; qq < QP_UW; ++qq) v += red[qq][q][l];
        Y[(long)(16 * yt + (l >> 4) + 4 * r) * n + 16 * blockIdx.x + (l & 15)] = v;
    }
}

// ---- fused form: one launch per panel ----
// Grid and roles as qp_update_kernel<true>'s, NW waves.  The panel's inputs (the sketch of parity k / 16, pivpos, rows >= k of the selected
// columns) are visible to every workgroup when the launch starts and the factorisation is deterministic, so EVERY workgroup factors the
// panel itself (qp_factor_panel: bit for bit what qp_panel_kernel computes), keeps the clean reflector panel and T in LDS and goes straight
// on to its own column block: no panel launch, no reflector panels in global memory, no cold read-back, and no workgroup ever waits for
// another.  What makes that safe in place -- nothing the factorisation reads may be written while some workgroup has yet to read it:
//   sketch   two buffers: the step reads parity k / 16 and writes the other one;
//   A        the update stores only to live columns, the factorisation gathers only the 16 selected ones, and a selected column counts
//            as retired in every workgroup (sel[] in LDS);
//   R0 / beta in place (rows k .. k + 15 of the selected columns, read by assemble_r_kernel), tau, jpvt, pivpos: written by the workgroup
//            that draws the LAST ticket of the launch from the chain's counter.  A ticket is drawn after all global loads of the workgroup's
//            factorisation have landed (past step 0 of the panel, consumed at the end: the round trip is hidden), so the last arriver knows
//            that nobody will read those locations again in this launch; it holds the same values as everybody else, consumes nothing from the
//            others (relaxed, no acquire), and the kernel boundary publishes its stores.  It also puts the counter back to zero.
//            A column block whose 16 columns were retired by earlier panels draws its ticket at once and leaves -- unless it is the last.
// The reflector tails below the diagonal of the selected columns are not written at all: Q is accumulated, nothing reads them.
// Phase 2 keeps the update kernel's arithmetic: tile rt belongs to "virtual wave" rt % QP_UW, a wave carries the virtual waves wave, wave + NW,
// ..., each with its own partial sums, and the cross-wave sums run over the QP_UW virtual waves in the same order -- bit-identical results.
// V in LDS: one copy, column c at c * LDV with LDV odd: the operand of V^T A (16 lanes <-> 16 columns at one row) and the operand of V W' (16
// lanes <-> 16 consecutive rows of one column) both hit 16 different banks.
template <int NW, int CPL, int TPW>
__global__ __launch_bounds__(64 * NW) void qp_step_kernel(Mat Am, QrWork w, int n, int k, Mat Lm, int q_first) {
    constexpr int YT = QP_YT;
    constexpr int NV = (QP_UW + NW - 1) / NW;                  // virtual waves per wave
    constexpr int LDV = 64 * NW * CPL + 1;
    __shared__ PanelShared<NW> sh;
    __shared__ double Vs[QP_B * LDV];
    __shared__ double Ts[QP_B * (QP_B + 1)];
    __shared__ double red[QP_UW][YT * 4][64];
    __shared__ double s_tau[QP_B];
    __shared__ unsigned s_ticket;
#ifdef DQ_QP_STAMPS
    __shared__ unsigned long long qst[40];
#endif
    const int chain = blockIdx.y;
    double* pw = w.pw + (long)chain * w.pw_stride;
    const bool qrole = (int)blockIdx.x >= q_first;             // uniform per workgroup
    const int cb = qrole ? (int)blockIdx.x - q_first : (int)blockIdx.x;
    double* A = Am.at(chain);
    const int par = (k / QP_B) & 1;
    const double* __restrict__ Yr = pw + (long)par * QP_SR * n;
    double* __restrict__ Yw = pw + (long)(par ^ 1) * QP_SR * n;
    unsigned* counter = reinterpret_cast<unsigned*>(pw + qp_off_ticket(n));
    int* pivpos = w.pivpos + (long)chain * w.pivpos_stride;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int r16 = lane & 15, kk = lane >> 4;
    const int col = 16 * cb + r16;
    double* Xc = (qrole ? pw + qp_off_qacc(n) : A) + (long)n * col;     // my column of the trailing matrix | of Qacc
    const int m_tiles = (n - k) / 16;
    // the block's own tiles first: the loads overlap the factorisation instead of costing a dependent round after it.  (Issued behind the
    // sketch they would not let the selection start any sooner: the loads sit under wave-uniform conditions, so the compiler cannot
    // count them and waits for all of them before the first use of the sketch either way.)
    const int pp_ld = pivpos[col];
    d4 X[NV][TPW];
#pragma unroll
    for (int vi = 0; vi < NV; ++vi) {
#pragma unroll
        for (int ti = 0; ti < TPW; ++ti) {
            const int vw = wave + NW * vi, rt = vw + QP_UW * ti;
            X[vi][ti] = d4{0.0, 0.0, 0.0, 0.0};
            if (vw < QP_UW && rt < m_tiles) {
#pragma unroll
                for (int r = 0; r < 4; ++r) X[vi][ti][r] = Xc[k + 16 * rt + kk + 4 * r];
            }
        }
    }
    const int pp = qrole ? -1 : pp_ld;
    const unsigned last_ticket = gridDim.x - 1;
    bool have_ticket = false;
    unsigned ticket = 0u;
    // ---- phase 1 ----
    double a[CPL][16], trow[QP_B], myscale;
    unsigned diag; int mycol;
    // late panels of the <4, 1> instance select on a compacted sketch: the buffer is the head of red[][][], which nothing uses before phase 2
    constexpr bool CMP = NW == 4 && CPL == 1;
    static_assert(!CMP || sizeof(red) >= sizeof(double) * QP_SEL * QP_CMAX, "the compaction buffer is the reduction buffer");
    __shared__ int s_ci[CMP ? QP_CMAX : 1];
    double* cy = nullptr; int* ci = nullptr;
    if constexpr (CMP) { if (w.pw_compact) { cy = &red[0][0][0]; ci = s_ci; } }
    const bool factored = qp_factor_panel<NW, CPL, CMP>(A, Yr, pivpos, n, k, sh, s_tau, a, trow, myscale, diag, mycol, cy, ci, [&] {
        // the sketch loads are in flight beside the tiles': the retired test costs no round of its own
        if (__ballot(pp < 0) != 0ULL) return false;            // every wave sees the same 16 columns: uniform
        if (t == 0) s_ticket = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        have_ticket = true;                                     // all 16 columns retired by earlier panels: nothing to update ...
        return s_ticket != last_ticket;                         // ... but the last arriver has the write-out to do: it factors the panel for that alone
    }, [&] {
        if (!have_ticket && t == 0) {
            // a zero offset in a vector register the compiler cannot see through: with a uniform address it turns the atomic into its
            // wave-aggregated form (mbcnt / readfirstlane), which waits for the round trip on the spot instead of at the end of the panel
            long off = 0;
            asm volatile("" : "+v"(off));
            ticket = __hip_atomic_fetch_add(counter + off, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    } QP_QST_ARG);
    if (!factored) return;
    const int c = lane & 15, g = lane >> 4;
#pragma unroll
    for (int b = 0; b < CPL; ++b) {                            // the clean reflector panel: unit diagonal, zeros above
        const int r0 = 64 * NW * b + 64 * wave + 16 * g;
        if (r0 >= k && r0 < n) {
            const bool isd = (diag >> b) & 1u;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const bool below = !isd || i > c;
                Vs[c * LDV + r0 + i] = below ? a[b][i] * myscale : (i == c ? 1.0 : 0.0);
            }
        }
    }
    if (wave == 0 && g == 0) {
#pragma unroll
        for (int i = 0; i < QP_B; ++i) Ts[c + (QP_B + 1) * i] = trow[i];
    }
    if (!have_ticket && t == 0) s_ticket = ticket;
    __syncthreads();
    QST(35)
    if (s_ticket == last_ticket) {                             // uniform: everybody else has read what this overwrites
        double* tau = w.tau + (long)chain * w.tau_stride;
        int* jpvt = w.jpvt + (long)chain * w.jpvt_stride;
#pragma unroll
        for (int b = 0; b < CPL; ++b) {
            if ((diag >> b) & 1u) {                             // this lane holds rows k .. k + 15 of column mycol
#pragma unroll
                for (int i = 0; i < 16; ++i) if (i <= c) A[(long)n * mycol + k + i] = a[b][i];
            }
        }
        if (wave == 0 && g == 0) { jpvt[k + c] = mycol; pivpos[mycol] = k + c; tau[k + c] = s_tau[c]; }
        if (t == 0) *counter = 0u;
        if (have_ticket) return;
    }
    QST(36)
    // ---- phase 2: qp_update_kernel<true> / qp_q_role with V and T from LDS ----
    bool sel_hit = false;
#pragma unroll
    for (int j = 0; j < QP_B; ++j) sel_hit |= sh.sel[j] == col;
    const bool live_col = qrole || (pp < 0 && !sel_hit);
    double tv[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) tv[s] = Ts[(kk + 4 * s) + (QP_B + 1) * r16];
    const bool first = qrole && k == 0;                        // before the first factor the accumulator is the identity: a select, no branch
#pragma unroll
    for (int vi = 0; vi < NV; ++vi)
#pragma unroll
        for (int ti = 0; ti < TPW; ++ti)
#pragma unroll
            for (int r = 0; r < 4; ++r) X[vi][ti][r] = first ? ((16 * (wave + NW * vi + QP_UW * ti) + kk + 4 * r == col) ? 1.0 : 0.0) : X[vi][ti][r];
#pragma unroll
    for (int vi = 0; vi < NV; ++vi) {
        const int vw = wave + NW * vi;
        if (vw < QP_UW) {
            d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int ti = 0; ti < TPW; ++ti) {
                const int rt = vw + QP_UW * ti;
                if (rt < m_tiles) {
                    const double* vrow = Vs + r16 * LDV + (k + 16 * rt + kk);
#pragma unroll
                    for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(vrow[4 * s], X[vi][ti][s], acc, 0, 0, 0);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) red[vw][r][lane] = acc[r];
        }
    }
    __syncthreads();
    d4 W;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        double v = red[0][r][lane];
#pragma unroll
        for (int q = 1; q < QP_UW; ++q) v += red[q][r][lane];
        W[r] = live_col ? v : 0.0;
    }
    d4 wp = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < 4; ++s) wp = __builtin_amdgcn_mfma_f64_16x16x4f64(tv[s], W[s], wp, 0, 0, 0);
    wp = -wp;
    __syncthreads();
    QST(37)
    double* L = Lm.at(chain);
#pragma unroll
    for (int vi = 0; vi < NV; ++vi) {
        const int vw = wave + NW * vi;
        if (vw < QP_UW) {
            d4 ya[YT];
#pragma unroll
            for (int yt = 0; yt < YT; ++yt) ya[yt] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int ti = 0; ti < TPW; ++ti) {
                const int rt = vw + QP_UW * ti;
                if (rt < m_tiles) {
                    const int r0 = k + 16 * rt;
#pragma unroll
                    for (int s = 0; s < 4; ++s) X[vi][ti] = __builtin_amdgcn_mfma_f64_16x16x4f64(Vs[(kk + 4 * s) * LDV + r0 + r16], wp[s], X[vi][ti], 0, 0, 0);
                    if (qrole) {
                        if (rt == 0) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) L[(long)n * (k + kk + 4 * r) + col] = X[vi][ti][r];     // Q[col][k + kk + 4 r] = Q^T[k + kk + 4 r][col]
                        } else {
#pragma unroll
                            for (int r = 0; r < 4; ++r) Xc[r0 + kk + 4 * r] = X[vi][ti][r];
                        }
                    } else {
                        if (live_col) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) Xc[r0 + kk + 4 * r] = X[vi][ti][r];
                        }
                        if (rt >= 1) {                             // rows of the NEXT trailing matrix: sketch them while they are in registers
#pragma unroll
                            for (int s = 0; s < 4; ++s) {
                                const unsigned bits = qp_row_bits((unsigned)(r0 + kk + 4 * s));
#pragma unroll
                                for (int yt = 0; yt < YT; ++yt) ya[yt] = __builtin_amdgcn_mfma_f64_16x16x4f64(qp_sign(bits, 16 * yt + r16), X[vi][ti][s], ya[yt], 0, 0, 0);
                            }
                        }
                    }
                }
            }
            if (!qrole) {
#pragma unroll
                for (int yt = 0; yt < YT; ++yt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) red[vw][4 * yt + r][lane] = ya[yt][r];
            }
        }
    }
    if (qrole) return;
    __syncthreads();
    for (int idx = t; idx < YT * 4 * 64; idx += 64 * NW) {
        const int l = idx & 63, q = idx >> 6, yt = q >> 2, r = q & 3;
        double v = red[0][q][l];
#pragma unroll
        for (int qq = 1; qq < QP_UW; ++qq) v += red[qq][q][l];
        Yw[(long)(16 * yt + (l >> 4) + 4 * r) * n + 16 * cb + (l & 15)] = v;
    }
#ifdef DQ_QP_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    QST(38)
    __syncthreads();
    if (t == 0 && (k == DQ_QP_STAMP_K || k == n / 2) && blockIdx.x == 0 && blockIdx.y == 0) {
        if (cy != nullptr && n - k <= QP_CMAX) printf("step k=%d n=%d: compaction (ranks, LDS pass, barrier, wave 0's read-back) %llu of the load segment\n", k, n, qst[1] - qst[39]);
        printf("step k=%d n=%d (100 MHz ticks): loads %llu | sel steps", k, n, qst[1] - qst[0]);
        for (int j = 0; j < 16; ++j) printf(" %llu", qst[2 + j] - qst[1 + j]);
        printf(" | gather %llu | panel steps", qst[18] - qst[17]);
        for (int j = 0; j < 16; ++j) printf(" %llu", qst[19 + j] - qst[18 + j]);
        printf(" | deposit + ticket %llu | last arriver %llu | W %llu | update + sketch %llu | total %llu\n", qst[35] - qst[34], qst[36] - qst[35],
               qst[37] - qst[36], qst[38] - qst[37], qst[38] - qst[0]);
    }
#endif
}

// the fused step keeps a whole reflector panel in LDS and a wave's tiles in registers: instances up to n = 576 (<3, 3>)
bool qr_panel_fused_fits(int n) { return n <= 576; }
// ... and where it is shorter than the pair it replaces (kernel durations, us: 24.4 against 19.9 + 5.3 at n = 64, 25.4 against 21.3 + 5.3 at 128, 29.6
// against 25.2 + 6.5 at 256, 40.9 against 35.1 + 9.2 at 384 / 512).  Not at n = 576: three waves do the update of 36 row tiles that eight waves
// do in the two-launch form, 50.2 against 39.2 + 10.4 us, and a cfg-5 sweep is 2.5 ms slower with it
bool qr_panel_fused_default(int n) { return n <= 512; }
// two_launch: the workspace also holds the reflector panels and T factors that qp_panel_kernel hands to qp_update_kernel
long qr_panel_work_doubles(int n, bool two_launch) { return two_launch ? qp_off_vtp(n) + (long)n * n : qp_off_vp(n); }
// argument guard of launch_qr_panel: n a multiple of 16 in [16, 1024] and the workspace present
static bool qr_panel_ok(int n, const QrWork& w, bool two_launch) {
    return n >= 16 && n <= 1024 && n % 16 == 0 && w.pw != nullptr && w.pivpos != nullptr && w.pw_stride >= qr_panel_work_doubles(n, two_launch);
}

int launch_qr_panel(Mat A, Mat L, QrWork w, int n, int n_chains, hipStream_t s) {
    const bool fused = !w.pw_two_launch && qr_panel_fused_fits(n);
    if (!qr_panel_ok(n, w, !fused)) { set_error("panel QR: n must be a multiple of 16 in [16, 1024] and the workspace present"); return -1; }
    const int nb = n / 16;
    const int tpw = (nb + QP_UW - 1) / QP_UW;
    // GRID column blocks, of which those from QFIRST on have the Q role
#define QP_UPD(U, K, GRID, QFIRST) do { const dim3 ugrid(GRID, n_chains); \
                          if (tpw <= 2) hipLaunchKernelGGL((qp_update_kernel<U, 2>), ugrid, dim3(64 * QP_UW), 0, s, A, w, n, K, L, QFIRST); \
                          else if (tpw <= 5) hipLaunchKernelGGL((qp_update_kernel<U, 5>), ugrid, dim3(64 * QP_UW), 0, s, A, w, n, K, L, QFIRST); \
                          else hipLaunchKernelGGL((qp_update_kernel<U, 8>), ugrid, dim3(64 * QP_UW), 0, s, A, w, n, K, L, QFIRST); } while (0)
    QP_UPD(false, 0, nb, nb);                                      // pivpos = -1 and the sketch of A (parity 0)
    for (int k = 0; k < n; k += QP_B) {
        const bool trailing = k + QP_B < n;                        // the last panel has no trailing matrix: its factor goes into Q alone
        const int grid = trailing ? 2 * nb : nb, q_first = trailing ? nb : 0;   // trailing update | Q accumulation
        if (fused) {
#define QP_STEP(NW, CPL, TPW) hipLaunchKernelGGL((qp_step_kernel<NW, CPL, TPW>), dim3(grid, n_chains), dim3(64 * NW), 0, s, A, w, n, k, L, q_first)
            if (n <= 64) QP_STEP(1, 1, 1); else if (n <= 128) QP_STEP(2, 1, 1); else if (n <= 256) QP_STEP(4, 1, 2); else if (n <= 512) QP_STEP(4, 2, 4);
            else QP_STEP(3, 3, 5);
#undef QP_STEP
            continue;
        }
#define QP_LAUNCH(NW, CPL) hipLaunchKernelGGL((qp_panel_kernel<NW, CPL>), dim3(1, n_chains), dim3(64 * NW), 0, s, A, w, n, k)
        if (n <= 64) QP_LAUNCH(1, 1); else if (n <= 128) QP_LAUNCH(2, 1); else if (n <= 256) QP_LAUNCH(4, 1); else if (n <= 512) QP_LAUNCH(4, 2);
        else if (n <= 576) QP_LAUNCH(3, 3); else if (n <= 768) QP_LAUNCH(4, 3); else QP_LAUNCH(4, 4);
#undef QP_LAUNCH
        QP_UPD(true, k, grid, q_first);
    }
#undef QP_UPD
    DQ_HIP(hipGetLastError());
    return 0;
}

}  // namespace dq
