// engine.hip -- the sweep engine (class DQMC of the reference, include/dqmc.h:21-93,
// source/dqmc.cpp) and the C ABI of include/dqmc_hip.h.
//
// An engine owns n_chains independent Markov chains on one GPU; every kernel
// launch advances all of them (blockIdx.y = chain).  All state lives in HBM
// across calls: fields (int8, slice-major), the per-slice exp(+-g*eta) vectors,
// the LDR stack, the current equal-time G and the workspaces.  The host only
// enqueues: a half sweep is one asynchronous stream of launches with no host
// round trip; acceptance decisions, pivoting and error checks happen on device.
#include "common.h"
#include "../../include/dqmc_hip.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

namespace dq {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
const char* get_error() { return g_err.c_str(); }

// hipFuncSetAttribute is per device: every device an engine (or the stateless context) lives on gets the attributes once
int init_device_kernels(int device) {
    static std::mutex mu; static bool done[64] = {};
    std::lock_guard<std::mutex> lk(mu);
    if (device < 0 || device >= 64) { set_error("device ordinal out of range"); return -1; }
    if (done[device]) return 0;
    DQ_HIP(hipSetDevice(device));
    DQ_TRY(update_init_device()); DQ_TRY(update_sm_init_device()); DQ_TRY(qr_init_device()); DQ_TRY(qr_colown_init_device());
    done[device] = true;
    return 0;
}

// ---------------------------------------------------------------------------
// Kernel families of to_LDR, the solves and the local update, decided here and nowhere else (the per-size instance inside a family
// is chosen next to its kernel) from n, the chain count, the CU reservation and the switches (README.md, "Environment switches").
// ---------------------------------------------------------------------------
struct Switches { bool qr_panel; int qr_panel_fused, gj_fused; bool qr_streaming, walk_submatrix, lu_classic, slice_multikernel, bbar_rider, slice_stream, panel_compact; };
static const Switches& switches() {           // read once per process
    static const Switches sw = [] {
        const char* panel = getenv("DQMC_QR_PANEL");
        const char* fused = getenv("DQMC_QR_PANEL_FUSED");          // unset (-1): where it measured faster; 0: nowhere; 1: wherever an instance exists
        const char* gj = getenv("DQMC_GJ_FUSED");                   // the same three states for the Gauss-Jordan solve (lu_gj.hip)
        const char* rider = getenv("DQMC_BBAR_RIDER");              // 0: the B-bar chain rides on the wraps again (wrap_*_piggy) instead of on the slice launches
        const char* stream = getenv("DQMC_SLICE_STREAM");           // 0: the persistent walk stores its pairs when a window closes (the dump) instead of one by one as they are accepted
        const char* compact = getenv("DQMC_PANEL_COMPACT");         // 0: the late panels of to_LDR and of the Gauss-Jordan solve (n <= 256) keep every column / row on its original lane, four waves to the last panel
        return Switches{!(panel && atoi(panel) == 0), fused ? (atoi(fused) != 0 ? 1 : 0) : -1, gj ? (atoi(gj) != 0 ? 1 : 0) : -1, getenv("DQMC_QR_STREAMING") != nullptr, getenv("DQMC_WALK_SUBMATRIX") != nullptr,
                        getenv("DQMC_LU_CLASSIC") != nullptr, getenv("DQMC_SLICE_MULTIKERNEL") != nullptr, !(rider && atoi(rider) == 0), !(stream && atoi(stream) == 0), !(compact && atoi(compact) == 0)};
    }();
    return sw;
}

// n = 704 ... 1024: 8.4 / 11.7 / 12.0 ms per inv(I + F1 F2) call with Gauss-Jordan against 9.9 / 14.0 / 14.1 with the blocked LU.
// Latency regime only: with many chains per launch the blocked LU + per-column substitution has the higher throughput
// (128 chains, cfg 3: 458 ms per step against 483 ms with the single-wave panels)
constexpr int GJ_MAX_N = 1024, GJ_MAX_CHAINS = 8;
constexpr int TRI_MAX_N = 640;      // any number of chains (128 chains at cfg 3: 432.9 against 437.3 ms per step)

// allow_panel = false: the caller has no panel workspace (the batched initialisation)
static QrFamily pick_qr(int n, int chains, bool allow_panel) {
    const Switches& sw = switches();
    if (sw.qr_streaming) return QrFamily::Streaming;
    // one global pivot decision per 16 columns instead of one per column; DQMC_QR_PANEL=0 keeps the column-pivoted kernels at every size
    // (the only way to reach qr_colown / qr_coop at n = 64 .. 1024 with few chains)
    if (allow_panel && sw.qr_panel && n >= 64 && n <= 1024 && n % 16 == 0 && chains <= 8) return QrFamily::Panel;
    if (n <= 256) return QrFamily::ColumnOwner;
    // the matrix does not fit one CU: ceil(n/32) cooperating workgroups while they fit the CU budget (co-residency), the
    // single-workgroup streaming kernel otherwise (many chains per launch: every CU is busy with its own chain anyway)
    return qrcp_coop_workgroups(n, chains) <= 200 ? QrFamily::Cooperative : QrFamily::Streaming;
}

struct KernelPlan {
    QrFamily qr;
    enum class Solve { GaussJordan, BlockedLu } solve;             // M^-1 RHS: lu_gj.hip / lu_blocked.hip + lu.hip
    enum class Rinv { Blocked, PerColumn } rinv;                    // R^-1 D of one to_LDR factor: tri_solve.hip / lu.hip
    static KernelPlan pick(int n, int chains) {
        return KernelPlan{pick_qr(n, chains, true),
                          n <= GJ_MAX_N && chains <= GJ_MAX_CHAINS && !switches().lu_classic ? Solve::GaussJordan : Solve::BlockedLu,
                          n <= TRI_MAX_N ? Rinv::Blocked : Rinv::PerColumn};
    }
};

// the local-update path of an engine (launch_update_slice, update.hip); reserved: the engine holds a CU reservation (slice_reserve)
static SlicePath pick_slice_path(int n, int chains, bool reserved) {
    const Switches& sw = switches();
    const bool walk = n <= 256;                                     // the register-resident delayed-update walk fits
    if (sw.slice_multikernel) return SlicePath::Pairs;
    // sub-matrix updates at n <= 256 are opt-in: 211 us per cfg-3 slice against 138 us for the delayed-update walk -- the k x k algebra
    // is a dependent chain on one wave per SIMD (860 clk per two-proposal pass, 1780 clk per accepted flip), see DESIGN.md
    if (reserved) return walk && !sw.walk_submatrix ? (sw.slice_stream ? SlicePath::PersistentWalk : SlicePath::PersistentWalkDump) : SlicePath::PersistentSubmatrix;
    if (!walk) return SlicePath::Pairs;
    // measured (cfg 3, sweeps/s, solo vs pairs): 64 chains 166 / 214, 128 chains 251 / 275, 256 chains 324 / 307 -- a chain's own CU
    // flushes slower than the whole chip does, so the solo kernel pays once there are enough chains to occupy every CU
    return chains >= 224 ? SlicePath::Solo : SlicePath::PairsTailSolo;
}
static bool is_persistent_walk(SlicePath p) { return p == SlicePath::PersistentWalk || p == SlicePath::PersistentWalkDump; }
static bool is_persistent(SlicePath p) { return is_persistent_walk(p) || p == SlicePath::PersistentSubmatrix; }

// ---------------------------------------------------------------------------
// Workspace + stable linear algebra on device (stablelinalg.cpp restated as
// launch sequences).  Shared by the engine and the stateless ABI calls.
// ---------------------------------------------------------------------------
struct LdrRef {                 // a batched LDR triple in HBM
    Mat L; Vec d; Mat R;
    int* jpvt = nullptr;        // [C][n] pivot order storage of this triple (may be null)
    bool* tri = nullptr;        // host flag: R is the permuted-triangular factor of ONE to_LDR (jpvt valid)
    Mat X{nullptr, 0};          // cache slot for R^-1 diag(1 / max(d, 1)) of this triple (may be null: no slot)
    bool* xok = nullptr;        // host flag: X holds that matrix for the current d and R
    void touch() const { if (xok) *xok = false; }                // d or R is about to be rewritten
};
// k batched LDR triples: L, R [k][C][nn], d and the pivot order of R [k][C][n], and the host flag `tri` of each triple.
// with_x: every triple also gets a cache slot X [k][C][nn] for R^-1 diag(1 / max(d, 1)) and its host flag `xok` (Ctx::r_inverse_scaled
// fills and reuses it); the slots are half as large again as L and R together, so only the engine's stack asks for them.
struct LdrStore {
    int n = 0, C = 0;
    DevPtr<double> L, d, R, X;
    DevPtr<int> jpvt;
    std::unique_ptr<bool[]> tri, xok;          // arrays on the heap: LdrRef::tri / xok stay valid when the store is moved
    int alloc(int k, int n_, int C_, bool with_x = false) {
        n = n_; C = C_;
        const size_t nn = (size_t)n * n;
        DQ_TRY(dev_alloc(L, (size_t)k * C * nn)); DQ_TRY(dev_alloc(d, (size_t)k * C * n));
        DQ_TRY(dev_alloc(R, (size_t)k * C * nn)); DQ_TRY(dev_alloc(jpvt, (size_t)k * C * n));
        if (with_x) DQ_TRY(dev_alloc(X, (size_t)k * C * nn));
        tri.reset(new bool[k]()); xok.reset(new bool[k]());
        return 0;
    }
    LdrRef at(int i) const {
        const long nn = (long)n * n;
        LdrRef f{Mat{L.get() + (long)i * C * nn, nn}, Vec{d.get() + (long)i * C * n, (long)n}, Mat{R.get() + (long)i * C * nn, nn},
                 jpvt.get() + (long)i * C * n, &tri[i]};
        if (X) { f.X = Mat{X.get() + (long)i * C * nn, nn}; f.xok = &xok[i]; }
        return f;
    }
};

struct Ctx {
    int n = 0, C = 0, device = 0;
    long nn = 0;
    hipStream_t stream = nullptr;
    static constexpr int NT = 6, NV = 5;       // matrices T0 .. T4 and the Gauss-Jordan scratch T5; vectors V0 .. V3 and the QR tau V4
    DevPtr<double> pool;                       // NT * C * nn
    DevPtr<double> vpool;                      // NV * C * n
    DevPtr<int> ipool;                         // 4 * C * n ints + info
    DevPtr<unsigned long long> qsync;          // cooperative QRCP records
    DevPtr<int> qabort;                        // cooperative QRCP abort words: C
    DevPtr<double> tinv;                       // Gauss-Jordan panel inverses: 2048 * C
    DevPtr<double> qpw;                        // panel-pivoted QR (qr_panel.hip): qr_panel_work_doubles(n, qpw_two_launch) * C, zeroed (the ticket counters)
    bool gj_fused = false;                     // the Gauss-Jordan solve takes one launch per panel (gj_step_kernel): where it measured faster, or DQMC_GJ_FUSED
    bool qpw_two_launch = false;               // ... in the two-launch form (panel kernel + update kernel): sizes the fused step is not used at, or DQMC_QR_PANEL_FUSED=0
    DevPtr<int> qpivpos;                       // ... and its pivot positions: n * C
    DevPtr<double> trinv;                      // blocked triangular solve: inverses of the 16 x 16 diagonal blocks, 16 * (n + 16) * C
    KernelPlan plan{};                         // the kernel families of this (n, C); each family's workspace above exists only when chosen

    Mat T(int k) const { return Mat{pool.get() + (long)k * C * nn, nn}; }
    Vec V(int k) const { return Vec{vpool.get() + (long)k * C * n, (long)n}; }
    int* jpvt() const { return ipool.get(); }
    int* lperm() const { return ipool.get() + (long)C * n; }
    int* rowpos() const { return ipool.get() + 2L * C * n; }
    int* rowpos_alt() const { return ipool.get() + 3L * C * n; }       // the fused Gauss-Jordan step alternates between the two
    int* info() const { return ipool.get() + 4L * C * n; }

    int init(int n_, int C_, int device_) {
        n = n_; C = C_; device = device_; nn = (long)n * n;
        DQ_HIP(hipSetDevice(device));
        DQ_TRY(init_device_kernels(device));
        DQ_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        DQ_TRY(dev_alloc(pool, (size_t)NT * C * nn));
        DQ_TRY(dev_alloc(vpool, (size_t)NV * C * n));
        DQ_TRY(dev_alloc(ipool, 4L * C * n + 4));
        plan = KernelPlan::pick(n, C);
        if (plan.qr == QrFamily::Cooperative) { DQ_TRY(dev_alloc(qsync, (size_t)qrcp_coop_sync_granules(n) * C)); DQ_TRY(dev_alloc(qabort, C)); }
        if (plan.qr == QrFamily::Panel) {
            const int fused = switches().qr_panel_fused;
            qpw_two_launch = !(fused < 0 ? qr_panel_fused_default(n) : fused == 1 && qr_panel_fused_fits(n));
            const size_t qpw_count = (size_t)qr_panel_work_doubles(n, qpw_two_launch) * C;
            DQ_TRY(dev_alloc(qpw, qpw_count)); DQ_TRY(dev_alloc(qpivpos, (size_t)n * C));
            DQ_HIP(hipMemsetAsync(qpw.get(), 0, sizeof(double) * qpw_count, stream));
        }
        if (plan.solve == KernelPlan::Solve::GaussJordan) {
            DQ_TRY(dev_alloc(tinv, (size_t)2048 * C));
            const int fused = switches().gj_fused;
            gj_fused = fused < 0 ? gj_fused_default(n) : fused == 1 && gj_fused_fits(n);
        }
        if (plan.rinv == KernelPlan::Rinv::Blocked) DQ_TRY(dev_alloc(trinv, (size_t)16 * (n + 16) * C));
        DQ_HIP(hipMemsetAsync(ipool.get(), 0, sizeof(int) * (4L * C * n + 4), stream));
        return 0;
    }
    ~Ctx() { if (stream) (void)hipStreamDestroy(stream); }

    int gemm(CMat A, CMat B, Mat Cm, CVec rs = CVec(), CVec ks = CVec(), CVec cs = CVec(), int transA = 0, int accumulate = 0, Mat CT = Mat{nullptr, 0}) {
        GemmDesc g; g.A = A; g.B = B; g.C = Cm; g.CT = CT; g.rs = rs; g.ks = ks; g.cs = cs; g.n = n; g.transA = transA; g.accumulate = accumulate;
        return launch_gemm(g, C, stream);
    }
    // stablelinalg::to_LDR (source/stablelinalg.cpp:35-55); A is destroyed
    // `direct`: out.R receives the QR's own R factor (not a product), so out can take the
    // triangular fast path later; its pivot order is written straight into out.jpvt.
    int to_ldr(Mat A, LdrRef out, bool direct = true) {
        const bool keep = direct && out.jpvt != nullptr;
        QrWork w{V(4).p, (long)n, keep ? out.jpvt : jpvt(), (long)n};
        w.sync = qsync.get(); w.sync_stride = qrcp_coop_sync_granules(n); w.abort_words = qabort.get(); w.info = info();
        w.pw = qpw.get(); w.pw_stride = qr_panel_work_doubles(n, qpw_two_launch); w.pw_two_launch = qpw_two_launch; w.pivpos = qpivpos.get(); w.pivpos_stride = n;
        w.pw_compact = switches().panel_compact;
        if (out.tri) *out.tri = keep;
        out.touch();
        return launch_to_ldr(plan.qr, A, out.L, out.d, out.R, w, n, C, stream);
    }
    // X = F.R^-1 diag(dinv), dinv = 1 / max(F.d, 1): permuted triangular solve when F.R is a single QR factor, LU otherwise.
    // *Xout is the matrix that holds X: the triple's own slot when it has one (computed once per (d, R): a valid slot costs no
    // launch), `scratch` otherwise.  X is only read afterwards.
    int r_inverse_scaled(LdrRef F, CVec dinv, Mat scratch, Mat lu_scratch, Mat* Xout) {
        const Mat X = F.X.p ? F.X : scratch;
        *Xout = X;
        if (F.xok && *F.xok) return 0;
        if (F.tri && *F.tri && F.jpvt) {
            if (plan.rinv == KernelPlan::Rinv::Blocked) DQ_TRY(launch_tri_solve(F.R, F.jpvt, n, X, dinv, trinv.get(), 16L * (n + 16), n, C, stream));
            else DQ_TRY(launch_lu_solve(F.R, F.jpvt, n, X, dinv, 2, n, C, stream));
        } else {
            DQ_TRY(launch_copy(F.R, lu_scratch, nn, C, stream));
            DQ_TRY(launch_lu_blocked(lu_scratch, lperm(), n, rowpos(), n, nullptr, 0, info(), n, C, stream));
            DQ_TRY(launch_lu_solve(lu_scratch, lperm(), n, X, dinv, 1, n, C, stream));
        }
        if (F.xok) *F.xok = true;
        return 0;
    }
    // stablelinalg::mat_mul_ldr (source/stablelinalg.cpp:69-79): out = M * F   (uses T0,T1)
    int mat_mul_ldr(CMat M, LdrRef F, LdrRef out) {
        DQ_TRY(gemm(M, F.L, T(0), CVec(), CVec(), CVec(F.d)));           // (M L) diag(d)
        LdrRef q{out.L, out.d, T(1)};
        DQ_TRY(to_ldr(T(0), q));
        if (out.tri) *out.tri = false;                                   // R becomes a product
        out.touch();
        return gemm(T(1), F.R, out.R);                                   // r * R
    }
    // stablelinalg::ldr_mul_mat (source/stablelinalg.cpp:57-67): out = F * M   (uses T0,T1)
    int ldr_mul_mat(LdrRef F, CMat M, LdrRef out) {
        DQ_TRY(gemm(F.R, M, T(0), CVec(F.d)));                            // diag(d) (R M)
        LdrRef q{T(1), out.d, out.R, out.jpvt, out.tri};                  // R = the QR's own factor
        q.xok = out.xok;                                                 // to_ldr marks out's cached X stale
        DQ_TRY(to_ldr(T(0), q));
        return gemm(F.L, T(1), out.L);                                   // L * q
    }
    // stablelinalg::ldr_mul_ldr (source/stablelinalg.cpp:81-92): out = F1 * F2   (uses T0,T1,T2)
    int ldr_mul_ldr(LdrRef F1, LdrRef F2, LdrRef out) {
        DQ_TRY(gemm(F1.R, F2.L, T(0), CVec(F1.d), CVec(), CVec(F2.d)));    // diag(d1) (R1 L2) diag(d2)
        LdrRef q{T(1), out.d, T(2)};
        DQ_TRY(to_ldr(T(0), q));
        if (out.tri) *out.tri = false;
        out.touch();
        DQ_TRY(gemm(F1.L, T(1), out.L));
        return gemm(T(2), F2.R, out.R);
    }
    // Y = M^-1 RHS (arma::solve): blocked Gauss-Jordan (result in `out`) or dgetrf + dgetrs (result overwrites RHS), as the plan says.
    // Returns the matrix holding Y in *Y.  M and RHS are destroyed.  (uses T5 as scratch)
    int solve(Mat M, Mat RHS, Mat out, double* logdet_acc, Mat* Y) {
        if (plan.solve == KernelPlan::Solve::GaussJordan) {
            DQ_TRY(launch_gj_solve(M, RHS, out, T(5), tinv.get(), lperm(), n, rowpos(), rowpos_alt(), n, logdet_acc, 1, info(), n, C, gj_fused, switches().panel_compact, stream));
            *Y = out; return 0;
        }
        DQ_TRY(launch_lu_blocked(M, lperm(), n, rowpos(), n, logdet_acc, 1, info(), n, C, stream));
        DQ_TRY(launch_lu_solve(M, lperm(), n, RHS, CVec(), 0, n, C, stream));
        *Y = RHS; return 0;
    }
    // stablelinalg::inv_I_plus_ldr (source/stablelinalg.cpp:94-126)   (uses T0..T4, V0,V1)
    // G = X M^-1 is evaluated as the reference does, through the transposed system M^T G^T = X^T;
    // log|det M| comes from that same factorisation (det M^T = det M).
    int inv_I_plus_ldr(LdrRef F, Mat G, double* logdet /*device, C*/) {
        DQ_TRY(launch_split_d(F.d, V(0), V(1), logdet, n, C, stream));                 // V0 = 1/Dl, V1 = Ds, logdet = sum log Dl
        Mat X; DQ_TRY(r_inverse_scaled(F, V(0), T(1), T(0), &X));                       // X = R^-1 diag(1/Dl)
        DQ_TRY(launch_add_scaled_cols(X, F.L, V(1), T(2), n, C, stream));               // M = X + L diag(Ds)
        DQ_TRY(launch_transpose_scale(T(2), T(3), CVec(), n, C, stream));               // M^T
        DQ_TRY(launch_transpose_scale(X, T(4), CVec(), n, C, stream));                  // X^T
        Mat Y; DQ_TRY(solve(T(3), T(4), T(0), logdet, &Y));                             // G^T; logdet += log|det M|
        return launch_transpose_scale(Y, G, CVec(), n, C, stream);
    }
    // stablelinalg::inv_I_plus_ldr_mul_ldr (source/stablelinalg.cpp:128-158)   (uses T0..T3, V0..V3)
    // GT (optional) receives G^T as well, from the product that writes G
    int inv_I_plus_ldr_mul_ldr(LdrRef F1, LdrRef F2, Mat G, Mat GT = Mat{nullptr, 0}) {
        DQ_TRY(launch_split_d2(F1.d, V(0), V(1), F2.d, V(2), V(3), n, C, stream));     // 1/D1l, D1s | 1/D2l, D2s
        Mat X; DQ_TRY(r_inverse_scaled(F2, V(2), T(1), T(0), &X));                      // X = R2^-1 diag(1/D2l)
        DQ_TRY(gemm(F1.L, X, T(2), V(0), CVec(), CVec(), 1));                           // TermA = diag(1/D1l) L1^T X
        DQ_TRY(gemm(F1.R, F2.L, T(2), V(1), CVec(), V(3), 0, 1));                       // M = TermA + diag(D1s) R1 L2 diag(D2s)
        DQ_TRY(launch_transpose_scale(F1.L, T(3), V(0), n, C, stream));                 // RHS = diag(1/D1l) L1^T
        Mat Y; DQ_TRY(solve(T(2), T(3), T(0), nullptr, &Y));                            // Y = M^-1 RHS
        return gemm(X, Y, G, CVec(), CVec(), CVec(), 0, 0, GT);                         // G = X Y
    }
    // stablelinalg::inv_invldr_plus_ldr (source/stablelinalg.cpp:160-190): G = [F1^-1 + F2]^-1 (negated on request)   (uses T0..T3, V0..V3)
    int inv_invldr_plus_ldr(LdrRef F1, LdrRef F2, Mat G, bool negate) {
        DQ_TRY(launch_split_d(F1.d, V(0), V(1), nullptr, n, C, stream));               // 1/D1l, D1s
        DQ_TRY(launch_split_d(F2.d, V(2), V(3), nullptr, n, C, stream));               // 1/D2l, D2s
        Mat X; DQ_TRY(r_inverse_scaled(F2, V(2), T(1), T(0), &X));                      // X = R2^-1 diag(1/D2l)
        DQ_TRY(gemm(F1.L, X, T(2), V(0), CVec(), CVec(), 1));                           // TermA = diag(1/D1l) L1^T X
        DQ_TRY(gemm(F1.R, F2.L, T(2), V(1), CVec(), V(3), 0, 1));                       // M = TermA + diag(D1s) R1 L2 diag(D2s)
        DQ_TRY(launch_scale_rows(F1.R, V(1), T(3), n, C, stream));                      // RHS = diag(D1s) R1
        Mat Y; DQ_TRY(solve(T(2), T(3), T(0), nullptr, &Y));                            // Y = M^-1 RHS
        DQ_TRY(gemm(X, Y, G));                                                          // G = X Y
        if (negate) DQ_TRY(launch_axpb_identity(G, G, -1.0, 0.0, n, C, stream));
        return 0;
    }
};

// ---------------------------------------------------------------------------
// Engine
// ---------------------------------------------------------------------------
// After a stream sync: read the status block (common.h), clear it, and report the first of its conditions in the order
// HANDOFF, CENSUS, COOP_QR, PIVOT as DQMC_ENUMERIC.  *bits (optional) receives word 0.
static int take_status(const Ctx& c, int* bits = nullptr) {
    int w[4] = {0, 0, 0, 0};
    DQ_HIP(hipMemcpy(w, c.info(), sizeof w, hipMemcpyDeviceToHost));
    if (bits) *bits = w[0];
    if (w[0] == 0) return 0;
    (void)hipMemset(c.info(), 0, sizeof w);
    if (w[0] & DQ_STATUS_HANDOFF) {
        set_error("persistent slice kernel: a workgroup that had checked in stopped answering (device fault or pre-emption beyond the spin bound); the chain state is undefined -- set the fields again and call dqmc_init; this engine uses the scan / flush kernel pairs from now on");
    } else if (w[0] & DQ_STATUS_CENSUS) {
        // n > 256: the census of slice_sm_kernel failed at slice w[1] - 1.  That launch and (device-side latch, update_sm.hip) every later
        // slice_sm_kernel launch enqueued behind it left their slices untouched; the wraps and stabilisations of the calls in flight ran.
        char msg[640];
        snprintf(msg, sizeof msg, "persistent sub-matrix slice kernel: its workgroups did not all become resident at time slice %d (device shared with other "
                 "work?).  That slice and every later slice of the call(s) in flight proposed NOTHING (fields unchanged there, acceptance counts 0, their part of "
                 "the random stream is spent); wraps and stabilisations ran, so fields, G and the stack are consistent with each other, but the sweep is not the "
                 "one the stream describes from that slice on.  This engine uses the scan / flush kernel pairs from now on: restore the fields of the last "
                 "completed sweep and call dqmc_init, or keep the state as a valid (shortened) sweep", w[1] - 1);
        set_error(msg);
    } else if (w[0] & DQ_STATUS_COOP_QR) {
        set_error("cooperative QRCP gave up waiting for a partner workgroup (not co-resident?)");
    } else {
        set_error("LU factorisation hit a zero or NaN pivot");
    }
    return DQMC_ENUMERIC;
}

struct Engine {
    int n = 0, nt = 0, n_stab = 0, n_stack = 0, C = 1, device = 0;
    long nn = 0;
    std::vector<int> loc_l_end;
    std::vector<double> g_host, gamma_host, eta_host;
    std::vector<unsigned char> seen;                             // scratch of check_stream
    Ctx ctx;                                                     // owns the stream; declared before every buffer below, so it outlives them
    hipStream_t s = nullptr;

    DevPtr<double> expK, invexpK;                                // [C][nn]
    // checkerboard break-up of exp(-+dtau K) (dqmc_set_checkerboard): wraps and B-bar products apply the pair factors directly
    bool cb = false; int cb_groups = 0;
    DevPtr<int> cb_partner;                                      // [cb_groups][n]
    DevPtr<double> cb_par;                                       // [C][4] cosh, sinh, f, 1/f
    DevPtr<int8_t> fields;                                       // [C][nt][n]
    DevPtr<double> expv, invexpv;                                // [C][nt][n]
    DevPtr<UpdateTables> tabs; DevPtr<double> tab8;              // [C], [C][8]
    bool gt_valid = false;                                       // GT == G^T right now (set by the wraps and the backward stabilisations, cleared by everything else that writes G)
    bool gt_check = false; long long gt_checks = 0; DevPtr<double> gt_err;   // dqmc_debug_gt_check: max|GT - G^T| [C] over the stabilisations that left GT valid
    DevPtr<double> G, Gtmp, GT;                                  // [C][nn]; GT: transposed copy for the local-update walk
    DevPtr<double> pg_eye, pg_ones;                              // identity [nn] and ones [n]: operands of the first piggybacked B-bar factor of a block (single chain)
    DevPtr<double> bb0, bb1;                                     // Bbar ping-pong
    long long rider_launches = 0;                                // slice launches that carried a B-bar product so far (dqmc_bbar_rider_launches)
    LdrStore stack;                                              // n_stack triples
    LdrStore spare;                                              // one spare triple (init)
    DevPtr<double> logdet;                                       // [C]
    DevPtr<int32_t> rs_perm; DevPtr<uint8_t> rs_k; DevPtr<double> rs_u;   // [C][nt][n]
    PinnedPtr h_stage;                                           // pinned staging for the random stream
    // dqmc_rng_seed: the stream is drawn on the device (rng.hip) from (rng_seed, rng_first_chain + chain, rng_counter); the counter is the
    // half sweep the next sweep call without arrays draws
    bool rng_seeded = false; uint64_t rng_seed = 0; uint32_t rng_first_chain = 0, rng_counter = 0;
    hipEvent_t stage_free = nullptr;
    DevPtr<double> Upanel, Wpanel;                               // [C][panel_rows][n]
    int panel_rows = UPDATE_KD;                                  // KD, or SLICE_RING_ROWS for the streaming persistent walk (create)
    DevPtr<double> Cpanel;                                       // [C][KD][KD]
    // The groups below are allocated on first use into a local group, which replaces the engine's only once all of it is allocated.
    // batched initialisation (init_batched): Bbar ping-pong [2][S][nn], tau [S][n] and the to_LDR of every block (S triples)
    struct InitBatch { DevPtr<double> bb, tau; LdrStore f; } ib;
    DevPtr<int> state;                                           // [C][4]
    DevPtr<double> prep;                                         // [C][4n]
    DevPtr<double> meas_now, meas_sum;                           // [C][3 + n] equal-time observables: last evaluation / bin sums
    // unequal-time path (sweep_unequal): Gtt / Gt0 / G0t [nt + 1][C][nn], the three before a stabilisation [3][C][nn], their errors
    // [C][3 n_stack], dynamical observables [C][3][nt + 1][n] (last / bin sums), B(tau, 0) ping-pong (2 triples)
    struct UnequalTime { DevPtr<double> G[3], tmp, err, meas_now, meas_sum; LdrStore bt; } ut;
    bool ut_valid = false; long long ut_meas_count = 0;
    struct HalfWarp { DevPtr<double> expK, invexpK, out; } hw;   // dqmc_half_warp: exp(-+ dtau K / 2) [nn] each, its result [C][nn]
    long long meas_count = 0;                                    // measurements accumulated in meas_sum
    DevPtr<char> slice_sync;                                     // [C][SLICE_SYNC_BYTES = 2 KiB] hand-off words of the persistent slice kernels (SliceSync, common.h)
    bool reserved = false;                                       // holds a CU reservation for the single-launch slice kernels (slice_reserve)
    SlicePath slice_path = SlicePath::Pairs;                     // the local-update path; lowered to the unreserved choice once a persistent kernel fails (sync_and_check)
    unsigned slice_epoch = 0;                                    // launches of the persistent slice kernel so far: the tag of its hand-off words (SliceSync, common.h)
    int slice_absent_l = -1;                                     // ...=<tile>:<slice>: only in the launch of that time slice
    int slice_late_tile = -1, slice_late_us = 0;                 // DQMC_DEBUG_SLICE_LATE=<tile>:<us>: that flush workgroup checks in only after <us> microseconds (test of a LATE arrival)
    int slice_absent_tile = -1;                                  // DQMC_DEBUG_SLICE_ABSENT=<tile>, read when the engine is created: that flush workgroup never checks in (test of the solo fall-back)
    DevPtr<int> acc;                                             // [C][nt]
    struct Exchange { DevPtr<int8_t> saved, recv; DevPtr<int> tab; } xch;   // replica exchange (replica.hip): own fields [C][nt][n], two received configurations, [2][C] ints
    DevPtr<double> err;                                          // [C][n_stack]
    DevPtr<DevStats> dstats;                                     // [C]
    bool stack_valid = false;
    // profiling of the local-update kernels
    bool profiling = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pairs;
    size_t ev_used = 0;
    double upd_ms = 0.0; long long upd_launches = 0; long long upd_accept_base = 0;

    Mat mG() const { return Mat{G.get(), nn}; }
    CVec ev(int l) const { return CVec(expv.get() + (long)l * n, (long)nt * n); }
    CVec iev(int l) const { return CVec(invexpv.get() + (long)l * n, (long)nt * n); }
    int stack_idx(int l) const { return l / n_stab; }            // include/dqmc.h:47
    int local_l(int l) const { return l % n_stab; }              // include/dqmc.h:48

    ~Engine() {                                                  // the buffers are freed after the sync, the stream (ctx) after them
        if (s) (void)hipStreamSynchronize(s);
        if (reserved) slice_release(device, n, C);
        for (auto& p : ev_pairs) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
        if (stage_free) (void)hipEventDestroy(stage_free);
    }

    int create(int device_, int C_, int n_, int nt_, int n_stab_, const double* g, const double* gamma, const double* eta,
               const double* eK, const double* ieK) {
        device = device_; C = C_; n = n_; nt = nt_; n_stab = n_stab_; nn = (long)n * n;
        n_stack = (int)std::ceil(static_cast<double>(nt) / n_stab);                       // source/dqmc.cpp:10
        loc_l_end.assign(n_stack, n_stab - 1);
        if (nt % n_stab != 0) loc_l_end[n_stack - 1] = nt % n_stab - 1;                    // source/dqmc.cpp:13-18
        g_host.assign(g, g + C); gamma_host.assign(gamma, gamma + 4); eta_host.assign(eta, eta + 4);
        DQ_TRY(ctx.init(n, C, device)); s = ctx.stream;
        reserved = slice_reserve(device, n, C);
        slice_path = pick_slice_path(n, C, reserved);
        if (const char* a = getenv("DQMC_DEBUG_SLICE_ABSENT")) { slice_absent_tile = atoi(a); if (const char* c = strchr(a, ':')) slice_absent_l = atoi(c + 1); }
        if (const char* a = getenv("DQMC_DEBUG_SLICE_LATE")) { slice_late_tile = atoi(a); if (const char* c = strchr(a, ':')) slice_late_us = atoi(c + 1); }
        DQ_TRY(dev_alloc(expK, C * nn)); DQ_TRY(dev_alloc(invexpK, C * nn));
        DQ_TRY(dev_alloc(fields, (size_t)C * nt * n)); DQ_TRY(dev_alloc(expv, (size_t)C * nt * n)); DQ_TRY(dev_alloc(invexpv, (size_t)C * nt * n));
        DQ_TRY(dev_alloc(tabs, C)); DQ_TRY(dev_alloc(tab8, (size_t)C * 8));
        if (C == 1) { DQ_TRY(dev_alloc(pg_eye, nn)); DQ_TRY(dev_alloc(pg_ones, (size_t)n)); DQ_TRY(launch_set_identity(Mat{pg_eye.get(), nn}, n, 1, s)); const std::vector<double> one_h((size_t)n, 1.0); DQ_HIP(hipMemcpy(pg_ones.get(), one_h.data(), sizeof(double) * n, hipMemcpyHostToDevice)); }
        DQ_TRY(dev_alloc(G, C * nn)); DQ_TRY(dev_alloc(Gtmp, C * nn)); DQ_TRY(dev_alloc(GT, C * nn)); DQ_TRY(dev_alloc(bb0, C * nn)); DQ_TRY(dev_alloc(bb1, C * nn));
        // X slots for the stack of the few-chain engines (the latency-bound ones, same limit as the panel QR family): n_stack C nn doubles
        DQ_TRY(stack.alloc(n_stack, n, C, C <= 8)); DQ_TRY(spare.alloc(1, n, C));
        DQ_TRY(dev_alloc(logdet, C));
        DQ_TRY(dev_alloc(rs_perm, (size_t)C * nt * n)); DQ_TRY(dev_alloc(rs_k, (size_t)C * nt * n)); DQ_TRY(dev_alloc(rs_u, (size_t)C * nt * n));
        panel_rows = slice_path == SlicePath::PersistentWalk ? SLICE_RING_ROWS : UPDATE_KD;     // the streaming walk's rings; every other path (and the one a failed persistent kernel is lowered to) uses the first KD rows
        DQ_TRY(dev_alloc(Upanel, (size_t)C * panel_rows * n)); DQ_TRY(dev_alloc(Wpanel, (size_t)C * panel_rows * n)); DQ_TRY(dev_alloc(Cpanel, (size_t)C * UPDATE_KD * UPDATE_KD));
        DQ_TRY(dev_alloc(state, (size_t)C * 4)); DQ_TRY(dev_alloc(prep, (size_t)C * 4 * n)); DQ_TRY(dev_alloc(meas_now, (size_t)C * (3 + n))); DQ_TRY(dev_alloc(meas_sum, (size_t)C * (3 + n))); DQ_HIP(hipMemsetAsync(meas_sum.get(), 0, sizeof(double) * C * (3 + n), s)); DQ_TRY(dev_alloc(slice_sync, (size_t)C * SLICE_SYNC_BYTES)); DQ_HIP(hipMemsetAsync(slice_sync.get(), 0, (size_t)C * SLICE_SYNC_BYTES, s)); DQ_TRY(dev_alloc(acc, (size_t)C * nt)); DQ_TRY(dev_alloc(err, (size_t)C * n_stack));
        DQ_TRY(dev_alloc(dstats, C));
        void* stage = nullptr;
        DQ_HIP(hipHostMalloc(&stage, (size_t)C * nt * n * (sizeof(int32_t) + sizeof(uint8_t) + sizeof(double)), hipHostMallocDefault)); h_stage.reset(static_cast<char*>(stage));
        DQ_HIP(hipEventCreateWithFlags(&stage_free, hipEventDisableTiming));
        DQ_HIP(hipEventRecord(stage_free, s));
        DQ_HIP(hipMemcpyAsync(expK.get(), eK, sizeof(double) * C * nn, hipMemcpyHostToDevice, s));
        DQ_HIP(hipMemcpyAsync(invexpK.get(), ieK, sizeof(double) * C * nn, hipMemcpyHostToDevice, s));
        DQ_HIP(hipMemsetAsync(fields.get(), 0, (size_t)C * nt * n, s));
        DQ_HIP(hipMemsetAsync(G.get(), 0, sizeof(double) * C * nn, s));
        DQ_HIP(hipMemsetAsync(dstats.get(), 0, sizeof(DevStats) * C, s));
        DQ_HIP(hipMemsetAsync(logdet.get(), 0, sizeof(double) * C, s));
        DQ_HIP(hipMemsetAsync(state.get(), 0, sizeof(int) * C * 4, s));
        // model tables, same expressions as source/model.cpp:99-122, :62-84
        std::vector<UpdateTables> ht(C); std::vector<double> h8((size_t)C * 8);
        static const int proposal[4][3] = {{1, 2, 3}, {0, 2, 3}, {0, 1, 3}, {0, 1, 2}};
        const double alpha = -1.0;
        for (int c = 0; c < C; ++c) {
            std::memset(&ht[c], 0, sizeof(UpdateTables));
            for (int o = 0; o < 4; ++o) for (int k = 0; k < 3; ++k) {
                const int nf = proposal[o][k];
                const double gammaR = gamma[nf] / gamma[o];
                const double d_eta = eta[nf] - eta[o];
                const double bosonR = std::exp(alpha * g[c] * d_eta);
                ht[c].rb[o][k] = gammaR * bosonR;
                ht[c].delta[o][k] = (1.0 / bosonR) - 1.0;
            }
            for (int f = 0; f < 4; ++f) { ht[c].ev[f] = std::exp(g[c] * eta[f]); ht[c].iev[f] = std::exp(-g[c] * eta[f]); h8[(size_t)c * 8 + f] = ht[c].ev[f]; h8[(size_t)c * 8 + 4 + f] = ht[c].iev[f]; }
        }
        DQ_HIP(hipMemcpyAsync(tabs.get(), ht.data(), sizeof(UpdateTables) * C, hipMemcpyHostToDevice, s));
        DQ_HIP(hipMemcpyAsync(tab8.get(), h8.data(), sizeof(double) * C * 8, hipMemcpyHostToDevice, s));
        DQ_TRY(launch_build_expv(fields.get(), (long)nt * n, nt, n, tab8.get(), expv.get(), invexpv.get(), (long)nt * n, C, s));
        DQ_HIP(hipStreamSynchronize(s));
        return 0;
    }

    // one launch of the checkerboard kernel on this engine's pair tables (chains / par_stride differ for the batched initialisation)
    int cb_apply(CMat in, Mat out, Mat outT, bool reverse, bool inverse, CVec rs_in, CVec cs_in, CVec rs_out, CVec cs_out, int chains, long par_stride) {
        CbDesc d; d.in = in; d.out = out; d.outT = outT; d.partner = cb_partner.get(); d.n_groups = cb_groups; d.reverse = reverse ? 1 : 0; d.inverse = inverse ? 1 : 0;
        d.par = cb_par.get(); d.par_stride = par_stride; d.rs_in = rs_in; d.cs_in = cs_in; d.rs_out = rs_out; d.cs_out = cs_out; d.n = n;
        return launch_cb_apply(d, chains, s);
    }
    // dqmc_set_checkerboard: pair tables to the device, then E and E^-1 as dense matrices (the kernel applied to I) for the
    // paths that stay GEMMs (the unequal-time series and the first factor of a B-bar product)
    int set_checkerboard(int n_groups, const int32_t* bonds, const int32_t* group_sizes, const double* ch, const double* sh, const double* f) {
        if (n_groups < 1 || n_groups > 64 || !bonds || !group_sizes || !ch || !sh || !f) { set_error("set_checkerboard: bad argument"); return DQMC_EINVAL; }
        if (n > 4096) { set_error("set_checkerboard: n_sites > 4096"); return DQMC_EINVAL; }
        std::vector<int> partner((size_t)n_groups * n);
        size_t b = 0;
        for (int g = 0; g < n_groups; ++g) {
            int* pt = partner.data() + (size_t)g * n;
            for (int i = 0; i < n; ++i) pt[i] = i;
            if (group_sizes[g] < 0 || group_sizes[g] > n / 2) { set_error("set_checkerboard: a group holds at most n_sites/2 bonds"); return DQMC_EINVAL; }
            for (int k = 0; k < group_sizes[g]; ++k, ++b) {
                const int i = bonds[2 * b], j = bonds[2 * b + 1];
                if (i < 0 || i >= n || j < 0 || j >= n || i == j) { set_error("set_checkerboard: bond site out of range"); return DQMC_EINVAL; }
                if (pt[i] != i || pt[j] != j) { set_error("set_checkerboard: the bonds of one group must be disjoint"); return DQMC_EINVAL; }
                pt[i] = j; pt[j] = i;
            }
        }
        std::vector<double> par((size_t)C * 4);
        for (int c = 0; c < C; ++c) {
            if (!(f[c] > 0.0) || !std::isfinite(ch[c]) || !std::isfinite(sh[c])) { set_error("set_checkerboard: diag_factor must be positive, cosh / sinh finite"); return DQMC_EINVAL; }
            par[4 * c] = ch[c]; par[4 * c + 1] = sh[c]; par[4 * c + 2] = f[c]; par[4 * c + 3] = 1.0 / f[c];
        }
        DQ_HIP(hipStreamSynchronize(s));
        if (!cb_par) DQ_TRY(dev_alloc(cb_par, (size_t)C * 4));
        DevPtr<int> pt;                                                 // the engine keeps its old table until the new one is on the device
        DQ_TRY(dev_alloc(pt, partner.size()));
        DQ_HIP(hipMemcpy(pt.get(), partner.data(), sizeof(int) * partner.size(), hipMemcpyHostToDevice));
        DQ_HIP(hipMemcpy(cb_par.get(), par.data(), sizeof(double) * par.size(), hipMemcpyHostToDevice));
        cb_partner = std::move(pt); cb_groups = n_groups; cb = true;
        Mat id{bb0.get(), nn};
        DQ_TRY(launch_set_identity(id, n, C, s));
        DQ_TRY(cb_apply(id, Mat{expK.get(), nn}, Mat{nullptr, 0}, false, false, CVec(), CVec(), CVec(), CVec(), C, 4)); // E = f E_{G-1} ... E_0
        DQ_TRY(cb_apply(id, Mat{invexpK.get(), nn}, Mat{nullptr, 0}, true, true, CVec(), CVec(), CVec(), CVec(), C, 4)); // E^-1 = E_0^-1 ... E_{G-1}^-1 / f
        stack_valid = false; gt_valid = false; ut_valid = false;
        DQ_HIP(hipStreamSynchronize(s));
        return 0;
    }

    // DQMC::calculate_Bbar (source/dqmc.cpp:88-105) without the multiply by I: result in *out
    int Bbar(int is, Mat* out) {
        const int l0 = is * n_stab;
        Mat cur{bb0.get(), nn}, nxt{bb1.get(), nn};
        DQ_TRY(launch_scale_rows(CMat(expK.get(), nn), ev(l0), cur, n, C, s));            // B_l0 = diag(expV) expK
        for (int loc = 1; loc <= loc_l_end[is]; ++loc) {
            if (cb) DQ_TRY(cb_apply(cur, nxt, Mat{nullptr, 0}, false, false, CVec(), CVec(), ev(l0 + loc), CVec(), C, 4));
            else DQ_TRY(ctx.gemm(CMat(expK.get(), nn), cur, nxt, ev(l0 + loc)));          // B_l * Bbar
            std::swap(cur, nxt);
        }
        *out = cur; return 0;
    }
    // DQMC::init_stacks + init_greenfunctions (source/dqmc.cpp:43-72)
    int init() {
        // Single chain, N <= 256, whole blocks: the n_stack products Bbar_i and their to_LDR factorisations do not depend on each
        // other (source/dqmc.cpp:47-53 computes them one after the other), so they run as ONE batch with the block index in the
        // kernels' chain dimension -- n_stab - 1 launches of the 64x64-tile GEMM for all blocks, one QRCP launch with a workgroup
        // per block on its own CU (20 x 0.84 ms side by side instead of in a row) -- and only the n_stack - 1 ldr_mul_ldr products,
        // which are a chain, stay sequential.  Halves the cost of an initialisation, i.e. of a replica-exchange round.
        if (C == 1 && n <= 256 && nt % n_stab == 0 && n_stack >= 2) return init_batched();
        const LdrRef tmp = spare.at(0);
        for (int i = n_stack - 1; i >= 0; --i) {
            Mat bb; DQ_TRY(Bbar(i, &bb));
            if (i == n_stack - 1) DQ_TRY(ctx.to_ldr(bb, stack.at(i)));
            else { DQ_TRY(ctx.to_ldr(bb, tmp)); DQ_TRY(ctx.ldr_mul_ldr(stack.at(i + 1), tmp, stack.at(i))); }
        }
        stack_valid = true;
        gt_valid = false;
        return ctx.inv_I_plus_ldr(stack.at(0), mG(), logdet.get());
    }
    int init_batched() {
        const int S = n_stack;
        if (!ib.tau) {
            InitBatch b; DQ_TRY(dev_alloc(b.bb, (size_t)2 * S * nn)); DQ_TRY(dev_alloc(b.tau, (size_t)S * n)); DQ_TRY(b.f.alloc(S, n, 1));
            ib = std::move(b);
        }
        const long bstride = (long)n_stab * n;                                            // exp(V) of block i starts n_stab slices further
        Mat cur{ib.bb.get(), nn}, nxt{ib.bb.get() + (size_t)S * nn, nn};
        DQ_TRY(launch_scale_rows(CMat(expK.get(), 0), CVec(expv.get(), bstride), cur, n, S, s)); // B_l0 of every block
        for (int loc = 1; loc < n_stab; ++loc) {
            if (cb) DQ_TRY(cb_apply(cur, nxt, Mat{nullptr, 0}, false, false, CVec(), CVec(), CVec(expv.get() + (long)loc * n, bstride), CVec(), S, 0));
            else {
                GemmDesc g; g.A = CMat(expK.get(), 0); g.B = cur; g.C = nxt; g.rs = CVec(expv.get() + (long)loc * n, bstride); g.n = n;
                DQ_TRY(launch_gemm(g, S, s));                                             // B_l * Bbar, all blocks
            }
            std::swap(cur, nxt);
        }
        // to_LDR(Bbar_i) for every block, S chains of the same choice as Ctx's minus the panel family (no panel workspace here);
        // one chain per store, so block i is chain i of the launch
        const LdrRef all = ib.f.at(0);
        QrWork w{ib.tau.get(), (long)n, all.jpvt, (long)n};
        w.info = ctx.info();
        DQ_TRY(launch_to_ldr(pick_qr(n, S, false), cur, all.L, all.d, all.R, w, n, S, s));
        // stack[S - 1] = its own factorisation (R a single permuted-triangular factor), then the chain of products
        const LdrRef last = stack.at(S - 1), own = ib.f.at(S - 1);
        DQ_TRY(launch_copy(own.L, last.L, nn, 1, s));
        DQ_TRY(launch_copy(own.R, last.R, nn, 1, s));
        DQ_HIP(hipMemcpyAsync(last.d.p, own.d.p, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
        DQ_HIP(hipMemcpyAsync(last.jpvt, own.jpvt, sizeof(int) * n, hipMemcpyDeviceToDevice, s));
        *last.tri = true; last.touch();
        for (int i = S - 2; i >= 0; --i) DQ_TRY(ctx.ldr_mul_ldr(stack.at(i + 1), ib.f.at(i), stack.at(i)));
        stack_valid = true;
        gt_valid = false;
        return ctx.inv_I_plus_ldr(stack.at(0), mG(), logdet.get());
    }
    // DQMC::propagate_GF_forward (source/dqmc.cpp:113-132): G = B_l G B_l^-1
    int wrap_forward(int l) {
        if (cb) {
            // T^T = (E G)^T;  (T E^-1)^T = E^-T T^T with E^-T = E_{G-1}^-1 ... E_0^-1 / f: groups 0 .. G-1, inverse;  G' = diag(ev) (T E^-1) diag(iev)
            DQ_TRY(cb_apply(mG(), Mat{nullptr, 0}, ctx.T(0), false, false, CVec(), CVec(), CVec(), CVec(), C, 4));
            gt_valid = use_gt();
            return cb_apply(ctx.T(0), Mat{GT.get(), nn}, mG(), false, true, CVec(), CVec(), iev(l), ev(l), C, 4);
        }
        DQ_TRY(ctx.gemm(CMat(expK.get(), nn), mG(), ctx.T(0)));
        gt_valid = use_gt();                                          // the GEMM that writes G writes GT as well
        return ctx.gemm(ctx.T(0), CMat(invexpK.get(), nn), mG(), ev(l), CVec(), iev(l), 0, 0, use_gt() ? Mat{GT.get(), nn} : Mat{nullptr, 0});
    }
    // The B-bar chain rides on the wraps (single chain, dense kinetic factor, N <= 256: the regime where a 256^3 product IS its launch).
    // calculate_Bbar (source/dqmc.cpp:88-105) is n_stab - 1 dependent products per stabilisation, 5.6 us each of which ~4.5 us are the launch:
    // each of them has an operand in common with a wrap product of the same sweep, so it is computed as a SECOND "chain" of that launch
    // (the GEMM kernels take the chain index in blockIdx.y and per-operand chain strides: chain 1's operands are simply other buffers).
    //   forward  (wrap BEFORE the update of its slice): the wrap of slice l starts with expK * G; beside it P <- diag(e^{V_{l-1}}) expK P
    //            with the fields slice l - 1 has just been given -- the factor of the block's last slice is one explicit product;
    //   backward (wrap AFTER the update): the wrap of slice l ends with T diag(e^{V_l}) expK; beside it P <- P diag(e^{V_l}) expK = P B_l.
    // The first factor of a block multiplies the identity.  Same products, same kernel, same association in the forward sweep as Bbar();
    // in the backward sweep the chain is associated from the other end.
    // With the persistent delayed-update kernel (bbar_rides()) a ridden product still cost ~3.4 us of the wrap it rode on (512 workgroups
    // on 256 CUs), so the products move on to the next SLICE launch, whose flush workgroups are idle until the walk's first window
    // (slice_rider, update.hip): the same operands, buffers and tile arithmetic, one launch later, and the wraps are single-chain again.
    //   forward : the launch of slice l (loc >= 1) carries P <- diag(e^{V_{l-1}}) expK P -- slice l - 1 is final, slice l's row is not read;
    //   backward: P <- P B_l is carried by the launch of slice l - 1; the product of a block's last slice in walking order (loc == 0)
    //             stays on its wrap, because the stabilisation right behind it needs P.
    // DQMC_BBAR_RIDER=0 keeps every product on the wraps.
    bool piggyback() const { return C == 1 && !cb && n <= 256 && pg_eye != nullptr; }
    bool bbar_rides() const { return piggyback() && is_persistent_walk(slice_path) && switches().bbar_rider; }
    SliceRider rider_forward(int l, const double* Pprev, double* Pnext) const {      // chain 1 of wrap_forward_piggy(l)
        SliceRider r; r.A = expK.get(); r.B = Pprev; r.C = Pnext; r.rs = expv.get() + (long)(l - 1) * n;
        return r;
    }
    SliceRider rider_backward(int l, const double* Pprev, double* Pnext) const {     // chain 1 of wrap_backward_piggy(l), without the scratch transpose
        SliceRider r; r.A = Pprev; r.B = expK.get(); r.C = Pnext; r.ks = expv.get() + (long)l * n;
        return r;
    }
    int wrap_forward_piggy(int l, const double* Pprev, double* Pnext) {
        GemmDesc g; g.A = CMat(expK.get(), 0); g.B = CMat(G.get(), (long)(Pprev - G.get())); g.C = Mat{ctx.T(0).p, (long)(Pnext - ctx.T(0).p)};
        g.rs = CVec(pg_ones.get(), (long)((expv.get() + (long)(l - 1) * n) - pg_ones.get())); g.n = n;
        DQ_TRY(launch_gemm(g, 2, s));
        gt_valid = use_gt();
        return ctx.gemm(ctx.T(0), CMat(invexpK.get(), nn), mG(), ev(l), CVec(), iev(l), 0, 0, use_gt() ? Mat{GT.get(), nn} : Mat{nullptr, 0});
    }
    int wrap_backward_piggy(int l, const double* Pprev, double* Pnext) {
        DQ_TRY(ctx.gemm(CMat(invexpK.get(), nn), mG(), ctx.T(0), CVec(), iev(l)));
        gt_valid = use_gt();
        GemmDesc g; g.A = CMat(ctx.T(0).p, (long)(Pprev - ctx.T(0).p)); g.B = CMat(expK.get(), 0); g.C = Mat{G.get(), (long)(Pnext - G.get())};
        g.ks = CVec(expv.get() + (long)l * n, 0); g.n = n;
        if (use_gt()) g.CT = Mat{GT.get(), (long)(ctx.T(1).p - GT.get())}; // chain 1's transposed copy goes to scratch
        return launch_gemm(g, 2, s);
    }
    // DQMC::propagate_GF_backward (source/dqmc.cpp:169-187): G = B_l^-1 G B_l
    int wrap_backward(int l) {
        if (cb) {
            // T^T = (E^-1 diag(iev) G diag(ev))^T;  (T E)^T = E^T T^T with E^T = f E_0 ... E_{G-1}: groups G-1 .. 0, forward
            DQ_TRY(cb_apply(mG(), Mat{nullptr, 0}, ctx.T(0), true, true, iev(l), ev(l), CVec(), CVec(), C, 4));
            gt_valid = use_gt();
            return cb_apply(ctx.T(0), Mat{GT.get(), nn}, mG(), true, false, CVec(), CVec(), CVec(), CVec(), C, 4);
        }
        DQ_TRY(ctx.gemm(CMat(invexpK.get(), nn), mG(), ctx.T(0), CVec(), iev(l)));
        gt_valid = use_gt();
        return ctx.gemm(ctx.T(0), CMat(expK.get(), nn), mG(), CVec(), ev(l), CVec(), 0, 0, use_gt() ? Mat{GT.get(), nn} : Mat{nullptr, 0});
    }
    // the walk reads rows of G from a transposed copy: the register walk (n <= 256) and the persistent sub-matrix kernel (any n)
    bool use_gt() const { return n <= 256 || slice_path == SlicePath::PersistentSubmatrix; }     // n > 256: only the persistent sub-matrix kernel reads and maintains GT
    UpdateDesc udesc() const {
        UpdateDesc d; d.G = mG(); d.fields = fields.get(); d.f_stride = (long)nt * n; d.expv = expv.get(); d.invexpv = invexpv.get(); d.v_stride = (long)nt * n;
        d.tabs = tabs.get(); d.perm = rs_perm.get(); d.kprop = rs_k.get(); d.u = rs_u.get(); d.rs_stride = (long)nt * n; d.Upanel = Upanel.get(); d.Wpanel = Wpanel.get(); d.Cpanel = Cpanel.get();
        d.panel_stride = (long)panel_rows * n; d.state = state.get(); d.state_stride = 4; d.prep = prep.get(); d.prep_stride = 4L * n; d.slice_sync = is_persistent(slice_path) ? slice_sync.get() : nullptr; d.slice_epoch = slice_epoch; d.slice_absent_tile = slice_absent_tile; d.slice_absent_l = slice_absent_l; d.slice_late_tile = slice_late_tile; d.slice_late_us = slice_late_us; d.GT = Mat{GT.get(), nn}; d.gt_valid = gt_valid ? 1 : 0; d.info = ctx.info(); d.acc_out = acc.get(); d.acc_stride = nt; d.n = n; d.nt = nt;
        return d;
    }
    // rider: a B-bar product for the flush workgroups of this launch (bbar_rides() only)
    int local_update(int l, const SliceRider* rider = nullptr) {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (profiling) {
            if (ev_used == ev_pairs.size()) { hipEvent_t a, b; DQ_HIP(hipEventCreate(&a)); DQ_HIP(hipEventCreate(&b)); ev_pairs.emplace_back(a, b); }
            e0 = ev_pairs[ev_used].first; e1 = ev_pairs[ev_used].second; ++ev_used;
            DQ_HIP(hipEventRecord(e0, s));
        }
        if (is_persistent(slice_path)) {
            // every launch of a persistent slice kernel gets its own number: the hand-off words carry it, so none has to be re-armed
            if (++slice_epoch >= SLICE_EPOCH_LIMIT) { DQ_HIP(hipMemsetAsync(slice_sync.get(), 0, (size_t)C * SLICE_SYNC_BYTES, s)); slice_epoch = 1; }
        }
        UpdateDesc d = udesc();
        if (rider) d.rider = *rider;
        DQ_TRY(launch_update_slice(slice_path, d, l, l, C, s));
        if (rider) ++rider_launches;
        if (profiling) DQ_HIP(hipEventRecord(e1, s));
        return 0;
    }
    // The random stream of `rows` slices [rows][n], checked in one pass without allocating: the device indexes G with perm and the
    // proposal table with kprop, so every slice must carry a permutation of the sites and proposal indices in {0, 1, 2} (what
    // std::shuffle and uniform_int(0, 2) produce, source/update.cpp:14, include/field.h:79).  `who` prefixes the error message.
    int check_stream(const char* who, const int32_t* perm, const uint8_t* kprop, const double* u, size_t rows) {
        if (!perm || !kprop || !u) { set_error(std::string(who) + ": null random-stream pointer"); return DQMC_EINVAL; }
        seen.assign((size_t)n, 0);
        for (size_t row = 0; row < rows; ++row) {
            const int32_t* pr = perm + row * n; const uint8_t* kr = kprop + row * n; const unsigned char mark = (unsigned char)(1 + (row & 1));
            if ((row & 1) == 0) std::fill(seen.begin(), seen.end(), 0);
            for (int idx = 0; idx < n; ++idx) {
                const int32_t i = pr[idx];
                if (i < 0 || i >= n || seen[i] == mark || kr[idx] > 2) { set_error(std::string(who) + ": perm is not a permutation of the sites, or kprop > 2"); return DQMC_EINVAL; }
                seen[i] = mark;
            }
        }
        return 0;
    }
    int upload_stream(const int32_t* perm, const uint8_t* kprop, const double* u) {
        const size_t cnt = (size_t)C * nt * n;
        DQ_TRY(check_stream("sweep", perm, kprop, u, (size_t)C * nt));
        DQ_HIP(hipEventSynchronize(stage_free));                   // previous H2D copies out of the staging buffer are done
        char* base = h_stage.get();
        double* hu = reinterpret_cast<double*>(base);
        int32_t* hp = reinterpret_cast<int32_t*>(base + cnt * sizeof(double));
        uint8_t* hk = reinterpret_cast<uint8_t*>(base + cnt * (sizeof(double) + sizeof(int32_t)));
        std::memcpy(hu, u, cnt * sizeof(double)); std::memcpy(hp, perm, cnt * sizeof(int32_t)); std::memcpy(hk, kprop, cnt);
        DQ_HIP(hipMemcpyAsync(rs_u.get(), hu, cnt * sizeof(double), hipMemcpyHostToDevice, s));
        DQ_HIP(hipMemcpyAsync(rs_perm.get(), hp, cnt * sizeof(int32_t), hipMemcpyHostToDevice, s));
        DQ_HIP(hipMemcpyAsync(rs_k.get(), hk, cnt, hipMemcpyHostToDevice, s));
        DQ_HIP(hipEventRecord(stage_free, s));
        return 0;
    }
    // the stream of half-sweep counter h into rs_*: stream order keeps it behind the readers of the previous half sweep, and nothing
    // leaves the host, so there is no staging buffer to wait for
    int fill_stream(uint32_t h) {
        return launch_rng_fill(rs_perm.get(), rs_k.get(), rs_u.get(), n, nt, rng_seed, rng_first_chain, h, C, s);
    }
    // the random stream of a sweep call: explicit arrays are uploaded; all three NULL draws the next half sweep of a seeded engine
    int stage_stream(const char* who, const int32_t* perm, const uint8_t* kprop, const double* u) {
        if (perm && kprop && u) return upload_stream(perm, kprop, u);
        if (perm || kprop || u) { set_error(std::string(who) + ": pass all three random-stream arrays or none"); return DQMC_EINVAL; }
        if (!rng_seeded) { set_error(std::string(who) + ": null random-stream pointer (the engine draws its own stream only after dqmc_rng_seed)"); return DQMC_EINVAL; }
        if (rng_counter == UINT32_MAX) { set_error(std::string(who) + ": the half-sweep counter of this seed is used up (2^32 - 1)"); return DQMC_ERANGE; }
        DQ_TRY(fill_stream(rng_counter));
        ++rng_counter;
        return 0;
    }
    // DQMC::sweep_0_to_beta (source/dqmc.cpp:337-396)
    int sweep_fwd() {
        int n_err = 0;
        DQ_HIP(hipMemsetAsync(err.get(), 0, sizeof(double) * C * n_stack, s));       // max_abs_diff folds into zeroed slots
        const bool pg = piggyback(), ride = bbar_rides();
        double* Pcur = bb0.get(); double* Pnxt = bb1.get();
        for (int l = 0; l < nt; ++l) {
            const int is = stack_idx(l), loc = local_l(l);
            if (pg && loc >= 1) {                                                             // P = B_{l-1} ... B_{l0}
                const double* Pprev = loc == 1 ? pg_eye.get() : Pcur;
                if (ride) { const SliceRider r = rider_forward(l, Pprev, Pnxt); DQ_TRY(wrap_forward(l)); DQ_TRY(local_update(l, &r)); }
                else { DQ_TRY(wrap_forward_piggy(l, Pprev, Pnxt)); DQ_TRY(local_update(l)); }
                std::swap(Pcur, Pnxt);
            } else { DQ_TRY(wrap_forward(l)); DQ_TRY(local_update(l)); }
            if (loc == loc_l_end[is]) {
                std::swap(G, Gtmp);                                                          // the wrapped G is kept for check_error, the stabilised one is written into the other buffer (no copy)
                Mat bb;
                if (pg) {                                                                     // the block's last factor, whose slice has only now been updated
                    if (loc == 0) DQ_TRY(launch_scale_rows(CMat(expK.get(), nn), ev(l), Mat{Pnxt, nn}, n, C, s));
                    else DQ_TRY(ctx.gemm(CMat(expK.get(), nn), CMat(Pcur, nn), Mat{Pnxt, nn}, ev(l)));
                    std::swap(Pcur, Pnxt); bb = Mat{Pcur, nn};
                } else DQ_TRY(Bbar(is, &bb));
                if (is == 0) DQ_TRY(ctx.to_ldr(bb, stack.at(0)));                                  // update_stack_forward :134-146
                else DQ_TRY(ctx.mat_mul_ldr(bb, stack.at(is - 1), stack.at(is)));
                gt_valid = false;                                                            // G is replaced below
                if (l == nt - 1) DQ_TRY(ctx.inv_I_plus_ldr(stack.at(is), mG(), logdet.get()));           // stabilize_GF_forward :148-161
                else DQ_TRY(ctx.inv_I_plus_ldr_mul_ldr(stack.at(is), stack.at(is + 1), mG()));
                DQ_TRY(launch_max_abs_diff(CMat(Gtmp.get(), nn), mG(), err.get() + n_err, n_stack, n, C, s)); // check_error :317-329
                ++n_err;
            }
        }
        return launch_fold_stats(dstats.get(), acc.get(), nt, nt, err.get(), n_stack, n_err, n, nt, C, s);
    }
    // DQMC::sweep_beta_to_0 (source/dqmc.cpp:398-456)
    int sweep_bwd() {
        int n_err = 0;
        DQ_HIP(hipMemsetAsync(err.get(), 0, sizeof(double) * C * n_stack, s));
        const bool pg = piggyback(), ride = bbar_rides();
        double* Pcur = bb0.get(); double* Pnxt = bb1.get();
        SliceRider pending; bool have_pending = false;                                        // P B_{l+1}, carried by the launch of slice l
        for (int l = nt - 1; l >= 0; --l) {
            DQ_TRY(local_update(l, have_pending ? &pending : nullptr));
            if (have_pending) { std::swap(Pcur, Pnxt); have_pending = false; }
            const int is = stack_idx(l);
            if (pg) {                                                                         // P = B_hi ... B_l
                const double* Pprev = local_l(l) == loc_l_end[is] ? pg_eye.get() : Pcur;
                if (ride && local_l(l) != 0) { DQ_TRY(wrap_backward(l)); pending = rider_backward(l, Pprev, Pnxt); have_pending = true; }
                else { DQ_TRY(wrap_backward_piggy(l, Pprev, Pnxt)); std::swap(Pcur, Pnxt); }
            } else DQ_TRY(wrap_backward(l));
            if (local_l(l) == 0) {
                std::swap(G, Gtmp);
                Mat bb;
                if (pg) bb = Mat{Pcur, nn}; else DQ_TRY(Bbar(is, &bb));
                if (is == n_stack - 1) DQ_TRY(ctx.to_ldr(bb, stack.at(is)));                       // update_stack_backward :189-201
                else DQ_TRY(ctx.ldr_mul_mat(stack.at(is + 1), bb, stack.at(is)));
                gt_valid = false;
                if (l == 0) DQ_TRY(ctx.inv_I_plus_ldr(stack.at(is), mG(), logdet.get()));                // stabilize_GF_backward :203-215
                else {                                                                       // the next launch is a local update: G = X Y writes GT as well
                    DQ_TRY(ctx.inv_I_plus_ldr_mul_ldr(stack.at(is - 1), stack.at(is), mG(), use_gt() ? Mat{GT.get(), nn} : Mat{nullptr, 0}));
                    gt_valid = use_gt();
                    if (gt_check && gt_valid) {                                              // diagnostic: GT against a transpose of G
                        DQ_TRY(launch_transpose_scale(mG(), ctx.T(0), CVec(), n, C, s));
                        DQ_TRY(launch_max_abs_diff(CMat(GT.get(), nn), ctx.T(0), gt_err.get(), 1, n, C, s));
                        ++gt_checks;
                    }
                }
                DQ_TRY(launch_max_abs_diff(CMat(Gtmp.get(), nn), mG(), err.get() + n_err, n_stack, n, C, s));
                ++n_err;
            }
        }
        return launch_fold_stats(dstats.get(), acc.get(), nt, nt, err.get(), n_stack, n_err, n, nt, C, s);
    }
    // DQMC::sweep_unequalTime (source/dqmc.cpp:458-515) with propagate_unequalTime_GF_forward :223-248, propagate_Bt0_Bbt :250-264,
    // stabilize_unequalTime :266-285.  No Monte Carlo moves: B_l comes from the current fields (what the reference's B_ / invB_
    // caches hold after sweep_beta_to_0), Gtt[0] is the current G, Bbt = stack[i + 1] as the backward sweep left it.
    Mat utm(int which, int l) const { return Mat{ut.G[which].get() + (long)l * C * nn, nn}; }
    int sweep_unequal() {
        if (!ut.tmp) {
            UnequalTime u;
            for (int w = 0; w < 3; ++w) DQ_TRY(dev_alloc(u.G[w], (size_t)(nt + 1) * C * nn));
            DQ_TRY(dev_alloc(u.tmp, (size_t)3 * C * nn)); DQ_TRY(dev_alloc(u.err, (size_t)C * 3 * n_stack));
            const size_t mcount = (size_t)C * 3 * (nt + 1) * n;
            DQ_TRY(dev_alloc(u.meas_now, mcount)); DQ_TRY(dev_alloc(u.meas_sum, mcount)); DQ_TRY(u.bt.alloc(2, n, C));
            DQ_HIP(hipMemsetAsync(u.meas_sum.get(), 0, sizeof(double) * mcount, s));
            ut = std::move(u);
        }
        auto bt = [&](int b) { return ut.bt.at(b); };
        int cur = 0, n_err = 0;
        DQ_HIP(hipMemsetAsync(ut.err.get(), 0, sizeof(double) * C * 3 * n_stack, s));
        DQ_TRY(launch_copy(mG(), utm(0, 0), nn, C, s));
        for (int l = 0; l < nt; ++l) {
            if (l == 0) {                                                                            // :234-239
                DQ_TRY(launch_copy(utm(0, 0), utm(1, 0), nn, C, s));
                DQ_TRY(launch_axpb_identity(utm(0, 0), utm(2, 0), 1.0, -1.0, n, C, s));
            }
            DQ_TRY(ctx.gemm(CMat(expK.get(), nn), utm(0, l), ctx.T(0)));                             // :240 Gtt = B Gtt B^-1
            DQ_TRY(ctx.gemm(ctx.T(0), CMat(invexpK.get(), nn), utm(0, l + 1), ev(l), CVec(), iev(l)));
            DQ_TRY(ctx.gemm(CMat(expK.get(), nn), utm(1, l), utm(1, l + 1), ev(l)));                 // :241 Gt0 = B Gt0
            DQ_TRY(ctx.gemm(utm(2, l), CMat(invexpK.get(), nn), utm(2, l + 1), CVec(), CVec(), iev(l))); // :242 G0t = G0t B^-1
            const int is = stack_idx(l);
            if (local_l(l) == loc_l_end[is]) {
                for (int w = 0; w < 3; ++w) DQ_TRY(launch_copy(utm(w, l + 1), Mat{ut.tmp.get() + (long)w * C * nn, nn}, nn, C, s));
                Mat bb; DQ_TRY(Bbar(is, &bb));
                if (is == 0) DQ_TRY(ctx.to_ldr(bb, bt(cur)));                                        // :255-259
                else { DQ_TRY(ctx.mat_mul_ldr(bb, bt(cur), bt(cur ^ 1))); cur ^= 1; }
                if (l == nt - 1) {                                                                   // :267-276
                    DQ_TRY(ctx.inv_I_plus_ldr(bt(cur), utm(0, l + 1), logdet.get()));
                    DQ_TRY(launch_axpb_identity(utm(0, l + 1), utm(1, l + 1), -1.0, 1.0, n, C, s));
                    DQ_TRY(launch_axpb_identity(utm(0, l + 1), utm(2, l + 1), -1.0, 0.0, n, C, s));
                } else {                                                                             // :278-282, Bbt = stack[is + 1]
                    DQ_TRY(ctx.inv_I_plus_ldr_mul_ldr(bt(cur), stack.at(is + 1), utm(0, l + 1)));
                    DQ_TRY(ctx.inv_invldr_plus_ldr(bt(cur), stack.at(is + 1), utm(1, l + 1), false));
                    DQ_TRY(ctx.inv_invldr_plus_ldr(stack.at(is + 1), bt(cur), utm(2, l + 1), true));
                }
                for (int w = 0; w < 3; ++w) {                                                        // check_error x 3, :502-507
                    DQ_TRY(launch_max_abs_diff(CMat(ut.tmp.get() + (long)w * C * nn, nn), utm(w, l + 1), ut.err.get() + n_err, 3L * n_stack, n, C, s));
                    ++n_err;
                }
            }
        }
        ut_valid = true;
        return launch_fold_stats(dstats.get(), acc.get(), nt, 0, ut.err.get(), 3L * n_stack, n_err, n, nt, C, s);
    }
    int sync_and_check() {
        DQ_HIP(hipStreamSynchronize(s));
        if (profiling && ev_used) {
            for (size_t k = 0; k < ev_used; ++k) { float ms = 0.f; DQ_HIP(hipEventElapsedTime(&ms, ev_pairs[k].first, ev_pairs[k].second)); upd_ms += ms; }
            upd_launches += (long long)ev_used; ev_used = 0;
        }
        int bits = 0;
        const int rc = take_status(ctx, &bits);
        if (bits & (DQ_STATUS_HANDOFF | DQ_STATUS_CENSUS)) {        // a persistent slice kernel failed: the kernel pairs from now on
            slice_path = pick_slice_path(n, C, false); gt_valid = false;
            if (bits & DQ_STATUS_HANDOFF) { (void)hipMemset(slice_sync.get(), 0, (size_t)C * SLICE_SYNC_BYTES); slice_epoch = 0; }
        }
        return rc;
    }
    // the HS fields in the order of the ABI, [C][n][nt] (an arma::imat nt x n per chain); the device keeps them as [C][nt][n]
    int download_fields(std::vector<int8_t>& f) const {
        std::vector<int8_t> dev((size_t)C * nt * n);
        DQ_HIP(hipMemcpy(dev.data(), fields.get(), dev.size(), hipMemcpyDeviceToHost));
        f.resize(dev.size());
        for (int c = 0; c < C; ++c) for (int i = 0; i < n; ++i) for (int l = 0; l < nt; ++l)
            f[(size_t)c * nt * n + l + (size_t)nt * i] = dev[(size_t)c * nt * n + (size_t)l * n + i];
        return 0;
    }
    // equal-time observables [C][3 + n] on the device -> scalars [C][3], chi_r [C][n] (either may be null)
    int copy_out_equal_time(const double* src, double* scalars, double* chi_r) const {
        const size_t w = 3 + (size_t)n;
        std::vector<double> tmp((size_t)C * w);
        DQ_HIP(hipMemcpy(tmp.data(), src, sizeof(double) * tmp.size(), hipMemcpyDeviceToHost));
        for (int c = 0; c < C; ++c) {
            if (scalars) std::copy(tmp.begin() + c * w, tmp.begin() + c * w + 3, scalars + 3 * (size_t)c);
            if (chi_r) std::copy(tmp.begin() + c * w + 3, tmp.begin() + (c + 1) * w, chi_r + (size_t)c * n);
        }
        return 0;
    }
};

// ---- stateless calls: one cached single-chain context per n, with the inputs and outputs of the calls --------------------------------
struct Stateless {
    Ctx ctx;                                   // declared first: its stream outlives the scratch below
    LdrStore ldr;                              // 3 triples: two uploaded factors (0, 1) and the result (2)
    DevPtr<double> mats;                       // 4 n x n matrices M(0) .. M(3): uploaded operands and results
    DevPtr<double> logdet;                     // 1: log|det| of dqmc_inv_I_plus_ldr
    Mat M(int k) const { return Mat{mats.get() + k * ctx.nn, ctx.nn}; }
};
static std::mutex g_ctx_mu;
static std::map<int, std::unique_ptr<Stateless>> g_ctx;

static int get_ctx(int n, Stateless** out) {
    if (n <= 0) { set_error("n must be positive"); return DQMC_EINVAL; }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) { set_error("no HIP device available: this library requires a gfx950 GPU"); return DQMC_ENODEVICE; }
    auto it = g_ctx.find(n);
    if (it == g_ctx.end()) {
        std::unique_ptr<Stateless> x(new Stateless);
        DQ_TRY(x->ctx.init(n, 1, 0));
        DQ_TRY(x->ldr.alloc(3, n, 1)); DQ_TRY(dev_alloc(x->mats, 4L * n * n)); DQ_TRY(dev_alloc(x->logdet, 1));
        it = g_ctx.emplace(n, std::move(x)).first;
    }
    *out = it->second.get();
    return hipSetDevice(0) == hipSuccess ? 0 : DQMC_ENODEVICE;
}
// triple k of the stateless scratch receives a factor from the host: its R is not known to be a single QR factor
static int upload_ldr(Stateless* x, int k, const double* L, const double* d, const double* R, LdrRef* out) {
    const Ctx& c = x->ctx;
    *out = x->ldr.at(k); *out->tri = false;
    DQ_HIP(hipMemcpyAsync(out->L.p, L, sizeof(double) * c.nn, hipMemcpyHostToDevice, c.stream));
    DQ_HIP(hipMemcpyAsync(out->R.p, R, sizeof(double) * c.nn, hipMemcpyHostToDevice, c.stream));
    DQ_HIP(hipMemcpyAsync(out->d.p, d, sizeof(double) * c.n, hipMemcpyHostToDevice, c.stream));
    return 0;
}
static int download_ldr(Ctx* c, LdrRef f, double* L, double* d, double* R) {
    DQ_HIP(hipMemcpyAsync(L, f.L.p, sizeof(double) * c->nn, hipMemcpyDeviceToHost, c->stream));
    DQ_HIP(hipMemcpyAsync(R, f.R.p, sizeof(double) * c->nn, hipMemcpyDeviceToHost, c->stream));
    DQ_HIP(hipMemcpyAsync(d, f.d.p, sizeof(double) * c->n, hipMemcpyDeviceToHost, c->stream));
    DQ_HIP(hipStreamSynchronize(c->stream));
    return take_status(*c);
}

}  // namespace dq

using namespace dq;

struct dqmc_engine { Engine e; };

// the prologue of every engine call: a non-null handle, `e` its engine, the engine's device current
#define ENGINE_CALL(h) if (!(h)) { set_error("null engine"); return DQMC_EINVAL; } Engine& e = (h)->e; DQ_HIP(hipSetDevice(e.device))

namespace dq {
int engine_fields_view(dqmc_engine* h, EngineFieldsView* v) {
    if (!h || !v) { set_error("null engine"); return DQMC_EINVAL; }
    Engine& e = h->e;
    v->device = e.device; v->n = e.n; v->nt = e.nt; v->n_chains = e.C; v->fields = e.fields.get(); v->stream = e.s;
    return 0;
}
int engine_fields_changed(dqmc_engine* h) {
    ENGINE_CALL(h);
    e.stack_valid = false; e.gt_valid = false;
    return launch_build_expv(e.fields.get(), (long)e.nt * e.n, e.nt, e.n, e.tab8.get(), e.expv.get(), e.invexpv.get(), (long)e.nt * e.n, e.C, e.s);
}
int engine_exchange_scratch(dqmc_engine* h, int8_t** saved, int8_t** recv, int** tab) {
    ENGINE_CALL(h);
    if (!e.xch.tab) {
        Engine::Exchange x; DQ_TRY(dev_alloc(x.saved, (size_t)e.C * e.nt * e.n)); DQ_TRY(dev_alloc(x.recv, (size_t)2 * e.nt * e.n)); DQ_TRY(dev_alloc(x.tab, (size_t)2 * e.C));
        e.xch = std::move(x);
    }
    *saved = e.xch.saved.get(); *recv = e.xch.recv.get(); *tab = e.xch.tab.get();
    return 0;
}
}  // namespace dq

#define API_LOCK std::lock_guard<std::mutex> _lk(g_ctx_mu)

extern "C" {

const char* dqmc_last_error(void) { return get_error(); }
const char* dqmc_backend(void) { return "hip:gfx950"; }
int dqmc_device_count(void) { int c = 0; if (hipGetDeviceCount(&c) != hipSuccess) return 0; return c; }

int dqmc_to_ldr(int n, const double* M, double* L, double* d, double* R) {
    API_LOCK; Stateless* x; DQ_TRY(get_ctx(n, &x)); Ctx* c = &x->ctx;
    if (!M || !L || !d || !R) { set_error("null pointer"); return DQMC_EINVAL; }
    DQ_HIP(hipMemcpyAsync(x->M(0).p, M, sizeof(double) * c->nn, hipMemcpyHostToDevice, c->stream));
    LdrRef out = x->ldr.at(0);
    DQ_TRY(c->to_ldr(x->M(0), out));
    return download_ldr(c, out, L, d, R);
}
int dqmc_ldr_mul_mat(int n, const double* L, const double* d, const double* R, const double* M, double* Lo, double* d_o, double* Ro) {
    API_LOCK; Stateless* x; DQ_TRY(get_ctx(n, &x)); Ctx* c = &x->ctx;
    LdrRef F; DQ_TRY(upload_ldr(x, 0, L, d, R, &F));
    DQ_HIP(hipMemcpyAsync(x->M(0).p, M, sizeof(double) * c->nn, hipMemcpyHostToDevice, c->stream));
    LdrRef out = x->ldr.at(2);
    DQ_TRY(c->ldr_mul_mat(F, x->M(0), out));
    return download_ldr(c, out, Lo, d_o, Ro);
}
int dqmc_mat_mul_ldr(int n, const double* M, const double* L, const double* d, const double* R, double* Lo, double* d_o, double* Ro) {
    API_LOCK; Stateless* x; DQ_TRY(get_ctx(n, &x)); Ctx* c = &x->ctx;
    LdrRef F; DQ_TRY(upload_ldr(x, 0, L, d, R, &F));
    DQ_HIP(hipMemcpyAsync(x->M(0).p, M, sizeof(double) * c->nn, hipMemcpyHostToDevice, c->stream));
    LdrRef out = x->ldr.at(2);
    DQ_TRY(c->mat_mul_ldr(x->M(0), F, out));
    return download_ldr(c, out, Lo, d_o, Ro);
}
int dqmc_ldr_mul_ldr(int n, const double* L1, const double* d1, const double* R1, const double* L2, const double* d2, const double* R2, double* Lo, double* d_o, double* Ro) {
    API_LOCK; Stateless* x; DQ_TRY(get_ctx(n, &x)); Ctx* c = &x->ctx;
    LdrRef F1, F2; DQ_TRY(upload_ldr(x, 0, L1, d1, R1, &F1)); DQ_TRY(upload_ldr(x, 1, L2, d2, R2, &F2));
    LdrRef out = x->ldr.at(2);
    DQ_TRY(c->ldr_mul_ldr(F1, F2, out));
    return download_ldr(c, out, Lo, d_o, Ro);
}
int dqmc_inv_I_plus_ldr(int n, const double* L, const double* d, const double* R, double* G, double* logdet) {
    API_LOCK; Stateless* x; DQ_TRY(get_ctx(n, &x)); Ctx* c = &x->ctx;
    LdrRef F; DQ_TRY(upload_ldr(x, 0, L, d, R, &F));
    DQ_TRY(c->inv_I_plus_ldr(F, x->M(1), x->logdet.get()));
    DQ_HIP(hipMemcpyAsync(G, x->M(1).p, sizeof(double) * c->nn, hipMemcpyDeviceToHost, c->stream));
    double ld = 0.0;
    DQ_HIP(hipMemcpyAsync(&ld, x->logdet.get(), sizeof(double), hipMemcpyDeviceToHost, c->stream));
    DQ_HIP(hipStreamSynchronize(c->stream));
    if (logdet) *logdet = ld;
    return take_status(*c);
}
int dqmc_inv_I_plus_ldr_mul_ldr(int n, const double* L1, const double* d1, const double* R1, const double* L2, const double* d2, const double* R2, double* G) {
    API_LOCK; Stateless* x; DQ_TRY(get_ctx(n, &x)); Ctx* c = &x->ctx;
    LdrRef F1, F2; DQ_TRY(upload_ldr(x, 0, L1, d1, R1, &F1)); DQ_TRY(upload_ldr(x, 1, L2, d2, R2, &F2));
    DQ_TRY(c->inv_I_plus_ldr_mul_ldr(F1, F2, x->M(1)));
    DQ_HIP(hipMemcpyAsync(G, x->M(1).p, sizeof(double) * c->nn, hipMemcpyDeviceToHost, c->stream));
    DQ_HIP(hipStreamSynchronize(c->stream));
    return take_status(*c);
}
int dqmc_gemm(int n, const double* A, int transA, const double* B, int transB, double* Cm) {
    API_LOCK; Stateless* x; DQ_TRY(get_ctx(n, &x)); Ctx* c = &x->ctx;
    DQ_HIP(hipMemcpyAsync(x->M(0).p, A, sizeof(double) * c->nn, hipMemcpyHostToDevice, c->stream));
    DQ_HIP(hipMemcpyAsync(x->M(1).p, B, sizeof(double) * c->nn, hipMemcpyHostToDevice, c->stream));
    CMat Bm = x->M(1);
    if (transB) { DQ_TRY(launch_transpose_scale(x->M(1), x->M(2), CVec(), n, 1, c->stream)); Bm = x->M(2); }
    DQ_TRY(c->gemm(x->M(0), Bm, x->M(3), CVec(), CVec(), CVec(), transA ? 1 : 0));
    DQ_HIP(hipMemcpyAsync(Cm, x->M(3).p, sizeof(double) * c->nn, hipMemcpyDeviceToHost, c->stream));
    DQ_HIP(hipStreamSynchronize(c->stream));
    return 0;
}
int dqmc_rank1_update(int n, double* G, int i, double delta) {
    API_LOCK; Stateless* x; DQ_TRY(get_ctx(n, &x)); Ctx* c = &x->ctx;
    if (i < 0 || i >= n) { set_error("site index out of range"); return DQMC_ERANGE; }
    DQ_HIP(hipMemcpyAsync(x->M(0).p, G, sizeof(double) * c->nn, hipMemcpyHostToDevice, c->stream));
    DQ_TRY(launch_rank1(x->M(0), i, delta, x->M(1).p, 2L * n + 1, n, 1, c->stream));      // scratch: 2n + 1 doubles from M(1) on
    DQ_HIP(hipMemcpyAsync(G, x->M(0).p, sizeof(double) * c->nn, hipMemcpyDeviceToHost, c->stream));
    DQ_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

int dqmc_create_batch(dqmc_engine** out, int device, int n_chains, int n_sites, int nt, int n_stab, const double* g,
                      const double gamma[4], const double eta[4], const double* expK, const double* invexpK) {
    if (!out || n_chains <= 0 || n_sites <= 0 || nt <= 0 || n_stab <= 0 || !g || !gamma || !eta || !expK || !invexpK) { set_error("bad argument"); return DQMC_EINVAL; }
    if (n_sites > 1024) { set_error("n_sites > 1024 is not supported by the single-workgroup kernels"); return DQMC_EINVAL; }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) { set_error("no HIP device available: this library requires a gfx950 GPU"); return DQMC_ENODEVICE; }
    if (device < 0 || device >= count) { set_error("device ordinal out of range"); return DQMC_EINVAL; }
    dqmc_engine* h = new (std::nothrow) dqmc_engine;
    if (!h) return DQMC_ENOMEM;
    int rc = h->e.create(device, n_chains, n_sites, nt, n_stab, g, gamma, eta, expK, invexpK);
    if (rc) { delete h; return rc; }
    *out = h; return 0;
}
int dqmc_create(dqmc_engine** out, int device, int n_sites, int nt, int n_stab, double g, const double gamma[4], const double eta[4],
                const double* expK, const double* invexpK) {
    return dqmc_create_batch(out, device, 1, n_sites, nt, n_stab, &g, gamma, eta, expK, invexpK);
}
int dqmc_set_checkerboard(dqmc_engine* h, int n_groups, const int32_t* bonds, const int32_t* group_sizes, const double* cosh_t, const double* sinh_t,
                          const double* diag_factor) {
    ENGINE_CALL(h);
    return e.set_checkerboard(n_groups, bonds, group_sizes, cosh_t, sinh_t, diag_factor);
}
void dqmc_destroy(dqmc_engine* h) { if (h) { (void)hipSetDevice(h->e.device); delete h; } }
int dqmc_n_chains(dqmc_engine* h) { return h ? h->e.C : 0; }

int dqmc_set_fields(dqmc_engine* h, const int64_t* f) {
    ENGINE_CALL(h);
    std::vector<int8_t> tmp((size_t)e.C * e.nt * e.n);
    for (int c = 0; c < e.C; ++c) for (int i = 0; i < e.n; ++i) for (int l = 0; l < e.nt; ++l) {
        const int64_t v = f[(size_t)c * e.nt * e.n + l + (size_t)e.nt * i];
        if (v < 0 || v > 3) { set_error("field value outside {0,1,2,3}"); return DQMC_EINVAL; }
        tmp[(size_t)c * e.nt * e.n + (size_t)l * e.n + i] = (int8_t)v;
    }
    DQ_HIP(hipStreamSynchronize(e.s));
    DQ_HIP(hipMemcpy(e.fields.get(), tmp.data(), tmp.size(), hipMemcpyHostToDevice));
    DQ_TRY(launch_build_expv(e.fields.get(), (long)e.nt * e.n, e.nt, e.n, e.tab8.get(), e.expv.get(), e.invexpv.get(), (long)e.nt * e.n, e.C, e.s));
    DQ_HIP(hipStreamSynchronize(e.s));
    return 0;
}
int dqmc_get_fields(dqmc_engine* h, int64_t* f) {
    ENGINE_CALL(h);
    DQ_TRY(e.sync_and_check());
    std::vector<int8_t> tmp; DQ_TRY(e.download_fields(tmp));
    std::copy(tmp.begin(), tmp.end(), f);
    return 0;
}
int dqmc_init(dqmc_engine* h) { ENGINE_CALL(h); DQ_TRY(e.init()); return e.sync_and_check(); }
int dqmc_get_G(dqmc_engine* h, double* G) {
    ENGINE_CALL(h); DQ_TRY(e.sync_and_check());
    DQ_HIP(hipMemcpy(G, e.G.get(), sizeof(double) * e.C * e.nn, hipMemcpyDeviceToHost)); return 0;
}
int dqmc_set_G(dqmc_engine* h, const double* G) {
    ENGINE_CALL(h); DQ_HIP(hipStreamSynchronize(e.s));
    DQ_HIP(hipMemcpy(e.G.get(), G, sizeof(double) * e.C * e.nn, hipMemcpyHostToDevice)); e.gt_valid = false; return 0;
}
int dqmc_get_logdet(dqmc_engine* h, double* ld) {
    ENGINE_CALL(h); DQ_TRY(e.sync_and_check());
    DQ_HIP(hipMemcpy(ld, e.logdet.get(), sizeof(double) * e.C, hipMemcpyDeviceToHost)); return 0;
}
int dqmc_n_stack(dqmc_engine* h) { return h ? h->e.n_stack : 0; }
int dqmc_get_stack(dqmc_engine* h, int i, double* L, double* d, double* R) {
    ENGINE_CALL(h);
    if (i < 0 || i >= e.n_stack) { set_error("LDR Stack index out of bounds"); return DQMC_ERANGE; }
    if (!e.stack_valid) { set_error("stack not initialised: call dqmc_init first"); return DQMC_EINVAL; }
    DQ_TRY(e.sync_and_check());
    LdrRef f = e.stack.at(i);
    DQ_HIP(hipMemcpy(L, f.L.p, sizeof(double) * e.C * e.nn, hipMemcpyDeviceToHost));
    DQ_HIP(hipMemcpy(R, f.R.p, sizeof(double) * e.C * e.nn, hipMemcpyDeviceToHost));
    DQ_HIP(hipMemcpy(d, f.d.p, sizeof(double) * e.C * e.n, hipMemcpyDeviceToHost));
    return 0;
}
int dqmc_sweep_0_to_beta(dqmc_engine* h, const int32_t* perm, const uint8_t* kprop, const double* u) {
    ENGINE_CALL(h);
    if (!e.stack_valid) { set_error("dqmc_init must be called before sweeping"); return DQMC_EINVAL; }
    DQ_TRY(e.stage_stream("sweep_0_to_beta", perm, kprop, u)); return e.sweep_fwd();
}
int dqmc_sweep_beta_to_0(dqmc_engine* h, const int32_t* perm, const uint8_t* kprop, const double* u) {
    ENGINE_CALL(h);
    if (!e.stack_valid) { set_error("dqmc_init must be called before sweeping"); return DQMC_EINVAL; }
    DQ_TRY(e.stage_stream("sweep_beta_to_0", perm, kprop, u)); return e.sweep_bwd();
}
int dqmc_sync(dqmc_engine* h) { ENGINE_CALL(h); return e.sync_and_check(); }
int dqmc_rng_seed(dqmc_engine* h, uint64_t seed, uint32_t first_chain, uint32_t counter) {
    ENGINE_CALL(h);
    if ((uint64_t)first_chain + (uint64_t)e.C - 1 > UINT32_MAX) { set_error("rng_seed: first_chain + n_chains - 1 exceeds 32 bits"); return DQMC_EINVAL; }
    e.rng_seeded = true; e.rng_seed = seed; e.rng_first_chain = first_chain; e.rng_counter = counter;
    return 0;
}
int dqmc_rng_state(dqmc_engine* h, uint64_t* seed, uint32_t* first_chain, uint32_t* counter, int* seeded) {
    if (!h) { set_error("null engine"); return DQMC_EINVAL; }
    const Engine& e = h->e;
    if (seed) *seed = e.rng_seed;
    if (first_chain) *first_chain = e.rng_first_chain;
    if (counter) *counter = e.rng_counter;
    if (seeded) *seeded = e.rng_seeded ? 1 : 0;
    return 0;
}
int dqmc_rng_draw(dqmc_engine* h, uint32_t counter, int32_t* perm, uint8_t* kprop, double* u) {
    ENGINE_CALL(h);
    if (!perm || !kprop || !u) { set_error("rng_draw: null pointer"); return DQMC_EINVAL; }
    if (!e.rng_seeded) { set_error("rng_draw: the engine has no seed (dqmc_rng_seed)"); return DQMC_EINVAL; }
    // rs_* are scratch between sweep calls: every sweep fills or uploads them before it reads them
    DQ_TRY(e.fill_stream(counter));
    DQ_TRY(e.sync_and_check());
    const size_t cnt = (size_t)e.C * e.nt * e.n;
    DQ_HIP(hipMemcpy(perm, e.rs_perm.get(), cnt * sizeof(int32_t), hipMemcpyDeviceToHost));
    DQ_HIP(hipMemcpy(kprop, e.rs_k.get(), cnt, hipMemcpyDeviceToHost));
    DQ_HIP(hipMemcpy(u, e.rs_u.get(), cnt * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}
int dqmc_get_stats(dqmc_engine* h, dqmc_stats* out) {
    ENGINE_CALL(h); DQ_TRY(e.sync_and_check());
    static_assert(sizeof(DevStats) == sizeof(dqmc_stats), "stats layout");
    DQ_HIP(hipMemcpy(out, e.dstats.get(), sizeof(DevStats) * e.C, hipMemcpyDeviceToHost)); return 0;
}
int dqmc_wrap_forward(dqmc_engine* h, int l) {
    ENGINE_CALL(h);
    if (l < 0 || l >= e.nt) { set_error("time slice out of range"); return DQMC_ERANGE; }
    return e.wrap_forward(l);
}
int dqmc_wrap_backward(dqmc_engine* h, int l) {
    ENGINE_CALL(h);
    if (l < 0 || l >= e.nt) { set_error("time slice out of range"); return DQMC_ERANGE; }
    return e.wrap_backward(l);
}
int dqmc_local_update_slice(dqmc_engine* h, int l, const int32_t* perm, const uint8_t* kprop, const double* u, int* accepted) {
    ENGINE_CALL(h);
    if (l < 0 || l >= e.nt) { set_error("time slice out of range"); return DQMC_ERANGE; }
    DQ_TRY(e.check_stream("local_update_slice", perm, kprop, u, e.C));       // one slice per chain, same contract as the sweeps
    DQ_HIP(hipStreamSynchronize(e.s));
    for (int c = 0; c < e.C; ++c) {
        const size_t off = ((size_t)c * e.nt + l) * e.n;
        DQ_HIP(hipMemcpy(e.rs_perm.get() + off, perm + (size_t)c * e.n, sizeof(int32_t) * e.n, hipMemcpyHostToDevice));
        DQ_HIP(hipMemcpy(e.rs_k.get() + off, kprop + (size_t)c * e.n, e.n, hipMemcpyHostToDevice));
        DQ_HIP(hipMemcpy(e.rs_u.get() + off, u + (size_t)c * e.n, sizeof(double) * e.n, hipMemcpyHostToDevice));
    }
    DQ_TRY(e.local_update(l));
    DQ_TRY(launch_fold_stats(e.dstats.get(), e.acc.get() + l, e.nt, 1, e.err.get(), e.n_stack, 0, e.n, e.nt, e.C, e.s));
    DQ_TRY(e.sync_and_check());
    if (accepted) for (int c = 0; c < e.C; ++c) DQ_HIP(hipMemcpy(accepted + c, e.acc.get() + (size_t)c * e.nt + l, sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}
int dqmc_rng_fill_time(dqmc_engine* h, int launches, double* ms_per_launch) {
    ENGINE_CALL(h);
    if (launches < 1 || !ms_per_launch) { set_error("rng_fill_time: launches >= 1 and a result pointer"); return DQMC_EINVAL; }
    if (!e.rng_seeded) { set_error("rng_fill_time: the engine has no seed (dqmc_rng_seed)"); return DQMC_EINVAL; }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    DQ_HIP(hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); set_error("rng_fill_time: hipEventCreate failed"); return DQMC_ENODEVICE; }
    int rc = e.fill_stream(e.rng_counter);                          // first launch of the kernel outside the timed window
    if (rc == 0 && hipEventRecord(e0, e.s) != hipSuccess) rc = DQMC_ENODEVICE;
    for (int k = 0; k < launches && rc == 0; ++k) rc = e.fill_stream(e.rng_counter);
    if (rc == 0 && hipEventRecord(e1, e.s) != hipSuccess) rc = DQMC_ENODEVICE;
    if (rc == 0) rc = e.sync_and_check();
    float ms = 0.f;
    if (rc == 0 && hipEventElapsedTime(&ms, e0, e1) != hipSuccess) rc = DQMC_ENODEVICE;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (rc == 0) *ms_per_launch = (double)ms / launches;
    return rc;
}
int dqmc_calculate_Bbar(dqmc_engine* h, int is, double* out) {
    ENGINE_CALL(h);
    if (is < 0 || is >= e.n_stack) { set_error("stack index out of range"); return DQMC_ERANGE; }
    Mat bb; DQ_TRY(e.Bbar(is, &bb)); DQ_HIP(hipStreamSynchronize(e.s));
    DQ_HIP(hipMemcpy(out, bb.p, sizeof(double) * e.C * e.nn, hipMemcpyDeviceToHost)); return 0;
}
// AttractiveHubbard::global_action (source/model.cpp:140-159); the field sums run on the host copy
int dqmc_global_action(dqmc_engine* h, double* S) {
    ENGINE_CALL(h); DQ_TRY(e.sync_and_check());
    std::vector<int8_t> tmp; std::vector<double> ld(e.C);
    DQ_TRY(e.download_fields(tmp));
    DQ_HIP(hipMemcpy(ld.data(), e.logdet.get(), sizeof(double) * e.C, hipMemcpyDeviceToHost));
    const double alpha = -1.0;
    const size_t per = (size_t)e.nt * e.n;
    for (int c = 0; c < e.C; ++c) {
        double lb = 0.0, lg = 0.0;
        for (size_t k = 0; k < per; ++k) {                                // arma::imat memory order
            const int f = tmp[c * per + k];
            lb += alpha * e.g_host[c] * e.eta_host[f]; lg += std::log(e.gamma_host[f]);
        }
        S[c] = -2.0 * ld[c] - (lb + lg);
    }
    return 0;
}
int dqmc_sweep_unequal_time(dqmc_engine* h) {
    ENGINE_CALL(h);
    if (!e.stack_valid) { set_error("sweep_unequal_time: call dqmc_init first"); return DQMC_EINVAL; }
    return e.sweep_unequal();
}
int dqmc_get_G_tau(dqmc_engine* h, int which, int l, double* out) {
    ENGINE_CALL(h);
    if (which < 0 || which > 2 || l < 0 || l > e.nt) { set_error("get_G_tau: which in 0..2, l in 0..nt"); return DQMC_ERANGE; }
    if (!e.ut_valid) { set_error("get_G_tau: run dqmc_sweep_unequal_time first"); return DQMC_EINVAL; }
    DQ_TRY(e.sync_and_check());
    DQ_HIP(hipMemcpy(out, e.utm(which, l).p, sizeof(double) * e.C * e.nn, hipMemcpyDeviceToHost));
    return 0;
}
// DQMC::half_warp (source/dqmc.cpp:288-315): invexpK_half * M * expK_half, two GEMMs on the engine's stream
int dqmc_half_warp(dqmc_engine* h, const double* expK_half, const double* invexpK_half, int which, int l, double* out) {
    ENGINE_CALL(h);
    if (!out) { set_error("half_warp: out is NULL"); return DQMC_EINVAL; }
    if (which < -1 || which > 2 || (which >= 0 && (l < 0 || l > e.nt))) { set_error("half_warp: which in -1..2, l in 0..nt"); return DQMC_ERANGE; }
    if (which >= 0 && !e.ut_valid) { set_error("half_warp: run dqmc_sweep_unequal_time first"); return DQMC_EINVAL; }
    if ((expK_half == nullptr) != (invexpK_half == nullptr)) { set_error("half_warp: pass both half-step matrices or neither"); return DQMC_EINVAL; }
    if (expK_half) {
        if (!e.hw.out) { Engine::HalfWarp x; DQ_TRY(dev_alloc(x.expK, e.nn)); DQ_TRY(dev_alloc(x.invexpK, e.nn)); DQ_TRY(dev_alloc(x.out, (size_t)e.C * e.nn)); e.hw = std::move(x); }
        DQ_HIP(hipStreamSynchronize(e.s));                         // pageable host memory: the copies below are synchronous with respect to the host
        DQ_HIP(hipMemcpy(e.hw.expK.get(), expK_half, sizeof(double) * e.nn, hipMemcpyHostToDevice));
        DQ_HIP(hipMemcpy(e.hw.invexpK.get(), invexpK_half, sizeof(double) * e.nn, hipMemcpyHostToDevice));
    } else if (!e.hw.out) { set_error("half_warp: no half-step matrices uploaded yet"); return DQMC_EINVAL; }
    const CMat M = which < 0 ? CMat(e.mG()) : CMat(e.utm(which, l));
    DQ_TRY(e.ctx.gemm(CMat(e.hw.invexpK.get(), 0), M, e.ctx.T(0)));                // chain stride 0: one matrix for every chain
    DQ_TRY(e.ctx.gemm(e.ctx.T(0), CMat(e.hw.expK.get(), 0), Mat{e.hw.out.get(), e.nn}));
    DQ_TRY(e.sync_and_check());
    DQ_HIP(hipMemcpy(out, e.hw.out.get(), sizeof(double) * e.C * e.nn, hipMemcpyDeviceToHost));
    return 0;
}
int dqmc_measure_unequal_time(dqmc_engine* h, int L1, int L2, int accumulate, double* out) {
    ENGINE_CALL(h);
    if (L1 < 1 || L2 < 1 || L1 * L2 != e.n) { set_error("measure_unequal_time: L1*L2 must equal n_sites"); return DQMC_EINVAL; }
    if (!e.ut_valid) { set_error("measure_unequal_time: run dqmc_sweep_unequal_time first"); return DQMC_EINVAL; }
    const long stride = 3L * (e.nt + 1) * e.n;
    if (accumulate) {
        DQ_TRY(launch_measure_unequal_time(e.ut.G[0].get(), e.ut.G[1].get(), e.ut.G[2].get(), e.ut.meas_sum.get(), stride, L1, L2, e.nt, 1, e.C, e.s));
        ++e.ut_meas_count; return 0;
    }
    if (!out) { set_error("measure_unequal_time: out is NULL"); return DQMC_EINVAL; }
    DQ_TRY(launch_measure_unequal_time(e.ut.G[0].get(), e.ut.G[1].get(), e.ut.G[2].get(), e.ut.meas_now.get(), stride, L1, L2, e.nt, 0, e.C, e.s));
    DQ_TRY(e.sync_and_check());
    DQ_HIP(hipMemcpy(out, e.ut.meas_now.get(), sizeof(double) * e.C * stride, hipMemcpyDeviceToHost));
    return 0;
}
int dqmc_measure_unequal_fetch(dqmc_engine* h, double* out_sum, int64_t* n_measurements, int reset) {
    ENGINE_CALL(h); DQ_TRY(e.sync_and_check());
    if (!e.ut.meas_sum) { set_error("measure_unequal_fetch: nothing measured yet"); return DQMC_EINVAL; }
    const size_t cnt = (size_t)e.C * 3 * (e.nt + 1) * e.n;
    if (out_sum) DQ_HIP(hipMemcpy(out_sum, e.ut.meas_sum.get(), sizeof(double) * cnt, hipMemcpyDeviceToHost));
    if (n_measurements) *n_measurements = e.ut_meas_count;
    if (reset) { DQ_HIP(hipMemset(e.ut.meas_sum.get(), 0, sizeof(double) * cnt)); e.ut_meas_count = 0; }
    return 0;
}
int dqmc_measure_equal_time(dqmc_engine* h, int L1, int L2, double* scalars, double* chi_r) {
    ENGINE_CALL(h);
    if (L1 < 1 || L2 < 1 || L1 * L2 != e.n) { set_error("measure_equal_time: L1*L2 must equal n_sites"); return DQMC_EINVAL; }
    DQ_TRY(launch_measure_equal_time(CMat(e.G.get(), e.nn), e.meas_now.get(), 3 + e.n, L1, L2, 0, e.C, e.s));
    DQ_TRY(e.sync_and_check());
    return e.copy_out_equal_time(e.meas_now.get(), scalars, chi_r);
}
int dqmc_measure_accumulate(dqmc_engine* h, int L1, int L2) {
    ENGINE_CALL(h);
    if (L1 < 1 || L2 < 1 || L1 * L2 != e.n) { set_error("measure_accumulate: L1*L2 must equal n_sites"); return DQMC_EINVAL; }
    DQ_TRY(launch_measure_equal_time(CMat(e.G.get(), e.nn), e.meas_sum.get(), 3 + e.n, L1, L2, 1, e.C, e.s)); // asynchronous, in stream order after the sweep
    ++e.meas_count;
    return 0;
}
int dqmc_measure_fetch(dqmc_engine* h, double* scalars_sum, double* chi_r_sum, int64_t* n_measurements, int reset) {
    ENGINE_CALL(h); DQ_TRY(e.sync_and_check());
    DQ_TRY(e.copy_out_equal_time(e.meas_sum.get(), scalars_sum, chi_r_sum));
    if (n_measurements) *n_measurements = e.meas_count;
    if (reset) { DQ_HIP(hipMemset(e.meas_sum.get(), 0, sizeof(double) * e.C * (3 + e.n))); e.meas_count = 0; }
    return 0;
}
int dqmc_update_kernel_time(dqmc_engine* h, double* ms, int64_t* n_launches, int64_t* n_accepted) {
    ENGINE_CALL(h); DQ_TRY(e.sync_and_check());
    std::vector<DevStats> st(e.C);
    DQ_HIP(hipMemcpy(st.data(), e.dstats.get(), sizeof(DevStats) * e.C, hipMemcpyDeviceToHost));
    long long acc = 0; for (auto& x : st) acc += x.n_accepted;
    if (ms) *ms = e.upd_ms; if (n_launches) *n_launches = e.upd_launches; if (n_accepted) *n_accepted = acc - e.upd_accept_base;
    e.upd_ms = 0.0; e.upd_launches = 0; e.upd_accept_base = acc;
    return 0;
}
// diagnostic: 1 when the next local update of this engine takes a persistent single-launch slice kernel (Engine::slice_path), 0 for
// the kernel pairs and the solo kernel
int dqmc_debug_snapshot(dqmc_engine* h, double* wrap_err, int* accepted, unsigned int* sync_words, unsigned int* slice_epoch) {
    ENGINE_CALL(h);
    DQ_HIP(hipStreamSynchronize(e.s));
    if (wrap_err) DQ_HIP(hipMemcpy(wrap_err, e.err.get(), sizeof(double) * e.n_stack, hipMemcpyDeviceToHost));
    if (accepted) DQ_HIP(hipMemcpy(accepted, e.acc.get(), sizeof(int) * e.nt, hipMemcpyDeviceToHost));
    if (sync_words) DQ_HIP(hipMemcpy(sync_words, e.slice_sync.get(), sizeof(unsigned int) * 80, hipMemcpyDeviceToHost));
    if (slice_epoch) *slice_epoch = e.slice_epoch;
    return 0;
}
int dqmc_bbar_rider_launches(dqmc_engine* h, int64_t* n_launches) {
    ENGINE_CALL(h);
    if (n_launches) *n_launches = e.rider_launches;
    return 0;
}
int dqmc_debug_gt_check(dqmc_engine* h, int on, double* max_err, int64_t* n_checks) {
    ENGINE_CALL(h); DQ_TRY(e.sync_and_check());
    if (!e.gt_err) { DQ_TRY(dev_alloc(e.gt_err, e.C)); DQ_HIP(hipMemset(e.gt_err.get(), 0, sizeof(double) * e.C)); }
    if (max_err) DQ_HIP(hipMemcpy(max_err, e.gt_err.get(), sizeof(double) * e.C, hipMemcpyDeviceToHost));
    if (n_checks) *n_checks = e.gt_checks;
    DQ_HIP(hipMemset(e.gt_err.get(), 0, sizeof(double) * e.C));
    e.gt_checks = 0; e.gt_check = on != 0;
    return 0;
}
int dqmc_slice_path(dqmc_engine* h) {
    if (!h) return -1;
    Engine& e = h->e;
    if (!is_persistent(e.slice_path)) return 0;
    // 2: at least one launch of the persistent kernel fell back to the solo walk (a flush workgroup had not become resident in time)
    unsigned solo = 0;
    for (int c = 0; c < e.C && !solo; ++c) {
        SliceSync hs; if (hipMemcpy(&hs, e.slice_sync.get() + (size_t)c * SLICE_SYNC_BYTES, 64, hipMemcpyDeviceToHost) != hipSuccess) break;
        solo = hs.solo_count;
    }
    return solo ? 2 : 1;
}
int dqmc_set_profiling(dqmc_engine* h, int on) {
    ENGINE_CALL(h); DQ_TRY(e.sync_and_check());
    e.profiling = on != 0; return 0;
}

}  // extern "C"
