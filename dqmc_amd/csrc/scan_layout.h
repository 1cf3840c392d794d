// scan_layout.h -- the LDS layout of the Metropolis walk kernels (update.hip: ScanShared), stated once.
// Plain C++: host code (and tests/uw_bank_model.cpp) include it without the HIP runtime.
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define DQ_LAYOUT_FN __host__ __device__ constexpr
#else
#define DQ_LAYOUT_FN constexpr
#endif

namespace dq {

constexpr int UPDATE_KD = 32;    // delayed-update window (accepted flips per flush)

// Row pitch of the pending-pair store UW[kd][pitch] in double2 (16-byte) units: the smallest value >= n that is 1 (mod 16).
// Per accepted flip lane r of every 16-lane row reads the pivot's entry of pair r (and of pair 16 + r): UW[r * pitch + i], a
// ds_read_b128.  The LDS serves that instruction in four groups of 16 lanes, each of which holds all 16 values of r, and the bank of
// byte address a is (a / 4) mod 64.  With pitch = n (a multiple of 16 at every lattice the walk is used on) the rows are 4 n dwords
// = 0 (mod 64) apart: the D distinct rows of a group meet on the same four banks and the read takes 4 D LDS cycles.  With
// pitch = 1 (mod 16) consecutive rows start 4 dwords apart (mod 64): sixteen rows cover the 64 banks exactly once, 4 cycles for
// every k and every pivot site (tests/test_uw_pitch.py checks both statements on a model of the lane groups).
DQ_LAYOUT_FN int uw_pitch(int n) { return ((n + 14) / 16) * 16 + 1; }

// bytes of dynamic LDS: UW[kd][uw_pitch(n)] | diag, dlt, rbv, ur [n] | tables[32] | site[n] | newf[n] (padded) | (register variant) diag2[n] | acc_site[KD] | 4 spare words (verdicts of the persistent kernel's wave 0)
DQ_LAYOUT_FN size_t scan_lds_bytes(int n, int kd, bool regs) {
    return ((((size_t)16 * kd * uw_pitch(n) + (size_t)n * 32 + 256 + (size_t)n * 4 + (size_t)n) + 63) & ~(size_t)63)
           + (regs ? (size_t)n * 8 + 4 * (UPDATE_KD + 4) : 0);
}

// window depth at n sites.  LDS budget: 16*kd*n + n*(5*8+4+1) + tables <= ~150 KiB (stated on the unpadded rows, as it was before
// the pitch: the depth sets the rounding order of the rank-1 sums, so it stays what it was; the padding adds at most 16*15*kd =
// 7.5 KiB, which SCAN_LDS_LIMIT still holds -- checked for every n by tests/test_uw_pitch.py)
DQ_LAYOUT_FN int pick_kd(int n) {
    const long budget = 150 * 1024 - (long)n * 48 - 1024;
    const long kd = budget / (16L * n);
    return kd > UPDATE_KD ? UPDATE_KD : kd < 1 ? 1 : (int)kd;
}

constexpr size_t SCAN_LDS_LIMIT = 160 * 1024;    // the dynamic LDS the walk kernels are allowed (update_init_device): a CU's whole LDS

}  // namespace dq
