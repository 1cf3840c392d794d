#!/bin/bash
# diagnostic builds with s_memtime stamps (never used for timing results): libraries under scripts/stamp_build/, read by
# scripts/sm_stamps.py (update kernels), scripts/qr_stamps.py (column-owner QRCP) and scripts/gj_stamps.py (Gauss-Jordan panel / fused step)
set -e
cd "$(dirname "$0")/.."
mkdir -p scripts/stamp_build
# STAMP_K=<k>: the panel the QR / Gauss-Jordan stamp builds print (default 0), e.g. STAMP_K=192 for a compacted panel at n = 256
F="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -DDQ_QP_STAMP_K=${STAMP_K:-0} -DDQ_GJ_STAMP_K0=${STAMP_K:-0}"
L="-L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib"
/opt/rocm/bin/hipcc $F -DDQ_SCAN_STAMPS -c dqmc_amd/csrc/update.hip -o scripts/stamp_build/update.o
/opt/rocm/bin/hipcc $F -DDQ_SM_STAMPS -c dqmc_amd/csrc/update_sm.hip -o scripts/stamp_build/update_sm.o
/opt/rocm/bin/hipcc $F -DDQ_QR_STAMPS -c dqmc_amd/csrc/qr_colown.hip -o scripts/stamp_build/qr_colown.o
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o scripts/stamp_build/libdqmc_hip_scan.so $(ls dqmc_amd/csrc/*.o | grep -v "csrc/update.o") scripts/stamp_build/update.o $L
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o scripts/stamp_build/libdqmc_hip_sm.so $(ls dqmc_amd/csrc/*.o | grep -v "csrc/update_sm.o") scripts/stamp_build/update_sm.o $L
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o scripts/stamp_build/libdqmc_hip_qr.so $(ls dqmc_amd/csrc/*.o | grep -v "csrc/qr_colown.o") scripts/stamp_build/qr_colown.o $L
/opt/rocm/bin/hipcc $F -DDQ_GJ_STAMPS -c dqmc_amd/csrc/lu_gj.hip -o scripts/stamp_build/lu_gj.o
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o scripts/stamp_build/libdqmc_hip_gjst.so $(ls dqmc_amd/csrc/*.o | grep -v "csrc/lu_gj.o") scripts/stamp_build/lu_gj.o $L
/opt/rocm/bin/hipcc $F -DDQ_QP_STAMPS -c dqmc_amd/csrc/qr_panel.hip -o scripts/stamp_build/qr_panel.o
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o scripts/stamp_build/libdqmc_hip_qpst.so $(ls dqmc_amd/csrc/*.o | grep -v "csrc/qr_panel.o") scripts/stamp_build/qr_panel.o $L
