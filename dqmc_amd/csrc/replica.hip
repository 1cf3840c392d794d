// replica.hip -- replica exchange (parallel tempering) between the chains of engines, one rank per GPU:
// update::partner_rank / update::replica_exchange (source/update.cpp:34-117) and the MPI_Barrier / MPI_Reduce of the
// reference's driver (source/main.cpp:148,186-187) behind the C ABI of include/dqmc_hip.h.  A batched engine with C chains
// stands for C consecutive replicas; pairs inside it swap on the device (exchange_trial_kernel / exchange_restore_kernel),
// pairs that cross to another rank use the transport below.
//
// The reference's four messages per round (MPI_Sendrecv of the field array, two MPI_Sendrecv of one double, one
// MPI_Send/MPI_Recv of the decision) become point-to-point operations of a dqmc_comm:
//   rccl       grouped ncclSend / ncclRecv on the engine's stream, HBM to HBM (the field array never visits the host:
//              fields live in HBM as int8 [nt][n], 51 kB at cfg 4); the two actions travel as ONE message of two
//              doubles; pairs are disjoint, so on 8 GPUs a round is 4 concurrent single-link xGMI transfers.
//   callbacks  an MPI_Sendrecv-shaped host function supplied by the caller (MPI, or the in-process hub of
//              dqmc_host.hpp for replicas that are threads of one process); fields are staged through the host.
// The expensive part of a round is not the wire but the one or two from-scratch re-initialisations
// (init_stacks + init_greenfunctions, source/update.cpp:75-80,109-115), which run on the engine as dqmc_init does.
#include "common.h"
#include "../../include/dqmc_hip.h"

#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

using namespace dq;

struct dqmc_comm {
    int rank = 0, world = 1, device = 0;
    bool rccl = false;
    ncclComm_t nc = nullptr;
    hipStream_t stream = nullptr;            // collectives of the driver (barrier, allreduce); p2p of a round uses the engine's stream
    DevPtr<double> dbuf;                     // device scratch: 8 doubles (send 0..3, recv 4..7)
    dqmc_sendrecv_fn fn = nullptr; void* user = nullptr;
    std::vector<int8_t> h_send, h_recv;      // callback transport staging
};

#define DQ_NCCL(call)                                                                   \
    do {                                                                                \
        ncclResult_t _r = (call);                                                       \
        if (_r != ncclSuccess) {                                                        \
            ::dq::set_error(std::string(#call) + ": " + ncclGetErrorString(_r));        \
            return DQMC_ENODEVICE;                                                      \
        }                                                                               \
    } while (0)

static int have_device() {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) { set_error("no HIP device available: this library requires a gfx950 GPU"); return DQMC_ENODEVICE; }
    return 0;
}

// pairwise exchange of device buffers on `s`
static int p2p(dqmc_comm* c, const void* send, void* recv, size_t bytes, int partner, int tag, hipStream_t s) {
    if (c->rccl && !c->nc) { set_error("communicator aborted after an earlier wire error: destroy it and create a new one"); return DQMC_EINVAL; }
    if (c->rccl) {
        DQ_NCCL(ncclGroupStart());
        DQ_NCCL(ncclSend(send, bytes, ncclInt8, partner, c->nc, s));
        DQ_NCCL(ncclRecv(recv, bytes, ncclInt8, partner, c->nc, s));
        DQ_NCCL(ncclGroupEnd());
        return 0;
    }
    c->h_send.resize(bytes); c->h_recv.resize(bytes);
    DQ_HIP(hipMemcpyAsync(c->h_send.data(), send, bytes, hipMemcpyDeviceToHost, s));
    DQ_HIP(hipStreamSynchronize(s));
    if (c->fn(c->user, c->h_send.data(), c->h_recv.data(), bytes, partner, tag) != 0) { set_error("replica exchange: the sendrecv callback failed"); return DQMC_EINVAL; }
    DQ_HIP(hipMemcpyAsync(recv, c->h_recv.data(), bytes, hipMemcpyHostToDevice, s));
    DQ_HIP(hipStreamSynchronize(s));
    return 0;
}
// pairwise exchange of a few doubles held on the host
static int p2p_host(dqmc_comm* c, const double* send, double* recv, int count, int partner, int tag, hipStream_t s) {
    if (!c->rccl) {
        if (c->fn(c->user, send, recv, sizeof(double) * count, partner, tag) != 0) { set_error("replica exchange: the sendrecv callback failed"); return DQMC_EINVAL; }
        return 0;
    }
    DQ_HIP(hipMemcpyAsync(c->dbuf.get(), send, sizeof(double) * count, hipMemcpyHostToDevice, s));
    DQ_TRY(p2p(c, c->dbuf.get(), c->dbuf.get() + 4, sizeof(double) * count, partner, tag, s));
    DQ_HIP(hipMemcpyAsync(recv, c->dbuf.get() + 4, sizeof(double) * count, hipMemcpyDeviceToHost, s));
    DQ_HIP(hipStreamSynchronize(s));
    return 0;
}

// ---- the field moves of a round, on the engine's stream ----
// desc[c]: the chain in this engine that chain c swaps with (>= 0), -1 - s: chain c takes the configuration received into slot s of
// `recv` (its partner lives on another rank), XCHG_NONE: no partner this attempt.  Every pair is disjoint, so the lower chain of an
// in-engine pair swaps both chains element by element in place, and no element is read after another block wrote it.
constexpr int XCHG_NONE = -(1 << 30);

template <class T>
__global__ void exchange_trial_kernel(T* fields, T* saved, const T* recv, const int* desc, long words) {
    const int c = blockIdx.y, d = desc[c];
    if (d == XCHG_NONE || (d >= 0 && d < c)) return;
    T* f = fields + (long)c * words; T* sv = saved + (long)c * words;
    if (d >= 0) {
        T* fp = fields + (long)d * words; T* sp = saved + (long)d * words;
        for (long k = blockIdx.x * (long)blockDim.x + threadIdx.x; k < words; k += (long)gridDim.x * blockDim.x) {
            const T a = f[k], b = fp[k];
            sv[k] = a; sp[k] = b; f[k] = b; fp[k] = a;
        }
    } else {
        const T* r = recv + (long)(-1 - d) * words;
        for (long k = blockIdx.x * (long)blockDim.x + threadIdx.x; k < words; k += (long)gridDim.x * blockDim.x) { sv[k] = f[k]; f[k] = r[k]; }
    }
}
// chains of a rejected pair take their own configuration back (source/update.cpp:108-111)
template <class T>
__global__ void exchange_restore_kernel(T* fields, const T* saved, const int* desc, const int* accepted, long words) {
    const int c = blockIdx.y;
    if (desc[c] == XCHG_NONE || accepted[c]) return;
    T* f = fields + (long)c * words; const T* sv = saved + (long)c * words;
    for (long k = blockIdx.x * (long)blockDim.x + threadIdx.x; k < words; k += (long)gridDim.x * blockDim.x) f[k] = sv[k];
}

template <class T>
static int launch_exchange_as(bool restore, int8_t* fields, int8_t* saved, const int8_t* recv, const int* tab, size_t bytes, int chains, hipStream_t s) {
    const long words = (long)(bytes / sizeof(T));
    const dim3 grid((unsigned)std::min<long>((words + 255) / 256, 64), (unsigned)chains);
    if (restore) hipLaunchKernelGGL(exchange_restore_kernel<T>, grid, dim3(256), 0, s, (T*)fields, (const T*)saved, tab, tab + chains, words);
    else hipLaunchKernelGGL(exchange_trial_kernel<T>, grid, dim3(256), 0, s, (T*)fields, (T*)saved, (const T*)recv, tab, words);
    DQ_HIP(hipGetLastError());
    return 0;
}
// tab = [desc[C]][accepted[C]] on the device; a chain's configuration is `bytes` int8 ([nt][n]), moved 16 bytes at a time when it can be
static int launch_exchange(bool restore, int8_t* fields, int8_t* saved, const int8_t* recv, const int* tab, size_t bytes, int chains, hipStream_t s) {
    if (bytes % 16 == 0) return launch_exchange_as<uint4>(restore, fields, saved, recv, tab, bytes, chains, s);
    return launch_exchange_as<uint8_t>(restore, fields, saved, recv, tab, bytes, chains, s);
}

// One round of update::replica_exchange (source/update.cpp:47-117) for every chain of `e`: chain k of rank r is replica r*C + k of a
// world of W = ranks * C.  Pairs inside the engine are decided here from dqmc_global_action; a pair that crosses to another rank (at
// most chains 0 and C - 1) runs the single-chain protocol of the reference over `c`: tag 0 the fields, tag 1 {S', S, status}, tag 3
// the decision (that every rank holds the same C is settled before, dqmc_replica_exchange_batch).  The boundary pairs of every phase
// are taken in the order of their lower global index on every rank, so blocking pairwise exchanges cannot wait in a cycle
// (the pair with the smallest index still open always has both ends at it).
static int exchange_round(dqmc_engine* e, dqmc_comm* c, int exchange_attempt, const double* u, dqmc_exchange_result* res) {
    EngineFieldsView v;
    DQ_TRY(engine_fields_view(e, &v));
    const int C = v.n_chains;
    if (c && c->rccl && c->device != v.device) { set_error("replica exchange: the communicator and the engine are on different devices"); return DQMC_EINVAL; }
    const int rank = c ? c->rank : 0, world = (c ? c->world : 1) * C;
    struct Boundary { int chain, partner_rank, slot; };
    std::vector<int> desc((size_t)2 * C, XCHG_NONE);                           // [desc[C]][accepted[C]], uploaded as tab
    std::vector<Boundary> edge;
    for (int k = 0; k < C; ++k) {
        const int g = rank * C + k, pg = dqmc_partner_rank(g, world, exchange_attempt);
        desc[C + k] = 1;
        if (pg < 0 || pg >= world || pg == g) continue;                           // source/update.cpp:55-57
        res[k].partner = pg; res[k].decider = g < pg ? 1 : 0;
        if (pg / C == rank) desc[k] = pg % C;
        else edge.push_back(Boundary{k, pg / C, 0});
    }
    std::sort(edge.begin(), edge.end(), [&](const Boundary& a, const Boundary& b) {
        return std::min(rank * C + a.chain, res[a.chain].partner) < std::min(rank * C + b.chain, res[b.chain].partner);
    });
    if (edge.size() > 2) { set_error("replica exchange: more than two pairs leave the engine"); return DQMC_EINVAL; }
    for (size_t b = 0; b < edge.size(); ++b) { edge[b].slot = (int)b; desc[edge[b].chain] = -1 - (int)b; }
    bool any = false;
    for (int k = 0; k < C; ++k) any = any || res[k].partner >= 0;
    if (!any) return 0;
    DQ_HIP(hipSetDevice(v.device));
    if (c && c->rccl && !c->dbuf) { set_error("replica exchange: communicator has no device scratch"); return DQMC_EINVAL; }
    const size_t bytes = (size_t)v.nt * v.n;
    int8_t* saved = nullptr; int8_t* recv = nullptr; int* tab = nullptr;
    DQ_TRY(engine_exchange_scratch(e, &saved, &recv, &tab));
    hipStream_t s = v.stream;
    // the device tables are uploaded from `desc` on the engine's stream; every return waits for the stream first, so no copy is still
    // reading `desc` when it goes away
    struct StreamDrain { hipStream_t s; ~StreamDrain() { (void)hipStreamSynchronize(s); } } drain{s};
    // A step that fails on THIS rank (a breakdown in dqmc_init on the trial fields, say) must not leave a partner blocked in its
    // next receive: local failures are remembered, the remaining messages are still exchanged and carry a status word, every pair of
    // the engine is treated as rejected (own fields restored) and the round returns an error on both ends of a boundary pair.  A
    // failure of the transport itself ends the round at once; on the RCCL transport the communicator is aborted so that the peer's
    // pending receive returns.
    int lrc = 0; std::string lmsg;
    auto local = [&](int rc) { if (rc != 0 && lrc == 0) { lrc = rc; lmsg = dqmc_last_error(); } return rc; };
    auto wire = [&](int rc) {
        if (rc != 0 && c->rccl && c->nc) { (void)ncclCommAbort(c->nc); c->nc = nullptr; }
        return rc;
    };
    DQ_TRY(dqmc_sync(e));                                                       // the sweep that precedes the round has finished
    // --- the fields of the boundary partners (MPI_Sendrecv tag 0, source/update.cpp:59-69) ---
    for (const Boundary& b : edge)
        DQ_TRY(wire(p2p(c, v.fields + (size_t)b.chain * bytes, recv + (size_t)b.slot * bytes, bytes, b.partner_rank, 0, s)));
    // --- S_r({s}_r), then the trial state on the partner's fields: S_r({s}_partner) (:72-81) ---
    std::vector<double> S((size_t)C, 0.0), Sp((size_t)C, 0.0);
    local(dqmc_global_action(e, S.data()));                                        // synchronises: the received fields have landed
    DQ_HIP(hipMemcpyAsync(tab, desc.data(), sizeof(int) * 2 * C, hipMemcpyHostToDevice, s));
    DQ_TRY(launch_exchange(false, v.fields, saved, recv, tab, bytes, C, s));
    if (local(engine_fields_changed(e)) == 0 && local(dqmc_init(e)) == 0) local(dqmc_global_action(e, Sp.data()));
    for (int k = 0; k < C; ++k) {
        res[k].S = S[k]; res[k].S_prime = Sp[k];
        if (desc[k] >= 0) { res[k].S_partner = S[desc[k]]; res[k].S_prime_partner = Sp[desc[k]]; }
    }
    // --- the cross actions (tags 1 and 2 of the reference, :83-90) and this rank's status, one message of three doubles ---
    std::vector<char> broken((size_t)C, lrc != 0 ? 1 : 0);
    bool partner_failed = false;
    for (const Boundary& b : edge) {
        dqmc_exchange_result& r = res[b.chain];
        const double mine[3] = {r.S_prime, r.S, lrc ? 1.0 : 0.0};
        double theirs[3] = {0.0, 0.0, 0.0};
        DQ_TRY(wire(p2p_host(c, mine, theirs, 3, b.partner_rank, 1, s)));
        r.S_prime_partner = theirs[0]; r.S_partner = theirs[1];
        if (theirs[2] != 0.0) { broken[b.chain] = 1; partner_failed = true; }
    }
    // --- decision by the lower global index (:92-105): rng.bernoulli(p) of the decider, include/utility.h:34-37 ---
    for (int k = 0; k < C; ++k) {
        dqmc_exchange_result& r = res[k];
        if (r.partner < 0) continue;
        r.deltaS = (r.S_prime + r.S_prime_partner) - (r.S + r.S_partner);         // the decider's is the one that counts
        if (r.decider) r.accepted = (!broken[k] && u[k] < std::fmin(1.0, std::exp(-r.deltaS))) ? 1 : 0;
    }
    for (int k = 0; k < C; ++k)
        if (desc[k] >= 0 && !res[k].decider) res[k].accepted = res[desc[k]].accepted;
    for (const Boundary& b : edge) {
        dqmc_exchange_result& r = res[b.chain];
        const double flag_mine = r.decider && r.accepted ? 1.0 : 0.0;
        double flag_theirs = 0.0;
        DQ_TRY(wire(p2p_host(c, &flag_mine, &flag_theirs, 1, b.partner_rank, 3, s)));
        if (!r.decider) r.accepted = (!broken[b.chain] && flag_theirs != 0.0) ? 1 : 0;
    }
    // --- rejected: restore the own fields and re-initialise (:108-115); one init covers every chain ---
    bool any_rejected = false;
    for (int k = 0; k < C; ++k) {
        desc[C + k] = res[k].partner < 0 || res[k].accepted ? 1 : 0;
        any_rejected = any_rejected || !desc[C + k];
    }
    if (any_rejected) {
        DQ_HIP(hipMemcpyAsync(tab + C, desc.data() + C, sizeof(int) * C, hipMemcpyHostToDevice, s));
        DQ_TRY(launch_exchange(true, v.fields, saved, recv, tab, bytes, C, s));
        DQ_TRY(engine_fields_changed(e));
        DQ_TRY(dqmc_init(e));
    }
    if (lrc != 0) { set_error("replica exchange: " + lmsg + " (round treated as rejected on both ranks, own fields restored)"); return lrc; }
    if (partner_failed) { set_error("replica exchange: the partner rank reported a failure during the round (treated as rejected, own fields restored)"); return DQMC_ENUMERIC; }
    return 0;
}

extern "C" {

int dqmc_partner_rank(int rank, int world_size, int exchange_attempt) {       // source/update.cpp:34-45
    const bool even_attempt = (exchange_attempt % 2 == 0);
    const int off = even_attempt ? ((rank % 2 == 0) ? 1 : -1) : ((rank % 2 == 0) ? -1 : 1);
    return (rank + off + world_size) % world_size;
}

int dqmc_comm_unique_id(void* id) {
    if (!id) { set_error("null id"); return DQMC_EINVAL; }
    DQ_TRY(have_device());
    static_assert(sizeof(ncclUniqueId) == DQMC_UNIQUE_ID_BYTES, "unique id size");
    ncclUniqueId u;
    DQ_NCCL(ncclGetUniqueId(&u));
    std::memcpy(id, &u, sizeof(u));
    return 0;
}

int dqmc_comm_create_rccl(dqmc_comm** out, const void* id, int world_size, int rank, int device) {
    if (!out || !id || world_size < 1 || rank < 0 || rank >= world_size) { set_error("bad argument"); return DQMC_EINVAL; }
    DQ_TRY(have_device());
    int count = 0; DQ_HIP(hipGetDeviceCount(&count));
    if (device < 0 || device >= count) { set_error("device ordinal out of range"); return DQMC_EINVAL; }
    DQ_HIP(hipSetDevice(device));
    dqmc_comm* c = new (std::nothrow) dqmc_comm;
    if (!c) return DQMC_ENOMEM;
    c->rank = rank; c->world = world_size; c->device = device; c->rccl = true;
    ncclUniqueId u; std::memcpy(&u, id, sizeof(u));
    ncclResult_t r = ncclCommInitRank(&c->nc, world_size, u, rank);
    if (r != ncclSuccess) { set_error(std::string("ncclCommInitRank: ") + ncclGetErrorString(r)); delete c; return DQMC_ENODEVICE; }
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess || dev_alloc(c->dbuf, 8) != 0) {
        set_error("dqmc_comm_create_rccl: stream / scratch allocation failed"); dqmc_comm_destroy(c); return DQMC_ENODEVICE;
    }
    *out = c; return 0;
}

int dqmc_comm_create_callbacks(dqmc_comm** out, int world_size, int rank, dqmc_sendrecv_fn fn, void* user) {
    if (!out || !fn || world_size < 1 || rank < 0 || rank >= world_size) { set_error("bad argument"); return DQMC_EINVAL; }
    dqmc_comm* c = new (std::nothrow) dqmc_comm;
    if (!c) return DQMC_ENOMEM;
    c->rank = rank; c->world = world_size; c->rccl = false; c->fn = fn; c->user = user; c->device = -1;
    *out = c; return 0;
}

void dqmc_comm_destroy(dqmc_comm* c) {
    if (!c) return;
    if (c->device >= 0) (void)hipSetDevice(c->device);
    if (c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
    if (c->nc) (void)ncclCommDestroy(c->nc);
    delete c;                                // frees dbuf
}
int dqmc_comm_rank(dqmc_comm* c) { return c ? c->rank : -1; }
int dqmc_comm_world_size(dqmc_comm* c) { return c ? c->world : 0; }
const char* dqmc_comm_transport(dqmc_comm* c) { return !c ? "" : c->rccl ? "rccl" : "callbacks"; }

int dqmc_comm_allreduce_sum(dqmc_comm* c, double* x, int count) {
    if (!c || !x || count < 1 || count > 4) { set_error("allreduce_sum: 1..4 doubles"); return DQMC_EINVAL; }
    if (c->world == 1) return 0;
    if (c->rccl && !c->nc) { set_error("communicator aborted after an earlier wire error: destroy it and create a new one"); return DQMC_EINVAL; }
    if (c->rccl) {
        DQ_HIP(hipSetDevice(c->device));
        DQ_HIP(hipMemcpyAsync(c->dbuf.get(), x, sizeof(double) * count, hipMemcpyHostToDevice, c->stream));
        DQ_NCCL(ncclAllReduce(c->dbuf.get(), c->dbuf.get() + 4, count, ncclDouble, ncclSum, c->nc, c->stream));
        DQ_HIP(hipMemcpyAsync(x, c->dbuf.get() + 4, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream));
        DQ_HIP(hipStreamSynchronize(c->stream));
        return 0;
    }
    // callbacks: rank 0 collects (pairwise exchanges in rank order), then hands the sums back -- O(world) tiny messages
    double mine[4], got[4];
    std::memcpy(mine, x, sizeof(double) * count);
    if (c->rank == 0) {
        for (int r = 1; r < c->world; ++r) {
            if (c->fn(c->user, mine, got, sizeof(double) * count, r, 4) != 0) { set_error("allreduce: the sendrecv callback failed"); return DQMC_EINVAL; }
            for (int k = 0; k < count; ++k) x[k] += got[k];
        }
        for (int r = 1; r < c->world; ++r)
            if (c->fn(c->user, x, got, sizeof(double) * count, r, 5) != 0) { set_error("allreduce: the sendrecv callback failed"); return DQMC_EINVAL; }
    } else {
        if (c->fn(c->user, mine, got, sizeof(double) * count, 0, 4) != 0 || c->fn(c->user, mine, got, sizeof(double) * count, 0, 5) != 0) {
            set_error("allreduce: the sendrecv callback failed"); return DQMC_EINVAL;
        }
        std::memcpy(x, got, sizeof(double) * count);
    }
    return 0;
}
// Loop-back check of a communicator's transport: the rank exchanges a pattern with ITSELF through the same grouped
// send / receive path a round uses (ncclSend + ncclRecv to the own rank, or the callback), and, on RCCL, runs one
// ncclAllReduce; the only way to exercise the RCCL code path on a machine with a single GPU.
int dqmc_comm_selftest(dqmc_comm* c) {
    if (!c) { set_error("comm_selftest: null communicator"); return DQMC_EINVAL; }
    if (!c->rccl) { set_error("comm_selftest: RCCL transport only (a callback transport is checked by calling the callback)"); return DQMC_EINVAL; }
    if (!c->nc) { set_error("communicator aborted after an earlier wire error: destroy it and create a new one"); return DQMC_EINVAL; }
    DQ_HIP(hipSetDevice(c->device));
    const size_t bytes = 4096;
    DevPtr<int8_t> a, b;
    DQ_TRY(dev_alloc(a, bytes)); DQ_TRY(dev_alloc(b, bytes));
    std::vector<int8_t> h(bytes), g(bytes, 0);
    for (size_t k = 0; k < bytes; ++k) h[k] = (int8_t)((k * 7 + c->rank) & 3);
    if (hipMemcpyAsync(a.get(), h.data(), bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess || hipMemsetAsync(b.get(), 0, bytes, c->stream) != hipSuccess) { set_error("comm_selftest: copy failed"); return DQMC_ENODEVICE; }
    DQ_TRY(p2p(c, a.get(), b.get(), bytes, c->rank, 0, c->stream));
    if (hipMemcpyAsync(g.data(), b.get(), bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) { set_error("comm_selftest: copy back failed"); return DQMC_ENODEVICE; }
    if (std::memcmp(h.data(), g.data(), bytes) != 0) { set_error("comm_selftest: loop-back data mismatch"); return DQMC_ENUMERIC; }
    const double x[2] = {1.5 + c->rank, -2.0}; double y[2] = {0.0, 0.0};
    DQ_TRY(p2p_host(c, x, y, 2, c->rank, 1, c->stream));
    if (y[0] != x[0] || y[1] != x[1]) { set_error("comm_selftest: loop-back of two doubles mismatch"); return DQMC_ENUMERIC; }
    double z[2] = {1.0, (double)c->rank};
    if (hipMemcpyAsync(c->dbuf.get(), z, sizeof(z), hipMemcpyHostToDevice, c->stream) != hipSuccess) { set_error("comm_selftest: copy failed"); return DQMC_ENODEVICE; }
    ncclResult_t r = ncclAllReduce(c->dbuf.get(), c->dbuf.get() + 4, 2, ncclDouble, ncclSum, c->nc, c->stream);
    if (r != ncclSuccess) { set_error(std::string("comm_selftest: ncclAllReduce: ") + ncclGetErrorString(r)); return DQMC_ENODEVICE; }
    if (hipMemcpyAsync(z, c->dbuf.get() + 4, sizeof(z), hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) { set_error("comm_selftest: copy back failed"); return DQMC_ENODEVICE; }
    const double want1 = 0.5 * c->world * (c->world - 1);
    if (z[0] != (double)c->world || z[1] != want1) { set_error("comm_selftest: all-reduce result mismatch"); return DQMC_ENUMERIC; }
    return 0;
}
int dqmc_comm_barrier(dqmc_comm* c) { double z = 0.0; return dqmc_comm_allreduce_sum(c, &z, 1); }

int dqmc_replica_exchange_round(dqmc_engine* e, dqmc_comm* c, int exchange_attempt, double u, dqmc_exchange_result* res) {
    if (!e || !c || !res) { set_error("replica exchange: null argument"); return DQMC_EINVAL; }
    std::memset(res, 0, sizeof(*res));
    res->partner = -1;
    EngineFieldsView v;
    DQ_TRY(engine_fields_view(e, &v));
    if (v.n_chains != 1) { set_error("replica exchange: one chain per rank (a batched engine holds several: dqmc_replica_exchange_batch)"); return DQMC_EINVAL; }
    return exchange_round(e, c, exchange_attempt, &u, res);
}

int dqmc_replica_exchange_batch(dqmc_engine* e, dqmc_comm* c, int exchange_attempt, const double* u, dqmc_exchange_result* res) {
    // Argument errors are found locally; with a communicator the ranks then agree on them in one all-reduce before anything moves,
    // so that a rank that refuses (or holds another number of chains, which would give it another pairing) cannot leave the others
    // blocked in a receive.  Every rank adds {C, C^2, bytes, bytes^2}: the shapes are all equal iff sum^2 = ranks * sum of squares
    // (small integers, exact in doubles); a refusing rank adds {-1, 1, 0, 0}, which no valid shape matches.
    std::string bad;
    EngineFieldsView v{};
    if (!e || !res) bad = "null engine or result array";
    else {
        DQ_TRY(engine_fields_view(e, &v));
        for (int k = 0; k < v.n_chains; ++k) { std::memset(res + k, 0, sizeof(*res)); res[k].partner = -1; }
        if (!u) bad = "null uniform array u";
        else if (!c && v.n_chains == 1) bad = "a single chain without a communicator has nobody to swap with";
        else if (c && c->rccl && c->device != v.device) bad = "the communicator and the engine are on different devices";
    }
    if (c && c->world > 1) {
        const double C = bad.empty() ? v.n_chains : -1.0, b = bad.empty() ? (double)v.nt * v.n : 0.0;
        double x[4] = {C, C * C, b, b * b};
        DQ_TRY(dqmc_comm_allreduce_sum(c, x, 4));
        const double R = c->world;
        if (bad.empty() && (x[0] * x[0] != R * x[1] || x[2] * x[2] != R * x[3]))
            bad = "every rank must hold the same number of chains of the same size (another rank differs, or refused its arguments)";
    }
    if (!bad.empty()) { set_error("replica exchange: " + bad); return DQMC_EINVAL; }
    const long world = (long)(c ? c->world : 1) * v.n_chains;
    if (world % 2 != 0) {                                                         // source/main.cpp:58-62
        set_error("replica exchange: the number of replicas (" + std::to_string(world) + " = ranks x chains) needs to be even");
        return DQMC_EINVAL;
    }
    return exchange_round(e, c, exchange_attempt, u, res);
}

}  // extern "C"
