// muse_comm.cpp -- exchange of the per-sim accumulators between ranks (collectives C1-C3 of SURVEY.md §2).
//
// The reference gathers map results to the master process through Distributed.pmap
// (src/util.jl:74-83) and reduces them there (src/muse.jl:183,188,446,529).  Here every rank owns a
// contiguous block of sims on its own GPU and the per-rank score blocks / H accumulators are
// exchanged once per map.  Messages are <= 64 KB, so the cost is latency, not bandwidth.  Two transports:
// RCCL collectives over xGMI (any topology), and -- for the ranks of one node, whose hosts are the consumers
// of the blocks -- a shared-memory segment (shm_gather.hpp) that needs no collective kernel at all.
// Each is a Comm with its own state behind the same few operations; the extern "C" entry points validate and dispatch.
//
// librccl is opened lazily (dlopen) so that libmuse_hip.so loads on hosts without a usable RCCL.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/muse_hip.h"
#include "comm_handoff.h"
#include "host_loop.h"
#include "shm_gather.hpp"
#include "switches.hpp"

// Minimal slice of the public RCCL/NCCL C API (rccl.h: ncclGetUniqueId, ncclCommInitRank,
// ncclAllGather, ncclAllReduce, ncclCommDestroy).
typedef struct ncclComm* ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId;
typedef int ncclResult_t;
enum { ncclFloat64 = 8 };
enum { ncclSum = 0 };

// accessors implemented in muse_engine.cpp (the context layout is private to that file)
extern "C" {
int muse_ctx_comm_slot(muse_ctx* ctx, void*** comm, int* device, void** stream, int* ntheta);
int muse_ctx_comm_buffer(muse_ctx* ctx, size_t doubles, double** buf);
int muse_internal_map_async(muse_ctx* ctx, uint64_t seed, int64_t sim_begin, int64_t sim_end, int include_data, int nmaps,
                            const double* thetas, double atol, int z0_mode, int area, int64_t map_stride, double* scores_dev);
int muse_ctx_set_comm_reserve(muse_ctx* ctx, int cus);
int muse_ctx_switches(muse_ctx* ctx, const muse::Switches** sw, int* debug);
int muse_wait_event(void* event);
int muse_internal_loop_usable(muse_ctx* ctx, int nsims, int64_t nlocal);
int muse_internal_run_loop_shard(muse_ctx* ctx, uint64_t seed, const double* theta0, const muse_run_options* o, int64_t sim_lo, int64_t sim_hi,
                                 int include_data, void* board_dev, void* const* peer_boards, int npeers, unsigned int tag_base,
                                 int32_t* niter_out, double* theta_out, double* hist_out, double* gsims_out, muse_info* info_out);
}
namespace muse {   // muse_kernels.hip
hipError_t launch_board_handshake(unsigned long long* own, unsigned long long* const* store, int nstore, int nranks, int rank, unsigned int tag,
                                  unsigned long long slot0, unsigned long long ticks, unsigned int* result, hipStream_t st);
}

namespace {
struct Rccl {
    void* h = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;  // optional
    ncclResult_t (*AllGather)(const void*, void*, size_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
Rccl g_rccl;

bool load_rccl() {
    if (g_rccl.h) return true;
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return false;
    g_rccl.GetUniqueId = (decltype(g_rccl.GetUniqueId))dlsym(h, "ncclGetUniqueId");
    g_rccl.CommInitRank = (decltype(g_rccl.CommInitRank))dlsym(h, "ncclCommInitRank");
    g_rccl.CommDestroy = (decltype(g_rccl.CommDestroy))dlsym(h, "ncclCommDestroy");
    g_rccl.CommCount = (decltype(g_rccl.CommCount))dlsym(h, "ncclCommCount");
    g_rccl.AllGather = (decltype(g_rccl.AllGather))dlsym(h, "ncclAllGather");
    g_rccl.AllReduce = (decltype(g_rccl.AllReduce))dlsym(h, "ncclAllReduce");
    g_rccl.GetErrorString = (decltype(g_rccl.GetErrorString))dlsym(h, "ncclGetErrorString");
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.CommDestroy || !g_rccl.AllGather || !g_rccl.AllReduce)
        return false;
    g_rccl.h = h;
    return true;
}

// return-on-failure checks of the three kinds of call made here: error code + message (muse_last_error)
std::string rccl_str(ncclResult_t r) { return g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?"; }
int rccl_error(const char* what, ncclResult_t r) { return muse_set_error(MUSE_ERR_RCCL, (std::string(what) + ": " + rccl_str(r)).c_str()); }
int hip_error(const char* what, hipError_t e) { return muse_set_error(MUSE_ERR_HIP, (std::string(what) + ": " + hipGetErrorString(e)).c_str()); }
int shm_error(int w, const char* what) {   // (muse_shm::Gather's waits: 2 the abort word was raised, 1 timed out)
    return muse_set_error(MUSE_ERR_RCCL, (std::string("shared-memory transport: ") + (w == 2 ? "a peer rank failed (" : "timed out waiting for the peers (") + what + ")").c_str());
}
#define RCCLCHK(expr) do { const ncclResult_t r_ = (expr); if (r_ != 0) return rccl_error(#expr, r_); } while (0)
#define HIPCHK2(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) return hip_error(#expr, e_); } while (0)
#define SHMCHK(expr, what) do { const int w_ = (expr); if (w_ != 0) return shm_error(w_, what); } while (0)

constexpr int kAreas = 4;        // result areas of the engine (muse_hip.h: result_area in [0, 4))
constexpr int kRunHostLoop = 1;  // Comm::run_device_loop: nothing has run, the host-driven loop is to run the job

// A gathered map as the entry point received it: the solver launch of this rank's elements, whose scores go into this
// rank's block [nmaps][rows_per_rank][ntheta] of the exchange.
struct GatherMap {
    uint64_t seed;
    int64_t sim_begin, sim_end;
    int include_data, nmaps;
    const double* thetas;
    double atol;
    int z0_mode;
    int64_t rows_per_rank;
    int ntheta;
    size_t count() const { return (size_t)nmaps * (size_t)rows_per_rank * (size_t)ntheta; }   // doubles per rank
    int64_t elements() const { return (sim_end - sim_begin) + (include_data ? 1 : 0); }
    int launch(muse_ctx* ctx, int area, double* scores_dev) const {   // (scores_dev NULL: to the area's pinned block)
        return muse_internal_map_async(ctx, seed, sim_begin, sim_end, include_data, nmaps, thetas, atol, z0_mode, area, rows_per_rank, scores_dev);
    }
};

// Rank r's share of the S simulations of a sharded muse! loop (distributed.py: the first S mod nranks ranks get one more):
// simulations [lo, hi), and `count` elements with the data element, which lives on rank 0.
struct Share { int64_t lo, hi, count; };
Share share_of(int S, int nranks, int r) {
    const int64_t base = S / nranks, extra = S % nranks, lo = (int64_t)r * base + (r < extra ? r : extra), hi = lo + base + (r < extra ? 1 : 0);
    return {lo, hi, (hi - lo) + (r == 0 ? 1 : 0)};
}

// One per context/rank: what the two transports share, and the operations each of them implements.  `stream` is lane 0's
// (the solver's) stream at the time of the call.
struct Comm {
    muse_ctx* const ctx;
    const int nranks, rank, device;
    const muse::Switches* const sw;  // the context's environment switches (switches.hpp: read once, by muse_ctx_create)
    Comm(muse_ctx* c, int n, int r, int dev, const muse::Switches* s) : ctx(c), nranks(n), rank(r), device(dev), sw(s) {}
    virtual ~Comm() {}
    virtual int transport() const = 0;
    virtual int ranks_seen(int* nranks_out) = 0;
    // synchronous, host to host: all-gather into recv [nranks][count], or (sum) the sum over the ranks, which may go back over `send`
    virtual int collective(hipStream_t stream, const double* send, size_t count, double* recv, bool sum) = 0;
    virtual int start(hipStream_t stream, int area, const GatherMap& m) = 0;   // the solver launch (and the hand-over of its gather)
    virtual int wait(int area, double* g_all_out, muse_info* info_out) = 0;    // every rank's block has landed
    virtual void close() = 0;                                                  // tear-down (the caller deletes)
    // The score boards of the sharded device loop exist on the shared-memory transport only.
    virtual void board_status(hipStream_t, int status_out[6], double wait_us_out[2]) {
        const int none[6] = {MUSE_BOARD_NONE, -1, -1, 0, 0, MUSE_BOARD_NONE};
        memcpy(status_out, none, sizeof none);
        wait_us_out[0] = wait_us_out[1] = 0.0;
    }
    // this rank's share of a muse! run as ONE persistent launch: MUSE_OK (done), kRunHostLoop, or an error
    virtual int run_device_loop(hipStream_t, uint64_t, const double*, const muse_run_options*, const Share&, int, int32_t*, double*, double*,
                                double*, muse_info*) {
        return kRunHostLoop;
    }
};

// ---- RCCL ------------------------------------------------------------------------------------------------------------
// The communicator, a stream of its own for the collectives (so that the all-gather of batch k overlaps the solver launch
// of batch k+1), and per result area the device send/receive buffers plus a pinned host landing block.
struct RcclComm : Comm {
    using Comm::Comm;
    struct Area {
        double *send_dev = nullptr, *recv_dev = nullptr, *recv_pin = nullptr;
        size_t cap = 0, count = 0;   // doubles per rank: of the buffers, of the gather in flight
        hipEvent_t kdone = nullptr;  // solver launch of the area finished (recorded on the solver stream)
        hipEvent_t gdone = nullptr;  // gathered block landed in recv_pin (recorded on cstream)
        bool pending = false;
    } area[kAreas];
    ncclComm_t comm = nullptr;
    hipStream_t cstream = nullptr;
    bool own_stream = true, direct_host = false;
    // The collective of a gathered map is enqueued by a worker thread of the communicator: the caller's thread returns
    // as soon as the solver is launched (measured on the host: solver launch 7.5 us; stream-wait + ncclAllGather +
    // event 14-18 us -- in one thread the N > 1 step was host-bound at ~25 us of enqueueing against a 22 us solver).
    // One communicator, one collective stream: a gather occupies that stream for 35-40 us (one rank), which is what
    // bounds a strongly scaled step; duplicates of the communicator (ncclCommSplit) on streams of their own, one per
    // result area, were measured to make everything worse (collective kernels of several steps resident at once take
    // the CUs the cluster solver needs: 85 us per step against 37).
    std::thread worker;
    muse::AreaHandoff<kAreas> handoff;   // caller -> worker: the areas whose gather is to be enqueued
    std::mutex mu;                       // serialises every use of `comm` (RCCL: one thread at a time) and the worker's error
    int worker_rc = 0;                   // first error of the worker (reported by wait)
    std::string worker_err;

    int transport() const override { return MUSE_TRANSPORT_RCCL; }
    int ranks_seen(int* nranks_out) override {
        if (!g_rccl.CommCount) return muse_set_error(MUSE_ERR_RCCL, "librccl has no ncclCommCount");
        std::lock_guard<std::mutex> lk(mu);
        RCCLCHK(g_rccl.CommCount(comm, nranks_out));
        return MUSE_OK;
    }
    int collective(hipStream_t st, const double* send, size_t count, double* recv, bool sum) override {
        double* buf;   // device: [count] to send, and behind it [nranks][count] of an all-gather
        const int rc = muse_ctx_comm_buffer(ctx, sum ? count : count * (size_t)(nranks + 1), &buf);
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(mu);
        HIPCHK2(hipMemcpyAsync(buf, send, count * sizeof(double), hipMemcpyHostToDevice, st));
        if (sum) RCCLCHK(g_rccl.AllReduce(buf, buf, count, ncclFloat64, ncclSum, comm, st));
        else RCCLCHK(g_rccl.AllGather(buf, buf + count, count, ncclFloat64, comm, st));
        HIPCHK2(hipMemcpyAsync(recv, sum ? buf : buf + count, (sum ? count : count * nranks) * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK2(hipStreamSynchronize(st));
        return MUSE_OK;
    }
    int open(const void* id, hipStream_t stream) {
        HIPCHK2(hipSetDevice(device));
        ncclUniqueId uid;
        memcpy(&uid, id, MUSE_UNIQUE_ID_BYTES);
        RCCLCHK(g_rccl.CommInitRank(&comm, nranks, uid, rank));
        if (sw && sw->comm_one_stream) cstream = stream;  // tuning aid: collectives in line with the solver
        else {
            // Highest priority: the persistent solver kernel fills every CU (LDS- and VGPR-bound, nothing can
            // co-reside), so a collective can only be dispatched in the gap between two solver launches -- with
            // default priority it loses that race to the next solver launch (measured: 86 vs 73 us per step).
            int lo = 0, hi = 0;
            HIPCHK2(hipDeviceGetStreamPriorityRange(&lo, &hi));
            HIPCHK2(hipStreamCreateWithPriority(&cstream, hipStreamNonBlocking, hi));
        }
        direct_host = sw && sw->comm_direct_host;
        own_stream = cstream != stream;
        for (Area& a : area) {
            HIPCHK2(hipEventCreateWithFlags(&a.kdone, hipEventDisableTiming));
            HIPCHK2(hipEventCreateWithFlags(&a.gdone, hipEventDisableTiming));
        }
        worker = std::thread([this] { work(); });
        muse_ctx_set_comm_reserve(ctx, 16);  // the all-gather kernel of step k runs beside the (cluster) solver launch of step k+1
        return MUSE_OK;
    }
    void close() override {
        hipSetDevice(device);
        muse_ctx_set_comm_reserve(ctx, 0);
        handoff.stop();
        if (worker.joinable()) worker.join();
        if (cstream) hipStreamSynchronize(cstream);
        if (comm && g_rccl.h) g_rccl.CommDestroy(comm);
        for (Area& a : area) {
            hipFree(a.send_dev); hipFree(a.recv_dev); hipHostFree(a.recv_pin);
            if (a.kdone) hipEventDestroy(a.kdone);
            if (a.gdone) hipEventDestroy(a.gdone);
        }
        if (cstream && own_stream) hipStreamDestroy(cstream);
    }

    // The worker: waits for an area, then  collective stream <- wait(solver done) ; all-gather ; copy ; record(gdone).
    void work() {
        (void)hipSetDevice(device);
        for (int ai; handoff.take(ai); handoff.enqueued(ai)) enqueue_gather(area[ai]);
    }
    void enqueue_gather(Area& a) {
        const size_t cnt = a.count;
        std::lock_guard<std::mutex> lk(mu);  // RCCL calls on one communicator must not overlap
        hipError_t e = hipStreamWaitEvent(cstream, a.kdone, 0);
        ncclResult_t r = 0;
        if (e == hipSuccess) {
            if (direct_host) {
                // the collective's receive buffer IS the pinned host block (device-mapped): no copy operation follows
                r = g_rccl.AllGather(a.send_dev, a.recv_pin, cnt, ncclFloat64, comm, cstream);
            } else {
                r = g_rccl.AllGather(a.send_dev, a.recv_dev, cnt, ncclFloat64, comm, cstream);
                if (r == 0) e = hipMemcpyAsync(a.recv_pin, a.recv_dev, cnt * nranks * sizeof(double), hipMemcpyDeviceToHost, cstream);
            }
        }
        if (e == hipSuccess && r == 0) e = hipEventRecord(a.gdone, cstream);
        if ((e != hipSuccess || r != 0) && worker_rc == 0) {
            worker_rc = r != 0 ? MUSE_ERR_RCCL : MUSE_ERR_HIP;
            worker_err = r != 0 ? "ncclAllGather: " + rccl_str(r) : std::string("collective stream: ") + hipGetErrorString(e);
        }
    }

    // ---- sharded map: solver launch + device-side all-gather, pipelined over the result areas ------------
    int ensure_gather_buffers(Area& a, size_t doubles_per_rank) {
        if (doubles_per_rank <= a.cap) return MUSE_OK;
        HIPCHK2(hipStreamSynchronize(cstream));
        hipFree(a.send_dev); hipFree(a.recv_dev); hipHostFree(a.recv_pin);
        a.send_dev = a.recv_dev = a.recv_pin = nullptr;
        a.cap = 0;
        const size_t cap = doubles_per_rank + doubles_per_rank / 2 + 16;
        if (hipMalloc(&a.send_dev, cap * sizeof(double)) != hipSuccess || hipMalloc(&a.recv_dev, cap * nranks * sizeof(double)) != hipSuccess)
            return muse_set_error(MUSE_ERR_ALLOC, "hipMalloc(gather buffers) failed");
        HIPCHK2(hipHostMalloc(&a.recv_pin, cap * nranks * sizeof(double), hipHostMallocDefault));
        a.cap = cap;
        return MUSE_OK;
    }
    int start(hipStream_t ks, int ai, const GatherMap& m) override {
        Area& a = area[ai];
        if (a.pending) return muse_set_error(MUSE_ERR_INVALID, "a gather is still in flight on this result area");
        int rc = ensure_gather_buffers(a, m.count());
        if (rc) return rc;
        // (the area's previous gather has been awaited -- pending is clear -- so its send buffer is free again)
        if (m.elements() < m.rows_per_rank)  // padding rows of a short block are zeros
            HIPCHK2(hipMemsetAsync(a.send_dev, 0, m.count() * sizeof(double), ks));
        rc = m.launch(ctx, ai, a.send_dev);
        if (rc) return rc;
        HIPCHK2(hipEventRecord(a.kdone, ks));
        a.count = m.count();
        a.pending = true;
        handoff.post(ai);   // hand the collective to the worker
        return MUSE_OK;
    }
    int wait(int ai, double* g_all_out, muse_info* info_out) override {
        Area& a = area[ai];
        if (!a.pending) return muse_set_error(MUSE_ERR_INVALID, "no gather in flight on this result area");
        {   // the worker is microseconds behind; bounded all the same (a worker that has died must not hang the caller)
            const double t0 = muse_shm::now_s();
            unsigned spins = 0;
            while (!handoff.is_enqueued(ai)) {
                MUSE_CPU_RELAX();
                if ((++spins & 0xfff) == 0 && muse_shm::now_s() - t0 > 30.0) {
                    a.pending = false;
                    return muse_set_error(MUSE_ERR_RCCL, "the communicator's worker thread did not enqueue the gather within 30 s");
                }
            }
        }
        a.pending = false;
        {
            std::lock_guard<std::mutex> lk(mu);
            if (worker_rc) {
                const int wrc = worker_rc;
                worker_rc = 0;
                return muse_set_error(wrc, worker_err.c_str());
            }
        }
        const int rc = muse_wait_event(a.gdone);
        if (rc) return rc;
        if (g_all_out) memcpy(g_all_out, a.recv_pin, a.count * nranks * sizeof(double));
        return muse_batch_wait(ctx, ai, nullptr, info_out);  // the solver's own completion, error flag, local infos
    }
};

// ---- shared memory ---------------------------------------------------------------------------------------------------
// The id of a shared-memory communicator: magic | capacity per block | segment name.
struct ShmId {
    uint64_t magic;
    uint64_t block_doubles;
    char name[MUSE_UNIQUE_ID_BYTES - 16];
};
static_assert(sizeof(ShmId) == MUSE_UNIQUE_ID_BYTES, "the id travels in the same 128 bytes as RCCL's");
constexpr size_t kShmDefaultBlock = 16384;
constexpr size_t kBoardBytes = 256 * 1024;   // the score board: 32 768 granules -- (nsims + 1) * ntheta <= 16 384
constexpr size_t kBoardHandshakeBytes = 4096;   // behind them: the set-up hand-shake's slots (a granule pair per rank, up to 64 ranks)
constexpr size_t kBoardTotalBytes = kBoardBytes + kBoardHandshakeBytes;
constexpr unsigned long long kBoardHandshakeSlot = kBoardBytes / sizeof(unsigned long long);

// The set-up hand-shake of one board kind (ShmComm::prove_board; muse_comm_board_status).
struct BoardCheck {
    int handshake = -1;             // 1 every rank saw every peer, 0 some rank did not, -1 not tried
    unsigned long long seen = 0;    // the ranks THIS rank saw
    double wait_us = 0.0;           // how long its hand-shake kernel polled
    const char* verdict() const { return handshake == 1 ? "ok" : handshake == 0 ? "FAILED" : "not tried"; }
};

struct ShmComm : Comm {
    using Comm::Comm;
    muse_shm::Gather* shm = nullptr;   // areas 0..kAreas-1: the gathered maps; area kAreas: the synchronous collectives
    struct Area {
        uint64_t seq = 0;    // sequence number of the area's last exchange (the same on every rank)
        size_t count = 0;    // doubles per rank of the gather in flight: [nmaps][rows_per_rank][ntheta]
        size_t nlocal = 0;   // doubles this rank's solver produced PER MAP for it
        int nmaps = 1;
        bool pending = false;
    } area[kAreas];
    uint64_t coll_seq = 0;   // ... and of the last synchronous collective
    // The node's score board of the sharded DEVICE loop (muse_run_sharded): a region of the shared segment that this process
    // has registered with the HIP runtime, so that its GPU reads and writes it in place.  Every rank's workers store their
    // scores there as tagged granules; every rank's stepper polls all of them.  No host is in the loop between two maps.
    unsigned long long* board_dev = nullptr;   // this GPU's pointer to it (null: not available -- the host loop runs)
    void* board_host = nullptr;
    unsigned int board_tag = 0;      // the last tag used (the same on every rank: every rank makes the same calls)
    // ... and, where the runtime allows it, a board per GPU in DEVICE memory instead: every rank allocates one and maps every peer's
    // (hipIpcGetMemHandle / hipIpcOpenMemHandle, the handles exchanged through the segment); a worker's score is stored into every
    // rank's board -- posted writes, over xGMI between GPUs -- and a stepper polls its OWN GPU's memory: no PCIe round trip in the
    // iteration.  A collective decision at init (every rank must have opened every handle); the host board otherwise.
    unsigned long long* ipc_own = nullptr;
    void* ipc_peers[8] = {nullptr};   // [rank]: the peer's board as mapped here (own: ipc_own)
    bool ipc_ok = false, boards_tried = false;
    BoardCheck dev_boards, host_board;
    unsigned int* hs_result = nullptr;   // pinned: the hand-shake kernel's {mask lo, mask hi, ticks}
    int last_loop = MUSE_BOARD_NONE;     // what the last muse_run_sharded call ran
    bool dev_loop_off = false;       // the device loop failed once on some rank (a shared GPU): host loop from then on, on every rank

    int transport() const override { return MUSE_TRANSPORT_SHM; }
    int ranks_seen(int* nranks_out) override { *nranks_out = shm->attached(); return MUSE_OK; }
    // Over the segment's last area, in pieces of at most one block; the sum over ranks is taken in rank order.
    int collective(hipStream_t, const double* send, size_t count, double* recv, bool sum) override {
        muse_shm::Gather& g = *shm;
        const size_t B = g.block_doubles;
        for (size_t off = 0; off < count; off += B) {
            const size_t m = count - off < B ? count - off : B;
            const uint64_t s = ++coll_seq;
            SHMCHK(g.wait_consumed(kAreas, s - 1), "collective: previous piece");
            memcpy(g.block(kAreas, rank), send + off, m * sizeof(double));
            g.publish_ready(kAreas, s);
            SHMCHK(g.wait_ready(kAreas, s), "collective");
            if (sum) {
                for (size_t i = 0; i < m; ++i) {
                    double acc = g.block(kAreas, 0)[i];
                    for (int q = 1; q < nranks; ++q) acc += g.block(kAreas, q)[i];
                    recv[off + i] = acc;
                }
            } else {
                for (int q = 0; q < nranks; ++q) memcpy(recv + (size_t)q * count + off, g.block(kAreas, q), m * sizeof(double));
            }
            g.publish_consumed(kAreas, s);
        }
        return MUSE_OK;
    }
    // a yes/no vote: the number of ranks that said yes (0 if the exchange itself failed; `rc_out` tells)
    double vote(bool yes, int* rc_out = nullptr) {
        double flag[1] = {yes ? 1.0 : 0.0};
        const int rc = collective(nullptr, flag, 1, flag, true);
        if (rc_out) *rc_out = rc;
        return rc == MUSE_OK ? flag[0] : 0.0;
    }

    int start(hipStream_t, int ai, const GatherMap& m) override {
        Area& a = area[ai];
        if (a.pending) return muse_set_error(MUSE_ERR_INVALID, "a gather is still in flight on this result area");
        // the plain launch (scores to this area's pinned block); the exchange happens in wait
        if (m.count() > shm->block_doubles)
            return muse_set_error(MUSE_ERR_INVALID, "nmaps * rows_per_rank * ntheta exceeds the block capacity the communicator's id was "
                                                    "created with (muse_comm_unique_id_ex: block_doubles)");
        const int rc = m.launch(ctx, ai, nullptr);
        if (rc) return rc;
        a.count = m.count();
        a.nlocal = (size_t)m.elements() * m.ntheta;
        a.nmaps = m.nmaps;
        a.seq += 1;
        a.pending = true;
        return MUSE_OK;
    }
    int wait(int ai, double* g_all_out, muse_info* info_out) override {
        Area& a = area[ai];
        if (!a.pending) return muse_set_error(MUSE_ERR_INVALID, "no gather in flight on this result area");
        muse_shm::Gather& g = *shm;
        a.pending = false;
        // every rank has copied this rank's previous block of the area out (true at once in a pipelined loop)
        SHMCHK(g.wait_consumed(ai, a.seq - 1), "gathered map: previous block");
        double* mine = g.block(ai, rank);
        const int rc = muse_batch_wait(ctx, ai, mine, info_out);  // solver's completion, error flag; scores -> my block
        if (rc) {
            g.raise_abort();  // the peers must not wait a minute for a block that will not come
            return rc;
        }
        {   // padding rows of a short block (after every map's own rows) are zeros
            const size_t per_map = a.count / (size_t)a.nmaps;
            if (a.nlocal < per_map)
                for (int m = 0; m < a.nmaps; ++m) memset(mine + (size_t)m * per_map + a.nlocal, 0, (per_map - a.nlocal) * sizeof(double));
        }
        g.publish_ready(ai, a.seq);
        SHMCHK(g.wait_ready(ai, a.seq), "gathered map");
        if (g_all_out)
            for (int q = 0; q < nranks; ++q) memcpy(g_all_out + (size_t)q * a.count, g.block(ai, q), a.count * sizeof(double));
        g.publish_consumed(ai, a.seq);
        return MUSE_OK;
    }

    void close() override {
        if (board_host || ipc_own || hs_result) {
            hipSetDevice(device);
            (void)hipDeviceSynchronize();   // (nothing of this process may still be polling the board)
        }
        if (board_host) (void)hipHostUnregister(board_host);
        if (hs_result) (void)hipHostFree(hs_result);
        if (ipc_ok) {
            // (every rank closes its views before anyone frees: one more exchange; a peer that is gone already just times out)
            for (int q = 0; q < nranks; ++q)
                if (q != rank && ipc_peers[q]) (void)hipIpcCloseMemHandle(ipc_peers[q]);
            const double keep = shm->timeout_s;
            shm->timeout_s = keep < 5.0 ? keep : 5.0;
            (void)vote(true);
            shm->timeout_s = keep;
            (void)hipFree(ipc_own);
            (void)hipGetLastError();
        }
        delete shm;
    }

    // One hand-shake over a board kind (collective): this rank's one-wavefront kernel stores its tagged pair into `store[0..nstore)` and
    // polls `own` for every rank's pair (muse_kernels.hip: board_handshake_kernel), bounded by the switch handshake_ms (default 50 ms);
    // then the ranks tell each other whether they saw everybody.
    BoardCheck prove_board(hipStream_t stream, unsigned long long* own, unsigned long long* const* store, int nstore, unsigned int tag) {
        const double bound_ms = sw && sw->handshake_ms > 0 ? sw->handshake_ms : 50.0;
        const unsigned long long ticks = (unsigned long long)(bound_ms * 1e5);   // s_memrealtime: 100 MHz
        bool ok = hs_result != nullptr;
        if (ok) {
            hs_result[0] = hs_result[1] = hs_result[2] = 0;
            // (the ranks leave the collective before this within microseconds of each other; the launch itself is a few more)
            ok = muse::launch_board_handshake(own, store, nstore, nranks, rank, tag, kBoardHandshakeSlot, ticks, hs_result, stream) == hipSuccess &&
                 hipStreamSynchronize(stream) == hipSuccess;
            (void)hipGetLastError();
        }
        BoardCheck b;
        b.seen = ok ? ((unsigned long long)hs_result[1] << 32) | hs_result[0] : 0ull;
        b.wait_us = ok ? (double)hs_result[2] * 0.01 : 0.0;
        const unsigned long long full = nranks >= 64 ? ~0ull : ((1ull << nranks) - 1ull);
        b.handshake = vote(ok && b.seen == full) == (double)nranks ? 1 : 0;
        return b;
    }

    // The score boards of the sharded device loop, set up ONCE per communicator -- by muse_comm_board_status or by the first
    // muse_run_sharded call, collective over the segment either way: the one in pinned host memory -- the segment's extra region, mapped
    // into this GPU's address space where the runtime allows it -- and a board per GPU in device memory, every rank's mapped into every
    // rank (ipc_*).  Each kind is then PROVED by a hand-shake (prove_board) before the loop may use it: a store into
    // another GPU's board that its poll never sees costs milliseconds here, not a bounded wait inside the first user call.
    void setup_boards(hipStream_t stream) {
        if (boards_tried) return;
        boards_tried = true;
        muse_shm::Gather* g = shm;
        const muse::Switches none;
        const muse::Switches& s = sw ? *sw : none;
        if (hipSetDevice(device) == hipSuccess && !hs_result && hipHostMalloc(&hs_result, 64, hipHostMallocDefault) != hipSuccess) hs_result = nullptr;
        (void)hipGetLastError();
        if (!s.no_board && g->extra() && g->extra_bytes() >= kBoardTotalBytes && nranks <= 64 &&
            hipHostRegister(g->extra(), g->extra_bytes(), hipHostRegisterMapped | hipHostRegisterPortable) == hipSuccess) {
            void* dp = nullptr;
            if (hipHostGetDevicePointer(&dp, g->extra(), 0) == hipSuccess && dp) {
                board_host = g->extra();
                board_dev = (unsigned long long*)dp;
            } else {
                (void)hipHostUnregister(g->extra());
            }
        }
        (void)hipGetLastError();
        ipc_ok = false;
        dev_boards = host_board = BoardCheck();
        if (nranks <= 8) {
            bool ok = !s.no_ipc_board && !s.no_board && hipSetDevice(device) == hipSuccess;
            hipIpcMemHandle_t mine;
            memset(&mine, 0, sizeof mine);
            if (ok) {
                void* p = nullptr;
                // The board is written by OTHER GPUs and polled by this one: uncached, or fine-grained, device memory.  Plain hipMalloc
                // memory is coarse-grained and cached in this GPU's L2 -- a poll of it is not guaranteed ever to see a peer's store -- so
                // without either kind there is no device board (every rank then uses the host board).
                if (hipExtMallocWithFlags(&p, kBoardTotalBytes, hipDeviceMallocUncached) != hipSuccess) {
                    (void)hipGetLastError();
                    p = nullptr;
                    if (hipExtMallocWithFlags(&p, kBoardTotalBytes, hipDeviceMallocFinegrained) != hipSuccess) {
                        (void)hipGetLastError();
                        p = nullptr;
                    }
                }
                ok = p != nullptr && hipMemset(p, 0, kBoardTotalBytes) == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
                     hipIpcGetMemHandle(&mine, p) == hipSuccess;
                ipc_own = (unsigned long long*)p;
            }
            (void)hipGetLastError();
            // every rank's {ok, handle}: 1 + 8 doubles per rank (the 64 handle bytes travel as 8 doubles' bit patterns)
            static_assert(sizeof(hipIpcMemHandle_t) == 64, "handle exchanged as 8 doubles");
            double send[9], recv[9 * 8];
            send[0] = ok ? 1.0 : 0.0;
            memcpy(send + 1, &mine, 64);
            if (collective(nullptr, send, 9, recv, false) != MUSE_OK) ok = false;
            bool all = ok;
            for (int q = 0; q < nranks && all; ++q) all = recv[9 * q] == 1.0;
            if (all) {
                for (int q = 0; q < nranks; ++q) {
                    if (q == rank) { ipc_peers[q] = ipc_own; continue; }
                    hipIpcMemHandle_t h;
                    memcpy(&h, recv + 9 * q + 1, 64);
                    void* pp = nullptr;
                    if (hipIpcOpenMemHandle(&pp, h, hipIpcMemLazyEnablePeerAccess) != hipSuccess || !pp) { all = false; (void)hipGetLastError(); break; }
                    ipc_peers[q] = pp;
                }
            }
            ipc_ok = vote(all) == (double)nranks;   // did EVERY rank open EVERY handle
            if (ipc_ok) {   // mapped everywhere: now prove that a store into a peer's board is SEEN by the peer's poll
                unsigned long long* stores[8];
                // (test hook: the granules land 64 slots early -- inside the board, beside what the peer polls)
                const long miss = (s.handshake_fail & 1) ? -64 : 0;
                for (int q = 0; q < nranks; ++q) stores[q] = (unsigned long long*)ipc_peers[q] + miss;
                dev_boards = prove_board(stream, ipc_own, stores, nranks, 0x7ff00001u);
                ipc_ok = dev_boards.handshake == 1;
            }
            if (!ipc_ok) {
                for (int q = 0; q < nranks; ++q)
                    if (q != rank && ipc_peers[q]) { (void)hipIpcCloseMemHandle(ipc_peers[q]); }
                for (int q = 0; q < 8; ++q) ipc_peers[q] = nullptr;
                if (ipc_own) (void)hipFree(ipc_own);
                ipc_own = nullptr;
                (void)hipGetLastError();
            }
        }
        // the host board: every rank must have it mapped, and every rank's GPU must see every rank's stores through PCIe
        if (vote(board_dev != nullptr) == (double)nranks) {
            unsigned long long* stores[1] = {board_dev + ((s.handshake_fail & 2) ? -64 : 0)};
            host_board = prove_board(stream, board_dev, stores, 1, 0x7ff00002u);
        }
        if (host_board.handshake != 1 && board_host) {   // (a board some rank cannot use is no board: the loop is host-driven on every rank)
            (void)hipHostUnregister(board_host);
            (void)hipGetLastError();
            board_host = board_dev = nullptr;
        }
        if (s.run_timing)
            fprintf(stderr, "[muse_comm] rank %d of %d: board hand-shake -- device boards %s (saw 0x%llx, %.1f us), host board %s (saw 0x%llx, %.1f us)\n",
                    rank, nranks, dev_boards.verdict(), dev_boards.seen, dev_boards.wait_us, host_board.verdict(), host_board.seen, host_board.wait_us);
    }
    void board_status(hipStream_t stream, int status_out[6], double wait_us_out[2]) override {
        setup_boards(stream);   // collective: every rank is here (or in its first muse_run_sharded call)
        const int status[6] = {ipc_ok ? MUSE_BOARD_DEVICE : board_dev ? MUSE_BOARD_HOST : MUSE_BOARD_NONE, dev_boards.handshake, host_board.handshake,
                               (int)(dev_boards.seen & 0x7fffffffull), (int)(host_board.seen & 0x7fffffffull), last_loop};
        memcpy(status_out, status, sizeof status);
        wait_us_out[0] = dev_boards.wait_us;
        wait_us_out[1] = host_board.wait_us;
    }

    // The device loop: ONE persistent launch per rank runs every iteration; the ranks' scores meet on the node's board (pinned host
    // memory that every GPU maps, or the boards in device memory), every rank's stepper takes the same step from the same bits -- no
    // host between two maps.  Every rank must take the same loop: the decision is the minimum over the ranks of what each can do.
    int run_device_loop(hipStream_t stream, uint64_t seed, const double* theta0, const muse_run_options* o, const Share& mine, int nt,
                        int32_t* niter_out, double* theta_out, double* hist_out, double* gsims_out, muse_info* info_out) override {
        setup_boards(stream);   // (every rank makes its first call here together: collective; failure on any rank = the next board on all)
        int dbg = 0;
        (void)muse_ctx_switches(ctx, nullptr, &dbg);
        const bool sw_host_board = (sw && sw->host_board) || (dbg & muse::kDebugHostBoard);
        const bool sw_host_loop = (sw && sw->sharded_host_loop) || (dbg & muse::kDebugShardedHostLoop);
        const bool ipc = ipc_ok && !sw_host_board;   // (the same answer on every rank: every rank sets the same switches)
        // (count >= 1: with fewer simulations than ranks some rank owns no element -- its loop launch would be refused while its
        //  peers' ran: the minimum over the ranks sends such a job to the host-driven loop)
        const bool want = (ipc || board_dev) && !dev_loop_off && !sw_host_loop && mine.count >= 1 &&
                          (uint64_t)(o->nsims + 1) * (uint64_t)nt * 2 <= kBoardBytes / sizeof(unsigned long long) && board_tag < 0x70000000u &&
                          muse_internal_loop_usable(ctx, o->nsims, mine.count) != 0;
        int rc = MUSE_OK;
        const bool all_want = vote(want, &rc) == (double)nranks;
        if (rc) return rc;
        last_loop = !all_want ? MUSE_BOARD_NONE : ipc ? MUSE_BOARD_DEVICE : MUSE_BOARD_HOST;
        if ((sw && sw->run_timing) || (dbg & muse::kDebugRunTiming))   // tuning aid / tests: which loop, through which board
            fprintf(stderr, "[muse_run_sharded] rank %d of %d: %s\n", rank, nranks,
                    !all_want ? "host-driven loop" : ipc ? "persistent launch, boards in device memory (hipIpc)"
                                                         : "persistent launch, board in pinned host memory");
        if (!all_want) return kRunHostLoop;
        const unsigned int tag_base = board_tag;
        board_tag += (unsigned)o->maxsteps + 1;
        rc = muse_internal_run_loop_shard(ctx, seed, theta0, o, mine.lo, mine.hi, rank == 0 ? 1 : 0, ipc ? (void*)ipc_own : (void*)board_dev,
                                          ipc ? ipc_peers : nullptr, ipc ? nranks : 0, tag_base, niter_out, theta_out, hist_out, gsims_out,
                                          info_out);
        // a rank whose workgroups were not all resident (rc 1001) stalls every rank's stepper: all of them time out -- but
        // make the outcome a collective decision anyway; and a rank that FAILED (rc < 0: before or after its launch) takes every
        // rank out with an error -- its peers' steppers have waited for scores that never came
        double bad[1] = {(rc == 1001 ? 1.0 : 0.0) + (rc < 0 ? 1000.0 : 0.0)};
        const int rc2 = collective(nullptr, bad, 1, bad, true);
        if (rc < 0) return rc;
        if (rc2) return rc2;
        if (bad[0] >= 1000.0) {
            last_loop = MUSE_BOARD_NONE;
            return muse_set_error(MUSE_ERR_RCCL, "muse_run_sharded: a peer rank's share of the persistent loop failed (its own call reports why)");
        }
        if (bad[0] == 0.0) return MUSE_OK;
        last_loop = MUSE_BOARD_NONE;
        dev_loop_off = true;
        if (o->z0_warm)   // (the aborted attempt has touched the resident MAPs the run was to start from)
            return muse_set_error(MUSE_ERR_HIP, "muse_run_sharded: the workgroups of the loop kernel were not all resident at once on "
                                                "some rank; later calls run the host loop");
        return kRunHostLoop;   // ... a cold start is simply run again, by the host loop: the same bits
    }
};

// The way in from a context: its communicator slot and, if initialised (required unless `need` is false), the
// communicator; lane 0's stream; the device; the model's ntheta.
struct Way { Comm** slot = nullptr; Comm* comm = nullptr; hipStream_t stream = nullptr; int device = 0, ntheta = 0; };
int way_in(muse_ctx* ctx, Way& w, bool need = true) {
    const int rc = muse_ctx_comm_slot(ctx, (void***)&w.slot, &w.device, (void**)&w.stream, &w.ntheta);
    if (rc) return rc;
    w.comm = *w.slot;
    if (need && !w.comm) return muse_set_error(MUSE_ERR_INVALID, "muse_comm_init was not called");
    return MUSE_OK;
}
}  // namespace

extern "C" {

int muse_comm_unique_id(void* id_out) {
    if (!id_out) return muse_set_error(MUSE_ERR_INVALID, "id_out is NULL");
    if (!load_rccl()) return muse_set_error(MUSE_ERR_RCCL, "librccl could not be loaded");
    ncclUniqueId id;
    RCCLCHK(g_rccl.GetUniqueId(&id));
    memcpy(id_out, &id, MUSE_UNIQUE_ID_BYTES);
    return MUSE_OK;
}

int muse_comm_unique_id_ex(int transport, int64_t block_doubles, void* id_out) {
    if (transport == MUSE_TRANSPORT_RCCL) return muse_comm_unique_id(id_out);
    if (transport != MUSE_TRANSPORT_SHM) return muse_set_error(MUSE_ERR_INVALID, "unknown transport");
    if (!id_out || block_doubles < 0) return muse_set_error(MUSE_ERR_INVALID, "bad arguments");
    static std::atomic<unsigned> counter{0};
    ShmId id;
    memset(&id, 0, sizeof id);
    id.magic = muse_shm::kMagic;
    id.block_doubles = ((block_doubles ? (size_t)block_doubles : kShmDefaultBlock) + 7) & ~(size_t)7;  // whole cache lines
    timespec ts;
    clock_gettime(CLOCK_REALTIME, &ts);
    snprintf(id.name, sizeof id.name, "/muse_gather_%d_%llx_%u", (int)getpid(),
             (unsigned long long)ts.tv_sec * 1000000000ull + (unsigned long long)ts.tv_nsec, counter.fetch_add(1));
    memcpy(id_out, &id, MUSE_UNIQUE_ID_BYTES);
    return MUSE_OK;
}

int muse_comm_transport(muse_ctx* ctx, int* transport_out) {
    Way w;
    if (const int rc = way_in(ctx, w)) return rc;
    if (!transport_out) return muse_set_error(MUSE_ERR_INVALID, "transport_out is NULL");
    *transport_out = w.comm->transport();
    return MUSE_OK;
}

int muse_comm_ranks_seen(muse_ctx* ctx, int* nranks_out) {
    Way w;
    if (const int rc = way_in(ctx, w)) return rc;
    if (!nranks_out) return muse_set_error(MUSE_ERR_INVALID, "nranks_out is NULL");
    return w.comm->ranks_seen(nranks_out);
}

int muse_comm_board_status(muse_ctx* ctx, int status_out[6], double wait_us_out[2]) {
    Way w;
    if (const int rc = way_in(ctx, w)) return rc;
    if (!status_out || !wait_us_out) return muse_set_error(MUSE_ERR_INVALID, "NULL argument");
    w.comm->board_status(w.stream, status_out, wait_us_out);
    return MUSE_OK;
}

int muse_comm_init(muse_ctx* ctx, int nranks, int rank, const void* id) {
    Way w;
    if (const int rc = way_in(ctx, w, false)) return rc;
    if (!id || nranks < 1 || rank < 0 || rank >= nranks) return muse_set_error(MUSE_ERR_INVALID, "bad communicator arguments");
    if (w.comm) return muse_set_error(MUSE_ERR_INVALID, "communicator already initialised");
    const muse::Switches* sw = nullptr;
    (void)muse_ctx_switches(ctx, &sw, nullptr);
    ShmId sid;
    memcpy(&sid, id, sizeof sid);
    if (sid.magic == muse_shm::kMagic) {
        sid.name[sizeof sid.name - 1] = 0;
        muse_shm::Gather* g = new muse_shm::Gather();
        if (sw && sw->shm_timeout_s > 0) g->timeout_s = sw->shm_timeout_s;
        std::string err;
        if (!g->open(sid.name, nranks, rank, kAreas + 1, (size_t)sid.block_doubles, err, kBoardTotalBytes)) {
            delete g;
            return muse_set_error(MUSE_ERR_RCCL, ("shared-memory transport: " + err).c_str());
        }
        ShmComm* st = new ShmComm(ctx, nranks, rank, w.device, sw);
        st->shm = g;
        *w.slot = st;
        return MUSE_OK;   // (the score boards are set up by muse_comm_board_status or the first muse_run_sharded call: collective, and
                          //  nothing a communicator that only gathers maps has to go through)
    }
    if (!load_rccl()) return muse_set_error(MUSE_ERR_RCCL, "librccl could not be loaded");
    RcclComm* st = new RcclComm(ctx, nranks, rank, w.device, sw);
    const int rc = st->open(id, w.stream);
    if (rc) delete st;   // (the worker has not been started)
    else *w.slot = st;
    return rc;
}

int muse_comm_destroy(muse_ctx* ctx) {
    Way w;
    if (const int rc = way_in(ctx, w, false)) return rc;
    if (w.comm) {
        w.comm->close();
        delete w.comm;
    }
    *w.slot = nullptr;
    return MUSE_OK;
}

int muse_allgather_scores(muse_ctx* ctx, const double* send, int64_t count, double* recv_out) {
    Way w;
    if (const int rc = way_in(ctx, w)) return rc;
    if (!send || !recv_out || count < 0) return muse_set_error(MUSE_ERR_INVALID, "bad arguments");
    if (count == 0) return MUSE_OK;
    return w.comm->collective(w.stream, send, (size_t)count, recv_out, false);
}

int muse_allreduce_sum(muse_ctx* ctx, double* hostbuf, int64_t count) {
    Way w;
    if (const int rc = way_in(ctx, w)) return rc;
    if (!hostbuf || count < 0) return muse_set_error(MUSE_ERR_INVALID, "bad arguments");
    if (count == 0) return MUSE_OK;
    return w.comm->collective(w.stream, hostbuf, (size_t)count, hostbuf, true);
}

int muse_map_and_score_multi_gather_async(muse_ctx* ctx, uint64_t seed, int64_t sim_begin, int64_t sim_end,
                                          int include_data, int nmaps, const double* thetas, double atol, int z0_mode,
                                          int64_t rows_per_rank, int area) {
    Way w;
    if (const int rc = way_in(ctx, w)) return rc;
    if (area < 0 || area >= kAreas) return muse_set_error(MUSE_ERR_INVALID, "bad result_area");
    const GatherMap m = {seed, sim_begin, sim_end, include_data, nmaps, thetas, atol, z0_mode, rows_per_rank, w.ntheta};
    if (sim_end < sim_begin || rows_per_rank < m.elements() || rows_per_rank < 1)
        return muse_set_error(MUSE_ERR_INVALID, "rows_per_rank must be >= this rank's element count (and >= 1)");
    if (nmaps < 1) return muse_set_error(MUSE_ERR_INVALID, "nmaps must be >= 1");
    return w.comm->start(w.stream, area, m);
}

int muse_map_and_score_batch_gather_async(muse_ctx* ctx, uint64_t seed, int64_t sim_begin, int64_t sim_end,
                                          int include_data, const double* theta, double atol, int z0_mode,
                                          int64_t rows_per_rank, int area) {
    return muse_map_and_score_multi_gather_async(ctx, seed, sim_begin, sim_end, include_data, 1, theta, atol, z0_mode, rows_per_rank, area);
}

int muse_batch_wait_gathered(muse_ctx* ctx, int area, double* g_all_out, muse_info* info_out) {
    Way w;
    if (const int rc = way_in(ctx, w)) return rc;
    if (area < 0 || area >= kAreas) return muse_set_error(MUSE_ERR_INVALID, "bad result_area");
    return w.comm->wait(area, g_all_out, info_out);
}

// ---- the muse! outer loop over the ranks of a communicator (src/muse.jl:159-232 with the pmap of :169 over a pool of GPUs) ---
// muse_run with this rank's share (share_of) of every map.  The transport's device loop if every rank can take it
// (Comm::run_device_loop); otherwise muse_run's host loop (host_loop.h) with, per iteration, ONE gathered map (the solver launch
// and the exchange of the score blocks), after which every rank holds every score in simulation order and takes the same step
// (step.hpp) -- so the ranks agree on theta bit for bit without exchanging it, and the trajectory is the unsharded muse_run's.
// No Python, no torch tensor and no allocation sits between two maps.  info_out (may be NULL): THIS rank's solver infos,
// [maxsteps][count of this rank's elements] (the data element first on rank 0).
int muse_run_sharded(muse_ctx* ctx, uint64_t seed, const double* theta0, const muse_run_options* o, int32_t* niter_out,
                     double* theta_out, double* hist_out, double* gsims_out, muse_info* info_out) {
    Way w;
    if (const int rc = way_in(ctx, w)) return rc;
    if (!theta0 || !o || !niter_out || !theta_out || !hist_out || !gsims_out) return muse_set_error(MUSE_ERR_INVALID, "NULL argument");
    if (o->nsims < 2 || o->maxsteps < 1) return muse_set_error(MUSE_ERR_INVALID, "muse_run_sharded needs nsims >= 2 and maxsteps >= 1");
    if (o->prior_kind != 0 && o->prior_kind != 1) return muse_set_error(MUSE_ERR_INVALID, "prior_kind must be 0 (flat) or 1 (Gaussian)");
    const int nt = w.ntheta;
    if (nt > muse::kMaxTheta) return muse_set_error(MUSE_ERR_INVALID, "the native muse! loops take ntheta <= MUSE_MAX_THETA");
    const int S = o->nsims, world = w.comm->nranks, rank = w.comm->rank;
    const Share mine = share_of(S, world, rank);
    const int rc = w.comm->run_device_loop(w.stream, seed, theta0, o, mine, nt, niter_out, theta_out, hist_out, gsims_out, info_out);
    if (rc != kRunHostLoop) return rc;
    const int64_t rows = share_of(S, world, 0).count;   // rows of a rank's block of the gather: the largest share, which is rank 0's
    std::vector<double> gall((size_t)world * rows * nt);
    auto run_map = [&](int, const double* theta, int z0_mode, double* g, muse_info* info) {
        int e = muse_map_and_score_batch_gather_async(ctx, seed, mine.lo, mine.hi, rank == 0 ? 1 : 0, theta, o->atol, z0_mode, rows, 0);
        if (!e) e = muse_batch_wait_gathered(ctx, 0, gall.data(), info);
        if (e) return e;
        // every score in the reference's order: the data element (rank 0's first row), then the simulations by rank
        for (int r = 0; r < world; ++r) {
            const int64_t cnt = share_of(S, world, r).count;
            memcpy(g, gall.data() + (size_t)r * rows * nt, (size_t)cnt * nt * sizeof(double));
            g += cnt * nt;
        }
        return (int)MUSE_OK;
    };
    return muse::host_muse_loop("muse_run_sharded", nt, theta0, o, mine.count, run_map, niter_out, theta_out, hist_out, gsims_out, info_out);
}

}  // extern "C"
