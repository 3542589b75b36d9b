// Internal to the runtime (runtime/*.cpp): the context and data objects behind the C ABI of include/mlhip.h, error mapping,
// and the functions the ABI entry points of the four families (context / data / EM / K-means) share. Not installed.
#pragma once
#include "mlhip.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>   // types only: the library is dlopen'ed on first use (librccl is 570 MB; single-GPU users never pay for it)

#include <dlfcn.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <exception>
#include <functional>
#include <mutex>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <ctime>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "device/device.hpp"
#include "host/em_math.hpp"
#include "runtime/pass_history.hpp"

namespace mlhip_rt {

extern thread_local std::string g_error;   // context.cpp

struct InvalidArgument : std::runtime_error { using std::runtime_error::runtime_error; };
struct NoDevice : std::runtime_error { using std::runtime_error::runtime_error; };
struct Unsupported : std::runtime_error { using std::runtime_error::runtime_error; };
struct DomainError : std::runtime_error { using std::runtime_error::runtime_error; };

/// The covariance mode of an EM call (host/em_math.hpp). host::covariance_from_abi decodes the ABI's `covariance_type` -- the one place
/// that refuses a bad one; `guarded` reports its std::invalid_argument as MLHIP_E_INVALID_ARGUMENT.
using mlhip::host::Covariance;
using mlhip::host::covariance_doubles;
using mlhip::host::covariance_from_abi;
static_assert((int)Covariance::Full == MLHIP_COVARIANCE_FULL && (int)Covariance::Diagonal == MLHIP_COVARIANCE_DIAGONAL &&
                  (int)Covariance::Tied == MLHIP_COVARIANCE_TIED,
              "mlhip.h names the covariance types by Covariance");

#define HIP_CHECK(expr)                                                                                   \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess)                                                                             \
            throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(e_) + " at " #expr);  \
    } while (0)

/// What a failed all-reduce hook becomes: a library-owned hook (RCCL, a device group's in-process sum) leaves its reason in the
/// calling thread's error text; a caller's hook only has its return code.
inline std::runtime_error hook_failure()
{
    return std::runtime_error(g_error.empty() ? std::string("all-reduce hook failed") : "all-reduce hook failed: " + g_error);
}

template <class F> int guarded(F&& f)
{
    g_error.clear();                   // (mlhip_last_error speaks of the LAST call; hook_failure reads what a hook left during this one)
    try { f(); return MLHIP_OK; }
    catch (const InvalidArgument& e) { g_error = e.what(); return MLHIP_E_INVALID_ARGUMENT; }
    catch (const std::invalid_argument& e) { g_error = e.what(); return MLHIP_E_INVALID_ARGUMENT; }
    catch (const DomainError& e) { g_error = e.what(); return MLHIP_E_DOMAIN; }
    catch (const NoDevice& e) { g_error = e.what(); return MLHIP_E_NO_DEVICE; }
    catch (const Unsupported& e) { g_error = e.what(); return MLHIP_E_UNSUPPORTED; }
    catch (const std::exception& e) { g_error = e.what(); return MLHIP_E_RUNTIME; }
}

/// Blocks a context's data handles have given back, kept for the next handle: a fit of the reference's benchmark size (N = 10k, d = 4,
/// K = 3) spends 1.3 of its 2.6 ms in hipMalloc / hipHostMalloc / hipFree (some 25 device and 7 pinned blocks per handle; hipFree
/// also synchronises the device). One pool per context = per stream: a block goes from one handle to the next in stream order, and
/// a handle is only released behind a stream synchronisation (mlhip_data_free), so no work of the previous owner is pending on it.
/// Blocks keep their exact allocation size and are handed out only for requests of at most that size and more than half of it
/// (powers of two up to 1 MB, multiples of 1 MB above), up to a capped total; the rest goes back to the driver.
/// MLHIP_POOL=0: every buffer straight from / to the driver.
struct BufferPool {
    static constexpr size_t kMaxBlock = size_t(64) << 20, kMaxDevice = size_t(512) << 20, kMaxPinned = size_t(64) << 20;
    std::mutex m;                                   // (a group's worker thread allocates, its caller's thread releases)
    std::vector<std::pair<size_t, void*>> dev, pin;
    size_t dev_bytes = 0, pin_bytes = 0;
    bool enabled = [] { const char* e = std::getenv("MLHIP_POOL"); return !(e && e[0] == '0'); }();

    static size_t block_size(size_t b)
    {
        if (b <= 256) return 256;
        if (b <= (size_t(1) << 20)) { size_t s = 256; while (s < b) s <<= 1; return s; }
        return (b + (size_t(1) << 20) - 1) & ~((size_t(1) << 20) - 1);
    }
    void* take(bool pinned, size_t cap)
    {
        std::lock_guard<std::mutex> lock(m);
        auto& v = pinned ? pin : dev;
        for (size_t i = 0; i < v.size(); ++i)
            if (v[i].first == cap) {
                void* p = v[i].second;
                v[i] = v.back(); v.pop_back();
                (pinned ? pin_bytes : dev_bytes) -= cap;
                return p;
            }
        return nullptr;
    }
    /// false: not kept (the caller frees it).
    bool give(bool pinned, size_t cap, void* p)
    {
        if (!enabled || cap > kMaxBlock) return false;
        std::lock_guard<std::mutex> lock(m);
        size_t& total = pinned ? pin_bytes : dev_bytes;
        if (total + cap > (pinned ? kMaxPinned : kMaxDevice)) return false;
        (pinned ? pin : dev).emplace_back(cap, p);
        total += cap;
        return true;
    }
    void drain()
    {
        std::lock_guard<std::mutex> lock(m);
        for (auto& b : dev) (void)hipFree(b.second);
        for (auto& b : pin) (void)hipHostFree(b.second);
        dev.clear(); pin.clear(); dev_bytes = pin_bytes = 0;
    }
};

/// Growable device (hipMalloc) or pinned host (hipHostMalloc) buffer; its destructor releases the block. `bytes` is what was asked
/// for (the largest request so far: sizes derived from it -- grids, capacities -- do not depend on which block the pool handed out),
/// `cap` the block behind it. `pool` points at its owner's pool field (a data handle's mlhip_data::pool), read at every allocation
/// and release: detaching a handle from its context is one store there. Null: straight from / to the driver (local scratch, the
/// context's own buffers, a group's slots). Moving and swapping exchange the BLOCKS; a buffer stays with the pool it was declared with.
template <bool Pinned> struct Buffer {
    void* p = nullptr;
    size_t bytes = 0, cap = 0;
    BufferPool* const* pool = nullptr;
    Buffer() = default;
    explicit Buffer(BufferPool* const* owner_pool) : pool(owner_pool) {}
    Buffer(const Buffer&) = delete;
    Buffer& operator=(const Buffer&) = delete;
    Buffer(Buffer&& o) noexcept : p(o.p), bytes(o.bytes), cap(o.cap), pool(o.pool) { o.p = nullptr; o.bytes = o.cap = 0; }
    Buffer& operator=(Buffer&& o) noexcept
    {
        if (this != &o) {
            release();
            p = o.p; bytes = o.bytes; cap = o.cap;
            o.p = nullptr; o.bytes = o.cap = 0;
        }
        return *this;
    }
    ~Buffer() { release(); }
    void reserve(size_t b)
    {
        if (b <= bytes) return;
        if (b <= cap) { bytes = b; return; }
        release();
        BufferPool* from = pool ? *pool : nullptr;
        const size_t want = from && from->enabled ? BufferPool::block_size(b) : b;
        if (from && from->enabled) p = from->take(Pinned, want);
        if (!p) {
            if (Pinned) HIP_CHECK(hipHostMalloc(&p, want, hipHostMallocDefault));
            else HIP_CHECK(hipMalloc(&p, want));
        }
        bytes = b; cap = want;
    }
    void release()
    {
        BufferPool* to = pool ? *pool : nullptr;
        if (p && !(to && to->give(Pinned, cap, p))) (void)(Pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr; bytes = 0; cap = 0;
    }
    template <class T> T* as() const { return static_cast<T*>(p); }
};
using DevBuf = Buffer<false>;
using PinnedBuf = Buffer<true>;

struct Timer {
    double total_ms = 0;
    uint64_t launches = 0;
};

/// RCCL entry points, resolved from librccl.so.1 the first time a communicator is asked for. A process that already
/// holds an RCCL (e.g. the copy bundled with PyTorch-ROCm, same soname) gets that one back from dlopen.
struct Rccl {
    void* handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;      // (only the device group needs it)
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;                          // (optional: a device group cancels the collectives of a failed task)
    ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    ncclResult_t (*GetVersion)(int*) = nullptr;

    static Rccl& get()
    {
        static Rccl r = [] {
            Rccl x;
            const char* env = std::getenv("MLHIP_RCCL_LIBRARY");
            const char* names[] = {env, "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
            for (const char* n : names) {
                if (!n || !*n) continue;
                x.handle = dlopen(n, RTLD_NOW | RTLD_LOCAL);
                if (x.handle) break;
            }
            if (!x.handle) return x;
            auto sym = [&](const char* name) { return dlsym(x.handle, name); };
            x.GetUniqueId = reinterpret_cast<decltype(x.GetUniqueId)>(sym("ncclGetUniqueId"));
            x.CommInitRank = reinterpret_cast<decltype(x.CommInitRank)>(sym("ncclCommInitRank"));
            x.CommInitAll = reinterpret_cast<decltype(x.CommInitAll)>(sym("ncclCommInitAll"));
            x.CommDestroy = reinterpret_cast<decltype(x.CommDestroy)>(sym("ncclCommDestroy"));
            x.CommAbort = reinterpret_cast<decltype(x.CommAbort)>(sym("ncclCommAbort"));
            x.CommCount = reinterpret_cast<decltype(x.CommCount)>(sym("ncclCommCount"));
            x.AllReduce = reinterpret_cast<decltype(x.AllReduce)>(sym("ncclAllReduce"));
            x.GetErrorString = reinterpret_cast<decltype(x.GetErrorString)>(sym("ncclGetErrorString"));
            x.GetVersion = reinterpret_cast<decltype(x.GetVersion)>(sym("ncclGetVersion"));
            if (!(x.GetUniqueId && x.CommInitRank && x.CommDestroy && x.CommCount && x.AllReduce && x.GetErrorString)) {
                dlclose(x.handle);
                x.handle = nullptr;
            }
            return x;
        }();
        if (!r.handle)
            throw std::runtime_error("RCCL is not available: librccl.so.1 could not be loaded (set MLHIP_RCCL_LIBRARY)");
        return r;
    }
    void check(ncclResult_t rc, const char* what) const
    {
        if (rc != ncclSuccess) throw std::runtime_error(std::string("RCCL error in ") + what + ": " + GetErrorString(rc));
    }
};

}  // namespace mlhip_rt
using namespace mlhip_rt;   // (internal header: the runtime's own translation units only)

struct mlhip_group;   // group.cpp

struct mlhip_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    int num_cus = 256;
    // Device group (mlhip_ctx_create_group): `group` is set on the context the caller holds -- it owns no stream of its own, every
    // entry point fans out to the group's shard contexts; `member_of` / `shard` are set on those.
    mlhip_group* group = nullptr;
    mlhip_group* member_of = nullptr;
    int shard = 0;
    size_t stage_bytes = size_t(128) << 20;   // upload staging chunk (two pinned + two device buffers of this size)
    // all-reduce hook
    mlhip_allreduce_fn reduce_fn = nullptr;
    void* reduce_user = nullptr;
    int reduce_on_device = 0, world_size = 1, rank = 0;
    ncclComm_t comm = nullptr;   // library-owned RCCL communicator (mlhip_ctx_init_rccl); its all-reduce is the hook then
    BufferPool pool;         // blocks of released data handles, for the next one
    // data handles alive on this context: destroying the context DETACHES them (their buffers stop referring to the pool, their context
    // pointer goes null), so a handle freed after its context releases its memory to the driver instead of touching freed state
    std::mutex handles_m;
    std::vector<mlhip_data*> handles;
    void adopt(mlhip_data* h) { std::lock_guard<std::mutex> lock(handles_m); handles.push_back(h); }
    void disown(mlhip_data* h)
    {
        std::lock_guard<std::mutex> lock(handles_m);
        handles.erase(std::remove(handles.begin(), handles.end(), h), handles.end());
    }
    // scratch
    DevBuf small_dev;        // for all-reducing short host vectors through a device hook
    PinnedBuf small_host;
    DevBuf up_stage[2];      // upload staging (kept across uploads: pinned allocations are slow)
    PinnedBuf up_pin[2];
    // timing
    bool timing = false;
    typedef std::pair<hipEvent_t, hipEvent_t> EventPair;
    std::vector<EventPair> spare_events;
    std::vector<std::pair<const char*, EventPair>> pending;     // (names are string literals)
    std::map<std::string, Timer> timers;

    void use() const { HIP_CHECK(hipSetDevice(device)); }
    void sync() const { HIP_CHECK(hipStreamSynchronize(stream)); }

    /// Device time of a launch by a pair of HIP events on the stream the kernel goes to. The pair is only RECORDED here;
    /// the elapsed times are read when somebody asks (resolve_timers), so a timed region runs as it does untimed: no
    /// synchronisation between launches, the clocks the chip holds under a back-to-back stream of kernels.
    template <class F> void timed(const char* name, F&& launch)
    {
        if (!timing) { launch(); return; }
        if (pending.size() >= 4096) resolve_timers();
        EventPair e;
        if (!spare_events.empty()) { e = spare_events.back(); spare_events.pop_back(); }
        else { HIP_CHECK(hipEventCreate(&e.first)); HIP_CHECK(hipEventCreate(&e.second)); }
        HIP_CHECK(hipEventRecord(e.first, stream));
        launch();
        HIP_CHECK(hipEventRecord(e.second, stream));
        pending.push_back({name, e});
    }

    void resolve_timers()
    {
        if (pending.empty()) return;
        HIP_CHECK(hipEventSynchronize(pending.back().second.second));
        for (auto& p : pending) {
            float ms = 0;
            HIP_CHECK(hipEventElapsedTime(&ms, p.second.first, p.second.second));
            Timer& t = timers[p.first];
            t.total_ms += ms;
            t.launches += 1;
            spare_events.push_back(p.second);
        }
        pending.clear();
    }

    /// The installed hook on a DEVICE buffer, on the context's stream. Timed as "allreduce" (event pair around the collective
    /// on the stream: on a rank that arrives early this includes the wait for the slowest rank -- what a first multi-GPU run
    /// needs to see).
    void reduce_device(double* buf, size_t count)
    {
        int rc = 0;
        g_error.clear();
        timed("allreduce", [&] { rc = reduce_fn(reduce_user, buf, count, 1, stream); });
        if (rc != 0) throw hook_failure();
    }

    /// End-of-fit guard of a row-sharded job: parameters are never broadcast -- every rank applies the same closing arithmetic
    /// to the same all-reduced sums -- so ranks that received different sums (a collective that is not bitwise reproducible
    /// across ranks, a rank on different data) would drift apart silently. Every rank puts a 48-bit checksum of its results
    /// (three exactly representable 16-bit pieces) into its own slot of a zero vector, the vector is summed across ranks,
    /// and every rank compares all slots. One small collective per fit. MLHIP_RANK_CHECK=0 disables.
    void check_ranks_agree(const char* what, std::initializer_list<std::pair<const double*, size_t>> blocks)
    {
        if (!reduce_fn || world_size <= 1) return;
        static const bool on = [] { const char* e = std::getenv("MLHIP_RANK_CHECK"); return !(e && e[0] == '0'); }();
        if (!on) return;
        uint64_t h = 1469598103934665603ull;                         // FNV-1a over the bytes of the blocks
        for (const auto& b : blocks) {
            const unsigned char* p = reinterpret_cast<const unsigned char*>(b.first);
            for (size_t i = 0; i < b.second * sizeof(double); ++i) { h ^= p[i]; h *= 1099511628211ull; }
        }
        double mine[3];
        for (int j = 0; j < 3; ++j) mine[j] = (double)((h >> (16 * j)) & 0xffffu);
        const std::vector<double> v = exchange_slots(mine, 3);
        for (int r = 1; r < world_size; ++r)
            for (int j = 0; j < 3; ++j)
                if (v[3 * (size_t)r + j] != v[j])
                    throw std::runtime_error(std::string("ranks disagree on ") + what + " at the end of the fit (rank " + std::to_string(r) +
                                             " differs from rank 0): the statistics all-reduce did not give every rank the same sums");
    }

    /// The installed hook on a HOST buffer.
    void reduce_host(double* v, size_t count)
    {
        if (reduce_fn(reduce_user, v, count, 0, stream) != 0) throw hook_failure();
    }

    /// Sum `count` host doubles across ranks (no-op single rank).
    void allreduce_host(double* v, size_t count)
    {
        if (!reduce_fn) return;
        if (reduce_on_device) {
            small_dev.reserve(count * sizeof(double));
            HIP_CHECK(hipMemcpyAsync(small_dev.p, v, count * sizeof(double), hipMemcpyHostToDevice, stream));
            reduce_device(small_dev.as<double>(), count);
            HIP_CHECK(hipMemcpyAsync(v, small_dev.p, count * sizeof(double), hipMemcpyDeviceToHost, stream));
            sync();
        } else {
            reduce_host(v, count);
        }
    }

    /// The ranks that take part in a host exchange and this rank's place among them: (1, 0) without a hook.
    int slot_world() const { return reduce_fn ? world_size : 1; }
    int slot_rank() const { return reduce_fn ? rank : 0; }

    /// Every rank's `count` doubles in rank order (slot_world() x count): each rank writes its values into its own slot of a zero
    /// vector and the vector is summed across ranks -- 0 + v is v, so every value arrives as it was sent. One collective; none on a
    /// single rank.
    std::vector<double> exchange_slots(const double* mine, size_t count)
    {
        const size_t world = (size_t)slot_world();
        std::vector<double> all(world * count, 0.0);
        std::copy(mine, mine + count, all.begin() + (size_t)slot_rank() * count);
        if (world > 1) allreduce_host(all.data(), all.size());
        return all;
    }

    /// `count` doubles of a device buffer, summed across ranks, into a host buffer, in two halves (mlhip_kmeans_iterate runs its
    /// closing kernel between them): the device hook on the stream ...
    void reduce_on_stream(double* dev, size_t count)
    {
        if (reduce_fn && reduce_on_device) reduce_device(dev, count);
    }
    /// ... then down, wait, and the host hook where that is the installed kind. Single rank: the plain read-back.
    void fetch_reduced(double* host, const double* dev, size_t count)
    {
        HIP_CHECK(hipMemcpyAsync(host, dev, sizeof(double) * count, hipMemcpyDeviceToHost, stream));
        sync();
        if (reduce_fn && !reduce_on_device) reduce_host(host, count);
    }
    void reduce_to_host(double* host, double* dev, size_t count)
    {
        reduce_on_stream(dev, count);
        fetch_reduced(host, dev, count);
    }

    /// `count` doubles of a device buffer summed across ranks in place, nothing waits with a device hook; a host hook goes down
    /// through `stage` (pinned), and up again. No-op on a single rank.
    void reduce_in_place(double* dev, double* stage, size_t count)
    {
        if (!reduce_fn) return;
        if (reduce_on_device) { reduce_device(dev, count); return; }
        HIP_CHECK(hipMemcpyAsync(stage, dev, sizeof(double) * count, hipMemcpyDeviceToHost, stream));
        sync();
        reduce_host(stage, count);
        HIP_CHECK(hipMemcpyAsync(dev, stage, sizeof(double) * count, hipMemcpyHostToDevice, stream));
    }
};

/// What the last E-step left on the device for a data handle, and what has to be rebuilt before somebody reads the N x K block:
///   kNone        -- nothing usable (the workspace was resized for another K, or lw was borrowed as scratch);
///   kBlock       -- lw (and lse, once the E-step or the self-normalising statistics pass wrote it);
///   kRecords     -- lse and the full-covariance records in params_dev (after a fused step, the resident loop, a lagged loop that
///                   ran one iteration ahead): ensure_lw reruns the E-step kernel on the same records;
///   kModeRecords -- lse, the records of a diagonal or tied one-kernel pass in params_dev and the parameters' host copy in their
///                   mode's form (kept): ensure_lw expands them to full covariances (host::covariances_as_full).
/// Only the members below assign the fields.
struct EstepState {
    enum What { kNone, kBlock, kRecords, kModeRecords };
    What what = kNone;
    int rec_layout = 0;           // record layout currently in params_dev: 0 = valu, 2 = mfma4 (CloseArgs::layout codes)
    bool rec_fold = false;        // mfma4 records in FOLD form (vector slot = -W (mu - shift)): layout.hpp kEstepFoldLimit
    int n_ll = 0;                 // log-likelihood partials the last pass wrote
    // source of the last statistics pass (for the per-component refinement pass)
    int stats_mode = 0;
    const double* stats_resp = nullptr;
    size_t stats_ld = 0;
    // kModeRecords: the mode and the parameters of that pass (the N x K block is rebuilt from them on demand)
    struct Kept {
        Covariance mode = Covariance::Full;
        std::vector<double> mixing, means;                    // [K], [K][d]
        std::vector<double> covariance;                       // covariance_doubles(mode, K, d): the K x d variances / the one d x d covariance
    } kept;

    // The block is one the screened E-step may start from (launch_estep): every entry an evaluated value or an upper bound of one, under
    // the records ScreenState keeps. Every member that changes what the block is clears it.
    bool screenable = false;

    void invalidate() { what = kNone; screenable = false; }
    void block_written(int grid) { what = kBlock; n_ll = grid; screenable = false; }
    void block_screenable() { screenable = what == kBlock; }
    /// The records ScreenState keeps are no longer the block's (its history starts again with another K).
    void block_not_screenable() { screenable = false; }
    /// A weighted block: the E-step's log-likelihood partials were replaced by `grid` partials of w_i lse_i (launch_estep).
    void ll_weighted(int grid) { n_ll = grid; }
    void records_only(int grid) { what = kRecords; n_ll = grid; screenable = false; }
    /// A one-kernel pass of `mode` (diagonal, tied) left its records and `grid` log-likelihood partials.
    void mode_records_only(Covariance mode, int grid) { what = kModeRecords; kept.mode = mode; n_ll = grid; screenable = false; }
    /// A later (speculative) pass overwrote lw / lse; the records in params_dev still stand.
    void block_overwritten() { if (what == kBlock) what = kRecords; screenable = false; }
    /// The parameters behind the records of `mode` in params_dev (mlhip_em_iterate: set once, when the loop is over).
    void parameters(Covariance mode, int K, int d, const double* mixing, const double* means, const double* covariance)
    {
        kept.mode = mode;
        kept.mixing.assign(mixing, mixing + K);
        kept.means.assign(means, means + (size_t)K * d);
        kept.covariance.assign(covariance, covariance + covariance_doubles(mode, K, d));
    }
    void records_are(int layout, bool fold) { rec_layout = layout; rec_fold = fold; }
    void stats_from(int mode, const double* resp, size_t ld) { stats_mode = mode; stats_resp = resp; stats_ld = ld; }

    /// What a later call needs of this state apart from the record buffer itself (mlhip_em_iterate_restarts keeps the best restart's
    /// while the next one runs): the N x K block is not part of it -- a state put back is one whose block has to be rebuilt.
    /// The source of the last statistics pass (stats_mode / stats_resp / stats_ld) is not part of it either: it only serves the
    /// refinement pass INSIDE the step that ran the statistics, and every step sets it before it reads it (stats_from).
    struct Small {
        What what = kNone;
        int rec_layout = 0;
        bool rec_fold = false;
        int n_ll = 0;
        Kept kept;
    };
    Small small() const { return Small{what == kBlock ? kRecords : what, rec_layout, rec_fold, n_ll, kept}; }
    void put_back(const Small& s) { what = s.what; rec_layout = s.rec_layout; rec_fold = s.rec_fold; n_ll = s.n_ll; kept = s.kept; screenable = false; }

    bool on_device() const { return what != kNone; }
    bool needs_rebuild() const { return what == kRecords || what == kModeRecords; }
    bool mode_records() const { return what == kModeRecords; }
};

/// The history of the self-normalising statistics passes of a data handle (run_mstats): both kernels add the number of nonzero
/// responsibilities to a device word, which is copied to the pass's slot of a pinned ring (PassRing: its counts are read without a
/// wait). Only the members below assign the fields.
class StatsHistory {
public:
    explicit StatsHistory(BufferPool* const* pool) : nz_dev_(pool), nz_host_(pool) {}
    /// A pass with K begins: the device word the kernel counts into, cleared on the stream.
    unsigned long long* begin(int K, hipStream_t stream)
    {
        ring_.begin(K);
        nz_dev_.reserve(sizeof(unsigned long long));
        nz_host_.reserve(3 * sizeof(unsigned long long));
        HIP_CHECK(hipMemsetAsync(nz_dev_.p, 0, sizeof(unsigned long long), stream));
        return nz_dev_.as<unsigned long long>();
    }
    /// Whether the pass that has begun runs the sparse kernel (sparse_stats_wanted).
    bool sparse_wanted(uint32_t n, int force, bool supported) const { return sparse_stats_wanted(ring_, counts(), n, force, supported); }
    /// The kernel is on the stream: its count goes to the pass's slot.
    void end(hipStream_t stream)
    {
        HIP_CHECK(hipMemcpyAsync(nz_host_.as<unsigned long long>() + ring_.slot(), nz_dev_.p, sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                 stream));
        ring_.finish(true);
    }
    const PassRing& ring() const { return ring_; }
    const unsigned long long* counts() const { return nz_host_.as<unsigned long long>(); }

private:
    DevBuf nz_dev_;
    PinnedBuf nz_host_;
    PassRing ring_;
};

/// What the screened E-step (em_screen.cpp, em_estep_screen.hip) keeps on a data handle. Passes of the screened kernel's DOMAIN
/// (launch_estep) are counted; the TRACKED ones among them -- those that may screen or leave a block a later pass may screen from --
/// keep the rest: the records the N x K block belongs to, which of its values are evaluated ones, and the ring of their candidate
/// counts. A tracked pass that runs dense -- one sent back for want of information included -- leaves no count and a block of
/// evaluated values only. Only the members below assign the fields; EstepState::screenable says whether the block is still theirs.
class ScreenState {
public:
    explicit ScreenState(BufferPool* const* pool) : rec_(pool), exact_(pool), consts_(pool), dev_(pool), host_(pool) {}
    /// This pass of `dt` is tracked with K: the buffers, and the history from its start with another K than the last tracked pass's.
    void track(mlhip_data* dt, int K);
    /// The tracked pass on `a`, where it is wanted (screen_wanted; `force`: EmRoute::screen) and every component's bound carries
    /// information: the screened kernel's grid. 0: the dense kernel has to run.
    int run(mlhip_data* dt, const mlhip::EstepArgs& a, int force);
    /// A pass of the domain is on the stream, screened or dense; a tracked one leaves the block with its records (`a.params`) for the next.
    void pass_done(mlhip_data* dt, const mlhip::EstepArgs& a, bool tracked, bool screened);
    /// mlhip_em_screen_counts, added to `counts`; the caller has waited for the stream.
    void add_counts(uint64_t counts[4]) const;

private:
    DevBuf rec_;                  // the records the block belongs to (a copy: the ring of mlhip_em_iterate and params_dev move on)
    DevBuf exact_;                // one word per sample, bit k = "the stored value of component k is an evaluated one"
    DevBuf consts_;               // 4 doubles per component: the bound constants of the step from rec_ to the pass's records
    DevBuf dev_;                  // [components without information (32 bits), padding | candidates]: one memset clears both
    PinnedBuf host_;              // [the tracked ring's three candidate counts | the first word of dev_]
    bool all_exact_ = true;       // a dense pass wrote the block: exact_ is not read
    PassRing tracked_;
    uint64_t n_screened_ = 0, n_dense_ = 0, n_no_info_ = 0;   // passes of the domain, tracked or not; send-backs (those count as dense too)
};

struct mlhip_data {
    // The context's pool while the context lives (null after it: blocks go back to the driver). Declared first: every buffer below
    // is bound to this field by its initialiser, so a new buffer needs its declaration and nothing else.
    BufferPool* pool = nullptr;
    mlhip_ctx* ctx = nullptr;
    // A block uploaded through a device group: `parts[s]` is shard s's resident block (rows first_row[s] .. first_row[s+1] of the
    // caller's sample); nothing else below is used then.
    std::vector<mlhip_data*> parts;
    std::vector<uint64_t> first_row;
    int d = 0, D = 0;
    uint32_t n = 0, n_pad = 0;
    uint64_t n_global = 0;
    size_t ldx = 0;
    DevBuf xt{&pool};             // [D][ldx]
    DevBuf shift_dev{&pool};      // d doubles
    std::vector<double> shift;    // host copy
    // Row weights (mlhip_data_set_weights; a group's handle mirrors `weighted` / `weight_sum` of its parts): n_pad doubles, zero
    // beyond n. wresp: [em_K][ldr], w_i r_ik of the last statistics pass of a weighted block on a route without the self-
    // normalising statistics kernel (run_mstats), or the one column of a refinement pass.
    DevBuf weights{&pool}, wresp{&pool};
    bool weighted = false;
    double weight_sum = 0;        // W over all ranks
    // Tied-covariance extension: T = sum_i w_i xt_i xt_i^T over ALL ranks (packed, stats_count(d) doubles; the K = 1, r = 1 statistics
    // pass), formed by the first tied kernel step on the handle; empty: not formed yet. mlhip_data_set_weights drops it.
    std::vector<double> total_scatter;
    /// Rows behind the host arrays of a call on this handle: this block's -- a group's handle holds the whole sample.
    uint64_t rows() const { return parts.empty() ? (uint64_t)n : n_global; }
    /// What the log-likelihood and the mixing proportions are divided by: W, or the row count of an unweighted block.
    double total_weight() const { return weighted ? weight_sum : (double)n_global; }
    // Covariance ridge (mlhip_data_set_covariance_ridge; a group's handle mirrors its parts'): what every M-step on this handle adds
    // to the diagonal of each covariance it FORMS -- on the host and as an argument of the device closings. Finite, >= 0.
    double ridge = MLHIP_DEFAULT_COVARIANCE_RIDGE;
    // EM workspace (sized for em_K)
    int em_K = 0;
    size_t ldr = 0;
    DevBuf lw{&pool}, lse{&pool}, esum{&pool}, ll_partials{&pool}, params_dev{&pool}, partials{&pool}, stats_dev{&pool}, resp_dev{&pool},
        labels_dev{&pool};
    PinnedBuf params_host{&pool}, stats_host{&pool};
    EstepState estep;
    bool has_estep_results(int K) const { return estep.on_device() && em_K == K; }
    // mlhip_em_iterate (em_loop.cpp): parameters and the E-steps' records stay on the device between iterations, in a ring of three --
    // iteration i reads the records of slot i % 3 (params_dev / params_next / params_prev take turns) and writes pack and records
    // (i + 1) % 3; it_pack: [info (1 + 2K) | mixing (K) | means (K d) | covariances]; one pinned read-back slot and event per pack
    DevBuf params_next{&pool}, params_prev{&pool}, it_pack[3] = {DevBuf{&pool}, DevBuf{&pool}, DevBuf{&pool}};
    DevBuf it_sync{&pool}, it_xch{&pool};   // device-resident loop (em_resident.hip): arrival counter / give-up flag, exchange blocks
    DevBuf close_work{&pool};     // closing arithmetic at d > 64 (em_close_big.hip): the components' L and W
    PinnedBuf it_info_slot[3] = {PinnedBuf{&pool}, PinnedBuf{&pool}, PinnedBuf{&pool}};
    PinnedBuf it_history{&pool};  // [result words | log-likelihood history] of the resident loop
    hipEvent_t it_event[3] = {nullptr, nullptr, nullptr};
    // mlhip_em_iterate_restarts (em_restarts.cpp): the records behind the E-step state of the best restart so far while another one
    // runs; the batched route's per-restart rings, scratch and statistics (one block, carved by the loop) and its pinned info blocks
    DevBuf rs_kept{&pool}, rs_dev{&pool};
    PinnedBuf rs_info{&pool};
    DevBuf refine_shift{&pool}, refine_stats{&pool};   // the per-component refinement pass
    // The pass history behind the two history-dependent route choices of a fit (pass_history.hpp): both keep running across calls,
    // and so across the restarts of mlhip_em_iterate_restarts, and start again only with another K; a weighted block enters neither
    // (route.cpp forces both choices off).
    StatsHistory stats_history{&pool};
    ScreenState screen{&pool};
    // K-means workspace
    DevBuf km_labels[2] = {DevBuf{&pool}, DevBuf{&pool}};
    DevBuf km_cent{&pool}, km_cent_next{&pool}, km_partials{&pool}, km_out{&pool}, km_mind{&pool}, km_probe{&pool}, km_scale{&pool},
        km_cnorm{&pool}, km_xt_pad{&pool};
    PinnedBuf km_host{&pool};
    DevBuf kpp_w{&pool}, kpp_scr{&pool};   // mlhip_kpp_draw: the running-minimum weights, block sums / offsets / result
    DevBuf fp_w{&pool}, fp_scr{&pool};     // mlhip_kpp_draw_fixed_point: the running-minimum weights; [slots | block sums | block maxima | centroid]
    PinnedBuf fp_host{&pool};              // its read-back slots
    int km_cur = 0;
    bool km_have_old = false;
    // Weighted K-means (mlhip_kmeans_*_weighted): max|x_j| over ALL ranks as ensure_km_workspace found it (d doubles, host), and the
    // power-of-two factors of the weighted exact sums (KmWeightedArgs::factors), derived once per weight vector from the largest
    // weight of the whole sample; mlhip_data_set_weights drops them.
    std::vector<double> km_colmax;
    DevBuf km_wfactors{&pool};
    bool km_wfactors_valid = false;

    mlhip_data() = default;
    mlhip_data(const mlhip_data&) = delete;      // (the buffers point at this object's pool field)
    mlhip_data& operator=(const mlhip_data&) = delete;
    ~mlhip_data()
    {
        for (mlhip_data* p : parts) mlhip_data_free(p);
        for (auto& e : it_event) if (e) (void)hipEventDestroy(e);
    }
};

namespace mlhip_rt {

using namespace mlhip;


constexpr int kMaxLlPartials = 2048;

/// MLHIP_TRACE=1: wall-clock microseconds of the host-visible phases of one EM iteration on stderr.
struct PhaseTrace {
    bool on;
    std::chrono::steady_clock::time_point t;
    PhaseTrace() : on([] { const char* e = std::getenv("MLHIP_TRACE"); return e && e[0] == '1'; }()), t(std::chrono::steady_clock::now()) {}
    void mark(const char* name)
    {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[mlhip] %-22s %8.1f us\n", name, std::chrono::duration<double, std::micro>(now - t).count());
        t = now;
    }
};

inline void require(bool ok, const char* msg) { if (!ok) throw InvalidArgument(msg); }
/// A covariance ridge (mlhip.h): finite and >= 0 (NaN fails the comparison).
inline void require_ridge(double ridge) { require(ridge >= 0 && std::isfinite(ridge), "the covariance ridge must be finite and >= 0"); }

/// What one K-means pass runs on: the data block (a zero-padded copy where the matrix-core kernel needs one) and its rows.
struct KmBlock {
    const double* xt;
    int D;
};

// ---- routes (route.cpp): which kernels one EM or K-means entry-point call runs, decided once per call from the shape (the
// tuning rules next to the kernels) and the routing switches of DESIGN.md §7 -- the only place the library reads those. Sizing,
// launching and reporting take their decisions from the route.

/// The E-step kernels: scalar-fed (em_estep.hip, d <= 128), 4x4 matrix-core (em_estep_mfma4.hip, d = 12 .. 128), and above d = 128
/// the matrix-core tier (big_dim.hip, d <= 1024) or the plain one (generic_dim.hip).
enum class Estep { kScalarFed, kMatrix4, kBigDim, kPlain };

struct EmRoute {
    Estep estep = Estep::kScalarFed;
    bool records_on_device = false;    // d > 64: a fit's first records are factored by the closing kernels (em_close_big.hip)
    bool fold_allowed = false;         // d <= 32: the matrix-core E-step may take its FOLD form (kEstepFoldLimit)
    bool estep_rows = false;           // D = 24, 32: the matrix-core E-step's FOLD, lw-only launches walk their blocks row-quad major
    bool fused = false;                // E-step + statistics in one kernel (em_fused_small.hip)
    int fused_form = kFusedLdsFeed;    // FusedArgs::form
    bool self_norm = false;            // the matrix-core E-step writes lw only, the statistics kernel normalises it
    int sparse = -1;                   // self-normalising statistics: 1 the sparse kernel, 0 the dense one, -1 by call history
    int screen = -1;                   // E-step passes of a fit: 1 screened wherever the block allows, 0 dense, -1 by call history
    bool balanced = true;              // d <= 32: the wide statistics kernel deals balanced (column block, row block) units
    bool diag_exact = false;           // diagonal mode: the exact density form always
    bool diag_kernel = false;          // diagonal mode: the one-kernel iteration (em_diag.hip), else the full-covariance kernels
    bool device_close = false;         // mlhip_em_iterate closes every iteration on the device (em_close.hip)
    bool resident = false;             // mlhip_em_iterate may run the whole loop in one launch (em_resident.hip)
    /// MstatsArgs::plain: the plain tier above d = 128, whole column blocks per wave at d <= 32.
    int stats_plain(int d) const { return d > kMaxDim ? estep == Estep::kPlain : !balanced; }
};
/// The kernels of K components on this block. Diagonal: the diagonal-covariance kernel where it exists (em_diag.hip), else the
/// full-covariance kernels. Tied: the full-covariance kernels of the composed step, the matrix-core E-step never in its FOLD form.
EmRoute em_route(const mlhip_data* data, int K, Covariance mode);

/// A tied-covariance step: the one-kernel iteration (em_tied.hip: unweighted blocks, d <= 32, K <= 64, unless MLHIP_TIED=composed or
/// the composed step was measured faster: route.cpp) or COMPOSED -- one full-covariance step on the route of K full components on
/// this block, with the covariance replicated and the result pooled. (mlhip.h names the routes by these values.)
enum TiedKernel : int { kTiedComposed = 0, kTiedKernel = 1 };
/// The route of one EM step or loop in a covariance mode: what em_step and em_iterate dispatch on.
struct ModeRoute {
    Covariance mode = Covariance::Full;
    EmRoute em;                        // em_route(data, K, mode)
    int tied_kernel = kTiedComposed;   // Tied only
};
ModeRoute mode_route(const mlhip_data* data, int K, Covariance mode);

/// mlhip_em_score: the scalar-fed score kernel (em_score.hip) and the matrix-core E-step's SCORE form (em_estep_mfma4.hip) where the
/// E-step's route is scalar-fed / matrix-core; composed -- the E-step kernel on row chunks into a bounded scratch block, then
/// em_score_finish_kernel -- above d = 128 and under MLHIP_SCORE=composed. (mlhip.h names the kernels by these values.)
enum ScoreKernel : int { kScoreScalarFed = 0, kScoreMatrix4 = 1, kScoreComposed = 2 };
constexpr uint64_t kScoreScratchBytes = uint64_t(256) << 20;
struct ScoreRoute {
    int kernel = kScoreScalarFed;
    EmRoute em;                        // the E-step's route for the same block and K: record layout, where the records are factored
    uint32_t chunk_rows = 0;           // composed: rows per chunk, a multiple of kSampleTile (MLHIP_SCORE_ROWS, else by kScoreScratchBytes)
};
ScoreRoute score_route(const mlhip_data* data, int K);

/// mlhip_em_sample / _sample_data: the kernel em_sample_route (device/em_sample.hip) names for the shape -- under
/// MLHIP_SAMPLE_TABLE=global the global-table form where the LDS-table form would run (same bits) -- and the rows the host-output form
/// generates per chunk: a pool block of at most kSampleChunkBytes, whole 64-row tiles (MLHIP_SAMPLE_ROWS overrides; the rows do not
/// depend on it). (mlhip.h names the kernels by SampleKernel's values.)
constexpr uint64_t kSampleChunkBytes = uint64_t(64) << 20;
struct SampleRoute {
    int kernel = kSampleLdsTable;
    uint64_t chunk_rows = 64;
};
SampleRoute sample_route(int d, uint32_t K);

/// mlhip_em_conditional_means: the E-step tier of the observed block's shape (em_route, full covariances, exact form), the finishing
/// kernel em_condition_route (device/em_condition.hip) names for (dO, dM) -- MLHIP_CONDITION=plain: the plain tier everywhere -- and the
/// rows per chunk: the largest whole number of sample tiles whose K + dM doubles per row (log-responsibilities and output) stay within
/// kScoreScratchBytes (MLHIP_CONDITION_ROWS=n overrides, rounded UP to whole tiles; the rows do not depend on it). `skip`: the
/// kernel passes over components no row of a wave has a share in (MLHIP_CONDITION_SKIP=0: it runs them all; same bits).
/// (mlhip.h names the kernels by ConditionKernel's values.)
struct ConditionRoute {
    EmRoute em;
    int kernel = kConditionRegisters;
    uint32_t chunk_rows = 0;
    bool skip = true;
};
ConditionRoute condition_route(const mlhip_data* data, int K, int dM);
/// mlhip_em_conditional_samples: condition_route's E-step tier and kernel tier (the same switches), and the rows per chunk sized so
/// that the K log-responsibilities and the output of min(n_draws, kConditionSampleDraws) draws per row stay within kScoreScratchBytes
/// (MLHIP_CONDITION_ROWS=n overrides, rounded UP to whole tiles). `draws`: how many draws one launch behind a chunk's E-step takes --
/// as many of n_draws as fit the same bound beside the chunk's log-responsibilities, at least 1. No row depends on either.
constexpr uint32_t kConditionSampleDraws = 8;
struct ConditionSampleRoute {
    EmRoute em;
    int kernel = kConditionRegisters;
    uint32_t chunk_rows = 0, draws = 1;
};
ConditionSampleRoute condition_sample_route(const mlhip_data* data, int K, int dM, uint32_t n_draws);
/// mlhip_em_conditional_variances: condition_route's E-step tier, switches and chunking, with the kernel tier
/// em_condition_variance_route (device/em_condition_variance.hip) names for (dO, dM) in the form asked for, and the rows per chunk
/// sized for the K log-responsibilities plus `out_doubles` per row: the call's outputs (dM or dM^2, dM more with the mean) and, on
/// the plain tier, that kernel's 2 dM doubles of work. No row depends on the chunk.
ConditionRoute condition_variance_route(const mlhip_data* data, int K, int dM, bool full, bool with_means);
/// mlhip_em_conditional_cdfs / mlhip_em_conditional_quantiles: condition_route's E-step tier, switches and chunking, with the kernel
/// tier em_condition_quantile_route (device/em_condition_quantile.hip) names for (dO, dM) and the call, and the rows per chunk sized so
/// that the K log-responsibilities, the mean if asked for, and the CDF's values and output -- or the blocks (and trip counts) of
/// min(n_prob, kConditionQuantileGroup) probabilities -- stay within kScoreScratchBytes (MLHIP_CONDITION_ROWS=n overrides, rounded UP
/// to whole tiles). `group`: how many probabilities one launch behind a chunk's E-step takes -- as many as fit the same bound, at
/// least 1, and at most MLHIP_CONDITION_GROUP=n where that is set. No row depends on either.
constexpr uint32_t kConditionQuantileGroup = 8;
struct ConditionQuantileRoute {
    EmRoute em;
    int kernel = kConditionRegisters;
    uint32_t chunk_rows = 0, group = 1;
    bool skip = true;
};
ConditionQuantileRoute condition_quantile_route(const mlhip_data* data, int K, int dM, bool quantile, uint32_t n_prob, bool with_means,
                                                bool with_iterations);
/// mlhip_silhouette: the tier silhouette_tier (device/silhouette.hip) names for d -- MLHIP_SILHOUETTE=plain: the plain tier at every
/// d --, the register tier's column feed (scalar loads; MLHIP_SILHOUETTE_FEED=lds: the LDS feed), the pair kernel's grid where
/// MLHIP_SILHOUETTE_GRID=n gives one, and the evaluated rows per block: the largest whole number of row tiles whose chunk sums (one
/// double per chunk and row) stay within kScoreScratchBytes, at least one tile (MLHIP_SILHOUETTE_ROWS=n overrides, rounded UP to whole
/// tiles). No bit depends on any of them. (mlhip.h names the tiers by SilhouetteKernel's values.)
struct SilhouetteRoute {
    int kernel = kSilhouetteRegisters, feed = kSilhouetteScalarFeed;
    uint32_t rows_override = 0;
    int grid = 0;
    uint32_t block_rows(uint64_t n_chunks, uint64_t m) const;
};
SilhouetteRoute silhouette_route(const mlhip_data* data);
/// mlhip_em_impute, the rows grouped by their pattern of NaNs (host/impute_plan.hpp); on either route the complete rows go through
/// mlhip_em_score and the rows of all NaN are formed on the host.
///   COMPOSED  every group of at most `rows` rows of one pattern through the conditional-means pass of that pattern (condition_route:
///             its kernels, chunks and switches) with the model conditioned on the host: every shape, launches grow with the patterns;
///   KERNEL    2 <= d <= 32 (MLHIP_IMPUTE=composed: COMPOSED there too): the records of at most `patterns` patterns at a time built on
///             the device (em_impute_records.hip; 0: as many as kImputeRecordBytes hold), then per chunk of `rows` rows one launch of
///             the evaluation kernel (em_impute.hip) per padding class present.
/// `rows`: MLHIP_IMPUTE_ROWS=n, else kImputeRows (composed) / the rows whose coordinates fill kImputeRowBytes (kernel). `grid_cap`:
/// MLHIP_IMPUTE_GRID=n. No row depends on any of them. (mlhip.h names the routes by ImputeKind's values.)
enum ImputeKind : int { kImputeComposed = 0, kImputeKernel = 1 };
constexpr uint32_t kImputeRows = uint32_t(1) << 20;
constexpr uint64_t kImputeRowBytes = uint64_t(64) << 20, kImputeRecordBytes = uint64_t(256) << 20;
struct ImputeRoute {
    int kind = kImputeComposed;
    uint32_t rows = kImputeRows, patterns = 0;
    int grid_cap = 0;
    bool skip = true;
};
ImputeRoute impute_route(int d, int K);
/// The argument checks of mlhip_em_condition and mlhip_em_condition_covariances behind their null checks; returns the covariance mode.
Covariance check_condition_arguments(uint32_t d, uint32_t K, int covariance_type, const uint32_t* observed, uint32_t n_observed);

/// mlhip_em_iterate_restarts: R loops one after the other (every shape and mode), or BATCHED -- the restarts still running share the
/// three launches of an iteration (em_restarts.hip) -- where the solo iteration is the fused kernel in its vector-unit form on at
/// most one workgroup per CU: full covariances, an unweighted block, a single rank without an all-reduce hook. The batch is taken from
/// kRestartsBatchFrom restarts on; MLHIP_EM_RESTARTS=sequential / batch forces either where the batch exists. (mlhip.h names the
/// routes by these values.)
enum RestartsKind : int { kRestartsSequential = 0, kRestartsBatched = 1 };
// Measured (profiles/em_restarts_timing.txt: 50 iterations per restart, one batched call against R solo calls, N = 1 000 / 10 000 /
// 65 536 at d = 2, K = 3 and N = 10 000 at d = 4, K = 3): at R = 2 the batch loses at three of the four shapes (0.73 - 0.91 of the
// solo calls' speed: 25 - 26 us per batched iteration against two resident iterations of 9 - 12 us), from R = 4 on it wins at all of
// them (1.36 - 2.26x at R = 4, 5.4 - 7.0x at R = 32). R = 3 was not measured and stays sequential.
constexpr uint32_t kRestartsBatchFrom = MLHIP_RESTARTS_BATCH_FROM;
constexpr size_t kRestartsScratchBytes = size_t(64) << 20;   // the batched route's device block: caps the restarts of one launch
struct RestartsRoute {
    int kind = kRestartsSequential;
    int per_launch = 1;                // restarts one launch carries (<= mstats::kRestartsMaxBatch, and what the scratch holds)
    int grid = 0;                      // batched: the solo pass's grid for this block (em_fused_valu_small_grid)
    EmRoute em;                        // the solo route of one restart
};
/// Doubles of device memory one restart of the batched route needs (two record slots, a pack, partial blocks, statistics).
size_t restarts_doubles_per_restart(int d, int K, int grid);
RestartsRoute restarts_route(const mlhip_data* data, int K, Covariance mode, uint32_t R);

struct KmRoute {
    bool pad = false;                  // the block runs on a copy zero-padded to a multiple of 4 dimensions (km_xt_pad)
    int kernel = kKmDirect;            // KmeansArgs::kernel
    bool resident = false;             // mlhip_kmeans_iterate runs the whole loop in one launch (kmeans_resident.hip)
};
KmRoute km_route(const mlhip_data* data, int K);

// ---- shared between the families (definitions: context.cpp, data.cpp, em.cpp, kmeans.cpp) ----

int env_int(const char* name, int fallback);

/// memcpy split over a few threads: one core moves ~10 GB/s (less into untouched pages), below the PCIe rate it feeds.
void copy_bytes(void* dst, const void* src, size_t bytes);

void finish_upload(mlhip_data* dt);

mlhip_data* upload_common(mlhip_ctx* ctx, const double* x, bool on_device, uint32_t d, uint64_t n, int64_t ld);

/// Device -> pageable host copy of `cols` columns of `col_bytes` bytes each (source / destination pitches given), staged through
/// the context's two pinned buffers: the CPU unpacks chunk i while the DMA engine fetches chunk i+1. A direct copy into
/// pageable memory runs at ~3 GB/s on this platform; this one at PCIe rate.
void download_columns(mlhip_ctx* ctx, char* dst, size_t dst_pitch, const char* src, size_t src_pitch, size_t col_bytes, size_t cols);

void ensure_em_workspace(mlhip_data* dt, int K);

/// Layout (CloseArgs::layout codes) and form of a set of E-step records.
struct RecordForm {
    int layout;
    bool fold;
};

/// The K component records for the route's E-step kernel, from host parameters into `target`: the host factorization through `staging`,
/// or (d > 64) the device factorization with `work` as its scratch; touches nothing else of the handle (prepare_estep passes the
/// handle's buffers, mlhip_em_score buffers of its own). `allow_fold`: matrix-core records may take the FOLD form.
RecordForm build_records(mlhip_data* dt, const EmRoute& r, int K, const double* mixing, const double* means, const double* covs,
                         bool allow_fold, DevBuf& target, PinnedBuf& staging, DevBuf& work);

/// Builds the per-component records for the route's E-step kernel and uploads them to params_dev, whose descriptor they become -- or
/// to `target` (mlhip_em_iterate's ring), whose descriptor is the caller's to keep. Returns the records' form.
RecordForm prepare_estep(mlhip_data* dt, const EmRoute& r, int K, const double* mixing, const double* means, const double* covs,
                         DevBuf* target = nullptr);

/// E-step kernel on the records in params_dev: fills lw and -- unless the statistics kernel is going to normalise the
/// log-responsibilities itself (`with_lse` false, matrix-core kernel only) -- lse and the log-likelihood partials.
/// `records` / `fold`: another record buffer than params_dev and its form (mlhip_em_iterate keeps a ring of them); default: params_dev
/// and its form.
/// `may_screen`: a pass of a fit (mlhip_em_step, mlhip_em_iterate) -- the only ones that may take the screened kernel instead
/// (em_estep_screen.hip; the rule is screen_wanted's, pass_history.hpp); rebuilds for labels / responsibilities, scoring, conditioning and restarts never do.
void launch_estep(mlhip_data* dt, const EmRoute& r, int K, bool with_lse = true, const DevBuf* records = nullptr, int fold = -1,
                  bool may_screen = false);

void run_estep(mlhip_data* dt, const EmRoute& r, int K, const double* mixing, const double* means, const double* covs,
               bool with_lse = true, bool may_screen = false);

/// After a fused step only lse exists on the device; whoever needs the log-responsibility block (labels,
/// responsibilities, a separate M-step, the refinement pass) gets it rebuilt from the same parameter records.
void ensure_lw(mlhip_data* dt, const EmRoute& r, int K);

/// All-reduces the reduced statistics buffer [K*F stats, ll_sum] and leaves it in stats_host.
void collect_stats(mlhip_data* dt, int K, size_t count = 0);

/// The fused kernel's arguments on the records in `records` (null: params_dev).
FusedArgs fused_args(const mlhip_data* dt, const EmRoute& r, int K, const DevBuf* records);

/// What a fused pass (launch_fused_step, or the resident loop that runs the same pass) leaves behind on the handle.
void fused_pass_done(mlhip_data* dt, int grid);

/// The fused kernel + reduction on the records already in params_dev; statistics end in stats_dev (and, with `collect`, all-
/// reduced in stats_host).
void launch_fused_step(mlhip_data* dt, const EmRoute& r, int K, bool collect, const DevBuf* records = nullptr);

/// One EM iteration's device work in a single kernel where the route has it (r.fused): no N x K block in HBM. Returns false
/// otherwise.
bool run_fused_step(mlhip_data* dt, const EmRoute& r, int K, const double* mixing, const double* means, const double* covs);

/// Runs the statistics kernel on log-responsibilities (mode kFromLogResp: the E-step's lw/lse) or on plain
/// responsibilities `resp_dev` ([K][ld_resp], ld_resp >= n_pad), all-reduces, leaves [K*F stats, ll_sum] in stats_host.
/// A weighted block's responsibilities are multiplied by the rows' weights on the way (by the self-normalising kernel while it
/// stages, else into wresp; the source is not changed) unless `use_weights` is false (mlhip_xxt_xy: its rows are not an EM sample).
void run_mstats(mlhip_data* dt, const EmRoute& r, int K, int mode, const double* resp_dev, size_t ld_resp, bool with_ll,
                bool collect = true, bool use_weights = true);

double log_two_pi();

double ll_from_stats(const mlhip_data* dt, int K);

/// What every entry point on a data handle checks first: a context with a handle of its own -- a single context (made current) with a
/// block uploaded to it, or a device group's with a block uploaded through the group -- and K >= 1.
void check_call(mlhip_ctx* ctx, mlhip_data* dt, uint32_t K);

/// Ratio (mean offset from the shared shift)^2 / variance above which a component's covariance is recomputed about its
/// own mean. The one-GEMM statistics share one shift (the global mean), so Sigma_k = M2'/S0 - m m^T cancels
/// ~log10(ratio) digits: measured relative error ~3e-15 * ratio. 1e4 keeps every covariance within ~3e-11 of the
/// two-pass form the reference uses (ML/EM.cpp:245-250). MLHIP_REFINE_RATIO overrides; <= 0 disables the refinement.
double refine_ratio();

/// Second statistics pass for ONE component with the shift at that component's new mean (K = 1 launch of the same
/// kernels on column k of the responsibilities of the last pass), all-reduced like the first; replaces covariance k
/// (and adds the tiny mean correction). Tight clusters far from the global mean need it; the headline shapes never do.
void refine_component(mlhip_data* dt, const EmRoute& r, int k, double* mean_k, double* cov_k);

void finalize_out(mlhip_data* dt, const EmRoute& r, int K, double* mixing_out, double* means_out, double* cov_out);

/// One diagonal-covariance EM iteration's device work (em_diag.hip) with the statistics shift at `shift_dev`; leaves the
/// all-reduced [K * (2d+1) statistics, ll_sum] in stats_host. The records must already be in params_dev.
void run_diag_kernel(mlhip_data* dt, const EmRoute& r, int K, const double* shift_dev, bool collect = true,
                     const DevBuf* records = nullptr);

void ensure_km_workspace(mlhip_data* dt, int K);

KmBlock km_block(mlhip_data* dt, const KmRoute& r, int K);

/// Host centroids [K][d] -> the device table km_cent [K][D] (padded coordinates zero).
void km_upload_centroids(mlhip_data* dt, int K, const KmBlock& b, const double* centroids);

/// Assignment (+ optional accumulation) against the table in km_cent, partials reduced into km_out =
/// [inertia, changed, counts, sums] and summed across ranks there when the all-reduce works on device memory.
/// `weighted`: the assignment runs with accumulate = 0 and the weighted sweep (the weighted form of device/kmeans.hip's update sweep) follows it: km_out then
/// holds the weighted inertia, the row count n_changed, the weighted counts and sums sum_i w_i x_i (ensure_km_weighted first).
void km_launch(mlhip_data* dt, const KmRoute& r, int K, const KmBlock& b, bool accumulate, double* min_dist_out, bool weighted = false);

/// km_out -> km_host (`count` doubles), summed across ranks on the host when the all-reduce works on host memory.
void km_fetch(mlhip_data* dt, size_t count);

/// Assignment (+ optional accumulation); leaves all-reduced [inertia, changed, counts, sums] in km_host.
void run_kmeans(mlhip_data* dt, const KmRoute& r, int K, const double* centroids, bool accumulate, double* min_dist_out = nullptr,
                bool weighted = false);

/// What a weighted K-means call on a block with weights attached needs on top of ensure_km_workspace: the factors of the
/// weighted exact sums (derived from the largest weight of the whole sample, exchanged across ranks like the column maxima; cached
/// until mlhip_data_set_weights), the partial-block scratch sized for 3d + 3 words per cluster. DomainError when max w * max|x_j|
/// overflows for some dimension j (the handle stays usable).
void ensure_km_weighted(mlhip_data* dt, int K);

/// update_step's closing arithmetic on the host (ML/KMeans.cpp:180-192 as sums / counts; empty cluster -> origin, :184).
void km_close_host(const double* r, int K, int d, double* counts, double* centroids_out);

/// The step loop of KMeans::fit_once (ML/KMeans.cpp:80-110). With the all-reduce on device memory (or none) the centroid
/// table never leaves the device between trips: sums -> means -> next table by launch_kmeans_close, one read-back per trip
/// for the two stopping tests. With a host-memory all-reduce (gloo rehearsals) every trip goes through run_kmeans.
/// `weighted`: every trip is a weighted step (km_launch); never the resident one-launch loop.
void km_iterate(mlhip_data* dt, const KmRoute& route, int K, double* centroids, double* old_centroids, uint32_t max_steps, double atol,
                uint32_t* steps_done, int* converged, double* inertia, double* counts, bool weighted = false);

/// The covariance array of `mode` as K full covariance matrices (host::covariances_as_full).
std::vector<double> as_full(Covariance mode, int K, int d, const double* covariance);

/// One full-covariance EM iteration with the closing arithmetic on the HOST (the body of mlhip_em_step).
void em_step_full(mlhip_data* data, const EmRoute& r, int K, const double* mixing, const double* means, const double* covariances,
                  double* log_likelihood, double* mixing_out, double* means_out, double* covariances_out);

/// Records of a diagonal-covariance parameter set -> `target` (padded to whole 16-component row blocks with neutral records).
void upload_diag_records(mlhip_data* data, int K, const double* mixing, const double* means, const double* variances, DevBuf& target);

/// Same cancellation guard as the full-covariance path (refine_ratio): a component whose mean sits far from the shared shift,
/// measured in its own standard deviations, gets its variances from a second pass with the shift at its new mean (the E part of
/// that pass re-evaluates the SAME input parameters, still in params_dev).
void refine_diag(mlhip_data* data, const EmRoute& r, int K, const double* mixing_out, double* means_out, double* variances_out);

void em_step_diag(mlhip_data* data, const EmRoute& r, int K, const double* mixing, const double* means, const double* variances,
                  double* log_likelihood, double* mixing_out, double* means_out, double* variances_out);

/// The K = 1, r = 1 statistics pass (what mlhip_sample_covariance runs): leaves the all-reduced packed sum_i w_i xt_i xt_i^T in
/// stats_host. Resizes the EM workspace to K = 1 (E-step results on the handle are dropped).
void run_total_scatter(mlhip_data* data);

/// One tied-covariance EM iteration (the body of mlhip_em_step_tied): cov / cov_out hold d*d doubles.
void em_step_tied(mlhip_data* data, const ModeRoute& r, int K, const double* mixing, const double* means, const double* cov,
                  double* log_likelihood, double* mixing_out, double* means_out, double* cov_out);

/// One EM iteration in the mode of `r` with the closing arithmetic on the host: em_step_full, em_step_diag or em_step_tied. The
/// covariance arrays hold covariance_doubles(r.mode, K, d) doubles.
void em_step(mlhip_data* data, const ModeRoute& r, int K, const double* mixing, const double* means, const double* covs,
             double* log_likelihood, double* mixing_out, double* means_out, double* covs_out);

/// ML/EM.cpp:161-168: from the second trip on, |ll - ll_old| < atol + rtol max(|ll_old|, |ll|) stops the loop.
struct ConvergenceTest {
    double atol, rtol;
    uint32_t* steps_done;
    int* converged;
    double* log_likelihood;
    double* history;
    double old_ll = -HUGE_VAL;
    bool operator()(uint32_t step, double ll)
    {
        if (history) history[step] = ll;
        *log_likelihood = ll;
        *steps_done = step + 1;
        if (step > 0) {
            const double change = std::fabs(ll - old_ll);
            if (change < atol + rtol * std::max(std::fabs(old_ll), std::fabs(ll))) { *converged = 1; return true; }
        }
        old_ll = ll;
        return false;
    }
};

/// The loop of EM::fit (ML/EM.cpp:143-170) with everything between two convergence tests on the device (em_loop.cpp): E-step,
/// statistics, all-reduce, closing arithmetic + next records (em_close.hip); per iteration the host reads back 1 + 2K doubles (log-
/// likelihood sum, refinement flags, FOLD criterion) and decides. A flagged component (far, tight cluster) sends that one
/// iteration through the host closing with its refinement pass, exactly as mlhip_em_step would. Without device closing
/// (the route's device_close; tied covariances always) the whole loop runs through em_step. Resolves mode_route(data, K, mode) itself;
/// covs: covariance_doubles(mode, K, d) doubles.
void em_iterate(mlhip_data* data, Covariance mode, int K, double* mixing, double* means, double* covs, uint32_t max_steps, double atol,
                double rtol, uint32_t* steps_done, int* converged, double* log_likelihood, double* history);

/// The batched loop of mlhip_em_iterate_restarts (em_restarts.cpp): restarts [0, R) of full-covariance EM on a single rank's block;
/// arrays as in mlhip.h. Restarts it could not finish itself (a refinement flag) are run through em_iterate from their starts.
/// Leaves the E-step state of restart *best on the handle.
void em_iterate_restarts_batched(mlhip_data* data, const RestartsRoute& route, int K, uint32_t R, double* mixing, double* means, double* covs,
                                 uint32_t max_steps, double atol, double rtol, uint32_t* steps_done, int* converged, double* log_likelihood,
                                 double* history, uint32_t* best);
/// The selection rule of mlhip_em_select_restart (mlhip.h).
uint32_t select_restart(uint32_t R, const double* log_likelihood, const int* converged);

/// The all-reduce hook of a context that owns an RCCL communicator: one ncclAllReduce(double, sum), in place, on the
/// context's stream -- ordered with the kernels before it and the copies after it, no host synchronisation.
int rccl_allreduce_hook(void* user, double* buf, size_t count, int on_device, void* stream);

void drop_rccl(mlhip_ctx* ctx);

void init_rccl(mlhip_ctx* ctx, const ncclUniqueId& id, int world_size, int rank);

/// A failed C-ABI status (with the calling thread's message) as the exception `guarded` maps back to it: the device group calls
/// the entry points of its shards on worker threads and hands their failures to the thread of the caller.
[[noreturn]] void throw_status(int status, const std::string& message);
inline void check_status(int status) { if (status != MLHIP_OK) throw_status(status, g_error); }

/// mlhip_ctx_create for one device, without the environment defaults (context.cpp).
mlhip_ctx* create_single_context(int device_id);
void destroy_single_context(mlhip_ctx* ctx);

// ---- device group (group.cpp): one caller-visible context over n shards. An entry point called with a group's context checks its
// arguments as for a single context (check_call; host arrays are the caller's WHOLE arrays, mlhip_data::rows() rows) and then calls
// itself on every shard through fan_out; results are what a single context would return.

/// One shard's side of a fanned-out call: its ordinary context, its part of the block, its rows of the caller's sample, and the
/// three rules by which the caller's arguments become the shard's.
struct Shard {
    int index = 0;
    mlhip_ctx* ctx = nullptr;
    mlhip_data* part = nullptr;
    uint64_t first_row = 0, n_rows = 0;

    /// The shard's rows of a per-row array of the caller's, `ld` values per row (null stays null).
    template <class T> T* rows(T* p, int64_t ld = 1) const { return p ? p + (int64_t)first_row * ld : nullptr; }
    /// An output every shard computes alike (all-reduced statistics behind it): the caller's array on shard 0, scratch of `count`
    /// values elsewhere (null stays null) -- starting from `init` where the array is in/out. `init` is a copy the entry point made
    /// BEFORE the fan-out, as is every input that may alias an output: shard 0 writes the caller's arrays while the others still read
    /// (so a call that fails on some shard leaves the caller's output ARRAYS unspecified).
    template <class T> T* replicated(T* out, size_t count, const T* init = nullptr)
    {
        if (index == 0 || !out) return out;
        T* mine = scratch_of<T>(count);
        if (init) std::copy(init, init + count, mine);
        return mine;
    }
    /// A scalar output: every shard writes one of its own, and shard 0's goes to the caller once ALL shards have succeeded (null stays
    /// null). `stopped_at` ("iterations", "steps"): the call fails unless every shard's value is the same.
    template <class T> T* scalar(T* out, const char* stopped_at = nullptr)
    {
        if (!out) return out;
        T* mine = scratch_of<T>(1);
        scalars.push_back({out, mine, sizeof(T), stopped_at});
        return mine;
    }

    struct Scalar { void* caller; const void* mine; size_t bytes; const char* stopped_at; };
    std::vector<Scalar> scalars;                                  // (in the order of the call's arguments: the same on every shard)
    std::vector<std::unique_ptr<unsigned char[]>> scratch;

private:
    template <class T> T* scratch_of(size_t count)
    {
        static_assert(std::is_trivial<T>::value && alignof(T) <= alignof(std::max_align_t), "plain values only");
        scratch.emplace_back(new unsigned char[count * sizeof(T)]());
        return reinterpret_cast<T*>(scratch.back().get());
    }
};

/// f(shard) on every shard's thread (ShardTeam: a failure of one shard fails the call on the caller's thread, the group recovers
/// before the next one); f returns the status of the shard's own mlhip_* call.
void fan_out(mlhip_ctx* ctx, mlhip_data* data, const std::function<int(Shard&)>& f);
/// The same over a row split given by the caller (first_row: shards + 1 entries) -- a call that has rows but no block yet
/// (mlhip_em_sample); `data` may be null, the shards' `part` is null then.
void fan_out_rows(mlhip_ctx* ctx, const std::vector<uint64_t>& first_row, mlhip_data* data, const std::function<int(Shard&)>& f);
/// The contiguous, balanced row shards that tile [0, n): shard s holds rows [first[s], first[s + 1]) (the split of
/// ml_amd.dist.shard_bounds, so that a group reproduces the multi-process job of the same size).
std::vector<uint64_t> balanced_rows(uint64_t n, int shards);
/// f on the block itself -- a "shard" that is the whole of it: the caller's context, its block, first row 0 --, or, with a group's
/// context, on every shard's part on that shard's thread with its device made current. f throws as an entry point's body does.
/// (A shard's checks are the outer call's: check_call and the argument checks that passed for the group hold for each of its parts.)
void on_block_or_shards(mlhip_ctx* ctx, mlhip_data* data, const std::function<void(Shard&)>& f);

// ---- the chunked pass of the conditioning calls (em_condition.cpp): mlhip_em_conditional_means / _samples / _variances / _cdfs /
// _quantiles all run the marginal mixture's E-step in its exact form on chunks of whole tiles and their own kernel behind every chunk.

/// The scratch of an exact-form, LSE-writing E-step on chunks of at most `chunk` rows (whole tiles) of a block, and its launch: what
/// the conditioning pass and the composed route of mlhip_em_score run. The buffers are the call's own, from the handle's pool.
struct ChunkEstep {
    DevBuf lw, lse, ll;                                          // K x chunk log-responsibilities, their log-sum-exp, the partials
    uint32_t chunk = 0;
    explicit ChunkEstep(mlhip_data* dt) : lw(&dt->pool), lse(&dt->pool), ll(&dt->pool) {}
    void reserve(int K, uint32_t chunk_rows);
    /// The E-step kernel of `em` (fold = 0, with_lse = 1) for rows [row, row + rows) of the block on `records`; rows <= chunk.
    void launch(mlhip_data* dt, const EmRoute& em, int K, const DevBuf& records, uint32_t row, uint32_t rows);
};

/// A mixture conditioned on observed coordinates as every conditioning call takes it (mlhip_em_condition's outputs): the marginal
/// mixture over x_O and, per component, the regression of x_M on x_O.
struct ConditionedModel {
    int K, dM;
    const double *mixing, *means_observed, *covs_observed, *maps, *means_missing;
};
/// Writes the `tail` doubles (+0.0 as given) behind record k's [mu_O | mu_M | A^T].
using ConditionTail = std::function<void(int k, double* tail)>;
/// The conditioning kernels' table on the host: K records [mu_O | mu_M | A^T | tail] in the paddings of `kernel` (device.hpp
/// condition_pad): +0.0, and -0.0 in the rows of A^T beyond dO (a padded coordinate's term is fma(-0.0, +0.0, t) = t for every t, a t
/// of -0.0 included: device/em_condition_common.hpp). `fill` may be empty where `tail` is 0.
std::vector<double> condition_table(int kernel, const ConditionedModel& m, int dO, size_t tail, const ConditionTail& fill);

/// One conditioning call on one block. The constructor builds the marginal mixture's E-step records (always the exact form: no FOLD),
/// uploads the table and reserves the E-step's scratch; run() walks the chunks. Every buffer is the call's own, taken from the
/// handle's pool: the handle's E-step state, weights, ridge and label history stay as they were.
class ConditionPass {
public:
    /// `unsupported`: what to say where `kernel` has no padding for (dO, dM).
    ConditionPass(mlhip_data* dt, const ConditionedModel& m, const EmRoute& em, int kernel, uint32_t chunk_rows, size_t tail,
                  const ConditionTail& fill, const char* unsupported);
    /// Per chunk of rows: the E-step, then behind(c, row) with c the chunk that starts at `row` (c.n rows; padded_samples(c.n) <=
    /// chunk: the chunk is whole tiles) -- the caller launches its kernel and downloads what it wrote --, then log_density's rows where
    /// that is not null: lse less dO log(2 pi) / 2, the constant the kernels' lw leave out. Ends with the call's one ctx->sync().
    void run(double* log_density, const std::function<void(const ConditionChunk& c, uint32_t row)>& behind);
    /// rows x width elements at `src` on the device to rows `ld` elements apart on the host (a leading dimension above the width: the
    /// rows come down contiguous and are spread by the CPU). The copy waits for the stream: the source is free for the next launch.
    template <class T> void download_rows(T* dst, int64_t ld, const void* src, uint32_t rows, size_t width)
    {
        const bool spread = ld != (int64_t)width;
        if (spread) packed_.resize(sizeof(T) * rows * width);
        char* to = spread ? packed_.data() : reinterpret_cast<char*>(dst);
        download_columns(dt_->ctx, to, 0, static_cast<const char*>(src), 0, sizeof(T) * width * rows, 1);
        if (spread)
            for (uint32_t i = 0; i < rows; ++i) std::memcpy(dst + (int64_t)i * ld, to + sizeof(T) * width * i, sizeof(T) * width);
    }

private:
    mlhip_data* dt_;
    EmRoute em_;
    ConditionChunk c_{};
    DevBuf records_, work_, table_;
    PinnedBuf staging_;
    std::vector<double> host_table_;                             // (the upload reads it until the stream has been waited for)
    ChunkEstep estep_;
    std::vector<char> packed_;
};

/// The body of mlhip_em_conditional_means on one block (em_condition.cpp). `resp` (rows x K, `ld_resp` >= K doubles apart; may be null):
/// the shares r_k = exp_nonpos(lw_k - lse) the conditioning kernel weights with, formed by em_resp_kernel from the same chunk's lw / lse
/// (mlhip_em_impute's composed route asks for them).
void em_conditional_means(mlhip_data* dt, const ConditionedModel& m, double* out, int64_t ld_out, double* log_density, double* resp,
                          int64_t ld_resp);

// What is not a plain fan-out:
namespace grp {
mlhip_ctx* create(int n_shards, const int* device_ids);
void destroy(mlhip_ctx* ctx);
void synchronize(mlhip_ctx* ctx);
int shard_count(const mlhip_ctx* ctx);
mlhip_ctx* shard_context(const mlhip_ctx* ctx, int shard);
const char* reduce_kind(const mlhip_ctx* ctx);
mlhip_data* upload(mlhip_ctx* ctx, const double* x, bool on_device, uint32_t d, uint64_t n, int64_t ld);
/// The group's handle over n rows from parts the shards make themselves: `source` runs on every shard's thread with that shard's
/// context and its rows [first_row, first_row + rows) of the balanced split and returns the shard's block (upload: upload_common on
/// its rows of the caller's block; mlhip_em_sample_data: the rows the shard generated on its own GPU).
using PartSource = std::function<mlhip_data*(mlhip_ctx* shard, uint64_t first_row, uint64_t rows)>;
mlhip_data* upload_parts(mlhip_ctx* ctx, uint32_t d, uint64_t n, const PartSource& source);
/// (the shards one after the other: they continue each other's running means)
void random_partition_means(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, const uint32_t* order, const uint32_t* offsets, double* means,
                            double* sizes);
/// (every shard the part of the row range it holds)
void em_responsibilities(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, double* resp, int64_t ldr, uint64_t first, uint64_t count);
void timing_get(mlhip_ctx* ctx, const char* name, double* avg_ms, uint64_t* launches);
}  // namespace grp

}  // namespace mlhip_rt
