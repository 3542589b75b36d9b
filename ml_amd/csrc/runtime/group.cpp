// Device group: ONE caller-visible context over n shards (`mlhip_ctx_create(n_devices, device_ids)`, "one host
// thread drives all devices"), so that the reference's one-process API -- bool EM::fit(Eigen::Ref<const MatrixXd>) (ML/EM.cpp:91),
// KMeans::fit (ML/KMeans.cpp:25) -- reaches every GPU of the node without a launcher. The caller's d x N block is row-sharded over
// the shards at upload; every entry point of mlhip.h called with the group's context fans out to the shards' ordinary contexts, one
// persistent host thread per shard, and the shards' statistics meet in the per-iteration all-reduce exactly as the ranks of a
// multi-process job do (the shard contexts carry world_size = n, rank = shard, and run the unchanged per-context code):
//   * shards on distinct GPUs: one RCCL communicator per shard from ncclCommInitAll, ncclAllReduce on the shard's stream;
//   * otherwise (several shards on one GPU -- how a one-GPU box rehearses the 8-GPU configurations at full size -- or
//     MLHIP_GROUP_REDUCE=direct): an in-process all-reduce -- every shard copies its buffer into its own slot, waits (on its stream) for
//     the other shards' slots, and sums all slots in shard order with the same kernel: bit-identical on every shard, reproducible from
//     run to run, no library involved (slots on other GPUs are read through peer access over xGMI).
#include "internal.hpp"
#include "shard_team.hpp"

struct mlhip_group {
    int n = 0;
    std::vector<mlhip_ctx*> shard;      // owned: ordinary contexts with world_size = n, rank = shard index
    std::vector<int> devices;
    enum Reduce { kNone, kRccl, kDirect } reduce = kNone;
    std::string rccl_error;             // why an automatic choice fell back from RCCL to the in-process sum (empty: it did not)
    std::string direct_kind_text;       // "group-direct (RCCL unavailable: ...)" for mlhip_ctx_reduce_kind
    ShardTeam team;                     // the shard threads, their barrier, the failure protocol (shard_team.hpp)
    std::atomic<bool> dead{false};      // RCCL mode, after a failure: the communicators were aborted, the group can only be closed
    // ---- in-process all-reduce (kDirect): the protocol is SlotAllreduce (shard_team.hpp); these are the device objects it moves --
    // two generations of one slot per shard, an event pair per slot
    struct DeviceOps;
    std::vector<DevBuf> slot[2];
    std::vector<hipEvent_t> ready[2], consumed[2];
    mlhip_rt::SlotAllreduce<DeviceOps> exchange;
    // ---- test hooks, read ONCE when the group is created (tests/test_gpu_group.py): MLHIP_GROUP_TEST_PERTURB=s -- shard s's copy of
    // a statistics sum differs in its last digits (the checksum exchange must fail the fit); MLHIP_GROUP_TEST_FAIL=s:k -- shard s
    // fails, alone, in its k-th all-reduce (the others must come back with its error instead of waiting for it)
    int test_perturb_shard = -1, test_fail_shard = -1;
    uint64_t test_fail_at = 0;
    std::vector<uint64_t> allreduces;   // per shard, counted for the hook above
};

/// SlotAllreduce's device operations: shard r's stream, the slots' buffers and events. (Slots on other GPUs are read through peer access.)
struct mlhip_group::DeviceOps {
    mlhip_group* g;
    hipStream_t stream(int r) const { return g->shard[(size_t)r]->stream; }
    void sync_stream(int r) { HIP_CHECK(hipStreamSynchronize(stream(r))); }
    void reserve_slots(int r, size_t doubles) { for (int p = 0; p < 2; ++p) g->slot[p][(size_t)r].reserve(sizeof(double) * doubles); }
    void release_slots(int r) { for (int p = 0; p < 2; ++p) g->slot[p][(size_t)r].release(); }
    void wait_consumed(int r, int p, int q) { HIP_CHECK(hipStreamWaitEvent(stream(r), g->consumed[p][(size_t)q], 0)); }
    void publish(int r, int p, const double* buf, size_t count)
    {
        HIP_CHECK(hipMemcpyAsync(g->slot[p][(size_t)r].p, buf, sizeof(double) * count, hipMemcpyDeviceToDevice, stream(r)));
        HIP_CHECK(hipEventRecord(g->ready[p][(size_t)r], stream(r)));
    }
    void wait_ready(int r, int p, int q) { HIP_CHECK(hipStreamWaitEvent(stream(r), g->ready[p][(size_t)q], 0)); }
    void sum(int r, int p, double* buf, size_t count)
    {
        GroupSumSlots slots{};
        for (int q = 0; q < g->n; ++q) slots.p[q] = g->slot[p][(size_t)q].as<double>();
        launch_group_sum(slots, g->n, buf, count, stream(r));
        HIP_CHECK(hipGetLastError());
    }
    void mark_consumed(int r, int p) { HIP_CHECK(hipEventRecord(g->consumed[p][(size_t)r], stream(r))); }
};

namespace mlhip_rt {
namespace {

/// After a failed task the shards' streams may hold half an all-reduce and -- when a slot growth was interrupted -- the shards may
/// disagree on the slots' capacity: SlotAllreduce::recover (every shard drains its stream, all meet, every shard drops its slots,
/// all meet again).
void recover_shard(mlhip_group* g, int s)
{
    mlhip_ctx* c = g->shard[(size_t)s];
    (void)hipSetDevice(c->device);
    mlhip_group::DeviceOps ops{g};
    if (g->exchange.active()) {
        g->exchange.recover(ops, g->team.barrier, s);
    } else {
        (void)hipStreamSynchronize(c->stream);
        g->team.barrier.wait();
    }
}

/// A shard failed on its own (out of memory, a HIP error): the others may be INSIDE ncclAllReduce + hipStreamSynchronize waiting for
/// it, where no barrier of ours can reach them. RCCL mode: abort every communicator -- the blocked streams return with an error --
/// and mark the group dead (aborted communicators cannot be used again; the caller creates a new group).
void cancel_collectives(mlhip_group* g)
{
    if (g->reduce != mlhip_group::kRccl) return;
    g->dead.store(true);
    try {
        const Rccl& r = Rccl::get();
        if (!r.CommAbort) return;
        for (mlhip_ctx* c : g->shard)
            if (c->comm) (void)r.CommAbort(c->comm);
    } catch (...) {
    }
}

void run_on_shards(mlhip_group* g, const std::function<void(int)>& f)
{
    if (g->dead.load())
        throw std::runtime_error("this device group failed inside an RCCL collective and its communicators were aborted: close it "
                                 "(mlhip_ctx_destroy) and create a new one");
    g->team.run(f);
}

/// The all-reduce hook of a shard in kDirect mode (see the head of this file). Every shard calls it with the same count, in the same
/// order, each from its own thread with its own device current.
int direct_allreduce_hook(void* user, double* buf, size_t count, int on_device, void* stream_)
{
    auto* c = static_cast<mlhip_ctx*>(user);
    mlhip_group* g = c ? c->member_of : nullptr;
    if (!g || !on_device || static_cast<hipStream_t>(stream_) != c->stream) return 1;
    try {
        const int r = c->shard;
        if (g->test_fail_shard == r && ++g->allreduces[(size_t)r] == g->test_fail_at)
            throw std::runtime_error("injected failure of one shard (MLHIP_GROUP_TEST_FAIL)");
        mlhip_group::DeviceOps ops{g};
        g->exchange.allreduce(ops, g->team.barrier, r, buf, count);
        if (g->test_perturb_shard == r && count > 64) {
            // (tests only) this shard's copy of a statistics sum is made to differ in its last digits: the end-of-fit checksum
            // exchange of the shards must catch it (short vectors -- that exchange itself -- are left alone)
            double v = 0;
            HIP_CHECK(hipMemcpyAsync(&v, buf, sizeof v, hipMemcpyDeviceToHost, c->stream));
            HIP_CHECK(hipStreamSynchronize(c->stream));
            v *= 1.0 + 1e-12;
            HIP_CHECK(hipMemcpyAsync(buf, &v, sizeof v, hipMemcpyHostToDevice, c->stream));
            HIP_CHECK(hipStreamSynchronize(c->stream));
        }
        return 0;
    } catch (const std::exception& e) {
        g_error = e.what();
        return 1;
    }
}

mlhip_group* group_of(const mlhip_ctx* ctx)
{
    require(ctx && ctx->group, "not a device group context");
    return ctx->group;
}

/// GPUs `from_devices` read the memory of GPU `to_device` from now on -- or, where one of them cannot, the call is refused (a kernel
/// that reads memory it cannot reach faults, and a fault can take the node's GPUs down). `remedy`: what the caller can do instead.
void enable_peer_access(const std::vector<int>& from_devices, int to_device, const char* remedy)
{
    for (int dev : from_devices) {
        if (dev == to_device) continue;
        int can = 0;
        HIP_CHECK(hipDeviceCanAccessPeer(&can, dev, to_device));
        if (!can)
            throw Unsupported("device group: GPU " + std::to_string(dev) + " cannot read the memory of GPU " + std::to_string(to_device) +
                              " (no peer access): " + remedy);
        HIP_CHECK(hipSetDevice(dev));
        const hipError_t e = hipDeviceEnablePeerAccess(to_device, 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) HIP_CHECK(e);
        (void)hipGetLastError();
    }
}

std::vector<int> distinct_devices(const mlhip_group* g)
{
    std::vector<int> unique;
    for (int dev : g->devices)
        if (std::find(unique.begin(), unique.end(), dev) == unique.end()) unique.push_back(dev);
    return unique;
}

}  // namespace

[[noreturn]] void throw_status(int status, const std::string& message)
{
    switch (status) {
    case MLHIP_E_INVALID_ARGUMENT: throw InvalidArgument(message);
    case MLHIP_E_DOMAIN: throw DomainError(message);
    case MLHIP_E_NO_DEVICE: throw NoDevice(message);
    case MLHIP_E_UNSUPPORTED: throw Unsupported(message);
    default: throw std::runtime_error(message);
    }
}

std::vector<uint64_t> balanced_rows(uint64_t n, int shards)
{
    std::vector<uint64_t> first((size_t)shards + 1, 0);
    const uint64_t base = n / (uint64_t)shards, rem = n % (uint64_t)shards;
    for (int s = 0; s < shards; ++s) first[(size_t)s + 1] = first[(size_t)s] + base + ((uint64_t)s < rem ? 1 : 0);
    return first;
}

void fan_out(mlhip_ctx* ctx, mlhip_data* data, const std::function<int(Shard&)>& f)
{
    fan_out_rows(ctx, data->first_row, data, f);
}

void fan_out_rows(mlhip_ctx* ctx, const std::vector<uint64_t>& first_row, mlhip_data* data, const std::function<int(Shard&)>& f)
{
    mlhip_group* g = group_of(ctx);
    std::vector<Shard> view((size_t)g->n);
    for (int s = 0; s < g->n; ++s) {
        Shard& sh = view[(size_t)s];
        sh.index = s;
        sh.ctx = g->shard[(size_t)s];
        sh.part = data ? data->parts[(size_t)s] : nullptr;
        sh.first_row = first_row[(size_t)s];
        sh.n_rows = first_row[(size_t)s + 1] - sh.first_row;
        sh.scratch.reserve(8);                                // (so that the shard's thread allocates its outputs only)
        sh.scalars.reserve(4);
    }
    run_on_shards(g, [&](int s) { check_status(f(view[(size_t)s])); });
    const std::vector<Shard::Scalar>& first = view[0].scalars;
    for (const Shard& sh : view)
        for (size_t i = 0; i < first.size(); ++i)
            if (first[i].stopped_at && std::memcmp(first[i].mine, sh.scalars[i].mine, first[i].bytes) != 0)
                throw std::runtime_error(std::string("device group: the shards stopped at different ") + first[i].stopped_at);
    for (const Shard::Scalar& v : first) std::memcpy(v.caller, v.mine, v.bytes);
}

namespace grp {

mlhip_ctx* create(int n_shards, const int* device_ids)
{
    require(n_shards >= 1 && n_shards <= kGroupMaxShards, "a device group has 1 to 64 shards");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        throw NoDevice("no HIP device available: this library has no CPU fallback (needs an AMD GPU, built for gfx950)");
    auto* g = new mlhip_group;
    auto* ctx = new mlhip_ctx;
    ctx->group = g;
    try {
        g->n = n_shards;
        bool distinct = true;
        for (int s = 0; s < n_shards; ++s) {
            const int dev = device_ids ? device_ids[s] : s % count;
            require(dev >= 0 && dev < count, "device group: no such GPU");
            for (int q : g->devices) distinct = distinct && q != dev;
            g->devices.push_back(dev);
        }
        for (int s = 0; s < n_shards; ++s) {
            mlhip_ctx* c = create_single_context(g->devices[(size_t)s]);
            g->shard.push_back(c);
            c->member_of = g;
            c->shard = s;
            c->stage_bytes = size_t(32) << 20;             // n x 4 staging buffers: keep the pinned footprint small
        }
        ctx->device = g->devices[0];
        ctx->num_cus = g->shard[0]->num_cus;
        if (n_shards > 1) {
            // how the shards' statistics meet: RCCL between distinct GPUs, the in-process sum otherwise
            const char* env = std::getenv("MLHIP_GROUP_REDUCE");
            const std::string want = env ? env : "";
            require(want.empty() || want == "rccl" || want == "direct", "MLHIP_GROUP_REDUCE must be rccl or direct");
            bool rccl = want == "rccl" || (want.empty() && distinct && mlhip_rccl_available());
            if (rccl && !distinct) throw Unsupported("device group: RCCL refuses two ranks on one GPU (use MLHIP_GROUP_REDUCE=direct)");
            if (rccl) {
                const Rccl& r = Rccl::get();
                if (!r.CommInitAll) throw std::runtime_error("librccl has no ncclCommInitAll");
                std::vector<ncclComm_t> comms((size_t)n_shards, nullptr);
                const ncclResult_t rc = r.CommInitAll(comms.data(), n_shards, g->devices.data());
                if (rc != ncclSuccess) {
                    if (want == "rccl") r.check(rc, "ncclCommInitAll");
                    rccl = false;                            // (auto: fall back to the in-process sum -- and say so, once)
                    g->rccl_error = std::string("ncclCommInitAll: ") + r.GetErrorString(rc);
                    g->direct_kind_text = "group-direct (RCCL unavailable: " + g->rccl_error + ")";
                    std::fprintf(stderr, "[mlhip] device group: RCCL between the %d GPUs is not available (%s); the shards' statistics are "
                                         "summed in-process over peer access instead (MLHIP_GROUP_REDUCE=rccl makes this an error)\n",
                                 n_shards, g->rccl_error.c_str());
                } else {
                    for (int s = 0; s < n_shards; ++s) {
                        mlhip_ctx* c = g->shard[(size_t)s];
                        c->comm = comms[(size_t)s];
                        c->reduce_fn = rccl_allreduce_hook;
                        c->reduce_user = c;
                    }
                    g->reduce = mlhip_group::kRccl;
                }
            }
            if (!rccl) {
                const std::vector<int> unique = distinct_devices(g);
                for (int dev : unique)
                    enable_peer_access(unique, dev, "the in-process all-reduce needs it; use RCCL: MLHIP_GROUP_REDUCE=rccl");
                for (int p = 0; p < 2; ++p) {
                    g->slot[p].resize((size_t)n_shards);
                    g->ready[p].assign((size_t)n_shards, nullptr);
                    g->consumed[p].assign((size_t)n_shards, nullptr);
                }
                g->exchange.init(n_shards);
                for (int s = 0; s < n_shards; ++s) {
                    mlhip_ctx* c = g->shard[(size_t)s];
                    c->use();
                    for (int p = 0; p < 2; ++p) {
                        HIP_CHECK(hipEventCreateWithFlags(&g->ready[p][(size_t)s], hipEventDisableTiming));
                        HIP_CHECK(hipEventCreateWithFlags(&g->consumed[p][(size_t)s], hipEventDisableTiming));
                    }
                    c->reduce_fn = direct_allreduce_hook;
                    c->reduce_user = c;
                }
                g->reduce = mlhip_group::kDirect;
            }
            for (mlhip_ctx* c : g->shard) {
                c->reduce_on_device = 1;
                c->world_size = n_shards;
                c->rank = c->shard;
            }
            host::set_host_ranks(n_shards);                 // the shards' host threads share this machine's cores
        }
        // (test hooks: read once, here -- never on the path of an all-reduce)
        if (const char* e = std::getenv("MLHIP_GROUP_TEST_PERTURB")) g->test_perturb_shard = std::atoi(e);
        if (const char* e = std::getenv("MLHIP_GROUP_TEST_FAIL")) {
            g->test_fail_shard = std::atoi(e);
            const char* colon = std::strchr(e, ':');
            g->test_fail_at = colon ? std::strtoull(colon + 1, nullptr, 10) : 1;
        }
        g->allreduces.assign((size_t)n_shards, 0);
        g->team.start(n_shards, [g](int s) { recover_shard(g, s); }, [g](int) { cancel_collectives(g); });
    } catch (...) {
        destroy(ctx);
        throw;
    }
    return ctx;
}

void destroy(mlhip_ctx* ctx)
{
    if (!ctx) return;
    mlhip_group* g = ctx->group;
    if (g) {
        g->team.stop();
        if (g->n > 1) host::set_host_ranks(1);               // (the shards' share of the host cores was a property of this group)
        for (size_t s = 0; s < g->shard.size(); ++s) {
            mlhip_ctx* c = g->shard[s];
            (void)hipSetDevice(c->device);
            if (c->stream) (void)hipStreamSynchronize(c->stream);
        }
        for (size_t s = 0; s < g->shard.size(); ++s) {
            mlhip_ctx* c = g->shard[s];
            (void)hipSetDevice(c->device);
            for (int p = 0; p < 2; ++p) {
                if (s < g->slot[p].size()) g->slot[p][s].release();
                if (s < g->ready[p].size() && g->ready[p][s]) (void)hipEventDestroy(g->ready[p][s]);
                if (s < g->consumed[p].size() && g->consumed[p][s]) (void)hipEventDestroy(g->consumed[p][s]);
            }
            destroy_single_context(c);                       // (drops the shard's RCCL communicator too)
        }
        delete g;
    }
    {
        std::lock_guard<std::mutex> lock(ctx->handles_m);
        for (mlhip_data* h : ctx->handles) h->ctx = nullptr;   // (group blocks that outlive the group: their parts are detached already)
        ctx->handles.clear();
    }
    delete ctx;
}

void synchronize(mlhip_ctx* ctx)
{
    for (mlhip_ctx* c : group_of(ctx)->shard) { c->use(); c->sync(); }
}

int shard_count(const mlhip_ctx* ctx) { return ctx->group ? ctx->group->n : 1; }

mlhip_ctx* shard_context(const mlhip_ctx* ctx, int shard)
{
    mlhip_group* g = group_of(ctx);
    require(shard >= 0 && shard < g->n, "no such shard");
    return g->shard[(size_t)shard];
}

const char* reduce_kind(const mlhip_ctx* ctx)
{
    if (ctx->group) {
        switch (ctx->group->reduce) {
        case mlhip_group::kRccl: return "group-rccl";
        case mlhip_group::kDirect:
            // (an automatic choice that fell back from RCCL carries the reason: the bench line shows it)
            return ctx->group->rccl_error.empty() ? "group-direct" : ctx->group->direct_kind_text.c_str();
        default: return "none";
        }
    }
    if (!ctx->reduce_fn) return "none";
    if (ctx->reduce_fn == rccl_allreduce_hook) return "rccl";
    return ctx->reduce_on_device ? "hook-device" : "hook-host";
}

mlhip_data* upload(mlhip_ctx* ctx, const double* x, bool on_device, uint32_t d, uint64_t n, int64_t ld)
{
    mlhip_group* g = group_of(ctx);
    require(x != nullptr || n == 0, "null data");
    require(d >= 1, "At least one dimension required");
    require(ld >= (int64_t)d, "ld must be >= d");
    if (padded_dim((int)d) < 0) throw Unsupported("dimension d > 4096 is not supported");
    if (on_device && n) {
        // a block already in device memory must be readable from every shard's GPU: its own GPU, or a peer with access enabled
        hipPointerAttribute_t attr{};
        if (hipPointerGetAttributes(&attr, x) != hipSuccess) { (void)hipGetLastError(); throw InvalidArgument("x_dev is not a device pointer"); }
        enable_peer_access(distinct_devices(g), attr.device, "upload the block from host memory");
    }
    return upload_parts(ctx, d, n, [&](mlhip_ctx* shard, uint64_t first_row, uint64_t rows) {
        return upload_common(shard, x ? x + (int64_t)first_row * ld : nullptr, on_device, d, rows, ld);
    });
}

mlhip_data* upload_parts(mlhip_ctx* ctx, uint32_t d, uint64_t n, const PartSource& source)
{
    mlhip_group* g = group_of(ctx);
    require(d >= 1, "At least one dimension required");
    auto* gd = new mlhip_data;
    try {
        gd->ctx = ctx;
        gd->d = (int)d;
        gd->D = padded_dim((int)d);
        if (gd->D < 0) throw Unsupported("dimension d > 4096 is not supported");
        gd->n_global = n;
        gd->n = (uint32_t)std::min<uint64_t>(n, 0xffffffffull);
        gd->parts.assign((size_t)g->n, nullptr);
        gd->first_row = balanced_rows(n, g->n);
        run_on_shards(g, [&](int s) {
            const uint64_t lo = gd->first_row[(size_t)s], rows = gd->first_row[(size_t)s + 1] - lo;
            gd->parts[(size_t)s] = source(g->shard[(size_t)s], lo, rows);
        });
        gd->shift = gd->parts[0]->shift;
        require(gd->parts[0]->n_global == n, "device group: the shards disagree on the sample size");
    } catch (...) {
        delete gd;
        throw;
    }
    ctx->adopt(gd);
    return gd;
}

void random_partition_means(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, const uint32_t* order, const uint32_t* offsets, double* means,
                            double* sizes)
{
    mlhip_group* g = group_of(ctx);
    // The running means are order dependent (ML/Clustering.cpp:33-35): the shards continue each other's K d chains in row order,
    // one after the other. A cluster's rows are listed ascending, so a shard's share of every list is one contiguous piece.
    std::vector<uint32_t> local_order, local_offsets((size_t)K + 1);
    for (int s = 0; s < g->n; ++s) {
        const uint64_t lo = data->first_row[(size_t)s], hi = data->first_row[(size_t)s + 1];
        local_order.clear();
        for (uint32_t k = 0; k < K; ++k) {
            local_offsets[k] = (uint32_t)local_order.size();
            const uint32_t* b = order + offsets[k];
            const uint32_t* e = order + offsets[k + 1];
            const uint32_t* from = std::lower_bound(b, e, lo, [](uint32_t v, uint64_t bound) { return (uint64_t)v < bound; });
            const uint32_t* to = std::lower_bound(from, e, hi, [](uint32_t v, uint64_t bound) { return (uint64_t)v < bound; });
            for (const uint32_t* p = from; p < to; ++p) local_order.push_back((uint32_t)(*p - lo));
        }
        local_offsets[K] = (uint32_t)local_order.size();
        require(local_order.size() == hi - lo, "order must list every row exactly once, ascending within a cluster");
        check_status(mlhip_random_partition_means(g->shard[(size_t)s], data->parts[(size_t)s], K, local_order.data(), local_offsets.data(),
                                                  means, sizes));
    }
}

void em_responsibilities(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, double* resp, int64_t ldr, uint64_t first, uint64_t count)
{
    fan_out(ctx, data, [&](Shard& sh) {
        const uint64_t lo = std::max(first, sh.first_row), hi = std::min(first + count, sh.first_row + sh.n_rows);
        if (lo >= hi) return (int)MLHIP_OK;                   // (no collective inside: a shard may sit this one out)
        return mlhip_em_responsibilities_rows(sh.ctx, sh.part, K, lo - sh.first_row, hi - lo, resp + (lo - first), ldr);
    });
}

/// The slowest shard's average (launch counts of that shard): what bounds the group's step.
void timing_get(mlhip_ctx* ctx, const char* name, double* avg_ms, uint64_t* launches)
{
    *avg_ms = 0;
    *launches = 0;
    for (mlhip_ctx* c : group_of(ctx)->shard) {
        double ms = 0;
        uint64_t cnt = 0;
        check_status(mlhip_timing_get(c, name, &ms, &cnt));
        if (cnt && ms >= *avg_ms) { *avg_ms = ms; *launches = cnt; }
    }
}

}  // namespace grp
}  // namespace mlhip_rt
