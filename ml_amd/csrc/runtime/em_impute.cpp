// mlhip_em_impute: every NaN of a host block replaced by E[x_j | x_O(i)] under a mixture, O(i) the coordinates row i has (the
// definition: mlhip.h). The host plan (host/impute_plan.hpp) groups the rows by pattern; the complete rows go through mlhip_em_score,
// the rows of all NaN are formed on the host, and the others take the route of impute_route (internal.hpp):
//   COMPOSED  every group through the conditional-means pass of its pattern (em_condition.cpp), the model conditioned on the host;
//   KERNEL    (2 <= d <= 32) the patterns' records built on the device for a chunk of patterns at a time (em_impute_records.hip),
//             then per chunk of rows -- gathered in plan order, so a tile is a run of rows -- one launch of the evaluation kernel
//             (em_impute.hip) per padding class present; the results come down compact and are scattered on the host.
// Everything is computed into the call's own result buffers and copied to the caller's arrays at the end: a domain error writes
// nothing. Row i's result is a pure function of row i and the parameters on every path, so the grouping, the chunks and the shards
// of a device group change no bit.
#include "internal.hpp"

#include "host/impute_plan.hpp"

namespace mlhip_rt {
namespace {

struct ImputeModel {
    int d, K;
    const double *mixing, *means, *covs;                         // covs: K full matrices
};

/// A block uploaded for the call, released with it.
struct Block {
    mlhip_data* h = nullptr;
    Block(mlhip_ctx* ctx, const double* x, uint32_t d, uint32_t n) { check_status(mlhip_data_upload(ctx, x, d, n, d, &h)); }
    Block(const Block&) = delete;
    Block& operator=(const Block&) = delete;
    ~Block() { if (h) mlhip_data_free(h); }
};

/// The call's blocks are this rank's own rows and nothing in it is a collective: while it runs, uploads take their shift from the
/// block alone (a job's ranks hold different patterns, so they would not even make the same number of uploads).
struct NoCollective {
    mlhip_ctx* ctx;
    mlhip_allreduce_fn fn;
    explicit NoCollective(mlhip_ctx* c) : ctx(c), fn(c->reduce_fn) { ctx->reduce_fn = nullptr; }
    ~NoCollective() { ctx->reduce_fn = fn; }
};

/// Wall-clock time of a host phase of the call under the context's timers (mlhip_timing_get: "impute_plan", "impute_upload",
/// "impute_download"), taken only while timing is enabled. A phase that waits for the stream includes what it waited for.
struct HostPhase {
    mlhip_ctx* ctx;
    const char* name;
    std::chrono::steady_clock::time_point t0;
    HostPhase(mlhip_ctx* c, const char* n) : ctx(c), name(n), t0(std::chrono::steady_clock::now()) {}
    ~HostPhase()
    {
        if (!ctx->timing) return;
        Timer& t = ctx->timers[name];
        t.total_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        t.launches += 1;
    }
};

/// What the call has computed so far, in the caller's layouts; copied to the caller's arrays once every group has succeeded.
struct ImputeResult {
    std::vector<double> out, log_density, resp;
};

/// The rows order[first .. first + rows) of pattern p, 1 <= dO <= d - 1, through the conditional-means pass.
void impute_group(mlhip_ctx* ctx, const ImputeModel& m, const host::ImputePlan& plan, uint32_t p, uint32_t first, uint32_t rows, const double* x,
                  ImputeResult& res, bool want_density, bool want_resp)
{
    const int d = m.d, K = m.K, dO = (int)plan.n_observed[p], dM = d - dO;
    std::vector<unsigned int> observed, missing;
    for (int c = 0; c < d; ++c) (plan.observed(p, (uint32_t)c) ? observed : missing).push_back((unsigned int)c);
    std::vector<double> mu_o((size_t)K * dO), s_oo((size_t)K * dO * dO), maps((size_t)K * dM * dO), mu_m((size_t)K * dM);
    try {
        host::condition(Covariance::Full, K, d, m.means, m.covs, observed.data(), dO, mu_o.data(), s_oo.data(), maps.data(), mu_m.data());
    } catch (const std::domain_error& e) {
        throw DomainError(e.what());
    }
    std::vector<double> packed((size_t)rows * dO), y((size_t)rows * dM), dens(want_density ? rows : 0), shares(want_resp ? (size_t)rows * K : 0);
    for (uint32_t i = 0; i < rows; ++i) {
        const double* row = x + (size_t)plan.order[first + i] * d;
        for (int c = 0; c < dO; ++c) packed[(size_t)i * dO + c] = row[observed[c]];
    }
    Block block(ctx, packed.data(), (uint32_t)dO, rows);
    const ConditionedModel cm{K, dM, m.mixing, mu_o.data(), s_oo.data(), maps.data(), mu_m.data()};
    em_conditional_means(block.h, cm, y.data(), dM, want_density ? dens.data() : nullptr, want_resp ? shares.data() : nullptr, K);
    for (uint32_t i = 0; i < rows; ++i) {
        const size_t at = plan.order[first + i];
        for (int j = 0; j < dM; ++j) res.out[at * d + missing[j]] = y[(size_t)i * dM + j];
        if (want_density) res.log_density[at] = dens[i];
        if (want_resp) std::copy_n(shares.data() + (size_t)i * K, K, res.resp.data() + at * K);
    }
}

/// The complete rows order[first .. first + rows): the log-density of mlhip_em_score, and the shares of the exact E-step on the same
/// block where they are asked for.
void impute_complete(mlhip_ctx* ctx, const ImputeModel& m, const host::ImputePlan& plan, uint32_t first, uint32_t rows, const double* x,
                     ImputeResult& res, bool want_density, bool want_resp)
{
    if (!want_density && !want_resp) return;
    const int d = m.d, K = m.K;
    std::vector<double> packed((size_t)rows * d), dens(want_density ? rows : 0);
    for (uint32_t i = 0; i < rows; ++i) std::copy_n(x + (size_t)plan.order[first + i] * d, d, packed.data() + (size_t)i * d);
    Block block(ctx, packed.data(), (uint32_t)d, rows);
    mlhip_data* dt = block.h;
    if (want_density) {
        check_status(mlhip_em_score(ctx, dt, (uint32_t)K, MLHIP_COVARIANCE_FULL, m.mixing, m.means, m.covs, dens.data(), nullptr));
        for (uint32_t i = 0; i < rows; ++i) res.log_density[plan.order[first + i]] = dens[i];
    }
    if (!want_resp) return;
    const ScoreRoute r = score_route(dt, K);
    DevBuf records{&dt->pool}, work{&dt->pool}, shares{&dt->pool};
    PinnedBuf staging{&dt->pool};
    build_records(dt, r.em, K, m.mixing, m.means, m.covs, false, records, staging, work);   // (the exact form: no FOLD)
    ChunkEstep estep(dt);
    estep.reserve(K, r.chunk_rows);
    shares.reserve(sizeof(double) * (size_t)estep.chunk * K);
    std::vector<double> columns;
    for (uint32_t row = 0; row < dt->n; row += estep.chunk) {
        const uint32_t n = std::min(estep.chunk, dt->n - row);
        estep.launch(dt, r.em, K, records, row, n);
        RespArgs a{estep.lw.as<double>(), estep.chunk, estep.lse.as<double>(), n, K, shares.as<double>(), n, nullptr};
        ctx->timed("em_responsibilities", [&] { launch_em_responsibilities(a, ctx->stream); });
        HIP_CHECK(hipGetLastError());
        columns.resize((size_t)n * K);
        download_columns(ctx, reinterpret_cast<char*>(columns.data()), 0, shares.as<char>(), 0, sizeof(double) * n * K, 1);
        ctx->sync();
        for (uint32_t i = 0; i < n; ++i)
            for (int k = 0; k < K; ++k) res.resp[(size_t)plan.order[first + row + i] * K + k] = columns[(size_t)k * n + i];
    }
}

/// A row of all NaN: out_j = +0.0, then fma(pi_k, mu_k[j], out_j) for ascending k where pi_k != 0; log-density 0; shares pi.
void impute_all_missing(const ImputeModel& m, const host::ImputePlan& plan, uint32_t first, uint32_t rows, ImputeResult& res, bool want_density,
                        bool want_resp)
{
    std::vector<double> prior((size_t)m.d, 0.0);
    for (int k = 0; k < m.K; ++k) {
        if (!(m.mixing[k] != 0.0)) continue;
        for (int j = 0; j < m.d; ++j) prior[j] = std::fma(m.mixing[k], m.means[(size_t)k * m.d + j], prior[j]);
    }
    for (uint32_t i = 0; i < rows; ++i) {
        const size_t at = plan.order[first + i];
        std::copy(prior.begin(), prior.end(), res.out.begin() + at * m.d);
        if (want_density) res.log_density[at] = 0.0;
        if (want_resp) std::copy_n(m.mixing, m.K, res.resp.data() + at * m.K);
    }
}

bool partial(const host::ImputePlan& plan, uint32_t p) { return (int64_t)p != plan.complete && (int64_t)p != plan.all_missing; }

/// The runs [p0, p1) of consecutive patterns with 1 <= dO <= d - 1 whose records the kernel route builds in one launch: at most
/// route.patterns patterns (0: no such bound) and kImputeRecordBytes of records, at least one pattern.
std::vector<std::pair<uint32_t, uint32_t>> pattern_chunks(const host::ImputePlan& plan, const ImputeRoute& route, int K)
{
    std::vector<std::pair<uint32_t, uint32_t>> chunks;
    const uint64_t budget = kImputeRecordBytes / sizeof(double);
    uint32_t p = 0;
    while (p < plan.patterns()) {
        if (!partial(plan, p)) { ++p; continue; }
        const uint32_t p0 = p;
        uint64_t doubles = 0;
        while (p < plan.patterns() && partial(plan, p) && (route.patterns == 0 || p - p0 < route.patterns)) {
            const int dO = (int)plan.n_observed[p];
            const uint64_t more = (uint64_t)K * impute_record_doubles(host::impute_pad(dO), host::impute_pad((int)plan.d - dO));
            if (p > p0 && doubles + more > budget) break;
            doubles += more;
            ++p;
        }
        chunks.emplace_back(p0, p);
    }
    return chunks;
}

/// The model on the device for the records kernel: [means (K x d) | covariances (K x d x d) | log pi (K)].
struct DeviceModel {
    std::vector<double> host;
    DevBuf dev;
    const double *means, *covs, *log_mixing;
    DeviceModel(mlhip_ctx* ctx, BufferPool* const* pool, const ImputeModel& m) : dev(pool)
    {
        const size_t kd = (size_t)m.K * m.d, kdd = kd * m.d;
        host.resize(kd + kdd + m.K);
        std::copy_n(m.means, kd, host.data());
        std::copy_n(m.covs, kdd, host.data() + kd);
        for (int k = 0; k < m.K; ++k) host[kd + kdd + k] = std::log(m.mixing[k]);
        dev.reserve(sizeof(double) * host.size());
        HIP_CHECK(hipMemcpyAsync(dev.p, host.data(), sizeof(double) * host.size(), hipMemcpyHostToDevice, ctx->stream));
        means = dev.as<double>(); covs = means + kd; log_mixing = covs + kdd;
    }
};

/// The descriptors of the patterns [p0, p1), their records one after the other; returns the records' doubles.
size_t describe_patterns(const host::ImputePlan& plan, uint32_t p0, uint32_t p1, int K, std::vector<ImputePattern>& pats)
{
    pats.assign(p1 - p0, ImputePattern{});
    size_t doubles = 0;
    for (uint32_t p = p0; p < p1; ++p) {
        ImputePattern& pat = pats[p - p0];
        for (uint32_t c = 0; c < plan.d; ++c) {
            if (plan.observed(p, c)) pat.observed[pat.dO++] = c;
            else pat.missing[pat.dM++] = c;
        }
        pat.po = (uint32_t)host::impute_pad((int)pat.dO); pat.pm = (uint32_t)host::impute_pad((int)pat.dM);
        pat.rec_base = (uint32_t)doubles;
        doubles += (size_t)K * impute_record_doubles((int)pat.po, (int)pat.pm);
    }
    return doubles;
}

/// Builds the records of `pats` into `records` and waits for them. DomainError where a pivot was refused: nothing else is read then.
void build_pattern_records(mlhip_ctx* ctx, const ImputeModel& m, const DeviceModel& model, const std::vector<ImputePattern>& pats,
                           size_t doubles, DevBuf& pats_dev, DevBuf& records, DevBuf& flag)
{
    pats_dev.reserve(sizeof(ImputePattern) * pats.size());
    records.reserve(sizeof(double) * doubles);
    flag.reserve(sizeof(uint32_t));
    HIP_CHECK(hipMemcpyAsync(pats_dev.p, pats.data(), sizeof(ImputePattern) * pats.size(), hipMemcpyHostToDevice, ctx->stream));
    HIP_CHECK(hipMemsetAsync(flag.p, 0, sizeof(uint32_t), ctx->stream));
    ImputeRecordsArgs a{};
    a.d = m.d; a.K = m.K; a.means = model.means; a.covs = model.covs; a.log_mixing = model.log_mixing;
    a.patterns = pats_dev.as<ImputePattern>(); a.n_patterns = (uint32_t)pats.size();
    a.records = records.as<double>(); a.flag = flag.as<uint32_t>();
    ctx->timed("em_impute_records", [&] { launch_em_impute_records(a, ctx->stream); });
    HIP_CHECK(hipGetLastError());
    uint32_t refused = 0;
    HIP_CHECK(hipMemcpyAsync(&refused, flag.p, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    if (refused) throw DomainError("EM: the observed block of a covariance is not positive definite for a row's pattern");
}

/// The rows of every pattern with 1 <= dO <= d - 1 on the kernel route.
void impute_kernel(mlhip_ctx* ctx, const ImputeModel& m, const host::ImputePlan& plan, const ImputeRoute& route, const double* x,
                   ImputeResult& res, bool want_density, bool want_resp)
{
    const int d = m.d, K = m.K;
    BufferPool* pool = &ctx->pool;
    const DeviceModel model(ctx, &pool, m);
    DevBuf pats_dev{&pool}, records{&pool}, flag{&pool}, xs{&pool}, tiles_dev{&pool}, y{&pool}, lse{&pool}, shares{&pool};
    std::vector<ImputePattern> pats;
    std::vector<ImputeTile> tiles;
    std::vector<double> rows_host, y_host, lse_host, shares_host;
    const double half_log_two_pi = log_two_pi() / 2;
    for (const auto& chunk : pattern_chunks(plan, route, K)) {
        const uint32_t p0 = chunk.first, p1 = chunk.second;
        const size_t doubles = describe_patterns(plan, p0, p1, K, pats);
        build_pattern_records(ctx, m, model, pats, doubles, pats_dev, records, flag);
        for (uint32_t pos0 = plan.bounds[p0]; pos0 < plan.bounds[p1]; pos0 += route.rows) {
            const uint32_t pos1 = std::min<uint64_t>(plan.bounds[p1], (uint64_t)pos0 + route.rows), n = pos1 - pos0;
            std::unique_ptr<HostPhase> phase(new HostPhase(ctx, "impute_upload"));
            rows_host.resize((size_t)n * d);
            for (uint32_t i = 0; i < n; ++i) std::copy_n(x + (size_t)plan.order[pos0 + i] * d, d, rows_host.data() + (size_t)i * d);
            const std::vector<host::ImputeClass> classes = host::impute_tiles(plan, p0, p1, pos0, pos1);
            tiles.clear();
            size_t out_doubles = 0;
            for (const host::ImputeClass& cls : classes)
                for (const host::ImputeTile& t : cls.tiles) {
                    tiles.push_back({t.pattern - p0, t.first - pos0, t.rows, (uint32_t)out_doubles});
                    out_doubles += ((size_t)t.rows * pats[t.pattern - p0].dM + 1) & ~size_t(1);   // (every tile 16-byte aligned)
                }
            xs.reserve(sizeof(double) * rows_host.size());
            tiles_dev.reserve(sizeof(ImputeTile) * tiles.size());
            y.reserve(sizeof(double) * out_doubles);
            lse.reserve(sizeof(double) * n);
            if (want_resp) shares.reserve(sizeof(double) * (size_t)n * K);
            HIP_CHECK(hipMemcpyAsync(xs.p, rows_host.data(), sizeof(double) * rows_host.size(), hipMemcpyHostToDevice, ctx->stream));
            HIP_CHECK(hipMemcpyAsync(tiles_dev.p, tiles.data(), sizeof(ImputeTile) * tiles.size(), hipMemcpyHostToDevice, ctx->stream));
            phase.reset();
            size_t at = 0;
            for (const host::ImputeClass& cls : classes) {
                ImputeArgs a{};
                a.x = xs.as<double>(); a.d = d; a.K = K;
                a.patterns = pats_dev.as<ImputePattern>(); a.records = records.as<double>();
                a.tiles = tiles_dev.as<ImputeTile>() + at; a.n_tiles = (uint32_t)cls.tiles.size();
                a.po = cls.po; a.pm = cls.pm;
                a.y = y.as<double>(); a.lse = lse.as<double>();
                a.resp = want_resp ? shares.as<double>() : nullptr; a.ldr = n;
                a.skip = route.skip; a.grid_cap = route.grid_cap;
                int grid = 0;
                ctx->timed("em_impute", [&] { grid = launch_em_impute(a, ctx->num_cus, ctx->stream); });
                if (grid < 0) throw Unsupported("imputation kernel not instantiated for this shape");
                HIP_CHECK(hipGetLastError());
                at += cls.tiles.size();
            }
            phase.reset(new HostPhase(ctx, "impute_download"));
            y_host.resize(out_doubles);
            lse_host.resize(n);
            download_columns(ctx, reinterpret_cast<char*>(y_host.data()), 0, y.as<char>(), 0, sizeof(double) * out_doubles, 1);
            download_columns(ctx, reinterpret_cast<char*>(lse_host.data()), 0, lse.as<char>(), 0, sizeof(double) * n, 1);
            if (want_resp) {
                shares_host.resize((size_t)n * K);
                download_columns(ctx, reinterpret_cast<char*>(shares_host.data()), 0, shares.as<char>(), 0, sizeof(double) * n * K, 1);
            }
            ctx->sync();
            for (const ImputeTile& t : tiles) {
                const ImputePattern& pat = pats[t.pattern];
                const double offset = (double)pat.dO * half_log_two_pi;
                for (uint32_t i = 0; i < t.rows; ++i) {
                    const size_t row = plan.order[pos0 + t.first + i];
                    for (uint32_t j = 0; j < pat.dM; ++j) res.out[row * d + pat.missing[j]] = y_host[t.out_base + (size_t)i * pat.dM + j];
                    if (want_density) res.log_density[row] = lse_host[t.first + i] - offset;
                    if (want_resp)
                        for (int k = 0; k < K; ++k) res.resp[row * K + k] = shares_host[(size_t)k * n + t.first + i];
                }
            }
        }
    }
}

void em_impute(mlhip_ctx* ctx, const ImputeModel& m, const double* x, uint32_t n, double* out, double* log_density, double* resp)
{
    if (!n) return;
    ctx->use();
    const NoCollective alone(ctx);
    const ImputeRoute route = impute_route(m.d, m.K);
    std::unique_ptr<HostPhase> planning(new HostPhase(ctx, "impute_plan"));
    const host::ImputePlan plan = host::impute_plan(x, n, (uint32_t)m.d, m.d);
    planning.reset();
    ImputeResult res;
    res.out.assign(x, x + (size_t)n * m.d);                      // (the observed entries keep their bits)
    if (log_density) res.log_density.resize(n);
    if (resp) res.resp.resize((size_t)n * m.K);
    if (route.kind == kImputeKernel) impute_kernel(ctx, m, plan, route, x, res, log_density != nullptr, resp != nullptr);
    for (uint32_t p = 0; p < plan.patterns(); ++p) {
        if (partial(plan, p) && route.kind == kImputeKernel) continue;
        for (uint32_t first = plan.bounds[p]; first < plan.bounds[p + 1]; first += route.rows) {
            const uint32_t rows = std::min(route.rows, plan.bounds[p + 1] - first);
            if ((int64_t)p == plan.complete) impute_complete(ctx, m, plan, first, rows, x, res, log_density != nullptr, resp != nullptr);
            else if ((int64_t)p == plan.all_missing) impute_all_missing(m, plan, first, rows, res, log_density != nullptr, resp != nullptr);
            else impute_group(ctx, m, plan, p, first, rows, x, res, log_density != nullptr, resp != nullptr);
        }
    }
    std::copy(res.out.begin(), res.out.end(), out);
    if (log_density) std::copy(res.log_density.begin(), res.log_density.end(), log_density);
    if (resp) std::copy(res.resp.begin(), res.resp.end(), resp);
}

/// Kernel launches of the call for a plan, behind the uploads. Complete rows: one scoring kernel per group of at most route.rows rows.
/// COMPOSED: per group of one pattern's rows one E-step and one conditioning kernel (counted as one conditioning chunk: a group
/// within kScoreScratchBytes). KERNEL: per pattern chunk one records launch, and per row chunk of it one evaluation launch per
/// padding class present.
uint64_t impute_launches(const host::ImputePlan& plan, const ImputeRoute& route, int K)
{
    uint64_t launches = 0;
    for (uint32_t p = 0; p < plan.patterns(); ++p) {
        const uint64_t groups = ((uint64_t)(plan.bounds[p + 1] - plan.bounds[p]) + route.rows - 1) / route.rows;
        if ((int64_t)p == plan.complete) launches += groups;
        else if (partial(plan, p) && route.kind == kImputeComposed) launches += 2 * groups;
    }
    if (route.kind != kImputeKernel) return launches;
    for (const auto& chunk : pattern_chunks(plan, route, K)) {
        ++launches;
        for (uint32_t pos0 = plan.bounds[chunk.first]; pos0 < plan.bounds[chunk.second]; pos0 += route.rows)
            launches += host::impute_tiles(plan, chunk.first, chunk.second, pos0, (uint32_t)std::min<uint64_t>(plan.bounds[chunk.second], (uint64_t)pos0 + route.rows)).size();
    }
    return launches;
}

void check_impute_shape(uint32_t d, uint32_t K, uint64_t n)
{
    require(K >= 1, "At least one component required");
    require(d >= 1 && d <= (uint32_t)kGenericMaxDim, "the dimension must be 1 .. 4096");
    require(n < 0xffffff00ull, "too many rows (n must fit 32 bits)");
    for (int c = 1; c <= host::kImputeKernelMaxDim; ++c)
        if (host::impute_pad(c) != condition_pad(kConditionRegisters, c)) throw std::logic_error("impute_pad is not condition_pad");
}

}  // namespace
}  // namespace mlhip_rt

extern "C" {

int mlhip_em_impute(mlhip_ctx* ctx, uint32_t d, uint32_t K, int covariance_type, const double* mixing, const double* means,
                    const double* covariances, const double* x, uint64_t n, double* out, double* log_density, double* responsibilities)
{
    return guarded([&] {
        require(ctx != nullptr, "null context");
        require(mixing && means && covariances, "null argument");
        require(n == 0 || (x && out), "null argument");
        check_impute_shape(d, K, n);
        const Covariance mode = covariance_from_abi(covariance_type);
        if (!n) return;
        if (ctx->group) {
            // (every shard imputes its own rows: no collective, nothing to put together but the rows' places in the caller's arrays)
            fan_out_rows(ctx, balanced_rows(n, grp::shard_count(ctx)), nullptr, [&](Shard& sh) {
                return mlhip_em_impute(sh.ctx, d, K, covariance_type, mixing, means, covariances, sh.rows(x, d), sh.n_rows, sh.rows(out, d),
                                       sh.rows(log_density), sh.rows(responsibilities, K));
            });
            return;
        }
        std::vector<double> full;
        if (mode != Covariance::Full) {
            full = as_full(mode, (int)K, (int)d, covariances);
            covariances = full.data();
        }
        em_impute(ctx, ImputeModel{(int)d, (int)K, mixing, means, covariances}, x, (uint32_t)n, out, log_density, responsibilities);
    });
}

int mlhip_em_impute_plan(const double* x, uint64_t n, uint32_t d, uint32_t* n_patterns, uint32_t* order, uint32_t* bounds, uint32_t* n_observed)
{
    return guarded([&] {
        require(n_patterns != nullptr, "null argument");
        require(n == 0 || x, "null argument");
        check_impute_shape(d, 1, n);
        const host::ImputePlan plan = host::impute_plan(x, (uint32_t)n, d, d);
        *n_patterns = plan.patterns();
        if (order) std::copy(plan.order.begin(), plan.order.end(), order);
        if (bounds) std::copy(plan.bounds.begin(), plan.bounds.end(), bounds);
        if (n_observed) std::copy(plan.n_observed.begin(), plan.n_observed.end(), n_observed);
    });
}

int mlhip_em_impute_route(uint32_t d, uint32_t K, const double* x, uint64_t n, int* route, uint64_t* launches)
{
    return guarded([&] {
        require(route != nullptr, "null argument");
        require(n == 0 || x || !launches, "null argument");
        check_impute_shape(d, K, n);
        static_assert(kImputeComposed == MLHIP_IMPUTE_COMPOSED && kImputeKernel == MLHIP_IMPUTE_KERNEL, "mlhip.h names the routes by ImputeKind");
        static_assert(host::kImputeKernelMaxDim == kImputeMaxDim && host::kImputeTileRows == 64, "the plan's tiles are the kernel's");
        const ImputeRoute r = impute_route((int)d, (int)K);
        *route = r.kind;
        if (launches) *launches = impute_launches(host::impute_plan(x, (uint32_t)n, d, d), r, (int)K);
    });
}

int mlhip_em_impute_condition(mlhip_ctx* ctx, uint32_t d, uint32_t K, int covariance_type, const double* mixing, const double* means,
                              const double* covariances, const uint32_t* observed, uint32_t n_observed, double* means_observed,
                              double* whitening, double* coefficients, double* maps, double* means_missing)
{
    return guarded([&] {
        require(ctx != nullptr && !ctx->group, "a single context is required");
        require(mixing && means && covariances && observed && means_observed && whitening && coefficients && maps && means_missing, "null argument");
        const Covariance mode = check_condition_arguments(d, K, covariance_type, observed, n_observed);
        require(d <= (uint32_t)kImputeMaxDim, "the kernel route's records exist up to d = 32");
        for (uint32_t c = 1; c < n_observed; ++c) require(observed[c - 1] < observed[c], "observed must be ascending");
        ctx->use();
        std::vector<double> full;
        if (mode != Covariance::Full) {
            full = as_full(mode, (int)K, (int)d, covariances);
            covariances = full.data();
        }
        const ImputeModel m{(int)d, (int)K, mixing, means, covariances};
        BufferPool* pool = &ctx->pool;
        const DeviceModel model(ctx, &pool, m);
        std::vector<ImputePattern> pats(1);
        ImputePattern& pat = pats[0];
        std::vector<char> seen(d, 0);
        for (uint32_t c = 0; c < n_observed; ++c) { pat.observed[pat.dO++] = observed[c]; seen[observed[c]] = 1; }
        for (uint32_t c = 0; c < d; ++c) if (!seen[c]) pat.missing[pat.dM++] = c;
        const int po = host::impute_pad((int)pat.dO), pm = host::impute_pad((int)pat.dM);
        pat.po = (uint32_t)po; pat.pm = (uint32_t)pm;
        const size_t ps = impute_record_doubles(po, pm);
        DevBuf pats_dev{&pool}, records{&pool}, flag{&pool};
        build_pattern_records(ctx, m, model, pats, ps * K, pats_dev, records, flag);
        std::vector<double> rec(ps * K);
        HIP_CHECK(hipMemcpyAsync(rec.data(), records.p, sizeof(double) * rec.size(), hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
        const size_t dO = pat.dO, dM = pat.dM;
        for (uint32_t k = 0; k < K; ++k) {
            const double* r = rec.data() + ps * k;
            std::copy_n(r, dO, means_observed + k * dO);
            std::copy_n(r + po, dM, means_missing + k * dM);
            const double* at = r + po + pm;
            for (size_t j = 0; j < dM; ++j)
                for (size_t c = 0; c < dO; ++c) maps[(k * dM + j) * dO + c] = at[c * pm + j];
            const double* w = at + (size_t)po * pm;
            for (size_t j = 0; j < dO; ++j)
                for (size_t l = 0; l < dO; ++l) whitening[(k * dO + j) * dO + l] = l <= j ? w[j * (j + 1) / 2 + l] : 0.0;
            coefficients[k] = w[(size_t)po * (po + 1) / 2];
        }
    });
}

}  // extern "C"
