// mlhip_em_condition / mlhip_em_conditional_means: E[x_M | x_O] of every row of a resident block of OBSERVED coordinates under a
// mixture conditioned on them (the definition: mlhip.h; the kernels: device/em_condition.hip) -- and the chunked pass every
// conditioning call runs (ConditionPass, internal.hpp). The host conditions the model (host::condition: marginal parameters and the
// regression maps A_k); the device runs the marginal mixture's E-step in its exact form on chunks of whole tiles, as mlhip_em_score's
// composed route does, and the call's own kernel behind every chunk.
#include "internal.hpp"

namespace mlhip_rt {

void ChunkEstep::reserve(int K, uint32_t chunk_rows)
{
    chunk = chunk_rows;
    lw.reserve(sizeof(double) * (size_t)chunk * K);
    lse.reserve(sizeof(double) * chunk);
    ll.reserve(sizeof(double) * kMaxLlPartials);
}

void ChunkEstep::launch(mlhip_data* dt, const EmRoute& em, int K, const DevBuf& records, uint32_t row, uint32_t rows)
{
    mlhip_ctx* ctx = dt->ctx;
    EstepArgs a{};
    a.xt = dt->xt.as<double>() + row; a.ldx = dt->ldx; a.n = rows; a.D = dt->D;
    a.params = records.as<double>(); a.K = K;
    a.lw = lw.as<double>(); a.ldr = chunk; a.lse = lse.as<double>();
    a.ll_partials = ll.as<double>(); a.n_ll_partials = kMaxLlPartials;
    a.shift = dt->shift_dev.as<double>(); a.fold = 0; a.with_lse = 1;
    a.num_cus = ctx->num_cus;
    a.plain = em.estep == Estep::kPlain;
    int grid = 0;
    ctx->timed("em_estep", [&] {
        grid = em.estep == Estep::kMatrix4 ? launch_em_estep_mfma4(a, ctx->num_cus, ctx->stream) : launch_em_estep(a, ctx->stream);
    });
    if (grid < 0) throw Unsupported("E-step kernel not instantiated for this dimension");
}

std::vector<double> condition_table(int kernel, const ConditionedModel& m, int dO, size_t tail, const ConditionTail& fill)
{
    const int K = m.K, dM = m.dM;
    const size_t po = (size_t)condition_pad(kernel, dO), pm = (size_t)condition_pad(kernel, dM), ps = condition_record_doubles(kernel, dO, dM);
    const size_t stride = ps + tail;
    std::vector<double> table(stride * K, 0.0);
    for (int k = 0; k < K; ++k) {
        double* rec = table.data() + stride * k;
        std::copy_n(m.means_observed + (size_t)k * dO, dO, rec);
        std::copy_n(m.means_missing + (size_t)k * dM, dM, rec + po);
        const double* A = m.maps + (size_t)k * dM * dO;
        for (int c = 0; c < dO; ++c)
            for (int j = 0; j < dM; ++j) rec[po + pm + (size_t)c * pm + j] = A[(size_t)j * dO + c];
        std::fill(rec + po + pm + (size_t)dO * pm, rec + ps, -0.0);
        if (tail) fill(k, rec + ps);
    }
    return table;
}

ConditionPass::ConditionPass(mlhip_data* dt, const ConditionedModel& m, const EmRoute& em, int kernel, uint32_t chunk_rows, size_t tail,
                             const ConditionTail& fill, const char* unsupported)
    : dt_(dt), em_(em), records_(&dt->pool), work_(&dt->pool), table_(&dt->pool), staging_(&dt->pool), estep_(dt)
{
    const int dO = dt->d;
    if (condition_pad(kernel, dO) < 0 || condition_pad(kernel, m.dM) < 0) throw Unsupported(unsupported);
    build_records(dt, em, m.K, m.mixing, m.means_observed, m.covs_observed, false, records_, staging_, work_);
    host_table_ = condition_table(kernel, m, dO, tail, fill);
    table_.reserve(sizeof(double) * host_table_.size());
    HIP_CHECK(hipMemcpyAsync(table_.p, host_table_.data(), sizeof(double) * host_table_.size(), hipMemcpyHostToDevice, dt->ctx->stream));
    estep_.reserve(m.K, chunk_rows);
    c_.ldx = dt->ldx; c_.dO = dO; c_.dM = m.dM; c_.K = m.K;
    c_.lw = estep_.lw.as<double>(); c_.ldr = chunk_rows; c_.lse = estep_.lse.as<double>();
    c_.table = table_.as<double>(); c_.kernel = kernel;
}

void ConditionPass::run(double* log_density, const std::function<void(const ConditionChunk& c, uint32_t row)>& behind)
{
    // (ML/EM.cpp:197-198 applies the constant to the mean)
    const double offset = (double)c_.dO * log_two_pi() / 2;
    for (uint32_t row = 0; row < dt_->n; row += estep_.chunk) {
        const uint32_t rows = std::min(estep_.chunk, dt_->n - row);
        estep_.launch(dt_, em_, c_.K, records_, row, rows);
        c_.xt = dt_->xt.as<double>() + row; c_.n = rows;
        behind(c_, row);
        if (!log_density) continue;
        download_rows(log_density + row, 1, estep_.lse.p, rows, 1);
        for (uint32_t i = 0; i < rows; ++i) log_density[row + i] -= offset;
    }
    dt_->ctx->sync();
}

void on_block_or_shards(mlhip_ctx* ctx, mlhip_data* data, const std::function<void(Shard&)>& f)
{
    if (!ctx->group) {
        Shard whole;
        whole.ctx = ctx; whole.part = data; whole.n_rows = data->n;
        f(whole);
        return;
    }
    // (every shard works on its own rows: no collective, nothing to put together but the rows' places in the caller's arrays)
    fan_out(ctx, data, [&](Shard& sh) {
        return guarded([&] {
            sh.ctx->use();
            f(sh);
        });
    });
}

Covariance check_condition_arguments(uint32_t d, uint32_t K, int covariance_type, const uint32_t* observed, uint32_t n_observed)
{
    require(K >= 1, "At least one component required");
    require(d >= 1 && d <= (uint32_t)kGenericMaxDim, "the dimension must be 1 .. 4096");
    const Covariance mode = covariance_from_abi(covariance_type);
    require(n_observed >= 1 && n_observed < d, "between 1 and d - 1 coordinates must be observed");
    std::vector<char> seen(d, 0);
    for (uint32_t c = 0; c < n_observed; ++c) {
        require(observed[c] < d, "observed coordinate out of range");
        require(!seen[observed[c]], "observed coordinate given twice");
        seen[observed[c]] = 1;
    }
    static_assert(sizeof(unsigned int) == sizeof(uint32_t), "coordinates are 32-bit");
    return mode;
}

void em_conditional_means(mlhip_data* dt, const ConditionedModel& m, double* out, int64_t ld_out, double* log_density, double* resp,
                          int64_t ld_resp)
{
    mlhip_ctx* ctx = dt->ctx;
    if (!dt->n) return;
    const ConditionRoute r = condition_route(dt, m.K, m.dM);
    ConditionPass pass(dt, m, r.em, r.kernel, r.chunk_rows, 0, {}, "conditioning kernel not instantiated for this shape");
    DevBuf y{&dt->pool}, shares{&dt->pool};
    y.reserve(sizeof(double) * (size_t)r.chunk_rows * m.dM);
    std::vector<double> columns;
    if (resp) shares.reserve(sizeof(double) * (size_t)r.chunk_rows * m.K);
    pass.run(log_density, [&](const ConditionChunk& chunk, uint32_t row) {
        ConditionArgs c{};
        static_cast<ConditionChunk&>(c) = chunk;
        c.out = y.as<double>(); c.skip = r.skip;
        int grid = 0;
        ctx->timed("em_condition", [&] { grid = launch_em_condition(c, ctx->num_cus, ctx->stream); });
        if (grid < 0) throw Unsupported("conditioning kernel not instantiated for this shape");
        HIP_CHECK(hipGetLastError());
        pass.download_rows(out + (int64_t)row * ld_out, ld_out, y.p, chunk.n, (size_t)m.dM);
        if (!resp) return;
        // the shares the kernel above weighted with: em_resp_kernel's exp_nonpos(lw_k - lse) on the same block, component-major
        RespArgs a{chunk.lw, chunk.ldr, chunk.lse, chunk.n, m.K, shares.as<double>(), chunk.n, nullptr};
        ctx->timed("em_responsibilities", [&] { launch_em_responsibilities(a, ctx->stream); });
        HIP_CHECK(hipGetLastError());
        columns.resize((size_t)chunk.n * m.K);
        pass.download_rows(columns.data(), (int64_t)chunk.n * m.K, shares.p, 1, (size_t)chunk.n * m.K);
        for (uint32_t i = 0; i < chunk.n; ++i)
            for (int k = 0; k < m.K; ++k) resp[(int64_t)(row + i) * ld_resp + k] = columns[(size_t)k * chunk.n + i];
    });
}

}  // namespace mlhip_rt

extern "C" {

int mlhip_em_condition(uint32_t d, uint32_t K, int covariance_type, const double* means, const double* covariances, const uint32_t* observed,
                       uint32_t n_observed, double* means_observed, double* covariances_observed, double* maps, double* means_missing)
{
    return guarded([&] {
        require(means && covariances && observed && means_observed && covariances_observed && maps && means_missing, "null argument");
        const Covariance mode = check_condition_arguments(d, K, covariance_type, observed, n_observed);
        try {
            host::condition(mode, (int)K, (int)d, means, covariances, observed, (int)n_observed, means_observed, covariances_observed, maps,
                            means_missing);
        } catch (const std::domain_error& e) {
            throw DomainError(e.what());
        }
    });
}

int mlhip_em_conditional_means(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, uint32_t dM, const double* mixing, const double* means_observed,
                               const double* covariances_observed, const double* maps, const double* means_missing, double* out,
                               int64_t ld_out, double* log_density)
{
    return guarded([&] {
        check_call(ctx, data, K);
        require(mixing && means_observed && covariances_observed && maps && means_missing && out, "null argument");
        const uint32_t dO = (uint32_t)(data->parts.empty() ? data->d : data->parts[0]->d);
        require(dM >= 1 && dO + dM <= (uint32_t)kGenericMaxDim, "observed and missing coordinates together must be 2 .. 4096");
        require(ld_out >= (int64_t)dM, "ld_out must be >= dM");
        const ConditionedModel m{(int)K, (int)dM, mixing, means_observed, covariances_observed, maps, means_missing};
        on_block_or_shards(ctx, data, [&](Shard& sh) { em_conditional_means(sh.part, m, sh.rows(out, ld_out), ld_out, sh.rows(log_density), nullptr, 0); });
    });
}

int mlhip_em_condition_route(const mlhip_data* data, uint32_t K, uint32_t dM, int* kernel)
{
    return guarded([&] {
        require(data && kernel && K >= 1 && dM >= 1, "bad argument");
        if (!data->parts.empty()) data = data->parts[0];        // (a group's block: every shard takes the same route)
        require((uint32_t)data->d + dM <= (uint32_t)kGenericMaxDim, "observed and missing coordinates together must be 2 .. 4096");
        static_assert(kConditionRegisters == MLHIP_CONDITION_REGISTERS && kConditionPlain == MLHIP_CONDITION_PLAIN,
                      "mlhip.h names the kernels by ConditionKernel");
        *kernel = condition_route(data, (int)K, (int)dM).kernel;
    });
}

}  // extern "C"
