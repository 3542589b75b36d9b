// mlhip_em_condition / mlhip_em_conditional_means: E[x_M | x_O] of every row of a resident block of OBSERVED coordinates under a
// mixture conditioned on them (the definition: mlhip.h; the kernels: device/em_condition.hip). The host conditions the model
// (host::condition: marginal parameters and the regression maps A_k); the device runs the marginal mixture's E-step in its exact form
// on chunks of whole tiles, as mlhip_em_score's composed route does, and the conditioning kernel behind every chunk. Every buffer is
// the call's own, taken from the context's pool: the handle's E-step state, weights, ridge and label history stay as they were.
#include "internal.hpp"

namespace mlhip_rt {

std::vector<double> condition_table(int kernel, int K, int dO, int dM, const double* means_observed, const double* maps,
                                    const double* means_missing, const double* factors)
{
    const size_t po = (size_t)condition_pad(kernel, dO), pm = (size_t)condition_pad(kernel, dM), ps = condition_record_doubles(kernel, dO, dM);
    const size_t stride = factors ? condition_sample_record_doubles(kernel, dO, dM) : ps;
    std::vector<double> table(stride * K, 0.0);
    for (int k = 0; k < K; ++k) {
        double* rec = table.data() + stride * k;
        std::copy_n(means_observed + (size_t)k * dO, dO, rec);
        std::copy_n(means_missing + (size_t)k * dM, dM, rec + po);
        const double* A = maps + (size_t)k * dM * dO;
        for (int c = 0; c < dO; ++c)
            for (int j = 0; j < dM; ++j) rec[po + pm + (size_t)c * pm + j] = A[(size_t)j * dO + c];
        // (a padded coordinate's term is fma(-0.0, +0.0, t) = t for every t, a t of -0.0 included: device/em_condition.hip)
        std::fill(rec + po + pm + (size_t)dO * pm, rec + ps, -0.0);
        if (!factors) continue;
        const double* G = factors + (size_t)k * dM * dM;
        for (int j = 0; j < dM; ++j)
            for (int c = 0; c <= j; ++c) rec[ps + (size_t)j * (j + 1) / 2 + c] = G[(size_t)j * dM + c];
    }
    return table;
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

namespace {

void em_conditional_means(mlhip_data* dt, int K, int dM, const double* mixing, const double* means_observed, const double* covs_observed,
                          const double* maps, const double* means_missing, double* out, int64_t ld_out, double* log_density)
{
    mlhip_ctx* ctx = dt->ctx;
    if (!dt->n) return;
    const int dO = dt->d;
    const ConditionRoute r = condition_route(dt, K, dM);
    if (condition_pad(r.kernel, dO) < 0 || condition_pad(r.kernel, dM) < 0) throw Unsupported("conditioning kernel not instantiated for this shape");
    const uint32_t chunk = r.chunk_rows;
    DevBuf records{&dt->pool}, work{&dt->pool}, table{&dt->pool}, lw{&dt->pool}, lse{&dt->pool}, ll{&dt->pool}, y{&dt->pool};
    PinnedBuf staging{&dt->pool};
    build_records(dt, r.em, K, mixing, means_observed, covs_observed, false, records, staging, work);   // (always the exact form: no FOLD)
    const std::vector<double> host_table = condition_table(r.kernel, K, dO, dM, means_observed, maps, means_missing, nullptr);
    table.reserve(sizeof(double) * host_table.size());
    HIP_CHECK(hipMemcpyAsync(table.p, host_table.data(), sizeof(double) * host_table.size(), hipMemcpyHostToDevice, ctx->stream));
    lw.reserve(sizeof(double) * (size_t)chunk * K);
    lse.reserve(sizeof(double) * chunk);
    ll.reserve(sizeof(double) * kMaxLlPartials);
    y.reserve(sizeof(double) * (size_t)chunk * dM);
    std::vector<double> packed;                                 // ld_out > dM: a chunk comes down contiguous and is spread by the CPU
    if (ld_out != (int64_t)dM) packed.resize((size_t)std::min(chunk, dt->n) * dM);
    // the kernels' lw leave the density's constant out, like the E-step's (ML/EM.cpp:197-198 applies it to the mean)
    const double offset = (double)dO * log_two_pi() / 2;
    for (uint32_t row = 0; row < dt->n; row += chunk) {
        const uint32_t rows = std::min(chunk, dt->n - row);   // (padded_samples(rows) <= chunk: the chunk is whole tiles)
        EstepArgs a{};
        a.xt = dt->xt.as<double>() + row; a.ldx = dt->ldx; a.n = rows; a.D = dt->D;
        a.params = records.as<double>(); a.K = K;
        a.lw = lw.as<double>(); a.ldr = chunk; a.lse = lse.as<double>();
        a.ll_partials = ll.as<double>(); a.n_ll_partials = kMaxLlPartials;
        a.shift = dt->shift_dev.as<double>(); a.fold = 0; a.with_lse = 1;
        a.num_cus = ctx->num_cus;
        a.plain = r.em.estep == Estep::kPlain;
        int grid = 0;
        ctx->timed("em_estep", [&] {
            grid = r.em.estep == Estep::kMatrix4 ? launch_em_estep_mfma4(a, ctx->num_cus, ctx->stream) : launch_em_estep(a, ctx->stream);
        });
        if (grid < 0) throw Unsupported("E-step kernel not instantiated for this dimension");
        ConditionArgs c{};
        c.xt = a.xt; c.ldx = a.ldx; c.n = rows; c.dO = dO; c.dM = dM; c.K = K;
        c.lw = a.lw; c.ldr = a.ldr; c.lse = a.lse;
        c.table = table.as<double>(); c.out = y.as<double>();
        c.skip = r.skip; c.kernel = r.kernel;
        ctx->timed("em_condition", [&] { grid = launch_em_condition(c, ctx->num_cus, ctx->stream); });
        if (grid < 0) throw Unsupported("conditioning kernel not instantiated for this shape");
        HIP_CHECK(hipGetLastError());
        // (the copies wait for the stream: the scratch is free for the next chunk, and host_table for the end of the call)
        double* dst = out + (int64_t)row * ld_out;
        download_columns(ctx, reinterpret_cast<char*>(packed.empty() ? dst : packed.data()), 0, y.as<char>(), 0, sizeof(double) * dM * rows, 1);
        if (!packed.empty())
            for (uint32_t i = 0; i < rows; ++i) std::memcpy(dst + (int64_t)i * ld_out, packed.data() + (size_t)i * dM, sizeof(double) * dM);
        if (log_density) {
            download_columns(ctx, reinterpret_cast<char*>(log_density + row), 0, lse.as<char>(), 0, sizeof(double) * rows, 1);
            for (uint32_t i = 0; i < rows; ++i) log_density[row + i] -= offset;
        }
    }
    ctx->sync();
}

}  // namespace
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
        if (ctx->group) {
            // (every shard conditions its own rows: no collective, nothing to put together but the rows' places in the caller's arrays)
            fan_out(ctx, data, [&](Shard& sh) {
                return mlhip_em_conditional_means(sh.ctx, sh.part, K, dM, mixing, means_observed, covariances_observed, maps, means_missing,
                                                  sh.rows(out, ld_out), ld_out, sh.rows(log_density));
            });
            return;
        }
        em_conditional_means(data, (int)K, (int)dM, mixing, means_observed, covariances_observed, maps, means_missing, out, ld_out, log_density);
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
