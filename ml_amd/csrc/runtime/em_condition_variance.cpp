// mlhip_em_conditional_variances: Var[x_M | x_O] of every row of a resident block of OBSERVED coordinates under a mixture conditioned
// on them (the definition: mlhip.h; the kernels: device/em_condition_variance.hip). The host conditions the model (host::condition,
// host::condition_covariances); the device runs the conditioning pass (ConditionPass, runtime/em_condition.cpp) with ONE launch of
// the variance kernel behind every chunk: it forms the mean first, by the mean kernel's steps, and the centred second moment in a
// second sweep.
#include "internal.hpp"

namespace mlhip_rt {
namespace {

/// `covs_missing`: the K conditioned covariances C_k, dM x dM row-major.
void em_conditional_variances(mlhip_data* dt, const ConditionedModel& m, const double* covs_missing, bool full, double* variances,
                              int64_t ld_variances, double* means_out, int64_t ld_means, double* log_density)
{
    mlhip_ctx* ctx = dt->ctx;
    if (!dt->n) return;
    const int dO = dt->d, dM = m.dM;
    const ConditionRoute r = condition_variance_route(dt, m.K, dM, full, means_out != nullptr);
    const uint32_t chunk = r.chunk_rows;
    const size_t width = full ? (size_t)dM * dM : (size_t)dM;
    // the record's tail c: diag(C_k), or the packed lower triangle, in the padded dM
    const size_t tail = condition_variance_record_doubles(r.kernel, dO, dM, full) - condition_record_doubles(r.kernel, dO, dM);
    ConditionPass pass(dt, m, r.em, r.kernel, chunk, tail, [&](int k, double* c) {
        const double* Ck = covs_missing + (size_t)k * dM * dM;
        for (int a = 0; a < dM; ++a) {
            if (!full) { c[a] = Ck[(size_t)a * dM + a]; continue; }
            for (int b = 0; b <= a; ++b) c[(size_t)a * (a + 1) / 2 + b] = Ck[(size_t)a * dM + b];
        }
    }, "conditional variance kernel not instantiated for this shape");
    DevBuf v{&dt->pool}, y{&dt->pool}, scratch{&dt->pool};
    v.reserve(sizeof(double) * (size_t)chunk * width);
    if (means_out) y.reserve(sizeof(double) * (size_t)chunk * dM);
    if (r.kernel == kConditionPlain) scratch.reserve(sizeof(double) * (size_t)chunk * 2 * dM);
    pass.run(log_density, [&](const ConditionChunk& chunk_args, uint32_t row) {
        ConditionVarianceArgs c{};
        static_cast<ConditionChunk&>(c) = chunk_args;
        c.out = v.as<double>();
        c.means = means_out ? y.as<double>() : nullptr;
        c.work = r.kernel == kConditionPlain ? scratch.as<double>() : nullptr;
        c.full = full; c.skip = r.skip;
        int grid = 0;
        ctx->timed("em_condition_variance", [&] { grid = launch_em_condition_variance(c, ctx->num_cus, ctx->stream); });
        if (grid < 0) throw Unsupported("conditional variance kernel not instantiated for this shape");
        HIP_CHECK(hipGetLastError());
        pass.download_rows(variances + (int64_t)row * ld_variances, ld_variances, v.p, c.n, width);
        if (means_out) pass.download_rows(means_out + (int64_t)row * ld_means, ld_means, y.p, c.n, (size_t)dM);
    });
}

}  // namespace
}  // namespace mlhip_rt

extern "C" {

int mlhip_em_conditional_variances(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, uint32_t dM, const double* mixing, const double* means_observed,
                                   const double* covariances_observed, const double* maps, const double* means_missing,
                                   const double* covariances_missing, int full, double* variances, int64_t ld_variances, double* means_out,
                                   int64_t ld_means, double* log_density)
{
    return guarded([&] {
        check_call(ctx, data, K);
        require(mixing && means_observed && covariances_observed && maps && means_missing && covariances_missing, "null argument");
        const uint32_t dO = (uint32_t)(data->parts.empty() ? data->d : data->parts[0]->d);
        require(dM >= 1 && dO + dM <= (uint32_t)kGenericMaxDim, "observed and missing coordinates together must be 2 .. 4096");
        require(full == 0 || full == 1, "full must be 0 or 1");
        const int64_t width = full ? (int64_t)dM * dM : (int64_t)dM;
        require(ld_variances >= width, "ld_variances must be >= dM (dM * dM with full)");
        require(!means_out || ld_means >= (int64_t)dM, "ld_means must be >= dM");
        if (!data->rows()) return;
        require(variances, "null argument");
        const ConditionedModel m{(int)K, (int)dM, mixing, means_observed, covariances_observed, maps, means_missing};
        on_block_or_shards(ctx, data, [&](Shard& sh) {
            em_conditional_variances(sh.part, m, covariances_missing, full != 0, sh.rows(variances, ld_variances), ld_variances,
                                     sh.rows(means_out, ld_means), ld_means, sh.rows(log_density));
        });
    });
}

int mlhip_em_condition_variance_route(const mlhip_data* data, uint32_t K, uint32_t dM, int full, int* kernel)
{
    return guarded([&] {
        require(data && kernel && K >= 1 && dM >= 1 && (full == 0 || full == 1), "bad argument");
        if (!data->parts.empty()) data = data->parts[0];        // (a group's block: every shard takes the same route)
        require((uint32_t)data->d + dM <= (uint32_t)kGenericMaxDim, "observed and missing coordinates together must be 2 .. 4096");
        *kernel = condition_variance_route(data, (int)K, (int)dM, full != 0, false).kernel;
    });
}

}  // extern "C"
