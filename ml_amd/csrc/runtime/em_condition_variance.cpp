// mlhip_em_conditional_variances: Var[x_M | x_O] of every row of a resident block of OBSERVED coordinates under a mixture conditioned
// on them (the definition: mlhip.h; the kernels: device/em_condition_variance.hip). The host conditions the model (host::condition,
// host::condition_covariances); the device runs the marginal mixture's E-step in its exact form on chunks of whole tiles, exactly as
// mlhip_em_conditional_means does (runtime/em_condition.cpp), and ONE launch of the variance kernel behind every chunk: it forms the
// mean first, by the mean kernel's steps, and the centred second moment in a second sweep. Every buffer is the call's own, taken from
// the context's pool: the handle's E-step state, weights, ridge and label history stay as they were.
#include "internal.hpp"

namespace mlhip_rt {
namespace {

struct ConditionedModel {
    int K, dM;
    const double *mixing, *means_observed, *covs_observed, *maps, *means_missing, *covs_missing;
};

/// The conditioning kernels' records (condition_table) with c behind each: diag(C_k), or the packed lower triangle, in the padded dM.
std::vector<double> variance_table(int kernel, const ConditionedModel& m, int dO, bool full)
{
    const int K = m.K, dM = m.dM;
    const std::vector<double> base = condition_table(kernel, K, dO, dM, m.means_observed, m.maps, m.means_missing, nullptr);
    const size_t ps = condition_record_doubles(kernel, dO, dM), stride = condition_variance_record_doubles(kernel, dO, dM, full);
    std::vector<double> table(stride * K, 0.0);
    for (int k = 0; k < K; ++k) {
        double* rec = table.data() + stride * k;
        std::copy_n(base.data() + ps * k, ps, rec);
        const double* Ck = m.covs_missing + (size_t)k * dM * dM;
        for (int a = 0; a < dM; ++a) {
            if (!full) { rec[ps + a] = Ck[(size_t)a * dM + a]; continue; }
            for (int b = 0; b <= a; ++b) rec[ps + (size_t)a * (a + 1) / 2 + b] = Ck[(size_t)a * dM + b];
        }
    }
    return table;
}

/// A chunk's rows x width doubles from the device to rows `ld` doubles apart on the host.
void download_rows(mlhip_ctx* ctx, std::vector<double>& packed, double* dst, int64_t ld, const DevBuf& src, uint32_t rows, size_t width)
{
    const bool spread = ld != (int64_t)width;
    if (spread) packed.resize((size_t)rows * width);
    download_columns(ctx, reinterpret_cast<char*>(spread ? packed.data() : dst), 0, src.as<char>(), 0, sizeof(double) * width * rows, 1);
    if (spread)
        for (uint32_t i = 0; i < rows; ++i) std::memcpy(dst + (int64_t)i * ld, packed.data() + (size_t)i * width, sizeof(double) * width);
}

void em_conditional_variances(mlhip_data* dt, const ConditionedModel& m, bool full, double* variances, int64_t ld_variances, double* means_out,
                              int64_t ld_means, double* log_density)
{
    mlhip_ctx* ctx = dt->ctx;
    if (!dt->n) return;
    const int dO = dt->d, K = m.K, dM = m.dM;
    const ConditionRoute r = condition_variance_route(dt, K, dM, full, means_out != nullptr);
    if (condition_pad(r.kernel, dO) < 0 || condition_pad(r.kernel, dM) < 0) throw Unsupported("conditional variance kernel not instantiated for this shape");
    const uint32_t chunk = r.chunk_rows;
    const size_t width = full ? (size_t)dM * dM : (size_t)dM;
    DevBuf records{&dt->pool}, work{&dt->pool}, table{&dt->pool}, lw{&dt->pool}, lse{&dt->pool}, ll{&dt->pool}, v{&dt->pool}, y{&dt->pool},
        scratch{&dt->pool};
    PinnedBuf staging{&dt->pool};
    build_records(dt, r.em, K, m.mixing, m.means_observed, m.covs_observed, false, records, staging, work);   // (always the exact form: no FOLD)
    const std::vector<double> host_table = variance_table(r.kernel, m, dO, full);
    table.reserve(sizeof(double) * host_table.size());
    HIP_CHECK(hipMemcpyAsync(table.p, host_table.data(), sizeof(double) * host_table.size(), hipMemcpyHostToDevice, ctx->stream));
    lw.reserve(sizeof(double) * (size_t)chunk * K);
    lse.reserve(sizeof(double) * chunk);
    ll.reserve(sizeof(double) * kMaxLlPartials);
    v.reserve(sizeof(double) * (size_t)chunk * width);
    if (means_out) y.reserve(sizeof(double) * (size_t)chunk * dM);
    if (r.kernel == kConditionPlain) scratch.reserve(sizeof(double) * (size_t)chunk * 2 * dM);
    std::vector<double> packed;                                 // a leading dimension above the width: a chunk comes down contiguous and is spread by the CPU
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
        ConditionVarianceArgs c{};
        c.xt = a.xt; c.ldx = a.ldx; c.n = rows; c.dO = dO; c.dM = dM; c.K = K;
        c.lw = a.lw; c.ldr = a.ldr; c.lse = a.lse;
        c.table = table.as<double>(); c.out = v.as<double>();
        c.means = means_out ? y.as<double>() : nullptr;
        c.work = r.kernel == kConditionPlain ? scratch.as<double>() : nullptr;
        c.full = full; c.skip = r.skip; c.kernel = r.kernel;
        ctx->timed("em_condition_variance", [&] { grid = launch_em_condition_variance(c, ctx->num_cus, ctx->stream); });
        if (grid < 0) throw Unsupported("conditional variance kernel not instantiated for this shape");
        HIP_CHECK(hipGetLastError());
        // (the copies wait for the stream: the scratch is free for the next chunk, and host_table for the end of the call)
        download_rows(ctx, packed, variances + (int64_t)row * ld_variances, ld_variances, v, rows, width);
        if (means_out) download_rows(ctx, packed, means_out + (int64_t)row * ld_means, ld_means, y, rows, (size_t)dM);
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
        if (ctx->group) {
            // (every shard conditions its own rows: no collective, nothing to put together but the rows' places in the caller's arrays)
            fan_out(ctx, data, [&](Shard& sh) {
                return mlhip_em_conditional_variances(sh.ctx, sh.part, K, dM, mixing, means_observed, covariances_observed, maps, means_missing,
                                                      covariances_missing, full, sh.rows(variances, ld_variances), ld_variances,
                                                      means_out ? sh.rows(means_out, ld_means) : nullptr, ld_means, sh.rows(log_density));
            });
            return;
        }
        const ConditionedModel m{(int)K, (int)dM, mixing, means_observed, covariances_observed, maps, means_missing, covariances_missing};
        em_conditional_variances(data, m, full != 0, variances, ld_variances, means_out, ld_means, log_density);
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
