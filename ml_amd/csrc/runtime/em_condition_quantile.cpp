// mlhip_em_conditional_cdfs / mlhip_em_conditional_quantiles: the per-coordinate predictive CDF P(x_j <= v | x_O) and its inverse for
// every row of a resident block of OBSERVED coordinates under a mixture conditioned on them (the definitions: mlhip.h; the kernels:
// device/em_condition_quantile.hip; Phi: device/normal_cdf.hpp). The host conditions the model (host::condition,
// host::condition_covariances, mlhip_em_condition_scales); the device runs the conditioning pass (ConditionPass,
// runtime/em_condition.cpp) and behind every chunk ONE launch of the CDF kernel, or one launch of the quantile kernel per group of
// probabilities.
#include "internal.hpp"
#include "../device/normal_cdf.hpp"

namespace mlhip_rt {
namespace {

struct QuantileCall {
    const double *scales, *inverse_scales;                      // K x dM: s_kj = sqrt(C_k[j][j]) and 1 / s_kj
    bool quantile;
    const double* values; int64_t ld_values;                    // CDF
    const double *probabilities, *z; uint32_t n_prob;           // quantile: the probabilities and their normal quantiles
    double* out; int64_t ld_out;
    uint64_t block_rows;                                         // quantile: rows between the blocks of two probabilities in the caller's arrays
    double* means_out; int64_t ld_means;
    double* log_density;
    uint32_t* iterations;
};

void em_conditional_quantiles(mlhip_data* dt, const ConditionedModel& m, const QuantileCall& q)
{
    mlhip_ctx* ctx = dt->ctx;
    if (!dt->n || (q.quantile && !q.n_prob)) return;
    const int dO = dt->d, dM = m.dM;
    const ConditionQuantileRoute r = condition_quantile_route(dt, m.K, dM, q.quantile, q.n_prob, q.means_out != nullptr, q.iterations != nullptr);
    const uint32_t chunk = r.chunk_rows, group = q.quantile ? r.group : 1;
    const size_t ldq = ((size_t)chunk * dM + 1) & ~(size_t)1;   // (even: every probability's block starts 16-byte aligned)
    // the record's tail: [s | w], each in the padded dM (+0.0 beyond dM)
    const size_t tail = condition_quantile_record_doubles(r.kernel, dO, dM) - condition_record_doubles(r.kernel, dO, dM);
    ConditionPass pass(dt, m, r.em, r.kernel, chunk, tail, [&](int k, double* sw) {
        std::copy_n(q.scales + (size_t)k * dM, dM, sw);
        std::copy_n(q.inverse_scales + (size_t)k * dM, dM, sw + tail / 2);
    }, "conditional quantile kernel not instantiated for this shape");
    DevBuf out{&dt->pool}, y{&dt->pool}, vals{&dt->pool}, its{&dt->pool}, pz{&dt->pool};
    if (q.quantile) {                                            // [probabilities | their normal quantiles]
        pz.reserve(sizeof(double) * 2 * q.n_prob);
        HIP_CHECK(hipMemcpyAsync(pz.p, q.probabilities, sizeof(double) * q.n_prob, hipMemcpyHostToDevice, ctx->stream));
        HIP_CHECK(hipMemcpyAsync(pz.as<double>() + q.n_prob, q.z, sizeof(double) * q.n_prob, hipMemcpyHostToDevice, ctx->stream));
    }
    out.reserve(sizeof(double) * ldq * group);
    if (q.means_out) y.reserve(sizeof(double) * (size_t)chunk * dM);
    if (!q.quantile) vals.reserve(sizeof(double) * (size_t)chunk * dM);
    if (q.iterations) its.reserve(sizeof(uint32_t) * ldq * group);
    std::vector<double> gathered;                               // ld_values > dM: the CPU gathers a chunk's values before they go up
    pass.run(q.log_density, [&](const ConditionChunk& chunk_args, uint32_t row) {
        const uint32_t rows = chunk_args.n;
        ConditionQuantileArgs c{};
        static_cast<ConditionChunk&>(c) = chunk_args;
        c.out = out.as<double>(); c.ldq = ldq; c.skip = r.skip;
        int grid = 0;
        if (!q.quantile) {
            const double* src = q.values + (int64_t)row * q.ld_values;
            if (q.ld_values != (int64_t)dM) {
                gathered.resize((size_t)rows * dM);
                for (uint32_t i = 0; i < rows; ++i) std::memcpy(gathered.data() + (size_t)i * dM, src + (int64_t)i * q.ld_values, sizeof(double) * dM);
                src = gathered.data();
            }
            // (`gathered` is not touched again before the download below has waited for the stream, this copy included)
            HIP_CHECK(hipMemcpyAsync(vals.p, src, sizeof(double) * (size_t)rows * dM, hipMemcpyHostToDevice, ctx->stream));
            c.values = vals.as<double>();
            c.means = q.means_out ? y.as<double>() : nullptr;
            ctx->timed("em_condition_cdf", [&] { grid = launch_em_condition_cdf(c, ctx->num_cus, ctx->stream); });
            if (grid < 0) throw Unsupported("conditional CDF kernel not instantiated for this shape");
            HIP_CHECK(hipGetLastError());
            pass.download_rows(q.out + (int64_t)row * q.ld_out, q.ld_out, out.p, rows, (size_t)dM);
        }
        for (uint32_t q0 = 0; q.quantile && q0 < q.n_prob; q0 += group) {
            const uint32_t nq = std::min(group, q.n_prob - q0);
            c.probabilities = pz.as<double>() + q0; c.z = pz.as<double>() + q.n_prob + q0; c.n_prob = nq;
            c.iterations = q.iterations ? its.as<uint32_t>() : nullptr;
            c.means = q.means_out && q0 == 0 ? y.as<double>() : nullptr;   // (the first launch behind a chunk carries the mean)
            ctx->timed("em_condition_quantile", [&] { grid = launch_em_condition_quantile(c, ctx->num_cus, ctx->stream); });
            if (grid < 0) throw Unsupported("conditional quantile kernel not instantiated for this shape");
            HIP_CHECK(hipGetLastError());
            for (uint32_t g = 0; g < nq; ++g) {
                const int64_t at = (int64_t)((uint64_t)(q0 + g) * q.block_rows + row);
                pass.download_rows(q.out + at * q.ld_out, q.ld_out, out.as<double>() + ldq * g, rows, (size_t)dM);
                if (q.iterations) pass.download_rows(q.iterations + at * (int64_t)dM, (int64_t)dM, its.as<uint32_t>() + ldq * g, rows, (size_t)dM);
            }
        }
        if (q.means_out) pass.download_rows(q.means_out + (int64_t)row * q.ld_means, q.ld_means, y.p, rows, (size_t)dM);
    });
}

/// The checks both calls share, before any device work; returns dO.
uint32_t check_quantile_call(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, uint32_t dM, const ConditionedModel& m, const double* scales,
                             const double* inverse_scales, int64_t ld_out, bool with_means, int64_t ld_means)
{
    check_call(ctx, data, K);
    require(m.mixing && m.means_observed && m.covs_observed && m.maps && m.means_missing && scales && inverse_scales, "null argument");
    const uint32_t dO = (uint32_t)(data->parts.empty() ? data->d : data->parts[0]->d);
    require(dM >= 1 && dO + dM <= (uint32_t)kGenericMaxDim, "observed and missing coordinates together must be 2 .. 4096");
    require(ld_out >= (int64_t)dM, "ld_out must be >= dM");
    require(!with_means || ld_means >= (int64_t)dM, "ld_means must be >= dM");
    return dO;
}

/// The call on the block, or on every shard's rows of it.
void run(mlhip_ctx* ctx, mlhip_data* data, const ConditionedModel& m, const QuantileCall& q)
{
    on_block_or_shards(ctx, data, [&](Shard& sh) {
        QuantileCall part = q;
        part.values = sh.rows(q.values, q.ld_values);
        part.out = sh.rows(q.out, q.ld_out);
        part.means_out = sh.rows(q.means_out, q.ld_means);
        part.log_density = sh.rows(q.log_density);
        part.iterations = sh.rows(q.iterations, (int64_t)m.dM);
        em_conditional_quantiles(sh.part, m, part);
    });
}

}  // namespace
}  // namespace mlhip_rt

extern "C" {

int mlhip_normal_cdf(const double* a, uint64_t n, double* out)
{
    return guarded([&] {
        require(n == 0 || (a && out), "null argument");
        for (uint64_t i = 0; i < n; ++i) out[i] = mlhip::normal_cdf(a[i]);
    });
}

int mlhip_normal_quantile(const double* p, uint64_t n, double* out)
{
    return guarded([&] {
        require(n == 0 || (p && out), "null argument");
        for (uint64_t i = 0; i < n; ++i) require(p[i] > 0.0 && p[i] < 1.0, "a probability must lie strictly inside (0, 1)");
        for (uint64_t i = 0; i < n; ++i) out[i] = mlhip::normal_quantile(p[i]);
    });
}

int mlhip_em_condition_scales(uint32_t K, uint32_t dM, const double* covariances_missing, double* scales, double* inverse_scales)
{
    return guarded([&] {
        require(covariances_missing && scales && inverse_scales, "null argument");
        require(K >= 1 && dM >= 1 && dM < (uint32_t)kGenericMaxDim, "K must be >= 1 and dM 1 .. 4095");
        for (uint32_t k = 0; k < K; ++k)
            for (uint32_t j = 0; j < dM; ++j) {
                const double c = covariances_missing[((size_t)k * dM + j) * dM + j];
                if (!(c > 0.0) || !std::isfinite(c)) throw DomainError("a conditioned variance is not positive and finite");
                const double s = std::sqrt(c);
                scales[(size_t)k * dM + j] = s;
                inverse_scales[(size_t)k * dM + j] = 1.0 / s;
            }
    });
}

int mlhip_em_conditional_cdfs(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, uint32_t dM, const double* mixing, const double* means_observed,
                              const double* covariances_observed, const double* maps, const double* means_missing, const double* scales,
                              const double* inverse_scales, const double* values, int64_t ld_values, double* out, int64_t ld_out,
                              double* means_out, int64_t ld_means, double* log_density)
{
    return guarded([&] {
        const ConditionedModel m{(int)K, (int)dM, mixing, means_observed, covariances_observed, maps, means_missing};
        check_quantile_call(ctx, data, K, dM, m, scales, inverse_scales, ld_out, means_out != nullptr, ld_means);
        require(ld_values >= (int64_t)dM, "ld_values must be >= dM");
        if (!data->rows()) return;
        require(values && out, "null argument");
        QuantileCall q{};
        q.scales = scales; q.inverse_scales = inverse_scales;
        q.quantile = false; q.values = values; q.ld_values = ld_values; q.out = out; q.ld_out = ld_out;
        q.means_out = means_out; q.ld_means = ld_means; q.log_density = log_density;
        run(ctx, data, m, q);
    });
}

int mlhip_em_conditional_quantiles(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, uint32_t dM, const double* mixing, const double* means_observed,
                                   const double* covariances_observed, const double* maps, const double* means_missing, const double* scales,
                                   const double* inverse_scales, const double* probabilities, uint32_t n_probabilities, double* out,
                                   int64_t ld_out, double* means_out, int64_t ld_means, double* log_density, uint32_t* iterations)
{
    return guarded([&] {
        const ConditionedModel m{(int)K, (int)dM, mixing, means_observed, covariances_observed, maps, means_missing};
        check_quantile_call(ctx, data, K, dM, m, scales, inverse_scales, ld_out, means_out != nullptr, ld_means);
        require(n_probabilities == 0 || probabilities, "null argument");
        for (uint32_t i = 0; i < n_probabilities; ++i)
            require(probabilities[i] > 0.0 && probabilities[i] < 1.0, "a probability must lie strictly inside (0, 1)");   // (a NaN fails both)
        if (!data->rows() || !n_probabilities) return;
        require(out, "null argument");
        std::vector<double> z(n_probabilities);
        for (uint32_t i = 0; i < n_probabilities; ++i) z[i] = mlhip::normal_quantile(probabilities[i]);
        QuantileCall q{};
        q.scales = scales; q.inverse_scales = inverse_scales;
        q.quantile = true; q.probabilities = probabilities; q.z = z.data(); q.n_prob = n_probabilities; q.out = out; q.ld_out = ld_out;
        q.block_rows = data->rows(); q.means_out = means_out; q.ld_means = ld_means; q.log_density = log_density; q.iterations = iterations;
        run(ctx, data, m, q);
    });
}

int mlhip_em_condition_quantile_route(const mlhip_data* data, uint32_t K, uint32_t dM, int quantile, int* kernel)
{
    return guarded([&] {
        require(data && kernel && K >= 1 && dM >= 1 && (quantile == 0 || quantile == 1), "bad argument");
        if (!data->parts.empty()) data = data->parts[0];        // (a group's block: every shard takes the same route)
        require((uint32_t)data->d + dM <= (uint32_t)kGenericMaxDim, "observed and missing coordinates together must be 2 .. 4096");
        *kernel = condition_quantile_route(data, (int)K, (int)dM, quantile != 0, 1, false, false).kernel;
    });
}

}  // extern "C"
