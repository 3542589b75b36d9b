// mlhip_em_conditional_cdfs / mlhip_em_conditional_quantiles: the per-coordinate predictive CDF P(x_j <= v | x_O) and its inverse for
// every row of a resident block of OBSERVED coordinates under a mixture conditioned on them (the definitions: mlhip.h; the kernels:
// device/em_condition_quantile.hip; Phi: device/normal_cdf.hpp). The host conditions the model (host::condition,
// host::condition_covariances, mlhip_em_condition_scales); the device runs the marginal mixture's E-step in its exact form on chunks of
// whole tiles, exactly as mlhip_em_conditional_means does (runtime/em_condition.cpp), and behind every chunk ONE launch of the CDF
// kernel, or one launch of the quantile kernel per group of probabilities. Every buffer is the call's own, taken from the context's
// pool: the handle's E-step state, weights, ridge and label history stay as they were.
#include "internal.hpp"
#include "../device/normal_cdf.hpp"

namespace mlhip_rt {
namespace {

struct ConditionedModel {
    int K, dM;
    const double *mixing, *means_observed, *covs_observed, *maps, *means_missing, *scales, *inverse_scales;
};

struct QuantileCall {
    bool quantile;
    const double* values; int64_t ld_values;                    // CDF
    const double *probabilities, *z; uint32_t n_prob;           // quantile: the probabilities and their normal quantiles
    double* out; int64_t ld_out;
    uint64_t block_rows;                                         // quantile: rows between the blocks of two probabilities in the caller's arrays
    double* means_out; int64_t ld_means;
    double* log_density;
    uint32_t* iterations;
};

/// The conditioning kernels' records (condition_table) with [s | w] behind each, in the padded dM (+0.0 beyond dM).
std::vector<double> quantile_table(int kernel, const ConditionedModel& m, int dO)
{
    const int K = m.K, dM = m.dM;
    const std::vector<double> base = condition_table(kernel, K, dO, dM, m.means_observed, m.maps, m.means_missing, nullptr);
    const size_t ps = condition_record_doubles(kernel, dO, dM), stride = condition_quantile_record_doubles(kernel, dO, dM);
    const size_t pm = (size_t)condition_pad(kernel, dM);
    std::vector<double> table(stride * K, 0.0);
    for (int k = 0; k < K; ++k) {
        double* rec = table.data() + stride * k;
        std::copy_n(base.data() + ps * k, ps, rec);
        std::copy_n(m.scales + (size_t)k * dM, dM, rec + ps);
        std::copy_n(m.inverse_scales + (size_t)k * dM, dM, rec + ps + pm);
    }
    return table;
}

/// A chunk's rows x width elements from the device to rows `ld` elements apart on the host.
template <class T>
void download_rows(mlhip_ctx* ctx, std::vector<T>& packed, T* dst, int64_t ld, const char* src, uint32_t rows, size_t width)
{
    const bool spread = ld != (int64_t)width;
    if (spread) packed.resize((size_t)rows * width);
    download_columns(ctx, reinterpret_cast<char*>(spread ? packed.data() : dst), 0, src, 0, sizeof(T) * width * rows, 1);
    if (spread)
        for (uint32_t i = 0; i < rows; ++i) std::memcpy(dst + (int64_t)i * ld, packed.data() + (size_t)i * width, sizeof(T) * width);
}

void em_conditional_quantiles(mlhip_data* dt, const ConditionedModel& m, const QuantileCall& q)
{
    mlhip_ctx* ctx = dt->ctx;
    if (!dt->n || (q.quantile && !q.n_prob)) return;
    const int dO = dt->d, K = m.K, dM = m.dM;
    const ConditionQuantileRoute r = condition_quantile_route(dt, K, dM, q.quantile, q.n_prob, q.means_out != nullptr, q.iterations != nullptr);
    if (condition_pad(r.kernel, dO) < 0 || condition_pad(r.kernel, dM) < 0) throw Unsupported("conditional quantile kernel not instantiated for this shape");
    const uint32_t chunk = r.chunk_rows, group = q.quantile ? r.group : 1;
    const size_t ldq = ((size_t)chunk * dM + 1) & ~(size_t)1;   // (even: every probability's block starts 16-byte aligned)
    DevBuf records{&dt->pool}, work{&dt->pool}, table{&dt->pool}, lw{&dt->pool}, lse{&dt->pool}, ll{&dt->pool}, out{&dt->pool}, y{&dt->pool},
        vals{&dt->pool}, its{&dt->pool}, pz{&dt->pool};
    PinnedBuf staging{&dt->pool};
    build_records(dt, r.em, K, m.mixing, m.means_observed, m.covs_observed, false, records, staging, work);   // (always the exact form: no FOLD)
    const std::vector<double> host_table = quantile_table(r.kernel, m, dO);
    table.reserve(sizeof(double) * host_table.size());
    HIP_CHECK(hipMemcpyAsync(table.p, host_table.data(), sizeof(double) * host_table.size(), hipMemcpyHostToDevice, ctx->stream));
    if (q.quantile) {                                            // [probabilities | their normal quantiles]
        pz.reserve(sizeof(double) * 2 * q.n_prob);
        HIP_CHECK(hipMemcpyAsync(pz.p, q.probabilities, sizeof(double) * q.n_prob, hipMemcpyHostToDevice, ctx->stream));
        HIP_CHECK(hipMemcpyAsync(pz.as<double>() + q.n_prob, q.z, sizeof(double) * q.n_prob, hipMemcpyHostToDevice, ctx->stream));
    }
    lw.reserve(sizeof(double) * (size_t)chunk * K);
    lse.reserve(sizeof(double) * chunk);
    ll.reserve(sizeof(double) * kMaxLlPartials);
    out.reserve(sizeof(double) * ldq * group);
    if (q.means_out) y.reserve(sizeof(double) * (size_t)chunk * dM);
    if (!q.quantile) vals.reserve(sizeof(double) * (size_t)chunk * dM);
    if (q.iterations) its.reserve(sizeof(uint32_t) * ldq * group);
    std::vector<double> packed;                                 // a leading dimension above dM: a chunk goes up / comes down contiguous, the CPU gathers / spreads
    std::vector<uint32_t> packed_trips;
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
        ConditionQuantileArgs c{};
        c.xt = a.xt; c.ldx = a.ldx; c.n = rows; c.dO = dO; c.dM = dM; c.K = K;
        c.lw = a.lw; c.ldr = a.ldr; c.lse = a.lse;
        c.table = table.as<double>(); c.out = out.as<double>(); c.ldq = ldq;
        c.skip = r.skip; c.kernel = r.kernel;
        if (!q.quantile) {
            const double* src = q.values + (int64_t)row * q.ld_values;
            if (q.ld_values != (int64_t)dM) {
                packed.resize((size_t)rows * dM);
                for (uint32_t i = 0; i < rows; ++i) std::memcpy(packed.data() + (size_t)i * dM, src + (int64_t)i * q.ld_values, sizeof(double) * dM);
                src = packed.data();
            }
            // (`packed` is not touched again before the download below has waited for the stream, this copy included)
            HIP_CHECK(hipMemcpyAsync(vals.p, src, sizeof(double) * (size_t)rows * dM, hipMemcpyHostToDevice, ctx->stream));
            c.values = vals.as<double>();
            c.means = q.means_out ? y.as<double>() : nullptr;
            ctx->timed("em_condition_cdf", [&] { grid = launch_em_condition_cdf(c, ctx->num_cus, ctx->stream); });
            if (grid < 0) throw Unsupported("conditional CDF kernel not instantiated for this shape");
            HIP_CHECK(hipGetLastError());
            download_rows(ctx, packed, q.out + (int64_t)row * q.ld_out, q.ld_out, out.as<char>(), rows, (size_t)dM);
        }
        for (uint32_t q0 = 0; q.quantile && q0 < q.n_prob; q0 += group) {
            const uint32_t nq = std::min(group, q.n_prob - q0);
            c.probabilities = pz.as<double>() + q0; c.z = pz.as<double>() + q.n_prob + q0; c.n_prob = nq;
            c.iterations = q.iterations ? its.as<uint32_t>() : nullptr;
            c.means = q.means_out && q0 == 0 ? y.as<double>() : nullptr;   // (the first launch behind a chunk carries the mean)
            ctx->timed("em_condition_quantile", [&] { grid = launch_em_condition_quantile(c, ctx->num_cus, ctx->stream); });
            if (grid < 0) throw Unsupported("conditional quantile kernel not instantiated for this shape");
            HIP_CHECK(hipGetLastError());
            // (the copies wait for the stream: the scratch is free for the next launch, and host_table for the end of the call)
            for (uint32_t g = 0; g < nq; ++g) {
                const int64_t at = (int64_t)((uint64_t)(q0 + g) * q.block_rows + row);
                download_rows(ctx, packed, q.out + at * q.ld_out, q.ld_out, out.as<char>() + sizeof(double) * ldq * g, rows, (size_t)dM);
                if (q.iterations)
                    download_rows(ctx, packed_trips, q.iterations + at * (int64_t)dM, (int64_t)dM, its.as<char>() + sizeof(uint32_t) * ldq * g, rows,
                                  (size_t)dM);
            }
        }
        if (q.means_out) download_rows(ctx, packed, q.means_out + (int64_t)row * q.ld_means, q.ld_means, y.as<char>(), rows, (size_t)dM);
        if (q.log_density) {
            download_columns(ctx, reinterpret_cast<char*>(q.log_density + row), 0, lse.as<char>(), 0, sizeof(double) * rows, 1);
            for (uint32_t i = 0; i < rows; ++i) q.log_density[row + i] -= offset;
        }
    }
    ctx->sync();
}

/// The checks both calls share, before any device work; returns dO.
uint32_t check_quantile_call(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, uint32_t dM, const ConditionedModel& m, int64_t ld_out, bool with_means,
                             int64_t ld_means)
{
    check_call(ctx, data, K);
    require(m.mixing && m.means_observed && m.covs_observed && m.maps && m.means_missing && m.scales && m.inverse_scales, "null argument");
    const uint32_t dO = (uint32_t)(data->parts.empty() ? data->d : data->parts[0]->d);
    require(dM >= 1 && dO + dM <= (uint32_t)kGenericMaxDim, "observed and missing coordinates together must be 2 .. 4096");
    require(ld_out >= (int64_t)dM, "ld_out must be >= dM");
    require(!with_means || ld_means >= (int64_t)dM, "ld_means must be >= dM");
    return dO;
}

/// One call on a single context's block, or on every shard of a group's: each shard handles its own rows, no collective, nothing to
/// put together but the rows' places in the caller's arrays.
void run(mlhip_ctx* ctx, mlhip_data* data, const ConditionedModel& m, const QuantileCall& q)
{
    if (!ctx->group) {
        em_conditional_quantiles(data, m, q);
        return;
    }
    fan_out(ctx, data, [&](Shard& sh) {
        return guarded([&] {
            sh.ctx->use();
            QuantileCall part = q;
            part.values = q.values ? sh.rows(q.values, q.ld_values) : nullptr;
            part.out = sh.rows(q.out, q.ld_out);
            part.means_out = sh.rows(q.means_out, q.ld_means);
            part.log_density = sh.rows(q.log_density);
            part.iterations = sh.rows(q.iterations, (int64_t)m.dM);
            em_conditional_quantiles(sh.part, m, part);
        });
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
        const ConditionedModel m{(int)K, (int)dM, mixing, means_observed, covariances_observed, maps, means_missing, scales, inverse_scales};
        check_quantile_call(ctx, data, K, dM, m, ld_out, means_out != nullptr, ld_means);
        require(ld_values >= (int64_t)dM, "ld_values must be >= dM");
        if (!data->rows()) return;
        require(values && out, "null argument");
        QuantileCall q{};
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
        const ConditionedModel m{(int)K, (int)dM, mixing, means_observed, covariances_observed, maps, means_missing, scales, inverse_scales};
        check_quantile_call(ctx, data, K, dM, m, ld_out, means_out != nullptr, ld_means);
        require(n_probabilities == 0 || probabilities, "null argument");
        for (uint32_t i = 0; i < n_probabilities; ++i)
            require(probabilities[i] > 0.0 && probabilities[i] < 1.0, "a probability must lie strictly inside (0, 1)");   // (a NaN fails both)
        if (!data->rows() || !n_probabilities) return;
        require(out, "null argument");
        std::vector<double> z(n_probabilities);
        for (uint32_t i = 0; i < n_probabilities; ++i) z[i] = mlhip::normal_quantile(probabilities[i]);
        QuantileCall q{};
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
