// mlhip_em_condition_covariances / mlhip_em_conditional_samples: draws from p(x_M | x_O) for every row of a resident block of OBSERVED
// coordinates (the definition: mlhip.h; the kernels: device/em_condition_sample.hip). The host conditions the model (host::condition,
// host::condition_covariances); the device runs the marginal mixture's E-step in its exact form on chunks of whole tiles, exactly as
// mlhip_em_conditional_means does (runtime/em_condition.cpp), and the drawing kernel behind every chunk, a group of draws per launch.
// A row's draw is a pure function of its global index, the draw's number and the seed, so the chunks, the groups of draws and the
// shards of a device group leave no seam. Every buffer is the call's own, taken from the context's pool: the handle's E-step state,
// weights, ridge and label history stay as they were.
#include "internal.hpp"

namespace mlhip_rt {
namespace {

struct ConditionedModel {
    int K, dM;
    const double *mixing, *means_observed, *covs_observed, *maps, *means_missing, *factors;
};

/// `out` / `labels`: the block's rows of the caller's arrays, whose draws lie `draw_rows` rows apart (the whole sample's row count:
/// a shard's rows sit inside every draw's block of the caller's).
void em_conditional_samples(mlhip_data* dt, const ConditionedModel& m, uint64_t seed, uint64_t first_row, uint32_t first_draw, uint32_t n_draws,
                            double* out, int64_t ld_out, uint64_t draw_rows, uint32_t* labels)
{
    mlhip_ctx* ctx = dt->ctx;
    if (!dt->n || !n_draws) return;
    const int dO = dt->d, K = m.K, dM = m.dM;
    const ConditionSampleRoute r = condition_sample_route(dt, K, dM, n_draws);
    if (condition_pad(r.kernel, dO) < 0 || condition_pad(r.kernel, dM) < 0) throw Unsupported("conditional sampling kernel not instantiated for this shape");
    const uint32_t chunk = r.chunk_rows;
    const size_t ldq = ((size_t)chunk * dM + 1) & ~(size_t)1;  // (even: every draw's block starts 16-byte aligned)
    DevBuf records{&dt->pool}, work{&dt->pool}, table{&dt->pool}, lw{&dt->pool}, lse{&dt->pool}, ll{&dt->pool}, y{&dt->pool}, lb{&dt->pool};
    PinnedBuf staging{&dt->pool};
    build_records(dt, r.em, K, m.mixing, m.means_observed, m.covs_observed, false, records, staging, work);   // (always the exact form: no FOLD)
    const std::vector<double> host_table = condition_table(r.kernel, K, dO, dM, m.means_observed, m.maps, m.means_missing, m.factors);
    table.reserve(sizeof(double) * host_table.size());
    HIP_CHECK(hipMemcpyAsync(table.p, host_table.data(), sizeof(double) * host_table.size(), hipMemcpyHostToDevice, ctx->stream));
    lw.reserve(sizeof(double) * (size_t)chunk * K);
    lse.reserve(sizeof(double) * chunk);
    ll.reserve(sizeof(double) * kMaxLlPartials);
    y.reserve(sizeof(double) * ldq * r.draws);
    if (labels) lb.reserve(sizeof(uint32_t) * (size_t)chunk * r.draws);
    std::vector<double> packed;                                 // ld_out > dM: a draw's rows come down contiguous and are spread by the CPU
    if (ld_out != (int64_t)dM) packed.resize((size_t)std::min(chunk, dt->n) * dM);
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
        for (uint32_t q0 = 0; q0 < n_draws; q0 += r.draws) {
            const uint32_t nq = std::min(r.draws, n_draws - q0);
            ConditionSampleArgs c{};
            c.xt = a.xt; c.ldx = a.ldx; c.n = rows; c.dO = dO; c.dM = dM; c.K = K;
            c.lw = a.lw; c.ldr = a.ldr; c.lse = a.lse;
            c.table = table.as<double>();
            c.seed = seed; c.first_row = first_row + row; c.first_draw = first_draw + q0; c.n_draws = nq;
            c.out = y.as<double>(); c.ldq = ldq; c.labels = labels ? lb.as<uint32_t>() : nullptr;
            c.kernel = r.kernel;
            ctx->timed("em_condition_sample", [&] { grid = launch_em_condition_sample(c, ctx->num_cus, ctx->stream); });
            if (grid < 0) throw Unsupported("conditional sampling kernel not instantiated for this shape");
            HIP_CHECK(hipGetLastError());
            // (the copies wait for the stream: the scratch is free for the next launch, and host_table for the end of the call)
            for (uint32_t g = 0; g < nq; ++g) {
                const int64_t at = (int64_t)((uint64_t)(q0 + g) * draw_rows + row);
                double* dst = out + at * ld_out;
                download_columns(ctx, reinterpret_cast<char*>(packed.empty() ? dst : packed.data()), 0, y.as<char>() + sizeof(double) * ldq * g, 0,
                                 sizeof(double) * dM * rows, 1);
                if (!packed.empty())
                    for (uint32_t i = 0; i < rows; ++i) std::memcpy(dst + (int64_t)i * ld_out, packed.data() + (size_t)i * dM, sizeof(double) * dM);
                if (labels)
                    download_columns(ctx, reinterpret_cast<char*>(labels + at), 0, lb.as<char>() + sizeof(uint32_t) * (size_t)rows * g, 0,
                                     sizeof(uint32_t) * rows, 1);
            }
        }
    }
    ctx->sync();
}

}  // namespace
}  // namespace mlhip_rt

extern "C" {

int mlhip_em_condition_covariances(uint32_t d, uint32_t K, int covariance_type, const double* covariances, const uint32_t* observed,
                                   uint32_t n_observed, double* covariances_missing, double* factors)
{
    return guarded([&] {
        require(covariances && observed && covariances_missing, "null argument");
        const Covariance mode = check_condition_arguments(d, K, covariance_type, observed, n_observed);
        try {
            host::condition_covariances(mode, (int)K, (int)d, covariances, observed, (int)n_observed, covariances_missing, factors);
        } catch (const std::domain_error& e) {
            throw DomainError(e.what());
        }
    });
}

int mlhip_em_conditional_samples(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, uint32_t dM, const double* mixing, const double* means_observed,
                                 const double* covariances_observed, const double* maps, const double* means_missing, const double* factors,
                                 uint64_t seed, uint64_t first_row, uint32_t first_draw, uint32_t n_draws, double* out, int64_t ld_out,
                                 uint32_t* labels)
{
    return guarded([&] {
        check_call(ctx, data, K);
        require(mixing && means_observed && covariances_observed && maps && means_missing && factors, "null argument");
        const uint32_t dO = (uint32_t)(data->parts.empty() ? data->d : data->parts[0]->d);
        require(dM >= 1 && dO + dM <= (uint32_t)kGenericMaxDim, "observed and missing coordinates together must be 2 .. 4096");
        require(ld_out >= (int64_t)dM, "ld_out must be >= dM");
        require((uint64_t)first_draw + n_draws <= 0xFFFFFFFFull, "first_draw + n_draws must be <= 2^32 - 1");
        const uint64_t n = data->rows();
        require(first_row + n >= first_row, "first_row + n must fit 64 bits");
        if (!n || !n_draws) return;
        require(out, "null argument");
        const ConditionedModel m{(int)K, (int)dM, mixing, means_observed, covariances_observed, maps, means_missing, factors};
        if (ctx->group) {
            // (every shard draws for its own rows under their global indices: no collective, nothing to put together but the rows'
            // places in every draw's block of the caller's arrays)
            fan_out(ctx, data, [&](Shard& sh) {
                return guarded([&] {
                    sh.ctx->use();
                    em_conditional_samples(sh.part, m, seed, first_row + sh.first_row, first_draw, n_draws, sh.rows(out, ld_out), ld_out, n,
                                           sh.rows(labels));
                });
            });
            return;
        }
        em_conditional_samples(data, m, seed, first_row, first_draw, n_draws, out, ld_out, n, labels);
    });
}

int mlhip_em_conditional_sample_route(const mlhip_data* data, uint32_t K, uint32_t dM, int* kernel)
{
    return guarded([&] {
        require(data && kernel && K >= 1 && dM >= 1, "bad argument");
        if (!data->parts.empty()) data = data->parts[0];        // (a group's block: every shard takes the same route)
        require((uint32_t)data->d + dM <= (uint32_t)kGenericMaxDim, "observed and missing coordinates together must be 2 .. 4096");
        *kernel = condition_sample_route(data, (int)K, (int)dM, 1).kernel;
    });
}

}  // extern "C"
