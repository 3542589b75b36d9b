// mlhip_em_condition_covariances / mlhip_em_conditional_samples: draws from p(x_M | x_O) for every row of a resident block of OBSERVED
// coordinates (the definition: mlhip.h; the kernels: device/em_condition_sample.hip). The host conditions the model (host::condition,
// host::condition_covariances); the device runs the conditioning pass (ConditionPass, runtime/em_condition.cpp) with the drawing
// kernel behind every chunk, a group of draws per launch. A row's draw is a pure function of its global index, the draw's number and
// the seed, so the chunks, the groups of draws and the shards of a device group leave no seam.
#include "internal.hpp"

namespace mlhip_rt {
namespace {

/// `factors`: K x dM x dM row-major lower factors of the conditioned covariances. `out` / `labels`: the block's rows of the caller's
/// arrays, whose draws lie `draw_rows` rows apart (the whole sample's row count: a shard's rows sit inside every draw's block of the
/// caller's).
void em_conditional_samples(mlhip_data* dt, const ConditionedModel& m, const double* factors, uint64_t seed, uint64_t first_row,
                            uint32_t first_draw, uint32_t n_draws, double* out, int64_t ld_out, uint64_t draw_rows, uint32_t* labels)
{
    mlhip_ctx* ctx = dt->ctx;
    if (!dt->n || !n_draws) return;
    const int dO = dt->d, dM = m.dM;
    const ConditionSampleRoute r = condition_sample_route(dt, m.K, dM, n_draws);
    const uint32_t chunk = r.chunk_rows;
    const size_t ldq = ((size_t)chunk * dM + 1) & ~(size_t)1;  // (even: every draw's block starts 16-byte aligned)
    // the record's tail: the factor's lower triangle packed row by row, in the padded dM
    const size_t tail = condition_sample_record_doubles(r.kernel, dO, dM) - condition_record_doubles(r.kernel, dO, dM);
    ConditionPass pass(dt, m, r.em, r.kernel, chunk, tail, [&](int k, double* g) {
        const double* G = factors + (size_t)k * dM * dM;
        for (int j = 0; j < dM; ++j)
            for (int c = 0; c <= j; ++c) g[(size_t)j * (j + 1) / 2 + c] = G[(size_t)j * dM + c];
    }, "conditional sampling kernel not instantiated for this shape");
    DevBuf y{&dt->pool}, lb{&dt->pool};
    y.reserve(sizeof(double) * ldq * r.draws);
    if (labels) lb.reserve(sizeof(uint32_t) * (size_t)chunk * r.draws);
    pass.run(nullptr, [&](const ConditionChunk& chunk_args, uint32_t row) {
        const uint32_t rows = chunk_args.n;
        for (uint32_t q0 = 0; q0 < n_draws; q0 += r.draws) {
            const uint32_t nq = std::min(r.draws, n_draws - q0);
            ConditionSampleArgs c{};
            static_cast<ConditionChunk&>(c) = chunk_args;
            c.seed = seed; c.first_row = first_row + row; c.first_draw = first_draw + q0; c.n_draws = nq;
            c.out = y.as<double>(); c.ldq = ldq; c.labels = labels ? lb.as<uint32_t>() : nullptr;
            int grid = 0;
            ctx->timed("em_condition_sample", [&] { grid = launch_em_condition_sample(c, ctx->num_cus, ctx->stream); });
            if (grid < 0) throw Unsupported("conditional sampling kernel not instantiated for this shape");
            HIP_CHECK(hipGetLastError());
            for (uint32_t g = 0; g < nq; ++g) {
                const int64_t at = (int64_t)((uint64_t)(q0 + g) * draw_rows + row);
                pass.download_rows(out + at * ld_out, ld_out, y.as<double>() + ldq * g, rows, (size_t)dM);
                if (labels) pass.download_rows(labels + at, 1, lb.as<uint32_t>() + (size_t)rows * g, rows, 1);
            }
        }
    });
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
        const ConditionedModel m{(int)K, (int)dM, mixing, means_observed, covariances_observed, maps, means_missing};
        // (every shard draws for its own rows under their global indices)
        on_block_or_shards(ctx, data, [&](Shard& sh) {
            em_conditional_samples(sh.part, m, factors, seed, first_row + sh.first_row, first_draw, n_draws, sh.rows(out, ld_out), ld_out, n,
                                   sh.rows(labels));
        });
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
