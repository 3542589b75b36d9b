// mlhip_em_score: per-sample log-density and label of a resident block under caller-given mixture parameters -- the batch form of
// EM::assign_responsibilities (reference ML/EM.cpp:176-188). One pass, no N x K block; every buffer is the call's own (taken from the
// context's pool, given back at the end), so what earlier calls left on the handle -- E-step results, records, label history, the
// statistics pass's call history -- stays as it was.
#include "internal.hpp"

namespace mlhip_rt {
namespace {

/// The composed route: the E-step kernel of `r.em` in its LSE-writing form on chunks of r.chunk_rows rows into a scratch block of
/// K x chunk doubles, each followed by em_score_finish_kernel.
void score_composed(mlhip_data* dt, const ScoreRoute& r, int K, const DevBuf& records, double* lse_out, uint32_t* labels_out)
{
    mlhip_ctx* ctx = dt->ctx;
    ChunkEstep estep(dt);
    estep.reserve(K, r.chunk_rows);
    for (uint32_t row = 0; row < dt->n; row += estep.chunk) {
        const uint32_t rows = std::min(estep.chunk, dt->n - row);   // (padded_samples(rows) <= chunk: the chunk is whole tiles)
        estep.launch(dt, r.em, K, records, row, rows);
        ctx->timed("em_score", [&] {
            launch_em_score_finish(estep.lw.as<double>(), estep.chunk, estep.lse.as<double>(), rows, K, lse_out ? lse_out + row : nullptr,
                                   labels_out ? labels_out + row : nullptr, ctx->stream);
        });
        HIP_CHECK(hipGetLastError());
    }
    ctx->sync();                                         // (the scratch goes back to the pool behind the last kernel)
}

void em_score(mlhip_data* dt, int K, Covariance mode, const double* mixing, const double* means, const double* covs, double* log_density,
              uint32_t* labels)
{
    mlhip_ctx* ctx = dt->ctx;
    if (!dt->n || (!log_density && !labels)) return;
    const ScoreRoute r = score_route(dt, K);
    const int d = dt->d;
    std::vector<double> full;
    if (mode != Covariance::Full) {
        // The same kernels on diagonal matrices, as ensure_lw (em.cpp) does after a diagonal step, or on K components that all carry
        // the one tied covariance; no kernels of their own. The record builders work per component, so the tied matrix is factored K
        // times: K - 1 wasted factorizations, microseconds at d <= 32 but K d^3 / 3 flop each at large d (on the device above d = 64)
        // -- records derived from one factorization are not built
        full = as_full(mode, K, d, covs);
        covs = full.data();
    }
    DevBuf records{&dt->pool}, work{&dt->pool}, lse_dev{&dt->pool}, labels_dev{&dt->pool};
    PinnedBuf staging{&dt->pool};
    build_records(dt, r.em, K, mixing, means, covs, false, records, staging, work);   // (always the exact form: no FOLD)
    if (log_density) lse_dev.reserve(sizeof(double) * dt->n_pad);
    if (labels) labels_dev.reserve(sizeof(uint32_t) * dt->n_pad);
    if (r.kernel == kScoreComposed) {
        score_composed(dt, r, K, records, lse_dev.as<double>(), labels_dev.as<uint32_t>());
    } else {
        ScoreArgs a{};
        a.xt = dt->xt.as<double>(); a.ldx = dt->ldx; a.n = dt->n; a.D = dt->D;
        a.params = records.as<double>(); a.K = K;
        a.lse = lse_dev.as<double>(); a.labels = labels_dev.as<uint32_t>();
        int grid = 0;
        ctx->timed("em_score", [&] {
            grid = r.kernel == kScoreMatrix4 ? launch_em_score_mfma4(a, ctx->num_cus, ctx->stream) : launch_em_score(a, ctx->stream);
        });
        if (grid < 0) throw Unsupported("score kernel not instantiated for this dimension");
        HIP_CHECK(hipGetLastError());
        ctx->sync();
    }
    if (labels) download_columns(ctx, reinterpret_cast<char*>(labels), 0, labels_dev.as<char>(), 0, sizeof(uint32_t) * dt->n, 1);
    if (log_density) {
        download_columns(ctx, reinterpret_cast<char*>(log_density), 0, lse_dev.as<char>(), 0, sizeof(double) * dt->n, 1);
        // the kernels' lw leave the density's constant out, like the E-step's (ML/EM.cpp:197-198 applies it to the mean)
        const double offset = (double)d * log_two_pi() / 2;
        for (uint32_t i = 0; i < dt->n; ++i) log_density[i] -= offset;
    }
}

}  // namespace
}  // namespace mlhip_rt

extern "C" {

int mlhip_em_score(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, int covariance_type, const double* mixing, const double* means,
                   const double* covariances, double* log_density, uint32_t* labels)
{
    return guarded([&] {
        check_call(ctx, data, K);
        require(mixing && means && covariances, "null argument");
        const Covariance mode = covariance_from_abi(covariance_type);
        if (ctx->group) {
            // (every shard scores its own rows: no collective, nothing to put together but the rows' places in the caller's arrays)
            fan_out(ctx, data, [&](Shard& sh) {
                return mlhip_em_score(sh.ctx, sh.part, K, covariance_type, mixing, means, covariances, sh.rows(log_density), sh.rows(labels));
            });
            return;
        }
        em_score(data, (int)K, mode, mixing, means, covariances, log_density, labels);
    });
}

int mlhip_em_score_route(const mlhip_data* data, uint32_t K, int* kernel)
{
    return guarded([&] {
        require(data && kernel && K >= 1, "bad argument");
        if (!data->parts.empty()) data = data->parts[0];        // (a group's block: every shard takes the same route)
        static_assert(kScoreScalarFed == MLHIP_SCORE_SCALAR_FED && kScoreMatrix4 == MLHIP_SCORE_MATRIX4 && kScoreComposed == MLHIP_SCORE_COMPOSED,
                      "mlhip.h names the kernels by ScoreKernel");
        *kernel = score_route(data, (int)K).kernel;
    });
}

}  // extern "C"
