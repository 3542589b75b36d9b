// Routes: which kernels one EM or K-means entry-point call runs. The shape rules are the kernels' own (device/*.hip, plain functions
// of the shape); the routing switches of DESIGN.md §7 are read here, once per call, and nowhere else.
#include "internal.hpp"

namespace mlhip_rt {
namespace {

/// First character of an environment variable; '\0' when it is unset or empty.
char env_char(const char* name)
{
    const char* e = std::getenv(name);
    return e ? e[0] : '\0';
}

/// 0 / 1 when the variable starts with that digit, -1 (automatic) otherwise.
int env_force(const char* name)
{
    const char c = env_char(name);
    return c == '0' || c == '1' ? c - '0' : -1;
}

struct Switches {
    bool estep_valu;            // MLHIP_ESTEP=valu
    bool estep_rows;            // off under MLHIP_ESTEP_ORDER=column
    bool fold, self_norm, balanced, fused, diag_ab, big_dim, device_close, records, resident;   // on unless "0"
    int sparse, sfeed;          // MLHIP_MSTATS_SPARSE, MLHIP_FUSED_SFEED: 0 / 1 forced, -1 automatic
    int screen;                 // MLHIP_ESTEP_SCREEN: 0 / 1 forced, -1 automatic
    int fused_valu;             // MLHIP_FUSED_VALU: 0 never, 2 wherever built, -1 by shape
    int kmeans;                 // MLHIP_KMEANS=valu / mfma: kKmDirect / kKmMatrix forced, -1 automatic
    bool score_composed;        // MLHIP_SCORE=composed
    long score_rows;            // MLHIP_SCORE_ROWS=n: rows per chunk of the composed scoring route (0: by the scratch bound)
    int tied;                   // MLHIP_TIED=composed / kernel: kTiedComposed / kTiedKernel forced (the kernel: where it exists), -1 automatic
    int restarts;               // MLHIP_EM_RESTARTS=sequential / batch: kRestartsSequential / kRestartsBatched forced (the batch: where it exists), -1 automatic
    bool sample_global;         // MLHIP_SAMPLE_TABLE=global: the sampler reads its table from global memory where it would fit LDS
    long sample_rows;           // MLHIP_SAMPLE_ROWS=n: rows per chunk of the host-output sampler (0: by kSampleChunkBytes)
    bool condition_plain;       // MLHIP_CONDITION=plain: the conditioning pass takes its plain tier at every shape
    long condition_rows;        // MLHIP_CONDITION_ROWS=n: rows per chunk of the conditioning pass (0: by the scratch bound)
    bool condition_skip;        // on unless MLHIP_CONDITION_SKIP=0: components without a share in a wave's rows are passed over
    long condition_group;       // MLHIP_CONDITION_GROUP=n: at most n probabilities per launch of the quantile search (0: as many as fit the scratch bound)
    bool silhouette_plain;      // MLHIP_SILHOUETTE=plain: the silhouette takes its plain tier at every d
    int silhouette_feed;        // MLHIP_SILHOUETTE_FEED=scalar / lds: kSilhouetteScalarFeed / kSilhouetteLdsFeed forced, -1 automatic
    long silhouette_rows;       // MLHIP_SILHOUETTE_ROWS=n: evaluated rows per block (0: by the scratch bound)
    long silhouette_grid;       // MLHIP_SILHOUETTE_GRID=n: workgroups of the pair kernel (0: by the CU count)
    int impute;                 // MLHIP_IMPUTE=composed / kernel: kImputeComposed / kImputeKernel forced where it exists, -1 automatic
    long impute_rows;           // MLHIP_IMPUTE_ROWS=n: rows per chunk of mlhip_em_impute (0: by the route's bound)
    long impute_patterns;       // MLHIP_IMPUTE_PATTERNS=n: patterns whose records the kernel route builds at a time (0: by the scratch bound)
    long impute_grid;           // MLHIP_IMPUTE_GRID=n: at most n workgroups per evaluation launch (0: by the CU count; the tests' switch)
};

Switches read_switches()
{
    Switches s;
    const char* estep = std::getenv("MLHIP_ESTEP");
    s.estep_valu = estep && std::strcmp(estep, "valu") == 0;
    s.fold = env_char("MLHIP_ESTEP_FOLD") != '0';
    const char* order = std::getenv("MLHIP_ESTEP_ORDER");
    s.estep_rows = !(order && std::strcmp(order, "column") == 0);
    s.self_norm = env_char("MLHIP_SELF_NORM") != '0';
    s.balanced = env_char("MLHIP_MSTATS_BALANCED") != '0';
    s.fused = env_char("MLHIP_FUSED") != '0';
    s.diag_ab = env_char("MLHIP_DIAG_AB") != '0';
    s.big_dim = env_char("MLHIP_BIG_DIM") != '0';
    s.device_close = env_char("MLHIP_DEVICE_CLOSE") != '0';
    const int records = env_force("MLHIP_DEVICE_RECORDS");   // (unset: follows MLHIP_DEVICE_CLOSE)
    s.records = records >= 0 ? records == 1 : s.device_close;
    s.resident = env_char("MLHIP_RESIDENT") != '0';
    s.sparse = env_force("MLHIP_MSTATS_SPARSE");
    s.sfeed = env_force("MLHIP_FUSED_SFEED");
    s.screen = env_force("MLHIP_ESTEP_SCREEN");
    const char valu = env_char("MLHIP_FUSED_VALU");
    s.fused_valu = valu == '0' ? 0 : valu == '2' ? 2 : -1;
    const char km = env_char("MLHIP_KMEANS");
    s.kmeans = km == 'v' ? kKmDirect : km == 'm' ? kKmMatrix : -1;
    const char* score = std::getenv("MLHIP_SCORE");
    s.score_composed = score && std::strcmp(score, "composed") == 0;
    const char* rows = std::getenv("MLHIP_SCORE_ROWS");
    s.score_rows = rows && *rows ? std::atol(rows) : 0;
    const char* tied = std::getenv("MLHIP_TIED");
    s.tied = !tied ? -1 : std::strcmp(tied, "composed") == 0 ? kTiedComposed : std::strcmp(tied, "kernel") == 0 ? kTiedKernel : -1;
    const char* restarts = std::getenv("MLHIP_EM_RESTARTS");
    s.restarts = !restarts ? -1 : std::strcmp(restarts, "sequential") == 0 ? kRestartsSequential : std::strcmp(restarts, "batch") == 0 ? kRestartsBatched : -1;
    const char* sample_table = std::getenv("MLHIP_SAMPLE_TABLE");
    s.sample_global = sample_table && std::strcmp(sample_table, "global") == 0;
    const char* sample_rows = std::getenv("MLHIP_SAMPLE_ROWS");
    s.sample_rows = sample_rows && *sample_rows ? std::atol(sample_rows) : 0;
    const char* condition = std::getenv("MLHIP_CONDITION");
    s.condition_plain = condition && std::strcmp(condition, "plain") == 0;
    const char* condition_rows = std::getenv("MLHIP_CONDITION_ROWS");
    s.condition_rows = condition_rows && *condition_rows ? std::atol(condition_rows) : 0;
    s.condition_skip = env_char("MLHIP_CONDITION_SKIP") != '0';
    const char* condition_group = std::getenv("MLHIP_CONDITION_GROUP");
    s.condition_group = condition_group && *condition_group ? std::atol(condition_group) : 0;
    const char* silhouette = std::getenv("MLHIP_SILHOUETTE");
    s.silhouette_plain = silhouette && std::strcmp(silhouette, "plain") == 0;
    const char* feed = std::getenv("MLHIP_SILHOUETTE_FEED");
    s.silhouette_feed = !feed ? -1 : std::strcmp(feed, "scalar") == 0 ? kSilhouetteScalarFeed : std::strcmp(feed, "lds") == 0 ? kSilhouetteLdsFeed : -1;
    const char* silhouette_rows = std::getenv("MLHIP_SILHOUETTE_ROWS");
    s.silhouette_rows = silhouette_rows && *silhouette_rows ? std::atol(silhouette_rows) : 0;
    const char* silhouette_grid = std::getenv("MLHIP_SILHOUETTE_GRID");
    s.silhouette_grid = silhouette_grid && *silhouette_grid ? std::atol(silhouette_grid) : 0;
    const char* impute = std::getenv("MLHIP_IMPUTE");
    s.impute = !impute ? -1 : std::strcmp(impute, "composed") == 0 ? kImputeComposed : std::strcmp(impute, "kernel") == 0 ? kImputeKernel : -1;
    const char* impute_rows = std::getenv("MLHIP_IMPUTE_ROWS");
    s.impute_rows = impute_rows && *impute_rows ? std::atol(impute_rows) : 0;
    const char* impute_patterns = std::getenv("MLHIP_IMPUTE_PATTERNS");
    s.impute_patterns = impute_patterns && *impute_patterns ? std::atol(impute_patterns) : 0;
    const char* impute_grid = std::getenv("MLHIP_IMPUTE_GRID");
    s.impute_grid = impute_grid && *impute_grid ? std::atol(impute_grid) : 0;
    return s;
}

}  // namespace

SampleRoute sample_route(int d, uint32_t K)
{
    const Switches sw = read_switches();
    SampleRoute r;
    r.kernel = em_sample_route(d, K);
    if (r.kernel == kSampleLdsTable && sw.sample_global) r.kernel = kSampleGlobalTable;
    const uint64_t rows = sw.sample_rows > 0 ? (uint64_t)sw.sample_rows : (kSampleChunkBytes / (sizeof(double) * (uint64_t)d)) & ~uint64_t(63);
    r.chunk_rows = std::max<uint64_t>(rows, 64);
    return r;
}

EmRoute em_route(const mlhip_data* data, int K, Covariance mode)
{
    const bool diag = mode == Covariance::Diagonal;
    const Switches sw = read_switches();
    const mlhip_ctx* ctx = data->ctx;
    const int d = data->d, D = data->D;
    // A weighted block (mlhip_data_set_weights) runs the E-step tier of its shape and either the self-normalising wide statistics
    // kernel in its weighted form or the statistics kernels on w_i r_ik: the fused, resident and diagonal kernels and the sparse
    // statistics kernel have no weighted form.
    const bool weighted = data->weighted;
    const bool diag_kernel = diag && !weighted && mstats::em_diag_supported(d, K);
    EmRoute r;
    r.diag_kernel = diag_kernel;
    if (estep_mfma4_supported(D) && !(D <= kRegDim && sw.estep_valu)) r.estep = Estep::kMatrix4;
    else if (D <= kMaxDim) r.estep = Estep::kScalarFed;
    else r.estep = sw.big_dim && big_dim_applies(D) ? Estep::kBigDim : Estep::kPlain;
    r.records_on_device = sw.records && em_close_big_supported(d);
    r.fold_allowed = sw.fold && D <= kRegDim;
    r.estep_rows = sw.estep_rows && r.estep == Estep::kMatrix4 && estep_mfma4_row_major_built(D);
    // (the fused kernel reads the scalar-fed E-step's records)
    r.fused = !diag_kernel && !weighted && sw.fused && r.estep == Estep::kScalarFed && mstats::em_fused_supported(d, K);
    if (r.fused) {
        if (sw.fused_valu != 0 && mstats::em_fused_valu_supported(d, K) &&
            (sw.fused_valu == 2 || mstats::em_fused_valu_preferred(d, K, data->n)))
            r.fused_form = kFusedValu;
        else if (sw.sfeed >= 0 && mstats::em_fused_lds_feed_supported(d))
            r.fused_form = sw.sfeed ? kFusedScalarFeed : kFusedLdsFeed;
        else
            r.fused_form = mstats::em_fused_scalar_feed(d, data->n) ? kFusedScalarFeed : kFusedLdsFeed;
    }
    // K within one row-block group of the wide statistics kernel: one exp per pair in the iteration (MLHIP_ESTEP=valu: at no d)
    r.self_norm = !diag_kernel && !r.fused && sw.self_norm && !sw.estep_valu && r.estep == Estep::kMatrix4 &&
                  em_mstats_self_norm_supported(d, K, ctx->num_cus);
    r.sparse = weighted ? 0 : sw.sparse;
    r.screen = weighted ? 0 : sw.screen;
    r.balanced = sw.balanced;
    r.diag_exact = !sw.diag_ab;
    r.device_close = sw.device_close && em_close_supported(d) && (!diag || diag_kernel);
    // single rank, the vector-unit form (em_loop.cpp checks the grid)
    r.resident = sw.resident && r.fused && r.fused_form == kFusedValu && !ctx->reduce_fn && ctx->world_size <= 1;
    // The composed route is the tied mode's accurate one (it is where the kernel's weighted, large and ill-conditioned cases go, and
    // what the kernel is compared with): its matrix-core E-step takes the exact form, never FOLD, whose 1e-13 in a
    // log-responsibility would be the route's largest error (tests/test_gpu_tied_hp.py, reach 0.9 x 64: 1.1e-14 against 1.9e-15).
    if (mode == Covariance::Tied) r.fold_allowed = false;
    return r;
}

ScoreRoute score_route(const mlhip_data* data, int K)
{
    const Switches sw = read_switches();
    ScoreRoute r;
    r.em = em_route(data, K, Covariance::Full);
    if (sw.score_composed || r.em.estep == Estep::kBigDim || r.em.estep == Estep::kPlain) r.kernel = kScoreComposed;
    else r.kernel = r.em.estep == Estep::kMatrix4 ? kScoreMatrix4 : kScoreScalarFed;
    // the composed route's scratch: the largest whole number of sample tiles whose K x rows doubles stay within kScoreScratchBytes
    uint64_t rows = sw.score_rows > 0 ? (uint64_t)sw.score_rows : kScoreScratchBytes / (sizeof(double) * (uint64_t)K);
    rows = rows / kSampleTile * kSampleTile;
    if (rows < (uint64_t)kSampleTile) rows = kSampleTile;
    if (rows > data->n_pad) rows = data->n_pad;
    r.chunk_rows = (uint32_t)rows;
    return r;
}

namespace {

/// Rows per chunk of a conditioning call whose scratch takes `per_row` doubles a row: the largest whole number of sample tiles within
/// kScoreScratchBytes -- MLHIP_CONDITION_ROWS=n overrides, rounded UP to whole tiles --, at least one tile and at most the block.
uint32_t condition_chunk_rows(const Switches& sw, const mlhip_data* data, uint64_t per_row)
{
    const uint64_t tile = kSampleTile;
    uint64_t rows = sw.condition_rows > 0 ? (uint64_t)sw.condition_rows : kScoreScratchBytes / sizeof(double) / per_row;
    rows = sw.condition_rows > 0 ? (rows + tile - 1) / tile * tile : rows / tile * tile;
    if (rows < tile) rows = tile;
    if (rows > data->n_pad) rows = data->n_pad;
    return (uint32_t)rows;
}

}  // namespace

ConditionRoute condition_route(const mlhip_data* data, int K, int dM)
{
    const Switches sw = read_switches();
    ConditionRoute r;
    r.em = em_route(data, K, Covariance::Full);
    r.kernel = sw.condition_plain ? kConditionPlain : em_condition_route(data->d, dM);
    r.skip = sw.condition_skip;
    r.chunk_rows = condition_chunk_rows(sw, data, (uint64_t)K + (uint64_t)dM);
    return r;
}

ConditionRoute condition_variance_route(const mlhip_data* data, int K, int dM, bool full, bool with_means)
{
    const Switches sw = read_switches();
    ConditionRoute r;
    r.em = em_route(data, K, Covariance::Full);
    r.kernel = sw.condition_plain ? kConditionPlain : em_condition_variance_route(data->d, dM, full);
    r.skip = sw.condition_skip;
    const uint64_t per_row = (uint64_t)K + (full ? (uint64_t)dM * dM : (uint64_t)dM) + (with_means ? (uint64_t)dM : 0) +
                             (r.kernel == kConditionPlain ? 2 * (uint64_t)dM : 0);
    r.chunk_rows = condition_chunk_rows(sw, data, per_row);
    return r;
}

ConditionQuantileRoute condition_quantile_route(const mlhip_data* data, int K, int dM, bool quantile, uint32_t n_prob, bool with_means,
                                                bool with_iterations)
{
    const Switches sw = read_switches();
    ConditionQuantileRoute r;
    r.em = em_route(data, K, Covariance::Full);
    r.kernel = sw.condition_plain ? kConditionPlain : em_condition_quantile_route(data->d, dM, quantile);
    r.skip = sw.condition_skip;
    // per row: the K log-responsibilities and the mean; the CDF's values and its output, or the blocks of a group of probabilities
    // (with the trip counts: a uint32 each, counted as a double)
    const uint64_t fixed = (uint64_t)K + (with_means ? (uint64_t)dM : 0) + (quantile ? 0 : (uint64_t)dM);
    const uint64_t block = (uint64_t)dM * (quantile && with_iterations ? 2 : 1);
    const uint64_t sized_for = quantile ? std::max<uint64_t>(1, std::min<uint64_t>(n_prob, kConditionQuantileGroup)) : 1;
    r.chunk_rows = condition_chunk_rows(sw, data, fixed + sized_for * block);
    const uint64_t per_row = kScoreScratchBytes / sizeof(double) / r.chunk_rows;
    const uint64_t fit = per_row > fixed ? (per_row - fixed) / block : 0;
    r.group = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(fit, std::max<uint32_t>(n_prob, 1)));
    if (sw.condition_group > 0 && (uint64_t)sw.condition_group < r.group) r.group = (uint32_t)sw.condition_group;   // (no bit depends on it)
    return r;
}

ConditionSampleRoute condition_sample_route(const mlhip_data* data, int K, int dM, uint32_t n_draws)
{
    const Switches sw = read_switches();
    ConditionSampleRoute r;
    r.em = em_route(data, K, Covariance::Full);
    r.kernel = sw.condition_plain ? kConditionPlain : em_condition_route(data->d, dM);
    const uint64_t sized_for = std::max<uint64_t>(1, std::min<uint64_t>(n_draws, kConditionSampleDraws));
    r.chunk_rows = condition_chunk_rows(sw, data, (uint64_t)K + sized_for * (uint64_t)dM);
    const uint64_t per_row = kScoreScratchBytes / sizeof(double) / r.chunk_rows;
    const uint64_t fit = per_row > (uint64_t)K ? (per_row - (uint64_t)K) / (uint64_t)dM : 0;
    r.draws = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(fit, n_draws));
    return r;
}

ImputeRoute impute_route(int d, int K)
{
    const Switches sw = read_switches();
    ImputeRoute r;
    // the kernel route exists where a row can have both kinds of coordinates and the register tier's paddings hold them
    const bool kernel_exists = d >= 2 && d <= kImputeMaxDim;
    r.kind = kernel_exists && sw.impute != kImputeComposed ? kImputeKernel : kImputeComposed;
    // rows per chunk: a pattern's rows per conditioning pass (composed), the rows whose d coordinates stay within kImputeRowBytes (kernel)
    const uint32_t bound = r.kind == kImputeKernel ? (uint32_t)std::max<uint64_t>(64, kImputeRowBytes / (sizeof(double) * (uint64_t)d) / 64 * 64) : kImputeRows;
    r.rows = sw.impute_rows > 0 ? (uint32_t)std::min<long>(sw.impute_rows, (long)bound) : bound;
    r.patterns = sw.impute_patterns > 0 ? (uint32_t)std::min<long>(sw.impute_patterns, 1l << 30) : 0;
    r.grid_cap = sw.impute_grid > 0 ? (int)std::min<long>(sw.impute_grid, 1l << 20) : 0;
    r.skip = sw.condition_skip;
    return r;
}

SilhouetteRoute silhouette_route(const mlhip_data* data)
{
    const Switches sw = read_switches();
    SilhouetteRoute r;
    r.kernel = sw.silhouette_plain ? (int)kSilhouettePlain : silhouette_tier(data->d);
    // The column feed of the register tier: scalar loads unless MLHIP_SILHOUETTE_FEED=lds (profiles/silhouette_timing.txt).
    r.feed = r.kernel == kSilhouetteRegisters && sw.silhouette_feed == kSilhouetteLdsFeed ? kSilhouetteLdsFeed : kSilhouetteScalarFeed;
    r.rows_override = sw.silhouette_rows > 0 ? (uint32_t)std::min<long>(sw.silhouette_rows, 1l << 30) : 0;
    r.grid = sw.silhouette_grid > 0 ? (int)std::min<long>(sw.silhouette_grid, 1l << 20) : 0;
    return r;
}

uint32_t SilhouetteRoute::block_rows(uint64_t n_chunks, uint64_t m) const
{
    const uint64_t tile = kSilhouetteRowTile, budget = kScoreScratchBytes / sizeof(double);
    uint64_t rows = rows_override ? (uint64_t)rows_override : budget / std::max<uint64_t>(n_chunks, 1);
    rows = rows_override ? (rows + tile - 1) / tile * tile : rows / tile * tile;
    if (rows < tile) rows = tile;
    const uint64_t all = (std::max<uint64_t>(m, 1) + tile - 1) / tile * tile;
    return (uint32_t)std::min(rows, all);
}

ModeRoute mode_route(const mlhip_data* data, int K, Covariance mode)
{
    ModeRoute r;
    r.mode = mode;
    r.em = em_route(data, K, mode);
    if (mode != Covariance::Tied) return r;
    const Switches sw = read_switches();
    // the kernel has no weighted form (like the diagonal one); every other shape, and MLHIP_TIED=composed, takes the composed route
    if (sw.tied == kTiedComposed || data->weighted || !mstats::em_tied_supported(data->d, K)) return r;
    // Measured (profiles/tied_timing.txt): where the full-covariance step is the fused kernel in its vector-unit form -- few components
    // in few dimensions, no padding to 16-component row blocks -- the composed step is the faster one (N = 10M, d = 4, K = 3: 0.135
    // against 0.261 ms; the ONE shape of that form that was timed, the rule extends it to the others): those shapes stay composed
    // unless MLHIP_TIED=kernel asks for the kernel.
    const bool composed_faster = r.em.fused && r.em.fused_form == kFusedValu;
    if (sw.tied == kTiedKernel || !composed_faster) r.tied_kernel = kTiedKernel;
    return r;
}

size_t restarts_doubles_per_restart(int d, int K, int grid)
{
    const size_t records = (size_t)K * estep_param_stride(d), pack = (size_t)K * (1 + d + (size_t)d * d);
    const size_t block = (size_t)mstats::em_fused_partial_rows(K) * mstats::em_fused_partial_cols(d);
    return 2 * records + pack + (size_t)grid * (block + 1) + (size_t)K * stats_count(d) + 1;
}

RestartsRoute restarts_route(const mlhip_data* data, int K, Covariance mode, uint32_t R)
{
    const Switches sw = read_switches();
    const mlhip_ctx* ctx = data->ctx;
    RestartsRoute r;
    r.em = em_route(data, K, mode);
    // Where the batch exists: the solo iteration is the vector-unit pass + reduction + device closing of ONE rank, and its grid is at
    // most one workgroup per CU (the partial-block scratch and the ll partials never cut such a grid: em_fused_small.hip).
    if (mode != Covariance::Full || data->weighted || ctx->reduce_fn || ctx->world_size > 1) return r;
    if (!r.em.fused || r.em.fused_form != kFusedValu || !r.em.device_close) return r;
    FusedArgs fa{};
    fa.n = data->n; fa.d = data->d; fa.K = K; fa.form = r.em.fused_form;
    fa.n_ll_partials = kMaxLlPartials;
    fa.partials_capacity = std::max(data->partials.bytes / sizeof(double), em_mstats_scratch_doubles(data->d, K, ctx->num_cus));
    const int grid = mstats::em_fused_valu_small_grid(fa, ctx->num_cus);
    if (grid <= 0) return r;
    const size_t fit = kRestartsScratchBytes / (sizeof(double) * restarts_doubles_per_restart(data->d, K, grid));
    if (fit < 1) return r;
    // Automatic: from kRestartsBatchFrom restarts on (the smallest R at which the batch was faster at every measured shape)
    if (sw.restarts == kRestartsSequential || (sw.restarts < 0 && R < kRestartsBatchFrom)) return r;
    r.kind = kRestartsBatched;
    r.grid = grid;
    r.per_launch = (int)std::min<size_t>(fit, (size_t)mstats::kRestartsMaxBatch);
    return r;
}

KmRoute km_route(const mlhip_data* data, int K)
{
    const Switches sw = read_switches();
    const mlhip_ctx* ctx = data->ctx;
    KmRoute r;
    // The matrix-core kernel needs a multiple of 4 dimensions. For d = 1, 2, 3, 5, 6 (stored with D = d or 6 rows) and many
    // clusters it still beats the direct-form kernel (d = 6, K = 256: 1.9 -> 1.2 ms at N = 10M), so such blocks get a copy
    // padded with zero rows once: zero coordinates add exactly 0 to every distance, labels and sums are unchanged.
    r.pad = data->D % 4 != 0 && K >= 128 && sw.kmeans < 0;
    const int D = r.pad ? (data->D + 3) & ~3 : data->D;
    const bool direct = sw.kmeans == kKmDirect || (sw.kmeans < 0 && kmeans_few_clusters(D, K, data->n));
    if ((!direct || D > kMidDim) && kmeans_mfma_supported(D, K)) r.kernel = kKmMatrix;   // (above d = 64 only the matrix-core kernel exists)
    else if (D > kMaxDim) r.kernel = sw.big_dim && big_dim_kmeans_applies(D) ? kKmBigDim : kKmPlain;
    else r.kernel = kKmDirect;
    // small blocks with few clusters, single rank: the whole step loop in one launch of one workgroup
    r.resident = sw.resident && !r.pad && !ctx->reduce_fn && ctx->world_size <= 1 && kmeans_resident_supported(D, data->d, K, data->n);
    return r;
}

}  // namespace mlhip_rt
