// EM family of the C ABI: E-step / statistics / closing orchestration of the gfx950 kernels per step (closing on the host), full,
// diagonal and tied covariances; the whole loop of EM::fit (mlhip_em_iterate: closing on the device) lives in em_loop.cpp.
#include "internal.hpp"

namespace mlhip_rt {


void ensure_em_workspace(mlhip_data* dt, int K)
{
    mlhip_ctx* ctx = dt->ctx;
    if (dt->em_K == K) return;
    dt->estep.invalidate();
    dt->ldr = dt->n_pad;
    dt->lw.reserve(sizeof(double) * dt->ldr * K);
    dt->lse.reserve(sizeof(double) * dt->n_pad);
    dt->ll_partials.reserve(sizeof(double) * kMaxLlPartials);
    size_t ps = (size_t)estep_param_stride(dt->D) * K * sizeof(double);
    if (estep_mfma4_supported(dt->D)) ps = std::max(ps, (size_t)estep_mfma4_param_stride(dt->D) * K * sizeof(double));
    dt->params_dev.reserve(ps);
    dt->params_host.reserve(ps);
    dt->partials.reserve(sizeof(double) * em_mstats_scratch_doubles(dt->d, K, ctx->num_cus));
    const size_t sb = sizeof(double) * ((size_t)K * stats_count(dt->d) + 1);
    dt->stats_dev.reserve(sb);
    dt->stats_host.reserve(sb);
    dt->em_K = K;
}


/// The K component records for the route's E-step kernel, from host parameters into `target`: the host factorization through `staging`,
/// or (d > 64) the device factorization with `work` as its scratch. `allow_fold`: matrix-core records may take the FOLD form.
RecordForm build_records(mlhip_data* dt, const EmRoute& r, int K, const double* mixing, const double* means, const double* covs,
                         bool allow_fold, DevBuf& target, PinnedBuf& staging, DevBuf& work)
{
    mlhip_ctx* ctx = dt->ctx;
    {   // (params_dev / params_next are swapped by mlhip_em_iterate and may have been sized for diagonal records)
        size_t ps = (size_t)estep_param_stride(dt->D) * K * sizeof(double);
        if (estep_mfma4_supported(dt->D)) ps = std::max(ps, (size_t)estep_mfma4_param_stride(dt->D) * K * sizeof(double));
        target.reserve(ps);
        staging.reserve(ps);
    }
    // d in 12..128: 4x4-block triangular matrix-core kernel (mfma4); below, and where the route asks for it, the scalar-fed one.
    const bool use_mfma4 = r.estep == Estep::kMatrix4;
    RecordForm form{use_mfma4 ? 2 : 0, false};
    // d > 64: the K factorizations on the device (em_close_big.hip launch_em_records_big -- the closing arithmetic's kernels, started
    // from the given covariances; the host's operations in the host's order, so the records are the host builders' except through
    // log()). On the host they were 60 ms at d = 1024, K = 4 -- once per fit, but a short fit is a few iterations.
    if (r.records_on_device) {
        const int d = dt->d;
        const size_t n_par = (size_t)K * ((size_t)d * d + d + 1);
        work.reserve(sizeof(double) * em_close_work_doubles(d, K));
        double* area = em_close_big_param_area(work.as<double>(), d, K);
        // (straight from the caller's arrays: the covariances alone are K d^2 doubles -- 0.5 GB at K = 64, d = 1024 --, no pinned copy of that)
        HIP_CHECK(hipMemcpyAsync(area, mixing, sizeof(double) * K, hipMemcpyHostToDevice, ctx->stream));
        HIP_CHECK(hipMemcpyAsync(area + K, means, sizeof(double) * K * d, hipMemcpyHostToDevice, ctx->stream));
        HIP_CHECK(hipMemcpyAsync(area + K + (size_t)K * d, covs, sizeof(double) * K * d * d, hipMemcpyHostToDevice, ctx->stream));
        CloseArgs ca{};
        ca.K = K; ca.d = d; ca.D = dt->D; ca.shift = dt->shift_dev.as<double>();
        ca.layout = form.layout;
        ca.mixing = area; ca.means = area + K; ca.covs = area + K + (size_t)K * d;
        ca.records = target.as<double>();
        ca.info = area + n_par;
        ca.work = work.as<double>();
        launch_em_records_big(ca, ctx->stream);
        HIP_CHECK(hipGetLastError());
        ctx->sync();                                     // (the caller's arrays may change once this returns)
    } else if (use_mfma4) {
        // FOLD form (no per-component mean subtraction in the kernel) while every |W_k (mu_k - shift)| is small enough for
        // the parity tolerances; the exact form otherwise. Every rank decides from the same parameters.
        form.fold = host::build_estep_params_mfma4(dt->d, dt->D, K, mixing, means, covs, allow_fold ? dt->shift.data() : nullptr,
                                                   kEstepFoldLimit, staging.as<double>());
        HIP_CHECK(hipMemcpyAsync(target.p, staging.p, sizeof(double) * estep_mfma4_param_stride(dt->D) * K,
                                 hipMemcpyHostToDevice, ctx->stream));
    } else {
        host::build_estep_params(dt->d, dt->D, K, mixing, means, covs, staging.as<double>());
        HIP_CHECK(hipMemcpyAsync(target.p, staging.p, sizeof(double) * estep_param_stride(dt->D) * K,
                                 hipMemcpyHostToDevice, ctx->stream));
    }
    return form;
}


/// Builds the per-component records for the route's E-step kernel and uploads them to params_dev (or `target`).
RecordForm prepare_estep(mlhip_data* dt, const EmRoute& r, int K, const double* mixing, const double* means, const double* covs, DevBuf* target)
{
    ensure_em_workspace(dt, K);
    const bool own = !target;
    if (own) target = &dt->params_dev;
    const RecordForm form = build_records(dt, r, K, mixing, means, covs, r.fold_allowed, *target, dt->params_host, dt->close_work);
    if (own) dt->estep.records_are(form.layout, form.fold);
    return form;
}


/// E-step kernel on the records in params_dev: fills lw and -- unless the statistics kernel is going to normalise the
/// log-responsibilities itself (`with_lse` false, matrix-core kernel only) -- lse and the log-likelihood partials.
/// This is the one place where a pass of a fit (`may_screen`) is routed to the dense or the screened kernel.
void launch_estep(mlhip_data* dt, const EmRoute& r, int K, bool with_lse, const DevBuf* records, int fold, bool may_screen)
{
    mlhip_ctx* ctx = dt->ctx;
    EstepArgs a{};
    a.xt = dt->xt.as<double>(); a.ldx = dt->ldx; a.n = dt->n; a.D = dt->D;
    a.params = (records ? records : &dt->params_dev)->as<double>(); a.K = K;
    a.lw = dt->lw.as<double>(); a.ldr = dt->ldr; a.lse = dt->lse.as<double>();
    a.ll_partials = dt->ll_partials.as<double>(); a.n_ll_partials = kMaxLlPartials;
    a.shift = dt->shift_dev.as<double>(); a.fold = (fold < 0 ? dt->estep.rec_fold : fold != 0) ? 1 : 0;
    a.with_lse = (with_lse || dt->estep.rec_layout != 2) ? 1 : 0;
    a.row_major = r.estep_rows ? 1 : 0;
    a.num_cus = ctx->num_cus;
    a.scratch = dt->partials.as<double>(); a.scratch_doubles = dt->partials.bytes / sizeof(double);   // (written by the statistics kernel AFTER the E-step, on the same stream)
    a.plain = r.estep == Estep::kPlain;
    // the screened kernel's domain: the FOLD, lw-only matrix-core pass of an unweighted block where the sparse statistics kernel exists
    const bool domain = may_screen && dt->estep.rec_layout == 2 && a.fold && !a.with_lse && !dt->weighted && r.estep == Estep::kMatrix4 &&
                        em_estep_screen_supported(dt->D, K) && em_mstats_sparse_supported(dt->d, K, ctx->num_cus);
    // ... and whether this pass may screen or leave a block a later pass may screen from: only then ScreenState keeps its history
    const bool tracked = domain && (r.screen == 1 || (r.screen < 0 && em_estep_screen_preferred(dt->D, K)));
    if (tracked) dt->screen.track(dt, K);
    int grid = 0;
    bool screened = false;
    ctx->timed("em_estep", [&] {
        if (tracked) {
            grid = dt->screen.run(dt, a, r.screen);
            screened = grid > 0;
        }
        if (!screened)
            grid = dt->estep.rec_layout == 2 ? launch_em_estep_mfma4(a, ctx->num_cus, ctx->stream) : launch_em_estep(a, ctx->stream);
    });
    if (grid < 0) throw Unsupported("E-step kernel not instantiated for this dimension");
    HIP_CHECK(hipGetLastError());
    dt->estep.block_written(grid);
    if (domain) dt->screen.pass_done(dt, a, tracked, screened);
    if (dt->weighted && a.with_lse) {
        // the log-likelihood of a weighted block is sum_i w_i lse_i: its partials replace the E-step's, lse itself stays per row
        // (without lse the weighted self-normalising statistics pass finishes both: launch_em_reduce)
        int wgrid = 0;
        ctx->timed("em_weights", [&] { wgrid = launch_weighted_ll(dt->weights.as<double>(), a.lse, dt->n, a.ll_partials, ctx->stream); });
        HIP_CHECK(hipGetLastError());
        dt->estep.ll_weighted(wgrid);
    }
}


void run_estep(mlhip_data* dt, const EmRoute& r, int K, const double* mixing, const double* means, const double* covs, bool with_lse,
               bool may_screen)
{
    prepare_estep(dt, r, K, mixing, means, covs);
    launch_estep(dt, r, K, with_lse, nullptr, -1, may_screen);
}


/// The covariance array of `mode` as K full covariance matrices (host::covariances_as_full).
std::vector<double> as_full(Covariance mode, int K, int d, const double* covariance)
{
    std::vector<double> covs(covariance_doubles(Covariance::Full, K, d));
    host::covariances_as_full(mode, K, d, covariance, covs.data());
    return covs;
}


/// After a fused step only lse exists on the device; whoever needs the log-responsibility block (labels,
/// responsibilities, a separate M-step, the refinement pass) gets it rebuilt from the same parameter records.
void ensure_lw(mlhip_data* dt, const EmRoute& r, int K)
{
    if (!dt->estep.needs_rebuild()) return;
    if (dt->estep.mode_records()) {
        // params_dev holds diagonal / tied records: the same parameters as full covariances for the E-step kernel
        const EstepState::Kept& p = dt->estep.kept;
        const std::vector<double> covs = as_full(p.mode, K, dt->d, p.covariance.data());
        prepare_estep(dt, r, K, p.mixing.data(), p.means.data(), covs.data());
    }
    launch_estep(dt, r, K);
}


/// All-reduces the reduced statistics buffer [K*F stats, ll_sum] and leaves it in stats_host.
void collect_stats(mlhip_data* dt, int K, size_t count)
{
    mlhip_ctx* ctx = dt->ctx;
    if (!count) count = (size_t)K * stats_count(dt->d) + 1;
    ctx->reduce_to_host(dt->stats_host.as<double>(), dt->stats_dev.as<double>(), count);
}


/// What every one-kernel pass takes: the handle's block and buffers, the records in `records` (null: params_dev), the statistics
/// shift at `shift_dev`.
static void one_pass_args(OnePassArgs& a, const mlhip_data* dt, int K, const double* shift_dev, const DevBuf* records)
{
    a.xt = dt->xt.as<double>(); a.ldx = dt->ldx; a.n = dt->n; a.d = dt->d;
    a.shift = shift_dev; a.params = (records ? records : &dt->params_dev)->as<double>(); a.K = K;
    a.lse = dt->lse.as<double>();
    a.partials = dt->partials.as<double>(); a.partials_capacity = dt->partials.bytes / sizeof(double);
    a.ll_partials = dt->ll_partials.as<double>(); a.n_ll_partials = kMaxLlPartials;
}


/// One one-kernel pass: `launch` (returns its grid) under the timer `timer`, then the fixed-order reduction of its partial blocks
/// [rows][cols] and log-likelihood partials into stats_dev = [K * F statistics, ll_sum]. Returns the grid.
template <class Launch>
static int run_one_pass(mlhip_data* dt, const OnePassArgs& a, const char* timer, const char* what, int rows, int cols, int F, Launch&& launch)
{
    mlhip_ctx* ctx = dt->ctx;
    int grid = 0;
    ctx->timed(timer, [&] { grid = launch(); });
    if (grid <= 0) throw std::runtime_error(std::string(what) + " EM kernel launch failed");
    launch_em_reduce_blocks(a.partials, grid, rows, cols, a.K, F, a.ll_partials, grid, dt->stats_dev.as<double>(), ctx->stream);
    HIP_CHECK(hipGetLastError());
    return grid;
}


FusedArgs fused_args(const mlhip_data* dt, const EmRoute& r, int K, const DevBuf* records)
{
    FusedArgs a{};
    one_pass_args(a, dt, K, dt->shift_dev.as<double>(), records);
    a.form = r.fused_form;
    return a;
}


/// What a fused pass (em_fused_small.hip, or the resident loop that runs the same pass) leaves behind: lse and `grid` log-likelihood
/// partials, no N x K block; a refinement pass reads the block ensure_lw rebuilds.
void fused_pass_done(mlhip_data* dt, int grid)
{
    dt->estep.records_only(grid);
    dt->estep.stats_from(kFromLogResp, dt->lw.as<double>(), dt->ldr);
}


/// The fused kernel + reduction on the records already in params_dev; statistics end in stats_dev (and, with `collect`, all-
/// reduced in stats_host).
void launch_fused_step(mlhip_data* dt, const EmRoute& r, int K, bool collect, const DevBuf* records)
{
    mlhip_ctx* ctx = dt->ctx;
    const FusedArgs a = fused_args(dt, r, K, records);
    const int grid = run_one_pass(dt, a, "em_fused", "fused", mstats::em_fused_partial_rows(K), mstats::em_fused_partial_cols(dt->d),
                                  stats_count(dt->d), [&] { return mstats::launch_em_fused_small(a, ctx->num_cus, ctx->stream); });
    fused_pass_done(dt, grid);
    if (collect) collect_stats(dt, K);
}


bool run_fused_step(mlhip_data* dt, const EmRoute& r, int K, const double* mixing, const double* means, const double* covs)
{
    if (!r.fused) return false;
    prepare_estep(dt, r, K, mixing, means, covs);
    launch_fused_step(dt, r, K, true);
    return true;
}


/// The statistics kernels' arguments for `K` columns of `resp` (log-responsibilities or responsibilities, by `mode`) about `shift`.
static MstatsArgs mstats_args(const mlhip_data* dt, const EmRoute& r, int K, int mode, const double* shift, const double* resp, size_t ld,
                              double* stats)
{
    MstatsArgs a{};
    a.xt = dt->xt.as<double>(); a.ldx = dt->ldx; a.n = dt->n; a.d = dt->d;
    a.shift = shift;
    a.lw = resp; a.ldr = ld; a.lse = dt->lse.as<double>();
    a.K = K; a.mode = mode;
    a.partials = dt->partials.as<double>(); a.partials_capacity = dt->partials.bytes / sizeof(double);
    a.stats = stats;
    a.plain = r.stats_plain(dt->d);
    return a;
}


/// Runs the statistics kernel on log-responsibilities (mode kFromLogResp: the E-step's lw/lse) or on plain
/// responsibilities `resp_dev` ([K][ld_resp], ld_resp >= n_pad), all-reduces, leaves [K*F stats, ll_sum] in stats_host.
void run_mstats(mlhip_data* dt, const EmRoute& r, int K, int mode, const double* resp_dev, size_t ld_resp, bool with_ll, bool collect,
                bool use_weights)
{
    mlhip_ctx* ctx = dt->ctx;
    ensure_em_workspace(dt, K);
    const bool weighted = use_weights && dt->weighted;
    const bool self_norm = mode == kFromLogRespSelfNorm;
    if (weighted && !self_norm) {
        // w_i r_ik as plain responsibilities (one rounding more than r_ik), then the statistics kernel of the shape in mode kFromResp
        // (the self-normalising wide kernel applies the weight itself while it stages: no second block)
        dt->wresp.reserve(sizeof(double) * dt->ldr * K);
        const double* src = mode == kFromResp ? resp_dev : dt->lw.as<double>();
        const size_t lds = mode == kFromResp ? ld_resp : dt->ldr;
        ctx->timed("em_weights", [&] {
            launch_weighted_resp(src, lds, dt->lse.as<double>(), mode, dt->weights.as<double>(), dt->n, dt->n_pad, K, dt->wresp.as<double>(),
                                 dt->ldr, ctx->stream);
        });
        HIP_CHECK(hipGetLastError());
        mode = kFromResp; resp_dev = dt->wresp.as<double>(); ld_resp = dt->ldr;
    }
    MstatsArgs a = mstats_args(dt, r, K, mode, dt->shift_dev.as<double>(), mode == kFromResp ? resp_dev : dt->lw.as<double>(),
                               mode == kFromResp ? ld_resp : dt->ldr, dt->stats_dev.as<double>());
    a.ll_partials = with_ll ? dt->ll_partials.as<double>() : nullptr;
    a.n_ll_partials = with_ll ? dt->estep.n_ll : 0;
    a.lse_out = dt->lse.as<double>(); a.ll_scratch = dt->ll_partials.as<double>();
    if (self_norm) {
        dt->esum.reserve(sizeof(double) * dt->n_pad);
        a.ll_out = dt->esum.as<double>();
        if (weighted) { a.mode = kFromLogRespSelfNormWeighted; a.weights = dt->weights.as<double>(); }
    }
    // after a self-normalising pass lse is in HBM like after an LSE-writing E-step: a refinement pass reads it
    dt->estep.stats_from(self_norm ? (int)kFromLogResp : mode, a.lw, a.ldr);
    int rc = 0;
    if (self_norm) {
        // the sparse kernel (em_mstats_sparse.hip) or the dense one, by the counts of the handle's earlier passes (sparse_stats_wanted)
        a.nz_count = dt->stats_history.begin(K, ctx->stream);
        const bool sparse = dt->stats_history.sparse_wanted(dt->n, r.sparse, em_mstats_sparse_supported(dt->d, K, ctx->num_cus));
        ctx->timed("em_mstats", [&] {
            rc = sparse ? launch_em_mstats_sparse(a, ctx->num_cus, ctx->stream) : launch_em_mstats(a, ctx->num_cus, ctx->stream);
        });
        dt->stats_history.end(ctx->stream);
    } else {
        ctx->timed("em_mstats", [&] { rc = launch_em_mstats(a, ctx->num_cus, ctx->stream); });
    }
    if (rc <= 0) throw std::runtime_error("statistics kernel launch failed (plan/scratch)");
    launch_em_reduce(a, ctx->num_cus, rc, ctx->stream);
    HIP_CHECK(hipGetLastError());
    if (collect) collect_stats(dt, K);
}


double log_two_pi()
{
    static const double v = std::log(2. * 3.14159265358979323846);   // ML/EM.cpp:197
    return v;
}


double ll_from_stats(const mlhip_data* dt, int K)
{
    const double log_2_pi = log_two_pi();
    const double sum = dt->stats_host.as<double>()[(size_t)K * stats_count(dt->d)];
    return sum / dt->total_weight() - (double)dt->d * log_2_pi / 2;
}


void check_call(mlhip_ctx* ctx, mlhip_data* dt, uint32_t K)
{
    require(ctx && dt, "null context or data");
    require(dt->ctx == ctx, "data belongs to another context");
    if (ctx->group) require((int)dt->parts.size() == grp::shard_count(ctx), "data was not uploaded through this device group");
    require(K >= 1, "At least one component required");
    if (!ctx->group) ctx->use();
}


/// Ratio (mean offset from the shared shift)^2 / variance above which a component's covariance is recomputed about its
/// own mean. The one-GEMM statistics share one shift (the global mean), so Sigma_k = M2'/S0 - m m^T cancels
/// ~log10(ratio) digits: measured relative error ~3e-15 * ratio. 1e4 keeps every covariance within ~3e-11 of the
/// two-pass form the reference uses (ML/EM.cpp:245-250). MLHIP_REFINE_RATIO overrides; <= 0 disables the refinement.
double refine_ratio()
{
    static const double r = [] {
        const char* e = std::getenv("MLHIP_REFINE_RATIO");
        return (e && *e) ? std::atof(e) : 1e4;
    }();
    return r;
}


/// Second statistics pass for ONE component with the shift at that component's new mean (K = 1 launch of the same
/// kernels on column k of the responsibilities of the last pass), all-reduced like the first; replaces covariance k
/// (and adds the tiny mean correction). Tight clusters far from the global mean need it; the headline shapes never do.
void refine_component(mlhip_data* dt, const EmRoute& r, int k, double* mean_k, double* cov_k)
{
    mlhip_ctx* ctx = dt->ctx;
    const int d = dt->d, F = stats_count(d);
    const EstepState& st = dt->estep;
    if (st.stats_mode == kFromLogResp) ensure_lw(dt, r, dt->em_K);   // after a fused step the block is not in HBM yet
    dt->refine_shift.reserve(sizeof(double) * d);
    dt->refine_stats.reserve(sizeof(double) * (F + 1));
    HIP_CHECK(hipMemcpyAsync(dt->refine_shift.p, mean_k, sizeof(double) * d, hipMemcpyHostToDevice, ctx->stream));
    int mode = st.stats_mode;
    const double* column = st.stats_resp + (size_t)k * st.stats_ld;
    if (dt->weighted && mode == kFromLogResp) {
        // the last pass of a weighted block normalised lw itself (self-normalising form): column k as w_i r_ik, like every other tier
        dt->wresp.reserve(sizeof(double) * dt->ldr);
        launch_weighted_resp(column, st.stats_ld, dt->lse.as<double>(), mode, dt->weights.as<double>(), dt->n, dt->n_pad, 1,
                             dt->wresp.as<double>(), dt->ldr, ctx->stream);
        HIP_CHECK(hipGetLastError());
        mode = kFromResp;
        column = dt->wresp.as<double>();
    }
    const MstatsArgs a = mstats_args(dt, r, 1, mode, dt->refine_shift.as<double>(), column, st.stats_ld, dt->refine_stats.as<double>());
    int rc = 0;
    ctx->timed("em_refine", [&] { rc = launch_em_mstats(a, ctx->num_cus, ctx->stream); });
    if (rc <= 0) throw std::runtime_error("statistics kernel launch failed (refinement pass)");
    launch_em_reduce(a, ctx->num_cus, rc, ctx->stream);
    HIP_CHECK(hipGetLastError());
    std::vector<double> s((size_t)F);
    ctx->reduce_to_host(s.data(), dt->refine_stats.as<double>(), (size_t)F);
    const double s0 = s[stats_index(d, d)];
    std::vector<double> m(d);
    for (int a2 = 0; a2 < d; ++a2) m[a2] = s[stats_index(d, a2)] / s0;          // ~0: the shift is the mean already
    for (int a2 = 0; a2 < d; ++a2)
        for (int b = 0; b <= a2; ++b) {
            const double v = (s[stats_index(a2, b)] - s[stats_index(d, a2)] * m[b]) / s0;
            cov_k[b * d + a2] = v;
            cov_k[a2 * d + b] = v;
        }
    for (int a2 = 0; a2 < d; ++a2) {
        cov_k[a2 * d + a2] += dt->ridge;                                        // ML/EM.cpp:252
        mean_k[a2] += m[a2];
    }
}


/// The cancellation guard's test for one component: some (mean offset from the shared shift)^2 exceeds limit * variance
/// (variance[a * stride]: a full matrix's diagonal, or a row of variances). Also catches a variance <= 0 from cancellation; a
/// non-finite offset or variance leaves the component alone -- NaN stays NaN (ML/EM.cpp:236).
static bool needs_refinement(int d, const double* mean, const double* shift, const double* variance, size_t stride, double limit)
{
    for (int a = 0; a < d; ++a) {
        const double off = mean[a] - shift[a], var = variance[a * stride];
        if (!std::isfinite(off) || !std::isfinite(var)) return false;
        if (off * off > limit * var) return true;
    }
    return false;
}


void finalize_out(mlhip_data* dt, const EmRoute& r, int K, double* mixing_out, double* means_out, double* cov_out)
{
    const int d = dt->d;
    host::finalize_mstep(d, K, dt->stats_host.as<double>(), dt->shift.data(), dt->total_weight(), dt->ridge, mixing_out,
                         means_out, cov_out);
    const double limit = refine_ratio();
    if (!(limit > 0)) return;
    // Every rank sees the same all-reduced statistics, hence flags the same components in the same order.
    for (int k = 0; k < K; ++k) {
        if (!(mixing_out[k] > 0) || !std::isfinite(mixing_out[k])) continue;    // empty / broken component: as the reference
        double* mu = means_out + (size_t)k * d;
        double* cov = cov_out + (size_t)k * d * d;
        if (needs_refinement(d, mu, dt->shift.data(), cov, (size_t)d + 1, limit)) refine_component(dt, r, k, mu, cov);
    }
}


/// One diagonal-covariance EM iteration's device work (em_diag.hip) with the statistics shift at `shift_dev`; leaves the
/// all-reduced [K * (2d+1) statistics, ll_sum] in stats_host. The records must already be in params_dev.
void run_diag_kernel(mlhip_data* dt, const EmRoute& r, int K, const double* shift_dev, bool collect, const DevBuf* records)
{
    mlhip_ctx* ctx = dt->ctx;
    DiagArgs a{};
    one_pass_args(a, dt, K, shift_dev, records);
    a.two_op = shift_dev == dt->shift_dev.as<double>() ? 1 : 0;     // (the records' a, b are relative to the data's shift)
    a.exact = r.diag_exact ? 1 : 0;
    const int grid = run_one_pass(dt, a, "em_diag", "diagonal", mstats::em_diag_partial_rows(K), mstats::em_diag_partial_cols(dt->d),
                                  diag_stats_count(dt->d), [&] { return mstats::launch_em_diag(a, ctx->num_cus, ctx->stream); });
    dt->estep.mode_records_only(Covariance::Diagonal, grid);
    if (collect) collect_stats(dt, K, (size_t)K * diag_stats_count(dt->d) + 1);
}


/// One full-covariance EM iteration with the closing arithmetic on the HOST (the body of mlhip_em_step).
void em_step_full(mlhip_data* data, const EmRoute& r, int K, const double* mixing, const double* means, const double* covariances,
                  double* log_likelihood, double* mixing_out, double* means_out, double* covariances_out)
{
    PhaseTrace tr;
    if (run_fused_step(data, r, K, mixing, means, covariances)) {
        tr.mark("fused E+M launch+sync+D2H");
    } else {
        run_estep(data, r, K, mixing, means, covariances, !r.self_norm, true);
        tr.mark("params+launch E");
        run_mstats(data, r, K, r.self_norm ? kFromLogRespSelfNorm : kFromLogResp, nullptr, 0, true);
        tr.mark("M launch+sync+D2H");
    }
    *log_likelihood = ll_from_stats(data, K);
    finalize_out(data, r, K, mixing_out, means_out, covariances_out);
    tr.mark("closing arithmetic");
}


/// Records of a diagonal-covariance parameter set -> `target` (padded to whole 16-component row blocks with neutral records).
void upload_diag_records(mlhip_data* data, int K, const double* mixing, const double* means, const double* variances, DevBuf& target)
{
    mlhip_ctx* ctx = data->ctx;
    const int KP = mstats::em_diag_partial_rows(K);
    const size_t rec_bytes = sizeof(double) * diag_param_doubles(data->D, KP);
    target.reserve(rec_bytes);
    data->params_host.reserve(rec_bytes);
    host::build_diag_params(data->d, data->D, K, KP, mixing, means, variances, data->shift.data(), data->params_host.as<double>());
    HIP_CHECK(hipMemcpyAsync(target.p, data->params_host.p, rec_bytes, hipMemcpyHostToDevice, ctx->stream));
    ctx->sync();                                     // params_host may be rewritten right away by the caller's next upload
}


/// Same cancellation guard as the full-covariance path (refine_ratio): a component whose mean sits far from the shared shift,
/// measured in its own standard deviations, gets its variances from a second pass with the shift at its new mean (the E part of
/// that pass re-evaluates the SAME input parameters, still in params_dev).
void refine_diag(mlhip_data* data, const EmRoute& r, int K, const double* mixing_out, double* means_out, double* variances_out)
{
    mlhip_ctx* ctx = data->ctx;
    const int d = data->d, F = diag_stats_count(d);
    const double limit = refine_ratio();
    if (!(limit > 0)) return;
    for (int k = 0; k < K; ++k) {
        if (!(mixing_out[k] > 0) || !std::isfinite(mixing_out[k])) continue;
        if (!needs_refinement(d, means_out + (size_t)k * d, data->shift.data(), variances_out + (size_t)k * d, 1, limit)) continue;
        data->refine_shift.reserve(sizeof(double) * data->D);
        HIP_CHECK(hipMemsetAsync(data->refine_shift.p, 0, sizeof(double) * data->D, ctx->stream));
        HIP_CHECK(hipMemcpyAsync(data->refine_shift.p, means_out + (size_t)k * d, sizeof(double) * d, hipMemcpyHostToDevice, ctx->stream));
        run_diag_kernel(data, r, K, data->refine_shift.as<double>());
        const double* s = data->stats_host.as<double>() + (size_t)k * F;
        const double s0 = s[2 * d];
        for (int a = 0; a < d; ++a) {
            const double m = s[a] / s0;                                      // ~0: the shift is the mean already
            variances_out[(size_t)k * d + a] = (s[d + a] - s[a] * m) / s0 + data->ridge;
            means_out[(size_t)k * d + a] += m;
        }
    }
}


void em_step_diag(mlhip_data* data, const EmRoute& r, int K, const double* mixing, const double* means, const double* variances,
                  double* log_likelihood, double* mixing_out, double* means_out, double* variances_out)
{
    const int d = data->d;
    if (!r.diag_kernel) {
        // Shapes the one-kernel diagonal iteration is not built for (d > 32 or K > 64) and weighted blocks: the same iteration through the
        // full-covariance kernels on diagonal matrices -- the E-step's Cholesky of a diagonal matrix is its square root, and
        // the diagonal of the M-step's full covariance IS the diagonal-mode variance (ML/EM.cpp:245-257 entry by entry); the
        // off-diagonal sums are computed and dropped. Slower than it could be, never refused.
        const std::vector<double> cov = as_full(Covariance::Diagonal, K, d, variances);
        std::vector<double> cov_out(cov.size());
        em_step_full(data, r, K, mixing, means, cov.data(), log_likelihood, mixing_out, means_out, cov_out.data());
        host::covariances_from_full(Covariance::Diagonal, K, d, mixing_out, cov_out.data(), variances_out);
        return;
    }
    ensure_em_workspace(data, K);
    // keep the input parameters: labels / responsibilities are produced from them on demand (ensure_lw)
    data->estep.parameters(Covariance::Diagonal, K, d, mixing, means, variances);
    upload_diag_records(data, K, mixing, means, variances, data->params_dev);
    run_diag_kernel(data, r, K, data->shift_dev.as<double>());
    const int F = diag_stats_count(d);
    const double* st = data->stats_host.as<double>();
    *log_likelihood = st[(size_t)K * F] / (double)data->n_global - (double)d * log_two_pi() / 2;   // ML/EM.cpp:197-198, 211
    host::finalize_mstep_diag(d, K, st, data->shift.data(), (double)data->n_global, data->ridge, mixing_out, means_out, variances_out);
    refine_diag(data, r, K, mixing_out, means_out, variances_out);
}


/// One tied-covariance EM iteration's device work (em_tied.hip) on the records [K padded records | whitening block] in params_dev;
/// leaves the all-reduced [K * (d+1) statistics, ll_sum] in stats_host.
static void run_tied_kernel(mlhip_data* dt, int K)
{
    mlhip_ctx* ctx = dt->ctx;
    TiedArgs a{};
    one_pass_args(a, dt, K, dt->shift_dev.as<double>(), nullptr);
    a.winv = a.params + (size_t)mstats::em_tied_partial_rows(K) * tied_param_stride(dt->D);
    const int grid = run_one_pass(dt, a, "em_tied", "tied", mstats::em_tied_partial_rows(K), mstats::em_tied_partial_cols(dt->d),
                                  tied_stats_count(dt->d), [&] { return mstats::launch_em_tied(a, ctx->num_cus, ctx->stream); });
    dt->estep.mode_records_only(Covariance::Tied, grid);
    collect_stats(dt, K, (size_t)K * tied_stats_count(dt->d) + 1);
}


/// Records of a tied-covariance parameter set -> params_dev: K records padded to whole 16-component row blocks with neutral ones,
/// then the shared whitening block (layout.hpp).
static void upload_tied_records(mlhip_data* data, int K, const double* mixing, const double* means, const double* cov)
{
    mlhip_ctx* ctx = data->ctx;
    const int KP = mstats::em_tied_partial_rows(K);
    const size_t rec_doubles = (size_t)KP * tied_param_stride(data->D);
    const size_t bytes = sizeof(double) * (rec_doubles + tied_winv_doubles(data->D));
    data->params_dev.reserve(bytes);
    data->params_host.reserve(bytes);
    double* h = data->params_host.as<double>();
    host::build_tied_params(data->d, data->D, K, KP, mixing, means, cov, data->shift.data(), h + rec_doubles, h);
    HIP_CHECK(hipMemcpyAsync(data->params_dev.p, data->params_host.p, bytes, hipMemcpyHostToDevice, ctx->stream));
    ctx->sync();                                     // params_host may be rewritten right away by the caller's next upload
}


void em_step_tied(mlhip_data* data, const ModeRoute& r, int K, const double* mixing, const double* means, const double* cov,
                  double* log_likelihood, double* mixing_out, double* means_out, double* cov_out)
{
    const int d = data->d;
    if (r.tied_kernel != kTiedKernel) {
        // COMPOSED: one full-covariance step on K copies of the covariance, on whatever route this shape takes (weights, the
        // refinement pass, big dimensions and the plain tier included), then  Sigma = sum_k pi_k Sigma_k  in ascending k -- the tied
        // M-step, since sum_k S0_k Sigma_k = T - sum_k S1_k S1_k^T / S0_k. Every Sigma_k carries the handle's ridge r I (ML/EM.cpp:252),
        // and sum_k pi_k = 1 up to rounding: the K ridges pool to the one ridge of the tied mode. Nothing is subtracted or re-added.
        // Slower than it could be, never refused.
        const std::vector<double> covs = as_full(Covariance::Tied, K, d, cov);
        std::vector<double> covs_out(covs.size());
        em_step_full(data, r.em, K, mixing, means, covs.data(), log_likelihood, mixing_out, means_out, covs_out.data());
        host::covariances_from_full(Covariance::Tied, K, d, mixing_out, covs_out.data(), cov_out);
        return;
    }
    // T = sum_i xt_i xt_i^T does not depend on the responsibilities: once per handle, all-reduced like the statistics
    if (data->total_scatter.empty()) {
        run_total_scatter(data);
        const double* t = data->stats_host.as<double>();
        data->total_scatter.assign(t, t + stats_count(d));
    }
    ensure_em_workspace(data, K);
    // keep the input parameters: labels / responsibilities are produced from them on demand (ensure_lw)
    data->estep.parameters(Covariance::Tied, K, d, mixing, means, cov);
    upload_tied_records(data, K, mixing, means, cov);
    run_tied_kernel(data, K);
    const int F = tied_stats_count(d);
    const double* st = data->stats_host.as<double>();
    *log_likelihood = st[(size_t)K * F] / (double)data->n_global - (double)d * log_two_pi() / 2;   // ML/EM.cpp:197-198, 211
    host::finalize_mstep_tied(d, K, st, data->total_scatter.data(), data->shift.data(), (double)data->n_global, data->ridge, mixing_out,
                              means_out, cov_out);
}


void em_step(mlhip_data* data, const ModeRoute& r, int K, const double* mixing, const double* means, const double* covs,
             double* log_likelihood, double* mixing_out, double* means_out, double* covs_out)
{
    switch (r.mode) {
    case Covariance::Full: em_step_full(data, r.em, K, mixing, means, covs, log_likelihood, mixing_out, means_out, covs_out); break;
    case Covariance::Diagonal: em_step_diag(data, r.em, K, mixing, means, covs, log_likelihood, mixing_out, means_out, covs_out); break;
    case Covariance::Tied: em_step_tied(data, r, K, mixing, means, covs, log_likelihood, mixing_out, means_out, covs_out); break;
    }
}


namespace {

/// mlhip_em_step / mlhip_em_step_diag / mlhip_em_step_tied (`step`) through a device group: the outputs may alias the inputs, so the shards read copies.
void group_em_step(decltype(&mlhip_em_step) step, mlhip_ctx* ctx, mlhip_data* data, uint32_t K, Covariance mode, const double* mixing,
                   const double* means, const double* covs, double* log_likelihood, double* mixing_out, double* means_out, double* covs_out)
{
    const size_t kd = (size_t)K * data->d, cov_doubles = covariance_doubles(mode, (int)K, data->d);
    const std::vector<double> pi(mixing, mixing + K), mu(means, means + kd), cv(covs, covs + cov_doubles);
    fan_out(ctx, data, [&](Shard& sh) {
        return step(sh.ctx, sh.part, K, pi.data(), mu.data(), cv.data(), sh.scalar(log_likelihood), sh.replicated(mixing_out, K),
                    sh.replicated(means_out, kd), sh.replicated(covs_out, cov_doubles));
    });
}

}  // namespace
}  // namespace mlhip_rt

extern "C" {


int mlhip_em_expectation(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, const double* mixing, const double* means,
                         const double* covariances, double* log_likelihood)
{
    return guarded([&] {
        check_call(ctx, data, K);
        require(mixing && means && covariances && log_likelihood, "null argument");
        if (ctx->group) {
            fan_out(ctx, data, [&](Shard& sh) {
                return mlhip_em_expectation(sh.ctx, sh.part, K, mixing, means, covariances, sh.scalar(log_likelihood));
            });
            return;
        }
        run_estep(data, em_route(data, (int)K, Covariance::Full), (int)K, mixing, means, covariances);
        double* slot = data->stats_dev.as<double>() + (size_t)K * stats_count(data->d);
        launch_ll_reduce(data->ll_partials.as<double>(), data->estep.n_ll, slot, ctx->stream);
        HIP_CHECK(hipGetLastError());
        double* host_slot = data->stats_host.as<double>() + (size_t)K * stats_count(data->d);
        HIP_CHECK(hipMemcpyAsync(host_slot, slot, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
        ctx->allreduce_host(host_slot, 1);
        *log_likelihood = ll_from_stats(data, (int)K);
    });
}

int mlhip_em_maximisation(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, double* mixing_out, double* means_out,
                          double* covariances_out)
{
    return guarded([&] {
        check_call(ctx, data, K);
        require(mixing_out && means_out && covariances_out, "null argument");
        if (ctx->group) {
            const size_t kd = (size_t)K * data->d;
            fan_out(ctx, data, [&](Shard& sh) {
                return mlhip_em_maximisation(sh.ctx, sh.part, K, sh.replicated(mixing_out, K), sh.replicated(means_out, kd),
                                            sh.replicated(covariances_out, kd * data->d));
            });
            return;
        }
        require(data->has_estep_results((int)K), "no E-step results on the device for this K");
        const EmRoute r = em_route(data, (int)K, Covariance::Full);
        ensure_lw(data, r, (int)K);
        run_mstats(data, r, (int)K, kFromLogResp, nullptr, 0, true);
        finalize_out(data, r, (int)K, mixing_out, means_out, covariances_out);
    });
}

int mlhip_em_step(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, const double* mixing, const double* means,
                  const double* covariances, double* log_likelihood, double* mixing_out, double* means_out,
                  double* covariances_out)
{
    return guarded([&] {
        check_call(ctx, data, K);
        require(mixing && means && covariances && log_likelihood && mixing_out && means_out && covariances_out, "null argument");
        if (ctx->group) {
            group_em_step(mlhip_em_step, ctx, data, K, Covariance::Full, mixing, means, covariances, log_likelihood, mixing_out,
                          means_out, covariances_out);
            return;
        }
        em_step(data, mode_route(data, (int)K, Covariance::Full), (int)K, mixing, means, covariances, log_likelihood, mixing_out, means_out, covariances_out);
    });
}

int mlhip_em_step_diag(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, const double* mixing, const double* means,
                       const double* variances, double* log_likelihood, double* mixing_out, double* means_out,
                       double* variances_out)
{
    return guarded([&] {
        check_call(ctx, data, K);
        require(mixing && means && variances && log_likelihood && mixing_out && means_out && variances_out, "null argument");
        if (ctx->group) {
            group_em_step(mlhip_em_step_diag, ctx, data, K, Covariance::Diagonal, mixing, means, variances, log_likelihood, mixing_out, means_out,
                          variances_out);
            return;
        }
        em_step(data, mode_route(data, (int)K, Covariance::Diagonal), (int)K, mixing, means, variances, log_likelihood, mixing_out, means_out, variances_out);
    });
}

int mlhip_em_step_tied(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, const double* mixing, const double* means,
                       const double* covariance, double* log_likelihood, double* mixing_out, double* means_out,
                       double* covariance_out)
{
    return guarded([&] {
        check_call(ctx, data, K);
        require(mixing && means && covariance && log_likelihood && mixing_out && means_out && covariance_out, "null argument");
        if (ctx->group) {
            group_em_step(mlhip_em_step_tied, ctx, data, K, Covariance::Tied, mixing, means, covariance, log_likelihood, mixing_out,
                          means_out, covariance_out);
            return;
        }
        em_step(data, mode_route(data, (int)K, Covariance::Tied), (int)K, mixing, means, covariance, log_likelihood, mixing_out, means_out, covariance_out);
    });
}

int mlhip_em_iterate(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, int covariance_type, double* mixing, double* means,
                     double* covariances, uint32_t max_steps, double absolute_tolerance, double relative_tolerance,
                     uint32_t* steps_done, int* converged, double* log_likelihood, double* log_likelihood_history)
{
    return guarded([&] {
        check_call(ctx, data, K);
        require(mixing && means && covariances && steps_done && converged && log_likelihood, "null argument");
        const Covariance mode = covariance_from_abi(covariance_type);
        require(max_steps >= 1, "at least one step required");
        if (absolute_tolerance < 0 || relative_tolerance < 0) throw DomainError("negative tolerance");
        const size_t kd = (size_t)K * data->d, cov_doubles = covariance_doubles(mode, (int)K, data->d);
        if (ctx->group) {
            // the parameters are in/out: shard 0 updates the caller's, the others copies of their own (the ranks' end-of-fit
            // checksum exchange inside the shards' calls holds them to bit-identical results)
            const std::vector<double> pi(mixing, mixing + K), mu(means, means + kd), cv(covariances, covariances + cov_doubles);
            fan_out(ctx, data, [&](Shard& sh) {
                return mlhip_em_iterate(sh.ctx, sh.part, K, covariance_type, sh.replicated(mixing, K, pi.data()), sh.replicated(means, kd, mu.data()),
                                        sh.replicated(covariances, cov_doubles, cv.data()), max_steps, absolute_tolerance, relative_tolerance,
                                        sh.scalar(steps_done, "iterations"), sh.scalar(converged, "iterations"), sh.scalar(log_likelihood),
                                        sh.replicated(log_likelihood_history, max_steps));
            });
            return;
        }
        em_iterate(data, mode, (int)K, mixing, means, covariances, max_steps, absolute_tolerance, relative_tolerance, steps_done, converged,
                   log_likelihood, log_likelihood_history);
        ctx->check_ranks_agree("the EM parameters", {{mixing, K}, {means, kd}, {covariances, cov_doubles}, {log_likelihood, 1}});
    });
}

int mlhip_em_maximisation_from(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, const double* resp, int64_t ldr,
                               double* mixing_out, double* means_out, double* covariances_out)
{
    return guarded([&] {
        check_call(ctx, data, K);
        require((resp || data->rows() == 0) && mixing_out && means_out && covariances_out, "null argument");   // (an empty shard has no rows)
        require(ldr >= 0 && (uint64_t)ldr >= data->rows(), "ldr must be >= n_local");
        if (ctx->group) {
            const size_t kd = (size_t)K * data->d;
            fan_out(ctx, data, [&](Shard& sh) {
                return mlhip_em_maximisation_from(sh.ctx, sh.part, K, sh.rows(resp), ldr, sh.replicated(mixing_out, K), sh.replicated(means_out, kd),
                                                 sh.replicated(covariances_out, kd * data->d));
            });
            return;
        }
        ensure_em_workspace(data, (int)K);
        data->resp_dev.reserve(sizeof(double) * data->ldr * K);
        HIP_CHECK(hipMemsetAsync(data->resp_dev.p, 0, sizeof(double) * data->ldr * K, ctx->stream));
        if (data->n)
            HIP_CHECK(hipMemcpy2DAsync(data->resp_dev.p, sizeof(double) * data->ldr, resp, sizeof(double) * ldr,
                                       sizeof(double) * data->n, K, hipMemcpyHostToDevice, ctx->stream));
        const EmRoute r = em_route(data, (int)K, Covariance::Full);
        run_mstats(data, r, (int)K, kFromResp, data->resp_dev.as<double>(), data->ldr, false);
        finalize_out(data, r, (int)K, mixing_out, means_out, covariances_out);
    });
}

int mlhip_em_maximisation_from_labels(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, const uint32_t* labels,
                                      double* mixing_out, double* means_out, double* covariances_out)
{
    return guarded([&] {
        check_call(ctx, data, K);
        require((labels || data->rows() == 0) && mixing_out && means_out && covariances_out, "null argument");
        if (ctx->group) {
            const size_t kd = (size_t)K * data->d;
            fan_out(ctx, data, [&](Shard& sh) {
                return mlhip_em_maximisation_from_labels(sh.ctx, sh.part, K, sh.rows(labels), sh.replicated(mixing_out, K), sh.replicated(means_out, kd),
                                                        sh.replicated(covariances_out, kd * data->d));
            });
            return;
        }
        ensure_em_workspace(data, (int)K);
        data->labels_dev.reserve(sizeof(uint32_t) * data->n_pad);
        if (data->n)
            HIP_CHECK(hipMemcpyAsync(data->labels_dev.p, labels, sizeof(uint32_t) * data->n, hipMemcpyHostToDevice, ctx->stream));
        // One-hot responsibilities are materialised in the (still unused) log-responsibility buffer of the workspace.
        data->estep.invalidate();
        launch_fill_responsibilities(data->labels_dev.as<uint32_t>(), data->n, (int)K, data->lw.as<double>(), data->ldr, ctx->stream);
        const EmRoute r = em_route(data, (int)K, Covariance::Full);
        run_mstats(data, r, (int)K, kFromResp, data->lw.as<double>(), data->ldr, false);
        finalize_out(data, r, (int)K, mixing_out, means_out, covariances_out);
    });
}

int mlhip_em_responsibilities_rows(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, uint64_t first_row, uint64_t n_rows, double* resp,
                                   int64_t ldr)
{
    return guarded([&] {
        check_call(ctx, data, K);
        require(first_row <= data->rows() && n_rows <= data->rows() - first_row,
                ctx->group ? "row range beyond the sample" : "row range beyond this block");
        require(resp || n_rows == 0, "null argument");
        require(ldr >= 0 && (uint64_t)ldr >= n_rows, "ldr must be >= the number of rows");
        if (ctx->group) { grp::em_responsibilities(ctx, data, K, resp, ldr, first_row, n_rows); return; }
        require(data->has_estep_results((int)K), "no E-step results on the device for this K");
        if (!n_rows) return;
        ensure_lw(data, em_route(data, (int)K, Covariance::Full), (int)K);
        const size_t ldo = (size_t)padded_samples(n_rows);
        data->resp_dev.reserve(sizeof(double) * ldo * K);
        RespArgs a{data->lw.as<double>() + first_row, data->ldr, data->lse.as<double>() + first_row, (uint32_t)n_rows, (int)K,
                   data->resp_dev.as<double>(), ldo, nullptr};
        launch_em_responsibilities(a, ctx->stream);
        HIP_CHECK(hipGetLastError());
        ctx->sync();
        download_columns(ctx, reinterpret_cast<char*>(resp), sizeof(double) * ldr, data->resp_dev.as<char>(), sizeof(double) * ldo,
                         sizeof(double) * n_rows, K);
    });
}

int mlhip_em_responsibilities(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, double* resp, int64_t ldr)
{
    if (!data) return mlhip_em_responsibilities_rows(ctx, data, K, 0, 0, resp, ldr);      // (reports the null argument)
    return mlhip_em_responsibilities_rows(ctx, data, K, 0, data->rows(), resp, ldr);
}

int mlhip_em_labels(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, uint32_t* labels)
{
    return guarded([&] {
        check_call(ctx, data, K);
        require(labels || data->rows() == 0, "null argument");
        if (ctx->group) {
            fan_out(ctx, data, [&](Shard& sh) { return mlhip_em_labels(sh.ctx, sh.part, K, sh.rows(labels)); });
            return;
        }
        require(data->has_estep_results((int)K), "no E-step results on the device for this K");
        ensure_lw(data, em_route(data, (int)K, Covariance::Full), (int)K);
        data->labels_dev.reserve(sizeof(uint32_t) * data->n_pad);
        RespArgs a{data->lw.as<double>(), data->ldr, data->lse.as<double>(), data->n, (int)K, nullptr, 0,
                   data->labels_dev.as<uint32_t>()};
        ctx->timed("em_resp", [&] { launch_em_responsibilities(a, ctx->stream); });
        HIP_CHECK(hipGetLastError());
        ctx->sync();
        download_columns(ctx, reinterpret_cast<char*>(labels), 0, data->labels_dev.as<char>(), 0, sizeof(uint32_t) * data->n, 1);
    });
}

int mlhip_em_statistics_count(uint32_t d, uint32_t* count_per_component)
{
    return guarded([&] {
        require(d >= 1 && count_per_component, "bad argument");
        *count_per_component = (uint32_t)stats_count((int)d);
    });
}

int mlhip_em_finalize_statistics_ridge(uint32_t d, uint32_t K, const double* statistics, const double* shift, double n_global, double ridge,
                                       double* mixing_out, double* means_out, double* covariances_out)
{
    return guarded([&] {
        require(d >= 1 && K >= 1 && statistics && shift && mixing_out && means_out && covariances_out, "bad argument");
        require_ridge(ridge);
        host::finalize_mstep((int)d, (int)K, statistics, shift, n_global, ridge, mixing_out, means_out, covariances_out);
    });
}

int mlhip_em_finalize_statistics(uint32_t d, uint32_t K, const double* statistics, const double* shift, double n_global,
                                 double* mixing_out, double* means_out, double* covariances_out)
{
    return mlhip_em_finalize_statistics_ridge(d, K, statistics, shift, n_global, MLHIP_DEFAULT_COVARIANCE_RIDGE, mixing_out, means_out,
                                              covariances_out);
}

int mlhip_em_finalize_statistics_tied_ridge(uint32_t d, uint32_t K, const double* statistics, const double* total_scatter, const double* shift,
                                            double total_weight, double ridge, double* mixing_out, double* means_out, double* covariance_out)
{
    return guarded([&] {
        require(d >= 1 && K >= 1 && statistics && total_scatter && shift && mixing_out && means_out && covariance_out, "bad argument");
        require_ridge(ridge);
        host::finalize_mstep_tied((int)d, (int)K, statistics, total_scatter, shift, total_weight, ridge, mixing_out, means_out, covariance_out);
    });
}

int mlhip_em_finalize_statistics_tied(uint32_t d, uint32_t K, const double* statistics, const double* total_scatter, const double* shift,
                                      double total_weight, double* mixing_out, double* means_out, double* covariance_out)
{
    return mlhip_em_finalize_statistics_tied_ridge(d, K, statistics, total_scatter, shift, total_weight, MLHIP_DEFAULT_COVARIANCE_RIDGE,
                                                   mixing_out, means_out, covariance_out);
}

int mlhip_em_tied_route(const mlhip_data* data, uint32_t K, int* kernel)
{
    return guarded([&] {
        require(data && kernel && K >= 1, "bad argument");
        if (!data->parts.empty()) data = data->parts[0];        // (a group's block: every shard takes the same route)
        static_assert(kTiedComposed == MLHIP_TIED_COMPOSED && kTiedKernel == MLHIP_TIED_KERNEL, "mlhip.h names the routes by TiedKernel");
        *kernel = mode_route(data, (int)K, Covariance::Tied).tied_kernel;
    });
}

int mlhip_process_covariance(uint32_t d, const double* covariance, double* inverse, double* sqrt_det)
{
    return guarded([&] {
        require(d >= 1 && covariance && inverse && sqrt_det, "bad argument");
        host::process_covariance((int)d, covariance, inverse, sqrt_det);
    });
}

int mlhip_em_plan(const mlhip_data* data, uint32_t K, uint32_t* flags)
{
    return guarded([&] {
        require(data && flags && K >= 1, "null argument");
        if (!data->parts.empty()) data = data->parts[0];        // (a group's block: every shard takes the same plan)
        const EmRoute r = em_route(data, (int)K, Covariance::Full);
        uint32_t f = 0;
        if (r.fused) f |= MLHIP_PLAN_FUSED;
        else {
            if (r.estep == Estep::kMatrix4) f |= MLHIP_PLAN_MATRIX_ESTEP;
            if (r.self_norm) f |= MLHIP_PLAN_SELF_NORM;
        }
        *flags = f;
    });
}

int mlhip_em_route(const mlhip_data* data, uint32_t K, int covariance_type, mlhip_em_route_info* out)
{
    return guarded([&] {
        // (the fields describe the full and the diagonal route; the tied one is mlhip_em_tied_route's)
        require(data && out && K >= 1 && (covariance_type == MLHIP_COVARIANCE_FULL || covariance_type == MLHIP_COVARIANCE_DIAGONAL), "bad argument");
        if (!data->parts.empty()) data = data->parts[0];
        const EmRoute r = em_route(data, (int)K, (Covariance)covariance_type);
        out->estep = r.estep == Estep::kScalarFed ? MLHIP_ESTEP_SCALAR_FED : r.estep == Estep::kMatrix4 ? MLHIP_ESTEP_MATRIX4
                   : r.estep == Estep::kBigDim ? MLHIP_ESTEP_BIG_DIM : MLHIP_ESTEP_PLAIN;
        out->fused = r.fused;
        static_assert(kFusedLdsFeed == MLHIP_FUSED_LDS_FEED && kFusedScalarFeed == MLHIP_FUSED_SCALAR_FEED && kFusedValu == MLHIP_FUSED_VALU,
                      "mlhip.h names the forms by FusedArgs::form");
        out->fused_form = r.fused_form;
        out->self_norm = r.self_norm;
        out->sparse = r.sparse;
        out->balanced = r.balanced;
        out->fold_allowed = r.fold_allowed;
        out->diag_kernel = r.diag_kernel;
        out->diag_exact = r.diag_exact;
        out->device_close = r.device_close;
        out->records_on_device = r.records_on_device;
        out->resident = r.resident;
    });
}

}  // extern "C"
