// mlhip_em_iterate_restarts: R loops of mlhip_em_iterate from R starts on one resident block, and the best of them.
//
//   * SEQUENTIAL route -- the solo loop (em_loop.cpp) R times on the one handle: every shape and mode, weighted blocks, multi-rank
//     jobs (a device group fans the whole call out to its shards, which take this route);
//   * BATCHED route    -- the restarts still running share the three launches of an iteration (em_restarts.hip: pass, reduction,
//     closing, each on a grid whose second dimension is the restart), the host reads every restart's info block from pinned memory
//     and applies ConvergenceTest per restart. A restart that has converged or run out of steps leaves the launches (a compact index
//     list in the kernel arguments names the ones that stay); one whose closing raises a refinement flag leaves the batch and is run
//     solo from its own start, like any other irregularity. Same pass, same grid, same reduction order, same closing arithmetic as
//     the solo launches: every restart is bit for bit what mlhip_em_iterate gives from its start.
//
// The winner is not fitted twice: BestState keeps the SMALL E-step state of the best restart so far -- the records of its last E-step,
// their layout and FOLD flag, in diagonal / tied mode the parameters ensure_lw rebuilds from -- while later restarts run, and puts it
// back at the end; the N x K block is rebuilt on demand, as after a speculative iteration of the lagged loop.
#include "internal.hpp"

namespace mlhip_rt {

/// Restart c takes the place of restart b under the rule of mlhip_em_select_restart (mlhip.h): a total order -- converged with a
/// number, then any number, then NaN; the greater log-likelihood; the smaller index -- so the running best does not depend on the
/// order the restarts finish in.
static bool restart_better(uint32_t c, uint32_t b, const double* ll, const int* converged)
{
    const int cc = std::isnan(ll[c]) ? 0 : converged[c] ? 2 : 1, cb = std::isnan(ll[b]) ? 0 : converged[b] ? 2 : 1;
    if (cc != cb) return cc > cb;
    if (cc != 0 && ll[c] != ll[b]) return ll[c] > ll[b];
    return c < b;
}

uint32_t select_restart(uint32_t R, const double* ll, const int* converged)
{
    for (int pass = 0; pass < 2; ++pass) {                    // the converged restarts, then all of them
        int64_t best = -1;
        for (uint32_t r = 0; r < R; ++r) {
            if ((pass == 0 && !converged[r]) || std::isnan(ll[r])) continue;
            if (best < 0 || ll[r] > ll[best]) best = r;        // strict: the first of equals stays
        }
        if (best >= 0) return (uint32_t)best;
    }
    return 0;
}

namespace {

/// The E-step state of the best restart so far: live on the handle (`in_place`), or its small part kept aside -- the records in
/// rs_kept, the rest in `small` -- while the handle runs other restarts.
struct BestState {
    mlhip_data* data;
    EstepState::Small small;
    bool in_place = false;

    /// Before another loop runs on the handle: the live state of the best restart goes aside (the record BUFFERS change places:
    /// the next loop builds its records anew anyway).
    void stash()
    {
        if (!in_place) return;
        small = data->estep.small();
        std::swap(data->rs_kept, data->params_dev);
        data->estep.invalidate();
        in_place = false;
    }
    /// A restart of the batched loop became the best: its records (device, `doubles` of them, valu layout) are copied aside.
    void keep_records(const double* records, size_t doubles, int n_ll)
    {
        data->rs_kept.reserve(std::max(sizeof(double) * doubles, data->params_dev.bytes));
        HIP_CHECK(hipMemcpyAsync(data->rs_kept.p, records, sizeof(double) * doubles, hipMemcpyDeviceToDevice, data->ctx->stream));
        small = EstepState::Small{};
        small.what = EstepState::kRecords;
        small.n_ll = n_ll;
        in_place = false;
    }
    /// The loop that just ran on the handle is the best one now.
    void live() { in_place = true; }
    /// When all restarts are over: the best one's state back on the handle.
    void put_back()
    {
        if (in_place) return;
        std::swap(data->rs_kept, data->params_dev);
        data->estep.put_back(small);
        in_place = true;
    }
};

/// One solo loop on the handle: restart r of the caller's arrays.
struct SoloRun {
    mlhip_data* data;
    int K;
    Covariance mode;
    size_t kd, n_cov;
    double *mixing, *means, *covs;
    uint32_t max_steps;
    double atol, rtol;
    uint32_t* steps_done;
    int* converged;
    double *log_likelihood, *history;

    void operator()(uint32_t r) const
    {
        double* pi = mixing + (size_t)r * K;
        double* mu = means + (size_t)r * kd;
        double* cv = covs + (size_t)r * n_cov;
        double* hist = history ? history + (size_t)r * max_steps : nullptr;
        em_iterate(data, mode, K, pi, mu, cv, max_steps, atol, rtol, steps_done + r, converged + r, log_likelihood + r, hist);
        data->ctx->check_ranks_agree("the EM parameters", {{pi, (size_t)K}, {mu, kd}, {cv, n_cov}, {log_likelihood + r, 1}});
    }
};

/// `runs` (ascending restart indices) one after the other through `solo`, the running best `*best` (valid when `have_best`) and its
/// state kept up to date.
void run_sequential(const SoloRun& solo, const std::vector<uint32_t>& runs, BestState& state, bool have_best, uint32_t* best)
{
    for (uint32_t r : runs) {
        state.stash();
        solo(r);
        if (!have_best || restart_better(r, *best, solo.log_likelihood, solo.converged)) {
            *best = r;
            have_best = true;
            state.live();
        }
    }
}

}  // namespace

void em_iterate_restarts_batched(mlhip_data* data, const RestartsRoute& route, int K, uint32_t R, double* mixing, double* means, double* covs,
                                 uint32_t max_steps, double atol, double rtol, uint32_t* steps_done, int* converged, double* log_likelihood,
                                 double* history, uint32_t* best)
{
    mlhip_ctx* ctx = data->ctx;
    const int d = data->d, g = route.grid;
    ensure_em_workspace(data, K);
    const size_t n_rec = (size_t)K * estep_param_stride(d), kd = (size_t)K * d, n_cov = kd * d, n_pack = K + kd + n_cov;
    const size_t block = (size_t)mstats::em_fused_partial_rows(K) * mstats::em_fused_partial_cols(d);
    const size_t n_stats = (size_t)K * stats_count(d) + 1, n_info = em_close_info_doubles(K);
    const uint32_t M = std::min<uint32_t>((uint32_t)route.per_launch, R);
    // The loop waits for every iteration before it launches the next (nothing runs ahead), so two record slots per restart -- an
    // iteration reads slot i % 2 and writes the other -- and ONE pack and info block do. One device block: [2][M] records | [M] packs |
    // [M][g] partial blocks | [M][g] ll partials | [M] statistics; pinned: [M] info blocks | [M] records on their way up
    data->rs_dev.reserve(sizeof(double) * M * restarts_doubles_per_restart(d, K, g));
    data->rs_info.reserve(sizeof(double) * M * (n_info + n_rec));
    double* const rec_pair = data->rs_dev.as<double>();
    double* const packs = rec_pair + 2 * M * n_rec;
    double* const partials = packs + M * n_pack;
    double* const ll_partials = partials + (size_t)M * g * block;
    double* const stats = ll_partials + (size_t)M * g;
    double* const info = data->rs_info.as<double>();
    double* const staging = info + M * n_info;

    RestartsArgs a{};
    a.xt = data->xt.as<double>(); a.ldx = data->ldx; a.n = data->n; a.d = d; a.K = K;
    a.shift = data->shift_dev.as<double>(); a.grid = g;
    a.records_stride = n_rec; a.pack_stride = n_pack; a.info_stride = n_info;
    a.partials = partials; a.partials_stride = (size_t)g * block;
    a.ll_partials = ll_partials; a.ll_stride = (size_t)g;
    a.stats = stats; a.stats_stride = n_stats;
    a.n_global = data->total_weight(); a.ridge = data->ridge; a.refine_limit = refine_ratio();
    const double ll_offset = (double)d * log_two_pi() / 2;                 // (em_loop.cpp read(): the same expression)

    BestState state{data, {}, false};
    bool have_best = false;
    std::vector<uint32_t> solo_runs;                                       // restarts the batch handed back: run solo from their starts
    for (uint32_t r = 0; r < R; ++r) { steps_done[r] = 0; converged[r] = 0; }

    for (uint32_t r0 = 0; r0 < R; r0 += M) {
        const uint32_t Mg = std::min(M, R - r0);
        // records R_0 of every start into record slot 0 (the host builder of the solo loop's prepare_estep)
        for (uint32_t m = 0; m < Mg; ++m) {
            const uint32_t r = r0 + m;
            host::build_estep_params(d, data->D, K, mixing + (size_t)r * K, means + r * kd, covs + r * n_cov, staging + m * n_rec);
        }
        HIP_CHECK(hipMemcpyAsync(rec_pair, staging, sizeof(double) * Mg * n_rec, hipMemcpyHostToDevice, ctx->stream));
        std::vector<ConvergenceTest> tests;
        for (uint32_t m = 0; m < Mg; ++m) {
            const uint32_t r = r0 + m;
            tests.push_back(ConvergenceTest{atol, rtol, steps_done + r, converged + r, log_likelihood + r,
                                            history ? history + (size_t)r * max_steps : nullptr});
        }
        std::vector<int64_t> last(Mg, -1);                                 // the last iteration of a restart that finished in the batch
        RestartsAlive alive{};
        alive.count = (int)Mg;
        for (uint32_t m = 0; m < Mg; ++m) alive.index[m] = (unsigned char)m;

        for (uint32_t i = 0; i < max_steps && alive.count > 0; ++i) {
            const size_t in = i % 2, out = (i + 1) % 2;
            a.alive = alive;
            a.records_in = rec_pair + in * M * n_rec;
            a.records_out = rec_pair + out * M * n_rec;
            a.mixing = packs; a.means = a.mixing + K; a.covs = a.means + kd;
            a.info = info;
            bool ok = true;
            ctx->timed("em_restarts_pass", [&] { ok = mstats::launch_em_restarts_pass(a, ctx->stream); });
            if (ok) ctx->timed("em_restarts_reduce", [&] { ok = mstats::launch_em_restarts_reduce(a, ctx->stream); });
            if (ok) ctx->timed("em_restarts_close", [&] { ok = mstats::launch_em_restarts_close(a, ctx->stream); });
            if (!ok) throw std::runtime_error("batched EM restarts kernels not instantiated for this shape");
            HIP_CHECK(hipGetLastError());
            ctx->sync();
            RestartsAlive next{};
            bool fetched = false;
            for (int y = 0; y < alive.count; ++y) {
                const uint32_t m = alive.index[y], r = r0 + m;
                const double* inf = a.info + m * n_info;
                bool flagged = false;
                for (int k = 0; k < K; ++k) flagged = flagged || inf[1 + k] != 0.0;
                if (flagged) { solo_runs.push_back(r); continue; }         // a far, tight component: the solo loop closes it on the host
                const double ll = inf[0] / data->total_weight() - ll_offset;
                if (tests[m](i, ll) || i + 1 == max_steps) {
                    last[m] = i;
                    const double* pack = a.mixing + m * n_pack;            // P_(i + 1): the newest parameters
                    HIP_CHECK(hipMemcpyAsync(mixing + (size_t)r * K, pack, sizeof(double) * K, hipMemcpyDeviceToHost, ctx->stream));
                    HIP_CHECK(hipMemcpyAsync(means + r * kd, pack + K, sizeof(double) * kd, hipMemcpyDeviceToHost, ctx->stream));
                    HIP_CHECK(hipMemcpyAsync(covs + r * n_cov, pack + K + kd, sizeof(double) * n_cov, hipMemcpyDeviceToHost, ctx->stream));
                    fetched = true;
                } else {
                    next.index[next.count++] = (unsigned char)m;
                }
            }
            if (fetched) ctx->sync();
            alive = next;
        }
        // the best of this group against the best so far; its records (the slot its last E-step read) are kept before the next group reuses the slots
        int64_t group_best = -1;
        for (uint32_t m = 0; m < Mg; ++m) {
            if (last[m] < 0) continue;
            const uint32_t r = r0 + m;
            if (!have_best || restart_better(r, *best, log_likelihood, converged)) { *best = r; have_best = true; group_best = m; }
        }
        if (group_best >= 0)
            state.keep_records(rec_pair + ((size_t)(last[group_best] % 2) * M + group_best) * n_rec, n_rec, g);
        ctx->sync();
    }

    // flagged restarts: the solo loop from their (untouched) starts, results and history written anew
    for (uint32_t r : solo_runs) { steps_done[r] = 0; converged[r] = 0; }
    const SoloRun solo{data, K, Covariance::Full, kd, n_cov, mixing, means, covs, max_steps, atol, rtol, steps_done, converged,
                       log_likelihood, history};
    run_sequential(solo, solo_runs, state, have_best, best);
    state.put_back();
    if (*best != select_restart(R, log_likelihood, converged)) throw std::runtime_error("EM restarts: the running selection disagrees with the rule");
}

}  // namespace mlhip_rt

extern "C" {

int mlhip_em_select_restart(uint32_t R, const double* log_likelihood, const int* converged, uint32_t* best)
{
    return guarded([&] {
        require(R >= 1 && log_likelihood && converged && best, "bad argument");
        *best = select_restart(R, log_likelihood, converged);
    });
}

int mlhip_em_restarts_route(const mlhip_data* data, uint32_t K, int covariance_type, uint32_t R, int* route, uint32_t* per_launch)
{
    return guarded([&] {
        require(data && route && per_launch && K >= 1 && R >= 1, "bad argument");
        const Covariance mode = covariance_from_abi(covariance_type);
        static_assert(kRestartsSequential == MLHIP_RESTARTS_SEQUENTIAL && kRestartsBatched == MLHIP_RESTARTS_BATCHED,
                      "mlhip.h names the routes by RestartsKind");
        static_assert(mstats::kRestartsMaxBatch == MLHIP_RESTARTS_MAX_BATCH, "mlhip.h states the cap of one launch");
        *route = MLHIP_RESTARTS_SEQUENTIAL;
        *per_launch = 1;
        if (!data->parts.empty()) return;                       // a group's block: its shards are ranks of an all-reduce
        const RestartsRoute r = restarts_route(data, (int)K, mode, R);
        *route = r.kind;
        *per_launch = (uint32_t)r.per_launch;
    });
}

int mlhip_em_iterate_restarts(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, int covariance_type, uint32_t R, double* mixing, double* means,
                              double* covariances, uint32_t max_steps, double absolute_tolerance, double relative_tolerance,
                              uint32_t* steps_done, int* converged, double* log_likelihood, double* log_likelihood_history, uint32_t* best)
{
    return guarded([&] {
        check_call(ctx, data, K);
        require(mixing && means && covariances && steps_done && converged && log_likelihood && best, "null argument");
        const Covariance mode = covariance_from_abi(covariance_type);
        require(R >= 1, "at least one restart required");
        require(max_steps >= 1, "at least one step required");
        if (absolute_tolerance < 0 || relative_tolerance < 0) throw DomainError("negative tolerance");
        const size_t kd = (size_t)K * data->d, n_cov = covariance_doubles(mode, (int)K, data->d);
        if (ctx->group) {
            // the parameters are in/out, as in mlhip_em_iterate: shard 0 updates the caller's, the others copies of their own; every
            // shard sees the same all-reduced log-likelihoods and selects the same restart
            const size_t n_pi = (size_t)R * K, n_mu = R * kd, n_cv = R * n_cov;
            const std::vector<double> pi(mixing, mixing + n_pi), mu(means, means + n_mu), cv(covariances, covariances + n_cv);
            fan_out(ctx, data, [&](Shard& sh) {
                return mlhip_em_iterate_restarts(sh.ctx, sh.part, K, covariance_type, R, sh.replicated(mixing, n_pi, pi.data()),
                                                 sh.replicated(means, n_mu, mu.data()), sh.replicated(covariances, n_cv, cv.data()),
                                                 max_steps, absolute_tolerance, relative_tolerance, sh.replicated(steps_done, R),
                                                 sh.replicated(converged, R), sh.replicated(log_likelihood, R),
                                                 sh.replicated(log_likelihood_history, (size_t)R * max_steps), sh.scalar(best, "restarts"));
            });
            return;
        }
        const RestartsRoute route = restarts_route(data, (int)K, mode, R);
        if (route.kind == kRestartsBatched) {
            em_iterate_restarts_batched(data, route, (int)K, R, mixing, means, covariances, max_steps, absolute_tolerance, relative_tolerance,
                                        steps_done, converged, log_likelihood, log_likelihood_history, best);
            return;
        }
        const SoloRun solo{data, (int)K, mode, kd, n_cov, mixing, means, covariances, max_steps, absolute_tolerance,
                           relative_tolerance, steps_done, converged, log_likelihood, log_likelihood_history};
        std::vector<uint32_t> runs(R);
        for (uint32_t r = 0; r < R; ++r) runs[r] = r;
        BestState state{data, {}, false};
        *best = 0;
        run_sequential(solo, runs, state, false, best);
        state.put_back();
        if (*best != select_restart(R, log_likelihood, converged)) throw std::runtime_error("EM restarts: the running selection disagrees with the rule");
    });
}

}  // extern "C"
