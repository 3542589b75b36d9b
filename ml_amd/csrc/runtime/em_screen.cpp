// The screened E-step of a fit (em_estep_screen.hip) on the host side: ScreenState's members -- what launch_estep (em.cpp) calls around
// a pass of the screened kernel's domain -- and mlhip_em_screen_counts. Whether a pass is asked to screen is screen_wanted's rule
// (pass_history.hpp).
#include "internal.hpp"

namespace mlhip_rt {

/// The stamps of a profiled screened pass (em_estep_screen.hip, PROF form), averaged over the workgroups that stamped a tile: one line
/// on stderr, microseconds of the 100 MHz clock. tools/estep_screen_phases.py reads it.
static void report_screen_stamps(const mlhip_data* dt, const DevBuf& stamps, int grid, int K)
{
    constexpr int NS = kScreenStamps;
    std::vector<unsigned long long> t((size_t)NS * grid);
    HIP_CHECK(hipMemcpy(t.data(), stamps.p, sizeof(unsigned long long) * t.size(), hipMemcpyDeviceToHost));
    const int tile_samples = em_estep_screen_tile(dt->D), waves = tile_samples / 32;
    const int rounds = std::min(kScreenStampRounds, (K + waves - 1) / waves);   // components wave 0 takes (the stamped ones)
    double stage = 0, buckets = 0, copy = 0, eval = 0, wait = 0, tile = 0;
    int used = 0;
    for (int b = 0; b < grid; ++b) {
        const unsigned long long* s = t.data() + (size_t)NS * b;
        if (!s[0] || !s[kScreenStampTileEnd]) continue;                                  // (the workgroup had no second tile)
        ++used;
        stage += (double)(s[1] - s[0]);
        buckets += (double)(s[2] - s[1]);
        unsigned long long prev = s[2];
        for (int j = 0; j < rounds; ++j) {
            copy += (double)(s[3 + 2 * j] - prev);
            eval += (double)(s[4 + 2 * j] - s[3 + 2 * j]);
            prev = s[4 + 2 * j];
        }
        wait += (double)(s[kScreenStampTileEnd] - s[kScreenStampLoopEnd]);
        tile += (double)(s[kScreenStampTileEnd] - s[0]);
    }
    if (!used) {
        std::fprintf(stderr, "[mlhip] screened E-step, N=%u d=%d K=%d grid=%d: no workgroup had a second tile to stamp\n", dt->n, dt->d, K, grid);
        return;
    }
    const double us = 0.01 / used;
    std::fprintf(stderr, "[mlhip] screened E-step, N=%u d=%d K=%d grid=%d, us per %d-sample tile (thread 0, mean of %d workgroups): stage %.2f, "
                 "buckets %.2f, record copy %.2f, evaluation %.2f (%d components of wave 0), end barrier %.2f, tile %.2f\n",
                 dt->n, dt->d, K, grid, tile_samples, used, stage * us, buckets * us, copy * us, eval * us, rounds, wait * us, tile * us);
}

}  // namespace mlhip_rt


void ScreenState::track(mlhip_data* dt, int K)
{
    if (tracked_.K() != K) dt->estep.block_not_screenable();
    tracked_.begin(K);
    rec_.reserve(sizeof(double) * estep_mfma4_param_stride(dt->D) * K);
    exact_.reserve(sizeof(unsigned long long) * dt->n_pad);
    consts_.reserve(sizeof(double) * 4 * K);
    dev_.reserve(2 * sizeof(unsigned long long));
    host_.reserve(4 * sizeof(unsigned long long));
}


/// The constants of the step from the block's records (rec_) to `a.params`, then -- when every component's bound carries
/// information -- the screened kernel (the decision is the host's: it waits for the constants kernel's count, a few microseconds on
/// a stream that has just been waited for).
int ScreenState::run(mlhip_data* dt, const EstepArgs& a, int force)
{
    mlhip_ctx* ctx = dt->ctx;
    const int K = a.K;
    if (!screen_wanted(dt->stats_history.ring(), dt->stats_history.counts(), tracked_, host_.as<unsigned long long>(), K, dt->n, force,
                       em_estep_screen_preferred(dt->D, K), dt->estep.screenable))
        return 0;
    unsigned long long* dev = dev_.as<unsigned long long>();
    unsigned long long* host = host_.as<unsigned long long>();
    HIP_CHECK(hipMemsetAsync(dev, 0, 2 * sizeof(unsigned long long), ctx->stream));
    launch_em_screen_constants(rec_.as<double>(), a.params, K, dt->d, dt->D, consts_.as<double>(), reinterpret_cast<unsigned*>(dev),
                               ctx->stream);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(host + 3, dev, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    if (host[3] != 0) {
        n_no_info_++;
        return 0;
    }
    ScreenArgs sa{};
    sa.xt = a.xt; sa.ldx = a.ldx; sa.n = a.n; sa.D = a.D;
    sa.params = a.params; sa.K = K; sa.shift = a.shift; sa.consts = consts_.as<double>();
    sa.lw = a.lw; sa.ldr = a.ldr;
    sa.exact = exact_.as<unsigned long long>(); sa.all_exact = all_exact_ ? 1 : 0;
    sa.cand_count = dev + 1;
    // MLHIP_ESTEP_SCREEN_PROFILE=1: the kernel's stamping form; the phases of every workgroup's second tile, averaged, on stderr (diagnostic)
    static const bool profile = [] { const char* e = std::getenv("MLHIP_ESTEP_SCREEN_PROFILE"); return e && e[0] == '1'; }();
    DevBuf stamps;
    if (profile) {
        stamps.reserve(sizeof(unsigned long long) * kScreenStamps * (256 / em_estep_screen_tile(dt->D)) * ctx->num_cus);   // (a slot set per workgroup of the grid)
        HIP_CHECK(hipMemsetAsync(stamps.p, 0, stamps.bytes, ctx->stream));
        sa.profile = stamps.as<unsigned long long>();
    }
    const int grid = launch_em_estep_screen(sa, ctx->num_cus, ctx->stream);
    if (grid <= 0) throw Unsupported("screened E-step kernel not instantiated for this dimension");
    if (profile) {
        HIP_CHECK(hipGetLastError());
        ctx->sync();
        report_screen_stamps(dt, stamps, grid, K);
    }
    HIP_CHECK(hipMemcpyAsync(host + tracked_.slot(), dev + 1, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    return grid;
}


void ScreenState::pass_done(mlhip_data* dt, const EstepArgs& a, bool tracked, bool screened)
{
    (screened ? n_screened_ : n_dense_)++;
    if (!tracked) return;
    // the block now belongs to these records: the next pass of the fit may start from it
    HIP_CHECK(hipMemcpyAsync(rec_.p, a.params, sizeof(double) * estep_mfma4_param_stride(dt->D) * a.K, hipMemcpyDeviceToDevice, dt->ctx->stream));
    all_exact_ = !screened;
    tracked_.finish(screened);
    dt->estep.block_screenable();
}


void ScreenState::add_counts(uint64_t counts[4]) const
{
    counts[0] += n_screened_; counts[1] += n_dense_; counts[2] += n_no_info_;
    counts[3] += newest_screened_candidates(tracked_, host_.as<unsigned long long>());
}


extern "C" {

int mlhip_em_screen_counts(mlhip_ctx* ctx, mlhip_data* data, uint64_t counts[4])
{
    return guarded([&] {
        require(ctx && data && counts, "null argument");
        require(data->ctx == ctx, "data belongs to another context");
        for (int j = 0; j < 4; ++j) counts[j] = 0;
        auto add = [&](mlhip_data* dt) {
            dt->ctx->use();
            dt->ctx->sync();
            dt->screen.add_counts(counts);
        };
        if (data->parts.empty()) add(data);
        else for (mlhip_data* part : data->parts) add(part);
    });
}

}  // extern "C"
