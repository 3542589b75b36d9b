// K-means family of the C ABI: assignment + exact update sums per step, the step loop of KMeans::fit_once in one call.
#include <cmath>
#include <vector>

#include "device/fixed_point.hpp"
#include "internal.hpp"

namespace mlhip_rt {


void ensure_km_workspace(mlhip_data* dt, int K)
{
    mlhip_ctx* ctx = dt->ctx;
    for (int b = 0; b < 2; ++b) dt->km_labels[b].reserve(sizeof(uint32_t) * dt->n_pad);
    dt->km_mind.reserve(sizeof(double) * dt->n_pad);
    if (!dt->km_scale.p) {
        // Per-dimension power-of-two scale of the exact fixed-point sums: |x_j| * 2^(94 - e_j) < 2^94 (device/kmeans.hip), applied
        // as two powers of two [f1 (d) | f2 (d)] so that neither step leaves the normal range whatever the column's magnitude is
        // (94 - e_j reaches 1167 on a column of subnormals: one factor would be +inf from max|x_j| < 2^-929 down).
        DevBuf scratch, mx;
        scratch.reserve(sizeof(double) * 1024 * dt->d);
        mx.reserve(sizeof(double) * dt->d);
        launch_column_maxabs(dt->xt.as<double>(), dt->ldx, dt->d, dt->n, scratch.as<double>(), mx.as<double>(), ctx->stream);
        std::vector<double> m(dt->d);
        HIP_CHECK(hipMemcpyAsync(m.data(), mx.p, sizeof(double) * dt->d, hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
        // Every rank must cut its coordinates on the SAME fixed-point grid (the limb sums are added across ranks): the
        // column maxima are exchanged through the sum hook, one slot per rank, and every rank takes the maximum.
        const std::vector<double> all = ctx->exchange_slots(m.data(), m.size());
        for (size_t t = 0; t < all.size(); ++t) {
            const double v = all[t];
            double& mj = m[t % m.size()];
            if (!(v <= mj)) mj = v;                                        // (keeps a NaN / inf of any rank)
        }
        dt->km_colmax = m;                                       // (the weighted sums' overflow test: ensure_km_weighted)
        std::vector<double> f(2 * (size_t)dt->d);
        for (int j = 0; j < dt->d; ++j) {
            if (!std::isfinite(m[j]))
                throw DomainError("K-means: the data contain non-finite values (the exact fixed-point update sums need finite coordinates)");
            int e = 0;
            if (m[j] > 0) (void)std::frexp(m[j], &e);   // m < 2^e
            const int E = 94 - e, h = E >= 0 ? E / 2 : -((-E) / 2);
            f[j] = std::ldexp(1.0, h);
            f[(size_t)dt->d + j] = std::ldexp(1.0, E - h);
        }
        dt->km_scale.reserve(sizeof(double) * f.size());
        HIP_CHECK(hipMemcpyAsync(dt->km_scale.p, f.data(), sizeof(double) * f.size(), hipMemcpyHostToDevice, ctx->stream));
        ctx->sync();
    }
    const int Dp = (dt->D + 3) & ~3;                              // (the K-means kernels may run on a zero-padded copy)
    dt->km_cent.reserve(sizeof(double) * (size_t)K * Dp);
    dt->km_cnorm.reserve(sizeof(double) * (size_t)((K + 15) & ~15));
    dt->km_partials.reserve(sizeof(double) * kmeans_scratch_doubles(dt->d, K, ctx->num_cus));
    const size_t ob = sizeof(double) * (2 + (size_t)K * (dt->d + 1));
    dt->km_out.reserve(ob);
    const size_t hb = ob > sizeof(double) * (size_t)K * Dp ? ob : sizeof(double) * (size_t)K * Dp;
    dt->km_host.reserve(hb);
}


void ensure_km_weighted(mlhip_data* dt, int K)
{
    mlhip_ctx* ctx = dt->ctx;
    ensure_km_workspace(dt, K);
    const size_t scratch = kmeans_weighted_scratch_doubles(dt->d, K, ctx->num_cus);
    if (scratch > kmeans_scratch_doubles(dt->d, K, ctx->num_cus)) dt->km_partials.reserve(sizeof(double) * scratch);
    if (dt->km_wfactors_valid) return;
    // the largest weight of the whole sample: the weight vector as a one-row block, exchanged across ranks like the column maxima
    const int d = dt->d;
    DevBuf scratch_dev, mx;
    scratch_dev.reserve(sizeof(double) * 1024);
    mx.reserve(sizeof(double));
    launch_column_maxabs(dt->weights.as<double>(), dt->n_pad, 1, dt->n, scratch_dev.as<double>(), mx.as<double>(), ctx->stream);
    HIP_CHECK(hipGetLastError());
    double wmax = 0.0;
    HIP_CHECK(hipMemcpyAsync(&wmax, mx.p, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    for (double v : ctx->exchange_slots(&wmax, 1))
        if (!(v <= wmax)) wmax = v;
    // (mlhip_data_set_weights accepted the weights: finite, >= 0, a positive total -- so 0 < wmax < inf)
    int ew = 0;
    (void)std::frexp(wmax, &ew);                                 // wmax < 2^ew
    std::vector<double> f(2 * (size_t)d + 2);
    for (int j = 0; j < d; ++j) {
        if (!std::isfinite(wmax * dt->km_colmax[j]))
            throw DomainError("weighted K-means: the largest weight times the largest |x_j| overflows");
        int ej = 0;
        if (dt->km_colmax[j] > 0) (void)std::frexp(dt->km_colmax[j], &ej);
        // |w x_j| 2^E < 2^94, applied as two powers of two so that neither step leaves the normal range; E is capped where the
        // products themselves are about to underflow (ej + ew < -1946)
        const int E = std::min(94 - ej - ew, 2040);
        const int h = E >= 0 ? E / 2 : -((-E) / 2);
        f[j] = std::ldexp(1.0, h);
        f[(size_t)d + j] = std::ldexp(1.0, E - h);
    }
    const int C = 94 - ew, hc = C >= 0 ? C / 2 : -((-C) / 2);
    f[2 * (size_t)d] = std::ldexp(1.0, hc);
    f[2 * (size_t)d + 1] = std::ldexp(1.0, C - hc);
    dt->km_wfactors.reserve(sizeof(double) * f.size());
    HIP_CHECK(hipMemcpyAsync(dt->km_wfactors.p, f.data(), sizeof(double) * f.size(), hipMemcpyHostToDevice, ctx->stream));
    ctx->sync();                                                 // (f is a local)
    dt->km_wfactors_valid = true;
}


KmBlock km_block(mlhip_data* dt, const KmRoute& r, int K)
{
    mlhip_ctx* ctx = dt->ctx;
    ensure_km_workspace(dt, K);
    KmBlock b{dt->xt.as<double>(), dt->D};
    if (r.pad) {                                                  // (zero rows: every distance, label and sum unchanged)
        const int Dp = (b.D + 3) & ~3;
        if (!dt->km_xt_pad.p) {
            dt->km_xt_pad.reserve(sizeof(double) * dt->ldx * Dp);
            HIP_CHECK(hipMemsetAsync(dt->km_xt_pad.p, 0, sizeof(double) * dt->ldx * Dp, ctx->stream));
            HIP_CHECK(hipMemcpyAsync(dt->km_xt_pad.p, dt->xt.p, sizeof(double) * dt->ldx * b.D, hipMemcpyDeviceToDevice, ctx->stream));
        }
        b.D = Dp;
        b.xt = dt->km_xt_pad.as<double>();
    }
    return b;
}


/// Host centroids [K][d] -> the device table km_cent [K][D] (padded coordinates zero).
void km_upload_centroids(mlhip_data* dt, int K, const KmBlock& b, const double* centroids)
{
    mlhip_ctx* ctx = dt->ctx;
    double* ch = dt->km_host.as<double>();
    for (int k = 0; k < K; ++k)
        for (int j = 0; j < b.D; ++j) ch[(size_t)k * b.D + j] = j < dt->d ? centroids[(size_t)k * dt->d + j] : 0.0;
    HIP_CHECK(hipMemcpyAsync(dt->km_cent.p, ch, sizeof(double) * (size_t)K * b.D, hipMemcpyHostToDevice, ctx->stream));
    ctx->sync();   // km_host is reused for the results
}


/// Assignment (+ optional accumulation) against the table in km_cent, partials reduced into km_out =
/// [inertia, changed, counts, sums] and summed across ranks there when the all-reduce works on device memory.
void km_launch(mlhip_data* dt, const KmRoute& r, int K, const KmBlock& b, bool accumulate, double* min_dist_out, bool weighted)
{
    mlhip_ctx* ctx = dt->ctx;
    const int nxt = dt->km_cur ^ 1;
    KmeansArgs a{};
    a.xt = b.xt; a.ldx = dt->ldx; a.n = dt->n; a.D = b.D; a.d = dt->d;
    a.centroids = dt->km_cent.as<double>(); a.K = K;
    a.scale = dt->km_scale.as<double>();
    a.labels = dt->km_labels[nxt].as<uint32_t>();
    a.old_labels = dt->km_labels[dt->km_cur].as<uint32_t>();
    a.have_old = dt->km_have_old ? 1 : 0;
    a.min_dist = min_dist_out ? min_dist_out : dt->km_mind.as<double>();   // a distance-only probe writes elsewhere
    a.accumulate = accumulate && !weighted ? 1 : 0;              // (weighted: the sums are the sweep's, after the assignment)
    a.partials = dt->km_partials.as<double>(); a.partials_capacity = dt->km_partials.bytes / sizeof(double);
    a.cnorm = dt->km_cnorm.as<double>();
    a.out = dt->km_out.as<double>();
    a.kernel = r.kernel;
    int rc = 0;
    ctx->timed("kmeans_assign", [&] { rc = launch_kmeans_assign(a, ctx->num_cus, ctx->stream); });
    if (rc == -1) throw Unsupported("K-means kernel not instantiated for this dimension");
    if (rc <= 0) throw std::runtime_error("K-means kernel launch failed");
    launch_kmeans_reduce(a, rc, ctx->stream);
    HIP_CHECK(hipGetLastError());
    if (weighted) {
        // labels, distances and n_changed are the unweighted call's; inertia, counts and sums come from the weighted sweep over the
        // UNPADDED block (the partial blocks are free again: the reduction above is ordered before it on the stream)
        KmWeightedArgs wa{};
        wa.xt = dt->xt.as<double>(); wa.ldx = dt->ldx; wa.n = dt->n; wa.d = dt->d;
        wa.labels = a.labels; wa.min_dist = a.min_dist;
        wa.weights = dt->weights.as<double>(); wa.factors = dt->km_wfactors.as<double>();
        wa.K = K; wa.with_sums = accumulate ? 1 : 0;
        wa.partials = a.partials; wa.partials_capacity = a.partials_capacity;
        wa.out = a.out;
        int wrc = 0;
        ctx->timed("kmeans_weighted", [&] { wrc = launch_kmeans_weighted(wa, ctx->num_cus, ctx->stream); });
        if (wrc <= 0) throw std::runtime_error("weighted K-means sweep launch failed");
        HIP_CHECK(hipGetLastError());
    }
    dt->km_cur = nxt;
    dt->km_have_old = true;
    ctx->reduce_on_stream(dt->km_out.as<double>(), 2 + (accumulate ? (size_t)K * (dt->d + 1) : 0));
}


/// km_out -> km_host (`count` doubles), summed across ranks on the host when the all-reduce works on host memory.
void km_fetch(mlhip_data* dt, size_t count)
{
    dt->ctx->fetch_reduced(dt->km_host.as<double>(), dt->km_out.as<double>(), count);
}


/// Assignment (+ optional accumulation); leaves all-reduced [inertia, changed, counts, sums] in km_host.
void run_kmeans(mlhip_data* dt, const KmRoute& r, int K, const double* centroids, bool accumulate, double* min_dist_out, bool weighted)
{
    const KmBlock b = km_block(dt, r, K);
    km_upload_centroids(dt, K, b, centroids);
    km_launch(dt, r, K, b, accumulate, min_dist_out, weighted);
    km_fetch(dt, 2 + (accumulate ? (size_t)K * (dt->d + 1) : 0));
}


/// update_step's closing arithmetic on the host (ML/KMeans.cpp:180-192 as sums / counts; empty cluster -> origin, :184).
void km_close_host(const double* r, int K, int d, double* counts, double* centroids_out)
{
    for (int k = 0; k < K; ++k) {
        const double c = r[2 + k];
        if (counts) counts[k] = c;
        for (int j = 0; j < d; ++j) centroids_out[(size_t)k * d + j] = c > 0 ? r[2 + K + (size_t)k * d + j] / c : 0.0;
    }
}


/// The step loop of KMeans::fit_once (ML/KMeans.cpp:80-110). With the all-reduce on device memory (or none) the centroid
/// table never leaves the device between trips: sums -> means -> next table by launch_kmeans_close, one read-back per trip
/// for the two stopping tests. With a host-memory all-reduce (gloo rehearsals) every trip goes through run_kmeans.
void km_iterate(mlhip_data* dt, const KmRoute& route, int K, double* centroids, double* old_centroids, uint32_t max_steps, double atol,
                uint32_t* steps_done, int* converged, double* inertia, double* counts, bool weighted)
{
    mlhip_ctx* ctx = dt->ctx;
    const int d = dt->d;
    const size_t kd = (size_t)K * d;
    const bool device_route = !(ctx->reduce_fn && !ctx->reduce_on_device);
    const KmBlock b = km_block(dt, route, K);
    std::vector<double> cur(centroids, centroids + kd), old(kd, 0.0), upd(kd);
    // Small blocks with few clusters in the dimensions of the direct-form kernel: the whole loop in ONE launch of one workgroup
    // (device/kmeans_resident.hip; bit-identical to the launches below).
    if (route.resident && !weighted) {
        const size_t n_out = 4 + (size_t)K + 2 * kd;
        dt->km_host.reserve(sizeof(double) * (n_out > (size_t)K * b.D ? n_out : (size_t)K * b.D));
        km_upload_centroids(dt, K, b, cur.data());
        KmResidentArgs a{};
        a.xt = b.xt; a.ldx = dt->ldx; a.n = dt->n; a.D = b.D; a.d = d; a.K = K;
        a.cent = dt->km_cent.as<double>(); a.scale = dt->km_scale.as<double>();
        a.labels[0] = dt->km_labels[0].as<uint32_t>(); a.labels[1] = dt->km_labels[1].as<uint32_t>();
        a.label_buf = dt->km_cur; a.have_old = dt->km_have_old ? 1 : 0;
        a.min_dist = dt->km_mind.as<double>();
        a.max_steps = max_steps; a.atol = atol;
        a.out = dt->km_host.as<double>();
        bool ok = false;
        ctx->timed("kmeans_resident", [&] { ok = launch_kmeans_resident(a, ctx->stream); });
        if (!ok) throw std::runtime_error("resident K-means kernel not instantiated for this dimension");
        HIP_CHECK(hipGetLastError());
        ctx->sync();
        const double* r = dt->km_host.as<double>();
        *steps_done = (uint32_t)std::llround(r[0]);
        *converged = r[1] != 0.0 ? 1 : 0;
        *inertia = r[2];
        dt->km_cur = (int)std::llround(r[3]);
        dt->km_have_old = true;
        if (counts) std::copy(r + 4, r + 4 + K, counts);
        std::copy(r + 4 + K, r + 4 + K + kd, centroids);
        if (old_centroids) std::copy(r + 4 + K + kd, r + 4 + K + 2 * kd, old_centroids);
        return;
    }
    if (device_route) {
        dt->km_cent_next.reserve(sizeof(double) * (size_t)K * b.D);
        km_upload_centroids(dt, K, b, cur.data());
    }
    *converged = 0;
    *steps_done = 0;
    for (uint32_t step = 0; step < max_steps; ++step) {
        if (device_route) {
            // (the closing arithmetic writes the block into the pinned km_host as well: no copy-engine transfer in the loop)
            km_launch(dt, route, K, b, true, nullptr, weighted);
            launch_kmeans_close(dt->km_out.as<double>(), K, d, b.D, dt->km_cent_next.as<double>(), dt->km_host.as<double>(), ctx->stream);
            HIP_CHECK(hipGetLastError());
            ctx->sync();
            const double* r = dt->km_host.as<double>();
            if (counts) std::copy(r + 2, r + 2 + K, counts);
            std::copy(r + 2 + K, r + 2 + K + kd, upd.begin());
        } else {
            run_kmeans(dt, route, K, cur.data(), true, nullptr, weighted);
            km_close_host(dt->km_host.as<double>(), K, d, counts, upd.data());
        }
        const double* r = dt->km_host.as<double>();
        *inertia = r[0];
        const uint64_t changed = (uint64_t)std::llround(r[1]);
        ++*steps_done;
        if (step > 0 && changed == 0) {   // same labels twice (:84-89): the centroids stay as they are
            *converged = 1;
            break;
        }
        old.swap(cur);                    // update_step (:180-192)
        cur.swap(upd);
        if (device_route) std::swap(dt->km_cent, dt->km_cent_next);
        if (step > 0) {
            double shift = 0;
            for (size_t t = 0; t < kd; ++t) {
                const double delta = cur[t] - old[t];
                shift += delta * delta;
            }
            if (shift < atol) {           // (:103-108) one more assignment under the final centroids
                if (device_route) {
                    km_launch(dt, route, K, b, false, nullptr, weighted);
                    km_fetch(dt, 2);
                } else {
                    run_kmeans(dt, route, K, cur.data(), false, nullptr, weighted);
                }
                *inertia = dt->km_host.as<double>()[0];
                *converged = 1;
                break;
            }
        }
    }
    std::copy(cur.begin(), cur.end(), centroids);
    if (old_centroids) std::copy(old.begin(), old.end(), old_centroids);
}

}  // namespace mlhip_rt

extern "C" {


namespace {
// The three Lloyd entry points in their two forms: `weighted` runs the weighted sweep after the (unchanged) assignment.
int kmeans_step_impl(bool weighted, mlhip_ctx* ctx, mlhip_data* data, uint32_t K, const double* centroids, double* inertia,
                     uint64_t* n_changed, double* counts, double* centroids_out)
{
    return guarded([&] {
        check_call(ctx, data, K);
        require(centroids && inertia && n_changed && counts && centroids_out, "null argument");
        if (weighted) require(data->weighted, "weighted K-means: no weights attached to the data (mlhip_data_set_weights)");
        if (ctx->group) {
            const size_t kd = (size_t)K * data->d;
            const std::vector<double> in(centroids, centroids + kd);   // (centroids_out may alias centroids)
            fan_out(ctx, data, [&](Shard& sh) {
                return kmeans_step_impl(weighted, sh.ctx, sh.part, K, in.data(), sh.scalar(inertia), sh.scalar(n_changed),
                                        sh.replicated(counts, K), sh.replicated(centroids_out, kd));
            });
            return;
        }
        if (weighted) ensure_km_weighted(data, (int)K);
        run_kmeans(data, km_route(data, (int)K), (int)K, centroids, true, nullptr, weighted);
        const double* r = data->km_host.as<double>();
        *inertia = r[0];
        *n_changed = (uint64_t)std::llround(r[1]);
        km_close_host(r, (int)K, data->d, counts, centroids_out);
    });
}

int kmeans_iterate_impl(bool weighted, mlhip_ctx* ctx, mlhip_data* data, uint32_t K, double* centroids, double* old_centroids,
                        uint32_t max_steps, double absolute_tolerance, uint32_t* steps_done, int* converged,
                        double* inertia, double* counts)
{
    return guarded([&] {
        check_call(ctx, data, K);
        require(centroids && steps_done && converged && inertia, "null argument");
        if (weighted) require(data->weighted, "weighted K-means: no weights attached to the data (mlhip_data_set_weights)");
        require(max_steps >= 1, "at least one step");
        require(absolute_tolerance >= 0, "negative tolerance");
        if (ctx->group) {
            const size_t kd = (size_t)K * data->d;
            const std::vector<double> start(centroids, centroids + kd);   // (in/out: shard 0 updates the caller's, the others copies)
            fan_out(ctx, data, [&](Shard& sh) {
                return kmeans_iterate_impl(weighted, sh.ctx, sh.part, K, sh.replicated(centroids, kd, start.data()),
                                           sh.replicated(old_centroids, kd), max_steps, absolute_tolerance, sh.scalar(steps_done, "steps"),
                                           sh.scalar(converged, "steps"), sh.scalar(inertia), sh.replicated(counts, K));
            });
            return;
        }
        if (weighted) ensure_km_weighted(data, (int)K);
        km_iterate(data, km_route(data, (int)K), (int)K, centroids, old_centroids, max_steps, absolute_tolerance, steps_done, converged, inertia,
                   counts, weighted);
        ctx->check_ranks_agree("the K-means centroids", {{centroids, (size_t)K * data->d}, {inertia, 1}});
    });
}

int kmeans_assign_impl(bool weighted, mlhip_ctx* ctx, mlhip_data* data, uint32_t K, const double* centroids, double* inertia,
                       uint64_t* n_changed)
{
    return guarded([&] {
        check_call(ctx, data, K);
        require(centroids && inertia && n_changed, "null argument");
        if (weighted) require(data->weighted, "weighted K-means: no weights attached to the data (mlhip_data_set_weights)");
        if (ctx->group) {
            fan_out(ctx, data, [&](Shard& sh) {
                return kmeans_assign_impl(weighted, sh.ctx, sh.part, K, centroids, sh.scalar(inertia), sh.scalar(n_changed));
            });
            return;
        }
        if (weighted) ensure_km_weighted(data, (int)K);
        run_kmeans(data, km_route(data, (int)K), (int)K, centroids, false, nullptr, weighted);
        const double* r = data->km_host.as<double>();
        *inertia = r[0];
        *n_changed = (uint64_t)std::llround(r[1]);
    });
}
}  // namespace

int mlhip_kmeans_step(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, const double* centroids, double* inertia,
                      uint64_t* n_changed, double* counts, double* centroids_out)
{
    return kmeans_step_impl(false, ctx, data, K, centroids, inertia, n_changed, counts, centroids_out);
}

int mlhip_kmeans_step_weighted(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, const double* centroids, double* inertia,
                               uint64_t* n_changed, double* counts, double* centroids_out)
{
    return kmeans_step_impl(true, ctx, data, K, centroids, inertia, n_changed, counts, centroids_out);
}

int mlhip_kmeans_iterate(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, double* centroids, double* old_centroids,
                         uint32_t max_steps, double absolute_tolerance, uint32_t* steps_done, int* converged,
                         double* inertia, double* counts)
{
    return kmeans_iterate_impl(false, ctx, data, K, centroids, old_centroids, max_steps, absolute_tolerance, steps_done, converged, inertia,
                               counts);
}

int mlhip_kmeans_iterate_weighted(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, double* centroids, double* old_centroids,
                                  uint32_t max_steps, double absolute_tolerance, uint32_t* steps_done, int* converged,
                                  double* inertia, double* counts)
{
    return kmeans_iterate_impl(true, ctx, data, K, centroids, old_centroids, max_steps, absolute_tolerance, steps_done, converged, inertia,
                               counts);
}

int mlhip_kmeans_assign(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, const double* centroids, double* inertia,
                        uint64_t* n_changed)
{
    return kmeans_assign_impl(false, ctx, data, K, centroids, inertia, n_changed);
}

int mlhip_kmeans_assign_weighted(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, const double* centroids, double* inertia,
                                 uint64_t* n_changed)
{
    return kmeans_assign_impl(true, ctx, data, K, centroids, inertia, n_changed);
}

int mlhip_kmeans_labels(mlhip_ctx* ctx, mlhip_data* data, uint32_t* labels)
{
    return guarded([&] {
        check_call(ctx, data, 1);
        require(labels || data->rows() == 0, "null argument");
        if (ctx->group) {
            fan_out(ctx, data, [&](Shard& sh) { return mlhip_kmeans_labels(sh.ctx, sh.part, sh.rows(labels)); });
            return;
        }
        require(data->km_have_old, "no K-means assignment on the device yet");
        ctx->sync();
        download_columns(ctx, reinterpret_cast<char*>(labels), 0, data->km_labels[data->km_cur].as<char>(), 0,
                         sizeof(uint32_t) * data->n, 1);
    });
}

int mlhip_kmeans_distances(mlhip_ctx* ctx, mlhip_data* data, double* dist2)
{
    return guarded([&] {
        check_call(ctx, data, 1);
        require(dist2 || data->rows() == 0, "null argument");
        if (ctx->group) {
            fan_out(ctx, data, [&](Shard& sh) { return mlhip_kmeans_distances(sh.ctx, sh.part, sh.rows(dist2)); });
            return;
        }
        require(data->km_have_old, "no K-means assignment on the device yet");
        ctx->sync();
        download_columns(ctx, reinterpret_cast<char*>(dist2), 0, data->km_mind.as<char>(), 0, sizeof(double) * data->n, 1);
    });
}

int mlhip_kpp_draw(mlhip_ctx* ctx, mlhip_data* data, const double* centroid, int first, double u, uint64_t first_row, uint64_t* index,
                   int* certain, double* weights_out)
{
    return guarded([&] {
        check_call(ctx, data, 1);
        require(centroid && index && certain, "null argument");
        require(data->n_global >= 2, "at least two rows");
        require(u >= 0.0 && u < 1.0, "u must be a canonical uniform draw");
        if (ctx->group) {
            require(first_row == 0, "a device group holds the whole sample: first_row must be 0");
            fan_out(ctx, data, [&](Shard& sh) {
                return mlhip_kpp_draw(sh.ctx, sh.part, centroid, first, u, sh.first_row, sh.scalar(index), sh.scalar(certain), sh.rows(weights_out));
            });
            return;
        }
        const uint64_t n_global = data->n_global;
        require(first_row + data->n <= n_global, "first_row beyond the sample");
        // distances to the new centroid -> km_probe (as mlhip_min_squared_distances, label history untouched)
        const int cur = data->km_cur;
        const bool have = data->km_have_old;
        data->km_probe.reserve(sizeof(double) * data->n_pad);
        const KmRoute route = km_route(data, 1);
        const KmBlock b = km_block(data, route, 1);
        km_upload_centroids(data, 1, b, centroid);
        km_launch(data, route, 1, b, false, data->km_probe.as<double>());
        if (have) data->km_cur = cur;
        data->km_have_old = have;
        const int nb = kpp_blocks(data->n);
        data->kpp_w.reserve(sizeof(double) * data->n_pad);
        data->kpp_scr.reserve(sizeof(double) * (2 * (size_t)nb + 4));
        double* bsum = data->kpp_scr.as<double>();
        double* boff = bsum + nb;
        double* out = boff + nb;
        // |cp_i - c~_i| <= (4 N + 16384) 2^-53 (data_kernels.hip); MLHIP_KPP_DELTA_SCALE widens it (tests: forces the host path)
        static const double scale = [] { const char* e = std::getenv("MLHIP_KPP_DELTA_SCALE"); return e ? std::atof(e) : 1.0; }();
        const double delta = scale * (4.0 * (double)n_global + 16384.0) * 0x1p-53;
        double* res = data->km_host.as<double>();
        ctx->timed("kpp_draw", [&] {
            launch_kpp_update(data->kpp_w.as<double>(), data->km_probe.as<double>(), data->n, first ? 1 : 0, (double)(n_global - 1), bsum,
                              boff, out, ctx->stream);
        });
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(res, out, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
        // the ranks' sums in rank order: this rank's offset and the total are the same sequence of additions on every rank
        const int world = ctx->slot_world(), rank = ctx->slot_rank();
        const std::vector<double> sums = ctx->exchange_slots(res, 1);
        double offset = 0.0, total = 0.0;
        for (int r = 0; r < world; ++r) {
            if (r == rank) offset = total;
            total += sums[(size_t)r];
        }
        ctx->timed("kpp_draw", [&] {
            launch_kpp_find(data->kpp_w.as<double>(), data->n, bsum, boff, offset, total, u, delta, first_row, n_global, out, ctx->stream);
        });
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(res, out, sizeof(double) * 3, hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
        double lo = res[1], hi = res[2];
        const std::vector<double> cand = ctx->exchange_slots(res + 1, 2);
        for (int r = 0; r < world; ++r) {
            lo = std::min(lo, cand[2 * (size_t)r]);
            hi = std::min(hi, cand[2 * (size_t)r + 1]);
        }
        const bool ok = std::isfinite(total) && total > 0.0 && lo == hi;
        *certain = ok ? 1 : 0;
        *index = ok ? (uint64_t)lo : 0;
        if (!ok && weights_out && data->n)
            download_columns(ctx, reinterpret_cast<char*>(weights_out), 0, data->kpp_w.as<char>(), 0, sizeof(double) * data->n, 1);
    });
}

int mlhip_kpp_weights(mlhip_ctx* ctx, mlhip_data* data, double* weights_out)
{
    return guarded([&] {
        check_call(ctx, data, 1);
        require(weights_out || data->rows() == 0, "null argument");
        if (ctx->group) {
            fan_out(ctx, data, [&](Shard& sh) { return mlhip_kpp_weights(sh.ctx, sh.part, sh.rows(weights_out)); });
            return;
        }
        require(data->kpp_w.p != nullptr, "no K-means++ draw on the device yet");
        ctx->sync();
        download_columns(ctx, reinterpret_cast<char*>(weights_out), 0, data->kpp_w.as<char>(), 0, sizeof(double) * data->n, 1);
    });
}

int mlhip_kpp_draw_fixed_point(mlhip_ctx* ctx, mlhip_data* data, const double* centroid, int first, double u, uint64_t first_row,
                               uint64_t* index)
{
    return guarded([&] {
        using fixed_point::u128;
        check_call(ctx, data, 1);
        require(centroid && index, "null argument");
        require(u >= 0.0 && u < 1.0, "u must be a canonical uniform draw");
        if (ctx->group) {
            require(first_row == 0, "a device group holds the whole sample: first_row must be 0");
            fan_out(ctx, data, [&](Shard& sh) {
                return mlhip_kpp_draw_fixed_point(sh.ctx, sh.part, centroid, first, u, sh.first_row, sh.scalar(index));
            });
            return;
        }
        const uint64_t n_global = data->n_global;
        require(first_row + data->n <= n_global, "first_row beyond the sample");
        require(first || data->fp_w.p, "no fixed-point K-means++ weights on the device yet: the first draw needs first != 0");
        const int d = data->d;
        const int nb = fp_kpp_blocks(data->n);
        data->fp_w.reserve(sizeof(double) * data->n_pad);
        data->fp_scr.reserve(sizeof(uint64_t) * (4 + 3 * (size_t)nb) + sizeof(double) * (size_t)d);
        data->fp_host.reserve(sizeof(uint64_t) * 4);
        uint64_t* slots = data->fp_scr.as<uint64_t>();   // [0] largest weight's bits, [1] / [2] the rank's totals, [3] the row
        uint64_t* bsum = slots + 4;                      // 2 per block
        uint64_t* bmax = bsum + 2 * (size_t)nb;          // 1 per block
        double* cdev = reinterpret_cast<double*>(bmax + nb);
        uint64_t* res = data->fp_host.as<uint64_t>();
        HIP_CHECK(hipMemcpyAsync(cdev, centroid, sizeof(double) * (size_t)d, hipMemcpyHostToDevice, ctx->stream));
        HIP_CHECK(hipMemsetAsync(slots, 0, sizeof(uint64_t) * 3, ctx->stream));
        ctx->timed("kpp_fixed_point", [&] {
            launch_fp_kpp_update(data->xt.as<double>(), data->ldx, d, data->n, cdev, first ? 1 : 0, data->fp_w.as<double>(), bmax, slots,
                                 ctx->stream);
        });
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(res, slots, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
        // Every value that crosses the (double) all-reduce is an integer below 2^53 in its rank's slot: the sums are exact.
        const size_t W = (size_t)ctx->slot_world(), R = (size_t)ctx->slot_rank();
        // 1. the largest exponent of the whole sample and whether any weight is non-finite: [exponent + bias | flag] per rank
        double my_ex[2] = {0.0, 0.0};
        const bool bad = res[0] >= 0x7ff0000000000000ull;
        if (bad) {
            my_ex[1] = 1.0;
        } else if (res[0] != 0) {
            double m = 0.0;
            std::memcpy(&m, &res[0], sizeof m);
            int e = 0;
            std::frexp(m, &e);
            my_ex[0] = (double)(e + fixed_point::kExponentBias);
        }
        const std::vector<double> ex = ctx->exchange_slots(my_ex, 2);
        int code = 0;
        bool any_bad = false;
        for (size_t r = 0; r < W; ++r) {
            code = std::max(code, (int)ex[2 * r]);
            any_bad = any_bad || ex[2 * r + 1] != 0.0;
        }
        if (any_bad) throw InvalidArgument("FixedPointKPP: a weight (squared distance to a chosen centroid) is not finite");
        // 2. the ranks' integer totals T_r = (a + b) 2^32 + c, exchanged as a = sum of the high parts (< 2^52), b, c = the upper and
        //    lower 32 bits of the sum of the low parts (< 2^64)
        u128 total = 0, offset = 0, mine = 0;
        const int E = code - fixed_point::kExponentBias;
        if (code != 0) {
            ctx->timed("kpp_fixed_point", [&] { launch_fp_kpp_quantise(data->fp_w.as<double>(), data->n, E, bsum, slots + 1, ctx->stream); });
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipMemcpyAsync(res + 1, slots + 1, sizeof(uint64_t) * 2, hipMemcpyDeviceToHost, ctx->stream));
            ctx->sync();
            const double my_tot[3] = {(double)res[1], (double)(res[2] >> 32), (double)(res[2] & 0xffffffffull)};
            const std::vector<double> tot = ctx->exchange_slots(my_tot, 3);
            for (size_t r = 0; r < W; ++r) {
                const u128 t_r = ((u128)((uint64_t)tot[3 * r] + (uint64_t)tot[3 * r + 1]) << 32) + (uint64_t)tot[3 * r + 2];
                if (r == R) { offset = total; mine = t_r; }
                total += t_r;
            }
        }
        if (total == 0) {                               // every weight 0 (or none): a uniform row, as for the first centroid
            *index = (uint64_t)fixed_point::scaled_floor(u, n_global);
            return;
        }
        // 3. the target t = floor(u T) and the row whose cumulative sum first exceeds it, on the rank that holds it
        const u128 target = fixed_point::scaled_floor(u, total);
        double pick = 0.0;
        if (target >= offset && target - offset < mine) {
            const u128 local = target - offset;
            HIP_CHECK(hipMemsetAsync(slots + 3, 0xff, sizeof(uint64_t), ctx->stream));
            ctx->timed("kpp_fixed_point", [&] {
                launch_fp_kpp_locate(data->fp_w.as<double>(), data->n, E, bsum, (uint64_t)local, (uint64_t)(local >> 64), first_row, slots + 3,
                                     ctx->stream);
            });
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipMemcpyAsync(res + 3, slots + 3, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
            ctx->sync();
            if (res[3] == ~0ull) throw std::runtime_error("FixedPointKPP: the device scan did not find the drawn row");
            pick = (double)res[3];
        }
        if (W > 1) ctx->allreduce_host(&pick, 1);       // (a plain sum of one double: only the owner's is non-zero)
        *index = (uint64_t)pick;
    });
}

int mlhip_min_squared_distances(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, const double* centroids, double* dist2)
{
    return guarded([&] {
        check_call(ctx, data, K);
        require(centroids && (dist2 || data->rows() == 0), "null argument");
        if (ctx->group) {
            fan_out(ctx, data, [&](Shard& sh) { return mlhip_min_squared_distances(sh.ctx, sh.part, K, centroids, sh.rows(dist2)); });
            return;
        }
        // Must disturb neither the label history used for n_changed nor the per-sample distances of the last assignment
        // (mlhip_kmeans_distances): the labels go to the spare buffer, the distances to a buffer of their own.
        const int cur = data->km_cur;
        const bool have = data->km_have_old;
        data->km_probe.reserve(sizeof(double) * data->n_pad);
        run_kmeans(data, km_route(data, (int)K), (int)K, centroids, false, data->km_probe.as<double>());
        if (have) {
            // The assignment wrote labels into the *other* buffer; keep the previous labels current.
            data->km_cur = cur;
        }
        data->km_have_old = have;
        ctx->sync();
        download_columns(ctx, reinterpret_cast<char*>(dist2), 0, data->km_probe.as<char>(), 0, sizeof(double) * data->n, 1);
    });
}

int mlhip_kmeans_route(const mlhip_data* data, uint32_t K, mlhip_kmeans_route_info* out)
{
    return guarded([&] {
        require(data && out && K >= 1, "bad argument");
        if (!data->parts.empty()) data = data->parts[0];
        static_assert(kKmDirect == MLHIP_KMEANS_DIRECT && kKmMatrix == MLHIP_KMEANS_MATRIX && kKmBigDim == MLHIP_KMEANS_BIG_DIM &&
                      kKmPlain == MLHIP_KMEANS_PLAIN, "mlhip.h names the kernels by KmeansArgs::kernel");
        const KmRoute r = km_route(data, (int)K);
        out->kernel = r.kernel;
        out->pad = r.pad;
        out->resident = r.resident;
    });
}

}  // extern "C"
