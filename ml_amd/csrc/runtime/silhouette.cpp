// mlhip_silhouette: exact silhouette values of rows of a resident block (the definition and the fixed arithmetic: mlhip.h; the
// kernels: device/silhouette.hip; the closing arithmetic: device/silhouette_finish.hpp). The host validates the labels, counts them
// and sorts the rows by label (a stable counting sort: O(N), against the O(N^2 d) of the pair loop) -- every argument error is found
// before any launch. The device gathers the cluster-sorted sample-major copy of the block's columns once per call and the evaluated
// rows' coordinates (dimension-major, a lane per row), then walks the evaluated rows in blocks: the pair kernel writes one sum per
// (chunk, row), the fold kernel adds a cluster's chunks in ascending order and closes. Every buffer is the call's own, taken from the
// context's pool: nothing the handle holds is read but the block, nothing is changed.
// Device group: the evaluated rows' coordinates are gathered on their owning shards and given to every shard; every shard forms the
// sums over its own columns (the same code, the fold kernel leaving the K sums per row), the host adds them in shard order and closes.
#include "internal.hpp"

#include "device/silhouette_finish.hpp"

namespace mlhip_rt {
namespace {

/// The rows of a block by label and the chunks their sorted order is cut into.
struct Partition {
    std::vector<uint32_t> counts;           // [K]
    std::vector<uint32_t> order;            // [n]: the rows, cluster by cluster, ascending within a cluster
    std::vector<uint32_t> chunk_first, chunk_len;
    std::vector<uint32_t> cluster_chunks;   // [K + 1]
    uint32_t longest = 0;                   // chunks of the largest cluster
};

Partition partition_rows(const uint32_t* labels, uint32_t n, uint32_t K)
{
    Partition p;
    p.counts.assign(K, 0);
    for (uint32_t i = 0; i < n; ++i) ++p.counts[labels[i]];
    std::vector<uint32_t> next((size_t)K + 1, 0);
    for (uint32_t c = 0; c < K; ++c) next[c + 1] = next[c] + p.counts[c];
    p.cluster_chunks.assign((size_t)K + 1, 0);
    for (uint32_t c = 0; c < K; ++c) {
        const uint32_t chunks = (p.counts[c] + kSilhouetteChunk - 1) / kSilhouetteChunk;
        p.cluster_chunks[c + 1] = p.cluster_chunks[c] + chunks;
        p.longest = std::max(p.longest, chunks);
        for (uint32_t t = 0; t < chunks; ++t) {
            p.chunk_first.push_back(next[c] + t * kSilhouetteChunk);
            p.chunk_len.push_back(std::min(kSilhouetteChunk, p.counts[c] - t * kSilhouetteChunk));
        }
    }
    p.order.resize(n);
    for (uint32_t i = 0; i < n; ++i) p.order[next[labels[i]]++] = i;
    return p;
}

void upload_words(mlhip_ctx* ctx, DevBuf& dst, const std::vector<uint32_t>& src)
{
    dst.reserve(sizeof(uint32_t) * std::max<size_t>(src.size(), 1));
    if (!src.empty()) HIP_CHECK(hipMemcpyAsync(dst.p, src.data(), sizeof(uint32_t) * src.size(), hipMemcpyHostToDevice, ctx->stream));
}

/// What one block's call computes for m evaluated rows. Their coordinates: rows `local_index` of this block (gathered on the device),
/// or `host_rows` (dimension-major, d rows of m doubles: a device group's, collected from the owning shards). Either the closed
/// values (own: the rows' labels, counts: the cluster sizes of the whole sample; a / b / s may be null) or, with `sums` ([K][m],
/// host), the sums over this block's columns.
struct Evaluated {
    uint64_t m = 0;
    const uint32_t* local_index = nullptr;
    const double* host_rows = nullptr;
    const uint32_t* own = nullptr;
    const uint32_t* counts = nullptr;
    double *a = nullptr, *b = nullptr, *s = nullptr;
    double* sums = nullptr;
};

void block_silhouette(mlhip_data* dt, const SilhouetteRoute& route, uint32_t K, const uint32_t* labels, const Evaluated& ev)
{
    mlhip_ctx* ctx = dt->ctx;
    ctx->use();
    const uint64_t m = ev.m;
    if (!m) return;
    if (!dt->n) {                                                 // (an empty shard of a group: no columns, every sum is +0)
        if (ev.sums) std::fill(ev.sums, ev.sums + (size_t)K * m, 0.0);
        return;
    }
    require(m <= 0xffffff00ull, "too many rows to evaluate in one call");
    const int d = dt->d, pad = silhouette_pad(route.kernel, d);
    if (pad < 0) throw Unsupported("silhouette kernel not instantiated for this dimension");
    const Partition p = partition_rows(labels, dt->n, K);
    const uint32_t n_chunks = (uint32_t)p.chunk_first.size();

    DevBuf order{&dt->pool}, cols{&dt->pool}, rows{&dt->pool}, index{&dt->pool}, first{&dt->pool}, len{&dt->pool}, chunks{&dt->pool},
        counts{&dt->pool}, own{&dt->pool}, partials{&dt->pool}, out{&dt->pool};
    upload_words(ctx, order, p.order);
    upload_words(ctx, first, p.chunk_first);
    upload_words(ctx, len, p.chunk_len);
    upload_words(ctx, chunks, p.cluster_chunks);
    // the cluster-sorted sample-major copy of this block's columns
    cols.reserve(sizeof(double) * (size_t)dt->n * pad);
    launch_silhouette_gather_columns(dt->xt.as<double>(), dt->ldx, d, order.as<uint32_t>(), dt->n, cols.as<double>(), pad, ctx->stream);
    // the evaluated rows, dimension-major: ldm doubles per coordinate
    const size_t ldm = (size_t)((m + kSilhouetteRowTile - 1) / kSilhouetteRowTile * kSilhouetteRowTile);
    rows.reserve(sizeof(double) * ldm * pad);
    if (ev.host_rows) {
        HIP_CHECK(hipMemsetAsync(rows.p, 0, sizeof(double) * ldm * pad, ctx->stream));
        HIP_CHECK(hipMemcpy2DAsync(rows.p, sizeof(double) * ldm, ev.host_rows, sizeof(double) * m, sizeof(double) * m, (size_t)d,
                                   hipMemcpyHostToDevice, ctx->stream));
    } else {
        index.reserve(sizeof(uint32_t) * m);
        HIP_CHECK(hipMemcpyAsync(index.p, ev.local_index, sizeof(uint32_t) * m, hipMemcpyHostToDevice, ctx->stream));
        launch_silhouette_gather_rows(dt->xt.as<double>(), dt->ldx, d, index.as<uint32_t>(), (uint32_t)m, rows.as<double>(), ldm, pad,
                                      ctx->stream);
    }
    if (!ev.sums) {
        counts.reserve(sizeof(uint32_t) * K);
        HIP_CHECK(hipMemcpyAsync(counts.p, ev.counts, sizeof(uint32_t) * K, hipMemcpyHostToDevice, ctx->stream));
        own.reserve(sizeof(uint32_t) * m);
        HIP_CHECK(hipMemcpyAsync(own.p, ev.own, sizeof(uint32_t) * m, hipMemcpyHostToDevice, ctx->stream));
    }
    const uint32_t block = route.block_rows(n_chunks, m);         // whole row tiles
    partials.reserve(sizeof(double) * (size_t)std::max<uint32_t>(n_chunks, 1) * block);
    const size_t out_rows = ev.sums ? (size_t)K : 3;
    out.reserve(sizeof(double) * out_rows * block);
    for (uint64_t row = 0; row < m; row += block) {
        const uint32_t count = (uint32_t)std::min<uint64_t>(block, m - row);
        SilhouetteArgs a{};
        a.rows = rows.as<double>() + row; a.ldm = ldm; a.m = count;
        a.cols = cols.as<double>(); a.d = d;
        a.chunk_first = first.as<uint32_t>(); a.chunk_len = len.as<uint32_t>(); a.n_chunks = n_chunks;
        a.partials = partials.as<double>(); a.ldp = block;
        a.kernel = route.kernel; a.feed = route.feed; a.grid = route.grid;
        int grid = 0;
        ctx->timed("silhouette", [&] { grid = launch_silhouette(a, ctx->num_cus, ctx->stream); });
        if (grid < 0) throw Unsupported("silhouette kernel not instantiated for this dimension");
        SilhouetteFoldArgs f{};
        f.partials = a.partials; f.ldp = a.ldp; f.m = count; f.K = K;
        f.cluster_chunks = chunks.as<uint32_t>();
        double* o = out.as<double>();
        if (ev.sums) { f.sums = o; f.lds = block; }
        else {
            f.counts = counts.as<uint32_t>(); f.own = own.as<uint32_t>() + row;
            f.a_out = ev.a ? o : nullptr; f.b_out = ev.b ? o + block : nullptr; f.s_out = ev.s ? o + 2 * (size_t)block : nullptr;
        }
        ctx->timed("silhouette_fold", [&] { launch_silhouette_fold(f, ctx->stream); });
        HIP_CHECK(hipGetLastError());
        // (the copies wait for the stream: the chunk sums and `out` are free for the next block)
        if (ev.sums) {
            HIP_CHECK(hipMemcpy2DAsync(ev.sums + row, sizeof(double) * m, o, sizeof(double) * block, sizeof(double) * count, (size_t)K,
                                       hipMemcpyDeviceToHost, ctx->stream));
        } else {
            double* host[3] = {ev.a, ev.b, ev.s};
            for (int v = 0; v < 3; ++v)
                if (host[v])
                    HIP_CHECK(hipMemcpyAsync(host[v] + row, o + (size_t)v * block, sizeof(double) * count, hipMemcpyDeviceToHost, ctx->stream));
        }
        ctx->sync();
    }
    ctx->sync();
}

/// The coordinates of rows `local_index` of one block on the host, dimension-major: out[j * ld + r].
void gather_rows_to_host(mlhip_data* dt, const std::vector<uint32_t>& local_index, double* out, size_t ld)
{
    mlhip_ctx* ctx = dt->ctx;
    ctx->use();
    const size_t m = local_index.size();
    if (!m) return;
    DevBuf index{&dt->pool}, rows{&dt->pool};
    index.reserve(sizeof(uint32_t) * m);
    HIP_CHECK(hipMemcpyAsync(index.p, local_index.data(), sizeof(uint32_t) * m, hipMemcpyHostToDevice, ctx->stream));
    rows.reserve(sizeof(double) * m * dt->d);
    launch_silhouette_gather_rows(dt->xt.as<double>(), dt->ldx, dt->d, index.as<uint32_t>(), (uint32_t)m, rows.as<double>(), m, dt->d,
                                  ctx->stream);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpy2DAsync(out, sizeof(double) * ld, rows.p, sizeof(double) * m, sizeof(double) * m, (size_t)dt->d, hipMemcpyDeviceToHost,
                               ctx->stream));
    ctx->sync();
}

void group_silhouette(mlhip_ctx* ctx, mlhip_data* data, const SilhouetteRoute& route, uint32_t K, const uint32_t* labels,
                      const std::vector<uint64_t>& eval, const std::vector<uint32_t>& counts, double* a_out, double* b_out, double* s_out)
{
    const size_t m = eval.size(), shards = data->parts.size();
    const int d = data->d;
    // the evaluated rows' coordinates from their owning shards, in the caller's order
    std::vector<std::vector<uint32_t>> local(shards);
    std::vector<std::vector<size_t>> place(shards);
    for (size_t r = 0; r < m; ++r) {
        const size_t s = (size_t)(std::upper_bound(data->first_row.begin(), data->first_row.end(), eval[r]) - data->first_row.begin()) - 1;
        local[s].push_back((uint32_t)(eval[r] - data->first_row[s]));
        place[s].push_back(r);
    }
    std::vector<double> coords((size_t)d * m);
    std::vector<std::vector<double>> mine(shards);
    fan_out(ctx, data, [&](Shard& sh) {
        return guarded([&] {
            const size_t s = (size_t)sh.index, ms = local[s].size();
            mine[s].resize((size_t)d * ms);
            gather_rows_to_host(sh.part, local[s], mine[s].data(), ms);
        });
    });
    for (size_t s = 0; s < shards; ++s)
        for (size_t r = 0; r < place[s].size(); ++r)
            for (int j = 0; j < d; ++j) coords[(size_t)j * m + place[s][r]] = mine[s][(size_t)j * place[s].size() + r];
    // every shard's sums over its own columns
    std::vector<std::vector<double>> sums(shards);
    fan_out(ctx, data, [&](Shard& sh) {
        return guarded([&] {
            const size_t s = (size_t)sh.index;
            sums[s].resize((size_t)K * m);
            Evaluated ev;
            ev.m = m; ev.host_rows = coords.data(); ev.sums = sums[s].data();
            block_silhouette(sh.part, route, K, labels + sh.first_row, ev);
        });
    });
    // the shards' sums in ascending shard order, then the closing arithmetic
    for (size_t r = 0; r < m; ++r) {
        const uint32_t own = labels[eval[r]];
        SilhouetteFinish f;
        f.begin(own);
        for (uint32_t c = 0; c < K; ++c) {
            double sum = 0.0;
            for (size_t s = 0; s < shards; ++s) sum += sums[s][(size_t)c * m + r];
            f.add(c, (double)counts[c], sum);
        }
        double a, b, sv;
        f.end((double)counts[own], a, b, sv);
        if (a_out) a_out[r] = a;
        if (b_out) b_out[r] = b;
        if (s_out) s_out[r] = sv;
    }
}

}  // namespace
}  // namespace mlhip_rt

extern "C" {

int mlhip_silhouette(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, const uint32_t* labels, const uint64_t* rows, uint64_t n_rows,
                     double* a_out, double* b_out, double* s_out)
{
    return guarded([&] {
        check_call(ctx, data, K);
        if (!ctx->group && ctx->reduce_fn && ctx->world_size > 1)
            throw Unsupported("the silhouette needs every column of the sample on one context or device group: not available across ranks");
        const uint64_t n = data->rows();
        require(labels != nullptr || n == 0, "null labels");
        require(n <= 0xffffffffull, "too many rows");
        std::vector<uint32_t> counts(K, 0);
        for (uint64_t i = 0; i < n; ++i) {
            require(labels[i] < K, "a label is not below K");
            ++counts[labels[i]];
        }
        uint32_t non_empty = 0;
        for (uint32_t c = 0; c < K; ++c) non_empty += counts[c] > 0;
        require(non_empty >= 2, "the silhouette needs at least two non-empty clusters");
        const uint64_t m = rows ? n_rows : n;
        if (rows)
            for (uint64_t r = 0; r < m; ++r) require(rows[r] < n, "a row index is not below the number of rows");
        if (!m) return;
        const mlhip_data* shape = data->parts.empty() ? data : data->parts[0];
        const SilhouetteRoute route = silhouette_route(shape);
        if (ctx->group) {
            std::vector<uint64_t> eval(m);
            for (uint64_t r = 0; r < m; ++r) eval[r] = rows ? rows[r] : r;
            group_silhouette(ctx, data, route, K, labels, eval, counts, a_out, b_out, s_out);
            return;
        }
        std::vector<uint32_t> index(m), own(m);
        for (uint64_t r = 0; r < m; ++r) {
            index[r] = (uint32_t)(rows ? rows[r] : r);
            own[r] = labels[index[r]];
        }
        Evaluated ev;
        ev.m = m; ev.local_index = index.data(); ev.own = own.data(); ev.counts = counts.data();
        ev.a = a_out; ev.b = b_out; ev.s = s_out;
        block_silhouette(data, route, K, labels, ev);
    });
}

int mlhip_silhouette_route(const mlhip_data* data, int* tier)
{
    return guarded([&] {
        require(data && tier, "null argument");
        if (!data->parts.empty()) data = data->parts[0];        // (a group's block: every shard takes the same tier)
        *tier = silhouette_route(data).kernel;
    });
}

int mlhip_silhouette_finish(uint32_t K, const uint64_t* counts, uint32_t own_label, const double* D, double* a, double* b, double* s)
{
    return guarded([&] {
        require(counts && D, "null argument");
        require(own_label < K, "the row's label is not below K");
        require(counts[own_label] > 0, "the row's own cluster is empty");
        bool other = false;
        for (uint32_t c = 0; c < K; ++c) other = other || (c != own_label && counts[c] > 0);
        require(other, "the silhouette needs at least two non-empty clusters");
        mlhip::SilhouetteFinish f;
        f.begin(own_label);
        for (uint32_t c = 0; c < K; ++c) f.add(c, (double)counts[c], D[c]);
        double av, bv, sv;
        f.end((double)counts[own_label], av, bv, sv);
        if (a) *a = av;
        if (b) *b = bv;
        if (s) *s = sv;
    });
}

}  // extern "C"
