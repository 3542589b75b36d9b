// mlhip_em_sample / mlhip_em_sample_data: rows [first_row, first_row + n) of the sample a (seed, mixture) pair defines (the
// definition: mlhip.h; the kernels: device/em_sample.hip). The host factors the covariances (host::cholesky_lower, what a fit's
// records are built from) and normalises the prefix sums of the mixing weights; the device draws. Every row is a pure function of its
// global index, so the chunks of the host-output form and the shards of a device group leave no seam. Every buffer is the call's own,
// taken from the context's pool.
#include "internal.hpp"

namespace mlhip_rt {
namespace {

/// What the kernels read, on the host: [factors, packed row by row | means] and the label thresholds.
struct SampleModel {
    int d = 0;
    uint32_t K = 0;
    size_t l_stride = 0;                  // 0: one factor for all components (tied)
    std::vector<double> table, thresholds;
};

/// The argument errors of both sampling calls that need no device (mlhip.h); returns the covariance mode.
Covariance check_sample_arguments(const mlhip_ctx* ctx, uint32_t d, uint32_t K, int covariance_type, const double* mixing, const double* means,
                            const double* covs, uint64_t first_row, uint64_t n)
{
    require(ctx && mixing && means && covs, "null argument");
    require(K >= 1, "At least one component required");
    require(d >= 1 && d <= (uint32_t)kGenericMaxDim, "the dimension must be 1 .. 4096");
    const Covariance mode = covariance_from_abi(covariance_type);
    double total = 0;
    for (uint32_t k = 0; k < K; ++k) {
        require(std::isfinite(mixing[k]) && mixing[k] >= 0, "mixing weights must be finite and >= 0");
        total += mixing[k];
    }
    require(total > 0 && std::isfinite(total), "the mixing weights' total must be positive and finite");
    for (size_t i = 0; i < (size_t)K * d; ++i) require(std::isfinite(means[i]), "means must be finite");
    require(first_row + n >= first_row, "first_row + n must fit 64 bits");
    return mode;
}

/// Packs the lower triangle of the column-major factor L row by row; DomainError unless it is a Cholesky factor (finite, positive
/// diagonal): the matrix behind it was not positive definite.
void pack_factor(int d, const double* L, double* packed)
{
    for (int j = 0; j < d; ++j) {
        for (int c = 0; c <= j; ++c) {
            const double v = L[(size_t)c * d + j];
            if (!std::isfinite(v) || (c == j && !(v > 0))) throw DomainError("covariance matrix is not positive definite");
            packed[(size_t)j * (j + 1) / 2 + c] = v;
        }
    }
}

SampleModel build_model(uint32_t d_, uint32_t K, Covariance mode, const double* mixing, const double* means, const double* covs)
{
    SampleModel m;
    const int d = (int)d_;
    m.d = d;
    m.K = K;
    const size_t tl = (size_t)d * (d + 1) / 2, dd = (size_t)d * d;
    const size_t factors = mode == Covariance::Tied ? 1 : K;
    m.l_stride = mode == Covariance::Tied ? 0 : tl;
    m.table.assign(factors * tl + (size_t)K * d, 0.0);
    if (mode == Covariance::Diagonal) {
        // L = sqrt(variance): the factor host::cholesky_lower gives for the same variances as a diagonal matrix, bit for bit
        for (uint32_t k = 0; k < K; ++k)
            for (int j = 0; j < d; ++j) {
                const double v = covs[(size_t)k * d + j];
                if (!(v > 0) || !std::isfinite(v)) throw DomainError("covariance matrix is not positive definite");
                m.table[k * tl + (size_t)j * (j + 1) / 2 + j] = std::sqrt(v);
            }
    } else {
        std::vector<double> L(dd);
        for (size_t k = 0; k < factors; ++k) {
            host::cholesky_lower(d, covs + k * dd, L.data());
            pack_factor(d, L.data(), m.table.data() + k * tl);
        }
    }
    std::copy(means, means + (size_t)K * d, m.table.begin() + factors * tl);
    // t_k = s_k / s_{K-1}, s the sequential prefix sums: ascending, t_{K-1} = 1 (never compared: the last component takes the rest)
    m.thresholds.resize(K);
    double s = 0;
    for (uint32_t k = 0; k < K; ++k) m.thresholds[k] = (s += mixing[k]);
    for (uint32_t k = 0; k < K; ++k) m.thresholds[k] /= s;
    return m;
}

/// A model on one context's device, and the launches against it.
struct DeviceModel {
    mlhip_ctx* ctx;
    BufferPool* pool;
    DevBuf table{&pool}, thresholds{&pool};
    SampleArgs args{};

    DeviceModel(mlhip_ctx* c, const SampleModel& m, uint64_t seed) : ctx(c), pool(&c->pool)
    {
        ctx->use();
        table.reserve(sizeof(double) * m.table.size());
        thresholds.reserve(sizeof(double) * m.thresholds.size());
        HIP_CHECK(hipMemcpyAsync(table.p, m.table.data(), sizeof(double) * m.table.size(), hipMemcpyHostToDevice, ctx->stream));
        HIP_CHECK(hipMemcpyAsync(thresholds.p, m.thresholds.data(), sizeof(double) * m.thresholds.size(), hipMemcpyHostToDevice, ctx->stream));
        ctx->sync();                                           // (the host vectors are the caller's to drop)
        args.d = m.d; args.K = m.K;
        args.table = table.as<double>(); args.table_doubles = m.table.size(); args.l_stride = m.l_stride;
        args.thresholds = thresholds.as<double>();
        args.seed = seed;
        args.kernel = sample_route(m.d, m.K).kernel;
    }
    DeviceModel(const DeviceModel&) = delete;
    DeviceModel& operator=(const DeviceModel&) = delete;

    /// Rows [first_row, first_row + n) into x (n x d, contiguous) and labels, device memory, either null; nothing waits.
    void generate(uint64_t first_row, uint64_t n, double* x, uint32_t* labels)
    {
        SampleArgs a = args;
        a.first_row = first_row; a.n = n; a.x = x; a.labels = labels;
        int grid = 0;
        ctx->timed("em_sample", [&] { grid = launch_em_sample(a, ctx->num_cus, ctx->stream); });
        if (grid < 0) throw Unsupported("sampling kernel not instantiated for this shape");
        HIP_CHECK(hipGetLastError());
    }
};

void em_sample_host(mlhip_ctx* ctx, const SampleModel& m, uint64_t seed, uint64_t first_row, uint64_t n, double* x, int64_t ld,
                    uint32_t* labels)
{
    DeviceModel dev(ctx, m, seed);
    const size_t d = (size_t)m.d;
    const uint64_t chunk = std::min<uint64_t>(sample_route(m.d, m.K).chunk_rows, n);
    DevBuf xb{&dev.pool}, lb{&dev.pool};
    if (x) xb.reserve(sizeof(double) * d * chunk);
    if (labels) lb.reserve(sizeof(uint32_t) * chunk);
    std::vector<double> packed;                                 // ld > d: a chunk comes down contiguous and is spread by the CPU
    if (x && ld != (int64_t)d) packed.resize(d * chunk);
    for (uint64_t row = 0; row < n; row += chunk) {
        const uint64_t rows = std::min(chunk, n - row);
        dev.generate(first_row + row, rows, xb.as<double>(), lb.as<uint32_t>());
        if (labels) download_columns(ctx, reinterpret_cast<char*>(labels + row), 0, lb.as<char>(), 0, sizeof(uint32_t) * rows, 1);
        if (!x) continue;
        double* dst = x + (int64_t)row * ld;
        download_columns(ctx, reinterpret_cast<char*>(packed.empty() ? dst : packed.data()), 0, xb.as<char>(), 0, sizeof(double) * d * rows, 1);
        if (!packed.empty())
            for (uint64_t i = 0; i < rows; ++i) std::memcpy(dst + (int64_t)i * ld, packed.data() + i * d, sizeof(double) * d);
    }
}

/// The handle form on one context: the block is generated sample-major into a pool buffer and becomes a handle the way a block
/// already in device memory does (upload_common, on_device).
mlhip_data* em_sample_block(mlhip_ctx* ctx, const SampleModel& m, uint64_t seed, uint64_t first_row, uint64_t n, uint32_t* labels)
{
    DeviceModel dev(ctx, m, seed);
    DevBuf xb{&dev.pool}, lb{&dev.pool};
    if (n) {
        xb.reserve(sizeof(double) * (size_t)m.d * n);
        if (labels) lb.reserve(sizeof(uint32_t) * n);
        dev.generate(first_row, n, xb.as<double>(), lb.as<uint32_t>());
        if (labels) download_columns(ctx, reinterpret_cast<char*>(labels), 0, lb.as<char>(), 0, sizeof(uint32_t) * n, 1);
    }
    return upload_common(ctx, n ? xb.as<double>() : nullptr, true, (uint32_t)m.d, n, m.d);   // (waits for the stream: the buffer may go)
}

constexpr uint64_t kMaxBlockRows = 0xffffff00ull;               // upload_common's bound on one rank's rows

}  // namespace
}  // namespace mlhip_rt

extern "C" {

int mlhip_em_sample(mlhip_ctx* ctx, uint32_t d, uint32_t K, int covariance_type, const double* mixing, const double* means,
                    const double* covariances, uint64_t seed, uint64_t first_row, uint64_t n, double* x, int64_t ld, uint32_t* labels)
{
    return guarded([&] {
        const Covariance mode = check_sample_arguments(ctx, d, K, covariance_type, mixing, means, covariances, first_row, n);
        require(x || labels, "null argument: neither x nor labels");
        require(!x || ld >= (int64_t)d, "ld must be >= d");
        if (!n) return;
        const SampleModel m = build_model(d, K, mode, mixing, means, covariances);
        if (ctx->group) {
            // (every shard draws its rows of the balanced split on its own GPU: no collective, nothing to put together but the rows'
            // places in the caller's arrays)
            int shards = 1;
            check_status(mlhip_ctx_shards(ctx, &shards));
            fan_out_rows(ctx, balanced_rows(n, shards), nullptr, [&](Shard& sh) {
                return guarded([&] {
                    if (sh.n_rows) em_sample_host(sh.ctx, m, seed, first_row + sh.first_row, sh.n_rows, sh.rows(x, ld), ld, sh.rows(labels));
                });
            });
            return;
        }
        em_sample_host(ctx, m, seed, first_row, n, x, ld, labels);
    });
}

int mlhip_em_sample_data(mlhip_ctx* ctx, uint32_t d, uint32_t K, int covariance_type, const double* mixing, const double* means,
                         const double* covariances, uint64_t seed, uint64_t first_row, uint64_t n, uint32_t* labels, mlhip_data** out)
{
    return guarded([&] {
        require(out, "null argument");
        const Covariance mode = check_sample_arguments(ctx, d, K, covariance_type, mixing, means, covariances, first_row, n);
        int shards = 1;
        if (ctx->group) check_status(mlhip_ctx_shards(ctx, &shards));
        require((n + (uint64_t)shards - 1) / (uint64_t)shards < kMaxBlockRows, "shard too large (n must fit 32 bits, like the reference's unsigned int)");
        const SampleModel m = build_model(d, K, mode, mixing, means, covariances);
        if (ctx->group) {
            *out = grp::upload_parts(ctx, d, n, [&](mlhip_ctx* shard, uint64_t lo, uint64_t rows) {
                return em_sample_block(shard, m, seed, first_row + lo, rows, labels ? labels + lo : nullptr);
            });
            return;
        }
        *out = em_sample_block(ctx, m, seed, first_row, n, labels);
    });
}

int mlhip_cholesky_lower(uint32_t d, const double* covariance, double* lower)
{
    return guarded([&] {
        require(d >= 1 && d <= (uint32_t)kGenericMaxDim && covariance && lower, "bad argument");
        host::cholesky_lower((int)d, covariance, lower);
        for (uint32_t j = 0; j < d; ++j)
            for (uint32_t i = j; i < d; ++i) {
                const double v = lower[(size_t)j * d + i];
                if (!std::isfinite(v) || (i == j && !(v > 0))) throw DomainError("covariance matrix is not positive definite");
            }
    });
}

int mlhip_em_sample_route(uint32_t d, uint32_t K, int* kernel)
{
    return guarded([&] {
        require(kernel && K >= 1 && d >= 1 && d <= (uint32_t)kGenericMaxDim, "bad argument");
        static_assert(kSampleLdsTable == MLHIP_SAMPLE_LDS_TABLE && kSampleGlobalTable == MLHIP_SAMPLE_GLOBAL_TABLE &&
                          kSamplePlain == MLHIP_SAMPLE_PLAIN,
                      "mlhip.h names the kernels by SampleKernel");
        *kernel = sample_route((int)d, K).kernel;
    });
}

}  // extern "C"
