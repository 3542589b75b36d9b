// Internal interface between the runtime (runtime.cpp) and the gfx950 kernels (*.hip).
// Everything here is launched on the caller's hipStream_t; no function synchronises.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "layout.hpp"

namespace mlhip {

// ---- data movement --------------------------------------------------------------------------------
/// dst[j*ldd + i0 + i] = src[i*lds + j] for i < n, j < d (sample-major -> dimension-major).
void launch_transpose_to_dim_major(const double* src, int64_t lds, int d, uint64_t n, double* dst, size_t ldd,
                                   uint64_t i0, hipStream_t stream);
/// sums[j] = sum_i xt[j*ldx + i] (deterministic two-stage reduction); scratch >= d * 1024 doubles.
/// maxabs[j] = max_i |xt[j*ldx + i]|; scratch >= d * 1024 doubles.
void launch_column_maxabs(const double* xt, size_t ldx, int d, uint64_t n, double* scratch, double* maxabs, hipStream_t stream);
void launch_column_sums(const double* xt, size_t ldx, int d, uint64_t n, double* scratch, double* sums, hipStream_t stream);

/// RandomPartition::init's running means on the resident block (data_kernels.hip): means[k*d + j] and sizes[k] are continued
/// over the rows order[offsets[k] .. offsets[k+1]) of cluster k, in that order. All pointers device memory.
void launch_random_partition(const double* xt, size_t ldx, int d, int K, const uint32_t* order, const uint32_t* offsets,
                             double* means, double* sizes, hipStream_t stream);

/// One K-means++ draw on the device (data_kernels.hip), in two launches around the ranks' exchange of their weight sums:
/// update: weights = first ? dist : min(weights, dist) over this rank's n rows, block sums / offsets, out[0] = this rank's sum,
///         out[1] = out[2] = default_index (the last row of the whole sample);
/// find:   the bounds [lo, hi] (global row indices, out[1] / out[2], as doubles) of the row std::discrete_distribution would return
///         for the canonical uniform u, given the sum of the ranks before this one (offset) and of all ranks (total).
/// bsum / boff: kpp_blocks(n) doubles of scratch each.
int kpp_blocks(uint32_t n);
void launch_kpp_update(double* weights, const double* dist, uint32_t n, int first, double default_index, double* bsum, double* boff,
                       double* out, hipStream_t stream);
void launch_kpp_find(const double* weights, uint32_t n, const double* bsum, const double* boff, double offset, double total, double u,
                     double delta, uint64_t row0, uint64_t n_global, double* out, hipStream_t stream);

/// One fixed-point K-means++ draw (FixedPointKPP) on the device (kpp_fixed_point.hip); fp_kpp_blocks(n) workgroups of 4096 rows.
/// update:   w = first ? |x_i - centroid|^2 : min(w, |x_i - centroid|^2) over the n rows of xt (centroid: d doubles of device memory);
///           bmax[b] = the bits of block b's largest new weight, *wmax = the largest of them;
/// quantise: q_i = floor(w_i 2^(52 - E)); bsum[2b], bsum[2b + 1] = the sums of q_i >> 32 and q_i mod 2^32 over block b, total[0] /
///           total[1] = their sums over the blocks;
/// (n = 0: nothing is launched, the outputs keep what the caller put there)
/// locate:   out[0] = row0 + the smallest row i with q_0 + ... + q_i > target (target = target_hi 2^64 + target_lo, below the sum
///           of all q_i; one workgroup). out[0] is left untouched when the target lies beyond the sum.
int fp_kpp_blocks(uint32_t n);
void launch_fp_kpp_update(const double* xt, size_t ldx, int d, uint32_t n, const double* centroid, int first, double* w, uint64_t* bmax,
                          uint64_t* wmax, hipStream_t stream);
void launch_fp_kpp_quantise(const double* w, uint32_t n, int E, uint64_t* bsum, uint64_t* total, hipStream_t stream);
void launch_fp_kpp_locate(const double* w, uint32_t n, int E, const uint64_t* bsum, uint64_t target_lo, uint64_t target_hi, uint64_t row0,
                          uint64_t* out, hipStream_t stream);

/// Fixed-order sum of the n <= kGroupMaxShards buffers slots.p[0..n) (`count` doubles each) into out: the all-reduce of a device
/// group whose shards share a process (runtime/group.cpp).
constexpr int kGroupMaxShards = 64;
struct GroupSumSlots { const double* p[kGroupMaxShards]; };
void launch_group_sum(const GroupSumSlots& slots, int n, double* out, size_t count, hipStream_t stream);

// ---- silhouette (silhouette.hip) -------------------------------------------------------------------
/// Columns per chunk of a cluster's run of sorted columns: with the sorted order it fixes the order of every sum (mlhip.h).
constexpr uint32_t kSilhouetteChunk = 256;
/// Evaluated rows one workgroup holds (one per lane); the runtime sizes its row blocks in whole tiles.
constexpr uint32_t kSilhouetteRowTile = 256;
constexpr int kSilhouetteMaxRegisters = 32;
enum SilhouetteKernel : int {
    kSilhouetteRegisters = 0,                  // d <= 32: lane = evaluated row, its coordinates in registers
    kSilhouettePlain = 1,                      // up to d = 4096: a lane walks its coordinates from memory (same operations, same bits)
};
enum SilhouetteFeed : int {
    kSilhouetteScalarFeed = 0,                 // columns as wave-uniform scalar loads from the sorted copy
    kSilhouetteLdsFeed = 1,                    // the chunk staged in LDS, read as same-address broadcasts (register tier only)
};
/// kSilhouetteRegisters for d <= 32, else kSilhouettePlain.
int silhouette_tier(int d);
/// Doubles per column of the sorted copy: the register tier's padding of d (2, 4, 8, 16, 32; zeros beyond d), d itself on the plain tier.
int silhouette_pad(int kernel, int d);
/// cols[c * stride + j] = xt[j * ldx + order[c]] for c < n, j < d, and +0.0 for d <= j < stride.
void launch_silhouette_gather_columns(const double* xt, size_t ldx, int d, const uint32_t* order, uint32_t n, double* cols, int stride,
                                      hipStream_t stream);
/// rows[j * ldm + r] = xt[j * ldx + index[r]] for r < m, j < d, and +0.0 for d <= j < pad.
void launch_silhouette_gather_rows(const double* xt, size_t ldx, int d, const uint32_t* index, uint32_t m, double* rows, size_t ldm, int pad,
                                   hipStream_t stream);
struct SilhouetteArgs {
    const double* rows; size_t ldm; uint32_t m;              // evaluated rows, dimension-major, silhouette_pad(kernel, d) rows of ldm
    const double* cols; int d;                               // the sorted copy, silhouette_pad(kernel, d) doubles per column
    const uint32_t* chunk_first; const uint32_t* chunk_len; uint32_t n_chunks;   // device: first sorted column and length of every chunk
    double* partials; size_t ldp;                            // out: partials[t * ldp + r], chunk t's sum for row r
    int kernel, feed;
    int grid;                                                // > 0: workgroups (a test's override; no bit depends on it)
};
/// Returns the workgroups launched (0: nothing to do), < 0: not built for the shape.
int launch_silhouette(const SilhouetteArgs& a, int num_cus, hipStream_t stream);
/// The chunk sums of every cluster added in ascending order (cluster c owns chunks cluster_chunks[c] .. cluster_chunks[c + 1]), then
/// either the sums themselves, sums[c * lds + r] (a device group's shard), or the closing arithmetic of silhouette_finish.hpp with the
/// cluster sizes `counts` and the rows' own labels: a_out / b_out / s_out, each may be null.
struct SilhouetteFoldArgs {
    const double* partials; size_t ldp; uint32_t m; uint32_t K;
    const uint32_t* cluster_chunks; const uint32_t* counts; const uint32_t* own;
    double* a_out; double* b_out; double* s_out;
    double* sums; size_t lds;
};
void launch_silhouette_fold(const SilhouetteFoldArgs& a, hipStream_t stream);

// ---- EM ----------------------------------------------------------------------------------------------
struct EstepArgs {
    const double* xt; size_t ldx; uint32_t n; int D;      // D = padded dimension
    const double* params; int K;                            // K records of estep_param_stride(D)
    double* lw; size_t ldr;                                 // out: unnormalised log-responsibilities [K][ldr]
    double* lse;                                            // out: log sum_k exp(lw) per sample
    double* ll_partials; int n_ll_partials;                 // out: per-block sums of lse (grid size)
    // em_estep_mfma4 only:
    const double* shift;                                    // device, D doubles (zero-padded): the fold's centre
    int fold;                                               // records carry -W (mu - shift) instead of the mean (d <= 32)
    int with_lse;                                           // 0: write lw only (the statistics kernel normalises)
    int row_major;                                          // fold && !with_lse: the blocks in row-quad-major order where that form is built (estep_mfma4_row_major_built)
    int num_cus;                                            // compute units of the context's device (0: ask the current device)
    double* scratch; size_t scratch_doubles;                // a block free for the launch (the statistics partials): the big tier's q parts
    int plain;                                              // d > kMaxDim: 1 = the plain tier even where big_dim.hip applies
    uint32_t* labels;                                       // em_estep_mfma4's SCORE form only (launch_em_score_mfma4): out, may be null
};
/// Returns the grid size used (= number of ll partials written), or <0 if D is not instantiated.
int launch_em_estep(const EstepArgs& a, hipStream_t stream);
/// d > kMaxDim (generic_dim.hip): the same passes in a plain form, any dimension.
int launch_em_estep_generic(const EstepArgs& a, hipStream_t stream);
/// 4x4-block triangular variant (em_estep_mfma4.hip); params use the estep_mfma4_param_stride(D) record layout.
int launch_em_estep_mfma4(const EstepArgs& a, int num_cus, hipStream_t stream);

/// Screened E-step (em_estep_screen.hip; FOLD records, lw only, 12 <= D <= 32, K <= 64): rewrites the block lw that an earlier pass
/// left, evaluating only the pairs the bound constants cannot prove zero. exact: padded_samples(n) words, bit k of word i = "lw[k][i]
/// is an evaluated value" (read unless all_exact, always rewritten). consts: 4 doubles per component (em_screen_bound.hpp).
struct ScreenArgs {
    const double* xt; size_t ldx; uint32_t n; int D;
    const double* params; int K;                            // the NEW records, estep_mfma4_param_stride(D) each
    const double* shift;                                    // device, D doubles (zero-padded)
    const double* consts;
    double* lw; size_t ldr;
    unsigned long long* exact; int all_exact;
    unsigned long long* cand_count;                         // += candidates among the n rows (may be null)
    unsigned long long* profile;                            // diagnostic: kScreenStamps clock stamps per workgroup (null: the plain kernel)
};
/// Stamp slots of a workgroup: 0 tile start, 1 end of stage (the maxima combined), 2 end of buckets, 3 + 2j / 4 + 2j wave 0's j-th record copied /
/// evaluated (j < kScreenStampRounds: wave 0's components at K = 64 in the four-wave form), then the two below.
constexpr int kScreenStampRounds = 16;
constexpr int kScreenStampLoopEnd = 3 + 2 * kScreenStampRounds;        // wave 0 out of the component loop
constexpr int kScreenStampTileEnd = kScreenStampLoopEnd + 1;           // behind the tile's last barrier
constexpr int kScreenStamps = 40;
bool em_estep_screen_supported(int D, int K);
/// Samples per tile of the form instantiated for D (128 or 256; < 0: not instantiated). A workgroup has tile / 32 waves, 256 / tile
/// workgroups share a CU, and the grid is at most that many per CU.
int em_estep_screen_tile(int D);
/// The shapes at which the runtime takes the screened pass by itself (measured faster than the dense kernel there).
bool em_estep_screen_preferred(int D, int K);
/// Returns the grid, or < 0 where the kernel is not instantiated.
int launch_em_estep_screen(const ScreenArgs& a, int num_cus, hipStream_t stream);
/// The constants of K components from the records the block belongs to and the new ones (both in FOLD form); *no_info += components
/// whose bound carries no information.
void launch_em_screen_constants(const double* rec_old, const double* rec_new, int K, int d, int D, double* consts,
                                unsigned* no_info, hipStream_t stream);

/// Scoring pass (em_score.hip; em_estep_mfma4.hip's SCORE form): per sample the log-sum-exp of the K log-densities-times-weights and
/// the label argmax_k lw (first maximum wins; 0xffffffff where lse is NaN) -- no N x K block. Both outputs hold padded_samples(n)
/// entries; either may be null.
struct ScoreArgs {
    const double* xt; size_t ldx; uint32_t n; int D;      // D = padded dimension
    const double* params; int K;                            // K records: estep_param_stride(D) (scalar-fed) / estep_mfma4_param_stride(D)
    double* lse; uint32_t* labels;                          // out
};
/// d <= 32, the scalar-fed tier. Returns the grid, or < 0 if D is not instantiated.
int launch_em_score(const ScoreArgs& a, hipStream_t stream);
/// 12 <= d <= 128 on the matrix cores: em_estep_mfma4_kernel's SCORE form, exact (never FOLD). In a code object of its own.
int launch_em_score_mfma4(const ScoreArgs& a, int num_cus, hipStream_t stream);
/// Label and lse of n rows from the lw [K][ldr] / lse an E-step kernel wrote (the composed scoring route's second kernel).
void launch_em_score_finish(const double* lw, size_t ldr, const double* lse, uint32_t n, int K, double* lse_out, uint32_t* labels_out,
                            hipStream_t stream);

/// Sampling pass (em_sample.hip): rows [first_row, first_row + n) of the sample that (seed, mixture) define, sample-major and
/// contiguous (row stride d) into x, their components into labels; either may be null. Every row is a pure function of its global
/// index, so the outputs do not depend on how a sample is cut into launches.
enum SampleKernel : int {
    kSampleLdsTable = 0,                       // d <= 64, the factors and means in LDS beside the staging tile
    kSampleGlobalTable = 1,                    // d <= 64, read per lane from global memory
    kSamplePlain = 2,                          // 64 < d <= 4096: normals to the output row, product in place there
};
struct SampleArgs {
    int d; uint32_t K;
    const double* table; size_t table_doubles;               // [factors: packed lower triangles, l_stride apart | means (K x d)]
    size_t l_stride;                                         // d (d+1)/2, or 0 when all components share one factor (tied)
    const double* thresholds;                                // K doubles: the normalised prefix sums of the mixing weights
    uint64_t seed, first_row, n;
    double* x; uint32_t* labels;                             // out: n x d (16-byte aligned), n
    int kernel;                                              // SampleKernel (em_sample_route, or the other table form of the same tier)
};
/// The kernel for a full model of K components in d dimensions: LDS table where K (d (d+1)/2 + d) doubles fit into the 64 KiB a
/// workgroup takes beside the staging tile (4 / 2 / 1 waves of 64 x (d | 1) doubles at d <= 16 / 32 / 64) and the K thresholds.
int em_sample_route(int d, uint32_t K);
/// Returns the grid (0: nothing to do), or < 0 where the kernel asked for is not built for the shape.
int launch_em_sample(const SampleArgs& a, int num_cus, hipStream_t stream);

/// Conditioning pass (em_condition.hip): E[x_M | x_O] of the n rows of a chunk from the log-responsibilities lw [K][ldr] / lse an
/// E-step kernel wrote for the marginal mixture over the observed coordinates (with_lse = 1, fold = 0) -- the composed route's
/// finishing kernel where em_score_finish_kernel stands in scoring. Row i's output is a pure function of row i and the parameters.
enum ConditionKernel : int {
    kConditionRegisters = 0,                   // dO <= 32 and dM <= 32: lane = row, x_O and the accumulators in registers
    kConditionPlain = 1,                       // up to d = 4096: table and accumulators in global memory
};
/// What every conditioning kernel reads of a chunk: the rows, the log-responsibilities an E-step kernel wrote for them and the table.
struct ConditionChunk {
    const double* xt; size_t ldx; uint32_t n;                // the observed coordinates, feature-major: row c = coordinate observed[c]
    int dO, dM, K;
    const double* lw; size_t ldr; const double* lse;         // K x ldr log-responsibilities and their log-sum-exp
    const double* table;                                     // K records of the kernel's *_record_doubles(kernel, dO, dM)
    int kernel;                                              // ConditionKernel
};
struct ConditionArgs : ConditionChunk {
    double* out;                                             // n x dM, row-major and contiguous (16-byte aligned)
    int skip;                                                // 1: a wave passes over a component none of its rows has a share in
};
/// kConditionRegisters where both paddings exist, else kConditionPlain.
int em_condition_route(int dO, int dM);
/// The paddings the record of `kernel` is laid out for: [mu_O (PO) | mu_M (PM) | A^T (PO x PM: row c = observed coordinate c)], +0.0
/// beyond dO / dM except the rows c >= dO of A^T, which hold -0.0 (an identity in the kernel's fma chain). The register tier pads to 4 / 8 / 16 / 32 each, the plain tier not at all.
int condition_pad(int kernel, int n);
inline size_t condition_record_doubles(int kernel, int dO, int dM)
{
    const size_t po = (size_t)condition_pad(kernel, dO), pm = (size_t)condition_pad(kernel, dM);
    return po + pm + po * pm;
}
/// Returns the grid (0: nothing to do), or < 0 where the kernel asked for is not built for the shape.
int launch_em_condition(const ConditionArgs& a, int num_cus, hipStream_t stream);

/// Imputation with a pattern per row (em_impute_records.hip, em_impute.hip; the definition: mlhip.h, mlhip_em_impute), d <= 32.
/// A pattern's K records stand one after the other from `rec_base` (in doubles) of the record buffer, each
///   [mu_O (PO) | mu_M (PM) | A^T (PO x PM: row c = observed coordinate c) | W (PO (PO + 1) / 2: the packed lower triangle of L^-1,
///    row j from j (j + 1) / 2) | coef]
/// in the paddings of condition_pad(kConditionRegisters, .): +0.0, except the rows c >= dO of A^T: -0.0 (a padded coordinate has
/// x_c = mu_c = +0.0, so its term of the map chain is fma(-0.0, +0.0, t) = t and its row of W adds fma(+0.0, +0.0, q) = q: identities
/// bit for bit).
constexpr int kImputeMaxDim = 32;
struct ImputePattern {
    uint32_t dO, dM, po, pm, rec_base;                           // po / pm: condition_pad(kConditionRegisters, dO / dM)
    uint32_t observed[kImputeMaxDim];                            // ascending; beyond dO: 0 (never read)
    uint32_t missing[kImputeMaxDim];                             // ascending; beyond dM: 0 (never read)
};
inline size_t impute_record_doubles(int po, int pm) { return (size_t)po + pm + (size_t)po * pm + (size_t)po * (po + 1) / 2 + 1; }
/// The records of `n_patterns` patterns x K components, one wave each: Sigma_k,OO gathered by the pattern's coordinates into LDS and
/// factored there (L L^T, the column-by-column form), W = L^-1, coef_k = log_mixing[k] - sum_j log L_jj, A_k = Sigma_k,MO Sigma_k,OO^-1
/// by a forward and a backward substitution per missing coordinate. A pivot that is not > 0 or not finite is an ordinary value here:
/// the wave stores 1 to *flag (a plain vector store; the host zeroes it before the launch), takes 1.0 for the pivot and goes on.
struct ImputeRecordsArgs {
    int d, K;
    const double* means;                                         // K x d
    const double* covs;                                          // K x d x d, full
    const double* log_mixing;                                    // K
    const ImputePattern* patterns; uint32_t n_patterns;
    double* records;                                             // out
    uint32_t* flag;                                              // out
};
void launch_em_impute_records(const ImputeRecordsArgs& a, hipStream_t stream);
/// One tile of the evaluation kernel: rows [first, first + rows) of the chunk's row block, all of pattern `pattern` (an index into
/// ImputeArgs::patterns), rows <= 64; their rows x dM results go to y + out_base (out_base even: 16-byte aligned), row-major.
struct ImputeTile {
    uint32_t pattern, first, rows, out_base;
};
/// The evaluation kernel on the tiles of ONE padding class (po, pm): lane = row, per row the steps 1 - 6 of the definition with the
/// record of the tile's pattern. Returns the grid (0: nothing to do), < 0 where the class is not instantiated. `grid_cap` > 0: at
/// most that many workgroups (the tests' way to make a wave take a second tile on a small block).
struct ImputeArgs {
    const double* x; int d;                                      // the chunk's rows, row-major and contiguous, NaNs and all
    int K;
    const ImputePattern* patterns;
    const double* records;
    const ImputeTile* tiles; uint32_t n_tiles;
    int po, pm;
    double* y;                                                   // out: per tile rows x dM
    double* lse;                                                 // out: per row of the chunk, the log-sum-exp of step 4
    double* resp; size_t ldr;                                    // out (may be null): resp[k * ldr + row]
    int skip;                                                    // 1: a wave passes over a component none of its rows has a share in
    int grid_cap;
};
int launch_em_impute(const ImputeArgs& a, int num_cus, hipStream_t stream);

/// Conditional draws (em_condition_sample.hip): x_M | x_O of the n rows of a chunk for the draws first_draw .. first_draw + n_draws - 1,
/// from the same lw / lse as the conditioning pass. Row (i, q) is a pure function of (seed, first_row + i, q), the row and the
/// parameters. The tiers and paddings are ConditionKernel's and condition_pad's; the record is the conditioning pass's with the
/// factor behind it: [mu_O | mu_M | A^T | G, the lower triangle packed row by row: (j, c) at j (j+1)/2 + c, for the PADDED dM].
struct ConditionSampleArgs : ConditionChunk {
    uint64_t seed, first_row;                                // first_row: the global index of the chunk's row 0
    uint32_t first_draw, n_draws;                            // (first_draw + n_draws <= 2^32 - 1: draw q is generator stream 1 + q)
    double* out; size_t ldq;                                 // n_draws blocks of n x dM (row-major), ldq doubles apart: even, 16-byte aligned
    uint32_t* labels;                                        // n_draws x n, or null
};
constexpr uint32_t kConditionSampleNoLabel = 0xFFFFFFFFu;    // the label of a row whose shares do not sum to a number
inline size_t condition_sample_record_doubles(int kernel, int dO, int dM)
{
    const size_t pm = (size_t)condition_pad(kernel, dM);
    return condition_record_doubles(kernel, dO, dM) + pm * (pm + 1) / 2;
}
/// Returns the grid (0: nothing to do), or < 0 where the kernel asked for is not built for the shape.
int launch_em_condition_sample(const ConditionSampleArgs& a, int num_cus, hipStream_t stream);

/// Conditional variance (em_condition_variance.hip): Var[x_M | x_O] of the n rows of a chunk from the same lw / lse as the conditioning
/// pass, whose steps it runs first. Row i's output is a pure function of row i and the parameters. The tiers and paddings are
/// ConditionKernel's and condition_pad's; the record is the conditioning pass's with c behind it: diag(C_k) (the padded dM doubles),
/// or with `full` the lower triangle of C_k packed row by row, (a, b) at a (a + 1) / 2 + b, for the PADDED dM.
struct ConditionVarianceArgs : ConditionChunk {
    double* out;                                             // n x dM, or n x dM x dM with `full`: row-major and contiguous (16-byte aligned)
    double* means;                                           // n x dM (16-byte aligned): E[x_M | x_O], the conditioning pass's bits; or null
    double* work;                                            // kConditionPlain: n x 2 dM doubles of the call's own; else unused
    int full;
    int skip;                                                // as ConditionArgs'
};
/// kConditionRegisters where the register tier is built for (dO, dM) in this form -- the diagonal form to 32 x 32, the full form to
/// the dM its accumulators fit the register file at (em_condition_variance.hip states the bound) --, else kConditionPlain.
int em_condition_variance_route(int dO, int dM, int full);
inline size_t condition_variance_record_doubles(int kernel, int dO, int dM, int full)
{
    const size_t pm = (size_t)condition_pad(kernel, dM);
    return condition_record_doubles(kernel, dO, dM) + (full ? pm * (pm + 1) / 2 : pm);
}
/// Returns the grid (0: nothing to do), or < 0 where the kernel asked for is not built for the shape.
int launch_em_condition_variance(const ConditionVarianceArgs& a, int num_cus, hipStream_t stream);

/// Conditional CDF and quantiles (em_condition_quantile.hip): per missing coordinate j the one-dimensional mixture sum_k r_k N(t_kj,
/// s_kj^2) of the n rows of a chunk, from the same lw / lse as the conditioning pass -- its CDF at a value per (row, coordinate), or
/// its quantiles at n_prob probabilities. Row i's output is a pure function of row i and the parameters. The tiers and paddings are
/// ConditionKernel's and condition_pad's; the record is the conditioning pass's with [s (the padded dM) | w = 1 / s (the same)] behind it.
struct ConditionQuantileArgs : ConditionChunk {
    const double* values;                                    // CDF: n x dM, row-major and contiguous (16-byte aligned); quantile: unused
    const double* probabilities; const double* z;            // quantile: n_prob probabilities and their normal quantiles (device memory)
    uint32_t n_prob;
    double* out;                                             // n x dM row-major (16-byte aligned); quantile: n_prob such blocks, ldq doubles apart
    uint32_t* iterations;                                    // quantile: trips per output, in out's layout (blocks ldq apart); or null
    size_t ldq;                                              // even
    double* means;                                           // n x dM (16-byte aligned): E[x_M | x_O], the conditioning pass's bits; or null
    int skip;                                                // as ConditionArgs'
};
/// kConditionRegisters where the register tier is built for (dO, dM) -- the CDF to 32 x 32, the quantile search to the dM its state
/// fits the register file at (em_condition_quantile.hip states the bound) --, else kConditionPlain.
int em_condition_quantile_route(int dO, int dM, int quantile);
inline size_t condition_quantile_record_doubles(int kernel, int dO, int dM)
{
    return condition_record_doubles(kernel, dO, dM) + 2 * (size_t)condition_pad(kernel, dM);
}
/// Return the grid (0: nothing to do), or < 0 where the kernel asked for is not built for the shape.
int launch_em_condition_cdf(const ConditionQuantileArgs& a, int num_cus, hipStream_t stream);
int launch_em_condition_quantile(const ConditionQuantileArgs& a, int num_cus, hipStream_t stream);

enum MstatsMode : int {
    kFromLogResp = 0,  // r = exp(lw - lse)          (after an E-step)
    kFromResp = 1,      // r = lw                     (plain responsibilities: caller-given, one-hot, or all ones)
    kFromLogRespSelfNorm = 2   // r = e_k / sum_k e_k with the normalisation done by the statistics kernel itself (wide kernel, one
                               // row-block group); launch_em_reduce then also finishes lse = max + log(sum) and the ll partials
    ,
    kFromLogRespSelfNormWeighted = 3   // mode 2 on a block with row weights (MstatsArgs::weights): r w_i is accumulated, the ll
                                       // partials are those of w_i lse_i; lse itself stays the sample's own
};
struct MstatsArgs {
    const double* xt; size_t ldx; uint32_t n; int d;        // d = true dimension
    const double* shift;                                     // device, d doubles
    const double* lw; size_t ldr; const double* lse; int K; int mode;   // lw: [K][ldr], ldr >= n_pad
    double* partials; size_t partials_capacity;              // scratch (doubles)
    const double* ll_partials; int n_ll_partials;            // summed into stats[K*F] (may be null/0)
    double* stats;                                           // out: device, K*F + 1 doubles
    double* ll_scratch;                                      // kFromLogRespSelfNorm: >= 1024 doubles for the ll partials
    double* lse_out; double* ll_out;                         // kFromLogRespSelfNorm: per-sample max (-> lse) and exp-sum (n_pad each)
    unsigned long long* nz_count;                            // kFromLogRespSelfNorm (may be null): += nonzero responsibilities
    int plain;                                               // 1: the plain forms -- d <= kRegDim: whole column blocks per wave (no
                                                             // balanced dealing); d > kMaxDim: the plain tier even where big_dim.hip applies
    const double* weights;                                   // kFromLogRespSelfNormWeighted: the rows' weights (n_pad doubles, zero beyond n)
};
int launch_em_mstats_generic(const MstatsArgs& a, hipStream_t stream);   // d > kMaxDim: writes ONE partial block [K][F]
/// 128 < d <= 1024 on the matrix cores (big_dim.hip); the plain tier above it (and where the caller asks for it: Args::plain).
bool big_dim_applies(int d);
bool big_dim_kmeans_applies(int d);                                       // (its K-means kernel: any d > 128)
int big_dim_splits(int d, int K, int num_cus);
int launch_em_estep_big(const EstepArgs& a, int num_cus, hipStream_t stream);
int launch_em_mstats_big(const MstatsArgs& a, int num_cus, hipStream_t stream);   // writes big_dim_splits partial blocks [K][F]
/// Whether the statistics kernel chosen for (d, K) can normalise log-responsibilities itself (mode kFromLogRespSelfNorm).
bool em_mstats_self_norm_supported(int d, int K, int num_cus);
/// The sparse self-normalising statistics kernel (em_mstats_sparse.hip): same inputs, partial blocks and per-sample outputs as the
/// self-normalising wide kernel, but it accumulates only the nonzero responsibilities. Returns the grid (the partial blocks
/// written) or <= 0.
bool em_mstats_sparse_supported(int d, int K, int num_cus);
int launch_em_mstats_sparse(const MstatsArgs& a, int num_cus, hipStream_t stream);
/// What the one-kernel EM passes (E-step + statistics in one launch: em_fused_small.hip, em_diag.hip, em_tied.hip) all take.
struct OnePassArgs {
    const double* xt; size_t ldx; uint32_t n; int d;
    const double* shift; const double* params; int K;
    double* lse;                                             // out: per-sample log-sum-exp
    double* partials; size_t partials_capacity;              // scratch: [grid][KP][FP]
    double* ll_partials; int n_ll_partials;                  // out: per-workgroup log-likelihood sums (grid of them)
};
/// Fused E-step + statistics for small shapes (em_fused_small.hip): params are the estep_param_stride(D) records.
struct FusedArgs : OnePassArgs {
    int form;                                                // FusedForm
};
enum FusedForm : int {
    kFusedLdsFeed = 0,                                       // matrix-core form, records fed from LDS
    kFusedScalarFeed = 1,                                    // matrix-core form, records fed from scalar registers
    kFusedValu = 2,                                          // vector-unit form (one instantiation per (d, K))
};
namespace mstats {
bool em_fused_supported(int d, int K);
/// Tuning rules of the fused kernel's forms (em_fused_small.hip), functions of the shape alone: where the vector-unit form is
/// built and where it is the faster one; where the matrix-core form can take its records from LDS and where scalar registers win.
bool em_fused_valu_supported(int d, int K);
bool em_fused_valu_preferred(int d, int K, uint32_t n);
bool em_fused_lds_feed_supported(int d);
bool em_fused_scalar_feed(int d, uint32_t n);
int em_fused_partial_rows(int K);
int em_fused_partial_cols(int d);
int launch_em_fused_small(const FusedArgs& a, int num_cus, hipStream_t stream);
/// The grid launch_em_fused_small would use for these arguments if they ask for the vector-unit form and it runs with at most one
/// workgroup per CU; 0 otherwise.
int em_fused_valu_small_grid(const FusedArgs& a, int num_cus);
}
/// The whole loop of EM::fit (ML/EM.cpp:143-170) in ONE launch for short fits (em_resident.hip): resident workgroups, one
/// hand-off of the partial statistics per iteration, the closing arithmetic and the convergence test on the device. Pointers in
/// ring order: iteration i reads the records of slot i % 3 (slot 0 on entry) and leaves parameters / records in slot (i + 1) % 3,
/// exactly what the launches of runtime/em_loop.cpp leave.
struct ResidentArgs {
    const double* xt; size_t ldx; uint32_t n; int d; int K;
    const double* shift;
    double* records[3];                                      // estep_param_stride(d) records (device)
    double* info[3]; double* mixing[3]; double* means[3]; double* covs[3];   // the packs' parts (device, or pinned host memory)
    double* xch;                                             // device: em_resident_exchange_doubles(d, K, vgrid) doubles
    unsigned* sync;                                          // device: [arrivals, give-up flag], zeroed before the launch
    int vgrid;                                               // partial blocks = workgroups (em_fused_valu_small_grid)
    double n_global, refine_limit, atol, rtol, ll_offset;    // log-likelihood = sum / n_global - ll_offset
    double ridge;                                            // added to every covariance's diagonal by the closing (CloseArgs::ridge)
    uint32_t max_steps;
    double* history;                                         // pinned host: max_steps log-likelihoods
    uint32_t* result;                                        // pinned host: [status, iterations evaluated, converged]; status 1 = loop over,
                                                             // 2 = iteration `result[1]` flagged a refinement (not closed), 3 = a wait gave up
    unsigned long long* profile;                             // null, or kResidentStamps clock stamps per iteration (MLHIP_RESIDENT_PROFILE=1)
};
namespace mstats {
constexpr int kResidentSlices = 32;                          // (= em_reduce_kernel's slices: the same summation order)
constexpr int kResidentMaxGrid = 64;                          // workgroups (= partial blocks = CUs used): N <= 16 384
constexpr int kResidentStamps = 24;
size_t em_resident_exchange_doubles(int d, int K, int vgrid);
bool em_resident_supported(int d, int K, int vgrid, int num_cus);
bool launch_em_resident(const ResidentArgs& a, hipStream_t stream);
}
/// One iteration of SEVERAL independent full-covariance EM loops on one block -- the restarts of mlhip_em_iterate_restarts -- in three
/// launches however many loops are alive (em_restarts.hip): the vector-unit pass on a grid (grid, count), the fixed-order reduction
/// and the closing arithmetic, each the text the solo launches run (em_fused_valu_body.hpp, em_reduce_body.hpp, em_close_body.hpp).
/// Row y of a launch works on restart alive.index[y]; every per-restart array is `*_stride` doubles apart.
namespace mstats {
constexpr int kRestartsMaxBatch = 32;                        // restarts one launch carries at most (the index list rides in the kernel arguments)
}
struct RestartsAlive {
    int count;
    unsigned char index[mstats::kRestartsMaxBatch];          // ascending
};
struct RestartsArgs {
    const double* xt; size_t ldx; uint32_t n; int d; int K;
    const double* shift;
    int grid;                                                // workgroups per restart = its partial blocks (em_fused_valu_small_grid)
    RestartsAlive alive;
    const double* records_in; double* records_out; size_t records_stride;   // estep_param_stride(d) records: this iteration's, the next one's
    double* partials; size_t partials_stride;                // [grid][KP][FP] per restart
    double* ll_partials; size_t ll_stride;                   // [grid] per restart
    double* stats; size_t stats_stride;                      // [K F + 1] per restart
    double* mixing; double* means; double* covs; size_t pack_stride;       // the new parameters (device)
    double* info; size_t info_stride;                        // pinned host memory: [ll_sum | refine flag (K) | max |W (mu - shift)| (K)]
    double n_global, ridge, refine_limit;                    // as CloseArgs
};
namespace mstats {
/// The three launches, in this order on one stream. d = 1, 2, 3, 4, 6 with K <= valu_max_k(d): the shapes of the vector-unit pass;
/// false: not built for the shape, nothing was launched.
bool launch_em_restarts_pass(const RestartsArgs& a, hipStream_t stream);
bool launch_em_restarts_reduce(const RestartsArgs& a, hipStream_t stream);
bool launch_em_restarts_close(const RestartsArgs& a, hipStream_t stream);
}
/// Diagonal-covariance EM iteration in one kernel (em_diag.hip): params are em_diag_partial_rows(K) records of
/// diag_param_stride(padded_dim(d)) -- K real ones, then neutral padding (coef = -inf) -- and shift holds padded_dim(d)
/// doubles (zeros beyond d).
struct DiagArgs : OnePassArgs {
    int two_op;                                              // the records' (a, b) operands were built for THIS shift (the data's): the
                                                             // mixed-feed kernel may take its two-operation density form; 0 for a
                                                             // refinement pass about another shift (exact form)
    int exact;                                               // 1: the exact density form always
};
namespace mstats {
bool em_diag_supported(int d, int K);                        // d <= 32, K <= 64
int em_diag_partial_rows(int K);
int em_diag_partial_cols(int d);
int em_diag_grid(int d, int K, uint32_t n, int num_cus);
/// Returns the number of per-workgroup partial blocks written (stats and log-likelihood alike), or < 0.
int launch_em_diag(const DiagArgs& a, int num_cus, hipStream_t stream);
}
/// Tied-covariance EM iteration in one kernel (em_tied.hip): winv holds the shared whitening matrix (tied_winv_doubles(D) doubles,
/// D = padded_dim(d)), params em_tied_partial_rows(K) records of tied_param_stride(D) -- K real ones, then neutral padding
/// (coef = -inf) -- and shift D doubles (zeros beyond d).
struct TiedArgs : OnePassArgs {                              // (a row of a partial block: [S1 (d) | S0])
    const double* winv;
};
namespace mstats {
bool em_tied_supported(int d, int K);                        // d <= 32, K <= 64
int em_tied_partial_rows(int K);
int em_tied_partial_cols(int d);
int em_tied_grid(int d, int K, uint32_t n, int num_cus);
/// Returns the number of per-workgroup partial blocks written (stats and log-likelihood alike), or < 0.
int launch_em_tied(const TiedArgs& a, int num_cus, hipStream_t stream);
}
/// M-step closing arithmetic + next E-step records on the device (em_close.hip): one workgroup per component.
struct CloseArgs {
    const double* stats; int K; int d; int D;                // all-reduced statistics [K][F] + ll sum (F: full or diagonal)
    const double* shift; double n_global;                    // shift: D doubles, zero padded
    int layout;                                              // full covariances: 0 = estep_param_stride records, 2 = mfma4 records
    double refine_limit;                                     // <= 0: no refinement flags
    double ridge;                                            // added to the diagonal of every covariance formed (the data handle's; ML/EM.cpp:252 has 1e-15)
    double* mixing; double* means; double* covs;             // out (device): [K], [K*d], [K*d*d] (diagonal: [K*d] variances)
    double* records;                                         // out (device): the next E-step's K records
    double* info;                                            // out (device): [ll_sum | refine flag (K) | max |W (mu - shift)| (K)]
    double* work;                                            // d > 64: em_close_work_doubles(d, K) doubles of device scratch
};
size_t em_close_info_doubles(int K);
bool em_close_supported(int d);                              // d <= 64: one wave per component, the matrices in LDS (em_close.hip);
                                                             // 64 < d <= 1024: panelled, the matrices in global memory (em_close_big.hip)
size_t em_close_work_doubles(int d, int K);                  // 0 for d <= 64
bool em_close_big_supported(int d);
size_t em_close_big_work_doubles(int d, int K);
void launch_em_close_big(const CloseArgs& a, hipStream_t stream);
double* em_close_big_param_area(double* work, int d, int K);   // K (d d + d + 1) + 2 K + 1 doubles behind the matrices
/// Records of GIVEN parameters (a fit's first E-step): a.mixing / a.means / a.covs are device inputs, a.stats and a.ridge unused.
void launch_em_records_big(const CloseArgs& a, hipStream_t stream);
void launch_em_close(const CloseArgs& a, hipStream_t stream);
void launch_em_close_diag(const CloseArgs& a, hipStream_t stream);
/// Fixed-order combination of `n_partials` blocks [KP][FP] (and of the log-likelihood partials) into stats[K*F (+1)].
void launch_em_reduce_blocks(const double* partials, int n_partials, int KP, int FP, int K, int F, const double* ll_partials,
                             int n_ll, double* stats, hipStream_t stream);
/// resp[k*ldr + i] = (labels[i] == k), or 1 everywhere when labels == nullptr; columns n..n_pad-1 are zeroed.
void launch_fill_responsibilities(const uint32_t* labels, uint32_t n, int K, double* resp, size_t ldr, hipStream_t stream);
/// Doubles of scratch the statistics kernel needs for (d, K).
size_t em_mstats_scratch_doubles(int d, int K, int num_cus);
/// Main statistics kernel; returns the number of per-workgroup partials written (>0) or <0 on error.
int launch_em_mstats(const MstatsArgs& a, int num_cus, hipStream_t stream);
/// Fixed-order combination of those partials (and of the log-likelihood partials) into a.stats.
void launch_em_reduce(const MstatsArgs& a, int num_cus, int n_partials, hipStream_t stream);
/// out[0] = sum of n_ll log-likelihood partials (fixed order).
void launch_ll_reduce(const double* ll_partials, int n_ll, double* out, hipStream_t stream);

// ---- row weights (em_weights.hip): the passes a weighted block adds next to the unweighted kernels ----
/// Partials one weights pass writes (one per workgroup): a function of n alone, so every pass over the same block sums in the same order.
int weights_grid(uint32_t n);
/// Attach pass over `n` weights (w has n_pad entries; the pass zeroes w[n .. n_pad)): sum_partials[b] = workgroup b's sum of the valid
/// weights (finite, >= 0), bad_partials[b] = how many of its weights are not valid. Returns the number of partials.
int launch_weights_attach(double* w, uint32_t n, uint32_t n_pad, double* sum_partials, double* bad_partials, hipStream_t stream);
/// ll_partials[b] = workgroup b's sum of w_i lse_i over the rows with w_i != 0, in the layout launch_ll_reduce / launch_em_reduce read.
/// Returns the number of partials (<= 1024).
int launch_weighted_ll(const double* w, const double* lse, uint32_t n, double* ll_partials, hipStream_t stream);
/// out[k*ldo + i] = w_i r_ik for i < n, 0 for n <= i < n_pad, with r_ik = exp(src - lse_i) (mode kFromLogResp) or src (kFromResp),
/// src = src[k*lds + i]: the plain responsibilities the statistics kernels then take in mode kFromResp.
/// After a weighted self-normalising statistics pass: em_lse_finish_kernel's work (lse[i] = max + log(esum[i]) in place) with the
/// partials of w_i lse_i in its layout and on its tree; `n_ll` workgroups, the number launch_em_reduce uses for the unweighted form.
void launch_weighted_lse_finish(double* lse, const double* esum, const double* w, uint32_t n, int n_ll, double* ll_partials,
                                hipStream_t stream);
void launch_weighted_resp(const double* src, size_t lds, const double* lse, int mode, const double* w, uint32_t n, uint32_t n_pad, int K,
                          double* out, size_t ldo, hipStream_t stream);

struct RespArgs {
    const double* lw; size_t ldr; const double* lse; uint32_t n; int K;
    double* resp; size_t ldo;       // out (may be null): resp[k*ldo + i]
    uint32_t* labels;               // out (may be null)
};
void launch_em_responsibilities(const RespArgs& a, hipStream_t stream);

// ---- K-means -----------------------------------------------------------------------------------------
struct KmeansArgs {
    const double* xt; size_t ldx; uint32_t n; int D; int d;
    const double* centroids; int K;            // device, [K][D] (padded coordinates zero)
    const double* scale;                       // device, 2 d doubles: per-dimension power-of-two scale of the exact sums, as two factors [f1 (d) | f2 (d)]
    uint32_t* labels; const uint32_t* old_labels; int have_old;
    double* min_dist;                          // out (may be null): per-sample min squared distance
    int accumulate;                            // also accumulate per-cluster sums / counts
    double* partials; size_t partials_capacity;
    double* cnorm;                             // device scratch, K rounded up to 16 doubles: -|c_k|^2/2 (chunked-table kernel)
    double* out;                               // device: [inertia, n_changed, counts(K), sums(K*d)]
    int kernel;                                // KmKernel: which assignment kernel runs
};
enum KmKernel : int {
    kKmDirect = 0,                             // direct form (kmeans.hip), d <= kMaxDim
    kKmMatrix = 1,                             // matrix-core search with exact recheck (kmeans_mfma.hip)
    kKmBigDim = 2,                             // d > kMaxDim, register-blocked (big_dim.hip)
    kKmPlain = 3,                              // d > kMaxDim, plain (generic_dim.hip)
};
size_t kmeans_scratch_doubles(int d, int K, int num_cus);
bool kmeans_mfma_supported(int D, int K);
/// Tuning rule: few clusters on many samples, where the direct-form kernel beats the matrix-core search (kmeans.hip).
bool kmeans_few_clusters(int D, int K, uint32_t n);
/// The whole step loop of KMeans::fit_once in one launch of one workgroup (kmeans_resident.hip): small blocks, few clusters, the
/// dimensions whose step runs on the direct-form kernel. `out` is host-visible pinned memory:
/// [steps, converged, inertia, label buffer, counts(K), centroids(K d), old centroids(K d)].
constexpr int kKmResidentMaxN = 4096, kKmResidentMaxK = 32;
struct KmResidentArgs {
    const double* xt; size_t ldx; uint32_t n; int D, d, K;
    double* cent;                              // device, [K][D]: the starting table in, the final one out
    const double* scale;                       // device, 2 d doubles (as KmeansArgs)
    uint32_t* labels[2]; int label_buf, have_old;   // the two label buffers, which one holds the assignment before, whether it does
    double* min_dist;
    uint32_t max_steps; double atol;
    double* out;
    int copies;                                // (set by the launcher)
};
bool kmeans_resident_supported(int D, int d, int K, uint64_t n);
bool launch_kmeans_resident(const KmResidentArgs& a, hipStream_t stream);
/// Assignment kernel; returns the number of per-workgroup partials (>0) or <0 on error.
int launch_kmeans_assign(const KmeansArgs& a, int num_cus, hipStream_t stream);
void launch_kmeans_assign_generic(const KmeansArgs& a, int grid, size_t pstride, hipStream_t stream);   // d > kMaxDim (generic_dim.hip)
/// 128 < d <= 1024 (big_dim.hip): the same exact arithmetic, register-blocked; returns the partial blocks used, 0: not applicable.
int launch_kmeans_assign_big(const KmeansArgs& a, int grid_max, size_t pstride, hipStream_t stream);
/// The update sums as a sweep of their own (kmeans.hip), over the `grid` partial blocks the assignment kernel just wrote: every route
/// whose accumulators do not fit LDS beside its assignment.
void launch_kmeans_update(const KmeansArgs& a, int grid, size_t pstride, hipStream_t stream);
void launch_kmeans_reduce(const KmeansArgs& a, int n_partials, hipStream_t stream);
/// update_step's closing arithmetic on the (all-reduced) output block [inertia, changed, counts(K), sums(K*d)]: the sums
/// become the means IN PLACE (empty cluster -> origin, ML/KMeans.cpp:184) and are written as the next centroid table
/// next[K][D] (padded coordinates zero). `mirror` (may be null): host-visible pinned memory that receives a copy of the whole block
/// from the same kernel -- the host then only waits for the stream; a separate hipMemcpyAsync of these 2 + K (d + 1) doubles goes
/// through a copy engine and costs more than the kernel itself.
void launch_kmeans_close(double* out, int K, int d, int D, double* next, double* mirror, hipStream_t stream);

/// Weighted update sweep + its reduction (kmeans.hip: the weighted forms of the update sweep and of the reduction), after an assignment that ran with accumulate = 0: out[0] becomes the
/// weighted inertia sum_i w_i min_dist_i and, with_sums != 0, out[2 ..] the weighted counts sum_i w_i (K) and the sums sum_i w_i x_i
/// (K*d), exact sums of the rounded products; out[1] (n_changed) is not touched. `factors` (device, 2d + 2 doubles, powers of two):
/// [f1 (d) | f2 (d) | c1 | c2] with f1_j f2_j = 2^(94 - ej - ew) and c1 c2 = 2^(94 - ew), max|x_j| < 2^ej, max w < 2^ew over all
/// ranks. xt is the UNPADDED block. Returns the partial blocks used, -2 if the scratch is too small.
struct KmWeightedArgs {
    const double* xt; size_t ldx; uint32_t n; int d;
    const uint32_t* labels; const double* min_dist;       // of the assignment just run
    const double* weights;                                 // n_pad doubles, zero beyond n
    const double* factors;
    int K; int with_sums;
    double* partials; size_t partials_capacity;
    double* out;
};
size_t kmeans_weighted_scratch_doubles(int d, int K, int num_cus);
int launch_kmeans_weighted(const KmWeightedArgs& a, int num_cus, hipStream_t stream);

}  // namespace mlhip
