/* mlhip.h -- C ABI of the MI355X (gfx950) Gaussian-mixture EM / K-means hot path.
 *
 * Drop-in boundary. The reference (romanwerpachowski/ML, "ML++") has no FFI of its own for this
 * path: the hot loops are private C++ member functions. Each entry point below is the device-side
 * replacement of one of them and cites the reference function it stands in for (paths relative to
 * the reference checkout). The C++ facade in include/ML/ (ml::EM, ml::Clustering::KMeans -- same
 * names and semantics as ML/EM.hpp, ML/KMeans.hpp) and the Python surface ml_amd.cppyml.clustering
 * (same names as cppyml/clustering.cpp) are built on these calls only.
 *
 * Conventions
 *  - plain C types only; every function returns 0 on success, <0 on error (MLHIP_E_*);
 *    mlhip_last_error() gives the thread-local message of the last failure;
 *  - matrices are column-major, one sample per column (d x N), exactly the memory of the reference's
 *    `Eigen::Ref<const Eigen::MatrixXd> data` (ML/Clustering.hpp:28-33) == a C-contiguous N x d numpy
 *    array (cppyml/clustering.cpp:27-30). `ld` = distance in doubles between consecutive samples;
 *  - all pointers are HOST pointers owned by the caller unless a name ends in `_dev`;
 *  - one context drives one GPU (one process per GPU) -- or, created as a device GROUP (mlhip_ctx_create_group), all the GPUs of
 *    the node from one process; a context is not thread-safe;
 *  - there is no CPU fallback: without a usable HIP device every compute entry point fails with
 *    MLHIP_E_NO_DEVICE.
 */
#ifndef MLHIP_H
#define MLHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MLHIP_OK 0
#define MLHIP_E_INVALID_ARGUMENT (-1) /* maps to std::invalid_argument in the facade */
#define MLHIP_E_DOMAIN (-2)           /* maps to std::domain_error */
#define MLHIP_E_RUNTIME (-3)          /* HIP / collective failure: std::runtime_error */
#define MLHIP_E_NO_DEVICE (-4)        /* no usable GPU: std::runtime_error */
#define MLHIP_E_UNSUPPORTED (-5)      /* shape outside what the kernels are built for */

typedef struct mlhip_ctx mlhip_ctx;   /* one GPU + stream + scratch */
typedef struct mlhip_data mlhip_data; /* a d x N sample block resident in HBM (row shard of this rank) */

const char* mlhip_last_error(void);
const char* mlhip_version(void);

/* ---- context ------------------------------------------------------------------------------------ */
int mlhip_device_count(int* count);
/* device_id < 0: take MLHIP_DEVICE, else LOCAL_RANK, else 0. */
int mlhip_ctx_create(int device_id, mlhip_ctx** out);
/* DEVICE GROUP: one context over n_shards shards, shard s on GPU device_ids[s] (NULL: s mod the number of visible GPUs; an id may
 * repeat -- several shards on one GPU is how a one-GPU box runs the 8-GPU configurations at full size). This is the single-process
 * multi-GPU form of the reference's API -- `bool EM::fit(Eigen::Ref<const MatrixXd>)` (ML/EM.cpp:91) and KMeans::fit (ML/KMeans.cpp:25)
 * take ONE d x N block in ONE process: mlhip_data_upload on a group row-shards the caller's block over the shards (contiguous, balanced),
 * and EVERY entry point below accepts the group's context with the caller's WHOLE arrays (all N rows of labels / responsibilities /
 * targets / weights; results are those of a single context, up to the summation order of the statistics). Inside, one host thread per
 * shard drives that shard's GPU with the ordinary per-context code, and the shards' statistics meet once per iteration:
 *   - shards on distinct GPUs: RCCL (ncclCommInitAll, ncclAllReduce on each shard's stream);
 *   - otherwise, or with MLHIP_GROUP_REDUCE=direct: an in-process all-reduce -- every shard sums all shards' buffers in shard order with
 *     the same kernel (peer access over xGMI between GPUs), so the shards hold bit-identical sums and runs are reproducible.
 * To its caller a group is ONE rank (mlhip_ctx_world: 1, 0); it takes no all-reduce hook or communicator of its own. */
int mlhip_ctx_create_group(int n_shards, const int* device_ids, mlhip_ctx** out);
/* What the C++ facade / Python surface use (ml::device::context()): a group when the environment asks for one -- MLHIP_DEVICES=0,1,2,3
 * (one shard per entry) or MLHIP_NUM_GPUS=n (ignored under a one-process-per-GPU launcher, i.e. when LOCAL_RANK is set) -- else
 * mlhip_ctx_create(-1). */
int mlhip_ctx_create_default(mlhip_ctx** out);
int mlhip_ctx_destroy(mlhip_ctx* ctx);
/* Shards of a context (1 for an ordinary one), the GPU of a shard, and how the statistics are summed: "none", "hook-host",
 * "hook-device", "rccl" (mlhip_ctx_init_rccl), "group-rccl", "group-direct" (a string constant). */
int mlhip_ctx_shards(const mlhip_ctx* ctx, int* n_shards);
int mlhip_ctx_shard_device(const mlhip_ctx* ctx, int shard, int* device_id);
int mlhip_ctx_reduce_kind(const mlhip_ctx* ctx, const char** kind);
int mlhip_ctx_synchronize(mlhip_ctx* ctx);
int mlhip_ctx_device(const mlhip_ctx* ctx, int* device_id);
/* The HIP stream (hipStream_t) every kernel of this context is launched on. */
int mlhip_ctx_stream(const mlhip_ctx* ctx, void** stream);

/* Row-sharded multi-GPU: the N samples are split across `world_size` ranks; the only
 * exchange is one sum all-reduce per iteration of the sufficient statistics. The library calls `fn` on the
 * buffer to be summed in place across ranks; with on_device != 0 `buf` is a device pointer valid on the
 * context's stream (hand it to RCCL / torch.distributed "nccl"), else a host pointer (gloo, MPI).
 * The hook must return only when `buf` holds the global sum and is safe to read from the context's stream.
 * fn == NULL restores single-rank behaviour. */
typedef int (*mlhip_allreduce_fn)(void* user, double* buf, size_t count, int on_device, void* stream);
int mlhip_ctx_set_allreduce(mlhip_ctx* ctx, mlhip_allreduce_fn fn, void* user, int on_device,
                            int world_size, int rank);

/* Native RCCL (no Python, no hook to write): the library opens its own communicator on the context's GPU and sums the
 * statistics with ncclAllReduce(ncclDouble, ncclSum) on the context's stream -- what a multi-GPU ml::EM::fit /
 * ml::Clustering::KMeans::fit (ML/EM.hpp:82, ML/KMeans.hpp:36) uses from C++. One process per GPU:
 *   rank 0:   mlhip_rccl_unique_id(id);  ...hand the 128 bytes to the other ranks (file, pipe, MPI_Bcast, a store)...
 *   all:      mlhip_ctx_init_rccl(ctx, id, world_size, rank);        (collective: returns when all ranks have joined)
 * mlhip_ctx_init_rccl_file does the hand-over through a file that all ranks can see (rank 0 writes it atomically,
 * the others wait for it up to MLHIP_RCCL_TIMEOUT_S seconds, default 120); use a fresh path per job.
 * librccl.so.1 is loaded on first use (override: MLHIP_RCCL_LIBRARY). RCCL refuses two ranks on the same GPU.
 * Rank 0 removes the rendezvous file once the communicator exists; files older than MLHIP_RCCL_STALE_S seconds (default 600:
 * the left-over of a job that died before that) are ignored by the waiting ranks, and so is a file whose job nonce differs (a hash
 * of MLHIP_RCCL_NONCE, TORCHELASTIC_RUN_ID, MASTER_ADDR, MASTER_PORT as the ranks see them -- the same within a launch).
 * mlhip_rccl_available() says whether librccl can be loaded in THIS process without touching a GPU: ranks of a job can agree on
 * it (over whatever channel they have) BEFORE anyone enters the collective mlhip_ctx_init_rccl*, where a rank that cannot load
 * the library would leave the others waiting. */
#define MLHIP_RCCL_UNIQUE_ID_BYTES 128
int mlhip_rccl_available(void);   /* 1 / 0; never fails */
int mlhip_rccl_unique_id(void* unique_id /* MLHIP_RCCL_UNIQUE_ID_BYTES bytes */);
int mlhip_ctx_init_rccl(mlhip_ctx* ctx, const void* unique_id, int world_size, int rank);
int mlhip_ctx_init_rccl_file(mlhip_ctx* ctx, const char* path, int world_size, int rank);
/* Number of ranks of the context's own RCCL communicator as RCCL reports it (ncclCommCount); 0 without one. */
int mlhip_ctx_rccl_ranks(const mlhip_ctx* ctx, int* nranks);
int mlhip_ctx_finalize_rccl(mlhip_ctx* ctx);

/* In-place sum of `count` host doubles across ranks through the installed hook (no-op without one). The facade
 * uses it to agree on initial parameters (rank 0 contributes them, the others contribute zeros). */
int mlhip_ctx_allreduce(mlhip_ctx* ctx, double* buf, size_t count);
int mlhip_ctx_world(const mlhip_ctx* ctx, int* world_size, int* rank);

/* ---- resident data ------------------------------------------------------------------------------ */
/* Copies this rank's d x n block to HBM (stored dimension-major for coalesced per-sample access) and
 * computes the statistics shift (global column mean; all-reduced when a hook is set). The host block is
 * only read during the call (the reference borrows `data` for the duration of fit, ML/EM.cpp:91).
 * 1 <= d <= 4096 (MLHIP_E_UNSUPPORTED above; 128 < d <= 1024: matrix-core kernels of device/big_dim.hip; above: plain, untuned kernels, device/generic_dim.hip), n < 2^32 - 256 per rank. */
int mlhip_data_upload(mlhip_ctx* ctx, const double* x, uint32_t d, uint64_t n, int64_t ld, mlhip_data** out);
/* Same, from a sample-major block already in device memory (e.g. a torch tensor's data_ptr()). */
int mlhip_data_upload_dev(mlhip_ctx* ctx, const double* x_dev, uint32_t d, uint64_t n, int64_t ld, mlhip_data** out);
int mlhip_data_free(mlhip_data* data);
int mlhip_data_shape(const mlhip_data* data, uint32_t* d, uint64_t* n_local, uint64_t* n_global);
/* Rows [first_row, first_row + n_rows) of the uploaded block that shard `shard` holds (an ordinary context: shard 0, all rows). */
int mlhip_data_shard_rows(const mlhip_data* data, int shard, uint64_t* first_row, uint64_t* n_rows);
/* Global column means used as the numerical shift of the second-moment accumulation (d doubles). */
int mlhip_data_shift(const mlhip_data* data, double* shift);

/* EXTENSION (no counterpart in the reference): frequency weights w_i of the block's rows -- de-duplicated or binned samples, importance
 * weights, coresets -- without replicating rows. `weights` holds this rank's n_local values (a device group: all N, sharded like the
 * rows); every w_i finite and >= 0, their total W over ALL ranks > 0 (checked on the device, W summed in a fixed order per shard and
 * all-reduced like the statistics; otherwise MLHIP_E_INVALID_ARGUMENT on every rank and the block is left UNWEIGHTED). NULL removes
 * the weights: every entry point then does exactly what it did before they were set. The array is only read during the call; the
 * weights stay with the handle until replaced or removed. E-step results the handle holds are dropped. With weights attached:
 *   * every log-likelihood the EM entry points report (mlhip_em_expectation / _step / _step_diag / _iterate and its history) is
 *     (1/W) sum_i w_i log sum_k pi_k N(x_i | mu_k, Sigma_k), and the convergence test of mlhip_em_iterate runs on it;
 *   * every M-step (mlhip_em_step / _step_diag / _iterate / _maximisation / _maximisation_from / _from_labels, the refinement pass
 *     about a component's own mean included) forms sum_i w_i r_ik vech(xt_i xt_i^T); mixing_k = S0_k / W; the caller's
 *     responsibilities / labels are not changed;
 *   * mlhip_sample_covariance is sum_i w_i (x_i - m)(x_i - m)^T / (W - 1) about m = sum_i w_i x_i / W.
 * With integer weights this is the unweighted result on the sample with row i repeated w_i times; scaling all weights by a constant
 * changes nothing beyond rounding. NOT weighted: per-row results (mlhip_em_responsibilities, mlhip_em_labels, mlhip_em_score: a row
 * of weight 0 still gets its responsibilities, its label and its density), the statistics shift (mlhip_data_shift stays the plain
 * column mean), mlhip_xxt_xy, mlhip_random_partition_means, mlhip_kmeans_step / _iterate / _assign and every kpp_* entry point:
 * they and the initialisers see rows, not weights, on a weighted handle too (a weighted EM fit with a K-means++ start relies on
 * that). The weighted K-means is a set of entry points of its own: mlhip_kmeans_step_weighted / _iterate_weighted / _assign_weighted.
 * A weighted block runs the E-step tier of its shape; where the unweighted fit runs the self-normalising statistics form (d = 12 ..
 * 128, K <= 64) so does the weighted one, with the weight applied while the kernel stages a responsibility (one exponential per pair,
 * no second N x K block); elsewhere one pass writes w_i r_ik for the statistics kernel of the shape. It never takes the fused,
 * resident, sparse or diagonal-kernel routes (mlhip_em_route reports the route it takes). Responsibilities and labels after a
 * weighted E-step are, bit for bit, those of the unweighted E-step on the same kernel route -- the default route wherever that is not
 * the fused kernel (there: the route of MLHIP_FUSED=0). */
int mlhip_data_set_weights(mlhip_ctx* ctx, mlhip_data* data, const double* weights);
/* W, the all-reduced total of the attached weights; n_global (as a double) for an unweighted block. */
int mlhip_data_weight_sum(const mlhip_data* data, double* total);

/* EXTENSION (scikit-learn's reg_covar; the reference hard-wires 1e-15, ML/EM.cpp:252): the covariance ridge r of the handle, what every
 * M-step on it adds to the diagonal of each covariance it FORMS -- full mode: every Sigma_k = S_k + r I; diagonal mode: every variance;
 * tied mode: the one Sigma, r once. It is read by mlhip_em_step / _step_diag / _step_tied / _iterate (all three covariance types, closed
 * on the host or on the device, the one-launch resident loop included), mlhip_em_maximisation / _maximisation_from /
 * _maximisation_from_labels and the refinement pass about a component's own mean: one plain fp64 add per diagonal entry on every
 * route, so two routes that agree bit for bit at the default agree bit for bit at any r. r finite and >= 0 (-0.0 counts as 0; r = 0 adds
 * 0.0); NaN, an infinity or a negative value: MLHIP_E_INVALID_ARGUMENT and the handle keeps its ridge. The default keeps the
 * reference's bits. The ridge is ABSOLUTE, in squared data units (at a uniform data scale of 2^-30 the default dominates every
 * variance): where that matters the caller scales it with the data. NOT touched: parameters a caller GIVES (the first E-step,
 * mlhip_em_expectation, mlhip_em_score use them as they are), mlhip_sample_covariance, the kernel routes (mlhip_em_route / _tied_route /
 * _score_route report what they reported). Setting the ridge drops nothing the handle holds: E-step results stay valid. A device group's
 * handle passes the value to every shard's part and mirrors it. In a multi-process job every rank sets its own handle; nothing is
 * all-reduced (ranks that disagree fail the end-of-fit checksum exchange of mlhip_em_iterate). */
#define MLHIP_DEFAULT_COVARIANCE_RIDGE 1e-15
int mlhip_data_set_covariance_ridge(mlhip_ctx* ctx, mlhip_data* data, double ridge);
int mlhip_data_covariance_ridge(const mlhip_data* data, double* ridge);

/* ---- Gaussian-mixture EM -------------------------------------------------------------------------- */
/* One EM iteration == EM::expectation_step + EM::maximisation_step (ML/EM.cpp:190-263, incl.
 * process_covariances :274-287) on the resident shard, statistics all-reduced across ranks.
 *   in : mixing[K], means[d*K] (column k = mean k), covariances[K*d*d] (symmetric, column-major each)
 *   out: *log_likelihood  = mean_i log sum_k pi_k N(x_i|mu_k,Sigma_k)  under the INPUT parameters (:211)
 *        mixing_out/means_out/covariances_out = the M-step result (:229-257, the handle's ridge, default 1e-15, included)
 * Output arrays may alias the input arrays. The E-step results stay available on the device for
 * mlhip_em_responsibilities / mlhip_em_labels (for small shapes, where the iteration runs as one fused kernel, the
 * N x K block is rebuilt from the same parameter records when one of them is called). */
int mlhip_em_step(mlhip_ctx* ctx, mlhip_data* data, uint32_t K,
                  const double* mixing, const double* means, const double* covariances,
                  double* log_likelihood, double* mixing_out, double* means_out, double* covariances_out);

/* EXTENSION (no counterpart in the reference, whose ml::EM is full-covariance only, ML/EM.hpp:175; BASELINE.json configs[1]):
 * one EM iteration with DIAGONAL covariances -- the loops of mlhip_em_step restricted to the diagonal, in one kernel
 * (X read once, no N x K block in HBM). variances / variances_out: K*d doubles, variances[k*d + j] = sigma_kj^2 (the handle's ridge, default 1e-15,
 * included on output, ML/EM.cpp:252). One fused kernel for d <= 32, K <= 64; other shapes run the full-covariance kernels on diagonal matrices. mlhip_em_responsibilities /
 * mlhip_em_labels afterwards work as after mlhip_em_step (the block is rebuilt from the same parameters on demand). */
int mlhip_em_step_diag(mlhip_ctx* ctx, mlhip_data* data, uint32_t K,
                       const double* mixing, const double* means, const double* variances,
                       double* log_likelihood, double* mixing_out, double* means_out, double* variances_out);

/* EXTENSION (no counterpart in the reference): one EM iteration with a TIED covariance -- K means and ONE covariance Sigma shared by
 * every component (scikit-learn's covariance_type='tied'; the LDA-style mixture). covariance / covariance_out: d*d doubles (symmetric,
 * column-major). The E-step, the log-likelihood, labels and responsibilities are those of mlhip_em_step on K components that all
 * carry Sigma; the M-step, with xt = x - shift, W the total weight (N when unweighted), S0_k = sum_i w_i r_ik, S1_k = sum_i w_i r_ik xt_i
 * and T = sum_i w_i xt_i xt_i^T (constant over a fit: formed once per handle, all-reduced once), is
 *   pi_k = S0_k / W,  mu_k = shift + S1_k / S0_k,  Sigma = (T - sum_k S1_k S1_k^T / S0_k) / W + r I     (r: the handle's ridge, default 1e-15 -- ML/EM.cpp:252 --, once)
 * == sum_k pi_k Sigma_k over mlhip_em_step's covariances; an empty component behaves as there. One kernel for unweighted blocks with
 * d <= 32, K <= 64 (the sample is whitened once, not once per component; K (d + 1) + 1 statistics are all-reduced); other shapes,
 * weighted blocks, the few-component shapes whose full-covariance step is the vector-unit fused kernel (measured faster composed;
 * MLHIP_TIED=kernel takes the kernel there too) and MLHIP_TIED=composed run mlhip_em_step on K copies of Sigma and pool its
 * covariances (slower than it could be, never refused). Output arrays may alias the input arrays. mlhip_em_responsibilities / _responsibilities_rows / mlhip_em_labels
 * afterwards work as after mlhip_em_step (the block is rebuilt from the same parameters on demand).
 * Conditioning: T / W - sum_k pi_k (mu_k - shift)(mu_k - shift)^T loses about log10(|T / W| / lambda_min(Sigma)) digits (the formula
 * scikit-learn uses); the composed route's refinement pass does not. */
int mlhip_em_step_tied(mlhip_ctx* ctx, mlhip_data* data, uint32_t K,
                       const double* mixing, const double* means, const double* covariance,
                       double* log_likelihood, double* mixing_out, double* means_out, double* covariance_out);

/* The iteration loop of EM::fit (ML/EM.cpp:143-170) in ONE call: up to max_steps trips of E-step + M-step, each followed by the
 * reference's convergence test |ll - ll_old| < absolute_tolerance + relative_tolerance * max(|ll_old|, |ll|) from the second
 * trip on (:161-168). Parameters are updated IN PLACE (covariances: K*d*d doubles, or K*d variances with
 * MLHIP_COVARIANCE_DIAGONAL); *log_likelihood is that of the last E-step (i.e. under the parameters before the last M-step, like
 * the reference). Between two tests everything stays on the device -- statistics, all-reduce, the M-step's closing arithmetic
 * and the K Cholesky / inverse factorizations of EM::process_covariances (:274-287), the next E-step's records -- and the
 * host reads back 1 + 2K doubles per iteration (d <= 1024: one wave per component with the matrices in LDS up to d = 64, panelled
 * factorizations in global memory above; beyond d = 1024, or with MLHIP_DEVICE_CLOSE=0, the loop runs through mlhip_em_step).
 * MLHIP_COVARIANCE_TIED (covariances: d*d doubles, the one shared matrix): every trip is one mlhip_em_step_tied, closed on the HOST --
 * closing tied iterations on the device is not built. Same results as calling mlhip_em_step in a loop, to the last bits of log().
 * log_likelihood_history (max_steps doubles) may be NULL. Tolerances 0 run exactly max_steps iterations. */
#define MLHIP_COVARIANCE_FULL 0
#define MLHIP_COVARIANCE_DIAGONAL 1
#define MLHIP_COVARIANCE_TIED 2
int mlhip_em_iterate(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, int covariance_type,
                     double* mixing, double* means, double* covariances,
                     uint32_t max_steps, double absolute_tolerance, double relative_tolerance,
                     uint32_t* steps_done, int* converged, double* log_likelihood, double* log_likelihood_history);

/* EXTENSION (the reference's EM has no restarts; its KMeans has set_number_initialisations): R loops of mlhip_em_iterate from R
 * starts on the one resident block, and the best of them. mixing (R*K), means (R*K*d) and covariances (R*n_cov doubles, n_cov = K*d*d /
 * K*d / d*d by covariance_type) hold start r at offset r*K, r*K*d, r*n_cov and are updated IN PLACE: the parameters of EVERY restart
 * come back. steps_done, converged and log_likelihood hold R entries, log_likelihood_history (may be NULL) max_steps entries per
 * restart (row r at r*max_steps). Every restart's numbers are bit for bit those of mlhip_em_iterate from the same start on the same
 * handle. *best is the restart mlhip_em_select_restart picks, and the handle is left holding the E-step state of THAT restart:
 * mlhip_em_responsibilities, _responsibilities_rows and mlhip_em_labels return what they would after its solo mlhip_em_iterate (the
 * winner is not fitted again: the records of its last E-step are kept, the N x K block is rebuilt from them on demand).
 * Routes (mlhip_em_restarts_route): SEQUENTIAL -- the solo loop R times, every shape and mode, weighted blocks, device groups and
 * multi-rank jobs (every rank sees the same log-likelihoods and selects the same restart); BATCHED -- full covariances on an
 * unweighted block of a single rank whose iteration is the fused kernel in its vector-unit form on at most one workgroup per CU
 * (d = 1, 2, 3, 4, 6, K <= 32 / 16 / 10 / 7 / 4 with K (d+1)(d+2)/2 <= 64, about N <= 256 CUs): the restarts still running share the three
 * launches of an iteration (em_restarts.hip), at most MLHIP_RESTARTS_MAX_BATCH per launch, more in successive groups; a restart
 * whose closing raises a refinement flag leaves the batch and is run solo from its start. R = 0 is an argument error; other
 * arguments are checked as by mlhip_em_iterate. */
#define MLHIP_RESTARTS_MAX_BATCH 32
#define MLHIP_RESTARTS_BATCH_FROM 4
int mlhip_em_iterate_restarts(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, int covariance_type, uint32_t R,
                              double* mixing, double* means, double* covariances,
                              uint32_t max_steps, double absolute_tolerance, double relative_tolerance,
                              uint32_t* steps_done, int* converged, double* log_likelihood, double* log_likelihood_history,
                              uint32_t* best);
/* The selection rule of mlhip_em_iterate_restarts as a plain host function (no GPU needed): among the restarts that converged the
 * greatest final log-likelihood wins, compared with a strict '>' in ascending r -- the first of equals wins; if none converged the
 * same rule runs over all restarts. A NaN log-likelihood never wins; if every log-likelihood is NaN, restart 0 wins. R >= 1. */
int mlhip_em_select_restart(uint32_t R, const double* log_likelihood, const int* converged, uint32_t* best);
/* Which route mlhip_em_iterate_restarts takes for R restarts of K components on `data` (diagnostic, nothing is launched), under the
 * switches as they are set now: *route is MLHIP_RESTARTS_SEQUENTIAL or MLHIP_RESTARTS_BATCHED, *per_launch the number of restarts one
 * launch carries (1 on the sequential route). The batch is taken automatically from MLHIP_RESTARTS_BATCH_FROM restarts on (measured:
 * profiles/em_restarts_timing.txt); MLHIP_EM_RESTARTS=sequential / batch forces either route where the batch exists and is ignored
 * where it does not. covariance_type as in mlhip_em_iterate. A device group's block always reports SEQUENTIAL. */
enum { MLHIP_RESTARTS_SEQUENTIAL = 0, MLHIP_RESTARTS_BATCHED = 1 };
int mlhip_em_restarts_route(const mlhip_data* data, uint32_t K, int covariance_type, uint32_t R, int* route, uint32_t* per_launch);

/* E-step only (ML/EM.cpp:190-219): leaves log-responsibilities on the device, returns the log-likelihood. */
int mlhip_em_expectation(mlhip_ctx* ctx, mlhip_data* data, uint32_t K,
                         const double* mixing, const double* means, const double* covariances,
                         double* log_likelihood);
/* M-step only (ML/EM.cpp:221-263) from the responsibilities left by the last E-step. */
int mlhip_em_maximisation(mlhip_ctx* ctx, mlhip_data* data, uint32_t K,
                          double* mixing_out, double* means_out, double* covariances_out);
/* M-step from caller-given responsibilities (n_local x K column-major, ldr >= n_local): the
 * `maximise_first` start (ML/EM.cpp:120-125). */
int mlhip_em_maximisation_from(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, const double* resp, int64_t ldr,
                               double* mixing_out, double* means_out, double* covariances_out);
/* M-step from hard labels (one-hot responsibilities, what ClosestCentroid::init produces,
 * ML/Clustering.cpp:72-89) without materialising N x K on the host. */
int mlhip_em_maximisation_from_labels(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, const uint32_t* labels,
                                      double* mixing_out, double* means_out, double* covariances_out);

/* Normalised responsibilities of the last E-step, this rank's n_local x K block, column-major
 * (EM::responsibilities(), ML/EM.hpp:132-135; rows /= row sum, ML/EM.cpp:214-218). */
int mlhip_em_responsibilities(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, double* resp, int64_t ldr);
/* Rows [first_row, first_row + n_rows) of that block only (n_rows x K, column-major, ldr >= n_rows): what a verbose fit prints
 * (`responsibilities_.topRows(10)`, ML/EM.cpp:155-156) and what a Python slice of the lazy property needs -- 10 rows cost 10 rows,
 * not the N x K block. */
int mlhip_em_responsibilities_rows(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, uint64_t first_row, uint64_t n_rows, double* resp,
                                   int64_t ldr);
/* argmax_k of those responsibilities, first maximum wins (EM::calculate_labels, ML/EM.cpp:289-304). */
int mlhip_em_labels(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, uint32_t* labels);

/* EXTENSION (not in the reference surface): per-sample log-density  log sum_k pi_k N(x_i | mu_k, Sigma_k)  and label
 * argmax_k of the log-responsibilities (first maximum wins; 0xffffffff where the density is NaN) of this rank's rows of `data`
 * under the given mixture -- the batch form of EM::assign_responsibilities (ML/EM.cpp:176-188), in the log domain: a row the
 * reference's linear-domain sum underflows on still gets its finite log-density. covariance_type as in mlhip_em_iterate (diagonal:
 * K*d variances; tied: the d*d shared matrix, scored by the full-covariance routes on K components that carry it). log_density (n_local doubles) and labels (n_local) may each be NULL. No N x K block is allocated (d <= 128: one
 * kernel that writes 8 + 4 bytes per row; above, and under MLHIP_SCORE=composed, the E-step kernel on row chunks into a scratch block
 * of at most 256 MB); nothing the handle holds from earlier calls (E-step results, records, label history, the statistics pass's call
 * history) is changed. A device group scores every shard's rows; a row-sharded job needs no communication. Arguments are checked
 * as by mlhip_em_expectation. */
int mlhip_em_score(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, int covariance_type,
                   const double* mixing, const double* means, const double* covariances,
                   double* log_density, uint32_t* labels);

/* EXTENSION (scikit-learn's GaussianMixture.sample; not in the reference surface): rows [first_row, first_row + n) of THE sample that a
 * seed and a mixture define, drawn on the device. Row i (its 64-bit global index) is a pure function of (seed, i), so the result does
 * not depend on the grid, on how a sample is cut into calls (first_row), on the chunks a call runs in or on the shards of a device
 * group, bit for bit. Definition -- Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl increments 0x9E3779B9, 0xBB67AE85), key
 * (seed & 0xffffffff, seed >> 32), counter (i & 0xffffffff, i >> 32, block, 0), output words w0..w3, U(lo, hi) = (((hi 2^32 + lo) >> 12)
 * + 1/2) 2^-52 (exact in fp64, strictly inside (0, 1)):
 *   label   (block 0): u = U(w0, w1); s_k the sequential fp64 prefix sums of `mixing`, t_k = s_k / s_{K-1}; label = #{k < K-1 : u >= t_k}
 *           (a component of weight 0 is never drawn, the last component absorbs the rounding);
 *   normals (block 1 + p, p = 0 .. ceil(d/2) - 1): u1 = U(w0, w1), u2 = U(w2, w3), r = sqrt(-2 log u1), z_2p = r cos(2 pi u2),
 *           z_2p+1 = r sin(2 pi u2) (for odd d the last value is dropped);
 *   row:    x_j = mu_kj + sum_{c <= j} L_k[j][c] z_c with L_k the lower Cholesky factor of Sigma_k (mlhip_cholesky_lower), evaluated as
 *           acc = mu_j, then acc = fma(L_jc, z_c, acc) for c = 0 .. j, on every route.
 * covariance_type and the layouts of mixing / means / covariances as in mlhip_em_score: diagonal input (L = sqrt(variance)) gives the
 * bits of the same variances passed as full diagonal matrices, tied input (one factor) those of K copies. A matrix that is not
 * positive definite: MLHIP_E_DOMAIN. x: n rows of d doubles, `ld` doubles apart; labels: n; either may be NULL, not both. The rows are
 * generated in chunks into a block from the context's pool (64 MiB; MLHIP_SAMPLE_ROWS=rows overrides) and copied down. A device group:
 * shard s draws its rows of the balanced split of mlhip_data_upload on its own GPU. The model's own random engine is not involved.
 * MLHIP_E_INVALID_ARGUMENT, before any device work: null pointers, K = 0, d = 0 or d > 4096, a bad covariance_type, a negative or
 * non-finite mixing weight or a total that is not positive, non-finite means, first_row + n beyond 64 bits, ld < d. n = 0 succeeds
 * and writes nothing. */
int mlhip_em_sample(mlhip_ctx* ctx, uint32_t d, uint32_t K, int covariance_type,
                    const double* mixing, const double* means, const double* covariances,
                    uint64_t seed, uint64_t first_row, uint64_t n, double* x, int64_t ld, uint32_t* labels);
/* The same rows as a resident block: generated sample-major into a pool buffer, they become a handle by the path of
 * mlhip_data_upload_dev and never leave the device; the handle is what mlhip_data_upload returns for the host copy of the same rows
 * (a device group's: assembled from the parts its shards drew themselves). labels (n, host) may be NULL. Also
 * MLHIP_E_INVALID_ARGUMENT: n beyond the per-rank row limit of mlhip_data_upload. n = 0: an empty block, as an empty upload. */
int mlhip_em_sample_data(mlhip_ctx* ctx, uint32_t d, uint32_t K, int covariance_type,
                         const double* mixing, const double* means, const double* covariances,
                         uint64_t seed, uint64_t first_row, uint64_t n, uint32_t* labels, mlhip_data** out);
/* Host helper, no GPU needed: the lower Cholesky factor the sampler uses (and a fit's records are built from), column-major d x d,
 * upper triangle zero. 1 <= d <= 4096; MLHIP_E_DOMAIN when the matrix is not positive definite. */
int mlhip_cholesky_lower(uint32_t d, const double* covariance, double* lower);
/* Which kernel the sampling calls run for K components in d dimensions (diagnostic, nothing is launched), under the switches as they
 * are set now. d <= 64: lane = row with the normals in registers, the wave's 64 x d tile staged through LDS and written as contiguous
 * 16 bytes per lane; the factors and means are read per lane from LDS (MLHIP_SAMPLE_LDS_TABLE) where the K (d (d+1)/2 + d) doubles of a
 * full model fit into the 64 KiB of a workgroup beside the staging tile (4 / 2 / 1 waves of 64 x (d | 1) doubles at d <= 16 / 32 / 64)
 * and the K thresholds, else -- and under MLHIP_SAMPLE_TABLE=global -- from global memory (MLHIP_SAMPLE_GLOBAL_TABLE; same bits).
 * 64 < d <= 4096: the plain tier (MLHIP_SAMPLE_PLAIN), normals into the output row and the product in place there. */
enum { MLHIP_SAMPLE_LDS_TABLE = 0, MLHIP_SAMPLE_GLOBAL_TABLE = 1, MLHIP_SAMPLE_PLAIN = 2 };
int mlhip_em_sample_route(uint32_t d, uint32_t K, int* kernel);

/* EXTENSION (Gaussian-mixture regression / imputation; not in the reference surface): a mixture over (x_O, x_M) conditioned on the
 * observed block. Host helper, no GPU needed. `observed`: n_observed distinct coordinates < d in any order, 1 <= n_observed <= d - 1
 * (column c of an observed row holds coordinate observed[c]); the missing coordinates M are the complement in ascending order, dM =
 * d - n_observed of them. means: K x d; covariances as in mlhip_em_score (diagonal and tied input count as the full matrices they
 * stand for). Outputs, per component k:
 *   means_observed       K x dO                  mu_k[O_c]
 *   covariances_observed K x dO x dO, full       Sigma_k,OO
 *   maps                 K x dM x dO, row-major  A_k = Sigma_k,MO Sigma_k,OO^-1, row j = missing coordinate j, computed as
 *                                                A_k = (L^-T (L^-1 Sigma_k,OM))^T with L L^T = Sigma_k,OO (mlhip_cholesky_lower's factor)
 *   means_missing        K x dM                  mu_k[M_j]
 * Diagonal input gives maps of +0.0, tied input K maps with equal bits. MLHIP_E_DOMAIN when a Sigma_k,OO is not positive definite.
 * MLHIP_E_INVALID_ARGUMENT, before any work: null pointers, K = 0, d = 0 or d > 4096, a bad covariance_type, n_observed = 0 or >= d,
 * a coordinate >= d, a coordinate given twice. */
int mlhip_em_condition(uint32_t d, uint32_t K, int covariance_type, const double* means, const double* covariances,
                       const uint32_t* observed, uint32_t n_observed,
                       double* means_observed, double* covariances_observed, double* maps, double* means_missing);
/* E[x_M | x_O] for every row of `data`, a resident block of the OBSERVED coordinates (its d is dO), under the conditioned mixture
 * mlhip_em_condition returns (mixing: the K weights of the joint model). With lw_k = log pi_k + log N(x_O | mu_k,O, Sigma_k,OO),
 * lse = log sum_k exp lw_k and r_k = exp(lw_k - lse):   out_j = sum_k r_k (mu_k,M[j] + sum_c A_k[j][c] (x_c - mu_k,O[c])).
 * The marginal mixture's E-step runs in its exact form on chunks of whole 256-row tiles (the kernels and the chunking of
 * mlhip_em_score's composed route; MLHIP_CONDITION_ROWS=rows overrides the chunk, rounded up to whole tiles) and the conditioning
 * kernel finishes each chunk in a fixed order: z_c = x_c - mu_k,O[c]; t_j = mu_k,M[j], t_j = fma(A_k[j][c], z_c, t_j) for ascending
 * c; y_j = +0.0, y_j = fma(r_k, t_j, y_j) for ascending k over the components with r_k != 0. A row's output is a pure function of
 * the row and the parameters: chunks, the row's place in the block and the shards of a device group (each conditions its own rows,
 * no collective) change no bit. out: rows x dM, `ld_out` >= dM doubles apart, host memory. log_density (rows; may be NULL):
 * lse - dO log(2 pi) / 2, the log-density of x_O under the marginal mixture -- the bits mlhip_em_score gives on its composed route.
 * Row weights are ignored, as in scoring; nothing the handle holds is changed. n = 0 succeeds and writes nothing. */
int mlhip_em_conditional_means(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, uint32_t dM, const double* mixing,
                               const double* means_observed, const double* covariances_observed, const double* maps,
                               const double* means_missing, double* out, int64_t ld_out, double* log_density);
/* Which conditioning kernel mlhip_em_conditional_means runs behind the E-step for dM missing coordinates on this block (diagnostic,
 * nothing is launched), under the switches as they are set now. dO <= 32 and dM <= 32: lane = row, x_O and the dM accumulators in
 * registers, the maps fed as scalar operands, the wave's 64 x dM tile staged through LDS into contiguous 16-byte stores
 * (MLHIP_CONDITION_REGISTERS); else, up to dO + dM = 4096, and everywhere under MLHIP_CONDITION=plain: table and accumulators in
 * global memory (MLHIP_CONDITION_PLAIN; same bits). MLHIP_CONDITION_SKIP=0 makes the kernels run the components that no row of a wave
 * has a share in (same bits). */
enum { MLHIP_CONDITION_REGISTERS = 0, MLHIP_CONDITION_PLAIN = 1 };
int mlhip_em_condition_route(const mlhip_data* data, uint32_t K, uint32_t dM, int* kernel);

/* EXTENSION (imputation of a table with gaps; not in the reference surface): every NaN of x replaced by its conditional expectation
 * under the mixture, every row conditioned on the coordinates IT has. x: n rows of d doubles, contiguous, HOST memory (a block with
 * NaNs has no usable shift, so it is no mlhip_data); a NaN of any sign and payload marks a missing coordinate. mixing, means,
 * covariances, covariance_type as in mlhip_em_score (diagonal and tied input count as the full matrices they stand for). out: n x d,
 * contiguous, host memory; log_density (n) and responsibilities (n x K, row-major) may be NULL.
 * Row i has the observed coordinates O ascending (c = 0 .. dO - 1) and the missing ones M ascending. For component k, L L^T = Sigma_k,OO,
 * W = L^-1 and A_k = Sigma_k,MO Sigma_k,OO^-1 (mlhip_em_condition's). Then
 *   1. z_c = x_c - mu_k,O[c];
 *   2. y_j = W[j][0] z_0, then fma over l = 1 .. j ascending; q = +0.0, then fma(y_j, y_j, q) for ascending j;
 *   3. lw_k = fma(-0.5, q, coef_k), coef_k = log pi_k - sum_j log L_jj;
 *   4. lse = the online log-sum-exp over ascending k of the E-step kernel; log_density = lse - dO log(2 pi) / 2;
 *   5. r_k = exp(lw_k - lse) (the E-step's exp of a non-positive argument): the responsibilities;
 *   6. t_j = mu_k,M[j], then fma(A_k[j][c], z_c, t_j) for ascending c; out_j = +0.0, then fma(r_k, t_j, out_j) for ascending k, ONLY
 *      where r_k != 0.
 * -- the exact E-step of the marginal mixture over x_O and the conditioning chain of mlhip_em_conditional_means, with the parameters
 * of the row's own pattern. An observed entry keeps its bits. A complete row: out is the input, log_density has the bits of
 * mlhip_em_score, the responsibilities are those of the exact E-step. A row of all NaN: out_j = +0.0, then fma(pi_k, mu_k[j], out_j) for
 * ascending k where pi_k != 0; log_density = 0; responsibilities = pi.
 * Row i's results are a pure function of row i and the parameters: the other rows, their order, how a table is cut into calls, the
 * row chunk (MLHIP_IMPUTE_ROWS=n), the pattern chunk (MLHIP_IMPUTE_PATTERNS=n), the shards of a device group (each imputes its own
 * rows, no collective; with an all-reduce hook installed every rank imputes its own rows, and no collective is made either) and
 * MLHIP_CONDITION_SKIP change no bit on a route. The rows are grouped by pattern on the host (mlhip_em_impute_plan); the complete rows
 * go through mlhip_em_score, the rows of all NaN are formed on the host. The others:
 *   COMPOSED (MLHIP_IMPUTE_COMPOSED), every d up to 4096: every group goes through the pass of mlhip_em_conditional_means with
 *            `observed` ascending and the model conditioned on the host -- bit for bit what that call gives for the group's rows, output
 *            and log-density. Its cost grows with the number of patterns: one upload, one host conditioning and two launches each.
 *   KERNEL   (MLHIP_IMPUTE_KERNEL), 2 <= d <= 32 and any K, the default there (MLHIP_IMPUTE=composed: COMPOSED): the records
 *            [mu_O | mu_M | A^T | W | coef] of the patterns are built on the device, one wave per (pattern, component)
 *            (device/em_impute_records.hip), for as many patterns at a time as 256 MiB hold; the evaluation kernel
 *            (device/em_impute.hip) then runs steps 1 - 6 with lane = row on 64-row tiles of ONE pattern each, one launch per pair
 *            of register paddings (4 / 8 / 16 / 32 for dO and dM) present in a chunk of rows: the launches do not grow with the
 *            patterns. The device's factorization is not the host's: the two routes agree within the sum of their error limits
 *            (DESIGN.md), not bit for bit.
 * MLHIP_E_DOMAIN where the Sigma_k,OO of some pattern of the block is not positive definite (mlhip_em_condition's error): NO output
 * is written, and the context stays usable. MLHIP_E_INVALID_ARGUMENT, before any device work: null pointers, K = 0, d = 0 or
 * d > 4096, a bad covariance_type, n >= 2^32 - 256. n = 0 succeeds and writes nothing. */
enum { MLHIP_IMPUTE_COMPOSED = 0, MLHIP_IMPUTE_KERNEL = 1 };
int mlhip_em_impute(mlhip_ctx* ctx, uint32_t d, uint32_t K, int covariance_type, const double* mixing, const double* means,
                    const double* covariances, const double* x, uint64_t n, double* out, double* log_density,
                    double* responsibilities);
/* The pattern grouping of a block, as mlhip_em_impute makes it (host only, no GPU): *n_patterns distinct patterns of observed
 * coordinates; order (n; may be NULL): the rows in a stable order in which the rows of one pattern are contiguous and ascending;
 * bounds (room for n + 1, *n_patterns + 1 written; may be NULL): pattern p holds order[bounds[p] .. bounds[p + 1]); n_observed (room
 * for n, *n_patterns written; may be NULL): the observed coordinates of pattern p. The patterns stand in ascending order of their masks
 * (bit c set: coordinate c observed; 64-bit words compared from coordinates 0 .. 63 on). */
int mlhip_em_impute_plan(const double* x, uint64_t n, uint32_t d, uint32_t* n_patterns, uint32_t* order, uint32_t* bounds,
                         uint32_t* n_observed);
/* The route mlhip_em_impute takes for a d-dimensional model of K components under the switches as they are set now, and -- launches
 * not NULL -- the kernel launches it makes behind the uploads for the block x (diagnostic, host only, nothing is launched). COMPOSED:
 * per group of at most MLHIP_IMPUTE_ROWS rows of one pattern one E-step and one conditioning kernel (a group larger than the
 * conditioning pass's scratch bound takes more). KERNEL: one records launch per pattern chunk and, per chunk of rows, one evaluation
 * launch per pair of paddings present -- the same count for 3 and for 300 patterns of the same paddings. Both: one scoring kernel per
 * group of complete rows. x may be NULL where launches is. */
int mlhip_em_impute_route(uint32_t d, uint32_t K, const double* x, uint64_t n, int* route, uint64_t* launches);
/* The records the KERNEL route builds on the device for ONE pattern, downloaded in mlhip_em_condition's layout (diagnostic; d <= 32,
 * a single context): observed: n_observed ASCENDING coordinates, 1 <= n_observed <= d - 1. means_observed K x dO; whitening K x dO x dO
 * row-major, W_k = L^-1 with L L^T = Sigma_k,OO, zero above the diagonal; coefficients K, log pi_k - sum_j log L_jj; maps K x dM x dO
 * row-major, A_k; means_missing K x dM. MLHIP_E_DOMAIN where a Sigma_k,OO is not positive definite (the kernel's flag word);
 * mlhip_em_condition's argument errors. */
int mlhip_em_impute_condition(mlhip_ctx* ctx, uint32_t d, uint32_t K, int covariance_type, const double* mixing, const double* means,
                              const double* covariances, const uint32_t* observed, uint32_t n_observed, double* means_observed,
                              double* whitening, double* coefficients, double* maps, double* means_missing);

/* EXTENSION (multiple imputation, predictive intervals; not in the reference surface): the covariances of the conditioned
 * components. Host helper, no GPU needed; d, K, covariance_type, covariances, observed, n_observed as in mlhip_em_condition, whose
 * argument checks are made here too, before any work. Per component k, with L L^T = Sigma_k,OO (the factor mlhip_em_condition uses)
 * and Y = L^-1 Sigma_k,OM (its forward substitution):
 *   covariances_missing  K x dM x dM             C_k = Sigma_k,M|O = Sigma_k,MM - Y^T Y; entry (a, b), b <= a, is Sigma_k[M_a][M_b] less
 *                                                Y[l][a] Y[l][b] for ascending l, and (b, a) a copy of it: symmetric by construction
 *   factors              K x dM x dM, row-major  G_k = the lower Cholesky factor of C_k (mlhip_cholesky_lower's), row j, column c at
 *                                                j dM + c, +0.0 above the diagonal; may be NULL
 * Diagonal input gives C_k = diag(sigma^2_M) and G_k = diag(sqrt(sigma^2_M)) exactly, tied input K copies with equal bits.
 * MLHIP_E_DOMAIN when a Sigma_k,OO or a C_k is not positive definite. */
int mlhip_em_condition_covariances(uint32_t d, uint32_t K, int covariance_type, const double* covariances, const uint32_t* observed,
                                   uint32_t n_observed, double* covariances_missing, double* factors);
/* Draws from p(x_M | x_O) for every row of `data`, a resident block of the OBSERVED coordinates (its d is dO), under the conditioned
 * mixture of mlhip_em_condition (mixing: the K weights of the joint model) and the factors G_k of mlhip_em_condition_covariances,
 * for the draws q = first_draw .. first_draw + n_draws - 1. Row i below is the row's GLOBAL index: first_row + its index in the block.
 *   Responsibilities  r_k = exp(lw_k - lse) from the marginal mixture's exact E-step, the values mlhip_em_conditional_means weights with.
 *   Label             Philox4x32-10 as in mlhip_em_sample, the same key, counter (i lo, i hi, 0, 1 + q); u = U(w0, w1); s_k the
 *                     sequential fp64 prefix sums of r_k for ascending k, S = s_{K-1}; label = the smallest k with u S < s_k (one
 *                     fp64 product); if there is none, the largest k with r_k != 0. A component with r_k = 0 has s_k = s_{k-1} and
 *                     is never drawn. A row whose S is a NaN gives a NaN in every coordinate and the label 0xFFFFFFFF.
 *   Normals           counter (i lo, i hi, 1 + p, 1 + q), p = 0 .. ceil(dM / 2) - 1; Box-Muller exactly as in mlhip_em_sample gives
 *                     zeta_0 .. zeta_{dM-1}.
 *   Row               with k = label: z_c = x_c - mu_k,O[c]; t_j = mu_k,M[j], t_j = fma(A_k[j][c], z_c, t_j) for ascending c (the
 *                     chain of mlhip_em_conditional_means); then t_j = fma(G_k[j][c], zeta_c, t_j) for c = 0 .. j; x~_j = t_j.
 * The fourth counter word is 1 + q and never 0, the word of mlhip_em_sample: data generated with a seed and imputed with the same
 * seed share no random word. Hence first_draw + n_draws <= 2^32 - 1. Row (i, q) is a pure function of (seed, i, q), the row's x_O
 * and the parameters: the grid, the chunks (those of mlhip_em_conditional_means: whole 256-row tiles, MLHIP_CONDITION_ROWS=rows
 * overrides; the draws go through in groups so that a chunk's scratch keeps that call's bound), the row's place in the block, how a
 * call is split over first_row or first_draw, the shards of a device group (each draws for its own rows under their global indices,
 * no collective) and the kernel tier change no bit.
 * out: n_draws blocks of rows x dM, draw-major, a row `ld_out` >= dM doubles after the one before and a block rows x ld_out doubles
 * after the one before, host memory. labels (n_draws x rows, may be NULL): the component every row was drawn from. Row weights are
 * ignored, as in scoring; nothing the handle holds is changed. n = 0 or n_draws = 0 succeeds and writes nothing. */
int mlhip_em_conditional_samples(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, uint32_t dM, const double* mixing,
                                 const double* means_observed, const double* covariances_observed, const double* maps,
                                 const double* means_missing, const double* factors, uint64_t seed, uint64_t first_row,
                                 uint32_t first_draw, uint32_t n_draws, double* out, int64_t ld_out, uint32_t* labels);
/* Which kernel mlhip_em_conditional_samples runs behind the E-step for dM missing coordinates on this block (diagnostic, nothing is
 * launched), under the switches as they are set now: the tiers of mlhip_em_condition_route. MLHIP_CONDITION_REGISTERS (dO <= 32 and
 * dM <= 32): lane = row, x_O, the chain and the normals in registers, maps and factor fed as scalar operands, only the components
 * some row of a wave drew are run, the wave's 64 x dM tile staged through LDS into contiguous 16-byte stores; MLHIP_CONDITION_PLAIN
 * (else, up to dO + dM = 4096, and everywhere under MLHIP_CONDITION=plain): thread = row, table from global memory; same bits. */
int mlhip_em_conditional_sample_route(const mlhip_data* data, uint32_t K, uint32_t dM, int* kernel);

/* EXTENSION (error bars on an imputed value, heteroscedastic regression bands; not in the reference surface): the PER-ROW predictive
 * covariance Var[x_M | x_O] for every row of `data`, a resident block of the OBSERVED coordinates (its d is dO), under the conditioned
 * mixture of mlhip_em_condition (mixing: the K weights of the joint model) and covariances_missing = the C_k of
 * mlhip_em_condition_covariances (K x dM x dM; only the lower triangle and the diagonal are read):
 *     Var[x_M | x_O] = sum_k r_k (C_k + (t_k - y)(t_k - y)^T),   t_k = mu_k,M + A_k (x_O - mu_k,O),   y = sum_k r_k t_k.
 * Per row, on every tier, with r_k = exp(lw_k - lse) from the marginal mixture's exact E-step (the values, the chunks and the switches
 * of mlhip_em_conditional_means), in this fixed order:
 *   Pass 1  steps 1 - 4 of mlhip_em_conditional_means unchanged: z_c = x_c - mu_k,O[c]; t_j = mu_k,M[j], t_j = fma(A_k[j][c], z_c, t_j)
 *           for ascending c; y_j = +0.0, y_j = fma(r_k, t_j, y_j) for ascending k over the components with r_k != 0. y_j has the bits
 *           mlhip_em_conditional_means gives.
 *   Pass 2  for ascending k, ONLY where r_k != 0: t_j by the same chain (the same bits as in pass 1); u_j = t_j - y_j; then
 *             diagonal form (full = 0)  s_j = fma(u_j, u_j, C_k[j][j]);           v_j  = fma(r_k, s_j, v_j),  from v_j  = +0.0;
 *             full form     (full = 1)  s = fma(u_a, u_b, C_k[a][b]) for b <= a;  V_ab = fma(r_k, s, V_ab),   from V_ab = +0.0;
 *                                       V_ba is a copy of V_ab.
 * Consequences: the diagonal of the full form has the bits of the diagonal form; the full form is exactly symmetric; the centred sum
 * cannot go below zero on the diagonal (it does not cancel the way sum_k r_k (C_k + t_k t_k^T) - y y^T does); a component with r_k = 0
 * leaves v as it is, as step 4 of the mean does, so the kernels' wave-level skip changes no bit (MLHIP_CONDITION_SKIP=0: same bits).
 * sum_k r_k is whatever the E-step gives: NOTHING IS RENORMALISED, in y or in v. A row's result is a pure function of the row and the
 * parameters: the chunks (whole 256-row tiles sized for the K log-responsibilities plus this call's outputs per row;
 * MLHIP_CONDITION_ROWS=rows overrides), the row's place in the block, a prefix of a longer block, the shards of a device group (each
 * conditions its own rows, no collective), the skip and the kernel tier change no bit.
 * variances: rows x dM doubles, or with full = 1 rows x dM*dM (row i holds V row-major), a row `ld_variances` >= dM (dM*dM) doubles
 * after the one before, host memory. means_out (rows x dM, `ld_means` >= dM apart; may be NULL) and log_density (rows; may be NULL)
 * carry the bits of mlhip_em_conditional_means' out and log_density. Row weights are ignored, as in scoring; nothing the handle holds
 * is changed (the call's own device scratch is at least 256 rows of K + its outputs per row: dM * dM doubles a row in the full form).
 * n = 0 succeeds and writes nothing. MLHIP_E_INVALID_ARGUMENT, before any device work: null pointers, K = 0, dM = 0, dO + dM > 4096,
 * full other than 0 / 1, a leading dimension below its row. */
int mlhip_em_conditional_variances(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, uint32_t dM, const double* mixing,
                                   const double* means_observed, const double* covariances_observed, const double* maps,
                                   const double* means_missing, const double* covariances_missing, int full, double* variances,
                                   int64_t ld_variances, double* means_out, int64_t ld_means, double* log_density);
/* Which kernel mlhip_em_conditional_variances runs behind the E-step for dM missing coordinates on this block in the form asked for
 * (diagnostic, nothing is launched), under the switches as they are set now. MLHIP_CONDITION_REGISTERS: lane = row, x_O, t, y and the
 * accumulators in registers, mu, A and C fed as scalar operands, the wave's output staged through LDS into contiguous 16-byte stores
 * -- the diagonal form at dO <= 32 and dM <= 32, the full form at dO <= 32 up to the largest dM whose dM (dM + 1) / 2 accumulators the
 * compiler keeps in registers without scratch (this function is where that bound is read; profiles/condition_variance_registers.txt
 * holds the report). MLHIP_CONDITION_PLAIN (else, up to dO + dM = 4096, and everywhere under MLHIP_CONDITION=plain): thread = row, the
 * output row is the accumulator, table from global memory; same bits. */
int mlhip_em_condition_variance_route(const mlhip_data* data, uint32_t K, uint32_t dM, int full, int* kernel);

/* EXTENSION (exact predictive intervals, medians, exceedance probabilities, the probability integral transform; not in the reference
 * surface). Host helpers, no GPU needed: the standard normal CDF the kernels below use (device/normal_cdf.hpp, the same text on host
 * and device: Phi(-t) = exp(-t^2/2) y P(s), one form for every argument, no table and no library call; relative error <= 6.01e-16
 * against a 40-digit reference wherever the result is a normal number, <= 1.84 spacings of the subnormals below; Phi(-inf) = 0,
 * Phi(+inf) = 1, Phi(0) = 0.5, NaN -> NaN; n values each) and its inverse (a rational start and four Halley steps on that CDF; odd
 * about 0.5 wherever 1 - p is a double; mlhip_normal_quantile(0.5) = +0.0; MLHIP_E_INVALID_ARGUMENT for a probability that is a
 * NaN or not strictly inside (0, 1)). */
int mlhip_normal_cdf(const double* a, uint64_t n, double* out);
int mlhip_normal_quantile(const double* p, uint64_t n, double* out);
/* Host helper, no GPU needed: from covariances_missing = the C_k of mlhip_em_condition_covariances (K x dM x dM; only the diagonal is
 * read) the two K x dM arrays the calls below take: scales s_kj = sqrt(C_k[j][j]) and inverse_scales w_kj = 1.0 / s_kj (one fp64
 * sqrt, one fp64 division). Diagonal input to mlhip_em_condition_covariances gives sqrt(sigma^2_M) exactly. MLHIP_E_DOMAIN where a
 * C_k[j][j] is <= 0 or not finite. */
int mlhip_em_condition_scales(uint32_t K, uint32_t dM, const double* covariances_missing, double* scales, double* inverse_scales);
/* Under the conditioned mixture of mlhip_em_condition (mixing: the K weights of the joint model), coordinate j of x_M given x_O follows
 * the ONE-DIMENSIONAL mixture sum_k r_k N(t_kj, s_kj^2): t_k = mu_k,M + A_k (x_O - mu_k,O), r_k = exp_nonpos(lw_k - lse) from the
 * marginal mixture's exact E-step (the values, the chunks and the switches of mlhip_em_conditional_means), s and w from
 * mlhip_em_condition_scales. `data` is a resident block of the OBSERVED coordinates (its d is dO). Per row, on every tier, with t_kj by
 * the chain of mlhip_em_conditional_means (z_c = x_c - mu_k,O[c]; t_j = mu_k,M[j], t_j = fma(A_k[j][c], z_c, t_j) for ascending c):
 *   mlhip_em_conditional_cdfs   P(x_j <= v_j | x_O) at the row's own value v_j per missing coordinate (values: rows x dM, `ld_values`
 *       apart): for ascending k, ONLY where r_k != 0:  a = (v_j - t_kj) * w_kj;  F_j = fma(r_k, normal_cdf(a), F_j), from F_j = +0.0.
 *       A NaN row or a NaN value gives NaN. out: rows x dM, `ld_out` >= dM apart.
 *   mlhip_em_conditional_quantiles   the v with F_j(v) = p S for every probability p (n_probabilities of them, each strictly inside
 *       (0, 1)); z = mlhip_normal_quantile(p) on the host. S = the sequential fp64 sum of r_k for ascending k from +0.0 (the s_{K-1} of
 *       mlhip_em_conditional_samples); T = p * S. Over the components with r_k != 0, ascending k: q_k = fma(s_kj, z, t_kj); lo = min
 *       q_k, hi = max q_k (the mixture's quantile lies between its components'; a NaN q_k makes both NaN); g = fma(r_k, q_k, g) from
 *       +0.0. Start: v = g / S clamped into [lo, hi] (the weighted mean of the q_k leaves it only by rounding) -- the ends included: a
 *       row with one dominant component has its answer ON an end (g / S is that component's own quantile), and an end is not
 *       evaluated otherwise. Where lo == hi -- K = 1, a row with one share, p = 0.5 with equal t_kj -- the result is lo and no trip is
 *       made; it is NaN where lo or T is a NaN or no component has a share. Else the bracket is widened to [lo - e, hi + e],
 *       e = 2^-50 max(|lo|, |hi|) (a candidate on an end, or a few roundings beyond it, is strictly inside), and trips n = 1, 2, ...:
 *         F = F_j(v) as above, f = sum_k fma(r_k, w_kj * normal_pdf(a), f) from +0.0, normal_pdf(a) = exp_nonpos(-0.5 * (t * t)) *
 *         3.98942280401432677940e-01 with t = min(|a|, 40) (a product by the rounded 1 / sqrt(2 pi), no division; NaN for a NaN);
 *         if F < T then lo = v else hi = v;
 *         the Newton candidate, taken on the logarithm of the nearer tail (near the root it is the plain Newton step; far out in a
 *         tail it neither creeps nor flies off):  c = v + log(T / F) * (F / f) if T + T < S (or T + T == S and F < T), else
 *         c = v - log((S - T) / (S - F)) * ((S - F) / f)   (log: the device library's);
 *         next = c if n <= 24 and lo < c < hi, else lo + (hi - lo) / 2;
 *         STOP with the result v (the last point evaluated) if |F - T| <= 2^-50 T, or |c - v| <= 2^-51 |v|, or next is not strictly
 *         inside (lo, hi), or n == MLHIP_QUANTILE_MAX_TRIPS; else v = next.
 *       The cap holds whatever the data: from trip 25 on every trip is a bisection, so the last 60 trips alone cut the bracket to 2^-60
 *       of its width, below the rounding of the q_k that span it; the first stop rule says F is within the accuracy of a sum of
 *       normal_cdf values, the second that the step is below v's own rounding, the third that the bracket has no double left to try. p = 0.5 gives z = +0.0 and q_k = t_kj exactly, so K
 *       = 1 returns the bits of mlhip_em_conditional_means there. A coordinate's search is a pure function of (row, parameters, p); the
 *       kernels run the dM coordinates of 64 rows in lock-step until none is left, and a coordinate that has stopped is not written
 *       again. out: n_probabilities blocks of rows x dM, probability-major, a row `ld_out` >= dM doubles after the one before and a
 *       block rows x ld_out doubles after the one before (the layout of mlhip_em_conditional_samples' draws). iterations (may be NULL):
 *       n_probabilities x rows x dM uint32, contiguous: the trips every output took (0 where no search ran). The probabilities go
 *       through in groups so that a chunk's scratch keeps the call's bound (MLHIP_CONDITION_GROUP=n: at most n per group): one launch per
 *       chunk and group.
 * means_out (rows x dM, `ld_means` >= dM apart; may be NULL) and log_density (rows; may be NULL) carry the bits of
 * mlhip_em_conditional_means' out and log_density. sum_k r_k is whatever the E-step gives: NOTHING IS RENORMALISED. A component with
 * r_k = 0 leaves every sum as it is, so the kernels' wave-level skip changes no bit (MLHIP_CONDITION_SKIP=0: same bits). A row's result
 * is a pure function of the row and the parameters: the chunks (whole 256-row tiles sized for the K log-responsibilities plus this
 * call's inputs and outputs per row; MLHIP_CONDITION_ROWS=rows overrides), the row's place in the block, a prefix of a longer block,
 * the shards of a device group (each handles its own rows, no collective), how the probabilities are grouped or split over calls, the
 * skip and the kernel tier change no bit. Row weights are ignored, as in scoring; nothing the handle holds is changed. n = 0 or
 * n_probabilities = 0 succeeds and writes nothing. MLHIP_E_INVALID_ARGUMENT, before any device work: null pointers, K = 0, dM = 0,
 * dO + dM > 4096, a leading dimension below its row, a probability that is a NaN or not strictly inside (0, 1). */
enum { MLHIP_QUANTILE_NEWTON_TRIPS = 24, MLHIP_QUANTILE_MAX_TRIPS = 84 };
int mlhip_em_conditional_cdfs(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, uint32_t dM, const double* mixing, const double* means_observed,
                              const double* covariances_observed, const double* maps, const double* means_missing, const double* scales,
                              const double* inverse_scales, const double* values, int64_t ld_values, double* out, int64_t ld_out,
                              double* means_out, int64_t ld_means, double* log_density);
int mlhip_em_conditional_quantiles(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, uint32_t dM, const double* mixing,
                                   const double* means_observed, const double* covariances_observed, const double* maps,
                                   const double* means_missing, const double* scales, const double* inverse_scales,
                                   const double* probabilities, uint32_t n_probabilities, double* out, int64_t ld_out, double* means_out,
                                   int64_t ld_means, double* log_density, uint32_t* iterations);
/* Which kernel mlhip_em_conditional_cdfs (quantile = 0) or mlhip_em_conditional_quantiles (quantile = 1) runs behind the E-step for dM
 * missing coordinates on this block (diagnostic, nothing is launched), under the switches as they are set now.
 * MLHIP_CONDITION_REGISTERS: lane = row, x_O, t and the per-coordinate state in registers, mu, A, s and w fed as scalar operands,
 * values in and results out through LDS as contiguous 16 bytes per lane -- the CDF at dO <= 32 and dM <= 32, the quantile search at
 * dO <= 32 up to the largest dM whose state (lo, hi, v, F, f and t per coordinate) the compiler keeps in registers without scratch
 * at every dO: dM <= 16 (profiles/condition_quantile_registers.txt holds the report). MLHIP_CONDITION_PLAIN (else, up to dO + dM =
 * 4096, and everywhere under MLHIP_CONDITION=plain): thread = row, table from global memory; same bits. */
int mlhip_em_condition_quantile_route(const mlhip_data* data, uint32_t K, uint32_t dM, int quantile, int* kernel);

/* (X - mean)(X - mean)^T / (N - 1) over ALL ranks' samples (EM::calculate_sample_covariance,
 * ML/EM.cpp:265-272). mean may be NULL. */
int mlhip_sample_covariance(mlhip_ctx* ctx, mlhip_data* data, double* mean, double* covariance);

/* X X^T (d x d, column-major) and X y (d) over ALL ranks' samples in one pass over the resident block: the dense
 * contraction of LinearRegression::calculate_XXt_beta (ML/LinearRegression.cpp:213-215), the "next" row f4 of SURVEY.md
 * section 8. `y` holds this rank's n_local target values. Runs on the statistics kernel (two weight rows: 1 and y). */
int mlhip_xxt_xy(mlhip_ctx* ctx, mlhip_data* data, const double* y, double* xxt, double* xy);

/* Host helpers, no GPU needed: the layout of the all-reduced sufficient statistics and the M-step closing
 * arithmetic applied to them (ML/EM.cpp:242, 250-257). Per component, F = (d+1)(d+2)/2 doubles: the packed lower
 * triangle (row-major: entry (a,b), a >= b, at a(a+1)/2 + b) of  sum_i r_ik xt_i xt_i^T  with
 * xt_i = [x_i - shift ; 1]; so S0 = (d,d), S1'_b = (d,b), M2'_ab = (a,b). `statistics` holds K such records. */
int mlhip_em_statistics_count(uint32_t d, uint32_t* count_per_component);
int mlhip_em_finalize_statistics(uint32_t d, uint32_t K, const double* statistics, const double* shift,
                                 double n_global, double* mixing_out, double* means_out, double* covariances_out);
/* Same with the covariance ridge given (mlhip_data_set_covariance_ridge: finite, >= 0, else MLHIP_E_INVALID_ARGUMENT); the function
 * above is this one at MLHIP_DEFAULT_COVARIANCE_RIDGE. */
int mlhip_em_finalize_statistics_ridge(uint32_t d, uint32_t K, const double* statistics, const double* shift, double n_global,
                                       double ridge, double* mixing_out, double* means_out, double* covariances_out);

/* The tied mode's counterpart (no GPU needed; the closing of both routes of mlhip_em_step_tied is this arithmetic). `statistics`: K
 * records of d + 1 doubles, [S1_k (d) | S0_k] with S1_k = sum_i w_i r_ik (x_i - shift); `total_scatter`: sum_i w_i xt_i xt_i^T,
 * xt_i = [x_i - shift ; 1], in the packed layout above (one component's record: (d+1)(d+2)/2 doubles; only the d x d part is read).
 * covariance_out: d*d doubles. */
int mlhip_em_finalize_statistics_tied(uint32_t d, uint32_t K, const double* statistics, const double* total_scatter, const double* shift,
                                      double total_weight, double* mixing_out, double* means_out, double* covariance_out);
/* Same with the covariance ridge given (added once); the function above is this one at MLHIP_DEFAULT_COVARIANCE_RIDGE. */
int mlhip_em_finalize_statistics_tied_ridge(uint32_t d, uint32_t K, const double* statistics, const double* total_scatter,
                                            const double* shift, double total_weight, double ridge, double* mixing_out,
                                            double* means_out, double* covariance_out);

/* Host helper, no GPU needed: covariance -> what EM::process_covariances (ML/EM.cpp:274-287) derives:
 * inverse (d*d), sqrt(det). Used by the facade for point queries (EM::assign_responsibilities). */
int mlhip_process_covariance(uint32_t d, const double* covariance, double* inverse, double* sqrt_det);

/* ---- K-means -------------------------------------------------------------------------------------- */
/* One Lloyd step == KMeans::assignment_step + the sums KMeans::update_step needs (ML/KMeans.cpp:167-192),
 * all-reduced across ranks.
 *   in : centroids[d*K]
 *   out: *inertia = sum_i min_k |x_i - c_k|^2 ; *n_changed = #labels differing from the previous call on
 *        this data (first call: n_global); counts[K]; centroids_out[d*K] = per-cluster means, an EMPTY cluster's
 *        centroid is the origin (:184). Labels stay on the device for mlhip_kmeans_labels. */
int mlhip_kmeans_step(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, const double* centroids,
                      double* inertia, uint64_t* n_changed, double* counts, double* centroids_out);
/* The step loop of KMeans::fit_once (ML/KMeans.cpp:80-110) in ONE call: up to max_steps trips of mlhip_kmeans_step with the
 * reference's two stopping rules -- the same labels as in the previous trip (:84-89; the centroids then stay as they are), or
 * from the second trip on a squared centroid shift |C - C_old|_F^2 below absolute_tolerance, followed by one more assignment
 * (:103-108). Between two tests everything stays on the device: the update's sums are all-reduced there, divided by the counts
 * (empty cluster -> origin, :184) and become the next trip's centroid table without a host round trip; the host reads back
 * 2 + K (d + 1) doubles per trip for the two tests. Same results, bit for bit, as the loop over mlhip_kmeans_step.
 *   in/out: centroids[d*K] (start -> final); out: old_centroids[d*K] (the table before the last update; may be NULL),
 *   counts[K] of the last update (may be NULL), *inertia of the last assignment, *steps_done, *converged. */
int mlhip_kmeans_iterate(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, double* centroids, double* old_centroids,
                         uint32_t max_steps, double absolute_tolerance, uint32_t* steps_done, int* converged,
                         double* inertia, double* counts);
/* Assignment only (KMeans::assignment_step, :167-178): labels + inertia, no update. */
int mlhip_kmeans_assign(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, const double* centroids,
                        double* inertia, uint64_t* n_changed);
/* EXTENSION (no counterpart in the reference): Lloyd's algorithm on a WEIGHTED sample -- the three calls above with the row weights
 * attached by mlhip_data_set_weights (MLHIP_E_INVALID_ARGUMENT without them), same signatures:
 *   *inertia = sum_i w_i min_k |x_i - c_k|^2 ; counts[k] = sum of the weights of cluster k's rows ; centroids_out = the weighted means
 *   sum_i w_i x_i / sum_i w_i per cluster, a cluster of total weight 0 (empty, or rows of weight 0 only) at the origin.
 * Labels, per-row distances (mlhip_kmeans_labels / _distances) and *n_changed (a count of ROWS) do not depend on the weights: they
 * are, bit for bit, those of the unweighted call -- the assignment kernel of the shape's route runs unchanged, without its own
 * accumulation, and one more sweep over X, the labels, the distances and the weights forms the sums (the weighted form of device/kmeans.hip's update sweep); the
 * weighted iterate never takes the one-launch resident loop. With integer weights the results are those of the unweighted calls on
 * the sample with row i repeated w_i times. The sums are exact sums of the rounded products w_i x_ij on a fixed-point grid set by the
 * largest weight and the largest |x_j| of the WHOLE sample (exchanged across ranks, cached on the handle until the weights change),
 * so they do not depend on the summation order, the grid or the number of shards; a product below 2^-94 max w max|x_j| contributes
 * nothing, likewise a weight below 2^-94 max w to the counts. MLHIP_E_DOMAIN when max w * max|x_j| overflows (the handle stays usable).
 * mlhip_kmeans_assign_weighted is the assignment plus an inertia-only sweep. */
int mlhip_kmeans_step_weighted(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, const double* centroids,
                               double* inertia, uint64_t* n_changed, double* counts, double* centroids_out);
int mlhip_kmeans_iterate_weighted(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, double* centroids, double* old_centroids,
                                  uint32_t max_steps, double absolute_tolerance, uint32_t* steps_done, int* converged,
                                  double* inertia, double* counts);
int mlhip_kmeans_assign_weighted(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, const double* centroids,
                                 double* inertia, uint64_t* n_changed);
int mlhip_kmeans_labels(mlhip_ctx* ctx, mlhip_data* data, uint32_t* labels);
/* Per-sample squared distance to the assigned centroid from the last assignment (n_local doubles): the very values
 * KMeans::assign_label returns (:153-165), so a caller can re-create the reference's sequential inertia sum (:176). */
int mlhip_kmeans_distances(mlhip_ctx* ctx, mlhip_data* data, double* dist2);
/* One draw of KPP::init (ML/Clustering.cpp:44-58) on the resident block(s): the weights become min(weights, |x_i - centroid|^2)
 * (first != 0: the distances themselves), and the row that std::discrete_distribution returns for the canonical uniform draw u is
 * located from tree-summed cumulative weights with a rigorous error bound. Row-sharded jobs: every rank calls it with the same
 * centroid and u and the global index of its first row (first_row; 0 on a single rank); the ranks exchange their weight sums and
 * candidates through the context's all-reduce. *certain != 0: *index is that row of the WHOLE sample, bit for bit what the
 * sequential sums of the reference give (the same on every rank). *certain == 0 (two rows closer than the bound, or a zero /
 * non-finite weight sum): this rank's weights have been copied to weights_out (n_local doubles; may be NULL) for the caller's
 * sequential evaluation. At least two rows in the whole sample. */
int mlhip_kpp_draw(mlhip_ctx* ctx, mlhip_data* data, const double* centroid, int first, double u, uint64_t first_row, uint64_t* index,
                   int* certain, double* weights_out);
/* The running-minimum weights the draws of mlhip_kpp_draw have left on the device (n_local doubles): fetched by the caller only when
 * a draw was not certain -- a certified draw never moves them (ML/Clustering.cpp:44-51 keeps them in a host vector). */
int mlhip_kpp_weights(mlhip_ctx* ctx, mlhip_data* data, double* weights_out);
/* One draw of FixedPointKPP (include/ML/Clustering.hpp; not the reference's KPP draws) on the resident block(s): the weights become
 * min(weights, |x_i - centroid|^2) (first != 0: the distances themselves; ascending-j fma chain), then with E the largest frexp
 * exponent of any weight of the WHOLE sample, q_i = floor(w_i 2^(52 - E)) and T = sum q_i (exact integers), *index is the smallest
 * row of the whole sample with q_0 + ... + q_i > floor(u T) -- or floor(u N) when T = 0. Every route (any number of ranks or shards,
 * the host restatement) gives the same row; only O(1) values per draw leave the device. Row-sharded jobs: every rank calls it with
 * the same centroid and u and the global index of its first row (first_row; 0 on a single rank); the ranks exchange their largest
 * exponents and integer totals through the context's all-reduce. MLHIP_E_INVALID_ARGUMENT on every rank when a weight is not
 * finite. */
int mlhip_kpp_draw_fixed_point(mlhip_ctx* ctx, mlhip_data* data, const double* centroid, int first, double u, uint64_t first_row,
                               uint64_t* index);
/* min_k |x_i - c_k|^2 per sample of this rank's shard (the weights of KPP::init, ML/Clustering.cpp:44-51). */
int mlhip_min_squared_distances(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, const double* centroids, double* dist2);

/* The running means of RandomPartition::init (ML/Clustering.cpp:27-37) over this rank's rows, bit-identical to the host loop
 * `c_k += (x_i - c_k) / ++n_k`: the caller makes the per-row cluster draws (the reference's std::uniform_int_distribution calls)
 * and passes their stable partition -- order[offsets[k] .. offsets[k+1]) = the local row indices drawn for cluster k, ascending;
 * offsets[0] = 0, offsets[K] = n_local. means (K x d, centroid k = d contiguous doubles: the reference's column-major d x K) and
 * sizes (K counts) are CONTINUED: zeros for a fresh start, the previous rank's result in a row-sharded job (ranks in row order). */
int mlhip_random_partition_means(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, const uint32_t* order, const uint32_t* offsets,
                                 double* means, double* sizes);

/* ---- silhouette -------------------------------------------------------------------------------------- */
/* Exact silhouette values of rows of the resident block under `labels` (Euclidean distance; every evaluated row against ALL rows of
 * the block): with n_c the rows labelled c and D_ic = sum_{j: l_j = c} |x_i - x_j| (j = i included: +0),
 *     a_i = D_{i,l_i} / (n_{l_i} - 1),   b_i = min over c != l_i with n_c > 0 of D_ic / n_c (the first minimum),
 *     s_i = (b_i - a_i) / max(a_i, b_i);
 * s_i = 0 and a_i = 0 for a row alone in its cluster, s_i = 0 where max(a_i, b_i) = 0 (scikit-learn's conventions); labels no row
 * carries are ignored. labels: one per row of the block, each < K -- this rank's rows; ALL rows of the sample on a device group.
 * rows: n_rows global row indices, in any order, repeats allowed; NULL: all rows in order (n_rows is then ignored). a_out / b_out /
 * s_out: one double per evaluated row, each may be NULL. Weights attached to the block play no part; coordinates that are not
 * finite are not looked for and come out as NaN wherever they enter.
 * The arithmetic is fixed: z = x_i - x_j (one rounding per coordinate), q = z_0 z_0, q = fma(z_j, z_j, q) for ascending j, the
 * distance sqrt(q) correctly rounded -- no expansion of the square, no matrix-core product. The columns j are taken cluster-sorted (a
 * stable counting sort of the rows by label), every cluster's run is cut into chunks of 256 columns, the distances of a chunk are
 * added one after the other and the chunk sums of a cluster in ascending order. A row's values are therefore a function of the data,
 * the labels and the block's shard layout alone: not of `rows`, the row blocks the call walks (sized so that the chunk sums stay
 * within the scoring routes' scratch bound; MLHIP_SILHOUETTE_ROWS=n overrides), the grid (MLHIP_SILHOUETTE_GRID=n), the tier
 * (MLHIP_SILHOUETTE=plain: the plain tier at every d) or the column feed (MLHIP_SILHOUETTE_FEED=lds / scalar).
 * Device group: every shard forms D_ic over its OWN columns by these rules (the evaluated rows' coordinates are collected from their
 * shards and given to all), the host adds the shards' sums in ascending shard order and closes; the values then depend on the shard
 * layout within rounding. A context that reduces through a caller's hook or RCCL ranks: MLHIP_E_UNSUPPORTED (a rank holds only its
 * own columns). MLHIP_E_INVALID_ARGUMENT, before any launch: null data or labels, a label >= K, a row index >= the sample's rows, or
 * fewer than two non-empty clusters. */
int mlhip_silhouette(mlhip_ctx* ctx, mlhip_data* data, uint32_t K, const uint32_t* labels, const uint64_t* rows, uint64_t n_rows,
                     double* a_out, double* b_out, double* s_out);
/* Which tier mlhip_silhouette runs on `data` under the switches as they are set now (diagnostic, nothing is launched): the register
 * tier for d <= 32, the plain tier above and under MLHIP_SILHOUETTE=plain. */
enum { MLHIP_SILHOUETTE_REGISTERS = 0, MLHIP_SILHOUETTE_PLAIN = 1 };
int mlhip_silhouette_route(const mlhip_data* data, int* tier);
/* The closing arithmetic of mlhip_silhouette for ONE row on the host (no GPU): counts: K cluster sizes, own_label < K the row's
 * label, D: its K sums of distances; a / b / s each may be NULL. MLHIP_E_INVALID_ARGUMENT: null counts or D, own_label >= K,
 * counts[own_label] = 0, or no other non-empty cluster. */
int mlhip_silhouette_finish(uint32_t K, const uint64_t* counts, uint32_t own_label, const double* D, double* a, double* b, double* s);

/* ---- timing (for bench.py / profiling) -------------------------------------------------------------- */
/* Average device time in ms of the named kernel family over its launches since the last reset, measured with
 * HIP events on the context's stream. name: "em_estep", "em_mstats", "em_score", "kmeans_assign", ... Returns count in *launches.
 * While enabled, every launch is bracketed by a pair of events that is only recorded; the times are read (one stream
 * synchronisation) when mlhip_timing_get / _reset / _enable(off) is called, so a timed region is not perturbed. */
int mlhip_timing_enable(mlhip_ctx* ctx, int on);
int mlhip_timing_reset(mlhip_ctx* ctx);
int mlhip_timing_get(mlhip_ctx* ctx, const char* name, double* avg_ms, uint64_t* launches);
/* Which kernels an EM iteration of K full-covariance components on `data` is made of (diagnostic: bench.py attributes the
 * algorithmic flops of ML/EM.cpp:190-263 to the kernels that execute them). Bits of *flags: */
#define MLHIP_PLAN_FUSED 1u          /* E-step + statistics in one kernel (small shapes, em_fused_small.hip) */
#define MLHIP_PLAN_MATRIX_ESTEP 2u   /* matrix-core E-step (em_estep_mfma4.hip), else the scalar-fed one */
#define MLHIP_PLAN_SELF_NORM 4u      /* the E-step writes log-responsibilities only; the statistics kernel normalises them
                                        (the one exponential per (sample, component) runs THERE) */
int mlhip_em_plan(const mlhip_data* data, uint32_t K, uint32_t* flags);

/* The whole route of one call (diagnostic; tests assert which kernel a case runs): what the library's routing decides, once
 * per entry-point call, from the block's shape, K and the MLHIP_* routing switches as they are set when this is called. Nothing
 * is launched. covariance_type: 0 full, 1 diagonal. A device group's block reports the route of its shards. Decisions taken
 * at launch -- sparse = -1, the resident loop's grid check, FOLD's per-iteration test against the parameters -- are not in here:
 * pin them by their switch or read the launch counters (mlhip_timing_get). */
enum { MLHIP_ESTEP_SCALAR_FED = 0, MLHIP_ESTEP_MATRIX4 = 1, MLHIP_ESTEP_BIG_DIM = 2, MLHIP_ESTEP_PLAIN = 3 };
enum { MLHIP_FUSED_LDS_FEED = 0, MLHIP_FUSED_SCALAR_FEED = 1, MLHIP_FUSED_VALU = 2 };
enum { MLHIP_KMEANS_DIRECT = 0, MLHIP_KMEANS_MATRIX = 1, MLHIP_KMEANS_BIG_DIM = 2, MLHIP_KMEANS_PLAIN = 3 };
typedef struct mlhip_em_route_info {
    int32_t estep;              /* MLHIP_ESTEP_* */
    int32_t fused;              /* E-step + statistics in one kernel */
    int32_t fused_form;         /* MLHIP_FUSED_* (meaningful when fused) */
    int32_t self_norm;          /* the statistics kernel normalises the log-responsibilities */
    int32_t sparse;             /* self-normalising statistics: 1 sparse kernel, 0 dense kernel, -1 by the call history */
    int32_t balanced;           /* d <= 32: the wide statistics kernel deals (column block, row block) units */
    int32_t fold_allowed;       /* the matrix-core E-step may take its FOLD form */
    int32_t diag_kernel;        /* covariance_type 1: the diagonal kernel exists for this (d, K) and runs */
    int32_t diag_exact;         /* diagonal mode: the exact density form always */
    int32_t device_close;       /* mlhip_em_iterate closes its iterations on the device */
    int32_t records_on_device;  /* d > 64: a fit's first records are factored on the device */
    int32_t resident;           /* mlhip_em_iterate may run the whole loop in one launch */
} mlhip_em_route_info;
typedef struct mlhip_kmeans_route_info {
    int32_t kernel;             /* MLHIP_KMEANS_* */
    int32_t pad;                /* the block runs on a copy zero-padded to a multiple of 4 dimensions */
    int32_t resident;           /* mlhip_kmeans_iterate runs the whole loop in one launch */
} mlhip_kmeans_route_info;
int mlhip_em_route(const mlhip_data* data, uint32_t K, int covariance_type, mlhip_em_route_info* out);
/* Which kernel mlhip_em_score runs for K components on `data` (diagnostic, nothing is launched): the scalar-fed score kernel and the
 * matrix-core E-step's SCORE form wherever mlhip_em_route reports MLHIP_ESTEP_SCALAR_FED / MLHIP_ESTEP_MATRIX4; composed above d = 128
 * and under MLHIP_SCORE=composed. */
enum { MLHIP_SCORE_SCALAR_FED = 0, MLHIP_SCORE_MATRIX4 = 1, MLHIP_SCORE_COMPOSED = 2 };
int mlhip_em_score_route(const mlhip_data* data, uint32_t K, int* kernel);
/* Which route mlhip_em_step_tied (and mlhip_em_iterate with MLHIP_COVARIANCE_TIED) takes for K components on `data` (diagnostic,
 * nothing is launched): the tied kernel for unweighted blocks with d <= 32, K <= 64 except where mlhip_em_route reports the fused kernel in its
 * vector-unit form (MLHIP_TIED=kernel: there too); composed elsewhere and under MLHIP_TIED=composed. */
enum { MLHIP_TIED_COMPOSED = 0, MLHIP_TIED_KERNEL = 1 };
int mlhip_em_tied_route(const mlhip_data* data, uint32_t K, int* kernel);
int mlhip_kmeans_route(const mlhip_data* data, uint32_t K, mlhip_kmeans_route_info* out);
/* The screened E-step (MLHIP_ESTEP_SCREEN; full covariances, 12 <= d <= 32, K <= 64, unweighted blocks) is chosen pass by pass at
 * launch. What the E-step passes of the fits on `data` did since the block was uploaded (diagnostic; tests assert the route a case
 * takes), summed over the shards of a device group: counts[0] passes that ran screened, counts[1] passes of the screened kernel's
 * domain that ran dense, counts[2] those among counts[1] that asked for the screened kernel and were sent back because a component's
 * bound carried no information, counts[3] the candidates (pairs evaluated) of the last screened pass. Waits for the stream. */
int mlhip_em_screen_counts(mlhip_ctx* ctx, mlhip_data* data, uint64_t counts[4]);

#ifdef __cplusplus
}
#endif
#endif /* MLHIP_H */
