/*
 * pcr_api.h -- C ABI of libpcr.so, the MI355X (gfx950) registration core.
 *
 * Plain pointers + sizes, no torch types.  Every pointer argument named as a
 * device buffer must be device (HBM) memory of the current HIP device; outputs
 * are caller-allocated (the reference's ownership rule,
 * dip/torch-nndistance/torch_nndistance/__init__.py:17-20,42-43).  Work is
 * enqueued on `stream` (a hipStream_t; NULL = legacy default stream, which is
 * what the reference launcher uses, nnd_cuda.cu:152-153) and is asynchronous
 * unless stated otherwise.
 *
 * Return value: PCR_OK (0) or a negative PCR_ERR_* code; pcr_last_error()
 * returns a thread-local message for the last failure.  (The reference CUDA
 * launcher prints and returns 0 / 1, nnd_cuda.cu:155-161; the Python layer
 * maps PCR_OK -> 1 and raises on failure.)
 *
 * Concurrency contract: scratch buffers come from a library-owned workspace
 * with one set of slots PER DEVICE (not per stream).  Calls for one device must
 * therefore be ordered: issue them on one stream at a time (or order the streams
 * with events), from any host thread.  Two libpcr calls running concurrently on
 * two streams of the same device would share scratch.  A slot that grows keeps
 * its previous buffer alive (HIP graphs captured earlier may still point at it);
 * pcr_workspace_release() frees every workspace buffer of the current device
 * after a device synchronize -- call it only when no captured graph that
 * contains libpcr kernels will be replayed again.
 */
#ifndef PCR_API_H
#define PCR_API_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCR_OK 0
#define PCR_ERR_ARG (-1)
#define PCR_ERR_HIP (-2)
#define PCR_ERR_NOMEM (-3)

typedef void *pcr_stream_t; /* hipStream_t */

const char *pcr_last_error(void);
int pcr_version(void);
int pcr_workspace_release(void);
/* end of process: synchronise every device the library used and free its
 * workspace, retired buffers and pooled profiling events (idempotent; the
 * library stays usable; a device that cannot be synchronised keeps its
 * buffers).  A HIP graph captured before it records freed buffers and must not
 * be replayed after it.  The Python layer runs it from atexit. */
int pcr_shutdown(void);
/* Concurrent sub-batches.  pcr_set_workspace_context(ctx) (thread-local, 0..3)
 * selects which copy of the library's scratch the calling thread's next calls
 * use: calls that run concurrently on different streams must use different
 * contexts.  pcr_set_concurrency(k) (1..4): k launches share the device, so
 * cooperative grids (ICP's workgroups per pair and its tail launch) are sized
 * to CUs / k and k of them can be resident at once. */
int pcr_set_workspace_context(int32_t ctx);
int pcr_set_concurrency(int32_t k);
/* Diagnostics: one trivial launch of `blocks` (1..256) 256-thread blocks,
 * cooperative or plain, writing out[b] = b -- nothing else of the library
 * (tools/exit_probe.py isolates an exit-time fault under the profiler). */
int pcr_coop_probe(int32_t *out, int32_t blocks, int32_t cooperative, pcr_stream_t stream);

/* Optional per-kernel timing with HIP events recorded on the launch stream
 * around the hot kernels (id 0 feature screen (pass 1), 1 nnd forward, 2 RANSAC verify,
 * 3 ICP, 4 RANSAC hypotheses, 5 feature rescan, 6 feature pack, 7 nnd grid query,
 * 8 feature screen pass 2, 9 / 10 the 3-term screens behind passes 1 / 2, 11 the 1-term
 * screens' regroup and finish, featnn_regroup9 / featnn_finish9).  pcr_profile_read synchronizes the pending
 * events and returns the accumulated milliseconds and launch count. */
void pcr_profile_enable(int32_t on);
int pcr_profile_read(int32_t id, double *total_ms, int64_t *count, int32_t reset);

/* Diagnostic: rows (src->tgt, tgt->src) that the feature-NN screen could not
 * certify and sent to the exact f64 rescan since the last reset.  Synchronizes
 * the device. */
int pcr_featnn_rescan_rows(int64_t *rows12, int64_t *rows21, int32_t reset);
/* Diagnostic: source rows (pass 1) and target columns of J (pass 2) that the
 * 1-term f16 feature screens could not certify and left to the 3-term split
 * screen since the last reset.  Synchronizes the device. */
int pcr_featnn_fallback_rows(int64_t *rows12, int64_t *cols21, int32_t reset);
/* Diagnostic: the chunks (16 f16 of every row) per 32-row tile that the last
 * f16 split-screen prepare stored in its packed operand images.  With S =
 * ceil(D / 16): S on the default route of pcr_feature_correspondences at D <=
 * 32 (the compact image: the hi halves only, all that featnn_row9 and the
 * threshold route read), 2 S + 1 (hi | lo | norms) for pcr_feature_match, D >
 * 32, the PCR_FEAT_THRESH=0 / PCR_FEAT_ROW9=0 / PCR_FEAT_ONE=0 routes, and
 * with PCR_FEAT_IMAGE=full (read per call: the full image on the default
 * route, same results).  0 before the first prepare. */
int pcr_featnn_image_chunks(int32_t *chunks);
/* diagnostic: copy `bytes` of pcr_feature_correspondences' scratch from its
 * last call (device to device, on `stream`) */
int pcr_featmut_debug_copy(void *dst, int64_t bytes, pcr_stream_t stream);

/* ---------------------------------------------------------------------------
 * a1 -- brute-force bidirectional 1-NN ("nnd" / Chamfer building block).
 * Replaces nnd_forward_cuda (dip/torch-nndistance/src/my_lib_cuda.cpp:25-41)
 * -> NmDistanceKernelLauncher (nnd_cuda.cu:132-162).
 *   xyz1 (b,n,3) f32, xyz2 (b,m,3) f32, contiguous AoS, device.
 *   dist1 (b,n) f32 / idx1 (b,n) i32: for each xyz1 point, min over xyz2 of
 *   (dx*dx+dy*dy)+dz*dz in f32 (no FMA) and the FIRST index attaining it;
 *   dist2/idx2 the same from xyz2 to xyz1.  Bit-exact with my_lib.cpp:3-25.
 *   m == 0 (resp. n == 0) yields dist 0, idx 0 (my_lib.cpp seed values).
 * ------------------------------------------------------------------------- */
int pcr_nnd_forward(const float *xyz1, const float *xyz2, int32_t b, int32_t n, int32_t m,
                    float *dist1, float *dist2, int32_t *idx1, int32_t *idx2,
                    pcr_stream_t stream);

/* ---------------------------------------------------------------------------
 * a1/a3 -- the same search over RAGGED batches, and in f64.  Replaces
 * pytorch3d.knn_points(x, y, lengths1, lengths2, K=1) inside
 * compute_truncated_chamfer_distance (c2p-net/deformationpyramid/model/
 * loss.py:60-160: x_lengths / y_lengths, computed in the inputs' dtype).
 *   n1 (b) / n2 (b) i32 device: valid points of each cloud (NULL = n / m);
 *   rows i < n1[k] search the first n2[k] points of the other cloud with
 *   pcr_nnd_forward's contract (same formula and first-index rule, in f32 or
 *   f64); rows past a length, and rows whose other cloud is empty, get
 *   (0, 0).  Outputs are (b,n) / (b,m) like pcr_nnd_forward.
 * ------------------------------------------------------------------------- */
int pcr_nnd_forward_ragged(const float *xyz1, const float *xyz2, int32_t b, int32_t n, int32_t m,
                           const int32_t *n1, const int32_t *n2, float *dist1, float *dist2,
                           int32_t *idx1, int32_t *idx2, pcr_stream_t stream);
int pcr_nnd_forward_f64(const double *xyz1, const double *xyz2, int32_t b, int32_t n, int32_t m,
                        const int32_t *n1, const int32_t *n2, double *dist1, double *dist2,
                        int32_t *idx1, int32_t *idx2, pcr_stream_t stream);

/* ---------------------------------------------------------------------------
 * a2 -- gradient of (dist1, dist2) w.r.t. (xyz1, xyz2).
 * Replaces nnd_backward_cuda (my_lib_cuda.cpp:44-72) -> NmDistanceGradKernel
 * (nnd_cuda.cu:164-222).  gxyz1 (b,n,3), gxyz2 (b,m,3) are fully written (the
 * caller need not zero them).  Deterministic: the scatter terms are summed in
 * the exact order of the reference CPU loop (my_lib.cpp:93-130), so the result
 * is bitwise reproducible and bit-identical to the CPU reference (the CUDA
 * reference uses float atomics and is not).
 * ------------------------------------------------------------------------- */
int pcr_nnd_backward(const float *xyz1, const float *xyz2, const float *graddist1,
                     const float *graddist2, const int32_t *idx1, const int32_t *idx2,
                     int32_t b, int32_t n, int32_t m, float *gradxyz1, float *gradxyz2,
                     pcr_stream_t stream);


/* ===========================================================================
 * Registration path (batched over P cloud pairs).  Layout: pair p's source
 * points are src_xyz[p*Nmax*3 .. +n_src[p]*3) (f32, AoS), features
 * src_feat[p*Nmax*D ..] (f32, row-major); likewise tgt with Mmax.  n_src /
 * n_tgt may be NULL (= all Nmax / Mmax points valid).
 * ======================================================================== */

/* ---------------------------------------------------------------------------
 * a5 -- exact feature-space 1-NN, both directions.  Replaces the KD-tree
 * SearchKNN(k=1) loops inside Open3D registration_ransac_based_on_feature_matching
 * (called at DataPreparation/RANSAC.py:43, dip/demo.py:43,
 * c2p-net/ngenet/utils/o3d.py:174) and vote.get_coor_points
 * (c2p-net/ngenet/models/vote.py:6-9).  nn12 (P,Nmax): argmin_j |f_i-g_j|^2,
 * nn21 (P,Mmax): argmin_i; distances in f64, lowest index on ties.  1 <= D <= 128.
 * ------------------------------------------------------------------------- */
int pcr_feature_match(const float *src_feat, const float *tgt_feat, int32_t P, int32_t Nmax,
                      int32_t Mmax, int32_t D, const int32_t *n_src, const int32_t *n_tgt,
                      int32_t *nn12, int32_t *nn21, pcr_stream_t stream);

/* mutual filter + ordered compaction: corres (P,Nmax,2) = (i, nn12[i]) for i with
 * nn21[nn12[i]] == i in increasing i, or all (i, nn12[i]) when fewer than
 * 3*ransac_n survive or mutual_filter == 0 (Open3D 0.13 semantics). */
int pcr_correspondences(const int32_t *nn12, const int32_t *nn21, int32_t P, int32_t Nmax,
                        int32_t Mmax, const int32_t *n_src, const int32_t *n_tgt,
                        int32_t mutual_filter, int32_t ransac_n, int32_t *corres,
                        int32_t *n_corres, pcr_stream_t stream);

/* feature matching + mutual filter in one call: the correspondences the
 * two calls above produce (bit-identical corres / n_corres, and nn12), without
 * computing nn21 for every target -- the filter reads nn21 only at j = nn12[i]
 * (Open3D 0.13 RegistrationRANSACBasedOnFeatureMatching with mutual_filter,
 * DataPreparation/RANSAC.py:43-52).  The column direction is screened only for
 * the targets some source picked, and decided from certified screen values
 * (csrc/featnn.hip featnn_row7).  With mutual_filter == 0 only nn12 is
 * computed.  nn12 (P,Nmax) out; corres (P,Nmax,2), n_corres (P) out. */
int pcr_feature_correspondences(const float *src_feat, const float *tgt_feat, int32_t P,
                                int32_t Nmax, int32_t Mmax, int32_t D, const int32_t *n_src,
                                const int32_t *n_tgt, int32_t mutual_filter, int32_t ransac_n,
                                int32_t *nn12, int32_t *corres, int32_t *n_corres,
                                pcr_stream_t stream);

/* RANSAC parameters (Open3D names; RANSAC.py:43-52). */
typedef struct pcr_ransac_params {
    double max_correspondence_distance; /* verification radius d                         */
    double edge_length_ratio;           /* CorrespondenceCheckerBasedOnEdgeLength; <=0 off */
    double distance_check;              /* CorrespondenceCheckerBasedOnDistance;   <=0 off */
    double confidence;                  /* RANSACConvergenceCriteria.confidence            */
    int32_t max_iteration;              /* RANSACConvergenceCriteria.max_iteration          */
    int32_t ransac_n;                   /* 3..8                                            */
    int32_t mutual_filter;              /* used by pcr_register_feature_ransac             */
    int32_t reserved;
    uint64_t seed;                      /* Philox key; hypothesis = f(seed, pair_id, itr)  */
} pcr_ransac_params;

/* ---------------------------------------------------------------------------
 * a6/a7 -- RANSAC hypothesize-and-verify on given correspondences.
 * Replaces Open3D RegistrationRANSACBasedOnCorrespondence.  corres (P,Kmax,2)
 * with n_corres[p] valid rows; pair_ids (P) optional (default p) keys the
 * hypothesis stream.  Outputs: T (P,16) f64 row-major 4x4, fitness_rmse (P,2),
 * stats (P,5) = {iterations, validated, best_itr, status(1 ok/0 none/-1 bad
 * input), n_correspondences}, corr_tgt (P,Nmax) target index per source point
 * or -1 (optional), inlier_mask (P, ceil(Nmax/32)) bitset (optional).
 * Asynchronous on the stream (no host round trip): hypotheses run in two
 * rounds, [0,1024) and [1024, max_iteration), the second launched behind the
 * first and returning at once when no pair's bound est_k lies beyond 1024.
 * Verification runs speculatively on persistent workgroups, the sequential rule
 * is replayed afterwards: results do not depend on the scheduling or the round
 * split.  Workspace per pair: ~135 B per hypothesis slot of the larger round
 * (max_iteration - 1024 rounded up to 256, at least 1024: ~13 MB per pair at
 * max_iteration 100000), 2 x Nmax x 4 B of target buffers, plus up to 256 MB
 * per device of per-hypothesis target slots (fewer slots only add one sweep per
 * pair).  Past 2^26 slots in all (P x max_iteration), or with
 * PCR_RANSAC_SYNC=1, the host instead runs rounds of 4096 while a pair is
 * still active (one 32-byte readback per round, ~540 KB per pair).
 * ------------------------------------------------------------------------- */
int pcr_ransac_batch(const float *src_xyz, const float *tgt_xyz, int32_t P, int32_t Nmax,
                     int32_t Mmax, const int32_t *n_src, const int32_t *n_tgt,
                     const int32_t *corres, const int32_t *n_corres, int32_t Kmax,
                     const uint32_t *pair_ids, const pcr_ransac_params *params, double *T,
                     double *fitness_rmse, int32_t *stats, int32_t *corr_tgt,
                     uint32_t *inlier_mask, pcr_stream_t stream);

/* ---------------------------------------------------------------------------
 * a5+a6+a7 composite: feature matching -> (mutual) correspondences -> RANSAC.
 * Replaces registration_ransac_based_on_feature_matching (RANSAC.py:43-52) for
 * P pairs at once; outputs as pcr_ransac_batch.  `scratch` sizing is internal.
 * ------------------------------------------------------------------------- */
int pcr_register_feature_ransac(const float *src_xyz, const float *tgt_xyz,
                                const float *src_feat, const float *tgt_feat, int32_t P,
                                int32_t Nmax, int32_t Mmax, int32_t D, const int32_t *n_src,
                                const int32_t *n_tgt, const uint32_t *pair_ids,
                                const pcr_ransac_params *params, double *T,
                                double *fitness_rmse, int32_t *stats, int32_t *corr_tgt,
                                uint32_t *inlier_mask, pcr_stream_t stream);

/* ICP parameters (Open3D ICPConvergenceCriteria defaults 1e-6, 1e-6, 30). */
typedef struct pcr_icp_params {
    double max_correspondence_distance;
    double relative_fitness;
    double relative_rmse;
    int32_t max_iteration;
    int32_t reserved;
} pcr_icp_params;

/* ---------------------------------------------------------------------------
 * a8 -- point-to-point ICP.  Replaces Open3D registration_icp
 * (DataPreparation/RANSAC.py:61-63).  init (P,16) f64; outputs T (P,16),
 * fitness_rmse (P,2), stats (P,2) = {iterations, n_correspondences}, corr_tgt
 * (P,Nmax) optional: target index of each source point in the final
 * correspondence set (Open3D result.correspondence_set) or -1.
 * ------------------------------------------------------------------------- */
int pcr_icp_batch(const float *src_xyz, const float *tgt_xyz, int32_t P, int32_t Nmax,
                  int32_t Mmax, const int32_t *n_src, const int32_t *n_tgt, const double *init,
                  const pcr_icp_params *params, double *T, double *fitness_rmse, int32_t *stats,
                  int32_t *corr_tgt, pcr_stream_t stream);

/* Robust kernel of point-to-plane ICP (Open3D RobustKernel): the weight of a
 * residual r, a = |r|.  k > 0 is the kernel's scale (unused by L2). */
enum {
    PCR_KERNEL_L2 = 0,     /* 1 */
    PCR_KERNEL_HUBER = 1,  /* a <= k ? 1 : k / a */
    PCR_KERNEL_CAUCHY = 2, /* 1 / (1 + (r/k)^2) */
    PCR_KERNEL_GM = 3,     /* k / (k + r^2)^2 */
    PCR_KERNEL_TUKEY = 4   /* a <= k ? (1 - (r/k)^2)^2 : 0 */
};

typedef struct pcr_icp_plane_params {
    int32_t kernel;   /* PCR_KERNEL_* */
    int32_t reserved;
    double k;
} pcr_icp_plane_params;

/* ---------------------------------------------------------------------------
 * Point-to-plane ICP with a robust kernel (Open3D registration_icp with
 * TransformationEstimationPointToPlane(kernel)).  As pcr_icp_batch, with
 * tgt_normals (P,Mmax,3) f32, the targets' normals, and the loop's Umeyama
 * step replaced by the weighted point-to-plane Gauss-Newton update (DESIGN.md
 * "Point-to-plane ICP").  The loop, the correspondence search, the stop rule
 * and the outputs are pcr_icp_batch's.  P == 0 returns PCR_OK; a null pointer
 * (corr_tgt, n_src and n_tgt may be null), a negative size, an unknown kernel
 * or k <= 0 for a kernel that uses it return PCR_ERR_ARG.
 * ------------------------------------------------------------------------- */
int pcr_icp_plane_batch(const float *src_xyz, const float *tgt_xyz, const float *tgt_normals,
                        int32_t P, int32_t Nmax, int32_t Mmax, const int32_t *n_src,
                        const int32_t *n_tgt, const double *init, const pcr_icp_params *params,
                        const pcr_icp_plane_params *plane, double *T, double *fitness_rmse,
                        int32_t *stats, int32_t *corr_tgt, pcr_stream_t stream);

/* ---------------------------------------------------------------------------
 * The C4 pipeline step (DataPreparation/RANSAC.py:109-122 per pair, with the
 * QualityCheck.py:25-31 Chamfer) for P resident pairs, no host round trip:
 * mutual feature correspondences (a5) -> RANSAC (a6/a7) -> ICP from the RANSAC
 * T (a8) -> aligned source (f64 T, f32 out) -> nnd both ways (a1) -> records.
 * Every buffer is device memory owned by the caller (inlier_mask optional).
 * records (P, 40) f64: [0,16) T_ransac, [16,32) T_icp, 32/33 RANSAC fitness /
 * rmse, 34/35 ICP fitness / rmse, 36 Chamfer = mean(d1) + mean(d2) (f64 sums
 * of the f32 distances in one fixed order: 1024 partial sums, partial t over
 * the indices t, t + 1024, ... in increasing order; each run of 64 partials
 * folded by a halving tree, p[l] += p[l + h] for h = 32 ... 1; the 16 results
 * added in order from 0.0; then sum1 / N + sum2 / M), 37 RANSAC iterations,
 * 38 RANSAC status, 39 correspondences after the mutual filter.
 * pcr_pipeline_records: the records alone, from buffers the stage calls filled.
 * Streams: the step forks once -- RANSAC's / ICP's target grids and the source
 * spatial order are built on a library-owned side stream of the calling
 * thread's (device, workspace context) while the feature stage runs on
 * `stream`, joined by an event before RANSAC -- and everything else, and the
 * completion, is on `stream` (a graph capture of the step sees the fork/join).
 * ------------------------------------------------------------------------- */
typedef struct pcr_pipeline_io {
    const float *src_xyz, *tgt_xyz;    /* (P,N,3), (P,M,3) */
    const float *src_feat, *tgt_feat;  /* (P,N,D), (P,M,D) */
    int32_t P, N, M, D;
    const uint32_t *pair_ids;          /* (P) or null */
    int32_t *nn12;                     /* (P,N) */
    int32_t *corres, *n_corres;        /* (P,N,2), (P) */
    double *T_ransac, *fit_ransac;     /* (P,16), (P,2) */
    int32_t *stats_ransac;             /* (P,5) */
    uint32_t *inlier_mask;             /* (P, ceil(N/32)) or null */
    double *T_icp, *fit_icp;           /* (P,16), (P,2) */
    int32_t *stats_icp;                /* (P,2) */
    float *aligned;                    /* (P,N,3) */
    float *d1, *d2;                    /* (P,N), (P,M) */
    int32_t *i1, *i2;                  /* (P,N), (P,M) */
    double *records;                   /* (P,40) */
} pcr_pipeline_io;
int pcr_pipeline_step(const pcr_pipeline_io *io, const pcr_ransac_params *ransac,
                      const pcr_icp_params *icp, pcr_stream_t stream);
int pcr_pipeline_records(const pcr_pipeline_io *io, pcr_stream_t stream);

/* ---------------------------------------------------------------------------
 * radius-limited 1-NN (Open3D KDTreeFlann::SearchHybrid(r, max_nn=1), used by
 * RANSAC verification / ICP): for each f64 query (P,Qmax,3) the nearest target
 * point with d^2 < float(r*r), lowest index on ties; idx -1 if none, d2 optional.
 * ------------------------------------------------------------------------- */
int pcr_radius_nn(const float *tgt_xyz, int32_t P, int32_t Mmax, const int32_t *n_tgt,
                  const double *queries, int32_t Qmax, const int32_t *n_q, double r,
                  int32_t *idx, double *d2, pcr_stream_t stream);

/* ---------------------------------------------------------------------------
 * a9 -- batched weighted Procrustes (B items of N points).  Replaces the
 * torch.svd Kabsch of ROPNet weighted_icp (model_utils.py:105-139; abs_weights=0,
 * eps=1e-8) and NDP rigid_fit (deformationpyramid/model/geometry.py:8-34;
 * abs_weights=1, eps=1e-4).  T (B,12) f64 = [R | t] row-major, tgt ~ R src + t.
 * ------------------------------------------------------------------------- */
int pcr_procrustes_batch(const float *src, const float *tgt, const float *weights, int32_t B,
                         int32_t N, int32_t abs_weights, double eps, double *T,
                         pcr_stream_t stream);
/* the same for f64 inputs (the reference functions are dtype-generic: f64
 * tensors run weighted_icp's torch.svd in f64, model_utils.py:120-133) */
int pcr_procrustes_batch_f64(const double *src, const double *tgt, const double *weights,
                             int32_t B, int32_t N, int32_t abs_weights, double eps, double *T,
                             pcr_stream_t stream);

/* out (B,N,3) f32 = (float)(R p + t) in f64 for each item's T (B,16) f64
 * row-major 4x4 (registration outputs).  Replaces the per-pair
 * source.transform(T) (Open3D PointCloud::Transform, RANSAC.py / QualityCheck.py)
 * before the Chamfer check. */
int pcr_transform_batch(const float *xyz, int32_t B, int32_t N, const double *T, float *out,
                        pcr_stream_t stream);

/* ---------------------------------------------------------------------------
 * a4 -- DIP local reference frames, batched.  Replaces lrf.get
 * (dip/lrf.py:19-78) called per sampled point by dip/demo.py:109-114.
 * Two phases so the reference's np.random.choice stream stays on the host:
 *   pcr_lrf_count   -> counts (P,Qmax): radius neighbours of each query
 *                      (d^2 < float(kernel^2), incl. the first hit);
 *   host            -> inds (P,Qmax,patch_size) = np.random.choice(
 *                      max(count, patch_size), patch_size, replace=False);
 *   pcr_lrf_compute -> patches (P,Qmax,patch_size,3) f64 (lRg^T (p - pt) /
 *                      kernel, zero rows past the count) and T (P,Qmax,16) f64
 *                      row-major [[xp yp zp | pt],[0 0 0 1]] (det -1, as the
 *                      reference).  max_count >= every count, <= 8192.
 * Points/queries f64 (Open3D stores double).  counts may be NULL in phase 2.
 * ------------------------------------------------------------------------- */
int pcr_lrf_count(const double *pts, int32_t P, int32_t Nmax, const int32_t *n_pts,
                  const double *queries, int32_t Qmax, const int32_t *n_q, double kernel,
                  int32_t *counts, pcr_stream_t stream);
int pcr_lrf_compute(const double *pts, int32_t P, int32_t Nmax, const int32_t *n_pts,
                    const double *queries, int32_t Qmax, const int32_t *n_q, double kernel,
                    int32_t patch_size, const int32_t *inds, int32_t max_count,
                    double *patches, double *T, int32_t *counts, pcr_stream_t stream);
/* Host only (no device work): the patch-index draws of dip/lrf.py:76,
 * np.random.choice(pop[c], k, replace=False) for c = 0..calls-1 in order, on the
 * caller's legacy RandomState MT19937 state (key[624], *pos as returned by
 * RandomState.get_state(); both updated as numpy would leave them).
 * out (calls, k) i32.  Fails with PCR_ERR_ARG when pop[c] < k, like numpy. */
int pcr_legacy_choice_batch(uint32_t *key, int32_t *pos, const int32_t *pop, int32_t calls,
                            int32_t k, int32_t *out);

/* ---------------------------------------------------------------------------
 * a10 -- NDP deformation-pyramid warp, all levels in one launch.  Replaces
 * Deformation_Pyramid.warp (c2p-net/deformationpyramid/model/nets.py:36-48)
 * over NDPLayer.forward (:111-161) for every head of the reference: motion
 * "SE3", "Sim3" or "sflow", rotation "axis_angle", "euler", "quaternion" or
 * "6D" (config/NDP.yaml ships SE3 / axis_angle, the C5 configuration).
 * Weights in nn.Linear layout
 * (out, in) f32, device pointers; w_hid holds the depth-1 MLP layers
 * contiguously; w_nr/b_nr NULL for levels without the nonrigidity branch.
 * levels is a HOST array of n_levels (<= 16) entries that share one head.
 * x_levels (n_levels,N,3)
 * and nonrigidity (n_levels,N) are optional per-level outputs (data[i]).
 * A point's result does not depend on its position in the cloud.  NaN
 * propagates as in the reference: a point a level made NaN (an axis_angle or
 * quaternion rotation branch that is exactly 0 divides 0 by 0; an euler one
 * gives R = I and a 6D one R = 0, both finite) is NaN in every later level's
 * points and nonrigidity (the ReLU keeps NaN, as torch's does).
 *
 * Head code = rotation format + 4 * motion (PCR_NDP_HEAD): format 0 axis_angle,
 * 1 euler, 2 quaternion, 3 6D; motion 0 SE3 (y = R x + t), 1 Sim3
 * (y = c R x + t, c = 1e-3 (w_s h + b_s) + 1), 2 sflow (y = x + t, code 8 only,
 * w_rot / b_rot unused).  Code 0 is SE3 / axis_angle: a zero-initialised
 * descriptor means what it always meant.  Rows of w_rot per format: 3, 3, 4, 6.
 * pcr_ndp_head_rows(head, what): what 0 the rows of w_rot, 1 the rows of the
 * aux / dO scratch of pcr_ndp_train, 2 the rows of its branch-gradient buffer,
 * 3 the first of the three translation rows, 4 the nonrigidity row, 5 the scale
 * row, 6 the first of the three R x rows of aux (5, 6: -1 unless Sim3); -1 for
 * an unknown head or what.
 * ------------------------------------------------------------------------- */
#define PCR_NDP_ROT_AXIS_ANGLE 0
#define PCR_NDP_ROT_EULER 1
#define PCR_NDP_ROT_QUATERNION 2
#define PCR_NDP_ROT_6D 3
#define PCR_NDP_MOTION_SE3 0
#define PCR_NDP_MOTION_SIM3 1
#define PCR_NDP_MOTION_SFLOW 2
#define PCR_NDP_HEAD(motion, rot) ((motion) == PCR_NDP_MOTION_SFLOW ? 8 : 4 * (motion) + (rot))
typedef struct pcr_ndp_level {
    const float *w_in, *b_in;   /* (W,6), (W) */
    const float *w_hid, *b_hid; /* (depth-1,W,W), (depth-1,W) */
    const float *w_rot, *b_rot; /* (R,W), (R), R = 3, 3, 4, 6 by format; unused for sflow */
    const float *w_trn, *b_trn; /* (3,W), (3) */
    const float *w_nr, *b_nr;   /* (1,W), (1) or NULL */
    int32_t m;                  /* level index + 1: omega = 2^(m + k0) */
    int32_t reserved;
    const float *w_s, *b_s;     /* (1,W), (1): the Sim3 scale branch, NULL otherwise */
    int32_t head;               /* head code, 0 = SE3 / axis_angle */
    int32_t reserved2;
} pcr_ndp_level;
int32_t pcr_ndp_head_rows(int32_t head, int32_t what);
int pcr_ndp_warp(const float *x, int32_t N, const pcr_ndp_level *levels, int32_t n_levels,
                 int32_t width, int32_t depth, int32_t k0, float *x_out, float *x_levels,
                 float *nonrigidity, pcr_stream_t stream);


/* ---------------------------------------------------------------------------
 * f2 -- KPConv input pyramid helpers (ngenet cpp_wrappers).
 *
 * pcr_grid_subsample replaces cpp_subsampling.subsample_batch
 * (c2p-net/ngenet/cpp_wrappers/cpp_subsampling/wrapper.cpp:59-330 ->
 * batch_grid_subsampling, grid_subsampling/grid_subsampling.cpp:109-211).
 *   points (n,3) f32 and features (n,fdim) f32 (or NULL, fdim 0) are device
 *   buffers; batch_len (nb) is a HOST array (cloud lengths, summing to <= n).
 *   Per cloud: voxels of side dl from the floor(min/dl)*dl corner, barycentre
 *   (f32 sums in input order, * (float)(1.0/count)) and mean features
 *   (f / (float)count), emitted in the reference's unordered_map iteration order
 *   and truncated to max_p per cloud (max_p < 1: n).  Writes out_points
 *   (capacity n*3), out_features (capacity n*fdim), out_batch_len (HOST, nb)
 *   and *out_total (HOST).  Bit-identical to the reference, order included.
 *   Synchronous (the emission order is replayed on the host).  Non-finite
 *   coordinates -> PCR_ERR_ARG (the reference's voxel index is undefined).
 *
 * pcr_voxel_map_order: host-only helper behind it -- the iteration order of a
 * std::unordered_map<size_t,...> after inserting the n distinct keys in order:
 * order[k] = insertion rank of the k-th visited key.
 *
 * pcr_radius_count / pcr_radius_neighbors replace cpp_neighbors.batch_query
 * (cpp_neighbors/wrapper.cpp:63-230 -> batch_nanoflann_neighbors,
 * neighbors/neighbors.cpp:211-332).
 *   queries (nq,3), supports (ns,3) f32 device; q_batches / s_batches (nb) HOST.
 *   Neighbours of a query: supports of its batch with f32
 *   (dx*dx + dy*dy) + dz*dz < radius*radius, by ascending distance (equal
 *   distances by ascending index), as global support indices.  counts (nq)
 *   device (optional) and *max_count (HOST) = the reference's row width.
 *   pcr_radius_neighbors writes out (nq,width) int32 device: the first `width`
 *   neighbours of each query, padded with ns (supports.size()); width =
 *   max_count is batch_query, min(max_count, max_nn) is dataloader.py
 *   batch_neighbors (:12-25).  Both synchronize the stream once.
 * ------------------------------------------------------------------------- */
int pcr_grid_subsample(const float *points, int32_t n, const int32_t *batch_len, int32_t nb,
                       const float *features, int32_t fdim, float dl, int32_t max_p,
                       float *out_points, float *out_features, int32_t *out_batch_len,
                       int32_t *out_total, pcr_stream_t stream);
int pcr_voxel_map_order(const uint64_t *keys, int32_t n, int32_t *order);
int pcr_radius_count(const float *queries, int32_t nq, const float *supports, int32_t ns,
                     const int32_t *q_batches, const int32_t *s_batches, int32_t nb, float radius,
                     int32_t *counts, int32_t *max_count, pcr_stream_t stream);
int pcr_radius_neighbors(const float *queries, int32_t nq, const float *supports, int32_t ns,
                         const int32_t *q_batches, const int32_t *s_batches, int32_t nb,
                         float radius, int32_t width, int32_t *out, int32_t *max_count,
                         pcr_stream_t stream);

/* ---------------------------------------------------------------------------
 * a5 (ii) -- the level voting of c2p-net/ngenet/models/vote.py:12-37 (after the
 * h / m / l feature-space 1-NN of get_coor_points, :6-9, on pcr_feature_match).
 *   tgt_xyz (m,3) f32, nn_h / nn_m / nn_l (n) i32 (source -> target at each
 *   level), feature rows (n,D) / (m,D) f32, all device.  For every source i:
 *   d12, d13, d23 = f32 Euclidean distances between its three targets (numpy's
 *   order, correctly rounded sqrt); sel_h = d12 < thr or d13 < thr, sel_m = d23
 *   < thr with thr = (float)(2 voxel_size); where !sel_h and sel_m the h rows
 *   are replaced in place: src_feat_h[i] <- src_feat_m[i] and
 *   tgt_feat_h[nn_m[i]] <- tgt_feat_m[nn_m[i]].  replaced (n) u8 optional.
 *   Asynchronous on `stream`.
 * ------------------------------------------------------------------------- */
int pcr_vote_apply(const float *tgt_xyz, int32_t m, const int32_t *nn_h, const int32_t *nn_m,
                   const int32_t *nn_l, int32_t n, double voxel_size, float *src_feat_h,
                   const float *src_feat_m, float *tgt_feat_h, const float *tgt_feat_m, int32_t D,
                   uint8_t *replaced, pcr_stream_t stream);

/* ---------------------------------------------------------------------------
 * f2 -- Open3D voxel down-sampling (dip/demo.py:73-74 pcd.voxel_down_sample,
 * Open3D 0.13 PointCloud::VoxelDownSample; oracle/voxel_oracle.cpp restates it).
 *   points (n,3) f64 device, optional normals / colors (n,3) f64 device (NULL:
 *   none); cloud_len (nb) HOST (lengths summing to <= n).  Per cloud: voxel
 *   min bound = min - voxel_size/2, voxel = int(floor((p - bound)/voxel_size)),
 *   per voxel the f64 sums in input order (normals with a NaN component
 *   skipped) divided by double(count), emitted in the iteration order of
 *   Open3D's unordered_map<Vector3i, ..., hash_eigen> (replayed on the host).
 *   Writes out_points / out_normals / out_colors (capacity n*3 each, device),
 *   out_cloud_len (HOST, nb) and *out_total (HOST).  Synchronous.  Errors as
 *   the reference: voxel_size <= 0, "voxel_size is too small"; non-finite
 *   coordinates -> PCR_ERR_ARG.
 * pcr_voxel3i_map_order: host-only helper behind it -- iteration order of that
 *   map after inserting the n distinct (x, y, z) int keys in order.
 * ------------------------------------------------------------------------- */
int pcr_voxel_down_sample(const double *points, int32_t n, const int32_t *cloud_len, int32_t nb,
                          double voxel_size, const double *normals, const double *colors,
                          double *out_points, double *out_normals, double *out_colors,
                          int32_t *out_cloud_len, int32_t *out_total, pcr_stream_t stream);
int pcr_voxel3i_map_order(const int32_t *xyz, int32_t n, int32_t *order);

/* ---------------------------------------------------------------------------
 * f1 -- normal estimation and FPFH, the preprocessing of
 * DataPreparation/RANSAC.py:12-22 (Open3D 0.13 PointCloud::estimate_normals
 * with KDTreeSearchParamHybrid(4 voxel, 30) and
 * pipelines.registration.compute_fpfh_feature with
 * KDTreeSearchParamHybrid(7 voxel, 100)), batched over P clouds.
 * Semantics restated in oracle/fpfh_oracle.c (Open3D absent: parity vs the
 * reference unpinned; GPU == restatement bit for bit).
 *
 * pcr_hybrid_search replaces KDTreeFlann::SearchHybrid(points[i], radius,
 *   max_nn) for every point of every cloud: the max_nn nearest points with
 *   f64 (dx*dx + dy*dy) + dz*dz < (double)(float)(radius^2), ascending
 *   (d2, index).  idx (P,Nmax,max_nn) local indices (-1 padded), d2 same shape
 *   f64, counts (P,Nmax).  1 <= max_nn <= 448.
 * pcr_estimate_normals: normals (P,Nmax,3) f64 (ComputeCovariance over the
 *   hybrid neighbourhood incl. the point, FastEigen3x3 smallest eigenvector;
 *   < 3 neighbours -> (0,0,1)).  prior_normals (P,Nmax,3) f64 or NULL: when
 *   given (the cloud already had normals) each result is flipped to agree
 *   with it, and a zero result takes it (EstimateNormals' has_normal branch).
 * pcr_compute_fpfh: fpfh (P,Nmax,33) f64 = Open3D's Feature::data_ (33, N)
 *   column-major; fpfh_f32 (optional) the same rounded to f32 (the input of
 *   pcr_feature_match); spfh (optional) the intermediate SPFH histograms.
 * Clouds are xyz (P,Nmax,3) f32 with n_pts (P) valid points (NULL = Nmax);
 * rows past a cloud's count are left untouched.
 * ------------------------------------------------------------------------- */
int pcr_hybrid_search(const float *xyz, int32_t P, int32_t Nmax, const int32_t *n_pts,
                      double radius, int32_t max_nn, int32_t *idx, double *d2, int32_t *counts,
                      pcr_stream_t stream);
int pcr_estimate_normals(const float *xyz, int32_t P, int32_t Nmax, const int32_t *n_pts,
                         double radius, int32_t max_nn, const double *prior_normals,
                         double *normals, pcr_stream_t stream);
int pcr_compute_fpfh(const float *xyz, const double *normals, int32_t P, int32_t Nmax,
                     const int32_t *n_pts, double radius, int32_t max_nn, double *fpfh,
                     float *fpfh_f32, double *spfh, pcr_stream_t stream);

/* ---------------------------------------------------------------------------
 * f4 -- device-side pieces of the NDP level optimisation
 * (c2p-net/deformationpyramid/model/registration.py:196-262), so one iteration
 * can be captured in a HIP graph and replayed without host round trips.
 *
 * pcr_ndp_control: the early-stop rule of :246-256 on the device (f64 on the f32
 *   loss, as Python evaluates loss.item()).  state (device f64[8]) =
 *   {active, break_count, loss_prev, steps, last_loss, step_flag, evaluated, 0},
 *   initialise to {1, 0, 1e6, 0, 0, 0, 0, 0} per level; stop_loss 1e-4.
 * pcr_adam_masked: torch.optim.Adam's update for n_tensors parameter tensors
 *   (a DEVICE table of pcr_adam_tensor), skipped when state[5] == 0; bias
 *   corrections from state[3] (steps taken, incremented by pcr_ndp_control).
 *   The rule runs first: it increments state[3] *before* Adam reads it, so the
 *   first applied step uses t = 1; state[3] must be >= 1 whenever state[5] is
 *   set (t = 0 divides by 1 - beta1^0 = 0).  The launch is masked by state[5]
 *   alone, not by pcr_set_gate: a gated level does not step because the rule
 *   that cleared state[0] also cleared state[5].  Each tensor's result does not
 *   depend on the other entries of the table; n_tensors <= 65535
 *   (PCR_ERR_ARG above), and n_tensors = 0 or max_numel = 0 launch nothing.
 * ------------------------------------------------------------------------- */
typedef struct pcr_adam_tensor {
    float *param;
    const float *grad;
    float *exp_avg;
    float *exp_avg_sq;
    int32_t n;
    int32_t reserved;
} pcr_adam_tensor;
int pcr_ndp_control(const float *loss, double *state, double break_threshold_ratio,
                    int32_t max_break_count, double stop_loss, pcr_stream_t stream);
int pcr_adam_masked(const pcr_adam_tensor *tensors, int32_t n_tensors, int32_t max_numel,
                    const double *state, double lr, double beta1, double beta2, double eps,
                    pcr_stream_t stream);
/* pcr_set_gate: the early stop that stops the work (registration.py:250-256
 *   `break`s out of the level).  While a gate is set on the calling thread
 *   (gate = the level's state, a device pointer), every kernel that
 *   pcr_nnd_forward / pcr_nnd_backward / pcr_ndp_train_forward /
 *   pcr_ndp_train_backward / pcr_ndp_chamfer_glue / pcr_ndp_chamfer_step /
 *   pcr_ndp_chamfer_loss / pcr_ndp_ldmk_loss launch reads gate[0] at entry
 *   and returns at once when it is 0 -- so the replays of a captured level graph
 *   left after the rule fired cost only their launches.  pcr_set_gate(NULL)
 *   restores ungated launches.  Thread-local; captured launches keep the pointer
 *   they were recorded with. */
int pcr_set_gate(const double *gate);

/* ---------------------------------------------------------------------------
 * f4 -- fused NDP level training step (one level of
 * registration.py:208-262 without PyTorch autograd).  One descriptor:
 *   x (N,3) level input; level weights in nn.Linear layout (level.w_hid /
 *   level.b_hid unused: the hidden layers are w_hid[k] / b_hid[k], k < depth-1,
 *   read in place so the optimizer updates them directly); width 128.
 *   Scratch (device, feature-major [F][N]): pe [6][N], H [depth][W][N],
 *   aux [A][N], dO [A][N], D [depth][W][N]; x_out (N,3) the warped points.
 *   g (N,3) = dL/dx_out (e.g. the Chamfer gradient), bce_scale = w_reg / N for
 *   a level with the nonrigidity branch (BCE(s, 0) mean), else 0.
 *   Branch rows, by level.head (one row map for aux, dO and the branch gradients):
 *     code 0 (SE3 / axis_angle): A = 8; rot 0-2, trn 3-5, nr 6; 7 gradient rows.
 *     codes 1-8: A = 16; rot 0-5 (the format's 3, 3, 4 or 6 rows first), trn 6-8,
 *       nr 9, scale 10; 11 gradient rows; aux alone also holds R x of a Sim3
 *       head in rows 11-13.
 *     aux: r = 1e-3 o_rot in the rot rows, y (the motion's output before the
 *     nonrigidity blend) in the trn rows, s in the nr row, c in the scale row.
 *     dO: dL/d(branch pre-activation).  Rows a head does not use are exact
 *     zeros in aux, dO and the branch gradients (pcr_ndp_head_rows gives the counts).
 * pcr_ndp_train_forward: x_out, and the saved activations.
 * pcr_ndp_train_backward: the gradients of every parameter of the level into
 *   grads (HOST array of device pointers): {w_in, b_in, w_hid[0], b_hid[0], ...,
 *   w_branch (B x W rows in the head's row map, B = 7 or 11), b_branch (B)}; part is
 *   scratch of pcr_ndp_train_partial_floats_head(N, width, depth, chunk, head)
 *   floats (pcr_ndp_train_partial_floats: head 0).  Width 128, depth <= 5.
 * ------------------------------------------------------------------------- */
typedef struct pcr_ndp_train {
    const float *x;
    int32_t N, width, depth, k0;
    pcr_ndp_level level;
    const float *w_hid[4], *b_hid[4];
    float *pe, *H, *aux, *x_out;
    const float *g;
    double bce_scale;
    float *dO, *D;
    /* optional Chamfer subset (null = off): inv (N) = k where inds[k] == p for a
     * duplicate-free inds, else -1; the forward also writes x_out[inds] to xs (K,3)
     * and the backward takes dL/dx_out of p from gsub[inv[p]] (0 off the subset)
     * instead of g, i.e. g = index_add(zeros, inds, gsub) without materialising it */
    const int32_t *inv;
    float *xs;
    const float *gsub;
    /* optional (null = off): the subset gradient as pcr_ndp_chamfer_step leaves
     * it (pcr_ndp_chamfer_gacc_words(K) int64, layout there); read instead of
     * gsub; K = gacc_k */
    const long long *gacc;
    int32_t gacc_k, reserved;
    /* optional landmark block (null = off; registration.py:213-227): the first
     * ldmk_n points of x are landmarks with targets ldmk_tgt (ldmk_n,3).  The
     * backward gives them dL/dx_out[p][c] = f32(2 / ldmk_n) * (x_out[p][c] -
     * ldmk_tgt[p][c]), read from x_out (the gradient of mean_k sum_c (x_out -
     * ldmk_tgt)^2; no gradient buffer), whatever inv / g say about them, and
     * multiplies the gradient of every other point (gacc or gsub through inv, or
     * g) once by f32(cd_scale).  inv and g may both be null (every gradient is
     * the landmarks').  1 <= ldmk_n <= N, else PCR_ERR_ARG.  The forward does not
     * read the block: landmarks and samples are rows of one (N,3) input. */
    const float *ldmk_tgt;
    int32_t ldmk_n, reserved3;
    double cd_scale;
} pcr_ndp_train;
int pcr_ndp_train_forward(const pcr_ndp_train *t, pcr_stream_t stream);
int pcr_ndp_train_backward(const pcr_ndp_train *t, float *part, int32_t chunk,
                           float *const *grads, pcr_stream_t stream);
int64_t pcr_ndp_train_partial_floats(int32_t N, int32_t width, int32_t depth, int32_t chunk);
int64_t pcr_ndp_train_partial_floats_head(int32_t N, int32_t width, int32_t depth, int32_t chunk,
                                          int32_t head);
/* pcr_ndp_chamfer_glue: the loss of registration.py:231-244 around the Chamfer
 *   pass, on the device, in a fixed reduction order:
 *   loss = sum(d1')/K + sum(d2')/M (+ w_reg * mean(-max(log(1 - s), -100)) when s
 *   is given), d' = d where d < trunc else 0; gd1 = 1/K and gd2 = 1/M where not
 *   truncated, else 0 (the dist gradients for pcr_nnd_backward; gd1 / gd2 may be
 *   null);
 *   log[min(*ctr, log_last)] = loss; ++*ctr (device int64).
 *   NaN in d1 / d2 stays (it is not >= trunc, its seed is 1/K), s == 1 counts
 *   exactly -100, s > 1 gives NaN.  K = 0 or M = 0 launches and gives NaN
 *   (0 / 0, as torch's mean of an empty tensor); pcr_ndp_chamfer_loss refuses
 *   them (PCR_ERR_ARG, nothing written). */
int pcr_ndp_chamfer_glue(const float *d1, int32_t K, const float *d2, int32_t M,
                         const float *s, int32_t N, double w_reg, double trunc,
                         float *gd1, float *gd2, float *loss, float *log, int64_t *ctr,
                         int32_t log_last, pcr_stream_t stream);

/* pcr_ndp_chamfer_*: the level's Chamfer pass with its gradient, specialised
 *   for the loop (csrc/ndp_chamfer.hip).  xs (K,3) = x_out[inds] (written by
 *   pcr_ndp_train_forward through inv), tgt (M,3) fixed for the level.
 *   d1/i1 (K), d2/i2 (M): pcr_nnd_forward's outputs bit for bit.  gacc
 *   (pcr_ndp_chamfer_gacc_words(K) = 1 + 6 K R int64, R =
 *   PCR_NDP_GACC_REPLICAS): the gradient of sum(d1')/K + sum(d2')/M w.r.t. xs
 *   (d' = d where d < trunc, else 0), each term exactly in a two-word fixed
 *   point whose exponent s follows the iteration's extents (every integer sum
 *   provably below 2^63): dL/dxs[k][c] = sum over r of
 *   hi[r][k][c] 2^-s + lo[r][k][c] 2^-(s+40), hi at gacc[1 + 3 (r K + k) + c],
 *   lo at gacc[1 + 3 K R + 3 (r K + k) + c]; gacc[0] = ((s + 2048) << 8) | f,
 *   f = 1 when a term was not finite -- consumed by pcr_ndp_train_backward
 *   (pcr_ndp_train.gacc).  K, M <= pcr_ndp_chamfer_max_points() (32768).
 *   scratch: pcr_ndp_chamfer_scratch_bytes(K, M) bytes, 256-byte aligned,
 *   owned by the caller for the level.
 * pcr_ndp_chamfer_prepare: the target grid and the subset cell (from xs0, the
 *   level's input subset) -- with the box path (default; PCR_NC_BOX=0: the grid
 *   path), both clouds' spatial orders and the target's leaf / group boxes;
 *   once per level, outside the captured graph.  The path is read from the
 *   environment by prepare and step alike: keep it unchanged between them.
 * pcr_ndp_chamfer_step: one iteration (gated like the other f4 launches).  The
 *   box path starts each query's search from its answer of the previous call,
 *   read from i1 / i2 before they are overwritten: any value is a valid start
 *   (out-of-range ones count as 0), the results are exact from every start,
 *   only the time depends on it. */
/* pcr_ndp_chamfer_loss: pcr_ndp_chamfer_glue's loss (no dist gradients: the
 *   Chamfer step made them) over 32 workgroups (fixed ranges, partials summed in
 *   block order), then -- when state is given -- pcr_ndp_control's rule on it,
 *   in one launch.  scratch: pcr_ndp_loss_scratch_bytes() bytes, zeroed once
 *   by the caller (the launch leaves it zeroed). */
int64_t pcr_ndp_loss_scratch_bytes(void);
int pcr_ndp_chamfer_loss(const float *d1, int32_t K, const float *d2, int32_t M, const float *s,
                         int32_t N, double w_reg, double trunc, float *loss, float *log, int64_t *ctr,
                         int32_t log_last, double *state, double break_threshold_ratio,
                         int32_t max_break_count, double stop_loss, void *scratch, pcr_stream_t stream);
/* pcr_ndp_ldmk_loss: pcr_ndp_chamfer_loss with the landmark term of
 *   registration.py:213-227 in front:
 *   loss = mean_k sum_c (x_out[k][c] - ldmk_tgt[k][c])^2 over the L landmarks (the
 *   first L rows of x_out) + f32(w_cd) * (sum(d1')/K + sum(d2')/M)
 *   [+ f32(w_reg) * mean(-max(log(1 - s), -100)) over the P entries of s], the
 *   same fixed reduction (32 workgroups, partials summed in block order), log
 *   entry, counter and -- when state is given -- early-stop rule, in one launch.
 *   K = M = 0 (d1, d2 may be null) is the landmark-only loss (w_cd <= 0 in the
 *   reference): no Chamfer part.  L >= 1; K and M both 0 or both >= 1; else
 *   PCR_ERR_ARG and nothing is written.  scratch:
 *   pcr_ndp_ldmk_loss_scratch_bytes() bytes, zeroed once by the caller. */
int64_t pcr_ndp_ldmk_loss_scratch_bytes(void);
int pcr_ndp_ldmk_loss(const float *x_out, const float *ldmk_tgt, int32_t L, const float *d1, int32_t K,
                      const float *d2, int32_t M, const float *s, int32_t P, double w_cd, double w_reg,
                      double trunc, float *loss, float *log, int64_t *ctr, int32_t log_last, double *state,
                      double break_threshold_ratio, int32_t max_break_count, double stop_loss, void *scratch,
                      pcr_stream_t stream);
#define PCR_NDP_GACC_REPLICAS 16
typedef struct pcr_ndp_chamfer {
    const float *xs;
    const float *tgt;
    int32_t K, M;
    double trunc;
    float *d1, *d2;
    int32_t *i1, *i2;
    long long *gacc;
    void *scratch;
} pcr_ndp_chamfer;
int64_t pcr_ndp_chamfer_scratch_bytes(int32_t K, int32_t M);
int64_t pcr_ndp_chamfer_gacc_words(int32_t K);
int32_t pcr_ndp_chamfer_max_points(void);
int pcr_ndp_chamfer_prepare(const pcr_ndp_chamfer *c, const float *xs0, pcr_stream_t stream);
int pcr_ndp_chamfer_step(const pcr_ndp_chamfer *c, pcr_stream_t stream);

/* ---------------------------------------------------------------------------
 * Point-set sampling and grouping: fps, ball_query and sample_and_group of
 * ROPNet/src/models/model_utils.py:6-102 (used by LocalFeatue.forward,
 * TFMR.py:48-71) and c2p-net/ngenet/utils/process.py:57-115 (used by
 * PPF.forward, ngenet/models/information_interactive.py:48-84).
 *
 * Shared contract.  Squared distance d2(a, b) = (dx*dx + dy*dy) + dz*dz in f32,
 * every operation rounded (no FMA), the direct form; the reference's expanded
 * |a|^2 + |b|^2 - 2 a.b agrees with it to rounding.  r2 is the f32 squared
 * radius, (float)((double)radius * radius) for the reference's `radius ** 2`;
 * j is a neighbour iff !(d2 > r2), so a distance equal to the radius is
 * inside.  Ties go to the lowest index.  Non-finite coordinates give
 * unspecified results.  All buffers are device memory; all entries are
 * asynchronous on `stream`; n >= 1 and n < 2^31 / 3.
 *
 * pcr_fps: farthest-point sampling.  xyz (b,n,3) f32, start (b) i32 with
 *   0 <= start < n (a PRECONDITION the library cannot see: the values live on
 *   the device; the kernel clamps them so that it never reads outside the
 *   cloud), m >= 1, idx (b,m) i32.  Per cloud: dist[j] = 1e10f, cur = start;
 *   for i < m: idx[i] = cur; for all j, d = d2(x[cur], x[j]) and dist[j] = d
 *   where d < dist[j]; cur = the first index of max(dist).  m > n is legal
 *   (the loop defines it).  One workgroup per cloud; clouds of up to 8192
 *   points run from registers, larger ones keep the rest in the workspace,
 *   with identical results.
 *
 * pcr_ball_query: xyz (b,n,3), query (b,q,3) f32, k >= 1, idx (b,q,k) i32,
 *   count (b,q) i32 or NULL.  Row = the ascending indices j that are
 *   neighbours of the query, cut to the first k; the columns after the last
 *   one repeat the row's first neighbour; a row without neighbours holds n in
 *   every column (the reference's sentinel).  count = the number of
 *   neighbours before the cut (the reference's density is count / n).  k > n
 *   is legal and pads the same way.
 *
 * pcr_group_ppf: sample_and_group with M = -1 (every point a centre) and the
 *   point-pair features of LocalFeatue / PPF in one call.  xyz (b,n,3),
 *   normals (b,n,3) f32 or NULL, r2 >= 0, k >= 1; idx (b,n,k) i32 or NULL
 *   receives the ball query of xyz against itself.  C = 10 channels with
 *   normals, 6 without; for centre i and its neighbour j, g = x_j - x_i:
 *   0-2 x_i, 3-5 g, 6 angle(n_i, g), 7 angle(n_j, g), 8 angle(n_i, n_j),
 *   9 |g|, with angle(a, c) = atan2f(|a x c|, a . c), cross components
 *   a1*c2 - a2*c1 ..., norms sqrtf((v0*v0 + v1*v1) + v2*v2), the dot
 *   ((+0 + a0*c0) + a1*c1) + a2*c2 (the +0 start is the reference's reduction:
 *   products that are all -0 sum to +0), so angle(0, .) = 0.  feat is (b,n,k,C)
 *   with channels_first = 0 and (b,C,k,n) -- the Conv2d layout of TFMR.py:71 --
 *   with channels_first = 1.  Channels 0-5 are exact; 6-9 up to the device's
 *   atan2f / sqrtf.
 *
 * pcr_knn_graph: the k-nearest-neighbour graph of get_graph_features
 *   (ngenet/models/information_interactive.py:7-23, called twice by
 *   GCN.forward, :107-130) without a (b,n,n) array or a sort.  xyz (b,n,3) f32,
 *   1 <= k <= 63, kk = min(k, n - 1).  For every point i, all n points of its
 *   cloud, i included, are ordered by the pair (d2(x_i, x_j), j) ascending;
 *   row i of idx (b,n,kk) i32 holds ranks 1 .. kk of that order.  Rank 0 is
 *   dropped, as the reference drops column 0 of its topk: without coincident
 *   points it is i itself; with coincident points it is the lowest-index point
 *   at distance 0 and the row may then contain i (the reference's choice there
 *   is an unspecified topk tie).  d2 (b,n,kk) f32 or NULL receives the
 *   distances of those ranks, ascending.  Exact and deterministic: every key
 *   of a row is distinct, so no chunking or scheduling can change the result.
 *   kk = 0 (n = 1) or b = 0 returns PCR_OK with no launch and needs no
 *   pointers.  No scratch.
 *
 * pcr_edge_features: the gather of get_graph_features.  feats (b,n,c) f32,
 *   c >= 1; idx (b,n,kk) i32 with 0 <= idx < n (a PRECONDITION like pcr_fps's
 *   start: the kernel clamps the values into [0, n) so that it never reads
 *   outside the cloud), 0 <= kk <= 63.  With channels_first = 0, out is
 *   (b,n,kk,2c): out[..., :c] = f_i and out[..., c:] = f_j - f_i, one f32
 *   subtraction, j = idx[b][i][rank].  With channels_first = 1 the same values
 *   as (b,2c,n,kk), what GCN feeds its Conv2d after
 *   .permute(0, 3, 1, 2).contiguous().  Every value is exact; element offsets
 *   are 64-bit.  kk = 0 or b = 0 returns PCR_OK with no launch.
 *
 * Both validate before any device work: a bad argument sets pcr_last_error
 *   ("k=64 outside 1..63", "null pointer", ...) and returns PCR_ERR_ARG.
 * ------------------------------------------------------------------------- */
int pcr_fps(const float *xyz, const int32_t *start, int32_t b, int32_t n, int32_t m, int32_t *idx,
            pcr_stream_t stream);
int pcr_ball_query(const float *xyz, const float *query, int32_t b, int32_t n, int32_t q, float r2,
                   int32_t k, int32_t *idx, int32_t *count, pcr_stream_t stream);
int pcr_group_ppf(const float *xyz, const float *normals, int32_t b, int32_t n, float r2, int32_t k,
                  int32_t channels_first, float *feat, int32_t *idx, pcr_stream_t stream);
int pcr_knn_graph(const float *xyz, int32_t b, int32_t n, int32_t k, int32_t *idx, float *d2,
                  pcr_stream_t stream);
int pcr_edge_features(const float *feats, const int32_t *idx, int32_t b, int32_t n, int32_t c,
                      int32_t kk, int32_t channels_first, float *out, pcr_stream_t stream);

/* ---------------------------------------------------------------------------
 * Similarity top-k matching: the correspondence stage of ROPNet's
 * TFMRModule.forward (ROPNet/src/models/TFMR.py:226-257) -- bmm similarity, row
 * maxima, the sort that keeps the most confident source rows, topk, the
 * index_put mask, the normalisation and the bmm against the target points --
 * without any (b,n1,m1) tensor.  Its outputs (src[sel], tgt_corr, the overlap
 * scores at sel) are what pcr_procrustes_batch consumes.
 *
 * Inputs.  fx (b,n1,c), fy (b,m1,c) f32: the normalised, gathered features
 *   (c = 5 x feat_dim = 960 in the reference); tgt (b,m1,3) f32.
 * Similarity.  S[i][j] is the f32 fmaf chain over ch = 0 .. c-1 ascending from
 *   +0: s = fmaf(x[i][ch], y[j][ch], s).  One accumulator of
 *   v_mfma_f32_32x32x2_f32 carried through every k-step computes exactly that
 *   (one rounding per product, subnormals kept), so there is no error bound
 *   and no rescan, and a CPU restatement matches bit for bit.  No split-K.
 * Top-k.  Per row the k largest by (S descending, j ascending); -0 equals +0
 *   (and is reported as +0), so ties go to the lowest index.  val (b,n1,k)
 *   f32 and idx (b,n1,k) i32, both in that order.
 * Row selection.  The rows of a batch ordered by (val[.][0] descending, i
 *   ascending); sel (b,n_keep) i32 holds the first n_keep.  The caller
 *   computes n_keep = int(top_prob * n1).
 * Weights and correspondences, per kept row, f32, every operation rounded:
 *   sum = ((v0 + v1) + ...) in top-k order, den = sum + 1e-8f, w_t = v_t / den
 *   (correctly rounded), tgt_corr[d] = ((w0 t0[d]) + w1 t1[d]) + ... with
 *   t_t = tgt[idx_t].  Negative or zero sums are not special-cased: the
 *   formulas are the reference's.
 * Non-finite features: values unspecified; every index stays in range, sel
 *   stays distinct, every kernel terminates.
 * Limits.  1 <= k <= 8, k <= m1; n1, m1 in 1 .. 2^24; c in 1 .. 65536 (looped in
 *   chunks of 32); 0 <= n_keep <= n1; b x ceil(n1 / 128) x ceil(m1 / 128) < 2^31.
 *   Anything else returns PCR_ERR_ARG with its message before any device work.
 *   b = 0 (and, for the selection, n_keep = 0) returns PCR_OK without a launch.
 *
 * pcr_tfmr_scratch_bytes: the bytes of the caller's scratch for these sizes
 *   (8 b n1 (ceil(m1 / 128) k + 1), rounded up to 256: the target tiles' lists
 *   and one key per row; nothing proportional to n1 m1), or -1 on bad sizes.
 * pcr_similarity_topk: val and idx of every row.  scratch: that many bytes,
 *   256-byte aligned, device memory; the call leaves the rows' selection keys
 *   in it.
 * pcr_tfmr_select: sel, w (b,n_keep,k), tgt_corr (b,n_keep,3) and idx_keep
 *   (b,n_keep,k), the kept rows' idx.  val, idx and scratch are the ones a
 *   pcr_similarity_topk call with the same b, n1, m1, k filled (on the same
 *   stream, or ordered behind it): the selection reads the keys it left.
 * Both are asynchronous on `stream`.
 * ------------------------------------------------------------------------- */
int64_t pcr_tfmr_scratch_bytes(int32_t b, int32_t n1, int32_t m1, int32_t c, int32_t k);
int pcr_similarity_topk(const float *fx, const float *fy, int32_t b, int32_t n1, int32_t m1, int32_t c,
                        int32_t k, float *val, int32_t *idx, void *scratch, pcr_stream_t stream);
int pcr_tfmr_select(const float *val, const int32_t *idx, const float *tgt, int32_t b, int32_t n1,
                    int32_t m1, int32_t k, int32_t n_keep, int32_t *sel, float *w, float *tgt_corr,
                    int32_t *idx_keep, const void *scratch, pcr_stream_t stream);

/* ---------------------------------------------------------------------------
 * Coherent Point Drift (Myronenko & Song 2010), the second alignment method of
 * the reference (DataPreparation/CPD.py:26-73 runs probreg's RigidCPD, AffineCPD
 * and NonRigidCPD on cupy in f32).  probreg is not available to this project, so
 * the contract below is CPD as published with probreg's conventions as far as
 * they are known; it is NOT pinned against probreg's own outputs.  The f64
 * restatement is tests/cpd_ref.py.
 *
 * Layout.  src (P,Mmax,3) f32 is Y, the set that moves, with n_src (P) valid
 *   points; tgt (P,Nmax,3) f32 is X with n_tgt (P).  n_src / n_tgt are device
 *   arrays or NULL (= all Mmax / Nmax points).  Rows past a pair's count are
 *   never read.  P <= 65535, Mmax, Nmax <= 2^24, 0 <= w < 1.
 * E-step at a transform T and sigma2, per pair (M = n_src, N = n_tgt):
 *   y^_m = (float)(T y_m), T applied in f64 as ((T0 x + T1 y) + T2 z) + T3;
 *   d_mn = (dx dx + dy dy) + dz dz in f32, every operation rounded;
 *   k_mn = exp(-d_mn / (2 sigma2)); c = (2 pi sigma2)^1.5 w / (1 - w) M / N;
 *   den_n = sum_m k_mn, replaced by FLT_EPSILON where it is 0;
 *   Pt1_n = den_n / (den_n + c); P1_m = sum_n k_mn / (den_n + c);
 *   PX_m = sum_n k_mn x_n / (den_n + c); Np = sum_m P1_m.
 *   A term whose argument is below -87 may be kept, flushed or skipped.
 *   No (M,N) array is formed.  The kernels evaluate k as one exp2 of
 *   fmaf(d, hi, d lo) with (hi, lo) the f32 pair of -log2(e) / (2 sigma2), add
 *   terms in f32 in groups of four consecutive points ((k0 + k1) + (k2 + k3)),
 *   the groups of a 512-point chunk in f64 in order, and the
 *   chunks in f64 in order; 1 / (den_n + c) is rounded to f32 before the row
 *   sums.  The row sweep sums, with v = k_mn / (den_n + c) in f32, the moments
 *   sum v, sum v (y^_m - x_n) and sum v d_mn, which are of the size of the
 *   residual and not of the clouds; P1_m = sum v and
 *   PX_m = P1_m y^_m - sum v (y^_m - x_n) in f64, then rounded to f32.  Np adds
 *   the f32 P1 in f64 (lane t of 256 adds t, t + 256, ...; halving tree).
 *   That order does not depend on P or on how a launch is split, and
 *   there are no float atomics: one call returns the same bytes every time and a
 *   pair's result does not depend on what else is in the batch.
 * Loop (pcr_cpd_register).  sigma2 starts at sum_mn |x_n - y_m|^2 / (3 M N) in
 *   f64 (on the sources as given, not on init's image of them) and T at init
 *   (P,16 row-major 4x4, rows 0..2 read) or the identity.  An iteration is the
 *   E-step at (T, sigma2) and the M-step in f64 from the row sweep's f64
 *   moments (P1, PX and sum_n v |x_n|^2 per source, before any rounding to f32):
 *   mux = sum PX / Np, muy = Y^T P1 / Np, Yc = Y - muy,
 *   A = PX^T Yc - mux (P1^T Yc), G = Yc^T dP1 Yc, and
 *   trXPX = sum Pt1_n |x_n - mux|^2.  Over the targets some source reaches
 *   (den_n != 0, where Pt1_n = sum_m v) it is evaluated as
 *   sum_mn v |x_n|^2 - Np |mux|^2, i.e. under the same weights v as P1 and PX,
 *   so that the residual below is a sum of squares under one set of weights and
 *   keeps its digits when sigma2 is far below the clouds' extent; the targets
 *   no source reaches (den_n = 0, v = 0 in every row) add their
 *   Pt1_n |x_n - mux|^2 with Pt1_n = eps / (eps + c), in f64, in a pass over the
 *   targets.  (That rule makes an outlier target pull sigma2 up once c falls
 *   towards FLT_EPSILON, for w > 0 as for w = 0; it is the contract's.)
 *   kind 0 (rigid): R = argmax tr(A^T R) over rotations (Horn's quaternion
 *     method, the optimum U diag(1,1,det(U V^T)) V^T), s = 1,
 *     sigma2 = (trXPX - 2 tr(A^T R) + tr G) / (3 Np);
 *   kind 1 (rigid + scale): s = tr(A^T R) / tr G,
 *     sigma2 = (trXPX - s tr(A^T R)) / (3 Np);
 *   both: B = s R, t = mux - B muy,
 *     q = (trXPX - 2 s tr(A^T R) + s^2 tr G) / (2 sigma2) + 1.5 Np ln sigma2;
 *   kind 2 (affine): B = A G^-1, t = mux - B muy,
 *     sigma2 = (trXPX - tr(A B^T)) / (3 Np),
 *     q = (trXPX - 2 tr(A B^T) + tr(B G B^T)) / (2 sigma2) + 1.5 Np ln sigma2;
 *   sigma2 is floored at FLT_EPSILON before q.  After the M-step of iteration
 *   i >= 1 (0-based) a pair stops if |q_i - q_(i-1)| < tol; tol <= 0 never stops
 *   (exactly maxiter iterations).  Every pair stops on its own and a stopped
 *   pair's outputs no longer change.
 *
 * pcr_cpd_scratch_bytes: the bytes of the caller's scratch for these sizes, or
 *   -1 on bad sizes.  No (M,N) array: the state records, inv, Pt1, P1, PX, the
 *   five f64 row moments per source and one f64 per target, 256 + 56 Mmax +
 *   16 Nmax bytes a pair.  On top of that, a sweep whose launch would have fewer than
 *   512 workgroups (P ceil(lanes / 256) < 512: a small batch of large clouds) is
 *   split over workgroups and keeps one f64 partial per lane and 512-point chunk
 *   of the staged axis, not per slice, because that is what makes the sums'
 *   order independent of P: 8 P Nmax ceil(Mmax / 512) bytes for the column sweep
 *   and 40 P Mmax ceil(Nmax / 512) for the row sweep.  That term is a product
 *   of both sizes.  It is bounded only by the split condition (P lanes < 131072):
 *   1 MiB + 5 MiB at P = 1 and 8192 x 8192, about 0.9 GB at P = 1 and
 *   100000 x 100000; batches of 512 / ceil(lanes / 256) pairs or more never pay it.
 * pcr_cpd_estep: one E-step.  T (P,16) f64 or NULL (the sources are already
 *   transformed; the non-rigid path); sigma2 (P) f64 device.  Outputs pt1
 *   (P,Nmax), p1 (P,Mmax), px (P,Mmax,3) f32 and n_p (P) f64; a pair with an
 *   empty cloud leaves its rows untouched.
 * pcr_cpd_register: the loop, maxiter x (column sweep, row sweep, M-step)
 *   enqueued on `stream` from a per-pair f64 state record in scratch; nothing
 *   goes through the host, and the sequence can be captured in a graph.  When
 *   the stream is not capturing and tol > 0, the count of stopped pairs is
 *   read after every eighth iteration (one stream synchronisation) and the
 *   launches left are dropped once every pair has stopped.  Outputs per pair:
 *   T (16 f64 row-major, B in the 3x3 block), scale (s; 1 for kinds 0 and 2),
 *   sigma2, q, iters (iterations run) and status: 0 ok; 1 n_src or n_tgt is 0
 *   (the pair's other outputs are left alone); 2 sigma2 or q became non-finite
 *   (the pair stops, T and scale keep the last finite iterate, sigma2 and q
 *   report the values that ended it).  maxiter = 0 returns init and the initial
 *   sigma2 with q = 0.
 * scratch: pcr_cpd_scratch_bytes(P, Mmax, Nmax) bytes of device memory,
 *   256-byte aligned.  All calls are asynchronous on `stream` except for the
 *   read described above.
 * ------------------------------------------------------------------------- */
int64_t pcr_cpd_scratch_bytes(int32_t P, int32_t Mmax, int32_t Nmax);
int pcr_cpd_estep(const float *src, const float *tgt, int32_t P, int32_t Mmax, int32_t Nmax,
                  const int32_t *n_src, const int32_t *n_tgt, const double *T, const double *sigma2,
                  double w, float *pt1, float *p1, float *px, double *n_p, void *scratch,
                  pcr_stream_t stream);
int pcr_cpd_register(const float *src, const float *tgt, int32_t P, int32_t Mmax, int32_t Nmax,
                     const int32_t *n_src, const int32_t *n_tgt, int32_t kind, double w,
                     int32_t maxiter, double tol, const double *init, double *T, double *scale,
                     double *sigma2, double *q, int32_t *iters, int32_t *status, void *scratch,
                     pcr_stream_t stream);

/* ---------------------------------------------------------------------------
 * KPConv forward and the neighbour max-pool of NgeNet's encoder: what
 * KPConv.forward and MaxPoolBlock.forward
 * (c2p-net/ngenet/models/KPConv/blocks.py:73-128, 182-188) compute from the
 * input pyramid (pcr_radius_neighbors builds its index tables), for inference,
 * without the (n,k,C_in) gather, the (n,k,K,3) differences or the (n,K,C_in)
 * kernel features in global memory.  The f64 restatement is
 * tests/kpconv_conv_ref.py.
 *
 * Inputs.  q_pts (n,3), s_pts (m,3), s_feats (m,c_in), kernel_points (K,3),
 *   weights (K,c_in,c_out): f32, row-major.  neigh_inds (n,k): int32 or int64,
 *   index_width = 4 or 8 bytes per index.
 * Pads.  An index outside [0, m) -- the reference's m, and any negative or larger
 *   value -- is a pad: it contributes nothing and is never dereferenced.
 * Influence of a real neighbour j on kernel point e, f32, every operation
 *   rounded: d2 = (dx dx + dy dy) + dz dz + 1e-8 with d = (s_j - q) - kp_e;
 *   h = max(0, 1 - sqrt(d2) / kp_extent) for PCR_KP_LINEAR, h = 1 for
 *   PCR_KP_CONSTANT (aggregation 'sum'; 'cloest' is not built).
 * Output.  out[i][o] = (sum_e sum_c (sum_j h[i][j][e] f[j][c]) W[e][c][o]) / cnt_i,
 *   cnt_i = max(1, #{real j : rowsum(f[j][:]) > 0}), rowsum the f32 sum of the
 *   support row in ascending channel order (a row summing to <= 0 is not
 *   counted; a query without counted neighbours divides by 1).  A query whose
 *   neighbours are all pads gives exact zeros.
 * Numerics.  f32 throughout; both contractions are f32 MFMA fmaf chains
 *   (v_mfma_f32_16x16x4_f32): over j ascending, then over (e, c) in passes of
 *   up to 64 channels; where a workgroup holds 32 output channels or fewer the
 *   (e, c) chain is split over two or four interleaved slices that are added in
 *   slice order.  The order depends on the sizes only and there are no atomics:
 *   two calls return the same bytes.  Against the f64
 *   restatement every output is within
 *   2^-24 sum_{j,e,c} ((k + K c_in + 16) h + 8) |f| |W| / cnt.
 * Non-finite inputs: values unspecified; every access stays in range and every
 *   kernel terminates.
 * Limits.  1 <= K <= 16, 1 <= k <= 256, c_in and c_out in 1 .. 2048 (no multiple
 *   of anything), m in 1 .. 2^24, n in 0 .. 2^24, kp_extent > 0 for the linear
 *   influence.  Anything else, or a null pointer, returns PCR_ERR_ARG with its
 *   message before any device work; n = 0 returns PCR_OK without a launch.
 * row_flags: m bytes of device scratch, the call's only one: a pre-pass writes
 *   rowsum > 0 per support row, the convolution is the second launch.
 *
 * pcr_neighbor_max: out[i][ch] = max_j feats[inds[i][j]][ch] over the k columns,
 *   a pad reading 0; feats (m,c) f32, out (n,c) f32.  Same index rule, widths
 *   and limits, with c in 1 .. 4096.  Exact on finite data (of equal values the
 *   first column's is returned).  No (n,k,c) tensor, no scratch.
 * Both are asynchronous on `stream`.
 * ------------------------------------------------------------------------- */
#define PCR_KP_LINEAR 0
#define PCR_KP_CONSTANT 1
int pcr_kpconv_forward(const float *q_pts, const float *s_pts, const float *s_feats, const void *neigh_inds,
                       int32_t index_width, int32_t n, int32_t m, int32_t k, const float *kernel_points,
                       const float *weights, int32_t K, int32_t c_in, int32_t c_out, float kp_extent,
                       int32_t influence, void *row_flags, float *out, pcr_stream_t stream);
int pcr_neighbor_max(const float *feats, const void *inds, int32_t index_width, int32_t n, int32_t m,
                     int32_t k, int32_t c, float *out, pcr_stream_t stream);

/* ---------------------------------------------------------------------------
 * Softmax attention without the score matrix: NgeNet's Cross_Attention and
 * overlap scores (c2p-net/ngenet/models/information_interactive.py:165-214,
 * NgeNet.py:170-179) and ROPNet's OverlapAttentionBlock
 * (ROPNet/src/models/TFMR.py:76-106), for inference.  No allocation
 * proportional to n m is made or needed.  The f64 restatement with the derived
 * bound is tests/attention_ref.py.
 *
 * Layout.  Every tensor is f32, channel-major with UNIT TOKEN STRIDE: element
 *   (batch, head, channel, token) of x is x[batch x_sb + head x_sh + channel x_sc
 *   + token], the strides in elements.  That takes the (B, dim, nhead, N) view of
 *   a Conv1d output (x_sh = N, x_sc = nhead N) and column slices of a wider
 *   tensor without a copy.  Strides are not checked: every element they name
 *   must lie in the tensor.  out must not overlap an input.
 *
 * pcr_attention_forward:
 *   out[b,h,c,i] = sum_j P_ij v[b,h,c,j],  P = softmax_j(scale sum_e q[b,h,e,i] k[b,h,e,j])
 *   with i < n queries, j < m keys, e < d, c < dv.
 * pcr_offset_attention_forward (no heads):
 *   a_ij = r_i sum_e q[b,e,i] k[b,e,j]   (row_scale r: (b, n) with batch stride
 *                                         r_sb, unit stride over i; null: r = 1)
 *   P = softmax_j(a),  c_j = sum_i P_ij,
 *   out[b,ch,j] = (sum_i v[b,ch,i] P_ij) / (1e-9f + c_j)       i, j < n.
 *
 * Numerics.  f32 throughout.  Scores are the f32 MFMA's fmaf chain over e
 *   ascending (v_mfma_f32_32x32x2_f32), times scale (r_i), each rounded.  Keys
 *   are walked in tiles of 32 with an online softmax: per tile the running
 *   maximum is raised, the sum and the accumulators are multiplied by
 *   expf(old max - new max) and the tile's weights expf(score - max) are added;
 *   expf is the library's (1 ulp), there is no deferred rescale.  P V is a second
 *   f32 MFMA chain over j ascending (dv <= 4: separately rounded multiply-adds),
 *   the quotient one f32 division.  Where b h ceil(n / 128) ceil(dv / 64) <= 64
 *   and m > 224 (8 tiles) the keys are split into up to 16 runs of whole tiles whose
 *   (accumulator, maximum, sum) partials go through `scratch` and are combined in
 *   run order.  The offset form's sweep 1 computes the rows' maxima and sums
 *   the same way into `scratch`; sweep 2 forms P_ij = expf(a_ij - max_i) *
 *   (1 / sum_i) and accumulates c_j and the numerator over i ascending.
 *   Every order depends on the sizes only and there are no atomics: two calls
 *   return the same bytes, and a batch element's result does not depend on b
 *   as long as the split (a function of b h n m dv) is the same.
 *   A key past m (a row past n) has weight exactly +0; no exp sees -inf - -inf.
 *   Bound against the f64 restatement: tests/attention_ref.py.
 * Non-finite inputs: the rows (columns) they touch are unspecified, possibly
 *   NaN; every access stays in range and every kernel terminates.
 * Limits.  b >= 0, h >= 1, d and dv in 1 .. 256, n in 0 .. 2^24, m in 1 .. 2^24.
 *   Anything else, or a null pointer, returns PCR_ERR_ARG with its message before
 *   any device work; b = 0 or n = 0 returns PCR_OK without a launch (m = 0 is
 *   an error).
 * Scratch.  pcr_attention_scratch_bytes: 0 unless the keys are split, then
 *   splits b h (dv + 2) n floats (at most 16 (1 + 2 / dv) times the output;
 *   the split needs the grid to be at most 64 workgroups).  A null scratch is
 *   accepted when it is 0.  pcr_offset_attention_scratch_bytes: 8 b n bytes.
 *   Both return -1 on bad sizes; scratch must be 16-byte aligned.
 * Both calls are asynchronous on `stream`.
 * ------------------------------------------------------------------------- */
int64_t pcr_attention_scratch_bytes(int32_t b, int32_t h, int32_t n, int32_t m, int32_t d, int32_t dv);
int pcr_attention_forward(const float *q, int64_t q_sb, int64_t q_sh, int64_t q_sc, const float *k,
                          int64_t k_sb, int64_t k_sh, int64_t k_sc, const float *v, int64_t v_sb,
                          int64_t v_sh, int64_t v_sc, float *out, int64_t o_sb, int64_t o_sh,
                          int64_t o_sc, int32_t b, int32_t h, int32_t n, int32_t m, int32_t d,
                          int32_t dv, float scale, void *scratch, pcr_stream_t stream);
int64_t pcr_offset_attention_scratch_bytes(int32_t b, int32_t n, int32_t d, int32_t dv);
int pcr_offset_attention_forward(const float *q, int64_t q_sb, int64_t q_sc, const float *k, int64_t k_sb,
                                 int64_t k_sc, const float *v, int64_t v_sb, int64_t v_sc,
                                 const float *row_scale, int64_t r_sb, float *out, int64_t o_sb,
                                 int64_t o_sc, int32_t b, int32_t n, int32_t d, int32_t dv,
                                 void *scratch, pcr_stream_t stream);

/* ---------------------------------------------------------------------------
 * DIP's PointNet descriptor forward (dip/network.py:50-100) in eval mode, for
 * inference: per patch x (3, P)
 *   T-net (tnet = 1):  3 -> 128 -> 256, max over points, -> 128 -> 9, + I = T
 *   xtrans = T x                                 (tnet = 0: xtrans = x)
 *   main:  3 -> 128 -> 256, max and argmax over points (mx, amx),
 *          -> 128 (hid) -> dim (f), l2-normalised where l2norm = 1.
 * Every layer but the last of a branch is followed by ReLU; BatchNorm (eval)
 * is folded into the weights by the caller.  No allocation proportional to
 * B P C is made or needed: no per-point activation reaches global memory.  The
 * f64 restatement with the derived bounds is tests/pointnet_ref.py.
 *
 * Weights.  pcr_pointnet_layers holds one branch: w1 (128, 3), w2 (256, 128),
 *   w3 (128, 256), w4 (dim, 128) -- (9, 128) in the T-net -- row-major (out, in),
 *   and the biases b1 .. b4; f32 device pointers, folded (W' = W s, b' = (b -
 *   mean) s + beta with s = gamma / sqrt(var + eps)).  pcr_pointnet_weights is a
 *   HOST struct of the two branches; `stn` is not read when tnet = 0.
 * Input.  Element (b, coord, point) of x is x[b x_sb + coord x_sc + point x_sp],
 *   strides in elements: a contiguous (B, 3, P) tensor and the transposed view
 *   of a (B, P, 3) one both go in without a copy.  Strides are not checked.
 * Outputs.  f (B, dim), mx (B, 256) required; amx (B, 256) int32, hid (B, 128)
 *   (fc1's post-ReLU output of the main branch), trans (B, 9) (written when
 *   tnet = 1 only) and xtrans (B, 3, P) may be null.  All contiguous.
 *
 * Numerics.  f32 throughout.
 *   Layer.  y[o] = b'[o] + sum_c W'[o][c] h[c] is one f32 fmaf chain over c
 *     ascending that STARTS from the bias: fmaf(W'[o][2], h[2], fmaf(W'[o][1],
 *     h[1], fmaf(W'[o][0], h[0], b'[o]))) ...  The 3-input layers run on the
 *     VALU (fmaf), every other layer on v_mfma_f32_32x32x2_f32 with the bias as
 *     the accumulator's initial value (k-step t adds channels 2 t, then 2 t + 1).
 *     ReLU is max(y, +0).
 *   Pool.  mx[o] is the maximum over points 0 .. P - 1 of conv2's post-ReLU
 *     output, amx[o] the lowest point index attaining it.  Points are walked in
 *     tiles of 64; those of a partly filled tile past P do not take part.
 *   Transform.  trans = t + I, one f32 add per element (the zeros of I too);
 *     xtrans[r][p] = (T[r][0] x[0][p] + T[r][1] x[1][p]) + T[r][2] x[2][p],
 *     every product and sum rounded.
 *   Normalisation.  f / max(sqrt(sum_o f[o]^2), 1e-12f): the squares, each
 *     rounded, are added to +0 over o ascending, one rounded add each; sqrt and
 *     the division are correctly rounded.
 *   Order.  Every order depends on (P, dim, tnet, l2norm) only and there are
 *     no atomics: two calls return the same bytes, and a patch's bytes do not
 *     depend on B or on its position in the batch.
 *   Composition.  A tnet = 1 call returns the same bytes as: (1) this entry
 *     with the T-net's four layers as `main`, tnet = 0, l2norm = 0, dim = 9;
 *     (2) trans = f + I and the transform above in f32 on the host; (3) this
 *     entry with the main layers, tnet = 0, on that xtrans.
 * Non-finite inputs: the patch's values are unspecified; every access stays in
 *   range and every kernel terminates.
 * Limits.  B in 0 .. 2^20, P in 1 .. 4096, dim in 1 .. 256.  Anything else, or a
 *   null required pointer (x, f, mx, w, a layer of a branch in use, scratch
 *   when tnet = 1), returns PCR_ERR_ARG with its message before any device work;
 *   B = 0 returns PCR_OK without a launch.
 * Scratch.  pcr_pointnet_scratch_bytes: 0 when tnet = 0, else B (256 + 16) floats
 *   (the T-net's pooled vector and matrix), rounded up to 256 bytes; -1 on bad
 *   sizes.  Scratch must be 16-byte aligned.
 * The call is asynchronous on `stream`.
 * ------------------------------------------------------------------------- */
typedef struct pcr_pointnet_layers {
    const float *w1, *b1, *w2, *b2, *w3, *b3, *w4, *b4;
} pcr_pointnet_layers;

typedef struct pcr_pointnet_weights {
    pcr_pointnet_layers stn;   /* the T-net: w4 (9, 128), b4 (9) */
    pcr_pointnet_layers main;  /* w4 (dim, 128), b4 (dim) */
} pcr_pointnet_weights;

int64_t pcr_pointnet_scratch_bytes(int32_t B, int32_t dim, int32_t tnet);
int pcr_pointnet_forward(const float *x, int64_t x_sb, int64_t x_sc, int64_t x_sp, int32_t B, int32_t P,
                         const pcr_pointnet_weights *w, int32_t dim, int32_t tnet, int32_t l2norm, float *f,
                         float *mx, int32_t *amx, float *hid, float *trans, float *xtrans, void *scratch,
                         pcr_stream_t stream);

/* ---------------------------------------------------------------------------
 * The consumers of the grouping front ends, fused for inference: the edge conv
 * of NgeNet's GCN (c2p-net/ngenet/models/information_interactive.py:107-130)
 * and the grouped local-feature MLP behind NgeNet's PPF (:26-84) and ROPNet's
 * LocalFeatue (ROPNet/src/models/TFMR.py:17-73).  Both norms take their
 * statistics over the whole cloud (no running statistics), so nothing folds
 * into the weights; no allocation proportional to n kk c or n K c is made or
 * needed.  The f64 restatement with the derived bounds is tests/groupmlp_ref.py.
 *
 * pcr_edge_conv: per cloud, point i, neighbour j = idx[i][e] (e < kk) and
 *   output channel o, with W = [Wa | Wb] of shape (co, 2 c) row-major, no bias:
 *     y[i][e][o] = sum_k Wa[o][k] f[i][k] + sum_k Wb[o][k] (f[j][k] - f[i][k])
 *     out[i][o]  = max_e lrelu(instance_norm(y)[i][e][o])
 *   the norm over all n kk values of (cloud, channel), biased variance, no affine.
 * pcr_group_mlp: x (b, n, K, cin) channels last (pcr_group_ppf's layout with
 *   channels_first = 0); `layers` (1 .. 3) times
 *     y_l = W_l h_{l-1}  (no bias),  h_l = act(norm(y_l)),  h_0 = x
 *   the norm over all n K values of (cloud, channel) (group = 1: InstanceNorm2d)
 *   or of (cloud, 32 consecutive channels) (group = 32: GroupNorm(c / 32, c)),
 *   with the optional affine gamma, beta (c_l) (null: 1, 0);
 *     out[i][o] = max_k h_L[i][k][o].
 *   act(v) = v for v > 0, else slope v (slope = 0: +0, ReLU).
 *
 * How it is computed (what the contract fixes).
 *   Layer.  Every y is ONE f32 fmaf chain over the input channels ascending from
 *     +0: layer 1 of the MLP on the VALU, every other product on
 *     v_mfma_f32_32x32x2_f32 (k-step t adds channels 2 t, then 2 t + 1).
 *   Edge conv.  P[i][o] = chain over Wa[o][.] f[i][.], Q[i][o] = chain over
 *     Wb[o][.] f[i][.]; R = P - Q (one f32 subtraction); y = R[i] + Q[j] (one f32
 *     add), the row's kk neighbours in order.  An index is clamped into [0, n)
 *     as pcr_edge_features does.
 *   Statistics.  Per (cloud, channel) sum y and sum y^2 are f64 sums of the f32
 *     y (the square formed in f64, exact): rows in ascending order within a
 *     tile; the tiles' partials are added in 16 runs of ceil(tiles / 16)
 *     consecutive tiles, each in ascending tile order, and the runs' sums in
 *     run order; with group = 32 the 32 channel sums are then added over
 *     channels ascending.  mean = S / m,
 *     var = S2 / m - mean^2 (clamped at 0), rstd = 1 / sqrt(var + eps), all f64.
 *   Coefficients.  a = gamma rstd, b = beta - mean (gamma rstd), computed in
 *     f64 and each rounded ONCE to f32.  h = act(fmaf(y, a, b)).
 *   Pool.  y -> act(fmaf(y, a, b)) is monotone, rounding included, so
 *     out = act(fmaf(a >= 0 ? max y : min y, a, b)) over the neighbours equals
 *     the max of the activated values bit for bit; only max and min of the last
 *     layer's y are kept per (point, channel).
 *   Tiles.  The MLP walks the cloud's n K rows in tiles of 64: K <= 64 puts
 *     floor(64 / K) whole points in a tile, K > 64 splits a point into
 *     ceil(K / 64) tiles.  The edge conv's statistics tile is 8 points.  The map
 *     depends on (n, K) only, never on the grid or on b; rows of a partly
 *     filled tile take no part in the statistics or the pool.  No atomics.
 *     A pass recomputes the layers before it (pass l: layers 1 .. l), with the
 *     same code, from finished coefficients.
 *   Consequences: two calls return the same bytes; a cloud's bytes do not depend
 *     on b or on its position in the batch; the y_1, y_2 of a 3-layer call equal
 *     byte for byte those of the 1- and 2-layer calls on the same leading layers.
 * Layout.  feats: element (batch, point, channel) is feats[batch f_sb + point
 *   f_sp + channel f_sc] (strides in elements, not checked), so (b, n, c) and
 *   (b, c, n) tensors both go in without a copy.  idx (b, n, kk) int32, x, the
 *   weights (c_l, c_{l-1}) row-major and every output are contiguous.  out is
 *   (b, n, c_L), or (b, c_L, n) with channels_first = 1.
 * Optional outputs (null in normal use; each is written by the stage itself):
 *   rq (b, n, 2 co): R | Q of the edge conv; y[l] (b, n, K, c_l): the pre-norm
 *   activations; stats (b, co, 2) / stats[l] (b, c_l / group, 2): f64 (mean, var).
 * Non-finite inputs: the clouds they touch are unspecified; every access stays
 *   in range and every kernel terminates.
 * Limits.  b in 0 .. 65535, n in 2 .. 2^20, kk in 1 .. 63, K in 1 .. 128, cin in
 *   1 .. 16, every width (c, co, c_l) a multiple of 32 in 32 .. 512, group 1 or
 *   32, eps >= 0.  Anything else, or a null required pointer, returns
 *   PCR_ERR_ARG with its message before any device work; b = 0 returns PCR_OK
 *   without a launch.
 * Scratch (16-byte aligned; the functions return -1 on bad sizes, the text in
 *   pcr_last_error).  pcr_edge_conv_scratch_bytes: R | Q, max, min (4 b n co
 *   floats), a | b (2 b co floats) and the partials (2 b ceil(n / 8) co
 *   doubles): no term in kk.  pcr_group_mlp_scratch_bytes: a | b per layer,
 *   max and min (2 b n ceil(K / 64) c_L floats) and the per-tile partials
 *   (2 b tiles max c_l doubles, tiles = ceil(n / floor(64 / K)) or n ceil(K / 64)):
 *   the only terms in K, one 64th of a materialised activation.
 * Both calls are asynchronous on `stream`.
 * ------------------------------------------------------------------------- */
typedef struct pcr_group_mlp_net {
    int32_t layers;         /* 1 .. 3 */
    int32_t width[3];       /* c_l */
    const float *w[3];      /* (c_l, c_{l-1}), c_0 = cin */
    const float *gamma[3];  /* (c_l) or null */
    const float *beta[3];   /* (c_l) or null */
    float *y[3];            /* optional (b, n, K, c_l) */
    double *stats[3];       /* optional (b, c_l / group, 2) */
} pcr_group_mlp_net;        /* a HOST struct of device pointers */

int64_t pcr_edge_conv_scratch_bytes(int32_t b, int32_t n, int32_t kk, int32_t c, int32_t co);
int pcr_edge_conv(const float *feats, int64_t f_sb, int64_t f_sp, int64_t f_sc, const int32_t *idx, int32_t b,
                  int32_t n, int32_t kk, int32_t c, int32_t co, const float *w, double eps, float slope,
                  int32_t channels_first, float *out, float *rq, double *stats, void *scratch,
                  pcr_stream_t stream);
int64_t pcr_group_mlp_scratch_bytes(int32_t b, int32_t n, int32_t K, int32_t layers, int32_t c1, int32_t c2,
                                    int32_t c3);
int pcr_group_mlp(const float *x, int32_t b, int32_t n, int32_t K, int32_t cin, const pcr_group_mlp_net *net,
                  int32_t group, double eps, float slope, int32_t channels_first, float *out, void *scratch,
                  pcr_stream_t stream);

/* ---------------------------------------------------------------------------
 * The unary family of NgeNet's KPConv blocks and decoder, fused for inference
 * (c2p-net/ngenet/models/KPConv/blocks.py:135-290, NgeNet.py:185-212): rows
 * times a weight, the norm over the whole stacked cloud, the residual add and
 * the LeakyReLU.  UnaryBlock, BatchNormBlock, the residual add of
 * ResnetBottleneckBlock and NearestUpsampleBlock + torch.cat + UnaryBlock are
 * each ONE call; the up-sampled rows and the concatenated operand are never in
 * global memory.  The f64 restatement with the derived bounds is
 * tests/unary_ref.py.
 *
 * pcr_unary_forward: for row i < n and output channel o < cout
 *     row_i     = [ x0[g0 ? g0[i] : i][0 .. c0) | x1[i][0 .. c1) ]
 *     y[i][o]   = sum_c w[o][c] row_i[c]          (w null: y[i][o] = row_i[o])
 *     pre[i][o] = norm ? fmaf(y, a[o], b[o]) : y + bias[o]   (bias null: y)
 *     z         = res ? pre + res[i][o] : pre
 *     out[i][o] = act ? (z > 0 ? z : slope z) : z
 *   the norm an InstanceNorm1d without affine over the n rows (biased variance).
 *
 * How it is computed (what the contract fixes).
 *   Product.  f32 in, f32 accumulate, on v_mfma_f32_32x32x2_f32, the exact-f32
 *     MFMA: per element one chain over the c0 + c1 inputs ascending from +0
 *     (k-step t adds inputs 2 t, then 2 t + 1; the concat seam may fall inside
 *     a k-step).  The gather and the concat happen while a 64-row tile is
 *     staged into LDS, 32 inputs at a time; inputs past c0 + c1, channels past
 *     cout and rows past n are staged as +0.  A g0[i] outside [0, m0) reads a
 *     row of zeros (KPConv's shadow row; the reference would raise).  Every
 *     access stays in range for any index value.
 *   Statistics.  Per channel sum y and sum y^2 are f64 sums of the f32 y (the
 *     square formed in f64, exact): rows in ascending order within a tile of 64
 *     rows; the tiles' partials are added in 16 runs of ceil(tiles / 16)
 *     consecutive tiles, each in ascending tile order, and the runs' sums in
 *     run order (the finalize kernel pcr_group_mlp uses).  mean = S / n,
 *     var = S2 / n - mean^2 (clamped at 0), rstd = 1 / sqrt(var + eps), all
 *     f64; a = rstd and b = -mean rstd are each rounded ONCE to f32.  No
 *     atomics.  Tile t is rows 64 t .. 64 t + 63: the map depends on n only,
 *     never on the grid.
 *   Apply.  pre = fmaf(y, a, b) with norm, else y + bias (one f32 add);
 *     z = pre + res (one f32 add); out = z > 0 ? z : slope z (one f32 product).
 *   Passes.  (1) product tile -> the raw y written to out, and the tile's
 *     partials; (2) finalize; (3) apply in place over out.  With norm = 0
 *     pass 1 alone writes the final value.  Pass 3 reads out back: it does not
 *     recompute the product, because the blocks' input is wider than their
 *     output (DESIGN.md "Unary blocks").  w null: (1') statistics of the rows
 *     themselves, (2), and (3) reading the rows where they are.
 *   Consequences: two calls return the same bytes; the bytes do not depend on
 *     the launch grid; y and stats of a call equal those of the same call
 *     without res and act; out of a call without norm, res and act equals
 *     y + bias bit for bit.
 * Layout.  x0 (m0, c0) and x1 (n, c1) with row strides ld0, ld1 in elements
 *   (>= c0, c1); g0 (n) int32; w (cout, c0 + c1) row-major (nn.Linear's);
 *   bias (cout); res, out and y (n, cout) contiguous; stats (cout, 2) f64
 *   (mean, var), only with norm.  out may not overlap an input except res.
 * Non-finite inputs: unspecified values; every access stays in range and every
 *   kernel terminates.
 * Limits.  n in 0 .. 2^22 (n >= 2 with norm: torch's InstanceNorm1d refuses one
 *   spatial element), m0 >= 1, c0 >= 1, c1 >= 0, c0 + c1 <= 2048, cout in
 *   1 .. 1024, eps >= 0, |slope| <= 1.  bias together with norm, stats without
 *   norm, w null with cout != c0 + c1, g0 null with m0 != n, x1 null with
 *   c1 != 0, or a null required pointer (args, x0, out, scratch) returns
 *   PCR_ERR_ARG with its message before any device work; n = 0 returns PCR_OK
 *   without a launch.
 * Scratch (16-byte aligned): a | b (2 cout floats) and the per-tile partials
 *   (2 ceil(n / 64) cout doubles).  pcr_unary_scratch_bytes returns -1 on bad
 *   sizes, the text in pcr_last_error.
 * The call is asynchronous on `stream`.
 * ------------------------------------------------------------------------- */
typedef struct pcr_unary_args {          /* a HOST struct of device pointers */
    int32_t n, m0, c0, c1, cout;
    const float *x0; int64_t ld0;        /* (m0, c0), row stride in elements */
    const int32_t *g0;                   /* (n) or null: row i reads x0[g0[i]], else x0[i] (then m0 == n) */
    const float *x1; int64_t ld1;        /* (n, c1) or null with c1 = 0 */
    const float *w;                      /* (cout, c0 + c1) row-major, or null: y = the row itself */
    const float *bias;                   /* (cout) or null; only with norm = 0 */
    int32_t norm; double eps;            /* InstanceNorm over the n rows, biased variance */
    int32_t act; float slope;            /* LeakyReLU, applied last */
    const float *res;                    /* (n, cout) contiguous or null */
    float *out;                          /* (n, cout) contiguous */
    float *y; double *stats;             /* optional: raw pre-norm y, (cout, 2) f64 mean / var */
} pcr_unary_args;

int64_t pcr_unary_scratch_bytes(int32_t n, int32_t cout);
int pcr_unary_forward(const pcr_unary_args *a, void *scratch, pcr_stream_t stream);

/* ---------------------------------------------------------------------------
 * Point-wise convolutions of ROPNet (CG.py:15-106, TFMR.py:76-130), fused for
 * inference: a Conv1d(k = 1) weight times channel-major clouds (B, C, N), the
 * GroupNorm over (cloud, channel group, all points), the biases, the
 * (Leaky)ReLU, the residual add BEHIND it and the max over points, as ONE
 * call.  The operand is up to five sources side by side, each optionally
 * minus a second tensor: torch.cat([x1 .. x5]), x - x_r and the
 * (B, 6144, N) ensemble of the CG's overlap decoder are never in global
 * memory.  The f64 restatement with the derived bounds is
 * tests/pointwise_ref.py.
 *
 * pcr_pointwise_forward: for cloud b, output channel o < cout, point i < n
 *     row[c]       = concat over s < nsrc of src_s[b][c][i] - (sub_s ? sub_s[b][c][i] : 0),  c < cin = sum c_s
 *     y[b][o][i]   = sum_c w[o][c] row[c]
 *     t            = (y + bias[o]) + cbias[b][o]        (two rounded f32 adds; null: skipped)
 *     pre          = gw ? fmaf(t, A[b][o], Bc[b][o]) : t
 *     z            = act ? (pre > 0 ? pre : slope pre) : pre
 *     out[b][o][i] = res ? z + res[b][o][i] : z          (the residual after the activation, TFMR.py:104-105)
 *     cmax[b][o]   = max_i out[b][o][i]                  (optional)
 *   the norm a GroupNorm over gw consecutive channels (cout % gw == 0) times the
 *   n points of one cloud, its statistics those of t (a Conv1d bias in front
 *   of a GroupNorm shifts a group's mean), biased variance, affine gamma /
 *   beta (null: 1, 0).
 *
 * How it is computed (what the contract fixes).
 *   Product.  f32 in, f32 accumulate, on v_mfma_f32_32x32x2_f32 with w as the A
 *     operand: per element one fmaf chain over the cin inputs ascending from +0
 *     (k-step t adds inputs 2 t, then 2 t + 1; a seam between sources may fall
 *     inside a k-step).  src - sub is one rounded f32 subtraction made while a
 *     64-point tile is staged into LDS, 32 inputs at a time; inputs past cin,
 *     channels past cout and points past n are staged as +0.  For n <= 4 the
 *     same chain runs on the VALU (fmaf(w, x, acc), the tail padded with +0 to
 *     the same multiple of 32): the same bytes as the tile path.
 *   Statistics.  f64 sums of t and t^2 (the square formed in f64, exact) per
 *     (cloud, 64-point tile, channel), points ascending; a channel's tiles are
 *     added as pcr_unary_forward's are (16 runs, norm_finalize.h), a group's
 *     channels ascending.  mean = S / (n gw), var = S2 / (n gw) - mean^2
 *     (clamped at 0), A = gamma / sqrt(var + eps), Bc = beta - mean A, in f64,
 *     each rounded ONCE to f32.  No atomics; tile t is points 64 t .. 64 t + 63.
 *   Passes.  (1) product tile -> t written to out, and the partials;
 *     (2) finalize; (3) apply in place over out.  With gw = 0 pass 1 alone
 *     writes the final values.
 *   cmax.  The maximum of each (tile, channel) from -inf, then the tiles in
 *     order: a max is exact in any order.  No float atomics.
 *   Consequences: two calls return the same bytes; the bytes do not depend on
 *     the launch grid; a cloud computed alone has the bytes it has inside a
 *     batch; sources given in pieces or minus a sub have the bytes of the
 *     same call on the materialised torch.cat / difference.
 * Layout.  Every source, sub, res and out has a batch stride and a channel
 *   stride in elements (any value; 0 repeats) and point stride 1.  w (cout, cin)
 *   row-major (nn.Conv1d's) with row stride w_ld in cin .. 8192 (a column slice
 *   of a wider weight is read where it lies); bias, gamma, beta (cout); cbias, cmax (b, cout);
 *   y (b, cout, n) contiguous; stats (b, cout / gw, 2) f64 (mean, var).  out may
 *   not overlap an input except res.
 * Non-finite inputs: unspecified values; every access stays in range and every
 *   kernel terminates.
 * Limits.  b in 0 .. 65535, n in 0 .. 2^22, nsrc in 1 .. 5, every c_s >= 1,
 *   cin <= 8192, cout in 1 .. 2048, eps >= 0, |slope| <= 1.  gamma / beta /
 *   stats without a norm, a gw that does not
 *   divide cout, out null other than with cmax and gw = 0, or a null required
 *   pointer returns PCR_ERR_ARG with its message before any device work; b = 0
 *   or n = 0 returns PCR_OK without a launch.
 * Scratch (16-byte aligned): A | Bc (2 b cout floats) and the per-tile partials
 *   (2 b ceil(n / 64) cout doubles; the tiles' maxima take their place once they
 *   are finalized).  Nothing is proportional to cin n.
 *   pcr_pointwise_scratch_bytes returns -1 on bad sizes, the text in
 *   pcr_last_error.
 * The call is asynchronous on `stream`.
 * ------------------------------------------------------------------------- */
#define PCR_POINTWISE_MAX_SOURCES 5
typedef struct pcr_pointwise_args {      /* a HOST struct of device pointers */
    int32_t b, n, nsrc, cout;
    int32_t c[PCR_POINTWISE_MAX_SOURCES];            /* channels of source s */
    const float *src[PCR_POINTWISE_MAX_SOURCES];
    int64_t src_bs[PCR_POINTWISE_MAX_SOURCES], src_cs[PCR_POINTWISE_MAX_SOURCES];
    const float *sub[PCR_POINTWISE_MAX_SOURCES];     /* null: nothing subtracted */
    int64_t sub_bs[PCR_POINTWISE_MAX_SOURCES], sub_cs[PCR_POINTWISE_MAX_SOURCES];
    const float *w; int64_t w_ld;        /* (cout, cin) row-major, row stride in elements */
    const float *bias, *cbias;           /* (cout), (b, cout) or null */
    int32_t gw; double eps;              /* GroupNorm over gw channels x n points; 0: none */
    const float *gamma, *beta;           /* (cout) or null */
    int32_t act; float slope;
    const float *res; int64_t res_bs, res_cs;        /* or null */
    float *out; int64_t out_bs, out_cs;
    float *cmax;                         /* (b, cout) or null */
    float *y; double *stats;             /* optional: the raw product y, (b, cout / gw, 2) f64 mean / var of t */
} pcr_pointwise_args;

int64_t pcr_pointwise_scratch_bytes(int32_t b, int32_t n, int32_t cout);
int pcr_pointwise_forward(const pcr_pointwise_args *a, void *scratch, pcr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PCR_API_H */
