/*
 * rsm.h -- C ABI of librsm_mi355.so: the MI355X-native (gfx950 / HIP) drop-in for the
 * CStereoMatching pyramidal dense-stereo path of seed93/reconstruction.
 *
 * The reference has no FFI layer; the seam this library replaces is the C++ class
 * surface the orchestrator uses (reference file:line, relative to the reference root):
 *   CStereoMatching::Init(...)            reconstruction/CStereoMatching.h:47, .cpp:5-13
 *   CStereoMatching::MatchAllLayer()      reconstruction/CStereoMatching.h:48, .cpp:15-34
 *   public fields Q,R_final,T_final,margin[2],MatchBlockRadius,m_ws,m_offset,Verbose
 *                                         reconstruction/CStereoMatching.h:38-45
 *   downstream contract: per emitted point CCloudOptimization::InsertPoint(3x1 CV_64F) in
 *   row-major pixel order (.cpp:749-751), cam[pair][v].bound = margin[v] (.cpp:27-28).
 * include/CStereoMatchingMI355.hpp is a header-only C++ adapter with exactly that surface
 * built on these entry points; INTEGRATION.md shows the patch a maintainer would apply.
 *
 * All entry points return 0 on success or a negative rsm_status; the library never calls
 * exit() (the reference does at CStereoMatching.cpp:827-830 -> RSM_E_DEGENERATE_MARGIN).
 * Plain pointers and sizes only; no C++ or torch types cross this boundary.
 * One rsm_ctx per GPU; a ctx is not re-entrant (like CStereoMatching), different ctxs
 * may be driven from different threads.
 */
#ifndef RSM_H
#define RSM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSM_NOMATCH (-10000) /* NOMATCH, reconstruction/CStereoMatching.h:9 */
#define RSM_MAX_LEVELS 12

typedef enum rsm_status {
    RSM_OK = 0,
    RSM_E_INVALID = -1,           /* bad argument */
    RSM_E_DEGENERATE_MARGIN = -2, /* YL>=YR || XL>=XR (reference: exit(0), .cpp:827-830) */
    RSM_E_HIP = -3,               /* HIP runtime error (rsm_last_error() has the text) */
    RSM_E_NOMEM = -4,
    RSM_E_STATE = -5,             /* call order (e.g. run before upload) */
    RSM_E_COMM = -6,              /* RCCL missing or failed (rsm_comm_last_error() has the text) */
    RSM_W_NOT_CONVERGED = 1       /* rsm_poisson_mesh / rsm_stage_poisson_solve: max_cycles reached above rel_residual; the results are valid */
} rsm_status;

/* struct Boundary, reconstruction/CManageData.h:10-14 (same field order) */
typedef struct rsm_boundary {
    int YL, YR, XL, XR;
    int width, height;
} rsm_boundary;

/* Inputs of one stereo pair = what MatchAllLayer reads after Rectify()
 * (.cpp:20: cam[pair][v].image/.mask, Q, R_final, T_final) + the Init() parameters. */
typedef struct rsm_pair_in {
    const uint8_t *image[2]; /* rectified top-level BGR 8UC3, row-major, stride 3*width  */
    const uint8_t *mask[2];  /* rectified+eroded top-level mask 8UC1, stride width       */
    int width, height;       /* top level = m_LowestLevelSize * 2^(m_PyrmNum-1) (.cpp:120) */
    int pyr_levels;          /* m_PyrmNum                                                */
    int radius;              /* MatchBlockRadius (Init radii; CReconstruction.cpp:17: 2)  */
    double ws;               /* m_ws (CReconstruction.cpp:17: 0.03)                       */
    int offset;              /* m_offset (CStereoMatching.h:47: 2)                        */
    int origin_width;        /* m_OriginSize.width (scale of .cpp:692)                    */
    double Q[16];            /* 4x4 row-major, after the sign flip of .cpp:138            */
    double R_final[9];       /* 3x3 row-major (.cpp:132)                                  */
    double T_final[3];       /* (.cpp:133)                                                */
    int verbose;             /* Verbose (.cpp:12)                                         */
} rsm_pair_in;

/* Outputs of one pair. Buffers are caller-allocated; NULL skips that output.
 * ZERO-INITIALISE the struct (memset / = {0}) before filling it in: the library reads EVERY pointer member, and members are
 * appended as the ABI grows -- `points16` came with ABI 2 (RSM_ABI_VERSION / rsm_abi_version(); a caller compiled against
 * the ABI 1 header, whose struct ends at v_top, must be rebuilt: an ABI 2 library reads 8 bytes beyond its struct). */
#define RSM_ABI_VERSION 2
typedef struct rsm_pair_out {
    double *disparity[2];   /* width*height fp64 each: disparity[0|1] after the last level  */
    rsm_boundary margin[2]; /* margin[0|1] at the top level (-> cam[pair][v].bound)         */
    int64_t n_points;       /* points DisparityToCloud emits (.cpp:732-759)                  */
    int64_t max_points;     /* capacity of xyz / bgr in points                               */
    double *xyz;            /* 3*max_points fp64: R_final*X + T_final, InsertPoint order     */
    uint8_t *bgr;           /* 3*max_points: colour of imagePyrm[top][0] (.cpp:756)          */
    int64_t v_top;          /* masked view-0 pixels inside margin[0] at the top level        */
    struct rsm_point16 *points16; /* max_points 16-byte records {float x, y, z; u8 b, g, r, pad}: the cloud as
                             * CCloudOptimization::InsertPoint keeps it (the fp64 point cast to float,
                             * CloudOptimization/CCloudOptimization.cpp:61) + the colour, packed on the GPU --
                             * 16 instead of 27 bytes per point over PCIe; NULL skips it (xyz / bgr likewise)  */
} rsm_pair_out;

typedef struct rsm_ctx rsm_ctx;

/* ---- lifetime --------------------------------------------------------------------------- */
int rsm_create(rsm_ctx **ctx, int hip_device);
void rsm_destroy(rsm_ctx *ctx);
const char *rsm_last_error(const rsm_ctx *ctx);
const char *rsm_version(void);
/* the ABI the library was built with (struct layouts of this header): compare with RSM_ABI_VERSION after loading it */
int rsm_abi_version(void);
/* GPUs visible to this process (hipGetDeviceCount; 0 when there is none or no HIP runtime) */
int rsm_device_count(void);

/* ---- one pair: host buffers in, host buffers out (replaces the loop body .cpp:20-31) ----- */
int rsm_match_pair(rsm_ctx *ctx, const rsm_pair_in *in, rsm_pair_out *out);

/* ---- the same, split so inputs can stay resident in HBM --------------------------------- */
/* H2D of the two rectified images + masks; (re)sizes the ctx workspace. */
int rsm_upload_pair(rsm_ctx *ctx, const rsm_pair_in *in);
/* Same, but image[]/mask[] are DEVICE pointers on this ctx's GPU (copied device-to-device). */
int rsm_upload_pair_device(rsm_ctx *ctx, const rsm_pair_in *in);
/* ConstructPyrm + all MatchOneLayer levels + DisparityToCloud on the resident pair.
 * Synchronous with respect to the host on return. */
int rsm_run_pair(rsm_ctx *ctx);
/* D2H of the results of the last rsm_run_pair. */
int rsm_download_pair(rsm_ctx *ctx, rsm_pair_out *out);
/* Page-locked host memory for the buffers of rsm_pair_in / rsm_pair_out (the reference keeps them in pageable cv::Mat
 * memory, CManageData.cpp:75-78 / CStereoMatching.cpp:21-31: a cv::Mat can wrap memory from rsm_host_alloc, or the memory
 * it already owns can be page-locked in place).  Downloads into page-locked memory run at the link's rate instead of through
 * the runtime's staging copy (a C2 pair's two fp64 maps + cloud: ~7 instead of 34 ms).  NULL / RSM_E_HIP on failure. */
void *rsm_host_alloc(size_t bytes);
void rsm_host_free(void *p);
int rsm_host_register(void *p, size_t bytes);
int rsm_host_unregister(void *p);
/* Device pointers of the last results (valid until the next upload/run/destroy):
 * fp64 disparity maps, n_points, packed cloud xyz (fp64 x3) and bgr (u8 x3). */
int rsm_result_device(rsm_ctx *ctx, const double **disparity0, const double **disparity1,
                      int64_t *n_points, const double **xyz, const uint8_t **bgr);

/* Copies the cloud of the last run device-to-device into caller-owned device buffers (e.g. the
 * buffers an RCCL gather sends from): up to max_points points, xyz fp64 x3 and/or bgr u8 x3. */
int rsm_export_cloud_device(rsm_ctx *ctx, double *d_xyz, uint8_t *d_bgr, int64_t max_points);

/* ---- several pairs at once (the pair loop of MatchAllLayer, .cpp:17-33, has no cross-pair data flow) -------- */
/* rsm_run_pair on n DIFFERENT contexts concurrently (one host thread each; contexts may share a GPU or sit on
 * different ones).  On one GPU two pairs in flight hide each other's launch-latency-bound small levels and host
 * syncs.  Returns the first non-zero status. */
int rsm_run_pairs(rsm_ctx *const *ctxs, int n);
/* Same, every context running its resident pair `repeats` times back to back without meeting the others in between
 * (steady-state throughput of a stream of pairs; bench.py). */
int rsm_run_pairs_repeat(rsm_ctx *const *ctxs, int n, int repeats);
/* The whole loop body for n_pairs pairs over a pool of contexts: a context takes the next pair from a queue as soon as
 * it is free (upload, run, download -- one pair's PCIe copies overlap another pair's kernels).  out[p] is filled as
 * by rsm_match_pair, in pair order, so the caller can replay InsertPoint / filter(CamPair) sequentially afterwards.
 * status (optional, n_pairs ints) receives each pair's status; a failed pair does not stop the others. */
int rsm_match_pairs(rsm_ctx *const *ctxs, int n_ctx, const rsm_pair_in *in, rsm_pair_out *out, int n_pairs, int *status);
/* Same with library-owned contexts: pairs sharded over n_gpus devices of this node (0 = all visible),
 * pairs_in_flight contexts per device (0 = 2) -- the single-process form of SURVEY 8(e); the one-process-per-GPU form
 * is rsm_gather_clouds below. */
int rsm_match_pairs_multi_gpu(const rsm_pair_in *in, int n_pairs, int n_gpus, int pairs_in_flight, rsm_pair_out *out,
                              int *status);

/* ---- multi-GPU, one process per GPU: RCCL gather of the per-pair clouds -------------------------- */
/* The record that travels: what CCloudOptimization::InsertPoint keeps of a point (CloudOptimization/
 * CCloudOptimization.cpp:61: the fp64 point cast to float) plus the colour of imagePyrm[top][0] (.cpp:756). */
typedef struct rsm_point16 {
    float x, y, z;
    uint8_t b, g, r, pad;
} rsm_point16;
/* Packs the cloud of the last rsm_run_pair into 16-byte records in a caller-owned DEVICE buffer (capacity
 * max_points); *n_points receives the number written.  This is the send buffer of rsm_gather_clouds. */
int rsm_pack_cloud16(rsm_ctx *ctx, rsm_point16 *d_dst, int64_t max_points, int64_t *n_points);

#define RSM_COMM_ID_BYTES 128   /* = NCCL_UNIQUE_ID_BYTES */
#define RSM_COMM_MAX_PAIRS 4096 /* pairs per gather */
typedef struct rsm_comm rsm_comm;
/* Rank 0 makes the id (ncclGetUniqueId) and hands its bytes to the other ranks by whatever launcher started them
 * (MPI, a file, torch.distributed's store, ...); then every rank creates its communicator on its GPU. */
int rsm_comm_unique_id(char id[RSM_COMM_ID_BYTES]);
int rsm_comm_create(rsm_comm **comm, const char id[RSM_COMM_ID_BYTES], int rank, int world, int hip_device);
/* The gather protocol is written against this small transport table; rsm_comm_create fills it with RCCL.  A pipeline
 * that already owns a transport (MPI, its own RCCL communicator) -- and the protocol tests, which run world 2/3/8 over
 * an in-process mock on host memory -- hand in theirs.  All functions return 0 or non-zero (failure); `buf` pointers
 * are whatever memory the caller of rsm_gather_clouds passes (device memory for RCCL).
 *   allreduce_sum_i64  in-place sum of n int64 in HOST memory over all ranks (collective)
 *   group_begin/_end   bracket the payload exchange; everything posted in between is complete when group_end returns
 *   send / recv        point-to-point; between one (sender, receiver) pair they match IN POSTING ORDER (RCCL's rule)
 *   copy               local copy (the root's own pairs) */
typedef struct rsm_transport {
    void *self;
    int (*allreduce_sum_i64)(void *self, int64_t *host_buf, int n);
    int (*group_begin)(void *self);
    int (*send)(void *self, const void *buf, uint64_t bytes, int peer);
    int (*recv)(void *self, void *buf, uint64_t bytes, int peer);
    int (*copy)(void *self, void *dst, const void *src, uint64_t bytes);
    int (*group_end)(void *self);
} rsm_transport;
int rsm_comm_create_transport(rsm_comm **comm, const rsm_transport *transport, int rank, int world);
void rsm_comm_destroy(rsm_comm *comm);
const char *rsm_comm_last_error(const rsm_comm *comm);
/* Fan-in of the clouds of all pairs to rank `root` -- the replacement of the global `cloud_in += cloud` accumulation
 * (CCloudOptimization.cpp:61,123) when pairs are sharded one process per GPU.  Every rank passes its n_local clouds
 * (device buffers of 16-byte records, their pair ids in [0, n_pairs_total) IN ANY ORDER, and point counts).  On the
 * root the clouds of ALL pairs arrive in d_out (device, capacity max_out records) in pair order; out_offsets (host,
 * n_pairs_total + 1) receives each pair's first record.  Collective: every rank of the communicator calls it, and
 * every rank returns the SAME status: a bad argument on one rank, a pair claimed by two ranks or a root buffer that
 * is too small make all ranks return RSM_E_INVALID before any payload moves (nobody is left waiting). */
int rsm_gather_clouds(rsm_comm *comm, int root, int n_local, const int *pair_ids, const rsm_point16 *const *d_clouds,
                      const int64_t *n_points, int n_pairs_total, rsm_point16 *d_out, int64_t max_out,
                      int64_t *out_offsets);
/* Counts only: every rank learns the point count of every pair (counts: n_pairs_total int64, host), e.g. to size the
 * root's buffer before rsm_gather_clouds.  Collective, same status on every rank, same checks as the gather. */
int rsm_gather_counts(rsm_comm *comm, int n_local, const int *pair_ids, const int64_t *n_points, int n_pairs_total,
                      int64_t *counts);
/* The transport-free core of rsm_gather_clouds, exposed for tests and for pipelines that post the transfers
 * themselves.  Step 1: every rank fills its contribution to the metadata vector (RSM_GATHER_META_WORDS(P) int64:
 * per pair the point count and the number of claims, the owner's rank, then an error count and the root's capacity);
 * the vectors are summed over the ranks.  Step 2: from the summed vector every rank derives the SAME verdict, the
 * pair offsets, and its own ordered list of transfers: a rank's sends ascend by pair id, and the root posts its
 * receives per peer in that same order -- the order in which point-to-point operations between two ranks match. */
#define RSM_GATHER_META_WORDS(P) (3 * (P) + 2)
typedef struct rsm_gather_op {
    int kind;          /* 0 = send to `peer`, 1 = receive from `peer`, 2 = local copy (root's own pair) */
    int peer;
    int pair;          /* pair id */
    int local_index;   /* index into the caller's local arrays (send / copy), -1 for a receive */
    int64_t offset;    /* first record of the pair in the root's output (receive / copy) */
    int64_t count;     /* records */
} rsm_gather_op;
int rsm_gather_meta_fill(int rank, int world, int root, int n_local, const int *pair_ids, const int64_t *n_points,
                         int n_pairs_total, int64_t max_out, int64_t *meta);
/* offsets: n_pairs_total + 1; ops: capacity max_ops (n_local + n_pairs_total always suffices), *n_ops written.
 * Returns RSM_OK, or RSM_E_INVALID when the summed metadata says the gather must not start (same on every rank). */
int rsm_gather_plan(int rank, int world, int root, int n_local, const int *pair_ids, const int64_t *n_points,
                    int n_pairs_total, const int64_t *meta_summed, int64_t *offsets, rsm_gather_op *ops, int max_ops,
                    int *n_ops);

/* Tuning / validation knobs.  None of them changes a result.  The tests hold every alternative path bit-identical -- the NCC
 * routing options ("wide_rows", "ncc_mid", "ncc_slide_max") on both sides of every threshold of the row routing -- except
 * those of "refine_prefill", "refine_skew_prio", "refine_skew_waves" / "refine_skew_waves_alone", "heavy_*", "shared_gpu"
 * and "filter_low_priority", which no test sets yet:
 *   "ncc_bytes" = 1        the generic byte-wise NCC kernel instead of the dot4 one
 *   "wide_rows" = 0 | 1 | 2 | 3   rows of wide pixels: 0 (default) = chosen per row on the device (k_rg_rows: the sliding window
 *                          sums when the row's widest interval has at most ncc_slide_max candidates and the row holds enough
 *                          wide pixels, the int8 row GEMM on the matrix cores otherwise) / 1 = the one-workgroup-per-pixel kernel
 *                          only / 2 = every such row through the int8 row GEMM / 3 = every such row through the sliding sums;
 *                          "no_rowgemm" = 1 is wide_rows = 1
 *   "ncc_mid" / "ncc_slide_max"   which rows of long-interval pixels leave the band kernel (intervals longer than ncc_mid
 *                          candidates; 0 = by window size from the measured crossover) and which of them take the sliding sums
 *                          (widest interval <= ncc_slide_max, default 512) rather than the int8 row GEMM
 *   "no_exact" = 1         (timing A/B only) skip the reference-order re-evaluation of near-tie pixels
 *   "refine_skew_from" / "refine_skew_T" / "refine_skew_min_px" / "refine_skew_waves" / "refine_skew_rows"   time-skewed refine
 *                          sweeps (k_refine_skew): T (2..4, default 4) sweeps per launch from that sweep of a level on (default
 *                          4; 0 = never) at levels with at least min_px margin pixels per direction (default 1 M: the two
 *                          largest levels of a 12 MP pair; a level narrower than 80 columns never), aiming at `waves` workgroups
 *                          (default 2560: two rounds of the 1280 a chip holds) or `rows` rows per chunk
 *   "refine_rekey_until"   a time-skewed launch that starts before this sweep (default 22; 0 = never, the schedule then wants
 *                          refine_skew_from = 22) is preceded by a re-key pass (k_refine_rekey): each live pixel's data-term cache
 *                          holds its current key and the neighbour key on the side the state is nearest to, so the early launches
 *                          miss at the settled rate.  "refine_rekey_side" = 1 installs the other neighbour instead (tests: a wrong
 *                          prediction costs misses, never bits)
 *   "refine_tile_T" / "refine_tile_from" / "refine_tile_min_px"   the levels BELOW refine_skew_min_px (bound by launch latency:
 *                          a sweep there is a few microseconds of work): T (2..8, default 4; 0 = off, one launch per sweep)
 *                          sweeps per launch on overlapped tiles (k_refine_tile: a workgroup stages a 32 x 16 tile grown by T
 *                          pixels and sweeps it T times in LDS) from that sweep of a level on (default 4), at levels with at least
 *                          min_px margin pixels per direction (default 0); the launches that start before "refine_rekey_until" are
 *                          preceded by the re-key pass, leftover sweeps run one per launch
 *   "refine_skew_waves_low"   the workgroups a time-skewed launch aims at on the levels below the top while other contexts of
 *                          the device are inside rsm_run_pair (default 640: C2's level 3 then runs 83-row chunks instead of 20-row
 *                          ones, fewer recomputed halo rows; a pair alone keeps "refine_skew_waves_alone"); 0 = the top level's aim
 *   "refine_upd_cap"       n > 0: a shard of the sweep kernels' cache-update list holds at most n records (tests: a full list
 *                          drops records, which costs later cache misses and never bits); 0 (default) = what was allocated
 *   "refine_skew_uw"       columns a strip of that kernel owns: 0 (default) = 66 - 2T, all that its last sweep can compute from 64
 *                          lanes; an even number below that (e.g. 56: every strip starts on a 128-byte line of the cache ways) for A/B
 *   "refine_skew_waves_alone"  the workgroups a time-skewed launch aims at while no other context of the device is inside
 *                          rsm_run_pair (default 3840; with pairs in flight `refine_skew_waves` applies); 0 = the same
 *   "refine_skew_prio"     p > 0: the time-skewed kernel's waves rotate their issue priority (s_setprio) every 2^p shader clocks, in step
 *                          over the whole chip, so that the workgroups of a CU -- which the hardware serves oldest first -- advance
 *                          alike; 0 (default) = off: it equalises them as designed and gains 7 % on a single round of workgroups,
 *                          nothing on the default two rounds
 *   "cu_share" = n         n > 1: the context's streams are confined to one of n equal shares of the compute units (the
 *                          context's creation ordinal on its device picks the share; measured slower than sharing the whole
 *                          chip in turns, profiles/LAB_NOTES.md 4); 0 / 1 = the whole chip.  The masked streams are BLOCKING streams
 *                          (hipExtStreamCreateWithCUMask has no non-blocking flag): legacy null-stream work of the process then
 *                          synchronises with them.  RSM_E_STATE while the context is inside rsm_run_pair
 *   "filter_list"          ... its list passes (a thread per query the tile pass left over, windows read from the lattice copy): bit 0
 *                          the 49 x 49 pass, bit 1 the 81 x 81 pass on what that leaves, bit 2 (needs bit 0 or a 24-pixel tile pass)
 *                          a wave per query over windows of 80, 160, 320 ... pixels for the few hundred those leave, then the
 *                          whole-chip search for the handful beyond -- no grid level at all; bits 3 / 4: the 49 x 49 / 81 x 81 pass in
 *                          that wave form too instead of a thread per query (coalesced reads of the lattice rows; on C2's cloud the
 *                          81 x 81 pass gains, 1.4 against 3.9 ms, the 49 x 49 pass does not); default 23, 0 = tile pass + grid ladder only
 *   "filter_wg_max"        ... the wave passes run four waves per query (the first pass over the window shared, a 4 096-entry selection list)
 *                          while at most this many queries are left: default 2048; 0 = always a wave per query (A/B; the same bits)
 *   "filter_normals_window" rsm_filter_last_cloud: the normals' radius search reads the pixel lattice (the k-nearest pass's copy, the removed
 *                          points blanked) while no point needs a window wider than this many pixels -- default 8, at most 40; beyond it, or
 *                          with 0, the filtered cloud is sorted into a grid of radius-cells as for a generic cloud (C2: 0.15 against 1.8 ms)
 *   "filter_low_priority"  1 (default): rsm_filter_last_cloud runs on a stream of the lowest priority the device offers -- with pairs in
 *                          flight the dispatcher then hands compute units to the other contexts' matching first (the adapter loop with
 *                          the filter inside: 36 C2 pairs, 6 in flight, 219 against 215 Mdisp/s; 5 in flight 210 against 196); 0: on the
 *                          context's own stream.  The environment variable RSM_FILTER_LOW_PRIORITY=0/1 sets the default of contexts
 *                          created afterwards (for callers that reach the library through the adapter only)
 *   "filter_window"        rsm_filter_last_cloud's pixel-window pass: 1 (default) radius from a sparse probe (remembered by the context:
 *                          probed again on every 8th call, for another k or image size, when it stops deciding 70 % of the queries and
 *                          after any "filter_*" option), 0 off (the generic grid
 *                          search decides every query), 7 / 12 / 16 / 20 / 24 that radius
 *   "filter_ladder_h"      rsm_filter_cloud / rsm_filter_last_cloud: the bit pattern of a positive finite float32 pins the search radius
 *                          of the k-nearest grid ladder's first level (each further level doubles it; its cells are a hair wider, see
 *                          csrc/cloud_grid.h); 0 (default) = from the cloud's sampled extent.  Route only: a level decides a query
 *                          only with all of its k + 1 nearest in hand, so the results are the same bits (tests; rsm_filter_last_grid)
 *   "shared_gpu" = 1       the caller's hint that other contexts use this context's GPU (pairs in flight): the lone-pair split
 *                          below is never used, whatever the library's own count says at the moment a level is enqueued;
 *                          rsm_run_pairs / rsm_match_pairs derive the same per call from their pool (the option stays as the caller
 *                          set it), RsmStereoAdapter sets it for its slots when it creates them
 *   "refine_prefill"       1 (default): the first sweep of a level also fills the second cache way (0: A/B)
 *   "refine_split"         1 (default): a pair that has the GPU to itself (no other context of the device inside rsm_run_pair,
 *                          no per-launch timing) runs the two directions of its time-skewed sections as separate launch chains
 *                          on its two streams (one's low-occupancy tail beside the other's head: one C2 pair 24.1 -> 23.0 ms);
 *                          not used with pairs in flight (measured slower there): the library counts the contexts of the device
 *                          that are inside rsm_run_pair when a level is enqueued, and "shared_gpu" rules it out altogether
 *   "heavy_exclusive" = 0 | 1 | 2   contexts sharing a GPU: no turns / the top level's refine sweeps take turns (default) /
 *                          every large level's; "heavy_min_px", "heavy_from_sweep" bound the sections that take turns;
 *                          "heavy_lanes" = 2 (default): a level's single-sweep part (fabric-bound) and its time-skewed part
 *                          (issue-bound) take turns separately, so one pair's may run beside the other kind of another pair's */
int rsm_set_option(rsm_ctx *ctx, const char *name, long long value);

/* ---- measurement ------------------------------------------------------------------------- */
/* Per-stage device time of the rsm_run_pair calls since the last rsm_profile_enable (which zeroes the counters),
 * measured with hipEvents on the ctx stream.
 * Enable before the run (on = 1: every stage and every 8th launch of the dominant kernel; on = 2: the latter only).
 * Stage names: rsm_profile_stage_name(i), i < rsm_profile_stage_count(). */
int rsm_profile_enable(rsm_ctx *ctx, int on);
int rsm_profile_stage_count(void);
const char *rsm_profile_stage_name(int stage);
/* ms[i] = summed device milliseconds of stage i, launches[i] = kernel launches in it,
 * bytes[i] = algorithmic bytes (SURVEY 8(d) model) those launches moved. */
int rsm_profile_get(rsm_ctx *ctx, double *ms, int64_t *launches, double *bytes);

/* ---- per-stage entry points (one direction; host buffers) for parity tests --------------- */
/* own/oth = margin[!IsZeroOne] / margin[IsZeroOne] of the reference functions. */
int rsm_stage_find_margin(rsm_ctx *ctx, const uint8_t *mask, int W, int H, int r, rsm_boundary *m);
int rsm_stage_pyr_down(rsm_ctx *ctx, const uint8_t *src, int W, int H, int channels, uint8_t *dst);
int rsm_stage_erode_ellipse(rsm_ctx *ctx, const uint8_t *mask, int W, int H, int ksize, uint8_t *dst255);
/* the NCC window-sum tables of one BGR image as the matchers build them: S1 / S2[y W + x] = sum / sum of squares of the (2r+1)^2 x 3 bytes
 * centred on (x, y), 0 where the window leaves the image; r in 1..15 */
int rsm_stage_box_sums(rsm_ctx *ctx, const uint8_t *img_bgr, int W, int H, int r, int32_t *S1, int32_t *S2);
int rsm_stage_initial_match(rsm_ctx *ctx, const uint8_t *img_own, const uint8_t *img_oth,
                            const uint8_t *mask_own, const uint8_t *mask_oth, int W, int H, int r,
                            int offset, const rsm_boundary *own, const rsm_boundary *oth,
                            const double *parent /* NULL = lowest level */, int Wp, int Hp,
                            int16_t *disp);
/* What the last rsm_stage_initial_match on this context decided, per row y < H (H = that call's): wide[y] = pixels that left
 * the band kernel, mid[y] = pixels whose interval is longer than the effective ncc_mid, widest[y] = the widest interval
 * (mid and widest stay 0 with wide_rows = 1, which skips that count), route[y] = 0 no wide pixel / 1 the one-workgroup-per-pixel
 * kernel / 2 the int8 row GEMM / 3 the sliding sums (-1: listed for both); *worklist = wide pixels appended in all, *ties =
 * pixels handed to the reference-order re-evaluation.  RSM_E_STATE before the first such call, RSM_E_INVALID for another H. */
int rsm_stage_last_ncc_routes(rsm_ctx *ctx, int H, int32_t *wide, int32_t *mid, int32_t *widest, int32_t *route,
                              int64_t *worklist, int64_t *ties);
int rsm_stage_smooth(rsm_ctx *ctx, int16_t *disp, int W, int H, const rsm_boundary *own);
int rsm_stage_order(rsm_ctx *ctx, int16_t *disp, int W, int H, const rsm_boundary *own);
int rsm_stage_uniqueness_pass_s16(rsm_ctx *ctx, int16_t *p, const int16_t *q, int W, int H,
                                  const rsm_boundary *own, const rsm_boundary *oth);
int rsm_stage_uniqueness_pass_f64(rsm_ctx *ctx, double *p, const double *q, int W, int H,
                                  const rsm_boundary *own, const rsm_boundary *oth);
int rsm_stage_set_boundary(rsm_ctx *ctx, const int16_t *disp, const uint8_t *mask_own, int W, int H,
                           const rsm_boundary *own, const rsm_boundary *oth, int16_t *BL, int16_t *BR);
int rsm_stage_rematch(rsm_ctx *ctx, const uint8_t *img_own, const uint8_t *img_oth,
                      const uint8_t *mask_own, const uint8_t *mask_oth, int W, int H, int r,
                      const rsm_boundary *own, const rsm_boundary *oth, int16_t *disp);
int rsm_stage_median(rsm_ctx *ctx, int16_t *disp, const uint8_t *mask_own, int W, int H,
                     const rsm_boundary *own);
int rsm_stage_refine(rsm_ctx *ctx, const int16_t *disp_in, const uint8_t *img_own,
                     const uint8_t *img_oth, int W, int H, int iterations, double ws,
                     const rsm_boundary *own, double *disp_out);
/* the specified exp(-t) of DisparityRefine's weights (CStereoMatching.cpp:665-666 call exp) on n values */
int rsm_stage_exp_neg(rsm_ctx *ctx, const double *t, int64_t n, double *out);
/* the same through the form the time-skewed refine kernel's common path evaluates (arguments below 512: no special-case code) */
int rsm_stage_exp_neg_small(rsm_ctx *ctx, const double *t, int64_t n, double *out);
/* DisparityRefine's two divisions (CStereoMatching.cpp:669,671) as the time-skewed kernel evaluates them on its common path --
 * the hardware's fp64 division sequence without its operand-scaling and fix-up steps -- beside the compiler's a / b, on n operand
 * pairs: the parity tests hold the two equal bit for bit over the operand range the kernel's guard admits */
int rsm_stage_div_unscaled(rsm_ctx *ctx, const double *a, const double *b, int64_t n, double *q_fast, double *q_ieee);
/* the cloud filter's square root (PCL's statistical outlier removal sums sqrt of float32 squared distances,
 * CCloudOptimization.cpp:25-61 via pcl::StatisticalOutlierRemoval) -- the compiler's correctly rounded sequence without its
 * denormal scaling -- against sqrtf on the n floats with bit patterns first_bits .. first_bits + n - 1: *mismatches = how many differ */
int rsm_stage_sqrt_check(rsm_ctx *ctx, uint32_t first_bits, int64_t n, int64_t *mismatches);
/* the cloud filter's split of a window candidate c into (row, column) (csrc/win_index.h: a multiplication and, for windows past
 * ~1625 pixels a side, one correction step) against the device's own c / ncx and c % ncx for every c < ncx * ncy (< 2^31):
 * *mismatches = how many differ */
int rsm_stage_win_index_check(rsm_ctx *ctx, int ncx, int ncy, int64_t *mismatches);
/* DisparityRefine's matching costs xi = (1 - arma::dot(vecL, vecR) / (normL * normR)) / 2 (CStereoMatching.cpp:624-629) of 3x3x3
 * windows, as the device restatements of the data term compute them (form 0: the first sweep's, 1: a lane per cache miss, 2: four
 * lanes per cache miss): out[c][((y-1) (W-2) + (x-1)) (W-2) + col] = xi(own column x, row y, other view's window left edge col + c),
 * c = 0..2, y in [1, H-1), x in [1, W-1), col in [0, W-3]; out holds 3 (H-2) (W-2)^2 doubles.  BGR images, W x H x 3. */
int rsm_stage_refine_xi(rsm_ctx *ctx, const uint8_t *img_own, const uint8_t *img_oth, int W, int H, int form, double *out);
int rsm_stage_cloud(rsm_ctx *ctx, const double *disp, const uint8_t *mask_org, const uint8_t *img_own,
                    int W, int H, const double *Q, double scale, const double *R_final,
                    const double *T_final, const rsm_boundary *own, double *xyz, uint8_t *bgr,
                    int64_t max_points, int64_t *n_points);

/* ---- Rectify (CStereoMatching::Rectify, reconstruction/CStereoMatching.cpp:117-168) -------- */
typedef struct rsm_rectify_in {
    double K[2][9];                   /* cam[pair][v].MatIntrinsics, row-major 3x3 (CManageData.cpp:59)   */
    double E[2][12];                  /* cam[pair][v].MatExtrinsics, row-major 3x4 (CManageData.cpp:60)   */
    int origin_width, origin_height;  /* m_OriginSize: size of the raw images (CManageData.cpp:68-69)     */
    int lowest_width, lowest_height;  /* m_LowestLevelSize                                                */
    int pyr_levels;                   /* m_PyrmNum                                                        */
    const uint8_t *image[2];          /* raw BGR images (cv::imread, .cpp:146), origin size, host memory  */
    const uint8_t *mask[2];           /* raw grey masks (.cpp:155), origin size, host memory              */
} rsm_rectify_in;

typedef struct rsm_rectify_out {
    double Q[16];                     /* after the sign flip of .cpp:138                                  */
    double R_final[9], T_final[3];    /* .cpp:132-133                                                     */
    double P[2][12];                  /* cam[pair][v].P after .cpp:143-145                                */
    int width, height;                /* largestSize (.cpp:120)                                           */
    uint8_t *image[2];                /* optional host copies of cam[pair][v].image, width*height*3       */
    uint8_t *mask[2];                 /* optional host copies of cam[pair][v].mask (eroded), width*height */
} rsm_rectify_out;

/* Rectifies one pair on the GPU (host fp64 stereoRectify, device maps / remap / mask erosion) and leaves the
 * rectified images resident exactly as rsm_upload_pair would, with Q / R_final / T_final set: rsm_run_pair
 * can follow directly.  radius / ws / offset / verbose are CStereoMatching::Init's parameters. */
int rsm_rectify_pair(rsm_ctx *ctx, const rsm_rectify_in *in, int radius, double ws, int offset, int verbose,
                     rsm_rectify_out *out);
/* cv::stereoRectify(K1, 0, K2, 0, (nx, ny), R, T, R1, R2, P1, P2, Q, flags = 0, alpha = -1) -- host only. */
int rsm_stereo_rectify(const double *K1, const double *K2, int nx, int ny, const double *R, const double *T,
                       double *R1, double *R2, double *P1, double *P2, double *Q);
/* stage entry points for the parity tests */
int rsm_stage_rect_map(rsm_ctx *ctx, const double *A, const double *R, const double *newA, int W, int H,
                       int16_t *map1, uint16_t *map2);
int rsm_stage_remap(rsm_ctx *ctx, const uint8_t *src, int Ws, int Hs, int channels, const int16_t *map1,
                    const uint16_t *map2, int W, int H, uint8_t *dst);
int rsm_stage_erode_gray(rsm_ctx *ctx, const uint8_t *src, int W, int H, int ksize, uint8_t *dst);

/* ---- cloud interchange ----------------------------------------------------- */
/* Writes the debug / interchange PLY of CStereoMatching::DisparityToCloud (.cpp:723-729 header, :754-756
 * records): binary_little_endian, per vertex float x,y,z (the fp64 point cast to float, .cpp:754) and uchar
 * blue,green,red.  Host-only (no GPU needed). Returns 0 or RSM_E_INVALID. */
int rsm_write_ply(const char *path, const double *xyz, const uint8_t *bgr, int64_t n_points);
/* the same file from 16-byte records (rsm_pair_out.points16: float xyz + BGR = one PLY vertex each) */
int rsm_write_ply16(const char *path, const struct rsm_point16 *points, int64_t n_points);

/* ---- per-pair cloud filter (CCloudOptimization::filter, CloudOptimization/CCloudOptimization.cpp:82-121) -- */
typedef struct rsm_filter_params {
    int sor_mean_k;        /* m_sor_meank  (CReconstruction.cpp:18: 100) */
    double sor_std_mul;    /* m_sor_stdThres (1) */
    double normal_radius;  /* m_mls_radius (2.5): NormalEstimation's search radius, .cpp:107 */
    float cam_center[3];   /* cam[pair][0].CamCenter (CManageData.cpp:61-62): the normals are turned toward it, .cpp:114-121 */
} rsm_filter_params;
/* StatisticalOutlierRemoval + radius-search PCA normals + the turn toward CamCenter on a cloud of n float points
 * (host buffers; PointXYZ order = InsertPoint order).  kept_index (capacity n) receives the indices of the points
 * that survive the outlier removal, in order; normals (capacity 4 * n floats) their (nx, ny, nz, curvature).
 * stats (optional, 4 doubles): mean, stddev, threshold of the mean-neighbour distances, points searched exhaustively. */
int rsm_filter_cloud(rsm_ctx *ctx, const float *xyz, int64_t n, const rsm_filter_params *params, int32_t *kept_index,
                     float *normals, int64_t *n_kept, double *stats);
/* The same on the cloud of the last rsm_run_pair, without leaving the GPU: the surviving points as 16-byte records
 * (the RCCL payload of rsm_gather_clouds, now without the outliers) and their normals (4 floats each, may be NULL)
 * in caller-owned DEVICE buffers of capacity max_points. */
int rsm_filter_last_cloud(rsm_ctx *ctx, const rsm_filter_params *params, rsm_point16 *d_points, float *d_normals,
                          int64_t max_points, int64_t *n_kept, double *stats);
/* What the last rsm_filter_last_cloud[_host] of this context did: info[0] = the radius (pixels) of the pixel-window k-nearest pass,
 * 0 when it did not run (the cloud of a matched pair is a depth map: the k nearest of most points lie within a small pixel window
 * around their own pixel, proven per point by a bound on the distance to every ray outside it -- csrc/k_filter_win.hip; the radius --
 * 7, 12 or 16 -- comes from a sparse probe), info[1] = queries it left to the generic grid search, info[2] = points in, info[3] =
 * points kept.  Option "filter_window" (rsm_set_option): 1 = probe (default), 0 = no window pass, 7 / 12 / 16 / 20 / 24 = that
 * radius (A/B; the results are the same bits either way). */
int rsm_filter_last_info(rsm_ctx *ctx, int64_t info[4]);
/* ... and its normals: info[0] = the pixel window (radius) their radius search ran over on the cloud's pixel lattice, 0 when it ran on a
 * grid of radius-cells over the filtered cloud instead; info[1] = the widest window any point needed (the search radius in pixel
 * spacings at the nearest point: a property of the rig), -1 when the lattice was not available.  Option "filter_normals_window". */
int rsm_filter_last_normals_info(rsm_ctx *ctx, int64_t info[2]);
/* ... and the k-nearest grid ladder of the last rsm_filter_cloud or rsm_filter_last_cloud[_host]: grid[0] = its first level's search
 * radius (0: no level ran -- the pixel-window passes decided every query), grid[1..3] = that level's grid origin (world x, y, z);
 * info[0..2] = its cells per world axis, info[3] = the levels run, info[4] = the first level's cell table kind t (k_sor_knn<t>; 1: per
 * cell, 2: per row of cells, 0: none; -1: no level ran), info[5] = bit t set when some level searched with kind t.  Option
 * "filter_ladder_h". */
int rsm_filter_last_grid(rsm_ctx *ctx, double grid[4], int64_t info[6]);
/* ... and the passes between the tile pass and the grid ladder of the last rsm_filter_last_cloud[_host] / rsm_stage_filter_depth_map:
 * every pass that took a wave (k_sor_window_wave) or a workgroup (k_sor_window_wg, option "filter_wg_max") per listed query -- the 24-
 * and 40-pixel passes where "filter_list" puts them there, then windows of 80, 160, ... pixels while at most 65536 queries are left.
 * *n_passes = how many ran (at most head[3]); passes (capacity 4 * max_passes) receives, per pass, its window radius in pixels, the
 * queries it was given, the queries it decided, and 1 for the workgroup form / 0 for the wave form.  head[0] = queries handed to the
 * grid ladder (0: it did not run), head[1] = queries handed to the whole-cloud search, head[2] = 1 when that search read the lattice
 * copy as its point array (no ladder level ran), head[3] = the most passes a report holds.  All zero when no window pass ran. */
int rsm_filter_last_passes(rsm_ctx *ctx, int64_t head[4], int64_t *passes, int64_t max_passes, int64_t *n_passes);
/* Stage entry for the tests: DisparityToCloud of a given top-level fp64 disparity map (rsm_stage_cloud's arguments) and the per-pair
 * filter of that cloud exactly as rsm_filter_last_cloud runs it on the cloud of a matched pair -- the same function behind both, so
 * every "filter_*" option and rsm_filter_last_info / _normals_info / _grid / _passes behave the same; no matching runs.  xyz (capacity
 * 3 * max_points floats) receives the UNFILTERED points in cloud order as InsertPoint keeps them (float32), kept_index (capacity
 * max_points) the indices of the survivors, normals (4 * max_points floats, may be NULL) theirs; *n_points / *n_kept their numbers
 * (RSM_E_INVALID when the cloud has more than max_points points); stats as rsm_filter_cloud. */
int rsm_stage_filter_depth_map(rsm_ctx *ctx, const double *disp, const uint8_t *mask_org, const uint8_t *img_own, int W, int H,
                               const double *Q, double scale, const double *R_final, const double *T_final,
                               const rsm_boundary *own, const rsm_filter_params *params, float *xyz, int32_t *kept_index,
                               float *normals, int64_t max_points, int64_t *n_points, int64_t *n_kept, double *stats);
/* The same with HOST output buffers (page-locked ones from rsm_host_alloc arrive at the link's rate): what a pipeline that
 * replaces the first half of CCloudOptimization::filter (CCloudOptimization.cpp:82-121) downloads instead of the raw cloud --
 * the surviving points and their oriented normals (the reference's cloud_normal, :110-121).  h_normals may be NULL. */
int rsm_filter_last_cloud_host(rsm_ctx *ctx, const rsm_filter_params *params, rsm_point16 *h_points, float *h_normals,
                               int64_t max_points, int64_t *n_kept, double *stats);
/* The radius outlier pass of CCloudOptimization::filter, pcl::RadiusOutlierRemoval between cloud_after_1step and cloud_filtered
 * (CCloudOptimization.cpp:90-96; the shipped reference has the block commented out, its Init and its tunings carry the two values).
 * rsm_filter_params cannot grow, so the pass is a setting of the context: it applies to rsm_filter_cloud, rsm_filter_last_cloud[_host]
 * and rsm_stage_filter_depth_map alike until it is changed.  p = NULL switches it off (the default: every entry then returns what it
 * returned without this function).  With S = the survivors of the StatisticalOutlierRemoval in their order and S_f its finite points,
 *   count(p) = #{ q in S_f : (dx dx + dy dy) + dz dz < r2 } in float32,  r2 = (float)(radius * radius);
 * the point itself counts (radiusSearch returns the query), coincident points count once each, a non-finite p has count 0; p stays iff
 * count(p) > min_neighbors (PCL 1.7.2's applyFilterIndices as published; parity unpinned).  min_neighbors = 0 removes exactly the
 * non-finite points.  kept_index, the points and *n_kept are then the survivors of both passes, the normals are computed on that cloud,
 * stats stay the first pass's, rsm_filter_last_info's info[3] is the final count; everything removed is n_kept = 0 and RSM_OK.
 * RSM_E_INVALID (rsm_last_error names the cause): min_neighbors < 0; a radius that is not finite or not positive, whose float32 square
 * is 0 or infinite, or whose float32 value is 0 (the search grid's cell edge). */
typedef struct rsm_outrem_params {
    int min_neighbors;     /* m_outrem_neighbor (CReconstruction.cpp:18: 50) */
    double radius;         /* m_outrem_radius (2) */
} rsm_outrem_params;
int rsm_filter_set_outrem(rsm_ctx *ctx, const rsm_outrem_params *p);
/* What that pass did in the last filter call of this context: info[0] = points in (the first pass's survivors), -1 when the pass was
 * off; info[1] = points removed; info[2] = the pixel window (radius) the count ran over on the cloud's pixel lattice, 0 when it ran on
 * a grid of radius-cells (the lattice serves while the k-nearest pass's copy is still there, "filter_normals_window" allows windows and
 * no point needs a wider one for the larger of this radius and normal_radius; the normals then take the same route); info[3] = the
 * non-finite points among the removed. */
int rsm_filter_last_outrem(rsm_ctx *ctx, int64_t info[4]);
/* Stage entry for the tests: the pass's count alone, on host buffers, over the whole cloud as S, by the grid route's kernel with its
 * early stop made visible: count[i] = min(count(p_i), cap), cap >= 1 (INT32_MAX: the full count).  n = 0 is RSM_OK.  The radius is
 * held to the setter's rules. */
int rsm_stage_radius_count(rsm_ctx *ctx, const float *xyz, int64_t n, double radius, int cap, int32_t *count);

/* ---- moving-least-squares smoothing (CCloudOptimization::run, CCloudOptimization.cpp:348-389) ----------- */
typedef struct rsm_mls_params {
    double search_radius;   /* m_mls_radius (CReconstruction.cpp:18: 2.5); the weight's Gaussian uses radius^2 */
    int polynomial_order;   /* 1 as .cpp:360; 2 = PCL's default; 0 = no polynomial fit (plane projection) */
} rsm_mls_params;
/* pcl::MovingLeastSquares (computeMLSPointNormal, upsampling NONE, normals computed) restated from PCL 1.7.2 (csrc/k_mls.hip):
 * every finite point with at least 3 finite points (itself included) within the radius is projected onto the local plane,
 * moved by the polynomial fit's height and given the fit's normal -- not renormalised, as PCL 1.7.2 leaves it -- then the normal
 * is negated when its float dot product with the point's reference normal is < 0 (.cpp:378-385; a NaN reference never flips).
 * RSM_E_INVALID: radius not finite or not > 0, order outside 0..2, n < 0 or above INT32_MAX, a NULL output pointer.
 * host buffers: xyz n*3, ref_normals n*4 (nx,ny,nz,curvature as rsm_filter_cloud returns them) or NULL = no flip;
 * out_xyz 3*n, out_normals 4*n (nx,ny,nz,curvature), src_index n; *n_out = points emitted, in input order */
int rsm_mls_cloud(rsm_ctx *ctx, const float *xyz, int64_t n, const float *ref_normals, const rsm_mls_params *p,
                  float *out_xyz, float *out_normals, int32_t *src_index, int64_t *n_out);
/* the same on DEVICE buffers of rsm_point16 records -- what rsm_filter_last_cloud leaves for each pair, concatenated,
 * or what rsm_gather_clouds delivers at the root (no normals there: pass NULL) */
int rsm_mls_cloud_device(rsm_ctx *ctx, const rsm_point16 *d_points, int64_t n, const float *d_ref_normals,
                         const rsm_mls_params *p, float *d_out_xyz, float *d_out_normals, int32_t *d_src_index,
                         int64_t *n_out);

/* ---- multi-view duplicate deletion (the isdelete branch of CCloudOptimization::run, CCloudOptimization.cpp:152-346) */
/* One pair of the rig as CCloudOptimization::filter(i) leaves it (.cpp:66-71) after Rectify and MatchAllLayer.  Host pointers. */
typedef struct rsm_dedup_view {
    double P[2][12];          /* cam[i][k].P, 3x4 row-major, k = 0 (left), 1 (right): R[i][k] / T[i][k] are its columns as float */
    float cam_center[3];      /* cam[i][0].CamCenter */
    rsm_boundary bound0;      /* cam[i][0].bound (MatchAllLayer's top-level margin); width or height <= 0: the pair owns no buckets */
    int width, height;        /* the rectified top level of both views */
    const uint8_t *image[2];  /* cam[i][k].image, BGR 8UC3, stride 3 * width */
    const uint8_t *mask[2];   /* cam[i][k].mask, 8UC1, stride width */
} rsm_dedup_view;
/* Every point goes to the left view of the pair its normal faces best, is bucketed by the pixel it projects to, and each bucket
 * whose left-mask pixel is 255 keeps one point per surface layer (the reference's rules, quirks included: DESIGN 9 f6).
 * index (capacity n) receives indicesptr -- indices into the input, in the reference's (pair, row, column) visiting order --
 * and *n_out its length; stats = {s1 (outside the bound), s2 (left mask 0), count0 (right-mask misses), buckets visited}.
 * host buffers: xyz n*3 float, normals4 n*4 float (the filter's normals after their flip: nx, ny, nz, curvature).
 * RSM_E_INVALID: a NULL output, n < 0 or above INT32_MAX, n > 0 with n_pairs < 1, a NULL image or mask, a bound whose width /
 * height disagree with XL..XR / YL..YR, a bound outside its image or closer than 2 px to its edge (the 5x5 windows). */
int rsm_dedup_cloud(rsm_ctx *ctx, const float *xyz, const float *normals4, int64_t n, const rsm_dedup_view *views, int n_pairs,
                    int32_t *index, int64_t *n_out, int64_t stats[4]);
/* the same on DEVICE buffers: n rsm_point16 records and n float4 normals (what rsm_filter_last_cloud leaves per pair, concatenated);
 * d_index (capacity n) as above; d_out_points / d_out_normals (capacity n each, may be NULL) receive the kept records and their
 * normals, in d_index order -- the input of rsm_mls_cloud_device.  The views' images stay host pointers. */
int rsm_dedup_cloud_device(rsm_ctx *ctx, const rsm_point16 *d_points, const float *d_normals4, int64_t n, const rsm_dedup_view *views,
                           int n_pairs, int32_t *d_index, rsm_point16 *d_out_points, float *d_out_normals, int64_t *n_out,
                           int64_t stats[4]);

/* ---- surface from the oriented cloud (where CCloudOptimization::run calls meshlab.bat's "Surface Reconstruction:
 * Poisson" on bigcloud.ply, .cpp:389-, and filter() calls mesh.bat's PoissonRecon --pointWeight 0 + SurfaceTrimmer) ------------------
 * Unscreened Poisson reconstruction (Kazhdan, Bolitho, Hoppe 2006) on a dense grid of 2^depth nodes per axis, marching tetrahedra, trim
 * by the dilated sample occupancy.  Not a bit-parity port of those tools: the method as DESIGN.md 9 (f7) defines it. */
typedef struct rsm_poisson_params {
    int depth;            /* 5..9: N = 2^depth nodes per axis */
    double scale;         /* finite, >= 1: the grid's side over the samples' largest extent (PoissonRecon's --scale, 1.1) */
    double rel_residual;  /* in (0, 1): the solve stops at ||b - L chi|| / ||b|| <= rel_residual ... */
    int max_cycles;       /* ... or after max_cycles >= 1 cycles (-> RSM_W_NOT_CONVERGED) */
    int trim_cells;       /* >= 0: faces survive within this many cells (Chebyshev) of a cell that holds a sample; 0 = no trim */
} rsm_poisson_params;
/* stats: [0] valid samples, [1] samples that took no part (non-finite, zero normal), [2] the relative residual reached, [3] cycles used,
 * [4] iso, [5..7] grid origin, [8] h, [9] N, [10] / [11] vertices / faces before the trim */
#define RSM_POISSON_STATS 12
/* n samples in host buffers (xyz n*3 float, normals4 n*4 float: nx, ny, nz, curvature as rsm_mls_cloud returns them).  The mesh stays
 * with the context until the next call; *n_vertices / *n_faces size the buffers of rsm_poisson_last_mesh.  Returns RSM_OK,
 * RSM_W_NOT_CONVERGED (a valid mesh from the chi reached) or an error.  No valid sample, or all points equal: an empty mesh, RSM_OK.
 * RSM_E_INVALID (rsm_last_error names the parameter): depth outside 5..9, scale not finite or < 1, rel_residual not in (0, 1),
 * max_cycles < 1, trim_cells < 0, n < 0 or above INT32_MAX, a NULL pointer. */
int rsm_poisson_mesh(rsm_ctx *ctx, const float *xyz, const float *normals4, int64_t n, const rsm_poisson_params *p, int64_t *n_vertices,
                     int64_t *n_faces, double *stats);
/* the same on DEVICE buffers, as rsm_mls_cloud_device leaves them (d_out_xyz, d_out_normals) */
int rsm_poisson_mesh_device(rsm_ctx *ctx, const float *d_xyz, const float *d_normals4, int64_t n, const rsm_poisson_params *p,
                            int64_t *n_vertices, int64_t *n_faces, double *stats);
/* copies the last mesh of this context out: xyz 3 * n_vertices float, faces 3 * n_faces int32 (either may be NULL); host / device buffers */
int rsm_poisson_last_mesh(rsm_ctx *ctx, float *xyz, int32_t *faces);
int rsm_poisson_last_mesh_device(rsm_ctx *ctx, float *d_xyz, int32_t *d_faces);
/* stage entry points (host buffers) for the tests.  rhs: samples -> grid = {origin x, y, z, h}, b (N^3 doubles, exact from the fixed-point
 * splat; the solver reads it rounded to float), occ (N^3 bytes), counts = {valid, not valid}; h = 0: nothing to mesh, b and occ are zero.
 * solve: b (N^3 floats) -> chi, the residual reached, cycles used, history (optional, max_cycles doubles: the residual after each cycle).
 * iso_mesh: a caller's chi (N^3 floats), iso, grid and occ (may be NULL with trim_cells = 0) -> the context's last mesh. */
int rsm_stage_poisson_rhs(rsm_ctx *ctx, const float *xyz, const float *normals4, int64_t n, const rsm_poisson_params *p, double grid[4],
                          double *b, uint8_t *occ, int64_t counts[2]);
int rsm_stage_poisson_solve(rsm_ctx *ctx, const float *b, int depth, double rel_residual, int max_cycles, float *chi, double *residual,
                            int *cycles, double *history);
int rsm_stage_iso_mesh(rsm_ctx *ctx, const float *chi, int depth, double iso, const double grid[4], const uint8_t *occ, int trim_cells,
                       int64_t *n_vertices, int64_t *n_faces);
/* ---- the density-adaptive form of the same call (mesh.bat: PoissonRecon --samplesPerNode 2; script1.mlx: SamplesPerNode 3) --------------
 * Opt-in; the plain call above keeps its behaviour and its bits.  Every sample gets the density rho of the cloud around it (the density
 * trim's count splat on 2^kernel_depth nodes per axis, read back at the sample), the depth d = min(depth, max(3, kernel_depth +
 * 1/2 log2(rho / samples_per_node))) at which a grid node would hold samples_per_node samples, and the weight w = min(1, 1 / (64 rho)).  It is
 * splatted with its weight at the two grid levels around d (levels 3..depth) instead of at the finest level with weight 1; the levels are
 * added up coarse to fine by trilinear prolongation with the volume factor 8 per level, and the iso-value is the w-weighted mean of chi at
 * the samples.  Where the cloud is thin the surface no longer caves in.  Solver, extraction and occupancy trim are the plain call's.  Not a
 * bit-parity port of PoissonRecon: the rules as DESIGN.md 9 (f14) defines them. */
typedef struct rsm_poisson_density_params {
    int kernel_depth;         /* 3..depth: the density is estimated on 2^kernel_depth nodes per axis; 0 = depth - 2 (PoissonRecon's default) */
    double samples_per_node;  /* finite, > 0 (mesh.bat: 2, script1.mlx: 3) */
} rsm_poisson_density_params;
/* stats: [0..11] as RSM_POISSON_STATS, [12] the kernel depth used, [13] the least d over the valid samples, [14] the number of samples with
 * d < depth, [15] the sum of w */
#define RSM_POISSON_WEIGHTED_STATS 16
/* as rsm_poisson_mesh[_device]: the mesh becomes the context's last mesh.  RSM_E_INVALID also for kernel_depth neither 0 nor in 3..depth
 * and samples_per_node not finite or <= 0. */
int rsm_poisson_mesh_weighted(rsm_ctx *ctx, const float *xyz, const float *normals4, int64_t n, const rsm_poisson_params *p,
                              const rsm_poisson_density_params *dp, int64_t *n_vertices, int64_t *n_faces, double *stats);
int rsm_poisson_mesh_weighted_device(rsm_ctx *ctx, const float *d_xyz, const float *d_normals4, int64_t n, const rsm_poisson_params *p,
                                     const rsm_poisson_density_params *dp, int64_t *n_vertices, int64_t *n_faces, double *stats);
/* stage entry point (host buffers) for the tests, as rsm_stage_poisson_rhs: b from the levels' sums in fp64.  depth_in (n doubles, may be
 * NULL; RSM_E_INVALID when one is not finite): each sample's d from the caller, clamped to 3..depth, instead of from its density; the
 * values at samples that take no part are not used.  rho, w, d (n doubles each, may be NULL): per sample, 0 where it takes no part. */
int rsm_stage_poisson_rhs_weighted(rsm_ctx *ctx, const float *xyz, const float *normals4, int64_t n, const rsm_poisson_params *p,
                                   const rsm_poisson_density_params *dp, const double *depth_in, double grid[4], double *b, uint8_t *occ,
                                   int64_t counts[2], double *rho, double *w, double *d);
/* ---- one level finer than the dense grid reaches: a finest level on a band of bricks (script1.mlx: OctDepth 10) ---------------------------
 * Opt-in; the calls above keep their behaviour, their bits and their range 5..9.  Here p->depth is the FINEST depth D, 6..10.  The dense
 * solve above runs at D - 1 on the same box; the level of 2^D nodes per axis exists only on the bricks (8^3 nodes each) within band_bricks
 * (Chebyshev) of a brick that holds a sample.  There the splat and right-hand side are the dense call's, the field starts from a quarter of
 * the trilinear prolongation of the coarse field and is corrected by float32 conjugate gradients (one symmetric red-black Gauss-Seidel sweep
 * as preconditioner) down to p->rel_residual; iso-value, marching tetrahedra and the occupancy trim are the dense call's, on the cells whose
 * eight corners lie in the band.  With trim_cells = 0 the mesh has borders where the band ends.  A face the trim keeps needs its cell in the
 * band: trim_cells <= 8 band_bricks - 1 (script1.mlx at depth 10 corresponds to trim_cells 8, which needs band_bricks 2; with 1 the most is
 * 7).  Not a bit-parity port of PoissonRecon's octree: the rules as DESIGN.md 9 (f16) defines them. */
typedef struct rsm_poisson_band_params {
    int band_bricks;     /* 1..4: the box dilation of the occupied bricks */
    int max_iterations;  /* >= 1: of the band solve (-> RSM_W_NOT_CONVERGED) */
} rsm_poisson_band_params;
#define RSM_POISSON_BAND_MAX_BRICKS (1 << 20) /* more active bricks than this: RSM_E_INVALID (such a cloud fills the volume, it is no surface) */
/* stats: [0..11] as RSM_POISSON_STATS with h, N and the origin of the fine grid, [2] / [3] the band solve's residual and iterations;
 * [12] active bricks, [13] occupied bricks, [14] the coarse solve's cycles, [15] its residual, [16] the band residual before the solve */
#define RSM_POISSON_BAND_STATS 17
/* as rsm_poisson_mesh[_device]: the mesh becomes the context's last mesh.  RSM_W_NOT_CONVERGED when either solve ended above rel_residual.
 * RSM_E_INVALID (rsm_last_error names the parameter) also for depth outside 6..10, band_bricks outside 1..4, max_iterations < 1,
 * trim_cells > 8 band_bricks - 1 and more than RSM_POISSON_BAND_MAX_BRICKS active bricks. */
int rsm_poisson_mesh_banded(rsm_ctx *ctx, const float *xyz, const float *normals4, int64_t n, const rsm_poisson_params *p,
                            const rsm_poisson_band_params *bp, int64_t *n_vertices, int64_t *n_faces, double *stats);
int rsm_poisson_mesh_banded_device(rsm_ctx *ctx, const float *d_xyz, const float *d_normals4, int64_t n, const rsm_poisson_params *p,
                                   const rsm_poisson_band_params *bp, int64_t *n_vertices, int64_t *n_faces, double *stats);
/* stage entry points (host buffers) for the tests.  Fields are brick-major: element slot * 512 + lx + 8 (ly + 8 lz), slot = the brick's place in
 * the ascending list `bricks` of linear brick indices bx + B (by + B bz), B = 2^depth / 8.
 * band_rhs: samples -> grid (fine), bricks, b (doubles, exact from the fixed point), occ (per fine cell), g (the guess; from chi_c, (N/2)^3
 * floats, when the caller gives one, else from the dense solve at depth - 1 with p's rel_residual and max_cycles), counts = {valid, not valid,
 * active bricks, occupied bricks}.  brick_room: the bricks the caller's buffers hold (RSM_E_INVALID when the band has more); max_bricks: the
 * cap, 0 = RSM_POISSON_BAND_MAX_BRICKS.  h = 0: nothing to mesh, counts[2] = 0.
 * band_solve: b (floats) and g on n_bricks bricks -> chi, the residual reached, the iterations, the residual before them, history (optional,
 * max_iterations doubles).  chi_c (optional, (N/2)^3 floats): the coarse field, which gives the guess at the band's inactive neighbours; NULL: 0.
 * band_iso_mesh: a caller's chi, iso, grid and occ (may be NULL with trim_cells = 0) on n_bricks bricks -> the context's last mesh. */
int rsm_stage_poisson_band_rhs(rsm_ctx *ctx, const float *xyz, const float *normals4, int64_t n, const rsm_poisson_params *p,
                               const rsm_poisson_band_params *bp, const float *chi_c, int64_t max_bricks, int64_t brick_room, double grid[4],
                               int32_t *bricks, double *b, uint8_t *occ, float *g, int64_t counts[4]);
int rsm_stage_poisson_band_solve(rsm_ctx *ctx, const int32_t *bricks, int64_t n_bricks, int depth, const float *b, const float *g,
                                 const float *chi_c, double rel_residual, int max_iterations, float *chi, double *residual, int *iterations,
                                 double *residual0, double *history);
int rsm_stage_band_iso_mesh(rsm_ctx *ctx, const int32_t *bricks, int64_t n_bricks, int depth, const float *chi, double iso,
                            const double grid[4], const uint8_t *occ, int trim_cells, int64_t *n_vertices, int64_t *n_faces);
/* ---- the banded call with the density-adaptive splat (script1.mlx: OctDepth 10 and SamplesPerNode 3 together) -----------------------------
 * Opt-in; the three calls above keep their behaviour and their bits.  p->depth is the finest depth D, 6..10, and bp is the banded call's.  Every
 * sample's rho, w and d = min(D, max(3, value)) are the density-adaptive call's at depth D, computed once; kernel_depth is 0 (D - 2) or 3..D - 1,
 * since the density grid exists in the coarse problem too.  The coarse problem is the density-adaptive one at D - 1 on the same box with the same
 * w and d clamped to D - 1.  On the fine grid the levels 3..D - 1 of the splat are dense and cascaded to level D - 1; the level D lives on the
 * bricks; the right-hand side on the band is that of the level-D sums plus the trilinear prolongation of the coarser levels, which also
 * stands for the field next to the band.  Guess, band solve, extraction and trim are the banded call's; the iso-value is the w-weighted mean of
 * chi at the samples.  Not a bit-parity port of PoissonRecon: the rules as DESIGN.md 9 (f17) defines them. */
/* stats: [0..16] as RSM_POISSON_BAND_STATS, [17] the kernel depth used, [18] the least d over the valid samples, [19] the number of samples
 * with d < D, [20] the sum of w */
#define RSM_POISSON_BAND_WEIGHTED_STATS 21
/* as rsm_poisson_mesh_banded[_device].  RSM_E_INVALID (rsm_last_error names the parameter) for everything that call refuses, for dp = NULL,
 * kernel_depth neither 0 nor in 3..D - 1 and samples_per_node not finite or <= 0. */
int rsm_poisson_mesh_banded_weighted(rsm_ctx *ctx, const float *xyz, const float *normals4, int64_t n, const rsm_poisson_params *p,
                                     const rsm_poisson_band_params *bp, const rsm_poisson_density_params *dp, int64_t *n_vertices, int64_t *n_faces,
                                     double *stats);
int rsm_poisson_mesh_banded_weighted_device(rsm_ctx *ctx, const float *d_xyz, const float *d_normals4, int64_t n, const rsm_poisson_params *p,
                                            const rsm_poisson_band_params *bp, const rsm_poisson_density_params *dp, int64_t *n_vertices,
                                            int64_t *n_faces, double *stats);
/* stage entry point (host buffers) for the tests: rsm_stage_poisson_band_rhs with this splat.  depth_in (n doubles, may be NULL; RSM_E_INVALID
 * when one is not finite): each sample's d from the caller, clamped to 3..D.  The coarse field, when chi_c is NULL, is that of the coarse
 * problem above.  rho, w, d (n doubles each, may be NULL): per sample, 0 where it takes no part. */
int rsm_stage_poisson_band_rhs_weighted(rsm_ctx *ctx, const float *xyz, const float *normals4, int64_t n, const rsm_poisson_params *p,
                                        const rsm_poisson_band_params *bp, const rsm_poisson_density_params *dp, const double *depth_in,
                                        const float *chi_c, int64_t max_bricks, int64_t brick_room, double grid[4], int32_t *bricks, double *b,
                                        uint8_t *occ, float *g, int64_t counts[4], double *rho, double *w, double *d);
/* binary little-endian PLY mesh: vertex float x, y, z; face list uchar int vertex_indices (what MeshLab and TextureStitcher read).  Host only. */
int rsm_write_ply_mesh(const char *path, const float *xyz, int64_t n_vertices, const int32_t *faces, int64_t n_faces);

/* ---- smoothing and clean-up of the surface (where meshlab.bat goes on after the Poisson filter: script1.mlx's "Laplacian Smooth", then
 * script2.mlx's "Remove Isolated pieces (wrt Diameter)", "Remove Duplicate Faces", "Remove Zero Area Faces", "Remove Faces from Non
 * Manifold Edges" -> bigmesh.ply) ------------------------------------------------------------------------------------------------------
 * Not a bit-parity port of MeshLab / VCG: the rules as DESIGN.md 9 (f8) defines them.  script2.mlx's last filter, "Close Holes", is
 * rsm_mesh_close_holes below. */
#define RSM_MESH_CLEAN_DUPLICATES 1u  /* flags: of the faces with the same three vertices the lowest index stays */
#define RSM_MESH_CLEAN_ZERO_AREA 2u   /*        faces with a repeated index or without area go */
#define RSM_MESH_CLEAN_NONMANIFOLD 4u /*        every face on an edge that more than two surviving faces share goes */
typedef struct rsm_mesh_clean_params {
    int smooth_steps;        /* >= 0: simultaneous Laplacian steps (script1: 5); 0 = no smoothing */
    int cotangent;           /* 0 / 1: weights 1 / cotangents clamped at 0 (script1: 1) */
    int boundary;            /* 1: border vertices move along the border (script1's 1D boundary smoothing); 0: they stay */
    double min_piece;        /* finite, >= 0: components with a bounding-box diameter below the threshold go; 0 removes nothing */
    int min_piece_relative;  /* 1: threshold = min_piece * (diameter of the box of all vertices); 0: threshold = min_piece (script2: 42.1253) */
    unsigned int flags;      /* RSM_MESH_CLEAN_* */
} rsm_mesh_clean_params;
/* stats: [0] / [1] vertices / faces in, [2] / [3] out, [4] border vertices (endpoints of an edge of one face) of the input, [5] components,
 * [6] components removed, [7..10] faces removed as isolated pieces / duplicates / zero area / on non-manifold edges, [11] vertices dropped,
 * [12] D = the diameter of the box of all (smoothed) vertices, [13] the threshold */
#define RSM_MESH_CLEAN_STATS 14
/* nv vertices (xyz nv*3 float) and nf faces (faces nf*3 int32) in host buffers -> the context's last mesh (rsm_poisson_last_mesh copies it
 * out; *n_vertices / *n_faces size its buffers).  An empty mesh in, or nothing left: an empty mesh, RSM_OK.  RSM_E_INVALID (rsm_last_error
 * names the cause): a face index outside [0, nv), a coordinate that is not finite, 3 nf >= 2^31, nv above INT32_MAX, a negative count,
 * smooth_steps < 0, cotangent / boundary / min_piece_relative not 0 or 1, min_piece negative or not finite, an unknown flag, a NULL pointer. */
int rsm_mesh_clean(rsm_ctx *ctx, const float *xyz, int64_t nv, const int32_t *faces, int64_t nf, const rsm_mesh_clean_params *p, int64_t *n_vertices,
                   int64_t *n_faces, double *stats);
/* the same on DEVICE buffers */
int rsm_mesh_clean_device(rsm_ctx *ctx, const float *d_xyz, int64_t nv, const int32_t *d_faces, int64_t nf, const rsm_mesh_clean_params *p,
                          int64_t *n_vertices, int64_t *n_faces, double *stats);
/* the same on the context's last mesh where it lies (what rsm_poisson_mesh left): no host round trip; the result replaces it */
int rsm_mesh_clean_last(rsm_ctx *ctx, const rsm_mesh_clean_params *p, int64_t *n_vertices, int64_t *n_faces, double *stats);
/* stage entry points (host buffers) for the tests.  smooth: the positions after `steps` steps (out_xyz nv*3 float; connectivity is untouched),
 * *n_border (may be NULL) = border vertices.  components: labels[f] = the lowest face index of f's component (faces are connected across a
 * shared edge, not across a shared vertex), -1 for a face with a repeated index; *n_components = the components found. */
int rsm_stage_mesh_smooth(rsm_ctx *ctx, const float *xyz, int64_t nv, const int32_t *faces, int64_t nf, int steps, int cotangent, int boundary,
                          float *out_xyz, int64_t *n_border);
int rsm_stage_mesh_components(rsm_ctx *ctx, const int32_t *faces, int64_t nv, int64_t nf, int32_t *labels, int64_t *n_components);

/* ---- the closing of the surface's small holes (script2.mlx's last filter, "Close Holes" with MaxHoleSize 30) ---------------------------
 * Not a bit-parity port of MeshLab / VCG: the rules as DESIGN.md 9 (f12) defines them.  The script runs the filter on a selection that its
 * earlier filters leave empty; here EVERY border loop is a candidate.  With the edge table of the clean-up, an entry 3 f + j whose edge no
 * other face has is a border entry, directed as its face; a vertex is simple when one border entry reaches it and one leaves it; border
 * entries are linked through simple vertices, and a component all of whose vertices are simple is a loop (everything else -- bow-ties,
 * faces oriented against each other, chains that end -- is open and is never closed).  A loop of at most max_hole_size edges that is not
 * the border of a lone triangle gets the least-area triangulation of its ring (Barequet-Sharir; no refinement, no fairing) that uses no
 * diagonal the mesh already has as an edge and no triangle without area; a loop without such a triangulation stays whole.  The vertices and
 * the input's faces are untouched and in place; the new faces follow them, hole by hole in the order of the holes' lowest entry, oriented
 * like their neighbours.  Opt-in: no other call changes. */
#define RSM_MESH_CLOSE_MAX_HOLE 64
typedef struct rsm_mesh_close_params {
    int max_hole_size;       /* 3..RSM_MESH_CLOSE_MAX_HOLE: loops of more edges stay open (script2: 30) */
} rsm_mesh_close_params;
/* stats: [0] / [1] vertices / faces in, [2] faces out, [3] border entries, [4] border components, [5] loops, [6] open components, [7] loops
 * closed, [8] loops skipped as too long, [9] lone triangles, [10] loops without an admissible triangulation, [11] faces added, [12] / [13]
 * the longest loop closed / seen */
#define RSM_MESH_CLOSE_STATS 14
/* nv vertices (xyz nv*3 float) and nf faces (faces nf*3 int32) in host buffers -> the context's last mesh, as rsm_mesh_clean
 * (rsm_poisson_last_mesh copies it out; *n_vertices = nv, *n_faces size its buffers; colours of the last mesh are dropped).  An empty mesh
 * in: an empty mesh, RSM_OK.  RSM_E_INVALID (rsm_last_error names the cause): max_hole_size outside 3..64, a face index outside [0, nv), a
 * coordinate that is not finite, 3 nf >= 2^31, nv above INT32_MAX, a negative count, a NULL pointer. */
int rsm_mesh_close_holes(rsm_ctx *ctx, const float *xyz, int64_t nv, const int32_t *faces, int64_t nf, const rsm_mesh_close_params *p, int64_t *n_vertices,
                         int64_t *n_faces, double *stats);
/* the same on DEVICE buffers */
int rsm_mesh_close_holes_device(rsm_ctx *ctx, const float *d_xyz, int64_t nv, const int32_t *d_faces, int64_t nf, const rsm_mesh_close_params *p,
                                int64_t *n_vertices, int64_t *n_faces, double *stats);
/* the same on the context's last mesh where it lies (what rsm_poisson_mesh / rsm_mesh_trim / rsm_mesh_clean left); the result replaces it */
int rsm_mesh_close_holes_last(rsm_ctx *ctx, const rsm_mesh_close_params *p, int64_t *n_vertices, int64_t *n_faces, double *stats);
/* stage entry points (host buffers) for the tests.  border_loops: per entry 3 f + j (3 nf int32 each) labels = the lowest entry of its border
 * component (-1: no border entry) and sizes = L for a loop's entries, 0 for an open component's, -1 otherwise; *n_components = the border
 * components.  hole_triangulate: a ring of L (3..64) finite points (ring_xyz L*3 float) and forbidden (L*L bytes or NULL: pair (i, j),
 * i + 2 <= j, (i, j) != (0, L-1), is forbidden when byte i*L + j is not 0) -> *weight = W(0, L-1), triangles ((L-2)*3 int32 of ring
 * positions, in the order of the output) and *n_triangles = L - 2; +inf and 0 when the ring has no admissible triangulation. */
int rsm_stage_mesh_border_loops(rsm_ctx *ctx, const int32_t *faces, int64_t nv, int64_t nf, int32_t *labels, int32_t *sizes, int64_t *n_components);
int rsm_stage_hole_triangulate(rsm_ctx *ctx, const float *ring_xyz, int L, const uint8_t *forbidden, double *weight, int32_t *triangles, int *n_triangles);

/* ---- the decimation of the final mesh (Demo/meshlab/decimation.mlx: "Quadric Edge Collapse Decimation", TargetFaceNum 100000, QualityThr
 * 0.3, PreserveTopology and OptimalPlacement on, AutoClean on) ---------------------------------------------------------------------------
 * Not a bit-parity port of MeshLab / VCG: the rules as DESIGN.md 9 (f13) defines them.  Faces with a repeated index go first.  Every vertex
 * gets the sum of its faces' plane quadrics (not normalised: a face weighs by 4 area^2) and of the border planes of its border edges, once;
 * a collapse adds the two quadrics.  Rounds: every unique edge of one or two faces without a locked endpoint (an endpoint of an edge of more
 * than two faces; with preserve_boundary every border vertex) that passes the link condition (preserve_topology) and leaves no two faces with
 * the same vertices is a candidate; its position is the quadric's optimum (3 x 3 solve by cofactors, refused when singular, not finite or
 * further than two edge lengths from the midpoint) or the best of Pa, Pb and the midpoint, rounded to float32 and judged as that; its cost is
 * max(error, min_error) over the clamped least shape quality of the faces around it.  The candidates of the lowest ceil(need / 2) ranks in
 * (cost, key) take part; an edge is selected when its rank is the least among the participating edges at its endpoints and their
 * neighbours (no two selected edges have adjacent endpoints); in rank order the selected edges are kept while the faces removed before them
 * are fewer than need = faces - target; b -> a (the lower index), V[a] = the position, Q[a] += Q[b]; faces with a repeated index leave in
 * order.  Rounds run until faces <= target, no candidate is left or max_rounds; the result has target or target - 1 faces while candidates
 * last.  At the end the vertices no face refers to go (the input's as well).  Opt-in: no other call changes. */
typedef struct rsm_mesh_decimate_params {
    int64_t target_faces;    /* >= 0 (decimation.mlx: 100000) */
    double target_fraction;  /* 0 = unused, else in (0, 1]: target = floor(fraction * faces in), and target_faces is not read (TargetPerc) */
    double quality_thr;      /* [0, 1]; 0 = no shape penalty (0.3) */
    int preserve_boundary;   /* 0 / 1: border vertices are locked (0) */
    double boundary_weight;  /* finite, > 0: the weight of a border edge's plane (1) */
    int preserve_normal;     /* 0 / 1: a collapse that turns a face's normal by 90 degrees or more is refused (0) */
    int preserve_topology;   /* 0 / 1: the link condition (1) */
    int optimal_placement;   /* 0 / 1: the quadric's optimum, else the best of the endpoints and the midpoint (1) */
    double min_error;        /* finite, >= 0: the floor of an edge's error (the binding's default: 1e-15) */
    int max_rounds;          /* 1..1000000 (the binding's default: 1000) */
} rsm_mesh_decimate_params;
/* stats: [0] / [1] vertices / faces in, [2] / [3] vertices / faces out, [4] faces with a repeated index dropped, [5] rounds, [6] collapses, [7]
 * collapses of border edges, [8..14] the edges of the last round that were no candidates: [8] of more than two faces, [9] a locked endpoint,
 * [10] the link condition's common neighbours, [11] both endpoints on the border but the edge not, [12] two faces with the same vertices, [13]
 * a normal turned over, [14] an error or cost that is not finite; [15] the locked vertices of the last round, [16] the largest number of
 * faces at a vertex met, [17] the largest cost collapsed, [18] target_reached (faces out <= target), [19] the target */
#define RSM_MESH_DECIMATE_STATS 20
/* nv vertices (xyz nv*3 float) and nf faces (faces nf*3 int32) in host buffers -> the context's last mesh, as rsm_mesh_clean
 * (rsm_poisson_last_mesh copies it out; *n_vertices, *n_faces size its buffers; colours of the last mesh are dropped).  An empty mesh in: an
 * empty mesh, RSM_OK.  A mesh at or below the target: only the repeated-index faces and the unreferenced vertices go.  RSM_E_INVALID
 * (rsm_last_error names the cause): a parameter outside its range above, a face index outside [0, nv), a coordinate that is not finite,
 * 3 nf >= 2^31, nv above INT32_MAX, a negative count, a NULL pointer. */
int rsm_mesh_decimate(rsm_ctx *ctx, const float *xyz, int64_t nv, const int32_t *faces, int64_t nf, const rsm_mesh_decimate_params *p, int64_t *n_vertices,
                      int64_t *n_faces, double *stats);
/* the same on DEVICE buffers */
int rsm_mesh_decimate_device(rsm_ctx *ctx, const float *d_xyz, int64_t nv, const int32_t *d_faces, int64_t nf, const rsm_mesh_decimate_params *p,
                             int64_t *n_vertices, int64_t *n_faces, double *stats);
/* the same on the context's last mesh where it lies; the result replaces it */
int rsm_mesh_decimate_last(rsm_ctx *ctx, const rsm_mesh_decimate_params *p, int64_t *n_vertices, int64_t *n_faces, double *stats);
/* stage entry points (host buffers) for the tests.  A quadric is 10 doubles: xx xy xz xd yy yz yd zz zd dd.  quadrics: out_q nv*10.
 * collapse_costs: per unique edge of the faces without a repeated index, in key order (room for 3 nf each): key = (a << 32) | b with a < b,
 * multiplicity, cost (+inf: not a candidate), reject (bits 0-3: 0 a candidate, else 1..7 in the order of stats [8..14]; bits 4-5 where a
 * position was computed -- codes 0, 6, 7 --: 0 the optimum, 1 Pa, 2 Pb, 3 the midpoint) and position (3 float); *n_edges of them.
 * collapse_round: one round with need = faces to remove on (xyz, faces, quadrics nv*10) -> out_xyz (nv*3), out_quadrics (nv*10), out_faces
 * (room for nf*3; *n_faces_out of them), selected_keys (room for 3 nf; *n_selected of them in priority order, the first *n_kept collapsed). */
int rsm_stage_mesh_quadrics(rsm_ctx *ctx, const float *xyz, int64_t nv, const int32_t *faces, int64_t nf, double boundary_weight, double *out_q);
int rsm_stage_mesh_collapse_costs(rsm_ctx *ctx, const float *xyz, int64_t nv, const int32_t *faces, int64_t nf, const double *quadrics,
                                  const rsm_mesh_decimate_params *p, uint64_t *keys, int32_t *multiplicity, double *cost, int32_t *reject, float *position,
                                  int64_t *n_edges);
int rsm_stage_mesh_collapse_round(rsm_ctx *ctx, const float *xyz, int64_t nv, const int32_t *faces, int64_t nf, const double *quadrics,
                                  const rsm_mesh_decimate_params *p, int64_t need, float *out_xyz, int32_t *out_faces, double *out_quadrics, int64_t *n_faces_out,
                                  uint64_t *selected_keys, int64_t *n_selected, int64_t *n_kept);

/* ---- the subdivision of the final mesh (Demo/meshlab/subdiv.mlx: "Subdivision Surfaces: Loop", Iterations 3, Threshold 1 % of the box
 * diagonal, whole mesh) ----------------------------------------------------------------------------------------------------------------------
 * Not a bit-parity port of MeshLab / VCG: the rules as DESIGN.md 9 (f15) defines them.  Per iteration every unique edge strictly longer than
 * thr is split by a new vertex (index nv + its rank in key order); the old vertices at a split edge move by Loop's rules (interior: the
 * beta_k ring average; border: 1/8, 3/4, 1/8 along the border; locked -- at an edge of three or more faces, with border edges but not
 * exactly two, or in no face -- stay); every face is replaced in place by 1 to 4 faces, orientation kept.  An iteration that splits
 * nothing ends the call.  LIMITS: only Loop's own weights (MeshLab's LoopWeight 0) are built -- LoopWeight 1 / 2 ("Enhance regularity" /
 * "Enhance continuity"; subdiv.mlx selects 2) rest on VCG's weight tables, which the reference tree does not hold, and any weight_scheme
 * but 0 is refused; vertex positions only: colours of the last mesh are dropped, not carried across.  Opt-in: no other call changes. */
typedef struct rsm_mesh_subdivide_params {
    int iterations;            /* 1..8 (subdiv.mlx: 3) */
    double threshold;          /* finite, >= 0: an edge splits when it is strictly longer; 0 splits every edge */
    double threshold_fraction; /* 0 = unused, else in (0, 1]: thr = fraction * the input's box diagonal, and threshold is not read (subdiv.mlx: 0.01) */
    int weight_scheme;         /* 0 (Loop's weights); 1 and 2 are not built and are refused */
} rsm_mesh_subdivide_params;
/* stats: [0] / [1] vertices / faces in, [2] / [3] vertices / faces out, [4] iterations run (those that split an edge), [5] thr, [6] edges
 * split, [7] of them border edges (one face), [8] of them edges of three or more faces, [9..12] faces with 0 / 1 / 2 / 3 split edges (those
 * with a repeated index under 0), [13] / [14] interior / border vertices moved -- [6..14] summed over the iterations run --, [15] the locked
 * vertices of the last mesh looked at, [16] the largest number of faces at a vertex met */
#define RSM_MESH_SUBDIVIDE_STATS 17
/* nv vertices (xyz nv*3 float) and nf faces (faces nf*3 int32) in host buffers -> the context's last mesh, as rsm_mesh_decimate
 * (rsm_poisson_last_mesh copies it out; *n_vertices, *n_faces size its buffers; colours of the last mesh are dropped).  An empty mesh, or
 * one without an edge longer than thr: the mesh as it came, [4] = 0, RSM_OK.  RSM_E_INVALID (rsm_last_error names the cause): a parameter
 * outside its range above, weight_scheme not 0, a face index outside [0, nv), a coordinate that is not finite, 3 nf >= 2^31, nv above
 * INT32_MAX, a negative count, a NULL pointer, an iteration whose result would pass those limits (named).  Every failed call leaves the last
 * mesh and its colours as they were. */
int rsm_mesh_subdivide(rsm_ctx *ctx, const float *xyz, int64_t nv, const int32_t *faces, int64_t nf, const rsm_mesh_subdivide_params *p, int64_t *n_vertices,
                       int64_t *n_faces, double *stats);
/* the same on DEVICE buffers */
int rsm_mesh_subdivide_device(rsm_ctx *ctx, const float *d_xyz, int64_t nv, const int32_t *d_faces, int64_t nf, const rsm_mesh_subdivide_params *p,
                              int64_t *n_vertices, int64_t *n_faces, double *stats);
/* the same on the context's last mesh where it lies; the result replaces it */
int rsm_mesh_subdivide_last(rsm_ctx *ctx, const rsm_mesh_subdivide_params *p, int64_t *n_vertices, int64_t *n_faces, double *stats);
/* stage entry point (host buffers) for the tests: the decisions of one iteration.  Per unique edge of the faces without a repeated index,
 * in key order (room for 3 nf each; *n_edges of them): key = (a << 32) | b with a < b, multiplicity, split (0 / 1), odd_position (3 floats;
 * zeros where the edge does not split); per vertex: vertex_class (0 interior, 1 border, 2 locked) and even_position (nv*3).  *thr (may be
 * NULL): the threshold used. */
int rsm_stage_mesh_subdivide_edges(rsm_ctx *ctx, const float *xyz, int64_t nv, const int32_t *faces, int64_t nf, const rsm_mesh_subdivide_params *p, uint64_t *keys,
                                   int32_t *multiplicity, int32_t *split, float *odd_position, int64_t *n_edges, int32_t *vertex_class, float *even_position,
                                   double *thr);

/* ---- the density trim of the surface (where mesh.bat runs PoissonRecon --density --samplesPerNode 2 and then SurfaceTrimmer --smooth 100
 * --trim 7 --aRatio 0.01) -------------------------------------------------------------------------------------------------------------
 * Not a bit-parity port of those tools: the rules as DESIGN.md 9 (f11) defines them.  Every vertex gets the depth at which a grid node
 * would hold samples_per_node of the samples around it (from a trilinear count splat on 2^kernel_depth nodes per axis of the Poisson call's
 * box), the values are smoothed over the mesh, the surface is cut along the iso-line value = trim (crossing triangles are split), and
 * pieces on either side of the cut smaller than island_ratio of the whole area change side.  Opt-in: rsm_poisson_mesh's trim_cells is the
 * occupancy trim and stays what it is; run the Poisson call with trim_cells = 0 before this one. */
typedef struct rsm_mesh_trim_params {
    int depth;               /* 5..9, the Poisson call's depth */
    double scale;            /* finite, >= 1, the Poisson call's scale: the same box */
    int kernel_depth;        /* 3..depth: the density is estimated on 2^kernel_depth nodes per axis; 0 = depth - 2 (PoissonRecon's default) */
    double samples_per_node; /* finite, > 0 (mesh.bat: 2) */
    int smooth_steps;        /* >= 0 (mesh.bat: 100) */
    double trim;             /* finite (mesh.bat: 7): vertices with value >= trim are kept */
    double island_ratio;     /* finite, in [0, 1) (mesh.bat: 0.01); 0 = no island rule */
} rsm_mesh_trim_params;
/* stats: [0] / [1] vertices / faces in, [2] / [3] out, [4] / [5] valid / invalid samples, [6] cut edges, [7] faces split, [8] faces with a
 * repeated index dropped, [9] zero-area triangles the splits emitted, [10] / [11] components on the kept / dropped side, [12] / [13]
 * components moved kept -> dropped / dropped -> kept, [14] Q_total (the area of both sides in units of D^2 2^-32), [15] / [16] the least /
 * largest value after smoothing (0 for an empty mesh), [17] D^2 (the squared diagonal of the box of the input vertices), [18] the density
 * grid's step (0: no valid sample or all of them equal -- every value is 0), [19] the kernel depth used */
#define RSM_MESH_TRIM_STATS 20
/* host buffers: xyz nv*3 float, faces nf*3 int32, n samples (samples_xyz n*3 float, samples_normals4 n*4 float or NULL: without normals a
 * finite point is a valid sample, with them the Poisson call's rule holds) -> the context's last mesh, as rsm_mesh_clean (rsm_poisson_last_mesh
 * copies it out; colours of the last mesh are dropped).  An empty mesh in, or nothing kept: an empty mesh, RSM_OK.  RSM_E_INVALID
 * (rsm_last_error names the cause): every range stated in the struct, a face index outside [0, nv), a coordinate that is not finite,
 * 3 nf >= 2^31, nv above INT32_MAX, n above INT32_MAX, a negative count, a NULL pointer. */
int rsm_mesh_trim(rsm_ctx *ctx, const float *xyz, int64_t nv, const int32_t *faces, int64_t nf, const float *samples_xyz, const float *samples_normals4,
                  int64_t n, const rsm_mesh_trim_params *p, int64_t *n_vertices, int64_t *n_faces, double *stats);
/* the same with every buffer on the DEVICE */
int rsm_mesh_trim_device(rsm_ctx *ctx, const float *d_xyz, int64_t nv, const int32_t *d_faces, int64_t nf, const float *d_samples_xyz,
                         const float *d_samples_normals4, int64_t n, const rsm_mesh_trim_params *p, int64_t *n_vertices, int64_t *n_faces, double *stats);
/* the same on the context's last mesh where it lies (what rsm_poisson_mesh left); the samples are host buffers; the result replaces it */
int rsm_mesh_trim_last(rsm_ctx *ctx, const float *samples_xyz, const float *samples_normals4, int64_t n, const rsm_mesh_trim_params *p, int64_t *n_vertices,
                       int64_t *n_faces, double *stats);
/* stage entry points (host buffers) for the tests.  density: the samples and p's depth, scale, kernel_depth and samples_per_node -> rho and
 * value at nv points (nv doubles each), counts = {valid, not valid}.  value_smooth: a caller's nv finite values -> the values after `steps`
 * steps.  split: a caller's nv finite values, trim and island_ratio -> the context's last mesh and stats (may be NULL; [4], [5], [18], [19]
 * stay 0); src_face / side / label (each 3 nf int32, may be NULL): per output face its source face, its side before the island rule
 * (1 = kept) and its component (the lowest triangle of the split mesh it is connected to on its side). */
int rsm_stage_mesh_density(rsm_ctx *ctx, const float *samples_xyz, const float *samples_normals4, int64_t n, const rsm_mesh_trim_params *p, const float *xyz,
                           int64_t nv, double *rho, double *value, int64_t counts[2]);
int rsm_stage_mesh_value_smooth(rsm_ctx *ctx, const int32_t *faces, int64_t nv, int64_t nf, const double *values, int steps, double *out_values);
int rsm_stage_mesh_split(rsm_ctx *ctx, const float *xyz, int64_t nv, const int32_t *faces, int64_t nf, const double *values, double trim, double island_ratio,
                         int64_t *n_vertices, int64_t *n_faces, double *stats, int32_t *src_face, int32_t *side, int32_t *label);

/* ---- colours of the final mesh from the rig's views (where CCloudOptimization::run hands tmp\bigmesh.ply and scans.txt to TextureStitcher,
 * .cpp:394-397; the scans are the per-view meshes filter() colours through texture_color, .cpp:127-143, :400-421) ------------------------
 * Not a bit-parity port of TextureStitcher (no source in the reference tree): the rules as DESIGN.md 9 (f9) defines them.  Its seam
 * levelling is rsm_mesh_stitch below.  n_pairs records of rsm_dedup_view give V = 2 n_pairs views, numbered in scans.txt's
 * order: every pair's view 0, then every pair's view 1 (v = k * n_pairs + i).  bound0 and cam_center are ignored -- the centre is
 * -M^-1 p4 of P in fp64 -- and a mask may be NULL: all 255.
 * A vertex is visible in a view when it lies in front of it (q2 > 0), its texture_color pixel is inside the image with mask 255, its
 * normal (the sum of its faces' normals, fp64) makes cos > min_cos with the direction to the view's centre, and the view's depth buffer of
 * the mesh holds nothing at that pixel or a depth within depth_eps behind which the vertex does not lie.
 * Option "meshcolor_big_box" (rsm_set_option, 1 .. 2^20, default 4096): a (face, view) item whose bounding box holds more pixels is
 * rasterised by a workgroup instead of one thread -- the same result either way. */
typedef struct rsm_mesh_color_params {
    int mode;          /* 0: the colour of the visible view of largest cos (ties: the lowest view); 1: the cos-weighted blend of the visible views */
    double min_cos;    /* in [-1, 1): views at a cos not above it do not see the vertex (0.2) */
    double depth_eps;  /* finite, >= 0, a length in scene units: the slack of the depth test (CloudOptimization: twice the Poisson grid step) */
} rsm_mesh_color_params;
/* stats: [0] vertices, [1] vertices coloured (at least one visible view), [2] vertices without a normal, [3] the sum of visible views over
 * the vertices, [4] (face, view) items drawn, [5] of them in the big-box tier */
#define RSM_MESH_COLOR_STATS 6
/* host buffers: xyz nv*3 float, faces nf*3 int32 -> rgb nv*3 bytes (red, green, blue; (127, 127, 127) where no view sees the vertex),
 * best_view nv int32 (-1 there; may be NULL).  An empty mesh: nothing written, RSM_OK.  RSM_E_INVALID (rsm_last_error names the cause): a
 * NULL pointer, n_pairs < 1 with nv > 0, mode outside 0..1, min_cos outside [-1, 1), depth_eps negative or not finite, a face index outside
 * [0, nv), a coordinate that is not finite, width / height < 1, a singular P, 3 nf >= 2^31, nv above INT32_MAX, a negative count. */
int rsm_mesh_color(rsm_ctx *ctx, const float *xyz, int64_t nv, const int32_t *faces, int64_t nf, const rsm_dedup_view *views, int n_pairs,
                   const rsm_mesh_color_params *p, uint8_t *rgb, int32_t *best_view, double *stats);
/* the same on DEVICE buffers (xyz, faces, rgb, best_view); the views' images stay host pointers, as in rsm_dedup_cloud_device */
int rsm_mesh_color_device(rsm_ctx *ctx, const float *d_xyz, int64_t nv, const int32_t *d_faces, int64_t nf, const rsm_dedup_view *views, int n_pairs,
                          const rsm_mesh_color_params *p, uint8_t *d_rgb, int32_t *d_best_view, double *stats);
/* the same on the context's last mesh where it lies (what rsm_poisson_mesh / rsm_mesh_clean left): the mesh is untouched, the colours stay
 * with the context until the mesh changes; rsm_mesh_last_colors copies them out (rgb 3 * n_vertices bytes, best_view n_vertices int32;
 * either may be NULL; RSM_E_STATE when the last mesh has no colours) */
int rsm_mesh_color_last(rsm_ctx *ctx, const rsm_dedup_view *views, int n_pairs, const rsm_mesh_color_params *p, double *stats);
int rsm_mesh_last_colors(rsm_ctx *ctx, uint8_t *rgb, int32_t *best_view);
/* stage entry points (host buffers) for the tests.  texture_color (.cpp:400-421) over n points: q = R p + T with R, T the float casts of
 * P12's columns, pixel = ROUND of the float quotients, rgb = the BGR image's pixel as red, green, blue, (127, 127, 127) outside the image
 * or where the quotient is not finite; no test of the depth's sign -- also what MyPlyIo::ReadAndWrite does to mesh_trimmer.ply.
 * mesh_depth: one view's depth buffer, width * height uint32: the largest float32 bit pattern of the inverse depth drawn at each pixel. */
int rsm_texture_color(rsm_ctx *ctx, const float *xyz, int64_t n, const double P12[12], const uint8_t *image, int width, int height, uint8_t *rgb);
int rsm_stage_mesh_depth(rsm_ctx *ctx, const float *xyz, int64_t nv, const int32_t *faces, int64_t nf, const double P12[12], int width, int height,
                         uint32_t *wbuf);
/* binary little-endian PLY: vertex float x, y, z, uchar red, green, blue; face list uchar int vertex_indices (MyPlyIo's property order,
 * my_ply_interface.cpp:35-50).  Host only. */
int rsm_write_ply_mesh_color(const char *path, const float *xyz, int64_t n_vertices, const int32_t *faces, int64_t n_faces, const uint8_t *rgb);

/* ---- the views' exposure seams levelled in the mesh's colours (the other half of TextureStitcher's job) ----------------
 * Starts from the best-view colouring c of rsm_mesh_color (mode 0; the colour params' mode must be 0) and solves, per channel and over the
 * coloured vertices, the screened gradient-domain system  sum_j (x_i - x_j) + lambda x_i = sum_j g_ij + lambda c_i  over each vertex's
 * incidences (its corner list: an interior edge counts twice, a border edge once; only coloured neighbours).  g_ij = c_i - c_j where both
 * ends take the same view; across a seam (views a = best_i, b = best_j) it is 0 with seam_gradient = 0, else the mean of the views' own
 * differences that exist: c_i - col_a(j) if view a sees j, col_b(i) - c_j if view b sees i (col_v = texture_color's pixel in view v, "sees"
 * = the colouring's visibility test).  Solver: Jacobi-preconditioned Chebyshev iteration with a fixed number of steps -- `iterations`, or with
 * iterations = 0 the least k with T_k(sigma) >= 1 / reduction (T_k the Chebyshev polynomial by its recurrence, sigma = (2 + lmin) / (2 - lmin),
 * lmin = lambda / (dmax + lambda), dmax the largest incidence count), after which the error in the M-norm is at most `reduction` times the
 * start's.  Bytes = clamp(floor(x + 0.5), 0, 255); uncoloured vertices stay (127, 127, 127).  A mesh without a seam comes back bit for bit.
 * The visibility masks are 64 bits: V = 2 n_pairs <= 64. */
typedef struct rsm_mesh_stitch_params {
    double lambda;      /* finite, > 0: the pull towards the colouring; a view's offset decays over about 1 / sqrt(lambda) edges (0.01) */
    int iterations;     /* 0 .. 1000000; 0 = from reduction */
    double reduction;   /* in (0, 1), used when iterations = 0 (1e-4) */
    int seam_gradient;  /* 0 / 1 (1) */
} rsm_mesh_stitch_params;
#define RSM_MESH_STITCH_MAX_ITERATIONS 1000000
/* stats: [0] vertices, [1] vertices coloured, [2] incidences between coloured vertices, [3] of them across a seam, [4] seam incidences with
 * two terms, [5] with one, [6] with none, [7] dmax, [8] steps run, [9] the relative residual ||b - A x|| / ||b - A c|| after them (reported,
 * not a stopping test; 0 when the start solves the system), [10] the largest |x - c|, [11] values clamped */
#define RSM_MESH_STITCH_STATS 12
/* The arguments of rsm_mesh_color[_device / _last] with the stitch params and stats after the colour params.  An empty mesh or no coloured
 * vertex: the colouring's bytes, RSM_OK.  RSM_E_INVALID (rsm_last_error names the cause): everything rsm_mesh_color refuses, mode != 0,
 * V = 2 n_pairs > 64, lambda not finite or not > 0, iterations outside 0 .. 1000000, reduction outside (0, 1) when it is used (or one
 * that needs more than 1000000 steps), seam_gradient not 0 or 1.  The _last form leaves the colours with the context as
 * rsm_mesh_color_last does: rsm_mesh_last_colors copies them out. */
int rsm_mesh_stitch(rsm_ctx *ctx, const float *xyz, int64_t nv, const int32_t *faces, int64_t nf, const rsm_dedup_view *views, int n_pairs,
                    const rsm_mesh_color_params *p, const rsm_mesh_stitch_params *sp, uint8_t *rgb, int32_t *best_view, double *stats);
int rsm_mesh_stitch_device(rsm_ctx *ctx, const float *d_xyz, int64_t nv, const int32_t *d_faces, int64_t nf, const rsm_dedup_view *views, int n_pairs,
                           const rsm_mesh_color_params *p, const rsm_mesh_stitch_params *sp, uint8_t *d_rgb, int32_t *d_best_view, double *stats);
int rsm_mesh_stitch_last(rsm_ctx *ctx, const rsm_dedup_view *views, int n_pairs, const rsm_mesh_color_params *p, const rsm_mesh_stitch_params *sp,
                         double *stats);
/* stage entry points (host buffers) for the tests.  visibility: vis[nv], bit v = view v sees the vertex.  rhs: a caller's colouring (rgb
 * nv*3 bytes, best_view in -1 .. V - 1, vis) -> G nv*3 doubles (0 for an uncoloured vertex), deg nv int32, counts = stats [2] .. [6].
 * solve: `iterations` (0 .. 1000000, taken as given) steps from a caller's best_view (its sign alone counts), rgb and G -> x nv*3 doubles
 * (c for an uncoloured vertex) and the relative residual. */
int rsm_stage_mesh_visibility(rsm_ctx *ctx, const float *xyz, int64_t nv, const int32_t *faces, int64_t nf, const rsm_dedup_view *views, int n_pairs,
                              const rsm_mesh_color_params *p, uint64_t *vis);
int rsm_stage_mesh_stitch_rhs(rsm_ctx *ctx, const float *xyz, int64_t nv, const int32_t *faces, int64_t nf, const rsm_dedup_view *views, int n_pairs,
                              const uint8_t *rgb, const int32_t *best_view, const uint64_t *vis, int seam_gradient, double *G, int32_t *deg, int64_t counts[5]);
int rsm_stage_mesh_stitch_solve(rsm_ctx *ctx, const int32_t *faces, int64_t nv, int64_t nf, const int32_t *best_view, const uint8_t *rgb, const double *G,
                                double lambda, int iterations, double *x, double *rel_residual);

/* ---- the vertices no view sees filled from the colours around them (TextureStitcher's mesh is coloured everywhere) --------
 * Run after rsm_mesh_color or rsm_mesh_stitch, on their rgb and best_view.  A vertex is known when best_view >= 0 (the sign alone counts),
 * else unknown.  The incidences of a vertex are its corner list's, as in rsm_mesh_stitch, but to every neighbour, known or not.
 * Front: round r = 1, 2, ... gives every unknown vertex without a level that has incidences to vertices of level < r (known: 0) the mean of
 * their values, in order, and the level r; it stops after the first round that reaches nothing, or after max_rounds rounds.  L = the largest
 * level.  The vertices it reached are the filled ones; the others (a component without a known vertex, or beyond max_rounds) keep their
 * bytes.  System, per channel over the filled vertices: sum_j (x_i - x_j) = 0 over the incidences to known (fixed) and filled neighbours.
 * Solver: rsm_mesh_stitch's Chebyshev iteration from the front's values on the interval [lmin, 2], lmin = 1 / (2 (L + 1))^2: `iterations`
 * steps, or with iterations = 0 the least k with T_k(sigma) >= 1 / reduction.  Filled bytes = clamp(floor(x + 0.5), 0, 255); known bytes
 * and best_view are untouched (a filled vertex keeps best_view -1).
 * The rounds go out RSM_MESH_FILL_ROUND_BATCH at a time; between two batches the largest level is read back.  A round that reaches nothing
 * is a no-op, so the result does not depend on that number (the front stage takes another one to show it). */
typedef struct rsm_mesh_fill_params {
    int max_rounds;     /* >= 0; 0 = until a round reaches nothing */
    int iterations;     /* 0 .. 1000000; 0 = from reduction */
    double reduction;   /* in (0, 1), used when iterations = 0 (1e-4) */
} rsm_mesh_fill_params;
#define RSM_MESH_FILL_MAX_ITERATIONS 1000000
#define RSM_MESH_FILL_ROUND_BATCH 16
/* stats: [0] vertices, [1] known, [2] filled, [3] unreached, [4] rounds L, [5] kept incidences of the filled vertices, [6] the largest of
 * their counts, [7] steps run, [8] values clamped, [9] the largest |x - x_front| over the filled vertices */
#define RSM_MESH_FILL_STATS 10
/* host buffers: faces nf*3 int32, rgb nv*3 bytes in and out, best_view nv int32 in, level nv int32 out (may be NULL): 0 known, 1 .. L filled,
 * -1 unreached.  An empty mesh, no unknown vertex, no known vertex: the input's bytes, RSM_OK.  RSM_E_INVALID (rsm_last_error names the
 * cause): a NULL pointer, a face index outside [0, nv), 3 nf >= 2^31, nv above INT32_MAX, a negative count, max_rounds < 0, iterations
 * outside 0 .. 1000000, reduction outside (0, 1) when it is used (or one that needs more than 1000000 steps). */
int rsm_mesh_fill_colors(rsm_ctx *ctx, const int32_t *faces, int64_t nv, int64_t nf, uint8_t *rgb, const int32_t *best_view, int32_t *level,
                         const rsm_mesh_fill_params *p, double *stats);
/* the same on DEVICE buffers (faces, rgb, best_view, level) */
int rsm_mesh_fill_colors_device(rsm_ctx *ctx, const int32_t *d_faces, int64_t nv, int64_t nf, uint8_t *d_rgb, const int32_t *d_best_view, int32_t *d_level,
                                const rsm_mesh_fill_params *p, double *stats);
/* the same on the context's last mesh and the colours rsm_mesh_color_last / rsm_mesh_stitch_last left with it (RSM_E_STATE when it has
 * none); rsm_mesh_last_colors then copies out the filled bytes and the unchanged best views */
int rsm_mesh_fill_colors_last(rsm_ctx *ctx, const rsm_mesh_fill_params *p, double *stats);
/* stage entry points (host buffers) for the tests.  front: rgb, best_view -> x nv*3 doubles (the bytes as doubles where the front wrote
 * nothing), level nv int32 (as above), *rounds = L; round_batch: 0 (RSM_MESH_FILL_ROUND_BATCH) or 1 .. 1024 rounds between two read-backs.  solve: `iterations` (0 .. 1000000, taken as given) steps from a caller's x, level
 * (0 known, 1 .. L filled, anything else unreached) and L >= 0 -> x (in and out; only filled rows change). */
int rsm_stage_mesh_fill_front(rsm_ctx *ctx, const int32_t *faces, int64_t nv, int64_t nf, const uint8_t *rgb, const int32_t *best_view, int max_rounds, int round_batch,
                              double *x, int32_t *level, int *rounds);
int rsm_stage_mesh_fill_solve(rsm_ctx *ctx, const int32_t *faces, int64_t nv, int64_t nf, const int32_t *level, int L, int iterations, double *x);

/* ---- kernel microbenchmark (MDE/s: pixel x candidate NCC evaluations) -------------------- */
/* Runs the NCC interval-argmax kernel `iters` times on a resident level-sized problem with
 * `cands` candidates per pixel and returns average milliseconds per launch. */
int rsm_bench_ncc(rsm_ctx *ctx, int W, int H, int r, int cands, int iters, double *ms_per_launch);

#ifdef __cplusplus
}
#endif
#endif /* RSM_H */
