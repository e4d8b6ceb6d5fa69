/* plp_front.h — C ABI of libplp_front.so, the MI355X-native feature front-end and matcher
 * that replaces the per-frame hot path of Structure-PLP-SLAM (src/PLPSLAM/feature,
 * src/PLPSLAM/match).  Plain pointers and sizes only; no C++/torch types cross this boundary.
 *
 * Each entry point cites the reference interface it replaces (paths relative to the
 * reference repository root).  All functions return a plp_status and never throw.
 *
 * Pointer naming: `h_` / unprefixed = host memory, `d_` = device (HBM) memory of the
 * context's GPU.  Batched `_device` entry points are asynchronous on `hip_stream`
 * (a hipStream_t passed as void*; NULL = HIP's default stream, so that callers working on the
 * default stream -- e.g. PyTorch's current stream -- stay ordered) unless stated otherwise.  The host-pointer entry
 * points use the context's own non-blocking stream and synchronise it before returning.
 */
#ifndef PLP_FRONT_H
#define PLP_FRONT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum plp_status {
    PLP_OK = 0,
    PLP_ERR_INVALID_ARG = 1,   /* what the reference reports via std::runtime_error / assert */
    PLP_ERR_NO_DEVICE = 2,     /* no usable MI355X / HIP runtime failure at create time */
    PLP_ERR_HIP = 3,           /* a HIP call failed; see plp_last_error() */
    PLP_ERR_CAPACITY = 4,      /* caller buffer too small (n_out still holds the needed size) */
    PLP_ERR_OVERFLOW = 5,      /* an internal per-level candidate buffer overflowed */
    PLP_ERR_UNSUPPORTED = 6
} plp_status;

const char* plp_strerror(plp_status s);
const char* plp_last_error(void);      /* thread-local detail string of the last failure */
int plp_version(void);                 /* 100*major + minor */
int plp_device_count(void);            /* number of visible HIP devices (0 on a CPU-only box) */

/* ------------------------------------------------------------------------------------------
 * Key point record: field-for-field cv::KeyPoint (28 bytes), the element type of
 * `std::vector<cv::KeyPoint>& keypts` in feature::orb_extractor::extract
 * (src/PLPSLAM/feature/orb_extractor.h:53-54).
 * ---------------------------------------------------------------------------------------- */
typedef struct plp_keypoint {
    float x, y;        /* pt, in level-0 pixel coordinates                                    */
    float size;        /* (unsigned)(31 * scale_factor[octave])     orb_extractor.cc:448,457  */
    float angle;       /* degrees in [0,360), intensity-centroid    orb_extractor.cc:708-735  */
    float response;    /* FAST-9/16 corner score                                              */
    int32_t octave;    /* pyramid level                                                        */
    int32_t class_id;  /* always -1                                                            */
} plp_keypoint;

/* ------------------------------------------------------------------------------------------
 * ORB extractor  — replaces feature::orb_extractor (src/PLPSLAM/feature/orb_extractor.h:38-176)
 * and feature::orb_params (src/PLPSLAM/feature/orb_params.h:34-73).
 * ---------------------------------------------------------------------------------------- */
typedef struct plp_orb plp_orb;   /* one per feature::orb_extractor instance; owns a HIP stream */

typedef struct plp_orb_params {   /* orb_params.h:52-60, defaults 2000 / 1.2 / 8 / 20 / 7 */
    uint32_t max_num_keypts;
    float scale_factor;
    uint32_t num_levels;
    uint32_t ini_fast_thr;
    uint32_t min_fast_thr;
    const float* mask_rects;      /* n_mask_rects x [x_min/cols, x_max/cols, y_min/rows, y_max/rows] */
    int32_t n_mask_rects;
} plp_orb_params;

void plp_orb_default_params(plp_orb_params* p);

/* orb_extractor::orb_extractor(const orb_params&)  (orb_extractor.cc:66-71).  Validation failures
 * that make orb_params throw std::runtime_error (orb_params.cc:40-54) return PLP_ERR_INVALID_ARG. */
plp_status plp_orb_create(const plp_orb_params* params, int device, plp_orb** out);
void plp_orb_destroy(plp_orb* ctx);

typedef enum plp_orb_param_id {
    PLP_ORB_MAX_NUM_KEYPOINTS = 0,     /* get/set_max_num_keypoints        orb_extractor.cc:162-171 */
    PLP_ORB_SCALE_FACTOR = 1,          /* get/set_scale_factor             :173-182 */
    PLP_ORB_NUM_SCALE_LEVELS = 2,      /* get/set_num_scale_levels         :184-193 */
    PLP_ORB_INITIAL_FAST_THRESHOLD = 3,/* get/set_initial_fast_threshold   :195-203 */
    PLP_ORB_MINIMUM_FAST_THRESHOLD = 4 /* get/set_minimum_fast_threshold   :205-213 */
} plp_orb_param_id;
plp_status plp_orb_set_param(plp_orb* ctx, plp_orb_param_id id, double value);  /* re-runs initialize() like the setters */
plp_status plp_orb_get_param(const plp_orb* ctx, plp_orb_param_id id, double* value);

/* get_scale_factors / get_inv_scale_factors / get_level_sigma_sq / get_inv_level_sigma_sq
 * (orb_extractor.cc:215-233); each output array holds num_levels floats (NULL = skip).
 * quota = num_keypts_per_level_ (orb_extractor.cc:245-253). */
plp_status plp_orb_get_tables(const plp_orb* ctx, int32_t* n_levels, float* scale_factors,
                              float* inv_scale_factors, float* level_sigma_sq, float* inv_level_sigma_sq,
                              uint32_t* quota);

/* orb_extractor::extract(in_image, in_image_mask, keypts, out_descriptors)  (orb_extractor.cc:73-160).
 * Host pointers, synchronous.  img: rows x cols CV_8UC1, `step` bytes per row.  mask: NULL or same
 * size (0 = masked).  kps/desc: caller buffers of `cap` records / cap x 32 bytes; *n_out receives the
 * number of key points (concatenated by level).  An empty image (rows==0||cols==0) is a no-op that
 * leaves *n_out untouched, as the reference does (:76-79). */
plp_status plp_orb_extract(plp_orb* ctx, const uint8_t* img, int32_t rows, int32_t cols, size_t step,
                           const uint8_t* mask, size_t mask_step,
                           plp_keypoint* kps, uint8_t* desc, int32_t cap, int32_t* n_out);

/* Batched replay form of extract(): B frames already resident in HBM, results stay in HBM.
 * d_imgs: B frames, frame b at d_imgs + b*frame_stride, `step` bytes per row.
 * d_mask: NULL, or masks at d_mask + b*mask_frame_stride (mask_frame_stride==0: one shared mask).
 * d_kps: B x cap records, d_desc: B x cap x 32 bytes, d_counts: B int32 (key points per frame;
 * a frame needing more than `cap` slots is truncated and flagged in plp_orb_last_batch_status).
 * Asynchronous on hip_stream. */
plp_status plp_orb_extract_batch_device(plp_orb* ctx, const uint8_t* d_imgs, int32_t B, int32_t rows,
                                        int32_t cols, size_t step, size_t frame_stride,
                                        const uint8_t* d_mask, size_t mask_step, size_t mask_frame_stride,
                                        plp_keypoint* d_kps, uint8_t* d_desc, int32_t cap,
                                        int32_t* d_counts, void* hip_stream);
/* Synchronises the last batch's stream and reports truncation / overflow (PLP_OK if none). */
plp_status plp_orb_last_batch_status(plp_orb* ctx);

/* Per-stage timing with HIP events recorded on the stream the kernels run on (profiling mode makes
 * every batch synchronous; leave it off in throughput runs).  ms7 = accumulated milliseconds of
 * {level-0 copy, pyramid, FAST cells, blur, quadtree, orientation+rBRIEF, whole batch}. */
plp_status plp_orb_set_profiling(plp_orb* ctx, int32_t enable);
plp_status plp_orb_get_stage_times(plp_orb* ctx, double* ms7, int64_t* n_batches);

/* orb_extractor::image_pyramid_ (public member, orb_extractor.h:101; read by match::stereo,
 * src/PLPSLAM/data/frame.cc:277-281).  Copies level `level` of frame `frame` of the last call to host. */
plp_status plp_orb_pyramid_level_size(const plp_orb* ctx, int32_t level, int32_t* rows, int32_t* cols);
plp_status plp_orb_pyramid_host(plp_orb* ctx, int32_t frame, int32_t level, uint8_t* dst, size_t dst_step);

/* match::stereo(...).compute(stereo_x_right, depths)  (src/PLPSLAM/match/stereo.cc:30-150, built in data/frame.cc:277-281):
 * per left key point the best right key point in its row band (Hamming < 75, octave +-1, disparity in [0, fx*b/b)),
 * 11x11 L1 patch slide on the pyramid level + parabola, 2x-median correlation rejection.  The image pyramids are the
 * ones `left` / `right` built in their last extract call (the reference passes orb_extractor::image_pyramid_).
 * Outputs: n_l floats each, -1 where no stereo match.  More than 65535 key points on either side are refused with
 * PLP_ERR_INVALID_ARG, as a `cap` above 65535 is by the batched entry (the kernel packs the right index into 16 bits). */
plp_status plp_stereo_compute(plp_orb* left, plp_orb* right, const plp_keypoint* kps_l, int32_t n_l, const plp_keypoint* kps_r, int32_t n_r,
                              const uint8_t* desc_l, const uint8_t* desc_r, float focal_x_baseline, float true_baseline,
                              float* stereo_x_right, float* depths);
/* Batched: key points / descriptors / counts as produced by plp_orb_extract_batch_device of the two extractors. */
plp_status plp_stereo_compute_batch_device(plp_orb* left, plp_orb* right, const plp_keypoint* d_kps_l, const int32_t* d_cnt_l,
                                           const plp_keypoint* d_kps_r, const int32_t* d_cnt_r, const uint8_t* d_desc_l,
                                           const uint8_t* d_desc_r, int32_t cap, int32_t B, float focal_x_baseline, float true_baseline,
                                           float* d_x_right, float* d_depths, void* hip_stream);

/* Stage read-back for parity tests (synchronous; host destination).
 *   PLP_ORB_DBG_BLURRED   : the 7x7 sigma-2 blurred level image (orb_extractor.cc:148-149), rows x cols u8 dense
 *   PLP_ORB_DBG_CANDIDATES: keypts_to_distribute of a level (orb_extractor.cc:359,433) as int32 triples
 *                           (x, y, score) in border-relative coordinates, reference order
 *   PLP_ORB_DBG_SELECTED  : per-level quadtree output (orb_extractor.cc:443) as int32 triples (x, y, score)
 * *n_out = number of bytes (BLURRED) or triples written. */
typedef enum plp_orb_debug_id { PLP_ORB_DBG_BLURRED = 0, PLP_ORB_DBG_CANDIDATES = 1, PLP_ORB_DBG_SELECTED = 2 } plp_orb_debug_id;
plp_status plp_orb_debug_read(plp_orb* ctx, plp_orb_debug_id what, int32_t frame, int32_t level,
                              void* dst, size_t dst_bytes, int64_t* n_out);

/* ------------------------------------------------------------------------------------------
 * Line front-end — replaces feature::LineFeatureTracker (src/PLPSLAM/feature/line_extractor.h:61-104):
 * LSD detection (LSDDetectorC::detect with the options of line_extractor.cc:113-122, which wraps
 * cv::createLineSegmentDetector) + LBD description (BinaryDescriptor::compute) + the length filter and
 * the 2-D line functions of line_extractor.cc:134-159.
 * ---------------------------------------------------------------------------------------- */
typedef struct plp_keyline {   /* field-for-field cv::line_descriptor::KeyLine, 68 bytes (descriptor_custom.hpp:139-174) */
    float angle;
    int32_t class_id;
    int32_t octave;
    float pt_x, pt_y;
    float response;
    float size;
    float startPointX, startPointY, endPointX, endPointY;
    float sPointInOctaveX, sPointInOctaveY, ePointInOctaveX, ePointInOctaveY;
    float lineLength;
    int32_t numOfPixels;
} plp_keyline;

typedef struct plp_line plp_line;   /* one per LineFeatureTracker instance */
/* LineFeatureTracker(camera::base*): the camera only feeds the identity "undistortion" remap
 * (line_extractor.cc:40-86,103), which is elided; no parameter is needed. */
plp_status plp_line_create(int device, plp_line** out);
void plp_line_destroy(plp_line* ctx);

/* extract_LSD_LBD(img, frame_keylsd, frame_lbd_descr, keyline_functions)  (line_extractor.cc:88-160).
 * Host pointers, synchronous.  kl: cap records, lbd: cap x 32 bytes, linefn: cap x 3 doubles
 * (normalised (sx,sy,1) x (ex,ey,1)); the reference APPENDS to keyline_functions (:158) — the caller's
 * facade appends these rows.  *n_out = number of kept lines. */
plp_status plp_line_extract(plp_line* ctx, const uint8_t* img, int32_t rows, int32_t cols, size_t step,
                            plp_keyline* kl, uint8_t* lbd, double* linefn, int32_t cap, int32_t* n_out);
/* Batched replay form: B frames resident in HBM, results stay in HBM (B x cap records each). Asynchronous. */
plp_status plp_line_extract_batch_device(plp_line* ctx, const uint8_t* d_imgs, int32_t B, int32_t rows, int32_t cols,
                                         size_t step, size_t frame_stride, plp_keyline* d_kl, uint8_t* d_lbd,
                                         double* d_linefn, int32_t cap, int32_t* d_counts, void* hip_stream);
plp_status plp_line_last_batch_status(plp_line* ctx);
/* HIP-event stage timing (profiling mode makes batches synchronous).  ms9 = accumulated ms of {11-tap blur + x0.5 resize,
 * gradient + bins, seed order, region growing, key lines, 5-tap blur + Sobel, LBD, finalize, whole batch}. */
plp_status plp_line_set_profiling(plp_line* ctx, int32_t enable);
plp_status plp_line_get_stage_times(plp_line* ctx, double* ms9, int64_t* n_batches);
/* Tuning / parity tests: waves that share one frame in LSD region growing.  0 (default) = automatic: a workgroup of up to 8 waves per
 * frame (one sequential main wave, helpers that grow regions of later seeds speculatively and hand them over, k_lsd_grow_mw) for batches
 * of at most 256 frames -- the single-frame call of data/frame.cc:1146-1163 --, one wave per frame for larger batches; 1 = always one wave
 * per frame; 2..8 = that many waves for every batch of at most 256 frames.  The results are identical whichever is used. */
plp_status plp_line_set_grow_waves(plp_line* ctx, int32_t waves);
/* The order in which LSD visits its seed pixels.  OpenCV's lsd.cpp (reached from LSDDetector_custom.cpp:244-257) sorts every pixel by
 * gradient bin with std::sort and a comparator that looks at the bin only: inside a bin the order is whatever the C++ library's
 * (unstable) algorithm leaves, and region growing depends on it.
 *   PLP_SEED_ORDER_LIBSTDCXX  (default) the permutation libstdc++'s std::sort produces (introsort replayed on the device,
 *                             seed_sort_kernels.hip): bit-identical to a reference built with GCC's library
 *   PLP_SEED_ORDER_STABLE     bin descending, row-major inside a bin (what the LSD paper describes; cheaper: only defined pixels are
 *                             sorted, ~4.5 ms less per 2048 frames) -- for callers that do not need the reference's tie order
 * 3.5 % of the key lines differ between the two. */
typedef enum plp_seed_order { PLP_SEED_ORDER_STABLE = 0, PLP_SEED_ORDER_LIBSTDCXX = 1 } plp_seed_order;
plp_status plp_line_set_seed_order(plp_line* ctx, int32_t order);
plp_status plp_line_get_seed_order(const plp_line* ctx, int32_t* order);
/* Gives back device memory the current settings do not need: the exact seed order's buffers (630 KB per frame of the largest 640 x 480 batch seen) while
 * PLP_SEED_ORDER_STABLE is selected, and the several-waves grower's region lists.  plp_line_set_seed_order itself frees nothing (a caller may alternate the two
 * orders per batch at no cost).  Waits for the device (hipFree): call it where a pause is acceptable.  The caller's current device is left as it was. */
plp_status plp_line_trim(plp_line* ctx);

/* Stage read-back for parity tests (synchronous, host destination, frame of the last call):
 *   SCALED   u8 sh x sw dense (the 11-tap blur + x0.5 image LSD works on)
 *   ORDER    int32 seed order (pixel index y*sw + x) of the pixels whose level-line angle is defined (gradient magnitude > rho):
 *            region growing starts nowhere else, so only those are ordered
 *   RAW      float x 4 per LSD segment (x1,y1,x2,y2), in detection order
 *   ALL_KL   plp_keyline of every segment longer than min_length (before the >= 60 px filter)
 *   ALL_LBD  32 bytes per ALL_KL record
 *   SOBEL_DX / SOBEL_DY  int16 rows x cols */
typedef enum plp_line_debug_id { PLP_LINE_DBG_SCALED = 0, PLP_LINE_DBG_ORDER = 1, PLP_LINE_DBG_RAW = 2, PLP_LINE_DBG_ALL_KL = 3,
                                 PLP_LINE_DBG_ALL_LBD = 4, PLP_LINE_DBG_SOBEL_DX = 5, PLP_LINE_DBG_SOBEL_DY = 6,
                                 PLP_LINE_DBG_GROW_STATS = 7 /* int32[4]; one wave per frame: regions grown, pixels accepted, exact (in-band) decisions, 0;
                                    several waves per frame: regions the main wave grew itself, helper results taken, rejected, number of waves */ } plp_line_debug_id;
plp_status plp_line_debug_read(plp_line* ctx, plp_line_debug_id what, int32_t frame, void* dst, size_t dst_bytes, int64_t* n_out);
/* Host model of the bin ranking of match::angle_checker (the reference sorts its 30 histogram bins by size with std::sort,
 * src/PLPSLAM/match/angle_checker.h:165-176; the kernels reproduce libstdc++'s algorithm so that ties fall as in a reference built with
 * GCC): idx = the indices 0..n-1, n <= 64, in that order.  depth_limit < 0 = the library's recursion budget.  No GPU needed. */
int32_t plp_model_index_sort_host(const int32_t* sizes, int32_t n, int32_t depth_limit, uint32_t* idx);
/* Host model of the sort the quadtree kernel runs on levels of a few hundred candidates (csrc/quadtree_model.hpp qt_rank): perm[r] = the index of the
 * entry of rank r by (keys[i] >> shift, i), i.e. a stable sort by the shifted key.  The shifted keys must be below 2^31.  No GPU needed.  Returns n, or -1
 * for a bad argument. */
int32_t plp_model_quadtree_rank_sort_host(const uint32_t* keys, int32_t n, int32_t shift, uint32_t* perm);
/* Host model of the exact seed sort (csrc/seed_sort_model.hpp): std::__introsort_loop, in place, on n entries whose sort key is bits 20..29
 * (larger first), computed as the rank-paired partitions the kernel runs; depth_limit < 0 = the library's 2 * floor(log2 n).  skip_key > 0:
 * parts that can only hold keys below it are left as they are, as the kernel leaves the undefined pixels of a frame (they are sorted along
 * but never seed a region); the order of the entries with keys >= skip_key after a stable sort by key is std::sort's all the same.
 * No GPU needed.  Returns 0, or -1 for a bad argument. */
int32_t plp_model_seed_introsort_host(uint32_t* entries, int64_t n, int32_t depth_limit, uint32_t skip_key);
/* Test entry: the KERNEL's introsort loop on caller-made entries (host pointer, in place), one workgroup, chosen recursion budget and skip key.
 * variant 0: the kernel configuration of large batches (4 waves, 4096-entry LDS window), 1: of batches up to 256 frames (16 waves, 24576 entries).
 * n_live (may be NULL): the length of the array's LIVE part.  With a skip key the kernel stops storing into the right part of a global-memory partition
 * whose pivot key lies below it once that part is the end of the live array (only keys below the skip key live there, nothing reads them again): entries
 * [0, n_live) equal the host model's, entries behind are unspecified (stale copies).  Without a skip key n_live = n. */
plp_status plp_seed_introsort_debug(int32_t device, uint32_t* entries, int64_t n, int32_t depth_limit, uint32_t skip_key, int32_t variant, int32_t* n_live);
/* How the exact seed sort's kernel partitions a segment of n_segment entries (longer than the variant's LDS window) of a frame whose seed array has n_frame
 * entries: the stoppers' entries change sides through an LDS tile of the returned number of ranks per side, tile after tile (at least 64 for every frame size).
 * masks_in_lds (may be NULL): 1 when the segment's chunk masks are held in LDS too.
 * No GPU needed.  Returns -1 for a bad argument. */
int32_t plp_seed_sort_tile_ranks(int64_t n_frame, int64_t n_segment, int32_t variant, int32_t* masks_in_lds);
/* Host model of the LSD gradient kernel's (float)cos((double)a), (float)sin((double)a) fast path (csrc/sincos_ziv.hpp): proven[i] = 0 marks the
 * arguments for which the kernel falls back to the general f64 routine.  Returns the number of proven arguments.  No GPU needed. */
int32_t plp_model_sincos_host(const float* a, int64_t n, float* c, float* s, uint8_t* proven);
/* Host build of the null vector the point triangulation uses (csrc/null4.hpp): for n row-major 4 x 4 matrices
 * A[16 i ..], out_v[4 i ..] = the column of V of the cyclic one-sided Jacobi whose column of A V has the smallest squared norm (ties: the
 * lowest index; sign unspecified), out_sweeps[i] (may be NULL) = the sweeps that rotated, 30 = the limit was reached.  The device runs the
 * same source.  No GPU needed.  Returns n, or -1 for a bad argument. */
int32_t plp_model_null_vector4_host(const double* A, int32_t n, double* out_v, int32_t* out_sweeps);
plp_status plp_line_scaled_size(const plp_line* ctx, int32_t* rows, int32_t* cols);
/* Diagnostics of frame 0 of the last batch, 12 values.  One wave per frame: shader cycles {whole wave, region_grow, region2rect, refine},
 * regions grown, pixels grown, 0 x 6.  Several waves per frame, the main wave's view: cycles {whole, waiting for helpers, growing regions
 * itself}, helper attempts | give-ups << 32, regions it grew itself, results taken | rejected << 32, cycles {taking results, publishing its
 * own regions, group set-up}, 0 x 3. */
plp_status plp_line_debug_grow_profile(plp_line* ctx, int64_t* out12);

/* ------------------------------------------------------------------------------------------
 * Hamming matchers, array form — replace the inner loops of the reference's src/PLPSLAM/match directory.
 *
 * The reference's matchers walk data::frame / data::landmark objects (match/projection.h,
 * match/robust.h); the host facade flattens what those loops read into plain arrays, calls one of
 * the entry points below and writes the returned associations back.  Targets = key points of the
 * current frame, queries = landmarks / last-frame key points / key-frame key points IN THE
 * REFERENCE'S ITERATION ORDER (results depend on it: an accepted query blocks its key point for all
 * later queries).  B independent problems per call; arrays are B x n_cap / B x m_cap, row-major.
 * ---------------------------------------------------------------------------------------- */
typedef struct plp_keyline plp_keyline_fwd_;
typedef struct plp_matcher plp_matcher;   /* owns a HIP stream and scratch; one per calling thread */
plp_status plp_matcher_create(int device, plp_matcher** out);
void plp_matcher_destroy(plp_matcher* ctx);

typedef enum plp_match_mode {
    PLP_MATCH_MODE_LANDMARKS = 0,   /* projection::match_frame_and_landmarks          match/projection.cc:37-121  */
    PLP_MATCH_MODE_LAST_FRAME = 1,  /* projection::match_current_and_last_frames      match/projection.cc:214-358 */
    PLP_MATCH_MODE_BRUTE_FORCE = 2, /* robust::brute_force_match                      match/robust.cc:257-385     */
    PLP_MATCH_MODE_LANDMARKS_LINE = 3,  /* projection::match_frame_and_landmarks_line      match/projection.cc:124-212 */
    PLP_MATCH_MODE_LAST_FRAME_LINE = 4, /* projection::match_current_and_last_frames_line  match/projection.cc:361-527 */
    PLP_MATCH_MODE_BOW = 5,         /* bow_tree::match_frame_and_keyframe / match_keyframes   match/bow_tree.cc:41-165, 167-307 */
    PLP_MATCH_MODE_FUSE = 6,        /* fuse::replace_duplication, the search part              match/fuse.cc:169-298        */
    PLP_MATCH_MODE_FUSE_LINE = 7,   /* fuse::replace_duplication_line, the search part         match/fuse.cc:335-470        */
    PLP_MATCH_MODE_TRIANGULATION = 8/* robust::match_for_triangulation                         match/robust.cc:43-216       */
} plp_match_mode;

/* plp_match_args.flags */
#define PLP_MATCH_FLAG_NO_CHI2 1        /* FUSE: no chi-square gates (fuse::detect_duplication fuse.cc:40-166,
                                           projection::match_keyframes_mutually projection.cc:894-1142) */
#define PLP_MATCH_FLAG_SIGNED_LEVEL 2   /* FUSE: octave window [q_level-1, q_level] in SIGNED arithmetic (detect_duplication
                                           declares `const int pred_scale_level`, fuse.cc:109,126) */
#define PLP_MATCH_FLAG_UNSIGNED_LEVEL 4 /* LAST_FRAME with level_window 1: the manual window of match_by_Sim3_transform
                                           (projection.cc:862) in unsigned arithmetic, q_level == 0 matches nothing */
#define PLP_MATCH_FLAG_MARK_INVALIDATED 8 /* out_match = -2 (instead of -1) for a key point whose match the orientation check
                                           removed: the reference writes nullptr there (projection.cc:350-354), which differs
                                           from "never matched" when the slot held an observation-less landmark before */
/* plp_match_args.level_window (LAST_FRAME / LAST_FRAME_LINE): 0 = from `direction`, 1 = [q_level-1, q_level],
 * 2 = [q_level-1, q_level+1] */

typedef struct plp_match_grid {     /* camera::base grid (camera/base.h:91) used by data::get_keypoints_in_cell */
    float min_x, min_y;             /* img_bounds_.min_x_/min_y_ (float, camera/base.h:78-81) */
    double inv_cell_width, inv_cell_height;   /* double, camera/base.h:158-160 */
    int32_t cols, rows;             /* 64 x 48 */
} plp_match_grid;

typedef struct plp_match_args {
    int32_t mode;                   /* plp_match_mode */
    int32_t B, n_cap, m_cap;        /* B > 0; n_cap = 0 (a frame without key points / key lines) or m_cap = 0 (no landmarks / queries) is a valid call: nothing can match --
                                     * the reference's loops do not run -- every out_match slot becomes -1, every out_num 0 (fuse modes: out_query_best -1); input pointers
                                     * of the empty side may be NULL */
    /* targets (current frame): data::frame::undist_keypts_, descriptors_, stereo_x_right_, and
     * "landmarks_[idx] && landmarks_[idx]->has_observation()" as a byte flag */
    const plp_keypoint* t_kps;      /* B x n_cap (ignored in brute-force mode) */
    const uint8_t* t_desc;          /* B x n_cap x 32 */
    const float* t_x_right;         /* B x n_cap or NULL */
    const uint8_t* t_occupied;      /* B x n_cap or NULL */
    const float* t_angle;           /* brute-force mode: B x n_cap key point angles of frame 1 */
    const int32_t* t_counts;        /* B, or NULL = n_cap everywhere */
    /* queries */
    const uint8_t* q_valid;         /* B x m_cap or NULL: the skip tests at the top of the reference loops */
    const float* q_reproj;          /* B x m_cap x 2: reproj_in_tracking_ / reprojected last-frame landmark */
    const float* q_x_right;         /* B x m_cap or NULL */
    const int32_t* q_level;         /* B x m_cap: scale_level_in_tracking_ / last_frm.keypts_[i].octave */
    const float* q_angle;           /* B x m_cap: needed when check_orientation */
    const uint8_t* q_desc;          /* B x m_cap x 32 */
    const uint8_t* q_has_obs;       /* B x m_cap or NULL (= all 1): landmark::has_observation() */
    const int32_t* q_counts;        /* B, or NULL */
    float margin, lowe_ratio;       /* match::base(lowe_ratio, check_orientation) */
    int32_t direction;              /* LAST_FRAME: 0 neither, 1 assume_forward, 2 assume_backward (all problems; see `directions`) */
    int32_t check_orientation;
    int32_t num_levels;
    const float* scale_factors;     /* HOST pointer, num_levels floats (frame::scale_factors_) */
    plp_match_grid grid;
    /* line modes (targets = key lines of the current frame, candidates by data::get_keylines_in_cell,
     * data/common.cc:315-363): t_kl replaces t_kps, t_desc = _lbd_descr, q_reproj/q_reproj2 = reprojected start /
     * end point, q_desc = Line::get_descriptor().  t_kp_octave[i] = undist_keypts_.at(i).octave, the key POINT
     * octave the reference reads with a LINE index (projection.cc:187,192; LANDMARKS_LINE only).  RGB-D stereo
     * gate of LAST_FRAME_LINE: t_x_right / t_x_right2 = _stereo_x_right_cooresponding_to_keylines first / second,
     * q_x_right / q_x_right2 = x_right of the reprojected start / end point, is_rgbd != 0. */
    const plp_keyline* t_kl;        /* B x n_cap */
    const int32_t* t_kp_octave;     /* B x n_cap */
    const float* t_x_right2;        /* B x n_cap or NULL */
    const float* q_reproj2;         /* B x m_cap x 2 */
    const float* q_x_right2;        /* B x m_cap or NULL */
    int32_t is_rgbd;
    int32_t num_levels_lsd;         /* last_frm._num_scale_levels_lsd (upper bound of the assume_forward window) */
    /* BOW mode: queries = key-frame features listed in BoW node order (the order the reference walks the feature
     * vector in), q_group / t_group = node id of every feature (frame features of one node are visited in ascending
     * index); q_valid = feature has a live landmark; t_occupied = static skip of a target (match_keyframes: key frame 2
     * feature without a live landmark); q_angle / t_angle when check_orientation.  Accept: best <= 50 and
     * lowe_ratio * second >= best.
     * FUSE mode: independent queries (no blocking): window margin * scale_factors[q_level] around q_reproj_d (all
     * octaves), then octave in [q_level - 1, q_level] WITH THE REFERENCE'S UNSIGNED ARITHMETIC (q_level == 0 rejects
     * everything, fuse.cc:236), the chi-square gates on the f64 reprojection (5.99146 / 7.81473 with
     * inv_level_sigma_sq, stereo when t_x_right >= 0), best <= 50.  Result per query in out_query_best. */
    const int32_t* q_group;         /* B x m_cap */
    const int32_t* t_group;         /* B x n_cap */
    const double* q_reproj_d;       /* B x m_cap x 2 (FUSE) */
    const float* inv_level_sigma_sq;/* HOST pointer, num_levels floats (FUSE) */
    int32_t* out_query_best;        /* B x m_cap (FUSE, FUSE_LINE): best key point / key line per query, -1 = none; q >= q_counts[b] not written */
    /* Variants of the same loops:
     *  - projection::match_frame_and_keyframe[_line] (projection.cc:529-645, 648-779) = LAST_FRAME[_LINE] with
     *    direction 0, t_x_right NULL / is_rgbd 0, t_occupied = "landmarks_[i] != nullptr", q_has_obs NULL and
     *    hamm_dist_thr = the caller's threshold;
     *  - projection::match_by_Sim3_transform (:781-892) = LAST_FRAME, level_window 1, PLP_MATCH_FLAG_UNSIGNED_LEVEL,
     *    hamm_dist_thr 50, check_orientation 0, t_occupied = "matched_lms_in_keyfrm[i] != nullptr";
     *  - projection::match_keyframes_mutually (:894-1142) = two FUSE calls with PLP_MATCH_FLAG_NO_CHI2 and
     *    hamm_dist_thr 100, then the cross check (:1124-1139) on the two out_query_best arrays;
     *  - fuse::detect_duplication (fuse.cc:40-166) = FUSE with NO_CHI2 | SIGNED_LEVEL.
     * FUSE_LINE: targets t_kl / t_desc (LBD), queries q_reproj_d = reprojected start point, q_reproj2_d = end point
     *  (f64), window = data::get_keylines_in_cell(margin * scale_factors[q_level]) without octave test, gate
     *  5.99146 < (e_sp^2 + e_ep^2) * inv_level_sigma_sq[keyline.octave] in f64, best <= 50 (fuse.cc:431-470).
     * TRIANGULATION: BOW-style node-guided search between two key frames; q = features of key frame 1 in BoW node
     *  order (q_valid = "has no landmark"), t = features of key frame 2 (t_occupied = "has a landmark"); q_x_right /
     *  t_x_right >= 0 mark stereo key points; q_level = undist_keypts_[idx_1].octave; gates in f64 on the bearings:
     *  epipole test (both mono: skip if 0.99862953475 < epipole . bearing_2) and check_epipolar_constraint
     *  (robust.cc:387-405); Hamming <= 50, equal distances: the LATER candidate wins (`best < dist` skips, :124);
     *  exclusive on t; angle check on q_angle - t_angle.  `epipolar` = per problem 12 doubles: E_12 row-major, then
     *  the epipole bearing in key frame 2. */
    int32_t hamm_dist_thr;          /* 0 = the mode's own threshold */
    int32_t level_window;
    int32_t flags;
    const double* q_reproj2_d;      /* B x m_cap x 2 (FUSE_LINE) */
    const double* q_bearing;        /* B x m_cap x 3 (TRIANGULATION) */
    const double* t_bearing;        /* B x n_cap x 3 (TRIANGULATION) */
    const double* epipolar;         /* B x 12 (TRIANGULATION) */
    /* outputs: out_match[b][t] = index of the query associated with key point t (-1 = none),
     * out_num[b] = the matcher's return value (num_matches).  Slots beyond a problem's count are not written and keep the caller's
     * values, on both entries: out_match[b][t] for t >= t_counts[b], out_query_best[b][q] (fuse modes) for q >= q_counts[b]. */
    int32_t* out_match;             /* B x n_cap */
    int32_t* out_num;               /* B */
    /* Rows between two problems' blocks in q_desc (0 = m_cap).  In a batched replay the queries of frame b are the features of the
     * frames before it: with q_desc_stride = the per-frame capacity, q_desc may point INTO the batch's own descriptor array (one
     * frame back, m_cap = cap; or two frames back, m_cap = 2 cap: overlapping windows) and no descriptor is copied. */
    int32_t q_desc_stride;
    /* Performance hint for the windowed point modes (LANDMARKS, LAST_FRAME), 0 = none: an upper bound the caller EXPECTS for t_counts[b]
     * (a tracker knows its extractor's max_num_keypoints; the arrays are usually strided by a larger capacity n_cap).  The matcher then
     * keeps only that many targets of a frame in LDS -- more of its workgroups fit a compute unit -- and reads the targets of a frame that
     * has more from memory: results never depend on the hint. */
    int32_t t_count_hint;
    /* LAST_FRAME / LAST_FRAME_LINE with level_window 0: the motion direction of every problem (B values, 0 neither, 1 assume_forward,
     * 2 assume_backward; any other value = neither), in the entry's pointer space -- what plp_project_last_frame[_lines]_* write to
     * out_direction.  NULL: `direction` applies to every problem.  Ignored by the other modes. */
    const int32_t* directions;
} plp_match_args;

/* All array pointers in `a` are DEVICE pointers (except scale_factors); asynchronous on hip_stream. */
plp_status plp_match_device(plp_matcher* ctx, const plp_match_args* a, void* hip_stream);
/* Same with HOST pointers for one call (B problems are staged to HBM and back); synchronous. */
plp_status plp_match_host(plp_matcher* ctx, const plp_match_args* a);

/* Batched replay (bench.py, replay_driver.py): the queries of the tracker's per-frame matcher calls, built on the
 * device from the features of the preceding frames of the batch -- what tracking_module does on the host with poses, here for a
 * camera that pans by (shift_x, shift_y) pixels per frame (example/run_tum_rgbd_slam_with_line.cc replayed without a map).
 * feat_*: [(halo + B)][cap] rows; row halo + b is frame b of this rank's block, rows 0 .. halo-1 the predecessor's tail (halo >= 2).
 *   last-frame queries  (frame b-1 moved by 1 x shift):  q1_reproj [B][cap][2], q1_level [B][cap], q1_angle [B][cap], q1_counts [B]
 *   local-landmark queries (frames b-2, b-1 moved by 2 x / 1 x shift): q2_reproj [B][2 cap][2], q2_level [B][2 cap], q2_valid [B][2 cap]
 * Descriptors are not copied: pass q_desc = feat_desc + (halo - 1) * cap * 32 (resp. halo - 2) with q_desc_stride = cap. */
plp_status plp_replay_point_queries_device(const plp_keypoint* feat_kps, const int32_t* feat_counts, int32_t halo, int32_t B, int32_t cap, float shift_x,
                                           float shift_y, float* q1_reproj, int32_t* q1_level, float* q1_angle, int32_t* q1_counts, float* q2_reproj,
                                           int32_t* q2_level, uint8_t* q2_valid, void* hip_stream);
/* key lines of frame b-1, both end points moved by the shift: q_sp / q_ep [B][cap][2], q_level [B][cap] (KeyLine::octave), q_counts [B].
 * Optional (all four or none, halo >= 2): the local LINE landmarks of frame b for projection::match_frame_and_landmarks_line
 * (match/projection.cc:124-212, called per frame from tracking_module.cc:1060) = key lines of frame b-2 moved by 2 x shift, then those of
 * frame b-1 moved by 1 x shift: q2_sp / q2_ep [B][2 cap][2], q2_level [B][2 cap], q2_valid [B][2 cap]; their LBD rows are read in place
 * (q_desc = feat_lbd + (halo - 2) * cap * 32, q_desc_stride = cap).
 * Optional: t_kp_octave [B][cap] = frame b's undist_keypts_[i].octave for i < cap (the key POINT octave that matcher reads with a LINE
 * index, projection.cc:187,192) from feat_kps [halo + B][kp_cap] / feat_kp_counts [halo + B]. */
plp_status plp_replay_line_queries_device(const plp_keyline* feat_kl, const int32_t* feat_counts, int32_t halo, int32_t B, int32_t cap, float shift_x,
                                          float shift_y, float* q_sp, float* q_ep, int32_t* q_level, int32_t* q_counts, float* q2_sp, float* q2_ep,
                                          int32_t* q2_level, uint8_t* q2_valid, const plp_keypoint* feat_kps, const int32_t* feat_kp_counts, int32_t kp_cap,
                                          int32_t* t_kp_octave, void* hip_stream);

/* Host boundary of the batched replay: the live rows of a padded per-frame array packed back to back, so that the device-to-host copy
 * moves the features that exist instead of the capacity they were allotted (the std::vector<cv::KeyPoint> / cv::Mat rows that
 * orb_extractor::extract and extract_LSD_LBD hand back hold exactly that many entries, feature/orb_extractor.cc:124-132).
 * dst[offsets[b] + i] = src[b][i] for i < min(counts[b], cap), rows of row_bytes bytes (a multiple of 4); offsets [B + 1] = exclusive
 * prefix sum of the clamped counts, offsets[B] = total rows.  compute_offsets != 0 computes them first; pass 0 to reuse the offsets of an
 * earlier call with the same counts (key points + descriptors + matches share one set).  Asynchronous on hip_stream. */
plp_status plp_pack_rows_device(const void* src, const int32_t* counts, int32_t B, int32_t cap, int32_t row_bytes, void* dst, int64_t* offsets,
                                int32_t compute_offsets, void* hip_stream);

/* area::match_in_consistent_area(frm_1, frm_2, prev_matched_pts, matched_indices_2_in_frm_1, margin)
 * (src/PLPSLAM/match/area.cc:33-153; monocular initialisation, module/initializer.cc:191-192).  Host pointers, one
 * problem, synchronous.  kps_1/kps_2 = undist_keypts_ of the two frames, prev_matched_pts = n1 x 2 floats (updated in
 * place for matched key points), matched_2_in_1 = n1 int32 (idx_2 or -1); *num_matches = return value.
 * PLP_ERR_INVALID_ARG, with no output written, for n2 > 65535, a grid of more than 65536 cells or a non-positive grid extent. */
plp_status plp_match_area_host(plp_matcher* ctx, const plp_keypoint* kps_1, const uint8_t* desc_1, int32_t n1, const plp_keypoint* kps_2,
                               const uint8_t* desc_2, int32_t n2, const plp_match_grid* grid, float* prev_matched_pts, int32_t margin,
                               float lowe_ratio, int32_t check_orientation, int32_t* matched_2_in_1, int32_t* num_matches);

/* cv::line_descriptor::BinaryDescriptorMatcher::match(query, train, matches) — exact 1-NN over LBD descriptors by
 * multi-index hashing (src/PLPSLAM/feature/line_descriptor/binary_descriptor_matcher.cpp:197-255, 597-818), used for the
 * stereo line association (data/frame.cc:496-533; its filter is plp_stereo_keylines_* below) and two-key-frame line triangulation
 * (mapping_module.cc:481-531).
 * train_idx[q] = DMatch.trainIdx (among equally near train lines: the one MIH discovers first), dist[q] = DMatch.distance.
 * Nothing within Hamming distance 128 -> (-1, 256) (the reference reads uninitialised memory there). */
plp_status plp_lbd_match_1nn_host(plp_matcher* ctx, const uint8_t* q, int32_t nq, const uint8_t* t, int32_t nt, int32_t* train_idx, int32_t* dist);
/* B problems: q is B x nq_cap x 32, t is B x nt_cap x 32, counts per problem (NULL = cap); asynchronous. */
plp_status plp_lbd_match_1nn_device(plp_matcher* ctx, const uint8_t* d_q, const int32_t* d_q_counts, int32_t nq_cap, const uint8_t* d_t,
                                    const int32_t* d_t_counts, int32_t nt_cap, int32_t B, int32_t* d_train_idx, int32_t* d_dist, void* hip_stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Post-extract per-key-point step of every data::frame constructor (src/PLPSLAM/data/frame.cc:68-86, 110-128, ...;
 * SURVEY.md 8(f) item 1), so that features can stay in HBM between extraction and matching:
 *   camera::perspective::undistort_keypoints            camera/perspective.cc:130-162 (cv::undistortPoints, EPS|MAX_ITER 20 1e-6,
 *                                                        float camera matrix / distortion vector as the reference stores them)
 *   camera::perspective::convert_keypoints_to_bearings  camera/perspective.cc:165-175
 *   data::frame::compute_stereo_from_depth              data/frame.cc:1169-1219 (key points, and key lines when given)
 * (data::assign_keypoints_to_grid, data/common.cc:205-231, is what the matcher's preparation kernel builds from undist.)
 * undist gets pt / angle / size / octave of the distorted key point, response 0 and class_id -1, as the reference's resize()
 * + field copies do.  depth: B x rows x cols f32 (depth_step = bytes per row) or NULL (then x_right / depths may be NULL);
 * key-line outputs are written only for lines with both end-point depths >= 0, like the reference (pre-fill them).
 * Device pointers, asynchronous on hip_stream. */
typedef struct plp_camera {
    double fx, fy, cx, cy;          /* camera::perspective fx_, fy_, cx_, cy_ */
    double k1, k2, p1, p2, k3;      /* distortion */
    double focal_x_baseline;        /* camera::base focal_x_baseline_ */
} plp_camera;
plp_status plp_post_extract_device(plp_matcher* ctx, const plp_camera* cam, const plp_keypoint* d_kps, const int32_t* d_counts, int32_t cap,
                                   int32_t B, const float* d_depth, int32_t rows, int32_t cols, size_t depth_step, size_t depth_frame_stride,
                                   plp_keypoint* d_undist, double* d_bearings, float* d_x_right, float* d_depths,
                                   const plp_keyline* d_kl, const int32_t* d_kl_counts, int32_t kl_cap, float* d_kl_depths,
                                   float* d_kl_x_right, void* hip_stream);
/* One frame, host pointers, synchronous (NULL for the parts that are not wanted, as above). */
plp_status plp_post_extract_host(plp_matcher* ctx, const plp_camera* cam, const plp_keypoint* kps, int32_t n, const float* depth, int32_t rows,
                                 int32_t cols, size_t depth_step, plp_keypoint* undist, double* bearings, float* x_right, float* depths,
                                 const plp_keyline* kl, int32_t n_kl, float* kl_depths, float* kl_x_right);

/* The same step for every camera model of the reference (camera::base model_type_, chosen by Camera.model in config.cc:62-72):
 *   PLP_CAMERA_PERSPECTIVE      as plp_post_extract_* above, bit for bit
 *   PLP_CAMERA_FISHEYE          camera::fisheye::undistort_keypoints          camera/fisheye.cc:172-204 (cv::fisheye::undistortPoints with
 *                                                                              R empty, P = K, on the float cv_cam_matrix_ / cv_dist_params_,
 *                                                                              :47-48; OpenCV 3.4.16's loop: 10 Newton steps, |theta_fix| < 1e-8;
 *                                                                              a point that does not converge or changes sides -> (-1e6, -1e6))
 *                               camera::fisheye::convert_keypoints_to_bearings fisheye.cc:206-216 (the perspective formula)
 *                               undist: pt from the result, angle / size / octave copied, response 0, class_id -1; depth and key lines
 *                               as for perspective (frame.cc:1169-1219 does not depend on the model)
 *   PLP_CAMERA_EQUIRECTANGULAR  camera::equirectangular::undistort_keypoints   camera/equirectangular.cc:70-73 (undist = dist, every field)
 *                               camera::equirectangular::convert_keypoints_to_bearings :75-88 (lon = (x / (float)cols - 0.5) 2 pi,
 *                                                                              lat = -(y / (float)rows - 0.5) pi, float division then f64)
 *                               monocular only (:36): depth or key lines -> PLP_ERR_UNSUPPORTED
 * Bearings of the two new models use f64 tan / sin / cos of the device, not glibc's.
 * Invalid: an unknown model; fx or fy 0 (perspective, fisheye); cols or rows <= 0 (equirectangular).  The camera is checked before
 * anything else; then the arguments as for plp_post_extract_* (nothing to do -> PLP_OK, nothing written). */
typedef enum { PLP_CAMERA_PERSPECTIVE = 0, PLP_CAMERA_FISHEYE = 1, PLP_CAMERA_EQUIRECTANGULAR = 2 } plp_camera_model_type;
typedef struct plp_camera_model {
    int32_t model;                       /* a plp_camera_model_type: camera::base model_type_ */
    int32_t cols, rows;                  /* camera::base cols_, rows_ (unsigned int in the reference) */
    double fx, fy, cx, cy;               /* perspective / fisheye; ignored for equirectangular */
    double k1, k2, p1, p2, k3, k4;       /* perspective: k1 k2 p1 p2 k3; fisheye: k1 k2 k3 k4 (yaml names) */
    double focal_x_baseline;             /* camera::base focal_x_baseline_ */
} plp_camera_model;
/* B frames, device pointers, asynchronous: the parameters of plp_post_extract_device. */
plp_status plp_post_extract_model_device(plp_matcher* ctx, const plp_camera_model* cam, const plp_keypoint* d_kps, const int32_t* d_counts,
                                         int32_t cap, int32_t B, const float* d_depth, int32_t rows, int32_t cols, size_t depth_step,
                                         size_t depth_frame_stride, plp_keypoint* d_undist, double* d_bearings, float* d_x_right, float* d_depths,
                                         const plp_keyline* d_kl, const int32_t* d_kl_counts, int32_t kl_cap, float* d_kl_depths,
                                         float* d_kl_x_right, void* hip_stream);
/* One frame, host pointers, synchronous: the parameters of plp_post_extract_host. */
plp_status plp_post_extract_model_host(plp_matcher* ctx, const plp_camera_model* cam, const plp_keypoint* kps, int32_t n, const float* depth,
                                       int32_t rows, int32_t cols, size_t depth_step, plp_keypoint* undist, double* bearings, float* x_right,
                                       float* depths, const plp_keyline* kl, int32_t n_kl, float* kl_depths, float* kl_x_right);

/* ------------------------------------------------------------------------------------------------------------------
 * Local-landmark visibility (the queries of PLP_MATCH_MODE_LANDMARKS[_LINE]): the loops over local_landmarks_ in
 * tracking_module::search_local_landmarks / search_local_landmarks_line (src/PLPSLAM/tracking_module.cc:908-1064), for B frames at once.
 *   points  data::frame::can_observe(lm, 0.5, reproj, x_right, pred_scale_level)          data/frame.cc:797-824
 *           landmark::is_inside_in_orb_scale / get_{min,max}_valid_distance (0.7 x, 1.3 x) data/landmark.h:91-96, landmark.cc:297-307
 *           landmark::predict_scale_level(float dist, frame*)                              landmark.cc:319-340
 *   lines   data::frame::can_observe_line (both end points, the midpoint when one is out)  data/frame.cc:827-878
 *           Line::is_inside_in_feature_scale (0.8 x, 1.2 x), Line::predict_scale_level    data/landmark_line.cc:354-387
 *   camera::{perspective,fisheye,equirectangular}::reproject_to_image                      camera/perspective.cc:190-209, fisheye.cc:231-249
 *                                                                                          (the undistorted perspective formula), equirectangular.cc:104-119
 * Numeric contract: DESIGN.md section 5, D5 (f64 in the reference's order, glibc-free logf = (float)log((double)x), the x86 int cast,
 * the stale line end points).
 * Landmark j of problem b is slot b * m_cap + j, in local_landmarks_ order; slots j >= counts[b] are neither read nor written.
 * skip[j] != 0 = "identifier_in_local_lm_search_ == curr_frm_.id_ || will_be_erased()" (tracking_module.cc:938-946): never valid, no can_observe.
 * Outputs per slot j < counts[b]:
 *   out_valid     can_observe[_line]'s result (0 for a skipped slot): is_observable_in_tracking_
 *   out_level     pred_scale_level (scale_level_in_tracking_), written for valid slots only
 *   points: out_reproj / out_x_right = (float) of the f64 reprojection (reproj_in_tracking_, x_right_in_tracking_; the facade's cast,
 *           facade/PLPSLAM/match/projection.h:435-436), written for valid slots only
 *   lines:  out_reproj / out_reproj2 = the values of the reference's temporaries reproj_sp / reproj_ep after slot j's turn, for EVERY slot:
 *           reproject_to_image does not write its output for a point with z <= 0 (perspective, fisheye), and the temporaries are declared
 *           once before the loop (tracking_module.cc:1010-1012), so such an end point carries the value of the most recent earlier
 *           non-skipped slot whose matching end point had z > 0 -- valid or not -- and (0, 0) before the first one (D5 item 5).
 *   out_num_valid[b] = number of valid slots (found_proj_candidate = out_num_valid[b] > 0; increase_num_observable per valid slot).
 * Reprojection only (projection::match_current_and_last_frames, match/projection.cc:254-262; points only): obs_mean_normal == NULL ->
 * valid = in the image, out_reproj / out_x_right as above, no distance or ray test, out_level not written (may be NULL), min / max ignored.
 * The host keeps the skip flags and the writes back to the landmark objects. */
typedef struct plp_observe_args {
    plp_camera_model camera;        /* model, cols, rows, fx, fy, cx, cy, focal_x_baseline are read (reproject_to_image has no distortion) */
    float img_bounds[4];            /* camera::base img_bounds_: min_x, max_x, min_y, max_y (float, camera/base.h:68-82) */
    float ray_cos_thr;              /* points: 0.5 at tracking_module.cc:949 */
    float log_scale_factor;         /* frame::log_scale_factor_ (points) / _log_scale_factor_lsd (lines) */
    int32_t num_levels;             /* frame::num_scale_levels_ (points) / _num_scale_levels_lsd (lines), >= 1 */
    int32_t B, m_cap;               /* B > 0 problems of m_cap >= 0 landmark slots */
    const double* pose;             /* B x 15: rot_cw_ row-major, trans_cw_, cam_center_ (as the frame holds them, frame.cc:745-751) */
    const int32_t* counts;          /* B, or NULL = m_cap everywhere */
    const double* pos_w;            /* B x m_cap x 3 (points: get_pos_in_world) / x 6 (lines: start point, end point) */
    const double* obs_mean_normal;  /* B x m_cap x 3 (points: get_obs_mean_normal), or NULL = reprojection only; ignored for lines */
    const float* min_valid_dist;    /* B x m_cap: the raw members min_valid_dist_ / _min_valid_dist (float) */
    const float* max_valid_dist;    /* B x m_cap: max_valid_dist_ / _max_valid_dist */
    const uint8_t* skip;            /* B x m_cap, or NULL = nothing skipped */
    float* out_reproj;              /* B x m_cap x 2 (lines: start point) */
    float* out_reproj2;             /* lines: B x m_cap x 2 end point; ignored for points */
    float* out_x_right;             /* points: B x m_cap or NULL; ignored for lines (the reference does not store it) */
    int32_t* out_level;             /* B x m_cap */
    uint8_t* out_valid;             /* B x m_cap */
    int32_t* out_num_valid;         /* B or NULL */
} plp_observe_args;
/* Invalid (PLP_ERR_INVALID_ARG, checked before anything is written, m_cap == 0 included): NULL ctx / args; the camera as for
 * plp_post_extract_model_* (unknown model, fx or fy 0, cols or rows <= 0); B <= 0, m_cap < 0, num_levels <= 0; NULL pose, pos_w,
 * out_reproj, out_valid; points with obs_mean_normal but NULL min / max_valid_dist or out_level; lines with NULL min / max_valid_dist,
 * out_reproj2 or out_level.  m_cap == 0: PLP_OK, out_num_valid set to 0, nothing else written.
 * _device: every array a DEVICE pointer, asynchronous on hip_stream (the outputs go to plp_match_device as q_reproj[2], q_x_right,
 * q_level, q_valid without a copy).  _host: HOST pointers, staged to HBM (the outputs too, so that every slot the kernel does not write
 * keeps the caller's value), the same kernel, synchronous. */
plp_status plp_observe_landmarks_device(plp_matcher* ctx, const plp_observe_args* args, void* hip_stream);
plp_status plp_observe_landmarks_host(plp_matcher* ctx, const plp_observe_args* args);
plp_status plp_observe_landmark_lines_device(plp_matcher* ctx, const plp_observe_args* args, void* hip_stream);
plp_status plp_observe_landmark_lines_host(plp_matcher* ctx, const plp_observe_args* args);

/* ------------------------------------------------------------------------------------------------------------------
 * Last-frame queries (the queries of PLP_MATCH_MODE_LAST_FRAME[_LINE]): the loops of projection::match_current_and_last_frames
 * (match/projection.cc:214-358) and match_current_and_last_frames_line (:361-527) in front of their searches, as called from
 * frame_tracker::motion_based_track, for B (current frame, last frame) pairs at once:
 *   direction  trans_lc = rot_lw (-rot_cw^T trans_cw) + trans_lw; assume_forward = trans_lc(2) > true_baseline_, assume_backward =
 *              -trans_lc(2) > true_baseline_, both false for a monocular setup (:219-236, :366-383).  -rot_cw^T trans_cw is read as the
 *              current pose row's cam_center_ (entries 12-14), which frame::update_pose_params forms from the same expression.
 *   points     a slot is valid when not skipped and camera_->reproject_to_image(rot_cw, trans_cw, pos_w) is in the image (:240-262)
 *   lines      both end points reprojected; kept when one is in the image and, if only one is, the midpoint 0.5 (sp + ep) is (:395-440)
 * Numeric contract: DESIGN.md section 5, D5 items 1-2 (the reprojection is the one plp_observe_* computes) and D6 (the end points of a line
 * whose out-of-image end point is behind the camera).
 * Slot j of problem b is key point (key line) j of the last frame, b * m_cap + j; slots j >= counts[b] are neither read nor written.
 * skip[j] != 0 = "!landmarks_[j] || outlier_flags_[j]" (_landmarks_line / _outlier_flags_line for lines): never valid, not reprojected.
 * Outputs per slot j < counts[b], in the layout PLP_MATCH_MODE_LAST_FRAME[_LINE] reads (q_valid, q_reproj[2], q_x_right[2], q_level,
 * q_angle; out_direction -> plp_match_args.directions), so they go to plp_match_device without a copy:
 *   out_valid     1 where the reference goes on to the search, else 0
 *   points: out_reproj / out_x_right = (float) of the f64 reprojection and x_right, out_level = keypts[j].octave, out_angle =
 *           keypts[j].angle (undist_keypts_ keep the octave of keypts_), all written for valid slots only
 *   lines:  out_reproj / out_reproj2 and out_x_right / out_x_right2 = reproj_sp / reproj_ep and x_right_sp / x_right_ep after slot j's
 *           turn, for EVERY slot: the reference declares them inside its loop, so an end point with z <= 0 of a kept line reads
 *           uninitialised values; the library defines them (D6) as the values of the most recent earlier non-skipped slot whose matching
 *           end point had z > 0, (0, 0) / 0 before the first one.  out_level = keylines[j].octave, written for valid slots only.
 *   out_direction[b] = 0 neither, 1 assume_forward, 2 assume_backward (written by both entries, also when m_cap == 0)
 *   out_num_valid[b] = number of valid slots */
typedef struct plp_last_frame_args {
    plp_camera_model camera;        /* model, cols, rows, fx, fy, cx, cy, focal_x_baseline are read (as plp_observe_args) */
    float img_bounds[4];            /* camera::base img_bounds_: min_x, max_x, min_y, max_y */
    int32_t setup_type;             /* camera::setup_type_t of the current frame's camera: 0 monocular, 1 stereo, 2 RGB-D */
    double true_baseline;           /* camera::base true_baseline_ (camera/base.h:144) */
    int32_t B, m_cap;               /* B > 0 problems of m_cap >= 0 slots */
    const int32_t* counts;          /* B: last_frm.num_keypts_ / _num_keylines, or NULL = m_cap everywhere */
    const double* pose_curr;        /* B x 15: the current frame's pose row (plp_observe_args.pose layout) */
    const double* pose_last;        /* B x 15: the last frame's pose row (rot_lw 0-8, trans_lw 9-11 are read) */
    const double* pos_w;            /* B x m_cap x 3 (points: landmarks_[j]->get_pos_in_world) / x 6 (lines: start point, end point) */
    const uint8_t* skip;            /* B x m_cap, or NULL = nothing skipped */
    const plp_keypoint* keypts;     /* points: B x m_cap, the last frame's undist_keypts_ (octave, angle); ignored for lines */
    const plp_keyline* keylines;    /* lines: B x m_cap, the last frame's _keylsd (octave); ignored for points */
    float* out_reproj;              /* B x m_cap x 2 (lines: start point) */
    float* out_reproj2;             /* lines: B x m_cap x 2 end point; ignored for points */
    float* out_x_right;             /* B x m_cap or NULL (lines: start point) */
    float* out_x_right2;            /* lines: B x m_cap or NULL, end point; ignored for points */
    int32_t* out_level;             /* B x m_cap */
    float* out_angle;               /* points: B x m_cap or NULL; ignored for lines */
    uint8_t* out_valid;             /* B x m_cap */
    int32_t* out_direction;         /* B */
    int32_t* out_num_valid;         /* B or NULL */
} plp_last_frame_args;
/* Invalid (PLP_ERR_INVALID_ARG, checked before anything is written, m_cap == 0 included): NULL ctx / args; the camera as for
 * plp_post_extract_model_*; setup_type outside 0..2; B <= 0, m_cap < 0; NULL pose_curr, pose_last, pos_w, out_reproj, out_level, out_valid,
 * out_direction; points with NULL keypts; lines with NULL keylines or out_reproj2.  m_cap == 0: PLP_OK, out_direction written,
 * out_num_valid set to 0, nothing else written.
 * _device: every array a DEVICE pointer, asynchronous on hip_stream.  _host: HOST pointers, staged to HBM (the outputs too, so that every
 * slot the kernel does not write keeps the caller's value), the same kernel, synchronous. */
plp_status plp_project_last_frame_device(plp_matcher* ctx, const plp_last_frame_args* args, void* hip_stream);
plp_status plp_project_last_frame_host(plp_matcher* ctx, const plp_last_frame_args* args);
plp_status plp_project_last_frame_lines_device(plp_matcher* ctx, const plp_last_frame_args* args, void* hip_stream);
plp_status plp_project_last_frame_lines_host(plp_matcher* ctx, const plp_last_frame_args* args);

/* ------------------------------------------------------------------------------------------------------------------
 * Fuse, Sim3 and relocalisation queries (the queries of PLP_MATCH_MODE_FUSE[_LINE] and of the key-frame / Sim3 variants of LAST_FRAME[_LINE]):
 * what seven loops of the reference do per landmark in front of their search, for B (key frame or frame, landmark list) problems at once.
 *   loop                                                               dist_mode  ray_test  line_dist_mode  search (plp_match_args)
 *   fuse::replace_duplication              match/fuse.cc:169-236       CENTER     1         -               FUSE
 *   fuse::replace_duplication_line         match/fuse.cc:335-420       CENTER     0         ENDPOINTS       FUSE_LINE
 *   fuse::detect_duplication               match/fuse.cc:40-111        CENTER     1         -               FUSE, NO_CHI2 | SIGNED_LEVEL
 *   projection::match_by_Sim3_transform    match/projection.cc:781-848 CENTER     1         -               LAST_FRAME, level_window 1, UNSIGNED_LEVEL
 *   projection::match_keyframes_mutually   :894-993 and :1029-1087     CAMERA     0         -               FUSE, NO_CHI2 (one call per pass)
 *   projection::match_frame_and_keyframe   :529-593                    CENTER     0         -               LAST_FRAME, level_window 2
 *   projection::match_frame_and_keyframe_line  :648-743                CENTER     0         MIDPOINT        LAST_FRAME_LINE
 * Per slot, in the reference's order (numeric contract: DESIGN.md section 5, D9):
 *   1  skip[j] != 0 -> SKIPPED.  The tests at the top of each loop read host objects and stay with the caller: !lm, will_be_erased(),
 *      is_observed_in_keyframe, valid_lms_in_keyfrm.count, already_matched.count, is_already_matched_in_keyfrm_1 / _2.
 *   2  camera_->reproject_to_image(R, t, pos_w) with R = pose entries 0-8, t = 9-11 (camera/perspective.cc:190-209, fisheye.cc:231-249,
 *      equirectangular.cc:104-119).  Points: not in the image -> NOT_IN_IMAGE.  Lines: both end points out -> NOT_IN_IMAGE; one out and
 *      the midpoint 0.5 * (sp + ep) out -> MIDPOINT_OUT.
 *   3  the distance range, an f64 comparison with the float results of get_min / max_valid_distance (points 0.7 x / 1.3 x, landmark.cc:297-307;
 *      lines 0.8 x / 1.2 x, landmark_line.cc:354-364) widened to double: dist < min || max < dist -> DISTANCE.
 *      dist: PLP_PROJECT_DIST_CENTER (pos_w - cam_center).norm(), cam_center = pose entries 12-14; PLP_PROJECT_DIST_CAMERA
 *      (R pos_w + t).norm() (pos_2.norm(), projection.cc:976, 1070).  Lines: PLP_PROJECT_LINE_ENDPOINTS tests both end-point distances
 *      (fuse.cc:398-411), PLP_PROJECT_LINE_MIDPOINT the midpoint's (projection.cc:722-730).
 *   4  ray_test: cam_to_lm_vec.dot(obs_mean_normal) < 0.5 * dist -> RAY (fuse.cc:98, 221; projection.cc:835; no division, 0.5 a double)
 *   5  pred_scale_level = predict_scale_level((float)dist, ...) (lines: of the midpoint distance, fuse.cc:414-416) -> KEPT
 * Slot j of problem b is b * m_cap + j; slots j >= counts[b] are neither read nor written.  Outputs per slot j < counts[b], in the layouts
 * plp_match_device reads (q_valid, q_reproj_d, q_reproj2_d, q_reproj, q_reproj2, q_x_right, q_x_right2, q_level), so nothing is copied or
 * compacted between the two calls; the search's own tables (q_desc, q_angle, q_has_obs, t_occupied) stay the caller's:
 *   out_valid     1 where the reference goes on to its search (KEPT), else 0
 *   out_status    a plp_project_status: where the reference leaves the iteration
 *   points: out_reproj_d = the f64 reprojection, out_reproj / out_x_right = its (float) and the (float) x_right, out_level =
 *           pred_scale_level; all written for valid slots only
 *   lines:  out_reproj_d / out_reproj2_d, out_reproj / out_reproj2, out_x_right / out_x_right2 = reproj_sp / reproj_ep and x_right_sp /
 *           x_right_ep after slot j's turn, for EVERY slot: all three line loops declare them inside the loop and reproject_to_image does
 *           not write them for z <= 0, so a kept line with an end point behind the camera reads uninitialised values (fuse.cc:364-367,
 *           418-420; projection.cc:682-688); the library defines them as D6 does: the values of the most recent earlier non-skipped slot
 *           whose matching end point was written, (0, 0) / 0 before the first one.  out_level is written for valid slots only.
 *   out_num_valid[b] = number of valid slots */
typedef enum plp_project_dist_mode { PLP_PROJECT_DIST_CENTER = 0, PLP_PROJECT_DIST_CAMERA = 1 } plp_project_dist_mode;
typedef enum plp_project_line_dist_mode { PLP_PROJECT_LINE_ENDPOINTS = 0, PLP_PROJECT_LINE_MIDPOINT = 1 } plp_project_line_dist_mode;
typedef enum plp_project_status {
    PLP_PROJECT_KEPT = 0, PLP_PROJECT_SKIPPED = 1, PLP_PROJECT_NOT_IN_IMAGE = 2, PLP_PROJECT_MIDPOINT_OUT = 3, PLP_PROJECT_DISTANCE = 4,
    PLP_PROJECT_RAY = 5
} plp_project_status;
typedef struct plp_project_args {
    plp_camera_model camera;        /* model, cols, rows, fx, fy, cx, cy, focal_x_baseline are read (as plp_observe_args) */
    float img_bounds[4];            /* camera::base img_bounds_: min_x, max_x, min_y, max_y */
    float log_scale_factor;         /* log_scale_factor_ of the key frame / frame (points) / _log_scale_factor_lsd (lines) */
    int32_t num_levels;             /* num_scale_levels_ (points) / _num_scale_levels_lsd (lines), >= 1 */
    int32_t B, m_cap;               /* B > 0 problems of m_cap >= 0 landmark slots */
    int32_t shared_landmarks;       /* != 0: pos_w, obs_mean_normal, min / max_valid_dist have m_cap rows in all and every problem reads the
                                       same rows (the forward pass of mapping_module::fuse_landmark_duplication: the current key frame's
                                       landmarks into every target); skip and the outputs stay B x m_cap */
    int32_t dist_mode;              /* a plp_project_dist_mode; lines: PLP_PROJECT_DIST_CENTER */
    int32_t ray_test;               /* points: != 0 needs obs_mean_normal and PLP_PROJECT_DIST_CENTER; lines: 0 */
    int32_t line_dist_mode;         /* lines: a plp_project_line_dist_mode; ignored for points */
    const double* pose;             /* B x 15: the 3 x 3 matrix handed to reproject_to_image row-major (0-8), its translation (9-11), cam_center
                                       (12-14; not read with PLP_PROJECT_DIST_CAMERA).  Formed by the caller with the reference's own lines:
                                       a key frame's rot_cw / trans_cw / cam_center; fuse.cc:46-50 and projection.cc:787-791 for a Sim3;
                                       projection.cc:906-908 with :941-942 and :1035-1036 for the two mutual passes (the matrix is the scaled
                                       s_rot_21w / s_rot_12w); :536-538 for a frame */
    const int32_t* counts;          /* B, or NULL = m_cap everywhere */
    const double* pos_w;            /* B x m_cap x 3 (points) / x 6 (lines: start point, end point); m_cap rows when shared_landmarks */
    const double* obs_mean_normal;  /* points: B x m_cap x 3, or NULL without ray_test; ignored for lines */
    const float* min_valid_dist;    /* B x m_cap: the raw members min_valid_dist_ / _min_valid_dist (float) */
    const float* max_valid_dist;    /* B x m_cap: max_valid_dist_ / _max_valid_dist */
    const uint8_t* skip;            /* B x m_cap, or NULL = nothing skipped */
    double* out_reproj_d;           /* B x m_cap x 2 or NULL (lines: start point): q_reproj_d */
    double* out_reproj2_d;          /* lines: B x m_cap x 2 with out_reproj_d, end point: q_reproj2_d; ignored for points */
    float* out_reproj;              /* B x m_cap x 2 or NULL (lines: start point): q_reproj of the LAST_FRAME modes */
    float* out_reproj2;             /* lines: B x m_cap x 2 with out_reproj, end point; ignored for points */
    float* out_x_right;             /* B x m_cap or NULL (lines: start point) */
    float* out_x_right2;            /* lines: B x m_cap or NULL, end point; ignored for points */
    int32_t* out_level;             /* B x m_cap or NULL */
    uint8_t* out_valid;             /* B x m_cap */
    uint8_t* out_status;            /* B x m_cap or NULL */
    int32_t* out_num_valid;         /* B or NULL */
} plp_project_args;
/* Invalid (PLP_ERR_INVALID_ARG, checked before anything is written, m_cap == 0 included): NULL ctx / args; the camera as for
 * plp_post_extract_model_*; B <= 0, m_cap < 0, num_levels <= 0; NULL pose, pos_w, min_valid_dist, max_valid_dist, out_valid; out_reproj_d and
 * out_reproj both NULL; dist_mode outside 0..1; points: ray_test with NULL obs_mean_normal or with PLP_PROJECT_DIST_CAMERA; lines:
 * line_dist_mode outside 0..1, dist_mode not PLP_PROJECT_DIST_CENTER, ray_test != 0, out_reproj_d without out_reproj2_d or out_reproj without
 * out_reproj2.  B > 65535: PLP_ERR_UNSUPPORTED.  m_cap == 0: PLP_OK, out_num_valid set to 0, nothing else written.  No launch dimension
 * limits m_cap (points: m_cap / 256 workgroups along x; lines: one workgroup per problem walks its slots in chunks of 256).
 * _device: every array a DEVICE pointer, asynchronous on hip_stream.  _host: HOST pointers, staged to HBM (the outputs too, so that every
 * slot the kernel does not write keeps the caller's value), the same kernel, synchronous. */
plp_status plp_project_landmarks_device(plp_matcher* ctx, const plp_project_args* args, void* hip_stream);   /* the five point loops above */
plp_status plp_project_landmarks_host(plp_matcher* ctx, const plp_project_args* args);
/* fuse::replace_duplication_line (match/fuse.cc:335-420) and projection::match_frame_and_keyframe_line (match/projection.cc:648-743) */
plp_status plp_project_landmark_lines_device(plp_matcher* ctx, const plp_project_args* args, void* hip_stream);
plp_status plp_project_landmark_lines_host(plp_matcher* ctx, const plp_project_args* args);

/* ------------------------------------------------------------------------------------------------------------------
 * Stereo key-line association: the filter every stereo data::frame constructor with lines runs on BinaryDescriptorMatcher::match's
 * left -> right result (data/frame.cc:389-427, again at :494-533), for B frames at once.  A match of left key line j is kept when
 *   DMatch.distance < 30 (float; the 1-NN's (-1, 256) is never kept, nor is a train index outside [0, count_right))
 *   sqrt(serr.dot(serr)) < 200 and sqrt(eerr.dot(eerr)) < 200, serr / eerr = getStartPoint() / getEndPoint() differences (startPointX/Y,
 *                    endPointX/Y, not the in-octave fields) as cv::Point2f, the dot x*x + y*y in float
 *   abs((abs(a1) - abs(a2))) * 180 / 3.14 < 5: the float abs, the float product divided in f64 by 3.14 and rounded to float (DESIGN.md
 *                    section 5, D7: the overload GCC's libstdc++ gives the unqualified call)
 * Slot j of problem b is left key line j, b * cap_left + j; slots j >= counts_left[b] are neither read nor written.  Outputs for every
 * slot j < counts_left[b], in the layout plp_post_extract_* and the last-frame line matcher's kl_x_right use:
 *   out_good_match[j]    the right index of a kept match, else -1: _good_matches_stereo as a dense array
 *   out_kl_depths[j][2]  (1.0, 1.0) for a kept match, else (-1, -1): _depths_cooresponding_to_keylines
 *   out_kl_x_right[j][2] the same values: _stereo_x_right_cooresponding_to_keylines
 * An empty right side (cap_right == 0 or counts_right[b] == 0) is valid: every slot -1 / (-1, -1), as the reference leaves them. */
typedef struct plp_stereo_keylines_args {
    int32_t B, cap_left, cap_right;     /* B > 0 frames, cap_left >= 0 left and cap_right >= 0 right key-line slots */
    const plp_keyline* keylines_left;   /* B x cap_left: _keylsd */
    const int32_t* counts_left;         /* B: _num_keylines, or NULL = cap_left everywhere */
    const plp_keyline* keylines_right;  /* B x cap_right: _keylsd_right */
    const int32_t* counts_right;        /* B, or NULL = cap_right everywhere */
    const int32_t* train_idx;           /* B x cap_left: train_idx of plp_lbd_match_1nn_* (left = query, right = train) */
    const int32_t* dist;                /* B x cap_left: its dist */
    int32_t* out_good_match;            /* B x cap_left */
    float* out_kl_depths;               /* B x cap_left x 2 */
    float* out_kl_x_right;              /* B x cap_left x 2 */
} plp_stereo_keylines_args;
/* Invalid (PLP_ERR_INVALID_ARG, checked before anything is written): NULL ctx / args; B <= 0, cap_left < 0, cap_right < 0; NULL out_good_match,
 * out_kl_depths, out_kl_x_right; NULL keylines_left when cap_left > 0; NULL keylines_right, train_idx, dist when cap_left > 0 and
 * cap_right > 0 (with cap_right == 0 they are not read).  cap_left == 0: PLP_OK, nothing written.
 * _device: every array a DEVICE pointer, asynchronous on hip_stream.  _host: HOST pointers, staged to HBM (the outputs too, so that every
 * slot the kernel does not write keeps the caller's value), the same kernel, synchronous. */
plp_status plp_stereo_keylines_device(plp_matcher* ctx, const plp_stereo_keylines_args* args, void* hip_stream);
plp_status plp_stereo_keylines_host(plp_matcher* ctx, const plp_stereo_keylines_args* args);

/* 3-D key lines: frame::triangulate_stereo_for_line(idx) (data/frame.cc:953-1123; keyframe::triangulate_stereo_for_line, keyframe.cc:647-820,
 * is the same code with the key frame's pose) for every key line of B frames, as the initialiser (module/initializer.cc:472-530) and the key
 * frame line triangulator (module/two_view_triangulator_line.cc:202-240) call it:
 *   RGB-D   (setup_type 2): when 0 < depth_sp and 0 < depth_ep (kl_depths, e.g. plp_post_extract_*'s), both end points unprojected,
 *           (x - cx) * depth * fx_inv in f64 rounded to float, fx_inv = 1.0 / fx (perspective.cc:42), then rot_wc * p + cam_center
 *   stereo  (setup_type 1): when good_match[j] >= 0 (plp_stereo_keylines_*'s), the planes of the left line through P1 = K [I | 0] and of its
 *           right partner through P2 = K [I | (-focal_x_baseline, 0, 0)] intersected into a Pluecker line, its end points trimmed against
 *           the left key line, then rot_wc * p + cam_center; kept when both WORLD z > 0 (as the reference checks, :1109)
 * Numeric contract: DESIGN.md section 5, D7 (f64 in the reference's order, every Eigen expression written out left to right; a non-finite
 * intermediate or end point gives the zero vector).  Slot j of problem b is key line j, b * cap + j; slots j >= counts[b] are neither read
 * nor written.  Outputs per slot j < counts[b]:
 *   out_pos_w[j][6]  (sp, ep) in world coordinates, or Vec6_t::Zero() where the reference returns it
 *   out_valid[j]     1 where the line was returned, 0 where the zero vector was */
typedef struct plp_keylines_3d_args {
    plp_camera_model camera;            /* PLP_CAMERA_PERSPECTIVE (frame.cc:957 static_casts to camera::perspective); fx, fy, cx, cy,
                                           focal_x_baseline are read */
    int32_t setup_type;                 /* camera::setup_type_t: 1 stereo, 2 RGB-D (monocular is the reference's assert) */
    int32_t B, cap, cap_right;          /* B > 0 frames of cap >= 0 key-line slots; stereo: cap_right >= 0 right key-line slots */
    const int32_t* counts;              /* B: _num_keylines, or NULL = cap everywhere */
    const double* pose;                 /* B x 15: the plp_observe_args.pose row; rot_wc_ = its rot_cw transposed, cam_center_ = entries 12-14 */
    const plp_keyline* keylines;        /* B x cap: _keylsd */
    const float* kl_depths;             /* RGB-D: B x cap x 2, _depths_cooresponding_to_keylines; ignored for stereo */
    const int32_t* good_match;          /* stereo: B x cap, plp_stereo_keylines_*'s out_good_match; ignored for RGB-D */
    const plp_keyline* keylines_right;  /* stereo: B x cap_right, _keylsd_right */
    const int32_t* counts_right;        /* stereo: B, or NULL = cap_right everywhere (a good_match outside [0, count) gives zero) */
    double* out_pos_w;                  /* B x cap x 6 */
    uint8_t* out_valid;                 /* B x cap, or NULL */
} plp_keylines_3d_args;
/* Invalid (checked before anything is written): NULL ctx / args; the camera as for plp_post_extract_model_* with key lines (equirectangular:
 * PLP_ERR_UNSUPPORTED); fisheye: PLP_ERR_UNSUPPORTED; setup_type not 1 or 2, B <= 0, cap < 0, cap_right < 0; NULL pose, keylines, out_pos_w;
 * RGB-D with NULL kl_depths; stereo with NULL good_match, or NULL keylines_right when cap_right > 0 (PLP_ERR_INVALID_ARG).  cap == 0: PLP_OK,
 * nothing written.  _device / _host as for plp_stereo_keylines_*. */
plp_status plp_keylines_3d_device(plp_matcher* ctx, const plp_keylines_3d_args* args, void* hip_stream);
plp_status plp_keylines_3d_host(plp_matcher* ctx, const plp_keylines_3d_args* args);

/* ------------------------------------------------------------------------------------------------------------------
 * Key-frame pair line triangulation: what follows the 1-NN of plp_lbd_match_1nn_* in mapping_module::triangulate_line_with_two_keyframes
 * (src/PLPSLAM/mapping_module.cc:482-601) and initializer::triangulate_line_with_two_keyframes (module/initializer.cc:585-667).
 * Numeric contract: DESIGN.md section 5, D8; the parallel form of the sequential duplicate check: DESIGN.md section 4.
 *
 * keyframe::compute_median_depth(abs) (data/keyframe.cc:825-857) for F key frames, one workgroup each:
 *   pos_c_z = ((r20 x + r21 y) + r22 z) + (double)(float)t_z   (the reference holds trans_cw_z in a float, :840), std::abs in f64 when
 *   abs_flag, rounded to float (the std::vector<float>); out_median = element (n - 1) / 2 of the ascending order of the n valid slots'
 *   depths (a zero is returned as +0.0), out_count = n.  n == 0, where the reference throws std::out_of_range: out_median 0.0f,
 *   out_count 0.  Finite inputs are a precondition.  Slots j >= counts[f] are not read. */
typedef struct plp_median_depth_args {
    int32_t F, m_cap;               /* F > 0 key frames of 0 <= m_cap <= 8192 landmark slots */
    int32_t abs_flag;               /* the `abs` argument (true at two_view_triangulator_line.cc:246-253) */
    const double* pose;             /* F x 15: the plp_observe_args.pose row (entries 6-8 and 11 are read) */
    const double* pos_w;            /* F x m_cap x 3: landmarks_[j]->get_pos_in_world(), in slot order */
    const uint8_t* valid;           /* F x m_cap: 0 = a nullptr slot; NULL = every slot holds a landmark */
    const int32_t* counts;          /* F: landmarks_.size(), or NULL = m_cap everywhere */
    float* out_median;              /* F */
    int32_t* out_count;             /* F */
} plp_median_depth_args;
/* Invalid (PLP_ERR_INVALID_ARG, checked before anything is written): NULL ctx / args; F <= 0, m_cap < 0; NULL pose, out_median, out_count;
 * NULL pos_w when m_cap > 0.  m_cap > 8192: PLP_ERR_UNSUPPORTED.  m_cap == 0 is valid (every key frame: 0.0f, 0).
 * _device: every array a DEVICE pointer, asynchronous on hip_stream.  _host: HOST pointers, staged (the outputs too), the same kernel,
 * synchronous. */
plp_status plp_median_depth_device(plp_matcher* ctx, const plp_median_depth_args* args, void* hip_stream);
plp_status plp_median_depth_host(plp_matcher* ctx, const plp_median_depth_args* args);

/* The loop over the matches (mapping_module.cc:502-600) with module::two_view_triangulator_line::triangulate
 * (module/two_view_triangulator_line.cc:52-296, .h:128-151), for P pairs of key frames in G groups, over a table of F key frames.
 * A group is one call sequence of the reference: one first key frame (cur = kf1, the query side of the 1-NN) against its neighbours
 * (kf2, the train side) in the order the reference visits them: pairs group_offsets[g] .. group_offsets[g + 1] - 1.  Within a group every
 * pair has the same kf1 and pairwise distinct kf2 != kf1.  Groups are independent: each starts from `occupied` as given.
 * Per pair p and query slot j < counts[kf1], out_status says where the reference leaves the iteration, in its order of evaluation: */
typedef enum plp_keyline_pair_status {
    PLP_KLP_CREATED = 0,          /* triangulate returned true: the reference creates the landmark (out_match, out_pos_w) */
    PLP_KLP_GATE_DISTANCE = 1,    /* no 1-NN, a train index outside kf2, or !(DMatch.distance < dist_thr)                 :506 */
    PLP_KLP_GATE_ENDPOINTS = 2,   /* !(distance_s < endpoint_thr && distance_e < endpoint_thr)                            :529 */
    PLP_KLP_GATE_ANGLE = 3,       /* !(angle < angle_thr)                                                                 :529 */
    PLP_KLP_OCCUPIED_CUR = 4,     /* skip_occupied: cur holds a landmark at the query slot (given, or created with an earlier neighbour) :564 */
    PLP_KLP_OCCUPIED_NGH = 5,     /* skip_occupied: ngh holds one at the train slot (given, or created by an earlier match of the pair)  :564 */
    PLP_KLP_NO_PARALLAX = 6,      /* none of the three ways to the end points applies            two_view_triangulator_line.cc:240-243 */
    PLP_KLP_TOO_CLOSE = 7,        /* an end point nearer than 0.3 median depths                                                :246-250 */
    PLP_KLP_TOO_LONG = 8,         /* longer than 0.9 median depths                                                             :253-256 */
    PLP_KLP_DEPTH = 9,            /* an end point behind one of the two cameras                                                :259-265 */
    PLP_KLP_REPROJ_MID = 10,      /* the midpoint's reprojection error                                                         :269-270 */
    PLP_KLP_REPROJ_END = 11,      /* an end point's distance to the key line                                                   :271-281 */
    PLP_KLP_SCALE = 12,           /* check_scale_factors                                                                       :284-292 */
    PLP_KLP_NON_FINITE = 13,      /* a non-finite end point or reprojection error (undefined in the -ffast-math reference): no landmark */
    PLP_KLP_KP_DEPTH_RANGE = 14   /* depths_.at(idx) with idx >= the number of key points, where the reference throws          :90, :93 */
} plp_keyline_pair_status;
typedef struct plp_keyline_pairs_args {
    plp_camera_model camera;        /* PLP_CAMERA_PERSPECTIVE (two_view_triangulator_line.cc:43 casts); fx, fy, cx, cy are read */
    int32_t setup_type;             /* camera::setup_type_t: 0 monocular, 1 stereo, 2 RGB-D */
    double true_baseline;           /* camera::base true_baseline_ */
    const float* scale_factors;     /* HOST, num_levels: keyframe::scale_factors_, read at keyline.octave (:284-289) */
    const float* level_sigma_sq;    /* HOST, num_levels: keyframe::level_sigma_sq_, read at keyline.octave (:269-278) */
    int32_t num_levels;             /* 1 .. 16; an octave outside [0, num_levels), where the reference's at() throws, is clamped */
    float scale_factor;             /* keyframe::scale_factor_: ratio_factor_ = 2.0f * scale_factor (:40) */
    float rays_parallax_deg_thr;    /* 1.0 at both call sites; cos_rays_parallax_thr_ = (float)cos(thr * M_PI / 180.0) is formed on the host */
    float dist_thr, endpoint_thr, angle_thr;   /* 50 / 400 / 20 (mapping_module.cc:506, :529), 30 / 200 / 5 (initializer.cc) */
    int32_t skip_occupied;          /* 1: "avoid duplicate triangulation" (mapping_module.cc:564); 0: the initialiser's loop, which has no such check */
    int32_t F, cap, kp_cap;         /* the table: F > 0 key frames of 0 <= cap <= 8192 key-line slots and kp_cap >= 0 key-point slots */
    const plp_keyline* keylines;    /* F x cap: _keylsd */
    const int32_t* counts;          /* F: _keylsd.size(), or NULL = cap everywhere */
    const double* line_functions;   /* F x cap x 3: _keyline_functions (the line extractor's third output) */
    const float* kl_x_right;        /* F x cap x 2: _stereo_x_right_cooresponding_to_keylines; .first is read, 0 <= .first = "is stereo" */
    const float* kp_depths;         /* F x kp_cap: the KEY POINTS' depths_, which the reference indexes with a key-line index (D8 item 2) */
    const int32_t* kp_counts;       /* F: depths_.size(), or NULL = kp_cap everywhere */
    const double* pose;             /* F x 15: the plp_observe_args.pose row */
    const float* median_depth;      /* F: compute_median_depth(true), e.g. plp_median_depth_*'s out_median; key frame 2's is the one read */
    const double* lines_3d;         /* F x cap x 6: triangulate_stereo_for_line(idx) of every key line (plp_keylines_3d_*'s out_pos_w, its
                                       zero rows included); may be NULL for a monocular setup, which never reads it */
    const uint8_t* occupied;        /* F x cap: get_landmark_line(idx) != nullptr before the call */
    int32_t P, G;                   /* P >= 0 pairs in G >= 0 groups */
    const int32_t* pairs;           /* P x 2: kf1, kf2 (indices into the table) */
    const int32_t* group_offsets;   /* G + 1, non-decreasing, inside [0, P] */
    const int32_t* train_idx;       /* P x cap: plp_lbd_match_1nn_* with kf1 = query, kf2 = train */
    const int32_t* dist;            /* P x cap: its dist */
    int32_t* out_match;             /* P x cap: the train index of the landmark the reference creates, else -1 */
    double* out_pos_w;              /* P x cap x 6: pos_w_line (sp, ep) where out_match >= 0, zero elsewhere */
    uint8_t* out_status;            /* P x cap: a plp_keyline_pair_status */
    uint8_t* out_occupied_cur;      /* G x cap: cur's slots after the group (`occupied` or a landmark created in the group), slots
                                       j < counts[kf1]; feed it back as `occupied` to chain calls */
} plp_keyline_pairs_args;
/* Slots j >= counts[kf1] of a pair are neither read nor written; a pair outside every group gets its geometry statuses without the
 * duplicate check.  Checked before anything is written: NULL ctx / args, the camera as for plp_post_extract_model_*, setup_type outside
 * 0..2, num_levels outside 1..16, F <= 0, cap < 0, kp_cap < 0, P < 0, G < 0, a NULL scale_factors / level_sigma_sq, and -- when P > 0,
 * G > 0 and cap > 0 -- a NULL keylines, line_functions, kl_x_right, pose, median_depth, occupied, pairs, group_offsets, train_idx, dist or
 * output, a NULL kp_depths with kp_cap > 0, a NULL lines_3d with a stereo or RGB-D setup (PLP_ERR_INVALID_ARG); a camera that is not
 * perspective, cap > 8192 or P > 2^31 / 8192 (PLP_ERR_UNSUPPORTED).  cap == 0, P == 0 or G == 0: PLP_OK, nothing written.
 * _host additionally checks (PLP_ERR_INVALID_ARG) that group_offsets is non-decreasing inside [0, P], that every kf1 / kf2 is inside
 * [0, F), and that the pairs of a group share kf1 and have pairwise distinct kf2 != kf1; on the _device path these are preconditions
 * (an index outside the table is not followed: the pair is left unwritten).
 * _device: every array but scale_factors / level_sigma_sq a DEVICE pointer; two kernels on hip_stream, no host synchronisation.
 * _host: HOST pointers, staged (the outputs too, so that every slot the kernels do not write keeps the caller's value), the same kernels,
 * synchronous. */
plp_status plp_triangulate_keyline_pairs_device(plp_matcher* ctx, const plp_keyline_pairs_args* args, void* hip_stream);
plp_status plp_triangulate_keyline_pairs_host(plp_matcher* ctx, const plp_keyline_pairs_args* args);

/* ------------------------------------------------------------------------------------------------------------------
 * Key-frame pair point triangulation: the point half of mapping_module::create_new_landmarks (src/PLPSLAM/mapping_module.cc:359-479)
 * around PLP_MATCH_MODE_TRIANGULATION.  Numeric contract: DESIGN.md section 5, D10.
 *
 * In front of the matcher, per pair (kf1 = cur, kf2 = ngh) of a table of F key frames:
 *   out_baseline = |cam_center(kf2) - cam_center(kf1)|, sqrt((dx dx + dy dy) + dz dz)                                    :382-383
 *   out_skip     = the `continue` of :386-402: monocular (setup_type 0)  out_baseline < 0.02 * (double)median_depth[kf2],
 *                  stereo / RGB-D  out_baseline < true_baseline
 *   out_epipolar = the 12 doubles of plp_match_args.epipolar: E_12 = create_E_21(rot_2w, trans_2w, rot_1w, trans_1w) row-major
 *                  (solve/essential_solver.cc:188-194, call at :429), then camera::*::reproject_to_bearing(rot_2w, trans_2w, cam_center_1)
 *                  (match/robust.cc:50-55).  robust.cc ignores that function's return value: for perspective and fisheye with z <= 0 the
 *                  vector is the UN-NORMALISED rot_2w cam_center_1 + trans_2w, as the reference leaves it.
 * All three are written for every pair, skipped or not. */
typedef struct plp_keyframe_pair_geometry_args {
    plp_camera_model camera;        /* model is read (the epipole's normalisation) */
    int32_t setup_type;             /* camera::setup_type_t: 0 monocular, 1 stereo, 2 RGB-D */
    double true_baseline;           /* camera::base true_baseline_ (stereo / RGB-D gate) */
    int32_t F, P;                   /* F > 0 key frames, P >= 0 pairs */
    const double* pose;             /* F x 15: the plp_observe_args.pose row */
    const float* median_depth;      /* F: compute_median_depth(true) (plp_median_depth_*'s out_median); read for a monocular setup only */
    const int32_t* pairs;           /* P x 2: kf1, kf2 */
    uint8_t* out_skip;              /* P */
    double* out_epipolar;           /* P x 12 */
    double* out_baseline;           /* P */
} plp_keyframe_pair_geometry_args;
/* Checked before anything is written (PLP_ERR_INVALID_ARG): NULL ctx / args, the camera as for plp_post_extract_model_*, setup_type
 * outside 0..2, F <= 0, P < 0, and -- when P > 0 -- a NULL pose, pairs or output, a NULL median_depth with a monocular setup.  P == 0:
 * PLP_OK, nothing written.  _host additionally checks that every kf1 / kf2 is inside [0, F); on the _device path that is a precondition
 * (a pair outside the table is left unwritten).
 * _device: DEVICE pointers, one kernel on hip_stream, no host synchronisation.  _host: HOST pointers, staged (the outputs too), the same
 * kernel, synchronous. */
plp_status plp_keyframe_pair_geometry_device(plp_matcher* ctx, const plp_keyframe_pair_geometry_args* args, void* hip_stream);
plp_status plp_keyframe_pair_geometry_host(plp_matcher* ctx, const plp_keyframe_pair_geometry_args* args);

/* Behind the matcher: module::two_view_triangulator::triangulate (module/two_view_triangulator.cc:45-122, .h:114-137) for every match of
 * every pair, with solve::triangulator::triangulate (solve/triangulator.h:105-119; the null vector as D10 defines it) and
 * keyframe::triangulate_stereo (data/keyframe.cc:589-640).  Per pair p and key point t < counts[kf2] of key frame 2, out_status says
 * where the reference leaves the iteration, in its order of evaluation: */
typedef enum plp_keypoint_pair_status {
    PLP_KPP_CREATED = 0,        /* triangulate returned true: the reference creates the landmark (out_idx_1, out_pos_w)                 */
    PLP_KPP_PAIR_SKIPPED = 1,   /* pair_skip[p]: the pair never reaches the matcher (mapping_module.cc:386-402)                         */
    PLP_KPP_NO_MATCH = 2,       /* match_q[p][t] is -1 or outside [0, m_cap)                                                            */
    PLP_KPP_NO_PARALLAX = 3,    /* none of the three ways to a position applies                             two_view_triangulator.cc:93-96 */
    PLP_KPP_DEPTH = 4,          /* behind one of the two cameras (never for equirectangular)                                      :99-102 */
    PLP_KPP_REPROJ_1 = 5,       /* check_reprojection_error in key frame 1                                                        :105-106 */
    PLP_KPP_REPROJ_2 = 6,       /* ... in key frame 2                                                                            :107-108 */
    PLP_KPP_SCALE = 7,          /* check_scale_factors                                                                           :114-119 */
    PLP_KPP_NON_FINITE = 8,     /* v[3] == 0, a non-finite position or reprojection error (undefined in the -ffast-math reference): no landmark */
    PLP_KPP_INDEX_RANGE = 9     /* idx_1 outside [0, counts[kf1]), where undist_keypts_.at(idx_1) throws                             :47 */
} plp_keypoint_pair_status;
typedef struct plp_keypoint_pairs_args {
    plp_camera_model camera;        /* all three models for a monocular setup; perspective and fisheye for stereo / RGB-D */
    int32_t setup_type;             /* 0 monocular: x_right and depths are not read (every stereo_x_right_ is -1); 1 stereo, 2 RGB-D */
    double true_baseline;           /* camera::base true_baseline_ (the stereo parallax) */
    const float* scale_factors;     /* HOST, num_levels: keyframe::scale_factors_, read at keypoint.octave */
    const float* level_sigma_sq;    /* HOST, num_levels: keyframe::level_sigma_sq_ */
    int32_t num_levels;             /* 1 .. 16; an octave outside [0, num_levels), where the reference's at() throws, is clamped */
    float scale_factor;             /* keyframe::scale_factor_ of both key frames: ratio_factor_ = 2.0f * scale_factor */
    float rays_parallax_deg_thr;    /* 1.0 (mapping_module.cc:436); cos_rays_parallax_thr_ = (float)cos(thr * M_PI / 180.0) is formed on the host */
    int32_t F, cap, m_cap, P;       /* F > 0 key frames of 0 <= cap <= 8192 key-point slots; m_cap > 0 query slots per pair; P >= 0 pairs */
    const plp_keypoint* keypts;     /* F x cap: undist_keypts_ (pt, octave) */
    const double* bearings;         /* F x cap x 3: bearings_ */
    const float* x_right;           /* F x cap: stereo_x_right_ (stereo / RGB-D) */
    const float* depths;            /* F x cap: depths_ (stereo / RGB-D) */
    const int32_t* counts;          /* F: num_keypts_, or NULL = cap everywhere */
    const double* pose;             /* F x 15: the plp_observe_args.pose row */
    const int32_t* pairs;           /* P x 2: kf1 (cur), kf2 (ngh) */
    const int32_t* match_q;         /* P x cap: plp_match_* out_match of the pair's TRIANGULATION problem (the query slot per key point of
                                       key frame 2, -1 = none); each query slot appears at most once per row */
    const int32_t* q_feature;       /* P x m_cap: the key-point index in key frame 1 of every query slot (the BoW node order of the
                                       matcher's queries); NULL = identity */
    const uint8_t* pair_skip;       /* P or NULL: plp_keyframe_pair_geometry_*'s out_skip */
    int32_t* out_idx_1;             /* P x cap: idx_1 of the match at key point t (also where the triangulation failed), -1 = NO_MATCH */
    double* out_pos_w;              /* P x cap x 3: pos_w where CREATED, zero elsewhere */
    uint8_t* out_status;            /* P x cap: a plp_keypoint_pair_status */
    uint8_t* occupied_1_io;         /* P x cap or NULL, in place: the byte at idx_1 becomes 1 for every CREATED (cur_keyfrm->add_landmark :464) */
    uint8_t* occupied_2_io;         /* P x cap or NULL, in place: the byte at t becomes 1 for every CREATED (ngh_keyfrm->add_landmark :465) */
} plp_keypoint_pairs_args;
/* Slots t >= counts[kf2] are neither read nor written.  A pair with pair_skip[p] != 0 gets PLP_KPP_PAIR_SKIPPED in out_status and nothing
 * else: out_idx_1, out_pos_w and the occupancy keep the caller's values.  Every other slot gets all three outputs; occupied_*_io change
 * only where a landmark is created.
 * Checked before anything is written (PLP_ERR_INVALID_ARG): NULL ctx / args, the camera as for plp_post_extract_model_*, setup_type outside
 * 0..2, num_levels outside 1..16, F <= 0, cap < 0, m_cap <= 0, P < 0, a NULL scale_factors / level_sigma_sq, and -- when P > 0 and cap > 0 --
 * a NULL keypts, bearings, pose, pairs, match_q or output, a NULL x_right or depths with a stereo or RGB-D setup.  A stereo or RGB-D setup
 * with the equirectangular camera, where the reference throws (keyframe.cc:637), cap > 8192 or P x max(cap, m_cap) > 2^31: PLP_ERR_UNSUPPORTED.
 * cap == 0 or P == 0: PLP_OK, nothing written.  _host additionally checks that every kf1 / kf2 is inside [0, F); on the _device path that
 * is a precondition (a pair outside the table is left unwritten).
 * _device: every array but scale_factors / level_sigma_sq a DEVICE pointer; one kernel on hip_stream, no host synchronisation.
 * _host: HOST pointers, staged (the outputs and the occupancy too, so that every slot the kernel does not write keeps the caller's value),
 * the same kernel, synchronous. */
plp_status plp_triangulate_keypoint_pairs_device(plp_matcher* ctx, const plp_keypoint_pairs_args* args, void* hip_stream);
plp_status plp_triangulate_keypoint_pairs_host(plp_matcher* ctx, const plp_keypoint_pairs_args* args);

/* ------------------------------------------------------------------------------------------------------------------
 * Landmark normals and valid distance ranges: landmark::update_normal_and_depth (src/PLPSLAM/data/landmark.cc:249-295) and
 * Line::update_information (data/landmark_line.cc:311-352) for L landmarks at once, over a table of F key frames -- what the reference
 * runs beside compute_descriptor (plp_landmark_descriptor_*) wherever landmark geometry changes: after triangulation, fusion
 * (mapping_module.cc:619-650), every bundle adjustment and a map load.  The outputs are the tables plp_observe_args / plp_project_args
 * read as obs_mean_normal, min_valid_dist and max_valid_dist.  Numeric contract: DESIGN.md section 5, D11.
 *
 * Landmark l owns the observations obs_offsets[l] .. obs_offsets[l + 1] - 1 of obs_kf / obs_idx (key frame, feature index), in the
 * iteration order of the caller's observations_ map; no limit on their number.  Points (landmark.cc):
 *   mean_normal = the left-to-right sum, in list order, of (pos_w - cam_center[obs_kf]).normalized() over EVERY observation (erased key
 *                 frames included, unlike compute_descriptor), then normalized(); normalized() = v / sqrt((x x + y y) + z z), a zero
 *                 vector stays zero                                                                                            :272-281, :293
 *   max         = (float)(|pos_w - cam_center[ref_kf]| * (double)scale_factors[octave]), octave = that of key point obs_idx of the
 *                 observation whose obs_kf == ref_kf (a precondition: at most one; the first is taken)                     :283-286, :291
 *   min         = max / scale_factors[num_levels - 1], float / float                                                               :292
 * Lines (landmark_line.cc), no normal:
 *   distance    = |0.5 * (sp + ep) - cam_center[ref_kf]|                                                                       :336-342
 *   level       = keylines[ref_kf][idx].octave, idx = the reference key frame's observation, or 0 when ref_kf is not among the
 *                 observations (observations[ref_kf] is operator[])                                                                :343
 *   max         = (float)(distance * (double)scale_factors_lsd[level])                                                       :344, :349
 *   min         = max / scale_factors[num_levels_lsd - 1]: the ORB table indexed with the LSD level count, as the reference has it   :350
 * out_status is written for every l < L; the value outputs only where it is PLP_LG_UPDATED (elsewhere they keep the caller's values,
 * as the reference leaves its members).  The status says where the reference leaves the function, in its order of evaluation: skipped,
 * no observations, a key frame outside the table (the loop over the observations and ref_keyfrm->get_cam_center() follow those pointers),
 * the reference key frame not observed, its feature index out of range, its octave out of range. */
typedef enum plp_landmark_geometry_status {
    PLP_LG_UPDATED = 0,           /* the value outputs were written                                                                       */
    PLP_LG_SKIPPED = 1,           /* skip[l]: will_be_erased_, the early return of landmark.cc:257-260 / landmark_line.cc:324-325         */
    PLP_LG_NO_OBSERVATIONS = 2,   /* an empty list                                                    landmark.cc:266-269 / landmark_line.cc:333-334 */
    PLP_LG_REF_NOT_OBSERVED = 3,  /* points only: ref_kf is not among the observations, observations.at(ref_keyfrm) throws (:285)         */
    PLP_LG_INDEX_RANGE = 4,       /* ref_kf or an obs_kf outside [0, F), or the reference key frame's feature index outside
                                     [0, counts[ref_kf]), where undist_keypts_.at() throws                                                 */
    PLP_LG_OCTAVE_RANGE = 5       /* the octave outside [0, num_levels) (lines: [0, num_levels_lsd)), where scale_factors_.at() throws    */
} plp_landmark_geometry_status;
typedef struct plp_landmark_geometry_args {
    int32_t F, cap;                 /* the table: F > 0 key frames of cap >= 0 key-point (lines: key-line) slots */
    const double* pose;             /* F x 15: the plp_observe_args.pose row; only entries 12-14, cam_center_, are read */
    const int32_t* counts;          /* F: num_keypts_ (lines: _keylsd.size()), or NULL = cap everywhere */
    const plp_keypoint* keypts;     /* points: F x cap, undist_keypts_; only octave is read.  Ignored for lines */
    const plp_keyline* keylines;    /* lines: F x cap, _keylsd; only octave is read.  Ignored for points */
    const float* scale_factors;     /* HOST, num_levels: keyframe::scale_factors_ */
    int32_t num_levels;             /* 1 .. 16: num_scale_levels_ */
    const float* scale_factors_lsd; /* lines: HOST, num_levels_lsd: _scale_factors_lsd.  Ignored for points */
    int32_t num_levels_lsd;         /* lines: 1 .. num_levels: _num_scale_levels_lsd.  Ignored for points */
    int32_t L;                      /* L >= 0 landmarks */
    const double* pos_w;            /* points: L x 3, pos_w_; lines: L x 6, _pos_w = (sp, ep) */
    const int32_t* ref_kf;          /* L: ref_keyfrm_ as a row of the table */
    const uint8_t* skip;            /* L, or NULL = none: will_be_erased_ */
    const int32_t* obs_offsets;     /* L + 1, non-decreasing from 0 */
    const int32_t* obs_kf;          /* obs_offsets[L]: the key frame of every observation, a row of the table */
    const int32_t* obs_idx;         /* obs_offsets[L]: its feature index in that key frame */
    double* out_mean_normal;        /* points: L x 3, mean_normal_.  Ignored for lines */
    float* out_min_valid_dist;      /* L: the raw member min_valid_dist_ / _min_valid_dist (not the 0.7 / 0.8 getter) */
    float* out_max_valid_dist;      /* L: max_valid_dist_ / _max_valid_dist (not the 1.3 / 1.2 getter) */
    uint8_t* out_status;            /* L: a plp_landmark_geometry_status */
} plp_landmark_geometry_args;
/* Checked before anything is written (PLP_ERR_INVALID_ARG): NULL ctx / args; F <= 0, cap < 0, L < 0; num_levels outside 1..16 or a NULL
 * scale_factors; lines: num_levels_lsd outside 1..16, above num_levels (the reference would read past scale_factors_) or a NULL
 * scale_factors_lsd; and -- when L > 0 -- a NULL pose, pos_w, ref_kf, obs_offsets, obs_kf, obs_idx, out_min_valid_dist,
 * out_max_valid_dist or out_status, a NULL keypts / out_mean_normal (points) or keylines (lines) -- keypts / keylines may be NULL when
 * cap == 0.  L == 0: PLP_OK, nothing written.  _host additionally checks that obs_offsets starts at 0 and is non-decreasing
 * (PLP_ERR_INVALID_ARG) and ends at most at 2^31 - 257 (PLP_ERR_UNSUPPORTED); on the _device path these are preconditions.
 * _device: every array but the two scale tables a DEVICE pointer; one kernel on hip_stream, no host synchronisation.
 * _host: HOST pointers, staged (the outputs too, so that every slot the kernel does not write keeps the caller's value), the same
 * kernel, synchronous. */
plp_status plp_landmark_geometry_device(plp_matcher* ctx, const plp_landmark_geometry_args* args, void* hip_stream);
plp_status plp_landmark_geometry_host(plp_matcher* ctx, const plp_landmark_geometry_args* args);
plp_status plp_landmark_line_geometry_device(plp_matcher* ctx, const plp_landmark_geometry_args* args, void* hip_stream);
plp_status plp_landmark_line_geometry_host(plp_matcher* ctx, const plp_landmark_geometry_args* args);
/* Host build of the same source (csrc/landmark_geometry.hpp), HOST pointers, one landmark after the other: lines == 0 the point entry,
 * else the line entry.  The same checks as the _host entries (no ctx).  No GPU needed.  Returns L, or -1 for a bad argument. */
int32_t plp_model_landmark_geometry_host(const plp_landmark_geometry_args* args, int32_t lines);

/* Input side: util::convert_to_grayscale (src/PLPSLAM/util/image_converter.cc:33-75, cv::cvtColor
 * RGB/BGR[A] -> gray on CV_8U) and util::convert_to_true_depth (:77-80, convertTo(CV_32F, 1 / depthmap_factor)), so that the
 * raw colour / 16-bit depth frames can go straight to HBM.  B frames, device pointers, asynchronous.
 * channels 3 or 4; color_order 0 = RGB(A), 1 = BGR(A).  src_is_u16 != 0: CV_16UC1 depth, else CV_32FC1. */
plp_status plp_convert_to_grayscale_device(plp_matcher* ctx, const uint8_t* d_src, int32_t rows, int32_t cols, size_t src_step,
                                           size_t src_frame_stride, int32_t channels, int32_t color_order, int32_t B, uint8_t* d_gray,
                                           size_t gray_step, size_t gray_frame_stride, void* hip_stream);
plp_status plp_convert_to_true_depth_device(plp_matcher* ctx, const void* d_src, int32_t src_is_u16, int32_t rows, int32_t cols, size_t src_step,
                                            size_t src_frame_stride, double depthmap_factor, int32_t B, float* d_dst, size_t dst_step,
                                            size_t dst_frame_stride, void* hip_stream);

/* util::stereo_rectifier (src/PLPSLAM/util/stereo_rectifier.cc:38-85), perspective model.
 * plp_rectify_map_device = the constructor's cv::initUndistortRectifyMap(K, D, R, K_rect, img_size, CV_32F, map_x, map_y)
 * for one eye (:61-62): K, R row-major 3x3 doubles and D (n_dist in {0, 4, 5, 8, 12}: k1 k2 p1 p2 [k3 [k4 k5 k6 [s1..s4]]])
 * as read from the yaml; rect_cam = the rectified camera, whose fx, fy, cx, cy are rounded to float like
 * camera::perspective::cv_cam_matrix_ (perspective.cc:47).  Writes rows x cols CV_32F maps (map_step bytes per row).
 * plp_remap_linear_device = rectify()'s cv::remap(in, out, map_x, map_y, cv::INTER_LINEAR) (:83-84) on B 8UC1 frames that
 * share one map pair: 1/32-pixel fixed point, 15-bit weights, constant border 0.  Device pointers, asynchronous. */
plp_status plp_rectify_map_device(plp_matcher* ctx, const double* K, const double* D, int32_t n_dist, const double* R,
                                  const plp_camera* rect_cam, int32_t rows, int32_t cols, float* d_map_x, float* d_map_y, size_t map_step,
                                  void* hip_stream);
/* The "fisheye" StereoRectifier.model (util/stereo_rectifier.cc:65-70, the TUM-VI yaml): cv::fisheye::initUndistortRectifyMap,
 * equidistant model with 4 coefficients.  Not bit-defined like the perspective map: OpenCV inverts K_rect * R by SVD (here
 * closed form) and the map goes through atan(); the tests hold it to 1e-4 px against the oracle.  The remap is the same. */
plp_status plp_rectify_map_fisheye_device(plp_matcher* ctx, const double* K, const double* D4, const double* R, const plp_camera* rect_cam,
                                          int32_t rows, int32_t cols, float* d_map_x, float* d_map_y, size_t map_step, void* hip_stream);
plp_status plp_remap_linear_device(plp_matcher* ctx, const uint8_t* d_src, int32_t rows, int32_t cols, size_t src_step, size_t src_frame_stride,
                                   const float* d_map_x, const float* d_map_y, size_t map_step, int32_t dst_rows, int32_t dst_cols, int32_t B,
                                   uint8_t* d_dst, size_t dst_step, size_t dst_frame_stride, void* hip_stream);

/* Planar_Mapping_module::create_ColorToPlane (src/PLPSLAM/planar_mapping_module.cc:185-345), the per-key-point part
 * (BASELINE config 5): labels[b][i] = colour label c0 + (c1 << 8) + (c2 << 16) of the CV_8UC3
 * instance mask under undistorted key point i, or 0 when the point is flagged invalid (valid == NULL: all valid), outside
 * the mask, on label 0, or (check_3x3_window) not surrounded by its own label.  The `> 0` neighbour tests of the
 * reference are kept (row 0 / column 0 are never looked at).  New data::Plane objects and add_landmark stay on the host.
 * Device pointers, asynchronous. */
plp_status plp_color_vote_device(plp_matcher* ctx, const uint8_t* d_mask, int32_t rows, int32_t cols, size_t mask_step,
                                 size_t mask_frame_stride, const plp_keypoint* d_undist, const uint8_t* d_valid, const int32_t* d_counts,
                                 int32_t cap, int32_t B, int32_t check_3x3_window, int32_t* d_labels, void* hip_stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Plane fitting: Planar_Mapping_module's RANSAC (src/PLPSLAM/planar_mapping_module.cc) for P planes at once.  `mode` selects
 *   PLP_PLANE_CREATE  estimate_plane_sequential_RANSAC (:412-591) with the gate in front of it in create_new_plane (:359)
 *   PLP_PLANE_UPDATE  update_plane_via_RANSAC (:593-733)
 * estimate_plane_sequential_Graph_cut_RANSAC (:1006-) needs a third-party library and is not offered.
 * Numeric contract: DESIGN.md section 5, D19 (slot order, the samples, estimate_plane_SVD as a written-down algorithm, the shape of
 * every sum), reformulation: DESIGN.md section 4.
 *
 * A plane's landmarks are given in slot form, [P][n_cap]; a slot is one entry of plane->get_landmarks() (`lms`), counts[p] = lms.size():
 *   pos_w   get_pos_in_world()
 *   flags   bit 0 (PLP_PLANE_LM_ERASED) will_be_erased(), bit 1 (PLP_PLANE_LM_OWNED) get_Owning_Plane() != nullptr; these read objects:
 *           the caller computes the byte
 * A slot is eligible for a sample when it is not erased (CREATE, :452) or not erased and owned (UPDATE, :623-628); a sample index is a
 * RANK among the eligible slots in slot order.  A hypothesis has m samples, with replacement: points_per_ransac (CREATE) or the smallest
 * m with !((double)m < (double)counts[p] * 0.8) (UPDATE, :620).  samples == NULL: rank k of iteration i is drawn from `seed` (D19 item 2;
 * plp_model_plane_draw_host).  A caller's rank outside [0, n_eligible) makes the hypothesis's residual DBL_MAX and its equation 0, and
 * its refit is not tried.
 * Every iteration computes [1] the fit of its samples, [2] the non-erased slots closer to it than dist_thresh[p], [3] -- when the gate
 * holds (CREATE: inlier_ratio > inliers_ratio_thr && inliers >= points_per_ransac, inlier_ratio = double(inliers) / double(counts[p]);
 * UPDATE: inliers >= points_per_ransac) -- the fit of those inliers and its error.  The loop over them is the reference's, literally:
 * best_error = min(best_error, residual) BEFORE `error < best_error` is tested; the plane gets every iteration's sample fit
 * unconditionally and its refit when accepted; CREATE breaks on error < error_thresh[p], UPDATE never.  So the plane ends with the
 * equation of the LAST iteration that ran, and step [4] keeps the slots of best_inliers_list that are closer than dist_thresh[p] to THAT.
 * Outputs per problem (the plane's state as the function leaves it):
 *   out_status       a plp_plane_status
 *   out_flags        PLP_PLANE_FLAG_INVALID: set_invalid() was called (:604, :724); PLP_PLANE_FLAG_NEED_REFINEMENT: set_need_refinement()
 *                    (:700); PLP_PLANE_FLAG_GATED: create_new_plane dropped the plane at :359
 *   out_equation[4] / out_best_error   get_equation() / get_best_error().  Where the function returns before its loop (TOO_FEW_POINTS,
 *                    NO_ELIGIBLE) they are equation_in / best_error_in (UPDATE) or keep the caller's values (CREATE)
 *   out_best_iter    the iteration whose inlier list is best_inliers_list, -1 when !best_found;  out_last_iter  the last that ran (-1: none)
 *   out_num_inliers / out_inliers [P][n_cap]   step [4]: plane_best_inlier_map_points.size() and its membership byte per slot, where step
 *                    [4] ran (OK, TOO_FEW_LEFT), else 0; slots at or above counts[p] keep the caller's values
 *   out_hyp_residual / out_hyp_inliers / out_hyp_error   optional, [P][iters]: every hypothesis's residual, inliers_list.size() and refit
 *                    error (DBL_MAX where the refit was not tried), whether or not the loop reached it; 0 / 0 / DBL_MAX where the function
 *                    returned before its loop */
typedef enum plp_plane_mode { PLP_PLANE_CREATE = 0, PLP_PLANE_UPDATE = 1 } plp_plane_mode;
typedef enum plp_plane_status {
    PLP_PLANE_OK = 0,
    PLP_PLANE_TOO_FEW_POINTS = 1,         /* :359 (with PLP_PLANE_FLAG_GATED), :423-436, :597-606 */
    PLP_PLANE_NO_ELIGIBLE = 2,            /* no slot may be sampled: the reference's while loop (:449, :620) would not end */
    PLP_PLANE_NOT_FOUND = 3,              /* !best_found                                                       :545, :698 */
    PLP_PLANE_ERROR_ABOVE_THRESHOLD = 4,  /* best_error > _final_error_thresh                                  :554, :698 */
    PLP_PLANE_TOO_FEW_LEFT = 5            /* UPDATE: step [4] kept fewer than points_per_ransac                       :722 */
} plp_plane_status;
enum { PLP_PLANE_LM_ERASED = 1, PLP_PLANE_LM_OWNED = 2 };
enum { PLP_PLANE_FLAG_INVALID = 1, PLP_PLANE_FLAG_NEED_REFINEMENT = 2, PLP_PLANE_FLAG_GATED = 4 };
typedef struct plp_plane_ransac_args {
    int32_t mode;                      /* a plp_plane_mode */
    int32_t P, n_cap;                  /* P >= 0 planes of n_cap >= 0 slots, n_cap <= 8192, P <= 65535 */
    int32_t points_per_ransac;         /* POINTS_PER_RANSAC, >= 1 */
    int32_t min_points_before_ransac;  /* MIN_NUMBER_POINTS_BEFORE_RANSAC (:359), >= 0; CREATE */
    int32_t iters;                     /* _iterationsCount, 1 .. 1024 */
    double inliers_ratio_thr;          /* _inliers_ratio_thr (:498); CREATE */
    uint64_t seed;                     /* samples == NULL: the generator's seed */
    int32_t m_cap;                     /* samples != NULL: ranks per hypothesis in `samples`; at least the largest m a problem can have:
                                          points_per_ransac (CREATE), the m of n_cap (UPDATE) */
    const int32_t* counts;             /* P: lms.size(), or NULL = n_cap everywhere */
    const double* pos_w;               /* P x n_cap x 3 */
    const uint8_t* flags;              /* P x n_cap: PLP_PLANE_LM_* */
    const double* dist_thresh;         /* P: _planar_distance_thresh */
    const double* error_thresh;        /* P: _final_error_thresh */
    const double* best_error_in;       /* P: plane->get_best_error() before the call (:609); UPDATE */
    const double* equation_in;         /* P x 4: the plane's equation before the call; UPDATE */
    const int32_t* samples;            /* P x iters x m_cap ranks, or NULL = drawn from seed */
    uint8_t* out_status;               /* P */
    uint8_t* out_flags;                /* P */
    double* out_equation;              /* P x 4 */
    double* out_best_error;            /* P */
    int32_t* out_best_iter;            /* P */
    int32_t* out_last_iter;            /* P */
    int32_t* out_num_inliers;          /* P */
    uint8_t* out_inliers;              /* P x n_cap */
    double* out_hyp_residual;          /* P x iters, or NULL */
    int32_t* out_hyp_inliers;          /* P x iters, or NULL */
    double* out_hyp_error;             /* P x iters, or NULL */
} plp_plane_ransac_args;
/* Checked before anything is written (PLP_ERR_INVALID_ARG): NULL ctx / args; an unknown mode; P < 0, n_cap < 0, iters < 1,
 * points_per_ransac < 1, min_points_before_ransac < 0; samples != NULL with m_cap below the largest m; and -- when P > 0 and n_cap > 0 -- a
 * NULL pos_w, flags, dist_thresh, error_thresh, (UPDATE) best_error_in, equation_in, or a NULL required output (out_status .. out_inliers).
 * n_cap > 8192, P > 65535 or iters > 1024: PLP_ERR_UNSUPPORTED.  P == 0 or n_cap == 0: PLP_OK, nothing written.
 * _device: every array a DEVICE pointer (the thresholds too: one derived from plp_median_depth_device needs no host round trip); two
 * kernels on hip_stream, no host synchronisation; bad samples are never an error.  The kernels hand the hypotheses to one another through
 * a buffer the context owns (12 doubles per hypothesis), so the calls of one context must be ordered on the device: one stream, or events
 * between streams.  _host: HOST pointers, staged (the outputs too, so that every slot the kernels do not write keeps the caller's value),
 * the same kernels, synchronous. */
plp_status plp_plane_ransac_device(plp_matcher* ctx, const plp_plane_ransac_args* args, void* hip_stream);
plp_status plp_plane_ransac_host(plp_matcher* ctx, const plp_plane_ransac_args* args);
/* Host builds of the same source (csrc/plane_fit.hpp), HOST pointers, no GPU and no context needed.
 * plp_model_plane_ransac_host: the entry above, one problem, one hypothesis and one partial sum after the other; the same checks.
 * Returns P, or -1 for a bad argument (plp_last_error() names it).
 * plp_model_plane_fit_host: estimate_plane_SVD (:735-771, D19 item 3) for n index lists into one point table pos_w (n_points x 3): list l
 * is indices[offsets[l] .. offsets[l+1]).  out_equation n x 4, out_residual n, out_sweeps n (may be NULL: the Jacobi sweeps that rotated).
 * An empty list or an index outside [0, n_points) gives equation 0 and residual DBL_MAX.  Returns n, or -1.
 * plp_model_plane_draw_host: the ranks the entries draw for problem p, iterations iter0 .. iter0 + n_iters - 1, m per iteration, among
 * n_eligible >= 1 eligible slots: out n_iters x m.  Returns n_iters, or -1. */
int32_t plp_model_plane_ransac_host(const plp_plane_ransac_args* args);
int32_t plp_model_plane_fit_host(const double* pos_w, int32_t n_points, const int32_t* indices, const int32_t* offsets, int32_t n,
                                 double* out_equation, double* out_residual, int32_t* out_sweeps);
int32_t plp_model_plane_draw_host(uint64_t seed, int32_t p, int32_t iter0, int32_t n_iters, int32_t m, int32_t n_eligible, int32_t* out);

/* Planar_Mapping_module::refine_points (:954-1004) over a landmark list: landmark i of plane row lm_plane[i] (-1: none) is skipped when
 * the plane is not active (active[pl] == 0: !is_valid() || need_refinement() || get_num_landmarks() < POINTS_PER_RANSAC, :960-962; the
 * caller computes the byte), when it is erased or not owned (flags as above, :970); else dist_old = calculate_distance(pos_w) -- already
 * a fabs -- and, when it is > 0, pos_w - normalized(n) * dist_old replaces pos_w if its distance is < dist_thresh[0] and < dist_old
 * (:977-989; a point on the negative side moves away and is rejected).  Operation order: D19.  out_changed[i] = 1 where pos_w[i] was
 * written, else 0 (every i < M is written).  M == 0: PLP_OK, nothing written.  PLP_ERR_INVALID_ARG: NULL ctx / args, M < 0, NP < 0, or
 * -- when M > 0 -- a NULL pos_w, lm_plane, flags, dist_thresh, out_changed, or (NP > 0) equation, active.
 * _device: DEVICE pointers, one kernel, asynchronous; _host: HOST pointers, staged, synchronous; plp_model_*: the host build. */
typedef struct plp_plane_refine_args {
    int32_t M, NP;
    double* pos_w;                     /* M x 3, updated in place */
    const int32_t* lm_plane;           /* M */
    const uint8_t* flags;              /* M: PLP_PLANE_LM_* */
    const double* equation;            /* NP x 4 */
    const uint8_t* active;             /* NP */
    const double* dist_thresh;         /* 1: _planar_distance_thresh */
    uint8_t* out_changed;              /* M */
} plp_plane_refine_args;
plp_status plp_plane_refine_points_device(plp_matcher* ctx, const plp_plane_refine_args* args, void* hip_stream);
plp_status plp_plane_refine_points_host(plp_matcher* ctx, const plp_plane_refine_args* args);
int32_t plp_model_plane_refine_points_host(const plp_plane_refine_args* args);

/* ------------------------------------------------------------------------------------------------------------------
 * Plane refinement: Planar_Mapping_module::refinement() (planar_mapping_module.cc:773-793) -- merge_planes (:795-898), refine_planes
 * (:900-952), refine_points (:954-1004) -- for G independent map snapshots over plane and landmark tables that are updated IN PLACE.
 * Numeric contract: DESIGN.md section 5, D26; reformulation: DESIGN.md section 4.  The reference's text is followed literally, quirks
 * included; defined here is only what it leaves to the order of an unordered_map or to std::random_device.
 *
 * Problem g is one map; every array is problem-major.
 * Planes, NP_cap rows per problem; a row is a data::Plane that is or was in _landmarks_plane:
 *   pl_state      PLP_PLANE_ROW_IN_DB | PLP_PLANE_ROW_VALID (is_valid()) | PLP_PLANE_ROW_NEED_REFINEMENT (need_refinement()).
 *                 get_all_landmark_planes() is BY DEFINITION the rows with IN_DB in ascending row; the loops of merge_planes index that
 *                 compacted vector
 *   pl_equation / pl_best_error   get_equation() / get_best_error(); _abs_n is sqrt((a a + b b) + c c) as set_equation stores it
 *   pl_count / pl_lm              Plane::_landmarks as landmark rows: get_landmarks() is slots 0 .. pl_count - 1 in slot order (D19 item 1);
 *                 a count is clamped to [0, n_cap]; a slot at or above the count is no entry: it holds the caller's value, or -- below the
 *                 largest count the row had during the call -- an entry the list held then.  A list names a landmark at most
 *                 once (it is a map keyed by id_); an entry outside [0, L) counts as will_be_erased() without an owner and is never written to
 * Landmarks, L rows per problem: pos_w (written by refine_points only), lm_erased (will_be_erased()), lm_owner (the row of
 * get_Owning_Plane(), -1 = none).  Membership (pl_lm) and ownership (lm_owner) are two relations, as in the reference: Plane::merge
 * (data/landmark_plane.cc:221-248) leaves other->_landmarks as it was, remove_landmarks_ownership() (:197-207) clears the owner of every
 * MEMBER whoever owns it, so a landmark can stand in two lists and an erased plane can still be named as owner.
 *
 * stages: PLP_PLANE_STAGE_MERGE | PLP_PLANE_STAGE_REFINE_PLANES | PLP_PLANE_STAGE_REFINE_POINTS; 7 is refinement() with its gate (:777:
 * fewer than two IN_DB rows: PLP_PLANE_REFINEMENT_TOO_FEW_PLANES, no table touched); a single bit is that function alone with its own
 * early returns (:799-808).
 * merge_planes: the double loop as written -- the candidate skip steps over ONE invalid j and tests the next j whatever its validity,
 * breaking when it runs off the end (:828-835); the parent's validity is tested once per i (:820), so a parent the else arm invalidates
 * (:873-881) goes on; the two-sided test, mixed outcomes neither continue nor merge (:853-860); `>` between the sizes (:864); Plane::merge
 * appends other's non-erased entries that the parent does not hold in other's slot order and owns every non-erased entry of other;
 * update_plane_via_RANSAC on the grown plane at once, set_need_refinement() whatever it returned (:870-871, :879-880); the rows on
 * planes_will_be_removed lose IN_DB after the loop (:889-895) and nothing else.  offset_delta = d_i * (1 / abs_i) - d_j * (1 / abs_j),
 * dot = ((n_i0 n_j0 + n_i1 n_j1) + n_i2 n_j2) * ((1 / abs_i) * (1 / abs_j)), OFFSET_DELTA_THRESHOLD = (double)offset_delta_factor *
 * dist_thresh[g] (:813), IEEE operations in that order.
 * update_plane_via_RANSAC (:593-733) is PLP_PLANE_UPDATE above, unchanged, on the row's current list: the flag byte of a slot is ERASED
 * from lm_erased and OWNED from lm_owner >= 0 at the time of the call; equation and best error as out_equation / out_best_error there;
 * PLP_PLANE_FLAG_INVALID clears VALID, PLP_PLANE_FLAG_NEED_REFINEMENT sets NEED_REFINEMENT; on PLP_PLANE_OK (:728-730) every old member's
 * owner becomes -1, the list becomes step [4]'s members in slot order and their owner the row.  The c-th update call of problem g (counted
 * from 0 in the reference's order, through the merge and then refine_planes) draws ransac_draw_one(seed + g, c, iter, k, n_eligible): it is
 * plp_model_plane_ransac_host with seed + g and samples drawn for problem c (plp_model_plane_draw_host(seed + g, c, ...)).
 * refine_planes over the IN_DB rows after the merge's removals, ascending: an invalid row goes to the erase list (:907-911); a row that
 * needs refinement is updated and on true loses NEED_REFINEMENT (:913-922); else a row of fewer than 2 * points_per_ransac members goes
 * to the erase list (:926-929); after the loop every member of a listed row loses its owner and the row IN_DB (:934-941).
 * refine_points over the IN_DB rows, ascending: rows that are invalid, need refinement or hold fewer than points_per_ransac members are
 * skipped (:960-965); every member that is not erased and has an owner -- any owner -- (:970) is moved as plp_plane_refine_points_* moves
 * it, with THIS row's equation.  A landmark in two active lists is moved twice, the second time from the first result.
 * Outputs per problem:
 *   out_status        a plp_plane_refinement_status.  OVERFLOW: a merge would take a list above n_cap; the problem stops there, its tables
 *                     are undefined, the caller restores its copy and grows n_cap (the convention of plp_covisibility_update_*)
 *   out_was_merged / out_planes_changed / out_points_changed   the return values of the three functions
 *   out_removed       [G][NP_cap]: bit 0 erased at :893, bit 1 erased at :939
 *   out_num_merges / out_merges [G][merge_cap][2]   (parent row, other row) in order; merges beyond merge_cap are counted, not listed, and
 *                     pairs at or above the number of merges keep the caller's values
 *   out_num_updates / out_update_status [G][NP_cap]   the calls of update_plane_via_RANSAC; the plp_plane_status of the row's last one in
 *                     this call, 255 = none
 *   out_lm_changed    [G][L]: 1 where refine_points wrote pos_w */
typedef enum plp_plane_refinement_status {
    PLP_PLANE_REFINEMENT_OK = 0,
    PLP_PLANE_REFINEMENT_TOO_FEW_PLANES = 1,   /* :777 */
    PLP_PLANE_REFINEMENT_OVERFLOW = 2          /* Plane::merge (landmark_plane.cc:235-242) past n_cap */
} plp_plane_refinement_status;
enum { PLP_PLANE_ROW_IN_DB = 1, PLP_PLANE_ROW_VALID = 2, PLP_PLANE_ROW_NEED_REFINEMENT = 4 };
enum { PLP_PLANE_STAGE_MERGE = 1, PLP_PLANE_STAGE_REFINE_PLANES = 2, PLP_PLANE_STAGE_REFINE_POINTS = 4 };
typedef struct plp_plane_refinement_args {
    int32_t G, NP_cap, n_cap, L;       /* G <= 65535 maps of NP_cap <= 4096 plane rows of n_cap <= 8192 slots and L landmarks */
    int32_t merge_cap;                 /* pairs per problem in out_merges, >= 0 */
    int32_t stages;                    /* PLP_PLANE_STAGE_*; 7: refinement() (:773-793) */
    int32_t points_per_ransac;         /* POINTS_PER_RANSAC, >= 1 (:602, :926, :962) */
    int32_t iters;                     /* _iterationsCount, 1 .. 1024 (:616) */
    int32_t offset_delta_factor;       /* _offset_delta_factor, an int in load_configuration (:813) */
    double dot_product_threshold;      /* DOT_PRODUCT_THRESHOLD (:854, :860) */
    uint64_t seed;                     /* problem g draws from seed + g */
    uint8_t* pl_state;                 /* G x NP_cap: PLP_PLANE_ROW_*, in/out (:820, :828, :889-895, :907-941) */
    double* pl_equation;               /* G x NP_cap x 4, in/out (:838-847, :649, :682) */
    double* pl_best_error;             /* G x NP_cap, in/out (:609, :650, :683) */
    int32_t* pl_count;                 /* G x NP_cap, in/out: get_num_landmarks() (:864, :926, :962) */
    int32_t* pl_lm;                    /* G x NP_cap x n_cap, in/out: get_landmarks() (:595, :967) */
    double* pos_w;                     /* G x L x 3, in/out (:975, :988) */
    const uint8_t* lm_erased;          /* G x L: will_be_erased() (:628, :656, :970) */
    int32_t* lm_owner;                 /* G x L, in/out: get_Owning_Plane() as a row, -1 = nullptr (:623, :970) */
    const double* dist_thresh;         /* G: _planar_distance_thresh (:663, :813, :985) */
    const double* error_thresh;        /* G: _final_error_thresh (:698) */
    uint8_t* out_status;               /* G */
    uint8_t* out_was_merged;           /* G (:897) */
    uint8_t* out_planes_changed;       /* G (:951) */
    uint8_t* out_points_changed;       /* G (:1003) */
    uint8_t* out_removed;              /* G x NP_cap (:893, :939) */
    int32_t* out_num_merges;           /* G */
    int32_t* out_merges;               /* G x merge_cap x 2 (:866-867, :875-876), or NULL when merge_cap == 0 */
    int32_t* out_num_updates;          /* G */
    uint8_t* out_update_status;        /* G x NP_cap (:870, :879, :917) */
    uint8_t* out_lm_changed;           /* G x L (:988) */
} plp_plane_refinement_args;
/* Checked before anything is written (PLP_ERR_INVALID_ARG): NULL ctx / args; G, NP_cap, n_cap, L or merge_cap < 0; points_per_ransac < 1;
 * iters < 1; stages outside 1 .. 7; and -- when G > 0 -- a NULL dist_thresh, error_thresh or G-sized output, (NP_cap > 0) a NULL plane table,
 * out_removed or out_update_status, (NP_cap > 0 and n_cap > 0) a NULL pl_lm, (L > 0) a NULL landmark table or out_lm_changed, (merge_cap > 0)
 * a NULL out_merges.  n_cap > 8192, iters > 1024, NP_cap > 4096 or G > 65535: PLP_ERR_UNSUPPORTED.  G == 0: PLP_OK, nothing written.
 * _device: every array a DEVICE pointer; one kernel on hip_stream, one workgroup per problem, no host synchronisation.  The kernel keeps the
 * hypotheses of an update and the marks of a merge in buffers the context owns, so the calls of one context must be ordered on the device:
 * one stream, or events between streams.  _host: HOST pointers, staged (tables and outputs, so that every slot the kernel does not write
 * keeps the caller's value), the same kernel, synchronous.  plp_model_plane_refinement_host: the host build of csrc/plane_refinement.hpp,
 * HOST pointers, no GPU and no context; returns G, or -1 for a refused argument (plp_last_error() names it). */
plp_status plp_plane_refinement_device(plp_matcher* ctx, const plp_plane_refinement_args* args, void* hip_stream);
plp_status plp_plane_refinement_host(plp_matcher* ctx, const plp_plane_refinement_args* args);
int32_t plp_model_plane_refinement_host(const plp_plane_refinement_args* args);

/* Bag-of-words transform: data::frame::compute_bow / data::keyframe::compute_bow
 * (src/PLPSLAM/data/frame.cc:785-795) = bow_vocab_->transform(to_desc_vec(descriptors_), bow_vec_, bow_feat_vec_, 4) of
 * DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB> (data/bow_vocabulary.h:22; the USE_DBOW2 build).  DBoW2 and the
 * vocabulary file are not part of the reference tree, so the tree is handed over flat (the host walks m_nodes once after
 * loadFromBinaryFile): node 0 is the root, children of node i are children[child_offset[i] .. child_offset[i+1]) in
 * the order of Node::children (ties go to the first), leaves carry word_id and weight.
 *   accumulate: 1 for TF / TF_IDF weighting (a word's weight is added once per feature), 0 for IDF / BINARY;
 *   norm: what ScoringObject::mustNormalize asks for: 0 none (DOT_PRODUCT), 1 L1 (L1_NORM, CHI_SQUARE, KL, BHATTACHARYYA), 2 L2.
 * Outputs per frame b (arrays [B][cap]):
 *   word_id / node_id  per feature (may be NULL): the word, and the node at level L - levelsup that FeatureVector files
 *                      the feature under; 0xFFFFFFFF for a stopped word (weight <= 0), which enters neither map.  node_id
 *                      is what PLP_MATCH_MODE_BOW takes as q_group / t_group.
 *   bow_word / bow_value / n_bow   the BowVector (std::map<WordId, WordValue>) in key order, normalised;
 *   fv_node / fv_feat / n_fv       the FeatureVector (std::map<NodeId, std::vector<unsigned>>) flattened in key order,
 *                                  the features of a node in increasing index.
 * Limits: cap <= 8192 (4096 until round 6: the per-frame maps are sorted in LDS, 16 bytes per descriptor).  One transform in flight per vocabulary handle.  Device pointers, asynchronous. */
typedef struct plp_bow_vocab plp_bow_vocab;
typedef struct plp_bow_tree {
    int32_t n_nodes;               /* >= 2 */
    int32_t L;                     /* depth levels (m_L), 6 for the ORB vocabulary */
    const int32_t* child_offset;   /* n_nodes + 1 */
    const int32_t* children;       /* n_nodes - 1 */
    const uint8_t* node_desc;      /* n_nodes x 32 (row 0, the root, is not read) */
    const double* node_weight;     /* n_nodes (read at leaves) */
    const uint32_t* node_word;     /* n_nodes (read at leaves) */
    int32_t accumulate;
    int32_t norm;
} plp_bow_tree;
plp_status plp_bow_vocab_create(int device, const plp_bow_tree* tree, plp_bow_vocab** out);   /* host pointers, copied */
void plp_bow_vocab_destroy(plp_bow_vocab* vocab);
plp_status plp_bow_transform_device(plp_bow_vocab* vocab, const uint8_t* d_desc, const int32_t* d_counts, int32_t cap, int32_t B, int32_t levelsup,
                                    uint32_t* d_word_id, uint32_t* d_node_id, uint32_t* d_bow_word, double* d_bow_value, int32_t* d_n_bow,
                                    uint32_t* d_fv_node, uint32_t* d_fv_feat, int32_t* d_n_fv, void* hip_stream);
/* One frame, host pointers, synchronous; the output arrays hold n entries. */
plp_status plp_bow_transform_host(plp_bow_vocab* vocab, const uint8_t* desc, int32_t n, int32_t levelsup, uint32_t* word_id, uint32_t* node_id,
                                  uint32_t* bow_word, double* bow_value, int32_t* n_bow, uint32_t* fv_node, uint32_t* fv_feat, int32_t* n_fv);

/* ------------------------------------------------------------------------------------------------------------------
 * Place recognition: data::bow_database::acquire_loop_candidates (src/PLPSLAM/data/bow_database.cc:97-168) and
 * acquire_relocalization_candidates (:170-236) with their helpers set_candidates_sharing_words (:247-287), compute_scores (:289-311),
 * align_scores_and_keyframes (:313-331) and align_total_scores_and_keyframes (:333-378), for Q queries against one database of N rows --
 * what module/relocalizer.cc:60 and module/loop_detector.cc:66-127 ask.  Numeric contract: DESIGN.md section 5, D12.
 *
 * The database is N BowVectors in the layout plp_bow_transform_device writes (row k: db_n[k] words, ascending, at db_word / db_value
 * + k * stride), the queries Q more with a stride of their own.  The reference's inverted index, its unordered sets and maps become masks
 * and arrays over the rows; nothing it returns depends on their iteration order.  Per query q (row k = key frame k):
 *   common[k]   = |words(q) AND words(k)| for an alive row, 0 for a dead one (never added, or erased)            num_common_words_ :258-284
 *   candidate   = common[k] > 0 && !reject[q][k]                                                                 init_candidates_ :276-279
 *   max_common  = max of common over candidates; thr = (unsigned)(0.8f * (float)max_common), an f32 product               :119-127
 *   score[k]    = (float)L1Scoring::score(query, row k) for candidates with thr < common[k]                               :294-308
 *   kept[k]     = candidate && thr < common[k] && min_score[q] <= score[k]                                                :318-328
 *   total[k]    = score[k] + score[c] (f32 adds, in covisibility order) over the c of covis[k] that are candidates with thr < common[c]
 *                 -- kept or not, a row naming itself included; best_kf[k] = k, or the c whose score is the first to exceed the best so
 *                 far; best_total = max(min_score[q], total[k] over kept k)                                               :337-375
 *   final[best_kf[k]] = 1 for kept k with 0.75f * best_total < total[k]                                                   :153-165
 * The score: DBoW2's L1Scoring (the ORB vocabulary's L1_NORM).  DBoW2 is not in the reference tree; the score is restated from the published
 * algorithm, as the transform is -- parity unpinned (csrc/bow_score.hpp: one f64 accumulator over the common words in ascending order).
 * scoring: the vocabulary's DBoW2 ScoringType; 0 (L1_NORM) is implemented, 1 .. 5 return PLP_ERR_UNSUPPORTED. */
typedef enum plp_bow_query_status {
    PLP_BOW_CANDIDATES = 0,       /* final holds the candidates                                                                    */
    PLP_BOW_NO_COMMON_WORDS = 1,  /* no candidate shares a word: the return of bow_database.cc:111 / :180                          */
    PLP_BOW_NO_SCORE = 2,         /* no score computed (:134 / :203).  Unreachable when max_common >= 1 -- the candidate that holds
                                     the maximum is above thr -- and kept because the reference has the branch                     */
    PLP_BOW_BELOW_MIN_SCORE = 3   /* nothing reaches min_score (:140 / :209)                                                        */
} plp_bow_query_status;
typedef struct plp_bow_query_args {
    int32_t scoring;                /* DBoW2 ScoringType of the vocabulary: 0 = L1_NORM */
    uint32_t n_words;               /* every word id is below n_words: a promise of the caller, used as an upper bound only (ids at or above it
                                       count as not shared).  Up to 1,310,720 the count runs over a bitmap of the query in LDS, above over
                                       the query's sorted words: the results are the same */
    int32_t N, stride;              /* the database: N >= 0 rows of stride slots, 1 <= stride <= 8192 */
    const uint32_t* db_word;        /* N x stride, ascending within a row */
    const double* db_value;         /* N x stride */
    const int32_t* db_n;            /* N: words of a row, taken as min(max(n, 0), stride) */
    const uint8_t* db_alive;        /* N, or NULL = all alive */
    int32_t Q, q_stride;            /* the queries: Q >= 0 rows of q_stride slots, 1 <= q_stride <= 8192 */
    const uint32_t* q_word;
    const double* q_value;
    const int32_t* q_n;             /* a query with n = 0 gets status 1 */
    const uint8_t* reject;          /* Q x N, or NULL = none: the query's connected key frames and the query itself (:107-108) */
    const float* min_score;         /* Q, a DEVICE array on the _device entry, or NULL = 0.0f for every query (relocalisation, :209, :217) */
    int32_t covis_cap;              /* 0 .. 16 slots of a covisibility row */
    const int32_t* covis;           /* N x covis_cap: get_top_n_covisibilities(10) of row k, in that order; an entry outside [0, N) is passed over */
    const int32_t* n_covis;         /* N: entries of a row, taken as min(max(n, 0), covis_cap); NULL = none */
    /* outputs, [Q][N] unless noted; any may be NULL */
    uint32_t* out_common;           /* 0 where nothing is shared or the row is dead */
    float* out_score;               /* -1.0f where not computed */
    float* out_total;               /* -1.0f where not kept */
    int32_t* out_best_kf;           /* -1 where not kept */
    uint8_t* out_final;             /* every byte written; all 0 unless status is 0 */
    int32_t* out_n_final;           /* [Q]: set bytes of final */
    uint32_t* out_max_common;       /* [Q] */
    float* out_best_total;          /* [Q]: min_score where status is not 0 */
    uint8_t* out_status;            /* [Q]: a plp_bow_query_status */
} plp_bow_query_args;
/* Checked before anything is written: NULL ctx / args, N < 0, Q < 0, a stride outside 1 .. 8192, covis_cap outside 0 .. 16, n_words == 0
 * (PLP_ERR_INVALID_ARG); scoring outside 0 .. 5 (PLP_ERR_INVALID_ARG), 1 .. 5 (PLP_ERR_UNSUPPORTED); with N > 0 a NULL db_word / db_value /
 * db_n, with Q > 0 a NULL q_word / q_value / q_n, with covis_cap > 0 and a non-NULL n_covis a NULL covis (PLP_ERR_INVALID_ARG).  Q == 0: PLP_OK,
 * nothing written.  N == 0: PLP_OK, out_n_final and out_max_common zeroed, out_best_total = min_score, out_status = 1.
 * _device: DEVICE pointers; four kernels on hip_stream and no host synchronisation (outputs passed as NULL live in a scratch buffer of the
 * context, which grows on the first call of a size).  _host: HOST pointers, staged, the same kernels, synchronous. */
plp_status plp_bow_query_device(plp_matcher* ctx, const plp_bow_query_args* args, void* hip_stream);
plp_status plp_bow_query_host(plp_matcher* ctx, const plp_bow_query_args* args);

/* Single scores with the same function: out_score[p] = (float)score(row a_row[p] of table A, row b_row[p] of table B), A's values as the
 * first argument.  loop_detector::compute_min_score_in_covisibilities (module/loop_detector.cc:238-266) is the minimum of these over the
 * covisibilities of a key frame and 1.0f; the will_be_erased filter (:248) and that minimum stay with the caller.  A row index outside its
 * table gives -1.0f.  Checks as above (strides, scoring, NULL arrays when P > 0 or a table has rows); P == 0: PLP_OK, nothing written. */
typedef struct plp_bow_score_pairs_args {
    int32_t scoring;
    int32_t NA, stride_a;           /* table A: NA rows */
    const uint32_t* a_word;
    const double* a_value;
    const int32_t* a_n;
    int32_t NB, stride_b;           /* table B (may be table A) */
    const uint32_t* b_word;
    const double* b_value;
    const int32_t* b_n;
    int32_t P;
    const int32_t* a_row;           /* P */
    const int32_t* b_row;           /* P */
    float* out_score;               /* P */
} plp_bow_score_pairs_args;
plp_status plp_bow_score_pairs_device(plp_matcher* ctx, const plp_bow_score_pairs_args* args, void* hip_stream);
plp_status plp_bow_score_pairs_host(plp_matcher* ctx, const plp_bow_score_pairs_args* args);
/* Host build of the score (csrc/bow_score.hpp), HOST pointers, before the narrowing to float.  No GPU and no context needed. */
double plp_model_bow_score_host(const uint32_t* wa, const double* va, int32_t na, const uint32_t* wb, const double* vb, int32_t nb);

/* ------------------------------------------------------------------------------------------------------------------
 * Loop candidates: solve::sim3_solver (src/PLPSLAM/solve/sim3_solver.cc), constructor and find_via_ransac, for P problems at once -- a
 * problem is one pair (current key frame 1, candidate key frame 2) of loop_detector::select_loop_candidate_via_Sim3
 * (module/loop_detector.cc:334-410): `sim3_solver solver(cur, candidate, matches, fix_scale, 20); solver.find_via_ransac(200);`.
 * Numeric contract: DESIGN.md section 5, D13 (the eigenvector of Horn's matrix by a written-down Jacobi in place of Eigen::EigenSolver,
 * f64 in the reference's order, the sample generator, points the camera does not reproject).
 *
 * The constructor's loop over the key points of key frame 1 (:70-115) is given in slot form, [P][n_cap], slot = idx1:
 *   valid       1 where the loop reaches :96, 0 where one of its four `continue`s fires: no match (:72), a NULL landmark (:80), a landmark
 *               that will_be_erased (:84), lm_2 not observed in key frame 2 (:91).  These read objects: the caller computes the byte
 *   pos_w_1/2   lm_1 / lm_2 ->get_pos_in_world()                                                                     :108, :111
 *   octave_1/2  undist_keypts_.at(idx1).octave of key frame 1, undist_keypts_.at(idx2).octave of key frame 2          :96-100
 * Common point k is the k-th valid slot in slot order (the order of common_pts_in_keyfrm_1_): that is what a sample index means.
 * The camera-frame points rot_cw * pos_w + trans_cw (:109, :112), their reprojections into their own images (:117-118) and the thresholds
 * 9.21034f * level_sigma_sq[octave] (a float product, :67, :102-103) are formed by the library.
 *
 * find_via_ransac (:121-191) runs `iters` hypotheses.  Hypothesis i takes the common points samples[p][i][0..2] (:149-154), compute_Sim3
 * (:193-288) and count_inliers (:290-325).  samples == NULL: the library draws them from `seed` (the reference draws from
 * std::random_device, util/random_array.cc:37-44: there is no order to reproduce; the generator is D13's, the same on host and device).
 * A caller's sample with an index outside [0, num_common) or a repeated index gives a hypothesis with 0 inliers.  The best hypothesis is
 * the reference's: strictly more inliers win (:168), so among equal counts the LOWEST iteration wins.
 * Outputs per problem:
 *   out_status       a plp_sim3_status
 *   out_num_common   num_common_pts_
 *   out_rot_12 (9, row-major) / out_trans_12 (3) / out_scale_12   get_best_rotation_12 / translation_12 / scale_12; zero unless PLP_SIM3_OK (:181-183)
 *   out_num_inliers  max_num_inliers (0 for PLP_SIM3_TOO_FEW_POINTS)
 *   out_best_iter    the iteration that gave it; -1 unless PLP_SIM3_OK, or when no hypothesis had an inlier
 *   out_inliers      optional, [P][n_cap] in slot order: the inlier flags of the best hypothesis (0 for a slot that is no common point;
 *                    all 0 unless PLP_SIM3_OK); slots at or above counts[p] keep the caller's values
 *   out_hyp_inliers  optional, [P][iters]: num_inliers of every hypothesis (0 for PLP_SIM3_TOO_FEW_POINTS, where the loop does not run)
 * An octave outside [0, num_levels) (where level_sigma_sq_.at() throws) and a common point behind its own camera (perspective, fisheye;
 * the reference leaves its reprojected_1_ / reprojected_2_ entry uninitialised, :352-356) make a common point that keeps its rank and is
 * no inlier of any hypothesis; a point the other camera does not reproject under a hypothesis (:336-340) is no inlier of it (D13). */
typedef enum plp_sim3_status {
    PLP_SIM3_OK = 0,               /* solution_is_valid_                                                                       :188 */
    PLP_SIM3_TOO_FEW_POINTS = 1,   /* num_common_pts_ < 3 || num_common_pts_ < min_num_inliers_                                 :130 */
    PLP_SIM3_TOO_FEW_INLIERS = 2   /* max_num_inliers < min_num_inliers_                                                       :177 */
} plp_sim3_status;
typedef struct plp_sim3_ransac_args {
    plp_camera_model camera;        /* keyfrm->camera_ of both key frames (:338, :354): model, cols, rows, fx, fy, cx, cy are read */
    int32_t P, n_cap;               /* P >= 0 problems of n_cap >= 0 slots (keyfrm_1_lms.size(), :70), n_cap <= 8192 */
    int32_t fix_scale;              /* fix_scale_ (:263): scale_21 = 1.0f */
    int32_t min_num_inliers;        /* min_num_inliers_ (:130, :177), >= 0; 20 at loop_detector.cc:370 */
    int32_t iters;                  /* max_num_iter (:145), >= 1; 200 at loop_detector.cc:371 */
    uint64_t seed;                  /* samples == NULL: the generator's seed */
    const float* level_sigma_sq_1;  /* HOST, num_levels: keyfrm_1_->level_sigma_sq_ (:99) */
    const float* level_sigma_sq_2;  /* HOST, num_levels: keyfrm_2_->level_sigma_sq_ (:100) */
    int32_t num_levels;             /* 1 .. 16 */
    const int32_t* counts;          /* P: slots in use, or NULL = n_cap everywhere */
    const uint8_t* valid;           /* P x n_cap (:72-94) */
    const double* pos_w_1;          /* P x n_cap x 3 (:108) */
    const double* pos_w_2;          /* P x n_cap x 3 (:111) */
    const int32_t* octave_1;        /* P x n_cap (:96, :99) */
    const int32_t* octave_2;        /* P x n_cap (:97, :100) */
    const double* pose_1;           /* P x 15: the plp_observe_args.pose row of key frame 1; entries 0-11, rot_cw and trans_cw, are read (:50-51) */
    const double* pose_2;           /* P x 15: key frame 2 (:52-53) */
    const int32_t* samples;         /* P x iters x 3 indices of common points (:149), or NULL = drawn from seed */
    uint8_t* out_status;            /* P */
    int32_t* out_num_common;        /* P */
    double* out_rot_12;             /* P x 9 (:171) */
    double* out_trans_12;           /* P x 3 (:172) */
    float* out_scale_12;            /* P (:173) */
    int32_t* out_num_inliers;       /* P (:170) */
    int32_t* out_best_iter;         /* P */
    uint8_t* out_inliers;           /* P x n_cap, or NULL */
    int32_t* out_hyp_inliers;       /* P x iters, or NULL */
} plp_sim3_ransac_args;
/* Checked before anything is written (PLP_ERR_INVALID_ARG): NULL ctx / args; the camera as for plp_post_extract_model_* (unknown model, fx
 * or fy 0, cols or rows <= 0); P < 0, n_cap < 0, iters < 1, min_num_inliers < 0; num_levels outside 1 .. 16 or a NULL level_sigma_sq_1 /
 * level_sigma_sq_2; and -- when P > 0 and n_cap > 0 -- a NULL valid, pos_w_1, pos_w_2, octave_1, octave_2, pose_1, pose_2, out_status,
 * out_num_common, out_rot_12, out_trans_12, out_scale_12, out_num_inliers or out_best_iter.  n_cap > 8192 or P > 65535: PLP_ERR_UNSUPPORTED.
 * P == 0 or n_cap == 0: PLP_OK, nothing written.
 * _device: every array but the two sigma tables a DEVICE pointer; three kernels on hip_stream, no host synchronisation; bad samples are
 * never an error.  The kernels hand the hypotheses to one another through buffers the context owns (38 doubles per hypothesis), so the
 * calls of one context must be ordered on the device: one stream, or events between streams.  _host: HOST pointers, staged (the outputs too, so that every slot the kernel does not write keeps the caller's value),
 * the same kernel, synchronous. */
plp_status plp_sim3_ransac_device(plp_matcher* ctx, const plp_sim3_ransac_args* args, void* hip_stream);
plp_status plp_sim3_ransac_host(plp_matcher* ctx, const plp_sim3_ransac_args* args);
/* Host builds of the same source (csrc/sim3.hpp), HOST pointers, no GPU and no context needed.
 * plp_model_sim3_ransac_host: the entry above, one problem and one hypothesis after the other; the same checks.  Returns P, or -1 for a
 * bad argument (plp_last_error() names it).
 * plp_model_horn_sim3_host: sim3_solver::compute_Sim3 (:193-288) for n pairs of row-major 3 x 3 point matrices (column c = sample c):
 * out_rot_12 / out_rot_21 n x 9, out_trans_12 / out_trans_21 n x 3, out_scale_12 / out_scale_21 n floats, out_sweeps n (may be NULL).
 * plp_model_sym_eig4_max_host: the unit eigenvector of the largest eigenvalue of n symmetric 4 x 4 matrices (row-major; the upper
 * triangle is read), ties to the lowest column, sign unspecified; out_sweeps = sweeps that rotated, 30 = the limit.  Both return n. */
int32_t plp_model_sim3_ransac_host(const plp_sim3_ransac_args* args);
int32_t plp_model_horn_sim3_host(const double* pts_1, const double* pts_2, int32_t n, int32_t fix_scale, double* out_rot_12, double* out_trans_12,
                                 float* out_scale_12, double* out_rot_21, double* out_trans_21, float* out_scale_21, int32_t* out_sweeps);
int32_t plp_model_sym_eig4_max_host(const double* N, int32_t n, double* out_v, int32_t* out_sweeps);
/* The samples the entries draw for problem p, iterations iter0 .. iter0 + n_iters - 1, of num_common >= 3 common points (D13's generator):
 * out n_iters x 3.  Returns n_iters, or -1 for a bad argument. */
int32_t plp_model_sim3_draw_host(uint64_t seed, int32_t p, int32_t iter0, int32_t n_iters, int32_t num_common, int32_t* out);

/* ------------------------------------------------------------------------------------------------------------------
 * Relocalisation: solve::pnp_solver (src/PLPSLAM/solve/pnp_solver.cc), constructor and find_via_ransac, for P problems at once -- a problem
 * is one candidate key frame of module::relocalizer::relocalize (module/relocalizer.cc:70-99):
 * `setup_pnp_solver(valid_indices, bearings, keypts, matched_landmarks, scale_factors)->find_via_ransac(30)`.
 * Numeric contract: DESIGN.md section 5, D14 (the four Eigen::JacobiSVD uses by one written-down one-sided Jacobi, f64 in the reference's
 * order, the sample generator, what the reference leaves undefined).
 *
 * extract_valid_indices + setup_pnp_solver (relocalizer.cc:254-291) are given in slot form, [P][n_cap], slot = key point of the frame:
 *   valid     1 where extract_valid_indices keeps the index: a landmark was matched (:261) that will not be erased (:265)
 *   bearing   curr_frm.bearings_.at(idx)                                                               relocalizer.cc:281, pnp_solver.cc:39
 *   pos_w     matched_landmarks.at(idx)->get_pos_in_world()                                            relocalizer.cc:287
 *   octave    curr_frm.keypts_.at(idx).octave                                                          relocalizer.cc:282, pnp_solver.cc:50
 * Match k is the k-th valid slot in slot order (the order of valid_indices): that is what a sample index means.  There is no camera: the
 * solver sees bearings only (pnp_solver.h:166: fx_ = fy_ = 1, cx_ = cy_ = 0), which covers all three camera models.
 * max_cos_errors_ (:47-51) is util::cos((float)(scale_factors[octave] * (1.0 * M_PI / 180.0))), a float per level formed by the library.
 *
 * find_via_ransac (:70-153) runs `iters` hypotheses.  Hypothesis i adds the matches samples[p][i][0..3] in that order (:103-108; signs_[0]
 * and pcs_[2] belong to the first), compute_pose (:230-290) and check_inliers (:155-181).  samples == NULL: the library draws them from
 * `seed` (the reference draws from std::random_device and shuffles, util/random_array.cc:37-88: there is no order to reproduce; the
 * generator is D14's, the same on host and device).  A caller's sample with an index outside [0, num_matches) or a repeated index, and a
 * sample whose four bearings all have z == 0 (add_correspondence skips them, :206; the reference then divides by zero correspondences),
 * give a hypothesis with 0 inliers.  The best hypothesis is the reference's: strictly more inliers win (:117), so among equal counts the
 * LOWEST iteration wins.  recompute (:136-152): compute_pose once more over all inliers of the best hypothesis in match order; when every
 * inlier has bearing z == 0 the best hypothesis' pose stays.
 * Outputs per problem:
 *   out_status       a plp_pnp_status
 *   out_num_matches  num_matches_
 *   out_rot_cw (9, row-major) / out_trans_cw (3)   get_best_rotation / get_best_translation; zero unless PLP_PNP_OK
 *   out_num_inliers  max_num_inliers (0 for PLP_PNP_TOO_FEW_MATCHES)
 *   out_best_iter    the iteration that gave it; -1 unless PLP_PNP_OK
 *   out_inliers      optional, [P][n_cap] in slot order: get_inlier_flags() of the best hypothesis, which recompute does not change (0 for a
 *                    slot that is no match; all 0 unless PLP_PNP_OK); slots at or above counts[p] keep the caller's values
 *   out_hyp_inliers  optional, [P][iters]: num_inliers of every hypothesis (0 for PLP_PNP_TOO_FEW_MATCHES, where the loop does not run)
 * An octave outside [0, num_levels) (where scale_factors.at() throws, :50) makes a match that keeps its rank and is no inlier of any
 * hypothesis; sampled, it is a correspondence like any other (its threshold is not read there). */
typedef enum plp_pnp_status {
    PLP_PNP_OK = 0,                /* solution_is_valid_                                                                       :128 */
    PLP_PNP_TOO_FEW_MATCHES = 1,   /* num_matches_ < 4 || num_matches_ < min_num_inliers_                                       :76 */
    PLP_PNP_TOO_FEW_INLIERS = 2    /* !(max_num_inliers > min_num_inliers_): strict, unlike plp_sim3_status                     :126 */
} plp_pnp_status;
typedef struct plp_pnp_ransac_args {
    int32_t P, n_cap;               /* P >= 0 problems of n_cap >= 0 slots (curr_frm.num_keypts_), n_cap <= 8192 */
    int32_t min_num_inliers;        /* min_num_inliers_ (:76, :126), >= 0; 10 by the constructor's default (pnp_solver.h) */
    int32_t iters;                  /* max_num_iter (:96), >= 1; 30 at relocalizer.cc:93 */
    int32_t recompute;              /* :131-152; true by find_via_ransac's default */
    uint64_t seed;                  /* samples == NULL: the generator's seed */
    const float* scale_factors;     /* HOST, num_levels: curr_frm.scale_factors_ (:50) */
    int32_t num_levels;             /* 1 .. 16 */
    const int32_t* counts;          /* P: slots in use, or NULL = n_cap everywhere */
    const uint8_t* valid;           /* P x n_cap (relocalizer.cc:258-270) */
    const double* bearing;          /* P x n_cap x 3 (:105) */
    const double* pos_w;            /* P x n_cap x 3 (:106) */
    const int32_t* octave;          /* P x n_cap (:50) */
    const int32_t* samples;         /* P x iters x 4 indices of matches (:99), or NULL = drawn from seed */
    uint8_t* out_status;            /* P */
    int32_t* out_num_matches;       /* P */
    double* out_rot_cw;             /* P x 9 (:120, :152) */
    double* out_trans_cw;           /* P x 3 (:121, :152) */
    int32_t* out_num_inliers;       /* P (:119) */
    int32_t* out_best_iter;         /* P */
    uint8_t* out_inliers;           /* P x n_cap, or NULL (:122) */
    int32_t* out_hyp_inliers;       /* P x iters, or NULL */
} plp_pnp_ransac_args;
/* Checked before anything is written (PLP_ERR_INVALID_ARG): NULL ctx / args; P < 0, n_cap < 0, iters < 1, min_num_inliers < 0; num_levels
 * outside 1 .. 16 or a NULL scale_factors; and -- when P > 0 and n_cap > 0 -- a NULL valid, bearing, pos_w, octave, out_status,
 * out_num_matches, out_rot_cw, out_trans_cw, out_num_inliers or out_best_iter.  n_cap > 8192 or P > 65535: PLP_ERR_UNSUPPORTED.
 * P == 0 or n_cap == 0: PLP_OK, nothing written.
 * _device: every array but scale_factors a DEVICE pointer; five kernels on hip_stream, no host synchronisation; bad samples are never an
 * error.  The kernels hand the ranks, the hypotheses and the refit's correspondences to one another through buffers the context owns, so
 * the calls of one context must be ordered on the device: one stream, or events between streams.  _host: HOST pointers, staged (the
 * outputs too, so that every slot the kernels do not write keeps the caller's value), the same kernels, synchronous. */
plp_status plp_pnp_ransac_device(plp_matcher* ctx, const plp_pnp_ransac_args* args, void* hip_stream);
plp_status plp_pnp_ransac_host(plp_matcher* ctx, const plp_pnp_ransac_args* args);
/* Host builds of the same source (csrc/pnp.hpp), HOST pointers, no GPU and no context needed.
 * plp_model_pnp_ransac_host: the entry above, one problem and one hypothesis after the other; the same checks.  Returns P, or -1 for a bad
 * argument (plp_last_error() names it).
 * plp_model_epnp_host: compute_pose (:230-290) for n lists of correspondences: list i holds pos_w / bearing rows offsets[i] .. offsets[i+1]
 * (add_correspondence skips bearing z == 0).  out_rot n x 9, out_trans n x 3, out_err n (the reprojection error returned), out_N n (the
 * chosen approximation 1 .. 3), out_sweeps n x 8 (may be NULL; PW0tPW0, MtM, the three least-squares systems, the three Abt).  A list
 * without a correspondence left gives zeros and N = 0.  Returns n.
 * plp_model_sym_jacobi_host: uses 1 and 2 of D14 for n symmetric dim x dim matrices (row-major), dim = 3 or 12: out_vals n x dim singular
 * values descending, out_ut n x dim x dim (row r = the vector of out_vals[r]), out_sweeps n (may be NULL; 60 = the limit).
 * plp_model_lstsq6_host: use 3 for n systems A (6 x k row-major) x = b, k = 3, 4 or 5: out_x n x k.
 * plp_model_rot_from_abt_host: use 4 for n 3 x 3 matrices (row-major): out_rot n x 9.  All return n, or -1 for a bad argument. */
int32_t plp_model_pnp_ransac_host(const plp_pnp_ransac_args* args);
int32_t plp_model_epnp_host(const double* pos_w, const double* bearing, const int32_t* offsets, int32_t n, double* out_rot, double* out_trans,
                            double* out_err, int32_t* out_N, int32_t* out_sweeps);
int32_t plp_model_sym_jacobi_host(const double* A, int32_t dim, int32_t n, double* out_vals, double* out_ut, int32_t* out_sweeps);
int32_t plp_model_lstsq6_host(const double* A, const double* b, int32_t k, int32_t n, double* out_x, int32_t* out_sweeps);
int32_t plp_model_rot_from_abt_host(const double* Abt, int32_t n, double* out_rot, int32_t* out_sweeps);
/* The samples the entries draw for problem p, iterations iter0 .. iter0 + n_iters - 1, of num_matches >= 4 matches (D14's generator):
 * out n_iters x 4.  Returns n_iters, or -1 for a bad argument. */
int32_t plp_model_pnp_draw_host(uint64_t seed, int32_t p, int32_t iter0, int32_t n_iters, int32_t num_matches, int32_t* out);
/* max_cos_errors_ per level (:47-51) for num_levels scale factors: out num_levels floats.  Returns num_levels, or -1. */
int32_t plp_model_pnp_thresholds_host(const float* scale_factors, int32_t num_levels, float* out);

/* ------------------------------------------------------------------------------------------------------------------
 * Map initialisation and the tracker's robust match: solve::essential_solver (src/PLPSLAM/solve/essential_solver.cc:33-253), constructor,
 * find_via_ransac, compute_E_21 and check_inliers, for P problems at once -- a problem is one pair of frames (1 = reference, 2 = current):
 * `essential_solver(ref_bearings, cur_bearings, ref_cur_matches).find_via_ransac(num_ransac_iters)` of initialize::bearing_vector::initialize
 * (initialize/bearing_vector.cc:55-75; 100 iterations, recompute true), the initialiser of the fisheye and equirectangular models
 * (module/initializer.cc:169-178), and `find_via_ransac(50, false)` of match::robust::match_frame_and_keyframe (match/robust.cc:233).
 * Numeric contract: DESIGN.md section 5, D24 (the two Eigen::JacobiSVD uses by D14's written-down one-sided Jacobi on A^T A and on the 3 x 3
 * matrix, the sign rule, f64 in the reference's order with the reference's float residuals and float score, the sample generator, what the
 * reference leaves undefined).
 *
 * The constructor's match list is given in slot form, [P][n_cap], slot = key-point index in frame 1:
 *   bearing_1   bearings_1_.at(idx1), [P][n_cap][3]; bearing_2: bearings_2_.at(idx2), [P][m_cap][3] (the post-extract step's layout)
 *   match       the index in frame 2 or a negative number: plp_match_*'s out_match, init_matches_ (bearing_vector.cc:58-65)
 * Match k of matches_12_ is the k-th matched slot in slot order (both callers list their matches in ascending idx1): that is what a sample
 * index means.  A match value at or above counts_2[p] (where bearings_2_.at() throws) is no match.
 *
 * find_via_ransac (:37-119) runs `iters` hypotheses.  Hypothesis i takes the matches samples[p][i][0..7] in that order (:73-78), compute_E_21
 * (:121-154) and check_inliers (:196-253).  samples == NULL: the library draws them from `seed` (the reference draws from
 * std::random_device, util/random_array.cc:37-44: there is no order to reproduce; the generator is D24's, the same on host and device).  A
 * caller's sample with an index outside [0, num_matches) or a repeated index gives a hypothesis of score 0, which cannot win.  The best
 * hypothesis is the reference's: a strictly greater score wins (:87), so among equal scores the LOWEST iteration wins; a NaN score never
 * wins.  recompute (:103-118): compute_E_21 once more over the inliers of the best hypothesis in match order and check_inliers once more;
 * its matrix, score and flags are the outputs, and its inliers may be fewer than eight with the status still PLP_ESSENTIAL_OK, as in the
 * reference.
 * Outputs per problem:
 *   out_status       a plp_essential_status
 *   out_num_matches  matches_12_.size()
 *   out_E_21 (9, row-major)   get_best_E_21(); zero unless PLP_ESSENTIAL_OK
 *   out_score        best_score_ (a float sum of float residuals in match order); 0 unless PLP_ESSENTIAL_OK
 *   out_num_inliers  the inlier matches of the matrix returned; 0 unless PLP_ESSENTIAL_OK
 *   out_best_iter    the iteration that won; -1 unless PLP_ESSENTIAL_OK
 *   out_inliers      optional, [P][n_cap] in slot order: is_inlier_match_ of the matrix returned (0 for a slot that is no match; all 0 unless
 *                    PLP_ESSENTIAL_OK); slots at or above counts_1[p] keep the caller's values
 *   out_hyp_score    optional, [P][iters]: the score of every hypothesis (0 for PLP_ESSENTIAL_TOO_FEW_MATCHES, where the loop does not run) */
typedef enum plp_essential_status {
    PLP_ESSENTIAL_OK = 0,               /* solution_is_valid_                                                                   :96 */
    PLP_ESSENTIAL_TOO_FEW_MATCHES = 1,  /* num_matches < 8                                                                      :45 */
    PLP_ESSENTIAL_INVALID = 2           /* !(best_score_ > 0.0 && num_inliers >= 8)                                             :96 */
} plp_essential_status;
typedef struct plp_essential_ransac_args {
    int32_t P, n_cap, m_cap;        /* P >= 0 problems of n_cap >= 0 slots (key points of frame 1) against m_cap >= 0 key points of frame 2; n_cap <= 8192 */
    int32_t iters;                  /* max_num_iter (:69), >= 1; 100 in the initialiser, 50 at robust.cc:233 */
    int32_t recompute;              /* :98-118; true in the initialiser, false at robust.cc:233 */
    uint64_t seed;                  /* samples == NULL: the generator's seed */
    const int32_t* counts_1;        /* P: slots in use, or NULL = n_cap everywhere */
    const int32_t* counts_2;        /* P: key points of frame 2, or NULL = m_cap everywhere */
    const double* bearing_1;        /* P x n_cap x 3 (:76) */
    const double* bearing_2;        /* P x m_cap x 3 (:77) */
    const int32_t* match;           /* P x n_cap */
    const int32_t* samples;         /* P x iters x 8 indices of matches (:72), or NULL = drawn from seed */
    uint8_t* out_status;            /* P */
    int32_t* out_num_matches;       /* P */
    double* out_E_21;               /* P x 9 (:90, :117) */
    float* out_score;               /* P (:89, :118) */
    int32_t* out_num_inliers;       /* P */
    int32_t* out_best_iter;         /* P */
    uint8_t* out_inliers;           /* P x n_cap, or NULL (:91, :118) */
    float* out_hyp_score;           /* P x iters, or NULL */
} plp_essential_ransac_args;
/* Checked before anything is written (PLP_ERR_INVALID_ARG): NULL ctx / args; P < 0, n_cap < 0, m_cap < 0, iters < 1; and -- when P > 0 and
 * n_cap > 0 -- a NULL bearing_1, match, bearing_2 (with m_cap > 0), out_status, out_num_matches, out_E_21, out_score, out_num_inliers or
 * out_best_iter.  n_cap > 8192, P > 65535 or iters > 65536: PLP_ERR_UNSUPPORTED.  P == 0 or n_cap == 0: PLP_OK, nothing written.
 * _device: every array a DEVICE pointer; five kernels on hip_stream, no host synchronisation; bad samples are never an error.  The kernels
 * hand the match list, the hypotheses, the refit's bearing pairs and the inlier codes to one another through buffers the context owns, so
 * the calls of one context must be ordered on the device: one stream, or events between streams.  _host: HOST pointers, staged (the
 * outputs too, so that every slot the kernels do not write keeps the caller's value), the same kernels, synchronous. */
plp_status plp_essential_ransac_device(plp_matcher* ctx, const plp_essential_ransac_args* args, void* hip_stream);
plp_status plp_essential_ransac_host(plp_matcher* ctx, const plp_essential_ransac_args* args);
/* Host builds of the same source (csrc/essential.hpp), HOST pointers, no GPU and no context needed.
 * plp_model_essential_ransac_host: the entry above, one problem and one hypothesis after the other; the same checks.  Returns P, or -1 for
 * a bad argument (plp_last_error() names it).
 * plp_model_essential_fit_host: compute_E_21 (:121-154) for n lists of bearing pairs: list i holds rows offsets[i] .. offsets[i+1] of
 * bearing_1 / bearing_2.  out_E_21 n x 9, out_sweeps n x 2 (may be NULL; the 9 x 9 and the 3 x 3 Jacobi, 60 = the limit).  Returns n.
 * plp_model_essential_check_host: check_inliers (:196-253) of n matrices E_21 (n x 9) against one problem (bearing_1 n_cap x 3, bearing_2
 * m_cap x 3, match n_cap; a match outside [0, m_cap) is none): out_score n, out_num_inliers n, out_inliers n x n_cap in slot order (may be
 * NULL).  Returns n.  Both return -1 for a bad argument. */
int32_t plp_model_essential_ransac_host(const plp_essential_ransac_args* args);
int32_t plp_model_essential_fit_host(const double* bearing_1, const double* bearing_2, const int32_t* offsets, int32_t n, double* out_E_21, int32_t* out_sweeps);
int32_t plp_model_essential_check_host(const double* bearing_1, const double* bearing_2, const int32_t* match, int32_t n_cap, int32_t m_cap, const double* E_21,
                                       int32_t n, float* out_score, int32_t* out_num_inliers, uint8_t* out_inliers);
/* The samples the entries draw for problem p, iterations iter0 .. iter0 + n_iters - 1, of num_matches >= 8 matches (D24's generator):
 * out n_iters x 8.  Returns n_iters, or -1 for a bad argument. */
int32_t plp_model_essential_draw_host(uint64_t seed, int32_t p, int32_t iter0, int32_t n_iters, int32_t num_matches, int32_t* out);

/* ------------------------------------------------------------------------------------------------------------------
 * Map initialisation, from the matrix to the pose: bearing_vector::reconstruct_with_E (src/PLPSLAM/initialize/bearing_vector.cc:84-107) for P
 * frame pairs -- essential_solver::decompose (solve/essential_solver.cc:156-186) and initialize::base::find_most_plausible_pose with its four
 * check_pose calls (initialize/base.cc:62-243; solve::triangulator::triangulate, solve/triangulator.h:86-103).  Numeric contract: DESIGN.md
 * section 5, D24 items c, f and g.  The inputs are the outputs of plp_essential_ransac_* (E_21 <- out_E_21, inliers <- out_inliers, in_status
 * <- out_status, the same match and bearing tables) and the post-extract step's undistorted key points of both frames (only pt is read), so
 * the two entries chain on one stream without the host.
 *
 * The four hypotheses are (rot_1, t), (rot_1, -t), (rot_2, t), (rot_2, -t) (:182-183), with D24 item c's rule for what the singular-value
 * routine leaves open; every inlier match is triangulated under each and passes the tests of check_pose in the reference's order.
 * Outputs per problem:
 *   out_status             a plp_two_view_status
 *   out_rot_ref_to_cur (9, row-major) / out_trans_ref_to_cur (3)   zero unless PLP_TWO_VIEW_OK (base.cc:83-84)
 *   out_hypothesis         0 .. 3, -1 unless PLP_TWO_VIEW_OK
 *   out_num_valid [P][4]   nums_valid_pts; out_parallax_deg [P][4] (float): init_parallax; both zero for PLP_TWO_VIEW_NO_SOLUTION
 *   out_triangulated_pts [P][n_cap][3], out_is_triangulated [P][n_cap]   triangulated_pts_ / is_triangulated_ of the chosen hypothesis,
 *                          indexed by slot (the reference key point); all zero unless PLP_TWO_VIEW_OK; a point that is not triangulated
 *                          (uninitialised in the reference) is zero; slots at or above counts_1[p] keep the caller's values
 *   out_hyp_is_triangulated   optional, [P][4][n_cap]: the flags of all four hypotheses (zero for PLP_TWO_VIEW_NO_SOLUTION) */
typedef enum plp_two_view_status {
    PLP_TWO_VIEW_OK = 0,
    PLP_TWO_VIEW_NO_SOLUTION = 1,           /* in_status[p] != 0: the RANSAC gave no matrix (bearing_vector.cc:72-81)                    */
    PLP_TWO_VIEW_TOO_FEW_TRIANGULATED = 2,  /* base.cc:92 */
    PLP_TWO_VIEW_AMBIGUOUS = 3,             /* base.cc:103 */
    PLP_TWO_VIEW_SMALL_PARALLAX = 4         /* base.cc:109 */
} plp_two_view_status;
typedef struct plp_two_view_pose_args {
    plp_camera_model camera;        /* camera_ of both frames: model, cols, rows, fx, fy, cx, cy, focal_x_baseline are read; all three models */
    float img_bounds[4];            /* camera::base img_bounds_: min_x, max_x, min_y, max_y (what reproject_to_image of perspective / fisheye returns) */
    int32_t P, n_cap, m_cap;        /* as plp_essential_ransac_args */
    int32_t min_num_triangulated;   /* min_num_triangulated_ (base.cc:92), >= 0; 50 */
    float parallax_deg_thr;         /* parallax_deg_thr_ (base.cc:109); 1.0 */
    float reproj_err_thr;           /* reproj_err_thr_ (base.cc:130); 4.0 */
    int32_t depth_is_positive;      /* base.cc:173-184; false at bearing_vector.cc:99 */
    const int32_t* counts_1;        /* P, or NULL = n_cap everywhere */
    const int32_t* counts_2;        /* P, or NULL = m_cap everywhere */
    const uint8_t* in_status;       /* P, or NULL: a problem whose byte is not 0 (PLP_ESSENTIAL_OK) is PLP_TWO_VIEW_NO_SOLUTION */
    const double* E_21;             /* P x 9, row-major */
    const uint8_t* inliers;         /* P x n_cap: is_inlier_match in slot order */
    const int32_t* match;           /* P x n_cap */
    const double* bearing_1;        /* P x n_cap x 3 */
    const double* bearing_2;        /* P x m_cap x 3 */
    const plp_keypoint* undist_1;   /* P x n_cap: ref_undist_keypts_ (pt is read) */
    const plp_keypoint* undist_2;   /* P x m_cap: cur_undist_keypts_ */
    uint8_t* out_status;            /* P */
    double* out_rot_ref_to_cur;     /* P x 9 */
    double* out_trans_ref_to_cur;   /* P x 3 */
    int32_t* out_hypothesis;        /* P */
    int32_t* out_num_valid;         /* P x 4 */
    float* out_parallax_deg;        /* P x 4 */
    double* out_triangulated_pts;   /* P x n_cap x 3 */
    uint8_t* out_is_triangulated;   /* P x n_cap */
    uint8_t* out_hyp_is_triangulated;   /* P x 4 x n_cap, or NULL */
} plp_two_view_pose_args;
/* Checked before anything is written (PLP_ERR_INVALID_ARG): NULL ctx / args; the camera as for plp_post_extract_model_* (unknown model, fx
 * or fy 0, cols or rows <= 0); P < 0, n_cap < 0, m_cap < 0, min_num_triangulated < 0; and -- when P > 0 and n_cap > 0 -- a NULL E_21, inliers,
 * match, bearing_1, undist_1, bearing_2 or undist_2 (with m_cap > 0), out_status, out_rot_ref_to_cur, out_trans_ref_to_cur, out_hypothesis,
 * out_num_valid, out_parallax_deg, out_triangulated_pts or out_is_triangulated.  n_cap > 8192 or P > 65535: PLP_ERR_UNSUPPORTED.  P == 0 or
 * n_cap == 0: PLP_OK, nothing written.
 * _device: every array a DEVICE pointer; one kernel on hip_stream, no host synchronisation.  The points and flags of the four hypotheses
 * wait in buffers the context owns, so the calls of one context must be ordered on the device: one stream, or events between streams.
 * _host: HOST pointers, staged (the outputs too, so that every slot the kernel does not write keeps the caller's value), the same kernel,
 * synchronous. */
plp_status plp_two_view_pose_device(plp_matcher* ctx, const plp_two_view_pose_args* args, void* hip_stream);
plp_status plp_two_view_pose_host(plp_matcher* ctx, const plp_two_view_pose_args* args);
/* Host builds of the same source (csrc/two_view.hpp), HOST pointers, no GPU and no context needed.
 * plp_model_two_view_pose_host: the entry above, one problem after the other; the same checks.  Returns P, or -1 for a bad argument.
 * plp_model_essential_decompose_host: decompose for n matrices (n x 9): out_rots n x 2 x 9 (rot_1, rot_2), out_trans n x 3.  Returns n.
 * plp_model_check_pose_host: check_pose of ONE (rot 9, trans 3) against problem 0 of args (its E_21, in_status and outputs are not read):
 * out_num_valid 1, out_parallax_deg 1, out_pts n_cap x 3, out_is_triangulated n_cap, out_code n_cap (may be NULL: per slot 0 = no inlier
 * match, 1 .. 7 = the `continue` of base.cc:158, 175, 180, 194, 200, 210, 215 that the match takes, 8 = valid with a small parallax, 9 =
 * valid and triangulated).  Returns 1, or -1. */
int32_t plp_model_two_view_pose_host(const plp_two_view_pose_args* args);
int32_t plp_model_essential_decompose_host(const double* E_21, int32_t n, double* out_rots, double* out_trans);
int32_t plp_model_check_pose_host(const plp_two_view_pose_args* args, const double* rot, const double* trans, int32_t* out_num_valid, float* out_parallax_deg,
                                  double* out_pts, uint8_t* out_is_triangulated, uint8_t* out_code);

/* ------------------------------------------------------------------------------------------------------------------
 * Map initialisation of the perspective and fisheye cameras (module/initializer.cc:166-172), the two solvers of
 * initialize::perspective::initialize (src/PLPSLAM/initialize/perspective.cc:84-120) for P frame pairs at once:
 *   solve::homography_solver   (src/PLPSLAM/solve/homography_solver.cc)   find_via_ransac :60-155, compute_H_21 :405-436, check_inliers :556-631,
 *                              and what find_via_graph_cut_ransac does with the matrix its RANSAC found, :388-402
 *   solve::fundamental_solver  (src/PLPSLAM/solve/fundamental_solver.cc)  find_via_ransac :50-144, compute_F_21 :299-332, check_inliers :349-426
 *   solve::normalize           (src/PLPSLAM/solve/common.cc:31-76), over ALL key points of a frame
 *   the choice between the two (perspective.cc:99-120)
 * Numeric contract: DESIGN.md section 5, D27.  sigma is 1.0 (perspective.cc:84-87).
 *
 * The match list is given in slot form as for the essential entry: match [P][n_cap], slot = key-point index in frame 1, the value the index in
 * frame 2 or a negative number; match k is the k-th matched slot in slot order; a value at or above counts_2[p] is no match.  The key points are
 * the frames' undist_keypts_ (pt is read).
 *
 * Each solver runs `iters` hypotheses.  Hypothesis i of H takes the matches samples_h[p][i][0..7], of F samples_f[p][i][0..7]; a NULL table is
 * drawn from `seed` (D27 item f: the two solvers draw from different streams).  A sample with an index outside [0, num_matches) or a repeated
 * index gives a hypothesis of score 0.  Per solver the best hypothesis is the reference's: a strictly greater score wins, among equals the
 * lowest iteration; a NaN score never wins.  recompute: the matrix is fitted once more over the inliers of the best hypothesis in match order and
 * checked once more (:133-154, :122-143).
 *
 * A given homography (the graph-cut path): with given_H_21 and given_H_num_inliers both non-NULL, a problem whose given_H_num_inliers[p] >= 0
 * runs no H hypothesis.  Its given_H_21[p] is scored by check_inliers (:398), which also gives its mask, and it is valid when that score is
 * > 0 and given_H_num_inliers[p] >= 8 (:401-402).  A negative given_H_num_inliers[p] leaves problem p to the RANSAC.  F is not affected.
 *
 * Outputs per problem:
 *   out_status_h / _f       a plp_perspective_status per solver
 *   out_num_matches         matches_12_.size()
 *   out_H_21 / out_F_21     (9, row-major) get_best_H_21() / get_best_F_21(); zero unless the solver's status is PLP_PERSPECTIVE_OK
 *   out_score_h / _f        get_best_score() as the reference leaves it: the score of the matrix held, also where the solution is not valid
 *                           (fewer than eight inliers); 0 for PLP_PERSPECTIVE_TOO_FEW_MATCHES
 *   out_best_iter_h / _f    the iteration that won; -1 unless OK, and -1 for a given homography
 *   out_num_inliers_h / _f  the inlier matches of the matrix returned; 0 unless OK
 *   out_rel_score_h         score_H / (score_H + score_F) as a float (perspective.cc:102); NaN when both are 0
 *   out_choice              a plp_perspective_choice, perspective.cc:105-120
 *   out_inliers             [P][n_cap] in slot order: is_inlier_match of the chosen solver (0 for a slot that is no match, all 0 for no choice);
 *                           slots at or above counts_1[p] keep the caller's values
 *   out_inliers_h / _f      optional, likewise per solver (all 0 unless OK)
 *   out_hyp_score_h / _f    optional, [P][iters]: the score of every hypothesis (0 where none runs) */
typedef enum plp_perspective_status {
    PLP_PERSPECTIVE_OK = 0,               /* solution_is_valid_                                     homography_solver.cc:131, :402; fundamental_solver.cc:120 */
    PLP_PERSPECTIVE_TOO_FEW_MATCHES = 1,  /* num_matches < 8                                        homography_solver.cc:78; fundamental_solver.cc:68 */
    PLP_PERSPECTIVE_INVALID = 2           /* !(best_score_ > 0.0 && num_inliers >= 8) */
} plp_perspective_status;
typedef enum plp_perspective_choice {
    PLP_PERSPECTIVE_CHOICE_NONE = 0,      /* perspective.cc:117-120 */
    PLP_PERSPECTIVE_CHOICE_H = 1,         /* 0.40 < rel_score_H and H valid                         perspective.cc:105 */
    PLP_PERSPECTIVE_CHOICE_F = 2          /* otherwise, F valid                                     perspective.cc:111 */
} plp_perspective_choice;
typedef struct plp_perspective_ransac_args {
    int32_t P, n_cap, m_cap;        /* P >= 0 problems of n_cap >= 0 key points of frame 1 against m_cap >= 0 of frame 2; n_cap <= 8192 */
    int32_t iters;                  /* num_ransac_iters_, >= 1 */
    int32_t recompute;              /* true in perspective.cc:90-95 */
    uint64_t seed;                  /* the generator's seed where a sample table is NULL */
    const int32_t* counts_1;        /* P: key points of frame 1, or NULL = n_cap everywhere */
    const int32_t* counts_2;        /* P: key points of frame 2, or NULL = m_cap everywhere */
    const plp_keypoint* undist_1;   /* P x n_cap: ref_undist_keypts_ */
    const plp_keypoint* undist_2;   /* P x m_cap: cur_undist_keypts_ */
    const int32_t* match;           /* P x n_cap */
    const int32_t* samples_h;       /* P x iters x 8 indices of matches, or NULL = drawn from seed */
    const int32_t* samples_f;       /* P x iters x 8, or NULL */
    const double* given_H_21;       /* P x 9, or NULL */
    const int32_t* given_H_num_inliers; /* P: statistics.inliers.size() of the caller's RANSAC, negative = none given; or NULL */
    uint8_t* out_status_h;          /* P */
    uint8_t* out_status_f;          /* P */
    int32_t* out_num_matches;       /* P */
    double* out_H_21;               /* P x 9 */
    double* out_F_21;               /* P x 9 */
    float* out_score_h;             /* P */
    float* out_score_f;             /* P */
    int32_t* out_best_iter_h;       /* P */
    int32_t* out_best_iter_f;       /* P */
    int32_t* out_num_inliers_h;     /* P */
    int32_t* out_num_inliers_f;     /* P */
    float* out_rel_score_h;         /* P */
    uint8_t* out_choice;            /* P */
    uint8_t* out_inliers;           /* P x n_cap */
    uint8_t* out_inliers_h;         /* P x n_cap, or NULL */
    uint8_t* out_inliers_f;         /* P x n_cap, or NULL */
    float* out_hyp_score_h;         /* P x iters, or NULL */
    float* out_hyp_score_f;         /* P x iters, or NULL */
} plp_perspective_ransac_args;
/* Checked before anything is written (PLP_ERR_INVALID_ARG): NULL ctx / args; P < 0, n_cap < 0, m_cap < 0, iters < 1; exactly one of given_H_21
 * and given_H_num_inliers; and -- when P > 0 and n_cap > 0 -- a NULL undist_1, match, undist_2 (with m_cap > 0) or required output (every out_
 * field that is not marked "or NULL").  n_cap > 8192, P > 65535 or iters > 65536: PLP_ERR_UNSUPPORTED.  P == 0 or n_cap == 0: PLP_OK,
 * nothing written.
 * _device: every array a DEVICE pointer; five kernels on hip_stream, no host synchronisation; bad samples are never an error.  The kernels hand
 * their work to one another through buffers the context owns, so the calls of one context must be ordered on the device.  _host: HOST
 * pointers, staged (the outputs too, so that every slot the kernels do not write keeps the caller's value), the same kernels, synchronous. */
plp_status plp_perspective_ransac_device(plp_matcher* ctx, const plp_perspective_ransac_args* args, void* hip_stream);
plp_status plp_perspective_ransac_host(plp_matcher* ctx, const plp_perspective_ransac_args* args);
/* Host builds of the same source (csrc/perspective_init.hpp), HOST pointers, no GPU and no context needed; -1 for a bad argument.
 * plp_model_perspective_ransac_host: the entry above, one problem and one hypothesis after the other; the same checks.  Returns P.
 * plp_model_normalize_keypoints_host: solve::normalize of n key points: out_normalized n x 2 floats (may be NULL), out_stats 4 floats (mean_x,
 * mean_y, 1 / dev_x, 1 / dev_y), out_transform 9.  Returns n.
 * plp_model_homography_fit_host / plp_model_fundamental_fit_host: compute_H_21 / compute_F_21 for n lists of point pairs: list i holds rows
 * offsets[i] .. offsets[i+1] of pts_1 / pts_2 (x, y floats, as normalised).  out n x 9, out_sweeps n (may be NULL; the 9 x 9 Jacobi).  Returns n.
 * plp_model_homography_check_host / plp_model_fundamental_check_host: check_inliers of n matrices (n x 9) against one problem (undist_1 n_cap,
 * undist_2 m_cap, match n_cap; a match outside [0, m_cap) is none): out_score n, out_num_inliers n, out_inliers n x n_cap in slot order (may be
 * NULL).  Returns n.
 * plp_model_perspective_draw_host: the samples the entries draw for problem p, iterations iter0 .. iter0 + n_iters - 1, of num_matches >= 8
 * matches; solver 0 = H, 1 = F.  out n_iters x 8.  Returns n_iters. */
int32_t plp_model_perspective_ransac_host(const plp_perspective_ransac_args* args);
int32_t plp_model_normalize_keypoints_host(const plp_keypoint* keypts, int32_t n, float* out_normalized, float* out_stats, double* out_transform);
int32_t plp_model_homography_fit_host(const float* pts_1, const float* pts_2, const int32_t* offsets, int32_t n, double* out_H_21, int32_t* out_sweeps);
int32_t plp_model_fundamental_fit_host(const float* pts_1, const float* pts_2, const int32_t* offsets, int32_t n, double* out_F_21, int32_t* out_sweeps);
int32_t plp_model_homography_check_host(const plp_keypoint* undist_1, const plp_keypoint* undist_2, const int32_t* match, int32_t n_cap, int32_t m_cap,
                                        const double* H_21, int32_t n, float* out_score, int32_t* out_num_inliers, uint8_t* out_inliers);
int32_t plp_model_fundamental_check_host(const plp_keypoint* undist_1, const plp_keypoint* undist_2, const int32_t* match, int32_t n_cap, int32_t m_cap,
                                         const double* F_21, int32_t n, float* out_score, int32_t* out_num_inliers, uint8_t* out_inliers);
int32_t plp_model_perspective_draw_host(int32_t solver, uint64_t seed, int32_t p, int32_t iter0, int32_t n_iters, int32_t num_matches, int32_t* out);

/* ------------------------------------------------------------------------------------------------------------------
 * Map initialisation of the perspective and fisheye cameras, from the chosen matrix to the pose: perspective::reconstruct_with_H and
 * reconstruct_with_F (src/PLPSLAM/initialize/perspective.cc:123-174) for P frame pairs -- homography_solver::decompose
 * (solve/homography_solver.cc:438-554; eight hypotheses, the normals are not formed) or fundamental_solver::decompose
 * (solve/fundamental_solver.cc:334-340; four), then initialize::base::find_most_plausible_pose(..., true) with one check_pose call per
 * hypothesis (initialize/base.cc:62-243), depth_is_positive true.  Numeric contract: DESIGN.md section 5, D27 items e and h, with D24 items
 * c, f and g.  The inputs are the outputs of the RANSAC entry above (in_choice <- out_choice, H_21 <- out_H_21, F_21 <- out_F_21, inliers <-
 * out_inliers, the same match and key-point tables) and the frames' bearings, so the two entries chain on one stream without the host.
 * The camera matrix of both frames is the camera's (get_camera_matrix, perspective.cc:176-199): perspective and fisheye; the
 * equirectangular model, where the reference throws, is PLP_ERR_UNSUPPORTED.
 * Outputs per problem as for plp_two_view_pose_args, over eight hypotheses:
 *   out_status             a plp_two_view_status, or PLP_PERSPECTIVE_POSE_NO_DECOMPOSITION; PLP_TWO_VIEW_NO_SOLUTION for in_choice[p] == 0
 *   out_hypothesis         0 .. 7 (H) or 0 .. 3 (F), -1 unless PLP_TWO_VIEW_OK
 *   out_num_valid [P][8], out_parallax_deg [P][8]   the first four used for F, the others zero; all zero without a decomposition
 *   out_hyp_is_triangulated   optional, [P][8][n_cap] */
typedef enum plp_perspective_pose_status {
    PLP_PERSPECTIVE_POSE_NO_DECOMPOSITION = 5   /* homography_solver::decompose returned false: the rank test of homography_solver.cc:462 */
} plp_perspective_pose_status;
typedef struct plp_perspective_pose_args {
    plp_camera_model camera;        /* camera_ of both frames; perspective or fisheye */
    float img_bounds[4];            /* camera::base img_bounds_: min_x, max_x, min_y, max_y */
    int32_t P, n_cap, m_cap;        /* as plp_perspective_ransac_args */
    int32_t min_num_triangulated;   /* min_num_triangulated_ (base.cc:92), >= 0; 50 */
    float parallax_deg_thr;         /* parallax_deg_thr_ (base.cc:109); 1.0 */
    float reproj_err_thr;           /* reproj_err_thr_ (base.cc:130); 4.0 */
    const int32_t* counts_1;        /* P, or NULL = n_cap everywhere */
    const int32_t* counts_2;        /* P, or NULL = m_cap everywhere */
    const uint8_t* in_choice;       /* P: a plp_perspective_choice */
    const double* H_21;             /* P x 9, row-major; read where in_choice[p] is PLP_PERSPECTIVE_CHOICE_H */
    const double* F_21;             /* P x 9; read where it is PLP_PERSPECTIVE_CHOICE_F */
    const uint8_t* inliers;         /* P x n_cap: is_inlier_match of the chosen solver in slot order */
    const int32_t* match;           /* P x n_cap */
    const double* bearing_1;        /* P x n_cap x 3 */
    const double* bearing_2;        /* P x m_cap x 3 */
    const plp_keypoint* undist_1;   /* P x n_cap */
    const plp_keypoint* undist_2;   /* P x m_cap */
    uint8_t* out_status;            /* P */
    double* out_rot_ref_to_cur;     /* P x 9 */
    double* out_trans_ref_to_cur;   /* P x 3 */
    int32_t* out_hypothesis;        /* P */
    int32_t* out_num_valid;         /* P x 8 */
    float* out_parallax_deg;        /* P x 8 */
    double* out_triangulated_pts;   /* P x n_cap x 3 */
    uint8_t* out_is_triangulated;   /* P x n_cap */
    uint8_t* out_hyp_is_triangulated;   /* P x 8 x n_cap, or NULL */
} plp_perspective_pose_args;
/* Checked before anything is written: as for plp_two_view_pose_args, with in_choice, H_21 and F_21 in the place of E_21, and the equirectangular
 * camera PLP_ERR_UNSUPPORTED.  _device: every array a DEVICE pointer; one kernel on hip_stream, no host synchronisation; the points and flags
 * of the hypotheses wait in buffers the context owns, so the calls of one context must be ordered on the device.  _host: HOST pointers,
 * staged, the same kernel, synchronous. */
plp_status plp_perspective_pose_device(plp_matcher* ctx, const plp_perspective_pose_args* args, void* hip_stream);
plp_status plp_perspective_pose_host(plp_matcher* ctx, const plp_perspective_pose_args* args);
/* Host builds (csrc/perspective_init.hpp), HOST pointers, no GPU and no context needed; -1 for a bad argument.
 * plp_model_perspective_pose_host: the entry above, one problem after the other; the same checks.  Returns P.
 * plp_model_homography_decompose_host: homography_solver::decompose of n matrices (n x 9) under the camera matrix cam_matrix (9, row-major,
 * of both frames): out_ok n (0 = it returned false, the poses then zero), out_rots n x 8 x 9, out_trans n x 8 x 3.  Returns n. */
int32_t plp_model_perspective_pose_host(const plp_perspective_pose_args* args);
int32_t plp_model_homography_decompose_host(const double* H_21, const double* cam_matrix, int32_t n, uint8_t* out_ok, double* out_rots, double* out_trans);

/* ------------------------------------------------------------------------------------------------------------------
 * Per-frame pose optimisation: optimize::pose_optimizer::optimize (src/PLPSLAM/optimize/pose_optimizer.cc:53-229) and
 * optimize::pose_optimizer_extended_line::optimize (optimize/pose_optimizer_extended_line.cc:62-305) for B frames at once, in slot form --
 * what the tracker runs after the last-frame match (module/frame_tracker.cc:83-96), after the local-map match (tracking_module.cc:750-759)
 * and up to three times per relocalisation candidate (module/relocalizer.cc:118, 164-168, 209-213).  l_cap == 0 is pose_optimizer, l_cap > 0
 * the extended optimiser.  Numeric contract: DESIGN.md section 5, D15 (the vertex, the edges, sin / cos, the order of the sums, the 6 x 6
 * Cholesky, g2o's Levenberg-Marquardt, what the reference leaves undefined); g2o is not linked.
 *
 * Slot = key point (key line) of the frame, [B][n_cap] ([B][l_cap]):
 *   valid        1 where frm.landmarks_.at(idx) is set and will not be erased                          :126-134 / :135-143
 *   undist       frm.undist_keypts_ (pt and octave are read)                                           :140-142
 *   x_right      frm.stereo_x_right_; NULL = every key point monocular (-1)                            :141
 *   pos_w        lm->get_pos_in_world()
 *   line_valid, keylines (startPoint, endPoint, octave), pos_w_lines (Pluecker, 6)                      pose_optimizer_extended_line.cc:173-202
 * A valid slot whose octave is outside [0, num_levels) (where inv_level_sigma_sq_.at() throws) is no observation: it is not counted and
 * its flag is left alone.  The edges are the perspective ones for PLP_CAMERA_PERSPECTIVE and PLP_CAMERA_FISHEYE
 * (pose_opt_edge_wrapper.h:127-217); PLP_CAMERA_EQUIRECTANGULAR is PLP_ERR_UNSUPPORTED (D15: its atan2 / asin cannot be held bit for bit).
 * An edge is two- or three-dimensional by x_right < 0 per key point; the Huber delta is sqrt(chi_sq_2D) for setup_type 0, else
 * sqrt(chi_sq_3D), per frame (:144), and sqrt(chi_sq_2D) for lines.
 * Outputs per frame:
 *   out_status        a plp_pose_opt_status
 *   out_pose          15 doubles: rot_cw (row-major), trans_cw, cam_center as frame::update_pose_params forms it; for
 *                     PLP_POSE_OPT_TOO_FEW_OBS the first 12 are the input's
 *   out_num_init_obs  num_init_obs
 *   out_num_valid     the function's return value, num_init_obs - num_bad_obs; 0 for PLP_POSE_OPT_TOO_FEW_OBS
 *   out_outlier       [B][n_cap]: frm.outlier_flags_; only observation slots are written
 *   out_outlier_lines [B][l_cap]: frm._outlier_flags_line; written only when num_init_obs >= 5 (:161-165), observation slots only
 *   out_trial_info    optional, [B][num_trials][4]: iterations run, rejected steps, num_bad_obs, why optimize() ended (1 all iterations,
 *                     2 the ten tries were used up, 3 rho == 0); a trial not run: 0 0 0 0
 *   out_trial_chi2    optional, [B][num_trials][2]: the robust chi2 of the kept estimate and lambda at the trial's end; not run: 0 0 */
typedef enum plp_pose_opt_status {
    PLP_POSE_OPT_OK = 0,
    PLP_POSE_OPT_TOO_FEW_OBS = 1     /* num_init_obs < 5: nothing optimised (:153 / :162) */
} plp_pose_opt_status;
typedef struct plp_pose_optimize_args {
    plp_camera_model camera;            /* model, fx, fy, cx, cy, focal_x_baseline are read */
    int32_t setup_type;                 /* camera::setup_type_t: 0 monocular, 1 stereo, 2 RGB-D */
    int32_t B, n_cap, l_cap;            /* B >= 0 frames; n_cap, l_cap in 0 .. 8192; l_cap == 0: no line edges */
    int32_t num_trials, num_each_iter;  /* >= 1; 4 and 10 by the constructors' defaults */
    int32_t pose_stride;                /* doubles between two rows of pose_in, >= 12 (15 for plp.frame_pose rows) */
    const float* inv_level_sigma_sq;    /* HOST, num_levels: frm.inv_level_sigma_sq_ */
    int32_t num_levels;                 /* 1 .. 16 */
    const float* inv_level_sigma_sq_lsd;/* HOST, num_levels_lsd: frm._inv_level_sigma_sq_lsd; may be NULL when l_cap == 0 */
    int32_t num_levels_lsd;             /* 1 .. 16 when l_cap > 0 */
    const double* pose_in;              /* B rows: rot_cw row-major (9), trans_cw (3); the rest of a row is not read */
    const int32_t* counts;              /* B: point slots in use, or NULL = n_cap */
    const int32_t* line_counts;         /* B: line slots in use, or NULL = l_cap */
    const uint8_t* valid;               /* B x n_cap */
    const plp_keypoint* undist;         /* B x n_cap */
    const float* x_right;               /* B x n_cap, or NULL */
    const double* pos_w;                /* B x n_cap x 3 */
    const uint8_t* line_valid;          /* B x l_cap */
    const plp_keyline* keylines;        /* B x l_cap */
    const double* pos_w_lines;          /* B x l_cap x 6 */
    uint8_t* out_status;                /* B */
    double* out_pose;                   /* B x 15 */
    int32_t* out_num_init_obs;          /* B */
    int32_t* out_num_valid;             /* B */
    uint8_t* out_outlier;               /* B x n_cap */
    uint8_t* out_outlier_lines;         /* B x l_cap */
    int32_t* out_trial_info;            /* B x num_trials x 4, or NULL */
    double* out_trial_chi2;             /* B x num_trials x 2, or NULL */
} plp_pose_optimize_args;
/* Checked before anything is written (PLP_ERR_INVALID_ARG): NULL ctx / args; an unknown camera model or setup_type; fx or fy 0; B, n_cap or
 * l_cap negative; num_trials or num_each_iter < 1; pose_stride < 12; num_levels outside 1 .. 16 or a NULL inv_level_sigma_sq; with l_cap > 0
 * num_levels_lsd outside 1 .. 16 or a NULL inv_level_sigma_sq_lsd; and -- when B > 0 -- a NULL pose_in, out_status, out_pose,
 * out_num_init_obs or out_num_valid, with n_cap > 0 a NULL valid, undist, pos_w or out_outlier, with l_cap > 0 a NULL line_valid, keylines,
 * pos_w_lines or out_outlier_lines.  The equirectangular camera, n_cap or l_cap > 8192, B > 65535: PLP_ERR_UNSUPPORTED.  B == 0: PLP_OK,
 * nothing written.
 * _device: every array but the two sigma tables a DEVICE pointer; two kernels on hip_stream, the whole trial loop inside the second, no host
 * synchronisation.  The kernels hand the ranks and the edges' last chi2 on through buffers the context owns, so the calls of one context must
 * be ordered on the device: one stream, or events between streams.  _host: HOST pointers, staged (the flag outputs too, so that every slot
 * the kernels do not write keeps the caller's value), the same kernels, synchronous. */
plp_status plp_pose_optimize_device(plp_matcher* ctx, const plp_pose_optimize_args* args, void* hip_stream);
plp_status plp_pose_optimize_host(plp_matcher* ctx, const plp_pose_optimize_args* args);
/* Host builds of the same source (csrc/pose_opt.hpp), HOST pointers, no GPU and no context needed.
 * plp_model_pose_optimize_host: the entry above, one frame and one edge after the other; the same checks.  Returns B, or the negated
 * plp_status of a refused call (-PLP_ERR_INVALID_ARG, -PLP_ERR_UNSUPPORTED; plp_last_error() names the reason).
 * plp_model_pose_linearize_host: one linearisation at the poses pose_in of the inputs in `args` (its outputs are not touched): the edges of
 * the observation slots whose `active` (B x n_cap; NULL = all) / `active_lines` (B x l_cap; NULL = all) byte is non-zero, Huber kernels on
 * (robust != 0) or off.  out_sums B x 28: H upper triangle row-major (21), b (6), robust chi2; out_chi2 B x n_cap and out_chi2_lines
 * B x l_cap (either may be NULL): the chi2 of every active edge, other slots keep their values.  Returns as the entry above.
 * plp_model_se3_exp_host: out = SE3Quat::exp(update) * est (shot_vertex::oplusImpl) for n pairs; update n x 6 (omega, upsilon), est and out
 * n x 7 (qx qy qz qw tx ty tz).
 * plp_model_chol6_host: (H + lambda I) x = b for n systems; H n x 21 (upper triangle row-major), b n x 6, lambda n, out_x n x 6, out_ok n
 * (0 = a pivot was not positive and finite; x is then zero).
 * plp_model_pose_sincos_host: D15's sin and cos of n doubles.  All three return n, or -1 for a bad argument. */
int32_t plp_model_pose_optimize_host(const plp_pose_optimize_args* args);
int32_t plp_model_pose_linearize_host(const plp_pose_optimize_args* args, int32_t robust, const uint8_t* active, const uint8_t* active_lines,
                                      double* out_sums, double* out_chi2, double* out_chi2_lines);
int32_t plp_model_se3_exp_host(const double* update, const double* est, int32_t n, double* out);
int32_t plp_model_chol6_host(const double* H, const double* b, const double* lambda, int32_t n, double* out_x, int32_t* out_ok);
int32_t plp_model_pose_sincos_host(const double* x, int32_t n, double* out_sin, double* out_cos);

/* ------------------------------------------------------------------------------------------------------------------
 * Sim3 refinement of loop candidates: optimize::transform_optimizer::optimize (src/PLPSLAM/optimize/transform_optimizer.cc:47-197) for P
 * problems at once, in slot form -- what loop_detector::select_loop_candidate_via_Sim3 runs per candidate between the mutual projection
 * match and its `num_optimized_inliers < 20` decision (module/loop_detector.cc:389-396).  A problem is one pair: the current key frame (1)
 * and a candidate (2).  Numeric contract: DESIGN.md section 5, D16 (the Sim3 vertex, exp, the two reprojection edges per match with g2o's
 * numeric Jacobian, the order of the sums, the 7 x 7 Cholesky, the two rounds) on top of D15; g2o is not linked.
 *
 * Slot = key point idx1 of key frame 1, [P][n_cap]:
 *   valid        1 where matched_lms_in_keyfrm_2.at(idx1) is set, lm_1 and lm_2 exist, neither will be erased and
 *                lm_2->get_index_in_keyframe(keyfrm_2) >= 0                                              :95-118
 *   pos_w_1/_2   lm_1 / lm_2 ->get_pos_in_world()
 *   undist_1/_2  keyfrm_1->undist_keypts_.at(idx1) / keyfrm_2->undist_keypts_.at(idx2) (pt and octave are read)
 * A valid slot with either octave outside [0, num_levels) (where inv_level_sigma_sq_.at() throws) is no observation: it is not counted and
 * its out_kept byte is left alone.  The edges are the perspective ones for PLP_CAMERA_PERSPECTIVE and PLP_CAMERA_FISHEYE
 * (mutual_reproj_edge_wrapper.h:106-256); PLP_CAMERA_EQUIRECTANGULAR is PLP_ERR_UNSUPPORTED (D15's reason).
 * Outputs per problem:
 *   out_status        a plp_transform_opt_status
 *   out_num_valid     num_valid_matches
 *   out_num_inliers   the function's return value; 0 for PLP_TRANSFORM_OPT_TOO_FEW_INLIERS
 *   out_rot_12 (9, row-major), out_trans_12 (3), out_scale_12 (double): g2o_Sim3_12 after the call; for
 *                     PLP_TRANSFORM_OPT_TOO_FEW_INLIERS the input's values (the Sim3 is not written back)
 *   out_world_to_1    optional, 13 doubles: g2o_Sim3_12 * Sim3(rot_2w, trans_2w, 1.0) as rot (9), trans (3), scale (loop_detector.cc:404),
 *                     formed from the returned Sim3 for either status
 *   out_kept          [P][n_cap]: 1 where matched_lms_in_keyfrm_2.at(idx1) is still set after the call (the drops of round 1 stand on the
 *                     early return); only observation slots are written
 *   out_round_info    optional, [P][2][4] per round: iterations run, rejected steps, matches dropped, why optimize() ended (1 all
 *                     iterations, 2 the ten tries were used up, 3 rho == 0); a round not run: 0 0 0 0
 *   out_round_chi2    optional, [P][2][2]: the robust chi2 of the kept estimate and lambda at the round's end; not run: 0 0 */
typedef enum plp_transform_opt_status {
    PLP_TRANSFORM_OPT_OK = 0,
    PLP_TRANSFORM_OPT_TOO_FEW_INLIERS = 1     /* fewer than 10 matches left after round 1 (:156), or no match at all */
} plp_transform_opt_status;
typedef struct plp_transform_optimize_args {
    plp_camera_model camera;            /* model, fx, fy, cx, cy are read; both key frames share it */
    int32_t fix_scale;                  /* transform_optimizer's fix_scale_ */
    int32_t num_iter;                   /* >= 1; 10 by the constructor's default */
    float chi_sq;                       /* > 0; 10 at loop_detector.cc:391 */
    int32_t P, n_cap;                   /* P >= 0 problems; n_cap in 0 .. 8192 */
    const float* inv_level_sigma_sq_1;  /* HOST, num_levels: keyfrm_1->inv_level_sigma_sq_ */
    const float* inv_level_sigma_sq_2;  /* HOST, num_levels: keyfrm_2->inv_level_sigma_sq_ */
    int32_t num_levels;                 /* 1 .. 16 */
    const int32_t* counts;              /* P: slots in use, or NULL = n_cap */
    const uint8_t* valid;               /* P x n_cap */
    const double* pos_w_1;              /* P x n_cap x 3 */
    const double* pos_w_2;              /* P x n_cap x 3 */
    const plp_keypoint* undist_1;       /* P x n_cap */
    const plp_keypoint* undist_2;       /* P x n_cap */
    const double* pose_1;               /* P rows of 15: rot_1w row-major (9), trans_1w (3); the rest is not read */
    const double* pose_2;               /* P rows of 15: rot_2w, trans_2w */
    const double* rot_12;               /* P x 9 */
    const double* trans_12;             /* P x 3 */
    const float* scale_12;              /* P: the solver's float (loop_detector.cc:382) */
    uint8_t* out_status;                /* P */
    int32_t* out_num_valid;             /* P */
    int32_t* out_num_inliers;           /* P */
    double* out_rot_12;                 /* P x 9 */
    double* out_trans_12;               /* P x 3 */
    double* out_scale_12;               /* P */
    double* out_world_to_1;             /* P x 13, or NULL */
    uint8_t* out_kept;                  /* P x n_cap */
    int32_t* out_round_info;            /* P x 2 x 4, or NULL */
    double* out_round_chi2;             /* P x 2 x 2, or NULL */
} plp_transform_optimize_args;
/* Checked before anything is written (PLP_ERR_INVALID_ARG): NULL ctx / args; an unknown camera model; fx or fy 0, or fx, fy, cx or cy not finite; P or
 * n_cap negative; num_iter < 1; chi_sq not positive; num_levels outside 1 .. 16 or a NULL sigma table; and -- when P > 0 -- a NULL pose_1, pose_2, rot_12,
 * trans_12, scale_12, out_status, out_num_valid, out_num_inliers, out_rot_12, out_trans_12 or out_scale_12, with n_cap > 0 a NULL valid,
 * pos_w_1, pos_w_2, undist_1, undist_2 or out_kept.  The equirectangular camera, n_cap > 8192, P > 65535: PLP_ERR_UNSUPPORTED.  P == 0:
 * PLP_OK, nothing written.
 * _device: every array but the two sigma tables a DEVICE pointer; three kernels on hip_stream, both rounds inside the second, no host
 * synchronisation.  The kernels hand the ranks, the edges' constants and last chi2 and the outcome on through buffers the context owns, so the calls of one context must
 * be ordered on the device: one stream, or events between streams.  _host: HOST pointers, staged (out_kept too, so that every slot the
 * kernels do not write keeps the caller's value), the same kernels, synchronous. */
plp_status plp_transform_optimize_device(plp_matcher* ctx, const plp_transform_optimize_args* args, void* hip_stream);
plp_status plp_transform_optimize_host(plp_matcher* ctx, const plp_transform_optimize_args* args);
/* Host builds of the same source (csrc/transform_opt.hpp), HOST pointers, no GPU and no context needed.
 * plp_model_transform_optimize_host: the entry above, one problem and one edge after the other; the same checks.  Returns P, or the negated
 * plp_status of a refused call.
 * plp_model_transform_linearize_host: one linearisation at the Sim3 of the inputs in `args` (its output pointers are neither written nor checked: they
 * may all be NULL; the checks of the inputs are the entry's): the two edges of
 * every observation slot whose `active` byte (P x n_cap; NULL = all) is non-zero.  out_sums P x 36: H upper triangle row-major (28), b (7),
 * robust chi2; out_chi2 P x n_cap x 2 (may be NULL): forward and backward chi2 of every active match, other slots keep their values.
 * plp_model_sim3_exp_host: out = Sim3(update) * est (transform_vertex::oplusImpl) for n pairs; update n x 7 (omega, upsilon, sigma), est and
 * out n x 8 (qx qy qz qw tx ty tz s); fix_scale != 0 takes sigma as 0.
 * plp_model_chol7_host: (H + lambda I) x = b for n systems; H n x 28 (upper triangle row-major), b n x 7, lambda n, out_x n x 7, out_ok n
 * (0 = a pivot was not positive and finite; x is then zero).
 * plp_model_pose_exp_host: D16's exp of n doubles (NaN outside [-700, 700]).  The last three return n, or -1 for a bad argument. */
int32_t plp_model_transform_optimize_host(const plp_transform_optimize_args* args);
int32_t plp_model_transform_linearize_host(const plp_transform_optimize_args* args, const uint8_t* active, double* out_sums, double* out_chi2);
int32_t plp_model_sim3_exp_host(const double* update, const double* est, int32_t fix_scale, int32_t n, double* out);
int32_t plp_model_chol7_host(const double* H, const double* b, const double* lambda, int32_t n, double* out_x, int32_t* out_ok);
int32_t plp_model_pose_exp_host(const double* x, int32_t n, double* out);

/* ------------------------------------------------------------------------------------------------------------------
 * Local bundle adjustment: optimize::local_bundle_adjuster::optimize (src/PLPSLAM/optimize/local_bundle_adjuster.cc:62-410) for G problems
 * at once over shared map tables -- what mapping_module runs for every new key frame (mapping_module.cc:251-261).  From the tables to the
 * optimised poses, positions and outlier observations without the host.  Numeric contract: DESIGN.md section 5, D17 (the sets, the orders,
 * the binary edge's two Jacobian blocks, the ordered sums, the Schur complement, the Cholesky of the reduced system, the two rounds) on top
 * of D15; g2o is not linked.  force_stop_flag is not modelled (NULL); covisibility selection is the caller's (kf_local).
 *
 * Key-frame table, F rows:
 *   pose          rot_cw row-major (9), trans_cw (3) per row; pose_stride doubles between rows
 *   kf_erased     keyframe::will_be_erased()                                                            :85, :139, :250
 *   kf_is_origin  id_ == 0: a local key frame that is held constant                                     :198
 *   undist        undist_keypts_ (pt and octave are read), kp_stride slots per row; x_right: stereo_x_right_, NULL = all monocular (-1)
 *   counts        key points per key frame, NULL = kp_stride
 * Landmark table, L rows, with the observation lists in the layout of plp_landmark_geometry_args:
 *   pos_w, lm_erased (will_be_erased(), :107), obs_offsets (L + 1), obs_kf, obs_idx (T = obs_offsets[L] entries)
 * Per problem: kf_local [G][F], the current key frame and the covisibilities the caller chose (:73-91).
 * Sets (:72-158): a key frame is local iff kf_local and not erased; a landmark is local iff not erased and a local key frame is among its
 * observations; a key frame is fixed iff it is not local, not erased and observes a local landmark.  One edge per observation of a local
 * landmark by a key frame that is not erased; an observation whose obs_kf is outside [0, F), whose obs_idx is outside [0, counts[kf]) or
 * whose octave is outside [0, num_levels) is not an edge (where the reference follows a null pointer or .at() throws).  Order: key frames
 * and landmarks in table order, edges in landmark order, then list order (a declared deviation: the reference's orders come from
 * unordered_map iteration).
 * Outputs per problem; slots that are not written keep the caller's values:
 *   out_status      a plp_local_ba_status
 *   out_kf_role     [G][F] a plp_local_ba_kf_role; out_lm_role [G][L]: 1 = local
 *   out_pose        [G][F][15]: set_cam_pose's result as plp_pose_optimize_args.out_pose, for PLP_LOCAL_BA_KF_FREE rows only
 *   out_pos_w       [G][L][3]: local landmarks only
 *   out_outlier     [G][T]: step [7]'s verdict (:345-369), one byte per observation entry, edges only
 *   out_round_info  optional, [G][2][4] per round: iterations run, rejected steps, edges moved to level 1 (round 1 only), why optimize()
 *                   ended (1 all iterations, 2 the ten tries were used up, 3 rho == 0; 0 = the round had no level-0 edge)
 *   out_round_chi2  optional, [G][2][2]: the robust chi2 of the kept estimate and lambda at the round's end */
typedef enum plp_local_ba_status {
    PLP_LOCAL_BA_OK = 0,
    PLP_LOCAL_BA_NO_EDGES = 1,        /* nothing to optimise: out_pose is the input's (with its cam_center), out_pos_w the input's            */
    PLP_LOCAL_BA_TOO_MANY_FREE = 2    /* _device only: more than 64 free key frames; nothing but out_status is written for the problem       */
} plp_local_ba_status;
typedef enum plp_local_ba_kf_role {
    PLP_LOCAL_BA_KF_NONE = 0,
    PLP_LOCAL_BA_KF_FREE = 1,         /* local and optimised                                                                                 */
    PLP_LOCAL_BA_KF_ORIGIN = 2,       /* local with kf_is_origin: a constant vertex                                                          */
    PLP_LOCAL_BA_KF_FIXED = 3         /* observes a local landmark: a constant vertex                                                        */
} plp_local_ba_kf_role;
typedef struct plp_local_ba_args {
    plp_camera_model camera;            /* model, fx, fy, cx, cy, focal_x_baseline are read */
    int32_t setup_type;                 /* camera::setup_type_t: 0 monocular, 1 stereo, 2 RGB-D: the Huber delta (:259-261) */
    int32_t num_first_iter, num_second_iter;   /* >= 1; 5 and 10 by the constructor's defaults */
    int32_t G, F, L, T;                 /* G >= 0 problems; F <= 1024 key frames; L, T <= 2^18; G <= 256, G * T and G * L <= 2^22 */
    int32_t kp_stride, pose_stride;     /* slots between two rows of undist / x_right; doubles between two pose rows, >= 12 */
    const float* inv_level_sigma_sq;    /* HOST, num_levels */
    int32_t num_levels;                 /* 1 .. 16 */
    const double* pose;                 /* F rows */
    const uint8_t* kf_erased;           /* F, or NULL = none */
    const uint8_t* kf_is_origin;        /* F, or NULL = none */
    const plp_keypoint* undist;         /* F x kp_stride */
    const float* x_right;               /* F x kp_stride, or NULL */
    const int32_t* counts;              /* F, or NULL */
    const double* pos_w;                /* L x 3 */
    const uint8_t* lm_erased;           /* L, or NULL = none */
    const int32_t* obs_offsets;         /* L + 1 */
    const int32_t* obs_kf;              /* T */
    const int32_t* obs_idx;             /* T */
    const uint8_t* kf_local;            /* G x F */
    uint8_t* out_status;                /* G */
    uint8_t* out_kf_role;               /* G x F */
    uint8_t* out_lm_role;               /* G x L */
    double* out_pose;                   /* G x F x 15 */
    double* out_pos_w;                  /* G x L x 3 */
    uint8_t* out_outlier;               /* G x T */
    int32_t* out_round_info;            /* G x 2 x 4, or NULL */
    double* out_round_chi2;             /* G x 2 x 2, or NULL */
} plp_local_ba_args;
/* Checked before anything is written (PLP_ERR_INVALID_ARG): NULL ctx / args; an unknown camera model or setup_type; fx or fy 0 or a
 * non-finite fx, fy, cx, cy; G, F, L, T or kp_stride negative; an iteration count < 1; pose_stride < 12; num_levels outside 1 .. 16 or a
 * NULL sigma table; and -- when G > 0 -- a NULL kf_local (F > 0), pose, undist (F > 0 and kp_stride > 0), pos_w (L > 0), obs_offsets,
 * obs_kf, obs_idx (T > 0) or a NULL required output of non-zero size.  The equirectangular camera, F > 1024, L or T > 2^18, G > 256,
 * G * T or G * L > 2^22: PLP_ERR_UNSUPPORTED (the context holds G (78 T + 25 L + 14 F + 384^2) doubles of state between the kernels).  G == 0: PLP_OK, nothing written.  _host and the host builds also check that obs_offsets rises from 0 to
 * T (PLP_ERR_INVALID_ARG) and that no problem has more than 64 free key frames (PLP_ERR_UNSUPPORTED), before anything is written; on the
 * _device path the first is a precondition (the kernels cut every run to the list) and the second a per-problem status.
 * _device: every array but the sigma table a DEVICE pointer; three kernels on hip_stream (the sets and edges; both rounds; the outputs), one
 * workgroup per problem, no host synchronisation.  The kernels hand their state on through buffers the context owns, so the calls of one
 * context must be ordered on the device: one stream, or events between streams.  _host: HOST pointers, staged (the outputs too, so that
 * every slot the kernels do not write keeps the caller's value), the same kernels, synchronous. */
plp_status plp_local_ba_device(plp_matcher* ctx, const plp_local_ba_args* args, void* hip_stream);
plp_status plp_local_ba_host(plp_matcher* ctx, const plp_local_ba_args* args);
/* Host builds of the same source (csrc/local_ba.hpp), HOST pointers, no GPU and no context needed.
 * plp_model_local_ba_host: the entry above with a team of one lane; the same checks.  Returns G, or the negated plp_status of a refused call.
 * plp_model_local_ba_linearize_host: one linearisation of problem 0 (G must be 1) at the inputs' estimates with every edge at level 0, Huber
 * kernels on (robust != 0) or off; the output pointers of `args` are neither read nor checked.  out_free_kf [64]: the table rows of the
 * active free key frames in order (-1 behind them); out_hpp [64][27]: every active pose's H upper triangle row-major (21) and b (6);
 * out_hll [L][9]: every active landmark's H (00 01 02 11 12 22) and b (3); out_w [T][18]: H_pl of every edge with an active free pose, 6 x 3
 * row-major; out_chi2 [1]: the robust chi2; out_edge_chi2 [T]: the chi2 of every edge.  Slots without a value keep the caller's.  Any of
 * them may be NULL.  Returns the number of active free poses, or the negated status.
 * plp_model_local_ba_solve_host: one damped Schur solve from given blocks: P <= 64 poses (hpp P x 27 as above), M landmarks (hll M x 9),
 * E edges in landmark order with e_pose (0 .. P - 1, or -1 for a constant pose), e_lm (non-decreasing, 0 .. M - 1) and w (E x 18).  A pose
 * or a landmark without an edge is not in the system (its x is 0).  out_xp P x 6, out_xl M x 3; returns 1 = solved, 0 = a pivot or a
 * 3 x 3 inverse failed (every x is then 0), -1 = a bad argument.
 * plp_model_inv3_host: the closed cofactor inverse of n symmetric 3 x 3 matrices (n x 6: 00 01 02 11 12 22), out n x 6, out_ok n
 * (0 = a coefficient of the inverse is not finite).  Returns n, or -1. */
int32_t plp_model_local_ba_host(const plp_local_ba_args* args);
int32_t plp_model_local_ba_linearize_host(const plp_local_ba_args* args, int32_t robust, int32_t* out_free_kf, double* out_hpp, double* out_hll,
                                          double* out_w, double* out_chi2, double* out_edge_chi2);
int32_t plp_model_local_ba_solve_host(int32_t P, int32_t M, int32_t E, const double* hpp, const double* hll, const int32_t* e_pose,
                                      const int32_t* e_lm, const double* w, double lambda, double* out_xp, double* out_xl);
int32_t plp_model_inv3_host(const double* a, int32_t n, double* out, int32_t* out_ok);

/* ------------------------------------------------------------------------------------------------------------------
 * Local bundle adjustment with line landmarks: optimize::local_bundle_adjuster_extended_line::optimize
 * (src/PLPSLAM/optimize/local_bundle_adjuster_extended_line.cc:70-674) for G problems at once over shared map tables -- what mapping_module runs
 * for every new key frame when line tracking is on (mapping_module.cc:252-257).  Numeric contract: DESIGN.md section 5, D28, on top of D17 and
 * D15: the 4-DoF line vertex in orthonormal representation (g2o/line3d.h:137-186), the binary line edge with g2o's numeric Jacobian on both
 * vertices (g2o/se3/reproj_edge_line3d_orthonormal.h:60-88), 4 x 4 marginalised blocks beside the 3 x 3 ones, and the line half of the outlier
 * schedule with the end-point depth test (:97-177 of the same file; :486-505, :555-573 of the adjuster).  g2o is not linked; force_stop_flag is
 * not modelled; step [8]'s map mutation (erase_landmark_line, erase_observation, prepare_for_erasing) stays with the caller.
 *
 * `points` is a whole plp_local_ba_args and every field means what it means there; L and T may be 0.  The line table, LL rows, uses the
 * observation-list layout of the landmarks: pluecker (get_PlueckerCoord(), moment then direction), line_erased (will_be_erased(), :371),
 * obs_offsets_lines (LL + 1), obs_kf_lines, obs_idx_lines (TL entries).  keylines is the key frames' _keylsd, kl_stride slots per key-frame row
 * (start point, end point and octave are read), kl_counts the key lines per key frame (NULL = kl_stride).
 * Sets (:108-224): a line is local iff not erased and a local key frame is among its observations; a key frame is fixed iff it is not local, not
 * erased and among the observations of a local landmark or a local line.  One line edge per observation of a local line by a key frame that is
 * not erased; an observation whose obs_kf_lines is outside [0, F), whose obs_idx_lines is outside [0, kl_counts[kf]) or whose octave is outside
 * [0, num_levels_lsd) is not an edge.  Order: key frames, landmarks, lines in table order; point edges before line edges; line edges in line
 * order, then list order.
 * Outputs per problem beside those of `points`; slots that are not written keep the caller's values:
 *   out_line_role      [G][LL]: 1 = local
 *   out_pluecker       [G][LL][6]: local lines only
 *   out_outlier_lines  [G][TL]: step [7]'s verdict (:555-573), one byte per observation entry, edges only
 * points.out_round_info[.][0][2] counts the point and the line edges moved to level 1 together.  A problem with neither a point nor a line edge
 * is PLP_LOCAL_BA_NO_EDGES (out_pluecker the input's). */
typedef struct plp_local_ba_lines_args {
    plp_local_ba_args points;             /* every field as the point adjuster reads it; L and T may be 0 */
    int32_t LL, TL;                       /* line landmarks, entries of their observation list; <= 2^18 each, G * TL and G * LL <= 2^22 */
    int32_t kl_stride, num_levels_lsd;    /* key-line slots per key-frame row; 1 .. 16 */
    const float* inv_level_sigma_sq_lsd;  /* HOST, num_levels_lsd: keyframe::_inv_level_sigma_sq_lsd */
    const plp_keyline* keylines;          /* F x kl_stride: _keylsd; start point, end point and octave are read */
    const int32_t* kl_counts;             /* F, or NULL = kl_stride */
    const double* pluecker;               /* LL x 6 (m, d): get_PlueckerCoord() */
    const uint8_t* line_erased;           /* LL, or NULL */
    const int32_t* obs_offsets_lines;     /* LL + 1 */
    const int32_t* obs_kf_lines;          /* TL */
    const int32_t* obs_idx_lines;         /* TL */
    uint8_t* out_line_role;               /* G x LL: 1 = local */
    double* out_pluecker;                 /* G x LL x 6: local lines only */
    uint8_t* out_outlier_lines;           /* G x TL: step [7]'s verdict, edges only */
} plp_local_ba_lines_args;
/* Checked before anything is written: everything the point adjuster checks of `points`, with its status codes; LL, TL or kl_stride negative,
 * num_levels_lsd outside 1 .. 16 or a NULL lsd sigma table, and -- when G > 0 -- a NULL obs_offsets_lines, pluecker (LL > 0), obs_kf_lines,
 * obs_idx_lines (TL > 0), keylines (F > 0 and kl_stride > 0) or a NULL required output of non-zero size: PLP_ERR_INVALID_ARG.  LL or TL > 2^18,
 * G * TL or G * LL > 2^22: PLP_ERR_UNSUPPORTED (the context holds G (96 TL + 89 LL + 5376) more doubles than the point adjuster's state).
 * _host and the host build also check that obs_offsets_lines rises from 0 to TL.  _device: every array but the two sigma tables a DEVICE
 * pointer; four kernels on hip_stream (the sets and edges; one per round; the outputs), one workgroup of 512 per problem, no host
 * synchronisation; the state lives in the context's buffers, so
 * the calls of one context must be ordered on the device.  _host: HOST pointers, staged (the outputs too), the same kernels, synchronous. */
plp_status plp_local_ba_lines_device(plp_matcher* ctx, const plp_local_ba_lines_args* args, void* hip_stream);
plp_status plp_local_ba_lines_host(plp_matcher* ctx, const plp_local_ba_lines_args* args);
/* Host builds of the same source (csrc/local_ba_lines.hpp), HOST pointers, no GPU and no context needed.
 * plp_model_local_ba_lines_host: the entry above with a team of one lane; the same checks.  Returns G, or the negated plp_status.
 * plp_model_line_oplus_host: Line3D::oplus for n lines: line n x 6, update n x 4 (the quaternion's vector part, the angle), out n x 6.  Returns n or -1.
 * plp_model_local_ba_lines_linearize_host: one linearisation of problem 0 (G must be 1) at the inputs' estimates with every edge at level 0; the
 * output pointers of `args` are neither read nor checked.  out_free_kf [64], out_hpp [64][27], out_hll [L][9], out_chi2 [1] as the point
 * adjuster's linearize build gives them, the sums running over the line edges too; out_hnn [LL][14]: every active line's H (upper triangle
 * row-major, 10) and b (4); out_w_lines [TL][24]: H_pl of every line edge with an active free pose, 6 x 4 row-major; out_edge_chi2_lines [TL].
 * Slots without a value keep the caller's; any may be NULL.  Returns the number of active free poses, or the negated status.
 * plp_model_local_ba_lines_solve_host: one damped Schur solve from given blocks with mixed 3- and 4-blocks: P <= 64 poses (hpp P x 27),
 * M landmarks (hll M x 9), N lines (hnn N x 14), E3 point edges in landmark order (e_pose, e_lm, w E3 x 18) and E4 line edges in line order
 * (e_pose_lines, e_line, w_lines E4 x 24); -1 in e_pose / e_pose_lines is a constant pose.  out_xp P x 6, out_xl M x 3, out_xn N x 4; returns
 * 1 = solved, 0 = a pivot or an inverse failed (every x is then 0), -1 = a bad argument. */
int32_t plp_model_local_ba_lines_host(const plp_local_ba_lines_args* args);
int32_t plp_model_line_oplus_host(const double* line, const double* update, int32_t n, double* out);
int32_t plp_model_local_ba_lines_linearize_host(const plp_local_ba_lines_args* args, int32_t robust, int32_t* out_free_kf, double* out_hpp,
                                                double* out_hll, double* out_hnn, double* out_w_lines, double* out_chi2,
                                                double* out_edge_chi2_lines);
int32_t plp_model_local_ba_lines_solve_host(int32_t P, int32_t M, int32_t N, int32_t E3, int32_t E4, const double* hpp, const double* hll,
                                            const double* hnn, const int32_t* e_pose, const int32_t* e_lm, const double* w,
                                            const int32_t* e_pose_lines, const int32_t* e_line, const double* w_lines, double lambda,
                                            double* out_xp, double* out_xl, double* out_xn);

/* ------------------------------------------------------------------------------------------------------------------
 * Global bundle adjustment: optimize::global_bundle_adjuster::optimize (src/PLPSLAM/optimize/global_bundle_adjuster.cc:64-311) over the whole
 * point map -- what module::loop_bundle_adjuster::optimize runs after a loop closure (Huber off) and module::initializer on its first two key
 * frames (Huber on) -- and the array half of the loop adjuster's map update (module/loop_bundle_adjuster.cc:109-181).  Numeric contract:
 * DESIGN.md section 5, D23, on top of D17 and D15; g2o is not linked.  ONE problem per call; the problem uses the whole device.
 *
 * The key-frame and landmark tables are plp_local_ba_args', field for field.  Sets (:91-184): every key frame that is not erased is a vertex,
 * kf_is_origin makes it constant; every landmark that is not erased and has an edge is a vertex; one edge per observation of such a landmark
 * by a key frame that is not erased, with D17's rules for what is no edge.  There is no kf_local, no fixed key frame, no level and one
 * optimize(num_iter); the Huber kernel is on or off for the whole run.
 * Outputs; slots that are not written keep the caller's values:
 *   out_status        [1] a plp_global_ba_status
 *   out_kf_optimized  [F] 1 = the key frame is not erased (a vertex); out_lm_optimized [L] 1 = the landmark has an edge
 *   out_pose          [F][15]: set_cam_pose's form, for EVERY key frame that is not erased (the origin and a key frame without an edge get the
 *                     converted input)
 *   out_pos_w         [L][3]: optimised landmarks only
 *   out_info          optional [4]: iterations, rejected steps, factorisations, why optimize() ended (plp_local_ba_args.out_round_info's code)
 *   out_chi2          optional [3]: the chi2 of the first linearisation, the chi2 of the kept estimate, lambda
 * stop: optional HOST flag (force_stop_flag), read before every iteration and before every try; if it is set when the run ends the status is
 * PLP_GLOBAL_BA_STOPPED and nothing else is written.  The host builds read it once, as a constant. */
#define PLP_GLOBAL_BA_MAX_KF 4096
#define PLP_GLOBAL_BA_PANEL 32          /* columns of a panel of the dense Cholesky of the reduced system (n = 6 P rows)               */
#define PLP_GLOBAL_BA_ROWS 64           /* rows of a workgroup of the launch that computes a panel's rows below the diagonal block     */
typedef enum plp_global_ba_status {
    PLP_GLOBAL_BA_OK = 0,
    PLP_GLOBAL_BA_NO_EDGES = 1,         /* nothing to optimise: out_pose is the input's (with its cam_center), no landmark is written  */
    PLP_GLOBAL_BA_STOPPED = 2           /* `stop` was set: nothing but out_status is written                                           */
} plp_global_ba_status;
typedef struct plp_global_ba_args {
    plp_camera_model camera;            /* model, fx, fy, cx, cy, focal_x_baseline are read */
    int32_t setup_type;                 /* 0 monocular, 1 stereo, 2 RGB-D: the Huber delta */
    int32_t num_iter;                   /* >= 1; 10 by the constructor's default */
    int32_t use_huber_kernel;           /* 0 / 1 */
    int32_t F, L, T;                    /* F <= 4096 key frames, L <= 2^20 landmarks, T <= 2^22 observations */
    int32_t kp_stride, pose_stride;
    const float* inv_level_sigma_sq;    /* HOST, num_levels */
    int32_t num_levels;                 /* 1 .. 16 */
    const double* pose;                 /* F rows */
    const uint8_t* kf_erased;           /* F, or NULL = none */
    const uint8_t* kf_is_origin;        /* F, or NULL = none */
    const plp_keypoint* undist;         /* F x kp_stride */
    const float* x_right;               /* F x kp_stride, or NULL */
    const int32_t* counts;              /* F, or NULL */
    const double* pos_w;                /* L x 3 */
    const uint8_t* lm_erased;           /* L, or NULL = none */
    const int32_t* obs_offsets;         /* L + 1 */
    const int32_t* obs_kf;              /* T */
    const int32_t* obs_idx;             /* T */
    const volatile int32_t* stop;       /* HOST, or NULL */
    uint8_t* out_status;                /* 1 */
    uint8_t* out_kf_optimized;          /* F */
    uint8_t* out_lm_optimized;          /* L */
    double* out_pose;                   /* F x 15 */
    double* out_pos_w;                  /* L x 3 */
    int32_t* out_info;                  /* 4, or NULL */
    double* out_chi2;                   /* 3, or NULL */
} plp_global_ba_args;
/* Checked before anything is written, as plp_local_ba_*: PLP_ERR_INVALID_ARG for NULL ctx / args, an unknown camera model or setup_type, fx or
 * fy 0 or a non-finite fx, fy, cx, cy, a negative F, L, T or kp_stride, num_iter < 1, pose_stride < 12, num_levels outside 1 .. 16 or a NULL
 * sigma table, a NULL obs_offsets, pose (F > 0), undist (F > 0 and kp_stride > 0), pos_w (L > 0), obs_kf or obs_idx (T > 0), a NULL required
 * output of non-zero size; PLP_ERR_UNSUPPORTED for the equirectangular camera (D15's reason), F > 4096, L > 2^20, T > 2^22.  _host and the
 * host builds also check that obs_offsets rises from 0 to T.
 * _device: every array but the sigma table and `stop` a DEVICE pointer.  Separate launches on hip_stream, phase by phase (the sets and edges;
 * per linearisation the edge pass and the sums; per try the 3 x 3 inverses, the Schur complement with one wave per free key frame, the dense
 * Cholesky panel by panel -- one launch for a panel's diagonal block, one over all workgroups for the rows below it --, the substitutions,
 * the update and the evaluation); no workgroup ever waits for another.  The entry reads the run's record back after the prepare launches
 * (to size the reduced system, which it allocates in the context) and after every try: plp_global_ba_device is SYNCHRONOUS with respect to
 * hip_stream, the only _device entry that is; it returns when the outputs are written.  The state lives in the context: one call at a time.
 * _host: HOST pointers, staged, the same kernels. */
plp_status plp_global_ba_device(plp_matcher* ctx, const plp_global_ba_args* args, void* hip_stream);
plp_status plp_global_ba_host(plp_matcher* ctx, const plp_global_ba_args* args);

/* The loop adjuster's map update after the global adjustment (module/loop_bundle_adjuster.cc:109-181), its array half: the correction is carried
 * along the spanning tree (kf_parent, -1 = none) from the origin to the key frames the adjuster did not optimise (created in the meantime):
 * after(c) = (pose(c) * pose_inv(p)) * after(p), p the parent, pose_inv as set_cam_pose stores it, after(p) the adjuster's pose_after [F][15] or
 * the same rule one step up; then every landmark moves: an optimised one to pos_after, any other one that is not erased with its reference key
 * frame, rot_wc_after (rot_before pos + t_before) + t_wc_after.  Every walk is bounded by F steps; no loop depends on kf_parent being a tree.
 *   out_kf_status  [F] a plp_loop_ba_kf_status; out_pose [F][15] and out_pose_before [F][12] for OPTIMIZED and PROPAGATED rows only
 *   out_lm_status  [L] a plp_loop_ba_lm_status; out_pos_w [L][3] for OPTIMIZED and MOVED rows only */
typedef enum plp_loop_ba_kf_status {
    PLP_LOOP_BA_KF_NOT_REACHED = 0,     /* the parent chain does not end at the origin within F steps (a broken link, an erased key frame, a cycle), or nothing on it was optimised */
    PLP_LOOP_BA_KF_OPTIMIZED = 1,       /* reached, kf_optimized: pose_after                                                           */
    PLP_LOOP_BA_KF_PROPAGATED = 2,      /* reached, not optimised: the correction of its nearest optimised ancestor                    */
    PLP_LOOP_BA_KF_ERASED = 3
} plp_loop_ba_kf_status;
typedef enum plp_loop_ba_lm_status {
    PLP_LOOP_BA_LM_NO_REF = 0,          /* not optimised and its reference key frame is outside the table or not reached (the reference's assert) */
    PLP_LOOP_BA_LM_OPTIMIZED = 1,
    PLP_LOOP_BA_LM_MOVED = 2,
    PLP_LOOP_BA_LM_ERASED = 3
} plp_loop_ba_lm_status;
typedef struct plp_loop_ba_propagate_args {
    int32_t F, L, pose_stride;          /* F <= 4096, L <= 2^20, pose_stride >= 12 */
    const double* pose;                 /* F rows: the poses BEFORE the correction */
    const uint8_t* kf_erased;           /* F, or NULL */
    const uint8_t* kf_is_origin;        /* F, or NULL */
    const int32_t* kf_parent;           /* F */
    const uint8_t* kf_optimized;        /* F: plp_global_ba_args.out_kf_optimized */
    const double* pose_after;           /* F x 15: plp_global_ba_args.out_pose */
    const double* pos_w;                /* L x 3 */
    const uint8_t* lm_erased;           /* L, or NULL */
    const int32_t* ref_kf;              /* L */
    const uint8_t* lm_optimized;        /* L */
    const double* pos_after;            /* L x 3 */
    double* out_pose;                   /* F x 15 */
    double* out_pose_before;            /* F x 12 */
    uint8_t* out_kf_status;             /* F */
    double* out_pos_w;                  /* L x 3 */
    uint8_t* out_lm_status;             /* L */
} plp_loop_ba_propagate_args;
/* PLP_ERR_INVALID_ARG: NULL ctx / args, negative F or L, pose_stride < 12, a NULL array of non-zero size other than kf_erased, kf_is_origin,
 * lm_erased; PLP_ERR_UNSUPPORTED above the caps.  _device: DEVICE pointers, two kernels (one lane per key frame, one per landmark), no host
 * synchronisation.  _host: HOST pointers, staged. */
plp_status plp_loop_ba_propagate_device(plp_matcher* ctx, const plp_loop_ba_propagate_args* args, void* hip_stream);
plp_status plp_loop_ba_propagate_host(plp_matcher* ctx, const plp_loop_ba_propagate_args* args);
/* Host builds of the same source (csrc/global_ba.hpp), HOST pointers, no GPU and no context needed.  plp_model_global_ba_host and
 * plp_model_loop_ba_propagate_host: the entries above; return 1, or the negated plp_status of a refused call.
 * plp_model_chol_dense_host: (A + lambda I) x = b for one dense symmetric system of any n >= 0 (A n x n row-major, its upper triangle is read):
 * the Cholesky in natural order and both substitutions of D23.  out_x n, out_ok 1 (0 = a pivot was not positive and finite; x is then zero).
 * Returns n, or -1 for a bad argument. */
int32_t plp_model_global_ba_host(const plp_global_ba_args* args);
int32_t plp_model_loop_ba_propagate_host(const plp_loop_ba_propagate_args* args);
int32_t plp_model_chol_dense_host(int32_t n, const double* A, const double* b, double lambda, double* out_x, int32_t* out_ok);
/* the same system through the panel kernels of plp_global_ba_device (HOST pointers, staged, synchronous): what tests compare the two forms with */
plp_status plp_chol_dense_host(plp_matcher* ctx, int32_t n, const double* A, const double* b, double lambda, double* out_x, int32_t* out_ok);

/* ------------------------------------------------------------------------------------------------------------------
 * The local map of B frames over one map snapshot: module::local_map_updater (src/PLPSLAM/module/local_map_updater.cc:60-273) as
 * tracking_module::update_local_map runs it (tracking_module.cc:837-906), and the landmarks search_local_landmarks[_line] skips because the
 * frame holds them (tracking_module.cc:911-946).  Integers only; contract: DESIGN.md section 5, D18 (the literal parts, and the orders
 * the reference leaves to an unordered_map and a std::set of pointers, which D18 defines: ascending key-frame row, the caller's child order).
 *
 * Map snapshot, shared by the B frames:
 *   kf_erased            keyframe::will_be_erased()                                                       local_map_updater.cc:122, :156
 *   kf_covis             [F][10] graph_node_->get_top_n_covisibilities(10) in its order, -1 behind the last              :179
 *   kf_parent            [F] get_spanning_parent(), -1 = none                                                            :199
 *   kf_children_offsets  [F + 1] into kf_children [C]: get_spanning_children() in the caller's order                     :189
 *   kf_lm                [F][cap] keyfrm->get_landmarks(): the landmark row of key point idx, -1 = none                  :213
 *   kf_counts            [F] key points per key frame, NULL = cap
 *   kf_lm_lines          [F][lcap] keyfrm->get_landmarks_line(), with kf_kl_counts; NULL = _b_use_line_tracking is off   :248, tracking_module.cc:898
 *   obs_offsets, obs_kf  lm->get_observations() in plp_landmark_geometry_args' layout; the key-frame rows only        :101-105
 *   lm_erased            [L] landmark::will_be_erased(), NULL = none; lm_erased_lines [LL] likewise       :221, :256, tracking_module.cc:847, :864
 * Per frame:
 *   frm_lm               [B][frm_stride] curr_frm_.landmarks_ as landmark rows, -1 = none; fcap slots of a row are read  :33, :94-100
 *   frm_counts           [B] num_keypts_, NULL = fcap                                                                    :34
 *   frm_lm_lines         [B][frm_stride_lines] curr_frm_._landmarks_line, flcap slots read, with frm_kl_counts; NULL = the frame holds no line
 * A row outside its table (frm_lm, kf_lm, obs_kf, kf_covis, kf_parent, kf_children and the line tables) counts as absent; a count is cut to
 * [0, its cap]; an observation run is cut to [0, T].
 * Outputs per frame; slots that are not written keep the caller's values:
 *   out_status        a plp_local_map_status
 *   out_num_first     first local key frames (:110-141); out_num_kf: first + second (:84-85), the true length even above k_cap
 *   out_local_kf      [B][k_cap] the local key frames in order, rows [0, min(out_num_kf, k_cap))
 *   out_first_weight  optional, [B][k_cap]: the weight of a first local key frame (:104), 0 for a second one
 *   out_nearest_kf    nearest_covisibility_ (:133-137), -1 = none (no key frame voted, or every one that did is erased)
 *   out_num_lm        local landmarks (:206-238), the true length even above m_cap; 0 after PLP_LOCAL_MAP_KF_OVERFLOW
 *   out_local_lm      [B][m_cap] rows [0, min(out_num_lm, m_cap)); out_held [B][m_cap]: 1 = a non-empty slot of the frame holds the landmark
 *                     (identifier_in_local_lm_search_ == curr_frm_.id_, tracking_module.cc:925, :939)
 *   out_num_lines, out_local_lines [B][ml_cap], out_held_lines [B][ml_cap]: the same for lines (:241-273, tracking_module.cc:994-1011),
 *                     written only when kf_lm_lines is given */
typedef enum plp_local_map_status {
    PLP_LOCAL_MAP_OK = 0,
    PLP_LOCAL_MAP_NO_KEYFRAMES = 1,   /* no weight at all: acquire_local_map() returns false (:78-81) and the tracker keeps its previous local map; every
                                         count is 0, out_nearest_kf -1, no list row is written                                                        */
    PLP_LOCAL_MAP_KF_OVERFLOW = 2,    /* out_num_kf > k_cap: rows [0, k_cap) of out_local_kf are written, the landmark lists are not (their counts are 0) */
    PLP_LOCAL_MAP_LM_OVERFLOW = 3,    /* out_num_lm > m_cap: rows [0, m_cap) are written; the line list is complete unless it overflows too               */
    PLP_LOCAL_MAP_LINE_OVERFLOW = 4   /* out_num_lines > ml_cap (and the point list fits): rows [0, ml_cap) are written                                   */
} plp_local_map_status;
typedef struct plp_local_map_args {
    int32_t B, F, C, L, LL, T;          /* B <= 65535 frames; F <= 8192 key frames (the weights of a frame are an LDS table); C children entries; L, LL landmark rows; T observation entries */
    int32_t cap, lcap;                  /* slots per row of kf_lm / kf_lm_lines, <= 8192 */
    int32_t fcap, flcap;                /* slots read per row of frm_lm / frm_lm_lines, <= 8192 */
    int32_t frm_stride, frm_stride_lines;   /* slots between two rows of frm_lm / frm_lm_lines; 0 = fcap / flcap */
    int32_t max_num_local_keyfrms;      /* tracking_module.cc:873 passes 60 */
    int32_t k_cap, m_cap, ml_cap;       /* rows per frame of the three output lists; k_cap * max(cap, lcap) < 2^31 */
    int64_t workspace_bytes;            /* the mark table (L + L / 32 words per frame, LL likewise) is kept for as many frames at a time as fit this
                                           many bytes, at least one; 0 = 256 MiB.  The frames are done in chunks of that many. */
    const uint8_t* kf_erased;           /* F, or NULL = none */
    const int32_t* kf_covis;            /* F x 10 */
    const int32_t* kf_parent;           /* F */
    const int32_t* kf_children_offsets; /* F + 1 */
    const int32_t* kf_children;         /* C */
    const int32_t* kf_lm;               /* F x cap */
    const int32_t* kf_counts;           /* F, or NULL */
    const int32_t* kf_lm_lines;         /* F x lcap, or NULL = no lines */
    const int32_t* kf_kl_counts;        /* F, or NULL */
    const int32_t* obs_offsets;         /* L + 1 */
    const int32_t* obs_kf;              /* T */
    const uint8_t* lm_erased;           /* L, or NULL = none */
    const uint8_t* lm_erased_lines;     /* LL, or NULL = none */
    const int32_t* frm_lm;              /* B x frm_stride */
    const int32_t* frm_counts;          /* B, or NULL */
    const int32_t* frm_lm_lines;        /* B x frm_stride_lines, or NULL */
    const int32_t* frm_kl_counts;       /* B, or NULL */
    uint8_t* out_status;                /* B */
    int32_t* out_num_first;             /* B */
    int32_t* out_num_kf;                /* B */
    int32_t* out_local_kf;              /* B x k_cap */
    int32_t* out_first_weight;          /* B x k_cap, or NULL */
    int32_t* out_nearest_kf;            /* B */
    int32_t* out_num_lm;                /* B */
    int32_t* out_local_lm;              /* B x m_cap */
    uint8_t* out_held;                  /* B x m_cap */
    int32_t* out_num_lines;             /* B; the three line outputs are required iff kf_lm_lines is given */
    int32_t* out_local_lines;           /* B x ml_cap */
    uint8_t* out_held_lines;            /* B x ml_cap */
} plp_local_map_args;
/* Checked before anything is written (PLP_ERR_INVALID_ARG): NULL ctx / args; a negative B, F, C, L, LL, T, cap, lcap, fcap, flcap, stride,
 * max_num_local_keyfrms or workspace_bytes; k_cap, m_cap or ml_cap < 0; a stride below its fcap / flcap (when not 0); and -- when B > 0 -- a
 * NULL kf_covis, kf_parent (F > 0), kf_children_offsets, kf_children (C > 0), kf_lm (F > 0 and cap > 0), obs_offsets, obs_kf (T > 0), frm_lm
 * (fcap > 0), or a NULL required output of non-zero size.  F > 8192, cap, lcap, fcap or flcap > 8192, B > 65535, k_cap * max(cap, lcap) >=
 * 2^31: PLP_ERR_UNSUPPORTED.  B == 0: PLP_OK, nothing written.  _host and the host build also check that obs_offsets rises from 0 to T and
 * kf_children_offsets from 0 to C (PLP_ERR_INVALID_ARG); on the _device path that is a precondition (the kernels cut every run to its list).
 * _device: every array a DEVICE pointer; k_local_map_keyframes once (a workgroup per frame), then per chunk of frames the clear of the mark
 * table, k_local_map_mark and k_local_map_compact for the points and again for the lines, all on hip_stream; the number of chunks follows
 * from the shapes, so nothing is synchronised.  The mark table is the context's: the calls of one context must be ordered on the device.
 * _host: HOST pointers, staged (the outputs too, so that every slot the kernels do not write keeps the caller's value), synchronous. */
plp_status plp_local_map_device(plp_matcher* ctx, const plp_local_map_args* args, void* hip_stream);
plp_status plp_local_map_host(plp_matcher* ctx, const plp_local_map_args* args);
/* Host build of the same source (csrc/local_map.hpp) with a team of one lane, HOST pointers, no GPU and no context needed; the same checks.
 * Returns B, or the negated plp_status of a refused call. */
int32_t plp_model_local_map_host(const plp_local_map_args* args);

/* ------------------------------------------------------------------------------------------------------------------
 * Map culling: module::local_map_cleaner (src/PLPSLAM/module/local_map_cleaner.cc:51-320), the two map-only calls of the mapping loop
 * (mapping_module.cc:204-284).  Integers and the two float comparisons of the text; contract: DESIGN.md section 5, D20.
 *
 * plp_cull_keyframes_*: remove_redundant_keyframes (:201-240) with count_redundant_observations (:242-320) for G problems over one map
 * snapshot.  A problem is one current key frame with its get_covisibilities() list, in the reference's order and at full length.  The loop
 * is sequential because prepare_for_erasing() of a removed key frame (keyframe.cc:872-926) erases its observations, which lowers
 * num_observations() of its landmarks and discards those left with at most 2 (landmark.cc:99-136); D20 gives that effect in closed form
 * over the set of key frames removed so far, and the entry computes exactly that.  The problems are independent readings of the snapshot.
 *
 * Map snapshot, shared by the G problems (the tables plp_local_ba_args and plp_local_map_args name alike):
 *   kf_lm            [F][cap] keyfrm->get_landmarks(): the landmark row of key point idx, -1 = none                          :251-258
 *   kf_counts        [F] key points per key frame, NULL = cap
 *   undist           [F][kp_stride] undist_keypts_; only `octave` is read                                                    :280, :298
 *   x_right          [F][kp_stride] stereo_x_right_; NULL = monocular, every observation weighs 1            landmark.cc:89-96, :108-115
 *   depths           [F][kp_stride] depths_ and depth_thr [F] depth_thr_; read only when !is_monocular                       :265-269
 *   kf_id            [F] id_                                                                                                 :215, :220
 *   kf_erased        [F] will_be_erased(), NULL = none.  The text has no test of it, so the entry never reads it: an erased covisibility is
 *                    counted and decided like any other.  The field keeps the snapshot's tables together.
 *   kf_cannot_erase  [F] cannot_be_erased_, NULL = none: prepare_for_erasing() returns early                         keyframe.cc:880-884
 *   obs_offsets, obs_kf, obs_idx   lm->get_observations() in plp_landmark_geometry_args' layout; they must agree with kf_lm (slot
 *                    (obs_kf[t], obs_idx[t]) holds the landmark whose run holds t), as observations_ and landmarks_ do
 *   lm_erased        [L] landmark::will_be_erased(), NULL = none                                                             :259
 *   lm_num_obs       [L] num_observations_ before the call; NULL = the sum over the observation list of 2 where x_right >= 0 and 1
 *                    otherwise (landmark.cc:84-97)
 * Problems:
 *   cur_kf           [G] the row of cur_keyfrm
 *   covis_offsets    [G + 1] into covis [Cv]: the rows of cur_keyfrm->graph_node_->get_covisibilities()                      :211
 *   origin_id        origin_keyfrm_id_ (:215); is_monocular: is_monocular_ (:266)
 * A row outside its table (cur_kf, covis, kf_lm, obs_kf, obs_idx against cap) counts as absent; a count is cut to [0, cap]; a run of
 * obs_offsets is cut to [0, T] and one of covis_offsets to [0, Cv].
 * Outputs; slots that are not written keep the caller's values:
 *   out_num_removed    [G] the return value (:239): PLP_CULL_KF_REMOVED and PLP_CULL_KF_REMOVED_HELD entries
 *   out_decision       [Cv] a plp_cull_keyframe_decision per entry
 *   out_num_valid, out_num_redundant   [Cv] num_valid_obs and num_redundant_obs as counted at that entry's turn (:229); not written for
 *                      a skipped entry
 *   out_kf_removed     optional, [G][F]: 1 = the problem's loop called prepare_for_erasing() on the key frame and it took effect
 *   out_lm_erased      optional, [G][L]: 1 = the point landmark will_be_erased() at the end of the problem's loop: lm_erased, or
 *                      discarded by erase_observation (landmark.cc:125-134).  With these two a caller that keeps the tables on the device
 *                      never walks the cascade. */
typedef enum plp_cull_keyframe_decision {
    PLP_CULL_KF_SKIP_ORIGIN = 0,     /* id_ == origin_keyfrm_id_ (:215-218)                                                                  */
    PLP_CULL_KF_SKIP_WINDOW = 1,     /* id_c <= id_cur && id_cur <= id_c + 2 in unsigned 32-bit arithmetic (:220-223)                        */
    PLP_CULL_KF_KEPT = 2,            /* !(0.9f <= (float)num_redundant / num_valid); 0 / 0 is NaN and keeps it (:232)                        */
    PLP_CULL_KF_REMOVED = 3,         /* counted, and prepare_for_erasing() took effect: later entries see the map without it                 */
    PLP_CULL_KF_REMOVED_HELD = 4,    /* counted in num_removed (:234), but cannot_be_erased_ left the map untouched                          */
    PLP_CULL_KF_ABSENT = 5           /* the entry's row, or the problem's cur_kf, is outside [0, F): not counted, nothing else written       */
} plp_cull_keyframe_decision;
typedef struct plp_cull_keyframes_args {
    int32_t F, L, T;                    /* F <= 8192 key frames (the removed set is an LDS bitmap); L landmark rows; T observation entries */
    int32_t cap, kp_stride;             /* slots per row of kf_lm, <= 8192; slots between two rows of undist, x_right and depths, 0 = cap */
    int32_t G, Cv;                      /* G <= 65535 problems; Cv entries of covis */
    uint32_t origin_id;
    int32_t is_monocular;
    const int32_t* kf_lm;               /* F x cap */
    const int32_t* kf_counts;           /* F, or NULL */
    const plp_keypoint* undist;         /* F x kp_stride */
    const float* x_right;               /* F x kp_stride, or NULL */
    const float* depths;                /* F x kp_stride; required iff !is_monocular */
    const float* depth_thr;             /* F; required iff !is_monocular */
    const uint32_t* kf_id;              /* F */
    const uint8_t* kf_erased;           /* F, or NULL; never read */
    const uint8_t* kf_cannot_erase;     /* F, or NULL */
    const int32_t* obs_offsets;         /* L + 1 */
    const int32_t* obs_kf;              /* T */
    const int32_t* obs_idx;             /* T */
    const uint8_t* lm_erased;           /* L, or NULL */
    const uint32_t* lm_num_obs;         /* L, or NULL */
    const int32_t* cur_kf;              /* G */
    const int32_t* covis_offsets;       /* G + 1 */
    const int32_t* covis;               /* Cv */
    int32_t* out_num_removed;           /* G */
    uint8_t* out_decision;              /* Cv */
    int32_t* out_num_valid;             /* Cv */
    int32_t* out_num_redundant;         /* Cv */
    uint8_t* out_kf_removed;            /* G x F, or NULL */
    uint8_t* out_lm_erased;             /* G x L, or NULL */
} plp_cull_keyframes_args;
/* Checked before anything is written (PLP_ERR_INVALID_ARG): NULL ctx / args; a negative F, L, T, cap, kp_stride, G or Cv; a kp_stride
 * below cap (when not 0); and -- when G > 0 -- a NULL cur_kf, covis_offsets, covis (Cv > 0), kf_id (F > 0), kf_lm or undist (F > 0 and
 * cap > 0), obs_offsets, obs_kf or obs_idx (T > 0), depths (F > 0 and cap > 0) or depth_thr (F > 0) when !is_monocular, out_num_removed, or
 * out_decision, out_num_valid or out_num_redundant (Cv > 0).  F > 8192, cap > 8192 or G > 65535: PLP_ERR_UNSUPPORTED.  G == 0: PLP_OK,
 * nothing written.  _host and the host build also check that obs_offsets rises from 0 to T and covis_offsets from 0 to Cv
 * (PLP_ERR_INVALID_ARG); on the _device path that is a precondition (the kernels cut every run to its list).
 * _device: every array a DEVICE pointer; k_cull_count (a workgroup per entry: the counts against the snapshot), k_cull_replay (a workgroup
 * per problem: the loop in order, recounting once a key frame is removed) and, with an optional mask, k_cull_dead_landmarks, all on hip_stream,
 * nothing synchronised.  The counts and the removed sets pass through buffers the context owns: the calls of one context must be ordered on
 * the device.  _host: HOST pointers, staged (the outputs too, so that every slot the kernels do not write keeps the caller's value),
 * synchronous. */
plp_status plp_cull_keyframes_device(plp_matcher* ctx, const plp_cull_keyframes_args* args, void* hip_stream);
plp_status plp_cull_keyframes_host(plp_matcher* ctx, const plp_cull_keyframes_args* args);
/* Host build of the same source (csrc/map_cull.hpp) with a team of one lane, HOST pointers, no GPU and no context needed; the same checks.
 * Returns G, or the negated plp_status of a refused call. */
int32_t plp_model_cull_keyframes_host(const plp_cull_keyframes_args* args);

/* plp_cull_landmarks_*: remove_redundant_landmarks (:51-131) or remove_redundant_landmarks_line (:133-199) for R fresh lists in ragged
 * form; points and lines are two calls with their own tables (or, where the rows share one table, two lists of one call).
 *   fresh_offsets    [R + 1] into fresh [N]: fresh_landmarks_ / _fresh_landmarks_line as landmark rows, in list order      :66, :148
 *   lm_erased        [L] will_be_erased(), NULL = none                                                                      :73, :155
 *   num_observed, num_observable   [L] the two terms of get_observed_ratio(): (float)num_observed / num_observable, compared < 0.3f;
 *                    0 / 0 and x / 0 behave as IEEE float does (NaN is not below, +inf is not below)          :79, :161, landmark.cc:453-457
 *   first_kf_id      [L] first_keyfrm_id_; num_obs [L] num_observations()                                                   :92, :105
 *   owning_plane     [L] get_Owning_Plane() != nullptr, NULL = none (the line list passes NULL)                             :83, :96
 *   cur_kf_id        [R] cur_keyfrm_id; num_obs_thr [R]: 2 or 3 by is_monocular_ for points (:55), 3 for lines (:137)
 * The id tests are unsigned 32-bit: 2 + first_kf_id <= cur_kf_id and 3 + first_kf_id <= cur_kf_id.  A row outside [0, L) leaves the buffer
 * as an erased one does (PLP_CULL_DROP).  A run of fresh_offsets is cut to [0, N].  Entries are independent.
 * Outputs (out_fresh must not overlap fresh):
 *   out_state        [N] a plp_cull_landmark_state per entry
 *   out_num_removed  [R] the return value: PLP_CULL_ERASE entries (:119, :187)
 *   out_num_fresh    [R] the length of the list afterwards; out_fresh [N]: its entries, the PLP_CULL_HOLD ones in order, from
 *                    fresh_offsets[r] on; the slots behind them keep the caller's values */
typedef enum plp_cull_landmark_state {
    PLP_CULL_HOLD = 0,               /* NotClear: stays in the buffer                                      */
    PLP_CULL_DROP = 1,               /* Valid: leaves the buffer only                                      */
    PLP_CULL_ERASE = 2               /* Invalid: counted, prepare_for_erasing(), leaves the buffer         */
} plp_cull_landmark_state;
typedef struct plp_cull_landmarks_args {
    int32_t R, N, L;                    /* lists, entries of fresh, landmark rows */
    const int32_t* fresh_offsets;       /* R + 1 */
    const int32_t* fresh;               /* N */
    const uint8_t* lm_erased;           /* L, or NULL */
    const uint32_t* num_observed;       /* L */
    const uint32_t* num_observable;     /* L */
    const uint32_t* first_kf_id;        /* L */
    const uint32_t* num_obs;            /* L */
    const uint8_t* owning_plane;        /* L, or NULL */
    const uint32_t* cur_kf_id;          /* R */
    const uint32_t* num_obs_thr;        /* R */
    uint8_t* out_state;                 /* N */
    int32_t* out_num_removed;           /* R */
    int32_t* out_num_fresh;             /* R */
    int32_t* out_fresh;                 /* N */
} plp_cull_landmarks_args;
/* Checked before anything is written (PLP_ERR_INVALID_ARG): NULL ctx / args; a negative R, N or L; and -- when R > 0 -- a NULL
 * fresh_offsets, cur_kf_id, num_obs_thr, out_num_removed or out_num_fresh, a NULL fresh, out_state or out_fresh (N > 0), a NULL
 * num_observed, num_observable, first_kf_id or num_obs (L > 0).  R == 0: PLP_OK, nothing written.  _host and the host build also check that
 * fresh_offsets rises from 0 to N.  _device: DEVICE pointers, k_cull_landmark_states (a workgroup per list) on hip_stream.  _host: HOST
 * pointers, staged, synchronous.  plp_model_cull_landmarks_host: the host build; returns R, or the negated plp_status. */
plp_status plp_cull_landmarks_device(plp_matcher* ctx, const plp_cull_landmarks_args* args, void* hip_stream);
plp_status plp_cull_landmarks_host(plp_matcher* ctx, const plp_cull_landmarks_args* args);
int32_t plp_model_cull_landmarks_host(const plp_cull_landmarks_args* args);

/* ------------------------------------------------------------------------------------------------------------------
 * The covisibility graph: data::graph_node (src/PLPSLAM/data/graph_node.cc:36-285) kept as tables.  Integers only; contract: DESIGN.md
 * section 5, D21.  Key-frame rows stand in for keyframe*: where the text orders by pointer, rows order it, ascending.
 *
 * plp_covisibility_update_*: update_connections() (:92-193) of the G key frames of `owners`, as if called one after another in list order
 * over one snapshot of kf_lm and the observation lists.  The loop is sequential only through add_connection (:36-59) and the assignment of
 * :180; D21 gives every key frame's final state in closed form (its base, then the overlays of the owners that name it), and the entry
 * computes exactly that.
 *
 * Map snapshot, read only (the tables plp_local_map_args and plp_cull_keyframes_args name alike):
 *   kf_lm            [F][cap] owner_keyfrm_->get_landmarks(): the landmark row of key point idx, -1 = none                    :94-102
 *   kf_counts        [F] key points per key frame, NULL = cap
 *   obs_offsets, obs_kf   lm->get_observations() in plp_landmark_geometry_args' layout                                       :108-120
 *   lm_erased        [L] landmark::will_be_erased(), NULL = none                                                             :103
 *   kf_id            [F] id_; only `!= 0` is read                                                                            :184
 * A landmark row outside [0, L) counts as absent, a count is cut to [0, cap], a run of obs_offsets to [0, T], an observation whose key
 * frame is outside [0, F) is not counted.  A landmark that sits in two slots counts twice.  The text has no test of a key frame's
 * will_be_erased(), so there is none.
 * State, updated in place, a row per key frame:
 *   kf_conn, kf_conn_w   [F][conn_cap] connected_keyfrms_and_weights_ in ascending row; kf_n_conn [F] its length
 *   kf_covis, kf_covis_w [F][covis_cap] ordered_covisibilities_ / ordered_weights_ in list order: descending (weight, row) (:165, :208);
 *                    kf_n_covis [F] its length.  A row that is written is written whole: -1 / 0 behind the last entry of either list.
 *                    The first 10 columns of kf_covis are plp_local_map_args' kf_covis
 *   kf_parent        [F] spanning_parent_ (plp_local_map_args' kf_parent); kf_parent_unset [F] spanning_parent_is_not_set_           :184-191
 * A state row outside [0, F) is dropped when its row is rewritten.  Weights stay below 2^31.
 * Problem:
 *   owners           [G] rows, in call order
 * Outputs; out_status is required, NULL = not wanted for the others:
 *   out_status       [G] a plp_covisibility_status
 *   out_nearest      [G] nearest_covisibility (:139-143): the largest row among the maximal weights; -1 unless OK / OVERFLOW
 *   out_max_weight   [G] max_weight; 0 unless OK / OVERFLOW
 *   out_touched      [F] 0 = the row's state was not written, 1 = written, 2 = not valid any more (see PLP_COVIS_OVERFLOW) */
typedef enum plp_covisibility_status {
    PLP_COVIS_OK = 0,
    PLP_COVIS_NO_SHARED = 1,         /* keyfrm_weights.empty() (:123-126): the call returned, nothing of the owner changed, not even its connected map */
    PLP_COVIS_ROW_ABSENT = 2,        /* the owner is outside [0, F)                                                                                   */
    PLP_COVIS_DUPLICATE = 3,         /* the owner appeared earlier in the list: not processed (the _host entry and the host build refuse such a list) */
    PLP_COVIS_OVERFLOW = 4           /* the owner's row outgrew conn_cap or covis_cap: kf_n_conn / kf_n_covis carry the length (above the cap), the
                                        row is written up to its cap in its order and out_touched is 2: the caller restores the row, grows the table
                                        and calls again.  A row that only received connections and outgrew a cap has out_touched 2 as well; so has a
                                        row for which an owner cut at conn_cap could not tell whether it connects to it                              */
} plp_covisibility_status;
typedef struct plp_covisibility_update_args {
    int32_t F, L, T;                    /* F <= 8192 key frames (the weights of an owner are an LDS table); L landmark rows; T observation entries */
    int32_t cap;                        /* slots per row of kf_lm, <= 8192 */
    int32_t conn_cap, covis_cap;        /* slots per row of kf_conn and of kf_covis, <= 8192 */
    int32_t G;                          /* owners, <= 8192 */
    const int32_t* kf_lm;               /* F x cap */
    const int32_t* kf_counts;           /* F, or NULL */
    const int32_t* obs_offsets;         /* L + 1 */
    const int32_t* obs_kf;              /* T */
    const uint8_t* lm_erased;           /* L, or NULL */
    const uint32_t* kf_id;              /* F */
    int32_t* kf_conn;                   /* F x conn_cap */
    int32_t* kf_conn_w;                 /* F x conn_cap */
    int32_t* kf_n_conn;                 /* F */
    int32_t* kf_covis;                  /* F x covis_cap */
    int32_t* kf_covis_w;                /* F x covis_cap */
    int32_t* kf_n_covis;                /* F */
    int32_t* kf_parent;                 /* F */
    uint8_t* kf_parent_unset;           /* F */
    const int32_t* owners;              /* G */
    uint8_t* out_status;                /* G */
    int32_t* out_nearest;               /* G, or NULL */
    int32_t* out_max_weight;            /* G, or NULL */
    uint8_t* out_touched;               /* F, or NULL */
} plp_covisibility_update_args;
/* Checked before anything is written (PLP_ERR_INVALID_ARG): NULL ctx / args; a negative F, L, T, cap, conn_cap, covis_cap or G; a NULL
 * kf_n_conn or kf_n_covis (F > 0), kf_conn or kf_conn_w (F > 0 and conn_cap > 0), kf_covis or kf_covis_w (F > 0 and covis_cap > 0); and --
 * when G > 0 -- a NULL owners, out_status, kf_id, kf_parent or kf_parent_unset (F > 0), kf_lm (F > 0 and cap > 0), obs_offsets or obs_kf
 * (T > 0).  F, cap, conn_cap, covis_cap or G above 8192: PLP_ERR_UNSUPPORTED.  G == 0: PLP_OK, nothing written.  F == 0: every owner is
 * PLP_COVIS_ROW_ABSENT.  _host and the host build also check that obs_offsets rises from 0 to T and that no owner appears twice
 * (PLP_ERR_INVALID_ARG); on the _device path the first is a precondition (the kernels cut every run to its list) and the second a status.
 * _device: every array a DEVICE pointer; k_covis_count (a workgroup per owner: the weights, nearest, the pairs, the owner's own lists into
 * the context's scratch) and k_covis_apply (a workgroup per key frame: the overlays, the row), all on hip_stream, nothing synchronised.  The
 * scratch grows on the first call of a size; the calls of one context must be ordered on the device.  _host: HOST pointers, staged (the
 * state and the outputs both ways), synchronous. */
plp_status plp_covisibility_update_device(plp_matcher* ctx, const plp_covisibility_update_args* args, void* hip_stream);
plp_status plp_covisibility_update_host(plp_matcher* ctx, const plp_covisibility_update_args* args);
/* Host build of the same source (csrc/covisibility.hpp) with a team of one lane, HOST pointers, no GPU and no context needed; the same
 * checks.  Returns G, or the negated plp_status of a refused call. */
int32_t plp_model_covisibility_update_host(const plp_covisibility_update_args* args);

/* plp_covisibility_erase_*: erase_all_connections() (:79-90) of every key frame k with erased[k] != 0, in any order (the result does not
 * depend on it): a surviving key frame j loses every such k that holds j in its connected map at the start of the call and that j holds
 * (erase_connection, :61-77), and rebuilds its ordered list from ALL of its connected map if it lost one (update_covisibility_orders,
 * :195-219); a stale k that j holds without k holding j stays, as in the text.  The erased rows end empty.  The parents are not touched
 * (keyframe::prepare_for_erasing mends the spanning tree, keyframe.cc:886-909).
 *   out_status       [F] PLP_COVIS_OK, or PLP_COVIS_OVERFLOW where the rebuilt list outgrew covis_cap (kf_n_covis carries the true length)
 *   out_touched      [F] as above */
typedef struct plp_covisibility_erase_args {
    int32_t F;                          /* <= 8192 */
    int32_t conn_cap, covis_cap;        /* <= 8192 */
    int32_t* kf_conn;                   /* F x conn_cap */
    int32_t* kf_conn_w;                 /* F x conn_cap */
    int32_t* kf_n_conn;                 /* F */
    int32_t* kf_covis;                  /* F x covis_cap */
    int32_t* kf_covis_w;                /* F x covis_cap */
    int32_t* kf_n_covis;                /* F */
    const uint8_t* erased;              /* F */
    uint8_t* out_status;                /* F */
    uint8_t* out_touched;               /* F, or NULL */
} plp_covisibility_erase_args;
/* Checks as above; F == 0: PLP_OK, nothing written.  _device: k_covis_erase twice on hip_stream (a workgroup per key frame: the surviving
 * rows, which read the erased ones, then the erased rows), no scratch.  plp_model_covisibility_erase_host returns F, or the negated
 * plp_status. */
plp_status plp_covisibility_erase_device(plp_matcher* ctx, const plp_covisibility_erase_args* args, void* hip_stream);
plp_status plp_covisibility_erase_host(plp_matcher* ctx, const plp_covisibility_erase_args* args);
int32_t plp_model_covisibility_erase_host(const plp_covisibility_erase_args* args);

/* ---- Loop closing: optimize::graph_optimizer::optimize (src/PLPSLAM/optimize/graph_optimizer.cc:53-350; csrc/pose_graph.hpp, DESIGN.md
 * section 5, D22) for G problems over one key-frame table and its graph tables (D21's layout).  A Sim3 is 8 doubles: the quaternion x y z w
 * (never normalised), the translation, the scale.
 *
 * Vertices (:85-129): every row with kf_erased == 0, ascending row (rows ascending in kf_id reproduce g2o's index mapping).  The estimate is
 * the problem's pre_corrected Sim3 of the row if listed, else Sim3(rot_cw, trans_cw, 1.0) of its pose row.  loop_kf is fixed.
 * Edges (:131-298), in insertion order, which is the order of every sum:
 *   [3.1] the problem's loop connections (lc_owner, lc_target) in list order -- the reference walks a std::map of std::sets in pointer order;
 *         ascending (owner, target) is this library's order and the caller's to keep -- unless get_weight(owner, target) on kf_conn /
 *         kf_conn_w (0: not connected) is below 100 and the pair is not (curr_kf, loop_kf); type PLP_POSE_GRAPH_EDGE_LOOP_CONNECTION   :154-181
 *   [3.2] for every row k ascending: the parent edge (:196-217; id(k) <= id(parent) leaves the key frame altogether, as the text's
 *         `continue` does), the loop edges kf_loop[kf_loop_offsets[k] .. kf_loop_offsets[k + 1]) with id(k) > id(other) (:222-243), the
 *         covisibilities of get_covisibilities_over_weight(100) -- the empty list when every entry reaches the weight -- that have a parent,
 *         are neither the parent nor a child (kf_parent[c] == k) nor a loop edge nor erased, with id(k) > id(c) and no edge of that pair yet
 *         (:248-297).  The relative pose Sim3_21 uses the problem's non_corrected Sim3 of a row where listed, else the vertex's initial one.
 *   An edge with an erased end, a row outside the table or both ends the same row is not inserted.  kf_id must be unique; the rows of
 *   kf_covis and kf_loop hold a key frame once.
 * A vertex without an edge is not in the system and keeps its estimate.  The error of an edge is (Sim3_21 * v1 * v2^-1).log() (g2o's
 * Sim3::log restated, log and acos without a library), the information the identity, no robust kernel; the Jacobians are g2o's central
 * differences through the vertex's update Sim3(x) * est (sigma = 0 under fix_scale).  Up to 50 Levenberg-Marquardt iterations
 * (csrc/levenberg.hpp); the linear system is solved by a block skyline Cholesky in vertex order (this replaces LinearSolverCSparse: the same
 * solution, other rounding).  Parity against a g2o build is unpinned: the definition is csrc/pose_graph.hpp = tests/pose_graph_ref.py.
 *
 * Outputs (:307-328), written for the rows that are vertices only:
 *   out_status       [G] plp_pose_graph_status; anything but OK / NO_EDGES: only out_status and out_num_edges are written
 *   out_num_edges    [G] the edges (TOO_MANY_EDGES: the number that would be needed)
 *   out_edges        [G][edge_cap][3] id1 row, id2 row, plp_pose_graph_edge_type, the first out_num_edges entries
 *   out_sim3_cw      [G][F][8] Sim3s_cw, the initial estimates            :100, :110
 *   out_corrected_wc [G][F][8] the inverse of the final estimate          :327
 *   out_pose         [G][F][15] rot_cw (the quaternion's toRotationMatrix), trans_cw = t / (double)(float)s, the camera centre   :319-325
 *   out_info         [G][4] iterations, rejected steps, why it ended (1 iterations, 2 tries, 3 rho == 0; 0 = not run), vertices in the system
 *   out_chi2         [G][2] chi2 and lambda at the end */
typedef enum plp_pose_graph_status {
    PLP_POSE_GRAPH_OK = 0,
    PLP_POSE_GRAPH_NO_EDGES = 1,             /* nothing to optimise: the outputs carry the initial estimates */
    PLP_POSE_GRAPH_ENVELOPE_TOO_LARGE = 2,   /* the skyline needs more than env_cap blocks */
    PLP_POSE_GRAPH_TOO_MANY_EDGES = 3,       /* more than edge_cap edges */
    PLP_POSE_GRAPH_BAD_LOOP_KF = 4           /* loop_kf is no vertex */
} plp_pose_graph_status;
typedef enum plp_pose_graph_edge_type {
    PLP_POSE_GRAPH_EDGE_LOOP_CONNECTION = 1, PLP_POSE_GRAPH_EDGE_PARENT = 2, PLP_POSE_GRAPH_EDGE_LOOP = 3, PLP_POSE_GRAPH_EDGE_COVIS = 4
} plp_pose_graph_edge_type;
typedef struct plp_pose_graph_args {
    int32_t G;                          /* <= 16 */
    int32_t F;                          /* <= 1024 */
    int32_t pose_stride;                /* >= 12 */
    int32_t conn_cap, covis_cap;        /* <= 65536 */
    int32_t edge_cap;                   /* edges per problem, 1 .. 16384 */
    int32_t env_cap;                    /* 7 x 7 blocks of a problem's skyline, 1 .. 65536 */
    int32_t max_iter;                   /* 50 in the reference */
    const double* pose;                 /* F x pose_stride */
    const uint8_t* kf_erased;           /* F, or NULL */
    const int32_t* kf_id;               /* F */
    const int32_t* kf_parent;           /* F */
    const int32_t* kf_conn;             /* F x conn_cap */
    const int32_t* kf_conn_w;           /* F x conn_cap */
    const int32_t* kf_n_conn;           /* F */
    const int32_t* kf_covis;            /* F x covis_cap */
    const int32_t* kf_covis_w;          /* F x covis_cap */
    const int32_t* kf_n_covis;          /* F */
    const int32_t* kf_loop_offsets;     /* F + 1, or NULL: no loop edges */
    const int32_t* kf_loop;             /* kf_loop_offsets[F] */
    const int32_t* loop_kf;             /* G */
    const int32_t* curr_kf;             /* G */
    const uint8_t* fix_scale;           /* G, or NULL: free scale */
    const int32_t* pre_offsets;         /* G + 1, or NULL */
    const int32_t* pre_row;
    const double* pre_sim3;             /* x 8 */
    const int32_t* non_offsets;         /* G + 1, or NULL */
    const int32_t* non_row;
    const double* non_sim3;             /* x 8 */
    const int32_t* lc_offsets;          /* G + 1, or NULL */
    const int32_t* lc_owner;
    const int32_t* lc_target;
    uint8_t* out_status;                /* G */
    int32_t* out_num_edges;             /* G, or NULL */
    int32_t* out_edges;                 /* G x edge_cap x 3, or NULL */
    double* out_sim3_cw;                /* G x F x 8, or NULL */
    double* out_corrected_wc;           /* G x F x 8, or NULL */
    double* out_pose;                   /* G x F x 15, or NULL */
    int32_t* out_info;                  /* G x 4, or NULL */
    double* out_chi2;                   /* G x 2, or NULL */
} plp_pose_graph_args;
/* PLP_ERR_INVALID_ARG: a NULL args, negative sizes, pose_stride < 12, max_iter < 0, edge_cap or env_cap < 1, a missing required array.
 * PLP_ERR_UNSUPPORTED, before anything is written: G > 16, F > 1024, edge_cap > 16384, env_cap > 65536, conn_cap or covis_cap > 65536 --
 * the state of a call is G (122 edge_cap + 98 env_cap + 60 F) doubles, at most 1.1 GB.  _host also checks that the offset lists ascend.
 * G == 0: PLP_OK.  _device: DEVICE pointers; k_pg_prepare, k_pg_solve (every iteration without the host) and k_pg_finish, one workgroup of
 * 512 per problem, on hip_stream, nothing synchronised; the state lives in the context.  _host: HOST pointers, staged, synchronous. */
plp_status plp_pose_graph_optimize_device(plp_matcher* ctx, const plp_pose_graph_args* args, void* hip_stream);
plp_status plp_pose_graph_optimize_host(plp_matcher* ctx, const plp_pose_graph_args* args);
/* Host builds of the same source with a team of one lane, HOST pointers, no GPU and no context needed; the same checks.  Return G, or the
 * negated plp_status.  _edges_ stops after the edge list (:131-298): out_status, out_num_edges, out_edges and out_sim3_cw only. */
int32_t plp_model_pose_graph_optimize_host(const plp_pose_graph_args* args);
int32_t plp_model_pose_graph_edges_host(const plp_pose_graph_args* args);
/* g2o's Sim3::log of n Sim3 (n x 8 -> n x 7: omega, upsilon, sigma), and its two scalar functions: log on 1e-300 <= x <= 1e300, acos on
 * -1 <= x <= 1, NaN outside (D22).  Return n, -1 for a refused call. */
int32_t plp_model_sim3_log_host(const double* sim3, int32_t n, double* out7);
int32_t plp_model_pose_log_host(const double* x, int32_t n, double* out);
int32_t plp_model_pose_acos_host(const double* x, int32_t n, double* out);
/* D22's block skyline solve of (H + lambda I) x = b on a given system of n <= 1024 vertices: first[i] <= i the first column block of row
 * block i, env the blocks first[i] .. i of every row block in order, each row block as seven scalar rows of 7 (i - first[i] + 1) (the upper
 * part of a diagonal block is not read), b (7 n).  Returns 1, 0 when a pivot is not positive and finite (x is then zero), -1 refused. */
int32_t plp_model_block_chol7_host(int32_t n, const int32_t* first, const double* env, const double* b, double lambda, double* out_x);

/* The landmark half of graph_optimizer::optimize (:331-350): out_pos_w[l] = corrected_Sim3_wc[ref].map(Sim3_cw[ref].map(pos_w[l])) with
 * ref = ref_kf[l], the row the caller resolves (ref_keyfrm_id_in_loop_fusion_ when the landmark's loop_fusion_identifier_ is the current key
 * frame's, else its reference key frame, :338-340); sim3_cw / corrected_wc are one problem's out_sim3_cw / out_corrected_wc (F x 8).
 * out_pos_w may be pos_w.  out_status [L]: plp_correct_landmark_status; only a corrected landmark's position is written. */
typedef enum plp_correct_landmark_status { PLP_CORRECT_LM_OK = 0, PLP_CORRECT_LM_ERASED = 1, PLP_CORRECT_LM_NO_VERTEX = 2 } plp_correct_landmark_status;
typedef struct plp_correct_landmarks_args {
    int32_t L, F;                       /* F <= 1024 */
    const double* pos_w;                /* L x 3 */
    const uint8_t* lm_erased;           /* L, or NULL */
    const int32_t* ref_kf;              /* L */
    const uint8_t* kf_erased;           /* F, or NULL */
    const double* sim3_cw;              /* F x 8 */
    const double* corrected_wc;         /* F x 8 */
    double* out_pos_w;                  /* L x 3 */
    uint8_t* out_status;                /* L */
} plp_correct_landmarks_args;
/* _device: DEVICE pointers, one lane per landmark (k_pg_correct_landmarks), asynchronous.  _host: HOST pointers, staged, synchronous. */
plp_status plp_correct_landmarks_device(plp_matcher* ctx, const plp_correct_landmarks_args* args, void* hip_stream);
plp_status plp_correct_landmarks_host(plp_matcher* ctx, const plp_correct_landmarks_args* args);
int32_t plp_model_correct_landmarks_host(const plp_correct_landmarks_args* args);

/* ------------------------------------------------------------------------------------------------------------------
 * The line map update every optimiser of the reference ends with (csrc/line_update.hpp): the two Pluecker
 * transforms of loop closing and the end-point trimming all four optimisers share.
 *
 * plp_trim_line_endpoints_*: endpoint_trimming (optimize/graph_optimizer.cc:424-532, module/loop_bundle_adjuster.cc:269-,
 * optimize/global_bundle_adjuster.cc:362-, optimize/local_bundle_adjuster_extended_line.cc:676-787) for L lines over a table of F key
 * frames, and the array half of what every call site does with its result: the Pluecker line pluecker[l] = (m, d) is reprojected into its
 * reference key frame with that key frame's CURRENT pose row, l = _K (transformation_line_cw L)(0..2), the key line's start and end point
 * are moved to their closest points on l, and the planes through them and the points on the x = 0 axis are intersected with the line's
 * Pluecker matrix (line3d_trim, D7).  The key line is keylines[ref_kf][idx], idx = obs_idx of the first observation whose obs_kf is
 * ref_kf (get_index_in_keyframe), -1 where there is none.
 *   PLP_TRIM_DEPTH_POSITIVE  accepted when 0 < z_c(sp) && 0 < z_c(ep) in the reference key frame (the graph, loop and global adjusters)
 *   PLP_TRIM_MAX_CHANGE      rejected when |sp - sp_old| / median_depth[ref_kf] > max_change || |ep - ep_old| / median_depth[ref_kf] >
 *                            max_change, the local adjuster's test (:773-786; no depth test); median_depth is what plp_median_depth_*
 *                            writes with abs_flag
 * A comparison with a NaN is false, as in the reference: DEPTH_POSITIVE rejects such a line, MAX_CHANGE accepts it.
 *   out_status  [L] a plp_trim_status, where the reference leaves the function, in its order of evaluation
 *   out_pos_w   [L][6] (sp, ep), written only where the status is PLP_TRIM_OK (set_pos_in_world_without_update_pluecker); may be pos_w_old
 *   out_erase   [L] 1 for NOT_OBSERVED and REJECTED (prepare_for_erasing), else 0 */
typedef enum plp_trim_mode { PLP_TRIM_DEPTH_POSITIVE = 0, PLP_TRIM_MAX_CHANGE = 1 } plp_trim_mode;
typedef enum plp_trim_status {
    PLP_TRIM_OK = 0,
    PLP_TRIM_SKIPPED = 1,               /* skip[l]: the caller never reaches the trim                                                   */
    PLP_TRIM_NO_REF = 2,                /* ref_kf outside [0, F) or erased: the reference follows a pointer it does not hold           */
    PLP_TRIM_NOT_OBSERVED = 3,          /* idx == -1: the trim returns false                                                            */
    PLP_TRIM_INDEX_RANGE = 4,           /* idx outside [0, counts[ref_kf]), where _keylsd.at() throws                                   */
    PLP_TRIM_REJECTED = 5               /* the mode's test                                                                              */
} plp_trim_status;
typedef struct plp_trim_line_endpoints_args {
    plp_camera_model camera;            /* PLP_CAMERA_PERSPECTIVE (the trim static_casts to camera::perspective); fx, fy, cx, cy are read */
    int32_t mode;                       /* a plp_trim_mode */
    double max_change;                  /* PLP_TRIM_MAX_CHANGE: 0.1 at :777 */
    int32_t L, F, cap, pose_stride;     /* L >= 0 lines, F >= 0 key frames of cap >= 0 key-line slots, pose_stride >= 12 */
    const double* pluecker;             /* L x 6: (m, d), what set_PlueckerCoord_without_update_endpoints took */
    const int32_t* ref_kf;              /* L: the reference key frame as a row of the table */
    const uint8_t* skip;                /* L, or NULL = none */
    const int32_t* obs_offsets;         /* L + 1, non-decreasing from 0: the layout of plp_landmark_geometry_args */
    const int32_t* obs_kf;              /* obs_offsets[L] */
    const int32_t* obs_idx;             /* obs_offsets[L] */
    const double* pose;                 /* F x pose_stride: rot_cw (row-major), trans_cw */
    const uint8_t* kf_erased;           /* F, or NULL */
    const plp_keyline* keylines;        /* F x cap: _keylsd; only the start and the end point are read */
    const int32_t* counts;              /* F: _keylsd.size(), or NULL = cap everywhere */
    const double* pos_w_old;            /* PLP_TRIM_MAX_CHANGE: L x 6, get_pos_in_world() */
    const float* median_depth;          /* PLP_TRIM_MAX_CHANGE: F, compute_median_depth(true) */
    double* out_pos_w;                  /* L x 6 */
    uint8_t* out_status;                /* L */
    uint8_t* out_erase;                 /* L */
} plp_trim_line_endpoints_args;
/* Checked before anything is written: PLP_ERR_INVALID_ARG for NULL ctx / args, an unknown camera model or mode, fx or fy 0 or a non-finite
 * fx, fy, cx, cy, a negative L, F or cap, pose_stride < 12, and -- when L > 0 -- a NULL pluecker, ref_kf, obs_offsets, out_pos_w, out_status
 * or out_erase, a NULL pose (F > 0), a NULL keylines (F > 0 and cap > 0), a NULL pos_w_old or median_depth (F > 0) in PLP_TRIM_MAX_CHANGE;
 * PLP_ERR_UNSUPPORTED for a camera that is not perspective.  L == 0: PLP_OK, nothing written.  _host and the host build also check that
 * obs_offsets rises from 0 (PLP_ERR_INVALID_ARG); obs_kf / obs_idx may be NULL when it ends at 0.
 * _device: DEVICE pointers, one lane per line (k_trim_line_endpoints), asynchronous.  _host: HOST pointers, staged (the outputs too), the
 * same kernel, synchronous.  plp_model_*_host: the host build of csrc/line_update.hpp, no GPU; returns L, or the negated plp_status. */
plp_status plp_trim_line_endpoints_device(plp_matcher* ctx, const plp_trim_line_endpoints_args* args, void* hip_stream);
plp_status plp_trim_line_endpoints_host(plp_matcher* ctx, const plp_trim_line_endpoints_args* args);
int32_t plp_model_trim_line_endpoints_host(const plp_trim_line_endpoints_args* args);

/* The line cloud of graph_optimizer::optimize (:352-403): out_pluecker[l] = (corrected_Sim3_wc_pluecker * Sim3_cw_pluecker) * pluecker[l],
 * each 6 x 6 matrix [s R, skew(t) R; 0, R] of the Sim3 of row corr_kf[l] (R = rotation().toRotationMatrix(), t the Sim3's translation); the
 * product of the two matrices is formed first.  ref_kf[l] is the row the reference tests (:362-373), corr_kf[l] the row the caller resolves
 * (:375-377).  out_pluecker may be pluecker; only an OK line's coordinates are written.  The trim of :407-417 is plp_trim_line_endpoints_*
 * on the same stream, with the corrected poses. */
typedef enum plp_correct_line_status {
    PLP_CORRECT_LINE_OK = 0,
    PLP_CORRECT_LINE_ERASED = 1,        /* lm_erased[l] (:357-360)                                                                       */
    PLP_CORRECT_LINE_NO_REF = 2,        /* ref_kf outside [0, F) or erased: prepare_for_erasing (:362-373)                              */
    PLP_CORRECT_LINE_NO_VERTEX = 3      /* corr_kf outside [0, F) or erased, where Sim3s_cw.at(id) throws                               */
} plp_correct_line_status;
typedef struct plp_correct_landmark_lines_args {
    int32_t L, F;                       /* F <= 1024 */
    const double* pluecker;             /* L x 6 */
    const uint8_t* lm_erased;           /* L, or NULL */
    const int32_t* ref_kf;              /* L */
    const int32_t* corr_kf;             /* L, or NULL = ref_kf */
    const uint8_t* kf_erased;           /* F, or NULL */
    const double* sim3_cw;              /* F x 8 */
    const double* corrected_wc;         /* F x 8 */
    double* out_pluecker;               /* L x 6 */
    uint8_t* out_status;                /* L */
} plp_correct_landmark_lines_args;
/* The checks of plp_correct_landmarks_*.  _device: DEVICE pointers, one lane per line (k_correct_landmark_lines), asynchronous.  _host: HOST
 * pointers, staged, synchronous.  The host build returns L, or the negated plp_status. */
plp_status plp_correct_landmark_lines_device(plp_matcher* ctx, const plp_correct_landmark_lines_args* args, void* hip_stream);
plp_status plp_correct_landmark_lines_host(plp_matcher* ctx, const plp_correct_landmark_lines_args* args);
int32_t plp_model_correct_landmark_lines_host(const plp_correct_landmark_lines_args* args);

/* The line cloud of loop_bundle_adjuster::optimize (:184-244) over what plp_loop_ba_propagate_* wrote: an optimised line takes
 * pluecker_after[l] (_pos_w_after_global_BA); any other line that is not erased goes L_c = T(pose_before[ref]) L, L_w = T(inverse of
 * pose_after[ref]) L_c, T(R, t) = [R, skew(t) R; 0, R], the inverse as set_cam_pose stores it (rot_cw transposed, cam_center).
 * out_status [L]: a plp_loop_ba_lm_status, NO_REF for a ref_kf outside the table or with a kf_status neither OPTIMIZED nor PROPAGATED;
 * out_pluecker [L][6] for OPTIMIZED and MOVED rows only, may be pluecker. */
typedef struct plp_loop_ba_propagate_lines_args {
    int32_t L, F;                       /* F <= 4096 */
    const double* pose_after;           /* F x 15: plp_loop_ba_propagate_args.out_pose */
    const double* pose_before;          /* F x 12: plp_loop_ba_propagate_args.out_pose_before */
    const uint8_t* kf_status;           /* F: plp_loop_ba_propagate_args.out_kf_status */
    const double* pluecker;             /* L x 6 */
    const uint8_t* lm_erased;           /* L, or NULL */
    const int32_t* ref_kf;              /* L */
    const uint8_t* line_optimized;      /* L, or NULL = none: _loop_BA_identifier == identifier */
    const double* pluecker_after;       /* L x 6; may be NULL when line_optimized is */
    double* out_pluecker;               /* L x 6 */
    uint8_t* out_status;                /* L */
} plp_loop_ba_propagate_lines_args;
/* PLP_ERR_INVALID_ARG: NULL ctx / args, negative L or F, a NULL required array of non-zero size; PLP_ERR_UNSUPPORTED for F > 4096.
 * _device: DEVICE pointers, one lane per line (k_loop_ba_propagate_lines), asynchronous.  _host: HOST pointers, staged, synchronous.  The
 * host build returns L, or the negated plp_status. */
plp_status plp_loop_ba_propagate_lines_device(plp_matcher* ctx, const plp_loop_ba_propagate_lines_args* args, void* hip_stream);
plp_status plp_loop_ba_propagate_lines_host(plp_matcher* ctx, const plp_loop_ba_propagate_lines_args* args);
int32_t plp_model_loop_ba_propagate_lines_host(const plp_loop_ba_propagate_lines_args* args);

/* landmark::compute_descriptor (src/PLPSLAM/data/landmark.cc:181-245) and Line::compute_descriptor
 * (data/landmark_line.cc:256-320), the search part, for L landmarks at once: landmark l owns the
 * descriptors descs[offsets[l] .. offsets[l+1]) (32 B rows, observation order); best_idx[l] = the row (relative to
 * offsets[l]) whose median Hamming distance to all rows of the landmark -- itself included, rank (unsigned)(0.5 * (n - 1)) --
 * is smallest, first such row; -1 for a landmark without rows.  At most 1024 rows per landmark: _host checks it (and that the offsets
 * ascend) and returns PLP_ERR_UNSUPPORTED with nothing written; _device cannot see the offsets and takes any n, but its kernel packs the
 * row into 16 bits of the key it minimises, so on the device entry the limit is the caller's to keep. */
plp_status plp_landmark_descriptor_device(plp_matcher* ctx, const uint8_t* d_descs, const int32_t* d_offsets, int32_t L, int32_t* d_best_idx,
                                          void* hip_stream);
plp_status plp_landmark_descriptor_host(plp_matcher* ctx, const uint8_t* descs, const int32_t* offsets, int32_t L, int32_t* best_idx);

/* Diagnostics: {exact full rescans, resolve rounds, 0, 0} accumulated over all calls of this context (synchronous). */
plp_status plp_match_debug_counters(plp_matcher* ctx, int64_t* out4);
/* The kernels plp_match_device / plp_match_host run for a call of this shape; host code only, no context or device.  Reads mode, B, n_cap,
 * m_cap, t_count_hint, grid.cols / grid.rows and whether t_x_right is NULL (no other pointer).  out4 = {top-k kernel, family, queries per
 * workgroup, resolve kernel}:
 *   top-k   1 k_match_prep + k_match_topk_cells, 2 k_match_topk_lds, 3 k_match_topk_lanes<family>, 4 k_match_topk<family>, 5 k_match_fuse
 *   family  0 none (k_match_fuse), 1 line, 2 group (BOW, TRIANGULATION), 3 point, 4 grid (the sorted resolve after k_match_prep)
 *   qpb     queries per workgroup of k_match_topk_cells / k_match_topk_lds, 0 for the others
 *   resolve 1 k_match_resolve_sorted, 2 k_match_resolve_generic<family>, 0 none (fuse modes)
 * An empty side (n_cap = 0 or m_cap = 0) runs no kernel: all four 0. */
plp_status plp_match_debug_plan(const plp_match_args* a, int32_t* out4);

/* compute_descriptor_distance_32 over all pairs (match/base.h:43-68): dist[q*nt + t], u16.
 * Device pointers, asynchronous.  (K16: input of brute-force style matchers on the host side.) */
plp_status plp_hamming_matrix_device(plp_matcher* ctx, const uint8_t* d_q, int32_t nq, const uint8_t* d_t, int32_t nt,
                                     uint16_t* d_dist, void* hip_stream);
plp_status plp_hamming_matrix_host(plp_matcher* ctx, const uint8_t* q, int32_t nq, const uint8_t* t, int32_t nt, uint16_t* dist);

#ifdef __cplusplus
}
#endif
#endif /* PLP_FRONT_H */
