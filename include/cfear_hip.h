/*
 * cfear_hip.h -- C-ABI of libcfear_hip.so: the MI355X (gfx950) implementation of the CFEAR
 * scan-registration hot path of TBV Radar SLAM (dan11003/tbv_slam_public).
 *
 * The reference has no FFI layer: its boundary is the C++ class API of the catkin library
 * `cfear_radarodometry` (cfear_radarodometry/CMakeLists.txt:46-72).  Each entry point below names
 * the reference function(s) it replaces (paths relative to
 * cfear_radarodometry/{include,src}/cfear_radarodometry/).  INTEGRATION.md shows the shim a
 * maintainer adds inside radarDriver / MapPointNormal / n_scan_normal_reg to call them.
 * Three neighbours of the path follow the same rules further down: covariance by cost sampling
 * (odometrykeyframefuser.cpp:261-380), CorAl alignment quality (coral_alignment_quality) and the radar
 * Scan Context arithmetic (place_recognition_radar) -- SURVEY.md 8(f).
 *
 * Conventions
 *   - plain C: pointers + sizes, caller-owned buffers, opaque handles, no C++/torch types;
 *   - every function returns an int status (CFEAR_OK = 0, < 0 = error); nothing exits or throws
 *     (the reference calls exit(0) on several errors, e.g. pointnormal.cpp:72-75);
 *   - data pointers may be HOST or DEVICE memory of the context's GPU (detected with
 *     hipPointerGetAttributes); all buffers of one call must live in the same space;
 *   - one cfear_ctx per host thread / HIP stream; calls on different contexts are independent
 *     (the reference builds a fresh n_scan_normal_reg per loop-closure candidate on the
 *     loop-closure thread, tbv_slam/src/tbv_slam/loopclosure.cpp:56);
 *   - calls with host pointers are synchronous; calls with device pointers are enqueued on the
 *     context's stream (use cfear_ctx_synchronize) unless they return values through host
 *     scalars, in which case they synchronise themselves;
 *   - float parameters that the reference holds as float (radarDriver::Parameters,
 *     radar_driver.h:40-45) are float here and widened to double exactly where the reference
 *     widens them.
 */
#ifndef CFEAR_HIP_H
#define CFEAR_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CFEAR_ABI_VERSION 1

/* ---- status codes ------------------------------------------------------------------------ */
#define CFEAR_OK 0
#define CFEAR_ERR_INVALID_ARGUMENT (-1)
#define CFEAR_ERR_HIP (-2)              /* a HIP runtime call failed; see cfear_last_error     */
#define CFEAR_ERR_CAPACITY (-3)         /* an output/workspace capacity was exceeded           */
#define CFEAR_ERR_TOO_FEW_RESIDUALS (-4)/* n_scan_normal.cpp:368-369, 444-447                  */
#define CFEAR_ERR_SOLVER (-5)           /* !summary_.IsSolutionUsable() (n_scan_normal.cpp:449)*/
#define CFEAR_ERR_EMPTY_CLOUD (-6)      /* pointnormal.cpp:72-75 ("error, cloud empty")        */
#define CFEAR_ERR_NO_DEVICE (-7)        /* no HIP device / kernels not loadable                */
#define CFEAR_ERR_IO (-8)               /* a file could not be opened / read / written         */
#define CFEAR_ERR_FORMAT (-9)           /* a file is not a simple_graph archive this reader understands */

/* ---- enums (values follow the reference's enums) ------------------------------------------ */
enum cfear_cost_metric { CFEAR_P2P = 0, CFEAR_P2L = 1, CFEAR_P2D = 2 };          /* registration.h:55 */
enum cfear_loss_type { CFEAR_LOSS_NONE = 0, CFEAR_LOSS_HUBER = 1, CFEAR_LOSS_CAUCHY = 2,
                       CFEAR_LOSS_SOFTLONE = 3, CFEAR_LOSS_COMBINED = 4,
                       CFEAR_LOSS_TUKEY = 5 };                                    /* registration.h:60 */
enum cfear_weight_option { CFEAR_W_UNIFORM = 0, CFEAR_W_SIM_N = 1, CFEAR_W_SIM_DIRECTION = 2,
                           CFEAR_W_SIM_SCALE = 3, CFEAR_W_COMBINED = 4 };         /* registration.h:50 */
enum cfear_filter_type { CFEAR_FILTER_KSTRONG = 0, CFEAR_FILTER_CACFAR = 1 };     /* radar_driver.h:25 */

/* ---- context ------------------------------------------------------------------------------ */
typedef struct cfear_ctx cfear_ctx;

int cfear_abi_version(void);
const char* cfear_status_string(int status);
/* hip_stream: a hipStream_t to enqueue on (e.g. torch's current stream; hipStreamLegacy / hipStreamPerThread are
 * accepted too), or NULL to create a private non-blocking stream.                                   */
int cfear_ctx_create(int device, void* hip_stream, cfear_ctx** out);
int cfear_ctx_destroy(cfear_ctx* ctx);
int cfear_ctx_synchronize(cfear_ctx* ctx);
/* ctx NULL: the text of the calling thread's last refusal by a call that was given no context (the calls that check
 * their host arguments before they need one); empty if there was none.                                               */
const char* cfear_last_error(const cfear_ctx* ctx);
/* The hipStream_t the context enqueues on (the caller's, or the private one cfear_ctx_create made): lets the host
 * order other work -- a collective, a copy -- behind the library's kernels without a host synchronisation.        */
int cfear_ctx_get_stream(const cfear_ctx* ctx, void** hip_stream);
/* Context options.  None is needed in production: they are TEST / MEASUREMENT hooks that select between routes the
 * library otherwise chooses by itself, so that the parity tests can drive every route with ordinary inputs and an A/B
 * run can compare two routes inside one process.  The library never reads the environment.
 *   CFEAR_OPT_FUSED_DECODE   1 (default): [range bins][azimuths] sweeps are decoded inside the filter kernels
 *                            (radar_driver.cpp:74-90 fused into the sweep); 0: rotation kernel + row sweep.  Read when
 *                            an odometry object is created and per filter call.
 *   CFEAR_OPT_MATCHER_LDS_KB 0 (default): the matcher sizes its LDS by the batch; 8..160: every registration runs in
 *                            that many KB, so that ordinary scans exercise the keyframe groups and the global tail of
 *                            the correspondence arrays (which only unusually large registrations reach otherwise).
 *   CFEAR_OPT_MATCHER_WAVES  0 (default): wavefronts per registration chosen by the batch; 2, 4, 8, 16 force a form.
 *   CFEAR_OPT_HOST_TIMELINE  1: the batched odometry prints where the host spends a frame (every 256 calls), and
 *                            cfear_sc_detect_batch where it spends every call (one line on stderr).
 *   CFEAR_OPT_SC_QUERY_CHUNK 0 (default): cfear_sc_detect_sequence and cfear_sc_detect_batch size their query chunks by a
 *                            device budget; n >= 1: at most n query nodes per chunk, so that small graphs cross chunk
 *                            boundaries (in a batch the chunks run over the concatenated detected nodes of all graphs).
 *   CFEAR_OPT_PGO_GRAPH_CHUNK n >= 1: cfear_pgo_solve_batch takes at most n graphs per chunk (on top of its device budget),
 *                            so that small batches cross chunk boundaries; INT32_MAX lifts the cap again.  A context that
 *                            never set it reads 0 and sizes its chunks by the budget alone; 0 itself is not a cap and,
 *                            unlike the options above, is refused.
 *   CFEAR_OPT_REPLAY_CHUNK   0 (default): cfear_odometry_replay_clouds sizes its frame chunks by the free device memory;
 *                            n >= 1: at most n frames per chunk, so that a short trace crosses chunk boundaries inside
 *                            a keyframe window.  (Numbered apart from the enum: the enum's count is part of the pinned ABI.)
 *   CFEAR_OPT_KSTRONG_ROW_PAIRS 1 (default): the k-strongest row sweep of 4-byte-aligned images of at most 4096 bins, without
 *                            peaks, gives one wavefront two adjacent rows and selects both in one ranking pass when they
 *                            hold at most 64 candidates together; 0: one row per wavefront, the table cfear_kstrong_plan
 *                            describes.  The results are the same bit for bit.  Read per filter call.  (Numbered apart
 *                            from the enum, as above.)
 * Returns CFEAR_ERR_INVALID_ARGUMENT for an unknown option or a value outside its range.                          */
enum cfear_option { CFEAR_OPT_FUSED_DECODE = 0, CFEAR_OPT_MATCHER_LDS_KB = 1, CFEAR_OPT_MATCHER_WAVES = 2,
                    CFEAR_OPT_HOST_TIMELINE = 3, CFEAR_OPT_SC_QUERY_CHUNK = 4, CFEAR_OPT_PGO_GRAPH_CHUNK = 5, CFEAR_OPT_COUNT = 6 };
#define CFEAR_OPT_REPLAY_CHUNK 100
#define CFEAR_OPT_KSTRONG_ROW_PAIRS 101
int cfear_ctx_set_option(cfear_ctx* ctx, int32_t option, int64_t value);
int cfear_ctx_get_option(const cfear_ctx* ctx, int32_t option, int64_t* value);
/* Per-kernel-family device time measured with hipEvents on the context's stream.
 * enable=1 brackets every launch with events (adds a sync per read-out, not per launch); enable=2 only the polar
 * filter's row kernels (kstrongest_rows / cacfar_rows: the one HBM-bound launch of the path), which costs a batched
 * pipeline 0.3 % instead of 1.7 %.
 * cfear_ctx_profile_read: names[i] (static strings), total_ms[i], launches[i], up to cap rows;
 * returns the number of rows; reset != 0 clears the accumulators.                             */
int cfear_ctx_profile_enable(cfear_ctx* ctx, int enable);
int cfear_ctx_profile_read(cfear_ctx* ctx, const char** names, double* total_ms, int64_t* launches,
                           int cap, int reset);

/* ---- F: polar filters ----------------------------------------------------------------------
 * Replaces radarDriver::Process (radar_driver.cpp:48-73) =
 *   StructuredKStrongest ctor + FilterKstrongest      radar_filters.cpp:198-237
 *   getPeaksFilteredPointCloud(cloud,false)           radar_filters.cpp:300-337
 *   getPeaksFilteredPointCloud(peaks,true) -> AxialNonMaxSupress   radar_filters.cpp:238-298
 *   AzimuthCACFAR::getFilteredPointCloud               cfar.cpp:35-71
 * Image: row-major uint8, rows = azimuths, cols = range bins, `stride` bytes between rows,
 * `batch_stride` bytes between the `batch` images.                                            */
typedef struct cfear_polar_desc {
  int32_t rows, cols, stride, batch;
  int64_t batch_stride;
} cfear_polar_desc;

/* Image decode of the non-Oxford sensors.  Replaces cv::rotate(image, image, ROTATE_90_COUNTERCLOCKWISE) in
 * radarDriver::Callback (radar_driver.cpp:74-90): those drivers publish the sweep as [range bins][azimuths];
 * the filters want rows = azimuths.  src_desc describes the SOURCE images (rows = range bins, cols = azimuths);
 * dst holds batch images of cols x rows bytes, dst[i][j] = src[j][cols - 1 - i].  src and dst both host or both
 * device; they must not overlap.                                                                             */
int cfear_polar_rotate_ccw(cfear_ctx* ctx, const uint8_t* src, const cfear_polar_desc* src_desc, uint8_t* dst,
                           int32_t dst_stride, int64_t dst_batch_stride);

typedef struct cfear_kstrong_params {   /* radarDriver::Parameters, radar_driver.h:40-45 */
  int32_t k_strongest;                  /* >= 1, <= 1024 */
  float z_min;                          /* converted float -> int -> uchar like radar_driver.cpp:58 */
  float range_res;
  float min_distance;
  int32_t want_peaks;                   /* also run AxialNonMaxSupress */
} cfear_kstrong_params;

/* All output pointers are optional (NULL = not wanted) and per image b of the batch:
 *   sel_range     int32 [batch][rows][k]  range bins kept per azimuth, ascending (intensity,range)
 *                                          order (= dense_filtered_), padded with -1
 *   sel_intensity uint8 [batch][rows][k]  their intensities, padded with 0
 *   sel_count     int32 [batch][rows]
 *   is_peak       uint8 [batch][rows][k]  1 where AxialNonMaxSupress keeps the bin (want_peaks)
 *   xyzi          float [batch][rows*k][4] compacted PointXYZI cloud (x,y,z=0,intensity),
 *                                          rows ascending, only bins > ceil(min_distance/range_res)
 *   n_points      int32 [batch]
 *   xyzi_peaks / n_peaks: the same for the peaks cloud (want_peaks)                           */
typedef struct cfear_kstrong_out {
  int32_t* sel_range;
  uint8_t* sel_intensity;
  int32_t* sel_count;
  uint8_t* is_peak;
  float* xyzi;
  int32_t* n_points;
  float* xyzi_peaks;
  int32_t* n_peaks;
} cfear_kstrong_out;

int cfear_filter_kstrongest(cfear_ctx* ctx, const uint8_t* polar, const cfear_polar_desc* desc,
                            const cfear_kstrong_params* par, const cfear_kstrong_out* out);

/* Which k-strongest row-sweep kernel a call launches: the selection the filter call above, the row-key call below and the
 * batched odometry make from the descriptor, the parameters and the image address, reported so that a test can name the
 * kernel instantiation its input reaches.  Pure host code: no context, no device, no GPU call.
 *   desc          the images as the row sweep gets them (rows = azimuths)
 *   base_address  the address of the first image's first byte in device memory; only its low four bits are looked at, so
 *                 the address modulo 16 serves as well
 * kstrongest_rows_kernel<NCHUNK, VEC, MASK>:
 *   nchunk        1, 2, 4 or 8 chunks of 1024 bins per row (16 bytes per lane and chunk): the smallest that covers cols
 *   vec           rows are read in 16-byte pieces: address, stride and batch stride are multiples of 4 (else byte by byte)
 *   mask          uchar((int)z_min) == 0: zero padding would pass the candidate test, so the byte-validity masks are applied
 *   table_index   4 log2(nchunk) + 2 vec + mask, 0 .. 15: the entry of the dispatch table the launcher takes its kernel
 *                 from -- the launcher reads THIS plan, so the report cannot differ from the launch
 *   u_zmin        the candidate threshold, (uint8_t)(int)z_min (radar_driver.cpp:58, radar_filters.cpp:212): 256 -> 0, 0.9 -> 0,
 *                 300 -> 44, -1 -> 255;  thi: u_zmin >= 128 (the other form of the byte compare)
 *   min_range_bin ceil(min_distance / range_res) (radar_filters.cpp:315): only kept bins beyond it enter the clouds
 *   kpad          entries of a row's key list, max(k rounded up to 4, 64);  lds_bytes: the launch's dynamic LDS (four rows)
 *   refused       0, or why the filter call refuses these arguments (everything else is 0 then): CFEAR_KSTRONG_REFUSED_*
 * Returns CFEAR_ERR_INVALID_ARGUMENT for a null pointer only.                                                              */
#define CFEAR_KSTRONG_REFUSED_DESC 1       /* a bad descriptor: rows, cols, batch < 1, stride < cols, overlapping images */
#define CFEAR_KSTRONG_REFUSED_COLS 2       /* cols > 8192 */
#define CFEAR_KSTRONG_REFUSED_K 3          /* k_strongest outside [1, 1024] */
#define CFEAR_KSTRONG_REFUSED_RANGE_RES 4  /* range_res <= 0 */
struct cfear_kstrong_plan {
  int32_t nchunk, vec, mask, table_index;
  int32_t u_zmin, thi, min_range_bin, kpad;
  int32_t refused, pad;
  int64_t lds_bytes;
};
int cfear_kstrong_plan(const cfear_polar_desc* desc, const cfear_kstrong_params* par, uint64_t base_address,
                       struct cfear_kstrong_plan* out);

/* The filter stage of the batched odometry on its own (device memory only): radarDriver::Callback's decode
 * (radar_driver.cpp:74-90), FilterKstrongest (radar_filters.cpp:209-237) and the selection of
 * getPeaksFilteredPointCloud(cloud, false) (radar_filters.cpp:309-337) in ONE pass over the sweep.  Per azimuth row the kept
 * bins beyond ceil(min_distance / range_res) as packed keys (intensity << 24 | range bin), in the reference's cloud order
 * (ascending (intensity, range)):
 *   row_keys   uint32 [batch][azimuths][k]     (k = k_strongest <= 64; entries beyond the row's count are unspecified)
 *   row_counts int32  [batch][azimuths][2]     {kept bins of the row, 0}
 * flags: CFEAR_ROWKEYS_BINS_MAJOR -- the images are [range bins][azimuths] (desc->rows = bins, desc->cols = azimuths) and
 * row r of the result is source column cols - 1 - r (cv::ROTATE_90_COUNTERCLOCKWISE).  The rotated image is never built:
 * one streaming pass lists, per azimuth, the bins >= uchar(z_min) (the only ones the filter can keep), a second picks the
 * k strongest of each list; azimuths with more than 256 such bins have their 16-column tile transposed in LDS and swept
 * there (CFEAR_ROWKEYS_TILE_SWEEP: every tile takes that route).  Needs 16-byte aligned images, cols % 16 == 0, rows % 4 == 0
 * and <= 4096 bins; any other geometry, a batch of fewer than 128 images (unless a route flag asks otherwise), or
 * CFEAR_ROWKEYS_TWO_PASS, takes cfear_polar_rotate_ccw's kernel into a workspace first -- same result.  The lists cost time
 * per bin >= z_min: beyond ~80 of them per azimuth CFEAR_ROWKEYS_TWO_PASS is the quicker route (the batched odometry measures
 * this and switches by itself).  want_peaks is ignored.                                                                        */
#define CFEAR_ROWKEYS_BINS_MAJOR 1
#define CFEAR_ROWKEYS_TWO_PASS 2
#define CFEAR_ROWKEYS_TILE_SWEEP 4
#define CFEAR_ROWKEYS_ROUTE_LISTS 16   /* candidate lists in global memory (default only when an image's lists do not fit the LDS) */
#define CFEAR_ROWKEYS_ROUTE_IMAGE 32   /* one workgroup per image, lists in LDS (the default route), whatever the batch size */
int cfear_filter_kstrongest_rowkeys(cfear_ctx* ctx, const uint8_t* polar, const cfear_polar_desc* desc,
                                    const cfear_kstrong_params* par, int32_t flags, uint32_t* row_keys, int32_t* row_counts);

/* Row keys of SEVERAL k-strongest parameter sets from ONE sweep.  FilterKstrongest keeps the k largest (intensity, range)
 * pairs among the bins >= uchar(z_min) and the near cut applies only when the cloud is built, so for k_c <= k_sup and
 * uchar(z_min_c) >= uchar(z_min_sup) the selection of (k_c, z_min_c) is the top k_c entries of the selection of
 * (k_sup, z_min_sup) restricted to intensity >= uchar(z_min_c).  sel_range / sel_intensity / sel_count: the lists
 * cfear_filter_kstrongest leaves for n_images images of `rows` azimuths at (k_sup, z_min_sup), k_sup <= 64.  Class c takes
 * image classes[c].image and gets what cfear_filter_kstrongest_rowkeys gives that image with the class's own parameters, bit
 * for bit, at a row stride of 64 keys:
 *   row_keys   uint32 [n_classes][rows][64]   (entries beyond the row's count are not written)
 *   row_counts int32  [n_classes][rows][2]    {kept bins of the row, 0}
 * All buffers are device memory except `classes` (host).  Refused with CFEAR_ERR_INVALID_ARGUMENT before any launch: k_sup
 * outside [1, 64]; a class with k_strongest outside [1, k_sup], uchar(z_min) below that of z_min_sup, image outside
 * [0, n_images) or range_res <= 0; n_images, rows or n_classes < 1; null pointers; host pointers where device memory is
 * required (and a device pointer for classes).                                                                            */
typedef struct cfear_rowkeys_class { int32_t image; int32_t k_strongest; float z_min, range_res, min_distance; } cfear_rowkeys_class;
int cfear_kstrong_rowkeys_derive(cfear_ctx* ctx, const int32_t* sel_range, const uint8_t* sel_intensity, const int32_t* sel_count,
                                 int32_t n_images, int32_t rows, int32_t k_sup, float z_min_sup,
                                 const cfear_rowkeys_class* classes, int32_t n_classes, uint32_t* row_keys, int32_t* row_counts);

/* Legacy filter: replaces k_strongest_filter / InsertStrongestK (radar_filters.cpp:25-78), which CorAl's standalone
 * kstrongRadar scan type still calls (coral_alignment_quality/src/alignment_checker/ScanType.cpp:104-114); TBV itself uses
 * the structured filter above.  Different rule: the first bin >= z_min of a row sets a floor, later bins
 * <= the running minimum are rejected even while fewer than k are held, ties at the cut keep the SMALLER ranges, points
 * sit at bin EDGES (range_res * bin) with a float azimuth, and the near cut is x^2 + y^2 > min_distance^2.  z_min,
 * range_res, min_distance are doubles as in the reference's signature.  xyzi float [batch][cap_points][4] (rows ascending,
 * within a row descending intensity, ascending range on ties -- the order of a stable sort; libstdc++'s std::sort is stable
 * up to 16 elements, i.e. k <= 15), n_points int32 [batch]; all three buffers host or all device.               */
int cfear_filter_kstrongest_legacy(cfear_ctx* ctx, const uint8_t* polar, const cfear_polar_desc* desc, int32_t k_strongest,
                                   double z_min, double range_res, double min_distance, float* xyzi, int32_t* n_points,
                                   int32_t cap_points);

typedef struct cfear_cacfar_params {    /* AzimuthCACFAR ctor, cfar.cpp:28-33; radar_driver.cpp:54 */
  int32_t window_size;                  /* cells per side */
  int32_t nb_guard_cells;
  float false_alarm_rate;
  float range_res;
  float z_min;                          /* static_threshold */
  float min_distance;
  double max_distance;                  /* radar_driver.cpp:54 passes 400.0 */
} cfear_cacfar_params;

/* xyzi float [batch][cap_points][4], n_points int32 [batch]; det_mask (optional) uint8
 * [batch][rows][cols] 0/1 per bin.  Detections are ordered (row, bin) like cfar.cpp:37-70.
 * A batch element with more than cap_points detections yields CFEAR_ERR_CAPACITY.            */
int cfear_filter_cacfar(cfear_ctx* ctx, const uint8_t* polar, const cfear_polar_desc* desc,
                        const cfear_cacfar_params* par, float* xyzi, int32_t* n_points,
                        int32_t cap_points, uint8_t* det_mask);

/* Which CA-CFAR kernel a call launches, and with which geometry: the selection cfear_filter_cacfar,
 * cfear_filter_cacfar_rowkeys and the batched odometry make from the filter's parameters and the row length, reported so
 * that a test can name the kernel instantiation its input reaches.  Pure host code: no context, no device, no GPU call.
 *   desc   the images as the filter call gets them (with CFEAR_ROWKEYS_BINS_MAJOR: rows = range bins, cols = azimuths)
 *   flags  CFEAR_ROWKEYS_BINS_MAJOR      the fused decode (cacfar_cols_kernel); implies the key output
 *          CFEAR_CACFAR_PLAN_KEYS        the key output of cfear_filter_cacfar_rowkeys / the batched odometry
 *                                        (cfear_filter_cacfar, the bitmap output, passes neither)
 *          CFEAR_CACFAR_PLAN_BASE(addr)  the image address modulo 16 (0 when omitted): rows are read in 16-byte pieces
 *                                        only from 4-byte boundaries, the fused decode wants 16
 * A row is cut into nch chunks of 256 D bins (D dwords per lane), the last one of 256 DL bins; colsp = the bins of all chunks.
 *   bin_lo, bin_hi  the bins that can pass the range window (min_distance < range_res bin < max_distance), [lo, hi); both 0
 *                   when nothing can pass (the window is empty, or z_min >= 255)
 *   need_cols       the bins the arithmetic of [bin_lo, bin_hi) reads: min(row length, bin_hi - 1 + guard + window), rounded
 *                   up to 16; nothing beyond is loaded
 *   lut_ok          the integer decision table exists (a finite scaling > 0 that fits it); pre_on: the lower-bound pre-filter
 *                   runs (lut_ok, guard + window <= 1024 and an aligned quad inside a window of every bin of an 8-bin block)
 *   wide            rows kernel, D = 4 only: more than four chunks (the eight-chunk instantiation)
 *   pad_lo, pad_hi  guard entries of the prefix table before bin 0 / beyond the row; lds_bytes: the launch's dynamic LDS
 *   table_index     the entry of the dispatch table the launcher takes its kernel from -- the launcher reads THIS plan, so
 *                   the report cannot differ from the launch.  Rows kernel (cols_route = 0), template arguments
 *                   <D, NCH, DL, KEYS, PRE>:
 *                      0 ..  7  D = 4:  4 wide + 2 keys + pre                        <4, 4 | 8, 4, keys, pre>
 *                      8 .. 11  D = 6, whole chunks:  8 + 2 (nch > 2) + keys         <6, 2 | 6, 6, keys, 1>
 *                     12 .. 13  D = 6, DL = 4 (two chunks):  12 + keys               <6, 2, 4, keys, 1>
 *                     14 .. 17  D = 8, whole chunks:  14 + 2 (nch > 2) + keys        <8, 2 | 4, 8, keys, 1>
 *                     18 .. 19  D = 8, DL = 6 (two chunks):  18 + keys               <8, 2, 6, keys, 1>
 *                   fused decode (cols_route = 1), <D, NCH, DL, PRE>:
 *                      0 .. 1   D = 4:  pre            <4, 4, 4, pre>
 *                      2, 3     D = 6:  DL = 4, 6      <6, 2, DL, 1>
 *                      4, 5     D = 8:  DL = 6, 8      <8, 2, DL, 1>
 *                   (D = 6 / 8 exist with the pre-filter only.  A shorter last chunk of D = 6, DL = 2 and of D = 8, DL = 2 / 4
 *                   never costs less than a geometry tried before it, so no parameter set selects it and none is built.)
 *   piece_rows      rows route: how many of the batch * rows rows are read from memory in 16-byte pieces; the others (rows on
 *                   addresses or strides that are no multiple of 4, and rows of a ragged image -- cols % 16 != 0 -- whose
 *                   last piece would end beyond rows * stride) are copied byte by byte.  total_rows = batch * rows.
 *   cols_supported  with CFEAR_ROWKEYS_BINS_MAJOR: the fused decode takes this geometry (azimuths % 16 == 0, bins % 16 == 0,
 *                   stride, batch_stride and address multiples of 16, rows * stride < 2^31, colsp <= 4096 and
 *                   lds_bytes <= 160 KiB - 256); where it is 0 cfear_filter_cacfar_rowkeys refuses the call and the batched
 *                   odometry rotates first.  0 without the flag.
 * Returns CFEAR_ERR_INVALID_ARGUMENT for a null pointer, a bad descriptor (as the filter calls refuse it) or bad
 * parameters (window_size < 1, nb_guard_cells < 0, range_res <= 0).                                                          */
#define CFEAR_CACFAR_PLAN_KEYS 0x100
#define CFEAR_CACFAR_PLAN_BASE(addr) ((int32_t)(((uintptr_t)(addr)) & 15) << 12)
struct cfear_cacfar_plan {
  int32_t D, DL, nch, wide;
  int32_t pre_on, lut_ok;
  int32_t need_cols, colsp, bin_lo, bin_hi;
  int32_t pad_lo, pad_hi;
  int32_t keys, cols_route, cols_supported, table_index;
  int64_t lds_bytes, piece_rows, total_rows;
};
int cfear_cacfar_plan(const cfear_polar_desc* desc, const cfear_cacfar_params* par, int32_t flags, struct cfear_cacfar_plan* out);

/* The CA-CFAR filter stage of the batched odometry on its own (device memory only): what cfear_odometry_process runs ahead of
 * the surface-point stage when filter_type = CFEAR_FILTER_CACFAR.  Per azimuth row the detections of
 * AzimuthCACFAR::getFilteredPointCloud (cfar.cpp:35-71) as packed keys instead of a cloud:
 *   row_keys   uint32 [batch][azimuths][kcap]  key = intensity << 24 | range bin (intensity = the bin's byte; the bin fits 13
 *                                              bits); a row's keys are in ASCENDING BIN order, the order of cfar.cpp's loop
 *   row_counts int32  [batch][azimuths][2]     {detections of the row, 0}
 * A row with more than kcap detections leaves its full count in row_counts and its FIRST kcap keys (the kcap smallest bins);
 * the others are dropped (the batched odometry reports such a scan with CFEAR_ERR_CAPACITY).  Entries of row_keys beyond
 * min(count, kcap) are not written.  The surface-point stage places a key's point at range_res * bin (the bin's edge,
 * cfar.cpp:43) and azimuth row / azimuths * 2 pi.
 * flags: CFEAR_ROWKEYS_BINS_MAJOR -- the images are [range bins][azimuths] and row r of the result is source column
 * cols - 1 - r (cv::ROTATE_90_COUNTERCLOCKWISE), decoded inside the filter; a geometry for which cfear_cacfar_plan reports
 * cols_supported = 0 returns CFEAR_ERR_INVALID_ARGUMENT (rotate with cfear_polar_rotate_ccw first, as the odometry does).
 * Other flag bits are refused.  kcap >= 1.                                                                                  */
int cfear_filter_cacfar_rowkeys(cfear_ctx* ctx, const uint8_t* polar, const cfear_polar_desc* desc,
                                const cfear_cacfar_params* par, int32_t flags, uint32_t* row_keys, int32_t* row_counts,
                                int32_t kcap);

/* Cen and Newman's 2018 landmark detector: replaces cen2018features (coral_alignment_quality/src/alignment_checker/
 * Utils.cpp:348-434) and the cloud loop of Cen2018Radar (ScanType.cpp:68-88).  Per azimuth row: f = v / 255, q = f - mean(f)
 * (serial float sum), p = q filtered with 3 * sigma_gauss Gaussian taps (BORDER_REFLECT101), sigma = sqrt(mean of 2 q^2 over
 * the bins with q < 0) (0.034 when there is none), y = q (1 - N(q - p)) + p (N(q - p) - N(p)) with N(x) = exp(-x^2 / 2 sigma^2);
 * every maximal run of bins with y > zq * sigma gives ONE target, element len / 2 of the run.  Points sit at the bin EDGE
 * (range_res * bin), azimuth (row + 1) / rows * 2 pi, intensity = the raw byte; ordered (row, bin).
 * min_range_bins: the reference hands sensor_min_distance (2.5, metres) to an `int min_range` that its loop uses as a BIN
 * index, so its near cut is bin 2 whatever the resolution; the parameter is therefore in bins and defaults to 2, not to
 * min_distance / range_res.
 * xyzi float [batch][cap_points][4], n_points int32 [batch]; optional: targets int32 [batch][cap_points][2] (azimuth, bin),
 * det_mask uint8 [batch][rows][cols] (y > thres; 0 below min_range_bins), row_stats float [batch][rows][2] (mean, sigma).
 * The image and every output are all host or all device memory.  An image with more than cap_points targets yields
 * CFEAR_ERR_CAPACITY (n_points then holds the counts, the buffers the first cap_points).  CFEAR_ERR_INVALID_ARGUMENT:
 * sigma_gauss even, below 1 or above 341, 3 * sigma_gauss > cols, min_range_bins < 0, zq not finite, range_res not finite.
 * The call waits for the counts on every route (it is synchronous).                                                      */
typedef struct cfear_cen2018_params {
  float zq;                             /* threshold in noise sigmas: 3.0 (ScanType.cpp:72) */
  int32_t sigma_gauss;                  /* 17; the filter has 3 * sigma_gauss taps */
  int32_t min_range_bins;               /* 2 (see above) */
  int32_t pad;
  double range_res;                     /* 0.04328 (ScanType.h:62) */
} cfear_cen2018_params;
void cfear_cen2018_params_default(cfear_cen2018_params* par);
int cfear_filter_cen2018(cfear_ctx* ctx, const uint8_t* polar, const cfear_polar_desc* desc, const cfear_cen2018_params* par,
                         float* xyzi, int32_t* n_points, int32_t cap_points, int32_t* targets, uint8_t* det_mask,
                         float* row_stats);

/* Cen and Newman's 2019 landmark detector: replaces cen2019features (coral_alignment_quality/src/alignment_checker/
 * Utils.cpp:436-594, declared in Utils.h:46), behind `evaluate_scans --scan-type cen2019`.  The reference stops at `targets`
 * (Cen2019Radar's constructor body is commented out, ScanType.cpp:90-101); the cloud here is Cen2018Radar's: range_res * bin
 * (the bin EDGE), azimuth (row + 1) / rows * 2 pi, intensity = the raw byte; ordered (row, bin).
 * Per sweep, in float with one rounding per operation: f = v * float(1 / 255.0); g = |f[r+1] - f[r-1]| (BORDER_REFLECT101: 0 in
 * the first and last bin) times float(1 / double(max g)); s = f - mean(f); h = s * (1 - g); mean and mean_h are fp64 sums
 * divided by rows * cols and rounded to float.  The pixels with h > mean_h are gone through in descending h (equal h: ascending
 * row * cols + bin; the reference's std::sort leaves that open): one whose bin is unmarked marks its bin and the contiguous
 * bins with s < 0 left of it -- and right of it if bin < rows - 1, the reference's comparison -- and counts if none of those
 * was marked; the walk ends after max_points counted ones.  Per row every maximal run of marked bins from min_range_bins on that
 * an UNMARKED bin ends (a run into the last column emits nothing) and that has a marked bin of row - 1 or row + 1 (wrapping)
 * within its extent emits one target: the last bin of the run with h > 0, else its first (getMaxInRegion as written).
 * A flat sweep (max g = 0: the reference computes NaN everywhere) has no target: zero points, CFEAR_OK, mean_h NaN.
 * xyzi float [batch][cap_points][4], n_points int32 [batch]; optional: targets int32 [batch][cap_points][2] (azimuth, bin),
 * region_mask uint8 [batch][rows][cols] (the marks R), image_stats float [batch][4] (mean, max g, mean_h, h of the last
 * candidate gone through; 0 if none), counts int32 [batch][3] (candidates, fresh candidates of the sweep -- those that would
 * count with max_points unbounded --, candidates gone through: the reference's j).
 * The image and every output are all host or all device memory.  An image with more than cap_points targets yields
 * CFEAR_ERR_CAPACITY (n_points then holds the counts, the buffers the first cap_points).  CFEAR_ERR_INVALID_ARGUMENT:
 * max_points < 0 (0 is valid and marks nothing), min_range_bins < 0, range_res not finite, rows * cols > 2^22 (the fp64 sum of
 * f is exact in any order up to there), cols < 2 or > 8192, rows > 30719.  The call is synchronous.                         */
typedef struct cfear_cen2019_params {
  int32_t max_points;                   /* 1000 (Utils.h:46) */
  int32_t min_range_bins;               /* 0 */
  double range_res;                     /* 0.04328 (ScanType.h:62) */
} cfear_cen2019_params;
void cfear_cen2019_params_default(cfear_cen2019_params* par);
int cfear_filter_cen2019(cfear_ctx* ctx, const uint8_t* polar, const cfear_polar_desc* desc, const cfear_cen2019_params* par,
                         float* xyzi, int32_t* n_points, int32_t cap_points, int32_t* targets, uint8_t* region_mask,
                         float* image_stats, int32_t* counts);

/* Which landmarks of cfear_filter_cen2019 hang on the order among equal h that cen2019features' std::sort leaves open
 * (DESIGN.md sections 3 and 4.20; tests/cen2019_audit_cpu.py is the definition).  The batch, its limits and its refusals are
 * cfear_filter_cen2019's.  Per sweep, with T = rows - 1, a run a maximal stretch of bins with s < 0 and a run's touchers its own
 * candidates, the candidate right of it and the one left of it if that sits at a bin < T:
 *   a candidate is SURELY fresh if in every run it touches it alone attains the largest h among the touchers, POSSIBLY fresh if
 *   it attains it; every order's fresh candidates lie between the two sets, so every order's walk ends at an h in [h_lo, h_hi],
 *   the h of the max_points-th largest surely fresh candidate and of the max_points-th largest possibly fresh one (-inf: fewer
 *   exist, the walk goes through everything; +inf: max_points == 0).  The candidates with h > h_hi are gone through under every
 *   order, those with h < h_lo under none; the BAND between is the order's to decide (a band of one candidate is the walk's last
 *   under every order: it counts as gone through and n_band is 0).
 *   R_in / R_out: the marks from the candidates above the band / with the band, the run that straddles column T marked whole
 *   only if its largest own h sits at bins < T alone (R_in) / at some bin < T (R_out).  R_in <= R(order) <= R_out for every order.
 *   A target is CERTAIN if R_in emits it from a run that is the same maximal run (from min_range_bins on) in R_out: every order
 *   emits it, at the same bin.
 *   The WITNESS is the sweep filtered with equal h in DESCENDING row * cols + bin: one legal order's outcome.
 * n_marks_in == n_marks_out ("clear"): no order of equal h changes a mark or a target of this sweep.  It does NOT say that a
 * reference build agrees: the result is conditional on mean_h (the order of its fp64 sum is a separate open point, DESIGN.md
 * section 4.10b) and on `g /= maxg`.  An exposed sweep need not change either: n_*_changed_reversed > 0 shows that one does.
 * records [batch]; optional: targets int32 [batch][cap_points][2] (the filter's, same order), certain uint8 [batch][cap_points]
 * (1 = certain, parallel to targets), marks uint8 [batch][rows][cols] (bit 0 R_in, bit 1 R, bit 2 R_out, bit 3 the witness's R).
 * cap_points may be 0 when targets and certain are NULL.  The image and every output are all host or all device memory.  A sweep
 * with more than cap_points targets yields CFEAR_ERR_CAPACITY when targets or certain is given: every record is complete, the
 * arrays hold the first cap_points.  A flat sweep has zeros in the integer fields and NaN levels.  A sweep's record and arrays
 * are bit-identical alone and at any batch position.  The call is synchronous.                                            */
typedef struct cfear_cen2019_order_record {
  int32_t n_candidates, n_fresh;        /* as counts[0], counts[1] of the filter (this library's order)                      */
  int32_t n_sure_fresh, n_possibly_fresh;
  int32_t n_band;                       /* candidates whose processing the order decides; 0: the cut is order-free           */
  int32_t n_rows_straddle_tied;         /* rows whose straddling run has its largest own h on both sides of T, among those
                                           gone through under some order                                                      */
  int32_t n_marks_in, n_marks, n_marks_out;   /* popcounts of R_in, this library's R, R_out                                  */
  int32_t n_targets, n_targets_certain; /* this library's targets; those certain under every order                           */
  int32_t n_targets_reversed, n_targets_changed_reversed;   /* the witness: its targets, the symmetric difference with ours  */
  int32_t n_marks_changed_reversed;
  float h_hi, h_lo;
} cfear_cen2019_order_record;           /* 64 bytes */
int cfear_cen2019_order_audit(cfear_ctx* ctx, const uint8_t* polar, const cfear_polar_desc* desc, const cfear_cen2019_params* par,
                              cfear_cen2019_order_record* records, int32_t* targets, uint8_t* certain, int32_t cap_points,
                              uint8_t* marks);

/* ---- C: motion compensation ----------------------------------------------------------------
 * Replaces Compensate(cloud, mot, ccw)  utils.cpp:96-107 (+ GetRelTimeStamp utils.h:28-32).
 * xyzi float [n][4] modified in place; mot = (x, y, theta) of the previous motion.           */
int cfear_compensate(cfear_ctx* ctx, float* xyzi, int32_t n, const double mot[3], int32_t ccw);

/* ---- N: oriented surface points ------------------------------------------------------------
 * cfear_scan is the device-resident MapPointNormal (pointnormal.h:110-243): the `cell`s plus the
 * float copy of their means that the matcher searches (pointnormal.cpp:151-162).              */
typedef struct cfear_scan cfear_scan;

typedef struct cfear_cell {             /* class cell, pointnormal.h:45-105 */
  double mean[2];                       /* u_ */
  double normal[2];                     /* snormal_ */
  double cov[4];                        /* cov_ row-major */
  double scale;                         /* scale_ (GetPlanarity) */
  double avg_intensity;                 /* avg_intensity_ */
  double lambda_min, lambda_max;
  int32_t nsamples;                     /* Nsamples_ */
  int32_t pad;
} cfear_cell;

typedef struct cfear_feature_params {   /* MapPointNormal ctor arguments, pointnormal.cpp:65 */
  float radius;                         /* par.res */
  double downsample_factor;             /* MapPointNormal::downsample_factor (static, =1) */
  double origin[2];
  int32_t weight_intensity;
  int32_t compensate;                   /* 1: run Compensate(mot, ccw) on the cloud first
                                           (odometrykeyframefuser.cpp:146-150), in place */
  double mot[3];
  int32_t ccw;
  int32_t pad;
} cfear_feature_params;

/* Replaces `new MapPointNormal(cloud, res, origin, weight_intensity, false)`
 * (pointnormal.cpp:65-90 -> ComputeNormals :265-297 -> cell::cell :7-63 ->
 * ComputeSearchTreeFromCells :151-162).  xyzi [n][4] host or device (modified in place only if
 * compensate).  n == 0 -> CFEAR_ERR_EMPTY_CLOUD.                                              */
int cfear_scan_create(cfear_ctx* ctx, float* xyzi, int32_t n, const cfear_feature_params* par,
                      cfear_scan** out);
/* Upload precomputed cells (loop closure consumes the MapPointNormal cached in each graph node,
 * types.h:119-122; also `raw` mode, pointnormal.cpp:76-82).  cells: host array.               */
int cfear_scan_from_cells(cfear_ctx* ctx, const cfear_cell* cells, int32_t n_cells, cfear_scan** out);
int cfear_scan_size(const cfear_scan* scan);                            /* GetSize()  */
int cfear_scan_get_cells(const cfear_scan* scan, cfear_cell* out_host, int32_t cap);  /* GetCells() */
/* MapPointNormal::GetClosestIdx (pointnormal.cpp:238-254) for n_queries points p (x, y doubles): idx[i] = index of
 * the cell whose float mean is nearest to float(p) (FLANN L2_Simple in float, lowest index on ties) if that squared
 * distance is < d * d, else -1 (the reference returns an empty vector).  queries_xy / idx both host or both device. */
int cfear_scan_closest_idx(const cfear_scan* scan, const double* queries_xy, int32_t n_queries, double d, int32_t* idx);
/* The tie-aware GetClosestIdx: ALL cells at the minimum float distance.  lo[i] is exactly cfear_scan_closest_idx's answer (the
 * lowest index, -1 beyond d), hi[i] the highest cell at the same float distance and count[i] how many there are (-1 and 0
 * beyond d).  hi and count may be NULL; every buffer host or every buffer device.  d must be greater than 0.            */
int cfear_scan_closest_ties(const cfear_scan* scan, const double* queries_xy, int32_t n_queries, double d, int32_t* lo, int32_t* hi,
                            int32_t* count);
/* Diagnostic: the route the surface-point kernels served this scan on (CFEAR_SURF_PATH_*), 0 for a scan that did not come
 * from them (cfear_scan_from_cells).  The thresholds between the routes are LDS arithmetic inside the kernels; the word
 * lets a test assert where its input ran.  A scan handed out by cfear_odometry_get_scan carries the word of the stream's
 * last frame.                                                                                                        */
int cfear_scan_surface_path(const cfear_scan* scan, uint32_t* path);
#define CFEAR_SURF_PATH_KIND_MASK 3u         /* which kernels made the cells:                                          */
#define CFEAR_SURF_PATH_FAST 1u              /*   the fast pipeline (prep, sort, finish)                               */
#define CFEAR_SURF_PATH_SINGLE 2u            /*   the single-kernel path with its LDS sort (a hand-over)               */
#define CFEAR_SURF_PATH_GLOBAL 3u            /*   the global-memory path (more than 16 384 points off the fast path)   */
#define CFEAR_SURF_PATH_ROWS 0x4u            /* rows mode: the cloud arrived as per-row key lists                      */
#define CFEAR_SURF_PATH_K64 0x8u             /* fast: 64 points per thread (more than 16 384 points), else 32          */
#define CFEAR_SURF_PATH_WFLOAT 0x10u         /* fast: float weights, else one byte per weight                          */
#define CFEAR_SURF_PATH_SLABS 0x20u          /* fast: several slabs (their number is in the SLAB_COUNT field)          */
#define CFEAR_SURF_PATH_READ2 0x40u          /* fast: grid beyond 65 536 cells, the points were read a second time     */
#define CFEAR_SURF_PATH_TIER16 0x80u         /* fast: some slab held voxels of the 16-lane tier (C > 64 candidates)    */
#define CFEAR_SURF_PATH_TIER4 0x100u         /*   ... of the 4-lane tier (16 < C <= 64)                                */
#define CFEAR_SURF_PATH_TIER1 0x200u         /*   ... of the 1-lane tier (6 <= C <= 16)                                */
#define CFEAR_SURF_PATH_TOP_BUCKET 0x400u    /* fast: a voxel with more than 4 096 candidates (saturated top bucket)   */
#define CFEAR_SURF_PATH_CEN_SCRATCH 0x800u   /* fast: a split voxel's centroid went through scratch (LDS list full)    */
#define CFEAR_SURF_PATH_PREPARED 0x1000u     /* hand-over: the cloud arrived compact and compensated                   */
#define CFEAR_SURF_PATH_REASON_SHIFT 13      /* hand-over: why the fast pipeline did not take the scan                 */
#define CFEAR_SURF_PATH_REASON_MASK 0xE000u
#define CFEAR_SURF_REASON_REACH 1u           /*   downsample factor != 1 (more than one voxel per radius)              */
#define CFEAR_SURF_REASON_ROTATION 2u        /*   compensation by more than 1e5 rad (or NaN)                           */
#define CFEAR_SURF_REASON_POINTS 3u          /*   more than 32 768 points                                              */
#define CFEAR_SURF_REASON_CELLS 4u           /*   grid beyond 2^18 cells                                               */
#define CFEAR_SURF_REASON_ORDER 5u           /*   occupancy, voxel cursors and order array exceed the LDS budget       */
#define CFEAR_SURF_REASON_ROWS3 6u           /*   three grid rows exceed the staging area                              */
#define CFEAR_SURF_PATH_SLAB_COUNT_SHIFT 16  /* fast: slabs, saturating at 255                                         */
#define CFEAR_SURF_PATH_SLAB_COUNT_MASK 0xFF0000u
int cfear_scan_destroy(cfear_scan* scan);

/* N clouds -> N scans in one call: the batched counterpart of cfear_scan_create, for callers without a live fuser (loop
 * closure on fresh sweeps, scan evaluation, training data from stored clouds).  Cloud i is the lengths[i] points behind
 * xyzi + 4 * offsets[i]; offsets and lengths are host arrays counted in points, xyzi is host or device memory and is NOT
 * modified (a cloud that gets compensated is compensated in a copy).  par is shared by the batch; with par->compensate set
 * cloud i is compensated by mots[3 i .. 3 i + 2], or by par->mot when mots is NULL (then par->mot serves every cloud).
 * One arena holds all N scans, max_cells cells each (1 .. 16 384), and one launch sequence of the surface-point kernels
 * serves them (a few sequences where their scratch memory bounds a launch: 1 GiB).
 * A cloud that fails does not stop the others: status[i] (host, [n_scans]) is CFEAR_ERR_EMPTY_CLOUD for lengths[i] == 0,
 * CFEAR_ERR_CAPACITY for a scan of more than max_cells cells (or a cloud beyond 2^20 points), CFEAR_OK otherwise; the call
 * returns the first status that is not CFEAR_OK, *out is valid whenever status was written (any return but
 * CFEAR_ERR_INVALID_ARGUMENT / CFEAR_ERR_HIP) and must be destroyed.
 * cfear_scan_batch_get hands out BORROWED handles, NULL for a scan that failed: views into the arena, valid until
 * cfear_scan_batch_destroy wherever a const cfear_scan* is taken -- cfear_register_batch, cfear_scan_table_create,
 * cfear_scan_get_cells, cfear_scan_closest_idx / _ties, cfear_scan_surface_path, the audits.  cfear_scan_destroy on a
 * borrowed handle is refused with CFEAR_ERR_INVALID_ARGUMENT and frees nothing.  A scan table holds its own reference: the
 * arena stays allocated until the last table that names one of its scans is destroyed as well.  A served scan's cells and
 * route word are the bits cfear_scan_create gives on the same cloud.                                                    */
typedef struct cfear_scan_batch cfear_scan_batch;
int cfear_scan_create_batch(cfear_ctx* ctx, const float* xyzi, const int64_t* offsets, const int32_t* lengths, int32_t n_scans,
                            const cfear_feature_params* par, const double* mots, int32_t max_cells, cfear_scan_batch** out,
                            int32_t* status);
int cfear_scan_batch_size(const cfear_scan_batch* batch);
int cfear_scan_batch_get(const cfear_scan_batch* batch, int32_t i, const cfear_scan** scan);
int cfear_scan_batch_destroy(cfear_scan_batch* batch);

/* ---- M: registration -----------------------------------------------------------------------
 * n_scan_normal_reg (n_scan_normal.h:27-85, n_scan_normal.cpp) in mode
 * incremental_last_to_previous: scans[0..n-2] are fixed targets, scans[n-1] is the free source. */
typedef struct cfear_reg_params {
  int32_t cost;                         /* cfear_cost_metric; n_scan_normal_reg ctor */
  int32_t loss;                         /* cfear_loss_type   */
  double loss_limit;                    /* loss_limit_ (0.1) */
  int32_t weight_opt;                   /* cfear_weight_option */
  int32_t max_itr_association;          /* SetParameters(.,) / default 8 */
  int32_t max_itr_solver;               /* options_.max_num_iterations, default 20 */
  int32_t min_itr;                      /* min_itr_ = 3 */
  double radius;                        /* radius_ = 2.0 (registration.h:122) */
  double cov_scale;                     /* SetD2dPar */
  double regularization;                /* SetD2dPar */
  double score_tolerance;               /* 1e-5 (n_scan_normal.h:74) */
  int32_t itr;                          /* GetCost only: the object's leftover itr_ (0 if fresh) */
  int32_t pad;
} cfear_reg_params;

/* Fills the n_scan_normal_reg defaults (P2L, Huber 0.1, Uniform, 8 x 20, radius 2.0). */
void cfear_reg_params_default(cfear_reg_params* p);

typedef struct cfear_reg_result {
  double pose[3];                       /* (x, y, theta) of the source after registration */
  double score;                         /* score_ = final_cost / num_residuals (getScore) */
  double final_cost;                    /* summary_.final_cost */
  int32_t num_residuals;                /* summary_.num_residuals (elements): of the last problem that was solved -- a
                                         * registration that ends with too few residuals in a later pass keeps the pass
                                         * before's, as summary_ does; 0 when none was solved */
  int32_t outer_iters;                  /* itr_ on exit (timing key "itrs") */
  int32_t lm_iters;                     /* total LM iterations */
  int32_t status;                       /* CFEAR_OK / CFEAR_ERR_TOO_FEW_RESIDUALS / CFEAR_ERR_SOLVER */
  double last_relative_decrease;        /* summary_.iterations.back().relative_decrease */
  double reserved;                      /* diagnostic: 1.0 when the registration is one the matcher's regular form (4 wavefronts,
                                         * 40 KB of LDS) is not good at -- dense scans; a caller that streams batches keeps
                                         * the large forms switched on while it sees these; 0.0 otherwise */
} cfear_reg_result;                     /* 72 bytes */

/* Replaces n_scan_normal_reg::Register (n_scan_normal.cpp:82-185).  poses_xyt [n_scans][3]
 * host, in/out: Affine3dToVectorXYeZ(Tsrc[i]) on entry; on return the last row holds the
 * registered source pose (Tsrc.back() = vectorToAffine3d(parameters.back())).  Returns the
 * result's status; reg_cov is the constant diag(0.01,0.01,0,0,0,1e-4) (n_scan_normal.cpp:171). */
int cfear_register(cfear_ctx* ctx, const cfear_scan* const* scans, int32_t n_scans,
                   double* poses_xyt, const cfear_reg_params* par, cfear_reg_result* result);

/* One launch, many independent registrations (loop-closure candidate batches,
 * loopclosure.cpp:35-97 called per candidate from :658-721).  results: host memory (the call
 * returns after the read-back) or DEVICE memory (the records stay on the GPU; the launch is
 * enqueued on the context's stream and not synchronised -- what a collective over the records
 * wants, cfear_register_batch_sharded).
 * The matcher runs in the form the batch calls for (wavefronts per registration x LDS per workgroup: 8 wavefronts up to two
 * workgroups per CU, 4 beyond, 2 for large batches of two-scan candidates); the forms add the fp64 sums in different
 * orders, so the SAME job may differ by a few ulp of cost / pose between a small and a large batch -- e.g. between world 1
 * and a sharded run.  Iteration counts and the accept / reject decisions are the same in every test of this repository
 * (tests/test_gpu_register.py::test_every_form_of_the_matcher_agrees), the poses agree to 1e-11.                       */
typedef struct cfear_reg_job {
  const cfear_scan* const* scans;       /* n_scans handles */
  int32_t n_scans;
  int32_t pad;
  const double* poses_xyt;              /* [n_scans][3] host */
} cfear_reg_job;
int cfear_register_batch(cfear_ctx* ctx, const cfear_reg_job* jobs, int32_t n_jobs,
                         const cfear_reg_params* par, cfear_reg_result* results);

/* The same for a loop-closure thread that registers candidate PAIRS among scans it keeps (every graph node's
 * cloud_normal_, types.h:119-122; loopclosure.cpp:658-721 walks the candidates of a query one by one): the scans' device
 * views are uploaded ONCE as a table, and a batch is then 56 bytes per candidate -- two table indices and the two poses of
 * loopclosure::Register's problem {to = fixed target, from = free source} (loopclosure.cpp:35-97) -- instead of a job
 * record with both scans' views (608 bytes) marshalled on the host per candidate and call; the records the matcher reads
 * are written by a small kernel on the device.  Results as for cfear_register_batch (host, or device: not synchronised).
 * The table keeps no reference on the scans: they must outlive it.                                                  */
typedef struct cfear_scan_table cfear_scan_table;
typedef struct cfear_candidate {
  int32_t target, source;               /* indices into the table */
  double target_xyt[3], source_xyt[3];  /* Affine3dToVectorXYeZ of the two poses; the source pose is the initial guess */
} cfear_candidate;                      /* 56 bytes */
int cfear_scan_table_create(cfear_ctx* ctx, const cfear_scan* const* scans, int32_t n_scans, cfear_scan_table** out);
int cfear_scan_table_size(const cfear_scan_table* table);
int cfear_scan_table_destroy(cfear_scan_table* table);
int cfear_register_candidates(cfear_ctx* ctx, const cfear_scan_table* table, const cfear_candidate* candidates,
                              int32_t n_candidates, const cfear_reg_params* par, cfear_reg_result* results);

/* Replaces n_scan_normal_reg::GetCost (n_scan_normal.cpp:186-211): one association pass at the
 * given poses + robust cost.  residuals (optional, host, cap entries) receives the robustified
 * residual vector; n_residuals its length; score = cost / max(n_residuals, 1).                */
int cfear_get_cost(cfear_ctx* ctx, const cfear_scan* const* scans, int32_t n_scans,
                   const double* poses_xyt, const cfear_reg_params* par, double* cost,
                   double* residuals, int32_t cap, int32_t* n_residuals, double* score);

/* GetCost for many (scan list, pose list) pairs in one launch (the 27 evaluations per registration of
 * approximateCovarianceBySampling, CFEARQuality over candidate batches).  results[j]: final_cost = robust
 * cost, score = cost / n_residuals, num_residuals, status (CFEAR_OK / CFEAR_ERR_TOO_FEW_RESIDUALS /
 * CFEAR_ERR_CAPACITY); pose echoes the evaluated source pose.  par->itr selects the radius as above. */
int cfear_get_cost_batch(cfear_ctx* ctx, const cfear_reg_job* jobs, int32_t n_jobs,
                         const cfear_reg_params* par, cfear_reg_result* results);

/* Diagnostic: which registrations hang on a nearest-neighbour tie.  FLANN's nearestKSearch with k = 1 returns ONE of several
 * equidistant targets (pointnormal.cpp:249), this library the lowest index; a reference build may legally pick another, and
 * where the tied cells differ the registered pose follows the pick.  The call replays the association
 * step of AddScanPairCost (n_scan_normal.cpp:213-261) at the poses of every job -- Tsrctotar, the float query, the radius by
 * itr (2 * radius when itr == 1), the direction test -- by brute force, keeps all minimisers of every query and counts.
 * It is a snapshot at the poses it is given: it says nothing about the passes a registration makes from there.
 *   records [n_jobs] and per_query (optional) may be host or device memory, both on the same side; device records stay
 *     there, stream-ordered and not synchronised, as the results of cfear_register_batch do.
 *   per_query [total][3] = {lo, hi, count} of every query: job j's block starts at the sum over the jobs before it of
 *     n_src * (n_scans - 1), the entry of fixed scan t and source cell s inside it is t * n_src + s; a query outside the
 *     radius has {-1, -1, 0}.  per_query_len = the caller's capacity in entries; too small: CFEAR_ERR_CAPACITY before
 *     anything is launched (the library computes the lengths from cfear_scan_size).
 * Refused with CFEAR_ERR_INVALID_ARGUMENT before anything is launched or written, cfear_last_error naming the job: null
 * pointers, n_jobs < 0, itr < 0, a job with n_scans < 2 (or more than the matcher takes), a pose that is not finite.
 * n_jobs == 0 is CFEAR_OK.                                                                                              */
#define CFEAR_TIE_TILE 1024             /* target cells per LDS tile of the audit's search (tests cross it on purpose)      */
typedef struct cfear_tie_record {
  int32_t n_queries;                    /* source cells x fixed scans of the job                                            */
  int32_t n_in_radius;
  int32_t n_associated;                 /* = blocks cfear_cost_prepare builds at these poses and this itr                   */
  int32_t n_tied;                       /* in radius, >= 2 target cells at the minimum float distance                       */
  int32_t n_tied_effective;             /* ... and some cell of the group differs bitwise from the lowest one in mean,
                                         * normal, cov, scale or nsamples: what the residual and the weight read            */
  int32_t max_group;                    /* largest tie group among in-radius queries (1 if none tied; 0 if none in radius)  */
  int32_t status, pad;                  /* CFEAR_OK or the status cfear_get_cost_batch would give the job                   */
} cfear_tie_record;                     /* 32 bytes */
int cfear_association_ties_batch(cfear_ctx* ctx, const cfear_reg_job* jobs, int32_t n_jobs, const cfear_reg_params* par, int32_t itr,
                                 cfear_tie_record* records, int32_t* per_query, int64_t per_query_len);

/* Diagnostic: which scans hang on the in-voxel summation order of pcl::VoxelGrid.  PCL sorts (voxel, point) pairs with an
 * unstable std::sort and sums a voxel's points sequentially in float (pointnormal.cpp:277-280), so the last bits of a centroid
 * are libstdc++'s to choose; this library pins input order.  Per scan -- the cloud MapPointNormal hands to VoxelGrid, after
 * compensation -- and per voxel, with leaf = (float)(radius / downsample_factor), inv_leaf = 1.0f / leaf,
 * r2 = (float)((double)radius * radius), u = 2^-24 and the voxel's n points in INPUT order:
 *   c_fwd, c_rev  the sequential float sums first to last and last to first, divided by (float)n; c_fwd is this library's centroid
 *   e             per axis, in fp64: S = sum x, A = sum |x|, g = (n-1)u / (1 - (n-1)u), mid = S / n, t = g A / n,
 *                 e = (t + u (|mid| + t)) + 2^-40 (|mid| + 1): the float centroid of EVERY order lies in [mid - e, mid + e]
 *   pair classes  against every point p of the scan, with the smallest and largest squared distance d2min, d2max from p to
 *                 that box: sure-in if d2max (1 + 8u) < r2, sure-out if d2min (1 - 8u) >= r2, exposed otherwise
 *   exposed       the voxel has an exposed pair; at the threshold: sure_in < 6 <= sure_in + exposed (pointnormal.cpp:291)
 *   changed       the float radius test (dx = c.x - p.x; d = dx * dx; d += dy * dy; d < r2) admits different points at
 *                 c_fwd and at c_rev: a witness that one legal order does differ
 * n_voxels_exposed == 0: no reference build can differ from this library through the in-voxel order on this scan;
 * n_voxels_changed_reversed > 0: at least one legal order does.  The truth lies between the two.
 *   xyzi [..][4] float, host or device; scan s holds lengths[s] points from point offsets[s] on (offsets NULL: the scans
 *     follow each other); offsets and lengths are host arrays.
 *   records [n_scans] and voxels (optional) are host or device memory, both on the same side.  A scan of no points has status
 *     CFEAR_ERR_EMPTY_CLOUD, one with a coordinate that is not finite CFEAR_ERR_INVALID_ARGUMENT, one of more than
 *     CFEAR_VOXEL_AUDIT_MAX_POINTS points -- or whose grid reaches beyond 2^23 voxels from the origin or holds 2^31 or more --
 *     CFEAR_ERR_CAPACITY, with n_points set and every counter 0; the other records are complete and the call returns the
 *     first such status.
 *   voxels [voxel_cap]: the rows of scan 0 in ascending voxel key -- the order of VoxelGrid's output --, then scan 1's, ...;
 *     *n_voxels_out (optional, host) = the rows of the batch.  More than voxel_cap: the table holds the first voxel_cap, every
 *     record is complete, and the call returns CFEAR_ERR_CAPACITY (behind a scan's status, if there is one).
 * The call reads the voxel counts back between its two launches, so it is synchronous on either side.
 * Refused with CFEAR_ERR_INVALID_ARGUMENT before anything is launched or written: null xyzi, lengths, params or records,
 * n_scans < 0, voxel_cap < 0, a radius or downsample_factor that is not finite and > 0, a negative length or offset.      */
#define CFEAR_VOXEL_AUDIT_TILE 1024          /* points per LDS tile of the audit's sweeps (tests cross it on purpose)          */
#define CFEAR_VOXEL_AUDIT_MAX_POINTS 40960   /* per scan: n_pairs_exposed <= points x voxels stays below 2^31                  */
typedef struct cfear_voxel_audit_params {
  float radius;                         /* MapPointNormal's radius (3.0)                                                    */
  float pad;
  double downsample_factor;             /* (1.0)                                                                            */
} cfear_voxel_audit_params;             /* 16 bytes */
void cfear_voxel_audit_params_default(cfear_voxel_audit_params* p);
typedef struct cfear_voxel_audit_record {
  int32_t status;
  int32_t n_points;
  int32_t n_voxels;
  int32_t n_centroids_reversed_differ;  /* voxels whose c_fwd and c_rev differ in a bit                                     */
  int32_t n_pairs_exposed;
  int32_t n_voxels_exposed;
  int32_t n_voxels_exposed_at_threshold;
  int32_t n_voxels_changed_reversed;
  int32_t max_voxel_points;
  int32_t pad;
  double max_halfwidth;                 /* the largest e of the scan, either axis                                           */
} cfear_voxel_audit_record;             /* 48 bytes */
typedef struct cfear_voxel_audit_voxel {
  uint32_t key;                         /* ijk0 + ijk1 * div_bx, as VoxelGrid computes it                                   */
  int32_t n_points;
  float c_fwd[2];
  float c_rev[2];
  double e[2];
  int32_t n_sure_in;
  int32_t n_exposed;
  int32_t changed_reversed;
  int32_t pad;
} cfear_voxel_audit_voxel;              /* 56 bytes */
int cfear_voxel_order_audit_batch(cfear_ctx* ctx, const float* xyzi, const int64_t* offsets, const int32_t* lengths, int32_t n_scans,
                                  const cfear_voxel_audit_params* par, cfear_voxel_audit_record* records,
                                  cfear_voxel_audit_voxel* voxels, int64_t voxel_cap, int64_t* n_voxels_out);

/* Covariance of a registration by cost sampling.  Replaces
 * OdometryKeyframeFuser::approximateCovarianceBySampling (odometrykeyframefuser.cpp:261-380) and
 * loopclosure::approximateCovarianceBySampling (tbv_slam/src/tbv_slam/loopclosure.cpp:99-208):
 * samples_per_axis^3 GetCost evaluations on a (yaw, x, y) grid around the registered source pose (one
 * kernel launch for all of them), quadratic least-squares fit, cov = 2 H^-1 * GetCovarianceScaler() *
 * covariance_scaler embedded in a 6x6 (x, y, -, -, -, yaw).                                       */
typedef struct cfear_cov_sampling_params {
  double xy_range;                      /* cov_sampling_xy_range: samples span +- xy_range / 2        */
  double yaw_range;                     /* cov_sampling_yaw_range                                     */
  int32_t samples_per_axis;             /* cov_sampling_samples_per_axis (3)                          */
  int32_t pad;
  double covariance_scaler;             /* cov_sampling_covariance_scaler (4.0)                       */
} cfear_cov_sampling_params;            /* 32 bytes */
void cfear_cov_sampling_params_default(cfear_cov_sampling_params* p);   /* odometrykeyframefuser.h:107-110 */
/* poses_xyt: the poses AFTER Register (T_vek); par: the registration parameters that produced them;
 * reg: that Register's result (final_cost, num_residuals -> GetCovarianceScaler; outer_iters -> the
 * radius GetCost uses).  cov36: row-major 6x6; samples (optional): [n^3][4] = x, y, yaw offset, cost in
 * the reference's loop order (yaw outer, x, y inner).  *success = 1 when the fit is convex and the
 * scaler defined (the reference then replaces reg_cov); otherwise cov36 holds Register's constant
 * diag(0.01, 0.01, 0, 0, 0, 1e-4).                                                                  */
int cfear_covariance_by_sampling(cfear_ctx* ctx, const cfear_scan* const* scans, int32_t n_scans,
                                 const double* poses_xyt, const cfear_reg_params* par,
                                 const cfear_reg_result* reg, const cfear_cov_sampling_params* sp,
                                 double* cov36, double* samples, int32_t* success);
/* Same for a batch (loop-closure candidates): regs [n_jobs], cov36 [n_jobs][36], samples (optional)
 * [n_jobs][n^3][4], success [n_jobs].                                                               */
int cfear_covariance_by_sampling_batch(cfear_ctx* ctx, const cfear_reg_job* jobs, int32_t n_jobs,
                                       const cfear_reg_params* par, const cfear_reg_result* regs,
                                       const cfear_cov_sampling_params* sp, double* cov36, double* samples,
                                       int32_t* success);
/* The fit alone, as a kernel (csrc/covfit.hip): per job the carry-over of failed samples (a sample whose status is not
 * CFEAR_OK keeps the previous cost, 0.0 before the first good one), the quadratic fit, the convexity test and
 * 2 H^-1 * regs[j].final_cost / (regs[j].num_residuals - 3) * covariance_scaler -- cov36 and success are bit for bit what the
 * host fit of cfear_covariance_by_sampling_batch makes of the same records.  A refused fit, or num_residuals - 3 == 0,
 * leaves diag(0.01, 0.01, 0, 0, 0, 1e-4) and success = 0.
 * regs [n_jobs], samples [n_jobs][n^3] (the records the matcher's sampling mode leaves: status and final_cost are read),
 * cov36 [n_jobs][36], success [n_jobs]: all four in host memory or all four in device memory (then the call is only enqueued
 * on the context's stream).  Refused before the context is used: null arguments, samples_per_axis outside [1, 15], pointers
 * in different memories.  n_jobs = 0: CFEAR_OK, the device untouched.                                                    */
int cfear_cov_fit_records(cfear_ctx* ctx, const cfear_reg_result* regs, const cfear_reg_result* samples, int32_t n_jobs,
                          const cfear_cov_sampling_params* sp, double* cov36, int32_t* success);
/* Covariance by cost sampling for candidate pairs of a scan table: the counterpart of cfear_register_candidates, with no host
 * round trip between the samples and the covariance (the candidates become job records on the device, the matcher samples
 * around centres it reads from device records, cov_fit_kernel fits).  Job j's problem is {table[target] fixed at target_xyt,
 * table[source] free}; its samples are centred on regs[j].pose where regs[j].status is CFEAR_OK and on the candidate's
 * source_xyt otherwise; the association radius follows regs[j].outer_iters.  par: the parameters of the registration that
 * made regs.  candidates: host or device memory.  regs [n], cov36 [n][36], success [n]: all host (one read-back at the end)
 * or all device (enqueued on the context's stream; with a device candidate list the call first waits for the 16-byte verdict
 * of the kernel that reads it).  Refused: null arguments, samples_per_axis outside [1, 15], regs / cov36 / success in
 * different memories, a candidate that names a scan outside the table ("candidate j ...").  n = 0: CFEAR_OK.             */
int cfear_covariance_by_sampling_candidates(cfear_ctx* ctx, const cfear_scan_table* table, const cfear_candidate* candidates,
                                            int32_t n_candidates, const cfear_reg_params* par, const cfear_reg_result* regs,
                                            const cfear_cov_sampling_params* sp, double* cov36, int32_t* success);

/* Ceres-compatible evaluation of one association set (what AddScanPairCost would hand to
 * ceres::Problem, n_scan_normal.cpp:264-318): prepare associates once at `poses_xyt`;
 * evaluate returns the RAW residuals r [n_res] and Jacobian J [n_res][3] (row-major, like
 * ceres::CostFunction::Evaluate), the per-block weights w [n_blocks] of ScaledLoss, and
 * normal_eq the robustified H = J^T J [9], g = J^T r [3], cost = 1/2 sum rho at x.            */
typedef struct cfear_cost cfear_cost;
int cfear_cost_prepare(cfear_ctx* ctx, const cfear_scan* const* scans, int32_t n_scans,
                       const double* poses_xyt, const cfear_reg_params* par, int32_t itr,
                       cfear_cost** out);
int cfear_cost_num_blocks(const cfear_cost* c);
int cfear_cost_num_residuals(const cfear_cost* c);
/* pairs int32 [n_blocks][3] = (target scan, target cell, source cell); weights [n_blocks]. */
int cfear_cost_get_blocks(const cfear_cost* c, int32_t* pairs, double* weights);
int cfear_cost_evaluate(cfear_cost* c, const double x[3], double* residuals, double* jacobian);
int cfear_cost_normal_eq(cfear_cost* c, const double x[3], double H[9], double g[3], double* cost);
int cfear_cost_destroy(cfear_cost* c);

/* ---- caller: CorAl alignment quality (loop-closure verification) ---------------------------------
 * Replaces CorAlRadarQuality (coral_alignment_quality/src/alignment_checker/AlignmentQuality.cpp:8-230)
 * as ScanLearningInterface::getCorAlQualityMeasure builds it (alignmentinterface.cpp:437-456): both
 * scans are kstrongStructuredRadar objects over the stored PEAK clouds, the source is placed at
 * src_pose * Toffset, every point of the merged cloud gets the entropy of its radius-neighbourhood in
 * its own cloud (sep) and in both clouds (joint).  quality_ = {joint, sep, overlap}; valid_ = overlap
 * >= 0.1.  Only ent_cfg = any (ComputeEntropy) is built: TBV never selects the kl variant.          */
typedef struct cfear_coral_params {
  double radius;                        /* AlignmentQuality::parameters::radius; TBV: 1.0              */
  int32_t weight_res_intensity;         /* weight_res_intensity; TBV: false                            */
  int32_t pad;
} cfear_coral_params;
void cfear_coral_params_default(cfear_coral_params* p);

typedef struct cfear_coral_job {
  const float* ref_xyzi;                /* [n_ref][4] x,y,z,intensity in the reference scan's sensor frame; host or device */
  const float* src_xyzi;                /* [n_src][4]                                                   */
  int32_t n_ref, n_src;
  double ref_pose[3];                   /* ref->GetAffine() as (x, y, theta)                           */
  double src_pose[3];                   /* src->GetAffine()                                            */
  double offset[3];                     /* Toffset (perturbation), applied as src_pose * Toffset       */
} cfear_coral_job;

typedef struct cfear_coral_result {
  double joint, sep, overlap;           /* quality_[0..2] (output_overlap = true)                      */
  int32_t valid;                        /* valid_                                                      */
  int32_t count_valid;                  /* points with both covariances and finite entropies           */
  int32_t status;                       /* CFEAR_OK / CFEAR_ERR_EMPTY_CLOUD / CFEAR_ERR_CAPACITY       */
  int32_t pad;                          /* diagnostic: CFEAR_CORAL_PATH_* of a served job, 0 otherwise */
} cfear_coral_result;                   /* 40 bytes */
/* Diagnostic, like cfear_reg_result.reserved: which code path served the job.  The kernel chooses it from the shape
 * of the merged cloud (points, occupied grid cells, grid size); results do not depend on it and callers should not.  */
#define CFEAR_CORAL_PATH_SCRATCH 1      /* sorted points in the per-job global scratch, not in LDS     */
#define CFEAR_CORAL_PATH_BSEARCH 2      /* cell lookup by binary searches, not by the occupancy bitmap */
#define CFEAR_CORAL_PATH_SORT_MASK 12   /* 0: two-level row sort                                       */
#define CFEAR_CORAL_PATH_SORT_RADIX 4
#define CFEAR_CORAL_PATH_SORT_BITONIC 8

/* Limits.  The kernel sorts the merged cloud into a uniform grid of radius * 1.0001 cells over its bounding box, rows
 * along y.  radius must be > 0 (not NaN), else CFEAR_ERR_INVALID_ARGUMENT.  CFEAR_ERR_CAPACITY:
 *   - n_ref + n_src > 16384 in any job: the call returns at entry, nothing is launched, no record is written;
 *   - per job, as results[j].status: more than 4096 grid rows (y extent / radius), more than 2^31 - 1 grid cells.
 *     The limits are not symmetric: two clusters 4200 radii apart along y are
 *     refused, along x they are served; radius 0.05 over a 300 m scan is refused.  A NaN coordinate among finite points
 *     is NOT refused: the bounding box skips it (fminf / fmaxf), the point is nobody's neighbour, and the job's measures
 *     stay finite.
 * An empty cloud is the job's status CFEAR_ERR_EMPTY_CLOUD and does not fail the call.  Any other failed job makes the
 * batch call return that job's status (the first such job's); every record is written all the same -- failed jobs as
 * zeros with their status, all others valid.  The per_point rows of a failed job are unspecified.
 *
 * per_point (optional, host): [n_src + n_ref][3] = joint_res_, sep_res_, sep_valid in the reference's
 * index order (source points first); invalid points hold the reference's initial 100.0.             */
int cfear_coral_quality(cfear_ctx* ctx, const cfear_coral_job* job, const cfear_coral_params* par,
                        cfear_coral_result* result, double* per_point);
/* One launch for a batch (the 13 perturbations of a training pair, a loop-closure candidate list);
 * clouds shared between jobs are uploaded once.  per_point (optional): jobs' arrays back to back.     */
int cfear_coral_quality_batch(cfear_ctx* ctx, const cfear_coral_job* jobs, int32_t n_jobs,
                              const cfear_coral_params* par, cfear_coral_result* results, double* per_point);

/* ---- caller: point-to-point alignment quality and keypoint repeatability -----------------------------
 * Replaces p2pQuality and keypointRepetability (coral_alignment_quality/src/alignment_checker/AlignmentQuality.cpp:
 * 235-328), the measures AlignmentQualityFactory::CreateQualityType (AlignmentQuality.h:260-312) builds for
 * Cen2018Radar, kstrongStructuredRadar and BFARScan scans with method "P2P" / "keypoint_repetability" and that
 * scanEvaluator (ScanEvaluator.cpp:57-114, the body of evaluate_scans) scores a sequence with.  The source cloud is
 * moved by Tchange = Tref.inverse() * Tsrc * Toffset (:260-264) with pcl::transformPointCloud's rounding, every moved
 * point asks pcl::KdTreeFLANN<PointXYZI>::radiusSearch over the reference cloud (3-D, d = dx dx + dy dy + dz dz in float,
 * kept when d < float(radius * radius), strictly) for its nearest neighbour, and
 *   p2pQuality            residuals_ = the nearest d of every source point that has one, in source order, pushed BEHIND
 *                         the {0, 0, 0} the base constructor leaves there (AlignmentQuality.h:92): quality_[0] = mean =
 *                         sum / (matched + 3), quality_ = {mean, 0, 0};
 *   keypointRepetability  quality_ = {matched / n_src, matched, n_src} -- read off the same record.
 * The caller composes Tchange (include/cfear_hip.hpp and api.py do, with the same fp64 formula), so a record is a pure
 * function of (ref, src, T, radius).  Eigen's Affine3d::inverse() is a general inverse: the reference's last bits of T
 * are not pinned.                                                                                 */
typedef struct cfear_p2p_job {
  const float* ref_xyzi;                /* [n_ref][4] x,y,z,intensity, host or device                   */
  const float* src_xyzi;                /* [n_src][4], host or device                                   */
  int32_t n_ref, n_src;
  double T[6];                          /* Tchange, row-major 2x3: x' = T0 x + T1 y + T2, y' = T3 x + T4 y + T5 */
} cfear_p2p_job;

typedef struct cfear_p2p_result {
  double mean;                          /* p2pQuality quality_[0] = sum / (matched + 3)                 */
  double sum;                           /* sum of the matched points' nearest squared distances         */
  int32_t matched;                      /* source points with a neighbour: keypointRepetability quality_[1] */
  int32_t n_src;                        /* keypointRepetability quality_[2]                             */
  int32_t status;                       /* CFEAR_OK / CFEAR_ERR_EMPTY_CLOUD / CFEAR_ERR_CAPACITY        */
  int32_t pad;                          /* diagnostic: CFEAR_CORAL_PATH_* of a served job, 0 otherwise  */
} cfear_p2p_result;                     /* 32 bytes */
/* pad, as cfear_coral_result.pad: which path of the grid index over the job's REFERENCE cloud served it (same bits, same
 * meanings: sorted points in the global scratch, binary-search lookup, sort kind).  The kernel chooses it from the shape of
 * that cloud; results do not depend on it and callers should not.                                                          */

/* Limits.  One workgroup sorts a reference cloud into a uniform grid of radius * 1.0001 cells over its bounding box and
 * serves every job of the batch that names it (same pointer, same n_ref): the perturbations of a scan pair cost one sort.
 * radius must be > 0 and finite and every T finite, else CFEAR_ERR_INVALID_ARGUMENT.  CFEAR_ERR_CAPACITY:
 *   - n_ref > CFEAR_P2P_MAX_REF_POINTS or n_src > CFEAR_P2P_MAX_SRC_POINTS in any job: the call returns at entry,
 *     nothing is launched, no record is written;
 *   - per job, as results[j].status: a NaN coordinate (x, y or z) in either cloud -- for the source cloud, after the
 *     transform as well (0 * inf) -- or a reference cloud whose grid has
 *     more than 4096 rows (y extent / radius), more than 2^31 - 1 cells, or a cell index beyond 2^22 (|x| or |y| /
 *     radius).  The source cloud may lie anywhere: points outside the grid have no neighbour.
 * An empty source or reference cloud is the job's status CFEAR_ERR_EMPTY_CLOUD and does not fail the call.  Any other
 * failed job makes the call return that job's status (the first such job's); every record is written all the same --
 * failed jobs as zeros with their status, all others valid.  The per_point row of a failed job is unspecified.
 *
 * matched, n_src and per_point are exact.  sum is added per thread in source order (stride 1024) and then over a fixed
 * tree, so it is within 2 n_src 2^-53, relatively, of the reference's serial sum; a job's record and per_point row do not
 * depend on the batch around it.
 *
 * results [n_jobs] and per_point (optional; the jobs' [n_src] floats back to back: the nearest d, or -1.0f where the point
 * has none) may each be host or device memory.  With device clouds and device outputs the call is only enqueued; the
 * statuses are then the caller's to read, and the call returns CFEAR_OK.                                             */
#define CFEAR_P2P_MAX_REF_POINTS 16384
#define CFEAR_P2P_MAX_SRC_POINTS 1048576
int cfear_p2p_quality(cfear_ctx* ctx, const cfear_p2p_job* job, double radius, cfear_p2p_result* result, float* per_point);
int cfear_p2p_quality_batch(cfear_ctx* ctx, const cfear_p2p_job* jobs, int32_t n_jobs, double radius,
                            cfear_p2p_result* results, float* per_point);

/* ---- caller: the Cartesian radar image and CorAlCartQuality -------------------------------------------
 * Replaces CartesianRadar (coral_alignment_quality/src/alignment_checker/ScanType.cpp:191-209), radar_polar_to_cartesian and
 * RotoTranslation (Utils.cpp:255-339) and CorAlCartQuality (AlignmentQuality.cpp:356-386), the measure
 * AlignmentQualityFactory::CreateQualityType (AlignmentQuality.h:260-312) builds for CartesianRadar scans (evaluate_scans
 * --scan-type kstrongCart) whatever pars.method says.
 *   cfear_polar_to_cartesian   f = float(u8) * float(1 / 255.0) (convertTo), then cv::remap with the float maps of Utils.cpp:
 *                              258-308: per Cartesian pixel a range bin and an azimuth index, quantised to 1/32 pixel with
 *                              cvRound (half to even), bilinear in float ((S00 w0 + S01 w1) + S10 w2) + S11 w3, taps outside
 *                              the sweep read 0.  The maps depend on (rows, W, radar_resolution, cart_resolution) only: the
 *                              HOST builds them (its libm's atan2f) once per geometry and the context keeps them.
 *   cfear_cart_quality_batch   per job RotoTranslation of the source image by (x, y, yaw) -- warpAffine with
 *                              getRotationMatrix2D about ((W - 1) / 2, (W - 1) / 2), then warpAffine of ITS OUTPUT by
 *                              (float(x) / image_res, float(y) / image_res) pixels; both with OpenCV's integer maps (the
 *                              matrix inverted in double, 10 fraction bits, + 16 >> 5: 1/32 pixel rounded half UP), bilinear,
 *                              border 0 -- and abs_diff = the sum of |warped - ref| over the W x W floats, added in double.
 *                              quality_ = {abs_diff, 0, 0}.
 * Quirks of the reference, kept:
 *   - the azimuth index of a pixel lies in [-1, rows - 1) and the cross-over interpolation is commented out (Utils.cpp:
 *     316-319): for an index below 0 row -1 reads zeros, so the seam behind the last azimuth is darkened;
 *   - RotoTranslation hands the yaw, in RADIANS, to getRotationMatrix2D, which takes degrees: a yaw of 0.5 rotates by 0.5
 *     degrees.  The entry point takes the yaw as the reference has it and does the same;
 *   - CorAlCartQuality takes Tsrc AND Tref from the source scan (AlignmentQuality.cpp:363-364), so Tchange = Tsrc^-1 Tsrc
 *     Toffset; and the CartesianRadar constructor calls radar_polar_to_cartesian with its default arguments (0.04328, 0.2384,
 *     300) whatever pars says, while CorAlCartQuality reads cart_resolution_ from pars.  Both are the callers' business:
 *     include/cfear_hip.hpp and api.py reproduce them, the entry points take explicit values and (x, y, yaw) per job.
 * NOT PINNED: the arithmetic of remap, warpAffine, getRotationMatrix2D and convertTo is restated from knowledge of OpenCV
 * 4.2's imgproc (tests/cart_cpu.py is the definition); no OpenCV build was compared.  cv::sum's order of additions is not
 * restated either: abs_diff is added per thread with a fixed stride, then over a fixed tree, an order that depends on W
 * only, so it is within 2 W^2 2^-53, relatively, of any other order and a job's record does not depend on the batch.  */
typedef struct cfear_cart_params {
  float radar_resolution;               /* 0.04328 */
  float cart_resolution;                /* 0.2384 */
  int32_t cart_pixel_width;             /* 300 */
  int32_t pad;
} cfear_cart_params;                    /* 16 bytes */
void cfear_cart_params_default(cfear_cart_params* par);

/* polar: batch sweeps (rows = azimuths, rows >= 2); cart: float [batch][W][W]; both host or both device memory.
 * CFEAR_ERR_INVALID_ARGUMENT: W < 1 or > CFEAR_CART_MAX_WIDTH, rows < 2, rows or cols > 32767 (the reference's `short`
 * coordinates), a resolution that is not finite and > 0.  With device memory the call is only enqueued.                */
#define CFEAR_CART_MAX_WIDTH 4096
int cfear_polar_to_cartesian(cfear_ctx* ctx, const uint8_t* polar, const cfear_polar_desc* desc, const cfear_cart_params* par,
                             float* cart);

typedef struct cfear_cart_job {
  const float* src;                     /* [W][W] the image that is warped, host or device              */
  const float* ref;                     /* [W][W] the image it is compared with, host or device         */
  double x, y, yaw;                     /* Affine3dToEigVectorXYeZ(Tchange)                             */
} cfear_cart_job;                       /* 40 bytes */

typedef struct cfear_cart_result {
  double abs_diff;                      /* CorAlCartQuality quality_[0]                                 */
  int32_t status;                       /* CFEAR_OK / CFEAR_ERR_INVALID_ARGUMENT                        */
  int32_t pad;
} cfear_cart_result;                    /* 16 bytes */

/* results [n_jobs] and warped (optional: float [n_jobs][W][W], the warped source images) may each be host or device
 * memory; images shared between jobs are uploaded once.  A job whose pose is not finite, or whose |x| or |y| over
 * image_res exceeds 2^20 pixels (which keeps OpenCV's saturate_cast<int> out of play), gets status
 * CFEAR_ERR_INVALID_ARGUMENT, a zero abs_diff and a zero warped image; the call completes and returns CFEAR_OK, the other
 * records are valid.  The call itself fails with CFEAR_ERR_INVALID_ARGUMENT for a null image, W out of range or an
 * image_res that is not finite and > 0.  With device memory throughout the call is only enqueued.                   */
int cfear_cart_quality_batch(cfear_ctx* ctx, const cfear_cart_job* jobs, int32_t n_jobs, int32_t cart_pixel_width,
                             float image_res, cfear_cart_result* results, float* warped);

/* ---- before the path: radar Scan Context (loop-candidate generation) ------------------------------
 * Replaces the arithmetic of RSCManager / SCManager (place_recognition_radar/src/place_recognition_radar/
 * RadarScancontext.cpp:59-131, 156-180; Scancontext.cpp:60-268): the ring x sector descriptor of a
 * local-map cloud (TBV: merged peak clouds of 2 N_aggregate + 1 nodes in the node's frame, loopclosure.cpp:
 * 552-590), its ring / sector keys, and distanceBtnScanContext.  The descriptor database, the odometry-
 * coupled ring-key search and the candidate ranking stay on the host (api.py RSCManager mirrors them). */
typedef struct cfear_sc_params {
  int32_t num_ring, num_sector;         /* PC_NUM_RING 40, PC_NUM_SECTORS 120                          */
  double max_radius;                    /* PC_MAX_RADIUS 80                                            */
  double search_ratio;                  /* SEARCH_RATIO 0.1                                            */
  int32_t desc_function;                /* 0 = "sum", 1 = "max"                                        */
  int32_t pad;
  double desc_divider;                  /* 1000 in TBV's launch defaults                               */
  double no_point;                      /* value of empty bins (reached only when desc_divider == 1)   */
} cfear_sc_params;
/* Limits, checked by every call that takes these parameters -- descriptors, distances, managers, whole-graph calls:
 * num_ring x num_sector in [1, 5120] (CFEAR_ERR_CAPACITY); search_ratio finite (CFEAR_ERR_INVALID_ARGUMENT); and the
 * distance kernel's LDS, 160 KiB, must hold (2 R S + 6 S) * 8 + (2 + m) * 4 bytes, m = 2 round(0.5 search_ratio S) + 1
 * (CFEAR_ERR_CAPACITY).  With one ring and search_ratio 0.1 that allows S <= 2543; 2 x 2560 and 1 x 5120 are refused. */
void cfear_sc_params_default(cfear_sc_params* p);
typedef struct cfear_sc_cloud {
  const float* xyzi;                    /* [n][4] x,y,z,intensity in the node's frame; host or device   */
  int32_t n, pad;
} cfear_sc_cloud;
/* Intensity domain: bins are summed with fp64 atomics ("sum") or take an order-preserving maximum ("max").  For
 * non-negative integer intensities whose bin sums stay below 2^53 -- every cloud TBV makes: raw u8 values or
 * value - zmin -- this is exactly the reference's rule (a bin still at NO_POINT = -1000 is replaced, otherwise added to /
 * maxed).  Outside that domain a bin holds the plain sum (its last bits may depend on the order of arrival when the
 * intensities are fractional) or the plain maximum of its intensities; the reference's replace rule is not followed
 * when a running value passes through -1000.  A result equal to NO_POINT after the division still becomes no_point.
 * MakeRadarCloudContext for n_clouds clouds x n_aug lateral shifts (shifts_y[0] is normally 0; TBV augments
 * with {-2, 2, -4, 4}).  desc [n_clouds][n_aug][num_ring * num_sector] row-major (ring, sector); ringkey
 * [..][num_ring] and sectorkey [..][num_sector] optional.  desc may be HOST or DEVICE memory (a descriptor
 * database kept in HBM feeds cfear_sc_distance_batch without crossing PCIe); the keys are host arrays -- the
 * retrieval policy that consumes them runs on the host.                                                */
int cfear_sc_descriptors(cfear_ctx* ctx, const cfear_sc_cloud* clouds, int32_t n_clouds,
                         const cfear_sc_params* par, const double* shifts_y, int32_t n_aug, double* desc,
                         double* ringkey, double* sectorkey);
/* distanceBtnScanContext for pairs[i] = (query index into desc_q, candidate index into desc_c); descriptors
 * host or device; dist / shift host [n_pairs] (shift = argmin column shift of the candidate).  The search space keeps
 * the reference's duplicates; shift is in [0, S) while round(0.5 search_ratio S) <= S.  Past that (search_ratio > 2)
 * the reference's (argmin - ii + S) % S turns negative; such a shift k is applied as k + S and reported as k, in
 * (-S, 0), like the reference's index arithmetic (whose circshift is undefined there).                 */
int cfear_sc_distance_batch(cfear_ctx* ctx, const double* desc_q, int32_t n_q, const double* desc_c, int32_t n_c,
                            const int32_t* pairs, int32_t n_pairs, const cfear_sc_params* par, double* dist,
                            int32_t* shift);

/* Raw-sweep Scan Context: RSCManager::MakeRadarContext (RadarScancontext.cpp:41-57), the descriptor TBV builds with
 * --raw_radar_scan true (loopclosure.cpp:573-577): cv::threshold(THRESH_TOZERO) of the 8-bit sweep, then cv::resize to
 * num_ring x num_sector with INTER_AREA, restated from OpenCV 4.2 (resize.cpp: computeResizeAreaTab + resizeArea_<uchar,
 * float> in float without FMA, or resizeAreaFast_<uchar, int> when both scales are integers; cvRound half to even).
 * Rings run along the image's rows, sectors along its columns, of the image the reader returns (PNGReaderInterface::Get
 * transposes when rows < cols): transpose = 1 reads an azimuth-major sweep [azimuths][bins] (the filters' layout)
 * transposed, transpose = 0 reads stored rows as rings.  The image is read only (the reference thresholds it in place).
 * Refused with CFEAR_ERR_INVALID_ARGUMENT: normalize = 1 (cv::normalize runs in OpenCV's AVX2 FMA dispatch and cannot be
 * restated exactly), interpolations other than CFEAR_SC_INTER_AREA, scales below 1, an integer 2 x 2 scale (OpenCV's SIMD
 * and scalar code round it differently), a non-finite threshold.  TBV reaches none of them.                           */
#define CFEAR_SC_INTER_AREA 3           /* cv::INTER_AREA */
typedef struct cfear_sc_raw_params {
  double radar_threshold;               /* 0: cvFloor(t); bins <= t become 0                                */
  int32_t transpose;                    /* 1: the stored sweep is [azimuths][bins] (rings over its columns) */
  int32_t normalize;                    /* must be 0                                                        */
  int32_t interpolation;                /* must be CFEAR_SC_INTER_AREA                                      */
  int32_t pad;
} cfear_sc_raw_params;                  /* 24 bytes */
void cfear_sc_raw_params_default(cfear_sc_raw_params* p);
/* desc->batch sweeps (host or device, any stride and batch_stride) -> desc_out [batch][num_ring * num_sector] (host or
 * device; (double) of the 8-bit cell), ringkey [batch][num_ring] and sectorkey [batch][num_sector] optional host arrays.
 * Only num_ring / num_sector of par are read.                                                                        */
int cfear_sc_raw_descriptors(cfear_ctx* ctx, const uint8_t* imgs, const cfear_polar_desc* desc, const cfear_sc_params* par,
                             const cfear_sc_raw_params* raw, double* desc_out, double* ringkey, double* sectorkey);

/* RSCManager as a library object (place_recognition_radar RadarScancontext.cpp:156-345): the descriptor database
 * lives in HBM; makeAndSaveScancontextAndKeysRadarCloud = add, detectLoopClosureID = detect.  Host policy (recent-node
 * exclusion, odometry likelihood, ring-key search, candidate ranking) runs in the library's C++.                    */
typedef struct cfear_sc_manager cfear_sc_manager;
typedef struct cfear_sc_manager_params {
  cfear_sc_params sc;
  int32_t num_candidates_from_tree;     /* NUM_CANDIDATES_FROM_TREE (10)                                 */
  int32_t n_candidates;                 /* N_CANDIDATES kept after ranking (3)                           */
  double odom_sigma_error;              /* 0.05                                                          */
  int32_t odometry_coupled_closure;     /* ring key extended by 10 x odometry similarity (true)          */
  int32_t augment_sc;                   /* lateral augmentations {-2, 2, -4, 4} m of the query (true)    */
  double distance_exclude_recent;       /* DISTANCE_EXCLUDE_RECENT (10 m)                                */
  int64_t pad;
} cfear_sc_manager_params;              /* 88 bytes */
void cfear_sc_manager_params_default(cfear_sc_manager_params* p);
typedef struct cfear_sc_candidate {     /* RSCManager::candidate */
  double min_dist, min_dist_sc, min_dist_odom;
  float yaw_diff_rad;
  int32_t nn_idx;
  int32_t argmin_shift;
  int32_t pad;
  double Taug[3];                       /* augmentation transform of the winning query as (x, y, theta)  */
} cfear_sc_candidate;                   /* 64 bytes */
int cfear_sc_manager_create(cfear_ctx* ctx, const cfear_sc_manager_params* par, cfear_sc_manager** out);
/* cloud: the node's local map [n][4] in the node frame (host or device); Todom: the node's pose (x, y, theta). */
int cfear_sc_manager_add(cfear_sc_manager* m, const float* xyzi, int32_t n_points, const double Todom[3]);
/* makeAndSaveScancontextAndKeysRadarRaw (RadarScancontext.cpp:148-154): the node's descriptor from its raw sweep (one
 * image, host or device, see cfear_sc_raw_descriptors); the node has no lateral augmentations whatever augment_sc says.
 * Raw and cloud nodes may share one database.                                                                       */
int cfear_sc_manager_add_raw(cfear_sc_manager* m, const uint8_t* img, const cfear_polar_desc* desc,
                             const cfear_sc_raw_params* raw, const double Todom[3]);
/* candidates for the node added last, closest first; *n_out <= n_candidates.                                   */
int cfear_sc_manager_detect(cfear_sc_manager* m, cfear_sc_candidate* out, int32_t cap, int32_t* n_out);
int cfear_sc_manager_size(const cfear_sc_manager* m);
int cfear_sc_manager_destroy(cfear_sc_manager* m);

/* Whole-graph Scan Context in cloud mode (ScanContextClosure: CreateContext, loopclosure.cpp:571-591, then
 * detectLoopClosureID) for a graph known before the first detection (tbv_slam_offline).  A node carries its cloud in its
 * own frame (peaks or not, as use_peaks chooses) and rows 0 and 1 of its 4 x 4 node -> world matrix and of the inverse,
 * as the caller computed them (GetPose().matrix(), GetPose().inverse().matrix()).  The local map of node i
 * (ScansToLocalMap, loopclosure.cpp:553-569) merges the nodes whose id lies in [id_i - n_aggregate, id_i + n_aggregate]:
 * every point goes to the world frame and back into node i's frame with pcl::transformPointCloud's arithmetic (double
 * products summed left to right, ((m0 x + m1 y) + m2 z) + m3, rounded to float); z and the intensity are carried.        */
typedef struct cfear_sc_node {
  cfear_sc_cloud cloud;                 /* [n][4] in the node frame, host or device                              */
  double T[8];                          /* node -> world, rows 0 and 1 of the 4 x 4 matrix                       */
  double Tinv[8];                       /* world -> node                                                         */
  int32_t id, pad;                      /* idx_ of the node; strictly increasing                                 */
} cfear_sc_node;                        /* 152 bytes */
/* MakeRadarCloudContext of the local maps of nodes centers[0 .. n_centers) (indices into nodes), with the lateral shifts
 * of cfear_sc_descriptors: bit-identical to cfear_sc_descriptors of the host-merged clouds.  desc [n_centers][n_aug]
 * [num_ring * num_sector], ringkey [..][num_ring] and sectorkey [..][num_sector] (optional): host or device.            */
int cfear_sc_local_map_descriptors(cfear_ctx* ctx, const cfear_sc_node* nodes, int32_t n_nodes, const int32_t* centers,
                                   int32_t n_centers, int32_t n_aggregate, const cfear_sc_params* par, const double* shifts_y,
                                   int32_t n_aug, double* desc, double* ringkey, double* sectorkey);
/* The candidates a streaming cfear_sc_manager returns when nodes 0 .. n_detect - 1 are added in order, each with its local
 * map and Todom = (T[3], T[7]), and each is detected right after it is added (n_detect <= n_nodes; nodes past n_detect only
 * join local maps).  out [n_detect][par->n_candidates] and n_out [n_detect] are host arrays.  The odometry similarity is
 * evaluated on the device: its hypot / exp may differ from the host's libm in the last place.
 * Refused with CFEAR_ERR_CAPACITY: num_candidates_from_tree > 64.                                                      */
int cfear_sc_detect_sequence(cfear_ctx* ctx, const cfear_sc_manager_params* par, const cfear_sc_node* nodes, int32_t n_nodes,
                             int32_t n_aggregate, int32_t n_detect, cfear_sc_candidate* out, int32_t* n_out);

/* The same for a batch of graphs in one call, in either descriptor mode, with the ranking on the device.  The graphs' nodes
 * lie one behind the other: graph g owns nodes [node_off[g], node_off[g + 1]) (node_off[0] = 0; empty graphs are allowed)
 * and detects its first n_detect[g] of them; nodes past that only join local maps.  Graph g's rows are what a fresh
 * cfear_sc_manager returns when its nodes 0 .. n_detect[g] - 1 are added in order -- _add with the local map, or _add_raw --
 * each detected right after it is added, with the odometry similarity evaluated on the device as in
 * cfear_sc_detect_sequence: in cloud mode they equal cfear_sc_detect_sequence of that graph alone byte for byte.
 *   CFEAR_SC_NODES_CLOUD  one point buffer xyzi [point_off[n_nodes]][4] (host or device), node i's cloud in its own frame at
 *                         [point_off[i], point_off[i + 1]); the local map of a node merges the nodes of ITS graph whose id
 *                         lies within n_aggregate (ScansToLocalMap, as above).  imgs / desc / raw are not read.
 *   CFEAR_SC_NODES_RAW    node i's descriptor is cfear_sc_raw_descriptors of sweep i of imgs (host or device; desc->batch
 *                         must be n_nodes), without lateral augmentations whatever augment_sc says (cfear_sc_manager_add_raw).
 *                         xyzi / point_off / n_aggregate / Tinv are not read.
 * out [sum n_detect][par->n_candidates] and n_out [sum n_detect] hold the detected nodes' rows in graph order, both in host
 * or both in device memory (device rows stay in HBM for a later stage; the call is then asynchronous unless an input was
 * staged).  nn_idx counts within the node's graph; records past n_out[i] are all-zero bytes.  Among equal min_dist the pair
 * visited first (augmentation, then search rank) ranks first, as the manager's stable sort leaves them.
 * Refused before anything is launched, out / n_out untouched, the message naming "graph g, node i" where one node is at
 * fault: everything cfear_sc_detect_sequence and cfear_sc_raw_descriptors refuse, a non-monotone node_off or point_off, a
 * null array with a positive count, n_detect[g] outside [0, nodes of g], ids that do not increase strictly within a graph,
 * an unknown mode, out and n_out in different memories.  n_graphs = 0 or no detected node: CFEAR_OK, the device untouched.
 * The arguments are checked before the context is: a null ctx is refused last (CFEAR_ERR_INVALID_ARGUMENT).            */
#define CFEAR_SC_NODES_CLOUD 0
#define CFEAR_SC_NODES_RAW 1
typedef struct cfear_sc_batch {
  int32_t n_graphs;
  int32_t mode;                         /* CFEAR_SC_NODES_CLOUD / CFEAR_SC_NODES_RAW, for the whole call          */
  const int32_t* node_off;              /* [n_graphs + 1] host                                                   */
  const int32_t* n_detect;              /* [n_graphs] host; NULL: every node                                     */
  const int32_t* ids;                   /* [n_nodes] host, strictly increasing within a graph; NULL: 0, 1, ...   */
  const double* T;                      /* [n_nodes][8] host: node -> world rows 0 and 1; Todom = (T[3], T[7])   */
  const double* Tinv;                   /* [n_nodes][8] host: world -> node (cloud mode)                         */
  const float* xyzi;                    /* cloud mode: [point_off[n_nodes]][4], host or device                   */
  const int64_t* point_off;             /* cloud mode: [n_nodes + 1] host                                        */
  int32_t n_aggregate;                  /* cloud mode                                                            */
  int32_t pad;
  const uint8_t* imgs;                  /* raw mode: n_nodes sweeps, host or device                              */
  const cfear_polar_desc* desc;         /* raw mode: their layout, batch = n_nodes                               */
  const cfear_sc_raw_params* raw;       /* raw mode                                                              */
} cfear_sc_batch;                       /* 96 bytes */
int cfear_sc_detect_batch(cfear_ctx* ctx, const cfear_sc_manager_params* par, const cfear_sc_batch* batch,
                          cfear_sc_candidate* out, int32_t* n_out);

/* ---- caller: loop-candidate verification --------------------------------------------------------------
 * What the loop-closure thread does per candidate (tbv_slam/src/tbv_slam/loopclosure.cpp:658-725), for a batch:
 * RegisterLoopCandidate (:320-364, loopclosure::Register :35-97), VerifyLoopCandidate (:365-384) =
 * ScanLearningInterface::PredAlignment (coral_alignment_quality/src/alignment_checker/alignmentinterface.cpp:349-367:
 * CorAl + CFEAR quality -> combined logistic score "alignment_quality") + VerificationModel (:220-238), then
 * ApplyConstratins (:261-274).  One registration launch, one CorAl launch, one GetCost launch for all candidates. */
typedef struct cfear_verify_params {
  double align_intercept;               /* combined_class: file format "intercept,coef..." (alignmentinterface.cpp:224-269) */
  double align_coef[6];                 /* over {CorAl joint, sep, overlap, CFEAR cost, #residuals, mean #cells} (:357-360)  */
  double loop_intercept;                /* verification model over par_.model_features = {odom-bounds, sc-sim,               */
  double loop_coef[3];                  /*   alignment_quality} (loopclosure.h:138); preset loopclosure.cpp:224-232          */
  double model_threshold;               /* par_.model_threshold (0.8)                                                        */
  int32_t all_candidates;               /* par_.all_candidates (true): every candidate above threshold, else only the best   */
  int32_t verification_disabled;        /* probability 0 for everything (loopclosure.cpp:377)                                */
  int32_t use_covariance_sampling;      /* par_.use_covariance_sampling_in_loop_closure (false)                              */
  int32_t pad;
  cfear_coral_params coral;             /* radius 1.0, weight_res_intensity false (alignmentinterface.cpp:444)               */
  cfear_cov_sampling_params sampling;   /* loopclosure.cpp:108-112: +-0.2 m, +-0.0022 rad, 3 per axis, scaler 4              */
} cfear_verify_params;                  /* 160 bytes */
void cfear_verify_params_default(cfear_verify_params* p);

typedef struct cfear_verify_job {
  const cfear_scan* from_scan;          /* (*graph_)[from].cloud_normal_  (the query node: source of the registration)       */
  const cfear_scan* to_scan;            /* (*graph_)[to].cloud_normal_    (the candidate: fixed target)                      */
  const float* from_peaks;              /* (*graph_)[from].cloud_peaks_ [n_from][4], sensor frame; host or device            */
  const float* to_peaks;                /* (*graph_)[to].cloud_peaks_                                                        */
  int32_t n_from, n_to;
  double from_pose[3];                  /* (*graph_)[from].GetPose() as (x, y, theta)                                        */
  double t_be_guess[3];                 /* constraint.t_be on entry (Scan Context yaw / lateral guess): Tto = Tfrom * t_be   */
  double sc_sim;                        /* quality["sc-sim"]                                                                 */
  double odom_bounds;                   /* quality["odom-bounds"], e.g. from cfear_verify_by_odometry                        */
  int32_t group;                        /* candidates of one query node share a group (ApplyConstratins runs per query)      */
  int32_t pad;
} cfear_verify_job;                     /* 112 bytes */

typedef struct cfear_verify_result {
  double t_be[3];                       /* constraint.t_be after registration = Trevised^-1 * Tto; Identity if it failed     */
  double cov[36];                       /* Cov (the reference stores information = Cov.inverse()); Identity if it failed     */
  double coral[3];                      /* X_CorAl = {joint, sep, overlap}                                                   */
  double cfear[3];                      /* X_CFEAR = {cost, #residuals, mean #cells}                                         */
  double alignment_quality;             /* quality["alignment_quality"]                                                      */
  double odom_bounds, sc_sim;           /* echoed features                                                                   */
  double probability;                   /* VerifyLoopCandidate                                                               */
  int32_t reg_ok;                       /* RegisterLoopCandidate's return                                                    */
  int32_t cov_sampled;                  /* the sampled covariance replaced Register's constant one                           */
  int32_t accepted;                     /* ApplyConstratins added the loop constraint                                        */
  int32_t rank;                         /* position in the query's probability-sorted candidate list                         */
  cfear_reg_result reg;                 /* the registration's own record                                                     */
} cfear_verify_result;                  /* 480 bytes */

/* results: host memory -- every field filled, ApplyConstratins applied over the batch; or DEVICE memory (a sharded caller
 * gathers the records there, cfear_rccl_allgather_device): the records are left on the device with accepted = rank = 0, the
 * call still waits for the chain and reports its errors, and the selection is the caller's, over the gathered list
 * (cfear_verify_apply_constraints; not available with use_covariance_sampling).                                       */
int cfear_verify_loop_candidates(cfear_ctx* ctx, const cfear_verify_job* jobs, int32_t n_jobs,
                                 const cfear_verify_params* par, cfear_verify_result* results);
/* ApplyConstratins (loopclosure.cpp:261-274) over host records: groups [n] = the candidates' query ids.  No context.
 * Per query the candidates are ordered by probability, larger first, ties in input order; `rank` is the position in that
 * order and a candidate is accepted when probability > model_threshold (strictly), every one or only rank 0.  A NaN
 * probability (odom_bounds of an empty odometry chain is 0/0, cfear_verify_by_odometry) ranks after every finite one of its
 * query, in input order, and is never accepted -- so it never takes the best place from a finite candidate.  (The
 * reference's std::sort is undefined with NaN keys; this is the rule chosen here, and the oracle's.)                    */
int cfear_verify_apply_constraints(const int32_t* groups, int32_t n, const cfear_verify_params* par, cfear_verify_result* results);
/* loopclosure::VerifyByOdometry (loopclosure.cpp:776-808).  rel_xyt [n][3]: the odometry constraints'
 * RelativeMotion(i, i+1), i = to .. from-1.  similarity = 1 - exp(-(max(|T_odom| - 5, 0) / travelled)^2 / 2 sigma^2);
 * 1 when verify_via_odometry is 0.  No context: pure host arithmetic.                                               */
int cfear_verify_by_odometry(const double* rel_xyt, int32_t n, double odom_sigma_error, int32_t verify_via_odometry,
                             double* similarity);

/* ---- caller: candidate batches sharded over the GPUs of one node, for a C++ host ------------------------------
 * Loop-closure candidates are independent (loopclosure.cpp:658-721), so a batch shards by contiguous blocks of
 * ceil(n / world) candidates per rank (one process, context and GPU per rank), with ONE all_gather of the fixed-size
 * result records at the end -- rank order = candidate order.  The host owns the communicator: the collective is a
 * callback gather(user, send, recv, bytes) that must place every rank's `bytes` bytes, rank after rank, into recv on
 * every rank and return 0.  cfear_rccl_allgather is that callback over an ncclComm_t (RCCL over xGMI), user = a
 * cfear_rccl_comm; librccl.so is resolved at run time.  jobs / n_jobs are the FULL candidate list on every rank and
 * results receives all n_jobs records on every rank.  world == 1 needs no callback (NULL); a callback that is given is
 * called at every world size, 1 included.  A rank whose own block fails still takes part in the exchange (its status rides
 * in an 8-byte trailer behind its block) and EVERY rank returns the first failed rank's status.  With cfear_rccl_allgather
 * as the callback cfear_register_batch_sharded keeps the records on the device: the kernel writes into the send buffer,
 * ncclAllGather moves them, one device-to-host copy returns all of them.                                                */
typedef int (*cfear_allgather_fn)(void* user, const void* send, void* recv_all, size_t bytes_per_rank);
typedef struct cfear_rccl_comm { cfear_ctx* ctx; void* nccl_comm; int32_t world, pad; } cfear_rccl_comm;
int cfear_rccl_allgather(void* user /* cfear_rccl_comm* */, const void* send, void* recv_all, size_t bytes_per_rank);
/* the same collective on DEVICE buffers: enqueued on the communicator's context stream, not synchronised */
int cfear_rccl_allgather_device(void* user /* cfear_rccl_comm* */, const void* d_send, void* d_recv_all, size_t bytes_per_rank);
/* A communicator of the library's own making for hosts that have none (librccl.so resolved at run time): rank 0 asks for
 * the 128-byte id and hands it to its peers by whatever means it has (MPI, a socket, torch.distributed); every rank then
 * calls cfear_rccl_comm_init with it.  The communicator's collectives run on streams of `ctx`.                          */
int cfear_rccl_unique_id(char id128[128]);
int cfear_rccl_comm_init(cfear_ctx* ctx, const char id128[128], int32_t world, int32_t rank, cfear_rccl_comm* out);
int cfear_rccl_comm_destroy(cfear_rccl_comm* comm);
int cfear_shard_range(int32_t n, int32_t world, int32_t rank, int32_t* lo, int32_t* hi, int32_t* per_rank);
/* the gather step alone: local = this rank's hi - lo records; all = n_total records in candidate order */
int cfear_gather_records(const void* local, int32_t n_total, int32_t record_bytes, int32_t world, int32_t rank,
                         cfear_allgather_fn gather, void* user, void* all);
int cfear_register_batch_sharded(cfear_ctx* ctx, const cfear_reg_job* jobs, int32_t n_jobs, const cfear_reg_params* par,
                                 int32_t rank, int32_t world, cfear_allgather_fn gather, void* user,
                                 cfear_reg_result* results);
/* Pipelined steps of a sharded candidate batch (loopclosure.cpp:658-721 hands candidates over as the odometry produces
 * nodes): a rank's block of an 8-way sharded batch is ~0.13 ms of kernel, so what sits around the kernel decides the
 * rate.  A pipe keeps up to `depth` steps in flight: submit() stages this rank's block of the FULL candidate list (pinned:
 * the device reads it in place), enqueues the expand kernel on the pipe's preparation stream (beside the previous step's
 * matcher), the matcher on the context's stream and all_gather -> device-to-host copy on the pipe's exchange stream, and
 * returns without waiting; collect() waits on ONE event and returns all n records in candidate
 * order (status rules as cfear_register_batch_sharded: every rank enters the collective, every rank returns the first
 * failed rank's status).  comm = NULL (world 1 only): no collective.  flags & CFEAR_PIPE_GRAPH: a slot's matcher launches
 * are captured into a hipGraph on its first step and replayed while the block's size and geometry, the parameters and the
 * context's scratch stay the same.  Steps are collected in any order, but a slot (ticket % depth) is free again only after its
 * collect.  The table must outlive the pipe.                                                                          */
typedef struct cfear_candidate_pipe cfear_candidate_pipe;
enum { CFEAR_PIPE_GRAPH = 1, CFEAR_PIPE_TIMING = 2 /* hipEvents around the exchange of every step (measurement) */ };
int cfear_candidate_pipe_create(cfear_ctx* ctx, const cfear_scan_table* table, int32_t max_candidates, int32_t rank,
                                int32_t world, const cfear_rccl_comm* comm, int32_t depth, int32_t flags,
                                cfear_candidate_pipe** out);
int cfear_candidate_pipe_submit(cfear_candidate_pipe* pipe, const cfear_candidate* candidates, int32_t n_total,
                                const cfear_reg_params* par, int64_t* ticket);
int cfear_candidate_pipe_collect(cfear_candidate_pipe* pipe, int64_t ticket, cfear_reg_result* results);
int cfear_candidate_pipe_destroy(cfear_candidate_pipe* pipe);
/* measurement: the exchange stream's time (all_gather + read-back, CFEAR_PIPE_TIMING) summed over the collected steps, their
 * number, and how many slots currently replay a captured graph */
int cfear_candidate_pipe_stats(const cfear_candidate_pipe* pipe, double* exchange_ms_sum, int64_t* steps_collected, int32_t* graph_slots);
/* verification: ApplyConstratins (loopclosure.cpp:261-274) is redone over the gathered list, because the candidates
 * of one query may sit on two ranks                                                                             */
int cfear_verify_loop_candidates_sharded(cfear_ctx* ctx, const cfear_verify_job* jobs, int32_t n_jobs,
                                         const cfear_verify_params* par, int32_t rank, int32_t world,
                                         cfear_allgather_fn gather, void* user, cfear_verify_result* results);

/* ---- caller: batched radarDriver + OdometryKeyframeFuser --------------------------------------
 * n_streams independent sequences advance one frame per call: filter (F) -> compensate (C) ->
 * surface points (N) -> Register against the keyframe window (M) -> keyframe policy.  Restates
 * radarDriver::CallbackOffline (radar_driver.cpp:163-176) + OdometryKeyframeFuser::processFrame
 * (odometrykeyframefuser.cpp:143-259) per stream; everything between the polar image and the
 * pose stays on the GPU.                                                                      */
typedef struct cfear_odometry_params {
  int32_t filter_type;                  /* cfear_filter_type */
  cfear_kstrong_params kstrong;
  cfear_cacfar_params cacfar;
  cfear_reg_params reg;
  float res;                            /* par.res */
  int32_t submap_scan_size;
  int32_t weight_intensity, use_guess, compensate, radar_ccw, use_keyframe;
  int32_t rotate_ccw;                   /* 1: the incoming images are [range bins][azimuths] (dataset != oxford), to be
                                           rotated first, radar_driver.cpp:74-90; desc then describes that source layout.
                                           (The k-strongest stage reads such images directly where their geometry allows --
                                           see cfear_filter_kstrongest_rowkeys -- and rotates them otherwise.)          */
  double min_keyframe_dist, min_keyframe_rot_deg, downsample_factor;
  int32_t estimate_cov_by_sampling;     /* par.estimate_cov_by_sampling (false), odometrykeyframefuser.h:104 */
  int32_t keep_nodes;                   /* 1: also build what RadarScan needs (types.h:119-122): the peaks cloud of every
                                           frame, compensated like the cloud (odometrykeyframefuser.cpp:146-150), so that
                                           cfear_odometry_get_scan / _get_cloud / _get_peaks can hand out graph nodes */
  cfear_cov_sampling_params cov_sampling;   /* cov_sampling_* (:107-110) */
} cfear_odometry_params;
void cfear_odometry_params_default(cfear_odometry_params* p);   /* CFEAR-3 preset, Oxford */
/* The reference's shipped configurations (cfear_radarodometry/launch/oxford/eval/params/baseline/oxford_cfear-{1,2,3,
 * 3-s10}:13-26) and sensor setups (tbv_slam/script/{oxford,mulran,kvarntorp,volvo}/run_tbv_simple.sh):
 *   CFEAR-1      P2L, 1 keyframe,  res 3.5, k 12, Huber 0.1, weight option 4, no intensity weights
 *   CFEAR-2      P2L, 3 keyframes, res 3.5, k 12, Huber 0.1
 *   CFEAR-3      P2P, 4 keyframes, res 3,   k 40, Huber 0.1, intensity weights (TBV's default)
 *   CFEAR-3-s10  P2P, 10 keyframes, res 3,  k 40, Cauchy 0.1, regularization 0.1
 *   Oxford       range_res 0.0438,    clockwise sweep,         rows = azimuths
 *   MulRan       range_res 0.0595238, counter-clockwise sweep, [range bins][azimuths] images (rotate_ccw)
 *   Kvarntorp / Volvo  range_res 0.175, counter-clockwise,     [range bins][azimuths] images
 * Everything else as cfear_odometry_params_default.  Returns CFEAR_ERR_INVALID_ARGUMENT for unknown ids.        */
enum cfear_preset { CFEAR_PRESET_CFEAR1 = 1, CFEAR_PRESET_CFEAR2 = 2, CFEAR_PRESET_CFEAR3 = 3, CFEAR_PRESET_CFEAR3_S10 = 4 };
enum cfear_dataset { CFEAR_DATASET_OXFORD = 0, CFEAR_DATASET_MULRAN = 1, CFEAR_DATASET_KVARNTORP = 2, CFEAR_DATASET_VOLVO = 3 };
int cfear_odometry_params_preset(cfear_odometry_params* p, int preset, int dataset);

/* The two per-frame decisions of OdometryKeyframeFuser as pure host functions (no context, no GPU), used by the batched
 * pipeline below and callable on their own:
 *   cfear_keyframe_based_fuse    KeyFrameBasedFuse (odometrykeyframefuser.cpp:62-73): diff = T_keyframe^-1 * Tcurrent as
 *                                (x, y, theta); 1 = add a keyframe (translation norm > min_keyframe_dist or |rotation| >
 *                                min_keyframe_rot_deg, both strict; always 1 without use_keyframe)
 *   cfear_acc_vel_sanity_check   AccelerationVelocitySanityCheck (:76-94): translations of the previous and the current
 *                                motion; 0 = acceleration > 200 m/s^2 or speed > 200 m/s at 4 Hz -> the caller keeps
 *                                its guess (:198-199)                                                              */
int cfear_keyframe_based_fuse(const double diff_xyt[3], int32_t use_keyframe, double min_keyframe_dist,
                              double min_keyframe_rot_deg);
int cfear_acc_vel_sanity_check(const double tmot_prev_xy[2], const double tmot_curr_xy[2]);

typedef struct cfear_odometry cfear_odometry;
typedef struct cfear_frame_info {
  double pose[3];                       /* Tcurrent (x,y,theta) */
  int32_t n_points, n_cells;
  int32_t keyframe_added;
  int32_t reg_status;                   /* cfear_reg_result.status, or 1 for the first frame */
  int32_t outer_iters, lm_iters;
  double score;
} cfear_frame_info;

int cfear_odometry_create(cfear_ctx* ctx, int32_t n_streams, const cfear_polar_desc* desc,
                          const cfear_odometry_params* par, cfear_odometry** out);
/* polar: [n_streams] images laid out per desc (desc.batch must equal n_streams), host or device.
 * info: host array [n_streams].                                                               */
int cfear_odometry_process(cfear_odometry* od, const uint8_t* polar, cfear_frame_info* info);
/* Same, and additionally enqueues the FILTER of the next frame's images (polar_next, may be NULL) behind
 * this frame's kernels, so the GPU sweeps the next polar batch while the host applies this frame's
 * keyframe policy.  The next call must then pass that same pointer as `polar`: the hit is decided by the
 * pointer value only (see cfear_odometry_discard_prefetch).  Return value: per-stream failures (empty sweep,
 * capacity) do not stop the other streams -- every info[b] is filled, info[b].reg_status holds the stream's
 * own status and the call returns the first such status; a failed prefetch is reported the same way after
 * this frame has been completed.                                                                  */
int cfear_odometry_process_prefetch(cfear_odometry* od, const uint8_t* polar, const uint8_t* polar_next,
                                    cfear_frame_info* info);
/* The same step for hosts whose sweeps do not sit at a constant stride (one ring buffer per sequence, sensor drivers
 * with their own allocations): stream b's image starts at base + offsets[b] bytes (device memory, laid out per desc
 * otherwise); offsets_next (may be NULL) names the next frame's images for the prefetch, which is recognised on the
 * next call by the same base and the same offsets.  offsets are HOST arrays [n_streams].  Available for the
 * k-strongest filter with k <= 64, rows = azimuths, keep_nodes = 0 (the fused filter output); otherwise
 * CFEAR_ERR_INVALID_ARGUMENT.                                                                                   */
int cfear_odometry_process_offsets(cfear_odometry* od, const uint8_t* base, const int64_t* offsets,
                                   const int64_t* offsets_next, cfear_frame_info* info);
/* Forget a prefetched filter output.  A prefetch hit is decided by the address (and offsets) of the images alone: a
 * host that REUSES a buffer for different content (drops a frame, rewrites a ring slot) must call this first, or the
 * stale filter output of the earlier content is consumed.                                                        */
int cfear_odometry_discard_prefetch(cfear_odometry* od);
/* The same step for callers whose own driver has filtered the sweep: OdometryKeyframeFuser::pointcloudCallback(cloud,
 * cloud_peaks, Tcurrent, t, cov) (odometrykeyframefuser.cpp:413-426) for every stream.  clouds [n_streams]: the filtered
 * clouds (x, y, z, intensity; host or device, <= rows * k points each); peaks [n_streams] (may be NULL): the peaks
 * clouds, kept (and compensated) only with par.keep_nodes.  Everything after the filter is unchanged.            */
int cfear_odometry_process_clouds(cfear_odometry* od, const cfear_sc_cloud* clouds, const cfear_sc_cloud* peaks,
                                  cfear_frame_info* info);
/* cov_current of every stream after the last processed frame (row-major 6x6, host [n_streams][36]):
 * Identity before the first registration and after a failed one (FormatScans' initial value survives),
 * Register's constant diag(0.01, 0.01, 0, 0, 0, 1e-4) otherwise, or the sampled covariance when
 * estimate_cov_by_sampling is set and the fit succeeded (odometrykeyframefuser.cpp:196, 203-208).
 * sampled (optional, [n_streams]) receives 1 where the sampled covariance was used.                */
int cfear_odometry_get_covariance(cfear_odometry* od, double* cov, int32_t* sampled);

/* ---- replay of a recorded trajectory ------------------------------------------------------------------------------
 * Registers frame t from the RECORDED pose of frame t - 1 and the RECORDED keyframe set, for every frame of one or more
 * sequences, as a few batched launches: no frame's input depends on another frame's result, so one legal divergence
 * between two builds cannot poison the frames behind it, and "how good is each registration" is
 * separated from "how does drift accumulate".  The trace may be another build's, ground truth or this library's own.
 * A frame's state is what cfear_odometry_process would hold had the trace been its own output, derived with the same
 * functions.  Per sequence, with trace poses P_0 .. P_n-1 (seq_offsets [n_seq + 1] delimits the sequences' frames):
 *   frame 0    the first keyframe, at P_0; no job: reg_status 1, is_keyframe 1, pose = guess = P_0.
 *   motion     M_1 = identity, M_t = P_t-2^-1 P_t-1; frame t's cloud is compensated by M_t (par->compensate,
 *              par->radar_ccw), its guess is P_t-1 M_t (par->use_guess; P_t-1 otherwise).
 *   keyframes  frame t >= 1 is one iff cfear_keyframe_based_fuse(xyt(P_lastkf^-1 P_t), ...): by the TRACE pose.
 *   window     the last min(submap_scan_size, count) keyframes among the frames before t, in order, at their trace poses.
 *   job        scans [window.., scan_t], poses [window trace poses.., guess_t], par->reg: what FormatScans builds.
 *   sanity     cfear_acc_vel_sanity_check on M_t and P_t-1^-1 pose.
 * A frame whose scan failed (empty cloud, capacity) reports that status in reg_status and runs no job; so does a frame
 * whose window holds such a scan; the other frames are unaffected and the call returns the first such status.
 * estimate_cov_by_sampling and keep_nodes are NOT part of a replay and are ignored; submap_scan_size <= 15.
 * The scans are made by the surface-point kernels and registered by the matcher through their launchers, unchanged; job
 * and result records are written and read on the device, one read-back of `out` ends each chunk of frames.
 * The matcher's forms agree to 1e-11 where a batch size changes the form (see cfear_reg_job): a replay of this library's
 * own trace meets the live poses to that, not necessarily to the bit -- the trace also keeps (x, y, theta) where the live
 * state keeps the matrix.
 * Refused with CFEAR_ERR_INVALID_ARGUMENT before anything is launched, the message naming the sequence or frame: a null
 * argument, n_seq < 1, seq_offsets that do not start at 0 or hold an empty sequence (not ascending), a trace pose that is
 * not finite, a cloud with n < 0 or without points, unknown flags, a desc.batch other than the number of frames.
 * cfear_odometry_replay is the same for raw sweeps: desc (batch = all frames, one behind the other at batch_stride) and polar
 * as cfear_odometry_process takes them, host or device; par->filter_type selects the filter, par->rotate_ccw the decode of
 * [range bins][azimuths] sources.  The filter runs through its own entry points, the clouds stay on the device.
 * CFEAR_REPLAY_AUDIT folds the two audits into every record, through their own entry points on the same scans, poses and
 * clouds: cfear_association_ties_batch twice -- at the guess with itr = 1 (n_tied_start, n_tied_effective_start) and at the
 * registered pose with itr = 2 (_end) --, cfear_voxel_order_audit_batch on every frame's compensated cloud, n_voxels_exposed
 * and n_voxels_changed_reversed summed over the job's scans (the frame's own scan where it has no job); exposed = 1 iff an
 * *_effective_* count or n_voxels_exposed is > 0.  Without the flag these fields are -1 and every other field is the same bits.
 * The caveats of DESIGN.md section 3 carry over: a tie is a snapshot at two poses -- one that exists only at an association
 * pass in between is invisible to it --, a tie between bitwise equal cells is not counted as effective, and nothing here
 * says which way FLANN decides a tie or which order libstdc++ leaves a voxel's points in: exposed = 0 says a reference build
 * has no such licence to differ on this frame, exposed = 1 only that it has one.                                       */
#define CFEAR_REPLAY_AUDIT 1
typedef struct cfear_replay_frame {
  double pose[3];                       /* Register's result for this frame (raw, before the sanity check)                */
  double guess[3];                      /* the start pose the job was given                                               */
  double dev[3];                        /* (x, y, theta) of T_trace(t)^-1 T_final(t); T_final = pose, or guess where sanity_ok = 0 */
  double score, final_cost, last_relative_decrease;
  int32_t n_points, n_cells, is_keyframe, n_targets;
  int32_t reg_status, outer_iters, lm_iters, num_residuals;
  int32_t sanity_ok;
  int32_t n_tied_start, n_tied_effective_start, n_tied_end, n_tied_effective_end;   /* CFEAR_REPLAY_AUDIT, else -1         */
  int32_t n_voxels_exposed, n_voxels_changed_reversed;                              /* summed over the job's scans; else -1 */
  int32_t exposed;                                                                  /* 1 / 0 with the audit, else -1       */
} cfear_replay_frame;                   /* 160 bytes, no implicit padding */
int cfear_odometry_replay(cfear_ctx* ctx, const cfear_polar_desc* desc, const uint8_t* polar, const cfear_odometry_params* par,
                          const double* trace_xyt, const int32_t* seq_offsets, int32_t n_seq, int32_t flags, cfear_replay_frame* out);
int cfear_odometry_replay_clouds(cfear_ctx* ctx, const cfear_sc_cloud* clouds, const cfear_odometry_params* par,
                                 const double* trace_xyt, const int32_t* seq_offsets, int32_t n_seq, int32_t flags,
                                 cfear_replay_frame* out);
/* The RadarScan of a stream's LAST processed frame (scan_, odometrykeyframefuser.cpp:172, 244) -- call after a frame
 * whose keyframe_added is set to collect a pose-graph node; valid until the next cfear_odometry_process:
 *   get_scan   a copy of cloud_normal_ (MapPointNormal) as a new handle (cfear_scan_destroy it)
 *   get_cloud  cloud_nopeaks_: the filtered cloud after Compensate (what the surface points were built from)
 *   get_peaks  cloud_peaks_: the AxialNonMaxSupress subset after Compensate (needs par.keep_nodes)
 * xyzi: host or device buffer [cap][4], or NULL to query the count in *n_out.                                  */
int cfear_odometry_get_scan(cfear_odometry* od, int32_t stream, cfear_scan** out);
int cfear_odometry_get_cloud(cfear_odometry* od, int32_t stream, float* xyzi, int32_t cap, int32_t* n_out);
int cfear_odometry_get_peaks(cfear_odometry* od, int32_t stream, float* xyzi, int32_t cap, int32_t* n_out);
int cfear_odometry_destroy(cfear_odometry* od);

/* ---- a parameter grid of odometry streams as one batch ------------------------------------------------------------------
 * The reference evaluates CFEAR as a grid of configurations over sequences (launch/oxford/eval/params/grid_search/: one
 * job per (sequence, configuration), dealt to processes by utils/worker).  A grid object advances all of those jobs one frame
 * per call: stream s runs configuration stream_config[s] on the images of sequence stream_sequence[s].  Per stream the state
 * and every field of cfear_frame_info are those of a cfear_odometry created with that configuration and fed that sequence's
 * images, with the failure semantics of cfear_odometry_process: a failed stream reports its own status and keeps its state,
 * the others go on, and the call returns the first such status.
 *
 * What the streams share is computed once:
 *   sweep     per sequence image ONE k-strongest row sweep serves all of its k-strongest streams: directly (the fused row
 *             keys) where they agree on (k, uchar(z_min), min range bin, range_res) -- one filter class --, else at
 *             (max k, min uchar(z_min)) into sel_* lists from which cfear_kstrong_rowkeys_derive writes every class's row
 *             keys.  CA-CFAR configurations get one sweep per distinct (sequence, cfear_cacfar_params).
 *   surface   one launch per distinct (res, downsample_factor, weight_intensity, radar_ccw, filter kind, range_res, row
 *             stride) over that group's jobs; a job reads its class's shared row keys with its own motion and compensate.
 *   matcher   one launch per distinct (cfear_reg_params, submap_scan_size) over that group's jobs.
 * All groups' results come down in one read-back per call.
 *
 * desc: the layout of the n_sequences = desc->batch images a call is given.  stream_sequence / stream_config: [n_streams], or
 * both NULL for the full product, sequence-major and configuration fastest (n_streams must then be desc->batch * n_configs):
 * the order of utils/worker's loops, stream s being the reference's job_<s + 1>.
 *
 * cfear_odometry_grid_plan: the grouping as pure host code (no context, no device); cfear_odometry_grid_create takes its
 * grouping from this very plan.  streams (optional) [n_streams]; totals (optional); why (optional, why_len bytes) receives
 * the reason of a refusal.  The streams of a surface group occupy surface_slot [first, first + n) of that group and those of
 * a matcher group matcher_slot [first, first + n): both slot orders are permutations of the streams in which every group is
 * contiguous, streams in index order inside a group.
 * Refused with CFEAR_ERR_INVALID_ARGUMENT, the message naming the configuration or stream: null desc or configs, n_configs
 * or n_streams < 1, only one of the two stream arrays, the full product with another n_streams, an index outside its range,
 * keep_nodes or estimate_cov_by_sampling set, a k-strongest configuration that the fused row-key hand-over of
 * cfear_odometry_create would not take (k > 64, more than 4096 azimuths, rows * k beyond the surface stage's capacity), more
 * than 4096 azimuths with CA-CFAR, rotate_ccw that differs between configurations, and whatever cfear_odometry_create
 * refuses for that configuration.  Graph nodes, constraints, sampled covariances and the prefetch are outside a grid.     */
typedef struct cfear_odometry_grid cfear_odometry_grid;
typedef struct cfear_grid_stream {
  int32_t sequence, config;
  int32_t sweep;                        /* index of the sweep that produces this stream's row keys                        */
  int32_t filter_class;                 /* index of its filter class (classes are numbered sweep by sweep)                */
  int32_t surface_group, matcher_group;
  int32_t surface_slot, matcher_slot;
} cfear_grid_stream;
typedef struct cfear_grid_totals {
  int32_t n_streams, n_sequences;
  int32_t n_sweeps;                     /* k-strongest + CA-CFAR                                                          */
  int32_t n_classes;                    /* over all sweeps                                                                */
  int32_t n_derived_classes;            /* of those, classes whose keys cfear_kstrong_rowkeys_derive writes               */
  int32_t max_classes_per_sequence;
  int32_t n_surface_groups, n_matcher_groups;
} cfear_grid_totals;
int cfear_odometry_grid_plan(const cfear_polar_desc* desc, const cfear_odometry_params* configs, int32_t n_configs,
                             const int32_t* stream_sequence, const int32_t* stream_config, int32_t n_streams,
                             cfear_grid_stream* streams, cfear_grid_totals* totals, char* why, int32_t why_len);
int cfear_odometry_grid_create(cfear_ctx* ctx, const cfear_polar_desc* desc, const cfear_odometry_params* configs, int32_t n_configs,
                               const int32_t* stream_sequence, const int32_t* stream_config, int32_t n_streams,
                               cfear_odometry_grid** out);
/* polar: desc->batch images laid out per desc, host or device.  info: host array [n_streams].                             */
int cfear_odometry_grid_process(cfear_odometry_grid* grid, const uint8_t* polar, cfear_frame_info* info);
int cfear_odometry_grid_destroy(cfear_odometry_grid* grid);

/* ---- after the path: pose-graph nodes on disk ------------------------------------------------
 * simple_graph.sgh = Boost binary archive of std::vector<std::pair<RadarScan, std::vector<Constraint3d>>>
 * (types.h:46-192, types.cpp:103-130; MapPointNormal::save/load pointnormal.h:206-228; serialization.h): what
 * OdometryKeyframeFuser::SaveGraph writes and the loop-closure tools read back ("advanced usage", README.md:113-168).
 * Pure host code, no context.  The archive layout is restated from Boost 1.71's sources; no reference-produced file
 * exists in the repository to pin it against (csrc/graph.hip says what is assumed).                              */
typedef struct cfear_pose3d { double p[3]; double q[4]; } cfear_pose3d;      /* Pose3d: translation, quaternion (x, y, z, w) */
void cfear_pose3d_from_xyt(const double xyt[3], cfear_pose3d* out);          /* PoseEigToCeres of a planar pose (types.cpp:25-32) */
void cfear_pose3d_to_xyt(const cfear_pose3d* p, double xyt[3]);
typedef struct cfear_graph_cloud {      /* pcl::PointCloud<PointXYZI>::Ptr: n < 0 = null pointer */
  const float* xyzi;                    /* [n][4] x, y, z, intensity */
  int32_t n;
  uint32_t seq;                         /* header.seq */
  uint64_t stamp;                       /* header.stamp */
  const char* frame_id;                 /* header.frame_id (NULL = "") */
} cfear_graph_cloud;
typedef struct cfear_graph_constraint { /* Constraint3d, types.h:152-186 */
  uint64_t id_begin, id_end;
  cfear_pose3d t_be;
  double information[36];               /* row-major 6x6 */
  int32_t type;                         /* ConstraintType: 0 odometry, 1 loop_appearance, 2 mini_loop, 3 candidate */
  int32_t n_quality;
  const char* const* quality_keys;      /* std::map<std::string, double> quality, in key order */
  const double* quality_values;
  const char* info;
} cfear_graph_constraint;
typedef struct cfear_graph_node {       /* RadarScan (types.h:88-142) + the constraints stored with it */
  cfear_pose3d T, Tgt;
  int32_t has_Tgt;
  uint32_t idx;                         /* idx_ */
  uint64_t stamp;                       /* stamp_ */
  double motion[16];                    /* motion_: Affine3d::data(), column-major 4x4 */
  cfear_graph_cloud cloud_peaks, cloud_nopeaks;
  int32_t has_normal;                   /* cloud_normal_ != NULL */
  int32_t input_is_nopeaks;             /* cloud_normal_->input_ is the cloud_nopeaks_ object (how the fuser builds nodes): stored once */
  cfear_graph_cloud normal_input;       /* cloud_normal_->input_ otherwise */
  const cfear_cell* cells;              /* cloud_normal_->cells */
  int32_t n_cells;
  float radius;                         /* radius_ */
  int32_t weight_intensity, pad;
  const cfear_graph_constraint* constraints;
  int32_t n_constraints, pad2;
} cfear_graph_node;
typedef struct cfear_graph cfear_graph;
/* SaveSimpleGraph.  Boost stores an object reached through several shared_ptrs once: here the buffer is the identity -- a
 * cloud whose `xyzi` pointer (and size) equals that of a cloud written earlier, in any slot of any node, is written as a
 * reference to it.  cfear_graph_load resolves such references (its nodes then hold equal copies) and rejects files whose
 * counts exceed what is left of the file (CFEAR_ERR_FORMAT) before allocating anything.                              */
int cfear_graph_save(const char* path, const cfear_graph_node* nodes, int32_t n_nodes);
int cfear_graph_load(const char* path, cfear_graph** out);                                    /* LoadSimpleGraph */
int cfear_graph_size(const cfear_graph* g);
int cfear_graph_node_at(const cfear_graph* g, int32_t i, cfear_graph_node* out);              /* pointers live until destroy */
int cfear_graph_destroy(cfear_graph* g);
/* ---- after the path: pose-graph optimisation -----------------------------------------------------
 * Replaces tbv_slam's CeresLeastSquares::Solve (tbv_slam/src/tbv_slam/ceresoptimizer.cpp:13-113) with its
 * PoseGraph3dErrorTerm (include/tbv_slam/ceresoptimizer.h:55-112): one 6-residual block per constraint,
 * sqrt_information = llt(I_scaled).matrixL() with I_scaled = diag(1/odom_vxx, 1/odom_vyy, 1, 1, 1, 1/odom_vtt) (both
 * types -- the loop_v* values are never read, :79-88) or the constraint's own information, times 1 / loop_scaling for
 * loop constraints; no loss on odometry, CauchyLoss(0.1) on loop_appearance; mini_loop / candidate constraints are not
 * optimised; the first node (smallest id) is constant; quaternions move on ceres::EigenQuaternionParameterization;
 * ceres::Solve with the default trust-region LM and max_num_iterations 200.  cfear_pgo_solve is host code and takes one
 * graph and no context; cfear_pgo_solve_batch below solves many on the device (csrc/pgo.hip says what runs where).  poses [n] in/out, ids [n] strictly ascending (the reference's node map order).                        */
typedef struct cfear_pgo_params {        /* tbv_slam::OptimizationParamsConfig as CeresLeastSquares::Parameters sets it */
  double loop_vxx, loop_vyy, loop_vtt, odom_vxx, odom_vyy, odom_vtt, loop_scaling;
  int32_t replace_cov_by_identity;
  int32_t max_num_iterations;            /* 200 (ceresoptimizer.cpp:52) */
  double loop_loss_limit;                /* CauchyLoss(0.1) (:36) */
} cfear_pgo_params;
void cfear_pgo_params_default(cfear_pgo_params* p);
typedef struct cfear_pgo_summary {
  double initial_cost, final_cost;       /* ceres::Solver::Summary */
  int32_t iterations;                    /* summary.iterations.size() - 1 */
  int32_t usable;                        /* IsSolutionUsable() */
  int32_t num_residual_blocks;
  int32_t linear_iterations;             /* conjugate-gradient iterations over all steps */
} cfear_pgo_summary;
int cfear_pgo_solve(cfear_pose3d* poses, const uint64_t* ids, int32_t n, const cfear_graph_constraint* constraints,
                    int32_t m, const cfear_pgo_params* par, cfear_pgo_summary* summary);
/* n_graphs independent graphs in one call, one wavefront each (csrc/pgo_batch.hip): graph g owns poses / ids
 * [node_offsets[g], node_offsets[g + 1]) and constraints [constraint_offsets[g], constraint_offsets[g + 1]); both offset
 * arrays hold n_graphs + 1 entries, start at 0 and end at n_nodes / n_constraints (the lengths of the arrays, so that a
 * mis-sized table is refused).  One parameter set for the batch, summaries [n_graphs].  Per graph the semantics are those
 * of cfear_pgo_solve, decision for decision: the same residual blocks in the same order, loss, constant first node,
 * parameterisation, column scaling, trust-region bookkeeping and tolerances; sums that the host runs serially are split
 * over the lanes in an order fixed by the graph alone, so iterations, usable and num_residual_blocks equal the host's and
 * poses and costs agree with it to summation-order noise (EXPERIMENTS.md, "Batched pose-graph optimisation").  A graph's poses and summary are
 * bit-identical whatever else the batch holds, wherever the graph sits in it and however the batch is chunked
 * (CFEAR_OPT_PGO_GRAPH_CHUNK).  All arrays are host memory; the call returns when poses and summaries are written.
 * A graph that cfear_pgo_solve would refuse (ids not ascending, a constraint on an unknown node, nothing to optimise,
 * information that is not positive definite) fails the whole call with CFEAR_ERR_INVALID_ARGUMENT before anything is
 * launched or written; a graph whose state exceeds one chunk's device budget (millions of nodes) fails it with
 * CFEAR_ERR_CAPACITY.  *failed_graph (optional) is the first such graph, or -1; cfear_last_error names it too.       */
int cfear_pgo_solve_batch(cfear_ctx* ctx, cfear_pose3d* poses, const uint64_t* ids, const int64_t* node_offsets, int64_t n_nodes,
                          const cfear_graph_constraint* constraints, const int64_t* constraint_offsets, int64_t n_constraints,
                          int32_t n_graphs, const cfear_pgo_params* par, cfear_pgo_summary* summaries, int32_t* failed_graph);

/* OdometryKeyframeFuser::AddToGraph (odometrykeyframefuser.cpp:428-445) for `stream`: the odometry constraint from the
 * keyframe added by the LAST processed frame to the keyframe before it -- id_begin / id_end are the stream's keyframe
 * ordinals (RadarScan::counter), t_be = Tfrom^-1 * Tto, type odometry.  The reference stores information = C.inverse()
 * of cov_current with its 3x3 block rotated into the from-frame.  Where C has an inverse -- the covariance sampled with
 * estimate_cov_by_sampling (Identity on z, roll and pitch) and the Identity a failed registration leaves -- information
 * is that full 6x6 inverse, as in the reference.  Register's constant diag(0.01, 0.01, 0, 0, 0, 1e-4) is singular, so
 * the reference's matrix is not finite -- there information is the inverse on the planar (x, y, yaw) sub-space and
 * zero elsewhere.  CFEAR_ERR_INVALID_ARGUMENT if the last PROCESSED frame added no keyframe or the first one: a frame
 * that failed (an empty cloud) counts as processed and leaves no constraint behind.                                */
int cfear_odometry_get_constraint(cfear_odometry* od, int32_t stream, cfear_graph_constraint* out);

/* ---- after the path: trajectory evaluation (the KITTI odometry metric) ---------------------------------------------
 * What every run script of the reference ends in: radar_kitti_benchmark/python/eval_odom.py --align 6dof, i.e.
 * KittiEvalOdom.eval of radar_kitti_benchmark/python/kitti_odometry.py (:636-784), for a batch of (estimate, ground
 * truth) pairs in one call.  Per pair: both trajectories are normalised by the inverse of their own first pose (:708-714),
 * the estimate is aligned (`6dof`: umeyama_alignment without scale, :32-79), the ground-truth distances are summed
 * serially (:123-141), and for every start frame 0, step_size, 2 step_size, ... and every length the segment ending at
 * the first frame whose distance EXCEEDS dist[first] + length gives one row (:197-249).  Inverses are general 3 x 4
 * inverses (np.linalg.inv), not transposes: the rotation blocks of a 6-decimal pose file are not orthonormal.
 * All figures are radians and fractions; write_result (:608-630) prints ave_t_err * 100 [%], ave_r_err / pi * 180 * 100
 * [deg / 100 m], the two rotation RPE figures and bias_theta * 180 / pi [deg], and the rest as they are.
 * A trajectory's results do not depend on the other trajectories of the batch.               */
#define CFEAR_EVAL_NUM_LENGTHS 8
#define CFEAR_EVAL_ALIGN_NONE 0
#define CFEAR_EVAL_ALIGN_6DOF 1
#define CFEAR_EVAL_ALIGN_SCALE 2        /* the devkit's scale, 7dof and scale_7dof: named so that they can be refused */
#define CFEAR_EVAL_ALIGN_7DOF 3
#define CFEAR_EVAL_ALIGN_SCALE_7DOF 4
typedef struct cfear_eval_params {
  int32_t step_size;                    /* 10 (eval_odom.py); >= 1                                                   */
  int32_t alignment;                    /* CFEAR_EVAL_ALIGN_NONE or _6DOF; anything else: CFEAR_ERR_INVALID_ARGUMENT */
  double lengths[CFEAR_EVAL_NUM_LENGTHS];   /* 100 ... 800 m (:90); positive and strictly ascending                  */
} cfear_eval_params;                    /* 72 bytes */
void cfear_eval_params_default(cfear_eval_params* p);
typedef struct cfear_eval_summary {
  double ave_t_err, ave_r_err;          /* means of t_err / len and r_err / len over all rows; 0 without rows (:264-287) */
  double ate;                           /* compute_ATE (:477-505): RMS position difference after the alignment       */
  double rpe_trans, rpe_trans_dev;      /* compute_RPE (:508-583) over consecutive frames: mean and population       */
  double rpe_rot, rpe_rot_dev;          /*   standard deviation of the translation and of the rotation error         */
  double bias_x, bias_y;                /* means of the relative error's x and y                                     */
  double bias_theta;                    /* mean of rot2eul(...)[0] as the devkit writes it (:14-18, :550-551): the angle
                                           about x, 0 for planar trajectories                                        */
  double rmse_trans;                    /* sqrt of the mean squared relative translation error                       */
  double seg_t_err[CFEAR_EVAL_NUM_LENGTHS], seg_r_err[CFEAR_EVAL_NUM_LENGTHS];   /* compute_segment_error (:442-475); 0 where seg_count is 0 */
  double align[12];                     /* the [r | t] the estimate was left-multiplied by (identity for `none`)     */
  int64_t n_rows;
  int32_t seg_count[CFEAR_EVAL_NUM_LENGTHS];
  int32_t n_poses;
  int32_t status;                       /* CFEAR_OK; CFEAR_ERR_SOLVER: a figure is not finite (a singular pose), or the
                                           6dof alignment is undetermined (all positions on one line; identity rotation used) */
} cfear_eval_summary;                   /* 360 bytes */
typedef struct cfear_eval_row {         /* one line of errors/NN.txt (:248), plus the pair and last_frame            */
  int32_t trajectory, first_frame, last_frame, pad;
  double length, r_err, t_err, speed;   /* r_err and t_err are already divided by the length; speed = len / (0.1 frames) */
} cfear_eval_row;                       /* 48 bytes */
/* est, gt: [..][12] doubles, the rows of the 3 x 4 pose as a KITTI line holds them; both host or both device, 16-byte
 * aligned.  Pair t is poses offsets[t] .. offsets[t] + lengths[t] - 1 of both arrays (offsets NULL: the pairs follow each
 * other); offsets and lengths are host arrays.  summaries [n_traj] and rows [row_cap] (optional; ordered by pair, start
 * frame, length) are host or device; *n_rows (optional, host) receives the number of rows of the batch.  With more rows
 * than row_cap the table holds the first row_cap and the call returns CFEAR_ERR_CAPACITY after completing the summaries.
 * Refused with CFEAR_ERR_INVALID_ARGUMENT, because the devkit does not define them: a pair with fewer than 2 poses,
 * step_size < 1, an alignment other than none / 6dof.  The call synchronises once (the 3 x 3 SVDs are host code).      */
int cfear_eval_trajectories(cfear_ctx* ctx, const double* est, const double* gt, const int64_t* offsets, const int32_t* lengths,
                            int32_t n_traj, const cfear_eval_params* par, cfear_eval_summary* summaries, cfear_eval_row* rows,
                            int64_t row_cap, int64_t* n_rows);
/* The refusals of cfear_eval_trajectories as host code, for callers that hold the two trajectories of a pair separately:
 * also refuses a pair whose estimate and ground truth differ in length (the devkit normalises only the estimate's keys). */
int cfear_eval_check(const cfear_eval_params* par, const int32_t* est_lengths, const int32_t* gt_lengths, int32_t n_traj);
/* Host helpers, no context.  cfear_kitti_read: load_poses_from_txt (:93-121), lines of 12 numbers or of 13 with the frame
 * index first (which must count 0, 1, 2, ...: CFEAR_ERR_FORMAT otherwise, as for any other line).  *n_out = poses in the
 * file; poses [cap][12] may be NULL with cap 0 to ask for the count; CFEAR_ERR_CAPACITY if the file holds more than cap.
 * cfear_kitti_write: EvalTrajectory::Write (cfear_radarodometry/src/cfear_radarodometry/eval_trajectory.cpp:169-183),
 * std::fixed with 6 decimals.  cfear_kitti_from_xyt: planar (x, y, theta) to [cos -sin 0 x; sin cos 0 y; 0 0 1 0];
 * stride = doubles between poses (3 for packed triples, 7 for the pose of consecutive cfear_frame_info records).      */
int cfear_kitti_read(const char* path, double* poses, int64_t cap, int64_t* n_out);
int cfear_kitti_write(const char* path, const double* poses, int64_t n);
int cfear_kitti_from_xyt(const double* xyt, int64_t n, int64_t stride, double* poses);

/* ---- after the path: synchronising estimate and ground truth by time -------------------------------------------------
 * What EvalTrajectory::Save() does before it writes anything (cfear_radarodometry/src/cfear_radarodometry/
 * eval_trajectory.cpp:265-315, cited as :line): One2OneCorrespondance (:400-423) interpolates the ground truth at the stamp
 * of every estimated pose and drops the estimates that no two ground-truth poses bracket -- the step that turns a 4 Hz
 * estimate and a 50 or 100 Hz ground truth into the equally long pair cfear_eval_trajectories and cfear_loop_stats_batch
 * take.  For a batch of pairs in one call (csrc/trajsync.hip), the reference's semantics quirk for
 * quirk:
 *   time          ros::Time::toSec(), (double)sec + 1e-9 * (double)nsec with sec = ns / 10^9 (roscpp's TimeBase::toSec,
 *                 restated: roscpp is not part of the reference tree).  ALL comparisons are on these doubles, which
 *                 resolve about 2.4e-7 s around 1.5e9 s: distinct stamps can compare equal.
 *   SearchByTime  (:424-442) a ground truth of 2 poses or fewer finds nothing (`<= 2`).  Otherwise j walks from the carried
 *                 position to n_gt - 2 and the first j with t[j] <= ts && ts <= t[j+1] wins.  A hit leaves the position at
 *                 j; a miss leaves it at the end and One2OneCorrespondance resets it to 0 (:412).  So the estimate stamps
 *                 may be in any order: one that steps back misses, and the next is searched from 0.
 *   pose_interp   (:461-491) alpha = (t - t1) / (t2 - t1), 0 when t2 == t1; translation (1 - alpha) p1 + alpha p2 with z
 *                 then set to 0; rotation Quaterniond(R1).slerp(alpha, Quaterniond(R2)).toRotationMatrix(), restated from
 *                 Eigen 3.3: the matrix -> quaternion conversion branches on the trace and otherwise picks the pivot by
 *                 m11 > m00, then m22 > m(i,i), without normalising; slerp is linear where |dot| >= 1 - DBL_EPSILON, else
 *                 acos / sin weights, the second negated for a negative dot; toRotationMatrix in its tx = 2x form.  No
 *                 product is fused.
 * CFEAR_SYNC_CHAINED carries the search position from one estimate of a pair to the next (One2OneCorrespondance);
 * CFEAR_SYNC_INDEPENDENT searches every stamp from the first ground-truth pose (Interpolate(t, out), eval_trajectory.h:
 * 141-144; tbv_slam_online.cpp:200-204).  They differ where a stamp lies in more than one interval.
 *
 * est, gt: [..][12] doubles, KITTI rows; stamps: nanoseconds (ros::Time::toNSec()).  Pair t is est_lengths[t] estimates from
 * est_offsets[t] and gt_lengths[t] ground-truth poses from gt_offsets[t] (an offsets array may be NULL: the pairs follow each
 * other).  Offsets, lengths and counts are host arrays; est, est_stamps, gt, gt_stamps and the four outputs are all host
 * or all device memory (device poses 16-byte aligned) and the outputs do not overlap the inputs.  Pair t writes its
 * counts[t] kept rows, compacted and in estimate order, at est_offsets[t] of every output -- so est_out, gt_out,
 * est_offsets and counts are arguments of cfear_eval_trajectories as they are; what lies behind a pair's kept rows is not
 * written.  Kept estimate poses are copied bit for bit, stamps_out holds the estimate's stamp, rows[i] names the estimate
 * (its index within the pair: gather whatever else is kept per estimate, such as the covariances of cfear_cov_write), the
 * interval and alpha.  est may be NULL (labelling stamps without poses); est_out is then unused.  A pair with no
 * estimates or no ground truth is legal and keeps nothing.
 * Refused with CFEAR_ERR_INVALID_ARGUMENT before anything is written, cfear_last_error naming the pair and the index:
 * null pointers, n_traj < 0, a negative length or offset, host and device buffers mixed, an unknown mode, a stamp that is
 * negative or whose seconds exceed 2^32 - 1 (ros::Time::sec is a uint32), and ground-truth stamps that descend within a
 * pair.  The reference would walk an unsorted ground truth serially; a bag's ground-truth topic is recorded in time
 * order and the parallel search needs that order, so an unsorted one is refused, not ignored.  Host buffers are checked
 * before a context is needed (ctx may then be NULL: the refusal is the same, its text is at cfear_last_error(NULL)),
 * device buffers by a kernel of their own, whose verdict is read together with counts: the call synchronises once.   */
#define CFEAR_SYNC_CHAINED 0
#define CFEAR_SYNC_INDEPENDENT 1
typedef struct cfear_sync_row {
  int32_t est_index, gt_index;          /* the estimate within its pair; the interval [gt_index, gt_index + 1] within its pair */
  double alpha;
} cfear_sync_row;                       /* 16 bytes */
int cfear_sync_trajectories(cfear_ctx* ctx, int32_t mode, const double* est, const int64_t* est_stamps, const int64_t* est_offsets,
                            const int32_t* est_lengths, const double* gt, const int64_t* gt_stamps, const int64_t* gt_offsets,
                            const int32_t* gt_lengths, int32_t n_traj, double* est_out, double* gt_out, int64_t* stamps_out,
                            cfear_sync_row* rows, int32_t* counts);
/* Host writers, no context (Save()'s directory and file naming, DatasetToSequence, stays with the caller).
 * cfear_tum_write: EvalTrajectory::WriteTUM (:185-211): per pose `sec.` + nsec zero-padded to 9 digits + a space, the
 * translation std::fixed with 4 decimals, the quaternion x y z w under std::defaultfloat with the precision still 4
 * (%.4g), from the matrix -> quaternion conversion above.  cfear_cov_write: EvalTrajectory::WriteCov (:214-232): the stamp,
 * then the 36 entries of cov [n][36] row-major, space-separated, %g at the stream's default precision of 6
 * (Eigen::StreamPrecision with DontAlignCols).  A stamp outside ros::Time's range: CFEAR_ERR_INVALID_ARGUMENT.          */
int cfear_tum_write(const char* path, const double* poses, const int64_t* stamps, int64_t n);
int cfear_cov_write(const char* path, const double* cov, const int64_t* stamps, int64_t n);

/* ---- after the path: training the classifiers (alignment_checker's LogisticRegression::fit) --------------------------
 * What the reference asks of sklearn.linear_model.LogisticRegression(class_weight="balanced", max_iter=1000) through
 * pybind11 (coral_alignment_quality/src/alignment_checker/alignmentinterface.cpp:192-222), for a batch of models in one
 * launch, one workgroup each (csrc/logreg.hip).  Per model, over (w in R^d, b):
 *     F = 1/2 w.w + C sum_i s_i [log(1 + exp(z_i)) - y_i z_i],  z_i = w.x_i + b,  y_i in {0, 1},
 *     s_i = n / (2 n_class(i)) with class_weight_balanced, else 1; the intercept is not penalised.
 * With both classes present F is strictly convex; the kernel minimises it in fp64 by a damped Newton iteration (LDL^T
 * of the Jacobi-scaled Hessian, Armijo backtracking) and stops when the Newton decrement is at most 1e-16 max(1, |F|)
 * or no trial step decreases F.  It is a second-order solve, so it lands on the minimiser where sklearn's L-BFGS may
 * stop short on unscaled features (EXPERIMENTS.md, "Fitting the classifiers").  Every sum has a fixed order: a
 * model's record is bit-identical at any batch position and whether its buffers were host or device memory.            */
#define CFEAR_LOGREG_MAX_FEATURES 8
typedef struct cfear_logreg_params {
  double C;                             /* 1.0: inverse regularisation strength, > 0                                 */
  int32_t class_weight_balanced;        /* 1                                                                         */
  int32_t fit_intercept;                /* 1                                                                         */
  int32_t max_iterations;               /* 100 Newton steps (the reference's 1000 bounds L-BFGS steps)               */
  int32_t pad;
} cfear_logreg_params;                  /* 24 bytes */
void cfear_logreg_params_default(cfear_logreg_params* p);
typedef struct cfear_logreg_job {
  const double* X;                      /* [n_rows][row_stride], host or device                                      */
  const double* y;                      /* [n_rows], host or device                                                  */
  const int32_t* columns;               /* host: n_features indices into a row, or NULL = 0 .. n_features - 1        */
  const uint8_t* row_mask;              /* [n_rows], host or device: 0 = the row is left out; or NULL                */
  int64_t n_rows;
  int32_t row_stride, n_features;       /* doubles between rows; 1 .. CFEAR_LOGREG_MAX_FEATURES                      */
} cfear_logreg_job;                     /* 48 bytes */
typedef struct cfear_logreg_result {
  double intercept, coef[CFEAR_LOGREG_MAX_FEATURES];   /* coef[n_features ..] = 0                                    */
  double objective, grad_inf;           /* F and the largest absolute entry of its gradient at the result            */
  double balanced_accuracy;             /* sklearn's balanced_accuracy_score of predict() on the used rows (:69-80)  */
  int64_t n_used, n_pos;                /* rows the mask leaves; of those, rows with y = 1                           */
  int64_t confusion[4];                 /* tn, fp, fn, tp at z > 0: confusion_matrix row-major (:83-94)              */
  int32_t iterations;                   /* Newton steps taken                                                        */
  int32_t status;                       /* CFEAR_OK; CFEAR_ERR_INVALID_ARGUMENT; CFEAR_ERR_SOLVER                    */
} cfear_logreg_result;                  /* 152 bytes */
/* Jobs that name the same X, y or row_mask pointer share one upload (at the longest extent any of them names), so the
 * CorAl, CFEAR and combined models of one table, or the folds of a cross-validation, cost one copy.  results [n_jobs] is
 * host memory; the call returns when it is written.  A job's own trouble is its status and leaves the call and the other
 * jobs alone: CFEAR_ERR_INVALID_ARGUMENT for no used rows, one class only (sklearn raises), a label that is not 0 or 1,
 * a used value that is not finite (the reference's DataValid exits the process); CFEAR_ERR_SOLVER when max_iterations
 * steps did not converge or an iterate is not finite -- the record then holds the last iterate.  The whole call is
 * refused with CFEAR_ERR_INVALID_ARGUMENT, before anything is launched, for n_jobs < 0, null pointers, n_features outside
 * 1 .. 8, a negative column index, or a row_stride smaller than n_features or than max(columns) + 1; n_jobs = 0 is OK.  */
int cfear_logreg_fit_batch(cfear_ctx* ctx, const cfear_logreg_job* jobs, int32_t n_jobs, const cfear_logreg_params* par,
                           cfear_logreg_result* results);

/* ---- after the path: loop candidates without descriptors (GTVicinityClosure, MiniClosure) ----------------------------
 * The two candidate generators of the reference's loop-closure thread that read only poses and odometry:
 * GTVicinityClosure::SearchAndAddConstraint (tbv_slam/src/tbv_slam/loopclosure.cpp:394-467), which finds the pairs the
 * loop classifiers are trained and evaluated on, and MiniClosure::SearchAndAddConstraint (:469-552, --miniloop-enabled).
 * For each origin node i of each graph, over the later nodes j = i + 1 .. n - 1, in fp64 (csrc/closure.hip):
 *     trav = trav + step[j - 1]                        trav starts at 0.0 for every origin: the reference's serial sum
 *     eucl = sqrt((dx * dx + dy * dy) + dz * dz)       p_i - p_j
 *     GTVicinity:  if eucl <= max_d_close and min_d_travel <= trav and trav <= max_d_travel:
 *                      rel = eucl / trav;  if rel < best: best = rel, to = j
 *     MiniClosure: if trav < min_d_travel: continue
 *                  if trav > max_d_travel: exhausted = 1; break
 *                  if eucl <= max_d_close: rel = eucl / trav;  if rel < best: best = rel, to = j
 * best starts at DBL_MAX, so the first j wins a tie and an infinite or NaN rel (eucl / 0 with min_d_travel = 0) never
 * wins.  This is the reference's FIRST SearchAndAddConstraint() call from fresh state on a complete graph (nothing
 * attempted yet, itr_current = begin); continuing a streaming closure thread is the caller's business, and `exhausted`
 * (origin_attempted_ would be set) is what it needs for that.  Every emitted pair also gets loopclosure::VerifyByOdometry
 * (:776-806) in the arithmetic of cfear_verify_by_odometry.                                                             */
#define CFEAR_CLOSURE_GTVICINITY 0
#define CFEAR_CLOSURE_MINI 1
#define CFEAR_CLOSURE_ORIGINS 64        /* origins (lanes) per workgroup of the sweep                                 */
#define CFEAR_CLOSURE_TILE 256          /* later nodes staged per LDS tile; both exported so that tests can straddle them */
typedef struct cfear_closure_params {
  int32_t mode;                         /* CFEAR_CLOSURE_GTVICINITY or CFEAR_CLOSURE_MINI                             */
  int32_t verify_via_odometry;          /* 1 (loopclosure.h:122); 0: odom_bounds of every pair is 1                  */
  double min_d_travel, max_d_travel, max_d_close;   /* 40, 4200, 15 (loopclosure.h:84-86) / 25, 500, 15 (:95-97)     */
  double odom_sigma_error;              /* 0.03 (:123)                                                               */
} cfear_closure_params;                 /* 40 bytes */
void cfear_closure_params_default(cfear_closure_params* p, int32_t mode);
typedef struct cfear_closure_candidate {   /* one per origin node */
  int32_t to;                           /* index within the graph of the chosen later node, -1 = none                */
  int32_t exhausted;                    /* MiniClosure: origin_attempted_ would be set; 0 in GTVicinity mode         */
  double eucl, trav, rel;               /* of the winner; 0 when to == -1                                            */
  double odom_bounds;                   /* VerifyByOdometry(from = to-node, to = origin); 0 when to == -1 or rel_xyt == NULL */
} cfear_closure_candidate;              /* 40 bytes */
/* n_graphs graphs in one call.  Graph g owns nodes [node_offsets[g], node_offsets[g + 1]) of the flat arrays; node_offsets
 * holds n_graphs + 1 entries, starts at 0 and ends at n_nodes.  positions [n_nodes][3], steps [n_nodes], rel_xyt
 * [n_nodes][3] (optional) and out [n_nodes] all hold ONE ENTRY PER NODE, so the one offset table serves them all:
 * steps[k] is the norm of t_be.p of the odometry constraint from flat node k to k + 1 as the caller computed it (its
 * rounding holds), rel_xyt[k] is ConstraintsHandler::RelativeMotion of the same two nodes as a planar (x, y, theta); the
 * entry of each graph's LAST node is ignored in both.  out[k].to counts within the graph.  Graphs of 0 or 1 nodes are
 * legal and emit nothing.  All arrays are host memory; the call returns when out is written.  A graph's records are
 * bit-identical whatever else the batch holds and wherever the graph sits in it.  Refused with
 * CFEAR_ERR_INVALID_ARGUMENT before anything is launched or written, *failed_graph (optional; -1 otherwise) and
 * cfear_last_error naming the graph: offsets that do not start at 0 (graph 0), do not end at n_nodes (the last graph) or
 * decrease; a used step that is negative or not finite; a position that is not finite.  Also refused, with
 * *failed_graph = -1: an unknown mode, a threshold that is NaN, null or device pointers.                              */
int cfear_closure_candidates_batch(cfear_ctx* ctx, const double* positions, const double* steps, const double* rel_xyt,
                                   const int64_t* node_offsets, int64_t n_nodes, int32_t n_graphs, const cfear_closure_params* par,
                                   cfear_closure_candidate* out, int32_t* failed_graph);

/* ---- after the path: scoring the loop detector (loop rows, ROC and precision-recall curves) ---------------------------
 * cfear_loop_stats_batch restates, for a batch of graphs and all their candidates in one launch (csrc/loopeval.hip),
 *   PoseGraph::UpdateStatistics (tbv_slam/src/tbv_slam/posegraph.cpp:332-371): the ground-truth-labelled row of a candidate,
 *   EvaluationManager::getCandidateLoopStatus (place_recognition_radar/src/place_recognition_radar/EvaluationManager.cpp:12-27).
 * Poses are planar (x, y, theta).  Per candidate, in fp64, whatever has_gt says (the reference computes Terror before it
 * asks has_Tgt_), with (c, s) the cosine and sine of an angle and d = p_to - p_from:
 *     Tgt_diff = Tfrom^-1 Tto:   cgd = cf ct + sf st,  sgd = cf st - sf ct,  xgd = cf dx + sf dy,  ygd = cf dy - sf dx
 *     diff = Tguess^-1 Tgt_diff: cd = cg cgd + sg sgd, sd = cg sgd - sg cgd,  ex = xgd - xg,  ey = ygd - yg,
 *                                diff.x = cg ex + sg ey,  diff.y = cg ey - sg ex,  diff.z = atan2(sd, cd)
 * diff.z is what Eigen's rotation().eulerAngles(0, 1, 2)[2] returns for a rotation about z: there the first two angles are
 * atan2(0, 1) = 0 and the third is atan2(R10, R00), the matrix entries themselves.
 * Only when has_gt[from]: candidate_loop_distance = sqrt((dx dx + dy dy) + 0.0) if has_gt[to] (else -1), and the search over
 * the nodes k < from of the same graph with from - k > min_index_gap and has_gt[k] for the smallest
 * d = sqrt((dx dx + dy dy) + 0.0); the strict `<` keeps the lowest k among equal distances.  It starts from
 * no_loop_distance with id_close = from and close_xy = p_from, which is also what a `from` without ground truth reports.
 * Flags: is_loop = closest_loop_distance < max_distance; transl_error = sqrt(diff.x^2 + diff.y^2);
 * rot_error = (180 / pi) |diff.z|; candidate_close = transl_error < max_registration_translation and rot_error <
 * max_registration_rotation_deg; prediction_pos_ok = !is_loop or candidate_close.                                       */
typedef struct cfear_loop_stats_params {
  double max_distance;                  /* 6     (EvaluationManager.cpp:14)                                            */
  double max_registration_translation;  /* 4     (:15)                                                                 */
  double max_registration_rotation_deg; /* 2.5   (:16)                                                                 */
  double no_loop_distance;              /* 100000 (posegraph.cpp:334)                                                  */
  int32_t min_index_gap;                /* 10    (posegraph.cpp:358)                                                   */
  int32_t pad;
} cfear_loop_stats_params;              /* 40 bytes */
void cfear_loop_stats_params_default(cfear_loop_stats_params* p);
typedef struct cfear_loop_candidate {
  int32_t graph;                        /* index into node_offsets                                                     */
  int32_t from, to;                     /* node indices within the graph                                               */
  int32_t guess_nr;                     /* >= 0                                                                        */
  double guess_xyt[3];                  /* Tguess: the candidate's estimate of Tfrom^-1 Tto                            */
} cfear_loop_candidate;                 /* 40 bytes */
typedef struct cfear_loop_row {
  double diff[3];                       /* Terror (x, y, theta): loop.csv's diff.x, diff.y, diff.z                     */
  double closest_loop_distance, candidate_loop_distance;
  double transl_error, rot_error;       /* getCandidateLoopStatus's two errors (metres, degrees)                       */
  double close_xy[2];                   /* position of node id_close                                                   */
  int32_t id_close;                     /* within the graph; = from when nothing was found                             */
  int32_t is_loop, candidate_close, prediction_pos_ok;
} cfear_loop_row;                       /* 88 bytes */
/* Graph g owns nodes [node_offsets[g], node_offsets[g + 1]) of gt_xyt [n_nodes][3] and has_gt [n_nodes]; node_offsets
 * (host, n_graphs + 1 entries) starts at 0 and ends at n_nodes.  gt_xyt, has_gt, candidates [n_cand] and rows [n_cand] are
 * all host or all device memory.  One wavefront serves a candidate; a row is bit-identical wherever its graph and its
 * candidate sit in the batch and whichever memory the buffers were.  A graph of 0 nodes is legal, n_cand = 0 is OK.  The
 * whole call is refused with CFEAR_ERR_INVALID_ARGUMENT before anything is written, cfear_last_error naming the culprit and
 * *failed_candidate (optional, -1 otherwise) its index: a candidate whose graph, from or to does not exist, whose guess
 * or whose from / to pose is not finite, or whose guess_nr is negative.  Also refused, with *failed_candidate = -1: offsets
 * that do not run from 0 to n_nodes without descending, a node with has_gt whose pose is not finite, a parameter that is
 * NaN, min_index_gap < 0, null pointers, host and device buffers mixed.  For host buffers every check is made before a
 * context is needed; device buffers are checked by a kernel of their own, before the rows are computed.                 */
int cfear_loop_stats_batch(cfear_ctx* ctx, const int64_t* node_offsets, const double* gt_xyt, const uint8_t* has_gt, int64_t n_nodes,
                           int32_t n_graphs, const cfear_loop_candidate* candidates, int64_t n_cand, const cfear_loop_stats_params* par,
                           cfear_loop_row* rows, int64_t* failed_candidate);

/* ---- loop candidates of batched graphs, verified from the detector's rows ------------------------------------------------
 * The body of ScanContextClosure::SearchAndAddConstraint (tbv_slam/src/tbv_slam/loopclosure.cpp:653-724) for a batch of
 * complete graphs, as one device stage between cfear_sc_detect_batch (or any candidate proposer) and the pose-graph solve:
 * the row -> (from, to, guess_nr) mapping, the `speedup` rule (:682-688), Tsrcguess = Taug^-1 * Rz(yaw) under transl_guess
 * (:692-696), VerifyByOdometry (:776-806) and the verification chain of cfear_verify_loop_candidates, without the host
 * seeing a candidate.  csrc/verify.hip; DESIGN.md has the data flow.
 * The graphs lie one behind the other as in cfear_sc_batch: graph g owns nodes [node_off[g], node_off[g + 1]).          */
typedef struct cfear_loop_graphs {
  int32_t n_graphs, pad;
  const int32_t* node_off;              /* [n_graphs + 1] host, from 0 to n_nodes                                         */
  const cfear_scan_table* table;        /* n_nodes entries: entry k = node k's cloud_normal_ (a scan may be named twice)  */
  const float* peaks_xyzi;              /* [peak_off[n_nodes]][4] cloud_peaks_ of all nodes, host (staged with one copy)
                                           or device: the point buffer cfear_sc_batch takes in cloud mode                */
  const int64_t* peak_off;              /* [n_nodes + 1] host                                                             */
  const double* poses_xyt;              /* [n_nodes][3] host: GetPose()                                                   */
  const double* rel_xyt;                /* [n_nodes][3] host: RelativeMotion(k, k + 1), the entry of a graph's last node
                                           ignored; NULL only with verify_via_odometry = 0                               */
} cfear_loop_graphs;                    /* 56 bytes */
typedef struct cfear_loop_verify_candidate {
  int32_t graph;                        /* index into node_off                                                            */
  int32_t from, to;                     /* within the graph, to < from                                                    */
  int32_t guess_nr;                     /* >= 0                                                                           */
  int32_t query;                        /* candidates of one query share it (ApplyConstratins runs per query); the rows
                                           form writes the flat node index of `from`                                     */
  int32_t skip;                         /* 1: not registered (the speedup rule)                                           */
  double guess_xyt[3];                  /* constraint.t_be on entry                                                       */
  double sc_sim;                        /* quality["sc-sim"]                                                              */
  double odom_term;                     /* what a skipped candidate reports as odom_bounds (min_dist_odom); else unused   */
} cfear_loop_verify_candidate;          /* 64 bytes */
typedef struct cfear_loop_verify_params {
  cfear_verify_params verify;           /* use_covariance_sampling is refused here                                        */
  double odom_sigma_error;              /* 0.03 (loopclosure.h:123)                                                       */
  int32_t verify_via_odometry;          /* 1 (:122); 0: odom_bounds of every candidate is exactly 1                       */
  int32_t transl_guess;                 /* 1 (:126); 0: the guess is (0, 0, yaw)                                          */
  int32_t speedup;                      /* 0 (:127); the shipped TBV-8 parameter files set it                             */
  int32_t odometry_coupled_closure;     /* 1: the detector's setting; the speedup rule needs both                         */
} cfear_loop_verify_params;             /* 184 bytes */
void cfear_loop_verify_params_default(cfear_loop_verify_params* p);
#define CFEAR_LOOP_SPEEDUP_ODOM 0.7     /* min_dist_odom above which `speedup` skips a row (loopclosure.cpp:683)          */
/* cands [n_cand], host or device.  Candidate j is verified as cfear_verify_loop_candidates verifies the job {table[from],
 * table[to], the two nodes' peaks, poses_xyt[from], guess_xyt, sc_sim, odom_bounds, group = query} with
 * odom_bounds = VerifyByOdometry(from, to) over rel_xyt[to .. from - 1] of its graph, computed on the device in the order of
 * cfear_verify_by_odometry (its sin / cos / exp are the device's: the last place may differ from the host's libm).
 * A candidate with skip set is not registered: reg_ok = 0, identity t_be and cov, zero coral / cfear / reg,
 * alignment_quality = -20, odom_bounds = odom_term, sc_sim as given, probability = 0, accepted = 0, rank = -1, and it takes
 * no part in ApplyConstratins.
 * results [n_cand]: host (ApplyConstratins applied per query) or device (accepted = rank = 0, the selection is the
 * caller's).  list_out [n_cand] (optional, host or device): the list as verified.  loops_out [n_cand] (optional, in the
 * memory of results): {graph, from, to, guess_nr, guess_xyt = the result's t_be}, what cfear_loop_stats_batch takes.
 * Refused before anything is launched or written, the message naming "graph g, node k" or "candidate j": node_off or
 * peak_off that do not start at 0 or descend, a table whose size is not n_nodes, a candidate whose graph, from or to does
 * not exist or with to >= from or a negative guess_nr, poses, guesses, sc_sim or used rel_xyt entries that are not finite,
 * null arrays with positive counts, use_covariance_sampling.  With host inputs every check is made before the context is
 * looked at and a null ctx is refused last.  A device list is checked by the kernel that reads it: the first bad candidate
 * is named and nothing is written to the outputs.  A candidate whose two peak clouds together exceed what one CorAl job takes
 * (16384 points) fails the call with CFEAR_ERR_CAPACITY naming it, the outputs untouched.  n_graphs = 0 or n_cand = 0: CFEAR_OK, the device
 * untouched.                                                                                                            */
int cfear_verify_graph_candidates(cfear_ctx* ctx, const cfear_loop_graphs* graphs, const cfear_loop_verify_candidate* cands,
                                  int32_t n_cand, const cfear_loop_verify_params* par, cfear_verify_result* results,
                                  cfear_loop_verify_candidate* list_out, cfear_loop_candidate* loops_out);
/* The same from Scan Context rows exactly as cfear_sc_detect_batch leaves them: rows [D][n_candidates] and n_out [D], both
 * host or both device, D = sum n_detect; n_detect [n_graphs] host (NULL: every node).  Row d of graph g is the query
 * from = d - (first row of g), its record s < n_out[d] the candidate {to = nn_idx, guess_nr = s}; records past n_out[d]
 * are ignored.  The candidates are compacted in (row, guess_nr) order; per candidate, on the device:
 *   guess  = Taug^-1 * (0, 0, (double)yaw_diff_rad) with transl_guess, else (0, 0, yaw)
 *   sc_sim = (double)(float)min_dist (:677)
 *   skip   = speedup and odometry_coupled_closure and min_dist_odom > 0.7, then sc_sim = min_dist unnarrowed and
 *            odom_term = min_dist_odom (:684)
 * results, list_out, loops_out hold D * n_candidates records each, of which the first *n_list are written.  Also refused:
 * n_detect[g] outside [0, nodes of g], rows and n_out in different memories, n_candidates < 1; host rows are checked on
 * the host (n_out outside [0, n_candidates] is a bad row), device rows by the kernel.                                    */
int cfear_verify_sc_rows(cfear_ctx* ctx, const cfear_loop_graphs* graphs, const cfear_sc_candidate* rows, const int32_t* n_out,
                         const int32_t* n_detect, int32_t n_candidates, const cfear_loop_verify_params* par,
                         cfear_verify_result* results, cfear_loop_verify_candidate* list_out, cfear_loop_candidate* loops_out,
                         int32_t* n_list);
/* Sampled covariances (use_covariance_sampling_in_loop_closure; loopclosure.cpp:62-71, 99-208) for candidates the two calls
 * above verified, as a pass of its own: list [n_list] and results [n_list] are their list_out and results, both in host
 * memory or both in device memory.  For every candidate with skip == 0 and results[j].reg_ok == 1: par->verify.sampling's
 * n^3 GetCost samples around results[j].reg.pose with scans {to, from} of its graph and the target fixed at
 * poses_xyt[from] * guess_xyt (P2L, Huber 0.1, uniform weights, the radius of reg.outer_iters), the fit of
 * cfear_cov_fit_records, and -- where the fit is accepted -- the x-y-z block rotated by the inverse of the registered yaw into
 * `cov`, with cov_sampled = 1.  A refused fit leaves the record as it is (Register's constant, rotated; cov_sampled = 0).  No
 * other byte of any record changes; skipped and failed candidates are left as they are.  par->verify.use_covariance_sampling
 * is not read, the graphs' peaks and rel_xyt neither.  Nothing crosses to the host between the samples and the covariance;
 * the call reads one 16-byte header back before the samples (how many candidates take part, and the verdict on the list).
 * Refused with nothing written, the message naming "graph g, node k" or "candidate j": node_off that does not start at 0 or
 * descends, poses that are not finite, a table whose size is not n_nodes, samples_per_axis outside [1, 15], list and results
 * in different memories, a candidate cfear_verify_graph_candidates would refuse, a registered pose that is not finite.  A
 * device list is checked by the kernel that reads it.  n_graphs = 0 or n_list = 0: CFEAR_OK, the device untouched.       */
int cfear_verify_sample_covariances(cfear_ctx* ctx, const cfear_loop_graphs* graphs, const cfear_loop_verify_candidate* list,
                                    int32_t n_list, const cfear_loop_verify_params* par, cfear_verify_result* results);

/* cfear_loop_curves_batch: what place_recognition_radar/python/LoopClosureEval.py and evaluation/3_loop_closure/
 * 3_loop_closure.py ask of sklearn for a table of (label, score) rows -- metrics.roc_curve, metrics.auc,
 * precision_recall_curve, and ComputeClassifierStatistics at a probability threshold -- for a batch of experiments in one
 * call, one workgroup each.  Per experiment, with integer counts until the final divisions:
 *   sort by score, descending (-0.0 reads as 0.0); idx = the last position of every run of equal scores;
 *   tps = cumsum(y)[idx], fps = 1 + idx - tps, thr = score[idx]              (n_thresholds entries)
 *   ROC: with more than two thresholds and drop_intermediate, keep the first, the last and every i whose second difference
 *        of fps or of tps is not 0; prepend (0, 0, +inf); fpr = fps / fps[last], tpr = tps / tps[last]     (n_roc entries)
 *   PR:  precision = tps / (tps + fps) (0 where that is 0 / 0), recall = tps / tps[last], both reversed, then 1 and 0
 *        appended (n_pr = n_thresholds + 1 entries); pr_thr = thr reversed (n_pr - 1 entries)
 *   reference_endpoints: tpr[last] = tpr[last - 1], recall[0] = recall[1], precision[0] = precision[1], as 3_loop_closure.py:
 *        157,164-165 does before it integrates and plots
 *   auc = sum_i (fpr[i + 1] - fpr[i]) (tpr[i + 1] + tpr[i]) / 2 over the arrays as returned, in a fixed order
 *   at the threshold: pred = score >= p_threshold; a label is read as 0 where y = 1, pred = 1 and pos_ok = 0
 *        (CorrectLabelForPosition, on a copy: the curves use y as given); confusion = {tn, fp, fn, tp}, accuracy,
 *        precision = tp / (tp + fp), recall = tp / (tp + fn), 0 where a denominator is 0.
 * An order-preserving 64-bit key is made of every score and sorted with the row's label beside it (the non-NaN doubles
 * need more than 63 bits, so the label cannot ride inside the key).  Experiments of up to CFEAR_LOOPEVAL_LDS_ROWS rows are
 * sorted in LDS (profile row "loop_curves_lds"); larger ones in global memory by the same workgroup, chunks of
 * CFEAR_LOOPEVAL_LDS_ROWS sorted and merged through LDS (profile row "loop_curves_global").                              */
#define CFEAR_LOOPEVAL_LDS_ROWS 16384
typedef struct cfear_loop_curves_params {
  double p_threshold;                   /* 0.9 (LoopClosureEval.py --p-threshold)                                      */
  int32_t drop_intermediate;            /* 1: roc_curve's default                                                      */
  int32_t reference_endpoints;          /* 1: the curves as the reference's scripts plot them; 0: as sklearn returns them */
} cfear_loop_curves_params;             /* 16 bytes */
void cfear_loop_curves_params_default(cfear_loop_curves_params* p);
typedef struct cfear_loop_curves_result {
  double auc;
  double accuracy, precision, recall;   /* at p_threshold, of the position-corrected labels                            */
  int64_t n_pos, n_neg;                 /* rows with y = 1 / y = 0                                                     */
  int64_t confusion[4];                 /* tn, fp, fn, tp at p_threshold                                               */
  int32_t n_thresholds, n_roc, n_pr;    /* distinct scores; entries of the roc_* arrays; of pr_precision and pr_recall */
  int32_t status;                       /* CFEAR_OK or CFEAR_ERR_INVALID_ARGUMENT                                      */
} cfear_loop_curves_result;             /* 96 bytes */
/* Experiment e owns rows [row_offsets[e], row_offsets[e + 1]) of y [n_rows] (0 or 1), score [n_rows] and pos_ok [n_rows]
 * (optional: NULL reads as all 1); row_offsets (host, n_exp + 1 entries) runs from 0 to n_rows.  y, score, pos_ok and the six
 * curve arrays are all host or all device memory.  Each curve array holds n_rows + n_exp doubles and experiment e's
 * entries start at row_offsets[e] + e: n_roc of roc_fpr, roc_tpr and roc_thr, n_pr of pr_precision and pr_recall, n_pr - 1
 * of pr_thr; entries beyond those are not written.  results [n_exp] is host memory; the call returns when it is written.
 * An experiment's own trouble is its status and leaves the others alone: CFEAR_ERR_INVALID_ARGUMENT for no rows, one class
 * only (sklearn yields NaN), a label other than 0 or 1, or a NaN score; its counts are then 0 and none of its curve
 * entries is written.  An experiment's arrays and record are bit-identical wherever it sits in the batch and whichever
 * memory the buffers were.  The whole call is refused with CFEAR_ERR_INVALID_ARGUMENT before anything is written
 * (*failed_experiment, optional, names the experiment, -1 otherwise) for offsets that do not run from 0 to n_rows without
 * descending, an experiment of more than 2^30 rows (CFEAR_ERR_CAPACITY), a NaN p_threshold, null pointers, host and
 * device buffers mixed; n_exp = 0 is OK.                                                                                */
int cfear_loop_curves_batch(cfear_ctx* ctx, const int64_t* row_offsets, const uint8_t* y, const double* score, const uint8_t* pos_ok,
                            int64_t n_rows, int32_t n_exp, const cfear_loop_curves_params* par, double* roc_fpr, double* roc_tpr,
                            double* roc_thr, double* pr_precision, double* pr_recall, double* pr_thr,
                            cfear_loop_curves_result* results, int32_t* failed_experiment);

/* ---- after the path: finishing a batch of pose graphs (Align, graph.txt, the trajectory files, the map) ----------------
 * What every run of the reference's SLAM executables ends in (tbv_slam/src/tbv_slam_offline.cpp:248-266): graph->Align(),
 * graph->SaveGraphString(), graph->OutputGraph(), and the map PoseGraphVis::ProcessFrame publishes on the way
 * (tbv_slam/src/tbv_slam/posegraph.cpp, cited as :line).  csrc/graphfinish.hip, DESIGN.md section 4.17.  The batch layout
 * is cfear_pgo_solve_batch's: flat per-node arrays, graph g owns nodes [node_offsets[g], node_offsets[g + 1]) in ascending
 * id order; node_offsets (host, n_graphs + 1 entries) runs from 0 to n_nodes without descending.
 *
 * cfear_graph_align_batch: PoseGraph::Align (:235-263) per graph.
 *   A = Tgt.p, B = T.p of the nodes with has_gt, in node order; best_fit_transform(A, B) (cfear_radarodometry/src/
 *   cfear_radarodometry/eval_trajectory.cpp:343-395): the centroids (sums divided by max(rows, 1)), H = sum (a - cA)(b - cB)^T,
 *   R = V U^T of its SVD with the third row of V^T negated when det R < 0, t = cB - R cA.  The sums are split over the lanes
 *   of one workgroup in an order the graph alone fixes; the SVD is the evaluator's host routine (cfear_eval_trajectories).
 *   Tgtalign = the general inverse of [R | t] (Affine3d::inverse(): cofactors times 1 / det, t' = -(R' t)); every node of
 *   the graph, with or without ground truth, becomes PoseEigToCeres(Tgtalign * GetPose()) (types.cpp:25-38): Eigen 3.3's
 *   toRotationMatrix, the product (a0 b0 + a1 b1) + a2 b2 (+ t), Eigen 3.3's matrix -> quaternion assignment (the trace
 *   branch when the trace is positive, else the largest diagonal entry by m11 > m00, then m22 > m(i,i)), then normalize():
 *   every coefficient divided by sqrt((xx + zz) + (yy + ww)).  The rewrite happens also when Tgtalign is the identity.
 *   ate = sum |Tgt.p - p_new| / max(n_gt, 1) over the nodes with ground truth: a mean, not an RMS.
 *   H exactly zero (no or one node with ground truth, or all of them at one place): R = I, t = cB - cA, CFEAR_OK, as the
 *   reference's JacobiSVD of a zero matrix returns identities.  H of rank 1 (all ground-truth positions on one line): the
 *   reference's result depends on the SVD implementation, so the graph's status is CFEAR_ERR_SOLVER, its poses are left
 *   untouched, align is the identity and ate is that of the untouched poses; the other graphs are not affected and the call
 *   returns CFEAR_OK.  A graph's poses and summary are bit-identical whatever else the batch holds and wherever it sits.
 * poses (in / out), gt and has_gt hold n_nodes entries and are all host or all device memory (device poses 8-byte aligned);
 * summaries [n_graphs] is host memory; the call synchronises (the SVDs are host code).                                   */
typedef struct cfear_graph_align_summary {
  double align[12];                     /* Tgtalign as [r | t], row-major 3 x 4: what every pose was left-multiplied by */
  double ate;
  int32_t n_gt;                         /* nodes with ground truth                                                      */
  int32_t status;                       /* CFEAR_OK or CFEAR_ERR_SOLVER                                                 */
} cfear_graph_align_summary;            /* 112 bytes */
int cfear_graph_align_batch(cfear_ctx* ctx, cfear_pose3d* poses, const cfear_pose3d* gt, const uint8_t* has_gt,
                            const int64_t* node_offsets, int64_t n_nodes, int32_t n_graphs, cfear_graph_align_summary* summaries);

/* cfear_graph_map_batch: the two maps of PoseGraphVis::ProcessFrame (:539-584) per graph.  The nodes whose ordinal within the
 * graph is a multiple of skip_frames are taken in node order and their cloud_peaks_ points appended in cloud order, each
 * through pcl::transformPointCloud<PointXYZI, double> with GetPose(): float(((m0 x + m1 y) + m2 z) + m3) for all three rows,
 * the intensity copied.  The ground-truth map takes the same points of the selected nodes that have ground truth through
 * PoseCeresToEig(Tgt) (the reference's Tgtalign there is the identity, :566).
 * xyzi [n_points][4] holds every node's cloud, node k's points at [cloud_offsets[k], cloud_offsets[k + 1]); cloud_offsets
 * (host, n_nodes + 1 entries) runs from 0 to n_points without descending; an empty cloud is legal.  poses, gt, has_gt and
 * xyzi are all host or all device memory, and so are map [map_cap][4] and map_gt [map_gt_cap][4] (of either kind; device
 * clouds and maps 16-byte aligned; map_gt is not used without want_gt_map).  summaries [n_graphs] (host) receives the point
 * range of each graph in the two maps; the graphs follow each other in batch order.  The ranges are computed on the host
 * from the offsets (has_gt is read back first when it is device memory) and written BEFORE anything else happens: a map
 * larger than its capacity gives CFEAR_ERR_CAPACITY with the summaries complete and nothing written to either map, so that
 * the caller can size the buffers (map may be NULL with map_cap 0) and call again.  Refused with
 * CFEAR_ERR_INVALID_ARGUMENT: skip_frames < 1 (the reference would compute % 0), offset tables that do not run from 0 to the
 * array lengths without descending, null pointers, buffers of mixed kinds.  One thread moves one point; a workgroup moves
 * one tile of CFEAR_GRAPH_MAP_TILE points of one node (exported so that tests can straddle it).                           */
#define CFEAR_GRAPH_MAP_TILE 256
typedef struct cfear_graph_map_params {
  int32_t skip_frames;                  /* 1: every node (PoseGraphVis::Parameters::skip_frames)                        */
  int32_t want_gt_map;                  /* 1                                                                            */
} cfear_graph_map_params;               /* 8 bytes */
typedef struct cfear_graph_map_summary {
  int64_t map_offset, map_points;       /* the graph's points in map                                                    */
  int64_t map_gt_offset, map_gt_points; /* ... and in map_gt (0, 0 without want_gt_map)                                 */
} cfear_graph_map_summary;              /* 32 bytes */
int cfear_graph_map_batch(cfear_ctx* ctx, const cfear_pose3d* poses, const cfear_pose3d* gt, const uint8_t* has_gt,
                          const int64_t* node_offsets, int64_t n_nodes, int32_t n_graphs, const float* xyzi,
                          const int64_t* cloud_offsets, int64_t n_points, const cfear_graph_map_params* par, float* map,
                          int64_t map_cap, float* map_gt, int64_t map_gt_cap, cfear_graph_map_summary* summaries);

/* Host writers, no context.  cfear_graph_string_write: PoseGraph::SaveGraphString (:177-187): per node RadarScan::ToString
 * (types.cpp:93-102) -- the 12 numbers of MatToString(GetPose().matrix()) (std::fixed, 6 decimals, one space between), a
 * space, std::to_string(stamp_) and a newline -- and the std::endl SaveGraphString appends: every node line is followed by
 * an empty line.  cfear_graph_output_write: PoseGraph::OutputGraph (:201-234): only the nodes with ground truth are
 * written, the pose to est_path and Tgt to gt_path (the reference's local names mgt / mest are swapped, the files are not);
 * when no node has ground truth every pose goes to est_path and gt_path is created empty.                               */
int cfear_graph_string_write(const char* path, const cfear_pose3d* poses, const uint64_t* stamps, int64_t n);
int cfear_graph_output_write(const char* est_path, const char* gt_path, const cfear_pose3d* poses, const cfear_pose3d* gt,
                             const uint8_t* has_gt, int64_t n);

#ifdef __cplusplus
}
#endif
#endif /* CFEAR_HIP_H */
