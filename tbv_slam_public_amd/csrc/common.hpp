// common.hpp -- shared host/device infrastructure of libcfear_hip.so (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/cfear_hip.h"
#include "batch_tables.hpp"
#include "owned.hpp"
#include "reg_layout.hpp"

#define CFEAR_WAVE 64

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// Owners of everything that outlives a call (a call's own memory goes through HostStage below): members of the handle
// structs, released by the struct's destructor in reverse declaration order -- so a struct declares the streams it owns
// before the buffers and events used on them, and its *_destroy synchronises those streams before it deletes the object.
// Kernels and HIP calls take the raw pointer (get()).
template <class T> using DevBuf = Owned<T, hipFree>;                  // device memory
template <class T> using PinnedBuf = Owned<T[], hipHostFree>;         // pinned host memory, indexed on the host
using Event = Owned<std::remove_pointer_t<hipEvent_t>, hipEventDestroy>;
using Stream = Owned<std::remove_pointer_t<hipStream_t>, hipStreamDestroy>;
using GraphExec = Owned<std::remove_pointer_t<hipGraphExec_t>, hipGraphExecDestroy>;
// The makers return an empty owner on failure and clear the sticky HIP error; 0 bytes allocate 256.
template <class T> DevBuf<T> dev_alloc(size_t bytes) {
  void* p = nullptr;
  if (hipMalloc(&p, bytes ? bytes : 256) != hipSuccess) { (void)hipGetLastError(); p = nullptr; }
  return DevBuf<T>((T*)p);
}
template <class T> PinnedBuf<T> pinned_alloc(size_t bytes) {
  void* p = nullptr;
  if (hipHostMalloc(&p, bytes ? bytes : 256, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); p = nullptr; }
  return PinnedBuf<T>((T*)p);
}
inline Event make_event(unsigned flags) {
  hipEvent_t e = nullptr;
  if (hipEventCreateWithFlags(&e, flags) != hipSuccess) { (void)hipGetLastError(); e = nullptr; }
  return Event(e);
}
inline Stream make_stream_nonblocking() {
  hipStream_t s = nullptr;
  if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); s = nullptr; }
  return Stream(s);
}

struct ProfRow {
  const char* name;
  double total_ms = 0.0;
  int64_t launches = 0;
  std::vector<std::pair<Event, Event>> pending;
};

// Workspace slots (cfear_ctx::ws).  Stages that are live at the same time use different slots; a slot with several users is
// never live in two of them at once (each user is done with it before it returns).
enum WsSlot : int {
  kWsImages = 0,          // staged polar images: filter host entry points; the rotated images of cfear_filter_row_keys
  kWsFilter = 1,          // filter host entry points: staged outputs and scratch
  kWsTrig = 2,            // cos / sin tables of the k-strongest cloud (cfear_ctx::trig_rows)
  kWsFilterRows = 3,      // k-strongest per-row counts; CA-CFAR detection bits and counts
  kWsSurface = 4,         // surface / scan host entry points: staged clouds, cells, queries, job records
  kWsSurfaceScratch = 5,  // cfear_scan_create's surface scratch
  kWsRegJobs = 6,         // matcher job records and results
  kWsRegScratch = 7,      // matcher scratch; also verify's registrations
  kWsClouds = 8,          // staged peak clouds: coral, verify, scan-context descriptors; scan-context distance buffers
  kWsCoral = 9,           // coral job records, results and per-point terms; scan-context descriptor buffers
  kWsCoralScratch = 10,   // coral scratch; also shard's allgather staging (never live at the same time)
  kWsSurfaceList = 11,    // the surface pipeline's fallback work list
  kWsKstrongCand = 12,    // fused k-strongest candidate lists
  kWsCandResults = 13,    // cfear_register_candidates: results for a host caller
  kWsVerify = 14,         // the verification chain's records and results
  kWsScSequence = 15,     // whole-graph Scan Context: node tables, descriptor database, query chunks
  kWsEval = 16,           // trajectory evaluation: staged and normalised poses, distances, tables, staged outputs
  kWsPgo = 17,            // batched pose-graph optimisation: one chunk's poses, tables and solver state
  kWsLogreg = 18,         // classifier fits: staged rows, labels and masks, job records, results
  kWsP2p = 19,            // p2p quality: group and job records, staged results and per-point minima
  kWsP2pScratch = 20,     // p2p quality: sorted reference clouds that do not fit the LDS
  kWsCart = 21,           // Cartesian image / CorAlCart quality: staged images, job records, partial sums, staged outputs
  kWsCartMap = 22,        // the fixed-point polar -> Cartesian map of the last geometry (cfear_ctx::cart_map_*)
  kWsClosure = 23,        // vicinity closure: staged positions, steps and motions, the block table, staged candidates
  kWsLoopEval = 24,       // loop rows and curves: staged graphs, candidates, scores and curves, job table, sort and scan scratch
  kWsTrajSync = 25,       // trajectory synchronisation: staged poses and stamps, pair and block tables, ranges, staged outputs
  kWsGraphFinish = 26,    // graph alignment and maps: staged poses, flags and clouds, graph, node and tile tables, sums, staged maps
  kWsTieAudit = 27,       // tie audit: job records, staged queries, staged records and per-query groups
  kWsVoxelAudit = 28,     // voxel-order audit: staged clouds, scan tables, leader lists and flags, staged records and voxel rows
  kWsCount
};

struct cfear_ctx {
  int device = 0;
  Stream owned_stream;        // empty when the caller supplied the stream; declared first, so everything below goes before it
  hipStream_t stream = nullptr;
  std::string last_error;
  int profile = 0;            // 0 off, 1 every kernel family, 2 the polar filter's row kernels only (the HBM-bound launch)
  std::vector<ProfRow> prof;
  std::vector<Event> event_pool;
  // grow-only device workspaces (indexed by WsSlot so stages of one pipeline do not alias)
  struct Ws { DevBuf<void> p; size_t bytes = 0; };
  Ws ws[kWsCount];
  // pinned host staging for small read-backs
  PinnedBuf<char> pinned;
  size_t pinned_bytes = 0;
  Event pinned_ev;                  // recorded behind the last asynchronous reader of `pinned` (HostStage::pinned)
  bool pinned_busy = false;
  // free list of scan slabs (capacity -> device pointers) so streaming does not hipMalloc
  struct Slab { DevBuf<void> p; int cap; };
  std::vector<Slab> free_slabs;
  int64_t live_scans = 0;
  // the largest arena a destroyed cfear_scan_batch left behind, so that create / destroy / create does not hipMalloc
  struct Arena { DevBuf<void> p; size_t bytes = 0; };
  Arena free_arena;
  int trig_rows = 0;      // rows the cos/sin tables in ws[kWsTrig] were built for
  // geometry the map in ws[kWsCartMap] was built for (cartesian.hip); cart_map_w = 0: none
  int cart_map_rows = 0, cart_map_w = 0;
  float cart_map_radar_res = 0.f, cart_map_cart_res = 0.f;
  int n_cu = 256;          // compute units of the device (cfear_ctx_create)
  int64_t opt[CFEAR_OPT_COUNT] = {1, 0, 0, 0};   // cfear_ctx_set_option (test / measurement hooks; include/cfear_hip.h)
  int64_t replay_chunk = 0;      // CFEAR_OPT_REPLAY_CHUNK
  int64_t kstrong_row_pairs = 1; // CFEAR_OPT_KSTRONG_ROW_PAIRS
  bool surf_list_dirty = true;   // the surface pipeline's hand-over counter may be non-zero (see cfear_surface_launch)
  std::vector<std::pair<const void*, int>> lds_allowed;   // kernels and the dynamic LDS they were already allowed on this device (cfear_allow_lds)
};

int cfear_set_error(cfear_ctx* ctx, int status, const char* fmt, ...);

#define CFEAR_CHECK(expr)                                                                       \
  do {                                                                                          \
    const int _rc = (expr);                                                                     \
    if (_rc != CFEAR_OK) return _rc;                                                            \
  } while (0)

#define CFEAR_HIP_CHECK(ctx, expr)                                                              \
  do {                                                                                          \
    hipError_t _e = (expr);                                                                     \
    if (_e != hipSuccess)                                                                       \
      return cfear_set_error((ctx), CFEAR_ERR_HIP, "%s failed: %s (%s:%d)", #expr,              \
                             hipGetErrorString(_e), __FILE__, __LINE__);                        \
  } while (0)

// true if p is device (or managed) memory visible to kernels without a copy
bool cfear_is_device_ptr(const void* p);
// grow-only workspace `slot` of at least `bytes`; returns nullptr on allocation failure
void* cfear_workspace(cfear_ctx* ctx, WsSlot slot, size_t bytes);
// One C-ABI call's boundary with host memory: everything that crosses from or into the caller's memory, and every host
// record or read-back of the callee, goes through a HostStage, so no copy from or into host memory outlives the call that
// enqueued it, on the error paths as well.  The call first plans what it needs -- in() / out() / piece() bind a pointer to
// the device address it resolves to, images() and cloud_in() stage polar images and peak clouds in their own slots -- then
// carve() allocates every piece with one cfear_workspace call (256-byte aligned) and enqueues the uploads.  Device memory
// of the caller is used in place.  finish() enqueues the copy-backs and synchronises, but only if the call touched host
// memory: an all-device call stays asynchronous (its pinned() record is marked busy on the stream instead of waited for).
// The destructor, and wait() / finish() when they fail, drain the stream if a copy was enqueued.
class HostStage {
 public:
  HostStage(cfear_ctx* ctx, WsSlot slot) : ctx_(ctx), slot_(slot) {}
  ~HostStage() { drain(); }
  HostStage(const HostStage&) = delete;
  HostStage& operator=(const HostStage&) = delete;

  // true if p is host memory; in() / out() / images() ask this of the caller's pointers, mixed() compares the answers
  bool is_host(const void* p);
  bool mixed() const { return host_ && device_; }
  bool any_host() const { return host_; }
  // in: p itself, or a piece that carve() uploads p's bytes to (and that finish() copies back when `back`); p may be null
  // when bytes is 0.  Returns true if p is staged.
  template <class T> bool in(T*& dev, T* p, size_t bytes, bool back = false) {
    if (!p || !bytes || !is_host(p)) { dev = p; return false; }
    plan(&dev, bind<T*>, bytes, p, back ? (void*)p : nullptr);
    return true;
  }
  // out: p itself, or a piece that finish() copies back to p.  A null p gets a piece that is not copied back.
  template <class T> bool out(T*& dev, T* p, size_t bytes) {
    if (p && !is_host(p)) { dev = p; return false; }
    plan(&dev, bind<T*>, bytes, nullptr, p);
    return p != nullptr;
  }
  template <class T> void piece(T*& dev, size_t bytes) { plan(&dev, bind<T*>, bytes, nullptr, nullptr); }
  // a batch of polar images (batch_stride between images when batch > 1): host images are staged densely in kWsImages
  cfear_polar_desc images(const uint8_t*& dev, const uint8_t* p, const cfear_polar_desc& desc);
  // peak clouds ([n] float4): one query per distinct pointer, host clouds staged once each in kWsClouds, at the longest n
  // any use names.  After carve(), cloud(p) is the device address of p (p itself if it was not staged).
  void cloud_in(const float* p, int n);
  const float4* cloud(const float* p) const;

  int carve();
  // a host record the call builds and uploads after carve(); owned by the stage, so it outlives the upload
  void* record(size_t bytes) { record_.assign(bytes, 0); return record_.data(); }
  // The same in the context's pinned staging (one per call), for records of megabytes -- a pageable source is staged
  // synchronously at a fraction of the PCIe rate -- and for records a kernel reads in place.  It does not make the call
  // synchronous: the staging is marked busy behind its upload (by finish(), behind the kernels, when it is read in place)
  // and handed out again once the stream is past the mark.  nullptr, with the error set, when the allocation fails.
  void* pinned(size_t bytes);
  int upload(void* dev, const void* host, size_t bytes);
  // a read-back into host memory the callee owns, enqueued at once; wait() -- or finish() -- waits for those enqueued so
  // far and reports the first that failed
  void fetch(void* host, const void* dev, size_t bytes);
  int wait();
  // a copy-back finish() enqueues (pitched when rows > 1)
  void back(void* host, const void* dev, size_t width, size_t rows = 1, size_t host_pitch = 0, size_t dev_pitch = 0) {
    backs_.push_back({host, dev, width, rows, host_pitch, dev_pitch});
  }
  int finish();

 private:
  template <class P> static void bind(void* where, char* addr) { *(P*)where = (P)addr; }
  void plan(void* where, void (*set)(void*, char*), size_t bytes, const void* up, void* down);
  void drain();

  struct Piece { void* where; void (*set)(void*, char*); size_t off, bytes; const void* up; void* down; };
  struct Back { void* host; const void* dev; size_t width, rows, host_pitch, dev_pitch; };
  struct Images { const uint8_t** where = nullptr; const uint8_t* p = nullptr; size_t img_bytes = 0; int64_t stride = 0; int batch = 0; };
  struct Cloud { bool host; int n; size_t off; };
  cfear_ctx* ctx_;
  WsSlot slot_;
  size_t bytes_ = 0, cloud_bytes_ = 0;
  std::vector<Piece> pieces_;
  std::vector<Back> backs_;
  Images images_;
  std::map<const float*, Cloud> clouds_;
  char* cloud_base_ = nullptr;
  std::vector<char> record_;
  void* pinned_ = nullptr;            // pinned() handed out and not yet marked busy
  hipError_t err_ = hipSuccess;       // the first copy-back or fetch() that failed
  bool host_ = false, device_ = false, sync_ = false, pending_ = false;
};
// The tables of a ragged batch (batch_tables.hpp) through a HostStage.  Constructed while the call plans its pieces; after
// carve(), upload() builds the host record -- in the context's pinned staging when `pinned` (HostStage::pinned) -- and
// uploads the first piece.  The second piece is the call's to fill at host_second() and to send with upload_second().
class StagedTables {
 public:
  StagedTables(HostStage& st, size_t record_bytes, size_t block_bytes, size_t second_bytes = 0, bool pinned = false)
      : st_(st), lay_(record_bytes, block_bytes, second_bytes), pinned_(pinned) {
    st.piece(d_first_, lay_.first);
    if (second_bytes) st.piece(d_second_, second_bytes);
  }
  int upload(const void* records, const void* blocks) {
    h_ = (char*)(pinned_ ? st_.pinned(lay_.first + lay_.second) : st_.record(lay_.first + lay_.second));
    if (!h_) return CFEAR_ERR_HIP;
    if (lay_.record_bytes) memcpy(h_, records, lay_.record_bytes);
    if (lay_.block_bytes) memcpy(h_ + lay_.blocks_at, blocks, lay_.block_bytes);
    return st_.upload(d_first_, h_, lay_.first);
  }
  template <class T> const T* records() const { return (const T*)d_first_; }
  template <class T> const T* blocks() const { return (const T*)(d_first_ + lay_.blocks_at); }
  template <class T> T* second() const { return (T*)d_second_; }
  template <class T> T* host_second() const { return (T*)(h_ + lay_.first); }
  int upload_second() { return st_.upload(d_second_, h_ + lay_.first, lay_.second); }

 private:
  HostStage& st_;
  TableLayout lay_;
  bool pinned_;
  char *d_first_ = nullptr, *d_second_ = nullptr, *h_ = nullptr;
};
// 0: all host, 1: all device, -1: mixed; null pointers are skipped
inline int memory_kind(std::initializer_list<const void*> ptrs) {
  int n = 0, dev = 0;
  for (const void* p : ptrs)
    if (p) { n++; dev += cfear_is_device_ptr(p); }
  return dev == 0 ? 0 : dev == n ? 1 : -1;
}
// hipFuncAttributeMaxDynamicSharedMemorySize, once per (context, kernel, size): the attribute is per device and contexts are
// per device, so a launch path asks every time and pays a linear look-up over a dozen entries instead of a runtime call
int cfear_allow_lds(cfear_ctx* ctx, const void* kernel, size_t bytes);

// profiling: wrap a kernel launch
int cfear_prof_row(cfear_ctx* ctx, const char* name);
void cfear_prof_begin(cfear_ctx* ctx, int row);
void cfear_prof_end(cfear_ctx* ctx, int row);

struct ProfScope {
  cfear_ctx* ctx;
  int row;
  ProfScope(cfear_ctx* c, const char* name) : ctx(c), row(-1) {
    if (ctx->profile == 1 || (ctx->profile == 2 && (!strcmp(name, "kstrongest_rows") || !strcmp(name, "cacfar_rows") || !strcmp(name, "kstrong_image")))) {
      row = cfear_prof_row(ctx, name);
      cfear_prof_begin(ctx, row);
    }
  }
  ~ProfScope() { if (row >= 0) cfear_prof_end(ctx, row); }
};

// ---------------------------------------------------------------------------------------------
// device-resident MapPointNormal ("scan"): SoA slab of `cap` cells
// ---------------------------------------------------------------------------------------------
struct ScanView {          // plain pointers into one slab; passed to kernels by value / in tables
  float2* mean_f;          // float copy of the means (pointnormal.cpp:151-162), NN search space
  double2* mean;           // u_
  double2* normal;         // snormal_
  double4* cov;            // cov_ row-major (c00,c01,c10,c11)
  double* scale;           // scale_
  double* avg_intensity;
  double2* lambda;         // (lambda_min, lambda_max)
  int32_t* nsamples;
  int32_t* n_cells;        // device counter (written by the surface kernel)
  // The matcher's search structure, prebuilt once per scan (grid_cells_block): the float means bucketed into a uniform
  // kScanGrid x kScanGrid grid over the scan's own extent -- what the reference keeps as a kd-tree per MapPointNormal
  // (pointnormal.cpp:151-162).  ONE block that a registration copies into LDS in 16-byte pieces:
  //   [kScanGridStartPad] u16  first record of every grid cell (row-major), entries past the last cell = n
  //   [np] float2              (x, y) of the records, grouped by grid cell            np = scan_grid_pad(n)
  //   [np] u16                 the records' cell indices (10 bytes per record in all: four keyframes + the LM arrays fit 40 KB)
  unsigned short* grid;
  float4* grid_geo;        // (x0, y0, cells per metre, 1 = tables valid | 0 = more cells than the 16-bit table can address)
  int32_t cap;
  int32_t pad;
};
// (kScanGrid, kScanGridCells, kScanGridStartPad, scan_grid_pad: reg_layout.hpp -- the matcher's LDS arithmetic is made of them)
__host__ __device__ inline size_t scan_grid_bytes(int n) { return (size_t)kScanGridStartPad * 2 + (size_t)scan_grid_pad(n) * 10; }
constexpr float kScanGridMinEdge = 2.0f;                       // cell edge floor [m]: the matcher's radius (registration.h:131)

struct cfear_scan {
  cfear_ctx* ctx;
  DevBuf<void> slab;       // moves to cfear_ctx::free_slabs with the last reference
  ScanView view;
  int32_t n_cells_host;    // -1 until read back
  uint32_t surf_path = 0;  // CFEAR_SURF_PATH_* of the surface-point launch that made the cells (0: none did)
  int32_t refs = 1;        // the caller's handle + one per scan table that names it (handles are used from one host thread)
  cfear_scan_batch* batch = nullptr;   // a borrowed view into that batch's arena (cfear_scan_create_batch): `slab` is empty, the
                                       // first reference is the batch's own and cfear_scan_destroy refuses to drop it
};
void cfear_scan_retain(cfear_scan* scan);   // a scan table's reference; cfear_scan_release drops it
// Drops one reference, the slab (or, with the last handle of a destroyed batch, the arena) is recycled with the last.  The
// public cfear_scan_destroy is this for a handle of the caller's own and a refusal for a borrowed one, whatever its count:
// a table's reference can only be dropped by the table.
int cfear_scan_release(cfear_scan* scan);

// N scans in one arena (cfear_scan_create_batch, surface.hip): scan i's slab is arena + i * cfear_scan_slab_bytes(max_cells).
// The arena outlives cfear_scan_batch_destroy for as long as a scan table still names one of its scans: the batch is freed
// with the last reference on its last scan (cfear_scan_destroy), and its arena goes to cfear_ctx::free_arena.
struct cfear_scan_batch {
  cfear_ctx* ctx = nullptr;
  DevBuf<void> arena;
  size_t arena_bytes = 0;
  std::vector<cfear_scan*> scans;      // [n_scans]; nullptr where the scan failed
  int32_t live = 0;                    // handles not yet deleted
  bool released = false;               // cfear_scan_batch_destroy was called: the handles' first reference is gone
};
void cfear_scan_batch_free(cfear_scan_batch* b);   // live == 0: recycles the arena and deletes the batch
// cfear_scan_create_batch behind its argument checks, cloud by cloud (surface.hip): clouds[i] = the lengths[i] >= 0 points of
// scan i, on_host[i] whether they are host memory, one_buffer whether they are all pieces of one buffer of the caller's
int cfear_scan_batch_build(cfear_ctx* ctx, const float* const* clouds, const char* on_host, bool one_buffer, const int32_t* lengths, int n_scans,
                           const cfear_feature_params* par, const double* mots, int max_cells, cfear_scan_batch** out, int32_t* status);

size_t cfear_scan_slab_bytes(int cap);
ScanView cfear_scan_view(void* slab, int cap);
int cfear_scan_alloc(cfear_ctx* ctx, int cap, cfear_scan** out);
int cfear_scan_clone_view(cfear_ctx* ctx, const ScanView& src, int n_cells, cfear_scan** out);

// ---------------------------------------------------------------------------------------------
// cross-file entry points (device-pointer level; used by the batched odometry pipeline)
// ---------------------------------------------------------------------------------------------
// Optional extras of the device-side k-strongest entry (the batched odometry pipeline):
//   row_keys / row_valid    the kept bins beyond min_distance of every row as packed keys (intensity << 24 | range bin)
//                           at [(b * rows + r) * k + j], j < row_valid[(b * rows + r) * 2], in the reference's cloud
//                           order (k <= 64); the surface-point kernel compacts the rows and converts them to PointXYZI,
//                           so neither sel_* arrays nor a cloud kernel are needed;
//   image_offsets           device [batch] byte offsets of the images from d_polar (streams whose sweeps do not sit at
//                           a constant stride: ring buffers, one buffer per sequence) instead of b * batch_stride.
struct cfear_kstrong_fused {
  uint32_t* row_keys = nullptr;
  int32_t* row_valid = nullptr;
  const int64_t* image_offsets = nullptr;
  uint32_t* cand_stats = nullptr;     // fused decode only: device [64] counters, += the candidates (bins >= z_min) of the batch
};
int cfear_kstrong_device(cfear_ctx* ctx, const uint8_t* d_polar, const cfear_polar_desc* desc,
                         const cfear_kstrong_params* par, const cfear_kstrong_out* o, bool dense_halo = false,
                         const cfear_kstrong_fused* fused = nullptr);
// Row keys of several parameter sets from one sweep's sel_* lists (kstrong_derive.hip).  A class as the kernel reads it;
// cfear_kstrong_derive_class fills one from the caller's record, 0 = refused (image, k or threshold outside the sweep's).
struct KstrongDeriveClass { int32_t image, k, u_zmin, min_range_bin; };
int cfear_kstrong_derive_class(const cfear_rowkeys_class* in, int n_images, int k_sup, int u_sup, KstrongDeriveClass* out);
// d_row_keys [n_classes][rows][64], d_row_counts [n_classes][rows][2]; everything in device memory, k_sup <= 64
int cfear_kstrong_derive_device(cfear_ctx* ctx, const int32_t* d_sel_range, const uint8_t* d_sel_intensity, const int32_t* d_sel_count,
                                int rows, int k_sup, const KstrongDeriveClass* d_classes, int n_classes, uint32_t* d_row_keys,
                                int32_t* d_row_counts);
// fused decode + sweep for [range bins][azimuths] sources (sd = the SOURCE images); key output only
bool cfear_kstrong_cols_supported(const uint8_t* d_src, const cfear_polar_desc* sd, const cfear_kstrong_params* par);
bool cfear_kstrong_cols_preferred(const uint8_t* d_src, const cfear_polar_desc* sd, const cfear_kstrong_params* par);   // ... and the batch is large enough to pay
int cfear_kstrong_cols_device(cfear_ctx* ctx, const uint8_t* d_src, const cfear_polar_desc* sd, const cfear_kstrong_params* par,
                              const cfear_kstrong_fused* fused, int route = 0);
int cfear_compensate_batch_device(cfear_ctx* ctx, float* d_xyzi, size_t cloud_stride_points, const int32_t* d_n,
                                  const double* d_mot, int n_clouds, int max_points, int ccw);
int cfear_rotate_ccw_device(cfear_ctx* ctx, const uint8_t* d_src, const cfear_polar_desc* src_desc, uint8_t* d_dst,
                            int dst_stride, int64_t dst_batch_stride);
// CA-CFAR for the batched odometry: per-row key lists (intensity << 24 | range bin, ascending bins; row_cnt[2 row] = the
// row's detections, which may exceed kcap -- the keys beyond are dropped and surface_prep_kernel reports the scan) in the
// layout of cfear_kstrong_fused, so surface_prep_kernel compacts and converts them (rho = range_res * bin, cfar.cpp:43).
struct cfear_cacfar_fused {
  uint32_t* row_keys = nullptr;
  int32_t* row_cnt = nullptr;
  int kcap = 0;
  // desc describes [range bins][azimuths] SOURCE images (rows = bins, cols = azimuths): the decode is fused into the filter
  // (cacfar_cols_kernel); only where cfear_cacfar_cols_supported() says so
  bool bins_major = false;
};
bool cfear_cacfar_cols_supported(const uint8_t* d_src, const cfear_polar_desc* sd, const cfear_cacfar_params* par);
int cfear_cacfar_device(cfear_ctx* ctx, const uint8_t* d_polar, const cfear_polar_desc* desc,
                        const cfear_cacfar_params* par, float* d_xyzi, int32_t* d_n_points,
                        int32_t cap_points, uint8_t* d_det_mask, const cfear_cacfar_fused* fused = nullptr);
size_t cfear_surface_lds_bytes();
size_t cfear_surface_scratch_bytes(int cap_points);   // per scan, for clouds of up to cap_points points
size_t cfear_surface_job_bytes();
int cfear_surface_max_points();
void cfear_surface_fill_job(void* dst, float* d_xyzi, const int32_t* d_n, int32_t n_host, int compensate,
                            const double mot[3], const ScanView& out);
// rows mode: the cloud is handed over as the fused filter output (cfear_kstrong_fused) and compacted by the kernel
// into d_xyzi (capacity cfear_surface_max_points()); d_n_out receives the point count.  rows <= 4096.
void cfear_surface_fill_job_rows(void* dst, float* d_xyzi, int32_t* d_n_out, const uint32_t* d_row_keys, const int32_t* d_row_cnt,
                                 int rows, int k, int compensate, const double mot[3], const ScanView& out);
// rows mode needs the polar -> Cartesian constants: call before cfear_surface_launch (per context)
// rho = range_off + range_res * bin: range_off = range_res / 2 for the k-strongest filter (radar_filters.cpp:324), 0 for CA-CFAR
struct cfear_surface_polar { const double* cos_t = nullptr; const double* sin_t = nullptr; double range_res = 0.0, range_off = 0.0; int rows = 0, k = 0; };
int cfear_trig_tables(cfear_ctx* ctx, int rows, double** d_cos, double** d_sin);
// max_cell_cap: the largest cell capacity (ScanView::cap) among the jobs' output slabs
int cfear_surface_launch(cfear_ctx* ctx, const void* d_jobs, int n_jobs, const cfear_feature_params* par,
                         char* d_scratch, int32_t* d_status, int32_t* d_ncells_out, int max_cell_cap, int cap_points,
                         const cfear_surface_polar* polar = nullptr, uint32_t* d_path_out = nullptr);
// the route word (CFEAR_SURF_PATH_*) of job `job` of the last launch over d_scratch, read from its scratch header (waits for the stream)
int cfear_surface_read_path(cfear_ctx* ctx, const char* d_scratch, int cap_points, int job, uint32_t* path);
// cfear_coral_quality_batch in two halves (coral.hip): launch, then read back -- host work of the caller in between
struct CoralPending {
  explicit CoralPending(cfear_ctx* ctx) : stage(ctx, kWsCoral) {}
  HostStage stage;                    // the staged clouds and job records; drained unless cfear_coral_collect completes
  void* d_res = nullptr;
  void* d_pp = nullptr;
  int n_jobs = 0, cap = 0;
};
int cfear_coral_enqueue(cfear_ctx* ctx, const cfear_coral_job* jobs, int32_t n_jobs, const cfear_coral_params* par, bool want_per_point,
                        CoralPending& pend);
int cfear_coral_collect(cfear_ctx* ctx, const cfear_coral_job* jobs, CoralPending& pend, cfear_coral_result* results, double* per_point);

// One CorAl job of coral_kernel (coral.hip): two peak clouds on the DEVICE and their poses
struct CoralJob {
  const float4* ref;
  const float4* src;
  const int32_t* n_ref_ptr;           // device-side counts (pipelines), or nullptr -> the host values
  const int32_t* n_src_ptr;
  int32_t n_ref, n_src;
  double ref_pose[3], src_pose[3], offset[3];
};
// coral_kernel over job records that already sit on the device (verify.hip builds them there): results to d_results [n_jobs]
// (device), nothing is synchronised.  cap = the largest n_ref + n_src among the jobs (the per-job scratch's size).
int cfear_coral_launch_device(cfear_ctx* ctx, const CoralJob* d_jobs, int n_jobs, int cap, const cfear_coral_params* par,
                              cfear_coral_result* d_results);
int cfear_coral_max_points();
// evaluate.hip's 3 x 3 alignment, also cfear_graph_align_batch's (graphfinish.hip): s = mean x (3), mean y (3), the covariance sum y x^T row-major (9) -> [r | t] with
// r = u diag(1, 1, det u det v) v^T and t = mean y - r mean x; false (and r = I) when the second singular value vanishes
bool cfear_align_from_sums(const double* s, double align[12]);


// ---------------------------------------------------------------------------------------------
// device helpers
// ---------------------------------------------------------------------------------------------
#if defined(__HIPCC__)

// Loads and stores through pointers that are KNOWN to address global memory but whose static type is generic (pointers kept
// in job records, LDS tables, ScanView): a generic pointer compiles to flat_load / flat_store, which count in lgkmcnt as
// well as vmcnt, so every wait for an LDS read behind one also waits for the memory round trip -- a loop that mixes LDS
// reads with such loads runs them one at a time.  T: a scalar or an ext_vector_type (HIP's double2 / float4 structs have
// no address-space-qualified copy constructors).
typedef uint32_t g_u32x4 __attribute__((ext_vector_type(4)));
typedef double g_f64x2 __attribute__((ext_vector_type(2)));
typedef double g_f64x4 __attribute__((ext_vector_type(4)));
typedef float g_f32x4 __attribute__((ext_vector_type(4)));
typedef float g_f32x2 __attribute__((ext_vector_type(2)));
template <class T>
__device__ __forceinline__ T gload(const void* p) { return *(const __attribute__((address_space(1))) T*)p; }
template <class T>
__device__ __forceinline__ void gstore(void* p, T v) { *(__attribute__((address_space(1))) T*)p = v; }
__device__ __forceinline__ double2 gload_d2(const double2* p) { const g_f64x2 v = gload<g_f64x2>(p); return make_double2(v.x, v.y); }
__device__ __forceinline__ double4 gload_d4(const double4* p) { const g_f64x4 v = gload<g_f64x4>(p); return make_double4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ float4 gload_f4(const float4* p) { const g_f32x4 v = gload<g_f32x4>(p); return make_float4(v.x, v.y, v.z, v.w); }

// DPP move: lanes without a valid source (or masked off) receive 0.
template <int CTRL, int ROW_MASK = 0xf, int BANK_MASK = 0xf, bool BOUND = true>
__device__ __forceinline__ int dpp_mov(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, BANK_MASK, BOUND);
}

// Inclusive prefix sum across the 64 lanes of a wavefront (row_shr Hillis-Steele inside each
// 16-lane DPP row, then row_bcast:15 / row_bcast:31 to carry row totals).  6 DPP adds, no LDS.
__device__ __forceinline__ int wave_incl_scan_i32(int v) {
  v += dpp_mov<0x111>(v);                      // row_shr:1
  v += dpp_mov<0x112>(v);                      // row_shr:2
  v += dpp_mov<0x114>(v);                      // row_shr:4
  v += dpp_mov<0x118>(v);                      // row_shr:8
  v += dpp_mov<0x142, 0xa, 0xf, false>(v);     // row_bcast:15 -> rows 1,3
  v += dpp_mov<0x143, 0xc, 0xf, false>(v);     // row_bcast:31 -> rows 2,3
  return v;
}

// Inclusive prefix maximum of non-negative values (same DPP ladder).
__device__ __forceinline__ int wave_incl_scan_max_i32(int v) {
  v = max(v, dpp_mov<0x111>(v));
  v = max(v, dpp_mov<0x112>(v));
  v = max(v, dpp_mov<0x114>(v));
  v = max(v, dpp_mov<0x118>(v));
  v = max(v, dpp_mov<0x142, 0xa, 0xf, false>(v));
  v = max(v, dpp_mov<0x143, 0xc, 0xf, false>(v));
  return v;
}

// Wave-uniform sum (result in an SGPR).
__device__ __forceinline__ int wave_sum_i32(int v) {
  return __builtin_amdgcn_readlane(wave_incl_scan_i32(v), 63);
}

// Sum of a double over each 16-lane DPP row; every lane of the row receives the row total.
// Order: pairwise butterfly (quad xor 1, xor 2, half-mirror, mirror) -- deterministic.
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
// DPP move with a bank mask: lanes of disabled banks (lane quads of each row) keep `old`.
template <int CTRL, int BANK>
__device__ __forceinline__ double dpp_sel_f64(double old, double src) {
  const int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(src), CTRL, 0xf, BANK, false);
  const int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(src), CTRL, 0xf, BANK, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double row16_sum_f64(double v) {
  v += dpp_f64<0xB1>(v);    // quad_perm [1,0,3,2]
  v += dpp_f64<0x4E>(v);    // quad_perm [2,3,0,1]
  v += dpp_f64<0x141>(v);   // row_half_mirror
  v += dpp_f64<0x140>(v);   // row_mirror
  return v;
}
// Wave total in lane 63 only: row sums, then (R3 + R2) + (R1 + R0) through row_bcast -- no readlanes.
__device__ __forceinline__ double wave_sum_lane63_f64(double v) {
  v = row16_sum_f64(v);
  {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, 0x142, 0xa, 0xf, false);   // row_bcast:15 -> rows 1,3
    hi = __builtin_amdgcn_update_dpp(0, hi, 0x142, 0xa, 0xf, false);
    v += __hiloint2double(hi, lo);
  }
  {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, 0x143, 0xc, 0xf, false);   // row_bcast:31 -> rows 2,3
    hi = __builtin_amdgcn_update_dpp(0, hi, 0x143, 0xc, 0xf, false);
    v += __hiloint2double(hi, lo);
  }
  return v;
}
__device__ __forceinline__ double readlane_f64(double v, int lane) {
  int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}
// Wave-uniform sum of a double: row sums, then rows 0..3 added in order.
__device__ __forceinline__ double wave_sum_f64(double v) {
  v = row16_sum_f64(v);
  return ((readlane_f64(v, 0) + readlane_f64(v, 16)) + readlane_f64(v, 32)) + readlane_f64(v, 48);
}
// Sum over a workgroup of 256 threads (4 wavefronts), the same value in every thread; red = 4 doubles of LDS.  Order: each
// wave's wave_sum_f64, then the four waves in order (evaluate.hip, graphfinish.hip).
__device__ __forceinline__ double block_sum(double v, double* red) {
  v = wave_sum_f64(v);
  __syncthreads();                                   // the previous sum's readers are done with red
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}
#endif  // __HIPCC__
