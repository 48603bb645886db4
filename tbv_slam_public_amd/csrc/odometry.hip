// odometry.hip -- batched radarDriver + OdometryKeyframeFuser: n_streams independent sequences advance
// one frame per call, polar image in -> SE(2) pose out, everything in between on the GPU.
//
// Restates per stream (cfear_radarodometry/src/cfear_radarodometry/):
//   radarDriver::CallbackOffline / Process            radar_driver.cpp:48-73, 163-176
//   OdometryKeyframeFuser::processFrame               odometrykeyframefuser.cpp:143-259
//     KeyFrameBasedFuse                               :62-73
//     AccelerationVelocitySanityCheck                 :76-94
//     FormatScans / AddToReference                    :470-494
// The frame policy (constant-velocity guess, sanity check, keyframe test, sliding keyframe window)
// is host code exactly as in the reference; the four stages F, C, N, M are three kernel launches
// over the whole batch (kstrongest_rows + kstrong_cloud, surface_points, register) and one small
// read-back (pose, counts) per call.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>

#include "odometry_policy.hpp"

// ---- frame policy as pure host functions (no GPU, no context): the two decisions OdometryKeyframeFuser takes per frame ----
// KeyFrameBasedFuse (odometrykeyframefuser.cpp:62-73): diff = T_keyframe^-1 * Tcurrent as (x, y, theta).  For a planar
// pose Matrix3d::eulerAngles(0,1,2) is (0, 0, theta), so its norm is |theta|.
extern "C" int cfear_keyframe_based_fuse(const double diff_xyt[3], int32_t use_keyframe, double min_keyframe_dist,
                                         double min_keyframe_rot_deg) {
  if (!use_keyframe) return 1;
  const double tn = std::sqrt(diff_xyt[0] * diff_xyt[0] + diff_xyt[1] * diff_xyt[1]);
  const double rot = std::fabs(diff_xyt[2]);
  return (tn > min_keyframe_dist || rot > (min_keyframe_rot_deg * M_PI / 180.0)) ? 1 : 0;
}
extern "C" int cfear_acc_vel_sanity_check(const double tmot_prev_xy[2], const double tmot_curr_xy[2]) {
  return pose2d_acc_vel_sane(tmot_prev_xy, tmot_curr_xy);        // pose2d.hpp: the replay's score kernel takes it from there too
}

// Fused decode of [range bins][azimuths] sweeps: candidates per azimuth beyond which the rotation kernel + row sweep are the
// quicker route (the lists cost ~17 ns of a 2048-sweep pass per candidate and azimuth: equal at ~84, tools/decode_bench.py
// [--dense]), and for how many frames that verdict stands before one frame measures again.
constexpr double kDecodeDense = 80.0;
constexpr int kDecodeHold = 32;

struct cfear_odometry {
  cfear_ctx* ctx = nullptr;
  // Every small copy of a frame runs here, ordered against the kernel stream by events: job tables and image offsets go up
  // while kernels run, the result block comes down while the next sweep runs.  A copy on the kernel stream itself makes the
  // kernel behind it wait for a copy-engine round trip.  (first: the buffers and events used on it go before it)
  Stream copy_stream;
  int n_streams = 0;
  cfear_polar_desc desc{};             // layout the filters see: rows = azimuths
  cfear_polar_desc in_desc{};          // layout of the caller's images (differs when par.rotate_ccw)
  cfear_odometry_params par{};
  int cap_points = 0, cell_cap = 0, slabs_per_stream = 0;
  size_t slab_bytes = 0;
  // device memory (one allocation each)
  DevBuf<uint8_t> d_polar;             // staging when the caller passes host images
  DevBuf<uint8_t> d_rot;               // rotated images (par.rotate_ccw)
  bool fused_decode = false;           // par.rotate_ccw: the filter stage decodes the source itself where it pays (no d_rot)
  // ... which it does on radar-like sweeps (a few dozen bins >= z_min per azimuth): the candidate lists cost time per
  // candidate, the rotation kernel + row sweep do not.  The decode reports the batch's candidates; beyond kDecodeDense per
  // azimuth the next kDecodeHold frames take the two-kernel route, then one frame probes again.
  DevBuf<uint32_t> d_decode_stats;     // [2 buffers][64]
  PinnedBuf<uint32_t> h_decode_stats;  // pinned copy
  bool decode_measured[2] = {false, false};
  int decode_hold = 0;
  DevBuf<char> d_sel;                  // sel_range | sel_intensity | sel_count
  DevBuf<float> d_xyzi2[2];                  // filter outputs are double-buffered: the next frame's filter
  DevBuf<int32_t> d_npts2[2];                //   may run while the host applies this frame's policy
  float* d_xyzi = nullptr;                   // buffer of the frame being processed (not owned, like d_npts, d_pk, d_npk)
  int32_t* d_npts = nullptr;
  // fused filter output (k-strongest without keep_nodes, k <= 64): per-row points + counts written by the polar sweep
  // itself; the surface-point kernel compacts them, so neither sel_* arrays nor a cloud kernel exist in this mode
  bool fused = false;
  // the same hand-over for CA-CFAR (no keep_nodes): cacfar_rows_kernel leaves per-row keys with a row capacity row_k
  bool fused_cfar = false;
  int row_k = 0;                                 // keys per row in d_rowpts2: k (k-strongest) or the CA-CFAR row capacity
  DevBuf<uint32_t> d_rowpts2[2];                 // [B][rows][k] packed keys (intensity << 24 | range bin)
  DevBuf<int32_t> d_rowcnt2[2];                 // [B][rows][2]
  DevBuf<int64_t> d_offsets2[2];                // [B] image offsets of the sweep in each filter buffer (process_offsets)
  PinnedBuf<int64_t> h_offsets;              // pinned staging, [2][B]
  std::vector<int64_t> prefetched_offsets;   // offsets the prefetched filter output was computed from
  // par.keep_nodes: the peaks cloud of every frame (cloud_peaks_ of RadarScan), double-buffered like the cloud
  DevBuf<float> d_pk2[2];
  DevBuf<int32_t> d_npk2[2];
  float* d_pk = nullptr;
  int32_t* d_npk = nullptr;
  DevBuf<double> d_mot;                      // [B][3] TprevMot of this frame (peaks compensation)
  PinnedBuf<double> h_mot;
  PinnedBuf<int32_t> h_npk;
  std::vector<int> last_slab;                // slab that holds each stream's last processed scan
  int cur_buf = 0;
  const uint8_t* prefetched = nullptr;       // polar pointer whose filter output sits in buffer cur_buf ^ 1
  Event ev_results;                          // this frame's read-back has landed (copy_stream)
  Event ev_jobs;                             // the registration job upload on copy_stream
  Event ev_surf_jobs;                        // the surface job upload on copy_stream
  Event ev_offsets[2];                       // the image-offset upload of each filter buffer on copy_stream
  Event ev_frame;                            // the frame's last work on the kernel stream: the read-back waits for it
  // The read-back moves to the copy stream only when the kernel stream is a stream object.  A context may also be given one
  // of the runtime's stream HANDLES (the null stream, hipStreamLegacy, hipStreamPerThread: small integers, not pointers), and
  // hipStreamWaitEvent on another stream reads the stream an event was recorded on through that value.  Behind such a
  // handle the read-back stays on the kernel stream, in front of the prefetched sweep.
  bool readback_on_copy_stream = false;
  DevBuf<char> d_slabs, d_surf_jobs, d_reg_jobs;
  // what a frame returns to the host lives in ONE device block (and one pinned block): results | status | n_cells |
  // n_points -- one read-back per frame instead of four small copies queued between the matcher and the next sweep
  DevBuf<char> d_out;
  PinnedBuf<char> h_out;
  size_t out_bytes = 0;
  // pointers into d_out / h_out (not owned)
  int32_t* d_npts_out = nullptr;       // n_points slot of the block (rows mode: written by surface_prep_kernel)
  cfear_reg_result* d_results = nullptr;
  int32_t* d_status = nullptr;
  int32_t* d_ncells = nullptr;         // gathered n_cells of the current scans
  DevBuf<char> d_surf_scratch, d_reg_scratch;
  // pinned host mirrors
  PinnedBuf<char> h_surf_jobs, h_reg_jobs;
  cfear_reg_result* h_results = nullptr;
  int32_t* h_status = nullptr;
  int32_t* h_npts = nullptr;
  int32_t* h_ncells = nullptr;
  // covariance by cost sampling (optional): n^3 GetCost records per stream and the cached fit
  DevBuf<cfear_reg_result> d_samples;
  PinnedBuf<cfear_reg_result> h_samples;
  CovFit fit;
  std::vector<double> cov;             // [n_streams][36] cov_current
  std::vector<int32_t> cov_sampled;    // [n_streams]
  std::vector<StreamState> streams;
  int big_regs = 0;                    // > 0: recent frames held registrations too large for 80 KB of LDS -> keep the second launch on
  std::vector<double> cost_est, cost_tmp;   // per stream: work of its last registration (residuals x iterations): orders the next batch
  std::vector<int> job_slot;                 // per stream: class | rank inside the class << 3 of this frame's registration (-1: none)
  std::vector<ScanView> views;         // [n_streams * slabs_per_stream]
};

// both streams idle: what an error exit and the teardown need before buffers are reused or freed
static void drain_streams(cfear_odometry* od) {
  if (od->copy_stream) (void)hipStreamSynchronize(od->copy_stream.get());
  (void)hipStreamSynchronize(od->ctx->stream);
}

extern "C" int cfear_odometry_destroy(cfear_odometry* od) {
  if (!od) return CFEAR_OK;
  (void)hipSetDevice(od->ctx->device);
  drain_streams(od);
  delete od;
  return CFEAR_OK;
}

extern "C" int cfear_odometry_create(cfear_ctx* ctx, int32_t n_streams, const cfear_polar_desc* desc,
                                     const cfear_odometry_params* par, cfear_odometry** out) {
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (!desc || !par || !out || n_streams < 1) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  *out = nullptr;
  if (desc->batch != n_streams) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "desc.batch must equal n_streams");
  if (par->submap_scan_size < 1 || par->submap_scan_size + 1 > kRegMaxScans)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "submap_scan_size must be in [1,%d]", kRegMaxScans - 1);
  if (!(par->res > 0.05f)) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "res must be > 0.05");   // odometrykeyframefuser.cpp:25
  if (par->estimate_cov_by_sampling && (par->cov_sampling.samples_per_axis < 1 || par->cov_sampling.samples_per_axis > 15))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "cov_sampling.samples_per_axis must be in [1,15]");
  {
    // the same argument rules as the standalone filter entry points (cfear_filter_kstrongest / cfear_filter_cacfar)
    const int fcols = par->rotate_ccw ? desc->rows : desc->cols;
    if (desc->rows <= 0 || desc->cols <= 0 || desc->stride < desc->cols ||
        (n_streams > 1 && desc->batch_stride < (int64_t)desc->rows * desc->stride))
      return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "bad polar descriptor");
    if (fcols > 8192) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "more than 8192 range bins unsupported");
    if (par->filter_type == CFEAR_FILTER_CACFAR) {
      if (par->cacfar.window_size < 1 || par->cacfar.nb_guard_cells < 0 || !(par->cacfar.range_res > 0.f))
        return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "bad CFAR parameters");
    } else if (par->filter_type == CFEAR_FILTER_KSTRONG) {
      if (par->kstrong.k_strongest < 1 || par->kstrong.k_strongest > 1024)
        return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "k_strongest must be in [1,1024]");
      if (!(par->kstrong.range_res > 0.f) || !(par->kstrong.min_distance >= 0.f))
        return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "range_res must be > 0 and min_distance >= 0");
    } else {
      return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "unknown filter_type %d", par->filter_type);
    }
  }
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  std::unique_ptr<cfear_odometry, FreeWith<cfear_odometry_destroy>> od(new cfear_odometry());
  od->ctx = ctx; od->n_streams = n_streams; od->desc = *desc; od->in_desc = *desc; od->par = *par;
  if (par->rotate_ccw) {               // radarDriver::Callback (radar_driver.cpp:74-90): [bins][azimuths] -> rows = azimuths
    od->desc.rows = desc->cols;
    od->desc.cols = desc->rows;
    od->desc.stride = (desc->rows + 127) / 128 * 128;    // rows on 128-byte lines: the rotation then writes whole lines
    od->desc.batch_stride = (int64_t)od->desc.rows * od->desc.stride;
  }
  const int B = n_streams, rows = od->desc.rows, k = par->kstrong.k_strongest;
  // CA-CFAR puts no bound on the detections of a row (cfar.cpp:35-71): room for 65 536 points per sweep (the surface
  // kernels take clouds beyond 16 384 points through their global-memory path); k-strongest keeps at most rows * k
  od->cap_points = par->filter_type == CFEAR_FILTER_CACFAR ? std::min(rows * od->desc.cols, 65536) : rows * k;
  od->cell_cap = 2048;
  od->slabs_per_stream = par->submap_scan_size + 2;
  od->slab_bytes = cfear_scan_slab_bytes(od->cell_cap);
  const size_t nsel = (size_t)B * rows * std::max(k, 1);
  // one buffer each; after the first failure nothing more is allocated
  bool ok = true;
  auto dev = [&ok](auto& buf, size_t bytes) { ok = ok && (buf = dev_alloc<typename std::decay_t<decltype(buf)>::element_type>(bytes)); };
  auto pin = [&ok](auto& buf, size_t bytes) { ok = ok && (buf = pinned_alloc<typename std::decay_t<decltype(buf)>::element_type>(bytes)); };
  od->fused = par->filter_type == CFEAR_FILTER_KSTRONG && !par->keep_nodes && k <= 64 && rows <= 4096 &&
              rows * k <= cfear_surface_max_points();
  od->row_k = k;
  // [range bins][azimuths] sources: decode fused into the sweep (CFEAR_OPT_FUSED_DECODE = 0 keeps the two-kernel route, for
  // A/B runs and the tests that compare the two)
  od->fused_decode = od->fused && par->rotate_ccw && ctx->opt[CFEAR_OPT_FUSED_DECODE] != 0;
  if (od->fused_decode) {
    dev(od->d_decode_stats, 2 * 64 * 4);
    pin(od->h_decode_stats, 2 * 64 * 4);
  }
  // CA-CFAR puts no bound on a row's detections either: 1024 keys per row (a row beyond that marks its scan
  // CFEAR_ERR_CAPACITY, like a sweep beyond cap_points)
  od->fused_cfar = par->filter_type == CFEAR_FILTER_CACFAR && !par->keep_nodes && rows <= 4096;
  if (od->fused_cfar) {
    od->row_k = std::min((od->desc.cols + 3) / 4 * 4, 1024);
    for (int i = 0; i < 2; i++) {
      dev(od->d_rowpts2[i], (size_t)B * rows * od->row_k * 4);
      dev(od->d_rowcnt2[i], (size_t)B * rows * 8);
    }
  }
  if (od->fused) {
    for (int i = 0; i < 2; i++) {
      dev(od->d_rowpts2[i], nsel * 4);
      dev(od->d_rowcnt2[i], (size_t)B * rows * 8);
      dev(od->d_offsets2[i], (size_t)B * 8);
    }
    pin(od->h_offsets, (size_t)B * 8 * 2);
  } else {
    dev(od->d_sel, nsel * 4 + 2 * (nsel + 256) + (size_t)B * rows * 4 + 1024);   // + is_peak (keep_nodes)
  }
  if (par->keep_nodes) {
    for (int i = 0; i < 2; i++) {
      dev(od->d_pk2[i], (size_t)B * od->cap_points * 16);
      dev(od->d_npk2[i], (size_t)B * 4);
    }
    dev(od->d_mot, (size_t)B * 3 * sizeof(double));
    pin(od->h_mot, (size_t)B * 3 * sizeof(double));
    pin(od->h_npk, (size_t)B * 4);
  }
  od->last_slab.assign(B, -1);
  for (int i = 0; i < 2; i++) {
    dev(od->d_xyzi2[i], (size_t)B * od->cap_points * 16);
    dev(od->d_npts2[i], (size_t)B * 4);
  }
  ok = ok && (od->ev_results = make_event(hipEventDisableTiming)) && (od->ev_jobs = make_event(hipEventDisableTiming)) &&
       (od->ev_surf_jobs = make_event(hipEventDisableTiming)) && (od->ev_offsets[0] = make_event(hipEventDisableTiming)) &&
       (od->ev_offsets[1] = make_event(hipEventDisableTiming)) && (od->ev_frame = make_event(hipEventDisableTiming)) &&
       (od->copy_stream = make_stream_nonblocking());
  od->readback_on_copy_stream = ctx->stream != nullptr && ctx->stream != hipStreamLegacy && ctx->stream != hipStreamPerThread;
  dev(od->d_slabs, (size_t)B * od->slabs_per_stream * od->slab_bytes);
  dev(od->d_surf_jobs, (size_t)B * cfear_surface_job_bytes());
  // records are laid out at the stride of the window (process_frame); rounded up to 16 bytes, the stride of the longest
  // window is 8 bytes MORE than a whole record
  const size_t reg_job_room = std::max(sizeof(RegJob), reg_job_stride(par->submap_scan_size + 1));
  dev(od->d_reg_jobs, (size_t)B * reg_job_room);
  od->out_bytes = (size_t)B * (sizeof(cfear_reg_result) + 12);
  dev(od->d_out, od->out_bytes);
  pin(od->h_out, od->out_bytes);
  if (ok) {
    auto carve = [&](char* base) {
      struct P { cfear_reg_result* r; int32_t *st, *nc, *np; } q;
      q.r = (cfear_reg_result*)base;
      q.st = (int32_t*)(base + (size_t)B * sizeof(cfear_reg_result));
      q.nc = q.st + B; q.np = q.nc + B;
      return q;
    };
    const auto d = carve(od->d_out.get()), h = carve(od->h_out.get());
    od->d_results = d.r; od->d_status = d.st; od->d_ncells = d.nc; od->d_npts_out = d.np;
    od->h_results = h.r; od->h_status = h.st; od->h_ncells = h.nc; od->h_npts = h.np;
  }
  dev(od->d_surf_scratch, (size_t)B * cfear_surface_scratch_bytes(od->cap_points));
  dev(od->d_reg_scratch, (size_t)B * reg_scratch_bytes(par->submap_scan_size * od->cell_cap));
  pin(od->h_surf_jobs, (size_t)B * cfear_surface_job_bytes());
  pin(od->h_reg_jobs, (size_t)B * reg_job_room);
  if (par->estimate_cov_by_sampling) {
    od->fit.prepare(par->cov_sampling.samples_per_axis, par->cov_sampling.xy_range * 0.5, par->cov_sampling.yaw_range * 0.5);
    dev(od->d_samples, (size_t)B * od->fit.m * sizeof(cfear_reg_result));
    pin(od->h_samples, (size_t)B * od->fit.m * sizeof(cfear_reg_result));
  }
  od->cov.assign((size_t)B * 36, 0.0);
  for (int b = 0; b < B; b++)
    for (int k = 0; k < 6; k++) od->cov[(size_t)b * 36 + k * 7] = 1.0;       // cov_current = Identity (:36)
  od->cov_sampled.assign(B, 0);
  if (!ok) return cfear_set_error(ctx, CFEAR_ERR_HIP, "odometry buffers: allocation failed");
  od->streams.resize(B);
  od->cost_est.assign(B, 0.0);
  od->views.resize((size_t)B * od->slabs_per_stream);
  for (int b = 0; b < B; b++) {
    for (int s = 0; s < od->slabs_per_stream; s++) {
      od->views[(size_t)b * od->slabs_per_stream + s] =
          cfear_scan_view(od->d_slabs.get() + ((size_t)b * od->slabs_per_stream + s) * od->slab_bytes, od->cell_cap);
      od->streams[b].free_slabs.push_back(od->slabs_per_stream - 1 - s);
    }
  }
  *out = od.release();
  return CFEAR_OK;
}

// ---- F: filter (radar_driver.cpp:48-73) of one batch of polar images into filter buffer `buf` -------
static int run_filter_enqueue(cfear_odometry* od, const uint8_t* polar, int buf, const int64_t* offsets) {
  cfear_ctx* ctx = od->ctx;
  const int B = od->n_streams, rows = od->desc.rows, k = od->par.kstrong.k_strongest;
  const cfear_odometry_params& par = od->par;
  const uint8_t* d_polar = polar;
  cfear_polar_desc dd = od->in_desc;
  const int64_t* d_offsets = nullptr;
  if (offsets) {
    if (!od->fused || par.rotate_ccw || !cfear_is_device_ptr(polar))
      return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "image offsets need device images, the k-strongest filter "
                             "(k <= 64, no keep_nodes) and rows = azimuths");
    // The table goes up on the copy stream, so the sweep does not queue behind a copy on its own stream.  Reuse: filter
    // buffer `buf` was last swept two frames ago (the previous frame, if no prefetch ran in between).  That sweep stands in
    // front of its frame's surface kernels and matcher on the kernel stream, and the host has waited for that frame's
    // ev_results since -- so neither d_offsets2[buf] nor this half of h_offsets (whose upload that sweep waited for) is
    // still in use.  The other half of both belongs to the frame in flight and is not touched.
    int64_t* h = od->h_offsets.get() + (size_t)buf * B;
    memcpy(h, offsets, (size_t)B * 8);
    CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(od->d_offsets2[buf].get(), h, (size_t)B * 8, hipMemcpyHostToDevice, od->copy_stream.get()));
    CFEAR_HIP_CHECK(ctx, hipEventRecord(od->ev_offsets[buf].get(), od->copy_stream.get()));
    CFEAR_HIP_CHECK(ctx, hipStreamWaitEvent(ctx->stream, od->ev_offsets[buf].get(), 0));
    d_offsets = od->d_offsets2[buf].get();
  }
  if (!cfear_is_device_ptr(polar)) {
    const size_t img_bytes = (size_t)od->in_desc.rows * od->in_desc.stride;
    if (!od->d_polar && !(od->d_polar = dev_alloc<uint8_t>(img_bytes * B))) return cfear_set_error(ctx, CFEAR_ERR_HIP, "staging allocation failed");
    const int64_t bs = B > 1 ? od->in_desc.batch_stride : (int64_t)img_bytes;
    if (bs == (int64_t)img_bytes) {          // a dense batch crosses PCIe as one copy
      CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(od->d_polar.get(), polar, img_bytes * B, hipMemcpyHostToDevice, ctx->stream));
    } else {
      for (int b = 0; b < B; b++)
        CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(od->d_polar.get() + (size_t)b * img_bytes, polar + (size_t)b * bs, img_bytes,
                                            hipMemcpyHostToDevice, ctx->stream));
    }
    d_polar = od->d_polar.get();
    dd.batch_stride = (int64_t)img_bytes;
  }
  od->decode_measured[buf] = false;
  if (od->fused_decode && od->decode_hold > 0) od->decode_hold--;
  else if (od->fused_decode && cfear_kstrong_cols_preferred(d_polar, &dd, &par.kstrong)) {
    cfear_kstrong_params kp = par.kstrong;
    kp.want_peaks = 0;
    cfear_kstrong_fused fz;
    fz.row_keys = od->d_rowpts2[buf].get();
    fz.row_valid = od->d_rowcnt2[buf].get();
    fz.cand_stats = od->d_decode_stats.get() + 64 * buf;
    const int rc = cfear_kstrong_cols_device(ctx, d_polar, &dd, &kp, &fz);
    if (rc != CFEAR_OK) return rc;
    CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(od->h_decode_stats.get() + 64 * buf, fz.cand_stats, 64 * 4, hipMemcpyDeviceToHost, ctx->stream));
    od->decode_measured[buf] = true;                         // read once this buffer's frame has been synchronised
    return CFEAR_OK;
  }
  // CA-CFAR on [range bins][azimuths] sweeps: the decode fused into the filter (cacfar_cols_kernel), one pass over the image
  // instead of three (CFEAR_OPT_FUSED_DECODE = 0 keeps rotate + cacfar_rows, for A/B runs and the tests that compare the two)
  if (par.rotate_ccw && od->fused_cfar && ctx->opt[CFEAR_OPT_FUSED_DECODE] != 0 && B >= 16 &&
      cfear_cacfar_cols_supported(d_polar, &dd, &par.cacfar)) {
    cfear_cacfar_params cp = par.cacfar;
    cfear_cacfar_fused fz;
    fz.row_keys = od->d_rowpts2[buf].get(); fz.row_cnt = od->d_rowcnt2[buf].get(); fz.kcap = od->row_k; fz.bins_major = true;
    return cfear_cacfar_device(ctx, d_polar, &dd, &cp, nullptr, nullptr, od->cap_points, nullptr, &fz);
  }
  if (par.rotate_ccw) {
    const size_t rot_bytes = (size_t)od->desc.rows * od->desc.stride;
    if (!od->d_rot && !(od->d_rot = dev_alloc<uint8_t>(rot_bytes * B))) return cfear_set_error(ctx, CFEAR_ERR_HIP, "rotation buffer allocation failed");
    const int rc = cfear_rotate_ccw_device(ctx, d_polar, &dd, od->d_rot.get(), od->desc.stride, (int64_t)rot_bytes);
    if (rc != CFEAR_OK) return rc;
    d_polar = od->d_rot.get();
    dd = od->desc;
  }
  if (par.filter_type == CFEAR_FILTER_CACFAR) {
    cfear_cacfar_params cp = par.cacfar;
    if (par.keep_nodes)    // CA-CFAR produces no peaks cloud (radar_driver.cpp:52-56)
      CFEAR_HIP_CHECK(ctx, hipMemsetAsync(od->d_npk2[buf].get(), 0, (size_t)B * 4, ctx->stream));
    if (od->fused_cfar) {
      cfear_cacfar_fused fz;
      fz.row_keys = od->d_rowpts2[buf].get(); fz.row_cnt = od->d_rowcnt2[buf].get(); fz.kcap = od->row_k;
      return cfear_cacfar_device(ctx, d_polar, &dd, &cp, nullptr, nullptr, od->cap_points, nullptr, &fz);
    }
    return cfear_cacfar_device(ctx, d_polar, &dd, &cp, od->d_xyzi2[buf].get(), od->d_npts2[buf].get(), od->cap_points, nullptr);
  }
  const size_t nsel = (size_t)B * rows * k;
  cfear_kstrong_out o{};
  if (od->fused) {
    cfear_kstrong_params kp = par.kstrong;
    kp.want_peaks = 0;
    cfear_kstrong_fused fz;
    fz.row_keys = od->d_rowpts2[buf].get();
    fz.row_valid = od->d_rowcnt2[buf].get();
    fz.image_offsets = d_offsets;
    return cfear_kstrong_device(ctx, d_polar, &dd, &kp, &o, par.rotate_ccw != 0, &fz);
  }
  o.sel_range = (int32_t*)od->d_sel.get();
  o.sel_intensity = (uint8_t*)(od->d_sel.get() + nsel * 4);
  o.sel_count = (int32_t*)(od->d_sel.get() + nsel * 4 + (nsel + 255) / 256 * 256);
  o.xyzi = od->d_xyzi2[buf].get();
  o.n_points = od->d_npts2[buf].get();
  cfear_kstrong_params kp = par.kstrong;
  kp.want_peaks = 0;     // the peaks cloud feeds CorAl / Scan Context, not the matcher
  if (par.keep_nodes) {  // ... unless the caller builds graph nodes from this pipeline (RadarScan::cloud_peaks_)
    kp.want_peaks = 1;
    o.is_peak = (uint8_t*)(od->d_sel.get() + nsel * 4 + (nsel + 255) / 256 * 256 + (size_t)B * rows * 4 + 256);
    o.xyzi_peaks = od->d_pk2[buf].get();
    o.n_peaks = od->d_npk2[buf].get();
  }
  if (od->cap_points != rows * k)
    return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "rows*k = %d exceeds %d points per scan", rows * k, od->cap_points);
  // the rotated buffer is a padded copy of what the reference holds as a dense cv::Mat: AxialNonMaxSupress's reads
  // past a row end must land on the next row's first bins (radar_filters.cpp:238-298), not on the padding
  return cfear_kstrong_device(ctx, d_polar, &dd, &kp, &o, par.rotate_ccw != 0);
}

static int run_filter(cfear_odometry* od, const uint8_t* polar, int buf, const int64_t* offsets = nullptr) {
  const int rc = run_filter_enqueue(od, polar, buf, offsets);
  // an error behind the offset upload: the caller may come back with other offsets before a frame has been synchronised
  if (rc != CFEAR_OK && offsets) drain_streams(od);
  return rc;
}

extern "C" int cfear_odometry_get_covariance(cfear_odometry* od, double* cov, int32_t* sampled) {
  if (!od || !cov) return CFEAR_ERR_INVALID_ARGUMENT;
  memcpy(cov, od->cov.data(), od->cov.size() * sizeof(double));
  if (sampled) memcpy(sampled, od->cov_sampled.data(), od->cov_sampled.size() * sizeof(int32_t));
  return CFEAR_OK;
}

extern "C" int cfear_odometry_process(cfear_odometry* od, const uint8_t* polar, cfear_frame_info* info) {
  return cfear_odometry_process_prefetch(od, polar, nullptr, info);
}

static int process_frame(cfear_odometry* od, const uint8_t* polar, const uint8_t* polar_next, const cfear_sc_cloud* clouds,
                         const cfear_sc_cloud* peaks, cfear_frame_info* info, const int64_t* offsets = nullptr,
                         const int64_t* offsets_next = nullptr);

extern "C" int cfear_odometry_process_offsets(cfear_odometry* od, const uint8_t* base, const int64_t* offsets,
                                              const int64_t* offsets_next, cfear_frame_info* info) {
  if (!od || !base || !offsets || !info) return CFEAR_ERR_INVALID_ARGUMENT;
  return process_frame(od, base, offsets_next ? base : nullptr, nullptr, nullptr, info, offsets, offsets_next);
}

extern "C" int cfear_odometry_discard_prefetch(cfear_odometry* od) {
  if (!od) return CFEAR_ERR_INVALID_ARGUMENT;
  od->prefetched = nullptr;
  od->prefetched_offsets.clear();
  // the discarded sweep and its offset upload may still be in flight, and the caller is about to reuse what they read
  (void)hipSetDevice(od->ctx->device);
  drain_streams(od);
  return CFEAR_OK;
}

extern "C" int cfear_odometry_process_prefetch(cfear_odometry* od, const uint8_t* polar, const uint8_t* polar_next,
                                               cfear_frame_info* info) {
  if (!od || !polar || !info) return CFEAR_ERR_INVALID_ARGUMENT;
  return process_frame(od, polar, polar_next, nullptr, nullptr, info);
}

// OdometryKeyframeFuser::pointcloudCallback(cloud, cloud_peaks, ...) (odometrykeyframefuser.cpp:413-426): the caller's
// own driver has already filtered the sweep; the clouds enter the pipeline where the filter would have left them.
extern "C" int cfear_odometry_process_clouds(cfear_odometry* od, const cfear_sc_cloud* clouds, const cfear_sc_cloud* peaks,
                                             cfear_frame_info* info) {
  if (!od || !clouds || !info) return CFEAR_ERR_INVALID_ARGUMENT;
  return process_frame(od, nullptr, nullptr, clouds, peaks, info);
}

// uploads one cloud per stream into the frame buffers `buf` (what run_filter would have produced)
static int load_clouds(cfear_odometry* od, const cfear_sc_cloud* clouds, float* d_dst, int32_t* d_n, int32_t* h_tmp) {
  cfear_ctx* ctx = od->ctx;
  const int B = od->n_streams;
  for (int b = 0; b < B; b++) {
    const int n = clouds ? clouds[b].n : 0;
    if (n < 0 || (n > 0 && !clouds[b].xyzi)) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "stream %d: null cloud", b);
    if (n > od->cap_points) return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "stream %d: %d points > %d", b, n, od->cap_points);
    h_tmp[b] = n;
    if (n > 0) {
      const bool dev = cfear_is_device_ptr(clouds[b].xyzi);
      CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(d_dst + (size_t)b * od->cap_points * 4, clouds[b].xyzi, (size_t)n * 16,
                                          dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    }
  }
  CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(d_n, h_tmp, (size_t)B * 4, hipMemcpyHostToDevice, ctx->stream));
  // h_tmp is reused by the next load / the read-back of this frame: make sure the copy has left the host buffer
  CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return CFEAR_OK;
}

namespace {
struct HostTimeline {          // CFEAR_OPT_HOST_TIMELINE = 1: where the host spends a frame (printed every 256 calls)
  bool on = false;
  double acc[8] = {0};
  int calls = 0;
  std::chrono::steady_clock::time_point last, exit_t;
  bool have_exit = false;
  void start() {
    if (!on) return;
    last = std::chrono::steady_clock::now();
    if (have_exit) acc[6] += std::chrono::duration<double, std::micro>(last - exit_t).count();
  }
  void mark(int k) {
    if (!on) return;
    const auto t = std::chrono::steady_clock::now();
    acc[k] += std::chrono::duration<double, std::micro>(t - last).count();
    last = t;
  }
  void end() {
    if (!on) return;
    exit_t = std::chrono::steady_clock::now(); have_exit = true;
    if (++calls % 256 == 0) {
      fprintf(stderr, "host us/frame: surf jobs+launch %.0f | reg jobs %.0f | enqueue rest %.0f | wait results %.0f | policy %.0f | outside the call %.0f\n",
              acc[0] / 256, acc[1] / 256, acc[2] / 256, acc[3] / 256, acc[4] / 256, acc[6] / 256);
      for (double& a : acc) a = 0;
    }
  }
};
HostTimeline g_tl;
}  // namespace

static int process_frame(cfear_odometry* od, const uint8_t* polar, const uint8_t* polar_next, const cfear_sc_cloud* clouds,
                         const cfear_sc_cloud* peaks, cfear_frame_info* info, const int64_t* offsets, const int64_t* offsets_next) {
  cfear_ctx* ctx = od->ctx;
  g_tl.on = ctx->opt[CFEAR_OPT_HOST_TIMELINE] != 0;
  g_tl.start();
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int B = od->n_streams;
  const cfear_odometry_params& par = od->par;
  int rc;
  if (clouds) {                                    // filtered clouds from the caller: no filter, no prefetch
    od->prefetched = nullptr;
    rc = load_clouds(od, clouds, od->d_xyzi2[od->cur_buf].get(), od->d_npts2[od->cur_buf].get(), od->h_npts);
    if (rc != CFEAR_OK) return rc;
    if (par.keep_nodes) {
      rc = load_clouds(od, peaks, od->d_pk2[od->cur_buf].get(), od->d_npk2[od->cur_buf].get(), od->h_npk.get());
      if (rc != CFEAR_OK) return rc;
    }
  } else if (od->prefetched == polar &&
             (offsets ? (od->prefetched_offsets.size() == (size_t)B &&
                         memcmp(od->prefetched_offsets.data(), offsets, (size_t)B * 8) == 0)
                      : od->prefetched_offsets.empty())) {   // this frame's filter already ran (or is running)
    od->cur_buf ^= 1;
  } else {
    rc = run_filter(od, polar, od->cur_buf, offsets);
    if (rc != CFEAR_OK) return rc;
  }
  od->prefetched = nullptr;
  od->prefetched_offsets.clear();
  od->d_xyzi = od->d_xyzi2[od->cur_buf].get();
  od->d_npts = od->d_npts2[od->cur_buf].get();
  od->d_pk = od->d_pk2[od->cur_buf].get();
  od->d_npk = od->d_npk2[od->cur_buf].get();
  const bool rows_mode = (od->fused || od->fused_cfar) && !clouds;     // the filter left per-row points: the surface kernel compacts them
  // ---- C + N: compensate with the previous motion, surface points (odometrykeyframefuser.cpp:146-161)
  const size_t sjb = cfear_surface_job_bytes();
  for (int b = 0; b < B; b++)
    if (od->streams[b].free_slabs.empty()) {
      drain_streams(od);           // this frame's sweep and its offset upload are in flight; the next call reuses their buffer
      return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "stream %d: no free scan slab", b);
    }
  for (int b = 0; b < B; b++) {
    StreamState& st = od->streams[b];
    st.cur_slab = st.free_slabs.back();
    st.free_slabs.pop_back();
    double mot[3];
    aff_to_xyt(st.Tmot, mot);                                     // Compensate(cloud, TprevMot, ccw)
    od->last_slab[b] = st.cur_slab;
    if (par.keep_nodes) { od->h_mot[3 * b] = mot[0]; od->h_mot[3 * b + 1] = mot[1]; od->h_mot[3 * b + 2] = mot[2]; }
    if (rows_mode)
      cfear_surface_fill_job_rows(od->h_surf_jobs.get() + (size_t)b * sjb, od->d_xyzi + (size_t)b * od->cap_points * 4, od->d_npts_out + b,
                                  od->d_rowpts2[od->cur_buf].get() + (size_t)b * od->desc.rows * od->row_k,
                                  od->d_rowcnt2[od->cur_buf].get() + (size_t)b * od->desc.rows * 2, od->desc.rows,
                                  od->row_k, par.compensate, mot,
                                  od->views[(size_t)b * od->slabs_per_stream + st.cur_slab]);
    else
      cfear_surface_fill_job(od->h_surf_jobs.get() + (size_t)b * sjb, od->d_xyzi + (size_t)b * od->cap_points * 4,
                             od->d_npts + b, 0, par.compensate, mot, od->views[(size_t)b * od->slabs_per_stream + st.cur_slab]);
  }
  // From here on every stream holds a slab: an error exit must hand the slabs back, or submap_scan_size + 2 failed
  // calls would drain a stream's free list.  It also leaves both streams idle: the next call fills the pinned tables and
  // uploads them on the copy stream at once, which only this frame's ev_results would otherwise have made safe.
  auto fail = [&](int code) {
    drain_streams(od);
    for (int b = 0; b < B; b++) {
      StreamState& st = od->streams[b];
      if (st.cur_slab >= 0) { st.free_slabs.push_back(st.cur_slab); st.cur_slab = -1; }
    }
    return code;
  };
#define OD_CHECK(expr)                                                                                        \
  do {                                                                                                        \
    hipError_t _e = (expr);                                                                                   \
    if (_e != hipSuccess)                                                                                     \
      return fail(cfear_set_error(ctx, CFEAR_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__)); \
  } while (0)
  // The table goes up on the copy stream now, while the sweep (prefetched a frame ago) may still run; the kernel stream
  // waits for it in front of the surface kernels.  Reuse: d_surf_jobs was last read by the previous frame's surface kernels,
  // h_surf_jobs by the upload those kernels waited for; they stand in front of that frame's matcher on the kernel stream, and
  // the host has waited for that frame's ev_results (or, after an error, for both streams) since.
  OD_CHECK(hipMemcpyAsync(od->d_surf_jobs.get(), od->h_surf_jobs.get(), (size_t)B * sjb, hipMemcpyHostToDevice, od->copy_stream.get()));
  OD_CHECK(hipEventRecord(od->ev_surf_jobs.get(), od->copy_stream.get()));
  OD_CHECK(hipStreamWaitEvent(ctx->stream, od->ev_surf_jobs.get(), 0));
  cfear_feature_params fp{};
  fp.radius = par.res;
  fp.downsample_factor = par.downsample_factor;
  fp.origin[0] = fp.origin[1] = 0.0;                              // Eigen::Vector2d(0,0), :161
  fp.weight_intensity = par.weight_intensity;
  fp.ccw = par.radar_ccw;
  cfear_surface_polar sp;
  if (rows_mode) {
    double *d_cos = nullptr, *d_sin = nullptr;
    rc = cfear_trig_tables(ctx, od->desc.rows, &d_cos, &d_sin);
    if (rc != CFEAR_OK) return fail(rc);
    sp.cos_t = d_cos; sp.sin_t = d_sin;
    sp.rows = od->desc.rows; sp.k = od->row_k;
    if (od->fused_cfar) {                 // cfar.cpp:43: range = range_resolution_ * double(range_bin)
      sp.range_res = (double)par.cacfar.range_res; sp.range_off = 0.0;
    } else {                              // radar_filters.cpp:324: range_res / 2 + range_res * bin
      sp.range_res = (double)par.kstrong.range_res; sp.range_off = sp.range_res / 2.0;
    }
  }
  rc = cfear_surface_launch(ctx, od->d_surf_jobs.get(), B, &fp, od->d_surf_scratch.get(), od->d_status, od->d_ncells, od->cell_cap, od->cap_points, rows_mode ? &sp : nullptr);
  if (rc != CFEAR_OK) return fail(rc);
  g_tl.mark(0);
  // ---- M: the registration jobs depend on host state only: they are built and uploaded (copy stream) while the
  //      surface kernels, already enqueued above, run -- 2.3 KB per stream, ~0.3 ms of host time for 2048 streams
  //      that would otherwise sit between the sweep and the surface kernels (:164-186) ------------------------
  const size_t rjb = reg_job_stride(par.submap_scan_size + 1);   // records cover the keyframe window + the new scan
  int n_jobs = 0;
  std::vector<ScanView> views(kRegMaxScans);
  std::vector<double> poses(3 * (size_t)kRegMaxScans);
  // Longest first: registrations differ by ~2x in work (cells, outer and LM iterations), and 2048 of them over the 512
  // workgroup slots of the chip end with whatever the last-started ones need.  A stream's previous registration is a
  // good estimate of its next one, so the batch is ordered by it (the job index is only a slot in the batch) -- in
  // four classes by the quartiles of the estimate, streams in index order inside a class: a full sort walked the
  // stream records in random order and cost more host time than the kernel saved.
  std::vector<double>& est = od->cost_est;
  // ... plus a class of its own for the heaviest 3 %: the registrations whose correspondences overflow the LDS arrays of
  // the matcher run ~1.5 x as long as the rest and must not be the last ones to start
  double cut[4] = {0.0, 0.0, 0.0, 0.0};
  {
    std::vector<double>& tmp = od->cost_tmp;
    tmp.assign(est.begin(), est.end());
    if (B >= 8) {
      const size_t ks[4] = {(size_t)B * 97 / 100, (size_t)B * 3 / 4, (size_t)B / 2, (size_t)B / 4};   // descending cuts
      for (int q = 0; q < 4; q++) {
        std::nth_element(tmp.begin(), tmp.begin() + ks[q], tmp.end());
        cut[q] = tmp[ks[q]];
      }
    }
  }
  // one pass for the guess and the class, a prefix over the five classes, one pass that writes every record at its slot
  // (five passes over the stream records -- one per class -- were 0.5 ms of host time per 4096 streams)
  std::vector<int>& slot = od->job_slot;
  slot.assign((size_t)B, -1);
  int cls_n[5] = {0, 0, 0, 0, 0};
  for (int b = 0; b < B; b++) {
    StreamState& st = od->streams[b];
    frame_policy_guess(st, par);                                              // :164-168
    st.job = -1;
    if (st.keyframes.empty()) continue;                                       // :171-177 first frame: no registration
    const double e = est[b];
    const int c = e >= cut[0] ? 0 : e >= cut[1] ? 1 : e >= cut[2] ? 2 : e >= cut[3] ? 3 : 4;
    slot[b] = c | (cls_n[c]++ << 3);                                          // class, rank inside it (stream order)
  }
  int cls_off[5];
  for (int c = 0; c < 5; c++) { cls_off[c] = n_jobs; n_jobs += cls_n[c]; }
  for (int b = 0; b < B; b++) {
    if (slot[b] < 0) continue;
    StreamState& st = od->streams[b];
    const int ns = (int)st.keyframes.size() + 1;                              // FormatScans :478-494
    for (int i = 0; i < ns - 1; i++) {
      views[i] = od->views[(size_t)b * od->slabs_per_stream + st.keyframes[i].slab];
      aff_to_xyt(st.keyframes[i].pose, &poses[3 * i]);
    }
    views[ns - 1] = od->views[(size_t)b * od->slabs_per_stream + st.cur_slab];
    aff_to_xyt(st.Tguess, &poses[3 * (ns - 1)]);
    st.job = cls_off[slot[b] & 7] + (slot[b] >> 3);
    cfear_reg_fill_job(od->h_reg_jobs.get() + (size_t)st.job * rjb, views.data(), ns, poses.data());
  }
  if (n_jobs > 0) {
    OD_CHECK(hipMemcpyAsync(od->d_reg_jobs.get(), od->h_reg_jobs.get(), (size_t)n_jobs * rjb, hipMemcpyHostToDevice, od->copy_stream.get()));
    OD_CHECK(hipEventRecord(od->ev_jobs.get(), od->copy_stream.get()));
  }
  g_tl.mark(1);
  // the matcher over this frame's jobs (+ the cost samples around its results); big_pass adds the large forms
  auto launch_register = [&](bool big_pass) -> int {
    RegLaunchHint hint;
    hint.big_pass = big_pass;
    int lrc = cfear_register_launch(ctx, od->d_reg_jobs.get(), n_jobs, &par.reg, par.submap_scan_size * od->cell_cap,
                                    od->d_reg_scratch.get(), od->d_results, nullptr, rjb, hint);
    if (lrc != CFEAR_OK) return lrc;
    if (par.estimate_cov_by_sampling) {
      // approximateCovarianceBySampling (:203-208, 261-316): n^3 GetCost evaluations around the pose the
      // registration just produced; pose and leftover itr_ are read from d_results on the device, so no host
      // round trip separates the two launches.
      RegCostMode mode;
      mode.samples_per_axis = od->fit.n;
      mode.n_samples = od->fit.m;
      mode.xy_half = par.cov_sampling.xy_range * 0.5;
      mode.yaw_half = par.cov_sampling.yaw_range * 0.5;
      mode.blocks_per_job = 1;                                    // one workgroup per stream: its scratch is reused
      mode.prior = od->d_results;
      lrc = cfear_register_launch(ctx, od->d_reg_jobs.get(), n_jobs, &par.reg, par.submap_scan_size * od->cell_cap,
                                  od->d_reg_scratch.get(), od->d_samples.get(), &mode, rjb, hint);
      if (lrc != CFEAR_OK) return lrc;
    }
    return CFEAR_OK;
  };
  auto read_samples = [&](hipStream_t s) -> int {
    if (!par.estimate_cov_by_sampling || n_jobs == 0) return CFEAR_OK;
    if (hipMemcpyAsync(od->h_samples.get(), od->d_samples.get(), (size_t)n_jobs * od->fit.m * sizeof(cfear_reg_result),
                       hipMemcpyDeviceToHost, s) != hipSuccess)
      return cfear_set_error(ctx, CFEAR_ERR_HIP, "sample read-back failed");
    return CFEAR_OK;
  };
  const bool launched_big = od->big_regs > 0;
  if (n_jobs > 0) {
    OD_CHECK(hipStreamWaitEvent(ctx->stream, od->ev_jobs.get(), 0));
    rc = launch_register(launched_big);
    if (rc != CFEAR_OK) return fail(rc);
  }
  if (par.keep_nodes) {
    // Compensate(*cloud_peaks, TprevMot, ccw) (odometrykeyframefuser.cpp:149): off the critical path, behind the matcher
    if (par.compensate) {
      OD_CHECK(hipMemcpyAsync(od->d_mot.get(), od->h_mot.get(), (size_t)B * 3 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
      rc = cfear_compensate_batch_device(ctx, od->d_pk, (size_t)od->cap_points, od->d_npk, od->d_mot.get(), B, od->cap_points, par.radar_ccw);
      if (rc != CFEAR_OK) return fail(rc);
    }
  }
  if (!rows_mode)     // the point counts came from the filter / the caller: bring them into the block first
    OD_CHECK(hipMemcpyAsync(od->d_npts_out, od->d_npts, (size_t)B * 4, hipMemcpyDeviceToDevice, ctx->stream));
  // What the host reads of the frame, in stream order behind the frame's last kernel-stream work; ev_results behind it.
  auto read_back = [&](hipStream_t s) -> int {
    const int src = read_samples(s);
    if (src != CFEAR_OK) return src;
    hipError_t e = hipSuccess;
    if (par.keep_nodes) e = hipMemcpyAsync(od->h_npk.get(), od->d_npk, (size_t)B * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(od->h_out.get(), od->d_out.get(), od->out_bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipEventRecord(od->ev_results.get(), s);
    return e == hipSuccess ? CFEAR_OK : cfear_set_error(ctx, CFEAR_ERR_HIP, "result read-back failed: %s", hipGetErrorString(e));
  };
  // The frame's kernel-stream work ends here.  The read-back comes down on the copy stream (below, behind the prefetch), so
  // the next sweep follows the matcher with no copy in between -- or here, where the kernel stream is a handle.
  if (od->readback_on_copy_stream) {
    OD_CHECK(hipEventRecord(od->ev_frame.get(), ctx->stream));
  } else {
    rc = read_back(ctx->stream);
    if (rc != CFEAR_OK) return fail(rc);
  }
  int prefetch_rc = CFEAR_OK;
  if (polar_next) {
    // (Tried twice: the sweep on its own low-priority stream.  Enqueued ahead of this frame's kernels it simply ran first
    // -- every kernel of the path fills the chip, the sweep holds all vector registers of its SIMDs and the matcher all
    // LDS of its CUs, so nothing co-resides: 2.51 ms per frame batch instead of 2.19.  Gated to start with the matcher,
    // to fill the ~0.2 ms in which the last uneven registrations leave CUs idle, its small workgroups took the LDS the
    // next 80 KB registration needed on every CU that drained: matcher 0.98 -> 1.47 ms, sweep 0.52 -> 1.32 ms, 2.68 ms
    // per frame batch.  Round 4, with 52 KB / 127-VGPR matcher workgroups -- three per CU, so that a finished one
    // leaves room for the sweep beside the other two -- and the sweep enqueued behind the surface kernels on a stream of
    // its own: matcher 1.35 -> 2.40 ms, sweep 1.12 -> 1.89 ms, 4.2 ms per 4096-stream frame batch instead of 3.5.  The
    // sweep's short-lived workgroups keep taking the LDS a registration needs; the two do not share a CU gracefully.)
    // The next frame's filter needs no state of this frame: enqueue it now so the GPU sweeps the next
    // polar batch while the host applies the keyframe policy below.
    // A failed prefetch does not throw this frame away: its kernels already ran and its policy is applied below;
    // the error is reported after the frame is complete and the next call simply filters again.
    prefetch_rc = run_filter(od, polar_next, od->cur_buf ^ 1, offsets_next);
    if (prefetch_rc == CFEAR_OK) {
      od->prefetched = polar_next;
      if (offsets_next) od->prefetched_offsets.assign(offsets_next, offsets_next + B);
    }
  }
  // The read-back is enqueued behind the prefetch so that the next sweep's offset upload, on the same copy stream, does
  // not wait for this frame's matcher.  Reuse: d_out, d_samples and d_npk are written next by the NEXT frame's surface
  // kernels, matcher and filter of this buffer, none of which is enqueued before the host has passed ev_results below (the
  // prefetched sweep writes the other filter buffer only); h_out, h_samples and h_npk were last written by the previous
  // frame's read-back, which the host waited for in that frame.
  if (od->readback_on_copy_stream) {
    OD_CHECK(hipStreamWaitEvent(od->copy_stream.get(), od->ev_frame.get(), 0));
    rc = read_back(od->copy_stream.get());
    if (rc != CFEAR_OK) return fail(rc);
  }
  g_tl.mark(2);
  OD_CHECK(hipEventSynchronize(od->ev_results.get()));
  g_tl.mark(3);
  if (n_jobs > 0 && !launched_big) {
    // A registration too large for the first form of a launch WITHOUT the large forms comes back as CFEAR_ERR_CAPACITY with
    // `reserved` set when a larger form holds it (matcher_kernel): the first dense frame of a run.  Run the frame's jobs again
    // with the large forms on (the job records are still on the device; everything else of the frame is unaffected) and keep
    // them on for the frames to come (big_regs below) -- without this the stream ran on its motion guess for ever.
    bool retry = false;
    for (int j = 0; j < n_jobs && !retry; j++) retry = od->h_results[j].status == CFEAR_ERR_CAPACITY && od->h_results[j].reserved != 0.0;
    if (retry) {
      rc = launch_register(true);
      if (rc != CFEAR_OK) return fail(rc);
      rc = read_samples(ctx->stream);
      if (rc != CFEAR_OK) return fail(rc);
      OD_CHECK(hipMemcpyAsync(od->h_results, od->d_results, (size_t)n_jobs * sizeof(cfear_reg_result), hipMemcpyDeviceToHost, ctx->stream));
      OD_CHECK(hipStreamSynchronize(ctx->stream));
    }
  }
  if (od->decode_measured[od->cur_buf]) {                  // this frame's sweeps went through the fused decode: how dense were they?
    od->decode_measured[od->cur_buf] = false;
    uint64_t cands = 0;
    for (int k = 0; k < 64; k++) cands += od->h_decode_stats[64 * od->cur_buf + k];
    if ((double)cands > kDecodeDense * (double)B * (double)od->desc.rows) od->decode_hold = kDecodeHold;
  }
  // ---- frame policy (:195-257) ------------------------------------------------------------------
  int first_error = CFEAR_OK;
  bool saw_big = false;
  for (int b = 0; b < B; b++) {
    StreamState& st = od->streams[b];
    FrameOutcome fo;
    fo.n_points = od->h_npts[b]; fo.n_cells = od->h_ncells[b]; fo.status = od->h_status[b];
    if (st.job >= 0) {
      fo.rr = od->h_results + st.job;
      if (par.estimate_cov_by_sampling) fo.samples = od->h_samples.get() + (size_t)st.job * od->fit.m;
    }
    const int src = frame_policy_apply(st, par, fo, &od->fit, od->cov.data() + (size_t)b * 36, &od->cov_sampled[b], &od->cost_est[b],
                                       &saw_big, info[b]);
    if (src != CFEAR_OK && first_error == CFEAR_OK)
      first_error = cfear_set_error(ctx, src, "stream %d: surface points failed (%s)", b, cfear_status_string(src));
  }
  for (int b = 0; b < B; b++) od->streams[b].cur_slab = -1;      // every slab is a keyframe or back on the free list
#undef OD_CHECK
  od->big_regs = saw_big ? 64 : std::max(0, od->big_regs - 1);     // large scans come in runs: keep the second launch for 64 frames
  g_tl.mark(4);
  g_tl.end();
  return first_error != CFEAR_OK ? first_error : prefetch_rc;
}

// ---- graph-node export: the RadarScan of the last processed frame (types.h:119-122; scan_ at
// odometrykeyframefuser.cpp:172, 244) --------------------------------------------------------------------------
extern "C" int cfear_odometry_get_scan(cfear_odometry* od, int32_t stream, cfear_scan** out) {
  if (!od || !out || stream < 0 || stream >= od->n_streams) return CFEAR_ERR_INVALID_ARGUMENT;
  cfear_ctx* ctx = od->ctx;
  *out = nullptr;
  if (od->last_slab[stream] < 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "stream %d: no frame processed yet", stream);
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const ScanView& v = od->views[(size_t)stream * od->slabs_per_stream + od->last_slab[stream]];
  const int rc = cfear_scan_clone_view(ctx, v, od->h_ncells[stream], out);
  if (rc != CFEAR_OK) return rc;
  // the route word of the stream's last frame: its scratch header stays as the kernels left it until the next process()
  uint32_t path = 0;
  const int rc_path = cfear_surface_read_path(ctx, od->d_surf_scratch.get(), od->cap_points, stream, &path);
  if (rc_path != CFEAR_OK) { cfear_scan_destroy(*out); *out = nullptr; return rc_path; }
  (*out)->surf_path = path;
  return CFEAR_OK;
}

static int copy_cloud_out(cfear_odometry* od, const float* d_src, int n, float* xyzi, int32_t cap, int32_t* n_out) {
  cfear_ctx* ctx = od->ctx;
  if (n_out) *n_out = n;
  if (!xyzi) return CFEAR_OK;
  if (n > cap) return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "%d points > cap %d", n, cap);
  if (n == 0) return CFEAR_OK;
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const bool dev = cfear_is_device_ptr(xyzi);
  CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(xyzi, d_src, (size_t)n * 16, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
  if (!dev) CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return CFEAR_OK;
}

extern "C" int cfear_odometry_get_cloud(cfear_odometry* od, int32_t stream, float* xyzi, int32_t cap, int32_t* n_out) {
  if (!od || stream < 0 || stream >= od->n_streams || cap < 0) return CFEAR_ERR_INVALID_ARGUMENT;
  if (od->last_slab[stream] < 0) return cfear_set_error(od->ctx, CFEAR_ERR_INVALID_ARGUMENT, "stream %d: no frame processed yet", stream);
  return copy_cloud_out(od, od->d_xyzi + (size_t)stream * od->cap_points * 4, od->h_npts[stream], xyzi, cap, n_out);
}

extern "C" int cfear_odometry_get_peaks(cfear_odometry* od, int32_t stream, float* xyzi, int32_t cap, int32_t* n_out) {
  if (!od || stream < 0 || stream >= od->n_streams || cap < 0) return CFEAR_ERR_INVALID_ARGUMENT;
  if (!od->par.keep_nodes) return cfear_set_error(od->ctx, CFEAR_ERR_INVALID_ARGUMENT, "peaks clouds are kept only with keep_nodes = 1");
  if (od->last_slab[stream] < 0) return cfear_set_error(od->ctx, CFEAR_ERR_INVALID_ARGUMENT, "stream %d: no frame processed yet", stream);
  return copy_cloud_out(od, od->d_pk + (size_t)stream * od->cap_points * 4, od->h_npk[stream], xyzi, cap, n_out);
}

// 6x6 inverse by Gauss-Jordan elimination with partial pivoting; false (and `inv` undefined) where a pivot column holds
// nothing but zeros or something not finite -- the matrix is singular as it stands, no tolerance is applied.
static bool inverse66(const double* m, double* inv) {
  double a[6][12];
  for (int r = 0; r < 6; r++)
    for (int c = 0; c < 6; c++) { a[r][c] = m[r * 6 + c]; a[r][6 + c] = r == c ? 1.0 : 0.0; }
  for (int k = 0; k < 6; k++) {
    int p = k;
    for (int r = k + 1; r < 6; r++) if (std::fabs(a[r][k]) > std::fabs(a[p][k])) p = r;
    if (a[p][k] == 0.0 || !std::isfinite(a[p][k])) return false;
    if (p != k) for (int c = 0; c < 12; c++) std::swap(a[p][c], a[k][c]);
    const double d = a[k][k];
    for (int c = 0; c < 12; c++) a[k][c] /= d;
    for (int r = 0; r < 6; r++) {
      const double f = a[r][k];
      if (r == k || f == 0.0) continue;
      for (int c = 0; c < 12; c++) a[r][c] -= f * a[k][c];
    }
  }
  for (int r = 0; r < 6; r++) for (int c = 0; c < 6; c++) inv[r * 6 + c] = a[r][6 + c];
  return true;
}

extern "C" int cfear_odometry_get_constraint(cfear_odometry* od, int32_t stream, cfear_graph_constraint* out) {
  if (!od || !out || stream < 0 || stream >= od->n_streams) return CFEAR_ERR_INVALID_ARGUMENT;
  const StreamState& st = od->streams[stream];
  if (!st.has_constraint) return cfear_set_error(od->ctx, CFEAR_ERR_INVALID_ARGUMENT, "stream %d: the last frame added no keyframe behind another one", stream);
  memset(out, 0, sizeof(*out));
  out->id_begin = st.c_from; out->id_end = st.c_to;
  double xyt[3];
  aff_to_xyt(st.c_Tdiff, xyt);
  cfear_pose3d_from_xyt(xyt, &out->t_be);
  out->type = 0;                                                  // ConstraintType::odometry
  // information = C.inverse() (:440) where C has one: the sampled covariance (Identity on z, roll, pitch) and the Identity
  // of a failed registration.  Register's constant diagonal is singular: there it is the inverse on the planar sub-space
  // (x, y, yaw) = indices 0, 1, 5 and zero elsewhere (see cfear_hip.h)
  if (inverse66(st.c_cov, out->information)) return CFEAR_OK;
  memset(out->information, 0, sizeof(out->information));
  const int ix[3] = {0, 1, 5};
  double M[9], I[9];
  for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) M[r * 3 + c] = st.c_cov[ix[r] * 6 + ix[c]];
  const double det = M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
  if (det != 0.0 && std::isfinite(det)) {
    I[0] = (M[4] * M[8] - M[5] * M[7]) / det; I[1] = (M[2] * M[7] - M[1] * M[8]) / det; I[2] = (M[1] * M[5] - M[2] * M[4]) / det;
    I[3] = (M[5] * M[6] - M[3] * M[8]) / det; I[4] = (M[0] * M[8] - M[2] * M[6]) / det; I[5] = (M[2] * M[3] - M[0] * M[5]) / det;
    I[6] = (M[3] * M[7] - M[4] * M[6]) / det; I[7] = (M[1] * M[6] - M[0] * M[7]) / det; I[8] = (M[0] * M[4] - M[1] * M[3]) / det;
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) out->information[ix[r] * 6 + ix[c]] = I[r * 3 + c];
  }
  return CFEAR_OK;
}
