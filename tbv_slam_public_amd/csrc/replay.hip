// replay.hip -- cfear_odometry_replay_clouds: every frame of a recorded trajectory registered from the trajectory's own
// state (include/cfear_hip.h), as chunks of batched launches.
//
// Host: the O(frames) state walk -- motions, guesses, the keyframe chain, which is serial by nature -- with the functions
// process_frame (odometry.hip) uses: pose2d.hpp, cfear_keyframe_based_fuse.  It depends on the trace only.
// Device, per chunk of frames: the chunk's clouds become scans in one arena (cfear_scan_batch_build: the surface-point
// kernels through cfear_surface_launch), replay_expand_kernel writes the matcher's job records from the scans' views and the
// per-frame table, matcher_kernel runs through cfear_register_launch, replay_score_kernel turns the result records and the
// trace into cfear_replay_frames.  Job and result records stay on the device; one read-back of the records ends a chunk.
// A chunk's arena lives until the last frame whose window holds one of its keyframes has been registered.
#include <algorithm>
#include <cmath>
#include <deque>
#include <memory>
#include <vector>

#include "registration.hpp"

namespace {

// one frame of a chunk, as the two kernels read it
struct ReplayIn {
  double trace[3], prev[3], guess[3], mot_xy[2];   // P_t, P_t-1, the job's start pose, the translation of M_t
  int32_t job;                                      // the frame's job among the chunk's, -1: none
  int32_t status;                                   // what reg_status reports without a job: 1 (first frame) or a scan's status
  int32_t cur, n_win;                               // the frame's own view, the views of its window
  int32_t is_keyframe, n_points, n_cells, pad;
  int32_t win[kRegMaxScans];
};
static_assert(sizeof(ReplayIn) % 8 == 0, "ReplayIn is uploaded as an array");
static_assert(sizeof(cfear_replay_frame) == 160, "cfear_replay_frame has no implicit padding (include/cfear_hip.h)");

// frame -> the job record matcher_kernel reads: scans [window.., the frame's own], poses [window trace poses.., guess]
// (expand_candidates_kernel of register.hip, from pairs to windows)
__global__ __launch_bounds__(256) void replay_expand_kernel(const ReplayIn* __restrict__ frames, int n, const ScanView* __restrict__ views,
                                                            const double* __restrict__ vpose, char* __restrict__ jobs, size_t stride) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const ReplayIn& f = frames[i];
  if (f.job < 0) return;
  RegJob* j = (RegJob*)(jobs + (size_t)f.job * stride);
  const int nw = min(f.n_win, kRegMaxScans - 1);
  j->n_scans = nw + 1; j->itr = 0;
  for (int k = 0; k < nw; k++) {
    const int v = f.win[k];
    j->poses[k][0] = vpose[3 * v]; j->poses[k][1] = vpose[3 * v + 1]; j->poses[k][2] = vpose[3 * v + 2];
    j->scans[k] = views[v];
  }
  j->poses[nw][0] = f.guess[0]; j->poses[nw][1] = f.guess[1]; j->poses[nw][2] = f.guess[2];
  j->scans[nw] = views[f.cur];
}

// result record + trace -> cfear_replay_frame: the sanity check, the final pose and its deviation from the trace, with the
// pose algebra of process_frame (odometry.hip: Tcurrent, Tmot_current, the guess where the check fails)
__global__ __launch_bounds__(256) void replay_score_kernel(const ReplayIn* __restrict__ frames, int n, const cfear_reg_result* __restrict__ res,
                                                           cfear_replay_frame* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const ReplayIn& f = frames[i];
  cfear_replay_frame o;
  for (int k = 0; k < 3; k++) { o.guess[k] = f.guess[k]; o.pose[k] = f.guess[k]; o.dev[k] = 0.0; }
  o.score = o.final_cost = o.last_relative_decrease = 0.0;
  o.n_points = f.n_points; o.n_cells = f.n_cells; o.is_keyframe = f.is_keyframe; o.n_targets = f.job >= 0 ? f.n_win : 0;
  o.reg_status = f.status; o.outer_iters = o.lm_iters = o.num_residuals = 0;
  o.sanity_ok = 1;
  o.n_tied_start = o.n_tied_effective_start = o.n_tied_end = o.n_tied_effective_end = -1;
  o.n_voxels_exposed = o.n_voxels_changed_reversed = -1;
  o.exposed = -1;
  const double* final_xyt = f.guess;
  if (f.job >= 0) {
    const cfear_reg_result r = res[f.job];
    for (int k = 0; k < 3; k++) o.pose[k] = r.pose[k];
    o.score = r.score; o.final_cost = r.final_cost; o.last_relative_decrease = r.last_relative_decrease;
    o.reg_status = r.status; o.outer_iters = r.outer_iters; o.lm_iters = r.lm_iters; o.num_residuals = r.num_residuals;
    const Aff2 Tcurrent = aff_from_xyt(r.pose);
    const Aff2 Tmot_current = aff_mul(aff_inv(aff_from_xyt(f.prev)), Tcurrent);
    const double curr_xy[2] = {Tmot_current.t0, Tmot_current.t1};
    o.sanity_ok = pose2d_acc_vel_sane(f.mot_xy, curr_xy);
    if (o.sanity_ok) final_xyt = o.pose;
  }
  if (f.job >= 0) {                                // on (x, y, theta) itself: exactly zero iff the final pose IS the trace pose (no job: 0)
    double ti[3];
    xyt_inverse(f.trace, ti);
    xyt_compose(ti, final_xyt, o.dev);
  }
  out[i] = o;
}

// what the state walk leaves per frame
struct FrameState {
  Aff2 T, Tmot, Tguess;
  double vpose[3];                                  // the pose a window carries this frame at: xyt of T
  int32_t is_keyframe = 0, first = 0, n_win = 0;
  int32_t win[kRegMaxScans];                        // frames of the window
  int32_t last_use = -1;                            // the last frame whose window holds this one
};

// a chunk's scans: frames [first, first + status.size())
struct ChunkScans {
  int first = 0;
  cfear_scan_batch* batch = nullptr;
  std::vector<int32_t> status;
  int last_use = -1;
  ~ChunkScans() { if (batch) (void)cfear_scan_batch_destroy(batch); }
};

}  // namespace

extern "C" int cfear_odometry_replay_clouds(cfear_ctx* ctx, const cfear_sc_cloud* clouds, const cfear_odometry_params* par,
                                            const double* trace_xyt, const int32_t* seq_offsets, int32_t n_seq, int32_t flags,
                                            cfear_replay_frame* out) {
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (!clouds || !par || !trace_xyt || !seq_offsets || !out) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  if (n_seq < 1) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "n_seq must be at least 1");
  if (flags & ~CFEAR_REPLAY_AUDIT) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "unknown flags %d", (int)flags);
  const bool audit = (flags & CFEAR_REPLAY_AUDIT) != 0;
  if (seq_offsets[0] != 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "sequence 0: seq_offsets must start at 0");
  for (int s = 0; s < n_seq; s++)
    if (seq_offsets[s + 1] <= seq_offsets[s])
      return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "sequence %d: empty, or seq_offsets not ascending", s);
  const int F = seq_offsets[n_seq];
  if (par->submap_scan_size < 1 || par->submap_scan_size > kRegMaxScans - 1)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "submap_scan_size must be in [1, %d]", kRegMaxScans - 1);
  CFEAR_CHECK(cfear_check_reg_params(ctx, &par->reg));
  int max_points = 1;
  for (int f = 0; f < F; f++) {
    for (int k = 0; k < 3; k++)
      if (!std::isfinite(trace_xyt[3 * (size_t)f + k])) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "frame %d: trace pose is not finite", f);
    if (clouds[f].n < 0 || (clouds[f].n > 0 && !clouds[f].xyzi)) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "frame %d: bad cloud", f);
    max_points = std::max(max_points, clouds[f].n);
  }
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));

  // ---- the state walk: what process_frame would hold had the trace been its own output --------------------------------
  std::vector<FrameState> fs((size_t)F);
  std::vector<double> mots(3 * (size_t)F, 0.0);
  for (int s = 0; s < n_seq; s++) {
    const int a = seq_offsets[s], b = seq_offsets[s + 1];
    std::vector<int> keyframes;
    for (int f = a; f < b; f++) {
      FrameState& st = fs[(size_t)f];
      st.T = aff_from_xyt(trace_xyt + 3 * (size_t)f);
      aff_to_xyt(st.T, st.vpose);
      st.Tmot = f - a >= 2 ? aff_mul(aff_inv(fs[(size_t)f - 2].T), fs[(size_t)f - 1].T) : aff_identity();   // st.Tmot of :806
      aff_to_xyt(st.Tmot, &mots[3 * (size_t)f]);                                                         // Compensate(cloud, TprevMot, ccw)
      if (f == a) {                                                     // the first frame becomes the first keyframe
        st.first = st.is_keyframe = 1;
        st.Tguess = st.T;
        keyframes.push_back(f);
        continue;
      }
      const Aff2& Tprev = fs[(size_t)f - 1].T;
      st.Tguess = par->use_guess ? aff_mul(Tprev, st.Tmot) : Tprev;     // :164-168
      st.n_win = (int)keyframes.size();
      for (int k = 0; k < st.n_win; k++) { st.win[k] = keyframes[(size_t)k]; fs[(size_t)keyframes[(size_t)k]].last_use = f; }
      double kd[3];
      aff_to_xyt(aff_mul(aff_inv(fs[(size_t)keyframes.back()].T), st.T), kd);
      if (cfear_keyframe_based_fuse(kd, par->use_keyframe, par->min_keyframe_dist, par->min_keyframe_rot_deg)) {
        st.is_keyframe = 1;
        keyframes.push_back(f);
        if ((int)keyframes.size() > par->submap_scan_size) keyframes.erase(keyframes.begin());
      }
    }
  }

  // ---- chunks ------------------------------------------------------------------------------------------------------
  const int max_cells = std::min(max_points, cfear_surface_max_points());      // a cloud has at most one cell per point
  int chunk = 4096;
  {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = (size_t)1 << 30; }
    const size_t per_frame = cfear_scan_slab_bytes(max_cells) + (size_t)max_points * 16;
    chunk = (int)std::max<size_t>(8, std::min<size_t>(4096, free_b / 8 / per_frame));
  }
  if (ctx->replay_chunk > 0) chunk = (int)std::min<int64_t>(ctx->replay_chunk, 1 << 20);
  cfear_feature_params fp{};
  fp.radius = par->res;
  fp.downsample_factor = par->downsample_factor;
  fp.weight_intensity = par->weight_intensity;
  fp.compensate = par->compensate;
  fp.ccw = par->radar_ccw;
  std::deque<std::unique_ptr<ChunkScans>> live;
  auto scan_of = [&](int f, int32_t* status) -> const cfear_scan* {
    for (const auto& c : live)
      if (f >= c->first && f < c->first + (int)c->status.size()) { *status = c->status[(size_t)(f - c->first)]; return c->batch->scans[(size_t)(f - c->first)]; }
    *status = CFEAR_ERR_INVALID_ARGUMENT;                                // (cannot happen: a chunk lives as long as its last_use says)
    return nullptr;
  };
  // which side a cloud is on: a cloud inside the device allocation the last query found needs no query of its own (a
  // caller's clouds are usually slices of a few buffers; 4 096 pointer queries were a third of a replay's host time)
  const char *dev_lo = nullptr, *dev_hi = nullptr;
  auto on_device = [&](const float* p) -> bool {
    if ((const char*)p >= dev_lo && (const char*)p < dev_hi) return true;
    if (!cfear_is_device_ptr(p)) return false;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) == hipSuccess) { dev_lo = (const char*)base; dev_hi = dev_lo + size; }
    else (void)hipGetLastError();
    return true;
  };
  int first_error = CFEAR_OK, first_error_frame = -1;
  std::vector<const float*> ptrs;
  std::vector<char> on_host;
  std::vector<int32_t> lengths;
  std::vector<ScanView> views;
  std::vector<double> vpose;
  std::vector<ReplayIn> table;
  std::vector<cfear_voxel_audit_record> vrec(audit ? (size_t)F : 0);      // the audit: every frame's compensated cloud, once
  for (int a = 0; a < F; a += chunk) {
    const int b = std::min(F, a + chunk), m = b - a;
    while (!live.empty() && live.front()->last_use < a) live.pop_front();   // no window of this chunk or a later one holds its scans
    // the chunk's scans
    ptrs.assign((size_t)m, nullptr); on_host.assign((size_t)m, 0); lengths.assign((size_t)m, 0);
    std::unique_ptr<ChunkScans> cs(new ChunkScans());
    cs->first = a;
    cs->status.assign((size_t)m, CFEAR_OK);
    const char* one_alloc = nullptr;                                     // the allocation's base, as hipMemGetAddressRange reported it
    bool seen = false;
    for (int k = 0; k < m; k++) {
      ptrs[(size_t)k] = clouds[a + k].xyzi;
      lengths[(size_t)k] = clouds[a + k].n;
      on_host[(size_t)k] = (char)(clouds[a + k].n > 0 && !on_device(clouds[a + k].xyzi));
      if (clouds[a + k].n > 0) {                                         // one device allocation holds every cloud of the chunk so far?
        const char* p0 = (const char*)clouds[a + k].xyzi;
        const char* alloc = !on_host[(size_t)k] && p0 >= dev_lo && p0 + (size_t)clouds[a + k].n * 16 <= dev_hi ? dev_lo : nullptr;
        if (!seen) { one_alloc = alloc; seen = true; }
        else if (alloc != one_alloc) one_alloc = nullptr;
      }
      cs->last_use = std::max(cs->last_use, std::max(a + k, fs[(size_t)(a + k)].last_use));
    }
    // Clouds handed in one by one may be separate allocations: the memory between two of them is only the caller's -- and may
    // only be copied along in one piece -- where the runtime says that ONE device allocation holds them all.
    const int rc = cfear_scan_batch_build(ctx, ptrs.data(), on_host.data(), /*one_buffer=*/one_alloc != nullptr, lengths.data(), m, &fp, mots.data() + 3 * (size_t)a, max_cells,
                                          &cs->batch, cs->status.data());
    if (!cs->batch) return rc;
    live.push_back(std::move(cs));
    // the view table (the chunk's frames first, then the earlier keyframes its windows hold) and the frame table
    views.clear(); vpose.clear();
    std::vector<int> view_frame;                                         // view -> frame
    auto view_of = [&](int f) -> int {
      if (f >= a) return f - a;
      for (size_t v = (size_t)m; v < view_frame.size(); v++) if (view_frame[v] == f) return (int)v;
      view_frame.push_back(f);
      return (int)view_frame.size() - 1;
    };
    for (int k = 0; k < m; k++) view_frame.push_back(a + k);
    table.assign((size_t)m, ReplayIn{});
    JobSizes sz(&par->reg);
    int n_jobs = 0, max_scans = 2;
    for (int k = 0; k < m; k++) {
      const int f = a + k;
      const FrameState& st = fs[(size_t)f];
      ReplayIn& r = table[(size_t)k];
      for (int q = 0; q < 3; q++) { r.trace[q] = trace_xyt[3 * (size_t)f + q]; r.prev[q] = st.first ? r.trace[q] : trace_xyt[3 * (size_t)(f - 1) + q]; }
      if (st.first) for (int q = 0; q < 3; q++) r.guess[q] = r.trace[q];       // pose = guess = P_0
      else aff_to_xyt(st.Tguess, r.guess);
      r.mot_xy[0] = st.Tmot.t0; r.mot_xy[1] = st.Tmot.t1;
      r.job = -1; r.cur = k; r.n_win = st.n_win; r.is_keyframe = st.is_keyframe; r.n_points = clouds[f].n;
      int32_t status = CFEAR_OK;
      const cfear_scan* own = scan_of(f, &status);
      r.n_cells = own ? own->n_cells_host : 0;
      r.status = status != CFEAR_OK ? status : 1;                        // 1: the first frame's reg_status
      if (status != CFEAR_OK && first_error == CFEAR_OK) { first_error = status; first_error_frame = f; }
      if (status != CFEAR_OK || st.first) continue;
      int sum_pad = 0, max_pad = 0;
      for (int w = 0; w < st.n_win; w++) {
        int32_t ws = CFEAR_OK;
        const cfear_scan* t = scan_of(st.win[w], &ws);
        if (ws != CFEAR_OK) { status = ws; break; }                      // a window that holds a failed scan: no job, its status
        r.win[w] = view_of(st.win[w]);
        sum_pad += scan_grid_pad(t->n_cells_host); max_pad = std::max(max_pad, scan_grid_pad(t->n_cells_host));
      }
      if (status != CFEAR_OK) { r.status = status; continue; }
      r.job = n_jobs++;
      max_scans = std::max(max_scans, st.n_win + 1);
      sz.add(st.n_win + 1, sum_pad, max_pad, own->n_cells_host);
    }
    const int n_views = (int)view_frame.size();
    views.resize((size_t)n_views); vpose.resize(3 * (size_t)n_views);
    for (int v = 0; v < n_views; v++) {
      int32_t status = CFEAR_OK;
      const cfear_scan* s = scan_of(view_frame[(size_t)v], &status);
      views[(size_t)v] = s ? s->view : ScanView{};
      for (int q = 0; q < 3; q++) vpose[3 * (size_t)v + q] = fs[(size_t)view_frame[(size_t)v]].vpose[q];
    }
    // upload, expand, match, score, read back
    HostStage st(ctx, kWsRegJobs);
    const size_t stride = reg_job_stride(max_scans);
    const size_t vb = (size_t)n_views * sizeof(ScanView), pb = (size_t)n_views * 24, tb = (size_t)m * sizeof(ReplayIn);
    char *d_up, *d_jobs;
    cfear_reg_result* d_res;
    cfear_replay_frame* d_out;
    st.piece(d_up, vb + pb + tb);
    st.piece(d_jobs, (size_t)std::max(n_jobs, 1) * stride);
    st.piece(d_res, (size_t)std::max(n_jobs, 1) * sizeof(cfear_reg_result));
    st.piece(d_out, (size_t)m * sizeof(cfear_replay_frame));
    char* scr = n_jobs ? (char*)cfear_workspace(ctx, kWsRegScratch, reg_scratch_bytes(sz.pairs_cap) * (size_t)n_jobs) : nullptr;
    if (n_jobs && !scr) return cfear_set_error(ctx, CFEAR_ERR_HIP, "workspace allocation failed");
    CFEAR_CHECK(st.carve());
    char* h_up = (char*)st.pinned(vb + pb + tb);
    if (!h_up) return CFEAR_ERR_HIP;
    memcpy(h_up, views.data(), vb);
    memcpy(h_up + vb, vpose.data(), pb);
    memcpy(h_up + vb + pb, table.data(), tb);
    CFEAR_CHECK(st.upload(d_up, h_up, vb + pb + tb));
    const ReplayIn* d_table = (const ReplayIn*)(d_up + vb + pb);
    if (n_jobs) {
      {
        ProfScope ps(ctx, "replay_expand");
        hipLaunchKernelGGL(replay_expand_kernel, dim3((m + 255) / 256), dim3(256), 0, ctx->stream, d_table, m, (const ScanView*)d_up,
                           (const double*)(d_up + vb), d_jobs, stride);
      }
      CFEAR_HIP_CHECK(ctx, hipGetLastError());
      CFEAR_CHECK(cfear_register_launch(ctx, d_jobs, n_jobs, &par->reg, sz.pairs_cap, scr, d_res, nullptr, stride, sz.hint(n_jobs)));
    }
    {
      ProfScope ps(ctx, "replay_score");
      hipLaunchKernelGGL(replay_score_kernel, dim3((m + 255) / 256), dim3(256), 0, ctx->stream, d_table, m, d_res, d_out);
    }
    CFEAR_HIP_CHECK(ctx, hipGetLastError());
    st.back(out + a, d_out, (size_t)m * sizeof(cfear_replay_frame));
    CFEAR_CHECK(st.finish());
    if (!audit) continue;
    // ---- CFEAR_REPLAY_AUDIT: the chunk's records are on the host; the two audits run through their own entry points on the
    //      same scans, poses and clouds, and are folded into the records here ------------------------------------------------
    {                                                                     // the voxel order of every compensated cloud
      const size_t stride = (size_t)std::max(1, *std::max_element(lengths.begin(), lengths.end()));
      DevBuf<float> vx = dev_alloc<float>((size_t)m * stride * 16);
      DevBuf<int32_t> d_n = dev_alloc<int32_t>((size_t)m * 4);
      DevBuf<double> d_mot = dev_alloc<double>((size_t)m * 24);
      if (!vx || !d_n || !d_mot) return cfear_set_error(ctx, CFEAR_ERR_HIP, "replay audit: hipMalloc failed");
      std::vector<int64_t> offs((size_t)m);
      for (int k = 0; k < m; k++) {
        offs[(size_t)k] = (int64_t)((size_t)k * stride);
        if (lengths[(size_t)k] > 0)
          CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(vx.get() + (size_t)k * stride * 4, ptrs[(size_t)k], (size_t)lengths[(size_t)k] * 16,
                                              on_host[(size_t)k] ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, ctx->stream));
      }
      CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(d_n.get(), lengths.data(), (size_t)m * 4, hipMemcpyHostToDevice, ctx->stream));
      CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(d_mot.get(), mots.data() + 3 * (size_t)a, (size_t)m * 24, hipMemcpyHostToDevice, ctx->stream));
      if (par->compensate)
        CFEAR_CHECK(cfear_compensate_batch_device(ctx, vx.get(), stride, d_n.get(), d_mot.get(), m, (int)stride, par->radar_ccw));
      CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));            // the uploads above read the caller's and this call's host memory
      cfear_voxel_audit_params vp;
      cfear_voxel_audit_params_default(&vp);
      vp.radius = par->res;
      vp.downsample_factor = par->downsample_factor;
      const int vrc = cfear_voxel_order_audit_batch(ctx, vx.get(), offs.data(), lengths.data(), m, &vp, vrec.data() + a, nullptr, 0, nullptr);
      if (vrc == CFEAR_ERR_HIP) return vrc;                               // (a scan's own status sits in its record)
      CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    }
    std::vector<cfear_reg_job> jobs((size_t)n_jobs);
    std::vector<const cfear_scan*> handles((size_t)n_jobs * kRegMaxScans);
    std::vector<double> jposes((size_t)n_jobs * kRegMaxScans * 3);
    std::vector<int> job_frame((size_t)n_jobs);
    for (int k = 0; k < m; k++) {
      const ReplayIn& r = table[(size_t)k];
      if (r.job < 0) continue;
      const FrameState& fst = fs[(size_t)(a + k)];
      const size_t j = (size_t)r.job;
      int32_t dummy;
      for (int w = 0; w < fst.n_win; w++) {
        handles[j * kRegMaxScans + (size_t)w] = scan_of(fst.win[w], &dummy);
        for (int q = 0; q < 3; q++) jposes[(j * kRegMaxScans + (size_t)w) * 3 + (size_t)q] = fs[(size_t)fst.win[w]].vpose[q];
      }
      handles[j * kRegMaxScans + (size_t)fst.n_win] = scan_of(a + k, &dummy);
      jobs[j].scans = handles.data() + j * kRegMaxScans;
      jobs[j].n_scans = fst.n_win + 1;
      jobs[j].pad = 0;
      jobs[j].poses_xyt = jposes.data() + j * kRegMaxScans * 3;
      job_frame[j] = a + k;
    }
    std::vector<cfear_tie_record> ties[2];
    for (int pass = 0; pass < 2 && n_jobs > 0; pass++) {                  // at the guess with itr = 1, at the registered pose with itr = 2
      for (int j = 0; j < n_jobs; j++) {
        const cfear_replay_frame& o = out[job_frame[(size_t)j]];
        double* src = jposes.data() + ((size_t)j * kRegMaxScans + (size_t)(jobs[(size_t)j].n_scans - 1)) * 3;
        for (int q = 0; q < 3; q++) src[q] = pass == 0 ? o.guess[q] : o.pose[q];
      }
      ties[pass].assign((size_t)n_jobs, cfear_tie_record{});
      const int trc = cfear_association_ties_batch(ctx, jobs.data(), n_jobs, &par->reg, pass + 1, ties[pass].data(), nullptr, 0);
      if (trc == CFEAR_ERR_HIP || trc == CFEAR_ERR_INVALID_ARGUMENT) return trc;
    }
    for (int k = 0; k < m; k++) {
      const ReplayIn& r = table[(size_t)k];
      const FrameState& fst = fs[(size_t)(a + k)];
      cfear_replay_frame& o = out[a + k];
      o.n_tied_start = o.n_tied_effective_start = o.n_tied_end = o.n_tied_effective_end = 0;
      o.n_voxels_exposed = vrec[(size_t)(a + k)].n_voxels_exposed;
      o.n_voxels_changed_reversed = vrec[(size_t)(a + k)].n_voxels_changed_reversed;
      if (r.job >= 0) {
        o.n_tied_start = ties[0][(size_t)r.job].n_tied; o.n_tied_effective_start = ties[0][(size_t)r.job].n_tied_effective;
        o.n_tied_end = ties[1][(size_t)r.job].n_tied; o.n_tied_effective_end = ties[1][(size_t)r.job].n_tied_effective;
        for (int w = 0; w < fst.n_win; w++) {                             // summed over the job's scans
          o.n_voxels_exposed += vrec[(size_t)fst.win[w]].n_voxels_exposed;
          o.n_voxels_changed_reversed += vrec[(size_t)fst.win[w]].n_voxels_changed_reversed;
        }
      }
      o.exposed = (o.n_tied_effective_start > 0 || o.n_tied_effective_end > 0 || o.n_voxels_exposed > 0) ? 1 : 0;
    }
  }
  if (first_error != CFEAR_OK)
    return cfear_set_error(ctx, first_error, "frame %d: surface points failed (%s)", first_error_frame, cfear_status_string(first_error));
  return CFEAR_OK;
}

// The sweep entry: the polar filter through its own entry points (the decode first for [range bins][azimuths] sources), the
// clouds kept on the device, then the replay above.
extern "C" int cfear_odometry_replay(cfear_ctx* ctx, const cfear_polar_desc* desc, const uint8_t* polar, const cfear_odometry_params* par,
                                     const double* trace_xyt, const int32_t* seq_offsets, int32_t n_seq, int32_t flags,
                                     cfear_replay_frame* out) {
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (!desc || !polar || !par || !trace_xyt || !seq_offsets || !out) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  if (n_seq < 1) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "n_seq must be at least 1");
  if (seq_offsets[0] != 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "sequence 0: seq_offsets must start at 0");
  for (int s = 0; s < n_seq; s++)
    if (seq_offsets[s + 1] <= seq_offsets[s])
      return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "sequence %d: empty, or seq_offsets not ascending", s);
  const int F = seq_offsets[n_seq];
  if (desc->batch != F)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "desc.batch = %d, but the sequences hold %d frames", (int)desc->batch, F);
  for (int f = 0; f < F; f++)
    for (int k = 0; k < 3; k++)
      if (!std::isfinite(trace_xyt[3 * (size_t)f + k])) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "frame %d: trace pose is not finite", f);
  if (desc->rows < 1 || desc->cols < 1 || desc->stride < desc->cols)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "bad image descriptor");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const bool cfar = par->filter_type == CFEAR_FILTER_CACFAR;
  const int rows = par->rotate_ccw ? desc->cols : desc->rows, cols = par->rotate_ccw ? desc->rows : desc->cols;   // azimuths x range bins
  const int k = par->kstrong.k_strongest;
  if (!cfar && (k < 1 || k > 1024)) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "k_strongest must be in [1, 1024]");
  const int cap = cfar ? std::min(rows * cols, 65536) : rows * k;          // as cfear_odometry_create sizes a stream's cloud
  const int64_t src_stride = F > 1 ? desc->batch_stride : (int64_t)desc->rows * desc->stride;
  const bool host = !cfear_is_device_ptr(polar);
  const int step = 256;                                                     // images per filter call
  DevBuf<float> xyzi = dev_alloc<float>((size_t)F * cap * 16);
  DevBuf<int32_t> d_n = dev_alloc<int32_t>((size_t)F * 4);
  DevBuf<int32_t> sel_range, sel_count;
  DevBuf<uint8_t> sel_int, d_rot;
  std::vector<uint8_t> h_rot;
  bool ok = xyzi && d_n;
  if (!cfar) {
    sel_range = dev_alloc<int32_t>((size_t)step * rows * k * 4);
    sel_int = dev_alloc<uint8_t>((size_t)step * rows * k);
    sel_count = dev_alloc<int32_t>((size_t)step * rows * 4);
    ok = ok && sel_range && sel_int && sel_count;
  }
  if (par->rotate_ccw) {
    if (host) h_rot.resize((size_t)step * rows * cols);
    else ok = ok && (d_rot = dev_alloc<uint8_t>((size_t)step * rows * cols));
  }
  if (!ok) return cfear_set_error(ctx, CFEAR_ERR_HIP, "replay: hipMalloc of the clouds failed");
  cfear_kstrong_params kp = par->kstrong;
  kp.want_peaks = 0;
  for (int f0 = 0; f0 < F; f0 += step) {
    const int c = std::min(step, F - f0);
    cfear_polar_desc d = *desc;
    d.batch = c;
    d.batch_stride = src_stride;
    const uint8_t* img = polar + (size_t)f0 * (size_t)src_stride;
    if (par->rotate_ccw) {                                                  // radar_driver.cpp:74-90
      uint8_t* dst = host ? h_rot.data() : d_rot.get();
      CFEAR_CHECK(cfear_polar_rotate_ccw(ctx, img, &d, dst, cols, (int64_t)rows * cols));
      d.rows = rows; d.cols = cols; d.stride = cols; d.batch_stride = (int64_t)rows * cols;
      img = dst;
    }
    float* cx = xyzi.get() + (size_t)f0 * cap * 4;
    if (cfar) {
      CFEAR_CHECK(cfear_filter_cacfar(ctx, img, &d, &par->cacfar, cx, d_n.get() + f0, cap, nullptr));
    } else {
      cfear_kstrong_out o{};
      o.sel_range = sel_range.get(); o.sel_intensity = sel_int.get(); o.sel_count = sel_count.get();
      o.xyzi = cx; o.n_points = d_n.get() + f0;
      CFEAR_CHECK(cfear_filter_kstrongest(ctx, img, &d, &kp, &o));
    }
  }
  std::vector<int32_t> n((size_t)F);
  CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(n.data(), d_n.get(), (size_t)F * 4, hipMemcpyDeviceToHost, ctx->stream));
  CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  std::vector<cfear_sc_cloud> clouds((size_t)F);
  for (int f = 0; f < F; f++) {
    clouds[(size_t)f].n = std::min(std::max(n[(size_t)f], 0), cap);
    clouds[(size_t)f].xyzi = clouds[(size_t)f].n > 0 ? xyzi.get() + (size_t)f * cap * 4 : nullptr;
    clouds[(size_t)f].pad = 0;
  }
  return cfear_odometry_replay_clouds(ctx, clouds.data(), par, trace_xyt, seq_offsets, n_seq, flags, out);
}
