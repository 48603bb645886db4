// odometry_grid.hip -- a parameter grid of odometry streams as one batch: stream s runs configuration stream_config[s] on
// the images of sequence stream_sequence[s] (the reference's grid_search / loss_function evaluations: one job per (sequence,
// configuration), utils/worker).  Per stream the state and the results are those of a cfear_odometry with that configuration
// (the frame policy is odometry_policy.hpp's, the same code); what the streams share is computed once:
//   sweep    one k-strongest sweep per sequence image -- directly into row keys where its streams form one filter class, else
//            at (max k, min uchar(z_min)) into sel_* lists from which kstrong_derive_kernel writes every class's row keys --
//            and one CA-CFAR sweep per distinct (sequence, cfear_cacfar_params)
//   surface  one cfear_surface_launch per group of equal surface parameters over a sub-range of ONE job table; a job reads
//            its class's shared row keys with its own motion and compensate flag
//   matcher  one cfear_register_launch per group of equal (cfear_reg_params, submap_scan_size) over a sub-range of ONE job
//            table, each group at its window's record stride
// One read-back per call (results | status | n_cells | n_points of all groups in one block).  The sweeps and the surface groups
// run on the context's stream one after another (they share per-context workspaces); the matcher groups, which share nothing,
// are dealt round-robin to that stream and up to three side streams of the object: a group of a few hundred registrations
// fills well under half the chip (EXPERIMENTS.md, "A parameter grid as one batch").
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <string>

#include "odometry_policy.hpp"
#include "polar_common.hpp"

namespace {

constexpr int kGridCellCap = 2048;         // cells per scan slab, as cfear_odometry_create
constexpr int kDerivedStride = 64;         // keys per row of a derived class (cfear_kstrong_rowkeys_derive)

struct GridSweep {
  int sequence = 0;
  bool cfar = false, derive = false;
  cfear_kstrong_params kp{};               // direct: the class's own; derive: (max k, the z_min of the lowest threshold)
  cfear_cacfar_params cp{};
  int first_class = 0, n_classes = 0;
};
struct GridClass {
  int sweep = 0, sequence = 0;
  bool cfar = false;
  int k = 0, u_zmin = 0, min_range_bin = 0;
  float range_res = 0.f;
  int row_k = 0;                           // keys per row of its key table
  cfear_kstrong_params kp{};               // the first stream's (what a direct sweep runs with)
};
struct GridSurfGroup {
  cfear_feature_params fp{};
  bool cfar = false;
  float range_res = 0.f;
  int row_k = 0, cap_points = 0, first = 0, n = 0;
};
struct GridRegGroup {
  cfear_reg_params reg{};
  int submap = 0, first = 0, n = 0;
};
struct GridPlan {
  cfear_polar_desc fdesc{};                // the images as the filters see them (rows = azimuths)
  int rotate = 0;
  std::vector<cfear_grid_stream> streams;
  std::vector<GridSweep> sweeps;
  std::vector<GridClass> classes;
  std::vector<GridSurfGroup> surf;
  std::vector<GridRegGroup> reg;
  cfear_grid_totals totals{};
};

int refuse(std::string& why, const char* fmt, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  why = buf;
  return CFEAR_ERR_INVALID_ARGUMENT;
}

int cfar_row_k(int cols) { return std::min((cols + 3) / 4 * 4, 1024); }

// What cfear_odometry_create refuses (for desc->batch streams of this configuration), and what a grid does not take.
int check_config(const cfear_polar_desc* desc, const cfear_odometry_params& p, int c, std::string& why) {
  if (p.submap_scan_size < 1 || p.submap_scan_size + 1 > kRegMaxScans)
    return refuse(why, "configuration %d: submap_scan_size must be in [1,%d]", c, kRegMaxScans - 1);
  if (!(p.res > 0.05f)) return refuse(why, "configuration %d: res must be > 0.05", c);
  if (p.estimate_cov_by_sampling) return refuse(why, "configuration %d: estimate_cov_by_sampling is outside a grid", c);
  if (p.keep_nodes) return refuse(why, "configuration %d: keep_nodes is outside a grid", c);
  const int frows = p.rotate_ccw ? desc->cols : desc->rows, fcols = p.rotate_ccw ? desc->rows : desc->cols;
  if (fcols > 8192) return refuse(why, "configuration %d: more than 8192 range bins unsupported", c);
  if (frows > 4096) return refuse(why, "configuration %d: more than 4096 azimuths unsupported", c);
  if (p.filter_type == CFEAR_FILTER_CACFAR) {
    if (p.cacfar.window_size < 1 || p.cacfar.nb_guard_cells < 0 || !(p.cacfar.range_res > 0.f))
      return refuse(why, "configuration %d: bad CFAR parameters", c);
  } else if (p.filter_type == CFEAR_FILTER_KSTRONG) {
    if (p.kstrong.k_strongest < 1 || p.kstrong.k_strongest > 64)
      return refuse(why, "configuration %d: k_strongest must be in [1,64]", c);
    if (!(p.kstrong.range_res > 0.f) || !(p.kstrong.min_distance >= 0.f))
      return refuse(why, "configuration %d: range_res must be > 0 and min_distance >= 0", c);
    if ((long long)frows * p.kstrong.k_strongest > cfear_surface_max_points())
      return refuse(why, "configuration %d: azimuths * k_strongest beyond %d points per scan", c, cfear_surface_max_points());
  } else {
    return refuse(why, "configuration %d: unknown filter_type %d", c, p.filter_type);
  }
  return CFEAR_OK;
}

int grid_plan(const cfear_polar_desc* desc, const cfear_odometry_params* configs, int n_configs, const int32_t* stream_sequence,
              const int32_t* stream_config, int n_streams, GridPlan& pl, std::string& why) {
  if (!desc || !configs) return refuse(why, "null argument");
  if (n_configs < 1) return refuse(why, "n_configs must be >= 1");
  if (n_streams < 1) return refuse(why, "n_streams must be >= 1");
  if ((stream_sequence == nullptr) != (stream_config == nullptr)) return refuse(why, "stream_sequence and stream_config go together");
  if (desc->rows <= 0 || desc->cols <= 0 || desc->stride < desc->cols || desc->batch < 1 ||
      (desc->batch > 1 && desc->batch_stride < (int64_t)desc->rows * desc->stride))
    return refuse(why, "bad polar descriptor");
  const int n_seq = desc->batch;
  if (!stream_sequence && (long long)n_streams != (long long)n_seq * n_configs)
    return refuse(why, "the full product has %lld streams, not %d", (long long)n_seq * n_configs, n_streams);
  pl.streams.assign(n_streams, cfear_grid_stream{});
  for (int s = 0; s < n_streams; s++) {
    const int q = stream_sequence ? stream_sequence[s] : s / n_configs, c = stream_config ? stream_config[s] : s % n_configs;
    if (q < 0 || q >= n_seq) return refuse(why, "stream %d: sequence %d outside [0,%d)", s, q, n_seq);
    if (c < 0 || c >= n_configs) return refuse(why, "stream %d: configuration %d outside [0,%d)", s, c, n_configs);
    pl.streams[s].sequence = q; pl.streams[s].config = c;
  }
  // every configuration is checked, used or not: a grid is written down before its streams are
  for (int c = 0; c < n_configs; c++) {
    const int rc = check_config(desc, configs[c], c, why);
    if (rc != CFEAR_OK) return rc;
    if ((configs[c].rotate_ccw != 0) != (configs[0].rotate_ccw != 0))
      return refuse(why, "configuration %d: rotate_ccw differs from configuration 0", c);
  }
  pl.rotate = configs[0].rotate_ccw != 0;
  pl.fdesc = *desc;
  if (pl.rotate) {                         // as cfear_odometry_create lays the rotated images out
    pl.fdesc.rows = desc->cols; pl.fdesc.cols = desc->rows;
    pl.fdesc.stride = (desc->rows + 127) / 128 * 128;
    pl.fdesc.batch_stride = (int64_t)pl.fdesc.rows * pl.fdesc.stride;
  }
  const int rows = pl.fdesc.rows, cols = pl.fdesc.cols;
  // ---- sweeps and filter classes, sequence by sequence: the k-strongest sweep first, then the CA-CFAR ones ----
  std::vector<std::vector<int>> by_seq(n_seq);
  for (int s = 0; s < n_streams; s++) by_seq[pl.streams[s].sequence].push_back(s);
  for (int q = 0; q < n_seq; q++) {
    const int class0 = (int)pl.classes.size();
    int ks_sweep = -1;
    for (int s : by_seq[q]) {
      const cfear_odometry_params& p = configs[pl.streams[s].config];
      if (p.filter_type != CFEAR_FILTER_KSTRONG) continue;
      if (ks_sweep < 0) {
        ks_sweep = (int)pl.sweeps.size();
        GridSweep sw; sw.sequence = q; sw.first_class = class0;
        pl.sweeps.push_back(sw);
      }
      const int u = (int)(uint8_t)(int)p.kstrong.z_min;
      const int mrb = (int)std::ceil((double)p.kstrong.min_distance / (double)p.kstrong.range_res);
      int found = -1;
      for (int i = class0; i < (int)pl.classes.size() && found < 0; i++) {
        const GridClass& g = pl.classes[i];
        if (g.k == p.kstrong.k_strongest && g.u_zmin == u && g.min_range_bin == mrb && g.range_res == p.kstrong.range_res) found = i;
      }
      if (found < 0) {
        GridClass g; g.sweep = ks_sweep; g.sequence = q; g.k = p.kstrong.k_strongest; g.u_zmin = u; g.min_range_bin = mrb;
        g.range_res = p.kstrong.range_res; g.kp = p.kstrong; g.kp.want_peaks = 0;
        found = (int)pl.classes.size();
        pl.classes.push_back(g);
      }
      pl.streams[s].sweep = ks_sweep; pl.streams[s].filter_class = found;
    }
    if (ks_sweep >= 0) {
      GridSweep& sw = pl.sweeps[ks_sweep];
      sw.n_classes = (int)pl.classes.size() - class0;
      sw.derive = sw.n_classes > 1;
      sw.kp = pl.classes[class0].kp;
      for (int i = class0; i < class0 + sw.n_classes; i++) {
        GridClass& g = pl.classes[i];
        g.row_k = sw.derive ? kDerivedStride : g.k;
        if (sw.derive) {
          sw.kp.k_strongest = std::max(sw.kp.k_strongest, g.k);
          if (g.u_zmin < (int)(uint8_t)(int)sw.kp.z_min) sw.kp.z_min = g.kp.z_min;
        }
      }
      if (sw.derive) pl.totals.n_derived_classes += sw.n_classes;
    }
    for (int s : by_seq[q]) {
      const cfear_odometry_params& p = configs[pl.streams[s].config];
      if (p.filter_type != CFEAR_FILTER_CACFAR) continue;
      int found = -1;
      for (int i = class0; i < (int)pl.classes.size() && found < 0; i++)
        if (pl.classes[i].cfar && memcmp(&pl.sweeps[pl.classes[i].sweep].cp, &p.cacfar, sizeof(p.cacfar)) == 0) found = i;
      if (found < 0) {
        GridSweep sw; sw.sequence = q; sw.cfar = true; sw.cp = p.cacfar; sw.first_class = (int)pl.classes.size(); sw.n_classes = 1;
        GridClass g; g.sweep = (int)pl.sweeps.size(); g.sequence = q; g.cfar = true; g.range_res = p.cacfar.range_res; g.row_k = cfar_row_k(cols);
        found = (int)pl.classes.size();
        pl.sweeps.push_back(sw);
        pl.classes.push_back(g);
      }
      pl.streams[s].sweep = pl.classes[found].sweep; pl.streams[s].filter_class = found;
    }
    pl.totals.max_classes_per_sequence = std::max(pl.totals.max_classes_per_sequence, (int)pl.classes.size() - class0);
  }
  // ---- surface and matcher groups, numbered in the order their first stream appears ----
  for (int s = 0; s < n_streams; s++) {
    const cfear_odometry_params& p = configs[pl.streams[s].config];
    const GridClass& g = pl.classes[pl.streams[s].filter_class];
    cfear_feature_params fp{};
    fp.radius = p.res; fp.downsample_factor = p.downsample_factor; fp.origin[0] = fp.origin[1] = 0.0;
    fp.weight_intensity = p.weight_intensity != 0; fp.ccw = p.radar_ccw != 0;
    const int cap = g.cfar ? std::min(rows * cols, 65536) : rows * g.k;
    int sg = -1;
    for (int i = 0; i < (int)pl.surf.size() && sg < 0; i++) {
      const GridSurfGroup& u = pl.surf[i];
      if (u.fp.radius == fp.radius && u.fp.downsample_factor == fp.downsample_factor && u.fp.weight_intensity == fp.weight_intensity &&
          u.fp.ccw == fp.ccw && u.cfar == g.cfar && u.range_res == g.range_res && u.row_k == g.row_k) sg = i;
    }
    if (sg < 0) {
      GridSurfGroup u; u.fp = fp; u.cfar = g.cfar; u.range_res = g.range_res; u.row_k = g.row_k;
      sg = (int)pl.surf.size();
      pl.surf.push_back(u);
    }
    pl.surf[sg].n++;
    pl.surf[sg].cap_points = std::max(pl.surf[sg].cap_points, cap);
    int mg = -1;
    for (int i = 0; i < (int)pl.reg.size() && mg < 0; i++)
      if (pl.reg[i].submap == p.submap_scan_size && memcmp(&pl.reg[i].reg, &p.reg, sizeof(p.reg)) == 0) mg = i;
    if (mg < 0) {
      GridRegGroup u; u.reg = p.reg; u.submap = p.submap_scan_size;
      mg = (int)pl.reg.size();
      pl.reg.push_back(u);
    }
    pl.reg[mg].n++;
    pl.streams[s].surface_group = sg; pl.streams[s].matcher_group = mg;
  }
  {
    int at = 0;
    for (GridSurfGroup& u : pl.surf) { u.first = at; at += u.n; u.n = 0; }
    at = 0;
    for (GridRegGroup& u : pl.reg) { u.first = at; at += u.n; u.n = 0; }
    for (int s = 0; s < n_streams; s++) {            // streams in index order inside a group
      GridSurfGroup& a = pl.surf[pl.streams[s].surface_group];
      GridRegGroup& b = pl.reg[pl.streams[s].matcher_group];
      pl.streams[s].surface_slot = a.first + a.n++;
      pl.streams[s].matcher_slot = b.first + b.n++;
    }
  }
  pl.totals.n_streams = n_streams; pl.totals.n_sequences = n_seq;
  pl.totals.n_sweeps = (int)pl.sweeps.size(); pl.totals.n_classes = (int)pl.classes.size();
  pl.totals.n_surface_groups = (int)pl.surf.size(); pl.totals.n_matcher_groups = (int)pl.reg.size();
  return CFEAR_OK;
}

}  // namespace

extern "C" int cfear_odometry_grid_plan(const cfear_polar_desc* desc, const cfear_odometry_params* configs, int32_t n_configs,
                                        const int32_t* stream_sequence, const int32_t* stream_config, int32_t n_streams,
                                        cfear_grid_stream* streams, cfear_grid_totals* totals, char* why, int32_t why_len) {
  GridPlan pl;
  std::string msg;
  const int rc = grid_plan(desc, configs, n_configs, stream_sequence, stream_config, n_streams, pl, msg);
  if (why && why_len > 0) snprintf(why, (size_t)why_len, "%s", msg.c_str());
  if (rc != CFEAR_OK) return rc;
  if (streams) memcpy(streams, pl.streams.data(), pl.streams.size() * sizeof(cfear_grid_stream));
  if (totals) *totals = pl.totals;
  return CFEAR_OK;
}

struct cfear_odometry_grid {
  cfear_ctx* ctx = nullptr;
  cfear_polar_desc in_desc{};
  GridPlan plan;
  std::vector<cfear_odometry_params> configs;
  int n_streams = 0, n_seq = 0;
  size_t slab_bytes = 0;
  DevBuf<uint8_t> d_polar, d_rot;            // staged host images; rotated images
  DevBuf<char> d_sel;                        // sel_range | sel_intensity | sel_count of ONE derived sweep (reused sweep by sweep)
  size_t sel_int_off = 0, sel_cnt_off = 0;
  DevBuf<KstrongDeriveClass> d_classes;      // [classes]: the records of the derived ones (the others unused)
  DevBuf<uint32_t> d_keys;                   // every class's row keys, class by class
  DevBuf<int32_t> d_cnt;                     // [classes][rows][2]
  std::vector<size_t> key_off;               // per class, in keys
  DevBuf<float> d_xyzi;                      // every stream's compacted cloud
  std::vector<size_t> xyzi_off;              // per stream, in points
  DevBuf<char> d_slabs, d_surf_jobs, d_reg_jobs, d_surf_scratch, d_reg_scratch, d_out;
  PinnedBuf<char> h_surf_jobs, h_reg_jobs, h_out;
  std::vector<size_t> surf_scratch_off, reg_scratch_off, reg_job_off, reg_stride;   // per group, bytes
  size_t reg_jobs_bytes = 0, out_bytes = 0;
  cfear_reg_result *d_results = nullptr, *h_results = nullptr;
  int32_t *d_status = nullptr, *d_ncells = nullptr, *d_npts = nullptr, *h_status = nullptr, *h_ncells = nullptr, *h_npts = nullptr;
  std::vector<StreamState> streams;
  std::vector<int> view0;                    // per stream: index of its first slab in views
  std::vector<ScanView> views;
  std::vector<double> cov, cost_est;         // the policy's side outputs (not handed out by a grid)
  std::vector<int32_t> cov_sampled;
  std::vector<std::vector<int>> reg_members; // per matcher group: its streams in slot order
  std::vector<int> reg_n_jobs;               // per matcher group: jobs of the current frame
  int big_regs = 0;
  // matcher groups beyond the first of a round run on these, forked from and joined into the context's stream by events
  static constexpr int kSide = 3;
  Stream side[kSide];
  Event ev_fork, ev_join[kSide];
};

// every stream of the object idle: what an error exit and the teardown need
static void grid_drain(cfear_odometry_grid* g) {
  for (auto& s : g->side) if (s) (void)hipStreamSynchronize(s.get());
  (void)hipStreamSynchronize(g->ctx->stream);
}

extern "C" int cfear_odometry_grid_destroy(cfear_odometry_grid* g) {
  if (!g) return CFEAR_OK;
  (void)hipSetDevice(g->ctx->device);
  grid_drain(g);
  delete g;
  return CFEAR_OK;
}

extern "C" int cfear_odometry_grid_create(cfear_ctx* ctx, const cfear_polar_desc* desc, const cfear_odometry_params* configs,
                                          int32_t n_configs, const int32_t* stream_sequence, const int32_t* stream_config,
                                          int32_t n_streams, cfear_odometry_grid** out) {
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (!out) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  *out = nullptr;
  std::unique_ptr<cfear_odometry_grid, FreeWith<cfear_odometry_grid_destroy>> g(new cfear_odometry_grid());
  g->ctx = ctx;
  std::string why;
  const int prc = grid_plan(desc, configs, n_configs, stream_sequence, stream_config, n_streams, g->plan, why);
  if (prc != CFEAR_OK) return cfear_set_error(ctx, prc, "%s", why.c_str());
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const GridPlan& pl = g->plan;
  g->in_desc = *desc; g->n_streams = n_streams; g->n_seq = desc->batch;
  g->configs.assign(configs, configs + n_configs);
  g->slab_bytes = cfear_scan_slab_bytes(kGridCellCap);
  const int S = n_streams, rows = pl.fdesc.rows;
  bool ok = true;
  auto dev = [&ok](auto& buf, size_t bytes) { ok = ok && (buf = dev_alloc<typename std::decay_t<decltype(buf)>::element_type>(std::max<size_t>(bytes, 16))); };
  auto pin = [&ok](auto& buf, size_t bytes) { ok = ok && (buf = pinned_alloc<typename std::decay_t<decltype(buf)>::element_type>(std::max<size_t>(bytes, 16))); };
  // filter classes: key tables one behind the other (the classes of a derived sweep at one stride, as the kernel writes them)
  size_t keys = 0;
  int k_sup_max = 0;
  for (const GridClass& c : pl.classes) { g->key_off.push_back(keys); keys += (size_t)rows * c.row_k; }
  for (const GridSweep& sw : pl.sweeps) if (sw.derive) k_sup_max = std::max(k_sup_max, sw.kp.k_strongest);
  dev(g->d_keys, keys * 4);
  dev(g->d_cnt, pl.classes.size() * (size_t)rows * 8);
  if (k_sup_max > 0) {
    const size_t nsel = (size_t)rows * k_sup_max;
    g->sel_int_off = nsel * 4;
    g->sel_cnt_off = g->sel_int_off + (nsel + 255) / 256 * 256;
    dev(g->d_sel, g->sel_cnt_off + (size_t)rows * 4);
    dev(g->d_classes, pl.classes.size() * sizeof(KstrongDeriveClass));
  }
  // streams: clouds and slabs
  size_t pts = 0, slabs = 0;
  g->view0.resize(S);
  for (int s = 0; s < S; s++) {
    const GridClass& c = pl.classes[pl.streams[s].filter_class];
    g->xyzi_off.push_back(pts);
    pts += c.cfar ? (size_t)std::min(rows * pl.fdesc.cols, 65536) : (size_t)rows * c.k;
    g->view0[s] = (int)slabs;
    slabs += (size_t)g->configs[pl.streams[s].config].submap_scan_size + 2;
  }
  dev(g->d_xyzi, pts * 16);
  dev(g->d_slabs, slabs * g->slab_bytes);
  // job tables and scratch, group by group
  const size_t sjb = cfear_surface_job_bytes();
  dev(g->d_surf_jobs, (size_t)S * sjb);
  pin(g->h_surf_jobs, (size_t)S * sjb);
  size_t at = 0;
  for (const GridSurfGroup& u : pl.surf) { g->surf_scratch_off.push_back(at); at += (size_t)u.n * cfear_surface_scratch_bytes(u.cap_points); }
  dev(g->d_surf_scratch, at);
  at = 0;
  size_t jobs_at = 0;
  for (const GridRegGroup& u : pl.reg) {
    g->reg_scratch_off.push_back(at);
    at += (size_t)u.n * reg_scratch_bytes(u.submap * kGridCellCap);
    g->reg_job_off.push_back(jobs_at);
    g->reg_stride.push_back(reg_job_stride(u.submap + 1));
    jobs_at += (size_t)u.n * g->reg_stride.back();
  }
  g->reg_jobs_bytes = jobs_at + sizeof(RegJob);     // a kernel may read a whole record behind the last short one
  dev(g->d_reg_scratch, at);
  dev(g->d_reg_jobs, g->reg_jobs_bytes);
  pin(g->h_reg_jobs, g->reg_jobs_bytes);
  g->out_bytes = (size_t)S * (sizeof(cfear_reg_result) + 12);
  dev(g->d_out, g->out_bytes);
  pin(g->h_out, g->out_bytes);
  // Side streams only behind a stream OBJECT: a context may also be given one of the runtime's stream handles (the null stream,
  // hipStreamLegacy, hipStreamPerThread), and an event recorded on such a handle must not be waited for on another stream
  // (odometry.hip, readback_on_copy_stream).  Behind a handle every group runs on the context's stream.
  const bool stream_object = ctx->stream != nullptr && ctx->stream != hipStreamLegacy && ctx->stream != hipStreamPerThread;
  if (pl.reg.size() > 1 && stream_object) {
    ok = ok && (g->ev_fork = make_event(hipEventDisableTiming));
    for (int i = 0; i < cfear_odometry_grid::kSide && i + 1 < (int)pl.reg.size(); i++)
      ok = ok && (g->side[i] = make_stream_nonblocking()) && (g->ev_join[i] = make_event(hipEventDisableTiming));
  }
  if (!ok) return cfear_set_error(ctx, CFEAR_ERR_HIP, "odometry grid buffers: allocation failed");
  auto carve = [&](char* base, cfear_reg_result*& r, int32_t*& st, int32_t*& nc, int32_t*& np) {
    r = (cfear_reg_result*)base;
    st = (int32_t*)(base + (size_t)S * sizeof(cfear_reg_result));
    nc = st + S; np = nc + S;
  };
  carve(g->d_out.get(), g->d_results, g->d_status, g->d_ncells, g->d_npts);
  carve(g->h_out.get(), g->h_results, g->h_status, g->h_ncells, g->h_npts);
  CFEAR_HIP_CHECK(ctx, hipMemset(g->d_out.get(), 0, g->out_bytes));
  if (g->d_classes) {                        // the derived classes' records, once
    std::vector<KstrongDeriveClass> h(pl.classes.size(), KstrongDeriveClass{0, 1, 0, 0});
    for (const GridSweep& sw : pl.sweeps) {
      if (!sw.derive) continue;
      const int u_sup = (int)(uint8_t)(int)sw.kp.z_min;
      for (int i = sw.first_class; i < sw.first_class + sw.n_classes; i++) {
        const GridClass& c = pl.classes[i];
        cfear_rowkeys_class in{0, c.k, c.kp.z_min, c.kp.range_res, c.kp.min_distance};   // image 0: a sweep has one image
        if (!cfear_kstrong_derive_class(&in, 1, sw.kp.k_strongest, u_sup, &h[i]))
          return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "filter class %d is no subset of its sweep", i);
      }
    }
    CFEAR_HIP_CHECK(ctx, hipMemcpy(g->d_classes.get(), h.data(), h.size() * sizeof(KstrongDeriveClass), hipMemcpyHostToDevice));
  }
  g->streams.resize(S);
  g->views.resize(slabs);
  for (int s = 0; s < S; s++) {
    const int n = g->configs[pl.streams[s].config].submap_scan_size + 2;
    for (int i = 0; i < n; i++) {
      g->views[(size_t)g->view0[s] + i] = cfear_scan_view(g->d_slabs.get() + ((size_t)g->view0[s] + i) * g->slab_bytes, kGridCellCap);
      g->streams[s].free_slabs.push_back(n - 1 - i);
    }
  }
  g->cov.assign((size_t)S * 36, 0.0);
  for (int s = 0; s < S; s++)
    for (int k = 0; k < 6; k++) g->cov[(size_t)s * 36 + k * 7] = 1.0;          // cov_current = Identity
  g->cov_sampled.assign(S, 0);
  g->cost_est.assign(S, 0.0);
  g->reg_members.resize(pl.reg.size());
  g->reg_n_jobs.assign(pl.reg.size(), 0);
  for (int s = 0; s < S; s++) g->reg_members[pl.streams[s].matcher_group].push_back(s);   // index order = slot order
  *out = g.release();
  return CFEAR_OK;
}

// ---- F: the sweeps of one frame -------------------------------------------------------------------------------------------
static int grid_sweeps(cfear_odometry_grid* g, const uint8_t* polar) {
  cfear_ctx* ctx = g->ctx;
  const GridPlan& pl = g->plan;
  const int Q = g->n_seq;
  const uint8_t* d_polar = polar;
  cfear_polar_desc dd = g->in_desc;
  if (!cfear_is_device_ptr(polar)) {
    const size_t img_bytes = (size_t)g->in_desc.rows * g->in_desc.stride;
    if (!g->d_polar && !(g->d_polar = dev_alloc<uint8_t>(img_bytes * Q))) return cfear_set_error(ctx, CFEAR_ERR_HIP, "staging allocation failed");
    const int64_t bs = Q > 1 ? g->in_desc.batch_stride : (int64_t)img_bytes;
    if (bs == (int64_t)img_bytes) {
      CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(g->d_polar.get(), polar, img_bytes * Q, hipMemcpyHostToDevice, ctx->stream));
    } else {
      for (int q = 0; q < Q; q++)
        CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(g->d_polar.get() + (size_t)q * img_bytes, polar + (size_t)q * bs, img_bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    d_polar = g->d_polar.get();
    dd.batch_stride = (int64_t)img_bytes;
  }
  if (pl.rotate) {                           // once per sequence image; the row sweeps follow (no fused decode in a grid)
    const size_t rot_bytes = (size_t)pl.fdesc.rows * pl.fdesc.stride;
    if (!g->d_rot && !(g->d_rot = dev_alloc<uint8_t>(rot_bytes * Q))) return cfear_set_error(ctx, CFEAR_ERR_HIP, "rotation buffer allocation failed");
    CFEAR_CHECK(cfear_rotate_ccw_device(ctx, d_polar, &dd, g->d_rot.get(), pl.fdesc.stride, (int64_t)rot_bytes));
    d_polar = g->d_rot.get();
    dd = pl.fdesc;
  }
  const int64_t img_stride = Q > 1 ? dd.batch_stride : (int64_t)dd.rows * dd.stride;
  cfear_polar_desc d1 = dd;
  d1.batch = 1; d1.batch_stride = (int64_t)dd.rows * dd.stride;
  const int rows = pl.fdesc.rows;
  for (const GridSweep& sw : pl.sweeps) {
    const uint8_t* img = d_polar + (int64_t)sw.sequence * img_stride;
    uint32_t* keys = g->d_keys.get() + g->key_off[sw.first_class];
    int32_t* cnt = g->d_cnt.get() + (size_t)sw.first_class * rows * 2;
    if (sw.cfar) {
      cfear_cacfar_params cp = sw.cp;
      cfear_cacfar_fused fz;
      fz.row_keys = keys; fz.row_cnt = cnt; fz.kcap = pl.classes[sw.first_class].row_k;
      CFEAR_CHECK(cfear_cacfar_device(ctx, img, &d1, &cp, nullptr, nullptr, std::min(rows * pl.fdesc.cols, 65536), nullptr, &fz));
    } else if (!sw.derive) {                 // one class: the fused row-key sweep, as the plain pipeline runs it
      cfear_kstrong_out none{};
      cfear_kstrong_fused fz;
      fz.row_keys = keys; fz.row_valid = cnt;
      CFEAR_CHECK(cfear_kstrong_device(ctx, img, &d1, &sw.kp, &none, pl.rotate != 0, &fz));
    } else {                                 // several: the superset's sel_* lists, then every class's keys from them
      cfear_kstrong_out o{};
      o.sel_range = (int32_t*)g->d_sel.get();
      o.sel_intensity = (uint8_t*)(g->d_sel.get() + g->sel_int_off);
      o.sel_count = (int32_t*)(g->d_sel.get() + g->sel_cnt_off);
      CFEAR_CHECK(cfear_kstrong_device(ctx, img, &d1, &sw.kp, &o, pl.rotate != 0));
      CFEAR_CHECK(cfear_kstrong_derive_device(ctx, o.sel_range, o.sel_intensity, o.sel_count, rows, sw.kp.k_strongest,
                                              g->d_classes.get() + sw.first_class, sw.n_classes, keys, cnt));
    }
  }
  return CFEAR_OK;
}

// The matcher over this frame's jobs, group by group; big_pass adds the large forms.  Group m runs on lane m % (1 + side
// streams): lane 0 is the context's stream, the others wait for everything enqueued on it so far (the job upload, the surface
// kernels) and are joined back into it before the read-back.
static int grid_register(cfear_odometry_grid* g, bool big_pass) {
  cfear_ctx* ctx = g->ctx;
  const GridPlan& pl = g->plan;
  RegLaunchHint hint;
  hint.big_pass = big_pass;
  int lanes = 1;
  while (lanes <= cfear_odometry_grid::kSide && g->side[lanes - 1]) lanes++;
  hipStream_t const main_stream = ctx->stream;
  bool used[cfear_odometry_grid::kSide] = {false, false, false};
  if (lanes > 1) CFEAR_HIP_CHECK(ctx, hipEventRecord(g->ev_fork.get(), main_stream));
  int rc = CFEAR_OK, lane = 0;
  for (size_t m = 0; m < pl.reg.size() && rc == CFEAR_OK; m++) {
    if (g->reg_n_jobs[m] == 0) continue;
    const GridRegGroup& u = pl.reg[m];
    if (lane > 0 && !used[lane - 1]) {
      if (hipStreamWaitEvent(g->side[lane - 1].get(), g->ev_fork.get(), 0) != hipSuccess) { rc = cfear_set_error(ctx, CFEAR_ERR_HIP, "stream fork failed"); break; }
      used[lane - 1] = true;
    }
    ctx->stream = lane == 0 ? main_stream : g->side[lane - 1].get();      // the launcher enqueues on the context's stream
    rc = cfear_register_launch(ctx, g->d_reg_jobs.get() + g->reg_job_off[m], g->reg_n_jobs[m], &u.reg, u.submap * kGridCellCap,
                               g->d_reg_scratch.get() + g->reg_scratch_off[m], g->d_results + u.first, nullptr, g->reg_stride[m], hint);
    ctx->stream = main_stream;
    lane = (lane + 1) % lanes;
  }
  for (int i = 0; i < cfear_odometry_grid::kSide; i++) {                  // join what was forked, also behind an error
    if (!used[i]) continue;
    if (hipEventRecord(g->ev_join[i].get(), g->side[i].get()) != hipSuccess || hipStreamWaitEvent(main_stream, g->ev_join[i].get(), 0) != hipSuccess)
      if (rc == CFEAR_OK) rc = cfear_set_error(ctx, CFEAR_ERR_HIP, "stream join failed");
  }
  return rc;
}

extern "C" int cfear_odometry_grid_process(cfear_odometry_grid* g, const uint8_t* polar, cfear_frame_info* info) {
  if (!g || !polar || !info) return CFEAR_ERR_INVALID_ARGUMENT;
  cfear_ctx* ctx = g->ctx;
  const GridPlan& pl = g->plan;
  const int S = g->n_streams, rows = pl.fdesc.rows;
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  for (int s = 0; s < S; s++)
    if (g->streams[s].free_slabs.empty()) return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "stream %d: no free scan slab", s);
  int rc = grid_sweeps(g, polar);
  if (rc != CFEAR_OK) { grid_drain(g); return rc; }
  // ---- C + N: one job per stream at its surface slot; its class's keys, its own motion and compensate flag
  const size_t sjb = cfear_surface_job_bytes();
  for (int s = 0; s < S; s++) {
    StreamState& st = g->streams[s];
    const cfear_grid_stream& gs = pl.streams[s];
    const cfear_odometry_params& par = g->configs[gs.config];
    const GridClass& c = pl.classes[gs.filter_class];
    st.cur_slab = st.free_slabs.back();
    st.free_slabs.pop_back();
    double mot[3];
    aff_to_xyt(st.Tmot, mot);                                     // Compensate(cloud, TprevMot, ccw)
    cfear_surface_fill_job_rows(g->h_surf_jobs.get() + (size_t)gs.surface_slot * sjb, g->d_xyzi.get() + g->xyzi_off[s] * 4,
                                g->d_npts + gs.surface_slot, g->d_keys.get() + g->key_off[gs.filter_class],
                                g->d_cnt.get() + (size_t)gs.filter_class * rows * 2, rows, c.row_k, par.compensate, mot,
                                g->views[(size_t)g->view0[s] + st.cur_slab]);
  }
  // From here on every stream holds a slab: an error exit hands the slabs back and leaves the stream idle.
  auto fail = [&](int code) {
    grid_drain(g);
    for (int s = 0; s < S; s++) {
      StreamState& st = g->streams[s];
      if (st.cur_slab >= 0) { st.free_slabs.push_back(st.cur_slab); st.cur_slab = -1; }
    }
    return code;
  };
#define GRID_CHECK(expr)                                                                                      \
  do {                                                                                                        \
    hipError_t _e = (expr);                                                                                   \
    if (_e != hipSuccess)                                                                                     \
      return fail(cfear_set_error(ctx, CFEAR_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__)); \
  } while (0)
  // (the pinned tables are free: every call ends with the stream idle)
  GRID_CHECK(hipMemcpyAsync(g->d_surf_jobs.get(), g->h_surf_jobs.get(), (size_t)S * sjb, hipMemcpyHostToDevice, ctx->stream));
  double *d_cos = nullptr, *d_sin = nullptr;
  rc = cfear_trig_tables(ctx, rows, &d_cos, &d_sin);
  if (rc != CFEAR_OK) return fail(rc);
  for (size_t i = 0; i < pl.surf.size(); i++) {
    const GridSurfGroup& u = pl.surf[i];
    cfear_surface_polar sp;
    sp.cos_t = d_cos; sp.sin_t = d_sin; sp.rows = rows; sp.k = u.row_k;
    sp.range_res = (double)u.range_res;
    sp.range_off = u.cfar ? 0.0 : sp.range_res / 2.0;             // cfar.cpp:43 / radar_filters.cpp:324
    rc = cfear_surface_launch(ctx, g->d_surf_jobs.get() + (size_t)u.first * sjb, u.n, &u.fp, g->d_surf_scratch.get() + g->surf_scratch_off[i],
                              g->d_status + u.first, g->d_ncells + u.first, kGridCellCap, u.cap_points, &sp);
    if (rc != CFEAR_OK) return fail(rc);
  }
  // ---- M: the registration jobs depend on host state only; a group's jobs are its streams with a keyframe, in slot order
  int n_jobs = 0;
  std::vector<ScanView> views(kRegMaxScans);
  std::vector<double> poses(3 * (size_t)kRegMaxScans);
  for (size_t m = 0; m < pl.reg.size(); m++) {
    int n = 0;
    for (int s : g->reg_members[m]) {
      StreamState& st = g->streams[s];
      frame_policy_guess(st, g->configs[pl.streams[s].config]);
      st.job = -1;
      if (st.keyframes.empty()) continue;                         // first frame: no registration
      const int ns = (int)st.keyframes.size() + 1;                // FormatScans :478-494
      for (int i = 0; i < ns - 1; i++) {
        views[i] = g->views[(size_t)g->view0[s] + st.keyframes[i].slab];
        aff_to_xyt(st.keyframes[i].pose, &poses[3 * i]);
      }
      views[ns - 1] = g->views[(size_t)g->view0[s] + st.cur_slab];
      aff_to_xyt(st.Tguess, &poses[3 * (ns - 1)]);
      cfear_reg_fill_job(g->h_reg_jobs.get() + g->reg_job_off[m] + (size_t)n * g->reg_stride[m], views.data(), ns, poses.data());
      st.job = pl.reg[m].first + n++;
    }
    g->reg_n_jobs[m] = n;
    n_jobs += n;
  }
  const bool launched_big = g->big_regs > 0;
  if (n_jobs > 0) {
    GRID_CHECK(hipMemcpyAsync(g->d_reg_jobs.get(), g->h_reg_jobs.get(), g->reg_jobs_bytes - sizeof(RegJob), hipMemcpyHostToDevice, ctx->stream));
    rc = grid_register(g, launched_big);
    if (rc != CFEAR_OK) return fail(rc);
  }
  GRID_CHECK(hipMemcpyAsync(g->h_out.get(), g->d_out.get(), g->out_bytes, hipMemcpyDeviceToHost, ctx->stream));
  GRID_CHECK(hipStreamSynchronize(ctx->stream));
  if (n_jobs > 0 && !launched_big) {
    // a registration too large for the first form of a launch without the large forms: run the frame's jobs again with them
    // on, and keep them on for the frames to come (as cfear_odometry_process does)
    bool retry = false;
    for (int s = 0; s < S && !retry; s++) {
      const int j = g->streams[s].job;
      retry = j >= 0 && g->h_results[j].status == CFEAR_ERR_CAPACITY && g->h_results[j].reserved != 0.0;
    }
    if (retry) {
      rc = grid_register(g, true);
      if (rc != CFEAR_OK) return fail(rc);
      GRID_CHECK(hipMemcpyAsync(g->h_results, g->d_results, (size_t)S * sizeof(cfear_reg_result), hipMemcpyDeviceToHost, ctx->stream));
      GRID_CHECK(hipStreamSynchronize(ctx->stream));
    }
  }
#undef GRID_CHECK
  // ---- frame policy, per stream with its own configuration ----
  int first_error = CFEAR_OK;
  bool saw_big = false;
  for (int s = 0; s < S; s++) {
    StreamState& st = g->streams[s];
    const int slot = pl.streams[s].surface_slot;
    FrameOutcome fo;
    fo.n_points = g->h_npts[slot]; fo.n_cells = g->h_ncells[slot]; fo.status = g->h_status[slot];
    if (st.job >= 0) fo.rr = g->h_results + st.job;
    const int src = frame_policy_apply(st, g->configs[pl.streams[s].config], fo, nullptr, g->cov.data() + (size_t)s * 36, &g->cov_sampled[s],
                                       &g->cost_est[s], &saw_big, info[s]);
    if (src != CFEAR_OK && first_error == CFEAR_OK)
      first_error = cfear_set_error(ctx, src, "stream %d: surface points failed (%s)", s, cfear_status_string(src));
    st.cur_slab = -1;                                             // the slab is a keyframe or back on the free list
  }
  g->big_regs = saw_big ? 64 : std::max(0, g->big_regs - 1);
  return first_error;
}
