// odometry_policy.hpp -- the per-stream frame policy of OdometryKeyframeFuser::processFrame (odometrykeyframefuser.cpp:
// 164-168, 195-257) as host code, once: the constant-velocity guess, the sanity check, the keyframe test, the sliding
// keyframe window, the slab hand-back and Register's constant covariance.  cfear_odometry (odometry.hip: one parameter set
// for all of its streams) and cfear_odometry_grid (odometry_grid.hip: one per stream) both advance their streams with it.
#pragma once
#include <vector>

#include "covfit.hpp"
#include "registration.hpp"

struct Keyframe { int slab; Aff2 pose; uint64_t idx = 0; };
struct StreamState {
  Aff2 T_prev = aff_identity(), Tmot = aff_identity(), Tcurrent = aff_identity();
  std::vector<Keyframe> keyframes;
  std::vector<int> free_slabs;
  int cur_slab = -1;
  Aff2 Tguess = aff_identity();
  int job = -1;              // index into this call's registration batch, -1 = first frame
  uint64_t n_keyframes = 0;  // RadarScan::counter of this stream
  bool has_constraint = false;          // the last frame added a keyframe behind another one (AddToGraph)
  uint64_t c_from = 0, c_to = 0;
  Aff2 c_Tdiff = aff_identity();
  double c_cov[36] = {0};
};

// :164-168: where the registration of this frame starts
inline void frame_policy_guess(StreamState& st, const cfear_odometry_params& par) {
  st.Tguess = par.use_guess ? aff_mul(st.T_prev, st.Tmot) : st.T_prev;
}

// What a frame's kernels left for one stream: the surface stage's counts and status, and -- where the stream had a keyframe
// to register against (st.job >= 0) -- its registration record and, with cost sampling, the fit.m records around it.
struct FrameOutcome {
  int32_t n_points = 0, n_cells = 0, status = CFEAR_OK;
  const cfear_reg_result* rr = nullptr;
  const cfear_reg_result* samples = nullptr;
};

// Applies the frame to the stream (:195-257) and fills its cfear_frame_info.  cv [36] / cov_sampled: the stream's cov_current;
// cost_est: the work of its registration (orders the next batch); saw_big is set where the registration needed a large form.
// Returns the surface stage's status where that failed (the stream then keeps its state), CFEAR_OK otherwise.
inline int frame_policy_apply(StreamState& st, const cfear_odometry_params& par, const FrameOutcome& o, CovFit* fit, double* cv,
                              int32_t* cov_sampled, double* cost_est, bool* saw_big, cfear_frame_info& fi) {
  memset(&fi, 0, sizeof(fi));
  fi.n_points = o.n_points;
  fi.n_cells = o.n_cells;
  st.has_constraint = false;                                    // whatever this frame does, the last constraint is no longer "the last frame's"
  if (o.status != CFEAR_OK) {
    // empty cloud / capacity: the reference would exit(0) (pointnormal.cpp:72-75); report and keep the state
    fi.reg_status = o.status;
    st.free_slabs.push_back(st.cur_slab);
    aff_to_xyt(st.Tcurrent, fi.pose);
    return o.status;
  }
  if (st.job < 0) {                                             // first frame becomes the first keyframe
    st.keyframes.push_back(Keyframe{st.cur_slab, aff_identity(), st.n_keyframes++});
    fi.keyframe_added = 1;
    fi.reg_status = 1;
    aff_to_xyt(st.Tcurrent, fi.pose);
    return CFEAR_OK;
  }
  const cfear_reg_result& rr = *o.rr;
  fi.reg_status = rr.status; fi.outer_iters = rr.outer_iters; fi.lm_iters = rr.lm_iters; fi.score = rr.score;
  *cost_est = (double)rr.num_residuals * (3.0 * rr.outer_iters + rr.lm_iters);   // association ~ 3 LM iterations
  if (rr.reserved != 0.0) *saw_big = true;
  {                                                             // cov_current = cov_vek.back() (:196)
    for (int k = 0; k < 36; k++) cv[k] = 0.0;
    if (rr.status == CFEAR_OK) { cv[0] = 0.1 * 0.1; cv[7] = 0.1 * 0.1; cv[35] = 0.01 * 0.01; }   // n_scan_normal.cpp:171-175
    else for (int k = 0; k < 6; k++) cv[k * 7] = 1.0;          // FormatScans' Identity66 survives a failed Register
    *cov_sampled = 0;
    if (par.estimate_cov_by_sampling && rr.num_residuals - 3 != 0) {         // GetCovarianceScaler (:433-439)
      const int m = fit->m;
      std::vector<double> costs(m);
      double sample_cost = 0.0;                                 // a failed GetCost keeps the previous value (:282, 307)
      for (int s = 0; s < m; s++) {
        const cfear_reg_result& sr = o.samples[s];
        if (sr.status == CFEAR_OK) sample_cost = sr.final_cost;
        costs[s] = sample_cost;
      }
      double c36[36];
      if (fit->solve(costs.data(), rr.final_cost / (double)(rr.num_residuals - 3), par.cov_sampling.covariance_scaler, c36)) {
        memcpy(cv, c36, sizeof(c36));
        *cov_sampled = 1;
      }
    }
  }
  // Tcurrent = T_vek.back(): Register rewrites Tsrc via vectorToAffine3d (registration failures are
  // ignored by the reference: `bool success` is shadowed, odometrykeyframefuser.cpp:184-193)
  Aff2 Tcurrent = aff_from_xyt(rr.pose);
  {                                                             // AccelerationVelocitySanityCheck :76-94
    const Aff2 Tmot_current = aff_mul(aff_inv(st.T_prev), Tcurrent);
    const double prev_xy[2] = {st.Tmot.t0, st.Tmot.t1}, curr_xy[2] = {Tmot_current.t0, Tmot_current.t1};
    if (!cfear_acc_vel_sanity_check(prev_xy, curr_xy)) Tcurrent = st.Tguess;            // :198-199
  }
  st.Tmot = aff_mul(aff_inv(st.T_prev), Tcurrent);              // :200
  const Aff2 Tkeydiff = aff_mul(aff_inv(st.keyframes.back().pose), Tcurrent);
  double kd[3];
  aff_to_xyt(Tkeydiff, kd);
  const bool fuse = cfear_keyframe_based_fuse(kd, par.use_keyframe, par.min_keyframe_dist, par.min_keyframe_rot_deg) != 0;   // :62-73
  if (fuse) {                                                   // :236-250, AddToReference :470-476
    {                                                           // AddToGraph :428-445: constraint to the latest keyframe
      const Keyframe& to = st.keyframes.back();
      st.has_constraint = true;
      st.c_from = st.n_keyframes; st.c_to = to.idx;
      st.c_Tdiff = aff_mul(aff_inv(Tcurrent), to.pose);         // Tfrom^-1 * Tto
      memcpy(st.c_cov, cv, sizeof(st.c_cov));
      // C.block<3,3>(0,0) = Tfrom^-1.rotation() * Cov.block<3,3>(0,0) * Tfrom^-1.rotation()^T
      const Aff2 Ti = aff_inv(Tcurrent);
      const double R[9] = {Ti.l0, Ti.l1, 0, Ti.l2, Ti.l3, 0, 0, 0, 1};
      double t[9], o3[9];
      for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) { t[r * 3 + c] = 0; for (int k = 0; k < 3; k++) t[r * 3 + c] += R[r * 3 + k] * cv[k * 6 + c]; }
      for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) { o3[r * 3 + c] = 0; for (int k = 0; k < 3; k++) o3[r * 3 + c] += t[r * 3 + k] * R[c * 3 + k]; }
      for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) st.c_cov[r * 6 + c] = o3[r * 3 + c];
    }
    st.keyframes.push_back(Keyframe{st.cur_slab, Tcurrent, st.n_keyframes++});
    if ((int)st.keyframes.size() > par.submap_scan_size) {
      st.free_slabs.push_back(st.keyframes.front().slab);
      st.keyframes.erase(st.keyframes.begin());
    }
    fi.keyframe_added = 1;
  } else {
    st.free_slabs.push_back(st.cur_slab);
  }
  st.Tcurrent = Tcurrent;
  st.T_prev = Tcurrent;                                         // :257
  aff_to_xyt(Tcurrent, fi.pose);
  return CFEAR_OK;
}
