// cfear_hip.hpp -- header-only C++ mirror of the reference's cfear_radarodometry classes over the C-ABI
// (include/cfear_hip.h).  Same class and method names as namespace CFEAR_Radarodometry:
//   radarDriver            radar_driver.h:32-118       CallbackOffline -> filtered cloud + peaks cloud
//   MapPointNormal         pointnormal.h:110-243       GetSize / GetCells / device handle
//   n_scan_normal_reg      n_scan_normal.h:27-85       SetParameters / Register / GetCost / getScore
// ROS / PCL / Eigen types are replaced by PODs so the header compiles anywhere a C++14 compiler and
// libcfear_hip.so exist; the Eigen/PCL adapters at the bottom are compiled only where those headers are
// installed (they are not in this image).  Errors are C++ exceptions carrying the C status code.
#pragma once
#include <cstdint>
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <ctime>
#include <fstream>
#include <iostream>
#include <map>
#include <memory>
#include <stdexcept>
#include <sstream>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "cfear_hip.h"

// Where Eigen, PCL and boost::shared_ptr exist (a ROS Noetic host; they are NOT in this image), the classes below also
// carry the reference's EXACT signatures -- Eigen::Affine3d poses, pcl::PointCloud<pcl::PointXYZI>::Ptr clouds,
// MapNormalPtr, Matrix6d covariances (n_scan_normal.h:37-41, pointnormal.h:110-118, odometrykeyframefuser.h:197-249) --
// forwarding to the POD methods.  tests/test_cpp_shim.py compiles this block against minimal stand-in headers (a syntax
// check of THIS header only; it proves nothing about Eigen or PCL).
#if defined(__has_include)
#if __has_include(<Eigen/Geometry>) && __has_include(<pcl/point_cloud.h>) && __has_include(<pcl/point_types.h>) && __has_include(<boost/shared_ptr.hpp>)
#define CFEAR_HIP_HAVE_EIGEN_PCL 1
#include <Eigen/Geometry>
#include <boost/shared_ptr.hpp>
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>
#if __has_include(<cv_bridge/cv_bridge.h>)
#define CFEAR_HIP_HAVE_CV_BRIDGE 1
#include <cv_bridge/cv_bridge.h>
#endif
#endif
#endif

namespace CFEAR_Radarodometry {

#ifdef CFEAR_HIP_HAVE_EIGEN_PCL
typedef Eigen::Matrix<double, 6, 6> Matrix6d;                // registration.h
typedef Eigen::Matrix<double, 6, 6> Covariance;             // types.h
typedef enum costmetric { P2P, P2L, P2D } cost_metric;                                        // registration.h:55
typedef enum losstype { None, Huber, Cauchy, SoftLOne, Combined, Tukey } loss_type;           // registration.h:60
typedef enum weight_options { Uniform = 0, Sim_N = 1, Sim_direciton = 2, Sim_scale = 3, Combined_weights = 4 } weightoption;   // :50
#endif

struct PointXYZI { float x, y, z, intensity; };            // 16-byte PointXYZI payload
typedef std::vector<PointXYZI> PointCloud;
struct Pose2d { double x, y, theta; };                     // Affine3dToVectorXYeZ (utils.cpp:115-122)

// eval_trajectory.h:57-64 as a POD: the KITTI row of the pose (the rows of the 3 x 4 matrix), the 6 x 6 covariance row-major,
// and the stamp in nanoseconds (ros::Time::toNSec())
struct poseStamped {
  std::array<double, 12> pose{{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}};
  std::array<double, 36> cov{};
  int64_t t = 0;
  poseStamped() {}
  poseStamped(const std::array<double, 12>& _pose, const std::array<double, 36>& _cov, int64_t _t) : pose(_pose), cov(_cov), t(_t) {}
  poseStamped(const Pose2d& p, int64_t _t) : t(_t) {
    cfear_kitti_from_xyt(&p.x, 1, 3, pose.data());
  }
};
typedef std::vector<poseStamped> poseStampedVector;

struct CfearError : std::runtime_error {
  int status;
  CfearError(int st, const std::string& msg) : std::runtime_error(msg), status(st) {}
};

class Context {                                            // one per host thread
 public:
  explicit Context(int device = 0, void* hip_stream = nullptr) {
    const int st = cfear_ctx_create(device, hip_stream, &ctx_);
    if (st != CFEAR_OK) throw CfearError(st, cfear_status_string(st));
  }
  ~Context() { cfear_ctx_destroy(ctx_); }
  Context(const Context&) = delete;
  Context& operator=(const Context&) = delete;
  cfear_ctx* get() const { return ctx_; }
  void check(int st) const { if (st != CFEAR_OK) throw CfearError(st, cfear_last_error(ctx_)); }
  void* Stream() const { void* s = nullptr; check(cfear_ctx_get_stream(ctx_, &s)); return s; }      // the hipStream_t it enqueues on
  void SetOption(cfear_option o, int64_t v) { check(cfear_ctx_set_option(ctx_, o, v)); }           // test / measurement hooks
  // The context of the calling thread on device 0, for the reference-signature constructors that take none
  // (the reference's objects are not shared between threads either).
  static Context& Default() { static thread_local Context c(0); return c; }
 private:
  cfear_ctx* ctx_ = nullptr;
};

#ifdef CFEAR_HIP_HAVE_EIGEN_PCL
inline Pose2d Affine3dToPose2d(const Eigen::Affine3d& T) {                                    // utils.cpp:115-122
  const Eigen::Vector3d eul = T.linear().eulerAngles(0, 1, 2);
  return Pose2d{T.translation()(0), T.translation()(1), eul(2)};
}
inline Eigen::Affine3d Pose2dToAffine3d(const Pose2d& p) {                                    // registration.cpp:128-135
  return Eigen::Translation3d(p.x, p.y, 0) * Eigen::AngleAxisd(p.theta, Eigen::Vector3d::UnitZ());
}
inline PointCloud FromPcl(const pcl::PointCloud<pcl::PointXYZI>& c) {
  PointCloud out(c.points.size());
  for (size_t i = 0; i < c.points.size(); i++) out[i] = PointXYZI{c.points[i].x, c.points[i].y, c.points[i].z, c.points[i].intensity};
  return out;
}
#endif

enum filtertype { kstrong, CACFAR };                       // radar_driver.h:25
inline filtertype Str2filter(const std::string& str) { return str == "CA-CFAR" ? CACFAR : kstrong; }       // radar_driver.cpp:7-13
inline std::string Filter2str(const filtertype& filter) { return filter == CACFAR ? "CA-CFAR" : "kstrong"; }   // :15-21

class radarDriver {
 public:
  struct Parameters {                                      // radar_driver.h:35-84
    float z_min = 60; float range_res = 0.0438f; int azimuths = 400, k_strongest = 12;
    int nb_guard_cells = 20, window_size = 10; float false_alarm_rate = 0.01f;
    float min_distance = 2.5f, max_distance = 200; filtertype filter_type_ = kstrong;
    std::string dataset = "oxford";                        // anything else: images arrive as [range bins][azimuths]
    std::string topic_filtered = "/Navtech/Filtered", radar_frameid = "sensor_est";
    std::string ToString() const {                         // radar_driver.h:65-82 (what the evaluation scripts log)
      std::ostringstream ss;
      ss << "range res, " << range_res << std::endl << "z min, " << z_min << std::endl << "min distance, " << min_distance << std::endl
         << "max distance, " << max_distance << std::endl << "k strongest, " << k_strongest << std::endl
         << "topic_filtered, " << topic_filtered << std::endl << "radar_frameid, " << radar_frameid << std::endl
         << "dataset, " << dataset << std::endl << "filter type, " << Filter2str(filter_type_) << std::endl
         << "nb guard cells, " << nb_guard_cells << std::endl << "window size, " << window_size << std::endl
         << "false alarm rate, " << false_alarm_rate << std::endl;
      return ss.str();
    }
  };
  radarDriver(Context& ctx, const Parameters& pars) : ctx_(ctx), par(pars) {}
  // image: row-major uint8; rows = azimuth for dataset "oxford" (CallbackOxford, radar_driver.cpp:99-111), otherwise
  // rows = range bins and the image is rotated 90 degrees counter-clockwise first (Callback, :74-90)
  std::vector<uint8_t> cv_polar_image;                     // the image the filters saw (non-Oxford: rotated copy)
  void CallbackOffline(const uint8_t* image, int rows, int cols, int stride, PointCloud& cloud, PointCloud& cloud_peaks) {
    if (par.dataset != "oxford") {
      cv_polar_image.resize((size_t)rows * cols);
      cfear_polar_desc s{rows, cols, stride, 1, 0};
      ctx_.check(cfear_polar_rotate_ccw(ctx_.get(), image, &s, cv_polar_image.data(), rows, 0));
      image = cv_polar_image.data();
      std::swap(rows, cols);
      stride = cols;
    }
    cfear_polar_desc d{rows, cols, stride, 1, 0};
    int32_t n = 0, n_pk = 0;
    if (par.filter_type_ == CACFAR) {                      // radar_driver.cpp:52-56
      cfear_cacfar_params p{par.window_size, par.nb_guard_cells, par.false_alarm_rate, par.range_res, par.z_min,
                            par.min_distance, 400.0};
      cloud.resize((size_t)rows * cols);
      ctx_.check(cfear_filter_cacfar(ctx_.get(), image, &d, &p, &cloud[0].x, &n, rows * cols, nullptr));
      cloud.resize(n);
      cloud_peaks.clear();
      return;
    }
    cfear_kstrong_params p{par.k_strongest, par.z_min, par.range_res, par.min_distance, 1};
    cloud.resize((size_t)rows * par.k_strongest);
    cloud_peaks.resize((size_t)rows * par.k_strongest);
    cfear_kstrong_out o{};
    o.xyzi = &cloud[0].x; o.n_points = &n; o.xyzi_peaks = &cloud_peaks[0].x; o.n_peaks = &n_pk;
    ctx_.check(cfear_filter_kstrongest(ctx_.get(), image, &d, &p, &o));
    cloud.resize(n);
    cloud_peaks.resize(n_pk);
  }
 private:
  Context& ctx_;
  Parameters par;
};

inline void Compensate(Context& ctx, PointCloud& cloud, const Pose2d& mot, bool ccw) {     // utils.cpp:96-107
  const double m[3] = {mot.x, mot.y, mot.theta};
  if (!cloud.empty()) ctx.check(cfear_compensate(ctx.get(), &cloud[0].x, (int32_t)cloud.size(), m, ccw ? 1 : 0));
}

// ---- statistics.h:19-42 / statistics.cpp: the global `timing` the callers document their stage times into ----------
class statistics {
 public:
  void Document(const std::string& name, const double& value, bool report = false) {
    t_[name].push_back(value);
    if (report) std::cout << "Statistics: \"" << name << "\" = " << value << std::endl;
  }
  void PresentStatistics() {
    std::cout << "-------------- EXECUTION STATISTICS ---------------" << std::endl;
    for (const auto& r : Compute())
      std::cout << "\"" << std::get<0>(r) << "\" - mean: " << std::get<1>(r) << ", sigma: " << std::get<2>(r) << ", N: " << std::get<3>(r) << std::endl;
    std::cout << "---------FINGERS CROSSED FOR GOOD RESUTLS --------" << std::endl;
  }
  std::string GetStatistics() {                                    // the text the evaluation scripts parse
    std::string str;
    for (const auto& r : Compute()) {
      str += std::get<0>(r) + std::string(" avg, ") + std::to_string(std::get<1>(r)) + "\n";
      str += std::get<0>(r) + std::string(" dev [\xcf\x83], ") + std::to_string(std::get<2>(r)) + "\n";   // "σ"; the VARIANCE, as in the reference
      str += std::get<0>(r) + std::string(" count, ") + std::to_string(std::get<3>(r)) + "\n";
    }
    return str;
  }
 private:
  typedef std::tuple<std::string, double, double, int> reports;    // name, mean, variance, N samples
  std::vector<reports> Compute() const {
    std::vector<reports> rep;
    for (const auto& kv : t_) {
      double sum = 0, var = 0;
      for (double v : kv.second) sum += v;
      const double mean = sum / (double)kv.second.size();
      for (double v : kv.second) var += (v - mean) * (v - mean);
      rep.emplace_back(kv.first, mean, var / (double)kv.second.size(), (int)kv.second.size());
    }
    return rep;
  }
  std::map<std::string, std::vector<double>> t_;
};
inline statistics& timing_singleton() { static statistics s; return s; }
static statistics& timing = timing_singleton();                    // `extern statistics timing` (statistics.h:38), header-only
inline double ToMs(double seconds) { return seconds * 1000.0; }
template <class Duration> inline auto ToMs(const Duration& dur) -> decltype(dur.toNSec() / 1000000.0) { return dur.toNSec() / 1000000.0; }   // ros::Duration (:40)
inline double ToMsClock(const double& t) { return 1000 * ((double)t) / ((double)CLOCKS_PER_SEC); }

// ---- StructuredKStrongest (radar_filters.h:84-113, radar_filters.cpp:198-337): the constructor filters (FilterKstrongest +
//      AxialNonMaxSupress), getPeaksFilteredPointCloud APPENDS the kept bins (all of them, or the peaks) to the cloud ------
class StructuredKStrongest {
 public:
  StructuredKStrongest(Context& ctx, const uint8_t* image, int rows, int cols, int stride, const int z_min, const int k_strongest,
                       const double min_distance, const double range_res) {
    cfear_polar_desc d{rows, cols, stride, 1, 0};
    cfear_kstrong_params p{k_strongest, (float)z_min, (float)range_res, (float)min_distance, 1};
    all_.resize((size_t)rows * k_strongest);
    peaks_.resize((size_t)rows * k_strongest);
    int32_t n = 0, n_pk = 0;
    cfear_kstrong_out o{};
    o.xyzi = &all_[0].x; o.n_points = &n; o.xyzi_peaks = &peaks_[0].x; o.n_peaks = &n_pk;
    ctx.check(cfear_filter_kstrongest(ctx.get(), image, &d, &p, &o));
    all_.resize(n);
    peaks_.resize(n_pk);
  }
  void getPeaksFilteredPointCloud(PointCloud& output_pointcloud, bool peaks = false) const {
    const PointCloud& src = peaks ? peaks_ : all_;
    output_pointcloud.insert(output_pointcloud.end(), src.begin(), src.end());
  }
#ifdef CFEAR_HIP_HAVE_CV_BRIDGE
  // the reference's signature (radar_filters.h:88, :90): a MONO8 cv_bridge image, clouds as pcl pointers (created when null)
  StructuredKStrongest(const cv_bridge::CvImagePtr& radar_image, const int z_min, const int k_strongest, const double min_distance,
                       const double range_res)
      : StructuredKStrongest(Context::Default(), radar_image->image.data, radar_image->image.rows, radar_image->image.cols,
                             (int)radar_image->image.step, z_min, k_strongest, min_distance, range_res) {}
  void getPeaksFilteredPointCloud(pcl::PointCloud<pcl::PointXYZI>::Ptr& output_pointcloud, bool peaks = false) const {
    if (!output_pointcloud) output_pointcloud = pcl::PointCloud<pcl::PointXYZI>::Ptr(new pcl::PointCloud<pcl::PointXYZI>());
    for (const PointXYZI& q : (peaks ? peaks_ : all_)) {
      pcl::PointXYZI p; p.x = q.x; p.y = q.y; p.z = q.z; p.intensity = q.intensity;
      output_pointcloud->push_back(p);
    }
  }
#endif
 private:
  PointCloud all_, peaks_;
};

// AzimuthCACFAR as the batched odometry runs it (no counterpart in the reference): the kernel selection of a call, and the
// filter stage on its own with per-row keys in device memory (cfear_hip.h: cfear_cacfar_plan, cfear_filter_cacfar_rowkeys)
inline struct cfear_cacfar_plan cacfar_plan(const cfear_polar_desc& desc, const cfear_cacfar_params& par, int32_t flags = 0) {
  struct cfear_cacfar_plan out;
  const int st = ::cfear_cacfar_plan(&desc, &par, flags, &out);
  if (st != CFEAR_OK) throw CfearError(st, cfear_status_string(st));
  return out;
}
inline void filter_cacfar_rowkeys(Context& ctx, const uint8_t* d_image, const cfear_polar_desc& desc, const cfear_cacfar_params& par,
                                  int32_t flags, uint32_t* d_row_keys, int32_t* d_row_counts, int32_t kcap) {
  ctx.check(cfear_filter_cacfar_rowkeys(ctx.get(), d_image, &desc, &par, flags, d_row_keys, d_row_counts, kcap));
}
// the k-strongest row sweep's kernel selection (cfear_hip.h: cfear_kstrong_plan); a refused call is reported in .refused
inline struct cfear_kstrong_plan kstrong_plan(const cfear_polar_desc& desc, const cfear_kstrong_params& par, uint64_t base_address = 0) {
  struct cfear_kstrong_plan out;
  const int st = ::cfear_kstrong_plan(&desc, &par, base_address, &out);
  if (st != CFEAR_OK) throw CfearError(st, cfear_status_string(st));
  return out;
}

// k_strongest_filter (radar_filters.cpp:40-78, with InsertStrongestK :25-38): the legacy filter CorAl's kstrongRadar calls;
// APPENDS to cloud
inline void k_strongest_filter(Context& ctx, const uint8_t* image, int rows, int cols, int stride, PointCloud& cloud, int k_strongest,
                               double z_min, double range_res, double min_distance) {
  cfear_polar_desc d{rows, cols, stride, 1, 0};
  PointCloud out((size_t)rows * k_strongest);
  int32_t n = 0;
  ctx.check(cfear_filter_kstrongest_legacy(ctx.get(), image, &d, k_strongest, z_min, range_res, min_distance, out.empty() ? nullptr : &out[0].x,
                                           &n, rows * k_strongest));
  cloud.insert(cloud.end(), out.begin(), out.begin() + n);
}
#ifdef CFEAR_HIP_HAVE_CV_BRIDGE
inline void k_strongest_filter(cv_bridge::CvImagePtr& cv_polar_image, pcl::PointCloud<pcl::PointXYZI>::Ptr& cloud, int k_strongest,
                               double z_min, double range_res, double min_distance) {          // radar_filters.cpp:40
  if (!cloud) cloud = pcl::PointCloud<pcl::PointXYZI>::Ptr(new pcl::PointCloud<pcl::PointXYZI>());
  PointCloud c;
  k_strongest_filter(Context::Default(), cv_polar_image->image.data, cv_polar_image->image.rows, cv_polar_image->image.cols,
                     (int)cv_polar_image->image.step, c, k_strongest, z_min, range_res, min_distance);
  for (const PointXYZI& q : c) { pcl::PointXYZI p; p.x = q.x; p.y = q.y; p.z = q.z; p.intensity = q.intensity; cloud->push_back(p); }
}
#endif

// cell::TransformCopy (pointnormal.cpp:515-529) on the POD cell.  The covariance follows the reference's expression literally:
// C = R * T * cov_ * R.transpose() with T an Affine2d multiplies cov_'s COLUMNS as points -- (R R) cov + (R t) 1^T, then * R^T --
// not the similarity transform R cov R^T one would expect; nothing in the reference reads cov_ of a transformed map.
inline cfear_cell TransformCopy(const cfear_cell& c, const Pose2d& T) {
  const double cs = std::cos(T.theta), sn = std::sin(T.theta);
  const double R[4] = {cs, -sn, sn, cs};
  const double RR[4] = {R[0] * R[0] + R[1] * R[2], R[0] * R[1] + R[1] * R[3], R[2] * R[0] + R[3] * R[2], R[2] * R[1] + R[3] * R[3]};
  const double Rt[2] = {R[0] * T.x + R[1] * T.y, R[2] * T.x + R[3] * T.y};
  const double M[4] = {RR[0] * c.cov[0] + RR[1] * c.cov[2] + Rt[0], RR[0] * c.cov[1] + RR[1] * c.cov[3] + Rt[0],
                       RR[2] * c.cov[0] + RR[3] * c.cov[2] + Rt[1], RR[2] * c.cov[1] + RR[3] * c.cov[3] + Rt[1]};
  cfear_cell o = c;
  o.cov[0] = M[0] * R[0] + M[1] * R[1]; o.cov[1] = M[0] * R[2] + M[1] * R[3];     // M * R^T
  o.cov[2] = M[2] * R[0] + M[3] * R[1]; o.cov[3] = M[2] * R[2] + M[3] * R[3];
  o.mean[0] = R[0] * c.mean[0] + R[1] * c.mean[1] + T.x; o.mean[1] = R[2] * c.mean[0] + R[3] * c.mean[1] + T.y;
  o.normal[0] = R[0] * c.normal[0] + R[1] * c.normal[1]; o.normal[1] = R[2] * c.normal[0] + R[3] * c.normal[1];
  return o;
}

class MapPointNormal {
 public:
  static double& downsample_factor() { static double f = 1.0; return f; }                   // pointnormal.cpp:5
  MapPointNormal(Context& ctx, PointCloud& cld, float radius, double ox = 0, double oy = 0, bool weight_intensity = false)
      : ctx_(ctx) {
    cfear_feature_params fp{};
    fp.radius = radius; fp.downsample_factor = downsample_factor(); fp.origin[0] = ox; fp.origin[1] = oy;
    fp.weight_intensity = weight_intensity ? 1 : 0;
    ctx_.check(cfear_scan_create(ctx_.get(), cld.empty() ? nullptr : &cld[0].x, (int32_t)cld.size(), &fp, &scan_));
  }
  MapPointNormal(Context& ctx, const std::vector<cfear_cell>& cells) : ctx_(ctx) {           // Boost load() path
    ctx_.check(cfear_scan_from_cells(ctx_.get(), cells.data(), (int32_t)cells.size(), &scan_));
  }
#ifdef CFEAR_HIP_HAVE_EIGEN_PCL
  // pointnormal.h:116 / pointnormal.cpp:65-90.  raw: one identity cell per point (cell::GetIdentityCell, pointnormal.h:59)
  MapPointNormal(const pcl::PointCloud<pcl::PointXYZI>::Ptr& cld, float radius, const Eigen::Vector2d& origin = Eigen::Vector2d(0, 0),
                 const bool weight_intensity = false, const bool raw = false) : ctx_(Context::Default()) {
    input_ = cld;                                                                  // pointnormal.cpp:78 (GetScan hands it back)
    if (raw) {
      std::vector<cfear_cell> cells(cld->points.size());
      for (size_t i = 0; i < cells.size(); i++) {
        cfear_cell c{};
        c.mean[0] = cld->points[i].x; c.mean[1] = cld->points[i].y;
        c.normal[0] = 1; c.normal[1] = 0; c.cov[0] = 0.1; c.cov[3] = 0.1;          // cov_ default Identity * 0.1 (pointnormal.h:68)
        c.scale = 1.0; c.avg_intensity = 1.0; c.lambda_min = 1; c.lambda_max = 1; c.nsamples = 1;
        cells[i] = c;
      }
      ctx_.check(cfear_scan_from_cells(ctx_.get(), cells.data(), (int32_t)cells.size(), &scan_));
      return;
    }
    PointCloud pts = FromPcl(*cld);
    cfear_feature_params fp{};
    fp.radius = radius; fp.downsample_factor = downsample_factor(); fp.origin[0] = origin(0); fp.origin[1] = origin(1);
    fp.weight_intensity = weight_intensity ? 1 : 0;
    ctx_.check(cfear_scan_create(ctx_.get(), pts.empty() ? nullptr : &pts[0].x, (int32_t)pts.size(), &fp, &scan_));
  }
  Eigen::Vector2d GetMean2d(const size_t i) { const cfear_cell& c = cached()[i]; return Eigen::Vector2d(c.mean[0], c.mean[1]); }       // :127
  Eigen::Vector2d GetNormal2d(const size_t i) { const cfear_cell& c = cached()[i]; return Eigen::Vector2d(c.normal[0], c.normal[1]); } // :131
  Eigen::Matrix2d GetCov2d(const size_t i) {                                                                                          // :135
    const cfear_cell& c = cached()[i];
    Eigen::Matrix2d m;
    m(0, 0) = c.cov[0]; m(0, 1) = c.cov[1]; m(1, 0) = c.cov[2]; m(1, 1) = c.cov[3];
    return m;
  }
  std::vector<int> GetClosestIdx(const Eigen::Vector2d& p, double d) const { return GetClosestIdx(p(0), p(1), d); }                   // :238
  pcl::PointCloud<pcl::PointXYZI>::Ptr GetScan() { return input_; }                                                                 // :170
  // PublishMap (pointnormal.h:235) draws RViz markers through a static ros::Publisher map: visualisation, out of scope --
  // kept as a no-op so that callers (odometrykeyframefuser.cpp:209-216) compile unchanged
  template <class MapPtr, class Affine>
  static void PublishMap(const std::string&, MapPtr, const Affine&, const std::string&, const int = 0, float = 1.0f) {}
  boost::shared_ptr<MapPointNormal> TransformMap(const Eigen::Affine3d& T) {                                                          // :168
    return boost::shared_ptr<MapPointNormal>(new MapPointNormal(ctx_, TransformCells(Affine3dToPose2d(T))));
  }
#endif
  ~MapPointNormal() { if (!borrowed_) cfear_scan_destroy(scan_); }
  MapPointNormal(const MapPointNormal&) = delete;
  MapPointNormal& operator=(const MapPointNormal&) = delete;
  size_t GetSize() const { return (size_t)cfear_scan_size(scan_); }
  std::vector<cfear_cell> GetCells() const {
    std::vector<cfear_cell> c(GetSize());
    if (!c.empty()) { const int n = cfear_scan_get_cells(scan_, c.data(), (int32_t)c.size()); if (n < 0) ctx_.check(n); }
    return c;
  }
  const cfear_cell& GetCell(const size_t i) { return cached()[i]; }                          // pointnormal.h:120
  std::vector<cfear_cell> TransformCells(const Pose2d& T) {                                  // pointnormal.h:140
    std::vector<cfear_cell> out = GetCells();
    for (cfear_cell& c : out) c = TransformCopy(c, T);
    return out;
  }
  // TransformMap (pointnormal.cpp:135-137 -> the constructor at :91-111): the cells moved into the frame T, searchable
  std::unique_ptr<MapPointNormal> TransformMap(const Pose2d& T) { return std::unique_ptr<MapPointNormal>(new MapPointNormal(ctx_, TransformCells(T))); }
  std::vector<int> GetClosestIdx(double px, double py, double d) const {                     // pointnormal.cpp:238-254
    const double q[2] = {px, py};
    int32_t idx = -1;
    ctx_.check(cfear_scan_closest_idx(scan_, q, 1, d, &idx));
    return idx >= 0 ? std::vector<int>{idx} : std::vector<int>{};
  }
  // The tie-aware GetClosestIdx (cfear_scan_closest_ties): ALL cells at the minimum float distance of p, which the 1-NN search
  // returns one of -- lo is GetClosestIdx's answer, hi the highest cell at that distance, count how many; {-1, -1, 0} beyond d.
  struct ClosestTies { int lo, hi, count; };
  ClosestTies GetClosestTies(double px, double py, double d) const {
    const double q[2] = {px, py};
    int32_t lo = -1, hi = -1, count = 0;
    ctx_.check(cfear_scan_closest_ties(scan_, q, 1, d, &lo, &hi, &count));
    return ClosestTies{lo, hi, count};
  }
  // the route the surface-point kernels served this scan on (CFEAR_SURF_PATH_*; 0 for a scan made from cells): diagnostic
  uint32_t SurfacePath() const { uint32_t p = 0; ctx_.check(cfear_scan_surface_path(scan_, &p)); return p; }
  const cfear_scan* device() const { return scan_; }
 private:
  friend class ScanBatch;
  MapPointNormal(Context& ctx, const cfear_scan* borrowed) : ctx_(ctx), scan_(const_cast<cfear_scan*>(borrowed)), borrowed_(true) {}
  const std::vector<cfear_cell>& cached() { if (cache_.empty()) cache_ = GetCells(); return cache_; }
  std::vector<cfear_cell> cache_;
  Context& ctx_;
  cfear_scan* scan_ = nullptr;
  bool borrowed_ = false;                 // a view into a ScanBatch's arena: the batch owns the cells
#ifdef CFEAR_HIP_HAVE_EIGEN_PCL
  pcl::PointCloud<pcl::PointXYZI>::Ptr input_;
#endif
};
#ifdef CFEAR_HIP_HAVE_EIGEN_PCL
typedef boost::shared_ptr<MapPointNormal> MapNormalPtr;                                       // pointnormal.h:108
#endif

// N clouds -> N scans in one call and one arena (cfear_scan_create_batch): what a caller without a live fuser uses to turn
// stored clouds into scans -- loop closure on fresh sweeps, scan evaluation, training data.  at(i) is a MapPointNormal that
// borrows scan i (nullptr where the scan failed: status(i) says why) and is valid while the batch lives.  motions: empty, or
// one (x, y, theta) per cloud to compensate it by (in a copy; the clouds stay as they are).
class ScanBatch {
 public:
  ScanBatch(Context& ctx, const std::vector<PointCloud>& clouds, float radius, int32_t max_cells, double ox = 0, double oy = 0,
            bool weight_intensity = false, const std::vector<Pose2d>& motions = std::vector<Pose2d>(), bool ccw = false)
      : ctx_(ctx), status_(clouds.size(), 0) {
    std::vector<float> xyzi;
    std::vector<int64_t> offsets(clouds.size());
    std::vector<int32_t> lengths(clouds.size());
    for (size_t i = 0; i < clouds.size(); i++) {
      offsets[i] = (int64_t)(xyzi.size() / 4);
      lengths[i] = (int32_t)clouds[i].size();
      if (!clouds[i].empty()) xyzi.insert(xyzi.end(), &clouds[i][0].x, &clouds[i][0].x + 4 * clouds[i].size());
    }
    cfear_feature_params fp{};
    fp.radius = radius; fp.downsample_factor = MapPointNormal::downsample_factor(); fp.origin[0] = ox; fp.origin[1] = oy;
    fp.weight_intensity = weight_intensity ? 1 : 0;
    fp.compensate = motions.empty() ? 0 : 1;
    fp.ccw = ccw ? 1 : 0;
    if (!motions.empty() && motions.size() != clouds.size()) throw std::invalid_argument("ScanBatch: one motion per cloud");
    const int rc = cfear_scan_create_batch(ctx_.get(), xyzi.empty() ? nullptr : xyzi.data(), offsets.data(), lengths.data(),
                                           (int32_t)clouds.size(), &fp, motions.empty() ? nullptr : &motions[0].x, max_cells, &h_,
                                           status_.data());
    if (!h_) ctx_.check(rc);                              // a cloud that failed is a status, not an exception
    scans_.resize(clouds.size());
    for (size_t i = 0; i < clouds.size(); i++) {
      const cfear_scan* s = nullptr;
      ctx_.check(cfear_scan_batch_get(h_, (int32_t)i, &s));
      if (s) scans_[i].reset(new MapPointNormal(ctx_, s));
    }
  }
  ~ScanBatch() { scans_.clear(); if (h_) cfear_scan_batch_destroy(h_); }
  ScanBatch(const ScanBatch&) = delete;
  ScanBatch& operator=(const ScanBatch&) = delete;
  size_t size() const { return scans_.size(); }
  MapPointNormal* at(size_t i) const { return scans_[i].get(); }
  int32_t status(size_t i) const { return status_[i]; }
  const cfear_scan_batch* get() const { return h_; }

 private:
  Context& ctx_;
  cfear_scan_batch* h_ = nullptr;
  std::vector<int32_t> status_;
  std::vector<std::unique_ptr<MapPointNormal>> scans_;
};

// The device views of a set of scans, uploaded once (cfear_scan_table): what the loop-closure thread keeps for the graph's
// nodes so that a candidate is two indices and two poses.  The library's table holds a reference of its own on
// every scan (a scan destroyed first keeps its cells until the table goes); this wrapper does not keep the MapPointNormals alive.
class ScanTable {
 public:
  ScanTable(Context& ctx, const std::vector<const MapPointNormal*>& scans) : ctx_(ctx), h_(nullptr) {
    std::vector<const cfear_scan*> h(scans.size());
    for (size_t i = 0; i < scans.size(); i++) h[i] = scans[i]->device();
    ctx_.check(cfear_scan_table_create(ctx_.get(), h.data(), (int32_t)h.size(), &h_));
  }
  ~ScanTable() { if (h_) cfear_scan_table_destroy(h_); }
  ScanTable(const ScanTable&) = delete;
  ScanTable& operator=(const ScanTable&) = delete;
  int size() const { return cfear_scan_table_size(h_); }
  const cfear_scan_table* get() const { return h_; }

 private:
  Context& ctx_;
  cfear_scan_table* h_;
};

class n_scan_normal_reg {
 public:
  explicit n_scan_normal_reg(Context& ctx, int cost = CFEAR_P2L, int loss = CFEAR_LOSS_HUBER, double loss_limit = 0.1,
                             int opt = CFEAR_W_UNIFORM) : ctx_(ctx) {                         // n_scan_normal.h:35
    cfear_reg_params_default(&par_);
    par_.cost = cost; par_.loss = loss; par_.loss_limit = loss_limit; par_.weight_opt = opt;
  }
  void SetParameters(unsigned max_itr_association, unsigned max_itr_solver) {                 // n_scan_normal.cpp:15-19
    par_.max_itr_association = (int32_t)max_itr_association; par_.max_itr_solver = (int32_t)max_itr_solver;
  }
  void SetD2dPar(double cov_scale, double regularization) { par_.cov_scale = cov_scale; par_.regularization = regularization; }
  // Register (n_scan_normal.cpp:82-185): Tsrc in/out; returns false exactly where the reference does.
  bool Register(const std::vector<const MapPointNormal*>& scans, std::vector<Pose2d>& Tsrc) {
    std::vector<const cfear_scan*> h(scans.size());
    for (size_t i = 0; i < scans.size(); i++) h[i] = scans[i]->device();
    const int st = cfear_register(ctx_.get(), h.data(), (int32_t)h.size(), &Tsrc[0].x, &par_, &summary_);
    if (st != CFEAR_OK && st != CFEAR_ERR_TOO_FEW_RESIDUALS && st != CFEAR_ERR_SOLVER) ctx_.check(st);
    par_.itr = summary_.outer_iters;                       // itr_ stays behind for GetCost (n_scan_normal.cpp:220)
    score_ = summary_.score;
    return st == CFEAR_OK;
  }
  bool GetCost(const std::vector<const MapPointNormal*>& scans, const std::vector<Pose2d>& Tsrc, double& score,
               std::vector<double>& residuals) {                                              // n_scan_normal.cpp:186-211
    std::vector<const cfear_scan*> h(scans.size());
    size_t total = 2;
    for (size_t i = 0; i < scans.size(); i++) { h[i] = scans[i]->device(); total += 2 * scans[i]->GetSize(); }
    residuals.resize(total);
    int32_t n = 0;
    double s = 0;
    const int st = cfear_get_cost(ctx_.get(), h.data(), (int32_t)h.size(), &Tsrc[0].x, &par_, &score, residuals.data(),
                                  (int32_t)total, &n, &s);
    if (st != CFEAR_OK && st != CFEAR_ERR_TOO_FEW_RESIDUALS) ctx_.check(st);
    residuals.resize(n);
    score_ = s;
    return st == CFEAR_OK;
  }
#ifdef CFEAR_HIP_HAVE_EIGEN_PCL
  n_scan_normal_reg() : n_scan_normal_reg(Context::Default()) {}                              // n_scan_normal.h:33
  n_scan_normal_reg(const cost_metric& cost, loss_type loss = Huber, double loss_limit = 0.1,
                    const weightoption opt = weightoption::Uniform)                           // n_scan_normal.h:35
      : n_scan_normal_reg(Context::Default(), (int)cost, (int)loss, loss_limit, (int)opt) {}
  // n_scan_normal.h:37 / n_scan_normal.cpp:82-185: on success EVERY Tsrc[i] is rewritten from its (x, y, theta) parameters
  // (:176-177) and every reg_cov[i] is the constant diag(0.01, 0.01, 0, 0, 0, 1e-4) (:171-175).
  // soft_constraints = true is REFUSED (CfearError, CFEAR_ERR_INVALID_ARGUMENT), not ignored: the reference's prior
  // (n_scan_normal.cpp:371-375) is mahalanobisDistanceError created as AutoDiffCostFunction<..., 1, 3> (n_scan_normal.h:279-282)
  // whose functor writes THREE residuals through an Eigen::Map (:271-275) -- two of them past the one-element output Ceres
  // hands it.  Its result is undefined in the reference, so there is nothing to be identical to; the shipped callers pass
  // false (offline_odometry.cpp:274, loopclosure.cpp:60).
  bool Register(std::vector<MapNormalPtr>& scans, std::vector<Eigen::Affine3d>& Tsrc, std::vector<Matrix6d>& reg_cov,
                bool soft_constraints = false) {
    if (soft_constraints)
      throw CfearError(CFEAR_ERR_INVALID_ARGUMENT, "Register(..., soft_constraints = true): the reference's prior is undefined "
                                                   "behaviour (3 residuals written into a 1-residual block) and is not provided");
    std::vector<const MapPointNormal*> h(scans.size());
    std::vector<Pose2d> poses(scans.size());
    for (size_t i = 0; i < scans.size(); i++) { h[i] = scans[i].get(); poses[i] = Affine3dToPose2d(Tsrc[i]); }
    const bool ok = Register(h, poses);
    if (ok) {
      Matrix6d m = Matrix6d::Zero();
      m(0, 0) = 0.1 * 0.1; m(1, 1) = 0.1 * 0.1; m(5, 5) = 0.01 * 0.01;
      for (size_t i = 0; i < scans.size(); i++) {
        if (i < reg_cov.size()) reg_cov[i] = m;
        Tsrc[i] = Pose2dToAffine3d(poses[i]);
      }
    }
    return ok;
  }
  bool GetCost(std::vector<MapNormalPtr>& scans, std::vector<Eigen::Affine3d>& Tsrc, double& score,
               std::vector<double>& residuals) {                                              // n_scan_normal.h:41
    std::vector<const MapPointNormal*> h(scans.size());
    std::vector<Pose2d> poses(scans.size());
    for (size_t i = 0; i < scans.size(); i++) { h[i] = scans[i].get(); poses[i] = Affine3dToPose2d(Tsrc[i]); }
    return GetCost(h, poses, score, residuals);
  }
#endif
  // loopclosure::Register for a whole list of candidate pairs among the scans of a table (loopclosure.cpp:35-97 per candidate):
  // one launch; results[i].status says what Register's bool would have.
  void RegisterCandidates(const ScanTable& table, const std::vector<cfear_candidate>& candidates, std::vector<cfear_reg_result>& results) {
    results.resize(candidates.size());
    ctx_.check(cfear_register_candidates(ctx_.get(), table.get(), candidates.data(), (int32_t)candidates.size(), &par_, results.data()));
  }
  // loopclosure::approximateCovarianceBySampling for the same list, around the poses RegisterCandidates left in `results`
  // (cfear_covariance_by_sampling_candidates: samples and fit on the device): cov36 [n][36] row-major, success [n].
  void CovarianceBySamplingCandidates(const ScanTable& table, const std::vector<cfear_candidate>& candidates,
                                      const std::vector<cfear_reg_result>& results, std::vector<double>& cov36, std::vector<int32_t>& success,
                                      const cfear_cov_sampling_params* sp = nullptr) {
    if (results.size() != candidates.size()) throw CfearError(CFEAR_ERR_INVALID_ARGUMENT, "CovarianceBySamplingCandidates: one registration record per candidate");
    cfear_cov_sampling_params def;
    cfear_cov_sampling_params_default(&def);
    cov36.assign(candidates.size() * 36, 0.0); success.assign(candidates.size(), 0);
    if (candidates.empty()) return;
    ctx_.check(cfear_covariance_by_sampling_candidates(ctx_.get(), table.get(), candidates.data(), (int32_t)candidates.size(), &par_, results.data(),
                                                       sp ? sp : &def, cov36.data(), success.data()));
  }
  const cfear_reg_params& params() const { return par_; }
  double getScore() const { return score_; }
  bool GetCovarianceScaler(double& cov_scale) const {                                         // n_scan_normal.cpp:433-439
    if (summary_.num_residuals - 3 == 0) return false;
    cov_scale = summary_.final_cost / (double)(summary_.num_residuals - 3);
    return true;
  }
  // OdometryKeyframeFuser::approximateCovarianceBySampling (odometrykeyframefuser.cpp:261-380) /
  // loopclosure::approximateCovarianceBySampling (loopclosure.cpp:99-208): T_vek = poses after Register of
  // THIS object; cov_sampled row-major 6x6.  Returns cov_sampled_success.
  bool approximateCovarianceBySampling(const std::vector<const MapPointNormal*>& scans, const std::vector<Pose2d>& T_vek,
                                       double cov_sampled[36], const cfear_cov_sampling_params* sp = nullptr) {
    cfear_cov_sampling_params def;
    cfear_cov_sampling_params_default(&def);
    std::vector<const cfear_scan*> h(scans.size());
    for (size_t i = 0; i < scans.size(); i++) h[i] = scans[i]->device();
    int32_t ok = 0;
    ctx_.check(cfear_covariance_by_sampling(ctx_.get(), h.data(), (int32_t)h.size(), &T_vek[0].x, &par_, &summary_,
                                            sp ? sp : &def, cov_sampled, nullptr, &ok));
    return ok != 0;
  }
  cfear_reg_result summary_{};
 private:
  Context& ctx_;
  cfear_reg_params par_;
  double score_ = 0;
};

// The covariance fit of cost sampling alone, as a kernel (cfear_cov_fit_records): regs [n], samples [n][samples_per_axis^3]
// as the matcher's sampling mode leaves them -> cov36 [n][36] row-major, success [n].
inline void CovFitRecords(Context& ctx, const std::vector<cfear_reg_result>& regs, const std::vector<cfear_reg_result>& samples,
                          const cfear_cov_sampling_params& sp, std::vector<double>& cov36, std::vector<int32_t>& success) {
  const size_t m = (size_t)sp.samples_per_axis * sp.samples_per_axis * sp.samples_per_axis;
  if (samples.size() != regs.size() * m) throw CfearError(CFEAR_ERR_INVALID_ARGUMENT, "CovFitRecords: samples_per_axis^3 sample records per job");
  cov36.assign(regs.size() * 36, 0.0); success.assign(regs.size(), 0);
  if (regs.empty()) return;
  ctx.check(cfear_cov_fit_records(ctx.get(), regs.data(), samples.data(), (int32_t)regs.size(), &sp, cov36.data(), success.data()));
}

// Which registrations hang on a nearest-neighbour tie (cfear_association_ties_batch): the association
// step of every job -- scans[j] with the free source last, poses[j] one per scan -- replayed at the poses given, one launch
// for the batch.  per_query (optional) receives {lo, hi, count} per query, offsets (optional) the first entry of every job
// and, as its last element, the total.
inline std::vector<cfear_tie_record> AssociationTies(Context& ctx, const std::vector<std::vector<const MapPointNormal*>>& scans,
                                                     const std::vector<std::vector<Pose2d>>& poses, const cfear_reg_params& par,
                                                     int itr = 1, std::vector<int32_t>* per_query = nullptr,
                                                     std::vector<int64_t>* offsets = nullptr) {
  const size_t n = scans.size();
  if (poses.size() != n) throw CfearError(CFEAR_ERR_INVALID_ARGUMENT, "AssociationTies: one pose list per job");
  std::vector<std::vector<const cfear_scan*>> h(n);
  std::vector<cfear_reg_job> jobs(n);
  std::vector<int64_t> off(n + 1, 0);
  for (size_t j = 0; j < n; j++) {
    if (scans[j].size() < 2 || poses[j].size() != scans[j].size())
      throw CfearError(CFEAR_ERR_INVALID_ARGUMENT, "AssociationTies: a job needs two scans or more and one pose per scan");
    for (const MapPointNormal* m : scans[j]) h[j].push_back(m->device());
    jobs[j].scans = h[j].data(); jobs[j].n_scans = (int32_t)h[j].size(); jobs[j].pad = 0; jobs[j].poses_xyt = &poses[j][0].x;
    off[j + 1] = off[j] + (int64_t)scans[j].back()->GetSize() * (int64_t)(scans[j].size() - 1);
  }
  std::vector<cfear_tie_record> records(n);
  if (per_query) per_query->assign((size_t)off[n] * 3, 0);
  ctx.check(cfear_association_ties_batch(ctx.get(), jobs.data(), (int32_t)n, &par, itr, records.data(),
                                         per_query && off[n] > 0 ? per_query->data() : nullptr, off[n]));
  if (offsets) *offsets = off;
  return records;
}

// Which scans hang on the in-voxel summation order of pcl::VoxelGrid (cfear_voxel_order_audit_batch):
// clouds[s] = the xyzi floats of scan s (four per point), the cloud MapPointNormal hands to VoxelGrid.  One call for the
// batch.  voxels (optional) receives every scan's rows in ascending voxel key, offsets (optional) the first row of every
// scan and, as its last element, the total.  A scan that is empty, not finite or too large carries its status in its
// record; only a refusal of the call throws.
inline std::vector<cfear_voxel_audit_record> VoxelOrderAudit(Context& ctx, const std::vector<std::vector<float>>& clouds, float radius = 3.0f,
                                                             double downsample_factor = 1.0,
                                                             std::vector<cfear_voxel_audit_voxel>* voxels = nullptr,
                                                             std::vector<int64_t>* offsets = nullptr) {
  const size_t n = clouds.size();
  std::vector<int32_t> lengths(n);
  std::vector<float> xyzi;
  for (size_t s = 0; s < n; s++) {
    if (clouds[s].size() % 4) throw CfearError(CFEAR_ERR_INVALID_ARGUMENT, "VoxelOrderAudit: a cloud holds four floats per point");
    lengths[s] = (int32_t)(clouds[s].size() / 4);
    xyzi.insert(xyzi.end(), clouds[s].begin(), clouds[s].end());
  }
  const int64_t cap = (int64_t)(xyzi.size() / 4);            // no scan has more voxels than points
  xyzi.resize(xyzi.size() + 4, 0.f);
  cfear_voxel_audit_params par;
  cfear_voxel_audit_params_default(&par);
  par.radius = radius;
  par.downsample_factor = downsample_factor;
  std::vector<cfear_voxel_audit_record> records(n);
  if (voxels) voxels->assign((size_t)cap, cfear_voxel_audit_voxel{});
  int64_t rows = 0;
  const int rc = cfear_voxel_order_audit_batch(ctx.get(), xyzi.data(), nullptr, lengths.data(), (int32_t)n, &par, records.data(),
                                               voxels && cap > 0 ? voxels->data() : nullptr, cap, &rows);
  bool carried = false;
  for (const cfear_voxel_audit_record& r : records) carried = carried || r.status == rc;
  if (rc != CFEAR_OK && !carried) ctx.check(rc);
  if (voxels) voxels->resize((size_t)rows);
  if (offsets) {
    offsets->assign(n + 1, 0);
    for (size_t s = 0; s < n; s++) (*offsets)[s + 1] = (*offsets)[s] + records[s].n_voxels;
  }
  return records;
}

// A recorded trajectory replayed frame by frame (cfear_odometry_replay_clouds): clouds[f] = the
// filtered cloud of frame f BEFORE compensation, trace[f] its recorded pose, seq_offsets the first frame of every sequence and,
// as its last element, the number of frames (empty: one sequence).  One record per frame; a frame whose cloud is empty
// carries the status in reg_status, as do the frames whose window holds it; only a refusal of the call throws.  audit folds the
// tie and voxel-order audits into the records (CFEAR_REPLAY_AUDIT, with the caveats of cfear_hip.h).  Raw sweeps go through
// cfear_odometry_replay directly.
inline std::vector<cfear_replay_frame> OdometryReplay(Context& ctx, const std::vector<PointCloud>& clouds, const std::vector<Pose2d>& trace,
                                                      const cfear_odometry_params& par,
                                                      const std::vector<int32_t>& seq_offsets = std::vector<int32_t>(), bool audit = false) {
  if (clouds.size() != trace.size() || clouds.empty()) throw CfearError(CFEAR_ERR_INVALID_ARGUMENT, "OdometryReplay: one cloud per trace pose");
  std::vector<cfear_sc_cloud> c(clouds.size());
  for (size_t f = 0; f < clouds.size(); f++) {
    c[f].xyzi = clouds[f].empty() ? nullptr : &clouds[f][0].x;
    c[f].n = (int32_t)clouds[f].size();
    c[f].pad = 0;
  }
  std::vector<int32_t> seq = seq_offsets;
  if (seq.empty()) seq = {0, (int32_t)clouds.size()};
  std::vector<cfear_replay_frame> out(clouds.size());
  const int rc = cfear_odometry_replay_clouds(ctx.get(), c.data(), &par, &trace[0].x, seq.data(), (int32_t)seq.size() - 1, audit ? CFEAR_REPLAY_AUDIT : 0, out.data());
  if (rc != CFEAR_OK && rc != CFEAR_ERR_EMPTY_CLOUD && rc != CFEAR_ERR_CAPACITY) ctx.check(rc);
  return out;
}

// radarDriver + OdometryKeyframeFuser for n independent sequences, one frame per call (cfear_odometry_*): the whole
// path polar image -> pose on the GPU; with par.keep_nodes the RadarScan of every frame can be collected.
// Sharded candidate steps kept in flight (cfear_candidate_pipe): what the loop-closure thread of a rank
// calls per candidate batch when the node's GPUs share the work (loopclosure.cpp:658-721: independent candidates).  comm: the
// host's ncclComm_t in a cfear_rccl_comm (or one made by cfear_rccl_comm_init), nullptr for a single rank without a collective.
class CandidatePipe {
 public:
  CandidatePipe(Context& ctx, const ScanTable& table, int max_candidates, int rank = 0, int world = 1, const cfear_rccl_comm* comm = nullptr,
                int depth = 2, int flags = 0) : ctx_(ctx), h_(nullptr) {
    ctx_.check(cfear_candidate_pipe_create(ctx_.get(), table.get(), max_candidates, rank, world, comm, depth, flags, &h_));
  }
  ~CandidatePipe() { if (h_) cfear_candidate_pipe_destroy(h_); }
  CandidatePipe(const CandidatePipe&) = delete;
  CandidatePipe& operator=(const CandidatePipe&) = delete;
  // every rank hands in the FULL list; returns without waiting
  int64_t submit(const std::vector<cfear_candidate>& all_candidates, const n_scan_normal_reg& reg) {
    int64_t ticket = -1;
    sizes_[ticket_slot(next_)] = all_candidates.size();
    ctx_.check(cfear_candidate_pipe_submit(h_, all_candidates.data(), (int32_t)all_candidates.size(), &reg.params(), &ticket));
    next_ = ticket + 1;
    return ticket;
  }
  // all records of that batch, every rank's block, candidate order
  void collect(int64_t ticket, std::vector<cfear_reg_result>& results) {
    results.resize(sizes_[ticket_slot(ticket)]);
    cfear_reg_result dummy;
    ctx_.check(cfear_candidate_pipe_collect(h_, ticket, results.empty() ? &dummy : results.data()));
  }

 private:
  static size_t ticket_slot(int64_t t) { return (size_t)(t % 16); }          // (depth <= 16)
  Context& ctx_;
  cfear_candidate_pipe* h_;
  int64_t next_ = 0;
  size_t sizes_[16] = {};
};

class OdometryKeyframeFuser {
 public:
  OdometryKeyframeFuser(Context& ctx, int n_streams, int rows, int cols, const cfear_odometry_params* par = nullptr)
      : ctx_(ctx), n_(n_streams) {
    cfear_odometry_params def;
    if (!par) { cfear_odometry_params_default(&def); par = &def; }
    cfear_polar_desc d{rows, cols, cols, n_streams, (int64_t)rows * cols};
    ctx_.check(cfear_odometry_create(ctx_.get(), n_streams, &d, par, &od_));
  }
  ~OdometryKeyframeFuser() { cfear_odometry_destroy(od_); }
  OdometryKeyframeFuser(const OdometryKeyframeFuser&) = delete;
  OdometryKeyframeFuser& operator=(const OdometryKeyframeFuser&) = delete;
  // polar: [n_streams][rows][cols] uint8 (host or device); polar_next (optional): next frame, filtered ahead
  std::vector<cfear_frame_info> processFrame(const uint8_t* polar, const uint8_t* polar_next = nullptr) {
    std::vector<cfear_frame_info> info((size_t)n_);
    ctx_.check(cfear_odometry_process_prefetch(od_, polar, polar_next, info.data()));
    return info;
  }
  // pointcloudCallback(cloud, cloud_peaks, ...) (odometrykeyframefuser.cpp:413-426) for every stream: filtered clouds in
  std::vector<cfear_frame_info> pointcloudCallback(const std::vector<const PointCloud*>& clouds,
                                                   const std::vector<const PointCloud*>& peaks = {}) {
    std::vector<cfear_sc_cloud> c((size_t)n_), p((size_t)n_);
    for (int i = 0; i < n_; i++) {
      c[i] = cfear_sc_cloud{clouds[i]->empty() ? nullptr : &(*clouds[i])[0].x, (int32_t)clouds[i]->size(), 0};
      if (!peaks.empty()) p[i] = cfear_sc_cloud{peaks[i]->empty() ? nullptr : &(*peaks[i])[0].x, (int32_t)peaks[i]->size(), 0};
    }
    std::vector<cfear_frame_info> info((size_t)n_);
    ctx_.check(cfear_odometry_process_clouds(od_, c.data(), peaks.empty() ? nullptr : p.data(), info.data()));
    return info;
  }
#ifdef CFEAR_HIP_HAVE_EIGEN_PCL
  // The reference's single-sequence object (odometrykeyframefuser.h:72-249): its Parameters by their names, its
  // constructor, and pointcloudCallback with the reference's argument list (Time: ros::Time or anything else; unused).
  struct Parameters {
    std::string cost_type = "P2L", loss_type_ = "Huber";
    weightoption weight_opt = weightoption::Uniform;
    int submap_scan_size = 3;
    bool weight_intensity_ = false, use_guess = true, compensate = true, radar_ccw = false, use_keyframe = true;
    double res = 3.5, min_keyframe_dist_ = 1.5, min_keyframe_rot_deg_ = 5, loss_limit_ = 0.1, covar_scale_ = 1.0, regularization_ = 0.0;
    bool estimate_cov_by_sampling = false;
    double cov_sampling_xy_range = 0.4, cov_sampling_yaw_range = 0.0043625, cov_sampling_covariance_scaler = 4.0;
    unsigned int cov_sampling_samples_per_axis = 3;
    int max_points = 400 * 40;                                  // capacity of a filtered cloud (rows * k of the driver)
  };
  explicit OdometryKeyframeFuser(const Parameters& pars, bool disable_callback = false) : ctx_(Context::Default()), n_(1) {
    (void)disable_callback;
    cfear_odometry_params p;
    cfear_odometry_params_default(&p);
    p.reg.cost = pars.cost_type == "P2P" ? CFEAR_P2P : pars.cost_type == "P2D" ? CFEAR_P2D : CFEAR_P2L;        // Str2Cost
    p.reg.loss = pars.loss_type_ == "Cauchy" ? CFEAR_LOSS_CAUCHY : pars.loss_type_ == "SoftLOne" ? CFEAR_LOSS_SOFTLONE
               : pars.loss_type_ == "Combined" ? CFEAR_LOSS_COMBINED : pars.loss_type_ == "Tukey" ? CFEAR_LOSS_TUKEY
               : pars.loss_type_ == "None" ? CFEAR_LOSS_NONE : CFEAR_LOSS_HUBER;                              // Str2loss
    p.reg.loss_limit = pars.loss_limit_; p.reg.weight_opt = (int)pars.weight_opt;
    p.reg.cov_scale = pars.covar_scale_; p.reg.regularization = pars.regularization_;
    p.res = (float)pars.res; p.submap_scan_size = pars.submap_scan_size; p.weight_intensity = pars.weight_intensity_;
    p.use_guess = pars.use_guess; p.compensate = pars.compensate; p.radar_ccw = pars.radar_ccw; p.use_keyframe = pars.use_keyframe;
    p.min_keyframe_dist = pars.min_keyframe_dist_; p.min_keyframe_rot_deg = pars.min_keyframe_rot_deg_;
    p.estimate_cov_by_sampling = pars.estimate_cov_by_sampling;
    p.cov_sampling.xy_range = pars.cov_sampling_xy_range; p.cov_sampling.yaw_range = pars.cov_sampling_yaw_range;
    p.cov_sampling.samples_per_axis = (int32_t)pars.cov_sampling_samples_per_axis;
    p.cov_sampling.covariance_scaler = pars.cov_sampling_covariance_scaler;
    p.keep_nodes = 1;
    p.kstrong.k_strongest = 1;                                 // the cloud entry sizes its buffers by rows * k
    cfear_polar_desc d{pars.max_points, 1, 1, 1, (int64_t)pars.max_points};
    ctx_.check(cfear_odometry_create(ctx_.get(), 1, &d, &p, &od_));
  }
  bool updated = false;                                        // odometrykeyframefuser.h:198
  template <class Time>
  void pointcloudCallback(pcl::PointCloud<pcl::PointXYZI>::Ptr& cloud_filtered, pcl::PointCloud<pcl::PointXYZI>::Ptr& cloud_filtered_peaks,
                          Eigen::Affine3d& Tcurr, const Time& t) {                                            // :223
    Covariance cov;
    pointcloudCallback(cloud_filtered, cloud_filtered_peaks, Tcurr, t, cov);
  }
  template <class Time>
  void pointcloudCallback(pcl::PointCloud<pcl::PointXYZI>::Ptr& cloud_filtered, pcl::PointCloud<pcl::PointXYZI>::Ptr& cloud_filtered_peaks,
                          Eigen::Affine3d& Tcurr, const Time& /*t*/, Covariance& cov_curr) {                  // :225
    const PointCloud c = FromPcl(*cloud_filtered), pk = FromPcl(*cloud_filtered_peaks);
    const std::vector<cfear_frame_info> info = pointcloudCallback(std::vector<const PointCloud*>{&c}, std::vector<const PointCloud*>{&pk});
    Tcurr = Pose2dToAffine3d(Pose2d{info[0].pose[0], info[0].pose[1], info[0].pose[2]});
    updated = info[0].keyframe_added != 0;
    double cov[36];
    ctx_.check(cfear_odometry_get_covariance(od_, cov, nullptr));
    for (int r = 0; r < 6; r++) for (int q = 0; q < 6; q++) cov_curr(r, q) = cov[r * 6 + q];
  }
#endif
  // graph_ of a stream (odometrykeyframefuser.h:197-249: AddToGraph :428-445, SaveGraph, GetLastNode): call AddToGraph
  // after a frame whose info.keyframe_added is set (the odometry must have been created with par.keep_nodes); the node
  // keeps the pose, the compensated clouds, the surface points and the odometry constraint to the keyframe before it.
  struct GraphNode {
    Pose2d T;
    unsigned idx = 0;
    uint64_t stamp = 0;
    PointCloud cloud_peaks, cloud_nopeaks;
    std::vector<cfear_cell> cells;
    bool has_constraint = false;
    cfear_graph_constraint constraint{};
    bool has_Tgt = false;
    Pose2d Tgt{0, 0, 0};
  };
  void AddToGraph(int stream, const cfear_frame_info& info, uint64_t stamp = 0) {
    if ((int)graph_.size() < n_) graph_.resize((size_t)n_);
    GraphNode nd;
    nd.T = Pose2d{info.pose[0], info.pose[1], info.pose[2]};
    nd.idx = (unsigned)graph_[stream].size();
    nd.stamp = stamp;
    nd.cloud_nopeaks = GetCloud(stream, false);
    nd.cloud_peaks = GetCloud(stream, true);
    cfear_scan* s = GetScan(stream);
    nd.cells.resize((size_t)std::max(cfear_scan_size(s), 0));
    const int got = nd.cells.empty() ? 0 : cfear_scan_get_cells(s, nd.cells.data(), (int32_t)nd.cells.size());   // returns the count
    cfear_scan_destroy(s);
    if (got < 0) ctx_.check(got);
    nd.has_constraint = cfear_odometry_get_constraint(od_, stream, &nd.constraint) == CFEAR_OK;   // none for the first keyframe
    if ((int)status_.size() < n_) status_.resize((size_t)n_);
    if (!graph_[stream].empty()) {                             // a fused keyframe behind the first one
      const GraphNode& last = graph_[stream].back();
      status_[(size_t)stream].distance_traveled += std::hypot(nd.T.x - last.T.x, nd.T.y - last.T.y);
      status_[(size_t)stream].frame_nr++;
    }
    graph_[stream].push_back(std::move(nd));
  }
  // AddGroundTruth (odometrykeyframefuser.cpp:446-463): a node whose stamp appears in gt_vek receives Tgt / has_Tgt_
  void AddGroundTruth(const std::vector<std::pair<uint64_t, Pose2d>>& gt_vek, int stream = 0) {
    std::map<uint64_t, Pose2d> stamp_map;
    for (const auto& gt : gt_vek) stamp_map[gt.first] = gt.second;
    if ((size_t)stream >= graph_.size()) return;
    for (GraphNode& nd : graph_[(size_t)stream]) {
      const auto it = stamp_map.find(nd.stamp);
      if (it != stamp_map.end()) { nd.Tgt = it->second; nd.has_Tgt = true; }
    }
  }
  // EvalTrajectory::GetGtVek() as it is (offline_odometry.cpp:137): planar poses from the KITTI rows
  void AddGroundTruth(const poseStampedVector& gt_vek, int stream = 0) {
    std::vector<std::pair<uint64_t, Pose2d>> v;
    for (const poseStamped& gt : gt_vek) v.emplace_back((uint64_t)gt.t, Pose2d{gt.pose[3], gt.pose[7], std::atan2(gt.pose[4], gt.pose[0])});
    AddGroundTruth(v, stream);
  }
#ifdef CFEAR_HIP_HAVE_EIGEN_PCL
  // the reference's argument (odometrykeyframefuser.h:240): poseStampedVector = elements with .pose (Eigen::Affine3d) and .t (ros::Time)
  template <class PoseStampedVector>
  auto AddGroundTruth(PoseStampedVector& gt_vek) -> decltype(gt_vek.begin()->t.toNSec(), void()) {
    std::vector<std::pair<uint64_t, Pose2d>> v;
    for (auto&& gt : gt_vek) v.emplace_back((uint64_t)gt.t.toNSec(), Affine3dToPose2d(gt.pose));
    AddGroundTruth(v, 0);
  }
#endif
  // GetStatus (odometrykeyframefuser.h:234): distance_traveled grows by |Tkeydiff.translation()| and frame_nr_ by one with
  // every fused keyframe after the first (odometrykeyframefuser.cpp:236, 243)
  std::string GetStatus(int stream = 0) const {
    const bool have = (size_t)stream < status_.size();
    return "Distance traveled: " + std::to_string(have ? status_[(size_t)stream].distance_traveled : 0.0) +
           ", nr sensor readings: " + std::to_string(have ? status_[(size_t)stream].frame_nr : 0u);
  }
  const GraphNode& GetLastNode(int stream = 0) const { return graph_.at((size_t)stream).back(); }
  size_t GraphSize(int stream = 0) const { return (size_t)stream < graph_.size() ? graph_[stream].size() : 0; }
  void SaveGraph(const std::string& path, int stream = 0, float radius = 3.0f, bool weight_intensity = true) const {  // SaveSimpleGraph, types.cpp:103-113
    const std::vector<GraphNode>& g = graph_.at((size_t)stream);
    std::vector<cfear_graph_node> nodes(g.size());
    for (size_t i = 0; i < g.size(); i++) {
      cfear_graph_node& n = nodes[i];
      n = cfear_graph_node{};
      const double xyt[3] = {g[i].T.x, g[i].T.y, g[i].T.theta};
      cfear_pose3d_from_xyt(xyt, &n.T);
      n.idx = g[i].idx; n.stamp = g[i].stamp;
      if (g[i].has_Tgt) { const double gxyt[3] = {g[i].Tgt.x, g[i].Tgt.y, g[i].Tgt.theta}; cfear_pose3d_from_xyt(gxyt, &n.Tgt); n.has_Tgt = 1; }
      for (int k = 0; k < 16; k++) n.motion[k] = (k % 5 == 0) ? 1.0 : 0.0;            // motion_ = Identity
      n.cloud_peaks = cfear_graph_cloud{g[i].cloud_peaks.empty() ? nullptr : &g[i].cloud_peaks[0].x, (int32_t)g[i].cloud_peaks.size(), 0, g[i].stamp, nullptr};
      n.cloud_nopeaks = cfear_graph_cloud{g[i].cloud_nopeaks.empty() ? nullptr : &g[i].cloud_nopeaks[0].x, (int32_t)g[i].cloud_nopeaks.size(), 0, g[i].stamp, nullptr};
      n.has_normal = 1; n.input_is_nopeaks = 1;
      n.cells = g[i].cells.data(); n.n_cells = (int32_t)g[i].cells.size();
      n.radius = radius; n.weight_intensity = weight_intensity ? 1 : 0;
      n.constraints = g[i].has_constraint ? &g[i].constraint : nullptr;
      n.n_constraints = g[i].has_constraint ? 1 : 0;
    }
    const int rc = cfear_graph_save(path.c_str(), nodes.data(), (int32_t)nodes.size());
    if (rc != CFEAR_OK) throw CfearError(rc, cfear_status_string(rc));
  }
  // scan_ of a stream's last frame (odometrykeyframefuser.cpp:172, 244): surface points + the two clouds
  cfear_scan* GetScan(int stream) { cfear_scan* s = nullptr; ctx_.check(cfear_odometry_get_scan(od_, stream, &s)); return s; }
  PointCloud GetCloud(int stream, bool peaks) {
    int32_t n = 0;
    ctx_.check((peaks ? cfear_odometry_get_peaks : cfear_odometry_get_cloud)(od_, stream, nullptr, 0, &n));
    PointCloud c((size_t)n);
    if (n) ctx_.check((peaks ? cfear_odometry_get_peaks : cfear_odometry_get_cloud)(od_, stream, &c[0].x, n, &n));
    return c;
  }
 private:
  Context& ctx_;
  cfear_odometry* od_ = nullptr;
  int n_;
  std::vector<std::vector<GraphNode>> graph_;
  struct Status { double distance_traveled = 0.0; unsigned frame_nr = 0; };
  std::vector<Status> status_;
};

// A parameter grid of odometry streams as one batch (cfear_odometry_grid): stream s runs configs[stream_config[s]] on the
// images of sequence stream_sequence[s]; with both lists empty the streams are the full product, sequence-major and
// configuration fastest (the reference's job_<s + 1> of a grid_search evaluation).
class OdometryGrid {
 public:
  struct Plan { std::vector<cfear_grid_stream> streams; cfear_grid_totals totals; };
  OdometryGrid(Context& ctx, int rows, int cols, const std::vector<cfear_odometry_params>& configs, int n_sequences,
               const std::vector<int32_t>& stream_sequence = {}, const std::vector<int32_t>& stream_config = {})
      : ctx_(ctx) {
    const bool product = stream_sequence.empty() && stream_config.empty();
    n_ = product ? n_sequences * (int)configs.size() : (int)stream_sequence.size();
    cfear_polar_desc d{rows, cols, cols, n_sequences, (int64_t)rows * cols};
    ctx_.check(cfear_odometry_grid_create(ctx_.get(), &d, configs.data(), (int32_t)configs.size(), product ? nullptr : stream_sequence.data(),
                                          product ? nullptr : stream_config.data(), n_, &grid_));
  }
  ~OdometryGrid() { cfear_odometry_grid_destroy(grid_); }
  OdometryGrid(const OdometryGrid&) = delete;
  OdometryGrid& operator=(const OdometryGrid&) = delete;
  // the grouping as host code: needs no context and no device; throws CfearError with the refusal's reason
  static Plan plan(int rows, int cols, const std::vector<cfear_odometry_params>& configs, int n_sequences,
                   const std::vector<int32_t>& stream_sequence = {}, const std::vector<int32_t>& stream_config = {}) {
    const bool product = stream_sequence.empty() && stream_config.empty();
    const int n = product ? n_sequences * (int)configs.size() : (int)stream_sequence.size();
    cfear_polar_desc d{rows, cols, cols, n_sequences, (int64_t)rows * cols};
    Plan p;
    p.streams.resize((size_t)(n > 0 ? n : 0));
    char why[256] = "";
    const int st = cfear_odometry_grid_plan(&d, configs.data(), (int32_t)configs.size(), product ? nullptr : stream_sequence.data(),
                                            product ? nullptr : stream_config.data(), n, p.streams.data(), &p.totals, why, (int32_t)sizeof(why));
    if (st != CFEAR_OK) throw CfearError(st, why);
    return p;
  }
  int size() const { return n_; }
  // polar: [n_sequences][rows][cols] uint8 (host or device)
  std::vector<cfear_frame_info> processFrame(const uint8_t* polar) {
    std::vector<cfear_frame_info> info((size_t)n_);
    ctx_.check(cfear_odometry_grid_process(grid_, polar, info.data()));
    return info;
  }
 private:
  Context& ctx_;
  cfear_odometry_grid* grid_ = nullptr;
  int n_ = 0;
};

}  // namespace CFEAR_Radarodometry

// CorAlRadarQuality (coral_alignment_quality AlignmentQuality.cpp:99-230) over two peak clouds.
namespace CorAlignment {
class CorAlRadarQuality {
 public:
  CorAlRadarQuality(CFEAR_Radarodometry::Context& ctx, const CFEAR_Radarodometry::PointCloud& ref,
                    const CFEAR_Radarodometry::Pose2d& ref_pose, const CFEAR_Radarodometry::PointCloud& src,
                    const CFEAR_Radarodometry::Pose2d& src_pose,
                    const CFEAR_Radarodometry::Pose2d& Toffset = CFEAR_Radarodometry::Pose2d{0, 0, 0}, double radius = 1.0,
                    bool weight_res_intensity = false) {
    cfear_coral_job j{};
    j.ref_xyzi = &ref[0].x; j.src_xyzi = &src[0].x;
    j.n_ref = (int32_t)ref.size(); j.n_src = (int32_t)src.size();
    j.ref_pose[0] = ref_pose.x; j.ref_pose[1] = ref_pose.y; j.ref_pose[2] = ref_pose.theta;
    j.src_pose[0] = src_pose.x; j.src_pose[1] = src_pose.y; j.src_pose[2] = src_pose.theta;
    j.offset[0] = Toffset.x; j.offset[1] = Toffset.y; j.offset[2] = Toffset.theta;
    cfear_coral_params p;
    cfear_coral_params_default(&p);
    p.radius = radius; p.weight_res_intensity = weight_res_intensity ? 1 : 0;
    ctx.check(cfear_coral_quality(ctx.get(), &j, &p, &res_, nullptr));
    valid_ = res_.valid != 0;
  }
  std::vector<double> GetQualityMeasure() const { return {res_.joint, res_.sep, res_.overlap}; }
  bool valid_ = false;
 private:
  cfear_coral_result res_{};
};

// Cen2018Radar (ScanType.h:148, ScanType.cpp:68-88): the Cen and Newman 2018 landmark cloud of one polar sweep.  Parameters
// carries the members of PoseScan::Parameters (ScanType.h:55-76) the constructor reads.  sensor_min_distance reaches
// cen2018features as `int min_range`, a BIN index (Utils.cpp:348, :402): int(2.5) = bin 2 whatever range_res is -- the mirror
// truncates it the same way.
class Cen2018Radar {
 public:
  struct Parameters {
    double sensor_min_distance = 2.5, range_res = 0.04328;
    bool compensate = true, ccw = false;
  };
  Cen2018Radar(CFEAR_Radarodometry::Context& ctx, const Parameters& pars, const uint8_t* image, int rows, int cols, int stride,
               const CFEAR_Radarodometry::Pose2d& T = CFEAR_Radarodometry::Pose2d{0, 0, 0},
               const CFEAR_Radarodometry::Pose2d& Tmotion = CFEAR_Radarodometry::Pose2d{0, 0, 0})
      : T_(T), Tmotion_(Tmotion) {
    cfear_polar_desc d{rows, cols, stride, 1, 0};
    cfear_cen2018_params p;
    cfear_cen2018_params_default(&p);                      // zq 3.0, sigma_gauss 17 (ScanType.cpp:72)
    p.min_range_bins = (int32_t)pars.sensor_min_distance;
    p.range_res = pars.range_res;
    const int32_t cap = rows * ((cols + 1) / 2);           // a row of n bins holds at most ceil(n / 2) runs
    cloud_.resize((size_t)cap);
    std::vector<int32_t> tg((size_t)cap * 2);
    int32_t n = 0;
    ctx.check(cfear_filter_cen2018(ctx.get(), image, &d, &p, &cloud_[0].x, &n, cap, tg.data(), nullptr, nullptr));
    cloud_.resize((size_t)n);
    targets_.assign(tg.begin(), tg.begin() + 2 * (size_t)n);
    if (pars.compensate) CFEAR_Radarodometry::Compensate(ctx, cloud_, Tmotion_, pars.ccw);      // ScanType.cpp:86-87
  }
#ifdef CFEAR_HIP_HAVE_CV_BRIDGE
  // the reference's constructor shape (ScanType.cpp:68)
  Cen2018Radar(const Parameters& pars, cv_bridge::CvImagePtr& polar, const Eigen::Affine3d& T, const Eigen::Affine3d& Tmotion)
      : Cen2018Radar(CFEAR_Radarodometry::Context::Default(), pars, polar->image.data, polar->image.rows, polar->image.cols,
                     (int)polar->image.step, CFEAR_Radarodometry::Affine3dToPose2d(T), CFEAR_Radarodometry::Affine3dToPose2d(Tmotion)) {}
#endif
  const CFEAR_Radarodometry::PointCloud& GetCloud() const { return cloud_; }
  const std::vector<int32_t>& GetTargets() const { return targets_; }       // (azimuth, bin) pairs: targets_ rows 0 and 1
  CFEAR_Radarodometry::Pose2d T_, Tmotion_;
 private:
  CFEAR_Radarodometry::PointCloud cloud_;
  std::vector<int32_t> targets_;
};

// cen2019features (Utils.h:46, Utils.cpp:495): the Cen and Newman 2019 targets of one polar sweep as (azimuth, bin) pairs.  The
// reference's fft_data is the uint8 sweep times float(1 / 255.0) (ScanType.cpp:94); here it is the uint8 sweep itself.
inline std::vector<int32_t> cen2019features(CFEAR_Radarodometry::Context& ctx, const uint8_t* image, int rows, int cols, int stride,
                                            int max_points = 1000, int min_range = 0) {
  cfear_polar_desc d{rows, cols, stride, 1, 0};
  cfear_cen2019_params p;
  cfear_cen2019_params_default(&p);
  p.max_points = max_points;
  p.min_range_bins = min_range;
  const int32_t cap = rows * ((cols + 1) / 2);             // a row of n bins holds at most ceil(n / 2) runs
  std::vector<float> xyzi((size_t)cap * 4);
  std::vector<int32_t> tg((size_t)cap * 2);
  int32_t n = 0;
  ctx.check(cfear_filter_cen2019(ctx.get(), image, &d, &p, xyzi.data(), &n, cap, tg.data(), nullptr, nullptr, nullptr));
  tg.resize(2 * (size_t)n);
  return tg;
}
// Which of those targets hang on the order among equal h that the reference's std::sort leaves open (cfear_cen2019_order_audit;
// DESIGN.md section 4.20).  record.n_marks_in == record.n_marks_out: no order changes this sweep.  targets are cen2019features',
// certain[k] says whether every order emits target k.
struct Cen2019OrderAudit {
  cfear_cen2019_order_record record;
  std::vector<int32_t> targets;      // (azimuth, bin) pairs
  std::vector<uint8_t> certain;
  bool clear() const { return record.n_marks_in == record.n_marks_out; }
};
inline Cen2019OrderAudit cen2019OrderAudit(CFEAR_Radarodometry::Context& ctx, const uint8_t* image, int rows, int cols, int stride,
                                           int max_points = 1000, int min_range = 0) {
  cfear_polar_desc d{rows, cols, stride, 1, 0};
  cfear_cen2019_params p;
  cfear_cen2019_params_default(&p);
  p.max_points = max_points;
  p.min_range_bins = min_range;
  const int32_t cap = rows * ((cols + 1) / 2);
  Cen2019OrderAudit out;
  out.targets.resize((size_t)cap * 2);
  out.certain.resize((size_t)cap);
  ctx.check(cfear_cen2019_order_audit(ctx.get(), image, &d, &p, &out.record, out.targets.data(), out.certain.data(), cap, nullptr));
  out.targets.resize(2 * (size_t)out.record.n_targets);
  out.certain.resize((size_t)out.record.n_targets);
  return out;
}
#ifdef CFEAR_HIP_HAVE_CV_BRIDGE
// the reference's shape: targets = Ones(3, n) with the azimuths in row 0 and the bins in row 1 (Utils.cpp:584-592); Targets is
// Eigen::MatrixXd there
template <class Targets>
double cen2019features(const cv::Mat& fft_data, Targets& targets, int max_points, int min_range) {
  const std::vector<int32_t> tg = cen2019features(CFEAR_Radarodometry::Context::Default(), fft_data.data, fft_data.rows, fft_data.cols,
                                                  (int)fft_data.step, max_points, min_range);
  const int n = (int)(tg.size() / 2);
  targets = Targets::Ones(3, n);
  for (int k = 0; k < n; k++) {
    targets(0, k) = tg[2 * (size_t)k];
    targets(1, k) = tg[2 * (size_t)k + 1];
  }
  return 0.0;
}
#endif

// p2pQuality, keypointRepetability (AlignmentQuality.h:119-150, AlignmentQuality.cpp:235-328) and scanEvaluator
// (ScanEvaluator.h:21-137, ScanEvaluator.cpp:4-114) over cfear_p2p_quality.  A PoseScan here is the cloud, the pose and the
// id the measures read (ScanType.h: GetCloudNoCopy, GetAffine, pose_id); Eigen::Affine3d becomes Pose2d.
struct PoseScan {
  CFEAR_Radarodometry::PointCloud cloud;
  CFEAR_Radarodometry::Pose2d T{0, 0, 0};
  int pose_id = 0;
  const CFEAR_Radarodometry::Pose2d& GetAffine() const { return T; }
};
typedef std::shared_ptr<PoseScan> PoseScan_S;

class AlignmentQuality {
 public:
  class parameters {                                                           // AlignmentQuality.h:53-86
   public:
    parameters() {}
    std::string method = "P2L";
    double radius = 3;
    bool weight_res_intensity = false;
    bool output_overlap = true;
    bool visualize = false;
  };
  AlignmentQuality(const parameters& par, const CFEAR_Radarodometry::Pose2d& Toffset) : par_(par), Toffset_(Toffset) {
    quality_ = {0, 0, 0};
    residuals_ = {0, 0, 0};                                                    // AlignmentQuality.h:92: p2pQuality pushes BEHIND these
  }
  virtual ~AlignmentQuality() {}
  virtual std::vector<double> GetResiduals() { return residuals_; }
  virtual std::vector<double> GetQualityMeasure() { return quality_; }
  // Tchange = Tref.inverse() * Tsrc * Toffset (AlignmentQuality.cpp:260-264) as cfear_p2p_job::T: the inverse is
  // (R^T, -R^T t), every product a plain fp64 multiply and add, left to right -- api.p2p_tchange is the same formula
  static std::array<double, 6> Tchange(const CFEAR_Radarodometry::Pose2d& ref, const CFEAR_Radarodometry::Pose2d& src,
                                       const CFEAR_Radarodometry::Pose2d& off) {
    typedef std::array<double, 6> A;                                           // l0 l1 l2 l3 t0 t1
    const auto aff = [](const CFEAR_Radarodometry::Pose2d& p) { const double c = std::cos(p.theta), s = std::sin(p.theta); return A{{c, -s, s, c, p.x, p.y}}; };
    const auto mul = [](const A& a, const A& b) {
      return A{{a[0] * b[0] + a[1] * b[2], a[0] * b[1] + a[1] * b[3], a[2] * b[0] + a[3] * b[2], a[2] * b[1] + a[3] * b[3],
                a[0] * b[4] + a[1] * b[5] + a[4], a[2] * b[4] + a[3] * b[5] + a[5]}};
    };
    const A r = aff(ref);
    const A inv{{r[0], r[2], r[1], r[3], -(r[0] * r[4] + r[2] * r[5]), -(r[1] * r[4] + r[3] * r[5])}};
    const A m = mul(mul(inv, aff(src)), aff(off));
    return A{{m[0], m[1], m[4], m[2], m[3], m[5]}};
  }
  parameters par_;
  const CFEAR_Radarodometry::Pose2d Toffset_;
  std::vector<double> quality_;
  std::vector<double> residuals_;
  bool valid_ = false;

 protected:
  // one cfear_p2p_quality call for (ref, src, Toffset); per_point: the nearest d of every source point, -1 without one
  cfear_p2p_result Run(CFEAR_Radarodometry::Context& ctx, const PoseScan& ref, const PoseScan& src, std::vector<float>* per_point) const {
    cfear_p2p_job j{};
    j.ref_xyzi = ref.cloud.empty() ? nullptr : &ref.cloud[0].x;
    j.src_xyzi = src.cloud.empty() ? nullptr : &src.cloud[0].x;
    j.n_ref = (int32_t)ref.cloud.size(); j.n_src = (int32_t)src.cloud.size();
    const std::array<double, 6> T = Tchange(ref.T, src.T, Toffset_);
    for (int k = 0; k < 6; k++) j.T[k] = T[(size_t)k];
    if (per_point) per_point->assign(src.cloud.size() + 1, -1.0f);
    cfear_p2p_result r{};
    ctx.check(cfear_p2p_quality(ctx.get(), &j, par_.radius, &r, per_point ? per_point->data() : nullptr));
    if (per_point) per_point->resize(src.cloud.size());
    return r;
  }
};
typedef std::shared_ptr<AlignmentQuality> AlignmentQuality_S;

class p2pQuality : public AlignmentQuality {
 public:
  p2pQuality(PoseScan_S ref, PoseScan_S src, const AlignmentQuality::parameters& par,
             const CFEAR_Radarodometry::Pose2d Toffset = CFEAR_Radarodometry::Pose2d{0, 0, 0})
      : p2pQuality(CFEAR_Radarodometry::Context::Default(), ref, src, par, Toffset) {}
  p2pQuality(CFEAR_Radarodometry::Context& ctx, PoseScan_S ref, PoseScan_S src, const AlignmentQuality::parameters& par,
             const CFEAR_Radarodometry::Pose2d Toffset = CFEAR_Radarodometry::Pose2d{0, 0, 0})
      : AlignmentQuality(par, Toffset) {
    std::vector<float> pp;
    record_ = Run(ctx, *ref, *src, &pp);
    for (float d : pp)
      if (d >= 0.0f) residuals_.push_back((double)d);                          // :283-285, source order
    quality_ = {record_.mean, 0, 0};                                           // GetQualityMeasure (:235-248): sum / (matched + 3)
  }
  std::vector<double> GetResiduals() override { return residuals_; }
  std::vector<double> GetQualityMeasure() override { return quality_; }
  cfear_p2p_result record_{};
};

class keypointRepetability : public AlignmentQuality {
 public:
  keypointRepetability(PoseScan_S ref, PoseScan_S src, const AlignmentQuality::parameters& par,
                       const CFEAR_Radarodometry::Pose2d Toffset = CFEAR_Radarodometry::Pose2d{0, 0, 0})
      : keypointRepetability(CFEAR_Radarodometry::Context::Default(), ref, src, par, Toffset) {}
  keypointRepetability(CFEAR_Radarodometry::Context& ctx, PoseScan_S ref, PoseScan_S src, const AlignmentQuality::parameters& par,
                       const CFEAR_Radarodometry::Pose2d Toffset = CFEAR_Radarodometry::Pose2d{0, 0, 0})
      : AlignmentQuality(par, Toffset) {
    record_ = Run(ctx, *ref, *src, nullptr);
    const double matched = (double)record_.matched, total = (double)record_.n_src;
    quality_ = {matched / total, matched, total};                               // NaN for an empty source cloud, as 0.0 / 0.0 there
  }
  cfear_p2p_result record_{};
};

// CartesianRadar (ScanType.h:160-178, ScanType.cpp:191-209): the sweep resampled into a W x W float image by
// cfear_polar_to_cartesian.  The reference's constructor calls radar_polar_to_cartesian with its DEFAULT arguments (0.04328,
// 0.2384, 300) whatever pars says and only stores pars.cart_resolution / cart_pixel_width, which CorAlCartQuality reads; so
// does this one (image_params overrides the geometry of the image for callers that want another).
class CartesianRadar : public PoseScan {
 public:
  struct Parameters {                                                          // PoseScan::Parameters, ScanType.h:55-91
    double sensor_min_distance = 2.5;
    float cart_resolution = 0.2384f;
    int cart_pixel_width = 300;
  };
  CartesianRadar(CFEAR_Radarodometry::Context& ctx, const Parameters& pars, const uint8_t* image, int rows, int cols, int stride,
                 const CFEAR_Radarodometry::Pose2d& pose = CFEAR_Radarodometry::Pose2d{0, 0, 0}, const cfear_cart_params* image_params = nullptr)
      : sensor_min_distance(pars.sensor_min_distance), cart_resolution_(pars.cart_resolution), cart_pixel_width_(pars.cart_pixel_width) {
    T = pose;
    cfear_polar_desc d{rows, cols, stride, 1, 0};
    cfear_cart_params p;
    cfear_cart_params_default(&p);
    if (image_params) p = *image_params;
    width_ = p.cart_pixel_width;
    cart_.assign((size_t)(width_ > 0 ? width_ : 0) * (size_t)(width_ > 0 ? width_ : 0), 0.0f);
    ctx.check(cfear_polar_to_cartesian(ctx.get(), image, &d, &p, cart_.data()));
  }
#ifdef CFEAR_HIP_HAVE_CV_BRIDGE
  // the reference's constructor shape (ScanType.cpp:191); Tmotion is not read there either
  CartesianRadar(const Parameters& pars, cv_bridge::CvImagePtr& polar, const Eigen::Affine3d& T, const Eigen::Affine3d& Tmotion)
      : CartesianRadar(CFEAR_Radarodometry::Context::Default(), pars, polar->image.data, polar->image.rows, polar->image.cols,
                       (int)polar->image.step, CFEAR_Radarodometry::Affine3dToPose2d(T)) { (void)Tmotion; }
#endif
  const std::string ToString() { return "CartesianRadar"; }
  std::vector<float> cart_;                                                    // [width_][width_]
  int width_ = 0;
  double sensor_min_distance, cart_resolution_;
  int cart_pixel_width_;
};
typedef std::shared_ptr<CartesianRadar> CartesianRadar_S;

// CorAlCartQuality (AlignmentQuality.h:184-200, AlignmentQuality.cpp:356-386): quality_ = {sum |RotoTranslation(src.cart,
// Tchange, ref.cart_resolution_) - ref.cart|, 0, 0}.  The reference takes Tsrc AND Tref from the source scan (:363-364), so
// Tchange = Tsrc^-1 Tsrc Toffset and the reference scan's pose is not read; RotoTranslation then hands the yaw, in radians,
// to getRotationMatrix2D as degrees (cfear_cart_quality_batch does the same).
class CorAlCartQuality : public AlignmentQuality {
 public:
  CorAlCartQuality(CartesianRadar_S ref, CartesianRadar_S src, const AlignmentQuality::parameters& par,
                   const CFEAR_Radarodometry::Pose2d Toffset = CFEAR_Radarodometry::Pose2d{0, 0, 0})
      : CorAlCartQuality(CFEAR_Radarodometry::Context::Default(), ref, src, par, Toffset) {}
  CorAlCartQuality(CFEAR_Radarodometry::Context& ctx, CartesianRadar_S ref, CartesianRadar_S src, const AlignmentQuality::parameters& par,
                   const CFEAR_Radarodometry::Pose2d Toffset = CFEAR_Radarodometry::Pose2d{0, 0, 0})
      : AlignmentQuality(par, Toffset) {
    if (ref->width_ != src->width_ || src->width_ <= 0)
      throw CFEAR_Radarodometry::CfearError(CFEAR_ERR_INVALID_ARGUMENT, "CorAlCartQuality: images of different widths");
    const std::array<double, 6> T = Tchange(src->T, src->T, Toffset_);         // both from the SOURCE scan
    cfear_cart_job j{};
    j.src = src->cart_.data(); j.ref = ref->cart_.data();
    j.x = T[2]; j.y = T[5]; j.yaw = std::atan2(T[3], T[4]);                    // Affine3dToEigVectorXYeZ of a planar pose
    ctx.check(cfear_cart_quality_batch(ctx.get(), &j, 1, src->width_, (float)ref->cart_resolution_, &record_, nullptr));
    if (record_.status != CFEAR_OK)
      throw CFEAR_Radarodometry::CfearError(record_.status, "CorAlCartQuality: the pose offset is not finite or beyond 2^20 pixels");
    quality_ = {record_.abs_diff, 0, 0};
  }
  cfear_cart_result record_{};
};

// AlignmentQualityFactory (AlignmentQuality.h:260-312), the branches this header has classes for: two CartesianRadar scans
// give CorAlCartQuality whatever pars.method says; plain PoseScans give p2pQuality or keypointRepetability by pars.method.
class AlignmentQualityFactory {
 public:
  static AlignmentQuality_S CreateQualityType(CFEAR_Radarodometry::Context& ctx, CartesianRadar_S ref, CartesianRadar_S src,
                                              const AlignmentQuality::parameters& pars,
                                              const CFEAR_Radarodometry::Pose2d& Toffset = CFEAR_Radarodometry::Pose2d{0, 0, 0}) {
    return AlignmentQuality_S(new CorAlCartQuality(ctx, ref, src, pars, Toffset));
  }
  static AlignmentQuality_S CreateQualityType(CFEAR_Radarodometry::Context& ctx, PoseScan_S ref, PoseScan_S src,
                                              const AlignmentQuality::parameters& pars,
                                              const CFEAR_Radarodometry::Pose2d& Toffset = CFEAR_Radarodometry::Pose2d{0, 0, 0}) {
    if (pars.method == "P2P") return AlignmentQuality_S(new p2pQuality(ctx, ref, src, pars, Toffset));
    if (pars.method == "keypoint_repetability") return AlignmentQuality_S(new keypointRepetability(ctx, ref, src, pars, Toffset));
    throw CFEAR_Radarodometry::CfearError(CFEAR_ERR_INVALID_ARGUMENT, "no quality metric for scan type with method " + pars.method);
  }
};

// One row of eval.txt (ScanEvaluator.h:21-52 declares the class; the rules are stated in tests/p2p_cpu.py): the pair's
// 1-based index, the two pose ids, the planar distance between the poses, the measure's three values, the offset and
// whether it counts as aligned (its absolute values add up to less than 1e-4).
class datapoint {
 public:
  double distance_;
  std::vector<double> residuals_;
  std::vector<double> perturbation_ = {0, 0, 0};
  std::vector<double> score_ = {0, 0, 0};
  int index_, ref_id_, src_id_;
  datapoint(const int index, const std::vector<double>& residuals, const std::vector<double>& perturbation,
            const std::vector<double>& score, PoseScan_S& ref, PoseScan_S& src)
      : residuals_(residuals), perturbation_(perturbation), score_(score), index_(index), ref_id_(ref->pose_id), src_id_(src->pose_id) {
    const double dx = ref->T.x - src->T.x, dy = ref->T.y - src->T.y;
    distance_ = std::sqrt(dx * dx + dy * dy);
  }
  // the column names of eval.txt; the fifth carries the reference's leading space
  static std::vector<std::string> HeaderToString() {
    static const char* const kColumns[11] = {"index", "ref_id", "src_id", "distance", " score1", "score2", "score3",
                                             "aligned", "error x", "error y", "error theta"};
    return std::vector<std::string>(kColumns, kColumns + 11);
  }
  // the row in the header's order: integers as %d, doubles as %f (std::to_string), aligned as 1 / 0
  const std::vector<std::string> ValsToString() {
    std::vector<std::string> row;
    for (int v : {index_, ref_id_, src_id_}) row.push_back(std::to_string(v));
    row.push_back(std::to_string(distance_));
    for (int k = 0; k < 3; k++) row.push_back(std::to_string(score_[(size_t)k]));
    row.push_back(aligned() ? "1" : "0");
    for (int k = 0; k < 3; k++) row.push_back(std::to_string(perturbation_[(size_t)k]));
    return row;
  }
  bool aligned() { return aligned(perturbation_); }
  static bool aligned(const std::vector<double>& perturbation) {
    double l1 = 0.0;
    for (size_t k = 0; k < perturbation.size(); k++) l1 += std::fabs(perturbation[k]);
    return l1 < 1e-4;
  }
};

// comma-joined, no trailing comma (what Utils.h declares as Vec2String)
inline const std::string Vec2String(const std::vector<std::string>& vec) {
  std::string joined;
  for (size_t k = 0; k < vec.size(); k++) {
    if (k) joined += ',';
    joined += vec[k];
  }
  return joined;
}

// scanEvaluator (ScanEvaluator.h:53-137 declares it) over a sequence held in memory: every pair (scan[k - 1], scan[k]),
// k >= scan_spacing, at the aligned offset and at offset_rotation_steps misaligned ones.  quality_par.method: "P2P" or
// "keypoint_repetability" (CorAlRadarQuality has its own class above).  One cfear_p2p_quality call per pair and offset;
// api.scanEvaluator puts the whole sequence into one batched call.
class scanEvaluator {
 public:
  class parameters {                                                           // the defaults of ScanEvaluator.h:58-113
   public:
    parameters() {}
    int scan_spacing = 1;
    double range_error = 0.5;
    double theta_range = 2 * M_PI / 4.0;
    int offset_rotation_steps = 2;
    double theta_error = 0.57 * M_PI / 180.0;
    std::string output_directory = "";
    std::string output_eval_file = "eval.txt";
  };
  scanEvaluator(std::vector<PoseScan_S>& reader, const parameters& eval_par, const AlignmentQuality::parameters& alignment_par)
      : scanEvaluator(CFEAR_Radarodometry::Context::Default(), reader, eval_par, alignment_par) {}
  scanEvaluator(CFEAR_Radarodometry::Context& ctx, std::vector<PoseScan_S>& reader, const parameters& eval_par,
                const AlignmentQuality::parameters& alignment_par)
      : par_(eval_par), quality_par_(alignment_par) {
    // what the reference asserts of its parameters, and the measures this mirror serves
    if (!(par_.range_error > 0.0 && par_.theta_range >= -2.220446049250313e-16 && par_.theta_error >= 0.0 && par_.scan_spacing >= 1))
      throw CFEAR_Radarodometry::CfearError(CFEAR_ERR_INVALID_ARGUMENT, "scanEvaluator: parameters out of range");
    const bool p2p = quality_par_.method == "P2P";
    if (!p2p && quality_par_.method != "keypoint_repetability")
      throw CFEAR_Radarodometry::CfearError(CFEAR_ERR_INVALID_ARGUMENT, "scanEvaluator: method must be P2P or keypoint_repetability");
    CreatePerturbations();
    for (size_t k = (size_t)par_.scan_spacing; k < reader.size(); k++) {        // pair number k - scan_spacing + 1
      PoseScan_S& ref = reader[k - 1];
      PoseScan_S& src = reader[k];
      for (const std::vector<double>& off : vek_perturbation_) {
        const CFEAR_Radarodometry::Pose2d Toffset{off[0], off[1], off[2]};
        std::unique_ptr<AlignmentQuality> q;
        if (p2p) q.reset(new p2pQuality(ctx, ref, src, quality_par_, Toffset));
        else q.reset(new keypointRepetability(ctx, ref, src, quality_par_, Toffset));
        datapoints_.emplace_back((int)(k - (size_t)par_.scan_spacing) + 1, q->GetResiduals(), off, q->GetQualityMeasure(), ref, src);
      }
    }
  }
  // the aligned offset first, then `steps` offsets of length range_error at the angles i / steps * theta_range, each with
  // the rotation theta_error
  void CreatePerturbations() {
    const int steps = par_.offset_rotation_steps;
    vek_perturbation_.assign(1, std::vector<double>(3, 0.0));
    for (int i = 0; i < steps; i++) {
      const double angle = (double)i / (double)steps * par_.theta_range;
      vek_perturbation_.push_back({par_.range_error * std::cos(angle), par_.range_error * std::sin(angle), par_.theta_error});
    }
  }
  void SaveEvaluation() { SaveEvaluation(par_.output_directory + "/" + par_.output_eval_file); }
  void SaveEvaluation(const std::string& path) {                               // header line, then one line per datapoint
    std::ofstream out(path);
    out << Vec2String(datapoint::HeaderToString()) << "\n";
    for (datapoint& d : datapoints_) out << Vec2String(d.ValsToString()) << "\n";
  }
  std::vector<std::vector<double>> vek_perturbation_;
  std::vector<datapoint> datapoints_;

 private:
  const parameters par_;
  const AlignmentQuality::parameters quality_par_;
};

// PythonClassifierInterface + LogisticRegression (alignmentinterface.h:32-119, alignmentinterface.cpp:14-279) without the
// embedded interpreter: fit() minimises the objective of sklearn's LogisticRegression(class_weight="balanced") on the GPU
// (cfear_logreg_fit_batch).  Eigen::MatrixXd X_ becomes row-major doubles with cols_ values a row.  Where the reference
// exits the process on invalid training data (:194-196) fit() throws CfearError.
class LogisticRegression {
 public:
  LogisticRegression() : ctx_(nullptr) {}                                     // the calling thread's default context
  explicit LogisticRegression(CFEAR_Radarodometry::Context& ctx) : ctx_(&ctx) {}
  void AddDataPoint(const std::vector<double>& X_i, const std::vector<double>& y_i) {         // :50-66: y_i.size() rows
    if (y_i.empty() || X_i.size() % y_i.size() != 0 || (!y_.empty() && X_i.size() / y_i.size() != cols_))
      throw CFEAR_Radarodometry::CfearError(CFEAR_ERR_INVALID_ARGUMENT, "AddDataPoint: rows of a different width");
    cols_ = X_i.size() / y_i.size();
    X_.insert(X_.end(), X_i.begin(), X_i.end());
    y_.insert(y_.end(), y_i.begin(), y_i.end());
  }
  void AddDataPoint(const std::vector<double>& x, double y) { AddDataPoint(x, std::vector<double>{y}); }
  bool DataValid() const {                                                     // :172-185
    if (y_.empty() || X_.size() != y_.size() * cols_) return false;
    for (double v : X_) if (!std::isfinite(v)) return false;
    for (double v : y_) if (!std::isfinite(v)) return false;
    return true;
  }
  void fit() {                                                                 // :192-222
    if (!DataValid()) throw CFEAR_Radarodometry::CfearError(CFEAR_ERR_INVALID_ARGUMENT, "training data invalid");
    CFEAR_Radarodometry::Context& ctx = ctx_ ? *ctx_ : CFEAR_Radarodometry::Context::Default();
    cfear_logreg_params par;
    cfear_logreg_params_default(&par);
    cfear_logreg_job job{};
    job.X = X_.data(); job.y = y_.data(); job.n_rows = (int64_t)y_.size();
    job.row_stride = job.n_features = (int32_t)cols_;
    ctx.check(cfear_logreg_fit_batch(ctx.get(), &job, 1, &par, &record_));
    if (record_.status != CFEAR_OK)
      throw CFEAR_Radarodometry::CfearError(record_.status, record_.status == CFEAR_ERR_SOLVER ? "logistic regression did not converge"
                                                                                               : "training data invalid: one class only, or a label that is not 0 or 1");
    coef_.assign(record_.coef, record_.coef + cols_);
    intercept_ = record_.intercept;
    is_fit_ = true;
  }
  bool IsFit() const { return is_fit_; }
  std::vector<double> predict_linear(const std::vector<double>& X) const {     // :271-279
    const size_t d = coef_.size(), n = d ? X.size() / d : 0;
    std::vector<double> score(n);
    for (size_t i = 0; i < n; i++) {
      double s = 0;
      for (size_t k = 0; k < d; k++) s += coef_[k] * X[i * d + k];
      score[i] = s + intercept_;
    }
    return score;
  }
  std::vector<double> predict_proba(const std::vector<double>& X) const {      // :21-33: P(y = 1); zeros when not fitted
    if (!is_fit_) return std::vector<double>(cols_ ? X.size() / cols_ : 0, 0.0);
    std::vector<double> p = predict_linear(X);
    for (double& v : p) v = 1.0 / (1.0 + std::exp(-v));
    return p;
  }
  std::vector<double> predict_proba() const { return predict_proba(X_); }
  std::vector<double> predict(const std::vector<double>& X) const {            // :36-47: the class, 1 where z > 0
    if (!is_fit_) return std::vector<double>(cols_ ? X.size() / cols_ : 0, 0.0);
    std::vector<double> p = predict_linear(X);
    for (double& v : p) v = v > 0.0 ? 1.0 : 0.0;
    return p;
  }
  std::vector<double> predict() const { return predict(X_); }
  // sklearn's confusion_matrix, row-major {tn, fp, fn, tp} (:83-94), and balanced_accuracy_score (:69-80; -1 as the reference)
  static std::array<int64_t, 4> ConfusionMatrix(const std::vector<double>& y_true, const std::vector<double>& y_pred) {
    std::array<int64_t, 4> c{{0, 0, 0, 0}};
    if (y_true.size() != y_pred.size()) return c;
    for (size_t i = 0; i < y_true.size(); i++) c[(y_true[i] != 0.0 ? 2 : 0) + (y_pred[i] != 0.0 ? 1 : 0)]++;
    return c;
  }
  std::array<int64_t, 4> ConfusionMatrix() const { return ConfusionMatrix(y_, predict()); }
  static double Accuracy(const std::vector<double>& y_true, const std::vector<double>& y_pred) {
    if (y_true.size() != y_pred.size() || y_true.empty()) return -1;
    const std::array<int64_t, 4> c = ConfusionMatrix(y_true, y_pred);
    double sum = 0;
    int classes = 0;
    if (c[0] + c[1] > 0) { sum += (double)c[0] / (double)(c[0] + c[1]); classes++; }
    if (c[2] + c[3] > 0) { sum += (double)c[3] / (double)(c[2] + c[3]); classes++; }
    return sum / classes;
  }
  double Accuracy() const { return Accuracy(y_, predict()); }
  void LoadData(const std::string& path) {                                     // :96-130: "y,x0,x1,..." per line
    std::ifstream file(path);
    std::string line;
    std::vector<double> X, y;
    while (std::getline(file, line)) {
      if (line.empty()) continue;
      std::stringstream ls(line);
      std::string value;
      std::getline(ls, value, ',');
      y.push_back(std::stod(value));
      while (std::getline(ls, value, ',')) X.push_back(std::stod(value));
    }
    if (!y.empty()) { cols_ = X.size() / y.size(); X_.swap(X); y_.swap(y); }
  }
  void SaveData(const std::string& path) const {                               // :149-170, the stream's default precision
    std::ofstream f(path, std::ofstream::out);
    if (!f.is_open()) return;
    for (size_t i = 0; i < y_.size(); i++) {
      f << y_[i];
      for (size_t k = 0; k < cols_; k++) f << "," << X_[i * cols_ + k];
      f << std::endl;
    }
  }
  void LoadCoefficients(const std::string& path) {                             // :224-253: "intercept,c0,c1,..."
    std::ifstream file(path);
    std::string line;
    std::vector<double> coefs;
    while (std::getline(file, line)) {
      if (line.empty()) continue;
      std::stringstream ls(line);
      std::string value;
      std::getline(ls, value, ',');
      intercept_ = std::stod(value);
      while (std::getline(ls, value, ',')) coefs.push_back(std::stod(value));
    }
    coef_ = coefs;
    if (!cols_) cols_ = coef_.size();
    is_fit_ = true;
  }
  void SaveCoefficients(const std::string& path) const {                       // :255-269
    std::ofstream f(path);
    if (!f.is_open()) return;
    f << intercept_ << ",";
    for (size_t i = 0; i < coef_.size(); i++) f << coef_[i] << (i + 1 != coef_.size() ? "," : "");
    f << "\n";
  }
  const std::vector<double>& coef() const { return coef_; }
  double intercept() const { return intercept_; }
  const cfear_logreg_result& record() const { return record_; }               // objective, grad_inf, iterations of the last fit()
  std::vector<double> X_, y_;                                                  // training rows [y_.size()][cols_] and labels
  size_t cols_ = 0;
 private:
  CFEAR_Radarodometry::Context* ctx_;
  std::vector<double> coef_;
  double intercept_ = 0.0;
  bool is_fit_ = false;
  cfear_logreg_result record_{};
};

// ScanLearningInterface (alignmentinterface.h:127-218, alignmentinterface.cpp:288-510) over the mirrors above: the 13
// perturbations of AddTrainingData, CorAl and CFEAR quality per pair, the classifiers fitted on the GPU.  A thin mirror:
// one quality call per perturbation (the Python mirror's AddTrainingDataBatch batches a whole sequence).
class ScanLearningInterface {
 public:
  struct s_scan {                                                              // :130-146 (cld is never read)
    CFEAR_Radarodometry::Pose2d T{0, 0, 0};
    const CFEAR_Radarodometry::PointCloud* cldPeaks = nullptr;
    const CFEAR_Radarodometry::MapPointNormal* CFEAR = nullptr;
  };
  explicit ScanLearningInterface(CFEAR_Radarodometry::Context& ctx, bool combined = true)
      : ctx_(ctx), cfear_class(ctx), coral_class(ctx), combined_class(ctx), combined_(combined) {
    const double e = range_error_, th[3] = {0.5 * M_PI / 180.0, 2 * M_PI / 180.0, 15 * M_PI / 180.0}, m[3] = {1, 2, 4};
    vek_perturbation_.push_back({0, 0, 0});                                    // CreatePerturbations (:479-495)
    for (int k = 0; k < 3; k++) {
      vek_perturbation_.push_back({m[k] * e, 0, th[k]}); vek_perturbation_.push_back({0, m[k] * e, th[k]});
      vek_perturbation_.push_back({-m[k] * e, 0, th[k]}); vek_perturbation_.push_back({0, -m[k] * e, th[k]});
    }
  }
  void AddTrainingData(const s_scan& current) {                                // :296-347
    if (frame_++ == 0) { prev_ = current; return; }
    if (std::hypot(current.T.x - prev_.T.x, current.T.y - prev_.T.y) < min_dist_btw_scans_) return;
    for (const CFEAR_Radarodometry::Pose2d& verr : vek_perturbation_) {
      const std::vector<double> xc = CorAlQuality(current, prev_, verr), xf = CFEARQuality(current, prev_, verr);
      const double y = std::fabs(verr.x) + std::fabs(verr.y) + std::fabs(verr.theta) < 0.0001 ? 1.0 : 0.0;
      if (combined_) {
        std::vector<double> x(xc);
        x.insert(x.end(), xf.begin(), xf.end());
        combined_class.AddDataPoint(x, y);
      } else {
        coral_class.AddDataPoint(xc, y);
        cfear_class.AddDataPoint(xf, y);
      }
    }
    prev_ = current;
  }
  void PredAlignment(const s_scan& current, const s_scan& prev, std::map<std::string, double>& quality) {      // :349-367
    const CFEAR_Radarodometry::Pose2d id{0, 0, 0};
    const std::vector<double> xc = CorAlQuality(current, prev, id), xf = CFEARQuality(current, prev, id);
    if (combined_) {
      std::vector<double> x(xc);
      x.insert(x.end(), xf.begin(), xf.end());
      quality["alignment_quality"] = combined_class.predict_linear(x)[0];
    } else {
      quality["coral"] = coral_class.predict_proba(xc)[0];
      quality["CFEAR"] = cfear_class.predict_proba(xf)[0];
    }
  }
  void FitModels(const std::string& = "LogisticRegression") {                  // :423-434
    if (combined_) combined_class.fit();
    else { coral_class.fit(); cfear_class.fit(); }
  }
  void LoadData(const std::string& dir) {                                      // :376-383
    if (combined_) combined_class.LoadData(dir + "/combined.txt");
    else { coral_class.LoadData(dir + "/CorAl.txt"); cfear_class.LoadData(dir + "/CFEAR.txt"); }
  }
  void SaveData(const std::string& dir) {                                      // :386-393
    if (combined_) combined_class.SaveData(dir + "/combined.txt");
    else { coral_class.SaveData(dir + "/CorAl.txt"); cfear_class.SaveData(dir + "/CFEAR.txt"); }
  }
  void LoadCoefficients(const std::string& dir) {                              // :396-403: dir is concatenated without "/"
    if (combined_) combined_class.LoadCoefficients(dir + "trained_alignment_classifier.txt");
    else { coral_class.LoadCoefficients(dir + "trained_alignment_classifier_CorAl.txt"); cfear_class.LoadCoefficients(dir + "trained_alignment_classifier_CFEAR.txt"); }
  }
  void SaveCoefficients(const std::string& dir) {                              // :405-412
    if (combined_) combined_class.SaveCoefficients(dir + "/trained_alignment_classifier.txt");
    else { coral_class.SaveCoefficients(dir + "/trained_alignment_classifier_CorAl.txt"); cfear_class.SaveCoefficients(dir + "/trained_alignment_classifier_CFEAR.txt"); }
  }
  LogisticRegression& Combined() { return combined_class; }
  LogisticRegression& CorAl() { return coral_class; }
  LogisticRegression& CFEAR() { return cfear_class; }
 private:
  std::vector<double> CorAlQuality(const s_scan& cur, const s_scan& prev, const CFEAR_Radarodometry::Pose2d& off) {      // :437-456
    return CorAlRadarQuality(ctx_, *cur.cldPeaks, cur.T, *prev.cldPeaks, prev.T, off).GetQualityMeasure();
  }
  std::vector<double> CFEARQuality(const s_scan& cur, const s_scan& prev, const CFEAR_Radarodometry::Pose2d& off) {      // :459-478, AlignmentQuality.cpp:330-354
    CFEAR_Radarodometry::n_scan_normal_reg reg(ctx_, CFEAR_P2L, CFEAR_LOSS_HUBER, 0.3);
    const double c = std::cos(prev.T.theta), s = std::sin(prev.T.theta);
    const std::vector<CFEAR_Radarodometry::Pose2d> T = {cur.T, {c * off.x - s * off.y + prev.T.x, s * off.x + c * off.y + prev.T.y, prev.T.theta + off.theta}};
    double score = 0;
    std::vector<double> residuals;
    if (!reg.GetCost({cur.CFEAR, prev.CFEAR}, T, score, residuals)) return {0, 0, 0};
    return {score, (double)residuals.size(), (double)(prev.CFEAR->GetSize() + cur.CFEAR->GetSize()) / 2.0};
  }
  CFEAR_Radarodometry::Context& ctx_;
  LogisticRegression cfear_class, coral_class, combined_class;
  const double range_error_ = 0.5, min_dist_btw_scans_ = 0.5;                  // :196-197
  s_scan prev_;
  unsigned frame_ = 0;
  bool combined_;
  std::vector<CFEAR_Radarodometry::Pose2d> vek_perturbation_;
};
}  // namespace CorAlignment

// RSCManager (place_recognition_radar/RadarScancontext.h): descriptor database + candidate retrieval.
class RSCManager {
 public:
  explicit RSCManager(CFEAR_Radarodometry::Context& ctx, const cfear_sc_manager_params* par = nullptr) : ctx_(ctx) {
    cfear_sc_manager_params def;
    if (!par) { cfear_sc_manager_params_default(&def); par = &def; }
    n_candidates_ = par->n_candidates;
    ctx_.check(cfear_sc_manager_create(ctx_.get(), par, &m_));
  }
  ~RSCManager() { cfear_sc_manager_destroy(m_); }
  RSCManager(const RSCManager&) = delete;
  RSCManager& operator=(const RSCManager&) = delete;
  void makeAndSaveScancontextAndKeysRadarCloud(const CFEAR_Radarodometry::PointCloud& cloud,          // RadarScancontext.cpp:156-180
                                               const CFEAR_Radarodometry::Pose2d& Todom) {
    const double T[3] = {Todom.x, Todom.y, Todom.theta};
    ctx_.check(cfear_sc_manager_add(m_, cloud.empty() ? nullptr : &cloud[0].x, (int32_t)cloud.size(), T));
  }
  // makeAndSaveScancontextAndKeysRadarRaw (:148-154): the node's raw 8-bit sweep, rows x cols with `stride` bytes per row (host
  // or device).  raw == nullptr: TBV's settings, transposed when rows < cols as PNGReaderInterface::Get does (utils.cpp:4-19)
  void makeAndSaveScancontextAndKeysRadarRaw(const uint8_t* image, int rows, int cols, int stride, const CFEAR_Radarodometry::Pose2d& Todom,
                                             const cfear_sc_raw_params* raw = nullptr) {
    cfear_sc_raw_params def;
    if (!raw) { cfear_sc_raw_params_default(&def); def.transpose = rows < cols ? 1 : 0; raw = &def; }
    const cfear_polar_desc d{rows, cols, stride, 1, (int64_t)rows * stride};
    const double T[3] = {Todom.x, Todom.y, Todom.theta};
    ctx_.check(cfear_sc_manager_add_raw(m_, image, &d, raw, T));
  }
#ifdef CFEAR_HIP_HAVE_CV_BRIDGE
  // the reference's signature (RadarScancontext.h; loopclosure.cpp:573-577 passes the reader's CV_8U image); unlike the
  // reference, the image is not thresholded in place
  void makeAndSaveScancontextAndKeysRadarRaw(cv::Mat& scan_mat, const CFEAR_Radarodometry::Pose2d& Todom) {
    makeAndSaveScancontextAndKeysRadarRaw(scan_mat.data, scan_mat.rows, scan_mat.cols, (int)scan_mat.step, Todom);
  }
#endif
  std::vector<cfear_sc_candidate> detectLoopClosureID() {                                             // :286-345
    std::vector<cfear_sc_candidate> out((size_t)std::max(n_candidates_, 1));
    int32_t n = 0;
    ctx_.check(cfear_sc_manager_detect(m_, out.data(), (int32_t)out.size(), &n));
    out.resize((size_t)n);
    return out;
  }
 private:
  CFEAR_Radarodometry::Context& ctx_;
  cfear_sc_manager* m_ = nullptr;
  int n_candidates_ = 3;
};

// Whole-graph Scan Context (cfear_sc_detect_sequence): ScanContextClosure's candidates for nodes 0 .. n_detect - 1 in one
// call, as RSCManager returns them node by node (tbv_slam_offline knows the graph before the first detection).  Each node
// gives its cloud in its own frame (peaks or not, as use_peaks chooses), rows 0 and 1 of its node -> world matrix and of the
// inverse (ScNodeRows(GetPose().matrix()), ScNodeRows(GetPose().inverse().matrix())), and its id.
typedef std::array<double, 8> ScNodeRows8;
template <class Matrix4>
inline ScNodeRows8 ScNodeRows(const Matrix4& m) {
  return ScNodeRows8{{m(0, 0), m(0, 1), m(0, 2), m(0, 3), m(1, 0), m(1, 1), m(1, 2), m(1, 3)}};
}
inline std::vector<cfear_sc_node> ScNodes(const std::vector<const CFEAR_Radarodometry::PointCloud*>& clouds,
                                          const std::vector<ScNodeRows8>& T, const std::vector<ScNodeRows8>& Tinv,
                                          const std::vector<int>& ids) {
  if (T.size() != clouds.size() || Tinv.size() != clouds.size() || ids.size() != clouds.size())
    throw CFEAR_Radarodometry::CfearError(CFEAR_ERR_INVALID_ARGUMENT, "one matrix pair and one id per cloud");
  std::vector<cfear_sc_node> nodes(clouds.size());
  for (size_t i = 0; i < clouds.size(); i++) {
    cfear_sc_node& n = nodes[i];
    n = cfear_sc_node{};
    n.cloud.xyzi = clouds[i]->empty() ? nullptr : &(*clouds[i])[0].x;
    n.cloud.n = (int32_t)clouds[i]->size();
    for (int j = 0; j < 8; j++) { n.T[j] = T[i][j]; n.Tinv[j] = Tinv[i][j]; }
    n.id = ids[i];
  }
  return nodes;
}
// -> candidates of every detected node, closest first
inline std::vector<std::vector<cfear_sc_candidate>> DetectLoopClosureSequence(
    CFEAR_Radarodometry::Context& ctx, const std::vector<const CFEAR_Radarodometry::PointCloud*>& clouds,
    const std::vector<ScNodeRows8>& T, const std::vector<ScNodeRows8>& Tinv, const std::vector<int>& ids, int n_aggregate,
    int n_detect, const cfear_sc_manager_params* par = nullptr) {
  cfear_sc_manager_params def;
  if (!par) { cfear_sc_manager_params_default(&def); par = &def; }
  const std::vector<cfear_sc_node> nodes = ScNodes(clouds, T, Tinv, ids);
  const int nc = std::max(par->n_candidates, 1);
  std::vector<cfear_sc_candidate> out((size_t)std::max(n_detect, 1) * nc);
  std::vector<int32_t> n_out((size_t)std::max(n_detect, 1));
  ctx.check(cfear_sc_detect_sequence(ctx.get(), par, nodes.data(), (int32_t)nodes.size(), n_aggregate, n_detect, out.data(),
                                     n_out.data()));
  std::vector<std::vector<cfear_sc_candidate>> res((size_t)std::max(n_detect, 0));
  for (size_t i = 0; i < res.size(); i++) res[i].assign(out.begin() + i * nc, out.begin() + i * nc + n_out[i]);
  return res;
}

// The same for a batch of graphs in one call (cfear_sc_detect_batch, cloud mode): every graph as DetectLoopClosureSequence
// takes it.  The clouds are gathered into the call's one point buffer, so they cross to the device in one copy.
// -> per graph, the candidates of every detected node, closest first (nn_idx counts within the graph)
struct ScGraph {
  std::vector<const CFEAR_Radarodometry::PointCloud*> clouds;
  std::vector<ScNodeRows8> T, Tinv;
  std::vector<int> ids;
  int n_detect = 0;
};
inline std::vector<std::vector<std::vector<cfear_sc_candidate>>> DetectLoopClosureBatch(
    CFEAR_Radarodometry::Context& ctx, const std::vector<ScGraph>& graphs, int n_aggregate,
    const cfear_sc_manager_params* par = nullptr) {
  cfear_sc_manager_params def;
  if (!par) { cfear_sc_manager_params_default(&def); par = &def; }
  std::vector<int32_t> node_off{0}, n_detect, ids;
  std::vector<int64_t> point_off{0};
  std::vector<double> T, Tinv;
  std::vector<float> xyzi;
  size_t rows = 0;
  for (const ScGraph& g : graphs) {
    if (g.T.size() != g.clouds.size() || g.Tinv.size() != g.clouds.size() || g.ids.size() != g.clouds.size())
      throw CFEAR_Radarodometry::CfearError(CFEAR_ERR_INVALID_ARGUMENT, "one matrix pair and one id per cloud");
    for (size_t i = 0; i < g.clouds.size(); i++) {
      if (!g.clouds[i]->empty()) xyzi.insert(xyzi.end(), &(*g.clouds[i])[0].x, &(*g.clouds[i])[0].x + 4 * g.clouds[i]->size());
      point_off.push_back((int64_t)(xyzi.size() / 4));
      T.insert(T.end(), g.T[i].begin(), g.T[i].end());
      Tinv.insert(Tinv.end(), g.Tinv[i].begin(), g.Tinv[i].end());
      ids.push_back(g.ids[i]);
    }
    node_off.push_back(node_off.back() + (int32_t)g.clouds.size());
    n_detect.push_back(g.n_detect);
    rows += (size_t)std::max(g.n_detect, 0);
  }
  cfear_sc_batch b = cfear_sc_batch();
  b.n_graphs = (int32_t)graphs.size();
  b.mode = CFEAR_SC_NODES_CLOUD;
  b.node_off = node_off.data(); b.n_detect = n_detect.data(); b.ids = ids.data();
  b.T = T.data(); b.Tinv = Tinv.data(); b.xyzi = xyzi.data(); b.point_off = point_off.data();
  b.n_aggregate = n_aggregate;
  const int nc = std::max(par->n_candidates, 1);
  std::vector<cfear_sc_candidate> out(std::max<size_t>(rows, 1) * nc);
  std::vector<int32_t> n_out(std::max<size_t>(rows, 1));
  ctx.check(cfear_sc_detect_batch(ctx.get(), par, &b, out.data(), n_out.data()));
  std::vector<std::vector<std::vector<cfear_sc_candidate>>> res(graphs.size());
  size_t row = 0;
  for (size_t g = 0; g < graphs.size(); g++) {
    res[g].resize((size_t)std::max(graphs[g].n_detect, 0));
    for (size_t i = 0; i < res[g].size(); i++, row++) res[g][i].assign(out.begin() + row * nc, out.begin() + row * nc + n_out[row]);
  }
  return res;
}

// Loop-candidate verification of tbv_slam::loopclosure (tbv_slam/src/tbv_slam/loopclosure.cpp:320-384, 261-274,
// 776-808) for a batch of candidates.
namespace tbv_slam {
struct LoopCandidate {
  const CFEAR_Radarodometry::MapPointNormal* from;         // (*graph_)[from].cloud_normal_
  const CFEAR_Radarodometry::MapPointNormal* to;
  const CFEAR_Radarodometry::PointCloud* from_peaks;       // (*graph_)[from].cloud_peaks_
  const CFEAR_Radarodometry::PointCloud* to_peaks;
  CFEAR_Radarodometry::Pose2d Tfrom;                       // (*graph_)[from].GetPose()
  CFEAR_Radarodometry::Pose2d t_be_guess;                  // constraint.t_be on entry
  double sc_sim, odom_bounds;                              // quality["sc-sim"], quality["odom-bounds"]
  int query;                                               // candidates of one query node are selected together
};
inline double VerifyByOdometry(const std::vector<CFEAR_Radarodometry::Pose2d>& relative_motions, double odom_sigma_error = 0.03,
                               bool verify_via_odometry = true) {
  double sim = 0.0;
  static_assert(sizeof(CFEAR_Radarodometry::Pose2d) == 3 * sizeof(double), "Pose2d must be three packed doubles");
  const int rc = cfear_verify_by_odometry(relative_motions.empty() ? nullptr : &relative_motions[0].x,
                                          (int32_t)relative_motions.size(), odom_sigma_error, verify_via_odometry ? 1 : 0, &sim);
  if (rc != CFEAR_OK) throw CFEAR_Radarodometry::CfearError(rc, cfear_status_string(rc));
  return sim;
}
inline std::vector<cfear_verify_result> VerifyLoopCandidates(CFEAR_Radarodometry::Context& ctx,
                                                              const std::vector<LoopCandidate>& cands,
                                                              const cfear_verify_params* par = nullptr) {
  cfear_verify_params def;
  if (!par) { cfear_verify_params_default(&def); par = &def; }
  std::vector<cfear_verify_job> jobs(cands.size());
  for (size_t i = 0; i < cands.size(); i++) {
    const LoopCandidate& c = cands[i];
    cfear_verify_job& j = jobs[i];
    j = cfear_verify_job{};
    j.from_scan = c.from->device(); j.to_scan = c.to->device();
    j.from_peaks = c.from_peaks->empty() ? nullptr : &(*c.from_peaks)[0].x; j.n_from = (int32_t)c.from_peaks->size();
    j.to_peaks = c.to_peaks->empty() ? nullptr : &(*c.to_peaks)[0].x; j.n_to = (int32_t)c.to_peaks->size();
    j.from_pose[0] = c.Tfrom.x; j.from_pose[1] = c.Tfrom.y; j.from_pose[2] = c.Tfrom.theta;
    j.t_be_guess[0] = c.t_be_guess.x; j.t_be_guess[1] = c.t_be_guess.y; j.t_be_guess[2] = c.t_be_guess.theta;
    j.sc_sim = c.sc_sim; j.odom_bounds = c.odom_bounds; j.group = c.query;
  }
  std::vector<cfear_verify_result> res(cands.size());
  ctx.check(cfear_verify_loop_candidates(ctx.get(), jobs.data(), (int32_t)jobs.size(), par, res.data()));
  return res;
}
}  // namespace tbv_slam

// Trajectory evaluation (cfear_eval_trajectories): the KITTI odometry metric of radar_kitti_benchmark/python/eval_odom.py
// for a batch of (estimate, ground truth) pairs.  A trajectory is [n][12] doubles, the rows of the 3 x 4 pose (what
// cfear_kitti_read returns and cfear_kitti_from_xyt builds from planar poses).  -> one summary per pair, and every segment
// row of the batch in `rows` when it is given.  Figures are radians and fractions (include/cfear_hip.h).
inline std::vector<cfear_eval_summary> EvalTrajectories(CFEAR_Radarodometry::Context& ctx, const std::vector<std::vector<double>>& est,
                                                        const std::vector<std::vector<double>>& gt,
                                                        const cfear_eval_params* par = nullptr,
                                                        std::vector<cfear_eval_row>* rows = nullptr) {
  cfear_eval_params def;
  if (!par) { cfear_eval_params_default(&def); par = &def; }
  if (est.size() != gt.size()) throw CFEAR_Radarodometry::CfearError(CFEAR_ERR_INVALID_ARGUMENT, "one ground truth per estimate");
  std::vector<int32_t> le(est.size()), lg(gt.size());
  std::vector<double> e, g;
  int64_t cap = 0;
  for (size_t i = 0; i < est.size(); i++) {
    le[i] = (int32_t)(est[i].size() / 12);
    lg[i] = (int32_t)(gt[i].size() / 12);
    e.insert(e.end(), est[i].begin(), est[i].begin() + (size_t)le[i] * 12);
    g.insert(g.end(), gt[i].begin(), gt[i].begin() + (size_t)lg[i] * 12);
    cap += ((int64_t)le[i] + std::max(par->step_size, 1) - 1) / std::max(par->step_size, 1) * CFEAR_EVAL_NUM_LENGTHS;
  }
  const int rc = cfear_eval_check(par, le.data(), lg.data(), (int32_t)le.size());
  if (rc != CFEAR_OK) throw CFEAR_Radarodometry::CfearError(rc, "evaluation refused: step_size, alignment, or a pair's lengths");
  std::vector<cfear_eval_summary> out(est.size());
  int64_t n_rows = 0;
  if (rows) rows->resize((size_t)cap);
  ctx.check(cfear_eval_trajectories(ctx.get(), e.data(), g.data(), nullptr, le.data(), (int32_t)le.size(), par, out.data(),
                                    rows ? rows->data() : nullptr, rows ? cap : 0, &n_rows));
  if (rows) rows->resize((size_t)n_rows);
  return out;
}

// Pose-graph optimisation of a batch (cfear_pgo_solve_batch): every graph's poses are replaced by its solution in ONE
// device call, one summary per graph.  par == nullptr: CeresLeastSquares::Parameters' defaults.  A graph the host solver
// would refuse fails the whole call before anything is solved: CfearError, with the graph's index in *failed_graph.
struct PoseGraph {
  std::vector<cfear_pose3d> poses;                   // in / out
  std::vector<uint64_t> ids;                         // strictly ascending, one per pose
  std::vector<cfear_graph_constraint> constraints;   // odometry (0) and loop_appearance (1) are optimised
};
inline std::vector<cfear_pgo_summary> SolvePoseGraphs(CFEAR_Radarodometry::Context& ctx, std::vector<PoseGraph>& graphs,
                                                      const cfear_pgo_params* par = nullptr, int32_t* failed_graph = nullptr) {
  cfear_pgo_params def;
  if (!par) { cfear_pgo_params_default(&def); par = &def; }
  std::vector<int64_t> node_off(1, 0), con_off(1, 0);
  std::vector<cfear_pose3d> poses;
  std::vector<uint64_t> ids;
  std::vector<cfear_graph_constraint> cons;
  for (const PoseGraph& g : graphs) {
    if (g.ids.size() != g.poses.size()) throw CFEAR_Radarodometry::CfearError(CFEAR_ERR_INVALID_ARGUMENT, "one id per pose");
    poses.insert(poses.end(), g.poses.begin(), g.poses.end());
    ids.insert(ids.end(), g.ids.begin(), g.ids.end());
    cons.insert(cons.end(), g.constraints.begin(), g.constraints.end());
    node_off.push_back((int64_t)poses.size());
    con_off.push_back((int64_t)cons.size());
  }
  std::vector<cfear_pgo_summary> out(graphs.size());
  ctx.check(cfear_pgo_solve_batch(ctx.get(), poses.data(), ids.data(), node_off.data(), (int64_t)poses.size(), cons.data(), con_off.data(),
                                  (int64_t)cons.size(), (int32_t)graphs.size(), par, out.data(), failed_graph));
  for (size_t g = 0; g < graphs.size(); g++)
    std::copy(poses.begin() + node_off[g], poses.begin() + node_off[g + 1], graphs[g].poses.begin());
  return out;
}

// Scoring the loop detector.  LoopStats (cfear_loop_stats_batch): PoseGraph::UpdateStatistics (posegraph.cpp:332-371) and
// EvaluationManager::getCandidateLoopStatus for every candidate of a batch of graphs in ONE device call; a graph is its
// planar ground-truth poses and one has_Tgt_ flag per node.  LoopCurves (cfear_loop_curves_batch): sklearn's roc_curve, auc
// and precision_recall_curve and the statistics at p_threshold for a batch of experiments, as LoopClosureEval.py and
// 3_loop_closure.py ask for them.  par == nullptr: the reference's constants.
struct LoopGraph {
  std::vector<CFEAR_Radarodometry::Pose2d> gt;       // Tgt of every node
  std::vector<uint8_t> has_gt;                       // has_Tgt_; empty: every node has ground truth
};
inline std::vector<cfear_loop_row> LoopStats(CFEAR_Radarodometry::Context& ctx, const std::vector<LoopGraph>& graphs,
                                             const std::vector<cfear_loop_candidate>& candidates,
                                             const cfear_loop_stats_params* par = nullptr, int64_t* failed_candidate = nullptr) {
  cfear_loop_stats_params def;
  if (!par) { cfear_loop_stats_params_default(&def); par = &def; }
  std::vector<int64_t> off(1, 0);
  std::vector<double> gt;
  std::vector<uint8_t> has;
  for (const LoopGraph& g : graphs) {
    if (!g.has_gt.empty() && g.has_gt.size() != g.gt.size()) throw CFEAR_Radarodometry::CfearError(CFEAR_ERR_INVALID_ARGUMENT, "one has_gt flag per pose");
    for (size_t k = 0; k < g.gt.size(); k++) {
      gt.push_back(g.gt[k].x); gt.push_back(g.gt[k].y); gt.push_back(g.gt[k].theta);
      has.push_back(g.has_gt.empty() ? 1 : g.has_gt[k]);
    }
    off.push_back((int64_t)has.size());
  }
  std::vector<cfear_loop_row> rows(candidates.size());
  ctx.check(cfear_loop_stats_batch(ctx.get(), off.data(), gt.data(), has.data(), (int64_t)has.size(), (int32_t)graphs.size(), candidates.data(),
                                   (int64_t)candidates.size(), par, rows.data(), failed_candidate));
  return rows;
}

// Loop candidates of a batch of graphs verified from the detector's rows (cfear_verify_sc_rows) or from a candidate list
// (cfear_verify_graph_candidates): the body of ScanContextClosure::SearchAndAddConstraint (loopclosure.cpp:653-724) as one
// device stage.  The graphs are added one behind the other; `table` holds one scan per node, in that order.
struct LoopVerifyGraphs {
  std::vector<int32_t> node_off = std::vector<int32_t>(1, 0);
  const CFEAR_Radarodometry::ScanTable* table = nullptr;        // cloud_normal_ of every node
  std::vector<float> peaks;                                      // cloud_peaks_ of every node, [points][4]
  std::vector<int64_t> peak_off = std::vector<int64_t>(1, 0);
  std::vector<CFEAR_Radarodometry::Pose2d> poses;                // GetPose()
  std::vector<CFEAR_Radarodometry::Pose2d> rel;                  // RelativeMotion(k, k + 1); a graph's last entry is ignored
  // one graph: a peaks cloud and a pose per node, and the odometry constraints' motions (one fewer, or none when
  // verify_via_odometry is off)
  void AddGraph(const std::vector<const CFEAR_Radarodometry::PointCloud*>& node_peaks, const std::vector<CFEAR_Radarodometry::Pose2d>& node_poses,
                const std::vector<CFEAR_Radarodometry::Pose2d>& motions) {
    if (node_peaks.size() != node_poses.size() || (!motions.empty() && motions.size() + 1 != node_poses.size()))
      throw CFEAR_Radarodometry::CfearError(CFEAR_ERR_INVALID_ARGUMENT, "one cloud and one pose per node, one motion per step");
    for (size_t i = 0; i < node_peaks.size(); i++) {
      if (!node_peaks[i]->empty()) peaks.insert(peaks.end(), &(*node_peaks[i])[0].x, &(*node_peaks[i])[0].x + 4 * node_peaks[i]->size());
      peak_off.push_back((int64_t)(peaks.size() / 4));
      poses.push_back(node_poses[i]);
      rel.push_back(i < motions.size() ? motions[i] : CFEAR_Radarodometry::Pose2d());
    }
    node_off.push_back(node_off.back() + (int32_t)node_peaks.size());
  }
  cfear_loop_graphs record() const {
    static_assert(sizeof(CFEAR_Radarodometry::Pose2d) == 3 * sizeof(double), "Pose2d must be three packed doubles");
    cfear_loop_graphs g = cfear_loop_graphs();
    g.n_graphs = (int32_t)node_off.size() - 1;
    g.node_off = node_off.data();
    g.table = table ? table->get() : nullptr;
    g.peaks_xyzi = peaks.empty() ? nullptr : peaks.data();
    g.peak_off = peak_off.data();
    g.poses_xyt = poses.empty() ? nullptr : &poses[0].x;
    g.rel_xyt = rel.empty() ? nullptr : &rel[0].x;
    return g;
  }
};
struct LoopVerifyOutput {
  std::vector<cfear_verify_result> results;          // one per compacted candidate, ApplyConstratins applied per query
  std::vector<cfear_loop_verify_candidate> list;     // the candidates as verified
  std::vector<cfear_loop_candidate> loops;           // guess_xyt = the registered t_be: what LoopStats takes
};
inline LoopVerifyOutput VerifyGraphCandidates(CFEAR_Radarodometry::Context& ctx, const LoopVerifyGraphs& graphs,
                                              const std::vector<cfear_loop_verify_candidate>& candidates,
                                              const cfear_loop_verify_params* par = nullptr) {
  cfear_loop_verify_params def;
  if (!par) { cfear_loop_verify_params_default(&def); par = &def; }
  const cfear_loop_graphs g = graphs.record();
  LoopVerifyOutput out;
  out.results.resize(candidates.size()); out.list.resize(candidates.size()); out.loops.resize(candidates.size());
  ctx.check(cfear_verify_graph_candidates(ctx.get(), &g, candidates.data(), (int32_t)candidates.size(), par, out.results.data(),
                                          out.list.data(), out.loops.data()));
  return out;
}
// rows [sum n_detect][n_candidates] and n_out [sum n_detect] as DetectLoopClosureBatch's call leaves them
inline LoopVerifyOutput VerifyScRows(CFEAR_Radarodometry::Context& ctx, const LoopVerifyGraphs& graphs,
                                     const std::vector<cfear_sc_candidate>& rows, const std::vector<int32_t>& n_out,
                                     const std::vector<int32_t>& n_detect, int n_candidates, const cfear_loop_verify_params* par = nullptr) {
  cfear_loop_verify_params def;
  if (!par) { cfear_loop_verify_params_default(&def); par = &def; }
  const cfear_loop_graphs g = graphs.record();
  LoopVerifyOutput out;
  out.results.resize(rows.size()); out.list.resize(rows.size()); out.loops.resize(rows.size());
  int32_t n = 0;
  ctx.check(cfear_verify_sc_rows(ctx.get(), &g, rows.data(), n_out.data(), n_detect.empty() ? nullptr : n_detect.data(), n_candidates, par,
                                 out.results.data(), out.list.data(), out.loops.data(), &n));
  out.results.resize((size_t)n); out.list.resize((size_t)n); out.loops.resize((size_t)n);
  return out;
}
// Sampled covariances for what either call above returned (cfear_verify_sample_covariances): `cov` and `cov_sampled` of the
// registered candidates in out.results are updated in place.
inline void VerifySampleCovariances(CFEAR_Radarodometry::Context& ctx, const LoopVerifyGraphs& graphs, LoopVerifyOutput& out,
                                    const cfear_loop_verify_params* par = nullptr) {
  cfear_loop_verify_params def;
  if (!par) { cfear_loop_verify_params_default(&def); par = &def; }
  if (out.list.size() != out.results.size()) throw CFEAR_Radarodometry::CfearError(CFEAR_ERR_INVALID_ARGUMENT, "VerifySampleCovariances: one record per candidate");
  const cfear_loop_graphs g = graphs.record();
  ctx.check(cfear_verify_sample_covariances(ctx.get(), &g, out.list.data(), (int32_t)out.list.size(), par, out.results.data()));
}

struct LoopExperiment {
  std::vector<uint8_t> y;                            // 0 or 1
  std::vector<double> score;
  std::vector<uint8_t> pos_ok;                       // empty (in every experiment of a call): all 1
};
struct LoopCurve {
  std::vector<double> roc_fpr, roc_tpr, roc_thr, pr_precision, pr_recall, pr_thr;
  cfear_loop_curves_result record;                   // record.status: the experiment's own (CFEAR_ERR_INVALID_ARGUMENT: empty arrays)
};
inline std::vector<LoopCurve> LoopCurves(CFEAR_Radarodometry::Context& ctx, const std::vector<LoopExperiment>& experiments,
                                         const cfear_loop_curves_params* par = nullptr) {
  cfear_loop_curves_params def;
  if (!par) { cfear_loop_curves_params_default(&def); par = &def; }
  std::vector<int64_t> off(1, 0);
  std::vector<uint8_t> y, ok;
  std::vector<double> score;
  for (const LoopExperiment& e : experiments) {
    if (e.y.size() != e.score.size() || (!e.pos_ok.empty() && e.pos_ok.size() != e.y.size()) || (e.pos_ok.empty() && !ok.empty() && !e.y.empty()))
      throw CFEAR_Radarodometry::CfearError(CFEAR_ERR_INVALID_ARGUMENT, "y, score and pos_ok hold one entry per row; pos_ok in every experiment or in none");
    y.insert(y.end(), e.y.begin(), e.y.end());
    score.insert(score.end(), e.score.begin(), e.score.end());
    ok.insert(ok.end(), e.pos_ok.begin(), e.pos_ok.end());
    off.push_back((int64_t)y.size());
  }
  if (!ok.empty() && ok.size() != y.size())
    throw CFEAR_Radarodometry::CfearError(CFEAR_ERR_INVALID_ARGUMENT, "pos_ok in every experiment or in none");
  const size_t total = y.size() + experiments.size();
  std::vector<double> a[6];
  for (auto& v : a) v.assign(total, 0.0);
  std::vector<cfear_loop_curves_result> rec(experiments.size());
  ctx.check(cfear_loop_curves_batch(ctx.get(), off.data(), y.data(), score.data(), ok.empty() ? nullptr : ok.data(), (int64_t)y.size(),
                                    (int32_t)experiments.size(), par, a[0].data(), a[1].data(), a[2].data(), a[3].data(), a[4].data(), a[5].data(),
                                    rec.data(), nullptr));
  std::vector<LoopCurve> out(experiments.size());
  for (size_t e = 0; e < experiments.size(); e++) {
    const size_t o = (size_t)off[e] + e, n_roc = (size_t)rec[e].n_roc, n_pr = (size_t)rec[e].n_pr;
    LoopCurve& c = out[e];
    c.record = rec[e];
    c.roc_fpr.assign(a[0].begin() + o, a[0].begin() + o + n_roc);
    c.roc_tpr.assign(a[1].begin() + o, a[1].begin() + o + n_roc);
    c.roc_thr.assign(a[2].begin() + o, a[2].begin() + o + n_roc);
    c.pr_precision.assign(a[3].begin() + o, a[3].begin() + o + n_pr);
    c.pr_recall.assign(a[4].begin() + o, a[4].begin() + o + n_pr);
    c.pr_thr.assign(a[5].begin() + o, a[5].begin() + o + (n_pr ? n_pr - 1 : 0));
  }
  return out;
}

// EvalTrajectory (eval_trajectory.h:70-184): the collector every executable of the reference ends in.  The Callback*Eigen
// methods append stamped poses; Save() runs One2OneCorrespondance (eval_trajectory.cpp:400-423) through
// cfear_sync_trajectories -- every estimate keeps the ground truth interpolated at its stamp, estimates without bracketing
// ground truth are dropped, and the two vectors are replaced by the synchronised ones -- and writes the five files of
// EvalTrajectory::Save (:265-315; three without a ground truth).  A stamped pose is a POD: the KITTI row of the pose, the
// 6 x 6 covariance and the stamp in nanoseconds (ros::Time::toNSec()).  GetGtVek() feeds OdometryKeyframeFuser::
// AddGroundTruth, as offline_odometry.cpp:134-137 does: after Save() its stamps are the estimate's.
#include <sys/stat.h>
namespace CFEAR_Radarodometry {

class EvalTrajectory {
 public:
  class Parameters {                                         // eval_trajectory.h:75-110, without the topics
   public:
    std::string est_output_dir = "", gt_output_dir = "";
    std::string sequence = "", method = "";
    int job_nr = -1;
  };
  explicit EvalTrajectory(const Parameters& pars, bool disable_callback = true, Context* ctx = nullptr) : par(pars), ctx_(ctx) { (void)disable_callback; }
  void CallbackEigen(const poseStamped& Test, const poseStamped& Tgt) { CallbackESTEigen(Test); CallbackGTEigen(Tgt); }
  void CallbackGTEigen(const poseStamped& Tgt) { gt_vek.push_back(Tgt); }
  void CallbackESTEigen(const poseStamped& Test) { est_vek.push_back(Test); }
  size_t GetSize() { return std::min(gt_vek.size(), est_vek.size()); }
  poseStampedVector& GetGtVek() { return gt_vek; }
  poseStampedVector& GetEstVek() { return est_vek; }
  // Interpolate(t, Tinterpolated), eval_trajectory.h:141-144: the search starts from the first ground-truth pose
  bool Interpolate(int64_t t, poseStamped& Tinterpolated) {
    std::vector<double> g;
    std::vector<int64_t> gs;
    Flatten(gt_vek, g, gs);
    const int32_t n_est = 1, n_gt = (int32_t)gt_vek.size();
    int32_t count = 0;
    cfear_sync_row row{};
    int64_t stamp = 0;
    std::array<double, 12> out{};
    context().check(cfear_sync_trajectories(context().get(), CFEAR_SYNC_INDEPENDENT, nullptr, &t, nullptr, &n_est, g.data(), gs.data(), nullptr, &n_gt, 1,
                                            nullptr, out.data(), &stamp, &row, &count));
    if (!count) return false;
    Tinterpolated = poseStamped(out, gt_vek[(size_t)row.gt_index].cov, t);        // the covariance of the pose before (:455)
    return true;
  }
  // Save(): the file name is Parameters::sequence as it is (the reference maps bag names to NN.txt in DatasetToSequence,
  // eval_trajectory.cpp:64-132; that table stays with the caller)
  void Save() {
    if (est_vek.empty() && gt_vek.empty()) throw CfearError(CFEAR_ERR_INVALID_ARGUMENT, "Nothing to evaluate");
    const std::string& name = par.sequence;
    const bool have_gt = !gt_vek.empty();
    if (have_gt) One2OneCorrespondance();
    std::vector<double> e, g, cov;
    std::vector<int64_t> es, gs;
    Flatten(est_vek, e, es);
    Flatten(gt_vek, g, gs);
    for (const poseStamped& p : est_vek) cov.insert(cov.end(), p.cov.begin(), p.cov.end());
    if (have_gt) {
      MakeDirs(par.gt_output_dir);
      Check(cfear_kitti_write((par.gt_output_dir + name).c_str(), g.data(), (int64_t)gs.size()), par.gt_output_dir + name);
      Check(cfear_tum_write((par.gt_output_dir + "tum_" + name).c_str(), g.data(), gs.data(), (int64_t)gs.size()), par.gt_output_dir + "tum_" + name);
    }
    MakeDirs(par.est_output_dir);
    Check(cfear_kitti_write((par.est_output_dir + name).c_str(), e.data(), (int64_t)es.size()), par.est_output_dir + name);
    Check(cfear_tum_write((par.est_output_dir + "tum_" + name).c_str(), e.data(), es.data(), (int64_t)es.size()), par.est_output_dir + "tum_" + name);
    Check(cfear_cov_write((par.est_output_dir + "cov_" + name).c_str(), cov.data(), es.data(), (int64_t)es.size()), par.est_output_dir + "cov_" + name);
  }

 private:
  Context& context() { return ctx_ ? *ctx_ : Context::Default(); }
  static void Check(int rc, const std::string& path) { if (rc != CFEAR_OK) throw CfearError(rc, path); }
  static void Flatten(const poseStampedVector& v, std::vector<double>& poses, std::vector<int64_t>& stamps) {
    for (const poseStamped& p : v) { poses.insert(poses.end(), p.pose.begin(), p.pose.end()); stamps.push_back(p.t); }
  }
  static void MakeDirs(const std::string& dir) {              // boost::filesystem::create_directories
    for (size_t at = 1; at <= dir.size(); at++)
      if (at == dir.size() || dir[at] == '/') ::mkdir(dir.substr(0, at).c_str(), 0777);
  }
  void One2OneCorrespondance() {
    std::vector<double> e, g;
    std::vector<int64_t> es, gs;
    Flatten(est_vek, e, es);
    Flatten(gt_vek, g, gs);
    const int32_t n_est = (int32_t)est_vek.size(), n_gt = (int32_t)gt_vek.size();
    int32_t count = 0;
    std::vector<double> e_out(e.size()), g_out(e.size());
    std::vector<int64_t> s_out(es.size());
    std::vector<cfear_sync_row> rows(es.size());
    context().check(cfear_sync_trajectories(context().get(), CFEAR_SYNC_CHAINED, e.data(), es.data(), nullptr, &n_est, g.data(), gs.data(), nullptr, &n_gt,
                                            1, e_out.data(), g_out.data(), s_out.data(), rows.data(), &count));
    poseStampedVector revised_est, revised_gt;
    for (int32_t i = 0; i < count; i++) {
      revised_est.push_back(est_vek[(size_t)rows[(size_t)i].est_index]);
      poseStamped gt_i;
      std::copy(g_out.begin() + (size_t)i * 12, g_out.begin() + (size_t)i * 12 + 12, gt_i.pose.begin());
      gt_i.cov = gt_vek[(size_t)rows[(size_t)i].gt_index].cov;
      gt_i.t = s_out[(size_t)i];
      revised_gt.push_back(gt_i);
    }
    est_vek = revised_est;
    gt_vek = revised_gt;
  }
  Parameters par;
  Context* ctx_;
  poseStampedVector est_vek, gt_vek;
};
}  // namespace CFEAR_Radarodometry

// The end of a pose-graph run (tbv_slam_offline.cpp:248-266): graph->Align(), graph->SaveGraphString(), graph->OutputGraph(),
// and the maps PoseGraphVis::ProcessFrame builds, over the PoseGraph records SolvePoseGraphs solved.  GraphTruth holds Tgt and
// has_Tgt_ of every node (empty: no node has ground truth).  AlignPoseGraphs (cfear_graph_align_batch) replaces every graph's
// poses in ONE device call; a graph whose ground-truth positions lie on one line keeps its poses and reports CFEAR_ERR_SOLVER
// in its own summary.  MapPoseGraphs (cfear_graph_map_batch) takes one cloud_peaks_ ([k][4] floats, flattened) per node.
struct GraphTruth {
  std::vector<cfear_pose3d> gt;
  std::vector<uint8_t> has_gt;
};
struct GraphMaps {
  std::vector<float> map, map_gt;                    // [points][4]
  std::vector<cfear_graph_map_summary> ranges;       // per graph: its points in the two maps
};
namespace graph_finish_detail {
inline void Flatten(const std::vector<PoseGraph>& graphs, const std::vector<GraphTruth>& truth, std::vector<cfear_pose3d>& poses,
                    std::vector<cfear_pose3d>& gt, std::vector<uint8_t>& has, std::vector<int64_t>& off) {
  if (truth.size() != graphs.size()) throw CFEAR_Radarodometry::CfearError(CFEAR_ERR_INVALID_ARGUMENT, "one GraphTruth per graph");
  const cfear_pose3d ident{{0, 0, 0}, {0, 0, 0, 1}};
  off.assign(1, 0);
  for (size_t g = 0; g < graphs.size(); g++) {
    const size_t n = graphs[g].poses.size();
    const bool none = truth[g].gt.empty() && truth[g].has_gt.empty();
    if (!none && (truth[g].gt.size() != n || truth[g].has_gt.size() != n))
      throw CFEAR_Radarodometry::CfearError(CFEAR_ERR_INVALID_ARGUMENT, "one ground-truth pose and one flag per node");
    poses.insert(poses.end(), graphs[g].poses.begin(), graphs[g].poses.end());
    for (size_t k = 0; k < n; k++) { gt.push_back(none ? ident : truth[g].gt[k]); has.push_back(none ? 0 : truth[g].has_gt[k]); }
    off.push_back((int64_t)poses.size());
  }
}
}  // namespace graph_finish_detail
inline std::vector<cfear_graph_align_summary> AlignPoseGraphs(CFEAR_Radarodometry::Context& ctx, std::vector<PoseGraph>& graphs,
                                                              const std::vector<GraphTruth>& truth) {
  std::vector<cfear_pose3d> poses, gt;
  std::vector<uint8_t> has;
  std::vector<int64_t> off;
  graph_finish_detail::Flatten(graphs, truth, poses, gt, has, off);
  std::vector<cfear_graph_align_summary> out(graphs.size());
  ctx.check(cfear_graph_align_batch(ctx.get(), poses.data(), gt.data(), has.data(), off.data(), (int64_t)poses.size(), (int32_t)graphs.size(),
                                    out.data()));
  for (size_t g = 0; g < graphs.size(); g++) std::copy(poses.begin() + off[g], poses.begin() + off[g + 1], graphs[g].poses.begin());
  return out;
}
inline GraphMaps MapPoseGraphs(CFEAR_Radarodometry::Context& ctx, const std::vector<PoseGraph>& graphs, const std::vector<GraphTruth>& truth,
                               const std::vector<std::vector<std::vector<float>>>& clouds, int skip_frames = 1, bool want_gt_map = true) {
  std::vector<cfear_pose3d> poses, gt;
  std::vector<uint8_t> has;
  std::vector<int64_t> off, coff(1, 0);
  graph_finish_detail::Flatten(graphs, truth, poses, gt, has, off);
  if (clouds.size() != graphs.size()) throw CFEAR_Radarodometry::CfearError(CFEAR_ERR_INVALID_ARGUMENT, "one list of clouds per graph");
  std::vector<float> xyzi;
  for (size_t g = 0; g < graphs.size(); g++) {
    if (clouds[g].size() != graphs[g].poses.size()) throw CFEAR_Radarodometry::CfearError(CFEAR_ERR_INVALID_ARGUMENT, "one cloud per node");
    for (const std::vector<float>& c : clouds[g]) {
      if (c.size() % 4) throw CFEAR_Radarodometry::CfearError(CFEAR_ERR_INVALID_ARGUMENT, "a cloud holds 4 floats per point");
      xyzi.insert(xyzi.end(), c.begin(), c.end());
      coff.push_back((int64_t)(xyzi.size() / 4));
    }
  }
  GraphMaps out;
  out.ranges.resize(graphs.size());
  const cfear_graph_map_params par{skip_frames, want_gt_map ? 1 : 0};
  auto call = [&](float* m, int64_t cap, float* mg, int64_t cap_gt) {
    return cfear_graph_map_batch(ctx.get(), poses.data(), gt.data(), has.data(), off.data(), (int64_t)poses.size(), (int32_t)graphs.size(), xyzi.data(),
                                 coff.data(), (int64_t)(xyzi.size() / 4), &par, m, cap, mg, cap_gt, out.ranges.data());
  };
  const int rc = call(nullptr, 0, nullptr, 0);       // the sizes: CFEAR_ERR_CAPACITY with the ranges complete
  if (rc != CFEAR_ERR_CAPACITY) ctx.check(rc);
  int64_t n = 0, n_gt = 0;
  for (const cfear_graph_map_summary& s : out.ranges) { n += s.map_points; n_gt += s.map_gt_points; }
  out.map.resize((size_t)n * 4);
  out.map_gt.resize((size_t)n_gt * 4);
  ctx.check(call(out.map.data(), n, out.map_gt.data(), n_gt));
  return out;
}
inline void SaveGraphString(const std::string& path, const PoseGraph& graph, const std::vector<uint64_t>& stamps) {
  if (stamps.size() != graph.poses.size()) throw CFEAR_Radarodometry::CfearError(CFEAR_ERR_INVALID_ARGUMENT, "one stamp per node");
  const int rc = cfear_graph_string_write(path.c_str(), graph.poses.data(), stamps.data(), (int64_t)stamps.size());
  if (rc != CFEAR_OK) throw CFEAR_Radarodometry::CfearError(rc, path);
}
inline void OutputGraph(const std::string& est_path, const std::string& gt_path, const PoseGraph& graph, const GraphTruth& truth) {
  const size_t n = graph.poses.size();
  const bool none = truth.gt.empty() && truth.has_gt.empty();
  if (!none && (truth.gt.size() != n || truth.has_gt.size() != n))
    throw CFEAR_Radarodometry::CfearError(CFEAR_ERR_INVALID_ARGUMENT, "one ground-truth pose and one flag per node");
  const int rc = cfear_graph_output_write(est_path.c_str(), gt_path.c_str(), graph.poses.data(), none ? nullptr : truth.gt.data(),
                                          none ? nullptr : truth.has_gt.data(), (int64_t)n);
  if (rc != CFEAR_OK) throw CFEAR_Radarodometry::CfearError(rc, est_path + ", " + gt_path);
}
