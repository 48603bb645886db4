// The graph-finishing entries of include/cfear_hip.hpp (AlignPoseGraphs, MapPoseGraphs, SaveGraphString, OutputGraph) compiled
// with the reference-side stand-ins.  `write <dir>` needs no GPU: the two writers into <dir>.  `run <dir>` needs one
// (tests/test_gpu_graphfinish.py): two graphs aligned and mapped in one call each, then written; it prints the statuses, the
// ATE of the first graph, its alignment's determinant and the map sizes.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "cfear_hip.hpp"

static cfear_pose3d planar(double x, double y, double theta) {
  cfear_pose3d p;
  const double xyt[3] = {x, y, theta};
  cfear_pose3d_from_xyt(xyt, &p);
  return p;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const std::string dir = std::string(argv[2]) + "/";
  try {
    // graph 0: an L-shaped walk, the estimate turned by 0.3 rad and shifted; graph 1: three nodes on one line
    std::vector<PoseGraph> graphs(2);
    std::vector<GraphTruth> truth(2);
    const double c = std::cos(0.3), s = std::sin(0.3);
    for (int i = 0; i < 6; i++) {
      const double x = i < 3 ? 2.0 * i : 4.0, y = i < 3 ? 0.0 : 2.0 * (i - 2);
      truth[0].gt.push_back(planar(x, y, 0.1 * i));
      truth[0].has_gt.push_back(i != 4);
      graphs[0].poses.push_back(planar(c * x - s * y + 1.0, s * x + c * y - 2.0, 0.1 * i + 0.3));
      graphs[0].ids.push_back((uint64_t)i);
    }
    for (int i = 0; i < 3; i++) {
      truth[1].gt.push_back(planar(1.0 * i, 0.0, 0.0));
      truth[1].has_gt.push_back(1);
      graphs[1].poses.push_back(planar(1.0 * i, 0.5, 0.0));
      graphs[1].ids.push_back((uint64_t)i);
    }
    const std::vector<uint64_t> stamps = {10, 20, 30, 40, 50, 60};
    if (!strcmp(argv[1], "run")) {
      CFEAR_Radarodometry::Context& ctx = CFEAR_Radarodometry::Context::Default();
      const std::vector<cfear_graph_align_summary> a = AlignPoseGraphs(ctx, graphs, truth);
      const double* m = a[0].align;
      const double det = m[0] * (m[5] * m[10] - m[6] * m[9]) - m[1] * (m[4] * m[10] - m[6] * m[8]) + m[2] * (m[4] * m[9] - m[5] * m[8]);
      std::vector<std::vector<std::vector<float>>> clouds(2);
      for (int i = 0; i < 6; i++) clouds[0].push_back(std::vector<float>((size_t)4 * (i + 1), 1.0f));
      for (int i = 0; i < 3; i++) clouds[1].push_back(std::vector<float>(8, 2.0f));
      const GraphMaps maps = MapPoseGraphs(ctx, graphs, truth, clouds, 2, true);
      printf("%d %d %d %d %.17g %.17g %lld %lld %lld %lld\n", a[0].status, a[1].status, a[0].n_gt, a[1].n_gt, a[0].ate, det,
             (long long)maps.ranges[0].map_points, (long long)maps.ranges[0].map_gt_points, (long long)maps.ranges[1].map_offset,
             (long long)(maps.map_gt.size() / 4));
    }
    SaveGraphString(dir + "graph.txt", graphs[0], stamps);
    OutputGraph(dir + "est.txt", dir + "gt.txt", graphs[0], truth[0]);
    OutputGraph(dir + "est_only.txt", dir + "gt_empty.txt", graphs[1], GraphTruth());
  } catch (const CFEAR_Radarodometry::CfearError& e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
