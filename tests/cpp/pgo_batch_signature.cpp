// The batched pose-graph entry of include/cfear_hip.hpp (SolvePoseGraphs) compiled with the reference-side stand-ins: a
// syntax check of the header on a host without a GPU (tests/test_pgo_batch_cpu.py); tests/test_gpu_pgo_batch.py runs it
// and reads the line it prints: graphs, then per graph usable, residual blocks, iterations, final cost, last x.
#include <cstdio>

#include "cfear_hip.hpp"

int main() {
  try {
    std::vector<PoseGraph> graphs(2);
    for (size_t g = 0; g < graphs.size(); g++) {
      const int n = 4 + 2 * (int)g;
      for (int i = 0; i < n; i++) {
        const double xyt[3] = {1.02 * i, 0.01 * i * i, 0.0};
        cfear_pose3d p;
        cfear_pose3d_from_xyt(xyt, &p);
        graphs[g].poses.push_back(p);
        graphs[g].ids.push_back(10u * (uint64_t)i);
        if (i == 0) continue;
        cfear_graph_constraint c = {};
        const double step[3] = {1.0, 0.0, 0.0};
        c.id_begin = 10u * (uint64_t)(i - 1);
        c.id_end = 10u * (uint64_t)i;
        cfear_pose3d_from_xyt(step, &c.t_be);
        for (int k = 0; k < 6; k++) c.information[k * 7] = 1.0;
        c.type = 0;
        graphs[g].constraints.push_back(c);
      }
    }
    CFEAR_Radarodometry::Context ctx;
    int32_t failed = 0;
    const std::vector<cfear_pgo_summary> s = SolvePoseGraphs(ctx, graphs, nullptr, &failed);
    printf("%d %d", (int)s.size(), (int)failed);
    for (size_t g = 0; g < s.size(); g++)
      printf(" %d %d %d %.17g %.17g", (int)s[g].usable, (int)s[g].num_residual_blocks, (int)s[g].iterations, s[g].final_cost,
             graphs[g].poses.back().p[0]);
    printf("\n");
  } catch (const CFEAR_Radarodometry::CfearError& e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
