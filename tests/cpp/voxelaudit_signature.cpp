// The voxel-order audit of include/cfear_hip.hpp (VoxelOrderAudit) compiled with the reference-side stand-ins: a syntax and
// layout check on a host without a GPU (tests/test_voxelaudit_cpu.py).  It prints the sizes of the record and of a voxel row;
// without a device the context cannot be made and the program exits 2.  With one it audits, through the C ABI, two scans -- six
// points in one voxel with a seventh in the next one, and an empty scan -- and prints the records and the first voxel row.
#include <cstddef>
#include <cstdio>

#include "cfear_hip.hpp"

static_assert(sizeof(cfear_voxel_audit_params) == 16 && offsetof(cfear_voxel_audit_params, downsample_factor) == 8, "cfear_voxel_audit_params layout");
static_assert(sizeof(cfear_voxel_audit_record) == 48 && offsetof(cfear_voxel_audit_record, max_voxel_points) == 32 &&
                  offsetof(cfear_voxel_audit_record, max_halfwidth) == 40,
              "cfear_voxel_audit_record layout");
static_assert(sizeof(cfear_voxel_audit_voxel) == 56 && offsetof(cfear_voxel_audit_voxel, c_rev) == 16 && offsetof(cfear_voxel_audit_voxel, e) == 24 &&
                  offsetof(cfear_voxel_audit_voxel, n_sure_in) == 40,
              "cfear_voxel_audit_voxel layout");
static_assert(CFEAR_VOXEL_AUDIT_TILE % 256 == 0, "a tile is staged by whole workgroups");
static_assert((long long)CFEAR_VOXEL_AUDIT_MAX_POINTS * CFEAR_VOXEL_AUDIT_MAX_POINTS < 2147483648ll, "n_pairs_exposed fits an int32");

int main() {
  using namespace CFEAR_Radarodometry;
  printf("%d %d\n", (int)sizeof(cfear_voxel_audit_record), (int)sizeof(cfear_voxel_audit_voxel));
  try {
    Context ctx;
    std::vector<float> cloud;
    for (int i = 0; i < 6; i++) {
      const float p[4] = {0.5f + 0.25f * (float)i, 1.0f + 0.125f * (float)i, 0.f, 100.f};
      cloud.insert(cloud.end(), p, p + 4);
    }
    const float far[4] = {4.0f, 1.0f, 0.f, 100.f};
    cloud.insert(cloud.end(), far, far + 4);
    std::vector<cfear_voxel_audit_voxel> voxels;
    std::vector<int64_t> offsets;
    const std::vector<cfear_voxel_audit_record> rec = VoxelOrderAudit(ctx, {cloud, {}}, 3.0f, 1.0, &voxels, &offsets);
    printf("%d %d %d %d %d | %d %d | %u %d %.9g %.9g %d %d | %lld\n", (int)rec[0].status, (int)rec[0].n_points, (int)rec[0].n_voxels,
           (int)rec[0].max_voxel_points, (int)rec[0].n_centroids_reversed_differ, (int)rec[1].status, (int)rec[1].n_points, (unsigned)voxels[0].key,
           (int)voxels[0].n_points, (double)voxels[0].c_fwd[0], (double)voxels[0].c_fwd[1], (int)voxels[0].n_sure_in, (int)voxels[0].n_exposed,
           (long long)offsets.back());
  } catch (const CfearError& e) {
    fprintf(stderr, "%s\n", e.what());
    return 2;
  }
  return 0;
}
