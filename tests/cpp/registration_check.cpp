// CPU check of tbv_slam_public_amd/csrc/reg_layout.hpp and pose2d.hpp (no HIP runtime), driven by
// tests/test_reg_layout_cpu.py.
//   registration_check         the invariants of the matcher's LDS map, job stride and scratch, and the pose algebra's
//                              identities; prints "ok" and returns 0, or the failures and 1
//   registration_check hint    for every line "max_cells cost huber" of the standard input, the (can, good) of mt_fit for
//                              a two-scan job of that size in the four LDS sizes the launch hint and the cost-only capacity
//                              test ask about, then small_pairs, big_pass, whole_cu of JobSizes(par).add(2, pad, pad, n).hint(1):
//                              eleven 0 / 1 per line, which the pytest holds against tests/verify_cases.py's restatement
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>

#include "../../tbv_slam_public_amd/csrc/pose2d.hpp"
#include "../../tbv_slam_public_amd/csrc/reg_layout.hpp"

static int g_bad = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) { if (g_bad < 20) std::printf("line %d: %s\n", __LINE__, #cond); g_bad++; } \
  } while (0)

static void fit_checks(size_t lds, int last, int sum_pad, int max_pad, int n_src, int fields, bool allow_gmatch) {
  const MtFit m = mt_fit(lds, last, sum_pad, max_pad, n_src, fields, allow_gmatch);
  if (m.can) {
    CHECK(m.off_region % 16 == 0);
    CHECK(m.off_region + (size_t)m.region == lds);
    CHECK(m.off_smean + 16 * (size_t)n_src <= m.off_match);
    CHECK(m.dense_cap % 4 == 0);
  }
  if (m.resident) CHECK((size_t)m.tables_all + (size_t)m.dense_cap * (8 * (size_t)fields + 2) + 16 <= (size_t)m.region);
  if (m.good) CHECK(m.can);
}

static void layout_checks() {
  const size_t lds[] = {kLdsPairs, regular_lds(true), regular_lds(false), kLdsCu / 2 - 256, kLdsCu - 256,
                        kLdsCu / 2 - 256 - kPartBigBytes, kLdsCu - 256 - kPartBigBytes};
  const int lasts[] = {1, 2, 15}, fields[] = {3, 5, 6};
  auto at = [&](int n_src, int cells) {        // every keyframe as large as the largest, or the others empty
    const int pad = scan_grid_pad(cells);
    CHECK(pad % 8 == 0 && pad >= cells && pad < cells + 8);
    for (size_t l : lds) for (int last : lasts) for (int f : fields) for (int g = 0; g < 2; g++) {
      fit_checks(l, last, last * pad, pad, n_src, f, g != 0);
      fit_checks(l, last, pad, pad, n_src, f, g != 0);
    }
  };
  for (int c = 0; c <= 3200; c++) at(c, c);                                      // the sizes the pair geometry asks about
  for (int n = 0; n <= 3200; n += 97) for (int c = 0; c <= 3200; c += 97) at(n, c);
  at(3200, 0); at(0, 3200); at(3200, 3200);

  const size_t full = kRegJobHeadBytes + (size_t)kRegMaxScans * kRegViewBytes;
  for (int m = 0; m <= kRegMaxScans; m++) {
    CHECK(reg_job_stride(m) % 16 == 0 && reg_job_stride(m) <= full + 15);
    CHECK(reg_job_stride(m) >= kRegJobHeadBytes + (size_t)m * kRegViewBytes);
  }
  CHECK(reg_job_stride(kRegMaxScans) >= full);
  for (int p = 0; p <= 3200 * 15; p += 7) CHECK(reg_scratch_bytes(p) % 256 == 0 && reg_scratch_bytes(p) >= (size_t)p * 54);
  CHECK(kFixedLds == 1792);
}

static double wrap(double a) { return std::atan2(std::sin(a), std::cos(a)); }

static void pose_checks() {
  std::mt19937_64 rng(20181);
  std::uniform_real_distribution<double> xy(-1e4, 1e4), th(-M_PI, M_PI);
  double p[48][3] = {{0, 0, 0}, {1e4, -1e4, M_PI}, {-1e4, 1e4, -M_PI}, {3.5, -2.25, M_PI / 2}};
  for (int i = 4; i < 48; i++) { p[i][0] = xy(rng); p[i][1] = xy(rng); p[i][2] = th(rng); }
  const Aff2 I = aff_identity();
  CHECK(I.l0 == 1 && I.l1 == 0 && I.l2 == 0 && I.l3 == 1 && I.t0 == 0 && I.t1 == 0);
  for (int i = 0; i < 48; i++) {
    const Aff2 A = aff_from_xyt(p[i]);
    const Aff2 C = aff_from_cs(std::cos(p[i][2]), std::sin(p[i][2]), p[i][0], p[i][1]);
    CHECK(std::memcmp(&A, &C, sizeof(Aff2)) == 0);
    const Aff2 E = aff_mul(aff_inv(A), A);
    CHECK(std::fabs(E.l0 - 1) <= 1e-12 && std::fabs(E.l1) <= 1e-12 && std::fabs(E.l2) <= 1e-12 && std::fabs(E.l3 - 1) <= 1e-12);
    CHECK(std::fabs(E.t0) <= 1e-12 && std::fabs(E.t1) <= 1e-12);
    double inv[3], z[3];
    xyt_inverse(p[i], inv);
    xyt_compose(inv, p[i], z);
    CHECK(std::fabs(z[0]) <= 1e-9 && std::fabs(z[1]) <= 1e-9 && std::fabs(wrap(z[2])) <= 1e-12);
    const int j = (i * 7 + 3) % 48;
    double ab[3], viaaff[3];
    xyt_compose(p[i], p[j], ab);
    aff_to_xyt(aff_mul(A, aff_from_xyt(p[j])), viaaff);
    CHECK(std::fabs(ab[0] - viaaff[0]) <= 1e-9 && std::fabs(ab[1] - viaaff[1]) <= 1e-9);
    CHECK(std::fabs(wrap(ab[2] - viaaff[2])) <= 1e-12);
  }
}

static int hint_lines() {
  char cost[8];
  int cells, huber;
  while (std::scanf("%d %7s %d", &cells, cost, &huber) == 3) {
    cfear_reg_params par;
    std::memset(&par, 0, sizeof(par));
    par.cost = !std::strcmp(cost, "P2P") ? CFEAR_P2P : (!std::strcmp(cost, "P2L") ? CFEAR_P2L : CFEAR_P2D);
    par.loss = huber ? CFEAR_LOSS_HUBER : 0;
    const int pad = scan_grid_pad(cells), f = reg_dense_fields(par.cost);
    const MtFit m[4] = {mt_fit(kLdsPairs, 1, pad, pad, cells, f, false), mt_fit(regular_lds(huber != 0), 1, pad, pad, cells, f, false),
                        mt_fit(kLdsCu / 2 - 256 - kPartBigBytes, 1, pad, pad, cells, f, true),
                        mt_fit(kLdsCu - 256 - kPartBigBytes, 1, pad, pad, cells, f, true)};
    const RegLaunchHint h = JobSizes(&par).add(2, pad, pad, cells).hint(1);
    for (const MtFit& x : m) std::printf("%d %d ", (int)x.can, (int)x.good);
    std::printf("%d %d %d\n", (int)h.small_pairs, (int)h.big_pass, (int)h.whole_cu);
    // the two functions the callers use say the same
    int pairs_cap = 0;
    RegLaunchHint g;
    cfear_reg_pair_geometry(&par, cells, cells, &pairs_cap, &g);
    if (g.small_pairs != h.small_pairs || g.big_pass != h.big_pass || g.whole_cu != h.whole_cu || pairs_cap != (cells > 1 ? cells : 1)) return 1;
    if (cfear_reg_cost_fits(&par, 2, pad, pad, cells) != m[3].can) return 1;
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "hint")) return hint_lines();
  layout_checks();
  pose_checks();
  if (g_bad) return 1;
  std::printf("ok\n");
  return 0;
}
