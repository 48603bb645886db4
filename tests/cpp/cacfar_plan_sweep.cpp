// CPU sweep of cfear_cacfar_plan (include/cfear_hip.h) for tests/test_cacfar_plan_cpu.py: window 1..128 x guard 0..64 x every
// need_cols from 16 to 8192 in steps of 16 x false-alarm rate {0.01, 1.0} (1.0 gives scaling = 0: no decision table, so the
// pre-filter is off whatever the windows are) x {bitmap output, key output, fused decode}.  The row length is the lever for
// need_cols (max_distance lies beyond every bin, so the reachable bins are the whole row).
// Prints, for the Python test to read:
//   hit <route> <table_index> <count> <window> <guard> <need> <pfa1>     first parameter set that reached the entry
//   geom <route> <D> <DL> <nch> <pre_on> <count>                          every chunk geometry that was selected
//   calls <n>, violations <n> and, per violated invariant, its first case
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "cfear_hip.h"

namespace {
struct Hit { long long count = 0; int window = 0, guard = 0, need = 0, pfa1 = 0; };
struct Acc {
  Hit hit[3][33];                   // [route][table_index + 1]
  long long geom[3][5][5][10][2];   // [route][D / 2][DL / 2][nch][pre_on]
  long long calls = 0, violations = 0;
  std::string first[16];
  Acc() { std::memset(geom, 0, sizeof(geom)); }
};

void violate(Acc& a, int which, const char* what, int route, int w, int g, int need, int pfa1, const struct cfear_cacfar_plan& p) {
  a.violations++;
  if (!a.first[which].empty()) return;
  char buf[512];
  std::snprintf(buf, sizeof(buf), "violated %s: route %d window %d guard %d need %d pfa1 %d -> D %d DL %d nch %d pre %d need_cols %d colsp %d "
                "bins [%d, %d) index %d supported %d lds %lld", what, route, w, g, need, pfa1, p.D, p.DL, p.nch, p.pre_on, p.need_cols, p.colsp,
                p.bin_lo, p.bin_hi, p.table_index, p.cols_supported, (long long)p.lds_bytes);
  a.first[which] = buf;
}

void sweep(Acc& a, int w_lo, int w_hi) {
  for (int w = w_lo; w < w_hi; w++)
    for (int g = 0; g <= 64; g++)
      for (int need = 16; need <= 8192; need += 16)
        for (int pfa1 = 0; pfa1 < 2; pfa1++)
          for (int route = 0; route < 3; route++) {
            cfear_polar_desc d;
            if (route == 2) { d.rows = need; d.cols = 16; d.stride = 16; }      // [range bins][azimuths]
            else { d.rows = 5; d.cols = need; d.stride = need; }
            d.batch = 1; d.batch_stride = (int64_t)d.rows * d.stride;
            cfear_cacfar_params par;
            par.window_size = w; par.nb_guard_cells = g; par.false_alarm_rate = pfa1 ? 1.0f : 0.01f; par.range_res = 1.0f;
            par.z_min = 20.0f; par.min_distance = -1.0f; par.max_distance = 1.0e9;
            const int32_t flags = route == 2 ? CFEAR_ROWKEYS_BINS_MAJOR : (route == 1 ? CFEAR_CACFAR_PLAN_KEYS : 0);
            struct cfear_cacfar_plan p;
            a.calls++;
            if (cfear_cacfar_plan(&d, &par, flags, &p) != CFEAR_OK) { violate(a, 0, "status", route, w, g, need, pfa1, p); continue; }
            if (p.need_cols != need || p.bin_lo != 0 || p.bin_hi != need) violate(a, 1, "need_cols is the row", route, w, g, need, pfa1, p);
            if (p.colsp < p.need_cols) violate(a, 2, "colsp >= need_cols", route, w, g, need, pfa1, p);
            if (p.colsp != (p.nch - 1) * 256 * p.D + 256 * p.DL || p.DL > p.D || (p.DL != p.D && p.nch != 2))
              violate(a, 3, "colsp = the chunks", route, w, g, need, pfa1, p);
            if (pfa1 && (p.lut_ok || p.pre_on)) violate(a, 4, "no table, no pre-filter", route, w, g, need, pfa1, p);
            if (p.pre_on && !p.lut_ok) violate(a, 5, "pre_on implies lut_ok", route, w, g, need, pfa1, p);
            if (p.keys != (route != 0) || p.cols_route != (route == 2)) violate(a, 6, "route flags", route, w, g, need, pfa1, p);
            if (route != 2) {
              if (p.colsp > 8192) violate(a, 7, "rows route: colsp <= 8192", route, w, g, need, pfa1, p);
              if (p.table_index < 0 || p.table_index >= 20) violate(a, 8, "rows route: an entry for every selection", route, w, g, need, pfa1, p);
              if (p.wide != (p.D == 4 && p.nch > 4)) violate(a, 9, "wide", route, w, g, need, pfa1, p);
              if (p.cols_supported) violate(a, 10, "cols_supported only with the flag", route, w, g, need, pfa1, p);
              if (p.piece_rows != p.total_rows || p.total_rows != 5) violate(a, 11, "aligned whole rows are read in pieces", route, w, g, need, pfa1, p);
            } else {
              if (p.cols_supported && (p.colsp > 4096 || p.lds_bytes > 160 * 1024 - 256 || p.table_index < 0 || p.table_index >= 6))
                violate(a, 12, "cols_supported implies colsp <= 4096, the LDS bound and an entry", route, w, g, need, pfa1, p);
              if (!p.cols_supported && p.colsp <= 4096 && p.lds_bytes <= 160 * 1024 - 256)
                violate(a, 13, "an aligned geometry within both bounds is supported", route, w, g, need, pfa1, p);
            }
            if (p.table_index >= -1 && p.table_index < 32) {
              Hit& h = a.hit[route][p.table_index + 1];
              if (h.count++ == 0) { h.window = w; h.guard = g; h.need = need; h.pfa1 = pfa1; }
            }
            if (p.D >= 4 && p.D <= 8 && p.DL >= 2 && p.DL <= 8 && p.nch >= 1 && p.nch <= 9) a.geom[route][p.D / 2][p.DL / 2][p.nch][p.pre_on ? 1 : 0]++;
            else violate(a, 14, "D, DL, nch in range", route, w, g, need, pfa1, p);
          }
}
}  // namespace

int main() {
  const int n_threads = 8;
  std::vector<Acc> acc(n_threads);
  std::vector<std::thread> th;
  for (int t = 0; t < n_threads; t++) th.emplace_back([&acc, t]() { sweep(acc[t], 1 + 16 * t, 1 + 16 * (t + 1)); });
  for (auto& t : th) t.join();
  Acc& s = acc[0];                  // (threads take ascending windows: the first hit of the lowest thread is the first overall)
  for (int t = 1; t < n_threads; t++) {
    const Acc& o = acc[t];
    for (int r = 0; r < 3; r++)
      for (int i = 0; i < 33; i++) {
        if (s.hit[r][i].count == 0 && o.hit[r][i].count) { const long long c = o.hit[r][i].count; s.hit[r][i] = o.hit[r][i]; s.hit[r][i].count = c; }
        else s.hit[r][i].count += o.hit[r][i].count;
      }
    for (size_t i = 0; i < sizeof(s.geom) / sizeof(long long); i++) (&s.geom[0][0][0][0][0])[i] += (&o.geom[0][0][0][0][0])[i];
    s.calls += o.calls; s.violations += o.violations;
    for (int i = 0; i < 16; i++) if (s.first[i].empty()) s.first[i] = o.first[i];
  }
  for (int r = 0; r < 3; r++)
    for (int i = 0; i < 33; i++)
      if (s.hit[r][i].count) std::printf("hit %d %d %lld %d %d %d %d\n", r, i - 1, s.hit[r][i].count, s.hit[r][i].window, s.hit[r][i].guard, s.hit[r][i].need, s.hit[r][i].pfa1);
  for (int r = 0; r < 3; r++)
    for (int D = 4; D <= 8; D += 2)
      for (int DL = 2; DL <= 8; DL += 2)
        for (int n = 1; n <= 9; n++)
          for (int pre = 0; pre < 2; pre++)
            if (s.geom[r][D / 2][DL / 2][n][pre]) std::printf("geom %d %d %d %d %d %lld\n", r, D, DL, n, pre, s.geom[r][D / 2][DL / 2][n][pre]);
  std::printf("calls %lld\nviolations %lld\n", s.calls, s.violations);
  for (int i = 0; i < 16; i++) if (!s.first[i].empty()) std::printf("%s\n", s.first[i].c_str());
  return 0;
}
