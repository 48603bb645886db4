// reg_layout.hpp -- what a registration needs from a launch of the matcher (matcher.hip): the job record's stride, the LDS
// map of a workgroup, the scratch of a job, and what the host learns about a batch while it marshals it.  Plain C++, no HIP
// include: shared by matcher_kernel (mt_carve), the host entry points (register.hip, verify.hip, tieaudit.hip) and a
// stand-alone program (tests/cpp/registration_check.cpp), which also holds tests/verify_cases.py's restatement to it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/cfear_hip.h"

#if defined(__HIPCC__)
#define REG_LAYOUT_FN __host__ __device__ inline
#else
#define REG_LAYOUT_FN inline
#endif

// ---- the search grid of a scan (ScanView::grid, common.hpp) ---------------------------------------------------------
constexpr int kScanGrid = 32;                                  // grid cells per axis
constexpr int kScanGridCells = kScanGrid * kScanGrid;
constexpr int kScanGridStartPad = kScanGridCells + 8;          // u16 entries per scan: a multiple of 16 bytes
REG_LAYOUT_FN int scan_grid_pad(int n) { return (n + 7) & ~7; }        // records per scan, padded: both record arrays are runs of 16-byte pieces

// ---- the job record (struct RegJob, registration.hpp) ----------------------------------------------------------------
// The scan views come LAST so that a batch whose jobs use at most m scans can be stored with the shorter stride
// reg_job_stride(m): a two-scan loop-closure candidate is 0.5 KB instead of 1.9 KB to build and upload.
constexpr int kRegMaxScans = 16;
constexpr size_t kRegJobHeadBytes = 8 + (size_t)kRegMaxScans * 24;   // n_scans, itr, poses: offsetof(RegJob, scans)
constexpr size_t kRegViewBytes = 96;                                 // sizeof(ScanView)
inline size_t reg_record_stride(size_t head_bytes, int max_scans) { return (head_bytes + (size_t)max_scans * kRegViewBytes + 15) & ~(size_t)15; }
inline size_t reg_job_stride(int max_scans) { return reg_record_stride(kRegJobHeadBytes, max_scans); }

inline int reg_dense_fields(int cost) { return cost == CFEAR_P2P ? 3 : (cost == CFEAR_P2L ? 5 : 6); }

// Global scratch of one workgroup: the u16 match table of the large forms, then the tail of the dense arrays.
REG_LAYOUT_FN size_t match_bytes_global(int pairs_cap) { return ((size_t)pairs_cap * 2 + 255) / 256 * 256; }
// Slot arrays in the job's global scratch (cost object / cost-only mode): 52 bytes per slot.
REG_LAYOUT_FN size_t slots_bytes(int cap) { return ((size_t)cap * 52 + 255) / 256 * 256; }
inline size_t reg_scratch_bytes(int pairs_cap) { return match_bytes_global(pairs_cap) + slots_bytes(pairs_cap); }

// ---------------------------------------------------------------------------------------------------
// LDS map of a registration workgroup.  Fixed block: the reduction's partials, the scan's int partials, the solver state.
// Behind it (mt_carve): keyframe transforms and pointers, the source means, the match table, then the REGION that holds the
// keyframes' tables and the dense correspondence arrays -- side by side when both fit, aliased when they do not.
// ---------------------------------------------------------------------------------------------------
constexpr int kRegStateDoubles = 48;                         // the LDS-resident solver state (matcher.hip: S_COUNT)
constexpr int kMaxNW = 16;
constexpr size_t kPartOff = 0;                               // [10][16] doubles: the block reduction's partials (one buffer: two
constexpr size_t kIpartOff = kMaxNW * 10 * 8;                //   barriers separate consecutive uses); [2][16] ints
constexpr size_t kStateOff = kIpartOff + 2 * kMaxNW * 4;
constexpr size_t kFixedLds = kStateOff + kRegStateDoubles * 8;   // 1792 bytes
constexpr int kPtrs = 6;                                     // per keyframe: mean, normal, nsamples, scale, cov, grid block
constexpr size_t kPartBigBytes = 10 * 4 * kMaxNW * 8;        // the partials of the 8- / 16-wavefront forms: at the END of their LDS

constexpr size_t kLdsCu = 160 * 1024;                        // LDS of a gfx950 compute unit
constexpr size_t kLdsPairs = 20 * 1024;                      // the 2-wavefront form for two-scan candidates: eight per CU
inline size_t regular_lds(bool huber) { return huber ? kLdsCu / 4 : (kLdsCu / 3) & ~(size_t)255; }   // four (three: matcher_kernel) per CU

// What a registration of these sizes gets from `lds_total` bytes: shared by the kernel (mt_carve) and the host (which form
// and how much LDS a batch wants).  sum_pad / max_pad: the keyframes' padded record counts (scan_grid_pad).
struct MtFit {
  size_t off_smean, off_match, off_region;
  int region;              // bytes of the region
  int tables_all;          // bytes of every keyframe's tables together
  int dense_cap;           // correspondences the LDS arrays hold
  bool gmatch;             // the match table lives in global scratch
  bool resident;           // tables and dense arrays side by side: staged once per registration
  bool can;                // the registration can run at all in this LDS
  bool good;               // ... and is one this LDS is GOOD for: tables in at most two groups, LDS arrays for 40 % of the pairs
};
REG_LAYOUT_FN MtFit mt_fit(size_t lds_total, int last, int sum_pad, int max_pad, int n_src, int fields, bool allow_gmatch) {
  MtFit m;
  size_t off = kFixedLds + (size_t)last * (12 * 8 + kPtrs * 8 + 16) + ((((size_t)last + 1) * 4 + 15) & ~(size_t)15);
  m.off_smean = off; off += (size_t)n_src * 16;
  const size_t n_pairs = (size_t)last * n_src;
  const size_t match_bytes = ((n_pairs + 7) & ~(size_t)7) * 2;
  const size_t need_one = (size_t)kScanGridStartPad * 2 + (size_t)max_pad * 10;
  m.off_match = off;
  // the match table: in LDS, unless that leaves no room for the largest keyframe's tables (1 400-cell scans in half a CU's
  // LDS) -- then in the job's global scratch (L2; written and read once per outer iteration by the same thread)
  m.gmatch = allow_gmatch && ((off + match_bytes + 15) & ~(size_t)15) + need_one > lds_total;
  if (!m.gmatch) off += match_bytes;
  off = (off + 15) & ~(size_t)15;
  m.off_region = off;
  m.tables_all = (int)((size_t)last * kScanGridStartPad * 2 + (size_t)sum_pad * 10);
  const size_t per = (size_t)fields * 8 + 2;
  m.can = sum_pad <= 65535 && n_src < 65536 && off + need_one <= lds_total && off + 4096 <= lds_total;
  m.region = m.can ? (int)(lds_total - off) : 0;
  const size_t dense_all = ((n_pairs + 3) & ~(size_t)3) * per;
  m.resident = m.can && (size_t)m.tables_all + dense_all + 16 <= (size_t)m.region;
  if (m.resident) m.dense_cap = (int)((n_pairs + 3) & ~(size_t)3);
  else m.dense_cap = (int)((size_t)m.region / per) & ~3;
  m.good = m.can && (m.resident || (m.tables_all <= 2 * m.region && 5 * (size_t)m.dense_cap >= 2 * n_pairs));
  return m;
}

// What the caller knows about the batch's registrations (the kernel decides per registration from the device-side sizes)
struct RegLaunchHint {
  bool small_pairs = false;   // every job is a two-scan candidate that fits 20 KB of LDS: the 2-wavefront form, eight per CU
  bool big_pass = false;      // registrations the regular form is not good at may be among them (dense scans): add the large forms
  bool whole_cu = false;      // cost-only launches: a job that does not fit half a CU's LDS is among them
};

// what the host learns about a batch while it marshals it: the scratch size and which forms its registrations want
struct JobSizes {
  int pairs_cap = 1, cost;
  bool huber, small_pairs = true, any_large = false, any_huge = false;
  explicit JobSizes(const cfear_reg_params* par) : cost(par->cost), huber(par->loss == CFEAR_LOSS_HUBER) {}
  JobSizes& add(int n_scans, int sum_pad, int max_pad, int n_src) {
    const int last = n_scans - 1, fields = reg_dense_fields(cost);
    pairs_cap = std::max(pairs_cap, last * std::max(n_src, 1));
    any_huge = any_huge || !mt_fit((uint32_t)(kLdsCu / 2 - 256 - kPartBigBytes), last, sum_pad, max_pad, n_src, fields, true).can;
    small_pairs = small_pairs && n_scans == 2 && mt_fit(kLdsPairs, last, sum_pad, max_pad, n_src, fields, false).good;
    any_large = any_large || !mt_fit(regular_lds(huber), last, sum_pad, max_pad, n_src, fields, false).good;
    return *this;
  }
  RegLaunchHint hint(int n_jobs) const { RegLaunchHint h; h.small_pairs = small_pairs && n_jobs > 0; h.big_pass = any_large; h.whole_cu = any_huge; return h; }
};

// launch geometry of a batch of two-scan jobs from its largest target / source (what cfear_register_candidates derives)
inline void cfear_reg_pair_geometry(const cfear_reg_params* par, int max_tar_cells, int max_src_cells, int* pairs_cap, RegLaunchHint* hint) {
  const JobSizes sz = JobSizes(par).add(2, scan_grid_pad(max_tar_cells), scan_grid_pad(max_tar_cells), max_src_cells);
  *pairs_cap = sz.pairs_cap; *hint = sz.hint(1);
}
// Whether a cost-only launch (cfear_get_cost_batch) can hold a registration of these sizes at all: the capacity of its last
// resort -- 8 wavefronts, a CU's whole LDS, the match table in global scratch (cfear_register_launch, hint.whole_cu).  What
// it cannot hold is the job's CFEAR_ERR_CAPACITY (the sizes the kernel would answer with write_capacity).
inline bool cfear_reg_cost_fits(const cfear_reg_params* par, int n_scans, int sum_pad, int max_pad, int n_src) {
  return mt_fit(kLdsCu - 256 - kPartBigBytes, n_scans - 1, sum_pad, max_pad, n_src, reg_dense_fields(par->cost), true).can;
}
