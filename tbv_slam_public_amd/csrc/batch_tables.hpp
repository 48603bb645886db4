// batch_tables.hpp -- the host arithmetic of a ragged batch: the offsets [n + 1] that cut flat arrays into the batch's units,
// the flat grid that launches no empty workgroups for them, and the layout of the tables a call uploads.  Plain C++, no HIP
// include: tests/cpp/batch_tables_check.cpp binds it to a stand-alone program.  StagedTables (common.hpp) puts a TableLayout
// through a HostStage.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

// What is wrong with offsets [n + 1] that should run from 0 to total without descending.  A table can have several faults
// and the entry points do not blame the same one (tests/test_batch_tables_cpu.py pins who blames what), so the report keeps
// them apart and the caller chooses.
struct OffsetsReport {
  int64_t n = 0;
  bool start_not_0 = false, end_not_total = false;
  int64_t descends = 0;      // the first range whose end lies before its start; n: none
  int64_t leaves = 0;        // the first range whose end lies beyond total; n: none
  int64_t bad_range() const { return std::min(descends, leaves); }
  bool fine() const { return !start_not_0 && !end_not_total && bad_range() == n; }
  // the range to blame when the table is read front to back: the start belongs to the first range, the end to the last;
  // -1: a fault and no range to blame (n = 0), -2: fine
  int64_t first_fault() const {
    if (start_not_0) return n > 0 ? 0 : -1;
    if (bad_range() < n) return bad_range();
    if (end_not_total) return n - 1;
    return -2;
  }
};
inline OffsetsReport check_offsets(const int64_t* off, int64_t n, int64_t total) {
  OffsetsReport r;
  r.n = r.descends = r.leaves = n;
  r.start_not_0 = off[0] != 0;
  r.end_not_total = off[n] != total;
  for (int64_t k = n - 1; k >= 0; k--) {
    if (off[k + 1] < off[k]) r.descends = k;
    if (off[k + 1] > total) r.leaves = k;
  }
  return r;
}

// The flat grid of a ragged batch: one (unit, first item) entry per tile of `tile` items, so a unit of no items gets no
// workgroup.  Block is the kernels' int2 (or any pair of 32-bit integers).  Adds the tiles of one unit; false once the grid
// holds more workgroups than a launch takes (the caller words the refusal).
template <class Block>
bool flat_grid_add(std::vector<Block>& grid, int32_t unit, int64_t length, int32_t tile) {
  for (int64_t i = 0; i < length; i += tile) grid.push_back(Block{unit, (int32_t)i});
  return grid.size() <= (size_t)INT32_MAX;
}

// One device piece holds a call's record table, padded to 16 bytes, and its block table behind it; a second piece, which
// follows the first in the host record, holds what the host writes later (after the first wait of the call).
struct TableLayout {
  size_t record_bytes, block_bytes;
  size_t blocks_at;          // the block table's offset in the first piece
  size_t first, second;      // bytes of the two pieces
  TableLayout(size_t record_bytes_, size_t block_bytes_, size_t second_bytes)
      : record_bytes(record_bytes_), block_bytes(block_bytes_), blocks_at((record_bytes_ + 15) & ~(size_t)15),
        first(blocks_at + block_bytes_), second(second_bytes) {}
};
