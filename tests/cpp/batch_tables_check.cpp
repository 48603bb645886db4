// CPU check of tbv_slam_public_amd/csrc/batch_tables.hpp (no HIP runtime): the offsets report on the malformed tables of
// tests/test_batch_tables_cpu.py, the flat grid at the tile's edges, and the 16-byte padding of a record table.  The tables
// are heap blocks of exactly n + 1 entries, so a build with -fsanitize=address,undefined reports a read past a table.
// Prints "ok" and returns 0, or the failures and 1.
#include <cstdio>
#include <vector>

#include "../../tbv_slam_public_amd/csrc/batch_tables.hpp"

static int g_bad = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); g_bad++; } \
  } while (0)

struct Block { int32_t unit, first; };              // the kernels' int2
struct EvalTraj { int64_t src, off; int32_t n, starts; };   // evaluate.hip's 24-byte record

// what check_offsets must say about a table: start, end, first descent, first range that leaves, who is blamed front to back
static void table(std::vector<int64_t> off, int64_t total, bool start, bool end, int64_t descends, int64_t leaves, int64_t first_fault) {
  const int64_t n = (int64_t)off.size() - 1;
  const OffsetsReport r = check_offsets(off.data(), n, total);
  CHECK(r.n == n && r.start_not_0 == start && r.end_not_total == end && r.descends == descends && r.leaves == leaves);
  CHECK(r.bad_range() == (descends < leaves ? descends : leaves));
  CHECK(r.first_fault() == first_fault);
  CHECK(r.fine() == (first_fault == -2));
}

int main() {
  const int64_t big = (int64_t)1 << 31;
  table({0, 3, 5, 8}, 8, false, false, 3, 3, -2);
  table({0, 0, 8, 8}, 8, false, false, 3, 3, -2);
  table({1, 3, 5, 8}, 8, true, false, 3, 3, 0);
  table({0, 3, 5, 7}, 8, false, true, 3, 3, 2);
  table({0, 3, 5, 9}, 8, false, true, 3, 2, 2);
  table({0, 5, 3, 8}, 8, false, false, 1, 3, 1);
  table({0, 3, 9, 8}, 8, false, false, 2, 1, 1);
  table({0, 9, 8, 8}, 8, false, false, 1, 0, 0);
  table({0, 5, 3, 7}, 8, false, true, 1, 3, 1);    // closure blames range 2 for this one: it looks at end_not_total first
  table({2, 1, 5, 8}, 8, true, false, 0, 3, 0);
  table({2}, 0, true, true, 0, 0, -1);
  table({2}, 2, true, false, 0, 0, -1);
  table({0}, 0, false, false, 0, 0, -2);
  table({0}, 4, false, true, 0, 0, -1);
  table({0, 2, 2 + big, 3 + big}, 3 + big, false, false, 3, 3, -2);

  // the flat grid, tile 256: a unit of no items gets no workgroup, 256 items one, 257 two
  const int64_t lengths[] = {0, 1, 255, 256, 257};
  const int expect[] = {0, 1, 1, 1, 2};
  std::vector<Block> grid;
  for (int u = 0; u < 5; u++) {
    const size_t before = grid.size();
    CHECK(flat_grid_add(grid, u, lengths[u], 256));
    CHECK(grid.size() - before == (size_t)expect[u]);
    for (size_t b = before; b < grid.size(); b++) CHECK(grid[b].unit == u && grid[b].first == (int32_t)(256 * (b - before)));
  }
  CHECK(grid.size() == 5 && grid[4].unit == 4 && grid[4].first == 256);
  CHECK(sizeof(Block) == 8);

  // three 24-byte records are 72 bytes and pad to 80; the block table follows, the second piece follows the first
  static_assert(sizeof(EvalTraj) == 24, "evaluate.hip's record");
  const TableLayout lay(3 * sizeof(EvalTraj), grid.size() * sizeof(Block), 3 * 112);
  CHECK(lay.blocks_at == 80 && lay.first == 80 + 40 && lay.second == 336 && lay.record_bytes == 72 && lay.block_bytes == 40);
  const TableLayout even(4 * 32, 0, 0);
  CHECK(even.blocks_at == 128 && even.first == 128 && even.second == 0);
  const TableLayout none(0, 0, 32);
  CHECK(none.blocks_at == 0 && none.first == 0 && none.second == 32);

  if (g_bad) return 1;
  std::printf("ok\n");
  return 0;
}
