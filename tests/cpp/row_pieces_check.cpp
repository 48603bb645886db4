// CPU check of tbv_slam_public_amd/csrc/row_pieces.hpp: where the row kernels read a 16-byte piece of an image row whole, the
// read ends inside the image.  Exhaustive over small images (rows 1..6, cols 1..40, stride cols..cols+20): every row, every
// 16-byte piece, through the conditions load_row (k-strongest) and cacfar_rows_kernel (CA-CFAR) apply.  The image is a heap
// block of exactly rows * stride bytes and every "whole" read is really made (memcpy of 16 bytes), so that a build with
// -fsanitize=address reports a read the arithmetic check would miss.
// Prints "<reads checked> <whole reads of partial pieces> <refused>" and returns 0, or the first failure and 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../tbv_slam_public_amd/csrc/row_pieces.hpp"

static long long g_sink = 0;

static bool read16(const uint8_t* img, long long size, long long at, const char* what, int rows, int cols, int stride, int r, int pos) {
  if (at < 0 || at + 16 > size) {
    std::printf("%s: rows %d cols %d stride %d row %d piece at %d reads [%lld, %lld) of %lld bytes\n", what, rows, cols, stride, r, pos,
                at, at + 16, size);
    return false;
  }
  uint8_t tmp[16];
  std::memcpy(tmp, img + at, 16);
  g_sink += tmp[0] + tmp[15];
  return true;
}

int main() {
  long long checked = 0, whole_partial = 0, refused = 0;
  for (int rows = 1; rows <= 6; rows++)
    for (int cols = 1; cols <= 40; cols++)
      for (int stride = cols; stride <= cols + 20; stride++) {
        const long long size = (long long)rows * stride;
        uint8_t* img = (uint8_t*)std::malloc((size_t)size);
        if (!img) return 2;
        std::memset(img, 7, (size_t)size);
        for (int r = 0; r < rows; r++) {
          // load_row: the piece at pos is read whole when it lies inside the row, or -- the row's last, partial piece --
          // when tail_safe says so (kstrong_row hands over cfear_piece_inside_image of that piece)
          const bool tail_safe = cfear_piece_inside_image(r, cols & ~15, rows, stride);
          for (int pos = 0; pos < cols; pos += 16) {
            const bool whole = pos + 16 <= cols || tail_safe;
            const bool inside = (long long)r * stride + pos + 16 <= size;
            checked++;
            if (whole && !read16(img, size, (long long)r * stride + pos, "load_row", rows, cols, stride, r, pos)) return 1;
            if (pos + 16 > cols) {
              whole_partial += whole;
              refused += !whole;
              if (whole != inside) {      // exact, not merely safe: a piece that ends inside the image is not sent down the byte path
                std::printf("load_row: rows %d cols %d stride %d row %d: whole %d but inside %d\n", rows, cols, stride, r, whole, inside);
                return 1;
              }
              if (stride >= 16 && r + 1 < rows && !whole) {      // the rule before the exact one, where it was right
                std::printf("load_row: rows %d cols %d stride %d row %d lost its whole read\n", rows, cols, stride, r);
                return 1;
              }
            }
          }
          // cacfar_rows_kernel: a direct row is read in pieces up to need_cols, any multiple of 16 up to the row length rounded up
          for (int need = 16; need <= ((cols + 15) & ~15); need += 16)
            for (unsigned mis = 0; mis < 4; mis++) {
              const bool direct = cfear_cfar_row_direct(mis, r, rows, stride, need);
              if (direct && (mis != 0 || stride % 4 != 0)) {
                std::printf("cacfar: rows %d cols %d stride %d row %d: pieces from a row that is not on a 4-byte boundary\n", rows, cols, stride, r);
                return 1;
              }
              const bool inside = (long long)r * stride + need <= size;
              if (mis == 0 && stride % 4 == 0 && direct != inside) {
                std::printf("cacfar: rows %d cols %d stride %d row %d need %d: direct %d but inside %d\n", rows, cols, stride, r, need, direct, inside);
                return 1;
              }
              if (direct)
                for (int pos = 0; pos < need; pos += 16) {
                  checked++;
                  if (!read16(img, size, (long long)r * stride + pos, "cacfar", rows, cols, stride, r, pos)) return 1;
                }
            }
        }
        std::free(img);
      }
  // the case of the finding: cols = 4, stride = 4, rows = 3 -- no row may be read whole
  for (int r = 0; r < 3; r++)
    if (cfear_piece_inside_image(r, 0, 3, 4) || cfear_cfar_row_direct(0u, r, 3, 4, 16)) { std::printf("4 x 3, stride 4: row %d read whole\n", r); return 1; }
  std::printf("%lld %lld %lld %lld\n", checked, whole_partial, refused, g_sink & 1);
  return 0;
}
