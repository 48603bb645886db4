// When may a kernel read 16 bytes of an image row in one piece?  Plain C++ (no HIP header): the row kernels of kstrong.hip and
// cacfar.hip include it (through polar_common.hpp), and tests/cpp/row_pieces_check.cpp checks it on the CPU against every small image.
#pragma once

#if defined(__HIPCC__)
#define CFEAR_ROW_HD __host__ __device__
#else
#define CFEAR_ROW_HD
#endif

// The 16 bytes at byte `pos` of row `r` end inside the rows * stride bytes of their image -- all a caller promises to be
// readable (a batch promises batch_stride >= rows * stride per image, so the same bound holds for every image of it).
// A row that ends inside its last 16-byte piece may have that piece read whole exactly where this holds: not in an image's
// last row, and with stride < 16 not in the rows just before it either (cols = 4, stride = 4, rows = 3: only byte reads).
CFEAR_ROW_HD inline bool cfear_piece_inside_image(int r, int pos, int rows, int stride) {
  return (long long)r * stride + pos + 16 <= (long long)rows * stride;
}

// cacfar_rows_kernel reads the bytes [0, need_cols) of a row in 16- or 8-byte pieces (need_cols = the bins the arithmetic can
// reach, rounded up to 16: up to 15 bytes beyond a ragged row): whether row r's bytes may be read that way.  base_mod4 = the
// row's address modulo 4 (global_load_dwordx4 asks for a 4-byte boundary and no more).
CFEAR_ROW_HD inline bool cfear_cfar_row_direct(unsigned base_mod4, int r, int rows, int stride, int need_cols) {
  return base_mod4 == 0 && (stride & 3) == 0 && cfear_piece_inside_image(r, need_cols - 16, rows, stride);
}
