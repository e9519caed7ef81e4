// ---- host side of the segmented PNG reconstruction (png.hip): one pass -> independent segments ---------------------------
// No device call and no HIP header: compiled by g++, runs without a GPU (contract: include/radnet_hip.h).
#include "radnet_hip.h"
#include "png_tile_rule.h"

namespace {

struct Column {
  const uint8_t* stream;
  int64_t pitch;
  int32_t rows, target;
  bool legal(int64_t r) const { return stream[r * pitch] <= 1; }      // None and Sub do not read the row above
  // the end (one past the last row) of the greedy segment that starts at row s
  int64_t end_of(int64_t s) const {
    const int64_t limit = s + target;
    if (limit >= rows) return rows;
    for (int64_t c = limit; c > s; --c)
      if (legal(c)) return c;
    for (int64_t c = limit + 1; c < rows; ++c)
      if (legal(c)) return c;
    return rows;
  }
};

// the filter-type byte of row r stands at stream[r * pitch]: pitch = 1 + rowbytes inside a scanline stream, 1 in a compact column
int plan(const uint8_t* stream, int64_t pitch, int64_t stream_offset, int32_t rows, int32_t rowbytes, int32_t target_rows, radnet_png_segment* out,
         int32_t cap) {
  if (!stream || !out || rows <= 0 || rowbytes <= 0 || cap <= 0 || stream_offset < 0 || target_rows < 0) return RADNET_ERR_ARG;
  const Column col{stream, pitch, rows, target_rows ? target_rows : RADNET_PNG_SEGMENT_TARGET_ROWS};
  const int64_t line = 1 + (int64_t)rowbytes;
  for (int64_t r = 0; r < rows; ++r)
    if (stream[r * col.pitch] > 4) return RADNET_ERR_ARG;
  int64_t n = 0;
  for (int64_t s = 0; s < rows; s = col.end_of(s)) ++n;
  // greedy segment i goes to out[i], or with more than cap of them to out[i * cap / n]: every entry gets one at least
  const bool merge = n > cap;
  int64_t i = 0, last = -1;
  for (int64_t s = 0; s < rows; ++i) {
    const int64_t e = col.end_of(s), slot = merge ? i * cap / n : i;
    if (slot != last) out[slot] = radnet_png_segment{stream_offset + s * line, 0, rowbytes};
    out[slot].rows += (int32_t)(e - s);
    last = slot;
    s = e;
  }
  return (int)(last + 1);
}

}  // namespace

extern "C" int radnet_png_plan_segments(const uint8_t* stream, int64_t stream_offset, int32_t rows, int32_t rowbytes, int32_t target_rows,
                                        radnet_png_segment* out, int32_t cap) {
  return plan(stream, 1 + (int64_t)rowbytes, stream_offset, rows, rowbytes, target_rows, out, cap);
}

extern "C" int radnet_png_plan_segments_column(const uint8_t* column, int64_t stream_offset, int32_t rows, int32_t rowbytes, int32_t target_rows,
                                               radnet_png_segment* out, int32_t cap) {
  return plan(column, 1, stream_offset, rows, rowbytes, target_rows, out, cap);
}

// ---- host side of the tiled reconstruction (png_tiles.hip): the plan of one segment, read off png_tile_rule.h --------------
namespace {

bool tile_args_ok(int32_t rows, int32_t rowbytes, int32_t bpp) {
  if (rows <= 0 || rowbytes <= 0 || rowbytes > (1 << 30)) return false;
  return (bpp == 1 || bpp == 2 || bpp == 3 || bpp == 4 || bpp == 6 || bpp == 8) && rowbytes % bpp == 0;
}

}  // namespace

extern "C" int radnet_png_plan_tiles(int32_t rows, int32_t rowbytes, int32_t bpp, radnet_png_tile_plan* out) {
  if (!out || !tile_args_ok(rows, rowbytes, bpp)) return RADNET_ERR_ARG;
  const png_tile_grid g = png_tile_grid_of(rows, rowbytes / bpp, RADNET_PNG_TILE_PIXELS);
  *out = radnet_png_tile_plan{g.bands, g.blocks, g.sweeps, RADNET_PNG_TILE_ROWS, RADNET_PNG_TILE_PIXELS};
  return RADNET_OK;
}

extern "C" int radnet_png_tiles_on_sweep(int32_t rows, int32_t rowbytes, int32_t bpp, int32_t sweep, int32_t* band_block_pairs, int32_t cap) {
  if (!tile_args_ok(rows, rowbytes, bpp) || cap < 0 || (cap > 0 && !band_block_pairs)) return RADNET_ERR_ARG;
  const png_tile_grid g = png_tile_grid_of(rows, rowbytes / bpp, RADNET_PNG_TILE_PIXELS);
  if (sweep < 0 || sweep >= g.sweeps) return RADNET_ERR_ARG;
  int32_t lo;
  const int32_t n = png_tiles_on_sweep(g, sweep, &lo);
  for (int32_t i = 0; i < n && i < cap; ++i) {
    band_block_pairs[2 * i] = lo + i;
    band_block_pairs[2 * i + 1] = sweep - 2 * (lo + i);
  }
  return n;
}
