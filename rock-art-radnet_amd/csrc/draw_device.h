// What the painters share (draw.hip's draw_kernel in its three instantiations, heat.hip's heat_paint_kernel): the tile scheme, the
// normalised form of a rectangle and its coverage tests, a text run and its dot test, the font's staging, the pixel load, mix and
// store, and the entries' host prologue.  Integer arithmetic only; whatever can leave int32 comes in as 64 bits and is clamped here.
#pragma once
#include "draw_font.h"
#include "radnet_internal.h"

constexpr int kDrawTileW = 32, kDrawTileH = 8;      // one workgroup per tile, one pixel per thread
constexpr int kDrawBatch = RADNET_DRAW_RECT_BATCH;  // entries normalised into LDS at a time, one per thread
static_assert(kDrawTileW * kDrawTileH == kDrawBatch, "one thread per pixel of the tile and per entry of a batch");
static_assert(kDrawBatch % 64 == 0, "whole waves");
constexpr int kDrawFontBytes = kDrawFontGlyphs * kDrawFontRows;
static_assert(kDrawFontBytes % 4 == 0 && kDrawFontBytes / 4 <= kDrawBatch, "one word per thread stages the font");

struct DrawBox {      // in image pixels, clipped: paints [ox1, ox2] x [oy1, oy2] except the open box (ix1, ix2) x (iy1, iy2)
  int ox1, oy1, ox2, oy2, ix1, iy1, ix2, iy2;
  int bgr;            // b | g << 8 | r << 16 (the scene: tau in bits 24..31)
  int live;           // 0, or which kind of entry can touch this workgroup's tile
};
constexpr int kDrawRect = 1, kDrawText = 2, kDrawLineX = 3, kDrawLineY = 4, kDrawDisc = 5;      // DrawBox::live

struct DrawRun {      // a text run: where its dots start
  int x0, y0;         // the left end of the run and the top of its cap rows (exact whenever the run reaches the image)
  int scale, offset;  // pixels per dot; the run's first byte in the character pool
};

struct DrawTile {     // the tile's first and last column and row inside the image
  int x0, y0, x1, y1;
};

__device__ __forceinline__ int draw_clampi(long long v, int lo, int hi) { return (int)(v < lo ? lo : (v > hi ? hi : v)); }

__device__ __forceinline__ DrawTile draw_tile(int block, int tiles_x, int h, int w) {
  const int ty = block / tiles_x, tx = block - ty * tiles_x;
  DrawTile t;
  t.x0 = tx * kDrawTileW;
  t.y0 = ty * kDrawTileH;
  t.x1 = min(t.x0 + kDrawTileW, w) - 1;
  t.y1 = min(t.y0 + kDrawTileH, h) - 1;
  return t;
}

// The filled box [x1, x2] x [y1, y2] (x1 <= x2, y1 <= y2), clipped; nothing is left out.
__device__ __forceinline__ DrawBox draw_filled_box(long long x1, long long y1, long long x2, long long y2, int bgr, int h, int w) {
  DrawBox b;
  b.ox1 = draw_clampi(x1, 0, w);                 // a box wholly right of the image: ox1 = w > ox2
  b.ox2 = draw_clampi(x2, -1, w - 1);
  b.oy1 = draw_clampi(y1, 0, h);
  b.oy2 = draw_clampi(y2, -1, h - 1);
  b.ix1 = w;
  b.ix2 = -1;
  b.iy1 = h;
  b.iy2 = -1;
  b.bgr = bgr;
  b.live = 0;
  return b;
}

// radnet_draw_rects_u8's rectangle: corners in either order, thickness < 0 fills, thickness t > 0 is the outline of half width t / 2.
__device__ __forceinline__ DrawBox draw_rect_box(int cx1, int cy1, int cx2, int cy2, int thickness, int bgr, int h, int w) {
  const long long x1 = min(cx1, cx2), x2 = max(cx1, cx2), y1 = min(cy1, cy2), y2 = max(cy1, cy2);
  const long long hw = thickness > 0 ? thickness / 2 : 0;
  DrawBox b = draw_filled_box(x1 - hw, y1 - hw, x2 + hw, y2 + hw, bgr, h, w);
  if (thickness > 0) {                           // the open inner box, clamped to one pixel outside the image (same pixel set)
    b.ix1 = draw_clampi(x1 + hw, -1, w);
    b.ix2 = draw_clampi(x2 - hw, -1, w);
    b.iy1 = draw_clampi(y1 + hw, -1, h);
    b.iy2 = draw_clampi(y2 - hw, -1, h);
  }
  return b;
}

// Can the box paint a pixel of the tile: it overlaps the tile and the tile is not wholly inside what the outline leaves out.
__device__ __forceinline__ bool draw_box_touches(const DrawBox& b, const DrawTile& t) {
  const bool overlaps = b.ox1 <= t.x1 && b.ox2 >= t.x0 && b.oy1 <= t.y1 && b.oy2 >= t.y0;
  const bool swallowed = t.x0 > b.ix1 && t.x1 < b.ix2 && t.y0 > b.iy1 && t.y1 < b.iy2;
  return overlaps && !swallowed;
}

__device__ __forceinline__ bool draw_box_covers(const DrawBox& b, int x, int y) {
  const bool outer = x >= b.ox1 && x <= b.ox2 && y >= b.oy1 && y <= b.oy2;
  const bool inner = x > b.ix1 && x < b.ix2 && y > b.iy1 && y < b.iy2;
  return outer && !inner;
}

// A text entry: the clipped box of the whole run -- b characters of 6 dots less the last gap, 7 + 1 rows -- and where its dots start.
__device__ __forceinline__ DrawBox draw_text_box(const radnet_prim& p, int h, int w, DrawRun& run) {
  const long long s = p.x2, top = (long long)p.y1 - kDrawFontCapRows * s;
  const long long right = (long long)p.x1 + ((long long)kDrawFontAdvance * p.b - 1) * s - 1;      // b = 0: left of x1, empty
  run.x0 = p.x1;
  run.y0 = draw_clampi(top, -(kDrawFontRows * RADNET_DRAW_TEXT_MAX_SCALE), h);      // clamped only where the run is off the image
  run.scale = (int)s;
  run.offset = p.a;
  return draw_filled_box(p.x1, top, right, (long long)p.y1 + s - 1, p.bgr, h, w);
}

// Is the pixel, which lies inside the run's box, a set dot: there 0 <= x - x0 < 2^32 and 0 <= y - y0 < 8 * scale, so unsigned 32-bit
// arithmetic is exact.  `font` is the staged copy in LDS; a glyph index outside the font is not painted rather than read.
__device__ __forceinline__ bool draw_text_dot(const DrawRun& run, const uint8_t* __restrict__ chars, const uint8_t* font, int x, int y) {
  const unsigned s = (unsigned)run.scale;
  const unsigned dot = ((unsigned)x - (unsigned)run.x0) / s, row = (unsigned)(y - run.y0) / s;
  const unsigned ch = dot / kDrawFontAdvance, col = dot - ch * kDrawFontAdvance;
  const unsigned glyph = (unsigned)chars[(long long)run.offset + ch] - kDrawFontFirst;
  return col < kDrawFontCols && glyph < kDrawFontGlyphs && row < kDrawFontRows &&
         ((font[glyph * kDrawFontRows + row] >> (kDrawFontCols - 1 - col)) & 1);
}

// The font into kDrawFontBytes / 4 words of LDS, one word per thread; readable after the workgroup's next barrier.
__device__ __forceinline__ void draw_stage_font(uint32_t* font_words, int tid) {
  if (tid < kDrawFontBytes / 4) font_words[tid] = reinterpret_cast<const uint32_t*>(&kDrawFont[0][0])[tid];
}

__device__ __forceinline__ int draw_load_bgr(const uint8_t* img, long long pitch, int x, int y) {
  const uint8_t* px = img + (long long)y * pitch + (long long)x * 3;
  return px[0] | (px[1] << 8) | (px[2] << 16);
}

__device__ __forceinline__ void draw_store_bgr(uint8_t* img, long long pitch, int x, int y, int bgr) {
  uint8_t* px = img + (long long)y * pitch + (long long)x * 3;
  px[0] = (uint8_t)(bgr & 255);
  px[1] = (uint8_t)((bgr >> 8) & 255);
  px[2] = (uint8_t)((bgr >> 16) & 255);
}

__device__ __forceinline__ int draw_mix(int c, int d, unsigned tau) {      // per channel (c (255 - tau) + d tau + 127) / 255
  int out = 0;
  for (int k = 0; k < 24; k += 8) {
    const unsigned cc = ((unsigned)c >> k) & 255u, dd = ((unsigned)d >> k) & 255u;
    out |= (int)((cc * (255u - tau) + dd * tau + 127u) / 255u) << k;
  }
  return out;
}

// What every painter's entry does around its own checks, in this order: no context; a negative count (`rows` names what is counted);
// count == 0 is RADNET_OK before anything else is looked at; a null image or table or an empty image; a short pitch; the entry's own
// refusals, check() returning RADNET_OK or what it recorded with RADNET_FAIL; more than 2^31 - 1 tiles; launch(grid, tiles_x).
template <class Check, class Launch>
int draw_front(radnet_ctx* ctx, const char* front, const char* rows, const uint8_t* img, int32_t h, int32_t w, int64_t pitch_bytes, const void* table_host,
               const void* table_dev, int32_t count, Check check, Launch launch) {
  if (!ctx) return RADNET_ERR_ARG;
  if (count < 0) RADNET_FAIL(ctx, RADNET_ERR_ARG, "%s: %d %s", front, count, rows);
  if (count == 0) return RADNET_OK;
  if (!img || !table_host || !table_dev || h <= 0 || w <= 0)
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "%s: null image or table, or an empty image (image %p of %d x %d, host table %p, device table %p)", front,
                (const void*)img, h, w, table_host, table_dev);
  if (pitch_bytes < 3 * (int64_t)w) RADNET_FAIL(ctx, RADNET_ERR_ARG, "%s: a pitch of %lld bytes for rows of %d pixels", front, (long long)pitch_bytes, w);
  if (const int rc = check()) return rc;
  const long long tiles_x = ((long long)w + kDrawTileW - 1) / kDrawTileW, tiles_y = ((long long)h + kDrawTileH - 1) / kDrawTileH;
  if (tiles_x * tiles_y >= (1ll << 31)) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "%s: an image of %d x %d", front, h, w);
  launch(dim3((unsigned)(tiles_x * tiles_y)), (int)tiles_x);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) RADNET_FAIL(ctx, RADNET_ERR_HIP, "launch %s_u8: %s", front, hipGetErrorString(e));
  return RADNET_OK;
}
