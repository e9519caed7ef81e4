// What the two painters of draw.hip share (draw_rects_kernel and draw_list_kernel): the tile scheme, the normalised form of a
// rectangle and its coverage tests.  Integer arithmetic only; whatever can leave int32 comes in as 64 bits and is clamped here.
#pragma once
#include "radnet_internal.h"

constexpr int kDrawTileW = 32, kDrawTileH = 8;      // one workgroup per tile, one pixel per thread
constexpr int kDrawBatch = RADNET_DRAW_RECT_BATCH;  // entries normalised into LDS at a time, one per thread
static_assert(kDrawTileW * kDrawTileH == kDrawBatch, "one thread per pixel of the tile and per entry of a batch");
static_assert(kDrawBatch % 64 == 0, "whole waves");

struct DrawBox {      // in image pixels, clipped: paints [ox1, ox2] x [oy1, oy2] except the open box (ix1, ix2) x (iy1, iy2)
  int ox1, oy1, ox2, oy2, ix1, iy1, ix2, iy2;
  int bgr;            // b | g << 8 | r << 16
  int live;           // can touch this workgroup's tile (draw_list_kernel: and which kind of entry it is)
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

__device__ __forceinline__ void draw_store_bgr(uint8_t* img, long long pitch, int x, int y, int bgr) {
  uint8_t* px = img + (long long)y * pitch + (long long)x * 3;
  px[0] = (uint8_t)(bgr & 255);
  px[1] = (uint8_t)((bgr >> 8) & 255);
  px[2] = (uint8_t)((bgr >> 16) & 255);
}
