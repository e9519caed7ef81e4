// Score maps as pictures: radnet_score_levels_u8, fp32 scores to one uint8 level per feature-map cell, and radnet_heat_paint_u8, maps
// of such levels painted through a colour table into a uint8 [H][W][3] device image in place.  The contracts stand in
// include/radnet_hip.h; the placement table is validated on the host by heat_check.cpp.  Compiled with -ffp-contract=off like the
// other exact units: the level rule rounds its product and its sum separately; the painter has no floating point at all.
//
// heat_paint_kernel keeps the scheme of draw.hip's draw_kernel and shares its helpers and its host prologue (draw_device.h): one workgroup
// per tile of kDrawTileW x kDrawTileH pixels, one pixel per thread, the table streamed through LDS in batches of RADNET_DRAW_RECT_BATCH
// entries, thread j marking whether entry j of the batch can touch the tile (uniform over the workgroup, so the walk does not diverge on
// it).  It is a kernel of its own because what a pixel keeps while it walks the table is not a value in table order but the MAXIMUM
// level of the placements that hold it, which no order of the table changes, and because of its epilogue: after the last batch a pixel
// that was held and whose level reaches min_level looks its colour up in the table in LDS, loads its three bytes if the mix needs them,
// and stores once; no atomics, one writer.
//
// The cell of a pixel: (X - x0) < w <= 2^20 and mw <= 2047 < 2^11, so (X - x0) * mw < 2^31 in unsigned arithmetic, and the operands
// are never negative inside the rectangle, so unsigned division is floor division.  x0 + w stays inside int32 (|x0| <= 2^24).
#include "draw_device.h"

namespace {

struct HeatEntry {
  int x0, y0, w, h, mw, mh;
  long long offset;
  int live;               // can touch this workgroup's tile
};

__global__ void __launch_bounds__(256) score_levels_kernel(const float* __restrict__ pred, int ld, int M, int first, int count, uint8_t* levels) {
  const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  const float* row = pred + m * ld + first;
  float s = row[0];
  for (int k = 1; k < count; ++k) {                  // fmaxf's rule, spelled out: a NaN never replaces a number
    const float v = row[k];
    if (v != v) continue;
    if (s != s || v > s) s = v;
  }
  const float t = s * 255.0f;                        // -ffp-contract=off: the product is rounded before the sum
  const float f = floorf(t + 0.5f);
  levels[m] = (uint8_t)(!(f >= 0.0f) ? 0 : (f > 255.0f ? 255 : (int)f));      // NaN compares false: level 0
}

__global__ void __launch_bounds__(kDrawBatch) heat_paint_kernel(uint8_t* img, int h, int w, long long pitch, const uint8_t* __restrict__ pool,
                                                                 const radnet_heat_place* __restrict__ places, int count,
                                                                 const uint8_t* __restrict__ lut_bgr, int tau, int min_level, int tiles_x) {
  __shared__ HeatEntry entries[kDrawBatch];
  __shared__ uint8_t lut[3 * 256];
  const int tid = threadIdx.x;
  const DrawTile tile = draw_tile((int)blockIdx.x, tiles_x, h, w);
  const int x = tile.x0 + (tid % kDrawTileW), y = tile.y0 + (tid / kDrawTileW);
  const bool inside = x < w && y < h;
  int level = -1;                                    // the maximum so far; -1: no placement holds the pixel

  lut[3 * tid] = lut_bgr[3 * tid];                   // kDrawBatch == 256 colours, one per thread; read after the barriers below (count >= 1)
  lut[3 * tid + 1] = lut_bgr[3 * tid + 1];
  lut[3 * tid + 2] = lut_bgr[3 * tid + 2];

  for (int first = 0; first < count; first += kDrawBatch) {
    const int n = min(kDrawBatch, count - first);
    if (tid < n) {
      const radnet_heat_place p = places[first + tid];
      HeatEntry e;
      e.x0 = p.x0, e.y0 = p.y0, e.w = p.w, e.h = p.h, e.mw = p.mw, e.mh = p.mh, e.offset = p.offset;
      e.live = p.x0 <= tile.x1 && p.x0 + p.w > tile.x0 && p.y0 <= tile.y1 && p.y0 + p.h > tile.y0;
      entries[tid] = e;
    }
    __syncthreads();
    for (int k = 0; k < n; ++k) {
      if (!entries[k].live) continue;                // uniform over the workgroup
      const int x0 = entries[k].x0, y0 = entries[k].y0, pw = entries[k].w, ph = entries[k].h;
      if (!(inside && x >= x0 && x < x0 + pw && y >= y0 && y < y0 + ph)) continue;      // per lane from here on
      const unsigned mw = (unsigned)entries[k].mw;
      const unsigned col = ((unsigned)(x - x0) * mw) / (unsigned)pw;
      const unsigned row = ((unsigned)(y - y0) * (unsigned)entries[k].mh) / (unsigned)ph;
      level = max(level, (int)pool[entries[k].offset + (long long)(row * mw + col)]);
    }
    __syncthreads();                                 // the next batch overwrites the entries
  }
  if (level < 0 || level < min_level) return;        // level >= 0 only for a pixel inside the image
  int value = lut[3 * level] | (lut[3 * level + 1] << 8) | (lut[3 * level + 2] << 16);
  if (tau != 0) value = draw_mix(value, draw_load_bgr(img, pitch, x, y), (unsigned)tau);
  draw_store_bgr(img, pitch, x, y, value);
}

}  // namespace

extern "C" int radnet_score_levels_u8(radnet_ctx* ctx, const float* pred, int32_t ld, int32_t M, int32_t first, int32_t count, uint8_t* levels) {
  if (!ctx) return RADNET_ERR_ARG;
  if (!pred || !levels) RADNET_FAIL(ctx, RADNET_ERR_ARG, "score_levels: null scores or levels (%p, %p)", (const void*)pred, (void*)levels);
  if (M < 1) RADNET_FAIL(ctx, RADNET_ERR_ARG, "score_levels: M = %d rows", M);
  if (first < 0) RADNET_FAIL(ctx, RADNET_ERR_ARG, "score_levels: first = %d", first);
  if (count < 1) RADNET_FAIL(ctx, RADNET_ERR_ARG, "score_levels: count = %d columns", count);
  if ((int64_t)ld < (int64_t)first + count) RADNET_FAIL(ctx, RADNET_ERR_ARG, "score_levels: ld = %d for the columns %d .. %d + %d", ld, first, first, count);
  hipLaunchKernelGGL(score_levels_kernel, dim3((unsigned)(((int64_t)M + 255) / 256)), dim3(256), 0, ctx->stream, pred, ld, M, first, count, levels);
  RADNET_CHECK_LAUNCH(ctx, "score_levels_u8");
  return RADNET_OK;
}

extern "C" int radnet_heat_paint_u8(radnet_ctx* ctx, uint8_t* img, int32_t h, int32_t w, int64_t pitch_bytes, const uint8_t* pool, int64_t pool_len,
                                    const radnet_heat_place* places_host, const radnet_heat_place* places_dev, int32_t count, const uint8_t* lut_bgr,
                                    int32_t tau, int32_t min_level) {
  return draw_front(
      ctx, "heat_paint", "placements", img, h, w, pitch_bytes, places_host, places_dev, count,
      [&]() -> int {
        if (!pool || !lut_bgr) RADNET_FAIL(ctx, RADNET_ERR_ARG, "heat_paint: a null pool or colour table (pool %p, colours %p)", (const void*)pool, (const void*)lut_bgr);
        if (tau < 0 || tau > 255) RADNET_FAIL(ctx, RADNET_ERR_ARG, "heat_paint: tau = %d, outside 0..255", tau);
        if (min_level < 0 || min_level > 255) RADNET_FAIL(ctx, RADNET_ERR_ARG, "heat_paint: min_level = %d, outside 0..255", min_level);
        char why[200];
        if (radnet_heat_check(places_host, count, pool_len, h, w, nullptr, why, (int32_t)sizeof(why)) != RADNET_OK) RADNET_FAIL(ctx, RADNET_ERR_ARG, "%s", why);
        return RADNET_OK;
      },
      [&](dim3 grid, int tiles_x) {
        hipLaunchKernelGGL(heat_paint_kernel, grid, dim3(kDrawBatch), 0, ctx->stream, img, h, w, (long long)pitch_bytes, pool, places_dev, count, lut_bgr, tau,
                           min_level, tiles_x);
      });
}
