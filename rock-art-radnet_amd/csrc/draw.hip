// Rectangles and text painted into a uint8 [H][W][3] device image in place: radnet_draw_rects_u8 (outlines and filled
// rectangles) and radnet_draw_list_u8 (an ordered list of rectangles and text runs; the labelled maps of RADNet.write_predictions).
// The contracts are the package's own and stand in include/radnet_hip.h: FILLED and thickness 1 are cv2.rectangle's pixel sets,
// thicker outlines have square outer corners; text is the dot-matrix font of draw_font.h.  Integer arithmetic only; compiled with
// -ffp-contract=off like the other exact units (there is no floating point in here).
//
// Both kernels: one workgroup per tile of kDrawTileW x kDrawTileH pixels, one pixel per thread.  The table streams through LDS in
// batches of RADNET_DRAW_RECT_BATCH entries: thread j normalises entry j of the batch (draw_device.h: corner order, the outer box
// clipped to the image, the open inner box the outline leaves out; for a text run the clipped box of the whole run) and marks whether
// it can touch the tile; then every pixel walks the batch in list order and keeps the colour of the LAST entry that covers it, in a
// register.  The mark is uniform over the workgroup, so the walk does not diverge on it.  A pixel no entry covers is not stored.  No
// atomics: every pixel has one writer, the result is that of painting the list in order.
//
// A text run is ONE entry whatever its length.  A pixel inside a live run's box works out which character, dot column and dot row
// it is from the run's origin and scale (two unsigned divisions by the scale), reads the character from the pool in global memory
// and the row byte from the font, which the workgroup staged into LDS (760 bytes) before the first batch.  That branch is per lane:
// only the lanes inside the box take it.
#include "draw_device.h"
#include "draw_font.h"

namespace {

__global__ void __launch_bounds__(kDrawBatch) draw_rects_kernel(uint8_t* img, int h, int w, long long pitch, const radnet_rect* __restrict__ rects,
                                                                 int count, int tiles_x) {
  __shared__ DrawBox boxes[kDrawBatch];
  const int tid = threadIdx.x;
  const DrawTile tile = draw_tile((int)blockIdx.x, tiles_x, h, w);
  const int x = tile.x0 + (tid % kDrawTileW), y = tile.y0 + (tid / kDrawTileW);
  int colour = 0;
  bool hit = false;

  for (int first = 0; first < count; first += kDrawBatch) {
    const int n = min(kDrawBatch, count - first);
    if (tid < n) {
      const radnet_rect r = rects[first + tid];
      DrawBox b = draw_rect_box(r.x1, r.y1, r.x2, r.y2, r.thickness, r.b | (r.g << 8) | (r.r << 16), h, w);
      b.live = draw_box_touches(b, tile);
      boxes[tid] = b;
    }
    __syncthreads();
    for (int k = 0; k < n; ++k) {
      if (!boxes[k].live) continue;                // uniform over the workgroup
      const DrawBox b = boxes[k];
      if (draw_box_covers(b, x, y)) {
        colour = b.bgr;
        hit = true;
      }
    }
    __syncthreads();                               // the next batch overwrites the boxes
  }
  if (hit && x < w && y < h) draw_store_bgr(img, pitch, x, y, colour);
}

struct DrawEntry {      // a normalised list entry: the box, and for a text run where its dots start
  DrawBox box;          // box.live: 0, or kLiveRect / kLiveText when the entry can touch the tile
  int x0, y0;           // text: the left end of the run and the top of its cap rows (exact whenever the run reaches the image)
  int scale, offset;    // text: pixels per dot; the run's first byte in the character pool
};
constexpr int kLiveRect = 1, kLiveText = 2;
constexpr int kFontBytes = kDrawFontGlyphs * kDrawFontRows;
static_assert(kFontBytes % 4 == 0, "the font is staged by words");

__global__ void __launch_bounds__(kDrawBatch) draw_list_kernel(uint8_t* img, int h, int w, long long pitch, const radnet_prim* __restrict__ prims,
                                                                int count, const uint8_t* __restrict__ chars, int tiles_x, int has_text) {
  __shared__ DrawEntry entries[kDrawBatch];
  __shared__ uint32_t font_words[kFontBytes / 4];
  const uint8_t* font = reinterpret_cast<const uint8_t*>(font_words);
  const int tid = threadIdx.x;
  const DrawTile tile = draw_tile((int)blockIdx.x, tiles_x, h, w);
  const int x = tile.x0 + (tid % kDrawTileW), y = tile.y0 + (tid / kDrawTileW);
  int colour = 0;
  bool hit = false;

  if (has_text && tid < kFontBytes / 4)            // read after the first barrier below
    font_words[tid] = reinterpret_cast<const uint32_t*>(&kDrawFont[0][0])[tid];
  static_assert(kFontBytes / 4 <= kDrawBatch, "one word per thread stages the font");

  for (int first = 0; first < count; first += kDrawBatch) {
    const int n = min(kDrawBatch, count - first);
    if (tid < n) {
      const radnet_prim p = prims[first + tid];
      DrawEntry e;
      if (p.kind == RADNET_PRIM_TEXT) {            // the box of the whole run: b characters of 6 dots less the last gap, 7 + 1 rows
        const long long s = p.x2, top = (long long)p.y1 - kDrawFontCapRows * s;
        const long long right = (long long)p.x1 + ((long long)kDrawFontAdvance * p.b - 1) * s - 1;      // b = 0: left of x1, empty
        e.box = draw_filled_box(p.x1, top, right, (long long)p.y1 + s - 1, p.bgr, h, w);
        e.x0 = p.x1;
        e.y0 = draw_clampi(top, -(kDrawFontRows * RADNET_DRAW_TEXT_MAX_SCALE), h);      // clamped only where the run is off the image
        e.scale = (int)s;
        e.offset = p.a;
        e.box.live = draw_box_touches(e.box, tile) ? kLiveText : 0;
      } else {
        e.box = draw_rect_box(p.x1, p.y1, p.x2, p.y2, p.a, p.bgr, h, w);
        e.x0 = e.y0 = e.scale = e.offset = 0;
        e.box.live = draw_box_touches(e.box, tile) ? kLiveRect : 0;
      }
      entries[tid] = e;
    }
    __syncthreads();
    for (int k = 0; k < n; ++k) {
      const int live = entries[k].box.live;
      if (!live) continue;                         // uniform over the workgroup
      const DrawBox b = entries[k].box;
      if (!draw_box_covers(b, x, y)) continue;     // per lane from here on
      bool on = true;
      if (live == kLiveText) {
        // inside the box: 0 <= x - x0 < 2^32 and 0 <= y - y0 < 8 * scale, so unsigned 32-bit arithmetic is exact
        const unsigned s = (unsigned)entries[k].scale;
        const unsigned dot = ((unsigned)x - (unsigned)entries[k].x0) / s, row = (unsigned)(y - entries[k].y0) / s;
        const unsigned ch = dot / kDrawFontAdvance, col = dot - ch * kDrawFontAdvance;
        const unsigned glyph = (unsigned)chars[(long long)entries[k].offset + ch] - kDrawFontFirst;
        on = col < kDrawFontCols && glyph < kDrawFontGlyphs && row < kDrawFontRows &&
             ((font[glyph * kDrawFontRows + row] >> (kDrawFontCols - 1 - col)) & 1);
      }
      if (on) {
        colour = b.bgr;
        hit = true;
      }
    }
    __syncthreads();                               // the next batch overwrites the entries
  }
  if (hit && x < w && y < h) draw_store_bgr(img, pitch, x, y, colour);
}

}  // namespace

extern "C" int radnet_draw_rects_u8(radnet_ctx* ctx, uint8_t* img, int32_t h, int32_t w, int64_t pitch_bytes, const radnet_rect* rects_host,
                                    const radnet_rect* rects_dev, int32_t count) {
  if (!ctx) return RADNET_ERR_ARG;
  if (count < 0) RADNET_FAIL(ctx, RADNET_ERR_ARG, "draw_rects: %d rectangles", count);
  if (count == 0) return RADNET_OK;
  if (!img || !rects_host || !rects_dev || h <= 0 || w <= 0)
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "draw_rects: null image or table, or an empty image (image %p of %d x %d, host table %p, device table %p)", (void*)img,
                h, w, (const void*)rects_host, (const void*)rects_dev);
  if (pitch_bytes < 3 * (int64_t)w) RADNET_FAIL(ctx, RADNET_ERR_ARG, "draw_rects: a pitch of %lld bytes for rows of %d pixels", (long long)pitch_bytes, w);
  for (int i = 0; i < count; ++i) {
    const radnet_rect& r = rects_host[i];
    if (r.thickness == 0) RADNET_FAIL(ctx, RADNET_ERR_ARG, "draw_rects: rectangle %d has thickness 0", i);
    if (r.b < 0 || r.b > 255 || r.g < 0 || r.g > 255 || r.r < 0 || r.r > 255)
      RADNET_FAIL(ctx, RADNET_ERR_ARG, "draw_rects: rectangle %d has the colour (%d, %d, %d)", i, r.b, r.g, r.r);
  }
  const long long tiles_x = ((long long)w + kDrawTileW - 1) / kDrawTileW, tiles_y = ((long long)h + kDrawTileH - 1) / kDrawTileH;
  if (tiles_x * tiles_y >= (1ll << 31)) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "draw_rects: an image of %d x %d", h, w);
  hipLaunchKernelGGL(draw_rects_kernel, dim3((unsigned)(tiles_x * tiles_y)), dim3(kDrawBatch), 0, ctx->stream, img, h, w, (long long)pitch_bytes, rects_dev,
                     count, (int)tiles_x);
  RADNET_CHECK_LAUNCH(ctx, "draw_rects_u8");
  return RADNET_OK;
}

extern "C" int radnet_draw_glyph_rows(int32_t code, uint8_t rows[8]) {
  if (!rows || code < kDrawFontFirst || code > kDrawFontLast) return RADNET_ERR_ARG;
  for (int r = 0; r < kDrawFontRows; ++r) rows[r] = kDrawFont[code - kDrawFontFirst][r];
  return RADNET_OK;
}

extern "C" int radnet_draw_list_u8(radnet_ctx* ctx, uint8_t* img, int32_t h, int32_t w, int64_t pitch_bytes, const radnet_prim* prims_host,
                                   const radnet_prim* prims_dev, int32_t count, const uint8_t* chars_host, const uint8_t* chars_dev,
                                   int32_t n_chars) {
  if (!ctx) return RADNET_ERR_ARG;
  if (count < 0) RADNET_FAIL(ctx, RADNET_ERR_ARG, "draw_list: %d entries", count);
  if (count == 0) return RADNET_OK;
  if (!img || !prims_host || !prims_dev || h <= 0 || w <= 0)
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "draw_list: null image or table, or an empty image (image %p of %d x %d, host table %p, device table %p)", (void*)img, h,
                w, (const void*)prims_host, (const void*)prims_dev);
  if (pitch_bytes < 3 * (int64_t)w) RADNET_FAIL(ctx, RADNET_ERR_ARG, "draw_list: a pitch of %lld bytes for rows of %d pixels", (long long)pitch_bytes, w);
  if (n_chars < 0 || (n_chars > 0 && (!chars_host || !chars_dev)))
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "draw_list: a character pool of %d bytes (host %p, device %p)", n_chars, (const void*)chars_host, (const void*)chars_dev);
  int has_text = 0;
  for (int i = 0; i < count; ++i) {
    const radnet_prim& p = prims_host[i];
    if (p.bgr < 0 || p.bgr > 0xFFFFFF) RADNET_FAIL(ctx, RADNET_ERR_ARG, "draw_list: entry %d has the colour 0x%08X", i, (unsigned)p.bgr);
    if (p.kind == RADNET_PRIM_RECT) {
      if (p.a == 0) RADNET_FAIL(ctx, RADNET_ERR_ARG, "draw_list: entry %d is a rectangle of thickness 0", i);
    } else if (p.kind == RADNET_PRIM_TEXT) {
      if (p.x2 < 1 || p.x2 > RADNET_DRAW_TEXT_MAX_SCALE) RADNET_FAIL(ctx, RADNET_ERR_ARG, "draw_list: entry %d has the text scale %d", i, p.x2);
      if (p.y2 != 0) RADNET_FAIL(ctx, RADNET_ERR_ARG, "draw_list: entry %d is text with y2 = %d, not 0", i, p.y2);
      if (p.a < 0 || p.b < 0 || (int64_t)p.a + p.b > n_chars)
        RADNET_FAIL(ctx, RADNET_ERR_ARG, "draw_list: entry %d takes %d characters at offset %d of a pool of %d", i, p.b, p.a, n_chars);
      for (int k = 0; k < p.b; ++k) {
        const int code = chars_host[p.a + k];
        if (code < kDrawFontFirst || code > kDrawFontLast)
          RADNET_FAIL(ctx, RADNET_ERR_ARG, "draw_list: entry %d has the byte 0x%02X as character %d", i, code, k);
      }
      has_text = 1;
    } else {
      RADNET_FAIL(ctx, RADNET_ERR_ARG, "draw_list: entry %d is of the unknown kind %d", i, p.kind);
    }
  }
  const long long tiles_x = ((long long)w + kDrawTileW - 1) / kDrawTileW, tiles_y = ((long long)h + kDrawTileH - 1) / kDrawTileH;
  if (tiles_x * tiles_y >= (1ll << 31)) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "draw_list: an image of %d x %d", h, w);
  hipLaunchKernelGGL(draw_list_kernel, dim3((unsigned)(tiles_x * tiles_y)), dim3(kDrawBatch), 0, ctx->stream, img, h, w, (long long)pitch_bytes, prims_dev,
                     count, chars_dev, (int)tiles_x, has_text);
  RADNET_CHECK_LAUNCH(ctx, "draw_list_u8");
  return RADNET_OK;
}
