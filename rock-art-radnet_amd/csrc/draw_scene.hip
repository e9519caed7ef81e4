// A scene painted into a uint8 [H][W][3] device image in place: radnet_draw_scene_u8, the ordered list of draw.hip with straight
// lines (solid and dashed), discs and rings, and with transparency; and radnet_grey3_u8, the grey copy the label views start from.
// The contracts stand in include/radnet_hip.h; the table is validated on the host by draw_scene_check.cpp.  Integer arithmetic
// only; compiled with -ffp-contract=off like the other exact units (there is no floating point in here).
//
// draw_scene_kernel keeps the scheme of draw_list_kernel: one workgroup per tile of kDrawTileW x kDrawTileH pixels, one pixel per
// thread, the table streamed through LDS in batches of RADNET_DRAW_RECT_BATCH entries, thread j normalising entry j of the batch and
// marking whether its cull box can touch the tile (uniform over the workgroup, so the walk does not diverge on it).  What differs is
// what a pixel keeps while it walks the list: not the colour of the last covering entry but the RUNNING VALUE of the pixel.  An opaque
// entry replaces it; a translucent one mixes into it, and if nothing has set it yet the pixel is loaded first -- once, since from
// then on the value is in the register.  A pixel some entry covered is stored once after the last batch; no atomics, one writer.
//
// Coverage is O(1) per pixel and entry.  A line is normalised to its major direction: a0 the smaller major coordinate, m0 the minor
// coordinate there, D >= 0 the major extent and dm the signed minor extent (|dm| <= D).  At major offset i = 0..D the centre is
//   m0 + floor((2 i dm + D) / (2 D))  =  m0 - i + (2 i (dm + D) + D) / (2 D),
// the right side with non-negative operands only (dm + D >= 0), so unsigned division is floor division; it takes 32 bits when
// D <= 8192 (2 * 8192 * 16384 + 8192 < 2^29) and 64 otherwise (i <= 2^25 and dm + D <= 2^26 by RADNET_DRAW_SCENE_MAX_COORD).  A
// pixel inside the cull box has i in [0, D].  The dash phase is the pixel's own major coordinate, which is never negative inside the
// image, so floormod is the unsigned remainder.  A disc compares dx^2 + dy^2 with rho^2 + rho in 64 bits: inside the cull box
// |dx|, |dy| <= rho_outer < 2^31, so the sum stays below 2^63.
#include "draw_device.h"
#include "draw_font.h"

namespace {

struct SceneEntry {     // a normalised entry: the cull box (box.bgr carries tau in bits 24..31) and what its kind's test needs
  DrawBox box;          // box.live: 0, or which kind of entry can touch the tile
  int p0, p1, p2, p3;   // text: x0, y0 (the left end of the run, the top of its cap rows), scale, offset in the pool
                        // line: a0, m0, D, dm + D          disc: cx, cy
  int p4, p5;           // line: the rows or columns below and above the centre, (t - 1) / 2 and t / 2
  long long q0, q1;     // line: the dash period on + off (0: solid) and on          disc: rho^2 + rho of the outer and of the inner
};                      //                                                              disc (-1: nothing is left out)
constexpr int kSceneRect = 1, kSceneText = 2, kSceneLineX = 3, kSceneLineY = 4, kSceneDisc = 5;
constexpr int kSceneFontBytes = kDrawFontGlyphs * kDrawFontRows;
static_assert(kSceneFontBytes % 4 == 0 && kSceneFontBytes / 4 <= kDrawBatch, "one word per thread stages the font");
constexpr int kSceneSmallLine = 8192;      // up to this major extent the centre's quotient fits 32 bits

__device__ __forceinline__ SceneEntry scene_normalise(const radnet_prim& p, int h, int w) {
  SceneEntry e;
  e.p0 = e.p1 = e.p2 = e.p3 = e.p4 = e.p5 = 0;
  e.q0 = e.q1 = 0;
  int kind;
  if (p.kind == RADNET_PRIM_TEXT) {                // the box of the whole run, as in draw_list_kernel
    const long long s = p.x2, top = (long long)p.y1 - kDrawFontCapRows * s;
    const long long right = (long long)p.x1 + ((long long)kDrawFontAdvance * p.b - 1) * s - 1;
    e.box = draw_filled_box(p.x1, top, right, (long long)p.y1 + s - 1, p.bgr, h, w);
    e.p0 = p.x1;
    e.p1 = draw_clampi(top, -(kDrawFontRows * RADNET_DRAW_TEXT_MAX_SCALE), h);
    e.p2 = (int)s;
    e.p3 = p.a;
    kind = kSceneText;
  } else if (p.kind == RADNET_PRIM_LINE) {
    const long long dx = (long long)p.x2 - p.x1, dy = (long long)p.y2 - p.y1;
    const bool xmajor = (dx < 0 ? -dx : dx) >= (dy < 0 ? -dy : dy);
    long long a0 = xmajor ? p.x1 : p.y1, m0 = xmajor ? p.y1 : p.x1, a1 = xmajor ? p.x2 : p.y2, m1 = xmajor ? p.y2 : p.x2;
    if (a1 < a0) {
      const long long a = a0, m = m0;
      a0 = a1, m0 = m1, a1 = a, m1 = m;
    }
    const long long lo = ((long long)p.a - 1) / 2, hi = p.a / 2;
    const long long mlo = min(m0, m1) - lo, mhi = max(m0, m1) + hi;
    e.box = xmajor ? draw_filled_box(a0, mlo, a1, mhi, p.bgr, h, w) : draw_filled_box(mlo, a0, mhi, a1, p.bgr, h, w);
    e.p0 = (int)a0;
    e.p1 = (int)m0;
    e.p2 = (int)(a1 - a0);
    e.p3 = (int)(m1 - m0 + a1 - a0);
    e.p4 = (int)lo;
    e.p5 = (int)hi;
    const int on = p.b & 0xFFFF, off = (p.b >> 16) & 0xFFFF;
    e.q0 = p.b ? on + off : 0;
    e.q1 = on;
    kind = xmajor ? kSceneLineX : kSceneLineY;
  } else if (p.kind == RADNET_PRIM_DISC) {
    const long long r = p.x2, hw = p.a > 0 ? p.a / 2 : 0, outer = r + hw, inner = r - hw - 1;
    e.box = draw_filled_box(p.x1 - outer, p.y1 - outer, p.x1 + outer, p.y1 + outer, p.bgr, h, w);
    e.p0 = p.x1;
    e.p1 = p.y1;
    e.q0 = outer * outer + outer;
    e.q1 = (p.a > 0 && r - hw >= 1) ? inner * inner + inner : -1;
    kind = kSceneDisc;
  } else {
    e.box = draw_rect_box(p.x1, p.y1, p.x2, p.y2, p.a, p.bgr, h, w);
    kind = kSceneRect;
  }
  e.box.live = kind;
  return e;
}

// the centre of a line at major offset i (0 <= i <= D), relative to m0
__device__ __forceinline__ long long scene_line_centre(int i, int D, int dmD) {
  if (D == 0) return 0;
  if (D <= kSceneSmallLine) return (long long)((2u * (unsigned)i * (unsigned)dmD + (unsigned)D) / (2u * (unsigned)D)) - i;
  return (long long)((2ull * (unsigned long long)i * (unsigned long long)dmD + (unsigned long long)D) / (2ull * (unsigned long long)D)) - i;
}

__device__ __forceinline__ int scene_mix(int c, int d, unsigned tau) {      // per channel (c (255 - tau) + d tau + 127) / 255
  int out = 0;
  for (int k = 0; k < 24; k += 8) {
    const unsigned cc = ((unsigned)c >> k) & 255u, dd = ((unsigned)d >> k) & 255u;
    out |= (int)((cc * (255u - tau) + dd * tau + 127u) / 255u) << k;
  }
  return out;
}

__global__ void __launch_bounds__(kDrawBatch) draw_scene_kernel(uint8_t* img, int h, int w, long long pitch, const radnet_prim* __restrict__ prims,
                                                                 int count, const uint8_t* __restrict__ chars, int tiles_x, int has_text) {
  __shared__ SceneEntry entries[kDrawBatch];
  __shared__ uint32_t font_words[kSceneFontBytes / 4];
  const uint8_t* font = reinterpret_cast<const uint8_t*>(font_words);
  const int tid = threadIdx.x;
  const DrawTile tile = draw_tile((int)blockIdx.x, tiles_x, h, w);
  const int x = tile.x0 + (tid % kDrawTileW), y = tile.y0 + (tid / kDrawTileW);
  int value = 0;                                   // the pixel after the entries so far, once `known`
  bool known = false, hit = false;

  if (has_text && tid < kSceneFontBytes / 4)       // read after the first barrier below
    font_words[tid] = reinterpret_cast<const uint32_t*>(&kDrawFont[0][0])[tid];

  for (int first = 0; first < count; first += kDrawBatch) {
    const int n = min(kDrawBatch, count - first);
    if (tid < n) {
      SceneEntry e = scene_normalise(prims[first + tid], h, w);
      if (!draw_box_touches(e.box, tile)) e.box.live = 0;
      entries[tid] = e;
    }
    __syncthreads();
    for (int k = 0; k < n; ++k) {
      const int live = entries[k].box.live;
      if (!live) continue;                         // uniform over the workgroup
      const DrawBox b = entries[k].box;
      if (!draw_box_covers(b, x, y)) continue;     // per lane from here on; a covered pixel lies inside the image
      bool on = true;
      if (live == kSceneText) {                    // as in draw_list_kernel: unsigned 32-bit arithmetic is exact inside the box
        const unsigned s = (unsigned)entries[k].p2;
        const unsigned dot = ((unsigned)x - (unsigned)entries[k].p0) / s, row = (unsigned)(y - entries[k].p1) / s;
        const unsigned ch = dot / kDrawFontAdvance, col = dot - ch * kDrawFontAdvance;
        const unsigned glyph = (unsigned)chars[(long long)entries[k].p3 + ch] - kDrawFontFirst;
        on = col < kDrawFontCols && glyph < kDrawFontGlyphs && row < kDrawFontRows &&
             ((font[glyph * kDrawFontRows + row] >> (kDrawFontCols - 1 - col)) & 1);
      } else if (live == kSceneLineX || live == kSceneLineY) {
        const int major = live == kSceneLineX ? x : y, minor = live == kSceneLineX ? y : x;
        const long long off = (long long)minor - entries[k].p1 - scene_line_centre(major - entries[k].p0, entries[k].p2, entries[k].p3);
        on = off >= -(long long)entries[k].p4 && off <= (long long)entries[k].p5;
        const unsigned period = (unsigned)entries[k].q0;
        if (on && period) on = (unsigned)major % period < (unsigned)entries[k].q1;
      } else if (live == kSceneDisc) {
        const long long dx = (long long)x - entries[k].p0, dy = (long long)y - entries[k].p1, d2 = dx * dx + dy * dy;
        on = d2 <= entries[k].q0 && d2 > entries[k].q1;
      }
      if (!on) continue;
      const unsigned tau = (unsigned)b.bgr >> 24;
      if (tau == 0) {
        value = b.bgr;
      } else {
        if (!known) {                              // the first entry to reach this pixel is translucent: the one load
          const uint8_t* px = img + (long long)y * pitch + (long long)x * 3;
          value = px[0] | (px[1] << 8) | (px[2] << 16);
        }
        value = scene_mix(b.bgr, value, tau);
      }
      known = hit = true;
    }
    __syncthreads();                               // the next batch overwrites the entries
  }
  if (hit && x < w && y < h) draw_store_bgr(img, pitch, x, y, value);
}

// one workgroup walks whole rows, so no pixel index is ever divided; a thread reads its pixel's three bytes before it writes them
__global__ void __launch_bounds__(256) grey3_kernel(const uint8_t* src, uint8_t* dst, int h, int w, long long src_pitch, long long dst_pitch) {
  for (int y = blockIdx.x; y < h; y += gridDim.x) {
    const uint8_t* in = src + (long long)y * src_pitch;
    uint8_t* out = dst + (long long)y * dst_pitch;
    for (int x = threadIdx.x; x < w; x += blockDim.x) {
      const unsigned b = in[3 * (long long)x], g = in[3 * (long long)x + 1], r = in[3 * (long long)x + 2];
      const uint8_t grey = (uint8_t)((1868u * b + 9617u * g + 4899u * r + 8192u) >> 14);
      out[3 * (long long)x] = grey;
      out[3 * (long long)x + 1] = grey;
      out[3 * (long long)x + 2] = grey;
    }
  }
}

}  // namespace

extern "C" int radnet_draw_scene_u8(radnet_ctx* ctx, uint8_t* img, int32_t h, int32_t w, int64_t pitch_bytes, const radnet_prim* prims_host,
                                    const radnet_prim* prims_dev, int32_t count, const uint8_t* chars_host, const uint8_t* chars_dev,
                                    int32_t n_chars) {
  if (!ctx) return RADNET_ERR_ARG;
  if (count < 0) RADNET_FAIL(ctx, RADNET_ERR_ARG, "draw_scene: %d entries", count);
  if (count == 0) return RADNET_OK;
  if (!img || !prims_host || !prims_dev || h <= 0 || w <= 0)
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "draw_scene: null image or table, or an empty image (image %p of %d x %d, host table %p, device table %p)", (void*)img,
                h, w, (const void*)prims_host, (const void*)prims_dev);
  if (pitch_bytes < 3 * (int64_t)w) RADNET_FAIL(ctx, RADNET_ERR_ARG, "draw_scene: a pitch of %lld bytes for rows of %d pixels", (long long)pitch_bytes, w);
  if (n_chars < 0 || (n_chars > 0 && (!chars_host || !chars_dev)))
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "draw_scene: a character pool of %d bytes (host %p, device %p)", n_chars, (const void*)chars_host, (const void*)chars_dev);
  char why[200];
  if (radnet_draw_scene_check(prims_host, count, chars_host, n_chars, nullptr, why, (int32_t)sizeof(why)) != RADNET_OK)
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "%s", why);
  int has_text = 0;
  for (int i = 0; i < count; ++i) has_text |= prims_host[i].kind == RADNET_PRIM_TEXT;
  const long long tiles_x = ((long long)w + kDrawTileW - 1) / kDrawTileW, tiles_y = ((long long)h + kDrawTileH - 1) / kDrawTileH;
  if (tiles_x * tiles_y >= (1ll << 31)) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "draw_scene: an image of %d x %d", h, w);
  hipLaunchKernelGGL(draw_scene_kernel, dim3((unsigned)(tiles_x * tiles_y)), dim3(kDrawBatch), 0, ctx->stream, img, h, w, (long long)pitch_bytes, prims_dev,
                     count, chars_dev, (int)tiles_x, has_text);
  RADNET_CHECK_LAUNCH(ctx, "draw_scene_u8");
  return RADNET_OK;
}

extern "C" int radnet_grey3_u8(radnet_ctx* ctx, const uint8_t* src, uint8_t* dst, int32_t h, int32_t w, int64_t src_pitch, int64_t dst_pitch) {
  if (!ctx) return RADNET_ERR_ARG;
  if (!src || !dst || h <= 0 || w <= 0)
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "grey3: null image or an empty one (source %p, destination %p, %d x %d)", (const void*)src, (void*)dst, h, w);
  if (src_pitch < 3 * (int64_t)w || dst_pitch < 3 * (int64_t)w)
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "grey3: pitches of %lld and %lld bytes for rows of %d pixels", (long long)src_pitch, (long long)dst_pitch, w);
  hipLaunchKernelGGL(grey3_kernel, dim3((unsigned)(h < 4096 ? h : 4096)), dim3(256), 0, ctx->stream, src, dst, h, w, (long long)src_pitch, (long long)dst_pitch);
  RADNET_CHECK_LAUNCH(ctx, "grey3_u8");
  return RADNET_OK;
}
