// Ordered tables painted into a uint8 [H][W][3] device image in place, one kernel body in three instantiations: radnet_draw_rects_u8
// (outlines and filled rectangles), radnet_draw_list_u8 (rectangles and text runs; the labelled maps of RADNet.write_predictions) and
// radnet_draw_scene_u8 (those plus straight lines, solid and dashed, discs and rings, any entry translucent; the figures and label
// views of faster_rcnn/figures.py); and radnet_grey3_u8, the grey copy the label views start from.  The contracts stand in
// include/radnet_hip.h: FILLED and thickness 1 are cv2.rectangle's pixel sets, thicker outlines have square outer corners; text is the
// dot-matrix font of draw_font.h.  The tables are validated on the host by draw_scene_check.cpp.  Integer arithmetic only; compiled
// with -ffp-contract=off like the other exact units (there is no floating point in here).
//
// draw_kernel<Front>: one workgroup per tile of kDrawTileW x kDrawTileH pixels, one pixel per thread.  The table streams through LDS
// in batches of RADNET_DRAW_RECT_BATCH entries: thread j normalises entry j of the batch (draw_device.h: corner order, the outer box
// clipped to the image, the open inner box an outline leaves out; for any other kind its clipped cull box and what its test needs) and
// marks whether it can touch the tile; then every pixel walks the batch in list order.  The mark is uniform over the workgroup, so the
// walk does not diverge on it; the kind's own test behind the box test is per lane.  What a pixel keeps in a register is its RUNNING
// VALUE: an opaque entry replaces it, and without mixing that is all -- the colour of the last covering entry; a translucent entry
// mixes into it, and if nothing has set it yet the pixel is loaded first, once.  A pixel some entry covered is stored once after the
// last batch, any other pixel not at all.  No atomics: one writer per pixel, the result is that of painting the table in order.
//
// A Front fixes at compile time the table's row, the LDS entry (40, 56 and 80 bytes: what every workgroup writes per entry, whether
// or not the entry reaches its tile, and the reason there are three), whether there is text, and whether values mix.  The kinds an
// entry type has are the overloads of draw_normalise and draw_covers for it, so no front carries another's code.
//
// A text run is ONE entry whatever its length: a pixel inside a live run's box works out its character, dot column and dot row from
// the run's origin and scale, reads the character from the pool in global memory and the row byte from the font, which the workgroup
// staged into LDS (760 bytes) before the first batch.  A line is normalised to its major direction: a0 the smaller major coordinate,
// m0 the minor coordinate there, D >= 0 the major extent and dm the signed minor extent (|dm| <= D).  At major offset i = 0..D the
// centre is
//   m0 + floor((2 i dm + D) / (2 D))  =  m0 - i + (2 i (dm + D) + D) / (2 D),
// the right side with non-negative operands only (dm + D >= 0), so unsigned division is floor division; it takes 32 bits when
// D <= 8192 (2 * 8192 * 16384 + 8192 < 2^29) and 64 otherwise (i <= 2^25 and dm + D <= 2^26 by RADNET_DRAW_SCENE_MAX_COORD).  A
// pixel inside the cull box has i in [0, D].  The dash phase is the pixel's own major coordinate, which is never negative inside the
// image, so floormod is the unsigned remainder.  A disc compares dx^2 + dy^2 with rho^2 + rho in 64 bits: inside the cull box
// |dx|, |dy| <= rho_outer < 2^31, so the sum stays below 2^63.
#include "draw_check.h"
#include "draw_device.h"

namespace {

struct DrawEntry {      // the list's entry: the box, and for a text run where its dots start
  DrawBox box;
  DrawRun run;
};

struct SceneEntry {     // the scene's entry: the cull box (box.bgr carries tau in bits 24..31) and what its kind's test needs
  DrawBox box;
  union {
    DrawRun run;
    struct { int a0, m0, D, dmD; } line;      // dmD = dm + D
    struct { int cx, cy; } disc;
  };
  int lo, hi;           // line: the rows or columns below and above the centre, (t - 1) / 2 and t / 2
  long long q0, q1;     // line: the dash period on + off (0: solid) and on          disc: rho^2 + rho of the outer and of the inner
};                      //                                                              disc (-1: nothing is left out)
static_assert(sizeof(DrawBox) == 40 && sizeof(DrawEntry) == 56 && sizeof(SceneEntry) == 80, "the LDS entries the fronts were measured with");
constexpr int kSceneSmallLine = 8192;      // up to this major extent the centre's quotient fits 32 bits

struct RectFront {      // radnet_draw_rects_u8
  using Row = radnet_rect;
  using Entry = DrawBox;
  static constexpr bool kText = false, kMix = false;
};
struct ListFront {      // radnet_draw_list_u8
  using Row = radnet_prim;
  using Entry = DrawEntry;
  static constexpr bool kText = true, kMix = false;
};
struct SceneFront {     // radnet_draw_scene_u8
  using Row = radnet_prim;
  using Entry = SceneEntry;
  static constexpr bool kText = true, kMix = true;
};

__device__ __forceinline__ const DrawBox& draw_box(const DrawBox& e) { return e; }
__device__ __forceinline__ const DrawBox& draw_box(const DrawEntry& e) { return e.box; }
__device__ __forceinline__ const DrawBox& draw_box(const SceneEntry& e) { return e.box; }

// ---- a row into its entry; box.live: the entry's kind if it can touch the tile, else 0 -----------------------------------------------
__device__ __forceinline__ void draw_normalise(const radnet_rect& r, int h, int w, const DrawTile& tile, DrawBox& e) {
  e = draw_rect_box(r.x1, r.y1, r.x2, r.y2, r.thickness, r.b | (r.g << 8) | (r.r << 16), h, w);
  e.live = draw_box_touches(e, tile) ? kDrawRect : 0;
}

__device__ __forceinline__ void draw_normalise(const radnet_prim& p, int h, int w, const DrawTile& tile, DrawEntry& e) {
  if (p.kind == RADNET_PRIM_TEXT) {
    e.box = draw_text_box(p, h, w, e.run);
    e.box.live = draw_box_touches(e.box, tile) ? kDrawText : 0;
  } else {
    e.box = draw_rect_box(p.x1, p.y1, p.x2, p.y2, p.a, p.bgr, h, w);
    e.run.x0 = e.run.y0 = e.run.scale = e.run.offset = 0;
    e.box.live = draw_box_touches(e.box, tile) ? kDrawRect : 0;
  }
}

__device__ __forceinline__ void draw_normalise(const radnet_prim& p, int h, int w, const DrawTile& tile, SceneEntry& e) {
  e.line.a0 = e.line.m0 = e.line.D = e.line.dmD = e.lo = e.hi = 0;
  e.q0 = e.q1 = 0;
  int kind;
  if (p.kind == RADNET_PRIM_TEXT) {
    e.box = draw_text_box(p, h, w, e.run);
    kind = kDrawText;
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
    e.line.a0 = (int)a0;
    e.line.m0 = (int)m0;
    e.line.D = (int)(a1 - a0);
    e.line.dmD = (int)(m1 - m0 + a1 - a0);
    e.lo = (int)lo;
    e.hi = (int)hi;
    const int on = p.b & 0xFFFF, off = (p.b >> 16) & 0xFFFF;
    e.q0 = p.b ? on + off : 0;
    e.q1 = on;
    kind = xmajor ? kDrawLineX : kDrawLineY;
  } else if (p.kind == RADNET_PRIM_DISC) {
    const long long r = p.x2, hw = p.a > 0 ? p.a / 2 : 0, outer = r + hw, inner = r - hw - 1;
    e.box = draw_filled_box(p.x1 - outer, p.y1 - outer, p.x1 + outer, p.y1 + outer, p.bgr, h, w);
    e.disc.cx = p.x1;
    e.disc.cy = p.y1;
    e.q0 = outer * outer + outer;
    e.q1 = (p.a > 0 && r - hw >= 1) ? inner * inner + inner : -1;
    kind = kDrawDisc;
  } else {
    e.box = draw_rect_box(p.x1, p.y1, p.x2, p.y2, p.a, p.bgr, h, w);
    kind = kDrawRect;
  }
  e.box.live = draw_box_touches(e.box, tile) ? kind : 0;
}

// ---- does an entry of kind `live`, whose box covers the pixel, paint it -------------------------------------------------------------
__device__ __forceinline__ bool draw_covers(const DrawBox&, int, int, int, const uint8_t*, const uint8_t*) { return true; }

__device__ __forceinline__ bool draw_covers(const DrawEntry& e, int live, int x, int y, const uint8_t* __restrict__ chars, const uint8_t* font) {
  return live != kDrawText || draw_text_dot(e.run, chars, font, x, y);
}

// the centre of a line at major offset i (0 <= i <= D), relative to m0
__device__ __forceinline__ long long draw_line_centre(int i, int D, int dmD) {
  if (D == 0) return 0;
  if (D <= kSceneSmallLine) return (long long)((2u * (unsigned)i * (unsigned)dmD + (unsigned)D) / (2u * (unsigned)D)) - i;
  return (long long)((2ull * (unsigned long long)i * (unsigned long long)dmD + (unsigned long long)D) / (2ull * (unsigned long long)D)) - i;
}

__device__ __forceinline__ bool draw_covers(const SceneEntry& e, int live, int x, int y, const uint8_t* __restrict__ chars, const uint8_t* font) {
  if (live == kDrawText) return draw_text_dot(e.run, chars, font, x, y);
  if (live == kDrawLineX || live == kDrawLineY) {
    const int major = live == kDrawLineX ? x : y, minor = live == kDrawLineX ? y : x;
    const long long off = (long long)minor - e.line.m0 - draw_line_centre(major - e.line.a0, e.line.D, e.line.dmD);
    bool on = off >= -(long long)e.lo && off <= (long long)e.hi;
    const unsigned period = (unsigned)e.q0;
    if (on && period) on = (unsigned)major % period < (unsigned)e.q1;
    return on;
  }
  if (live == kDrawDisc) {
    const long long dx = (long long)x - e.disc.cx, dy = (long long)y - e.disc.cy, d2 = dx * dx + dy * dy;
    return d2 <= e.q0 && d2 > e.q1;
  }
  return true;
}

// count and tiles_x stand side by side, and an entry is marked where it is normalised, as the measured kernels had them
template <class Front>
__global__ void __launch_bounds__(kDrawBatch) draw_kernel(uint8_t* img, int h, int w, long long pitch, const typename Front::Row* __restrict__ rows, int count,
                                                           int tiles_x, const uint8_t* __restrict__ chars, int has_text) {
  __shared__ typename Front::Entry entries[kDrawBatch];
  const int tid = threadIdx.x;
  const DrawTile tile = draw_tile((int)blockIdx.x, tiles_x, h, w);
  const int x = tile.x0 + (tid % kDrawTileW), y = tile.y0 + (tid / kDrawTileW);
  int value = 0;                                   // the pixel after the entries so far, once `hit`
  bool hit = false;
  const uint8_t* font = nullptr;
  if constexpr (Front::kText) {
    __shared__ uint32_t font_words[kDrawFontBytes / 4];
    if (has_text) draw_stage_font(font_words, tid);      // read after the first barrier below
    font = reinterpret_cast<const uint8_t*>(font_words);
  }

  for (int first = 0; first < count; first += kDrawBatch) {
    const int n = min(kDrawBatch, count - first);
    if (tid < n) {
      typename Front::Entry e;
      draw_normalise(rows[first + tid], h, w, tile, e);
      entries[tid] = e;
    }
    __syncthreads();
    for (int k = 0; k < n; ++k) {
      const int live = draw_box(entries[k]).live;
      if (!live) continue;                         // uniform over the workgroup
      const DrawBox b = draw_box(entries[k]);
      if (!draw_box_covers(b, x, y)) continue;     // per lane from here on; a covered pixel lies inside the image
      if (!draw_covers(entries[k], live, x, y, chars, font)) continue;
      if constexpr (Front::kMix) {
        const unsigned tau = (unsigned)b.bgr >> 24;
        if (tau == 0) {
          value = b.bgr;
        } else {
          if (!hit) value = draw_load_bgr(img, pitch, x, y);      // the first entry to reach this pixel is translucent: the one load
          value = draw_mix(b.bgr, value, tau);
        }
      } else {
        value = b.bgr;
      }
      hit = true;
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

// radnet_draw_list_u8 and radnet_draw_scene_u8: the same arguments, the front's dialect of the table
template <class Front>
int draw_prims(radnet_ctx* ctx, const DrawDialect& dialect, uint8_t* img, int32_t h, int32_t w, int64_t pitch_bytes, const radnet_prim* prims_host,
               const radnet_prim* prims_dev, int32_t count, const uint8_t* chars_host, const uint8_t* chars_dev, int32_t n_chars) {
  int has_text = 0;
  return draw_front(
      ctx, dialect.name, "entries", img, h, w, pitch_bytes, prims_host, prims_dev, count,
      [&]() -> int {
        if (n_chars < 0 || (n_chars > 0 && (!chars_host || !chars_dev)))
          RADNET_FAIL(ctx, RADNET_ERR_ARG, "%s: a character pool of %d bytes (host %p, device %p)", dialect.name, n_chars, (const void*)chars_host,
                      (const void*)chars_dev);
        char why[200];
        if (radnet_draw_prims_check(dialect, prims_host, count, chars_host, n_chars, nullptr, why, (int32_t)sizeof(why), &has_text) != RADNET_OK)
          RADNET_FAIL(ctx, RADNET_ERR_ARG, "%s", why);
        return RADNET_OK;
      },
      [&](dim3 grid, int tiles_x) {
        hipLaunchKernelGGL(draw_kernel<Front>, grid, dim3(kDrawBatch), 0, ctx->stream, img, h, w, (long long)pitch_bytes, prims_dev, count, tiles_x, chars_dev,
                           has_text);
      });
}

}  // namespace

extern "C" int radnet_draw_rects_u8(radnet_ctx* ctx, uint8_t* img, int32_t h, int32_t w, int64_t pitch_bytes, const radnet_rect* rects_host,
                                    const radnet_rect* rects_dev, int32_t count) {
  return draw_front(
      ctx, "draw_rects", "rectangles", img, h, w, pitch_bytes, rects_host, rects_dev, count,
      [&]() -> int {
        char why[200];
        if (radnet_draw_rects_check(rects_host, count, nullptr, why, (int32_t)sizeof(why)) != RADNET_OK) RADNET_FAIL(ctx, RADNET_ERR_ARG, "%s", why);
        return RADNET_OK;
      },
      [&](dim3 grid, int tiles_x) {
        hipLaunchKernelGGL(draw_kernel<RectFront>, grid, dim3(kDrawBatch), 0, ctx->stream, img, h, w, (long long)pitch_bytes, rects_dev, count, tiles_x,
                           (const uint8_t*)nullptr, 0);
      });
}

extern "C" int radnet_draw_list_u8(radnet_ctx* ctx, uint8_t* img, int32_t h, int32_t w, int64_t pitch_bytes, const radnet_prim* prims_host,
                                   const radnet_prim* prims_dev, int32_t count, const uint8_t* chars_host, const uint8_t* chars_dev,
                                   int32_t n_chars) {
  return draw_prims<ListFront>(ctx, kDrawListDialect, img, h, w, pitch_bytes, prims_host, prims_dev, count, chars_host, chars_dev, n_chars);
}

extern "C" int radnet_draw_scene_u8(radnet_ctx* ctx, uint8_t* img, int32_t h, int32_t w, int64_t pitch_bytes, const radnet_prim* prims_host,
                                    const radnet_prim* prims_dev, int32_t count, const uint8_t* chars_host, const uint8_t* chars_dev,
                                    int32_t n_chars) {
  return draw_prims<SceneFront>(ctx, kDrawSceneDialect, img, h, w, pitch_bytes, prims_host, prims_dev, count, chars_host, chars_dev, n_chars);
}

extern "C" int radnet_draw_glyph_rows(int32_t code, uint8_t rows[8]) {
  if (!rows || code < kDrawFontFirst || code > kDrawFontLast) return RADNET_ERR_ARG;
  for (int r = 0; r < kDrawFontRows; ++r) rows[r] = kDrawFont[code - kDrawFontFirst][r];
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
