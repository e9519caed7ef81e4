// Rectangle outlines and filled rectangles painted into a uint8 [H][W][3] device image in place (radnet_draw_rects_u8; the
// annotated maps of RADNet.write_predictions).  The contract is the package's own and stands in include/radnet_hip.h: FILLED and
// thickness 1 are cv2.rectangle's pixel sets, thicker outlines have square outer corners.  Integer arithmetic only; compiled with
// -ffp-contract=off like the other exact units (there is no floating point in here).
//
// One workgroup per tile of kTileW x kTileH pixels, one pixel per thread.  The table streams through LDS in batches of
// RADNET_DRAW_RECT_BATCH entries: thread j normalises entry j of the batch (corner order, the outer box clipped to the image, the
// open inner box the outline leaves out) and marks whether it can touch the tile; then every pixel walks the batch in list order
// and keeps the colour of the LAST entry that covers it, in a register.  The mark is uniform over the workgroup, so the walk does
// not diverge on it.  A pixel no entry covers is not stored.  No atomics: every pixel has one writer, the result is that of
// painting the list in order.
#include "radnet_internal.h"

namespace {

constexpr int kTileW = 32, kTileH = 8;
constexpr int kBatch = RADNET_DRAW_RECT_BATCH;
static_assert(kTileW * kTileH == kBatch, "one thread per pixel of the tile and per entry of a batch");
static_assert(kBatch % 64 == 0, "whole waves");

struct Box {          // in image pixels, clipped: paints [ox1, ox2] x [oy1, oy2] except the open box (ix1, ix2) x (iy1, iy2)
  int ox1, oy1, ox2, oy2, ix1, iy1, ix2, iy2;
  int bgr;            // b | g << 8 | r << 16
  int live;           // can touch this workgroup's tile
};

__device__ __forceinline__ int clampi(long long v, int lo, int hi) { return (int)(v < lo ? lo : (v > hi ? hi : v)); }

__global__ void __launch_bounds__(kBatch) draw_rects_kernel(uint8_t* img, int h, int w, long long pitch, const radnet_rect* __restrict__ rects,
                                                             int count, int tiles_x) {
  __shared__ Box boxes[kBatch];
  const int tid = threadIdx.x;
  const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
  const int tx0 = tx * kTileW, ty0 = ty * kTileH;
  const int tx1 = min(tx0 + kTileW, w) - 1, ty1 = min(ty0 + kTileH, h) - 1;      // the tile's last column and row inside the image
  const int x = tx0 + (tid % kTileW), y = ty0 + (tid / kTileW);
  int colour = 0;
  bool hit = false;

  for (int first = 0; first < count; first += kBatch) {
    const int n = min(kBatch, count - first);
    if (tid < n) {
      const radnet_rect r = rects[first + tid];
      const long long x1 = min(r.x1, r.x2), x2 = max(r.x1, r.x2), y1 = min(r.y1, r.y2), y2 = max(r.y1, r.y2);
      const long long hw = r.thickness > 0 ? r.thickness / 2 : 0;
      Box b;
      b.ox1 = clampi(x1 - hw, 0, w);               // a box wholly right of the image: ox1 = w > ox2
      b.ox2 = clampi(x2 + hw, -1, w - 1);
      b.oy1 = clampi(y1 - hw, 0, h);
      b.oy2 = clampi(y2 + hw, -1, h - 1);
      if (r.thickness > 0) {                       // the open inner box, clamped to one pixel outside the image (same pixel set)
        b.ix1 = clampi(x1 + hw, -1, w);
        b.ix2 = clampi(x2 - hw, -1, w);
        b.iy1 = clampi(y1 + hw, -1, h);
        b.iy2 = clampi(y2 - hw, -1, h);
      } else {                                     // FILLED: nothing is left out
        b.ix1 = w;
        b.ix2 = -1;
        b.iy1 = h;
        b.iy2 = -1;
      }
      b.bgr = r.b | (r.g << 8) | (r.r << 16);
      const bool overlaps = b.ox1 <= tx1 && b.ox2 >= tx0 && b.oy1 <= ty1 && b.oy2 >= ty0;
      const bool swallowed = tx0 > b.ix1 && tx1 < b.ix2 && ty0 > b.iy1 && ty1 < b.iy2;      // the whole tile is inside the outline
      b.live = overlaps && !swallowed;
      boxes[tid] = b;
    }
    __syncthreads();
    for (int k = 0; k < n; ++k) {
      if (!boxes[k].live) continue;                // uniform over the workgroup
      const Box b = boxes[k];
      const bool outer = x >= b.ox1 && x <= b.ox2 && y >= b.oy1 && y <= b.oy2;
      const bool inner = x > b.ix1 && x < b.ix2 && y > b.iy1 && y < b.iy2;
      if (outer && !inner) {
        colour = b.bgr;
        hit = true;
      }
    }
    __syncthreads();                               // the next batch overwrites the boxes
  }
  if (hit && x < w && y < h) {
    uint8_t* px = img + (long long)y * pitch + (long long)x * 3;
    px[0] = (uint8_t)(colour & 255);
    px[1] = (uint8_t)((colour >> 8) & 255);
    px[2] = (uint8_t)((colour >> 16) & 255);
  }
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
  const long long tiles_x = ((long long)w + kTileW - 1) / kTileW, tiles_y = ((long long)h + kTileH - 1) / kTileH;
  if (tiles_x * tiles_y >= (1ll << 31)) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "draw_rects: an image of %d x %d", h, w);
  hipLaunchKernelGGL(draw_rects_kernel, dim3((unsigned)(tiles_x * tiles_y)), dim3(kBatch), 0, ctx->stream, img, h, w, (long long)pitch_bytes, rects_dev,
                     count, (int)tiles_x);
  RADNET_CHECK_LAUNCH(ctx, "draw_rects_u8");
  return RADNET_OK;
}
