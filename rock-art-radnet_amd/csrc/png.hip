// The two per-byte steps of PNG decoding on the device (faster_rcnn/png.py does the container and the inflate on the host):
// scanline reconstruction ("unfiltering", PNG specification section 9) in place on the inflated stream of one pass, and the
// expansion of the reconstructed samples to the uint8 BGR HWC image cv2.imdecode(buf, IMREAD_COLOR) returns.  Integer
// arithmetic only; compiled with -ffp-contract=off like the other exact units (there is no floating point in here).
//
// Reconstruction depends on the byte to the left (a), the byte above (b) and the byte above-left (c), so the parallelism is a
// skewed wavefront.  One workgroup of kWaves waves walks the pass band by band (RADNET_PNG_UNFILTER_BAND_ROWS rows), one lane per
// row.  Inside a wave row l lags row l - 1 by one pixel: what lane l - 1 produced in the previous step is lane l's `b`, moved by
// one DPP wave shift, and last step's `b` is this step's `c`.  Wave w lags wave w - 1 by one whole chunk on top of that
// (lane offset w * (63 + T) + l pixels, T = pixels per chunk): the row above a wave's first row is complete, in global memory,
// one chunk behind, and is staged beside the wave's own 64 row segments.  Row data moves between global memory and LDS in
// chunks of RADNET_PNG_UNFILTER_CHUNK_BYTES per row, consecutive lanes on consecutive bytes.  Every loop bound is a function of
// (rows, rowbytes, bpp); workgroups never wait for each other: radnet_png_unfilter_u8 launches one, and
// radnet_png_unfilter_segments_u8 one per segment, where a segment (csrc/png_plan.cpp) is a run of rows whose first row does not
// read the row above it (row 0 of a pass, or filter type 0 / 1), so no segment reads a byte another one writes.  Rows that allow no
// such cut are spread over the device by png_tiles.hip (radnet_png_unfilter_tiles_u8), which shares png_predict.h with this file.
// The writer's half is the forward filter (radnet_png_filter_rows_u8, further down): a device image to the scanline stream, one
// workgroup per row, the adaptive choice of a row's filter type by integer sums.
#include "radnet_internal.h"
#include "png_predict.h"

namespace {

constexpr int kWaves = RADNET_PNG_UNFILTER_BAND_ROWS / 64;
constexpr int kChunk = RADNET_PNG_UNFILTER_CHUNK_BYTES;
constexpr int kLdsStride = kChunk + 4;      // 25 dwords per row segment: lanes reading one column of 64 rows hit 64 different banks
static_assert(RADNET_PNG_UNFILTER_BAND_ROWS % 64 == 0 && kWaves >= 1 && kWaves <= 16, "a band is a whole number of waves");
static_assert(kChunk % 24 == 0, "a chunk holds a whole number of pixels for every bpp in {1, 2, 3, 4, 6, 8}");
static_assert(kWaves * 65 * kLdsStride <= 65536, "static LDS");

// from_lane_above (the DPP wave shift) and predictor: png_predict.h

// The walk of one independent run of scanlines: `rows` rows of 1 + rowbytes bytes at `stream`, the row above row 0 counting as
// zeros.  A whole pass is such a run, and so is a segment of one that starts on a row of filter type 0 or 1 (png_plan.cpp).
// WAVES waves of one workgroup, lds[WAVES][65][kLdsStride]; every thread of the workgroup calls it with the same arguments.
template <int BPP, int WAVES>
__device__ __forceinline__ void unfilter_rows(uint8_t (*lds)[65][kLdsStride], uint8_t* stream, int rows, int rowbytes) {
  constexpr int T = kChunk / BPP;                  // pixels per chunk
  constexpr int kWaveLag = 63 + T;                 // pixels wave w lags wave w - 1
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long pitch = 1 + (long long)rowbytes;
  const int P = rowbytes / BPP;
  const int waves_used = min(WAVES, (rows + 63) / 64);
  const int n_iter = (P + (waves_used - 1) * kWaveLag + 63 + T - 1) / T;      // until the last lane of the last wave is through

  for (int band = 0; band < rows; band += WAVES * 64) {
    const int wave_r0 = band + w * 64;
    const int r = wave_r0 + lane;
    const bool valid = r < rows;
    const int ft = valid ? stream[r * pitch] : 0;
    int a[BPP], bprev[BPP];
#pragma unroll
    for (int j = 0; j < BPP; ++j) a[j] = bprev[j] = 0;

    for (int k = 0; k < n_iter; ++k) {
      const int ps0 = k * T - w * kWaveLag;        // lane 0's first pixel of this chunk; lane l's is ps0 - l
      const bool wave_on = wave_r0 < rows && ps0 + T > 0 && ps0 - 63 < P;
      if (wave_on) {
        // stage: row j of the wave at bytes [(ps0 - j) * BPP, + kChunk); j = 64: the row above the wave at lane 0's bytes
        for (int j = 0; j < 65; ++j) {
          const int rr = j < 64 ? wave_r0 + j : wave_r0 - 1;
          const int byte0 = (ps0 - (j < 64 ? j : 0)) * BPP;
          const bool row_ok = rr >= 0 && rr < rows;
          for (int i = lane; i < kChunk; i += 64) {
            const int pos = byte0 + i;
            lds[w][j][i] = (row_ok && pos >= 0 && pos < rowbytes) ? stream[rr * pitch + 1 + pos] : (uint8_t)0;
          }
        }
      }
      __syncthreads();
      if (wave_on) {
        uint8_t* mine = lds[w][lane];
        const uint8_t* above = lds[w][64];
#pragma unroll 2
        for (int s = 0; s < T; ++s) {
          const int p = ps0 - lane + s;
          int b[BPP], x[BPP];
#pragma unroll
          for (int j = 0; j < BPP; ++j) {
            b[j] = from_lane_above(a[j]);
            x[j] = mine[s * BPP + j];
          }
          if (lane == 0) {
#pragma unroll
            for (int j = 0; j < BPP; ++j) b[j] = above[s * BPP + j];
          }
          const bool on = valid && p >= 0 && p < P;
#pragma unroll
          for (int j = 0; j < BPP; ++j) {
            const int out = (x[j] + predictor(ft, a[j], b[j], bprev[j])) & 255;
            if (on) mine[s * BPP + j] = (uint8_t)out;
            a[j] = on ? out : 0;                   // left of the row and outside the image count as 0
            bprev[j] = b[j];
          }
        }
      }
      __syncthreads();
      if (wave_on) {
        for (int j = 0; j < 64; ++j) {
          const int rr = wave_r0 + j;
          if (rr >= rows) break;
          const int byte0 = (ps0 - j) * BPP;
          for (int i = lane; i < kChunk; i += 64) {
            const int pos = byte0 + i;
            if (pos >= 0 && pos < rowbytes) stream[rr * pitch + 1 + pos] = lds[w][j][i];
          }
        }
      }
      __syncthreads();                             // the next chunk of the wave below reads these rows from global memory
    }
  }
}

template <int BPP>
__global__ void __launch_bounds__(kWaves * 64) png_unfilter_kernel(uint8_t* stream, int rows, int rowbytes) {
  __shared__ uint8_t lds[kWaves][65][kLdsStride];  // per wave: 64 row segments, then the segment of the row above lane 0
  unfilter_rows<BPP, kWaves>(lds, stream, rows, rowbytes);
}

// One workgroup per table entry first + blockIdx.x: WAVES == 1 takes the segments of at most 64 rows (one wave, a 6.5 KB tile, so
// many workgroups share a CU), WAVES == kWaves the longer ones; an entry of the other kind is left to the other launch.  The
// branch is uniform over the workgroup, so every thread that enters unfilter_rows reaches its barriers.
template <int BPP, int WAVES>
__global__ void __launch_bounds__(WAVES * 64) png_unfilter_segments_kernel(uint8_t* base, const radnet_png_segment* __restrict__ segs, int first) {
  __shared__ uint8_t lds[WAVES][65][kLdsStride];
  const radnet_png_segment seg = segs[first + (int)blockIdx.x];
  if ((seg.rows <= 64) != (WAVES == 1)) return;
  unfilter_rows<BPP, WAVES>(lds, base + seg.offset, seg.rows, seg.rowbytes);
}

// ---- expansion to BGR ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int packed_sample(const uint8_t* row, int c, int depth) {      // depth 1 / 2 / 4, MSB first
  const int bit = c * depth;
  return (row[bit >> 3] >> (8 - depth - (bit & 7))) & ((1 << depth) - 1);
}

__global__ void __launch_bounds__(256) png_expand_kernel(const uint8_t* __restrict__ stream, int pass_h, int pass_w, int rowbytes, int color_type,
                                                         int depth, const uint8_t* __restrict__ palette_bgr, uint8_t* __restrict__ dst, int dst_w,
                                                         int y0, int x0, int dy, int dx) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)pass_h * pass_w) return;
  const int r = (int)(idx / pass_w), c = (int)(idx - (long long)r * pass_w);
  const uint8_t* row = stream + r * (1 + (long long)rowbytes) + 1;
  const int bs = depth == 16 ? 2 : 1;              // bytes per sample; a 16-bit sample keeps its high (first) byte
  uint8_t blue, green, red;
  if (color_type == 0 || color_type == 4) {
    int g;
    if (depth >= 8) g = row[(long long)c * bs * (color_type == 4 ? 2 : 1)];
    else g = packed_sample(row, c, depth) * (255 / ((1 << depth) - 1));
    blue = green = red = (uint8_t)g;
  } else if (color_type == 3) {
    const int i = depth == 8 ? row[c] : packed_sample(row, c, depth);
    blue = palette_bgr[i * 3];
    green = palette_bgr[i * 3 + 1];
    red = palette_bgr[i * 3 + 2];
  } else {
    const uint8_t* px = row + (long long)c * bs * (color_type == 6 ? 4 : 3);
    red = px[0];
    green = px[bs];
    blue = px[2 * bs];
  }
  uint8_t* d = dst + ((long long)(y0 + r * dy) * dst_w + (x0 + c * dx)) * 3;
  d[0] = blue;
  d[1] = green;
  d[2] = red;
}

// ---- forward filter (the writer's half) ------------------------------------------------------------------------------------------
// A filtered byte depends on raw bytes only -- x, the byte bpp to the left (a), the one above (b), the one above-left (c) -- so
// every row, and every byte of it, is independent: one workgroup per row, kFilterThreads consecutive stream bytes per sweep, one
// byte per thread.  CH == 3 reads the B, G, R image as R, G, B.  The loads are byte loads of two image rows the caches hold; the
// stores are byte stores to consecutive addresses (a stream row starts at any byte offset, so nothing wider is assumed).
constexpr int kFilterThreads = 256;

template <int CH>
__device__ __forceinline__ void raw_neighbours(const uint8_t* __restrict__ row, const uint8_t* __restrict__ above, int i, int& x, int& a, int& b, int& c) {
  int src = i;                                     // byte i of the stream row is byte src of the image row
  if (CH == 3) {
    const int px = i / 3;
    src = 3 * px + 2 - (i - 3 * px);
  }
  x = row[src];
  a = i >= CH ? row[src - CH] : 0;
  b = above ? above[src] : 0;
  c = (above && i >= CH) ? above[src - CH] : 0;
}

__device__ __forceinline__ int signed_size(int v) { return v > 128 ? 256 - v : v; }      // min(v, 256 - v) of a residual byte

template <int CH>
__global__ void __launch_bounds__(kFilterThreads) png_filter_rows_kernel(const uint8_t* __restrict__ img, int w, long long pitch, int mode,
                                                                          uint8_t* __restrict__ stream) {
  __shared__ unsigned wave_sums[kFilterThreads / 64][5];
  const int r = (int)blockIdx.x, tid = (int)threadIdx.x, n = w * CH;
  const uint8_t* row = img + (long long)r * pitch;
  const uint8_t* above = r > 0 ? row - pitch : nullptr;
  uint8_t* out = stream + (long long)r * (1 + (long long)n);
  int ft = mode;
  if (mode == 5) {
    unsigned sums[5] = {0, 0, 0, 0, 0};            // at most 128 * 2^24 = 2^31 each
    for (int i = tid; i < n; i += kFilterThreads) {
      int x, a, b, c;
      raw_neighbours<CH>(row, above, i, x, a, b, c);
#pragma unroll
      for (int f = 0; f < 5; ++f) sums[f] += (unsigned)signed_size((x - predictor(f, a, b, c)) & 255);
    }
#pragma unroll
    for (int f = 0; f < 5; ++f) {
      unsigned v = sums[f];
      for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
      if ((tid & 63) == 0) wave_sums[tid >> 6][f] = v;
    }
    __syncthreads();
    unsigned best = 0;
    ft = 0;
#pragma unroll
    for (int f = 0; f < 5; ++f) {                  // every thread folds the same numbers: the choice is uniform
      unsigned v = 0;
      for (int k = 0; k < kFilterThreads / 64; ++k) v += wave_sums[k][f];
      if (f == 0 || v < best) {                    // strictly smaller: on a tie the lowest type stays
        best = v;
        ft = f;
      }
    }
  }
  if (tid == 0) out[0] = (uint8_t)ft;
  for (int i = tid; i < n; i += kFilterThreads) {
    int x, a, b, c;
    raw_neighbours<CH>(row, above, i, x, a, b, c);
    out[1 + i] = (uint8_t)((x - predictor(ft, a, b, c)) & 255);
  }
}

int channels_of(int color_type) {
  switch (color_type) {
    case 0: return 1;
    case 2: return 3;
    case 3: return 1;
    case 4: return 2;
    case 6: return 4;
  }
  return 0;
}

bool legal_format(int color_type, int depth) {
  if (color_type == 0) return depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16;
  if (color_type == 3) return depth == 1 || depth == 2 || depth == 4 || depth == 8;
  if (color_type == 2 || color_type == 4 || color_type == 6) return depth == 8 || depth == 16;
  return false;
}

}  // namespace

extern "C" int radnet_png_unfilter_u8(radnet_ctx* ctx, uint8_t* stream, int32_t rows, int32_t rowbytes, int32_t bpp) {
  if (!ctx || !stream || rows <= 0 || rowbytes <= 0) return RADNET_ERR_ARG;
  if (!(bpp == 1 || bpp == 2 || bpp == 3 || bpp == 4 || bpp == 6 || bpp == 8) || rowbytes % bpp != 0)
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "png_unfilter: %d bytes per pixel with %d bytes per row", bpp, rowbytes);
  if (rowbytes > (1 << 30)) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "png_unfilter: %d bytes per row", rowbytes);
  const dim3 grid(1), block(kWaves * 64);
  switch (bpp) {
    case 1: hipLaunchKernelGGL(png_unfilter_kernel<1>, grid, block, 0, ctx->stream, stream, rows, rowbytes); break;
    case 2: hipLaunchKernelGGL(png_unfilter_kernel<2>, grid, block, 0, ctx->stream, stream, rows, rowbytes); break;
    case 3: hipLaunchKernelGGL(png_unfilter_kernel<3>, grid, block, 0, ctx->stream, stream, rows, rowbytes); break;
    case 4: hipLaunchKernelGGL(png_unfilter_kernel<4>, grid, block, 0, ctx->stream, stream, rows, rowbytes); break;
    case 6: hipLaunchKernelGGL(png_unfilter_kernel<6>, grid, block, 0, ctx->stream, stream, rows, rowbytes); break;
    default: hipLaunchKernelGGL(png_unfilter_kernel<8>, grid, block, 0, ctx->stream, stream, rows, rowbytes); break;
  }
  RADNET_CHECK_LAUNCH(ctx, "png_unfilter_u8");
  return RADNET_OK;
}

namespace {

template <int WAVES>
void launch_segments(radnet_ctx* ctx, uint8_t* base, const radnet_png_segment* segs, int first, int n, int bpp) {
  const dim3 grid((unsigned)n), block(WAVES * 64);
  switch (bpp) {
    case 1: hipLaunchKernelGGL((png_unfilter_segments_kernel<1, WAVES>), grid, block, 0, ctx->stream, base, segs, first); break;
    case 2: hipLaunchKernelGGL((png_unfilter_segments_kernel<2, WAVES>), grid, block, 0, ctx->stream, base, segs, first); break;
    case 3: hipLaunchKernelGGL((png_unfilter_segments_kernel<3, WAVES>), grid, block, 0, ctx->stream, base, segs, first); break;
    case 4: hipLaunchKernelGGL((png_unfilter_segments_kernel<4, WAVES>), grid, block, 0, ctx->stream, base, segs, first); break;
    case 6: hipLaunchKernelGGL((png_unfilter_segments_kernel<6, WAVES>), grid, block, 0, ctx->stream, base, segs, first); break;
    default: hipLaunchKernelGGL((png_unfilter_segments_kernel<8, WAVES>), grid, block, 0, ctx->stream, base, segs, first); break;
  }
}

}  // namespace

extern "C" int radnet_png_unfilter_segments_u8(radnet_ctx* ctx, uint8_t* base, int64_t base_len, const radnet_png_segment* segs_host,
                                               const radnet_png_segment* segs_dev, int32_t count, int32_t bpp) {
  if (!ctx) return RADNET_ERR_ARG;
  if (count < 0) RADNET_FAIL(ctx, RADNET_ERR_ARG, "png_unfilter_segments: %d segments", count);
  if (count == 0) return RADNET_OK;
  if (!base || !segs_host || !segs_dev || base_len <= 0)
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "png_unfilter_segments: null buffer or table (base %p of %lld bytes, host table %p, device table %p)", (void*)base,
                (long long)base_len, (const void*)segs_host, (const void*)segs_dev);
  if (!(bpp == 1 || bpp == 2 || bpp == 3 || bpp == 4 || bpp == 6 || bpp == 8))
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "png_unfilter_segments: %d bytes per pixel", bpp);
  // the index range each launch has to span: [lo, hi) of the segments of at most 64 rows and of the longer ones
  int lo[2] = {count, count}, hi[2] = {0, 0};
  for (int i = 0; i < count; ++i) {
    const radnet_png_segment& s = segs_host[i];
    if (s.rows <= 0 || s.rowbytes <= 0 || s.rowbytes % bpp != 0)
      RADNET_FAIL(ctx, RADNET_ERR_ARG, "png_unfilter_segments: segment %d has %d rows of %d bytes at %d bytes per pixel", i, s.rows, s.rowbytes, bpp);
    if (s.rowbytes > (1 << 30)) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "png_unfilter_segments: segment %d has %d bytes per row", i, s.rowbytes);
    const int64_t bytes = (int64_t)s.rows * (1 + (int64_t)s.rowbytes);       // below 2^62
    if (s.offset < 0 || s.offset > base_len || bytes > base_len - s.offset)
      RADNET_FAIL(ctx, RADNET_ERR_ARG, "png_unfilter_segments: segment %d (%lld bytes at offset %lld) leaves the buffer of %lld bytes", i, (long long)bytes,
                  (long long)s.offset, (long long)base_len);
    const int k = s.rows <= 64 ? 0 : 1;
    lo[k] = i < lo[k] ? i : lo[k];
    hi[k] = i + 1;
  }
  if (hi[0] > lo[0]) {
    launch_segments<1>(ctx, base, segs_dev, lo[0], hi[0] - lo[0], bpp);
    RADNET_CHECK_LAUNCH(ctx, "png_unfilter_segments_u8 (one-wave segments)");
  }
  if (hi[1] > lo[1]) {
    launch_segments<kWaves>(ctx, base, segs_dev, lo[1], hi[1] - lo[1], bpp);
    RADNET_CHECK_LAUNCH(ctx, "png_unfilter_segments_u8 (band-sized segments)");
  }
  return RADNET_OK;
}

extern "C" int radnet_png_expand_bgr_u8(radnet_ctx* ctx, const uint8_t* stream, int32_t pass_h, int32_t pass_w, int32_t rowbytes, int32_t color_type,
                                        int32_t bit_depth, const uint8_t* palette_bgr, uint8_t* dst, int32_t dst_h, int32_t dst_w, int32_t y0,
                                        int32_t x0, int32_t dy, int32_t dx) {
  if (!ctx || !stream || !dst || pass_h <= 0 || pass_w <= 0 || rowbytes <= 0 || dst_h <= 0 || dst_w <= 0) return RADNET_ERR_ARG;
  if (!legal_format(color_type, bit_depth)) RADNET_FAIL(ctx, RADNET_ERR_ARG, "png_expand: colour type %d with bit depth %d", color_type, bit_depth);
  if (color_type == 3 && !palette_bgr) RADNET_FAIL(ctx, RADNET_ERR_ARG, "png_expand: colour type 3 without a palette");
  const long long need = ((long long)pass_w * channels_of(color_type) * bit_depth + 7) / 8;
  if (rowbytes < need) RADNET_FAIL(ctx, RADNET_ERR_ARG, "png_expand: %d bytes per row hold fewer than %d pixels", rowbytes, pass_w);
  if (y0 < 0 || x0 < 0 || dy <= 0 || dx <= 0 || (long long)y0 + (long long)(pass_h - 1) * dy >= dst_h || (long long)x0 + (long long)(pass_w - 1) * dx >= dst_w)
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "png_expand: pass %d x %d from (%d, %d) by (%d, %d) outside %d x %d", pass_h, pass_w, y0, x0, dy, dx, dst_h, dst_w);
  const long long total = (long long)pass_h * pass_w;
  if (total >= (1ll << 31)) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "png_expand: %lld pixels", total);
  hipLaunchKernelGGL(png_expand_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, stream, pass_h, pass_w, rowbytes, color_type,
                     bit_depth, palette_bgr, dst, dst_w, y0, x0, dy, dx);
  RADNET_CHECK_LAUNCH(ctx, "png_expand_bgr_u8");
  return RADNET_OK;
}

extern "C" int radnet_png_filter_rows_u8(radnet_ctx* ctx, const uint8_t* img, int32_t h, int32_t w, int32_t channels, int64_t pitch_bytes, int32_t mode,
                                         uint8_t* stream) {
  if (!ctx) return RADNET_ERR_ARG;
  if (!img || !stream || h <= 0 || w <= 0) RADNET_FAIL(ctx, RADNET_ERR_ARG, "png_filter_rows: null image or stream, or an empty image (%d x %d)", h, w);
  if (channels != 1 && channels != 3) RADNET_FAIL(ctx, RADNET_ERR_ARG, "png_filter_rows: %d channels (1 or 3)", channels);
  if (mode < 0 || mode > 5) RADNET_FAIL(ctx, RADNET_ERR_ARG, "png_filter_rows: mode %d (0..4 fixed, 5 adaptive)", mode);
  const int64_t rowbytes = (int64_t)w * channels;
  if (rowbytes > (1 << 24)) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "png_filter_rows: %lld bytes per row (at most 2^24)", (long long)rowbytes);
  if (pitch_bytes < rowbytes) RADNET_FAIL(ctx, RADNET_ERR_ARG, "png_filter_rows: a pitch of %lld bytes for rows of %lld bytes", (long long)pitch_bytes, (long long)rowbytes);
  const dim3 grid((unsigned)h), block(kFilterThreads);
  if (channels == 3) hipLaunchKernelGGL(png_filter_rows_kernel<3>, grid, block, 0, ctx->stream, img, w, (long long)pitch_bytes, mode, stream);
  else hipLaunchKernelGGL(png_filter_rows_kernel<1>, grid, block, 0, ctx->stream, img, w, (long long)pitch_bytes, mode, stream);
  RADNET_CHECK_LAUNCH(ctx, "png_filter_rows_u8");
  return RADNET_OK;
}
