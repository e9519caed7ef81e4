// ---- CRC-32 of byte ranges of a device buffer (contract: include/radnet_hip.h, radnet_crc32_segments) ------------------------------------
// The sum is linear over GF(2), so it is cut wherever that suits the machine (csrc/crc32_rule.h: the identities and THE GRAIN RULE)
// and three launches carry every table, one segment of tens of MB as well as thousands of small ones:
//   crc32_scan    one workgroup: `result`, and the exclusive prefix sum of the segments' span counts (where each one's spans stand)
//   crc32_spans   one workgroup per span of 256 grains: a lane sums its 16 bytes, weighs the sum by its distance from the span's end
//                 -- one product with a constant -- and the xor of the 256 is the span's sum
//   crc32_finish  one workgroup per segment: the spans weighed the same way (beyond 256 of them by Horner's rule per lane), the up to
//                 15 tail bytes, the init folded in with x^(8 length), the final xor, the compare with `expect`
// The byte steps are bitwise: 32 shift / xor steps per 4 bytes in registers.  A table of 256 words in LDS would take 4 random lookups
// per 4 bytes, which conflict on the banks, and every workgroup would have to fill it first for 16 bytes per lane; bitwise a 35 MB
// stream is about 1.5 * 10^9 lane operations, tens of microseconds on 256 CUs, and the kernel stays bound by its loads.
// No workgroup waits on another, no loop is bounded by anything but a length or a count, no atomics but the two on `result`.
#include "radnet_internal.h"
#include "crc32_rule.h"

namespace {

__constant__ const crc_table<kCrcSpanGrains> kGrainWeight = crc_powers<kCrcSpanGrains>(kCrcGrain);      // x^(8 * 16 t)
__constant__ const crc_table<kCrcSpanGrains> kSpanWeight = crc_powers<kCrcSpanGrains>(kCrcSpan);        // x^(8 * 4096 t)
__constant__ const crc_table<64> kSquares = crc_squares();                                              // x^(8 * 2^k)
constexpr uint32_t kSpanStride = crc_shift(kCrcSpan * kCrcSpanGrains);                                  // x^(8 * 4096 * 256)

// the xor of v over the 256 lanes of the workgroup, in every lane
__device__ __forceinline__ uint32_t block_xor(uint32_t v, uint32_t* waves) {
  for (int d = 32; d >= 1; d >>= 1) v ^= __shfl_xor(v, d);
  __syncthreads();                         // the last call's readers are done with `waves`
  if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = v;
  __syncthreads();
  return waves[0] ^ waves[1] ^ waves[2] ^ waves[3];
}

__global__ __launch_bounds__(kCrcSpanGrains) void crc32_scan_kernel(const radnet_crc32_segment* __restrict__ table, int32_t count, uint32_t misalign,
                                                                     uint32_t* __restrict__ first, int32_t* __restrict__ result) {
  __shared__ uint32_t sums[kCrcSpanGrains];
  const int t = threadIdx.x;
  if (t == 0) {
    result[0] = count;
    result[1] = 0;
  }
  const int64_t per = ((int64_t)count + kCrcSpanGrains - 1) / kCrcSpanGrains;
  const int64_t lo = std::min<int64_t>(t * per, count), hi = std::min<int64_t>(lo + per, count);
  uint32_t mine = 0;
  for (int64_t i = lo; i < hi; ++i) mine += (uint32_t)crc_cut_of(misalign + (uint64_t)table[i].offset, table[i].length).spans;
  sums[t] = mine;
  __syncthreads();
  for (int d = 1; d < kCrcSpanGrains; d <<= 1) {      // inclusive scan
    const uint32_t left = t >= d ? sums[t - d] : 0;
    __syncthreads();
    sums[t] += left;
    __syncthreads();
  }
  uint32_t at = sums[t] - mine;
  for (int64_t i = lo; i < hi; ++i) {
    first[i] = at;
    at += (uint32_t)crc_cut_of(misalign + (uint64_t)table[i].offset, table[i].length).spans;
  }
  if (t == kCrcSpanGrains - 1) first[count] = sums[t];
}

__global__ __launch_bounds__(kCrcSpanGrains) void crc32_spans_kernel(const uint8_t* __restrict__ buf, const radnet_crc32_segment* __restrict__ table,
                                                                      int32_t count, uint32_t misalign, const uint32_t* __restrict__ first,
                                                                      uint32_t* __restrict__ part) {
  __shared__ uint32_t waves[4];
  const uint32_t w = blockIdx.x;
  if (w >= first[count]) return;           // the one idle workgroup of a table without spans
  // the segment of span w: first[k] <= w < first[k + 1]; empty segments share their neighbour's first[] and are stepped over
  int32_t lo = 0, hi = count;              // first[lo] <= w < first[hi]
  while (hi - lo > 1) {
    const int32_t mid = lo + (hi - lo) / 2;
    if (first[mid] <= w) lo = mid; else hi = mid;
  }
  const radnet_crc32_segment s = table[lo];
  const crc_cut cut = crc_cut_of(misalign + (uint64_t)s.offset, s.length);
  const int64_t q = (int64_t)(w - first[lo]) * kCrcSpanGrains + threadIdx.x;      // this lane's grain, counted from the body's end
  uint32_t v = 0;
  if (q < cut.grains) {
    const int64_t grain_end = s.offset + s.length - cut.tail - q * kCrcGrain, grain = grain_end - kCrcGrain;
    uint32_t word[4] = {0, 0, 0, 0};
    if (grain >= s.offset) {
      const uint4 x = *reinterpret_cast<const uint4*>(buf + grain);              // aligned: the rule counts from a 16-byte boundary
      word[0] = x.x; word[1] = x.y; word[2] = x.z; word[3] = x.w;
    } else {
      // the segment's first grain: the bytes in front of the segment count as zeros and are not read
      for (int64_t i = s.offset; i < grain_end; ++i) word[(i - grain) >> 2] |= (uint32_t)buf[i] << (8 * ((i - grain) & 3));
    }
    for (int j = 0; j < 4; ++j) v = crc_word(v, word[j]);
    v = crc_times(v, kGrainWeight.v[threadIdx.x]);
  }
  v = block_xor(v, waves);
  if (threadIdx.x == 0) part[w] = v;
}

__global__ __launch_bounds__(kCrcSpanGrains) void crc32_finish_kernel(const uint8_t* __restrict__ buf, const radnet_crc32_segment* __restrict__ table,
                                                                       int32_t count, uint32_t misalign, const uint32_t* __restrict__ first,
                                                                       const uint32_t* __restrict__ part, uint32_t* __restrict__ crc,
                                                                       int32_t* __restrict__ result) {
  __shared__ uint32_t waves[4];
  const int32_t k = blockIdx.x;
  if (k >= count) return;                  // the one idle workgroup of an empty table
  const int t = threadIdx.x;
  const radnet_crc32_segment s = table[k];
  const int64_t spans = (int64_t)(first[k + 1] - first[k]);
  const uint32_t* mine = part + first[k];  // mine[e]: the span e spans in front of the body's end
  // lane t takes the spans t, t + 256, ...: Horner's rule from the farthest one down, then its own distance
  uint32_t v = 0;
  if (t < spans) {
    for (int64_t e = t + (spans - 1 - t) / kCrcSpanGrains * kCrcSpanGrains; e >= t; e -= kCrcSpanGrains) v = crc_times(v, kSpanStride) ^ mine[e];
    v = crc_times(v, kSpanWeight.v[t]);
  }
  v = block_xor(v, waves);
  // x^(8 length): the product of one factor per set bit of the length, over the lanes of a wave
  uint32_t f = t < 63 && ((s.length >> t) & 1) ? kSquares.v[t] : kCrcOne;
  for (int d = 32; d >= 1; d >>= 1) f = crc_times(f, __shfl_xor(f, d));
  if (t == 0) {
    const crc_cut cut = crc_cut_of(misalign + (uint64_t)s.offset, s.length);
    for (int64_t i = s.offset + s.length - cut.tail; i < s.offset + s.length; ++i) v = crc_byte(v, buf[i]);
    v ^= crc_times(s.init ^ 0xFFFFFFFFu, f) ^ 0xFFFFFFFFu;
    crc[k] = v;
    if (v != s.expect) {
      atomicMin(&result[0], k);
      atomicAdd(&result[1], 1);
    }
  }
}

// the scratch of one call: first[count + 1], then part[spans].  It belongs to the context and only grows; a call that needs more
// waits for the stream first, since an earlier call's launches may still be reading the block that goes.
int scratch(radnet_ctx* ctx, uint64_t bytes, uint32_t** out) {
  if (bytes > ctx->crc_ws_bytes) {
    RADNET_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->crc_ws) (void)hipFree(ctx->crc_ws);
    ctx->crc_ws = nullptr;
    ctx->crc_ws_bytes = 0;
    const uint64_t want = std::max<uint64_t>(bytes + bytes / 2, 1u << 20);
    RADNET_CHECK_HIP(ctx, hipMalloc(&ctx->crc_ws, want));
    ctx->crc_ws_bytes = want;
  }
  *out = static_cast<uint32_t*>(ctx->crc_ws);
  return RADNET_OK;
}

}  // namespace

extern "C" int radnet_crc32_segments(radnet_ctx* ctx, const uint8_t* buf, int64_t n, const radnet_crc32_segment* table_host,
                                     const radnet_crc32_segment* table_dev, int32_t count, uint32_t* crc, int32_t* result) {
  if (!ctx) return RADNET_ERR_ARG;
  if (count < 0) RADNET_FAIL(ctx, RADNET_ERR_ARG, "crc32_segments: %d segments", count);
  if (n < 0) RADNET_FAIL(ctx, RADNET_ERR_ARG, "crc32_segments: a buffer of %lld bytes", (long long)n);
  if (!result || (n > 0 && !buf) || (count > 0 && (!table_host || !table_dev || !crc)))
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "crc32_segments: null pointer (buffer %p of %lld bytes, host table %p, device table %p, %d sums %p, result %p)",
                (const void*)buf, (long long)n, (const void*)table_host, (const void*)table_dev, count, (void*)crc, (void*)result);
  if (((uintptr_t)table_dev & 7) || ((uintptr_t)crc & 3) || ((uintptr_t)result & 3))
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "crc32_segments: device table %p (8-byte aligned), sums %p, result %p (4-byte aligned)", (const void*)table_dev,
                (void*)crc, (void*)result);
  const uint32_t misalign = (uint32_t)((uintptr_t)buf & (kCrcGrain - 1));
  radnet_crc32_plan plan;
  const int rc = radnet_crc32_plan_segments(table_host, count, n, (int32_t)misalign, &plan, nullptr, ctx->err, (int32_t)sizeof(ctx->err));
  if (rc != RADNET_OK) return rc;
  uint32_t* first = nullptr;
  const int got = scratch(ctx, (uint64_t)plan.ws_bytes, &first);
  if (got != RADNET_OK) return got;
  uint32_t* part = first + count + 1;
  // always the same three launches; a grid cannot be empty, so a table without spans or without segments starts one idle workgroup
  const dim3 block(kCrcSpanGrains);
  hipLaunchKernelGGL(crc32_scan_kernel, dim3(1), block, 0, ctx->stream, table_dev, count, misalign, first, result);
  RADNET_CHECK_LAUNCH(ctx, "crc32_segments (scan)");
  hipLaunchKernelGGL(crc32_spans_kernel, dim3((unsigned)std::max<int64_t>(plan.spans, 1)), block, 0, ctx->stream, buf, table_dev, count, misalign, first, part);
  RADNET_CHECK_LAUNCH(ctx, "crc32_segments (spans)");
  hipLaunchKernelGGL(crc32_finish_kernel, dim3((unsigned)std::max(count, 1)), block, 0, ctx->stream, buf, table_dev, count, misalign, first, part, crc, result);
  RADNET_CHECK_LAUNCH(ctx, "crc32_segments (finish)");
  return RADNET_OK;
}
