// ---- the IDAT payloads of an uploaded PNG file joined into its zlib stream (contract: include/radnet_hip.h, radnet_png_join_u8) ----------
// The unit of work is the OUTPUT grain -- the 16 bytes between two 16-byte boundaries of device memory, clipped to the stream -- so a
// file of one large IDAT and one of thousands of 8 KiB ones both fill the device, every byte has exactly one writer, and a full grain
// leaves in one aligned 16-byte store.  Where the bytes come from a lane finds by bisection over the table's dst column; the chunk
// headers and CRC fields between the payloads (12 bytes in a file) make src - dst anything mod 16, so the reads are byte loads: the
// simplest form that is right at every address and never touches a byte outside the file.
// One launch, no scratch memory, no atomics, no flags; no workgroup waits on another; every loop is bounded by the grain or log2(count).
#include "radnet_internal.h"

namespace {

constexpr int kJoinGrain = RADNET_PNG_JOIN_GRAIN;
constexpr int kJoinSpanGrains = RADNET_PNG_JOIN_SPAN_GRAINS;
static_assert(kJoinGrain == 16, "a grain is one uint4 store");

__global__ __launch_bounds__(kJoinSpanGrains) void png_join_kernel(const uint8_t* __restrict__ file, const radnet_png_piece* __restrict__ table,
                                                                    int32_t count, uint8_t* __restrict__ out, int64_t n, uint32_t misalign) {
  const int64_t grain = (int64_t)blockIdx.x * kJoinSpanGrains + threadIdx.x;
  const int64_t first = grain * kJoinGrain - (int64_t)misalign;      // out + first stands on a 16-byte boundary; negative for the first grain alone
  const int64_t lo = first > 0 ? first : 0, hi = first + kJoinGrain < n ? first + kJoinGrain : n;
  if (lo >= hi) return;
  uint64_t word[2] = {0, 0};               // the grain's bytes, byte i of the grain in bits 8 (i & 7) of word[i >> 3]
  int64_t p = lo;
  int32_t from = 0;                        // dst[from] <= p
  for (int round = 0; round < kJoinGrain && p < hi; ++round) {      // every round takes at least one byte
    // the piece of byte p: the last k with dst_k <= p.  p < n, so that piece is not empty and p lies inside it
    int32_t a = from, b = count;           // dst[a] <= p < dst[b] (dst[count] = n)
    while (b - a > 1) {
      const int32_t mid = a + (b - a) / 2;
      if (table[mid].dst <= p) a = mid; else b = mid;
    }
    const radnet_png_piece piece = table[a];
    const int64_t piece_end = piece.dst + piece.length, stop = piece_end < hi ? piece_end : hi;
    const uint8_t* s = file + piece.src + (p - piece.dst);
    for (; p < stop; ++p, ++s) {
      const uint32_t i = (uint32_t)(p - first);
      const uint64_t v = *s;
      if (i < 8) word[0] |= v << (8 * i); else word[1] |= v << (8 * (i - 8));
    }
    from = a + 1 < count ? a + 1 : a;      // when the grain goes on, p = dst[a + 1]
  }
  if (hi - lo == kJoinGrain) {
    *reinterpret_cast<uint4*>(out + first) = make_uint4((uint32_t)word[0], (uint32_t)(word[0] >> 32), (uint32_t)word[1], (uint32_t)(word[1] >> 32));
  } else {
    for (int64_t q = lo; q < hi; ++q) {    // a clipped grain: the stream's first or last
      const uint32_t i = (uint32_t)(q - first);
      out[q] = (uint8_t)((i < 8 ? word[0] >> (8 * i) : word[1] >> (8 * (i - 8))) & 0xFF);
    }
  }
}

}  // namespace

extern "C" int radnet_png_join_u8(radnet_ctx* ctx, const uint8_t* file, int64_t file_len, const radnet_png_piece* table_host,
                                  const radnet_png_piece* table_dev, int32_t count, uint8_t* out, int64_t n) {
  if (!ctx) return RADNET_ERR_ARG;
  if ((count > 0 && !table_host) || (n > 0 && (!file || !out || !table_dev)))
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "png_join: null pointer (file %p of %lld bytes, host table %p, device table %p of %d pieces, output %p of %lld bytes)",
                (const void*)file, (long long)file_len, (const void*)table_host, (const void*)table_dev, count, (void*)out, (long long)n);
  if ((uintptr_t)table_dev & 7) RADNET_FAIL(ctx, RADNET_ERR_ARG, "png_join: device table %p (8-byte aligned)", (const void*)table_dev);
  const uint32_t misalign = (uint32_t)((uintptr_t)out & (kJoinGrain - 1));
  radnet_png_join_plan plan;
  const int rc = radnet_png_plan_join(table_host, count, file_len, n, (int32_t)misalign, &plan, nullptr, ctx->err, (int32_t)sizeof(ctx->err));
  if (rc != RADNET_OK) return rc;
  if (n == 0) return RADNET_OK;            // nothing to write, whatever the pointers
  // n > 0 here, so file_len > 0 too (the pieces hold n bytes of the file) and both ranges are real
  if ((uintptr_t)out < (uintptr_t)file + (uint64_t)file_len && (uintptr_t)file < (uintptr_t)out + (uint64_t)n)
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "png_join: the output %p of %lld bytes overlaps the file %p of %lld bytes", (void*)out, (long long)n,
                (const void*)file, (long long)file_len);
  hipLaunchKernelGGL(png_join_kernel, dim3((unsigned)plan.spans), dim3(kJoinSpanGrains), 0, ctx->stream, file, table_dev, count, out, n, misalign);
  RADNET_CHECK_LAUNCH(ctx, "png_join");
  return RADNET_OK;
}
