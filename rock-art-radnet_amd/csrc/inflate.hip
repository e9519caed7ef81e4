// ---- inflate of run-length zlib streams on the device: speculative block search (contract: include/radnet_hip.h) -----------------
// The reader's compressed IDAT stream goes up instead of the inflated one.  radnet_inflate_find_blocks tries a dynamic block header
// at every bit offset (one thread each; almost all end at BTYPE or at the code-length code's Kraft sum), radnet_inflate_rle_measure
// decodes the unit behind every candidate without output, the host chains the units (inflate_plan.cpp) and radnet_inflate_rle_emit
// decodes the chained ones again into their places.  measure and emit are ONE kernel body (inflate_units_body.h, shared with
// inflate_lz.hip): a workgroup is one wave and takes one unit; the compressed bytes pass through a window in LDS, the code tables
// stand in LDS (a direct table for codes of at most kPrimaryBits bits, the canonical count / sorted-symbol walk for longer ones),
// lane 0 decodes a batch of tokens, the wave sums their lengths by prefix and all lanes expand them.  wave64, integers only, no
// inline assembly, no waits between workgroups.
#include "inflate_units_body.h"

namespace {

__global__ void __launch_bounds__(256) inflate_find_kernel(const uint8_t* __restrict__ z, long long n, u64 first_bit, unsigned* __restrict__ cand, int cand_cap,
                                                           unsigned* __restrict__ count) {
  const u64 nbits = 8ull * (u64)n, p = first_bit + (u64)blockIdx.x * 256 + threadIdx.x;
  if (p >= nbits) return;
  if (!dynamic_header_at(GlobalBits{z, n}, p, nbits)) return;
  const unsigned idx = atomicAdd(count, 1u);
  if (idx < (unsigned)cand_cap) cand[idx] = (unsigned)p;
}

struct ColumnPasses {
  long long offset[7];
  int rows[7], rowbytes[7], passes;
};

__global__ void __launch_bounds__(256) png_column_kernel(const uint8_t* __restrict__ stream, const ColumnPasses t, int total, uint8_t* __restrict__ column) {
  const int k = (int)(blockIdx.x * 256 + threadIdx.x);
  if (k >= total) return;
  int r = k, p = 0;
  while (p < t.passes - 1 && r >= t.rows[p]) r -= t.rows[p], ++p;
  column[k] = stream[t.offset[p] + (long long)r * (1 + t.rowbytes[p])];
}

}  // namespace

extern "C" int radnet_inflate_find_blocks(radnet_ctx* ctx, const uint8_t* z, int64_t n, int64_t first_bit, uint32_t* cand, int32_t cand_cap,
                                          uint32_t* count) {
  if (!ctx) return RADNET_ERR_ARG;
  const int rc = check_stream(ctx, "inflate_find_blocks", z, n);
  if (rc != RADNET_OK) return rc;
  if (!cand || !count || cand_cap < 0 || first_bit < 0 || first_bit >= 8 * n)
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "inflate_find_blocks: null candidates or count, a capacity of %d, or first_bit %lld outside the %lld bits", cand_cap,
                (long long)first_bit, (long long)(8 * n));
  const unsigned blocks = (unsigned)((8 * n - first_bit + 255) / 256);
  hipLaunchKernelGGL(inflate_find_kernel, dim3(blocks), dim3(256), 0, ctx->stream, z, (long long)n, (u64)first_bit, cand, (int)cand_cap, count);
  RADNET_CHECK_LAUNCH(ctx, "inflate_find_blocks");
  return RADNET_OK;
}

extern "C" int radnet_inflate_rle_measure(radnet_ctx* ctx, const uint8_t* z, int64_t n, radnet_inflate_unit* units, int32_t count) {
  if (!ctx) return RADNET_ERR_ARG;
  const int rc = check_stream(ctx, "inflate_rle_measure", z, n);
  if (rc != RADNET_OK) return rc;
  if (!units || count < 1) RADNET_FAIL(ctx, RADNET_ERR_ARG, "inflate_rle_measure: a null table or %d units", count);
  hipLaunchKernelGGL((inflate_units_kernel<false, false>), dim3((unsigned)count), dim3(kWave), 0, ctx->stream, z, (long long)n, (void*)units,
                     (const radnet_inflate_link*)nullptr, (uint8_t*)nullptr, (uint32_t*)nullptr, 0ll);
  RADNET_CHECK_LAUNCH(ctx, "inflate_rle_measure");
  return RADNET_OK;
}

extern "C" int radnet_inflate_rle_emit(radnet_ctx* ctx, const uint8_t* z, int64_t n, const radnet_inflate_link* links, int32_t count, uint8_t* out,
                                       int64_t out_len) {
  if (!ctx) return RADNET_ERR_ARG;
  const int rc = check_stream(ctx, "inflate_rle_emit", z, n);
  if (rc != RADNET_OK) return rc;
  if (!links || !out || count < 1 || out_len < 0)
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "inflate_rle_emit: a null table or output, %d units, or an output of %lld bytes", count, (long long)out_len);
  hipLaunchKernelGGL((inflate_units_kernel<true, false>), dim3((unsigned)count), dim3(kWave), 0, ctx->stream, z, (long long)n, (void*)nullptr, links, out,
                     (uint32_t*)nullptr, (long long)out_len);
  RADNET_CHECK_LAUNCH(ctx, "inflate_rle_emit");
  return RADNET_OK;
}

extern "C" int radnet_png_gather_column_u8(radnet_ctx* ctx, const uint8_t* stream, int64_t stream_len, const int64_t* offsets, const int32_t* rows,
                                           const int32_t* rowbytes, int32_t passes, uint8_t* column) {
  if (!ctx) return RADNET_ERR_ARG;
  if (!stream || !offsets || !rows || !rowbytes || !column || passes < 1 || passes > 7)
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "png_gather_column: a null pointer or %d passes (1..7)", passes);
  ColumnPasses t = {};
  long long total = 0;
  for (int p = 0; p < passes; ++p) {
    if (rows[p] < 1 || rowbytes[p] < 1 || offsets[p] < 0 || offsets[p] + (int64_t)rows[p] * (1 + (int64_t)rowbytes[p]) > stream_len)
      RADNET_FAIL(ctx, RADNET_ERR_ARG, "png_gather_column: pass %d (%d rows of 1 + %d bytes at %lld) does not lie in the %lld bytes", p, rows[p], rowbytes[p],
                  (long long)offsets[p], (long long)stream_len);
    t.offset[p] = offsets[p], t.rows[p] = rows[p], t.rowbytes[p] = rowbytes[p];
    total += rows[p];
  }
  if (total > 0x7fffffffll) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "png_gather_column: %lld rows", total);
  t.passes = passes;
  hipLaunchKernelGGL(png_column_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, stream, t, (int)total, column);
  RADNET_CHECK_LAUNCH(ctx, "png_gather_column_u8");
  return RADNET_OK;
}
