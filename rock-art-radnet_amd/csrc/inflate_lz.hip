// ---- inflate of ANY zlib stream on the device: far matches by pointer jumping (contract: include/radnet_hip.h) ---------------------
// radnet_inflate_find_blocks (inflate.hip) finds the dynamic headers whatever the distances are, and a unit's length in bits and in
// bytes does not depend on the bytes in front of it, so measure, chain and emit go as for run-length streams (one kernel body,
// inflate_units_body.h).  What differs is who supplies a match's bytes: emit writes the literals into `buf` and, for every output
// byte, the position it is a copy of into `src` -- itself for a literal, an earlier position for a byte of a match.  The stream is
// then a forest of pointers to literals; radnet_inflate_lz_resolve halves every path per launch (src[i] = src[src[i]]) and
// radnet_inflate_lz_gather reads each byte from its root.  No window is carried from unit to unit, no workgroup waits on another,
// no loop spins, and the result does not depend on the order of anything.
#include "inflate_units_body.h"

namespace {

// One pointer jump per position, in place.  src is read and written by other threads meanwhile (no __restrict__): src[i] is written
// by thread i alone and every value it ever holds is an ancestor of i, so whichever value of src[s] a thread sees, old or new, is
// an ancestor of s and therefore of i.  An entry with src[i] >= i is a root by definition: both loads are guarded by `< own index`,
// so any content of src is safe and every store lowers an entry.
__global__ void __launch_bounds__(256) inflate_lz_resolve_kernel(uint32_t* src, unsigned out_len, unsigned* changed) {
  __shared__ unsigned wrote;
  if (threadIdx.x == 0) wrote = 0;
  __syncthreads();
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  bool did = false;
  if (i < out_len) {
    const unsigned s = src[i];
    if (s < i) {
      const unsigned t = src[s];
      if (t < s) src[i] = t, did = true;
    }
  }
  const unsigned n = (unsigned)__popcll(__ballot(did));
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(&wrote, n);
  __syncthreads();
  if (threadIdx.x == 0 && wrote) atomicAdd(changed, wrote);
}

// buf[i] = buf[src[i]] where src[i] < i, in place: with src flat the byte read is a root's, which nobody writes
__global__ void __launch_bounds__(256) inflate_lz_gather_kernel(const uint32_t* __restrict__ src, uint8_t* buf, unsigned out_len) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= out_len) return;
  const unsigned s = src[i];
  if (s < i) buf[i] = buf[s];
}

}  // namespace

extern "C" int radnet_inflate_lz_measure(radnet_ctx* ctx, const uint8_t* z, int64_t n, radnet_inflate_lz_unit* units, int32_t count) {
  if (!ctx) return RADNET_ERR_ARG;
  const int rc = check_stream(ctx, "inflate_lz_measure", z, n);
  if (rc != RADNET_OK) return rc;
  if (!units || count < 1) RADNET_FAIL(ctx, RADNET_ERR_ARG, "inflate_lz_measure: a null table or %d units", count);
  hipLaunchKernelGGL((inflate_units_kernel<false, true>), dim3((unsigned)count), dim3(kWave), 0, ctx->stream, z, (long long)n, (void*)units,
                     (const radnet_inflate_link*)nullptr, (uint8_t*)nullptr, (uint32_t*)nullptr, 0ll);
  RADNET_CHECK_LAUNCH(ctx, "inflate_lz_measure");
  return RADNET_OK;
}

extern "C" int radnet_inflate_lz_emit(radnet_ctx* ctx, const uint8_t* z, int64_t n, const radnet_inflate_link* links, int32_t count, uint8_t* buf,
                                      uint32_t* src, int64_t out_len) {
  if (!ctx) return RADNET_ERR_ARG;
  const int rc = check_stream(ctx, "inflate_lz_emit", z, n);
  if (rc != RADNET_OK) return rc;
  if (!links || !buf || !src || count < 1 || out_len < 0)
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "inflate_lz_emit: a null table, output or source table, %d units, or an output of %lld bytes", count, (long long)out_len);
  if (out_len >= (1ll << 31)) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "inflate_lz_emit: an output of %lld bytes (positions leave 31 bits)", (long long)out_len);
  hipLaunchKernelGGL((inflate_units_kernel<true, true>), dim3((unsigned)count), dim3(kWave), 0, ctx->stream, z, (long long)n, (void*)nullptr, links, buf, src,
                     (long long)out_len);
  RADNET_CHECK_LAUNCH(ctx, "inflate_lz_emit");
  return RADNET_OK;
}

extern "C" int radnet_inflate_lz_resolve(radnet_ctx* ctx, uint32_t* src, int64_t out_len, int32_t rounds, uint32_t* changed) {
  if (!ctx) return RADNET_ERR_ARG;
  if (!src || !changed || out_len < 0 || rounds < 1 || rounds > RADNET_INFLATE_LZ_MAX_ROUNDS)
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "inflate_lz_resolve: a null table or counters, a table of %lld entries, or %d rounds (1..%d)", (long long)out_len, rounds,
                RADNET_INFLATE_LZ_MAX_ROUNDS);
  if (out_len >= (1ll << 31)) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "inflate_lz_resolve: a table of %lld entries (positions leave 31 bits)", (long long)out_len);
  if (out_len == 0) return RADNET_OK;
  const unsigned blocks = (unsigned)((out_len + 255) / 256);
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(inflate_lz_resolve_kernel, dim3(blocks), dim3(256), 0, ctx->stream, src, (unsigned)out_len, changed + r);
    RADNET_CHECK_LAUNCH(ctx, "inflate_lz_resolve");
  }
  return RADNET_OK;
}

extern "C" int radnet_inflate_lz_gather(radnet_ctx* ctx, const uint32_t* src, uint8_t* buf, int64_t out_len) {
  if (!ctx) return RADNET_ERR_ARG;
  if (!src || !buf || out_len < 0) RADNET_FAIL(ctx, RADNET_ERR_ARG, "inflate_lz_gather: a null table or buffer, or %lld bytes", (long long)out_len);
  if (out_len >= (1ll << 31)) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "inflate_lz_gather: %lld bytes (positions leave 31 bits)", (long long)out_len);
  if (out_len == 0) return RADNET_OK;
  hipLaunchKernelGGL(inflate_lz_gather_kernel, dim3((unsigned)((out_len + 255) / 256)), dim3(256), 0, ctx->stream, src, buf, (unsigned)out_len);
  RADNET_CHECK_LAUNCH(ctx, "inflate_lz_gather");
  return RADNET_OK;
}
