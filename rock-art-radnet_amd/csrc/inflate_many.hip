// ---- inflate of MANY zlib streams in one pass (contract: include/radnet_hip.h, radnet_inflate_stream) --------------------------------
// The streams of a batch stand in one device buffer and inflate into one output.  The search, the unit decoder and the emit are
// those of inflate.hip / inflate_lz.hip (ONE body, inflate_units_body.h); what this unit adds is the stream table and THE BOUNDARY
// RULE: a bit or a unit belongs to the stream that holds it, reads nothing behind that stream's end and writes nothing outside that
// stream's output.  A wave finds its stream by bisection over the device table (a uniform walk of log2(count) loads); the search,
// which has a thread per bit, bisects once per workgroup and keeps the few entries its 32 bytes can touch in LDS.
// wave64, integers only, no inline assembly, no waits between workgroups; the only atomic is the search's integer append.
#include "inflate_units_body.h"

namespace {

constexpr int kFindThreads = 256;                      // one bit each: 32 bytes of z per workgroup
constexpr int kFindStage = 16;                         // table entries a workgroup keeps: the one at or in front of its first byte and those that
                                                       // begin in its other 31 bytes, 3 bytes apart at least (radnet_inflate_streams_check): 1 + 11
static_assert(kFindStage >= 1 + (kFindThreads / 8 - 1 + 2) / 3, "every stream that touches a workgroup's bytes is staged");

// the last stream with z_offset <= byte, or -1: the offsets ascend
__device__ __forceinline__ int stream_at_or_before(const radnet_inflate_stream* __restrict__ streams, int count, long long byte) {
  int lo = -1, hi = count;                             // z_offset[lo] <= byte < z_offset[hi]
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (streams[mid].z_offset <= byte) lo = mid; else hi = mid;
  }
  return lo;
}

// the span of the stream that holds the global bit `start`, or the empty span of a bit in a gap (UnitSpan, inflate_units_body.h)
__device__ __forceinline__ UnitSpan span_of(const uint8_t* __restrict__ z, const radnet_inflate_stream* __restrict__ streams, int count, unsigned start) {
  const long long byte = (long long)(start >> 3);
  const int k = stream_at_or_before(streams, count, byte);
  if (k >= 0) {
    const radnet_inflate_stream s = streams[k];
    if (byte < s.z_offset + s.n) return UnitSpan{z + s.z_offset, (long long)s.n, (unsigned)(8 * s.z_offset), (long long)s.out_offset, (long long)(s.out_offset + s.expected)};
  }
  return UnitSpan{z, 0ll, start, 0ll, 0ll};
}

template <bool kEmit, bool kLz>
__global__ void __launch_bounds__(kWave) inflate_units_many_kernel(const uint8_t* __restrict__ z, const radnet_inflate_stream* __restrict__ streams, int n_streams,
                                                                   void* __restrict__ units, const radnet_inflate_link* __restrict__ links,
                                                                   uint8_t* __restrict__ out, uint32_t* __restrict__ src) {
  __shared__ UnitShared sh;
  const unsigned start = unit_start_bit<kEmit, kLz>(units, links, (int)blockIdx.x);
  inflate_unit<kEmit, kLz>(sh, span_of(z, streams, n_streams, start), units, links, out, src);
}

__global__ void __launch_bounds__(kFindThreads) inflate_find_many_kernel(const uint8_t* __restrict__ z, const radnet_inflate_stream* __restrict__ streams,
                                                                         int n_streams, unsigned* __restrict__ cand, int cand_cap,
                                                                         unsigned* __restrict__ count) {
  __shared__ long long at[kFindStage], len[kFindStage];
  const long long byte0 = (long long)blockIdx.x * (kFindThreads / 8);
  const int k0 = max(stream_at_or_before(streams, n_streams, byte0), 0);      // uniform over the workgroup
  const int staged = min(kFindStage, n_streams - k0);
  if ((int)threadIdx.x < staged) at[threadIdx.x] = streams[k0 + threadIdx.x].z_offset, len[threadIdx.x] = streams[k0 + threadIdx.x].n;
  __syncthreads();
  const u64 p = 8ull * (u64)byte0 + threadIdx.x;
  const long long byte = (long long)(p >> 3);
  int lo = -1, hi = staged;                            // at[lo] <= byte < at[hi]
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (at[mid] <= byte) lo = mid; else hi = mid;
  }
  if (lo < 0 || byte >= at[lo] + len[lo]) return;      // in front of every stream, in a gap, or behind the last one
  const u64 q = p - 8ull * (u64)at[lo], nbits = 8ull * (u64)len[lo];
  if (q < 16) return;                                  // the zlib header: a stream's search starts at its bit 16
  if (!dynamic_header_at(GlobalBits{z + at[lo], len[lo]}, q, nbits)) return;
  const unsigned idx = atomicAdd(count, 1u);
  if (idx < (unsigned)cand_cap) cand[idx] = (unsigned)p;
}

int check_table(radnet_ctx* ctx, const char* what, const void* z, int64_t z_len, const radnet_inflate_stream* streams_host,
                const radnet_inflate_stream* streams_dev, int32_t n_streams, int64_t out_len) {
  if (!z || !streams_host || !streams_dev || ((uintptr_t)streams_dev & 7))
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "%s: a null buffer or table (z %p, host table %p, device table %p, 8-byte aligned)", what, z, (const void*)streams_host,
                (const void*)streams_dev);
  char msg[256];
  const int rc = radnet_inflate_streams_check(streams_host, n_streams, z_len, out_len, nullptr, msg, (int32_t)sizeof msg);
  if (rc != RADNET_OK) RADNET_FAIL(ctx, rc, "%s: %s", what, msg);
  return RADNET_OK;
}

// the end of the last stream's output: what the entries without an output check the table against
int64_t output_end(const radnet_inflate_stream* streams_host, int32_t n_streams) {
  if (!streams_host || n_streams < 1 || n_streams > RADNET_INFLATE_MANY_MAX_STREAMS) return 0;      // the check speaks
  int64_t end = 0;
  for (int32_t k = 0; k < n_streams; ++k) {
    const radnet_inflate_stream& s = streams_host[k];
    if (s.out_offset >= 0 && s.expected >= 0 && s.expected <= INT64_MAX - s.out_offset && s.out_offset + s.expected > end) end = s.out_offset + s.expected;
  }
  return end;
}

template <bool kLz, class Unit>
int measure_many(radnet_ctx* ctx, const char* what, const uint8_t* z, int64_t z_len, const radnet_inflate_stream* streams_host,
                 const radnet_inflate_stream* streams_dev, int32_t n_streams, Unit* units, int32_t count) {
  if (!ctx) return RADNET_ERR_ARG;
  const int rc = check_table(ctx, what, z, z_len, streams_host, streams_dev, n_streams, output_end(streams_host, n_streams));
  if (rc != RADNET_OK) return rc;
  if (!units || count < 1) RADNET_FAIL(ctx, RADNET_ERR_ARG, "%s: a null table or %d units", what, count);
  hipLaunchKernelGGL((inflate_units_many_kernel<false, kLz>), dim3((unsigned)count), dim3(kWave), 0, ctx->stream, z, streams_dev, (int)n_streams, (void*)units,
                     (const radnet_inflate_link*)nullptr, (uint8_t*)nullptr, (uint32_t*)nullptr);
  RADNET_CHECK_LAUNCH(ctx, what);
  return RADNET_OK;
}

template <bool kLz>
int emit_many(radnet_ctx* ctx, const char* what, const uint8_t* z, int64_t z_len, const radnet_inflate_stream* streams_host,
              const radnet_inflate_stream* streams_dev, int32_t n_streams, const radnet_inflate_link* links, int32_t count, uint8_t* out, uint32_t* src,
              int64_t out_len) {
  if (!ctx) return RADNET_ERR_ARG;
  if (out_len < 0) RADNET_FAIL(ctx, RADNET_ERR_ARG, "%s: an output of %lld bytes", what, (long long)out_len);
  const int rc = check_table(ctx, what, z, z_len, streams_host, streams_dev, n_streams, out_len);
  if (rc != RADNET_OK) return rc;
  if (!links || !out || (kLz && !src) || count < 1) RADNET_FAIL(ctx, RADNET_ERR_ARG, "%s: a null table, output or source table, or %d units", what, count);
  hipLaunchKernelGGL((inflate_units_many_kernel<true, kLz>), dim3((unsigned)count), dim3(kWave), 0, ctx->stream, z, streams_dev, (int)n_streams, (void*)nullptr,
                     links, out, src);
  RADNET_CHECK_LAUNCH(ctx, what);
  return RADNET_OK;
}

}  // namespace

extern "C" int radnet_inflate_find_blocks_many(radnet_ctx* ctx, const uint8_t* z, int64_t z_len, const radnet_inflate_stream* streams_host,
                                               const radnet_inflate_stream* streams_dev, int32_t n_streams, uint32_t* cand, int32_t cand_cap,
                                               uint32_t* count) {
  if (!ctx) return RADNET_ERR_ARG;
  const int rc = check_table(ctx, "inflate_find_blocks_many", z, z_len, streams_host, streams_dev, n_streams, output_end(streams_host, n_streams));
  if (rc != RADNET_OK) return rc;
  if (!cand || !count || cand_cap < 0) RADNET_FAIL(ctx, RADNET_ERR_ARG, "inflate_find_blocks_many: null candidates or count, or a capacity of %d", cand_cap);
  const unsigned blocks = (unsigned)((8 * z_len + kFindThreads - 1) / kFindThreads);      // z_len >= 3 here: a stream lies inside it
  hipLaunchKernelGGL(inflate_find_many_kernel, dim3(blocks), dim3(kFindThreads), 0, ctx->stream, z, streams_dev, (int)n_streams, cand, (int)cand_cap, count);
  RADNET_CHECK_LAUNCH(ctx, "inflate_find_blocks_many");
  return RADNET_OK;
}

extern "C" int radnet_inflate_rle_measure_many(radnet_ctx* ctx, const uint8_t* z, int64_t z_len, const radnet_inflate_stream* streams_host,
                                               const radnet_inflate_stream* streams_dev, int32_t n_streams, radnet_inflate_unit* units, int32_t count) {
  return measure_many<false>(ctx, "inflate_rle_measure_many", z, z_len, streams_host, streams_dev, n_streams, units, count);
}

extern "C" int radnet_inflate_lz_measure_many(radnet_ctx* ctx, const uint8_t* z, int64_t z_len, const radnet_inflate_stream* streams_host,
                                              const radnet_inflate_stream* streams_dev, int32_t n_streams, radnet_inflate_lz_unit* units, int32_t count) {
  return measure_many<true>(ctx, "inflate_lz_measure_many", z, z_len, streams_host, streams_dev, n_streams, units, count);
}

extern "C" int radnet_inflate_rle_emit_many(radnet_ctx* ctx, const uint8_t* z, int64_t z_len, const radnet_inflate_stream* streams_host,
                                            const radnet_inflate_stream* streams_dev, int32_t n_streams, const radnet_inflate_link* links, int32_t count,
                                            uint8_t* out, int64_t out_len) {
  return emit_many<false>(ctx, "inflate_rle_emit_many", z, z_len, streams_host, streams_dev, n_streams, links, count, out, nullptr, out_len);
}

extern "C" int radnet_inflate_lz_emit_many(radnet_ctx* ctx, const uint8_t* z, int64_t z_len, const radnet_inflate_stream* streams_host,
                                           const radnet_inflate_stream* streams_dev, int32_t n_streams, const radnet_inflate_link* links, int32_t count,
                                           uint8_t* buf, uint32_t* src, int64_t out_len) {
  return emit_many<true>(ctx, "inflate_lz_emit_many", z, z_len, streams_host, streams_dev, n_streams, links, count, buf, src, out_len);
}
