// ---- deflate of the PNG scanline stream on the device: run-length tokens, one Huffman code (contract: include/radnet_hip.h) -------
// The writer's stream (radnet_png_filter_rows_u8) never leaves the device uncompressed: radnet_deflate_rle_scan_u8 counts the symbols
// and sums the Adler-32 parts, the host builds ONE code from the 286 counts (deflate_plan.cpp), radnet_deflate_rle_emit_u8 writes one
// deflate block per chunk and radnet_deflate_pack moves the blocks together.  Both passes tokenise with the same device function,
// tile by tile: a workgroup of 256 threads holds a tile of RADNET_DEFLATE_TILE bytes in LDS, 16 consecutive positions per thread.  A
// position's token follows from the first and the last position of its run, which come from a prefix maximum of the run starts and
// a suffix minimum of the run ends over the workgroup; bit offsets from a prefix sum.  wave64, integers only, no inline assembly.
#include "deflate_device.h"

namespace {

using namespace radnet_deflate_device;            // the cut, length symbols, tile load, prefix sum, bit window, Adler parts
constexpr int kNone = 1 << 20;
// the bits one tile can add (15 per position at most: a literal's longest code; a match spends at most 25 on three positions) behind
// a header or a carried partial word, and the word a token may spill into
constexpr int kWindowWords = kHeaderWords + kTile * kMaxLen / 32 + 4;

enum { kSkip = 0, kLiteral = 1, kMatch = 2 };

// per thread: the largest `start` of the threads in front of it (-1: none) and the smallest `end` of the threads behind it (kNone)
__device__ __forceinline__ void scan_runs(int start, int end, int tid, int* sh, int& start_in, int& end_in) {
  const int lane = tid & 63, wave = tid >> 6;
  int a = start, b = end;
  for (int d = 1; d < 64; d <<= 1) {
    const int oa = __shfl_up(a, d, 64), ob = __shfl_down(b, d, 64);
    if (lane >= d) a = max(a, oa);
    if (lane + d < 64) b = min(b, ob);
  }
  if (lane == 63) sh[wave] = a;
  if (lane == 0) sh[4 + wave] = b;
  int ea = __shfl_up(a, 1, 64), eb = __shfl_down(b, 1, 64);
  if (lane == 0) ea = -1;
  if (lane == 63) eb = kNone;
  __syncthreads();
  for (int w = 0; w < wave; ++w) ea = max(ea, sh[w]);
  for (int w = wave + 1; w < kThreads / 64; ++w) eb = min(eb, sh[4 + w]);
  start_in = ea;
  end_in = eb;
}

// THE TOKEN RULE on a tile of len bytes in LDS: f(k, i, byte, kind, match_length) for each of the thread's positions i = 16 tid + k
// below len, in order.  Every thread of the workgroup calls this (it holds a barrier); sh: 8 ints, free again at the caller's next
// barrier.
template <typename F>
__device__ __forceinline__ void tile_tokens(const uint8_t* tile, int len, int tid, int* sh, F&& f) {
  const int i0 = tid * kPer;
  const uint4 q = reinterpret_cast<const uint4*>(tile)[tid];
  const unsigned words[4] = {q.x, q.y, q.z, q.w};
  int b[kPer + 2];                                // the byte in front of the thread's positions, theirs, the byte behind; -1: none
  b[0] = (i0 > 0 && i0 < len) ? tile[i0 - 1] : -1;
  b[kPer + 1] = i0 + kPer < len ? tile[i0 + kPer] : -1;
#pragma unroll
  for (int k = 0; k < kPer; ++k) b[k + 1] = i0 + k < len ? (int)((words[k >> 2] >> (8 * (k & 3))) & 255u) : -1;
  unsigned starts = 0, ends = 0;
  int last_start = -1, first_end = kNone;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    if (i0 + k < len) {
      if (b[k + 1] != b[k]) starts |= 1u << k, last_start = i0 + k;
      if (b[k + 1] != b[k + 2]) {
        ends |= 1u << k;
        if (first_end == kNone) first_end = i0 + k;
      }
    }
  }
  int start_in, end_in;
  scan_runs(last_start, first_end, tid, sh, start_in, end_in);
  int run_end[kPer];
  int cur = end_in;
#pragma unroll
  for (int k = kPer - 1; k >= 0; --k) {
    if ((ends >> k) & 1) cur = i0 + k;
    run_end[k] = cur;
  }
  cur = start_in;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const int i = i0 + k;
    if (i < len) {
      if ((starts >> k) & 1) cur = i;
      const int j = i - cur, rest_all = run_end[k] - cur;      // position inside the run; the run's bytes behind its literal
      int kind = kLiteral, mlen = 0;
      if (j > 0) {
        const int full = rest_all / 258 * 258, r = rest_all - full, t = j - 1;
        if (t < full) {
          kind = t % 258 == 0 ? kMatch : kSkip;
          mlen = 258;
        } else if (r >= 3) {
          kind = t == full ? kMatch : kSkip;
          mlen = r;
        }
      }
      f(k, i, b[k + 1], kind, mlen);
    }
  }
}

__global__ void __launch_bounds__(kThreads) deflate_scan_kernel(const uint8_t* __restrict__ stream, long long n, unsigned* __restrict__ hist,
                                                                unsigned long long* __restrict__ parts) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[kTile];
  __shared__ unsigned counts[kSymbols];
  __shared__ int sh[8];
  __shared__ unsigned long long sums[kThreads / 64][2];
  const int tid = (int)threadIdx.x;
  const long long base = (long long)blockIdx.x * kChunk;
  const int len = (int)min((long long)kChunk, n - base);
  for (int s = tid; s < kSymbols; s += kThreads) counts[s] = s == kEob ? 1u : 0u;
  unsigned long long s1 = 0, s2 = 0;
  for (int t0 = 0; t0 < len; t0 += kTile) {
    const int tl = min(kTile, len - t0);
    __syncthreads();                              // the tile's readers of the round before are done; `counts` is set
    load_tile(tile, stream + base + t0, tl, tid);
    __syncthreads();
    tile_tokens(tile, tl, tid, sh, [&](int, int i, int byte, int kind, int mlen) {
      adler_add(s1, s2, len, t0 + i, byte);
      if (kind == kLiteral) {
        atomicAdd(&counts[byte], 1u);
      } else if (kind == kMatch) {
        int symbol, eb, ev;
        length_symbol(mlen, symbol, eb, ev);
        atomicAdd(&counts[symbol], 1u);
      }
    });
  }
  adler_store(s1, s2, tid, sums, parts, (long long)blockIdx.x);      // holds the barrier behind which `counts` is complete
  for (int s = tid; s < kSymbols; s += kThreads)
    if (counts[s]) atomicAdd(&hist[s], counts[s]);
}

struct EmitTables {
  uint32_t code[kSymbols];                        // bits | length << 16
  uint32_t header[kHeaderWords];                  // the header's bits, zero behind them
};

__global__ void __launch_bounds__(kThreads) deflate_emit_kernel(const uint8_t* __restrict__ stream, long long n, const EmitTables tables, int header_nbits,
                                                                int dist_nbits, uint8_t* __restrict__ pieces, long long piece_cap,
                                                                unsigned* __restrict__ sizes) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[kTile];
  __shared__ unsigned window[kWindowWords];       // the piece's bits from word `flushed` on
  __shared__ unsigned rcode[kSymbols];            // the code bit-reversed (the stream takes a code's most significant bit first) | length << 16
  __shared__ int sh[8], sh_sum[4], end_bits;
  const int tid = (int)threadIdx.x;
  const long long base = (long long)blockIdx.x * kChunk;
  const int len = (int)min((long long)kChunk, n - base);
  const bool last = base + len == n;
  uint8_t* piece = pieces + (long long)blockIdx.x * piece_cap;
  for (int s = tid; s < kSymbols; s += kThreads) {
    const unsigned c = tables.code[s], l = c >> 16;
    rcode[s] = l ? (__brev(c & 0xffffu) >> (32 - l)) | (l << 16) : 0u;
  }
  for (int w = tid; w < kWindowWords; w += kThreads) window[w] = w < kHeaderWords ? tables.header[w] | (w == 0 && last ? 1u : 0u) : 0u;
  int bitpos = header_nbits, flushed = 0;         // bits of the piece so far; whole words of it already in global memory
  for (int t0 = 0; t0 < len; t0 += kTile) {
    const int tl = min(kTile, len - t0);
    __syncthreads();
    load_tile(tile, stream + base + t0, tl, tid);
    __syncthreads();
    unsigned value[kPer];
    int nbits[kPer], mine = 0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) value[k] = 0, nbits[k] = 0;
    tile_tokens(tile, tl, tid, sh, [&](int k, int, int byte, int kind, int mlen) {
      if (kind == kLiteral) {
        const unsigned c = rcode[byte];
        value[k] = c & 0xffffu, nbits[k] = (int)(c >> 16);
      } else if (kind == kMatch) {
        int symbol, eb, ev;
        length_symbol(mlen, symbol, eb, ev);
        const unsigned c = rcode[symbol], l = c >> 16;
        value[k] = (c & 0xffffu) | ((unsigned)ev << l), nbits[k] = (int)l + eb + dist_nbits;
      }
      mine += nbits[k];
    });
    int total;
    int p = bitpos - 32 * flushed + scan_sum(mine, tid, sh_sum, total);
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      put_bits(window, p, value[k], nbits[k]);
      p += nbits[k];
    }
    bitpos += total;
    __syncthreads();
    flushed = flush_window(window, piece, bitpos, flushed, tid);      // whole words out, the partial one to the front
  }
  finish_piece(window, piece, bitpos, flushed, rcode[kEob], last, &end_bits, &sizes[blockIdx.x], tid);
}

__global__ void __launch_bounds__(kThreads) deflate_pack_kernel(const uint8_t* __restrict__ pieces, long long piece_cap, const unsigned* __restrict__ sizes,
                                                                int count, uint8_t* __restrict__ out, long long out_cap,
                                                                unsigned long long* __restrict__ total) {
  __shared__ unsigned long long sums[kThreads / 64];
  const int tid = (int)threadIdx.x, c = (int)blockIdx.x;
  unsigned long long before = 0;
  for (int i = tid; i < c; i += kThreads) before += sizes[i];
  for (int d = 32; d > 0; d >>= 1) before += __shfl_down(before, d, 64);
  if ((tid & 63) == 0) sums[tid >> 6] = before;
  __syncthreads();
  const long long offset = (long long)(sums[0] + sums[1] + sums[2] + sums[3]);
  const long long size = min((long long)sizes[c], piece_cap);
  if (c == count - 1 && tid == 0) *total = (unsigned long long)(offset + size);
  const long long stop = min(size, out_cap - offset);      // negative when the piece starts beyond out_cap: nothing is copied
  const uint8_t* piece = pieces + (long long)c * piece_cap;
  for (long long i = tid; i < stop; i += kThreads) out[offset + i] = piece[i];
}

}  // namespace

extern "C" int radnet_deflate_rle_scan_u8(radnet_ctx* ctx, const uint8_t* stream, int64_t n, uint32_t* hist, uint64_t* adler_parts) {
  if (!ctx) return RADNET_ERR_ARG;
  if (!stream || !hist || !adler_parts || n < 1)
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "deflate_rle_scan: null stream, histogram or Adler parts, or an empty stream (%lld bytes)", (long long)n);
  if (n >= (1ll << 32)) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "deflate_rle_scan: %lld bytes (a count could pass 2^32)", (long long)n);
  const unsigned chunks = (unsigned)((n + kChunk - 1) / kChunk);
  hipLaunchKernelGGL(deflate_scan_kernel, dim3(chunks), dim3(kThreads), 0, ctx->stream, stream, (long long)n, hist,
                     reinterpret_cast<unsigned long long*>(adler_parts));
  RADNET_CHECK_LAUNCH(ctx, "deflate_rle_scan_u8");
  return RADNET_OK;
}

extern "C" int radnet_deflate_rle_emit_u8(radnet_ctx* ctx, const uint8_t* stream, int64_t n, const radnet_deflate_code* code, const uint8_t* header_bits,
                                          int32_t header_nbits, int32_t dist_nbits, uint8_t* pieces, int64_t piece_cap, uint32_t* sizes) {
  if (!ctx) return RADNET_ERR_ARG;
  if (!stream || !code || !header_bits || !pieces || !sizes || n < 1)
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "deflate_rle_emit: null stream, code, header, pieces or sizes, or an empty stream (%lld bytes)", (long long)n);
  if (header_nbits < 3 || header_nbits > RADNET_DEFLATE_HEADER_MAX_BITS)
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "deflate_rle_emit: a block header of %d bits (3..%d)", header_nbits, RADNET_DEFLATE_HEADER_MAX_BITS);
  if (dist_nbits < 0 || dist_nbits > kMaxLen) RADNET_FAIL(ctx, RADNET_ERR_ARG, "deflate_rle_emit: a distance code of %d bits (0..15)", dist_nbits);
  for (int s = 0; s < kSymbols; ++s)
    if (code[s].length > kMaxLen || (code[s].bits >> code[s].length) != 0)
      RADNET_FAIL(ctx, RADNET_ERR_ARG, "deflate_rle_emit: symbol %d has the code 0x%x of %d bits (at most 15, the code within them)", s, code[s].bits,
                  code[s].length);
  if (code[kEob].length == 0) RADNET_FAIL(ctx, RADNET_ERR_ARG, "deflate_rle_emit: end-of-block (symbol 256) has no code");
  const int64_t need = radnet_deflate_piece_cap(code, header_nbits, dist_nbits);
  if (piece_cap < need) RADNET_FAIL(ctx, RADNET_ERR_ARG, "deflate_rle_emit: pieces of %lld bytes, this code needs %lld", (long long)piece_cap, (long long)need);
  if (n >= (1ll << 32)) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "deflate_rle_emit: %lld bytes (at most 2^32 - 1)", (long long)n);
  EmitTables tables;
  for (int s = 0; s < kSymbols; ++s) tables.code[s] = (uint32_t)code[s].bits | ((uint32_t)code[s].length << 16);
  uint8_t header[kHeaderWords * 4] = {0};
  memcpy(header, header_bits, (size_t)(header_nbits + 7) / 8);
  if (header_nbits & 7) header[header_nbits >> 3] &= (uint8_t)((1u << (header_nbits & 7)) - 1);      // bits behind the header are the tokens'
  for (int w = 0; w < kHeaderWords; ++w)
    tables.header[w] = (uint32_t)header[4 * w] | (uint32_t)header[4 * w + 1] << 8 | (uint32_t)header[4 * w + 2] << 16 | (uint32_t)header[4 * w + 3] << 24;
  tables.header[0] &= ~1u;                        // BFINAL is the kernel's: set in the last piece only
  const unsigned chunks = (unsigned)((n + kChunk - 1) / kChunk);
  hipLaunchKernelGGL(deflate_emit_kernel, dim3(chunks), dim3(kThreads), 0, ctx->stream, stream, (long long)n, tables, (int)header_nbits, (int)dist_nbits,
                     pieces, (long long)piece_cap, sizes);
  RADNET_CHECK_LAUNCH(ctx, "deflate_rle_emit_u8");
  return RADNET_OK;
}

extern "C" int radnet_deflate_pack(radnet_ctx* ctx, const uint8_t* pieces, int64_t piece_cap, const uint32_t* sizes, int32_t count, uint8_t* out,
                                   int64_t out_cap, uint64_t* total) {
  if (!ctx) return RADNET_ERR_ARG;
  if (!pieces || !sizes || !out || !total || count < 1 || piece_cap < 1 || out_cap < 0)
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "deflate_pack: null pieces, sizes, output or total, or %d pieces of %lld bytes into %lld", count, (long long)piece_cap,
                (long long)out_cap);
  if (count > 65536) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "deflate_pack: %d pieces (at most 65536)", count);
  hipLaunchKernelGGL(deflate_pack_kernel, dim3((unsigned)count), dim3(kThreads), 0, ctx->stream, pieces, (long long)piece_cap, sizes, (int)count, out,
                     (long long)out_cap, reinterpret_cast<unsigned long long*>(total));
  RADNET_CHECK_LAUNCH(ctx, "deflate_pack");
  return RADNET_OK;
}
