// ---- deflate with far matches on the device: LZ77 tokens, two Huffman codes (contract: include/radnet_hip.h, THE LZ TOKEN RULE) ----
// radnet_deflate_lz_scan_u8: a workgroup of 256 threads per chunk holds the chunk's 64 KiB and the table of greatest positions per
// hash (2^15 entries of 16 bits, another 64 KiB) in LDS.  Group by group -- a group is one position per thread -- every thread reads
// its hash's entry, barrier, enters its own position by an integer maximum, barrier: the entry a position reads holds positions of
// earlier groups only, whatever the order of the threads.  Entry 0 doubles as "empty": a candidate is accepted by its bytes, four
// equal bytes have equal hashes, and no entry can lie in front of position 0.  The lengths at distance 1 and `near` come per tile from
// a suffix minimum over the first unequal positions (run_lengths); the hash candidate's is counted byte by byte in LDS, and not at all
// where a nearer candidate already fills the room.  The greedy parse of a tile is sequential as stated; here the token starts are found by pointer
// doubling over "next token" links: 12 rounds mark every start of a tile of 4096 positions.  Counts go through LDS atomics.
// radnet_deflate_lz_emit_u8: the emit of deflate.hip with the tokens read from the table; a token is up to 48 bits.
// wave64, integers only, no inline assembly; no workgroup waits on another; every loop is bounded by the chunk.
#include "deflate_device.h"

namespace {

using namespace radnet_deflate_device;
constexpr int kGroup = RADNET_DEFLATE_LZ_GROUP, kGroupsPerTile = kTile / kGroup, kDistSymbols = RADNET_DEFLATE_DIST_SYMBOLS;
constexpr int kFarMin = RADNET_DEFLATE_LZ_FAR_MIN, kFarMin2 = RADNET_DEFLATE_LZ_FAR_MIN2, kFarD = RADNET_DEFLATE_LZ_FAR_D;
constexpr int kHashBits = 15, kWindow = 32768, kMaxMatch = 258, kRounds = 12;
constexpr unsigned kStart = 1u << 31;
static_assert(kGroup == kThreads && kTile % kGroup == 0, "a group is one position per thread");
static_assert((1 << kRounds) >= kTile, "pointer doubling reaches every token start of a tile");
static_assert(kChunk <= 65536, "positions are 16 bits in the table of greatest positions");
static_assert(kFarMin >= 4 && kFarMin2 >= kFarMin, "a hash candidate is accepted by at least the four bytes of its hash");
// a tile adds at most 16 bits per position: a literal 15, a match 48 on three positions at least
constexpr int kWindowWords = kHeaderWords + kTile * 16 / 32 + 4;

// RFC 1951, 3.2.5: the symbol of a match distance 1..32768, its number of extra bits and their value
__device__ __forceinline__ void distance_symbol(int dist, int& symbol, int& extra_bits, int& extra) {
  const int t = dist - 1;
  if (t < 4) {
    symbol = t, extra_bits = 0, extra = 0;
  } else {
    extra_bits = 30 - __clz(t);                   // floor(log2(t)) - 1
    symbol = 2 * extra_bits + 2 + ((t >> extra_bits) & 1);
    extra = t & ((1 << extra_bits) - 1);
  }
}

// the number of i < room with bytes[p + i] == bytes[p + i - d]
__device__ __forceinline__ int match_length(const uint8_t* bytes, int p, int d, int room) {
  int i = 0;
  while (i < room && bytes[p + i] == bytes[p + i - d]) ++i;
  return i;
}

// run[i] = the number of equal bytes byte[p + j] == byte[p + j - d], j = 0, 1, ..., from p = t0 + i on, counted up to the tile's end, for
// every position i of a tile of tl bytes: a thread finds the first unequal position among its 16 consecutive ones, a suffix minimum
// over the workgroup gives the first one behind them.  Every thread calls this (it holds a barrier); sh: 4 ints, free again at the
// caller's next barrier.  So a flat region costs a position one LDS read, not 258 compares.
__device__ __forceinline__ void run_lengths(const uint8_t* bytes, int t0, int tl, int d, int tid, int* sh, unsigned short* run) {
  constexpr int kNone = 1 << 20;
  const int lane = tid & 63, wave = tid >> 6, i0 = tid * kPer;
  int stop[kPer], cur = kNone;
#pragma unroll
  for (int k = kPer - 1; k >= 0; --k) {
    const int i = i0 + k, p = t0 + i;
    if (i < tl && (p < d || bytes[p] != bytes[p - d])) cur = i;
    stop[k] = cur;
  }
  int b = cur;
  for (int s = 1; s < 64; s <<= 1) {
    const int o = __shfl_down(b, s, 64);
    if (lane + s < 64) b = min(b, o);
  }
  if (lane == 0) sh[wave] = b;
  int behind = __shfl_down(b, 1, 64);
  if (lane == 63) behind = kNone;
  __syncthreads();
  for (int w = wave + 1; w < kThreads / 64; ++w) behind = min(behind, sh[w]);
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const int i = i0 + k;
    if (i < tl) run[i] = (unsigned short)(min(stop[k] == kNone ? behind : stop[k], tl) - i);
  }
}

// (length, distance) against the best so far: the longer wins, on equal length the smaller distance
__device__ __forceinline__ void choose(int length, int dist, int least, int& best_len, int& best_dist) {
  if (length >= least && (length > best_len || (length == best_len && dist < best_dist))) best_len = length, best_dist = dist;
}

__global__ void __launch_bounds__(kThreads) deflate_lz_scan_kernel(const uint8_t* __restrict__ stream, long long n, int near, unsigned* __restrict__ tokens,
                                                                   unsigned* __restrict__ hist_ll, unsigned* __restrict__ hist_d,
                                                                   unsigned long long* __restrict__ parts) {
  __shared__ __attribute__((aligned(16))) uint8_t bytes[kChunk];
  __shared__ unsigned head[1 << (kHashBits - 1)];                   // two 16-bit entries a word
  __shared__ unsigned short jump[kTile + 1];
  __shared__ uint8_t mark[kTile + 1];
  __shared__ unsigned short run1[kTile], run_near[kTile];           // equal bytes at distance 1 and at `near` from every position of the tile
  __shared__ int sh[4];
  __shared__ unsigned counts_ll[kSymbols], counts_d[kDistSymbols];
  __shared__ unsigned long long sums[kThreads / 64][2];
  const int tid = (int)threadIdx.x;
  const long long base = (long long)blockIdx.x * kChunk;
  const int len = (int)min((long long)kChunk, n - base);
  const uint8_t* g = stream + base;
  if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
    for (int i = tid; i < len / 16; i += kThreads) reinterpret_cast<uint4*>(bytes)[i] = reinterpret_cast<const uint4*>(g)[i];
    for (int i = (len & ~15) + tid; i < len; i += kThreads) bytes[i] = g[i];
  } else {
    for (int i = tid; i < len; i += kThreads) bytes[i] = g[i];
  }
  for (int i = tid; i < (1 << (kHashBits - 1)); i += kThreads) head[i] = 0u;
  for (int s = tid; s < kSymbols; s += kThreads) counts_ll[s] = s == kEob ? 1u : 0u;
  if (tid < kDistSymbols) counts_d[tid] = 0u;
  __syncthreads();
  unsigned long long s1 = 0, s2 = 0;
  for (int i = tid; i < len; i += kThreads) adler_add(s1, s2, len, i, bytes[i]);
  for (int t0 = 0; t0 < len; t0 += kTile) {
    const int tl = min(kTile, len - t0);
    run_lengths(bytes, t0, tl, 1, tid, sh, run1);
    __syncthreads();
    if (near > 1) run_lengths(bytes, t0, tl, near, tid, sh, run_near);
    unsigned cand[kGroupsPerTile];                // per position of the thread: length << 16 | distance - 1, 0: none accepted
#pragma unroll
    for (int gi = 0; gi < kGroupsPerTile; ++gi) {
      const int p = t0 + gi * kGroup + tid;
      const bool hashed = p + 4 <= len;
      unsigned h = 0;
      int q = -1;
      if (hashed) {
        const unsigned word = (unsigned)bytes[p] | (unsigned)bytes[p + 1] << 8 | (unsigned)bytes[p + 2] << 16 | (unsigned)bytes[p + 3] << 24;
        h = (word * 2654435761u) >> (32 - kHashBits);
        if (p >= kGroup) q = (int)((head[h >> 1] >> (16 * (h & 1))) & 0xffffu);
      }
      __syncthreads();                            // every read of this group is done
      if (hashed && p > 0) {                      // position 0 is what an empty entry holds
        const int shift = 16 * (int)(h & 1);
        unsigned old = head[h >> 1];
        while ((int)((old >> shift) & 0xffffu) < p) {
          const unsigned seen = atomicCAS(&head[h >> 1], old, (old & ~(0xffffu << shift)) | ((unsigned)p << shift));
          if (seen == old) break;
          old = seen;
        }
      }
      __syncthreads();                            // and every entry of it made, before the next group reads
      int best_len = 0, best_dist = 0;
      if (p < len) {
        const int room = min(kMaxMatch, t0 + tl - p);
        if (room >= 3) {
          choose(min((int)run1[p - t0], room), 1, 3, best_len, best_dist);      // 0 where p has no byte in front of it
          if (near > 1) choose(min((int)run_near[p - t0], room), near, 3, best_len, best_dist);
          const int d = p - q;
          // a candidate that fills the room at a smaller distance cannot be beaten: the hash candidate is not counted then
          if (q >= 0 && d <= kWindow && d != 1 && d != near && !(best_len == room && best_dist < d)) choose(match_length(bytes, p, d, room), d, d <= kFarD ? kFarMin : kFarMin2, best_len, best_dist);
        }
      }
      cand[gi] = best_len ? (unsigned)best_len << 16 | (unsigned)(best_dist - 1) : 0u;
    }
    // the greedy parse: next-token links, the tile's first position marked, and pointer doubling marks every token start
#pragma unroll
    for (int gi = 0; gi < kGroupsPerTile; ++gi) {
      const int i = gi * kGroup + tid;
      if (i < tl) {
        jump[i] = (unsigned short)min(tl, i + max(1, (int)(cand[gi] >> 16)));
        mark[i] = i == 0;
      }
    }
    if (tid == 0) jump[tl] = (unsigned short)tl, mark[tl] = 0;
    __syncthreads();
    for (int r = 0; r < kRounds; ++r) {
      unsigned short next[kGroupsPerTile];
#pragma unroll
      for (int gi = 0; gi < kGroupsPerTile; ++gi) {
        const int i = gi * kGroup + tid;
        if (i < tl && mark[i]) mark[jump[i]] = 1;                   // only token starts are ever marked, in whatever order
      }
#pragma unroll
      for (int gi = 0; gi < kGroupsPerTile; ++gi) {
        const int i = gi * kGroup + tid;
        next[gi] = i < tl ? jump[jump[i]] : (unsigned short)0;
      }
      __syncthreads();
#pragma unroll
      for (int gi = 0; gi < kGroupsPerTile; ++gi) {
        const int i = gi * kGroup + tid;
        if (i < tl) jump[i] = next[gi];
      }
      __syncthreads();
    }
#pragma unroll
    for (int gi = 0; gi < kGroupsPerTile; ++gi) {
      const int i = gi * kGroup + tid;
      if (i < tl) {
        const int p = t0 + i;
        unsigned token = 0;
        if (mark[i]) {
          token = kStart | cand[gi];
          int symbol, eb, ev;
          if (cand[gi]) {
            length_symbol((int)(cand[gi] >> 16), symbol, eb, ev);
            atomicAdd(&counts_ll[symbol], 1u);
            distance_symbol((int)(cand[gi] & 0xffffu) + 1, symbol, eb, ev);
            atomicAdd(&counts_d[symbol], 1u);
          } else {
            atomicAdd(&counts_ll[bytes[p]], 1u);
          }
        }
        tokens[base + p] = token;
      }
    }
    __syncthreads();                              // mark and jump are free for the next tile
  }
  adler_store(s1, s2, tid, sums, parts, (long long)blockIdx.x);     // holds the barrier behind which the counts are complete
  for (int s = tid; s < kSymbols; s += kThreads)
    if (counts_ll[s]) atomicAdd(&hist_ll[s], counts_ll[s]);
  if (tid < kDistSymbols && counts_d[tid]) atomicAdd(&hist_d[tid], counts_d[tid]);
}

struct EmitTables {
  uint32_t code_ll[kSymbols], code_d[kDistSymbols];      // bits | length << 16
  uint32_t header[kHeaderWords];                         // the header's bits, zero behind them
};

__device__ __forceinline__ unsigned reversed(unsigned c) {          // bits | length << 16 -> the bits reversed | length << 16
  const unsigned l = c >> 16;
  return l ? (__brev(c & 0xffffu) >> (32 - l)) | (l << 16) : 0u;
}

__global__ void __launch_bounds__(kThreads) deflate_lz_emit_kernel(const uint8_t* __restrict__ stream, long long n, const unsigned* __restrict__ tokens,
                                                                   const EmitTables tables, int header_nbits, uint8_t* __restrict__ pieces,
                                                                   long long piece_cap, unsigned* __restrict__ sizes) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[kTile];
  __shared__ unsigned window[kWindowWords];       // the piece's bits from word `flushed` on
  __shared__ unsigned rcode_ll[kSymbols], rcode_d[kDistSymbols];      // the codes bit-reversed | length << 16
  __shared__ int sh_sum[4], end_bits;
  const int tid = (int)threadIdx.x;
  const long long base = (long long)blockIdx.x * kChunk;
  const int len = (int)min((long long)kChunk, n - base);
  const bool last = base + len == n;
  uint8_t* piece = pieces + (long long)blockIdx.x * piece_cap;
  for (int s = tid; s < kSymbols; s += kThreads) rcode_ll[s] = reversed(tables.code_ll[s]);
  if (tid < kDistSymbols) rcode_d[tid] = reversed(tables.code_d[tid]);
  for (int w = tid; w < kWindowWords; w += kThreads) window[w] = w < kHeaderWords ? tables.header[w] | (w == 0 && last ? 1u : 0u) : 0u;
  int bitpos = header_nbits, flushed = 0;         // bits of the piece so far; whole words of it already in global memory
  for (int t0 = 0; t0 < len; t0 += kTile) {
    const int tl = min(kTile, len - t0);
    __syncthreads();
    load_tile(tile, stream + base + t0, tl, tid);
    __syncthreads();
    const int i0 = tid * kPer;
    unsigned long long value[kPer];
    int nbits[kPer], mine = 0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      value[k] = 0, nbits[k] = 0;
      const unsigned token = i0 + k < tl ? tokens[base + t0 + i0 + k] : 0u;
      const int mlen = (int)((token >> 16) & 0x7fffu);
      if (token & kStart) {
        if (mlen >= 3 && mlen <= kMaxMatch) {
          int symbol, eb, ev;
          length_symbol(mlen, symbol, eb, ev);
          const unsigned c = rcode_ll[symbol], l = c >> 16;
          unsigned long long v = (c & 0xffffu) | ((unsigned long long)ev << l);
          int nb = (int)l + eb;
          distance_symbol((int)(token & 0xffffu) + 1, symbol, eb, ev);
          const unsigned cd = rcode_d[min(symbol, kDistSymbols - 1)], ld = cd >> 16;
          v |= (unsigned long long)((cd & 0xffffu) | ((unsigned)ev << ld)) << nb;
          value[k] = v, nbits[k] = nb + (int)ld + eb;
        } else {
          const unsigned c = rcode_ll[tile[i0 + k]];
          value[k] = c & 0xffffu, nbits[k] = (int)(c >> 16);
        }
      }
      mine += nbits[k];
    }
    int total;
    int p = bitpos - 32 * flushed + scan_sum(mine, tid, sh_sum, total);
    // a table the first pass did not write for this stream could ask for more than a tile's bits or the piece's room: the piece ends
    // here, empty, and nothing is written out of bounds (uniform: every thread holds the same total)
    if (bitpos - 32 * flushed + total > 32 * (kWindowWords - 2) || (long long)(bitpos + total) + 128 > 8 * piece_cap) {
      if (tid == 0) sizes[blockIdx.x] = 0u;
      return;
    }
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      put_bits(window, p, (unsigned)value[k], min(nbits[k], 32));
      if (nbits[k] > 32) put_bits(window, p + 32, (unsigned)(value[k] >> 32), nbits[k] - 32);
      p += nbits[k];
    }
    bitpos += total;
    __syncthreads();
    flushed = flush_window(window, piece, bitpos, flushed, tid);
  }
  finish_piece(window, piece, bitpos, flushed, rcode_ll[kEob], last, &end_bits, &sizes[blockIdx.x], tid);
}

bool legal_code(const radnet_deflate_code* code, int count) {
  for (int s = 0; s < count; ++s)
    if (code[s].length > kMaxLen || (code[s].bits >> code[s].length) != 0) return false;
  return true;
}

}  // namespace

extern "C" int radnet_deflate_lz_scan_u8(radnet_ctx* ctx, const uint8_t* stream, int64_t n, int32_t near, uint32_t* tokens, uint32_t* hist_ll, uint32_t* hist_d,
                                         uint64_t* adler_parts) {
  if (!ctx) return RADNET_ERR_ARG;
  if (!stream || !tokens || !hist_ll || !hist_d || !adler_parts || n < 1)
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "deflate_lz_scan: null stream, token table, histogram or Adler parts, or an empty stream (%lld bytes)", (long long)n);
  if (near < 1 || near > kWindow) RADNET_FAIL(ctx, RADNET_ERR_ARG, "deflate_lz_scan: a near distance of %d (1..%d)", near, kWindow);
  if (reinterpret_cast<uintptr_t>(tokens) & 15) RADNET_FAIL(ctx, RADNET_ERR_ARG, "deflate_lz_scan: the token table is not 16-byte aligned");
  if (n >= (1ll << 32)) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "deflate_lz_scan: %lld bytes (a count could pass 2^32)", (long long)n);
  const unsigned chunks = (unsigned)((n + kChunk - 1) / kChunk);
  hipLaunchKernelGGL(deflate_lz_scan_kernel, dim3(chunks), dim3(kThreads), 0, ctx->stream, stream, (long long)n, (int)near, tokens, hist_ll, hist_d,
                     reinterpret_cast<unsigned long long*>(adler_parts));
  RADNET_CHECK_LAUNCH(ctx, "deflate_lz_scan_u8");
  return RADNET_OK;
}

extern "C" int radnet_deflate_lz_emit_u8(radnet_ctx* ctx, const uint8_t* stream, int64_t n, const uint32_t* tokens, const radnet_deflate_code* code_ll,
                                         const radnet_deflate_code* code_d, const uint8_t* header_bits, int32_t header_nbits, uint8_t* pieces,
                                         int64_t piece_cap, uint32_t* sizes) {
  if (!ctx) return RADNET_ERR_ARG;
  if (!stream || !tokens || !code_ll || !code_d || !header_bits || !pieces || !sizes || n < 1)
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "deflate_lz_emit: null stream, token table, code, header, pieces or sizes, or an empty stream (%lld bytes)", (long long)n);
  if (reinterpret_cast<uintptr_t>(tokens) & 15) RADNET_FAIL(ctx, RADNET_ERR_ARG, "deflate_lz_emit: the token table is not 16-byte aligned");
  if (header_nbits < 3 || header_nbits > RADNET_DEFLATE_HEADER_MAX_BITS)
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "deflate_lz_emit: a block header of %d bits (3..%d)", header_nbits, RADNET_DEFLATE_HEADER_MAX_BITS);
  if (!legal_code(code_ll, kSymbols))
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "deflate_lz_emit: a literal/length code of more than 15 bits, or bits that do not fit their length");
  if (!legal_code(code_d, kDistSymbols))
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "deflate_lz_emit: a distance code of more than 15 bits, or bits that do not fit their length");
  if (code_ll[kEob].length == 0) RADNET_FAIL(ctx, RADNET_ERR_ARG, "deflate_lz_emit: end-of-block (symbol 256) has no code");
  const int64_t need = radnet_deflate_lz_piece_cap(code_ll, code_d, header_nbits);
  if (piece_cap < need) RADNET_FAIL(ctx, RADNET_ERR_ARG, "deflate_lz_emit: pieces of %lld bytes, these codes need %lld", (long long)piece_cap, (long long)need);
  if (n >= (1ll << 32)) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "deflate_lz_emit: %lld bytes (at most 2^32 - 1)", (long long)n);
  EmitTables tables;
  for (int s = 0; s < kSymbols; ++s) tables.code_ll[s] = (uint32_t)code_ll[s].bits | ((uint32_t)code_ll[s].length << 16);
  for (int s = 0; s < kDistSymbols; ++s) tables.code_d[s] = (uint32_t)code_d[s].bits | ((uint32_t)code_d[s].length << 16);
  uint8_t header[kHeaderWords * 4] = {0};
  memcpy(header, header_bits, (size_t)(header_nbits + 7) / 8);
  if (header_nbits & 7) header[header_nbits >> 3] &= (uint8_t)((1u << (header_nbits & 7)) - 1);      // bits behind the header are the tokens'
  for (int w = 0; w < kHeaderWords; ++w)
    tables.header[w] = (uint32_t)header[4 * w] | (uint32_t)header[4 * w + 1] << 8 | (uint32_t)header[4 * w + 2] << 16 | (uint32_t)header[4 * w + 3] << 24;
  tables.header[0] &= ~1u;                        // BFINAL is the kernel's: set in the last piece only
  const unsigned chunks = (unsigned)((n + kChunk - 1) / kChunk);
  hipLaunchKernelGGL(deflate_lz_emit_kernel, dim3(chunks), dim3(kThreads), 0, ctx->stream, stream, (long long)n, tokens, tables, (int)header_nbits, pieces,
                     (long long)piece_cap, sizes);
  RADNET_CHECK_LAUNCH(ctx, "deflate_lz_emit_u8");
  return RADNET_OK;
}
