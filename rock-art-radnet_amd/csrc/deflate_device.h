// ---- what the two device deflates share (deflate.hip: run-length tokens; deflate_lz.hip: LZ77 tokens) ----------------------------------
// The cut of the stream, RFC 1951's length symbols, the tile load, the workgroup prefix sum, the bit window and its way into a piece,
// the Adler-32 parts.  Workgroups of 256 threads, wave64, integers only.
#pragma once
#include "radnet_internal.h"

namespace radnet_deflate_device {

constexpr int kChunk = RADNET_DEFLATE_CHUNK, kTile = RADNET_DEFLATE_TILE, kThreads = 256, kPer = kTile / kThreads;
constexpr int kSymbols = RADNET_DEFLATE_SYMBOLS, kEob = 256, kMaxLen = 15;
constexpr int kHeaderWords = RADNET_DEFLATE_HEADER_MAX_BITS / 32;
static_assert(kPer == 16 && kChunk % kTile == 0, "a thread reads its 16 positions as one uint4");

// RFC 1951, 3.2.5: the symbol of a match length 3..258, its number of extra bits and their value
__device__ __forceinline__ void length_symbol(int len, int& symbol, int& extra_bits, int& extra) {
  const int l = len - 3;
  if (len == 258) {
    symbol = 285, extra_bits = 0, extra = 0;
  } else if (l < 8) {
    symbol = 257 + l, extra_bits = 0, extra = 0;
  } else {
    extra_bits = 29 - __clz(l);                   // floor(log2(l)) - 2
    symbol = 261 + 4 * extra_bits + ((l >> extra_bits) & 3);
    extra = l & ((1 << extra_bits) - 1);
  }
}

// bytes [0, len) of a tile from global memory; a whole tile at a 16-byte aligned address moves as one uint4 per thread
__device__ __forceinline__ void load_tile(uint8_t* tile, const uint8_t* __restrict__ g, int len, int tid) {
  if (len == kTile && (reinterpret_cast<uintptr_t>(g) & 15) == 0) {
    reinterpret_cast<uint4*>(tile)[tid] = reinterpret_cast<const uint4*>(g)[tid];
  } else {
    for (int i = tid; i < len; i += kThreads) tile[i] = g[i];
  }
}

// exclusive prefix sum of v over the workgroup; total = the sum
__device__ __forceinline__ int scan_sum(int v, int tid, int* sh, int& total) {
  const int lane = tid & 63, wave = tid >> 6;
  int a = v;
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(a, d, 64);
    if (lane >= d) a += o;
  }
  if (lane == 63) sh[wave] = a;
  __syncthreads();
  int before = a - v;
  for (int w = 0; w < wave; ++w) before += sh[w];
  total = sh[0] + sh[1] + sh[2] + sh[3];
  return before;
}

// v's low nb bits (nb <= 32) into the window from bit p on; the window is zero where nothing has been put
__device__ __forceinline__ void put_bits(unsigned* window, int p, unsigned v, int nb) {
  if (nb == 0) return;
  const unsigned long long x = (unsigned long long)v << (p & 31);
  atomicOr(&window[p >> 5], (unsigned)x);
  if (x >> 32) atomicOr(&window[(p >> 5) + 1], (unsigned)(x >> 32));
}

// The Adler-32 parts of a chunk of len bytes: a thread adds every byte it owns, at offset i of the chunk, to its two sums ...
__device__ __forceinline__ void adler_add(unsigned long long& s1, unsigned long long& s2, int len, int i, int byte) {
  s1 += (unsigned)byte;
  s2 += (unsigned long long)(len - i) * (unsigned)byte;
}

// ... and the workgroup's sums go to parts[2 chunk] and parts[2 chunk + 1].  Every thread calls this; it holds one barrier.
__device__ __forceinline__ void adler_store(unsigned long long s1, unsigned long long s2, int tid, unsigned long long (*sums)[2],
                                            unsigned long long* __restrict__ parts, long long chunk) {
  for (int d = 32; d > 0; d >>= 1) {
    s1 += __shfl_down(s1, d, 64);
    s2 += __shfl_down(s2, d, 64);
  }
  if ((tid & 63) == 0) sums[tid >> 6][0] = s1, sums[tid >> 6][1] = s2;
  __syncthreads();
  if (tid < 2) parts[2 * chunk + tid] = sums[0][tid] + sums[1][tid] + sums[2][tid] + sums[3][tid];
}

// The window's whole words (the piece's bits from word `flushed` on, bitpos bits in all) go out to the piece and the partial word
// moves to the front.  Every thread calls this; the window's writers must have passed a barrier.  Returns the new `flushed`.
__device__ __forceinline__ int flush_window(unsigned* window, uint8_t* __restrict__ piece, int bitpos, int flushed, int tid) {
  const uint8_t* bytes = reinterpret_cast<const uint8_t*>(window);
  const int whole = (bitpos >> 5) - flushed;
  for (int i = tid; i < 4 * whole; i += kThreads) piece[4ll * flushed + i] = bytes[i];
  const unsigned carry = window[whole];
  __syncthreads();
  for (int w = tid; w <= whole; w += kThreads) window[w] = w == 0 ? carry : 0u;
  return flushed + whole;
}

// The end of a piece: end-of-block (its code bit-reversed | length << 16), then the sync flush -- 000, zero bits up to the byte,
// 00 00 FF FF -- or, in the last piece, zero bits up to the byte; the rest of the window goes out and the piece's size with it.
// Every thread calls this; end_bits: one int of LDS.
__device__ __forceinline__ void finish_piece(unsigned* window, uint8_t* __restrict__ piece, int bitpos, int flushed, unsigned eob, bool last,
                                             int* end_bits, unsigned* __restrict__ size, int tid) {
  const uint8_t* bytes = reinterpret_cast<const uint8_t*>(window);
  __syncthreads();
  if (tid == 0) {
    int p = bitpos - 32 * flushed;
    put_bits(window, p, eob & 0xffffu, (int)(eob >> 16));
    p += (int)(eob >> 16);
    if (!last) {
      p = (p + 3 + 7) & ~7;                       // 000: an empty stored block, not the last; zero bits up to the byte
      put_bits(window, p + 16, 0xffffu, 16);      // LEN 0, NLEN 0xFFFF
      p += 32;
    } else {
      p = (p + 7) & ~7;
    }
    *end_bits = p;
  }
  __syncthreads();
  const int tail = *end_bits >> 3;
  for (int i = tid; i < tail; i += kThreads) piece[4ll * flushed + i] = bytes[i];
  if (tid == 0) *size = (unsigned)(4 * flushed + tail);
}

}  // namespace radnet_deflate_device
