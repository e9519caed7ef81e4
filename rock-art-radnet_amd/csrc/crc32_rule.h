// The arithmetic and the grain rule of radnet_crc32_segments (include/radnet_hip.h states both in words), once: the planner
// (crc32_plan.cpp, g++), the launch code and the kernels (crc32.hip) all read them from here.  No HIP header; integers only.
//
// CRC-32 as zlib sums it: P = 0xEDB88320, reflected -- bit 31 of a register is the coefficient of x^0, bit 0 that of x^31.
// pure(B) is the register after the bytes B with init 0 and no final xor.  Three identities carry everything:
//   pure(A || B) = pure(A) * x^(8 |B|) + pure(B)   (the product mod P, + is xor)
//   pure(0^k || B) = pure(B)                       (leading zero bytes are free)
//   zlib.crc32(B, c0) = pure(B) + (c0 ^ 0xFFFFFFFF) * x^(8 |B|) + 0xFFFFFFFF
#pragma once
#include <stdint.h>

#include "radnet_hip.h"

#if defined(__HIPCC__)
#define RADNET_CRC_HD __host__ __device__ __forceinline__
#else
#define RADNET_CRC_HD inline
#endif

constexpr uint32_t kCrcPoly = 0xEDB88320u;
constexpr uint32_t kCrcOne = 0x80000000u;       // x^0
constexpr uint32_t kCrcX8 = 0x00800000u;        // x^8: one byte

// one step of the register: times x, mod P
RADNET_CRC_HD constexpr uint32_t crc_times_x(uint32_t v) { return (v >> 1) ^ (kCrcPoly & (0u - (v & 1u))); }

// a * b mod P: gfx950 has no carry-less multiply, so 32 shift / xor steps, none of them a branch
RADNET_CRC_HD constexpr uint32_t crc_times(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 31; i >= 0; --i) {
    p ^= b & (0u - ((a >> i) & 1u));
    b = crc_times_x(b);
  }
  return p;
}

// the register after one more byte
RADNET_CRC_HD constexpr uint32_t crc_byte(uint32_t v, uint32_t byte) {
  v ^= byte;
  for (int i = 0; i < 8; ++i) v = crc_times_x(v);
  return v;
}

// the register after four more bytes, the first in the low byte of `word`
RADNET_CRC_HD constexpr uint32_t crc_word(uint32_t v, uint32_t word) {
  v ^= word;
  for (int i = 0; i < 32; ++i) v = crc_times_x(v);
  return v;
}

// x^(8 len) mod P by squaring; len <= 0 gives x^0
RADNET_CRC_HD constexpr uint32_t crc_shift(int64_t len) {
  uint32_t r = kCrcOne, b = kCrcX8;
  for (uint64_t e = len > 0 ? (uint64_t)len : 0; e; e >>= 1) {
    if (e & 1) r = crc_times(r, b);
    b = crc_times(b, b);
  }
  return r;
}

template <int N>
struct crc_table {
  uint32_t v[N];
};

// v[i] = x^(8 step i): the weight of a unit that stands i units of `step` bytes in front of the end
template <int N>
constexpr crc_table<N> crc_powers(int64_t step) {
  crc_table<N> t{};
  const uint32_t s = crc_shift(step);
  uint32_t p = kCrcOne;
  for (int i = 0; i < N; ++i) {
    t.v[i] = p;
    p = crc_times(p, s);
  }
  return t;
}

// v[k] = x^(8 2^k): the factors of x^(8 len), one per bit of len
constexpr crc_table<64> crc_squares() {
  crc_table<64> t{};
  uint32_t p = kCrcX8;
  for (int k = 0; k < 64; ++k) {
    t.v[k] = p;
    p = crc_times(p, p);
  }
  return t;
}

constexpr int kCrcGrain = RADNET_CRC32_GRAIN;              // bytes of one lane's load
constexpr int kCrcSpanGrains = RADNET_CRC32_SPAN_GRAINS;   // lanes of one workgroup
constexpr int64_t kCrcSpan = (int64_t)kCrcGrain * kCrcSpanGrains;

// THE GRAIN RULE.  A segment of `length` bytes whose first byte stands `at` bytes behind a 16-byte boundary of device memory
// (at = the buffer's misalignment + the segment's offset; at + length stays below 2^64).  Its last `tail` (0..15) bytes, those
// behind the last 16-byte boundary inside it, are summed byte by byte.  The body in front of them is cut into grains of 16 bytes
// counted BACKWARDS from that boundary, so every grain but the first is one aligned 16-byte load and the first is padded in front
// with zeros, which are free; 256 grains, again counted from the body's end, are one span: one workgroup.
struct crc_cut {
  int64_t grains, spans;
  int32_t tail;
};

RADNET_CRC_HD crc_cut crc_cut_of(uint64_t at, int64_t length) {
  const uint64_t end = at + (uint64_t)length, aligned_end = end & ~(uint64_t)(kCrcGrain - 1);
  crc_cut c{0, 0, (int32_t)length};
  if (aligned_end > at) {
    c.tail = (int32_t)(end - aligned_end);
    c.grains = (int64_t)((aligned_end - at + (uint64_t)(kCrcGrain - 1)) / (uint64_t)kCrcGrain);
    c.spans = (c.grains + kCrcSpanGrains - 1) / kCrcSpanGrains;
  }
  return c;
}
