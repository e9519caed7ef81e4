// Device helpers shared by the fp32 GEMM kernels (conv_igemm_body.h, conv_wgrad_body.h, chain.hip): buffer-descriptor loads and
// stores, and one 32-deep K tile on the matrix cores (mfma_tile, mfma_tile_rows).
#pragma once
#include <hip/hip_runtime.h>
#include "conv_args.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {
#ifndef RADNET_CHAINS
#define RADNET_CHAINS 2
#endif
constexpr int kChainsSmallTile = RADNET_CHAINS;   // K-interleaved accumulator sets of the 64x64 / 128x64 / 64x128 tiles

#ifdef RADNET_DIAG_STAMPS
#define RADNET_STAMP(var) const unsigned long long var = __builtin_amdgcn_s_memtime()
#else
#define RADNET_STAMP(var)
#endif

__device__ __forceinline__ int div_magic(int m, unsigned long long magic) {
  return (int)(((unsigned long long)(unsigned)m * magic) >> 40);
}

// Buffer loads: the 128-bit resource descriptor carries the tensor's byte size, and the hardware returns 0 for
// any offset beyond it.  Padding taps, rows past M and columns past N are therefore expressed as the offset
// kOOB instead of a branch: all of a tile's loads issue back to back and are waited for once, at the LDS store.
// 2^31, not 2^32-1: every descriptor here covers < 2 GiB (checked by the launchers), so offset + 16 can neither
// wrap around in 32-bit range arithmetic nor fall inside the buffer.
constexpr unsigned kOOB = 0x80000000u;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ float4 buf_load4(__amdgpu_buffer_rsrc_t r, unsigned off) {
  f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0));
  return make_float4(v.x, v.y, v.z, v.w);
}
// voffset (per lane) + soffset (wave-uniform, an SGPR): the hardware adds them and range-checks the SUM without 32-bit
// wrap-around (tools/soffset_probe.hip: kOOB in either operand reads 0), so the uniform part of an address costs no VALU
__device__ __forceinline__ float4 buf_load4s(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)__builtin_amdgcn_readfirstlane(soff), 0));
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ float buf_load1s(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, (int)__builtin_amdgcn_readfirstlane(soff), 0));
}
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int2 buf_load2i(__amdgpu_buffer_rsrc_t r, unsigned off) {
  const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(r, (int)off, 0, 0);
  return make_int2((int)v.x, (int)v.y);
}
__device__ __forceinline__ float buf_load1(__amdgpu_buffer_rsrc_t r, unsigned off) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)off, 0, 0));
}
// sc1 (aux 16): write-through store / L1-bypassing agent-coherent load, for data handed to another workgroup in-launch
__device__ __forceinline__ float buf_load1_sc1(__amdgpu_buffer_rsrc_t r, unsigned off) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)off, 0, 16));
}
__device__ __forceinline__ float4 buf_load4_sc1(__amdgpu_buffer_rsrc_t r, unsigned off) {
  f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 16));
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void buf_store4_sc1(__amdgpu_buffer_rsrc_t r, unsigned off, float4 v) {
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  f32x4 f = {v.x, v.y, v.z, v.w};
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, f), r, (int)off, 0, 16);
}
__device__ __forceinline__ void buf_store1_sc1(__amdgpu_buffer_rsrc_t r, unsigned off, float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, (int)off, 0, 16);
}
__device__ __forceinline__ void buf_store1(__amdgpu_buffer_rsrc_t r, unsigned off, float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, (int)off, 0, 0);
}
typedef float f32x2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void buf_store2_sc1(__amdgpu_buffer_rsrc_t r, unsigned off, float2 v) {
  f32x2v f = {v.x, v.y};
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, f), r, (int)off, 0, 16);
}

__device__ __forceinline__ float f4_comp(const float4& v, int c) { return c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w; }

// One 32-deep K tile: 16 MFMA steps of depth 2, operand fragments prefetched from LDS into a register ring (one
// wave per SIMD has nobody else to hide the LDS latency behind).
// `staging(s)` is the caller's slice of operand staging for step s -- a global load of tile t+2 with its address
// arithmetic, or an LDS store of tile t+1 -- written HERE, between the MFMA steps, because that is where it has to
// execute: an MFMA occupies the matrix pipe for 64 cycles after it issues and the wave can issue independent VALU /
// memory instructions meanwhile.  With all loads in front of the first MFMA and all stores behind the last one
// (which is also where hipcc's scheduler moves them when it is free to), a lone wave per SIMD ran a 64x64 tile in
// 2070 cycles instead of 1024 (tools/stamp_probe.py).  sched_barrier(0) after every step keeps the slices in place.
struct NoStaging {
  __device__ __forceinline__ void operator()(int) const {}
};
//
// Dependent MFMAs: with one 32x32 accumulator per wave (64x64 tile) every MFMA waits for the previous one to
// retire, and a lone wave per SIMD ran at ~120 cycles per MFMA instead of 64.  CH > 1 keeps CH accumulator sets,
// step s adding into set s % CH (the caller sums the sets after the K loop), so CH*TM*TN MFMAs are independent.
// Fragments are fetched TWO steps ahead (3-slot register ring): an LDS read takes about as long as one MFMA.
template <int TM, int TN, int CH, typename Staging>
__device__ __forceinline__ void mfma_tile(const float* sA, const float* sB, int pitchA, int pitchB, int a_off, int b_off,
                                          f32x16 (&acc)[CH][TM][TN], Staging staging) {
  constexpr int kSteps = BK / 2;
  float a[3][TM], b[3][TN];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
#pragma unroll
    for (int i = 0; i < TM; ++i) a[p][i] = sA[2 * p * pitchA + a_off + i * 32];
#pragma unroll
    for (int j = 0; j < TN; ++j) b[p][j] = sB[2 * p * pitchB + b_off + j * 32];
  }
#pragma unroll
  for (int s = 0; s < kSteps; ++s) {
    const int cur = s % 3, nxt = (s + 2) % 3;
    if (s + 2 < kSteps) {
#pragma unroll
      for (int i = 0; i < TM; ++i) a[nxt][i] = sA[(2 * s + 4) * pitchA + a_off + i * 32];
#pragma unroll
      for (int j = 0; j < TN; ++j) b[nxt][j] = sB[(2 * s + 4) * pitchB + b_off + j * 32];
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
        acc[s % CH][i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cur][i], b[cur][j], acc[s % CH][i][j], 0, 0, 0);
    staging(s);
    // order inside the step: next step's LDS reads, this step's MFMAs, then the staging slice in their shadow
    __builtin_amdgcn_sched_group_barrier(0x100, TM + TN, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, TM * TN, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// The same tile for the forward / dgrad kernel, whose gathered operand arrives as 4 consecutive k of one row: it is
// kept ROW-major in LDS ([row][kRowPitch], one ds_write_b128 per chunk -- the transposed ds_write_b32 stores it
// replaces cost ~85 cycles of MFMA time each, tools/stamp_probe.py) and its fragments are read 4 k at a time with
// ds_read_b128.  That works because the order of k inside a tile is free as long as A and B agree: MFMA step
// s = 4q + j multiplies k = 8q + j in lanes 0-31 and k = 8q + 4 + j in lanes 32-63, so lane (row, h) reads the 16
// bytes at k = 8q + 4h once per q and uses component j in step 4q + j; the k-major operand (forward weights, [k][n])
// reads row 8q + 4h + j.  kRowPitch = 36 words: a ds_read_b128 lane group (16 lanes, rows {0-3,12-15,20-27} + 4g)
// lands on 16 distinct 4-bank sets, and the 8-lane groups of the ds_write_b128 cover 32 consecutive words.
constexpr int kRowPitch = BK + 4;
// KSTEPS = 16: the wave multiplies the whole 32-deep tile; KSTEPS = 8: half of it (8-wave workgroups: waves 4-7 take
// k = 16..31, the caller shifts a_off / b_off accordingly and sums the two halves after the K loop).
template <int TM, int TN, int CH, bool B_ROWMAJOR, int KSTEPS, typename Staging>
__device__ __forceinline__ void mfma_tile_rows(const float* sA, const float* sB, int pitchB, int a_off, int b_off,
                                               f32x16 (&acc)[CH][TM][TN], Staging staging) {
  constexpr int kSteps = KSTEPS;
  float4 af[2][TM], bq[2][TN];
  float bf[3][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i) af[0][i] = *reinterpret_cast<const float4*>(sA + a_off + i * 32 * kRowPitch);
  if (B_ROWMAJOR) {
#pragma unroll
    for (int j = 0; j < TN; ++j) bq[0][j] = *reinterpret_cast<const float4*>(sB + b_off + j * 32 * kRowPitch);
  } else {
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int j = 0; j < TN; ++j) bf[p][j] = sB[p * pitchB + b_off + j * 32];
  }
#pragma unroll
  for (int s = 0; s < kSteps; ++s) {
    const int q = s >> 2, c = s & 3;
    const bool group_reads = c == 1 && q + 1 < kSteps / 4;   // next group's 16-byte fragments, three steps ahead of their first use
    const bool step_reads = !B_ROWMAJOR && s + 2 < kSteps;
    if (group_reads) {
#pragma unroll
      for (int i = 0; i < TM; ++i) af[(q + 1) & 1][i] = *reinterpret_cast<const float4*>(sA + a_off + i * 32 * kRowPitch + 8 * (q + 1));
      if (B_ROWMAJOR) {
#pragma unroll
        for (int j = 0; j < TN; ++j) bq[(q + 1) & 1][j] = *reinterpret_cast<const float4*>(sB + b_off + j * 32 * kRowPitch + 8 * (q + 1));
      }
    }
    if (step_reads) {
      const int s2 = s + 2;
#pragma unroll
      for (int j = 0; j < TN; ++j) bf[s2 % 3][j] = sB[(8 * (s2 >> 2) + (s2 & 3)) * pitchB + b_off + j * 32];
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
        acc[s % CH][i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(f4_comp(af[q & 1][i], c), B_ROWMAJOR ? f4_comp(bq[q & 1][j], c) : bf[s % 3][j],
                                                                 acc[s % CH][i][j], 0, 0, 0);
    staging(s);
    // order inside the step: the LDS reads issued here, this step's MFMAs, then the staging slice in their shadow
    if (group_reads && (B_ROWMAJOR || step_reads)) __builtin_amdgcn_sched_group_barrier(0x100, TM + TN, 0);
    else if (group_reads) __builtin_amdgcn_sched_group_barrier(0x100, TM, 0);
    else if (step_reads) __builtin_amdgcn_sched_group_barrier(0x100, TN, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, TM * TN, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
}
}  // namespace
