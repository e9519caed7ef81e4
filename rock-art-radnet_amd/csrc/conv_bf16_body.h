// The GEMM body the bf16 matrix-core convs share (v_mfma_f32_32x32x16_bf16, fp32 accumulation): conv_bf16.hip (forward) and
// conv_bf16_bwd.hip (data and weight gradient) differ in their gathers and epilogues only; everything between the two is here, once.
//
//   * An output tile of BM rows x BN columns per workgroup, a reduction in 32-deep tiles.  4 wavefronts in a 2x2 arrangement; each
//     wave owns (BM/2)x(BN/2) of the output as 32x32 accumulator tiles: D[row][col], col = lane & 31,
//     row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) for accumulator register r.
//   * Both operands are row-major [row][32 k + 8 pad] bf16 in LDS (80-byte rows: 16-byte aligned, breaks the power-of-two row
//     stride), read as one ds_read_b128 per fragment: a lane of the 32x32x16 MFMA holds k = 8h + j, j = 0..7, of one row.  Two LDS
//     buffers, the global loads of tile t+1 in registers while tile t is multiplied: one barrier per reduction tile.  What a row, a
//     column and the reduction are is the caller's business: its gload(t) brings tile t into registers, its lstore(buf) rounds it to
//     bf16 and writes it to LDS.  Padding taps, ragged rows / columns and the reduction's padding are the out-of-range offset kOOB
//     that the hardware answers with zeros -- no branch in the loop.
//   * Ordered split of the reduction: blockIdx.z = slice of the reduction tiles.  Every slice writes its partial tile as a
//     write-through (sc1) slab and drains it, then takes a ticket from the tile's arrival counter; the last arrival sums ALL slabs
//     in slice order (its own read back too, with sc1 loads), so the result does not depend on arrival order, then runs the
//     caller's epilogue and leaves the counter at zero.  Slabs live in the context's workspace, counters in its aux block
//     (kAuxBf16SplitCounters): all three kernels use the same ones, which is safe because launches of one context are ordered and
//     every launch leaves its counters at zero.  No float atomics: two runs give the same bits.  split <= 1 is a single pass that
//     needs neither.
//   * Host side: the geometry and size checks of the three entry points, the output tile by radnet_bf16_tile_shape's rule, the
//     resolution of a split against workspace and counters, and the (timed) launch.
#pragma once
#include "radnet_internal.h"
#include <hip/hip_ext.h>

#include <initializer_list>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int BK = 32;          // reduction depth per LDS tile (two MFMA steps of 16)
constexpr int LDSROW = BK + 8;  // bf16 per LDS row: 80 bytes (16-byte aligned, breaks the power-of-two row stride)
constexpr int NTHREADS = 256;
constexpr unsigned kOOB = 0x80000000u;   // every descriptor covers < 2 GiB (bf16_too_large): offset + 16 stays out of range

__device__ __forceinline__ int div_magic(int m, unsigned long long magic) {
  return (int)(((unsigned long long)(unsigned)m * magic) >> 40);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ f32x4 buf_load4(__amdgpu_buffer_rsrc_t r, unsigned off) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0));
}
__device__ __forceinline__ u32x4 buf_load4u(__amdgpu_buffer_rsrc_t r, unsigned off) {
  return __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0);
}
__device__ __forceinline__ float buf_load1(__amdgpu_buffer_rsrc_t r, unsigned off) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)off, 0, 0));
}
__device__ __forceinline__ void buf_store1(__amdgpu_buffer_rsrc_t r, unsigned off, float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, (int)off, 0, 0);
}
// sc1 (aux 16): write-through store / L1-bypassing agent-coherent load, for the slabs handed to the last slice in-launch
__device__ __forceinline__ f32x4 buf_load4_sc1(__amdgpu_buffer_rsrc_t r, unsigned off) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 16));
}
__device__ __forceinline__ void buf_store4_sc1(__amdgpu_buffer_rsrc_t r, unsigned off, const f32x4& v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, (int)off, 0, 16);
}

// fp32 -> bf16, round to nearest, ties to even (v_cvt_pk_bf16_f32 on gfx950)
__device__ __forceinline__ uint16_t to_bf16_bits(float v) { return __builtin_bit_cast(uint16_t, (__bf16)v); }
__device__ __forceinline__ u32x4 pack8_bf16(const f32x4& lo, const f32x4& hi) {
  const bf16x8 b = {(__bf16)lo.x, (__bf16)lo.y, (__bf16)lo.z, (__bf16)lo.w, (__bf16)hi.x, (__bf16)hi.y, (__bf16)hi.z, (__bf16)hi.w};
  return __builtin_bit_cast(u32x4, b);
}

template <int BM, int BN>
__device__ __forceinline__ void bf16_zero(f32x16 (&acc)[BM / 64][BN / 64]) {
#pragma unroll
  for (int i = 0; i < BM / 64; ++i)
#pragma unroll
    for (int j = 0; j < BN / 64; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}

// reduction tiles [x, y) of slice z of `split` (split <= nrt: none is empty)
__device__ __forceinline__ int2 bf16_slice_tiles(int nrt, int split, unsigned z) {
  return make_int2((int)(((long long)nrt * z) / split), (int)(((long long)nrt * (z + 1)) / split));
}

// where a thread sits: its wave's row and column in the 2x2 arrangement; in its 32x32 tiles, fragment row / output column l31 and
// k half / output row group hi
struct Bf16Lane {
  int wm, wn, l31, hi;
};
__device__ __forceinline__ Bf16Lane bf16_lane() {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  return {wave >> 1, wave & 1, lane & 31, lane >> 5};
}

// acc = sum over the reduction tiles [t0, t1) of A tile x B tile
template <int BM, int BN, typename GLoad, typename LStore>
__device__ __forceinline__ void bf16_gemm_tiles(const uint16_t (&sa)[2][BM * LDSROW], const uint16_t (&sb)[2][BN * LDSROW], int t0, int t1,
                                                GLoad&& gload, LStore&& lstore, const Bf16Lane& ln, f32x16 (&acc)[BM / 64][BN / 64]) {
  constexpr int TM = BM / 64, TN = BN / 64;
  const int wm = ln.wm, wn = ln.wn, l31 = ln.l31, hi = ln.hi;
  bf16_zero<BM, BN>(acc);
  gload(t0);
  lstore(0);
  __syncthreads();
  for (int t = t0; t < t1; ++t) {
    const int cur = (t - t0) & 1;
    gload(t + 1 < t1 ? t + 1 : t);                   // the last iteration re-loads its own tile (never stored): no branch
#pragma unroll
    for (int s = 0; s < BK / 16; ++s) {
      bf16x8 af[TM], bfr[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i)
        af[i] = *reinterpret_cast<const bf16x8*>(&sa[cur][(wm * (BM / 2) + i * 32 + l31) * LDSROW + 16 * s + 8 * hi]);
#pragma unroll
      for (int j = 0; j < TN; ++j)
        bfr[j] = *reinterpret_cast<const bf16x8*>(&sb[cur][(wn * (BN / 2) + j * 32 + l31) * LDSROW + 16 * s + 8 * hi]);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
    lstore(cur ^ 1);
    __syncthreads();
  }
}

// The ordered in-launch split (grid z = split slices of every output tile): true in the workgroup that arrived last at its tile, with
// acc = the sum of all slices in slice order; false in the others, which are done.  Uniform for the workgroup.
// partial: slabs [tile][slice][BM*BN], the 16 registers of a lane's 32x32 accumulator contiguous (four 16-byte accesses);
// counters: one arrival counter per output tile, zero outside a launch.
template <int BM, int BN>
__device__ __forceinline__ bool bf16_ordered_split(float* partial, unsigned* counters, int split, f32x16 (&acc)[BM / 64][BN / 64]) {
  constexpr int TM = BM / 64, TN = BN / 64;
  __shared__ int s_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned tile_id = blockIdx.x + gridDim.x * blockIdx.y;
  const unsigned lane_off = (unsigned)((wave * TM * TN * 64 + lane) * 16) * 4u;
  const __amdgpu_buffer_rsrc_t rslab = make_rsrc(partial + ((size_t)tile_id * split + blockIdx.z) * (BM * BN), BM * BN * 4u);
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 v = {acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
        buf_store4_sc1(rslab, lane_off + (unsigned)(((i * TN + j) * 64 * 16 + q * 4) * 4), v);
      }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    const unsigned ticket = __hip_atomic_fetch_add(counters + tile_id, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = ticket == (unsigned)(split - 1);
    if (last) __hip_atomic_store(counters + tile_id, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
    s_last = last;
  }
  __syncthreads();
  if (s_last == 0) return false;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");      // compiler-only: keeps the slab loads below the ticket
  bf16_zero<BM, BN>(acc);
  for (int s = 0; s < split; ++s) {                // slices ADDED in slice order
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(partial + ((size_t)tile_id * split + s) * (BM * BN), BM * BN * 4u);
    f32x4 v[TM * TN * 4];
#pragma unroll
    for (int t = 0; t < TM * TN * 4; ++t) v[t] = buf_load4_sc1(rs, lane_off + (unsigned)(((t >> 2) * 64 * 16 + (t & 3) * 4) * 4));
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 w = v[(i * TN + j) * 4 + q];
          acc[i][j][4 * q] += w.x; acc[i][j][4 * q + 1] += w.y; acc[i][j][4 * q + 2] += w.z; acc[i][j][4 * q + 3] += w.w;
        }
  }
  return true;
}

// ---- host ------------------------------------------------------------------------------------------------------------------
// the forward convolution's geometry, as all three entry points need it (`what`: the entry point's name in the message)
inline int bf16_check_geometry(radnet_ctx* ctx, const radnet_conv_desc* d, const char* what) {
  if (d->nb <= 0 || d->h <= 0 || d->w_ <= 0 || d->oh <= 0 || d->ow <= 0 || d->kh <= 0 || d->kw <= 0 || d->stride <= 0 || d->n <= 0 || d->c <= 0)
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "%s: bad geometry", what);
  if ((d->oh - 1) * d->stride - d->pad_t >= d->h || (d->ow - 1) * d->stride - d->pad_l >= d->w_)
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "%s: output %dx%d inconsistent with input %dx%d", what, d->oh, d->ow, d->h, d->w_);
  return RADNET_OK;
}

// what the kernels' 32-bit arithmetic rests on: every buffer descriptor < 2 GiB (kOOB), every row / reduction extent < 2^20 (div_magic)
inline bool bf16_too_large(std::initializer_list<long long> bytes, std::initializer_list<long long> extents) {
  for (long long b : bytes)
    if (b >= (1ll << 31)) return true;
  for (long long e : extents)
    if (e >= (1 << 20)) return true;
  return false;
}

// One launch of L::kernel<BM, BN, SPLIT>(g) on the rows x cols output, g.split slices.  L names the kernel:
//   what, launch_name   prefix of the messages, name in a launch failure
//   halve_split         a split whose counters or slabs do not fit the context is halved until it does (by rule, never by timing:
//                       one pass needs neither); otherwise it is refused
//   timing_slot         radnet_ctx::slots
template <typename L, int BM, int BN, typename Args>
int bf16_launch(radnet_ctx* ctx, Args g, int rows, int cols, double flops) {
  const dim3 grid0(radnet_cdiv(rows, BM), radnet_cdiv(cols, BN), 1);
  const unsigned long long tiles = (unsigned long long)grid0.x * grid0.y;
  const auto slab_bytes = [&] { return tiles * (unsigned long long)g.split * BM * BN * 4ull; };
  if (L::halve_split)
    while (g.split > 1 && (tiles > kAuxBf16SplitCounterCount || !ctx->ws || slab_bytes() > ctx->ws_bytes)) g.split /= 2;
  if (g.split > 1) {
    if (tiles > kAuxBf16SplitCounterCount)
      RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "%s: %llu output tiles exceed the %zu split counters", L::what, tiles, kAuxBf16SplitCounterCount);
    if (!ctx->ws || ctx->ws_bytes < slab_bytes())
      RADNET_FAIL(ctx, RADNET_ERR_ARG, "%s: K split %d needs %llu bytes of workspace (radnet_set_workspace: %llu)", L::what, g.split, slab_bytes(),
                  (unsigned long long)ctx->ws_bytes);
    g.partial = (float*)ctx->ws;
    g.counters = reinterpret_cast<unsigned*>(ctx->aux + kAuxBf16SplitCounters);
  }
  const dim3 grid(grid0.x, grid0.y, g.split > 1 ? g.split : 1);
  const bool timed = ctx->timing != 0;
  if (timed) radnet_timing_arm(ctx);
  auto kernel = g.split > 1 ? L::template kernel<BM, BN, true>() : L::template kernel<BM, BN, false>();
  if (ctx->arm0) hipExtLaunchKernelGGL(kernel, grid, dim3(NTHREADS), 0, ctx->stream, ctx->arm0, ctx->arm1, 0, g);
  else hipLaunchKernelGGL(kernel, grid, dim3(NTHREADS), 0, ctx->stream, g);
  RADNET_CHECK_LAUNCH(ctx, L::launch_name);
  if (timed) radnet_timing_end_armed(ctx, L::timing_slot, flops);
  return RADNET_OK;
}

// the launch on the output tile of radnet_bf16_tile_shape's fixed rule on (rows, cols)
template <typename L, typename Args>
int bf16_launch_by_shape(radnet_ctx* ctx, const Args& g, long long rows, int cols, double flops) {
  long long tiles = 0;
  const int shape = radnet_bf16_tile_shape(rows, cols, &tiles);
  if (shape == 0) return bf16_launch<L, 128, 128>(ctx, g, (int)rows, cols, flops);
  if (shape == 1) return bf16_launch<L, 128, 64>(ctx, g, (int)rows, cols, flops);
  return bf16_launch<L, 64, 64>(ctx, g, (int)rows, cols, flops);
}

}  // namespace
