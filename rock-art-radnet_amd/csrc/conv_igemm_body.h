// Convolution as implicit GEMM on the gfx950 fp32 matrix cores (v_mfma_f32_32x32x2_f32).
//
// Stands in for keras Conv2D / TimeDistributed(Conv2D) + FixedBatchNormalization + Add + Activation
// of the reference graph (base_models/resnet50.py:41-147,183-186; rpn.py:41-64;
// FixedBatchNormalization.py:59-85) and for the TF autodiff gradients of those layers.
//
// Design (MI355X-first):
//   * NHWC activations, weights [K=(kh,kw,c)][N]: the im2col matrix is never materialised; each workgroup gathers
//     its A tile (BM output pixels x 32 k) straight from the activation tensor with 16-byte buffer loads (4
//     consecutive channels); padding taps, ragged rows / columns and tiles past the end are an out-of-range offset
//     that the hardware answers with zeros -- no branch anywhere in the K loop.
//   * 4 wavefronts in a 2x2 arrangement (optionally 8: two grids halving every K tile); each wave owns a
//     (BM/2)x(BN/2) block of the output as 32x32 MFMA tiles in accumulator registers for the whole K loop.  32-row (32-column)
//     tiles have one wave row (column): the waves left over split every K tile between them and are summed through LDS
//     (round 4: M = 980 / 2 394 / 160-row problems fill the chip without K slices).
//   * LDS double buffer.  The gathered operand (A; both operands in dgrad) is ROW-major [row][36]: written with one
//     ds_write_b128 per 4-k chunk, read 4 k at a time with ds_read_b128 -- the k order inside a tile is free as long
//     as both operands agree (mfma_tile_rows).  Forward weights stay k-major [k][BN+4] (conflict-free ds_read_b32).
//     wgrad keeps both operands reduction-major (mfma_tile).
//   * two register stages of global loads (tile t+2 in flight while t is multiplied); loads, address arithmetic and
//     LDS stores are single operations dealt out BETWEEN the MFMA steps: a wave cannot overlap its own VALU / memory
//     instructions with its own MFMAs (tools/mfma_loop_probe.hip), so what counts is the non-MFMA instruction count
//     per tile and having other waves on the SIMD.
//   * epilogue fused through buffer descriptors: frozen-BN scale/shift (+bias), residual add, ReLU / sigmoid; for
//     dgrad the residual-path gradient add and the producer's ReLU mask.
//   * split-K inside the launch: slices write sc1 (write-through) slabs, take a ticket from a per-tile arrival
//     counter, the last arriver reduces in slice order and applies the epilogue.
//   * fp32 MFMA runs at the fp32 vector rate (157 TFLOP/s peak), 16x less than bf16, so LDS and L2 bandwidth are far
//     from limiting; what matters is filling 256 CUs at batch 1 -- tile shape, K slices, workgroup order and waves per
//     workgroup are measured per problem shape (run_igemm).
#pragma once
#include "conv_device.h"

namespace {
// ---- forward / dgrad kernel -------------------------------------------------------------------------
// BMODE 0: B is [K][ldw] row-major (forward).  BMODE 1: B element (k=(pos,co), n=ci) lives at
//          w[((flip(pos)*cin_fwd + ci) * ldw) + co]  (dgrad: same weight buffer, read transposed).
// SMALLC : C == 4 (stem with the image padded to 4 channels): one 4-float chunk per kernel position.
// WAVES  : 4 = the 2x2 wave grid multiplies whole K tiles; 8 = two such grids share the tile, waves 4-7 taking the
//          second half of every 32-deep K tile (split-K INSIDE the workgroup: same LDS tile, half the staging work per
//          thread, twice the waves per SIMD for the same number of workgroups -- a wave cannot hide its own staging
//          instructions under its own MFMAs, another wave's can).  The halves are summed through LDS after the loop.
// LDS floats of one workgroup of conv_igemm_body (two buffers of an A and a B tile)
template <int BM, int BN, int BMODE>
constexpr int igemm_lds_floats() { return 2 * (BM * kRowPitch + ((BMODE == 0) ? BK * (BN + 4) : BN * kRowPitch)); }
// PERSIST kernels sum their K parts while the staging buffers already hold the next problem's first tile: own scratch behind them
template <int BM, int BN, int WAVES>
constexpr int igemm_persist_scratch_floats() {
  constexpr int WG = (BM >= 64 ? 2 : 1) * (BN >= 64 ? 2 : 1), KH = WAVES / WG;
  return (KH - 1) * BM * BN;
}

// ---- fused bottleneck tail (round 4) ----------------------------------------------------------------------------------
// A ResNet identity / conv block is 1x1 reduce -> 3x3 -> 1x1 expand (+ shortcut, ReLU) (resnet50.py:41-71, 74-128).  In stage 2
// (C = 64 / 256 on the 150x250 map) the two pointwise convs are memory-shaped launches: 1.2 GF each for 48 MB moved, 50-66 TFLOP/s,
// and three launches per block.  Cut the chain in front of the 3x3 instead of behind it and nothing needs a halo: a workgroup that
// holds a [BM rows x 64] tile of the 3x3 output holds ALL of that layer's channels for its rows, so it can go on, for the same rows,
//   y[rows][N2]  = relu(t2 . W2 * sc2 + sh2 + shortcut[rows][N2])          (branch2c, Add, Activation)
//   t'[rows][64] = relu(y . W3 * sc3 + sh3)                                 (the NEXT block's branch2a), optional
// with t2 and y passed between the three GEMMs through LDS; t2 is never written to memory, y once, and the next block's 1x1 input
// is not read back.  The tail GEMMs run on the same 2x2 (2x1) wave grid as the 3x3: A fragments from LDS in the K loop's own row-major
// layout (mfma_tile_rows), B fragments straight from the 64 KB weight matrices in L2 (every workgroup reads the same ones; one dword per
// lane and MFMA step, no staging, no barrier).  Frozen layers only: the block's intermediate activations do not exist afterwards.
template <int BM>
constexpr int bneck_lds_floats() { return 4 * BM * (BK + 4); }     // the 3x3 tile and one 64-column chunk of y, each as two 32-deep A tiles

// one 64-deep GEMM step of the tail: acc += A[rows][64] (LDS, two row-major 32-deep tiles) . B (fragments in registers)
// (ONE accumulator: the tail's registers decide how many workgroups share a CU, and those other waves fill the MFMA pipe between two
// dependent steps of this one)
__device__ __forceinline__ void bneck_mfma64(const float* sA, int buf_floats, int a_off, const float (&bw)[32], f32x16& acc) {
#pragma unroll
  for (int half = 0; half < 2; ++half)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 af = *reinterpret_cast<const float4*>(sA + half * buf_floats + a_off + 8 * q);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int s = 16 * half + 4 * q + c;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(f4_comp(af, c), bw[s], acc, 0, 0, 0);
      }
    }
}
// B fragments of such a step: lane (hi, l31) multiplies k = 32 half + 8 q + 4 hi + c in step (half, q, c) -- the order mfma_tile_rows uses
__device__ __forceinline__ void bneck_load_b(__amdgpu_buffer_rsrc_t rw, unsigned voff, unsigned row0, unsigned ld4, bool live, float (&bw)[32]) {
#pragma unroll
  for (int s = 0; s < 32; ++s) {
    const unsigned k = 32u * (s >> 4) + 8u * ((s & 15) >> 2) + (s & 3);
    bw[s] = buf_load1s(rw, voff, live ? (row0 + k) * ld4 : kOOB);
  }
}

template <int BM, int WAVES, bool HAS3>
__device__ __forceinline__ void bneck_tail(const GemmArgs& g, const TailArgs& tz, float* __restrict__ lds, const f32x16& acc, const int m0) {
  constexpr int WM = BM >= 64 ? 2 : 1, WN = 2;
  static_assert(WAVES == WM * WN, "the tail runs on the 3x3's wave grid, no K parts");
  constexpr int kBufT = BM * kRowPitch;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5, l31 = lane & 31;
  const int wm = wave / WN, wn = wave % WN;
  float* sT = lds;
  float* sY = lds + 2 * kBufT;
  const int col = wn * 32 + l31;                                   // this lane's column inside a 64-column chunk
  const int own_off = (wm * 32 + 4 * hi) * kRowPitch + l31;       // accumulator register 0 of this lane in a 32-deep A tile (k = its column)
  {
    const float sc = g.scale ? g.scale[col] : 1.f, sh = g.shift ? g.shift[col] : 0.f;
    float* dst = sT + wn * kBufT + own_off;
#pragma unroll
    for (int r = 0; r < 16; ++r) dst[((r & 3) + 8 * (r >> 2)) * kRowPitch] = fmaxf(acc[r] * sc + sh, 0.f);
  }
  __syncthreads();
  const int a_off = (wm * 32 + l31) * kRowPitch + 4 * hi;
  const __amdgpu_buffer_rsrc_t rw2 = make_rsrc(tz.w2, tz.w2_bytes), rw3 = make_rsrc(tz.w3, HAS3 ? tz.w3_bytes : 0u);
  const __amdgpu_buffer_rsrc_t radd = make_rsrc(tz.add, tz.add ? tz.add_bytes : 0u), ry = make_rsrc(tz.y, tz.y_bytes);
  const __amdgpu_buffer_rsrc_t rsc2 = make_rsrc(tz.sc2, tz.sc2 ? (unsigned)tz.N2 * 4u : 0u), rsh2 = make_rsrc(tz.sh2, tz.sh2 ? (unsigned)tz.N2 * 4u : 0u);
  const unsigned ldw2_4 = (unsigned)tz.ldw2 * 4u, ldw3_4 = (unsigned)tz.ldw3 * 4u, ldy4 = (unsigned)tz.ldy2 * 4u, lda4 = (unsigned)tz.ld_add2 * 4u;
  const unsigned bv2 = (unsigned)(4 * hi) * ldw2_4 + (unsigned)col * 4u;           // + 64 c columns, + k rows (SGPR part)
  const unsigned bv3 = (unsigned)(4 * hi) * ldw3_4 + (unsigned)col * 4u;           // + (64 c + k) rows
  const unsigned row0 = (unsigned)(m0 + wm * 32 + 4 * hi);
  const bool rows_ok = row0 < (unsigned)g.M;                       // rows past M further down fall off the descriptors' ends
  const bool has_sc2 = tz.sc2 != nullptr;
  f32x16 acc3;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc3[r] = 0.f;
  float bw2[32];
  bneck_load_b(rw2, bv2, 0u, ldw2_4, true, bw2);
  const int nchunks = tz.N2 >> 6;
  for (int c = 0; c < nchunks; ++c) {
    const unsigned ncol = (unsigned)(64 * c + col);
    const unsigned vy = rows_ok ? (row0 * (unsigned)tz.ldy2 + ncol) * 4u : kOOB;
    const unsigned va = rows_ok ? (row0 * (unsigned)tz.ld_add2 + ncol) * 4u : kOOB;
    float ad[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) ad[r] = buf_load1s(radd, va, (unsigned)((r & 3) + 8 * (r >> 2)) * lda4);
    const float sc2r = buf_load1(rsc2, ncol * 4u), sh2 = buf_load1(rsh2, ncol * 4u);
    const float sc2 = has_sc2 ? sc2r : 1.f;
    float bw3[32];
    if (HAS3) bneck_load_b(rw3, bv3, 64u * (unsigned)c, ldw3_4, true, bw3);
    f32x16 acc2;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc2[r] = 0.f;
    bneck_mfma64(sT, kBufT, a_off, bw2, acc2);
    // the next chunk's expand fragments travel under this chunk's epilogue and reduce step (columns move by 256 bytes per chunk)
    bneck_load_b(rw2, bv2 + 256u * (unsigned)(c + 1), 0u, ldw2_4, c + 1 < nchunks, bw2);
    if (HAS3 && c > 0) __syncthreads();                            // every wave is done reading the previous chunk from sY
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const unsigned rr = (unsigned)((r & 3) + 8 * (r >> 2));
      const float v = fmaxf(acc2[r] * sc2 + sh2 + ad[r], 0.f);
      buf_store1(ry, vy + rr * ldy4, v);
      if (HAS3) sY[wn * kBufT + own_off + rr * kRowPitch] = v;
    }
    if (HAS3) {
      __syncthreads();
      bneck_mfma64(sY, kBufT, a_off, bw3, acc3);
    }
  }
  if (HAS3) {
    const __amdgpu_buffer_rsrc_t rt = make_rsrc(tz.t, tz.t_bytes);
    const float sc3 = tz.sc3 ? tz.sc3[col] : 1.f, sh3 = tz.sh3 ? tz.sh3[col] : 0.f;
    const unsigned vt = rows_ok ? (row0 * (unsigned)tz.ldt + (unsigned)col) * 4u : kOOB;
    const unsigned ldt4 = (unsigned)tz.ldt * 4u;
#pragma unroll
    for (int r = 0; r < 16; ++r)
      buf_store1(rt, vt + (unsigned)((r & 3) + 8 * (r >> 2)) * ldt4, fmaxf(acc3[r] * sc3 + sh3, 0.f));
  }
}

// COH: the output is handed to other workgroups of the SAME launch (chain kernel): stores are write-through (sc1), as the
// split-K slabs are, so that a consumer on another XCD finds them in memory.
// PERSIST (batched launches, forward form, plain epilogue): the workgroup runs g.zper CONSECUTIVE problems of the batch on its output
// tile as one long K loop -- the loads of the next problem's first K tiles are issued under the last MFMA steps of the current one,
// the finished accumulators leave with fire-and-forget stores, and the workgroup pays ONE prologue and ONE drain instead of one per
// problem.  The 36 GEMMs of a Winograd layer have 4-8 K tiles each: as 432-720 one-tile workgroups they were all prologue and
// epilogue.
// FUSE (1 / 2): the accumulators do not leave through the epilogue but feed bneck_tail (2: with the next block's 1x1 reduce)
template <int BM, int BN, int BMODE, bool SMALLC, int WAVES, bool COH = false, bool PERSIST = false, int FUSE = 0>
__device__ __forceinline__ void conv_igemm_body(const GemmArgs& g, float* __restrict__ lds, const unsigned bid_x, const unsigned bid_y, const unsigned bid_z,
                                                const unsigned grid_x, [[maybe_unused]] const TailArgs* tz = nullptr) {
  constexpr int NT = 64 * WAVES;
  // Wave grid over the output tile: 2x2 for tiles of 64 rows / columns and more, a single wave row (column) for the 32-row
  // (32-column) tiles; the waves left over split every 32-deep K tile between them (KH parts: the 8-wave form of the 64x64
  // tile has KH = 2, the 4-wave 32x64 tile too, the 4-wave 32x32 tile KH = 4) and are summed through LDS after the loop.
  constexpr int WM = BM >= 64 ? 2 : 1, WN = BN >= 64 ? 2 : 1, WG = WM * WN;
  constexpr int KH = WAVES / WG;
  static_assert(WAVES % WG == 0 && (KH == 1 || KH == 2 || KH == 4), "wave count does not cover the tile's wave grid");
  constexpr int TM = BM / (32 * WM), TN = BN / (32 * WN);     // 32x32 tiles per wave in each direction
  constexpr int PB = BN + 4;                    // forward weights: k-major [BK][PB]
  constexpr int A_ITERS = BM * 8 / NT;          // float4 chunks per thread (A)
  constexpr int B_ITERS = BN * 8 / NT;
  static_assert(A_ITERS >= 1 && B_ITERS >= 1 && A_ITERS * NT == BM * 8 && B_ITERS * NT == BN * 8, "tile too small for this many threads");
  constexpr int kRowStep = NT / 8;              // rows between a thread's consecutive chunks
  constexpr int kStepsW = (BK / 2) / KH;        // MFMA steps of one wave per K tile
  constexpr int kKPart = BK / KH;               // depth of a wave's part of the K tile
  // one LDS buffer: A row-major [BM][kRowPitch]; B k-major [BK][PB] (forward) or row-major [BN][kRowPitch] (dgrad)
  constexpr int kBufA = BM * kRowPitch;
  constexpr int kBufB = (BMODE == 0) ? BK * PB : BN * kRowPitch;
  float* sA0 = lds;
  float* sB0 = lds + 2 * kBufA;

  RADNET_STAMP(t_start);
#ifdef RADNET_DIAG_STAMPS
  const unsigned long long rt_start = __builtin_amdgcn_s_memrealtime();
  unsigned long long t_first = t_start, t_loop = t_start;
#endif
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int hi = lane >> 5, l31 = lane & 31;
  const int wgi = wave % WG;                    // place in the wave grid
  const int wm = wgi / WN, wn = wgi % WN;
  const int khalf = wave / WG;                  // which part of every K tile (0 when the wave grid takes all waves)
  // Work assignment.  Plain launch: one workgroup per output tile.  Unit-table launch (g.units != null): the host
  // cut the linearised (tile, k-tile) iteration space into near-equal chunks so every CU gets the same amount of
  // MFMA work whatever the tile count (stream-K style); a unit is (tile, k range, partial slot or -1).
  int m0, n0, unit_kb = 0, unit_ke = 0, slot = -1, slot0 = 0, n_slices = 1, tile_id = 0;
  if (g.units != nullptr) {
    const int4 u0 = reinterpret_cast<const int4*>(g.units)[2 * bid_x];
    const int4 u1 = reinterpret_cast<const int4*>(g.units)[2 * bid_x + 1];
    m0 = u0.x * BM; n0 = u0.y * BN; unit_kb = u0.z; unit_ke = u0.w;
    slot = u1.x; slot0 = u1.y; n_slices = u1.z; tile_id = u1.w;
  } else {
    m0 = bid_x * BM; n0 = bid_y * BN;
  }

  // ---- per-thread A rows: decode m -> (image, oh, ow) once
  const int a_kc = tid & 7;
  // a_base = byte offset of (image, ih0, iw0, channel 0), possibly negative (halo); a tap (kh, kw, ci) then adds one
  // per-tile offset, and only the two range compares remain per load (no multiplies in the K loop: v_mul_lo_u32
  // is a 16-cycle instruction).  Rows past M get ih0 far below zero, which fails the range compare of every tap.
  int a_base[A_ITERS], a_ih0[A_ITERS], a_iw0[A_ITERS];
  const int a_cbytes = (SMALLC ? 4 : g.C) * 4;
#pragma unroll
  for (int i = 0; i < A_ITERS; ++i) {
    const int m = m0 + (tid >> 3) + kRowStep * i;
    const int mc = m < g.M ? m : 0;
    const int img = div_magic(mc, g.magic_ohow);
    const int rem = mc - img * g.OHOW;
    const int oh = div_magic(rem, g.magic_ow);
    const int ow = rem - oh * g.OW;
    a_ih0[i] = m < g.M ? oh * g.stride - g.pad_t : -(1 << 24);
    a_iw0[i] = ow * g.stride - g.pad_l;
    a_base[i] = ((img * g.H + (oh * g.stride - g.pad_t)) * g.W + a_iw0[i]) * a_cbytes;
  }

  // Channel-tiled layers (!SMALLC): everything that changes from K tile to K tile is wave-uniform -- the tap (kh, kw), the
  // first channel, the weight row -- and travels in the load's SGPR offset; what is left per lane is a constant offset and
  // ONE bit per tap ("this tap of this output row falls into the padding"), folded into bit 31 of the offset.  The
  // descriptor of x starts a_bias bytes early so that the per-lane part of a halo row is never negative.
  const unsigned a_bias = SMALLC ? 0u : (unsigned)((g.pad_t * g.W + g.pad_l) * g.C * 4);
  unsigned a_voff[A_ITERS], a_inv[A_ITERS];
  if (!SMALLC) {
#pragma unroll
    for (int i = 0; i < A_ITERS; ++i) {
      const bool row_ok = a_ih0[i] > -(1 << 23);
      unsigned inv = 0u;
      for (int p = 0, kh = 0, kw = 0; p < g.npos; ++p) {
        const bool ok = ((unsigned)(a_ih0[i] + kh) < (unsigned)g.H) & ((unsigned)(a_iw0[i] + kw) < (unsigned)g.W);
        inv |= (ok ? 0u : 1u) << p;
        if (++kw == g.KW) { kw = 0; ++kh; }
      }
      a_voff[i] = row_ok ? (unsigned)(a_base[i] + (int)a_bias + a_kc * 16) : 0u;
      a_inv[i] = row_ok ? inv : ~0u;
    }
  }

  // forward weights: byte offset of this thread's chunk (row kr, column n) in K tile 0; a tile adds BK rows
  int b_base[B_ITERS];
  bool b_nvalid[B_ITERS];
  unsigned b_voff[B_ITERS];
  const int b_tile_bytes = BK * g.ldw * 4;
  if (BMODE == 0) {
    constexpr int CPR = BN / 4;
#pragma unroll
    for (int i = 0; i < B_ITERS; ++i) {
      const int c = tid + NT * i;
      const int kr = c / CPR, n = n0 + (c - kr * CPR) * 4;
      b_base[i] = (kr * g.ldw + n) * 4;
      b_nvalid[i] = n < g.N;
      b_voff[i] = b_nvalid[i] ? (unsigned)b_base[i] : kOOB;
    }
  } else {
#pragma unroll
    for (int i = 0; i < B_ITERS; ++i) {       // dgrad: row n of w^T (forward input channel), this thread's 4 channels
      const int n = n0 + (tid >> 3) + kRowStep * i;
      b_voff[i] = n < g.N ? ((unsigned)n * (unsigned)g.ldw + (unsigned)a_kc * 4u) * 4u : kOOB;
    }
  }

  const int nk_total = (g.K + BK - 1) / BK;
  // batched launch (radnet_gemm_batched): problem blockIdx.z of a strided batch, same geometry; PERSIST: problems bz .. bz + nz - 1
  const long long bz = g.batch > 1 ? (long long)bid_z * (PERSIST ? g.zper : 1) : 0;
  const int nz = PERSIST ? ((int)bz + g.zper <= g.batch ? g.zper : g.batch - (int)bz) : 1;
  const int kt_begin = g.units != nullptr ? unit_kb : 0;
  const int kt_end = g.units != nullptr ? unit_ke : nk_total * nz;

  // running position of the current K tile: kernel position pos = (kh, kw) and first channel ci0, k0 = pos*C + ci0
  int pos = 0, ci0 = 0, kh_run = 0, kw_run = 0;
  if (!SMALLC) {
    int k0 = kt_begin * BK;
    pos = k0 / g.C;
    ci0 = k0 - pos * g.C;
    kh_run = pos / g.KW;
    kw_run = pos - kh_run * g.KW;
  }

  // (PERSIST: the descriptors span the nz problems; rows past M and columns past N are out of range through their per-lane kOOB bit,
  // not through the extent, and K has no ragged tile -- the launcher checks C % BK == 0)
  const unsigned span_x = PERSIST ? (unsigned)((nz - 1) * g.x_bstride * 4) : 0u, span_w = PERSIST ? (unsigned)((nz - 1) * g.w_bstride * 4) : 0u;
  const __amdgpu_buffer_rsrc_t rx = make_rsrc(reinterpret_cast<const char*>(g.x + bz * g.x_bstride) - a_bias, g.x_bytes ? g.x_bytes + a_bias + span_x : 0u);
  const __amdgpu_buffer_rsrc_t rw = make_rsrc(g.w + bz * g.w_bstride, g.w_bytes + span_w);
  const bool has_in_scale = g.in_scale != nullptr;
  const __amdgpu_buffer_rsrc_t rscale = make_rsrc(g.in_scale, has_in_scale ? (unsigned)g.C * 4u : 0u);
  // Two register stages: the loads of tile t+2 are issued while tile t is being multiplied and tile t+1 waits in the
  // other stage, so a memory round trip (1-2 us when the line comes from the Infinity Cache or HBM) has TWO tile
  // times to complete.
  struct Stage {
    float4 a[A_ITERS], b[B_ITERS], s;
  };
  Stage st0, st1;
  st0.s = make_float4(1, 1, 1, 1);
  st1.s = make_float4(1, 1, 1, 1);

  // Operand staging, cut into single operations so that mfma_tile can deal them out between the MFMA steps.
  // Entirely branch-free (a tile past the end of this workgroup's K range, live == false, loads from kOOB -> 0, and
  // its LDS store writes zeros into the buffer nobody reads again): the K loop body is ONE basic block.
  constexpr int kLoadOps = A_ITERS + B_ITERS;                                   // one 16-byte buffer load each
  constexpr int kStoreOps = A_ITERS + B_ITERS;                                  // one ds_write_b128 each
  // state of the tile being loaded (tile_begin -> load_op)
  int t_kt = 0, t_kh = 0, t_kw = 0, t_fpos = 0, t_aoff = 0;
  bool t_live = false, t_kv = false;
  unsigned s_a = kOOB, s_b = kOOB, s_sh = 0;       // wave-uniform: SGPR offsets of the tile's A / B loads, tap -> bit-31 shift
  unsigned p_item_a = 0u, p_item_b = 0u;           // PERSIST: byte offset of the running problem in the spanning descriptors
  int p_kin = 0;                                   //          K tile inside the running problem

  auto tile_begin = [&](int kt, bool live, Stage& st) {
    t_kt = kt;
    t_live = live;
    if (SMALLC) {
      const int p = kt * 8 + a_kc;           // kernel position of this thread's chunk
      t_kh = p / g.KW;
      t_kw = p - t_kh * g.KW;
      t_kv = live & (p < g.npos);
      t_aoff = (t_kh * g.W + t_kw) * 16;
    } else {
      // K = npos * C and C is a multiple of BK (launcher): a live tile lies inside one tap, all of its k are valid
      t_fpos = g.flip ? (g.npos - 1 - pos) : pos;
      s_a = live ? (unsigned)(((kh_run * g.W + kw_run) * g.C + ci0) * 4) + p_item_a : kOOB;
      s_sh = (unsigned)(31 - pos);
      s_b = !live ? kOOB : BMODE == 0 ? (PERSIST ? (unsigned)p_kin * (unsigned)b_tile_bytes + p_item_b : (unsigned)kt * (unsigned)b_tile_bytes)
                                      : ((unsigned)t_fpos * (unsigned)g.cin_fwd * (unsigned)g.ldw + (unsigned)ci0) * 4u;
      // raw value; consumed (and replaced by 1 when there is no in_scale: empty descriptor, reads 0) only at the LDS
      // store one tile later -- touching it here would make the wave wait for the load it has just issued
      if (BMODE == 1) st.s = buf_load4s(rscale, (unsigned)a_kc * 16u, live ? (unsigned)ci0 * 4u : kOOB);   // forward never scales its input
      // advance the running position to the following tile
      ci0 += BK;
      const bool wrap = ci0 >= g.C;
      ci0 = wrap ? 0 : ci0;
      if (PERSIST) {                           // a 1x1 problem ends where its channels end: the next tile is the next problem's first
        p_kin = wrap ? 0 : p_kin + 1;
        p_item_a += wrap ? (unsigned)(g.x_bstride * 4) : 0u;
        p_item_b += wrap ? (unsigned)(g.w_bstride * 4) : 0u;
      } else {
        pos += wrap ? 1 : 0;
        kw_run += wrap ? 1 : 0;
        const bool wrap_w = kw_run >= g.KW;
        kw_run = wrap_w ? 0 : kw_run;
        kh_run += wrap_w ? 1 : 0;
      }
    }
  };

  auto load_op = [&](int idx, Stage& st) {
    if (idx < A_ITERS) {
      // ---------------- A: implicit im2col gather (invalid taps load from kOOB -> 0)
      const int i = idx;
      if (SMALLC) {
        const int ih = a_ih0[i] + t_kh, iw = a_iw0[i] + t_kw;
        const bool ok = t_kv & ((unsigned)ih < (unsigned)g.H) & ((unsigned)iw < (unsigned)g.W);
        st.a[i] = buf_load4(rx, ok ? (unsigned)(a_base[i] + t_aoff) : kOOB);
      } else {
        st.a[i] = buf_load4s(rx, a_voff[i] | ((a_inv[i] << s_sh) & kOOB), s_a);       // two VALU: padding bit of this tap -> bit 31
      }
    } else if (SMALLC) {
      constexpr int CPR = BN / 4;            // float4 chunks per k row
      const int i = idx - A_ITERS;
      const int c = tid + NT * i;
      const int kr = c / CPR;
      const bool ok = t_live & (t_kt * BK + kr < g.K) & b_nvalid[i];   // N is a multiple of 4 (launcher checks)
      st.b[i] = buf_load4(rw, ok ? (unsigned)(b_base[i] + t_kt * b_tile_bytes) : kOOB);
    } else {
      st.b[idx - A_ITERS] = buf_load4s(rw, b_voff[idx - A_ITERS], s_b);            // no VALU at all
    }
  };

  // LDS stores: every operation is one ds_write_b128 of the 4 consecutive k (A, dgrad B) or n (forward B) a thread
  // loaded; the gathered operand is scaled on the way (dgrad: frozen-BN factor of the channel).
  auto store_op = [&](int op, int buf, const Stage& st) {
    float* sA = sA0 + buf * kBufA;
    float* sB = sB0 + buf * kBufB;
    if (op < A_ITERS) {
      const int i = op;
      float4 v = st.a[i];
      if (BMODE == 1) {                     // select, not a branch: the K loop stays one basic block
        v.x *= has_in_scale ? st.s.x : 1.f;
        v.y *= has_in_scale ? st.s.y : 1.f;
        v.z *= has_in_scale ? st.s.z : 1.f;
        v.w *= has_in_scale ? st.s.w : 1.f;
      }
      *reinterpret_cast<float4*>(sA + ((tid >> 3) + kRowStep * i) * kRowPitch + a_kc * 4) = v;
    } else if (BMODE == 0) {
      constexpr int CPR = BN / 4;
      const int i = op - A_ITERS;
      const int cc = tid + NT * i;
      const int kr = cc / CPR, n4 = cc - kr * CPR;
      *reinterpret_cast<float4*>(sB + kr * PB + n4 * 4) = st.b[i];
    } else {
      const int i = op - A_ITERS;
      *reinterpret_cast<float4*>(sB + ((tid >> 3) + kRowStep * i) * kRowPitch + a_kc * 4) = st.b[i];
    }
  };

  // independent 32x32 accumulators per wave (see mfma_tile): two K-interleaved sets for the tiles with fewer than 4
  constexpr int CH = (TM * TN >= 4) ? 1 : kChainsSmallTile;
  f32x16 accs[CH][TM][TN];
#pragma unroll
  for (int c = 0; c < CH; ++c)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) accs[c][i][j][r] = 0.f;

  if (kt_begin < kt_end) {
    tile_begin(kt_begin, true, st0);
#pragma unroll
    for (int op = 0; op < kLoadOps; ++op) load_op(op, st0);
    tile_begin(kt_begin + 1, kt_begin + 1 < kt_end, st1);
#pragma unroll
    for (int op = 0; op < kLoadOps; ++op) load_op(op, st1);
#pragma unroll
    for (int op = 0; op < kStoreOps; ++op) store_op(op, 0, st0);
    __syncthreads();
#ifdef RADNET_DIAG_STAMPS
    t_first = __builtin_amdgcn_s_memtime();
#endif
    // fragment offsets (see mfma_tile_rows): row-major operands start at (row, k = 4*hi), the k-major one at row 4*hi
    // (8-wave workgroups: waves 4-7 start at k = 16 of the tile)
    const int a_off = (wm * (BM / WM) + l31) * kRowPitch + 4 * hi + kKPart * khalf;
    const int b_off = (BMODE == 0) ? (4 * hi + kKPart * khalf) * PB + wn * (BN / WN) + l31 : (wn * (BN / WN) + l31) * kRowPitch + 4 * hi + kKPart * khalf;
    // invariant at the top of step(kt, buf): LDS buffer `buf` holds tile kt; stage `nxt` holds tile kt+1 (in flight or
    // landed); stage `cur` is free.  MFMA steps 0 .. kLoadOps-1 each carry one global load of tile kt+2, the steps
    // after them (all but the last, which has no MFMA behind it to hide under) the LDS stores of tile kt+1.
    constexpr int kSteps = kStepsW;
    constexpr int kStoreSteps = kSteps - 1 - kLoadOps;
    constexpr int kStoresPerStep = (kStoreOps + kStoreSteps - 1) / kStoreSteps;
    static_assert(kStoreSteps >= 1, "tile too large for the staging schedule");
    auto step = [&](int kt, int buf, Stage& cur, Stage& nxt) {
      tile_begin(kt + 2, kt + 2 < kt_end, cur);
      mfma_tile_rows<TM, TN, CH, BMODE != 0, kStepsW>(sA0 + buf * kBufA, sB0 + buf * kBufB, PB, a_off, b_off, accs, [&](int s) {
        if (s < kLoadOps) {
#ifndef RADNET_DIAG_SKIP_LOADS
          load_op(s, cur);
#endif
        } else if (s < kSteps - 1) {
#if defined(RADNET_DIAG_SINK_STORES)         // loads stay (consumed by an empty asm after their wait), the LDS stores go
#pragma unroll
          for (int q = 0; q < kStoresPerStep; ++q) {
            const int op = (s - kLoadOps) * kStoresPerStep + q;
            if (op < kStoreOps) {
              const float4 v = op < A_ITERS ? nxt.a[op < A_ITERS ? op : 0] : nxt.b[op < A_ITERS ? 0 : op - A_ITERS];
              asm volatile("" ::"v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w));
            }
          }
#elif !defined(RADNET_DIAG_SKIP_STORES)
#pragma unroll
          for (int q = 0; q < kStoresPerStep; ++q) {
            const int op = (s - kLoadOps) * kStoresPerStep + q;
            if (op < kStoreOps) store_op(op, buf ^ 1, nxt);
          }
#endif
        }
      });
#ifndef RADNET_DIAG_SKIP_BARRIER
      __syncthreads();
#endif
    };
    // PERSIST: a problem's last K tile has been multiplied -- its sums leave while the next problem's first tile sits in the other
    // LDS buffer and its second is in flight (nothing here waits for memory: plain stores, the K-part sums through LDS scratch of
    // their own; the scratch is rewritten one barrier-terminated step later at the earliest)
    [[maybe_unused]] int p_done = 0, p_out = 0;
    auto item_flush = [&]() {
#pragma unroll
      for (int c = 1; c < CH; ++c)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) accs[0][i][j] += accs[c][i][j];
      if (KH > 1) {
        constexpr int kPartFloats = WG * TM * TN * 16 * 64;
        float* red = lds + igemm_lds_floats<BM, BN, BMODE>() + (wgi * TM * TN * 16) * 64 + lane;
        if (khalf > 0) {
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
              for (int r = 0; r < 16; ++r) red[(khalf - 1) * kPartFloats + ((i * TN + j) * 16 + r) * 64] = accs[0][i][j][r];
        }
        __syncthreads();
        if (khalf == 0) {
#pragma unroll
          for (int h = 1; h < KH; ++h)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
              for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) accs[0][i][j][r] += red[(h - 1) * kPartFloats + ((i * TN + j) * 16 + r) * 64];
        }
      }
      const __amdgpu_buffer_rsrc_t ryp = make_rsrc(g.y + (bz + p_out) * g.y_bstride, g.y_bytes);
      const unsigned ldy4p = (unsigned)g.ldy * 4u;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn * (BN / WN) + j * 32 + l31;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const int mb = m0 + wm * (BM / WM) + i * 32 + 4 * hi;
          const unsigned vy = (khalf == 0 && n < g.N && mb < g.M) ? ((unsigned)mb * (unsigned)g.ldy + (unsigned)n) * 4u : kOOB;
#pragma unroll
          for (int r = 0; r < 16; ++r) buf_store1(ryp, vy + (unsigned)((r & 3) + 8 * (r >> 2)) * ldy4p, accs[0][i][j][r]);
        }
      }
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) accs[c][i][j][r] = 0.f;
      ++p_out;
    };
    for (int kt = kt_begin; kt < kt_end; kt += 2) {
      step(kt, 0, st0, st1);
      if (PERSIST && ++p_done == nk_total) { item_flush(); p_done = 0; }
      if (kt + 1 < kt_end) {
        step(kt + 1, 1, st1, st0);
        if (PERSIST && ++p_done == nk_total) { item_flush(); p_done = 0; }
      }
    }
  }
  if (PERSIST) return;                  // every problem's tile has been stored
  f32x16(&acc)[TM][TN] = accs[0];
#pragma unroll
  for (int c = 1; c < CH; ++c)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] += accs[c][i][j];
  // 8-wave workgroups: waves 4-7 hold the sums over the second half of every K tile; they hand them to waves 0-3
  // through the (now free) staging array and take no further part in the output -- every global access below is
  // predicated on live_out (offset kOOB otherwise), the barriers are reached by all eight waves.
  bool live_out = true;
  if (KH > 1) {
    static_assert((KH - 1) * WG * TM * TN * 16 * 64 <= igemm_lds_floats<BM, BN, BMODE>(), "K-part sums do not fit the staging array");
    constexpr int kPartFloats = WG * TM * TN * 16 * 64;
    float* red = lds + (wgi * TM * TN * 16) * 64 + lane;
    if (khalf > 0) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) red[(khalf - 1) * kPartFloats + ((i * TN + j) * 16 + r) * 64] = acc[i][j][r];
    }
    __syncthreads();
    if (khalf == 0) {
#pragma unroll
      for (int h = 1; h < KH; ++h)            // parts added in k order
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] += red[(h - 1) * kPartFloats + ((i * TN + j) * 16 + r) * 64];
    }
    __syncthreads();
    live_out = khalf == 0;
  }
  if constexpr (FUSE != 0) {
    static_assert(BN == 64 && BMODE == 0 && !SMALLC && !COH && !PERSIST && KH == 1 && TM == 1 && TN == 1, "the fused tail follows a whole-K [BM x 64] forward tile");
    bneck_tail<BM, WAVES, FUSE == 2>(g, *tz, lds, acc[0][0], m0);
    return;
  }
#ifdef RADNET_DIAG_STAMPS
  t_loop = __builtin_amdgcn_s_memtime();
  // stamps go to a buffer of their own; nothing the kernel outputs is computed from them.  The epilogue stamp is
  // taken by a trailing block below (after the stores have been ISSUED, plus a vmcnt(0) wait so it covers their
  // completion).
  auto write_stamps = [&]() {
    __builtin_amdgcn_s_waitcnt(0);
    const unsigned long long t_end = __builtin_amdgcn_s_memtime();
    if (g.stamps != nullptr && tid == 0) {
      unsigned long long* s = g.stamps + 8ull * (bid_x + (unsigned long long)grid_x * bid_y);
      s[0] = t_start; s[1] = t_first; s[2] = t_loop; s[3] = t_end;
      s[4] = rt_start; s[5] = __builtin_amdgcn_s_memrealtime();
      s[6] = ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32) | (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4);
      s[7] = (unsigned long long)(kt_end - kt_begin);
    }
  };
#endif

  // ---- epilogue: accumulator register r of a 32x32 tile = row (r&3)+8*(r>>2)+4*hi, column lane&31
  if (slot >= 0) {
    // K-split tile: every slice writes its partial sums as a dense BM x BN slab (no bounds: rows past M accumulated
    // zeros), then takes a ticket from the tile's arrival counter; the slice that draws the last ticket sums ALL
    // slabs in slot (= k) order -- its own included, read back from memory, so the result does not depend on who
    // arrived last -- and applies the epilogue.  Hand-off = cdna_hip_programming.md 6 Guideline 16 R1 / 5 'In-launch
    // split-K reduction', write-through form: every slab store carries sc1 and is drained (vmcnt(0)) by its wave
    // before the barrier, one lane takes the relaxed agent-scope ticket, and EVERY slab load of the reducer is an
    // sc1 load -- no release / acquire cache maintenance (the plain-store + fence form cost 5-12 us per workgroup
    // here: each release writes back the XCD's whole L2).  Correct for any placement of the slices on XCDs / CUs.
    // Slab layout is private to this kernel: each lane keeps the 16 registers of a 32x32 accumulator contiguous
    // (64 bytes), so a slab moves with four 16-byte accesses per accumulator instead of sixteen 4-byte ones.
    const unsigned lane_off = live_out ? (unsigned)((wgi * TM * TN * 64 + lane) * 16) * 4u : kOOB;
    const __amdgpu_buffer_rsrc_t rslab = make_rsrc(g.partial + (size_t)slot * (BM * BN), BM * BN * 4u);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          buf_store4_sc1(rslab, lane_off + (unsigned)(((i * TN + j) * 64 * 16 + q * 4) * 4),
                         make_float4(acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    volatile int* flag = reinterpret_cast<volatile int*>(lds);      // the staging array is free after the K loop
    if (tid == 0) {
      const unsigned ticket = __hip_atomic_fetch_add(g.counters + tile_id, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int last = ticket == (unsigned)(n_slices - 1);
      if (last) __hip_atomic_store(g.counters + tile_id, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
      flag[0] = last;
    }
    __syncthreads();
    if (flag[0] == 0) {
#ifdef RADNET_DIAG_STAMPS
      write_stamps();
#endif
      return;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");          // compiler-only: keeps the slab loads below the ticket
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // slices are ADDED in slot order (deterministic), but their loads are issued kGroup slices at a time: one memory
    // round trip per group instead of one per slice (a slice past the end reads from kOOB, i.e. zeros)
    constexpr int kGroup = (TM * TN == 1) ? 4 : (TM * TN == 2 ? 2 : 1);
    for (int s0 = 0; s0 < n_slices; s0 += kGroup) {
      float4 v[kGroup][TM * TN * 4];
#pragma unroll
      for (int u = 0; u < kGroup; ++u) {
        const __amdgpu_buffer_rsrc_t rsrc = make_rsrc(g.partial + (size_t)(slot0 + s0 + u) * (BM * BN), BM * BN * 4u);
        const unsigned off = (s0 + u < n_slices) ? lane_off : kOOB;
#pragma unroll
        for (int t = 0; t < TM * TN * 4; ++t) v[u][t] = buf_load4_sc1(rsrc, off + (unsigned)(((t >> 2) * 64 * 16 + (t & 3) * 4) * 4));
      }
#pragma unroll
      for (int u = 0; u < kGroup; ++u)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const float4 w = v[u][(i * TN + j) * 4 + q];
              acc[i][j][4 * q] += w.x; acc[i][j][4 * q + 1] += w.y; acc[i][j][4 * q + 2] += w.z; acc[i][j][4 * q + 3] += w.w;
            }
    }
  }
  // Branch-free like the operand loads, and with the same split of the address: per lane ONE offset per 32x32 tile (its
  // column in the tile's first row, kOOB for a column past N or a wave that holds no output), the row of accumulator
  // register r -- (r&3) + 8*(r>>2) rows further down -- in the SGPR offset.  Rows past M need no test: the descriptors end
  // with row M-1 (y_bytes = ((M-1)*ld + N)*4), the hardware drops the store / answers the load with 0.  Only the LOADS use
  // the SGPR operand: buffer stores with a non-zero SGPR offset ran the whole kernel at HALF speed on gfx950 (measured,
  // tools/concurrency_probe.py: 66 -> 33 TFLOP/s on a 1x1 layer), so the stores add the row offset in a VGPR.  All 16 residual
  // (and mask) loads of a 32x32 tile are issued back to back before the first store, so their latency is paid once per
  // tile instead of once per register (a conditional load -> store chain cannot be reordered by the compiler: y may
  // alias the addend).
  const __amdgpu_buffer_rsrc_t ry = make_rsrc(g.y + bz * g.y_bstride, g.y_bytes);
  const __amdgpu_buffer_rsrc_t radd = make_rsrc(g.addend, g.addend ? g.add_bytes : 0u);     // null -> every load returns 0
  const __amdgpu_buffer_rsrc_t rmask = make_rsrc(g.mask, g.mask ? g.mask_bytes : 0u);
  const bool has_mask = g.mask != nullptr;
  const unsigned ldy4 = (unsigned)g.ldy * 4u, lda4 = (unsigned)g.ld_add * 4u, ldm4 = (unsigned)g.ld_mask * 4u;
  // Round 4: straight-line code.  The first form tested `has_mask`, `act == 1`, `act == 2 && n < act_cols` per accumulator
  // register: the compiler kept them as branches -- 16 x (two scalar branches, a re-load of the kernel arguments with its wait,
  // for the mask an s_waitcnt vmcnt(0) per row) per 32x32 tile.  Now everything wave-uniform is decided once: the per-column
  // factors come through descriptors (null -> 0, replaced by 1 / 0 with a select), ReLU is a select on a uniform flag, the
  // sigmoid columns (rpn_out_class only) are a copy of the loop under ONE uniform branch, the mask exists in the dgrad form only.
  const bool has_scale = g.scale != nullptr, relu = g.act == 1;
  const __amdgpu_buffer_rsrc_t rsc = make_rsrc(g.scale, has_scale ? (unsigned)g.N * 4u : 0u);
  const __amdgpu_buffer_rsrc_t rsh = make_rsrc(g.shift, g.shift ? (unsigned)g.N * 4u : 0u);
  float scv[TN], shv[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int n = n0 + wn * (BN / WN) + j * 32 + l31;
    const unsigned off = n < g.N ? (unsigned)n * 4u : kOOB;
    scv[j] = buf_load1(rsc, off);
    shv[j] = buf_load1(rsh, off);
  }
  auto out_tiles = [&](auto sig_tag) {
    constexpr bool SIG = decltype(sig_tag)::value;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = n0 + wn * (BN / WN) + j * 32 + l31;
      const bool nv = n < g.N;
      const float sc = has_scale ? scv[j] : 1.f, sh = shv[j];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int mb = m0 + wm * (BM / WM) + i * 32 + 4 * hi;
        const bool col_ok = live_out & nv & (mb < g.M);        // mb >= M: every row of this lane is past the end
        const unsigned vy = col_ok ? ((unsigned)mb * (unsigned)g.ldy + (unsigned)n) * 4u : kOOB;
        const unsigned va = col_ok ? ((unsigned)mb * (unsigned)g.ld_add + (unsigned)n) * 4u : kOOB;
        const unsigned vm = col_ok ? ((unsigned)mb * (unsigned)g.ld_mask + (unsigned)n) * 4u : kOOB;
        float ad[16], mk[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
#ifdef RADNET_DIAG_SKIP_EPILOGUE                 // measurement only: 1 of 16 rows is loaded / stored
          if (r != 0) { ad[r] = 0.f; mk[r] = 1.f; continue; }
#endif
          const unsigned row = (unsigned)((r & 3) + 8 * (r >> 2));
          ad[r] = buf_load1s(radd, va, row * lda4);
          mk[r] = 1.f;
          if (BMODE == 1) mk[r] = buf_load1s(rmask, vm, row * ldm4);      // null mask: empty descriptor, reads 0 (selected away below)
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const unsigned row = (unsigned)((r & 3) + 8 * (r >> 2));
          float v = acc[i][j][r] * sc + sh + ad[r];
          if (BMODE == 1) v = (has_mask & !(mk[r] > 0.f)) ? 0.f : v;
          if (SIG) {
            const float sg = 1.f / (1.f + __expf(-v));
            v = n < g.act_cols ? sg : v;
          } else {
            const float vr = fmaxf(v, 0.f);
            v = relu ? vr : v;
          }
#ifdef RADNET_DIAG_SKIP_EPILOGUE
          if (r != 0) { asm volatile("" ::"v"(v)); continue; }
#endif
          if (COH) buf_store1_sc1(ry, vy + row * ldy4, v);
          else buf_store1(ry, vy + row * ldy4, v);      // one add; a STORE with a non-zero SGPR offset is slow (see above)
        }
      }
    }
  };
  if (g.act == 2) out_tiles(std::true_type{});
  else out_tiles(std::false_type{});
#ifdef RADNET_DIAG_STAMPS
  write_stamps();
#endif
}
}  // namespace
