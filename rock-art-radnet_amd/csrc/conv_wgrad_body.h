// ---- wgrad kernel -----------------------------------------------------------------------------------
// dW[k][n] (+)= sum_m im2col(x)[m][k] * (dy[m][n] * gscale[n]).  Output tile BMK (k) x BN (n); the
// reduction runs over output pixels m in steps of 32, optionally split across blockIdx.z (atomics).
#pragma once
#include "adam_update.h"
#include "conv_device.h"

namespace {
template <int BMK, int BN>
constexpr int wgrad_lds_floats() { return 2 * BK * ((BMK + 4) + (BN + 4)); }

// OPT: the epilogue honours the optimizer block of WgradArgs (conv_wgrad_multi_kernel); the other kernels' code is what it was.
template <int BMK, int BN, bool OPT = false>
__device__ __forceinline__ void conv_wgrad_body(const WgradArgs& g, float* __restrict__ lds, const unsigned bid_x, const unsigned bid_y, const unsigned bid_z) {
  constexpr int TM = BMK / 64, TN = BN / 64;
  constexpr int PA = BMK + 4, PB = BN + 4;
  constexpr int A_ITERS = BMK / 32, B_ITERS = BN / 32;
  constexpr int CPRA = BMK / 4, CPRB = BN / 4;
  float* sA0 = lds;
  float* sB0 = lds + 2 * BK * PA;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int hi = lane >> 5, l31 = lane & 31;
  const int wm = wave >> 1, wn = wave & 1;
  const int k0 = bid_x * BMK, n0 = bid_y * BN;

  // this block's k range lies inside one kernel position when C % BMK == 0 (launcher guarantees)
  const int pos = k0 / g.C;
  const int cbase = k0 - pos * g.C;

  const int a_k4 = tid % CPRA, a_mr = tid / CPRA;      // A_ITERS rows: a_mr + (NTHREADS/CPRA)*i
  const int b_n4 = tid % CPRB, b_mr = tid / CPRB;
  const bool a_kv = (k0 + a_k4 * 4) < g.K;
  const bool b_nv = (n0 + b_n4 * 4) < g.N;
  float4 gs = make_float4(1, 1, 1, 1);
  if (g.gscale != nullptr && b_nv) gs = *reinterpret_cast<const float4*>(g.gscale + n0 + b_n4 * 4);

  const int nmt = (g.M + BK - 1) / BK;
  const int zsplit = g.batch > 1 ? (int)(bid_z % (unsigned)g.splits) : (int)bid_z;
  const long long bp = g.batch > 1 ? (long long)(bid_z / (unsigned)g.splits) : 0;
  const int mt_begin = zsplit * g.mt_per_split;
  int mt_end = mt_begin + g.mt_per_split;
  if (mt_end > nmt) mt_end = nmt;

  const __amdgpu_buffer_rsrc_t rx = make_rsrc(reinterpret_cast<const char*>(g.x + bp * g.x_bstride) - g.x_bias, g.x_bytes + g.x_bias);
  const __amdgpu_buffer_rsrc_t rdy = make_rsrc(g.dy + bp * g.dy_bstride, g.dy_bytes);
  float4 ra[A_ITERS], rb[B_ITERS];
  // bias gradient: the workgroups of the first k tile see every (dy * gscale) row of their m range exactly once on
  // its way into LDS; they keep a running column sum and add it to db at the end (keras Conv2D bias / the beta-free
  // FixedBatchNormalization shift: d/db = sum over pixels of the scaled output gradient)
  const bool do_bias = g.db != nullptr && bid_x == 0;
  float4 csum = make_float4(0.f, 0.f, 0.f, 0.f);

  // Row table (host-built once per conv geometry, get_row_table): rowtab[tap][m] = byte offset of input pixel
  // (image, ih0 + kh, iw0 + kw, channel 0) of output row m -- kOOB where the tap falls into the padding or m >= M.  The
  // reduction index m advances by 32 per tile, so decoding m -> (image, oh, ow) inside the loop cost two multiply-high
  // divisions and three 16-cycle multiplies per load; with the table the gather is ONE vector add per load, everything
  // tile-dependent (table row, channel base, dy row, "tile past the end") is wave-uniform and sits in the loads' SGPR
  // offset (see conv_igemm_kernel).  The entries of tile t+2 are fetched while tile t is multiplied, one tile ahead of
  // the loads that use them.
  const __amdgpu_buffer_rsrc_t rtab = make_rsrc(g.rowtab + (size_t)pos * g.mpad, (unsigned)g.mpad * 4u);
  const unsigned s_tap = (unsigned)(cbase * 4);            // the tap is in the table; the k tile adds its first channel
  unsigned b_voff[B_ITERS], e_voff[A_ITERS];
#pragma unroll
  for (int i = 0; i < B_ITERS; ++i) b_voff[i] = b_nv ? (unsigned)(((b_mr + (NTHREADS / CPRB) * i) * g.ld_dy + n0 + b_n4 * 4) * 4) : kOOB;
#pragma unroll
  for (int i = 0; i < A_ITERS; ++i) e_voff[i] = (unsigned)((a_mr + (NTHREADS / CPRA) * i) * 4);
  const unsigned a_lane = a_kv ? (unsigned)a_k4 * 16u : kOOB;
  const unsigned dy_tile_bytes = (unsigned)(BK * g.ld_dy * 4);
  struct Entries {
    unsigned e[A_ITERS];
  };
  Entries ent0, ent1;

  constexpr int kLoadOps = A_ITERS + B_ITERS, kStoreOps = A_ITERS + B_ITERS;
  auto entry_op = [&](int i, int mt, Entries& en) {
    en.e[i] = __builtin_amdgcn_raw_buffer_load_b32(rtab, (int)e_voff[i], (int)__builtin_amdgcn_readfirstlane(mt < mt_end ? (unsigned)mt * (BK * 4u) : kOOB), 0);
  };
  auto load_op = [&](int idx, int mt, const Entries& en) {
    const bool live = mt < mt_end;         // a dead tile's table entries read 0: its loads go out of range through the SGPR offset
    if (idx < A_ITERS) {
      ra[idx] = buf_load4s(rx, en.e[idx] + a_lane, live ? s_tap : kOOB);
    } else {
      // rows past M lie past the end of the dy descriptor
      rb[idx - A_ITERS] = buf_load4s(rdy, b_voff[idx - A_ITERS], live ? (unsigned)mt * dy_tile_bytes : kOOB);
    }
  };
  auto store_op = [&](int idx, int buf) {
    float* sA = sA0 + buf * BK * PA;
    float* sB = sB0 + buf * BK * PB;
    if (idx < A_ITERS) {
      const int i = idx;
      *reinterpret_cast<float4*>(sA + (a_mr + (NTHREADS / CPRA) * i) * PA + a_k4 * 4) = ra[i];
    } else {
      const int i = idx - A_ITERS;
      float4 v = rb[i];
      v.x *= gs.x; v.y *= gs.y; v.z *= gs.z; v.w *= gs.w;
      *reinterpret_cast<float4*>(sB + (b_mr + (NTHREADS / CPRB) * i) * PB + b_n4 * 4) = v;
      // rows past M / columns past N / tiles past the end were loaded as 0
      csum.x += do_bias ? v.x : 0.f; csum.y += do_bias ? v.y : 0.f; csum.z += do_bias ? v.z : 0.f; csum.w += do_bias ? v.w : 0.f;
    }
  };

  constexpr int CH = (TM * TN >= 4) ? 1 : kChainsSmallTile;     // independent accumulator sets, see mfma_tile
  f32x16 accs[CH][TM][TN];
#pragma unroll
  for (int c = 0; c < CH; ++c)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) accs[c][i][j][r] = 0.f;

  if (mt_begin < mt_end) {
#pragma unroll
    for (int i = 0; i < A_ITERS; ++i) entry_op(i, mt_begin, ent0);
#pragma unroll
    for (int op = 0; op < kLoadOps; ++op) load_op(op, mt_begin, ent0);
#pragma unroll
    for (int i = 0; i < A_ITERS; ++i) entry_op(i, mt_begin + 1, ent1);
#pragma unroll
    for (int op = 0; op < kStoreOps; ++op) store_op(op, 0);
    __syncthreads();
    const int a_off = hi * PA + wm * (BMK / 2) + l31;
    const int b_off = hi * PB + wn * (BN / 2) + l31;
    // Same dealing-out of the staging operations between the MFMA steps as the forward kernel (one basic block per
    // tile, past-the-end tiles load from kOOB): steps 0.. carry the loads of tile mt+1 (and the table entries of
    // tile mt+2), the last steps but one its LDS stores -- one register stage, the loads have 7+ MFMA steps to land.
    constexpr int kSteps = BK / 2;
    constexpr int kStoreSteps = (kStoreOps < kSteps - 1 - kLoadOps) ? kStoreOps : kSteps - 1 - kLoadOps;
    constexpr int kStoresPerStep = (kStoreOps + kStoreSteps - 1) / kStoreSteps;
    constexpr int kFirstStoreStep = kSteps - 1 - kStoreSteps;
    static_assert(kStoreSteps >= 1, "tile too large for the 16-step staging schedule");
    auto step = [&](int mt, int buf, Entries& cur, Entries& nxt) {   // cur: entries of tile mt+1, nxt: receives mt+2
      mfma_tile<TM, TN, CH>(sA0 + buf * BK * PA, sB0 + buf * BK * PB, PA, PB, a_off, b_off, accs, [&](int s) {
        if (s < kLoadOps) {
          load_op(s, mt + 1, cur);
          if (s < A_ITERS) entry_op(s, mt + 2, nxt);
        } else if (s >= kFirstStoreStep && s < kSteps - 1) {
#pragma unroll
          for (int q = 0; q < kStoresPerStep; ++q) {
            const int op = (s - kFirstStoreStep) * kStoresPerStep + q;
            if (op < kStoreOps) store_op(op, buf ^ 1);
          }
        }
      });
      __syncthreads();
    };
    for (int mt = mt_begin; mt < mt_end; mt += 2) {
      step(mt, 0, ent1, ent0);
      if (mt + 1 < mt_end) step(mt + 1, 1, ent0, ent1);
    }
  }
  f32x16(&acc)[TM][TN] = accs[0];
#pragma unroll
  for (int c = 1; c < CH; ++c)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] += accs[c][i][j];

  const bool ordered = g.slabs != nullptr;      // uniform for the launch
  float4 bias_t = make_float4(0.f, 0.f, 0.f, 0.f);
  if (do_bias) {             // uniform per workgroup; the staging array is free after the loop's last barrier
    float4* red = reinterpret_cast<float4*>(lds);
    red[tid] = csum;
    __syncthreads();
    if (tid < CPRB) {
      float4 t = red[tid];
      for (int q = 1; q < NTHREADS / CPRB; ++q) {
        const float4 u = red[tid + q * CPRB];
        t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
      }
      bias_t = t;
      const int n = n0 + tid * 4;
      if (!ordered && n < g.N) {           // N is a multiple of 4
        atomicAdd(g.db + n, t.x);
        atomicAdd(g.db + n + 1, t.y);
        atomicAdd(g.db + n + 2, t.z);
        atomicAdd(g.db + n + 3, t.w);
      }
    }
    __syncthreads();
  }

  if (ordered) {
    // Same hand-off as the forward kernel's split-K (see there): sc1 slab stores drained before the barrier, one relaxed
    // agent-scope ticket per workgroup, the last arriver reads every slab back with sc1 loads and adds them in split order,
    // so the sum does not depend on which split came last.  The bias partials of the first k tile's workgroups travel the
    // same way.
    const unsigned tile = ((unsigned)bp * (unsigned)g.tiles_y + bid_y) * (unsigned)g.tiles_x + bid_x;
    const unsigned lane_off = (unsigned)((wave * TM * TN * 64 + lane) * 16) * 4u;
    const size_t total_tiles = (size_t)(g.batch > 1 ? g.batch : 1) * g.tiles_y * g.tiles_x;
    const __amdgpu_buffer_rsrc_t rslab = make_rsrc(g.slabs + ((size_t)tile * g.splits + zsplit) * (BMK * BN), BMK * BN * 4u);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          buf_store4_sc1(rslab, lane_off + (unsigned)(((i * TN + j) * 64 * 16 + q * 4) * 4),
                         make_float4(acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]));
    float* bias_slabs = g.slabs + total_tiles * g.splits * (size_t)(BMK * BN) + ((size_t)((unsigned)bp * g.tiles_y + bid_y) * g.splits) * BN;
    if (do_bias && tid < CPRB) {
      const __amdgpu_buffer_rsrc_t rb = make_rsrc(bias_slabs + (size_t)zsplit * BN, BN * 4u);
      buf_store4_sc1(rb, (unsigned)tid * 16u, bias_t);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    volatile int* flag = reinterpret_cast<volatile int*>(lds);
    if (tid == 0) {
      const unsigned ticket = __hip_atomic_fetch_add(g.counters + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int last = ticket == (unsigned)(g.splits - 1);
      if (last) __hip_atomic_store(g.counters + tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
      flag[0] = last;
    }
    __syncthreads();
    if (flag[0] == 0) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");          // compiler-only: keeps the slab loads below the ticket
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    constexpr int kGroup = (TM * TN == 1) ? 4 : 1;      // slabs in flight per round trip, bounded by the register budget of the K loop
    for (int s0 = 0; s0 < g.splits; s0 += kGroup) {
      float4 v[kGroup][TM * TN * 4];
#pragma unroll
      for (int u = 0; u < kGroup; ++u) {
        const __amdgpu_buffer_rsrc_t rsrc = make_rsrc(g.slabs + ((size_t)tile * g.splits + (s0 + u < g.splits ? s0 + u : 0)) * (BMK * BN), BMK * BN * 4u);
        const unsigned off = (s0 + u < g.splits) ? lane_off : kOOB;
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
    if (do_bias && tid < CPRB) {
      float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int z = 0; z < g.splits; ++z) {
        const __amdgpu_buffer_rsrc_t rb = make_rsrc(bias_slabs + (size_t)z * BN, BN * 4u);
        const float4 u = buf_load4_sc1(rb, (unsigned)tid * 16u);
        t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
      }
      const int n = n0 + tid * 4;
      if (n < g.N) {           // this workgroup is the only writer of db[n0 .. n0+BN) in the launch
        g.db[n] += t.x; g.db[n + 1] += t.y; g.db[n + 2] += t.z; g.db[n + 3] += t.w;
      }
    }
  }

  if (!ordered && g.atomic) {                    // RADNET_DETERMINISTIC=0: the splits add with fp32 atomics
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = n0 + wn * (BN / 2) + j * 32 + l31;
#pragma unroll
      for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int k = k0 + wm * (BMK / 2) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
          if (n < g.N && k < g.K) atomicAdd(g.dw + bp * g.dw_bstride + (size_t)k * g.ldw + n, acc[i][j][r]);
        }
      }
    }
    return;
  }
  if constexpr (OPT) {
    // Adam in the tile epilogue: this workgroup holds the final value of its tile -- its own sum when the launch is not split, the
    // ordered sum of the slices as their last arriver -- and no launch of the step reads the layer's weights any more (all data
    // gradients ran before this launch), so it updates w, m, v at the tile's place and the gradient never travels through memory.
    // Same element order as the stores below; adam_update1 is the routine of adam_kernel, bit for bit.
    if (g.ow != nullptr) {             // uniform for the problem
      const unsigned bytes = (unsigned)((size_t)g.K * (size_t)g.ldw * 4u);
      const __amdgpu_buffer_rsrc_t rw = make_rsrc(g.ow + bp * g.dw_bstride, bytes), rm = make_rsrc(g.om + bp * g.dw_bstride, bytes),
                                   rv = make_rsrc(g.ov + bp * g.dw_bstride, bytes);
      const unsigned ldw4 = (unsigned)g.ldw * 4u;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn * (BN / 2) + j * 32 + l31;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const int kb = k0 + wm * (BMK / 2) + i * 32 + 4 * hi;
          const unsigned voff = (n < g.N && kb < g.K) ? ((unsigned)kb * (unsigned)g.ldw + (unsigned)n) * 4u : kOOB;
          float pw[16], pm[16], pv[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const unsigned off = voff + (unsigned)((r & 3) + 8 * (r >> 2)) * ldw4;
            pw[r] = buf_load1(rw, off);
            pm[r] = buf_load1(rm, off);
            pv[r] = buf_load1(rv, off);
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const unsigned off = voff + (unsigned)((r & 3) + 8 * (r >> 2)) * ldw4;
            adam_update1(pw[r], acc[i][j][r], pm[r], pv[r], g.lr_t, g.beta1, g.beta2, g.eps, g.grad_scale);
            buf_store1(rw, off, pw[r]);
            buf_store1(rm, off, pm[r]);
            buf_store1(rv, off, pv[r]);
          }
        }
      }
      return;
    }
  }
  // Plain stores / ordered accumulate, straight-line (round 4; the first form decided ordered / accumulate / atomic and the two
  // bounds per accumulator register -- five branches each, and in accumulate mode a load + wait + store round trip per register):
  // rows past K and columns past N fall outside the descriptor, accumulate mode reads a tile's 16 old values in one round trip.
  const __amdgpu_buffer_rsrc_t rdw = make_rsrc(g.dw + bp * g.dw_bstride, (unsigned)((size_t)g.K * (size_t)g.ldw * 4u));
  const bool rmw = ordered && g.accumulate;
  const unsigned ldw4 = (unsigned)g.ldw * 4u;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int n = n0 + wn * (BN / 2) + j * 32 + l31;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int kb = k0 + wm * (BMK / 2) + i * 32 + 4 * hi;
      const unsigned voff = (n < g.N && kb < g.K) ? ((unsigned)kb * (unsigned)g.ldw + (unsigned)n) * 4u : kOOB;
      float old[16];
      if (rmw) {
#pragma unroll
        for (int r = 0; r < 16; ++r) old[r] = buf_load1(rdw, voff + (unsigned)((r & 3) + 8 * (r >> 2)) * ldw4);
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) old[r] = 0.f;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) buf_store1(rdw, voff + (unsigned)((r & 3) + 8 * (r >> 2)) * ldw4, rmw ? old[r] + acc[i][j][r] : acc[i][j][r]);
    }
  }
}
}  // namespace
