// Forward and data-gradient convolutions on the fp32 matrix cores: the kernels around conv_igemm_body (conv_igemm_body.h), their
// launch policy (tile choice, work-unit tables, the autotuner of run_igemm) and the C entry points.  Weight gradients:
// conv_wgrad.hip; the chain kernel: chain.hip.
#include "conv_host.h"
#include "conv_igemm_body.h"

namespace {
template <int BM, int BN, int WAVES>
__global__ void __launch_bounds__(64 * WAVES) conv_igemm_persist_kernel(GemmArgs g) {
  __shared__ __attribute__((aligned(16))) float lds[igemm_lds_floats<BM, BN, 0>() + igemm_persist_scratch_floats<BM, BN, WAVES>()];
  if (g.xcd_batch) {                    // see conv_igemm_kernel
    const unsigned gx = gridDim.x, gy = gridDim.y, total = gx * gy * gridDim.z;
    const unsigned lin = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z), per = total >> 3;
    const unsigned l2 = lin < (per << 3) ? (lin & 7u) * per + (lin >> 3) : lin;
    const unsigned z = l2 / (gx * gy), r = l2 - z * gx * gy, y = r / gx;
    conv_igemm_body<BM, BN, 0, false, WAVES, false, true>(g, lds, r - y * gx, y, z, gx);
    return;
  }
  conv_igemm_body<BM, BN, 0, false, WAVES, false, true>(g, lds, blockIdx.x, blockIdx.y, blockIdx.z, gridDim.x);
}

template <int BM, int BN, int BMODE, bool SMALLC, int WAVES>
__global__ void __launch_bounds__(64 * WAVES) conv_igemm_kernel(GemmArgs g) {
  __shared__ __attribute__((aligned(16))) float lds[igemm_lds_floats<BM, BN, BMODE>()];
  if (g.batch > 1 && g.xcd_batch) {
    // The hardware deals workgroup L (x fastest, then y, z) to XCD L % 8, and every XCD has its own L2: the tiles of ONE problem of
    // the batch -- which share that problem's operands (a Winograd position's filter slice is read by every row tile, its
    // transformed input by every column tile) -- land on eight L2s and each fetches its own copy (rpn_conv1's 36 GEMMs: 306 MB
    // fetched for 111 MB of operands).  Renumbered, XCD k runs the contiguous range [k, k + 1) * total / 8 of (problem, tile).
    const unsigned gx = gridDim.x, gy = gridDim.y, total = gx * gy * gridDim.z;
    const unsigned lin = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z), per = total >> 3;
    const unsigned l2 = lin < (per << 3) ? (lin & 7u) * per + (lin >> 3) : lin;
    const unsigned z = l2 / (gx * gy), r = l2 - z * gx * gy, y = r / gx;
    conv_igemm_body<BM, BN, BMODE, SMALLC, WAVES>(g, lds, r - y * gx, y, z, gx);
    return;
  }
  conv_igemm_body<BM, BN, BMODE, SMALLC, WAVES>(g, lds, blockIdx.x, blockIdx.y, blockIdx.z, gridDim.x);
}

// 3x3 conv + the pointwise convs behind it (bneck_tail): one workgroup per BM output rows, all 64 channels of the 3x3
template <int BM, int WAVES, int FUSE>
__global__ void __launch_bounds__(64 * WAVES) conv_bneck_kernel(GemmArgs g, TailArgs tz) {
  constexpr int kLds = igemm_lds_floats<BM, 64, 0>() > bneck_lds_floats<BM>() ? igemm_lds_floats<BM, 64, 0>() : bneck_lds_floats<BM>();
  __shared__ __attribute__((aligned(16))) float lds[kLds];
  conv_igemm_body<BM, 64, 0, false, WAVES, false, false, FUSE>(g, lds, blockIdx.x, 0u, 0u, gridDim.x, &tz);
}

// Two INDEPENDENT forward problems as one launch (round 4: branch2a and the shortcut conv of a conv_block read the same input,
// resnet50.py:100,111): workgroups [0, n1) run the first, [n1, n1 + n2) the second -- one launch floor (~4 us + a lockstep
// prologue / epilogue) instead of two, and the narrow branch2a grid (N = 128 .. 512) no longer has the chip to itself.  Plain grids,
// one tile shape for both.
template <int BM, int BN>
__global__ void __launch_bounds__(256) conv_fwd_pair_kernel(GemmArgs g1, GemmArgs g2, unsigned n1, unsigned gx1, unsigned gx2) {
  __shared__ __attribute__((aligned(16))) float lds[igemm_lds_floats<BM, BN, 0>()];
  const unsigned b = blockIdx.x;
  if (b < n1) {
    const unsigned by = b / gx1;
    conv_igemm_body<BM, BN, 0, false, 4>(g1, lds, b - by * gx1, by, 0u, gx1);
  } else {
    const unsigned c = b - n1, by = c / gx2;
    conv_igemm_body<BM, BN, 0, false, 4>(g2, lds, c - by * gx2, by, 0u, gx2);
  }
}

// ---- launch helpers -----------------------------------------------------------------------------------
struct TileChoice {
  int bm, bn, splits;
  int waves = 4;         // waves per workgroup (4, or 8 = K tile halved between two wave grids)
};

// Pick the output tile and split-K factor.  Cost model (CU-time in MAC units, 128 MAC/clk/CU):
//   rounds = ceil(units / 256 CUs); unit = tile MACs / tile efficiency + fixed prologue/epilogue cost;
//   split-K adds the partial-sum write + reduce pass and one more launch.
// ctx->tune (radnet_conv_autotune) replaces this guess with measured choices per problem shape.
TileChoice choose_tiles(int M, int N, int K, bool allow_split) {
  const int cand[4][2] = {{128, 128}, {128, 64}, {64, 128}, {64, 64}};
  const double eff[4] = {1.0, 0.95, 0.95, 0.85};
  const double kMacPerUs = 128.0 * 2100.0;          // per CU
  const double kFixed = 2.0 * kMacPerUs;            // ~2 us per work unit
  TileChoice best{64, 64, 1};
  double best_cost = 1e30;
  const int nk = radnet_cdiv(K, BK);
  for (int c = 0; c < 4; ++c) {
    const int bm = cand[c][0], bn = cand[c][1];
    if (bn > 64 && N <= 64) continue;
    if (bm > 64 && M <= 64) continue;
    const long long tiles = (long long)radnet_cdiv(M, bm) * radnet_cdiv(N, bn);
    for (int s = 1; s <= (allow_split ? 16 : 1); ++s) {
      if (s > 1 && nk / s < 6) break;
      const int kt = radnet_cdiv(nk, s);
      if (s > 1 && radnet_cdiv(nk, kt) != s) continue;   // would leave an empty split
      const long long units = tiles * s;
      const double rounds = (double)((units + kNumCU - 1) / kNumCU);
      double cost = rounds * ((double)bm * bn * kt * BK / eff[c] + kFixed);
      if (s > 1) cost += (2.0 + 8.0 * (double)M * N * s / 3.0e6) * kMacPerUs;
      if (cost < best_cost) {
        best_cost = cost;
        best = TileChoice{bm, bn, s};
      }
    }
  }
  return best;
}

// Work-unit table for a K-split launch: a unit = (output tile, K slice).  Whole-tile units apply the epilogue
// themselves (slot -1); the slices of a split tile write partial slabs and the last to arrive reduces them in the
// same launch (arrival counter per tile).  Tables live in device memory owned by the context (cached per shape).
radnet_unit_table* get_unit_table(radnet_ctx* ctx, int M, int N, int K, int bm, int bn, int chunks) {
  const std::array<int, 6> key{M, N, K, bm, bn, chunks};
  auto it = ctx->unit_tables.find(key);
  if (it != ctx->unit_tables.end()) return &it->second;
  const int Mt = radnet_cdiv(M, bm), Nt = radnet_cdiv(N, bn), nk = radnet_cdiv(K, BK);
  const long long T = (long long)Mt * Nt;
  std::vector<int> units;
  // Measured on MI355X: cutting the linearised iteration space into equal chunks (true stream-K) balances the CUs but
  // lost 15-20 % against the uniform split below, because the order of the units decides what the XCD L2s can
  // share: units that run together must read the SAME weight k-range (consecutive M tiles of one N tile and one
  // k slice).  So: `chunks` = slices per tile, units ordered (slice, tile_n, tile_m) -- tile_m fastest.
  const int S = chunks < 0 ? -chunks : chunks, kt = radnet_cdiv(nk, S);
  const int S_eff = radnet_cdiv(nk, kt);                      // no empty slice
  int slots = (int)T * S_eff;
  for (int s = 0; s < S_eff; ++s)
    for (int tn = 0; tn < Nt; ++tn)
      for (int tm = 0; tm < Mt; ++tm) {
        const int tile = tn * Mt + tm;
        // {tile_m, tile_n, kt_begin, kt_end | slot (-1 = whole tile, direct epilogue), first slot, slices, tile index}
        const int u[8] = {tm, tn, s * kt, std::min(nk, (s + 1) * kt), S_eff > 1 ? tile * S_eff + s : -1, tile * S_eff, S_eff, tile};
        units.insert(units.end(), u, u + 8);
      }
  if (S_eff <= 1) slots = 0;
  if (chunks < 0) {
    // XCD-aware order (chunks < 0): the hardware deals workgroup b to XCD b % 8, each XCD has its own 4 MiB L2.
    // Give every XCD a CONTIGUOUS run of the logical unit list, so the workgroups sharing one L2 are consecutive
    // M tiles of one (slice, N tile) and read the same weight rows.  Bijective for any unit count.
    const int U = (int)units.size() / 8, q = U / 8, r = U % 8;
    std::vector<int> hw(units.size());
    for (int b = 0; b < U; ++b) {
      const int x = b % 8, j = b / 8;
      const int base = x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q;
      std::copy(units.begin() + 8 * (size_t)(base + j), units.begin() + 8 * (size_t)(base + j) + 8, hw.begin() + 8 * (size_t)b);
    }
    units.swap(hw);
  }
  radnet_unit_table tb{};
  tb.n_units = (int)units.size() / 8;
  tb.n_split_tiles = S_eff > 1 ? (int)T : 0;
  tb.n_slots = slots;
  if (hipMalloc(&tb.d_units, units.size() * sizeof(int)) != hipSuccess) return nullptr;
  if (hipMemcpy(tb.d_units, units.data(), units.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
  if (tb.n_split_tiles) {
    // arrival counters: zeroed here once; every launch leaves them at zero again (the reducer resets its tile's)
    if (hipMalloc(&tb.d_counters, (size_t)T * sizeof(unsigned)) != hipSuccess) return nullptr;
    if (hipMemset(tb.d_counters, 0, (size_t)T * sizeof(unsigned)) != hipSuccess) return nullptr;
  }
  auto ins = ctx->unit_tables.emplace(key, tb);
  return &ins.first->second;
}

template <int BMODE, bool SMALLC, int WAVES>
void launch_igemm_w(hipStream_t st, const GemmArgs& g, const TileChoice& tc, dim3 grid, hipEvent_t e0, hipEvent_t e1) {
  dim3 block(64 * WAVES);
  // (capping workgroups per CU with extra dynamic LDS was measured: 7-25 % slower on every layer -- co-residency wins)
  if constexpr (WAVES == 4 && !SMALLC) {        // the 32-row tiles exist in the 4-wave form only (8 waves: fewer than one A chunk per thread)
    if (tc.bm == 32 && tc.bn == 64) { RADNET_LAUNCH((conv_igemm_kernel<32, 64, BMODE, SMALLC, WAVES>), grid, block, 0, st, e0, e1, g); return; }
    if (tc.bm == 32 && tc.bn == 32) { RADNET_LAUNCH((conv_igemm_kernel<32, 32, BMODE, SMALLC, WAVES>), grid, block, 0, st, e0, e1, g); return; }
  }
  if (tc.bm == 128 && tc.bn == 128) RADNET_LAUNCH((conv_igemm_kernel<128, 128, BMODE, SMALLC, WAVES>), grid, block, 0, st, e0, e1, g);
  else if (tc.bm == 128 && tc.bn == 64) RADNET_LAUNCH((conv_igemm_kernel<128, 64, BMODE, SMALLC, WAVES>), grid, block, 0, st, e0, e1, g);
  else if (tc.bm == 64 && tc.bn == 128) RADNET_LAUNCH((conv_igemm_kernel<64, 128, BMODE, SMALLC, WAVES>), grid, block, 0, st, e0, e1, g);
  else RADNET_LAUNCH((conv_igemm_kernel<64, 64, BMODE, SMALLC, WAVES>), grid, block, 0, st, e0, e1, g);
}

// persistent batched launch: the tile shapes that have the PERSIST form (forward, channel-tiled, 4 waves)
inline bool persist_shape(const TileChoice& tc) {
  return tc.waves != 8 && ((tc.bm == 64 && tc.bn == 64) || (tc.bm == 32 && tc.bn == 64) || (tc.bm == 64 && tc.bn == 128) || (tc.bm == 32 && tc.bn == 32));
}
void launch_igemm_persist(hipStream_t st, const GemmArgs& g, const TileChoice& tc, hipEvent_t e0, hipEvent_t e1) {
  dim3 grid(radnet_cdiv(g.M, tc.bm), radnet_cdiv(g.N, tc.bn), radnet_cdiv(g.batch, g.zper)), block(256);
  if (tc.bm == 64 && tc.bn == 64) RADNET_LAUNCH((conv_igemm_persist_kernel<64, 64, 4>), grid, block, 0, st, e0, e1, g);
  else if (tc.bm == 32 && tc.bn == 64) RADNET_LAUNCH((conv_igemm_persist_kernel<32, 64, 4>), grid, block, 0, st, e0, e1, g);
  else if (tc.bm == 64 && tc.bn == 128) RADNET_LAUNCH((conv_igemm_persist_kernel<64, 128, 4>), grid, block, 0, st, e0, e1, g);
  else RADNET_LAUNCH((conv_igemm_persist_kernel<32, 32, 4>), grid, block, 0, st, e0, e1, g);
}

template <int BMODE, bool SMALLC>
void launch_igemm(hipStream_t st, const GemmArgs& g, const TileChoice& tc, int n_units, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr) {
  dim3 grid(radnet_cdiv(g.M, tc.bm), radnet_cdiv(g.N, tc.bn), g.batch > 1 ? g.batch : 1);
  if (g.units != nullptr) grid = dim3(n_units, 1, 1);
  if (tc.waves == 8) launch_igemm_w<BMODE, SMALLC, 8>(st, g, tc, grid, e0, e1);
  else launch_igemm_w<BMODE, SMALLC, 4>(st, g, tc, grid, e0, e1);
}

// checks + derived fields of a forward / data-gradient problem (descriptor extents, division constants)
int prepare_igemm(radnet_ctx* ctx, GemmArgs& g, int bmode, bool smallc) {
  if (g.M <= 0 || g.N <= 0 || g.K <= 0) RADNET_FAIL(ctx, RADNET_ERR_ARG, "conv: empty problem M=%d N=%d K=%d", g.M, g.N, g.K);
  if (g.M >= (1 << 20) || g.OHOW >= (1 << 20)) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "conv: M=%d exceeds 2^20 rows", g.M);
  if ((g.ldw & 3) || (g.N & 3)) RADNET_FAIL(ctx, RADNET_ERR_ARG, "conv: N=%d and ldw=%d must be multiples of 4", g.N, g.ldw);
  if (((uintptr_t)g.x & 15) || ((uintptr_t)g.w & 15)) RADNET_FAIL(ctx, RADNET_ERR_ARG, "conv: x / w must be 16-byte aligned");
  if (!smallc && (g.C % BK) != 0) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "conv: channels %d not a multiple of %d (pad, or use c=4)", g.C, BK);
  if (!smallc && g.npos > 32) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "conv: %d kernel taps (the padding mask of a row holds 32)", g.npos);
  g.magic_ohow = radnet_div_magic((uint32_t)g.OHOW);
  g.magic_ow = radnet_div_magic((uint32_t)g.OW);
  {
    const uint64_t xb = (uint64_t)(g.M / g.OHOW) * g.H * g.W * g.C * 4ull;      // images * H * W * C floats
    const uint64_t wb = (bmode == 0) ? (uint64_t)g.K * g.ldw * 4ull : (uint64_t)g.npos * g.cin_fwd * g.ldw * 4ull;
    // x is addressed through a descriptor that starts one halo (pad_t rows + pad_l pixels) early: that too stays below 2^31
    const uint64_t halo = ((uint64_t)g.pad_t * g.W + g.pad_l) * g.C * 4ull;
    if (xb + halo >= (1ull << 31) || wb >= (1ull << 31)) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "conv: tensor larger than 2 GiB");
    g.x_bytes = (unsigned)xb;
    g.w_bytes = (unsigned)wb;
    const uint64_t ld_max = (uint64_t)std::max(g.ldy, std::max(g.addend ? g.ld_add : 0, g.mask ? g.ld_mask : 0));
    if ((uint64_t)g.M * ld_max * 4ull >= (1ull << 31)) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "conv: output larger than 2 GiB");
    if (g.ldy < g.N || (g.addend && g.ld_add < g.N) || (g.mask && g.ld_mask < g.N))
      RADNET_FAIL(ctx, RADNET_ERR_ARG, "conv: output / addend / mask row pitch smaller than n=%d", g.N);
    // last row ends at column N, not at the pitch: the tensor may be a column block of a wider one
    g.y_bytes = (unsigned)(((uint64_t)(g.M - 1) * g.ldy + g.N) * 4ull);
    g.add_bytes = g.addend ? (unsigned)(((uint64_t)(g.M - 1) * g.ld_add + g.N) * 4ull) : 0u;
    g.mask_bytes = g.mask ? (unsigned)(((uint64_t)(g.M - 1) * g.ld_mask + g.N) * 4ull) : 0u;
  }
  g.stamps = ctx->diag_stamps;
#ifdef RADNET_DIAG_STAMPS
  if (getenv("RADNET_DIAG_NOMEM")) g.x_bytes = g.w_bytes = 0;   // every operand load out of range: returns 0 without touching memory
#endif
  return RADNET_OK;
}

int run_igemm(radnet_ctx* ctx, GemmArgs& g, int bmode, bool smallc, int cls) {
  {
    const int rcp = prepare_igemm(ctx, g, bmode, smallc);
    if (rcp != RADNET_OK) return rcp;
  }
  const int nk = radnet_cdiv(g.K, BK);
  // TileChoice.splits = number of equal work chunks the iteration space is cut into (0/1 = one workgroup per tile)
  auto launch = [&](const TileChoice& t) -> int {
    radnet_unit_table* tb = nullptr;
    g.units = nullptr;
    g.partial = nullptr;
    g.counters = nullptr;
    // a batch is its own source of workgroups: no K slices.  |slices| = z > 1 on a batch = the persistent form, z consecutive problems
    // per workgroup (plain epilogue, dense problem strides, forward only, the tile shapes of persist_shape)
    g.zper = 0;
    if (g.batch > 1 && t.splits != 1 && t.splits != -1) {
      const int z = t.splits < 0 ? -t.splits : t.splits;
      const bool plain = !g.scale && !g.shift && !g.addend && !g.mask && !g.in_scale && g.act == 0 && g.npos == 1 && g.stride == 1;
      if (bmode != 0 || smallc || !plain || !persist_shape(t) || z > 12 || z > g.batch || g.x_bstride != (long long)g.M * g.C ||
          g.w_bstride != (long long)g.K * g.ldw || (uint64_t)z * (uint64_t)std::max(g.x_bstride, g.w_bstride) * 4ull >= (1ull << 31))
        return RADNET_ERR_UNSUPPORTED;
      g.zper = z;
    }
    if (t.bm < 64 || t.bn < 64) {               // 32-row tiles: 4 waves, channel-tiled layers, 32x64 and 32x32 only
      if (t.waves == 8 || smallc || t.bm != 32 || (t.bn != 64 && t.bn != 32)) return RADNET_ERR_UNSUPPORTED;
    }
    g.xcd_batch = (g.batch > 1 && t.splits < 0) ? 1 : 0;          // negative: the same grid, XCD-contiguous numbering
    if (g.batch <= 1 && (t.splits > 1 || t.splits < 0)) {
      tb = get_unit_table(ctx, g.M, g.N, g.K, t.bm, t.bn, t.splits);
      if (!tb) RADNET_FAIL(ctx, RADNET_ERR_HIP, "conv: cannot build the work-unit table");
      if ((uint64_t)tb->n_slots * t.bm * t.bn * sizeof(float) > ctx->ws_bytes) return RADNET_ERR_UNSUPPORTED;   // candidate skipped
      if (tb->n_split_tiles > 0 || t.splits < 0) {  // an un-split, un-swizzled table is just the plain launch
        g.units = tb->d_units;
        g.partial = (float*)ctx->ws;
        g.counters = tb->d_counters;
      } else {
        tb = nullptr;
      }
    }
    const int n_units = tb ? tb->n_units : 0;
    if (ctx->pair_capture != nullptr) {
      PairCapture* pc = (PairCapture*)ctx->pair_capture;
      pc->have_a = true;
      pc->a_ok = bmode == 1 && !smallc && (t.bm == 64 || t.bm == 32) && t.bn == 64 && t.waves != 8 && g.batch <= 1;
      pc->a_bm = t.bm;
      pc->ga = g;
      pc->a_slab_bytes = tb ? (uint64_t)tb->n_slots * t.bm * t.bn * sizeof(float) : 0;
      pc->ax = g.units != nullptr ? (unsigned)n_units : (unsigned)radnet_cdiv(g.M, t.bm);
      pc->ay = g.units != nullptr ? 1u : (unsigned)radnet_cdiv(g.N, t.bn);
      pc->flops += 2.0 * g.M * g.N * g.K;
      return RADNET_OK;
    }
    if (g.zper > 1) {
      launch_igemm_persist(ctx->stream, g, t, ctx->arm0, ctx->arm1);
    } else if (bmode == 0) {
      if (smallc) launch_igemm<0, true>(ctx->stream, g, t, n_units, ctx->arm0, ctx->arm1);
      else launch_igemm<0, false>(ctx->stream, g, t, n_units, ctx->arm0, ctx->arm1);
    } else {
      launch_igemm<1, false>(ctx->stream, g, t, n_units, ctx->arm0, ctx->arm1);
    }
    RADNET_CHECK_LAUNCH(ctx, "conv_igemm");
    return RADNET_OK;
  };
  // tile / split-K choice: measured once per problem shape when autotuning is on, else the cost model
  const radnet_shape_key key{g.batch > 1 ? 8 : (cls == 1 ? 1 : 0), g.M, g.N, g.K, g.C, g.npos, g.batch > 1 ? g.batch : g.stride};
  TileChoice tc{64, 64, 1};
  auto it = ctx->tuned->find(key);
  if (ctx->force_a > 0) {                      // radnet_force_config: tests sweep every tile / slice / order variant
    tc = TileChoice{ctx->force_a, ctx->force_b, ctx->force_splits, ctx->force_waves == 8 ? 8 : 4};
    if (g.batch <= 1 && tc.splits > 1 && nk / tc.splits < 1) RADNET_FAIL(ctx, RADNET_ERR_ARG, "conv: forced %d K slices but only %d K tiles", tc.splits, nk);
  } else if (it != ctx->tuned->end()) {
    tc = TileChoice{it->second.a, it->second.b, it->second.splits, it->second.waves == 8 ? 8 : 4};
  } else if (const radnet_tuned* nb = ctx->autotune == 2 ? radnet_tuned_neighbour(*ctx->tuned, key) : nullptr) {
    tc = TileChoice{nb->a, nb->b, nb->splits, nb->waves == 8 ? 8 : 4};
    (*ctx->tuned)[key] = *nb;
  } else if (ctx->autotune) {
    PairPause pause(ctx);                       // trial launches are real launches
    // 32-row tiles (round 4): M = 980 / 2 394 / 160 rows fill 256 CUs without K slices (no slab seam, no last-arriver tail) and
    // waste no rows where M is a multiple of 32 but not of 64; tried only where the 64x64 grid is small (they re-read B twice as often)
    const int cand[6][2] = {{128, 128}, {128, 64}, {64, 128}, {64, 64}, {32, 64}, {32, 32}};
    const long long tiles64 = (long long)radnet_cdiv(g.M, 64) * radnet_cdiv(g.N, 64) * (g.batch > 1 ? g.batch : 1);
    const int chunks[] = {1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 16};      // K slices per tile
    std::vector<std::pair<float, TileChoice>> seen;
    // A data gradient measured on behalf of radnet_conv_bwd is tuned WITHIN the shapes its one-launch form takes (64x64 tiles,
    // 4 waves): alone on the chip the 8-wave form often wins by a few per cent, but next to other lanes' launches the paired
    // launch beat "fastest dgrad + wgrad, one after the other" for every classifier layer measured in situ (tools/insitu_tune.py:
    // +2.7 % and +1.3 % on the whole step for the two layers the isolated choice had unpaired)
    const bool for_pair = pause.saved != nullptr && bmode == 1 && !smallc && g.batch <= 1;
    for (int c = 0; c < 6; ++c) {
      if ((cand[c][1] > 64 && g.N <= 64) || (cand[c][0] > 64 && g.M <= 64)) continue;
      if (for_pair && ((cand[c][0] != 64 && cand[c][0] != 32) || cand[c][1] != 64)) continue;
      if (cand[c][0] < 64 && (smallc || tiles64 > 6 * kNumCU)) continue;
      const long long tiles = (long long)radnet_cdiv(g.M, cand[c][0]) * radnet_cdiv(g.N, cand[c][1]);
      for (int s : chunks) {
        if (g.batch > 1 ? (s > 12 || s > g.batch) : (s > 1 && (ctx->ws == nullptr || nk / s < 2))) continue;      // slices shorter than 2 k-tiles (a batch: s = problems per workgroup)
        for (int sign = 1; sign >= -1; sign -= 2) {                             // -s = same slices, XCD-aware unit order
          if (sign < 0 && tiles * s * (g.batch > 1 ? g.batch : 1) < 16) continue;
          for (int waves = 4; waves <= ((for_pair || cand[c][0] < 64) ? 4 : 8); waves += 4) {        // 8 = K tile halved between two wave grids
            TileChoice t{cand[c][0], cand[c][1], sign * s, waves};
            float ms = 0.f;
            int rc = radnet_time_launches(ctx, [&]() { return launch(t); }, 3, &ms);
            if (rc == RADNET_ERR_UNSUPPORTED) continue;
            if (rc != RADNET_OK) return rc;
            seen.push_back({ms, t});
          }
        }
      }
    }
    // The 3-launch screening above is noisy (neighbouring candidates differ by a few per cent, a shared host by more):
    // the finalists are measured again, longer and twice, and the smaller figure of each decides.  Without this, two
    // processes tuned different tables and the same commit benched 3.4 or 3.7 ms per step.
    std::sort(seen.begin(), seen.end(), [](const std::pair<float, TileChoice>& a, const std::pair<float, TileChoice>& b) { return a.first < b.first; });
    float best = 1e30f;
    for (size_t i = 0; i < seen.size() && i < 6; ++i) {
      float ms = 0.f;
      const int rc = radnet_time_launches_twice(ctx, [&]() { return launch(seen[i].second); }, 12, &ms);
      if (rc != RADNET_OK) return rc;
      if (ms < best) { best = ms; tc = seen[i].second; }
    }
    (*ctx->tuned)[key] = radnet_tuned{tc.bm, tc.bn, tc.splits, best, tc.waves};
    if (getenv("RADNET_TUNE_LOG"))
      fprintf(stderr, "[radnet tune] %s M=%d N=%d K=%d C=%d -> tile %dx%d chunks %d waves %d : %.1f us (%.1f TFLOP/s)\n", cls == 1 ? "dgrad" : "fwd",
              g.M, g.N, g.K, g.C, tc.bm, tc.bn, tc.splits, tc.waves, best * 1e3, 2.0 * g.M * g.N * g.K / (best * 1e9));
  } else {
    tc = choose_tiles(g.M, g.N, g.K, ctx->ws != nullptr && g.batch <= 1);
  }
  radnet_timing_arm(ctx);
  int rc = launch(tc);
  if (rc == RADNET_ERR_UNSUPPORTED && ctx->force_a <= 0) {
    // a shared / loaded / adopted choice this launch cannot use: slabs larger than THIS context's workspace, or a K-split /
    // XCD-ordered unit table for a problem that is now launched as a batch (a batch is one plain grid per problem)
    tc.splits = (tc.splits < 0 ? -1 : 1);
    rc = launch(tc);
  }
  if (rc == RADNET_ERR_UNSUPPORTED)
    RADNET_FAIL(ctx, rc, "conv: launch shape tile %dx%d slices %d waves %d cannot run M=%d N=%d K=%d batch=%d (workspace %llu bytes)", tc.bm, tc.bn,
                tc.splits, tc.waves, g.M, g.N, g.K, g.batch, (unsigned long long)ctx->ws_bytes);
  if (rc != RADNET_OK) return rc;
  radnet_timing_end_armed(ctx, cls, 2.0 * g.M * g.N * g.K * (g.batch > 1 ? g.batch : 1));
  return RADNET_OK;
}
}  // namespace

#ifdef RADNET_DIAG_STAMPS
// diagnostic library only (not in include/radnet_hip.h): device buffer of 8 x u64 per workgroup of the next launches
extern "C" int radnet_diag_set_stamps(radnet_ctx* ctx, unsigned long long* dev_buf) {
  if (!ctx) return RADNET_ERR_ARG;
  ctx->diag_stamps = dev_buf;
  return RADNET_OK;
}
#endif

static int fwd_args(radnet_ctx* ctx, const radnet_conv_desc* d, GemmArgs& g) {
  if (!d->x || !d->w || !d->y) RADNET_FAIL(ctx, RADNET_ERR_ARG, "conv_fwd: null tensor");
  g = GemmArgs{};
  g.x = d->x; g.w = d->w; g.y = d->y;
  g.scale = d->scale; g.shift = d->shift; g.addend = d->addend; g.mask = nullptr; g.in_scale = nullptr;
  g.H = d->h; g.W = d->w_; g.C = d->c; g.OH = d->oh; g.OW = d->ow;
  g.KW = d->kw; g.npos = d->kh * d->kw; g.stride = d->stride; g.pad_t = d->pad_t; g.pad_l = d->pad_l;
  g.M = d->nb * d->oh * d->ow; g.N = d->n; g.K = g.npos * d->c;
  g.ldw = d->ldw; g.ldy = d->ldy; g.ld_add = d->ld_add; g.ld_mask = 0;
  g.act = d->act; g.act_cols = d->act_cols; g.flip = 0; g.cin_fwd = 0;
  g.OHOW = d->oh * d->ow;
  // geometry sanity: every output pixel's window must be addressable by the gather's bounds checks
  if ((d->oh - 1) * d->stride - d->pad_t >= d->h || (d->ow - 1) * d->stride - d->pad_l >= d->w_)
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "conv_fwd: output %dx%d inconsistent with input %dx%d", d->oh, d->ow, d->h, d->w_);
  return RADNET_OK;
}

extern "C" int radnet_conv_fwd(radnet_ctx* ctx, const radnet_conv_desc* d) {
  if (!ctx || !d) return RADNET_ERR_ARG;
  GemmArgs g;
  const int rc = fwd_args(ctx, d, g);
  return rc != RADNET_OK ? rc : run_igemm(ctx, g, 0, d->c == 4, 0);
}

// Two independent forward convolutions (same output grid and reduction depth: branch2a and the shortcut conv of a conv_block) as ONE
// launch where that measured faster than the two launches with their own tuned shapes (conv_fwd_pair_kernel; decided once per pair
// of shapes, kind 32 in the tuning table: slices 1 = paired with that tile, 2 = two launches); the two launches otherwise.
extern "C" int radnet_conv_fwd_pair(radnet_ctx* ctx, const radnet_conv_desc* d1, const radnet_conv_desc* d2) {
  if (!ctx || !d1 || !d2) return RADNET_ERR_ARG;
  GemmArgs g1, g2;
  int rc = fwd_args(ctx, d1, g1);
  if (rc == RADNET_OK) rc = fwd_args(ctx, d2, g2);
  if (rc != RADNET_OK) return rc;
  auto separate = [&]() -> int {
    GemmArgs a = g1, b = g2;
    int r = run_igemm(ctx, a, 0, d1->c == 4, 0);
    return r != RADNET_OK ? r : run_igemm(ctx, b, 0, d2->c == 4, 0);
  };
  static const bool disabled = radnet_env_flag("RADNET_NO_FWD_PAIR");
  const bool same_grid = g1.M == g2.M && g1.K == g2.K && g1.C == g2.C && g1.npos == g2.npos && g1.stride == g2.stride;
  if (disabled || !same_grid || d1->c == 4 || (g1.C % BK) != 0 || ctx->force_a > 0 || ctx->pair_capture != nullptr || !ctx->autotune) return separate();
  rc = prepare_igemm(ctx, g1, 0, false);
  if (rc == RADNET_OK) rc = prepare_igemm(ctx, g2, 0, false);
  if (rc != RADNET_OK) return rc;
  g1.units = g2.units = nullptr; g1.partial = g2.partial = nullptr; g1.counters = g2.counters = nullptr;
  g1.batch = g2.batch = 0; g1.xcd_batch = g2.xcd_batch = 0; g1.zper = g2.zper = 0;
  auto paired = [&](int bm, int bn) -> int {
    const unsigned gx1 = (unsigned)radnet_cdiv(g1.M, bm), gx2 = (unsigned)radnet_cdiv(g2.M, bm);
    const unsigned n1 = gx1 * (unsigned)radnet_cdiv(g1.N, bn), n2 = gx2 * (unsigned)radnet_cdiv(g2.N, bn);
    dim3 grid(n1 + n2), block(256);
    if (bm == 64 && bn == 64) RADNET_LAUNCH((conv_fwd_pair_kernel<64, 64>), grid, block, 0, ctx->stream, ctx->arm0, ctx->arm1, g1, g2, n1, gx1, gx2);
    else if (bm == 32 && bn == 64) RADNET_LAUNCH((conv_fwd_pair_kernel<32, 64>), grid, block, 0, ctx->stream, ctx->arm0, ctx->arm1, g1, g2, n1, gx1, gx2);
    else if (bm == 32 && bn == 32) RADNET_LAUNCH((conv_fwd_pair_kernel<32, 32>), grid, block, 0, ctx->stream, ctx->arm0, ctx->arm1, g1, g2, n1, gx1, gx2);
    else return RADNET_ERR_UNSUPPORTED;
    RADNET_CHECK_LAUNCH(ctx, "conv_fwd_pair");
    return RADNET_OK;
  };
  const radnet_shape_key key{32, g1.M, g1.N * 65536 + g2.N, g1.K, g1.C, g1.npos, g1.stride};
  auto it = ctx->tuned->find(key);
  if (it == ctx->tuned->end()) {
    // first use of this pair of shapes: the two launches (which measures each of them, if new) against the pair on every tile it has
    rc = separate();
    if (rc != RADNET_OK) return rc;
    float best = 0.f;
    rc = radnet_time_launches(ctx, separate, 12, &best);
    if (rc != RADNET_OK) return rc;
    radnet_tuned choice{64, 64, 2, best, 4};
    const int tiles[3][2] = {{64, 64}, {32, 64}, {32, 32}};
    for (const auto& t : tiles) {
      float ms = 0.f;
      rc = radnet_time_launches_twice(ctx, [&]() { return paired(t[0], t[1]); }, 12, &ms);
      if (rc != RADNET_OK) return rc;
      if (ms < choice.ms) choice = radnet_tuned{t[0], t[1], 1, ms, 4};
    }
    (*ctx->tuned)[key] = choice;
    if (getenv("RADNET_TUNE_LOG"))
      fprintf(stderr, "[radnet tune] fwd pair M=%d N=%d+%d K=%d -> %s (%.1f us; the two launches %.1f us)\n", g1.M, g1.N, g2.N, g1.K,
              choice.splits == 1 ? (choice.a == 64 ? "one launch, 64x64" : choice.b == 64 ? "one launch, 32x64" : "one launch, 32x32") : "two launches",
              choice.ms * 1e3, best * 1e3);
    it = ctx->tuned->find(key);
  }
  if (it->second.splits != 1) return separate();
  radnet_timing_arm(ctx);
  rc = paired(it->second.a, it->second.b);
  if (rc == RADNET_ERR_UNSUPPORTED) return separate();
  if (rc != RADNET_OK) return rc;
  radnet_timing_end_armed(ctx, 0, 2.0 * g1.M * (double)(g1.N + g2.N) * g1.K);
  return RADNET_OK;
}

// The back of a bottleneck block as one launch (conv_bneck_kernel): db = its 3x3 conv (stride 1, 'same', 64 output channels, ReLU), dc = its
// 1x1 expand on db's output (+ shortcut, ReLU), da = the NEXT block's 1x1 reduce on dc's output (64 columns, ReLU) or null.  db->y is NOT
// written by the fused launch (frozen layers only).  Decided once per shape (kind 33 in the tuning table: slices 1 = fused with tile_a rows
// per workgroup, 2 = the separate launches); anything the fused kernel does not take runs as the separate launches.
extern "C" int radnet_conv_bottleneck(radnet_ctx* ctx, const radnet_conv_desc* db, const radnet_conv_desc* dc, const radnet_conv_desc* da) {
  if (!ctx || !db || !dc) return RADNET_ERR_ARG;
  auto separate = [&]() -> int {
    int r = radnet_conv_fwd(ctx, db);
    if (r == RADNET_OK) r = radnet_conv_fwd(ctx, dc);
    if (r == RADNET_OK && da) r = radnet_conv_fwd(ctx, da);
    return r;
  };
  static const bool disabled = radnet_env_flag("RADNET_NO_BNECK_FUSE");
  const int M = db->nb * db->oh * db->ow;
  auto pointwise = [&](const radnet_conv_desc* d, const radnet_conv_desc* src) {
    return d->kh == 1 && d->kw == 1 && d->stride == 1 && d->pad_t == 0 && d->pad_l == 0 && d->x == src->y && d->c == src->n &&
           d->nb * d->oh * d->ow == M && d->act == 1 && d->y != nullptr && d->w != nullptr && (d->ldw & 3) == 0 && !((uintptr_t)d->w & 15);
  };
  bool ok = !disabled && ctx->autotune && ctx->force_a <= 0 && ctx->pair_capture == nullptr;
  ok = ok && db->kh == 3 && db->kw == 3 && db->stride == 1 && db->pad_t == 1 && db->pad_l == 1 && db->n == 64 && db->act == 1 && !db->addend && db->y &&
       db->c % BK == 0 && db->oh == db->h && db->ow == db->w_;
  ok = ok && pointwise(dc, db) && dc->n % 64 == 0 && dc->ldw >= dc->n && dc->ldy >= dc->n && (!dc->addend || dc->ld_add >= dc->n);
  ok = ok && (!da || (pointwise(da, dc) && da->n == 64 && !da->addend && da->ldw >= 64 && da->ldy >= 64));
  // radnet_conv_desc has no pitch for x: the separate launches read a pitched db->y (dc->y, with da) as a DENSE matrix, the fused kernel
  // hands the tile on through LDS and never sees the pitch.  Only dense intermediates mean the same thing to both.
  ok = ok && db->ldy == db->n && (!da || dc->ldy == dc->n);
  // the tail's byte offsets into dc->y, dc->addend and da->y are 32-bit
  ok = ok && (uint64_t)M * (uint64_t)std::max(std::max(dc->ldy, dc->ld_add), da ? da->ldy : 0) * 4ull < (1ull << 31);
  if (!ok) return separate();
  GemmArgs g;
  int rc = fwd_args(ctx, db, g);
  if (rc == RADNET_OK) rc = prepare_igemm(ctx, g, 0, false);
  if (rc != RADNET_OK) return rc;
  g.y = nullptr; g.y_bytes = 0;
  TailArgs tz{};
  tz.w2 = dc->w; tz.sc2 = dc->scale; tz.sh2 = dc->shift; tz.add = dc->addend; tz.y = dc->y;
  tz.N2 = dc->n; tz.ldw2 = dc->ldw; tz.ldy2 = dc->ldy; tz.ld_add2 = dc->ld_add;
  tz.w2_bytes = (unsigned)(((uint64_t)63 * dc->ldw + dc->n) * 4ull);
  tz.y_bytes = (unsigned)(((uint64_t)(M - 1) * dc->ldy + dc->n) * 4ull);
  tz.add_bytes = dc->addend ? (unsigned)(((uint64_t)(M - 1) * dc->ld_add + dc->n) * 4ull) : 0u;
  if (da) {
    tz.w3 = da->w; tz.sc3 = da->scale; tz.sh3 = da->shift; tz.t = da->y; tz.ldw3 = da->ldw; tz.ldt = da->ldy;
    tz.w3_bytes = (unsigned)(((uint64_t)(dc->n - 1) * da->ldw + 64) * 4ull);
    tz.t_bytes = (unsigned)(((uint64_t)(M - 1) * da->ldy + 64) * 4ull);
  }
  auto fused = [&](int bm) -> int {
    dim3 grid(radnet_cdiv(M, bm));
    if (bm == 64) {
      if (da) RADNET_LAUNCH((conv_bneck_kernel<64, 4, 2>), grid, dim3(256), 0, ctx->stream, ctx->arm0, ctx->arm1, g, tz);
      else RADNET_LAUNCH((conv_bneck_kernel<64, 4, 1>), grid, dim3(256), 0, ctx->stream, ctx->arm0, ctx->arm1, g, tz);
    } else if (bm == 32) {
      if (da) RADNET_LAUNCH((conv_bneck_kernel<32, 2, 2>), grid, dim3(128), 0, ctx->stream, ctx->arm0, ctx->arm1, g, tz);
      else RADNET_LAUNCH((conv_bneck_kernel<32, 2, 1>), grid, dim3(128), 0, ctx->stream, ctx->arm0, ctx->arm1, g, tz);
    } else {
      return RADNET_ERR_UNSUPPORTED;
    }
    RADNET_CHECK_LAUNCH(ctx, "conv_bneck");
    return RADNET_OK;
  };
  const radnet_shape_key key{33, M, dc->n * 65536 + (da ? 64 : 0), g.K, g.C, g.npos, g.stride};
  auto it = ctx->tuned->find(key);
  if (it == ctx->tuned->end()) {
    rc = separate();                     // measures the layers' own shapes, if new
    if (rc != RADNET_OK) return rc;
    float best = 0.f;
    rc = radnet_time_launches(ctx, separate, 12, &best);
    if (rc != RADNET_OK) return rc;
    radnet_tuned choice{64, 64, 2, best, 4};
    for (int bm : {64, 32}) {
      float ms = 0.f;
      rc = radnet_time_launches_twice(ctx, [&]() { return fused(bm); }, 12, &ms);
      if (rc != RADNET_OK) return rc;
      if (getenv("RADNET_TUNE_LOG")) fprintf(stderr, "[radnet tune] bottleneck tail M=%d N2=%d%s: fused %d rows %.1f us\n", M, dc->n, da ? "+64" : "", bm, ms * 1e3);
      if (ms < choice.ms) choice = radnet_tuned{bm, 64, 1, ms, 4};
    }
    (*ctx->tuned)[key] = choice;
    if (getenv("RADNET_TUNE_LOG"))
      fprintf(stderr, "[radnet tune] bottleneck tail M=%d N2=%d%s -> %s (%.1f us; the separate launches %.1f us)\n", M, dc->n, da ? "+64" : "",
              choice.splits == 1 ? (choice.a == 64 ? "one launch, 64 rows" : "one launch, 32 rows") : "separate launches", choice.ms * 1e3, best * 1e3);
    it = ctx->tuned->find(key);
  }
  if (it->second.splits != 1) return separate();
  radnet_timing_arm(ctx);
  rc = fused(it->second.a);
  if (rc == RADNET_ERR_UNSUPPORTED) return separate();
  if (rc != RADNET_OK) return rc;
  radnet_timing_end_armed(ctx, 0, 2.0 * M * (64.0 * g.K + 64.0 * dc->n + (da ? 64.0 * dc->n : 0.0)));
  return RADNET_OK;
}

extern "C" int radnet_gemm_batched(radnet_ctx* ctx, const float* a, const float* b, float* y, int32_t batch, int32_t m, int32_t n, int32_t k) {
  if (!ctx || !a || !b || !y) return RADNET_ERR_ARG;
  if (batch < 1 || batch > 65535) RADNET_FAIL(ctx, RADNET_ERR_ARG, "gemm_batched: batch %d", batch);
  GemmArgs g{};
  g.x = a; g.w = b; g.y = y;
  g.H = 1; g.W = m; g.C = k; g.OH = 1; g.OW = m;           // a 1x1 convolution over m 'pixels' of k channels
  g.KW = 1; g.npos = 1; g.stride = 1; g.pad_t = 0; g.pad_l = 0;
  g.M = m; g.N = n; g.K = k;
  g.ldw = n; g.ldy = n; g.ld_add = 0; g.ld_mask = 0;
  g.OHOW = m;
  g.batch = batch;
  g.x_bstride = (long long)m * k; g.w_bstride = (long long)k * n; g.y_bstride = (long long)m * n;
  return run_igemm(ctx, g, 0, false, 0);
}

extern "C" int radnet_conv_dgrad(radnet_ctx* ctx, const radnet_conv_desc* d) {
  if (!ctx || !d) return RADNET_ERR_ARG;
  if (!d->dy || !d->w || !d->dx) RADNET_FAIL(ctx, RADNET_ERR_ARG, "conv_dgrad: null tensor");
  if (d->stride != 1) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "conv_dgrad: stride %d (only 1)", d->stride);
  if (d->ld_dy != d->n) RADNET_FAIL(ctx, RADNET_ERR_ARG, "conv_dgrad: dy must be dense (ld_dy == n)");
  GemmArgs g{};
  g.x = d->dy; g.w = d->w; g.y = d->dx;
  g.scale = nullptr; g.shift = nullptr; g.addend = d->dx_add; g.mask = d->dx_mask; g.in_scale = d->gscale;
  // gather from dy (nb, oh, ow, n) with the kernel flipped; output pixels = forward input pixels
  g.H = d->oh; g.W = d->ow; g.C = d->n; g.OH = d->h; g.OW = d->w_;
  g.KW = d->kw; g.npos = d->kh * d->kw; g.stride = 1; g.pad_t = d->kh - 1 - d->pad_t; g.pad_l = d->kw - 1 - d->pad_l;
  g.M = d->nb * d->h * d->w_; g.N = d->c; g.K = g.npos * d->n;
  g.ldw = d->ldw; g.ldy = d->ld_dx; g.ld_add = d->ld_dx_add; g.ld_mask = d->ld_dx_mask;
  g.act = 0; g.act_cols = 0; g.flip = 1; g.cin_fwd = d->c;
  g.OHOW = d->h * d->w_;
  if (d->n % 4) RADNET_FAIL(ctx, RADNET_ERR_ARG, "conv_dgrad: n must be a multiple of 4");
  return run_igemm(ctx, g, 1, false, 1);
}
