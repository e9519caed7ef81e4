// Inference convolution as implicit GEMM on the gfx950 bf16 matrix cores (v_mfma_f32_32x32x16_bf16), fp32 accumulation.
//
// The predict-only twin of the fp32 forward kernel (conv_igemm_body.h, conv_mfma.hip) (keras Conv2D + FixedBatchNormalization + Add + Activation,
// base_models/resnet50.py:41-147,183-186; rpn.py:41-64) for frozen weights: bf16 MFMA runs at 16x the fp32 MFMA rate on
// gfx950 (no TF32 there), and at inference nothing accumulates the rounding over steps.  Tile, waves, LDS layout, the reduction loop
// and the ordered split are conv_bf16_body.h's; rows = output pixels m, columns = output channels n, reduction = k = (tap, c).
//
//   * Weights are cast ONCE per weight load (radnet_weights_to_bf16) into bf16 [N][Kp], Kp = K rounded up to the 32-deep K
//     tile, zero padded: a lane of the 32x32x16 MFMA holds B[k = 8h + j][col r], j = 0..7, so it reads its 8 k values of
//     one output channel as one 16-byte load, and the K padding needs no bounds test.
//   * Activations stay NHWC fp32 in HBM (RoI crop-resize, the head tail, proposals and NMS are untouched).  Each
//     workgroup gathers its A tile (BM output pixels x 32 k) straight from the activation tensor with 32-byte buffer loads
//     (8 consecutive channels of one tap: C % 8 == 0), rounds it to bf16 (round to nearest, ties to even) and writes it to
//     LDS.
//   * Fused epilogue as in conv_igemm_body.h: per-column scale / shift, residual addend, ReLU or sigmoid on [0, act_cols).
//   * K split (bf16-mixed training: small M, deep K -- radnet_conv_bf16_pick_split); ksplit <= 1 is the single-pass launch.
#include "conv_bf16_body.h"

namespace {

struct Bf16Args {
  const float* x;            // NHWC fp32 input
  const uint16_t* wt;        // bf16 weights [N][ldk]
  float* y;                  // output [M][ldy]
  const float* scale;        // per-column scale or null
  const float* shift;        // per-column shift or null
  const float* addend;       // residual [M][ld_add] or null
  float* partial;            // split: slabs [tile][slice][BM*BN] (context workspace)
  unsigned* counters;        // split: arrival counter per output tile (context aux block, zero outside a launch)
  int split;
  int H, W, C, OW, KW, stride, pad_t, pad_l;
  int M, N, K, nkt, ldk, ldy, ld_add, act, act_cols;
  int OHOW;
  unsigned long long magic_ohow, magic_ow, magic_c, magic_kw;
  unsigned x_bytes, w_bytes, y_bytes, add_bytes;
};

// wt[n][k] = bf16(w[k][n]) for k < K, 0 for K <= k < ldk
__global__ void __launch_bounds__(256) weights_to_bf16_kernel(const float* __restrict__ w, int K, int N, int ldw, uint16_t* __restrict__ wt,
                                                              int ldk) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)N * ldk) return;
  const int n = (int)(i / ldk), k = (int)(i - (long long)n * ldk);
  wt[i] = k < K ? to_bf16_bits(w[(long long)k * ldw + n]) : (uint16_t)0;
}

template <int BM, int BN, bool SPLIT>
__global__ void __launch_bounds__(NTHREADS) conv_bf16_fwd_kernel(Bf16Args g) {
  constexpr int TM = BM / 64, TN = BN / 64;          // 32x32 accumulator tiles per wave (2x2 waves)
  constexpr int AL = BM / 64, BL = BN / 64;          // 8-k chunks each thread stages per K tile (4 chunks per row)
  __shared__ __attribute__((aligned(16))) uint16_t sa[2][BM * LDSROW];
  __shared__ __attribute__((aligned(16))) uint16_t sb[2][BN * LDSROW];

  const int tid = threadIdx.x;
  const Bf16Lane ln = bf16_lane();
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const __amdgpu_buffer_rsrc_t rx = make_rsrc(g.x, g.x_bytes);
  const __amdgpu_buffer_rsrc_t rw = make_rsrc(g.wt, g.w_bytes);

  // staging: thread tid owns rows (tid >> 2) + 64 j of both operand tiles and the 8-k chunk (tid & 3) of each K tile
  const int ch = tid & 3;
  int pix[AL], ih0[AL], iw0[AL];
#pragma unroll
  for (int j = 0; j < AL; ++j) {
    const int m = m0 + (tid >> 2) + 64 * j;
    const int img = div_magic(m, g.magic_ohow);
    const int r = m - img * g.OHOW;
    const int oh = div_magic(r, g.magic_ow), ow = r - oh * g.OW;
    // a row past M gets an input row that no tap can reach: every load of it is out of range
    ih0[j] = m < g.M ? oh * g.stride - g.pad_t : -(1 << 20);
    iw0[j] = ow * g.stride - g.pad_l;
    pix[j] = img * g.H;
  }
  unsigned woff[BL];
#pragma unroll
  for (int j = 0; j < BL; ++j) {
    const int n = n0 + (tid >> 2) + 64 * j;
    woff[j] = n < g.N ? ((unsigned)n * (unsigned)g.ldk + 8u * ch) * 2u : kOOB;
  }

  f32x4 ra[AL][2];
  u32x4 rb[BL];
  auto gload = [&](int kt) {
    const int k0 = kt * BK + 8 * ch;                 // 8 consecutive channels of one tap (C % 8 == 0)
    const int tap = div_magic(k0, g.magic_c);
    const int c = k0 - tap * g.C;
    const int ky = div_magic(tap, g.magic_kw), kx = tap - ky * g.KW;
    const bool kok = k0 < g.K;
#pragma unroll
    for (int j = 0; j < AL; ++j) {
      const int ih = ih0[j] + ky, iw = iw0[j] + kx;
      const bool ok = kok & ((unsigned)ih < (unsigned)g.H) & ((unsigned)iw < (unsigned)g.W);
      const unsigned off = ok ? ((unsigned)((pix[j] + ih) * g.W + iw) * (unsigned)g.C + (unsigned)c) * 4u : kOOB;
      ra[j][0] = buf_load4(rx, off);
      ra[j][1] = buf_load4(rx, off + 16u);
    }
#pragma unroll
    for (int j = 0; j < BL; ++j) rb[j] = buf_load4u(rw, woff[j] + (unsigned)kt * (BK * 2u));
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int j = 0; j < AL; ++j)
      *reinterpret_cast<u32x4*>(&sa[buf][((tid >> 2) + 64 * j) * LDSROW + 8 * ch]) = pack8_bf16(ra[j][0], ra[j][1]);
#pragma unroll
    for (int j = 0; j < BL; ++j) *reinterpret_cast<u32x4*>(&sb[buf][((tid >> 2) + 64 * j) * LDSROW + 8 * ch]) = rb[j];
  };

  f32x16 acc[TM][TN];
  const int2 kt = SPLIT ? bf16_slice_tiles(g.nkt, g.split, blockIdx.z) : make_int2(0, g.nkt);
  bf16_gemm_tiles<BM, BN>(sa, sb, kt.x, kt.y, gload, lstore, ln, acc);
  if constexpr (SPLIT) {
    if (!bf16_ordered_split<BM, BN>(g.partial, g.counters, g.split, acc)) return;
  }

  // epilogue: D[row][col], col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  const __amdgpu_buffer_rsrc_t ry = make_rsrc(g.y, g.y_bytes);
  const __amdgpu_buffer_rsrc_t radd = make_rsrc(g.addend, g.addend ? g.add_bytes : 0u);     // null -> every load returns 0
  const __amdgpu_buffer_rsrc_t rsc = make_rsrc(g.scale, g.scale ? (unsigned)g.N * 4u : 0u);
  const __amdgpu_buffer_rsrc_t rsh = make_rsrc(g.shift, g.shift ? (unsigned)g.N * 4u : 0u);
  const bool has_scale = g.scale != nullptr, relu = g.act == 1, sig = g.act == 2;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int n = n0 + ln.wn * (BN / 2) + j * 32 + ln.l31;
    const bool nv = n < g.N;
    const unsigned noff = nv ? (unsigned)n * 4u : kOOB;
    const float sc = has_scale ? buf_load1(rsc, noff) : 1.f, sh = buf_load1(rsh, noff);
    const bool sig_col = sig & (n < g.act_cols);
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int mb = m0 + ln.wm * (BM / 2) + i * 32 + 4 * ln.hi;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = mb + (r & 3) + 8 * (r >> 2);
        const bool ok = nv & (m < g.M);
        const float ad = buf_load1(radd, ok ? ((unsigned)m * (unsigned)g.ld_add + (unsigned)n) * 4u : kOOB);
        float v = acc[i][j][r] * sc + sh + ad;
        const float sg = 1.f / (1.f + __expf(-v));
        v = sig_col ? sg : (relu ? fmaxf(v, 0.f) : v);
        buf_store1(ry, ok ? ((unsigned)m * (unsigned)g.ldy + (unsigned)n) * 4u : kOOB, v);
      }
    }
  }
}

struct FwdLaunch {
  static constexpr const char* what = "conv_fwd_bf16";
  static constexpr const char* launch_name = "conv_bf16_fwd_kernel";
  static constexpr bool halve_split = false;
  static constexpr int timing_slot = 0;
  template <int BM, int BN, bool SPLIT>
  static auto kernel() { return conv_bf16_fwd_kernel<BM, BN, SPLIT>; }
};

}  // namespace

extern "C" int radnet_weights_to_bf16(radnet_ctx* ctx, const float* w, int32_t k, int32_t n, int32_t ldw, uint16_t* wt, int32_t ldk) {
  if (!ctx) return RADNET_ERR_ARG;
  if (!w || !wt) RADNET_FAIL(ctx, RADNET_ERR_ARG, "weights_to_bf16: null tensor");
  if (k <= 0 || n <= 0 || ldw < n || ldk < k) RADNET_FAIL(ctx, RADNET_ERR_ARG, "weights_to_bf16: k=%d n=%d ldw=%d ldk=%d", k, n, ldw, ldk);
  const long long total = (long long)n * ldk;
  hipLaunchKernelGGL(weights_to_bf16_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, w, k, n, ldw, wt, ldk);
  RADNET_CHECK_LAUNCH(ctx, "weights_to_bf16_kernel");
  return RADNET_OK;
}

// output tile of the launch: a fixed rule of (rows, cols) -- the largest tile that still gives every CU a workgroup (0: 128x128, 1: 128x64,
// 2: 64x64).  The ONE copy of the rule: every launch (conv_bf16_body.h: bf16_launch_by_shape) and radnet_conv_bf16_tile_shape use it.
int radnet_bf16_tile_shape(long long rows, int cols, long long* tiles) {
  const long long t128 = (long long)radnet_cdiv(rows, 128) * radnet_cdiv(cols, 128), t128x64 = (long long)radnet_cdiv(rows, 128) * radnet_cdiv(cols, 64);
  if (cols > 64 && t128 >= 256) { *tiles = t128; return 0; }
  if (t128x64 >= 256) { *tiles = t128x64; return 1; }
  *tiles = (long long)radnet_cdiv(rows, 64) * radnet_cdiv(cols, 64);
  return 2;
}

extern "C" int64_t radnet_conv_bf16_tile_shape(int64_t rows, int32_t cols, int32_t* bm, int32_t* bn) {
  if (rows <= 0 || cols <= 0 || !bm || !bn) return 0;
  long long tiles = 0;
  const int shape = radnet_bf16_tile_shape(rows, cols, &tiles);
  *bm = shape == 2 ? 64 : 128;
  *bn = shape == 0 ? 128 : 64;
  return tiles;
}

extern "C" int32_t radnet_conv_bf16_pick_split(int64_t M, int32_t N, int32_t K) {
  if (M <= 0 || N <= 0 || K <= 0) return 1;
  long long tiles = 0;
  radnet_bf16_tile_shape(M, N, &tiles);
  const long long nkt = (K + BK - 1) / BK;
  int s = 1;
  while (tiles * s < 256 && nkt >= 16ll * s && s < 16) s *= 2;      // double while short of 256 workgroups and slices keep >= 8 K tiles
  return s;
}

extern "C" int radnet_conv_fwd_bf16(radnet_ctx* ctx, const radnet_conv_desc* d, const uint16_t* wt, int32_t ldk) {
  return radnet_conv_fwd_bf16_split(ctx, d, wt, ldk, 1);
}

extern "C" int radnet_conv_fwd_bf16_split(radnet_ctx* ctx, const radnet_conv_desc* d, const uint16_t* wt, int32_t ldk, int32_t ksplit) {
  if (!ctx || !d) return RADNET_ERR_ARG;
  if (!d->x || !wt || !d->y) RADNET_FAIL(ctx, RADNET_ERR_ARG, "conv_fwd_bf16: null tensor");
  if (d->c % 8 != 0) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "conv_fwd_bf16: %d input channels (needs a multiple of 8)", d->c);
  if (int rc = bf16_check_geometry(ctx, d, "conv_fwd_bf16")) return rc;
  const long long K = (long long)d->kh * d->kw * d->c, Kp = (K + BK - 1) / BK * BK;
  if (ldk < Kp || ldk % 8 != 0 || ((uintptr_t)wt & 15) || ((uintptr_t)d->x & 15))
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "conv_fwd_bf16: ldk=%d (needs >= %lld, a multiple of 8, 16-byte aligned operands)", ldk, Kp);
  const long long M = (long long)d->nb * d->oh * d->ow;
  if (d->ldy < d->n || (d->addend && d->ld_add < d->n) || (d->act == 2 && d->act_cols < 0))
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "conv_fwd_bf16: ldy=%d ld_add=%d for %d columns", d->ldy, d->ld_add, d->n);
  const long long x_bytes = (long long)d->nb * d->h * d->w_ * d->c * 4, w_bytes = (long long)d->n * ldk * 2;
  const long long y_bytes = ((M - 1) * d->ldy + d->n) * 4, add_bytes = d->addend ? ((M - 1) * d->ld_add + d->n) * 4 : 0;
  if (bf16_too_large({x_bytes, w_bytes, y_bytes, add_bytes}, {M, K}))
    RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "conv_fwd_bf16: problem too large (M=%lld K=%lld)", M, K);
  Bf16Args g{};
  g.x = d->x; g.wt = wt; g.y = d->y; g.scale = d->scale; g.shift = d->shift; g.addend = d->addend;
  g.H = d->h; g.W = d->w_; g.C = d->c; g.OW = d->ow; g.KW = d->kw; g.stride = d->stride; g.pad_t = d->pad_t; g.pad_l = d->pad_l;
  g.M = (int)M; g.N = d->n; g.K = (int)K; g.nkt = (int)(Kp / BK); g.ldk = ldk; g.ldy = d->ldy; g.ld_add = d->ld_add;
  g.act = d->act; g.act_cols = d->act_cols; g.OHOW = d->oh * d->ow;
  g.magic_ohow = radnet_div_magic((uint32_t)g.OHOW); g.magic_ow = radnet_div_magic((uint32_t)d->ow);
  g.magic_c = radnet_div_magic((uint32_t)d->c); g.magic_kw = radnet_div_magic((uint32_t)d->kw);
  g.x_bytes = (unsigned)x_bytes; g.w_bytes = (unsigned)w_bytes; g.y_bytes = (unsigned)y_bytes; g.add_bytes = (unsigned)add_bytes;
  if (ksplit > 64 || ksplit > g.nkt)
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "conv_fwd_bf16: K split %d (at most 64 and the %d K tiles)", ksplit, g.nkt);
  g.split = ksplit > 1 ? ksplit : 1;
  return bf16_launch_by_shape<FwdLaunch>(ctx, g, M, d->n, 2.0 * g.M * (double)g.N * g.K);
}
