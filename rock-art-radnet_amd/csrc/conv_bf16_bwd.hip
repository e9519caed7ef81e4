// Convolution backward on the gfx950 bf16 matrix cores (v_mfma_f32_32x32x16_bf16), fp32 accumulation: the data gradient and the
// weight gradient of the layers conv_bf16.hip runs forward (engine precision "bf16-train").
//
// With g[m][n] = dy[m][n] * gscale[n] as ONE fp32 multiply (g = dy without gscale) and bf16() = round to nearest, ties to even:
//   dgrad  dx[p][c] = mask( (sum_{ky,kx,n} bf16(g)[q(p,ky,kx)][n] * bf16(w)[(ky,kx,c)][n]) + dx_add[p][c] )      stride 1
//   wgrad  dw[k][n] (+)= sum_m bf16(im2col(x))[m][k] * bf16(g)[m][n]
// Both are ONE kernel template on conv_bf16_body.h's tile, LDS layout, reduction loop and ordered split (the forward's slabs and
// counters).  They differ in what a row, a column and the reduction are, i.e. in the gather and the epilogue:
//   * dgrad: rows = input pixels p, columns = input channels c, reduction = (tap, n), n innermost.  The A tile is gathered from
//     dy like the forward gathers x (8 consecutive n of one tap as two 16-byte buffer loads, out-of-range offset for taps that
//     fall off the output grid, ragged rows and the reduction's padding), multiplied by gscale and rounded on its way to LDS.
//     The B tile comes from a second bf16 image of the weights in the dgrad layout wd[c][ldkd] (radnet_weights_to_bf16_dgrad):
//     element tap * n8 + j of row c is bf16(w[(tap, c)][j]), n8 = n rounded up to 8, zero for j >= n and past taps * n8 -- 8
//     consecutive n of one (tap, c) are one 16-byte load.  Columns j >= n of dy are zeroed in the gather (rpn_heads: 60 of 64).
//   * wgrad: rows = k = (tap, c), columns = n, reduction = output pixels m -- the dimension that is contiguous in NEITHER operand
//     (x is [pixel][c], dy is [m][n]).  Both tiles are transposed ON THE LDS WRITE: a thread loads 8 consecutive channels of one
//     pixel (two 16-byte loads), rounds them and writes them as eight 2-byte stores into eight LDS rows at column m; the MFMA
//     fragments are then the same 16-byte row reads as everywhere else.  Lanes of a wave hold 32 consecutive m of two channel
//     groups, so the eight stores of a wave spread over 32 banks.  im2col (3x3 padding, stride 2) is the forward's
//     out-of-range-offset gather with the tap fixed per thread and the pixel moving.
#include "conv_bf16_body.h"

namespace {

constexpr int MODE_DGRAD = 0, MODE_WGRAD = 1;

struct BwdArgs {
  const float* x;            // wgrad: forward input NHWC
  const float* dy;           // [M][ld_dy]
  const float* gscale;       // per-output-channel factor on dy or null
  const uint16_t* wd;        // dgrad: bf16 weights in the dgrad layout [C][ldk]
  float* out;                // dgrad: dx [P][ld_out]; wgrad: dw [K][ld_out]
  const float* add;          // dgrad: dx_add or null; wgrad: dw itself when accumulating, else null
  const float* mask;         // dgrad: dx_mask or null
  float* partial;            // split: slabs [tile][slice][BM*BN] (context workspace)
  unsigned* counters;        // split: arrival counter per output tile (context aux block, zero outside a launch)
  int split;
  int H, W, C, OH, OW, KW, stride, pad_t, pad_l;      // the FORWARD convolution's geometry
  int rows, cols, nrt;       // output tile grid extents, number of 32-deep reduction tiles
  int N, n8, red, ldk;       // forward output channels; dgrad: n rounded up to 8, taps * n8, pitch of wd
  int M;                     // forward output pixels nb*oh*ow
  int ld_dy, ld_out, ld_add, ld_mask;
  int HW, OHOW;
  unsigned long long magic_hw, magic_w, magic_ohow, magic_ow, magic_c, magic_kw, magic_n8;
  unsigned x_bytes, dy_bytes, w_bytes, out_bytes, add_bytes, mask_bytes;
};

// ---- dgrad images of the weights -------------------------------------------------------------------------------------------
struct DgradImage {
  const float* w;            // [taps*c][ldw] fp32
  uint16_t* wd;              // [c][ldkd] bf16 bits
  int taps, c, n, ldw, ldkd, n8;
};
struct DgradImages {
  DgradImage l[16];
};

// wd[cc][tap * n8 + j] = bf16(w[(tap, cc)][j]) for tap < taps, j < n; 0 elsewhere.  blockIdx.y = layer of the registry.
__global__ void __launch_bounds__(256) weights_to_bf16_dgrad_kernel(DgradImages L) {
  const DgradImage g = L.l[blockIdx.y];
  const long long total = (long long)g.c * g.ldkd;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int cc = (int)(i / g.ldkd), kd = (int)(i - (long long)cc * g.ldkd);
    const int tap = kd / g.n8, j = kd - tap * g.n8;
    g.wd[i] = (tap < g.taps && j < g.n) ? to_bf16_bits(g.w[((long long)tap * g.c + cc) * g.ldw + j]) : (uint16_t)0;
  }
}

// ---- the kernel ------------------------------------------------------------------------------------------------------------
template <int BM, int BN, int MODE, bool SPLIT>
__global__ void __launch_bounds__(NTHREADS) conv_bf16_bwd_kernel(BwdArgs g) {
  constexpr int TM = BM / 64, TN = BN / 64;          // 32x32 accumulator tiles per wave (2x2 waves)
  constexpr int AL = BM / 64, BL = BN / 64;          // 8-element chunks each thread stages per reduction tile and operand
  __shared__ __attribute__((aligned(16))) uint16_t sa[2][BM * LDSROW];
  __shared__ __attribute__((aligned(16))) uint16_t sb[2][BN * LDSROW];

  const int tid = threadIdx.x;
  const Bf16Lane ln = bf16_lane();
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const __amdgpu_buffer_rsrc_t rx = make_rsrc(g.x, g.x_bytes);
  const __amdgpu_buffer_rsrc_t rdy = make_rsrc(g.dy, g.dy_bytes);
  const __amdgpu_buffer_rsrc_t rw = make_rsrc(g.wd, g.w_bytes);
  const __amdgpu_buffer_rsrc_t rgs = make_rsrc(g.gscale, g.gscale ? (unsigned)g.N * 4u : 0u);
  const bool has_gs = g.gscale != nullptr;

  // dgrad staging: thread tid owns rows (tid >> 2) + 64 j of both tiles and the 8-element chunk (tid & 3) of each reduction tile
  // wgrad staging: thread tid owns reduction element (pixel) tid & 31 of each tile and the rows 8 (tid >> 5) + 64 j .. + 7 of both tiles
  const int ch = tid & 3;
  const int mrow = tid & 31, grp = tid >> 5;
  int pix[AL], qh0[AL], qw0[AL];                     // dgrad: per staged row
  unsigned woff[BL];
  int aky[AL], akx[AL], ac[AL];                      // wgrad: tap and channel of the thread's 8 k rows (ac < 0: past K)
  int bn[BL];                                        // wgrad: first of the thread's 8 columns (< 0: past N)
  float gsb[BL][8];                                  // wgrad: gscale of those columns
  if constexpr (MODE == MODE_DGRAD) {
#pragma unroll
    for (int j = 0; j < AL; ++j) {
      const int p = m0 + (tid >> 2) + 64 * j;
      const int img = div_magic(p, g.magic_hw);
      const int r = p - img * g.HW;
      const int ih = div_magic(r, g.magic_w), iw = r - ih * g.W;
      // a row past the end gets an output row that no tap can reach: every load of it is out of range
      qh0[j] = p < g.rows ? ih + g.pad_t : -(1 << 20);
      qw0[j] = iw + g.pad_l;
      pix[j] = img * g.OH;
    }
#pragma unroll
    for (int j = 0; j < BL; ++j) {
      const int c = n0 + (tid >> 2) + 64 * j;
      woff[j] = c < g.cols ? ((unsigned)c * (unsigned)g.ldk + 8u * ch) * 2u : kOOB;
    }
  } else {
#pragma unroll
    for (int j = 0; j < AL; ++j) {
      const int k0 = m0 + 64 * j + 8 * grp;          // 8 consecutive channels of one tap (C % 8 == 0)
      const int tap = div_magic(k0, g.magic_c);
      aky[j] = div_magic(tap, g.magic_kw);
      akx[j] = tap - aky[j] * g.KW;
      ac[j] = k0 < g.rows ? k0 - tap * g.C : -1;
    }
#pragma unroll
    for (int j = 0; j < BL; ++j) {
      const int n = n0 + 64 * j + 8 * grp;           // N % 8 == 0: a chunk is inside or outside as a whole
      bn[j] = n < g.cols ? n : -1;
      const unsigned off = n < g.cols ? (unsigned)n * 4u : kOOB;
      const f32x4 a = buf_load4(rgs, off), b = buf_load4(rgs, off + 16u);
      const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
      for (int i = 0; i < 8; ++i) gsb[j][i] = has_gs ? v[i] : 1.f;
    }
  }

  f32x4 ra[AL][2];                                   // A chunk in flight (fp32)
  u32x4 rb[BL];                                      // dgrad: B chunk in flight (bf16)
  f32x4 rbf[BL][2];                                  // wgrad: B chunk in flight (fp32)
  f32x4 rg[2];                                       // dgrad: gscale of the A chunk's 8 columns
  int rnn = 0;                                       // dgrad: first column of the A chunk
  auto gload = [&](int t) {
    if constexpr (MODE == MODE_DGRAD) {
      const int k0 = t * BK + 8 * ch;                // 8 consecutive n of one tap (n8 % 8 == 0)
      const int tap = div_magic(k0, g.magic_n8);
      const int nn = k0 - tap * g.n8;
      const int ky = div_magic(tap, g.magic_kw), kx = tap - ky * g.KW;
      const bool kok = k0 < g.red;
      rnn = nn;
      rg[0] = buf_load4(rgs, (unsigned)nn * 4u);
      rg[1] = buf_load4(rgs, (unsigned)nn * 4u + 16u);
#pragma unroll
      for (int j = 0; j < AL; ++j) {
        const int qh = qh0[j] - ky, qw = qw0[j] - kx;
        const bool ok = kok & ((unsigned)qh < (unsigned)g.OH) & ((unsigned)qw < (unsigned)g.OW);
        const unsigned off = ok ? ((unsigned)((pix[j] + qh) * g.OW + qw) * (unsigned)g.ld_dy + (unsigned)nn) * 4u : kOOB;
        ra[j][0] = buf_load4(rdy, off);
        ra[j][1] = buf_load4(rdy, off + 16u);
      }
#pragma unroll
      for (int j = 0; j < BL; ++j) rb[j] = buf_load4u(rw, woff[j] + (unsigned)t * (BK * 2u));
    } else {
      const int m = t * BK + mrow;
      const bool mok = m < g.M;
      const int img = div_magic(m, g.magic_ohow);
      const int r = m - img * g.OHOW;
      const int oh = div_magic(r, g.magic_ow), ow = r - oh * g.OW;
      const int ihb = oh * g.stride - g.pad_t, iwb = ow * g.stride - g.pad_l, pb = img * g.H;
#pragma unroll
      for (int j = 0; j < AL; ++j) {
        const int ih = ihb + aky[j], iw = iwb + akx[j];
        const bool ok = mok & (ac[j] >= 0) & ((unsigned)ih < (unsigned)g.H) & ((unsigned)iw < (unsigned)g.W);
        const unsigned off = ok ? ((unsigned)((pb + ih) * g.W + iw) * (unsigned)g.C + (unsigned)ac[j]) * 4u : kOOB;
        ra[j][0] = buf_load4(rx, off);
        ra[j][1] = buf_load4(rx, off + 16u);
      }
#pragma unroll
      for (int j = 0; j < BL; ++j) {
        const unsigned off = (mok & (bn[j] >= 0)) ? ((unsigned)m * (unsigned)g.ld_dy + (unsigned)bn[j]) * 4u : kOOB;
        rbf[j][0] = buf_load4(rdy, off);
        rbf[j][1] = buf_load4(rdy, off + 16u);
      }
    }
  };
  auto lstore = [&](int buf) {
    if constexpr (MODE == MODE_DGRAD) {
      // g = dy * gscale (one fp32 multiply), columns >= N zeroed, then rounded
      float s[8] = {rg[0].x, rg[0].y, rg[0].z, rg[0].w, rg[1].x, rg[1].y, rg[1].z, rg[1].w};
      bool live[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        live[i] = rnn + i < g.N;
        s[i] = has_gs ? s[i] : 1.f;
      }
#pragma unroll
      for (int j = 0; j < AL; ++j) {
        const float v[8] = {ra[j][0].x, ra[j][0].y, ra[j][0].z, ra[j][0].w, ra[j][1].x, ra[j][1].y, ra[j][1].z, ra[j][1].w};
        float q[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) q[i] = live[i] ? v[i] * s[i] : 0.f;
        const f32x4 lo = {q[0], q[1], q[2], q[3]}, hi4 = {q[4], q[5], q[6], q[7]};
        *reinterpret_cast<u32x4*>(&sa[buf][((tid >> 2) + 64 * j) * LDSROW + 8 * ch]) = pack8_bf16(lo, hi4);
      }
#pragma unroll
      for (int j = 0; j < BL; ++j) *reinterpret_cast<u32x4*>(&sb[buf][((tid >> 2) + 64 * j) * LDSROW + 8 * ch]) = rb[j];
    } else {
      // transposed on the write: the thread's 8 channels of pixel `mrow` go to 8 LDS rows, column mrow
#pragma unroll
      for (int j = 0; j < AL; ++j) {
        const float v[8] = {ra[j][0].x, ra[j][0].y, ra[j][0].z, ra[j][0].w, ra[j][1].x, ra[j][1].y, ra[j][1].z, ra[j][1].w};
#pragma unroll
        for (int i = 0; i < 8; ++i) sa[buf][(64 * j + 8 * grp + i) * LDSROW + mrow] = to_bf16_bits(v[i]);
      }
#pragma unroll
      for (int j = 0; j < BL; ++j) {
        const float v[8] = {rbf[j][0].x, rbf[j][0].y, rbf[j][0].z, rbf[j][0].w, rbf[j][1].x, rbf[j][1].y, rbf[j][1].z, rbf[j][1].w};
#pragma unroll
        for (int i = 0; i < 8; ++i) sb[buf][(64 * j + 8 * grp + i) * LDSROW + mrow] = to_bf16_bits(v[i] * gsb[j][i]);
      }
    }
  };

  f32x16 acc[TM][TN];
  const int2 tr = SPLIT ? bf16_slice_tiles(g.nrt, g.split, blockIdx.z) : make_int2(0, g.nrt);
  bf16_gemm_tiles<BM, BN>(sa, sb, tr.x, tr.y, gload, lstore, ln, acc);
  if constexpr (SPLIT) {
    if (!bf16_ordered_split<BM, BN>(g.partial, g.counters, g.split, acc)) return;
  }

  // epilogue: D[row][col], col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  //   dgrad: dx = mask > 0 ? acc + dx_add : 0;   wgrad: dw = acc (+ dw)
  const __amdgpu_buffer_rsrc_t ro = make_rsrc(g.out, g.out_bytes);
  const __amdgpu_buffer_rsrc_t radd = make_rsrc(g.add, g.add ? g.add_bytes : 0u);       // null -> every load returns 0
  const __amdgpu_buffer_rsrc_t rmask = make_rsrc(g.mask, g.mask ? g.mask_bytes : 0u);
  const bool has_mask = (MODE == MODE_DGRAD) && g.mask != nullptr;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int n = n0 + ln.wn * (BN / 2) + j * 32 + ln.l31;
    const bool nv = n < g.cols;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int mb = m0 + ln.wm * (BM / 2) + i * 32 + 4 * ln.hi;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = mb + (r & 3) + 8 * (r >> 2);
        const bool ok = nv & (m < g.rows);
        const float ad = buf_load1(radd, ok ? ((unsigned)m * (unsigned)g.ld_add + (unsigned)n) * 4u : kOOB);
        float v = acc[i][j][r] + ad;
        if constexpr (MODE == MODE_DGRAD) {
          const float mk = buf_load1(rmask, ok ? ((unsigned)m * (unsigned)g.ld_mask + (unsigned)n) * 4u : kOOB);
          v = (!has_mask || mk > 0.f) ? v : 0.f;
        }
        buf_store1(ro, ok ? ((unsigned)m * (unsigned)g.ld_out + (unsigned)n) * 4u : kOOB, v);
      }
    }
  }
}

template <int MODE>
struct BwdLaunch {
  static constexpr const char* what = MODE == MODE_DGRAD ? "conv_dgrad_bf16" : "conv_wgrad_bf16";
  static constexpr const char* launch_name = what;
  static constexpr bool halve_split = true;
  static constexpr int timing_slot = MODE == MODE_DGRAD ? 1 : 2;
  template <int BM, int BN, bool SPLIT>
  static auto kernel() { return conv_bf16_bwd_kernel<BM, BN, MODE, SPLIT>; }
};

int cast_images(radnet_ctx* ctx, const DgradImages& L, int n_layers) {
  hipLaunchKernelGGL(weights_to_bf16_dgrad_kernel, dim3(512, (unsigned)n_layers), dim3(256), 0, ctx->stream, L);
  RADNET_CHECK_LAUNCH(ctx, "weights_to_bf16_dgrad_kernel");
  return RADNET_OK;
}

// 0, or the complaint about one image
const char* image_problem(const float* w, int taps, int c, int n, int ldw, const uint16_t* wd, int ldkd) {
  if (!w || !wd) return "null tensor";
  if (taps <= 0 || c <= 0 || n <= 0 || ldw < n) return "bad geometry";
  const long long kd = (long long)taps * ((n + 7) / 8 * 8), kdp = (kd + BK - 1) / BK * BK;
  if (ldkd < kdp || ldkd % 8 != 0 || ((uintptr_t)wd & 15)) return "ldkd must be >= taps * roundup(n, 8) rounded up to 32, a multiple of 8, wd 16-byte aligned";
  if ((long long)c * ldkd * 2 >= (1ll << 31)) return "image too large";
  return nullptr;
}

}  // namespace

extern "C" int radnet_weights_to_bf16_dgrad(radnet_ctx* ctx, const float* w, int32_t taps, int32_t c, int32_t n, int32_t ldw, uint16_t* wd,
                                            int32_t ldkd) {
  if (!ctx) return RADNET_ERR_ARG;
  if (const char* why = image_problem(w, taps, c, n, ldw, wd, ldkd)) RADNET_FAIL(ctx, RADNET_ERR_ARG, "weights_to_bf16_dgrad: %s (taps=%d c=%d n=%d ldw=%d ldkd=%d)", why, taps, c, n, ldw, ldkd);
  DgradImages L{};
  L.l[0] = DgradImage{w, wd, taps, c, n, ldw, ldkd, (n + 7) / 8 * 8};
  return cast_images(ctx, L, 1);
}

extern "C" int radnet_weights_to_bf16_dgrad_arena(radnet_ctx* ctx, const float* p, int64_t n_arena, const radnet_bf16_dgrad_image* layers,
                                                  int32_t n_layers) {
  if (!ctx) return RADNET_ERR_ARG;
  if (!p || n_arena <= 0 || n_layers < 0 || (n_layers > 0 && !layers)) RADNET_FAIL(ctx, RADNET_ERR_ARG, "weights_to_bf16_dgrad_arena: null arena or registry");
  if (n_layers > 16) RADNET_FAIL(ctx, RADNET_ERR_ARG, "weights_to_bf16_dgrad_arena: %d layers (at most 16)", n_layers);
  if (n_layers == 0) return RADNET_OK;
  DgradImages L{};
  for (int k = 0; k < n_layers; ++k) {
    const radnet_bf16_dgrad_image& s = layers[k];
    if (s.off < 0 || s.taps <= 0 || s.c <= 0 || s.ldw <= 0 || s.off + (int64_t)s.taps * s.c * s.ldw > n_arena)
      RADNET_FAIL(ctx, RADNET_ERR_ARG, "weights_to_bf16_dgrad_arena: layer %d lies outside the arena", k);
    if (const char* why = image_problem(p + s.off, s.taps, s.c, s.n, s.ldw, s.wd, s.ldkd)) RADNET_FAIL(ctx, RADNET_ERR_ARG, "weights_to_bf16_dgrad_arena: layer %d: %s", k, why);
    L.l[k] = DgradImage{p + s.off, s.wd, s.taps, s.c, s.n, s.ldw, s.ldkd, (s.n + 7) / 8 * 8};
  }
  return cast_images(ctx, L, n_layers);
}

extern "C" int32_t radnet_dgrad_bf16_pick_split(int64_t p, int32_t c, int32_t kd) { return radnet_conv_bf16_pick_split(p, c, kd); }
// rows of the weight gradient are K, its reduction the M output pixels
extern "C" int32_t radnet_wgrad_bf16_pick_split(int64_t m, int32_t n, int32_t k) {
  if (m <= 0 || n <= 0 || k <= 0) return 1;
  return radnet_conv_bf16_pick_split(k, n, (int32_t)std::min<int64_t>(m, 1 << 30));
}

extern "C" int radnet_conv_dgrad_bf16(radnet_ctx* ctx, const radnet_conv_desc* d, const uint16_t* wd, int32_t ldkd) {
  return radnet_conv_dgrad_bf16_split(ctx, d, wd, ldkd, 1);
}

extern "C" int radnet_conv_dgrad_bf16_split(radnet_ctx* ctx, const radnet_conv_desc* d, const uint16_t* wd, int32_t ldkd, int32_t ksplit) {
  if (!ctx || !d) return RADNET_ERR_ARG;
  if (!d->dy || !wd || !d->dx) RADNET_FAIL(ctx, RADNET_ERR_ARG, "conv_dgrad_bf16: null tensor");
  if (d->stride != 1) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "conv_dgrad_bf16: stride %d (stride 1 only, as radnet_conv_dgrad)", d->stride);
  if (int rc = bf16_check_geometry(ctx, d, "conv_dgrad_bf16")) return rc;
  const int n8 = (d->n + 7) / 8 * 8;
  if (d->n % 4 != 0 || d->ld_dy % 4 != 0 || d->ld_dy < n8)
    RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "conv_dgrad_bf16: n=%d ld_dy=%d (n and ld_dy multiples of 4, ld_dy >= n rounded up to 8)", d->n, d->ld_dy);
  if (((uintptr_t)d->dy & 15) || ((uintptr_t)wd & 15) || (d->gscale && ((uintptr_t)d->gscale & 15)))
    RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "conv_dgrad_bf16: dy, gscale and wd must be 16-byte aligned");
  const long long kd = (long long)d->kh * d->kw * n8, kdp = (kd + BK - 1) / BK * BK;
  if (ldkd < kdp || ldkd % 8 != 0) RADNET_FAIL(ctx, RADNET_ERR_ARG, "conv_dgrad_bf16: ldkd=%d (needs >= %lld, a multiple of 8)", ldkd, kdp);
  if (d->ld_dx < d->c || (d->dx_add && d->ld_dx_add < d->c) || (d->dx_mask && d->ld_dx_mask < d->c))
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "conv_dgrad_bf16: ld_dx=%d ld_dx_add=%d ld_dx_mask=%d for %d channels", d->ld_dx, d->ld_dx_add, d->ld_dx_mask, d->c);
  const long long P = (long long)d->nb * d->h * d->w_, M = (long long)d->nb * d->oh * d->ow;
  const long long dy_bytes = M * d->ld_dy * 4, w_bytes = (long long)d->c * ldkd * 2, out_bytes = ((P - 1) * d->ld_dx + d->c) * 4;
  const long long add_bytes = d->dx_add ? ((P - 1) * d->ld_dx_add + d->c) * 4 : 0, mask_bytes = d->dx_mask ? ((P - 1) * d->ld_dx_mask + d->c) * 4 : 0;
  if (bf16_too_large({dy_bytes, w_bytes, out_bytes, add_bytes, mask_bytes}, {P, M, kdp}))
    RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "conv_dgrad_bf16: problem too large (P=%lld kd=%lld)", P, kd);
  BwdArgs g{};
  g.dy = d->dy; g.gscale = d->gscale; g.wd = wd; g.out = d->dx; g.add = d->dx_add; g.mask = d->dx_mask;
  g.H = d->h; g.W = d->w_; g.C = d->c; g.OH = d->oh; g.OW = d->ow; g.KW = d->kw; g.stride = 1; g.pad_t = d->pad_t; g.pad_l = d->pad_l;
  g.rows = (int)P; g.cols = d->c; g.nrt = (int)(kdp / BK); g.N = d->n; g.n8 = n8; g.red = (int)kd; g.ldk = ldkd; g.M = (int)M;
  g.ld_dy = d->ld_dy; g.ld_out = d->ld_dx; g.ld_add = d->ld_dx_add; g.ld_mask = d->ld_dx_mask;
  g.HW = d->h * d->w_; g.OHOW = d->oh * d->ow;
  g.magic_hw = radnet_div_magic((uint32_t)g.HW); g.magic_w = radnet_div_magic((uint32_t)d->w_);
  g.magic_kw = radnet_div_magic((uint32_t)d->kw); g.magic_n8 = radnet_div_magic((uint32_t)n8);
  g.dy_bytes = (unsigned)dy_bytes; g.w_bytes = (unsigned)w_bytes; g.out_bytes = (unsigned)out_bytes; g.add_bytes = (unsigned)add_bytes;
  g.mask_bytes = (unsigned)mask_bytes;
  if (ksplit > 64 || ksplit > g.nrt) RADNET_FAIL(ctx, RADNET_ERR_ARG, "conv_dgrad_bf16: split %d (at most 64 and the %d reduction tiles)", ksplit, g.nrt);
  g.split = ksplit > 1 ? ksplit : 1;
  return bf16_launch_by_shape<BwdLaunch<MODE_DGRAD>>(ctx, g, g.rows, g.cols, 2.0 * P * (double)d->c * d->kh * d->kw * d->n);
}

extern "C" int radnet_conv_wgrad_bf16(radnet_ctx* ctx, const radnet_conv_desc* d, int32_t msplit) {
  if (!ctx || !d) return RADNET_ERR_ARG;
  if (!d->x || !d->dy || !d->dw) RADNET_FAIL(ctx, RADNET_ERR_ARG, "conv_wgrad_bf16: null tensor");
  if (int rc = bf16_check_geometry(ctx, d, "conv_wgrad_bf16")) return rc;
  if (d->c % 8 != 0 || d->n % 8 != 0 || d->ld_dy % 4 != 0)
    RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "conv_wgrad_bf16: c=%d n=%d ld_dy=%d (channel counts multiples of 8, ld_dy of 4)", d->c, d->n, d->ld_dy);
  if (((uintptr_t)d->x & 15) || ((uintptr_t)d->dy & 15) || (d->gscale && ((uintptr_t)d->gscale & 15)))
    RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "conv_wgrad_bf16: x, dy and gscale must be 16-byte aligned");
  if (d->ldw < d->n || d->ld_dy < d->n || d->dw_accumulate < 0 || d->dw_accumulate > 2)
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "conv_wgrad_bf16: ldw=%d ld_dy=%d dw_accumulate=%d for %d columns", d->ldw, d->ld_dy, d->dw_accumulate, d->n);
  const long long M = (long long)d->nb * d->oh * d->ow, K = (long long)d->kh * d->kw * d->c;
  const long long x_bytes = (long long)d->nb * d->h * d->w_ * d->c * 4, dy_bytes = ((M - 1) * d->ld_dy + d->n) * 4, out_bytes = ((K - 1) * d->ldw + d->n) * 4;
  if (bf16_too_large({x_bytes, dy_bytes, out_bytes}, {M, K}))
    RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "conv_wgrad_bf16: problem too large (M=%lld K=%lld)", M, K);
  BwdArgs g{};
  g.x = d->x; g.dy = d->dy; g.gscale = d->gscale; g.out = d->dw;
  g.add = d->dw_accumulate != 0 ? d->dw : nullptr;      // 1: add to what is there; 2: the caller zeroed it -- the same add
  g.H = d->h; g.W = d->w_; g.C = d->c; g.OH = d->oh; g.OW = d->ow; g.KW = d->kw; g.stride = d->stride; g.pad_t = d->pad_t; g.pad_l = d->pad_l;
  g.rows = (int)K; g.cols = d->n; g.nrt = radnet_cdiv(M, BK); g.N = d->n; g.M = (int)M;
  g.ld_dy = d->ld_dy; g.ld_out = d->ldw; g.ld_add = d->ldw;
  g.HW = d->h * d->w_; g.OHOW = d->oh * d->ow;
  g.magic_ohow = radnet_div_magic((uint32_t)g.OHOW); g.magic_ow = radnet_div_magic((uint32_t)d->ow);
  g.magic_c = radnet_div_magic((uint32_t)d->c); g.magic_kw = radnet_div_magic((uint32_t)d->kw);
  g.x_bytes = (unsigned)x_bytes; g.dy_bytes = (unsigned)dy_bytes; g.out_bytes = (unsigned)out_bytes; g.add_bytes = (unsigned)out_bytes;
  if (msplit > 64 || msplit > g.nrt) RADNET_FAIL(ctx, RADNET_ERR_ARG, "conv_wgrad_bf16: split %d (at most 64 and the %d reduction tiles)", msplit, g.nrt);
  g.split = msplit > 1 ? msplit : 1;
  int rc = bf16_launch_by_shape<BwdLaunch<MODE_WGRAD>>(ctx, g, g.rows, g.cols, 2.0 * M * (double)d->n * K);
  // bias gradient: the exact fp32 column sum of the UNROUNDED dy * gscale, added in index order
  if (rc == RADNET_OK && d->db) rc = radnet_colsum(ctx, d->dy, (int32_t)M, d->n, d->ld_dy, d->gscale, d->db, d->dw_accumulate != 0 ? 1 : 0);
  return rc;
}
