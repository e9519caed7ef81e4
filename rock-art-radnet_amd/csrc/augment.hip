// Train-time tile augmentation on the device (augmentation.py:17-31, 85-156, 303-478 of the reference; the host form is
// faster_rcnn/augmentation.py): the index gather behind the tile crop / flips / 90-degree rotations / strap slice, the strap
// extent, the 256-bin histogram behind the brightness mean and poisson's `v`, and the pointwise brightness / contrast / noise
// modes.  uint8 HWC images with 3 channels, arbitrary extents.  One straightforward pass each: a 2000 x 2000 tile is 12 MB.
// Compiled with -ffp-contract=off: the fp32 / fp64 expressions must round as written (they restate NumPy's and scikit-image's).
// No floating-point atomics (the reductions are integer: min / max / add).
#include "radnet_internal.h"

namespace {

constexpr int kAugReduceBlocks = 1024;      // grid cap of the two reductions (one flush of LDS partials per workgroup)

// ---- index gather ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) aug_gather_kernel(const uint8_t* __restrict__ src, int sw, int y0, int x0, int transform,
                                                         uint8_t* __restrict__ dst, int dh, int dw) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)dh * dw) return;
  const int y = (int)(idx / dw), x = (int)(idx - (long long)y * dw);
  const int yy = (transform & 1) ? dh - 1 - y : y, xx = (transform & 2) ? dw - 1 - x : x;
  const int wy = (transform & 4) ? xx : yy, wx = (transform & 4) ? yy : xx;
  const uint8_t* s = src + ((long long)(y0 + wy) * sw + (x0 + wx)) * 3;
  uint8_t* d = dst + idx * 3;
  d[0] = s[0];
  d[1] = s[1];
  d[2] = s[2];
}

// ---- strap extent ------------------------------------------------------------------------------------------------------------
__global__ void aug_extent_init_kernel(int* __restrict__ out) {
  out[0] = out[2] = 0x7fffffff;
  out[1] = out[3] = -1;
}

__global__ void __launch_bounds__(256) aug_extent_kernel(const uint8_t* __restrict__ img, int h, int w, int* __restrict__ out) {
  __shared__ int part[4];
  if (threadIdx.x == 0) {
    part[0] = part[2] = 0x7fffffff;
    part[1] = part[3] = -1;
  }
  __syncthreads();
  const long long total = (long long)h * w;
  int r0 = 0x7fffffff, r1 = -1, c0 = 0x7fffffff, c1 = -1;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
    if (img[idx * 3 + 1] != 0) {
      const int y = (int)(idx / w), x = (int)(idx - (long long)y * w);
      r0 = min(r0, y);
      r1 = max(r1, y);
      c0 = min(c0, x);
      c1 = max(c1, x);
    }
  }
  if (r1 >= 0) {
    atomicMin(&part[0], r0);
    atomicMax(&part[1], r1);
    atomicMin(&part[2], c0);
    atomicMax(&part[3], c1);
  }
  __syncthreads();
  if (threadIdx.x == 0 && part[1] >= 0) {
    atomicMin(&out[0], part[0]);
    atomicMax(&out[1], part[1]);
    atomicMin(&out[2], part[2]);
    atomicMax(&out[3], part[3]);
  }
}

// ---- histogram ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) aug_hist_kernel(const uint8_t* __restrict__ img, long long n, int step, unsigned* __restrict__ bins) {
  __shared__ unsigned local[256];
  local[threadIdx.x] = 0;
  __syncthreads();
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    atomicAdd(&local[img[i * step]], 1u);
  __syncthreads();
  if (local[threadIdx.x]) atomicAdd(&bins[threadIdx.x], local[threadIdx.x]);
}

// ---- Philox4x32-10 -----------------------------------------------------------------------------------------------------------
struct Uniforms {
  double a, b;
};

__device__ __forceinline__ Uniforms philox_uniforms(unsigned long long index, unsigned field_id, unsigned k0, unsigned k1) {
  unsigned c0 = (unsigned)index, c1 = (unsigned)(index >> 32), c2 = field_id, c3 = 0;
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned)p1;
    c3 = (unsigned)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  Uniforms u;
  u.a = ((double)((((unsigned long long)c0 << 32) | c1) >> 11) + 0.5) * 0x1p-53;
  u.b = ((double)((((unsigned long long)c2 << 32) | c3) >> 11) + 0.5) * 0x1p-53;
  return u;
}

// ---- pointwise modes ---------------------------------------------------------------------------------------------------------
// random_noise + img_as_ubyte for one element: v / 255.0, the mode, clip to [0, 1], rint(x * 255) half-to-even
template <int MODE>
__device__ __forceinline__ uint8_t noisy(uint8_t v, unsigned long long index, double p0, double p1, unsigned k0, unsigned k1, unsigned field_id) {
  const Uniforms u = philox_uniforms(index, field_id, k0, k1);
  const double f = (double)v / 255.0;
  double x;
  if (MODE == RADNET_AUG_SALT_PEPPER) {
    x = f;
    if (u.a <= p0) x = (u.b <= p1) ? 1.0 : 0.0;
  } else if (MODE == RADNET_AUG_GAUSSIAN) {
    const double z = sqrt(-2.0 * log(u.a)) * cos(6.283185307179586 * u.b);
    x = f + (p0 + p1 * z);
  } else {
    const double lam = f * p0;
    double p = exp(-lam), s = p;
    int k = 0;
    while (u.a > s && k < 1023) {
      k += 1;
      p *= lam / (double)k;
      s += p;
    }
    x = (double)k / p0;
  }
  x = fmin(fmax(x, 0.0), 1.0);
  return (uint8_t)fmin(fmax(rint(x * 255.0), 0.0), 255.0);
}

template <int MODE>
__global__ void __launch_bounds__(256) aug_pointwise_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, long long pixels, int grey,
                                                            double p0, double p1, unsigned k0, unsigned k1, unsigned field_id) {
  const long long pix = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= pixels) return;
  const uint8_t* s = src + pix * 3;
  uint8_t* d = dst + pix * 3;
  if (MODE == RADNET_AUG_BRIGHTNESS) {
    const float delta = (float)p0;
    for (int c = 0; c < 3; ++c) {
      float f = (float)s[c];
      if (p1 != 0.0) f -= delta; else f += delta;
      f = fminf(fmaxf(f, 0.f), 255.f);
      d[c] = s[c] == 0 ? (uint8_t)0 : (uint8_t)f;
    }
  } else if (MODE == RADNET_AUG_CONTRAST) {
    for (int c = 0; c < 3; ++c) {
      double f = fmin(fmax((double)s[c], p0), p1);
      if (p0 != p1) f = (f - p0) / (p1 - p0);
      d[c] = (uint8_t)(long long)(f * 255.0);
    }
  } else if (grey) {
    const uint8_t v = s[0] == 0 ? (uint8_t)0 : noisy<MODE>(s[0], (unsigned long long)pix, p0, p1, k0, k1, field_id);
    d[0] = d[1] = d[2] = v;
  } else {
    for (int c = 0; c < 3; ++c)
      d[c] = s[c] == 0 ? (uint8_t)0 : noisy<MODE>(s[c], (unsigned long long)pix * 3 + c, p0, p1, k0, k1, field_id);
  }
}

template <int MODE>
void launch_pointwise(radnet_ctx* ctx, const uint8_t* src, uint8_t* dst, long long pixels, int grey, double p0, double p1, uint64_t seed,
                      uint32_t field_id) {
  hipLaunchKernelGGL(aug_pointwise_kernel<MODE>, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, ctx->stream, src, dst, pixels, grey, p0, p1,
                     (unsigned)seed, (unsigned)(seed >> 32), field_id);
}

}  // namespace

extern "C" int radnet_aug_gather_u8(radnet_ctx* ctx, const uint8_t* src, int32_t sh, int32_t sw, int32_t y0, int32_t x0, int32_t wh, int32_t ww,
                                    int32_t transform, uint8_t* dst) {
  if (!ctx || !src || !dst || sh <= 0 || sw <= 0 || wh <= 0 || ww <= 0 || y0 < 0 || x0 < 0 || transform < 0 || transform > 7) return RADNET_ERR_ARG;
  if ((long long)y0 + wh > sh || (long long)x0 + ww > sw) RADNET_FAIL(ctx, RADNET_ERR_ARG, "aug_gather: window %d+%d x %d+%d outside %d x %d", y0, wh, x0, ww, sh, sw);
  const long long total = (long long)wh * ww;
  if (total >= (1ll << 31)) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "aug_gather: %lld output pixels", total);
  const int dh = (transform & 4) ? ww : wh, dw = (transform & 4) ? wh : ww;
  hipLaunchKernelGGL(aug_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, src, sw, y0, x0, transform, dst, dh, dw);
  RADNET_CHECK_LAUNCH(ctx, "aug_gather_u8");
  return RADNET_OK;
}

extern "C" int radnet_aug_extent_u8(radnet_ctx* ctx, const uint8_t* img, int32_t h, int32_t w, int32_t* out4) {
  if (!ctx || !img || !out4 || h <= 0 || w <= 0) return RADNET_ERR_ARG;
  const long long total = (long long)h * w;
  hipLaunchKernelGGL(aug_extent_init_kernel, dim3(1), dim3(1), 0, ctx->stream, out4);
  RADNET_CHECK_LAUNCH(ctx, "aug_extent_init");
  const long long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(aug_extent_kernel, dim3((unsigned)std::min<long long>(blocks, kAugReduceBlocks)), dim3(256), 0, ctx->stream, img, h, w, out4);
  RADNET_CHECK_LAUNCH(ctx, "aug_extent_u8");
  return RADNET_OK;
}

extern "C" int radnet_aug_histogram_u8(radnet_ctx* ctx, const uint8_t* img, int32_t h, int32_t w, int32_t all_channels, uint32_t* bins256) {
  if (!ctx || !img || !bins256 || h <= 0 || w <= 0) return RADNET_ERR_ARG;
  const long long n = (long long)h * w * (all_channels ? 3 : 1);
  if (n >= (1ll << 32)) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "aug_histogram: %lld elements overflow a 32-bit bin", n);
  RADNET_CHECK_HIP(ctx, hipMemsetAsync(bins256, 0, 256 * sizeof(uint32_t), ctx->stream));
  const long long blocks = (n + 255) / 256;
  hipLaunchKernelGGL(aug_hist_kernel, dim3((unsigned)std::min<long long>(blocks, kAugReduceBlocks)), dim3(256), 0, ctx->stream, img, n, all_channels ? 1 : 3,
                     bins256);
  RADNET_CHECK_LAUNCH(ctx, "aug_histogram_u8");
  return RADNET_OK;
}

extern "C" int radnet_aug_pointwise_u8(radnet_ctx* ctx, const uint8_t* src, uint8_t* dst, int32_t h, int32_t w, int32_t mode, int32_t grey, double p0,
                                       double p1, uint64_t noise_seed, uint32_t field_id) {
  if (!ctx || !src || !dst || h <= 0 || w <= 0) return RADNET_ERR_ARG;
  const long long pixels = (long long)h * w;
  if (pixels >= (1ll << 31)) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "aug_pointwise: %lld pixels", pixels);
  switch (mode) {
    case RADNET_AUG_BRIGHTNESS:
      if (!(p0 >= 0.0)) RADNET_FAIL(ctx, RADNET_ERR_ARG, "aug_pointwise: brightness delta %g", p0);
      launch_pointwise<RADNET_AUG_BRIGHTNESS>(ctx, src, dst, pixels, 0, p0, p1, 0, 0);
      break;
    case RADNET_AUG_CONTRAST:
      if (!(p0 <= p1)) RADNET_FAIL(ctx, RADNET_ERR_ARG, "aug_pointwise: contrast range %g > %g", p0, p1);
      launch_pointwise<RADNET_AUG_CONTRAST>(ctx, src, dst, pixels, 0, p0, p1, 0, 0);
      break;
    case RADNET_AUG_SALT_PEPPER:
      launch_pointwise<RADNET_AUG_SALT_PEPPER>(ctx, src, dst, pixels, grey, p0, p1, noise_seed, field_id);
      break;
    case RADNET_AUG_GAUSSIAN:
      if (!(p1 >= 0.0)) RADNET_FAIL(ctx, RADNET_ERR_ARG, "aug_pointwise: gaussian sigma %g", p1);
      launch_pointwise<RADNET_AUG_GAUSSIAN>(ctx, src, dst, pixels, grey, p0, p1, noise_seed, field_id);
      break;
    case RADNET_AUG_POISSON:
      if (!(p0 >= 1.0 && p0 <= 256.0)) RADNET_FAIL(ctx, RADNET_ERR_ARG, "aug_pointwise: poisson v %g outside [1, 256]", p0);
      launch_pointwise<RADNET_AUG_POISSON>(ctx, src, dst, pixels, grey, p0, p1, noise_seed, field_id);
      break;
    default:
      RADNET_FAIL(ctx, RADNET_ERR_ARG, "aug_pointwise: mode %d", mode);
  }
  RADNET_CHECK_LAUNCH(ctx, "aug_pointwise_u8");
  return RADNET_OK;
}
