// keras.optimizers.Adam (Keras 2 update rule, train.py:236-252) over one flat fp32 arena: radnet_adam_step, _affine, _fused, _bf16.
// One update routine (adam_at), one flat sweep (adam_sweep) and one host path (adam_prepare) serve all four entry points; what
// differs is the work of the layers an entry point lists, which leave the sweep for workgroups of their own behind it in the grid:
//   adam_kernel       3x3 kernels whose Winograd F(4x4,3x3) filter transform is rewritten from the new weights (radnet_adam_step_fused)
//   adam_bf16_kernel  conv kernels whose bf16 image is rewritten from the new weights                             (radnet_adam_step_bf16)
// Two kernels, not one: the Winograd transform costs adam_kernel its registers, and the bf16 path would pay for them in occupancy.
// Every arena (p, g, m, v) must be 16-byte aligned -- all paths read float4 -- and ALL FOUR entry points refuse one that is not
// (radnet_adam_step_bf16 alone did once); every caller in the tree passes whole allocations.
#include "radnet_internal.h"
#include "adam_update.h"
#include "radnet_wino4.h"

namespace {

constexpr int kAdamWinoMax = 12;
constexpr int kAdamBf16Max = 16;
constexpr int kAdamBf16Tile = 64;
constexpr int kAdamGapMax = kAdamBf16Max + 1;      // n listed layers leave n + 1 gaps

// What both kernels take.  aff_*: optionally the folded epilogue shifts of the convs whose biases live in float4 chunks
// [aff_off4, aff_off4 + aff_n4) of the arena are refreshed from the just-updated biases in the same pass: shift = scale * bias + t0
// (FixedBatchNormalization.py:59-85 folded; one launch fewer on the classifier lane per step).
// The flat sweep runs over the arena WITHOUT the listed layers: its index j lies in gap q when pref[q] <= j < pref[q + 1] and stands
// for float4 gap0[q] + j - pref[q] (a sweep over the whole arena that skips the layers spends its time skipping them).
struct AdamArgs {
  float4 *p, *g, *m, *v;
  float lr_t, b1, b2, eps, gs;
  int zero_grad;
  long long aff_off4, aff_n4;
  const float4 *aff_scale, *aff_t0;
  float4* aff_shift;
  long long gap0[kAdamGapMax], pref[kAdamGapMax + 1];
  int ngap;
  unsigned sweep_blocks;          // workgroups of the flat sweep (the layers' workgroups follow)
};

__device__ __forceinline__ void adam_one(float4& pp, const float4& gg, float4& mm, float4& vv, float lr_t, float b1, float b2, float eps, float gs) {
  adam_update1(pp.x, gg.x, mm.x, vv.x, lr_t, b1, b2, eps, gs);
  adam_update1(pp.y, gg.y, mm.y, vv.y, lr_t, b1, b2, eps, gs);
  adam_update1(pp.z, gg.z, mm.z, vv.z, lr_t, b1, b2, eps, gs);
  adam_update1(pp.w, gg.w, mm.w, vv.w, lr_t, b1, b2, eps, gs);
}

// Adam on float4 chunk i of the arena; returns the new weights.
__device__ __forceinline__ float4 adam_at(const AdamArgs& a, long long i) {
  float4 pp = a.p[i], mm = a.m[i], vv = a.v[i];
  adam_one(pp, a.g[i], mm, vv, a.lr_t, a.b1, a.b2, a.eps, a.gs);
  a.p[i] = pp;
  a.m[i] = mm;
  a.v[i] = vv;
  if (a.zero_grad) a.g[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  return pp;
}

// The flat sweep of workgroups [0, sweep_blocks) over the gaps, with the shift refresh.  The gap of j is found on wave-uniform
// table entries (scalar loads, a select per gap).
__device__ __forceinline__ void adam_sweep(const AdamArgs& a) {
  const long long rest = a.pref[a.ngap];
  for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < rest; j += (long long)a.sweep_blocks * blockDim.x) {
    long long at = a.gap0[0];
    for (int q = 1; q < a.ngap; ++q) {
      const long long first = a.pref[q], to = a.gap0[q] - first;      // both loaded before the compare: one wait per gap
      at = j >= first ? to : at;
    }
    const long long i = at + j;
    const float4 pp = adam_at(a, i);
    if (a.aff_shift != nullptr && i >= a.aff_off4 && i < a.aff_off4 + a.aff_n4) {
      const long long s = i - a.aff_off4;
      const float4 sc = a.aff_scale[s], c = a.aff_t0[s];
      a.aff_shift[s] = make_float4(sc.x * pp.x + c.x, sc.y * pp.y + c.y, sc.z * pp.z + c.z, sc.w * pp.w + c.w);
    }
  }
}

// radnet_adam_step_fused: 3x3 kernels [3][3][C][N] inside the arena whose Winograd F(4x4,3x3) transform U = G g G^T [36][C][N] is
// rewritten in the same launch.  A workgroup owns 64 consecutive float4 chunks (c, 4 n) of a layer with all nine taps -- phase 1,
// every thread: the Adam update of its share of the 9 x 64 chunks, coalesced, new weights also into LDS; phase 2, one thread per
// chunk: the transform of its nine float4 values, wino4_filter_kernel's code, 36 coalesced 16-byte stores.  The transformed filters
// cost their own bytes (4x the kernels') and no launch (three launches cost the classifier lane as much as the Winograd forward
// gives: DESIGN.md 4).
struct AdamWino {
  long long off4[kAdamWinoMax];   // first float4 of the layer's kernel in the arena
  int cn4[kAdamWinoMax];          // C * N / 4: float4 chunks per tap (a multiple of 64)
  int unit0[kAdamWinoMax + 1];    // first workgroup (relative to the first Winograd workgroup) of each layer; [n] = their total
  float* u[kAdamWinoMax];
  int n;
  int load_only;                  // radnet_adam_step_tail: the layers' weights are already updated (Adam in the weight gradient's tile
                                  // epilogue, conv_wgrad_body.h): phase 1 only reads them, phase 2 transforms them as ever
};
__global__ void __launch_bounds__(256) adam_kernel(AdamArgs a, AdamWino wz) {
  if (blockIdx.x < a.sweep_blocks) {
    adam_sweep(a);
    return;
  }
  __shared__ float4 taps[9][64];
  const int unit = (int)(blockIdx.x - a.sweep_blocks);
  int layer = 0;
  for (int l = 1; l < wz.n; ++l)
    if (unit >= wz.unit0[l]) layer = l;
  const int cn4 = wz.cn4[layer];
  const long long j0 = (long long)(unit - wz.unit0[layer]) * 64;
  for (int it = threadIdx.x; it < 9 * 64; it += 256) {
    const int tap = it >> 6, jj = it & 63;
    const long long i = wz.off4[layer] + (long long)tap * cn4 + j0 + jj;
    taps[tap][jj] = wz.load_only ? a.p[i] : adam_at(a, i);
  }
  __syncthreads();
  // phase 2: wino4_filter_kernel's own code on the same vector type (one thread per float4 chunk), so that both produce the same bits
  // (dealing the six output rows to three waves changed nothing measurable -- 84 against 85 us -- and the compiler's FMA choices with it)
  if (threadIdx.x < 64) {
    float4 t[6][3];
#pragma unroll
    for (int bb = 0; bb < 3; ++bb) {
      float4 col[3], o[6];
#pragma unroll
      for (int aa = 0; aa < 3; ++aa) col[aa] = taps[aa * 3 + bb][threadIdx.x];
      g6(col, o);
#pragma unroll
      for (int aa = 0; aa < 6; ++aa) t[aa][bb] = o[aa];
    }
    float4* dst = reinterpret_cast<float4*>(wz.u[layer]) + j0 + threadIdx.x;
#pragma unroll
    for (int aa = 0; aa < 6; ++aa) {
      float4 o[6];
      g6(t[aa], o);
#pragma unroll
      for (int bb = 0; bb < 6; ++bb) dst[(long long)(6 * aa + bb) * cn4] = o[bb];
    }
  }
}

// radnet_adam_step_bf16 (bf16-mixed training): conv kernels [k][ldw] inside the arena whose bf16 [n][ldk] image -- the operand the
// bf16 forward convs read (conv_bf16.hip) -- is rewritten in the same launch.  A workgroup owns a 64 k x 64 n tile; phase 1, every
// thread: the Adam update of four float4 chunks of its rows, coalesced along n, new weights into LDS (zeros for rows k..ldk);
// phase 2: the tile transposed out of LDS, eight consecutive k of one output column per thread, rounded as weights_to_bf16_kernel
// rounds (to nearest, ties to even) and written as one 16-byte store -- coalesced along k.  Same adam_one, same conversion:
// bit-identical to Adam followed by radnet_weights_to_bf16.
struct AdamBf16 {
  long long off4[kAdamBf16Max];   // first float4 of the layer's kernel in the arena
  int k[kAdamBf16Max], n[kAdamBf16Max], ldw4[kAdamBf16Max], ldk[kAdamBf16Max];
  int ntn[kAdamBf16Max];          // n tiles per k tile row: cdiv(ldw, 64)
  int unit0[kAdamBf16Max + 1];    // first workgroup (relative to the first tile workgroup) of each layer; [n] = their total
  uint16_t* wt[kAdamBf16Max];
  int nl;
};
__global__ void __launch_bounds__(256) adam_bf16_kernel(AdamArgs a, AdamBf16 lz) {
  if (blockIdx.x < a.sweep_blocks) {
    adam_sweep(a);
    return;
  }
  __shared__ float tile[kAdamBf16Tile][kAdamBf16Tile + 1];     // [k][n], odd pitch: the transposed reads hit 64 different banks
  const int unit = (int)(blockIdx.x - a.sweep_blocks);
  int layer = 0;
  for (int l = 1; l < lz.nl; ++l)
    if (unit >= lz.unit0[l]) layer = l;
  const int u = unit - lz.unit0[layer];
  const int k0 = (u / lz.ntn[layer]) * kAdamBf16Tile, n0 = (u % lz.ntn[layer]) * kAdamBf16Tile;
  const int K = lz.k[layer], ldw4 = lz.ldw4[layer];
  const int c4 = threadIdx.x & 15;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int r = (threadIdx.x >> 4) + 16 * it;
    const int kk = k0 + r, j4 = n0 / 4 + c4;
    float4 pp = make_float4(0.f, 0.f, 0.f, 0.f);
    if (kk < K && j4 < ldw4) pp = adam_at(a, lz.off4[layer] + (long long)kk * ldw4 + j4);
    tile[r][4 * c4] = pp.x; tile[r][4 * c4 + 1] = pp.y; tile[r][4 * c4 + 2] = pp.z; tile[r][4 * c4 + 3] = pp.w;
  }
  __syncthreads();
  const int N = lz.n[layer], ldk = lz.ldk[layer];
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int q = threadIdx.x + 256 * it;           // 64 columns x 8 chunks of 8 k
    const int c = q >> 3, kc = (q & 7) * 8;
    const int col = n0 + c, kk = k0 + kc;
    if (col >= N || kk >= ldk) continue;            // ldk % 8 == 0: a chunk lies wholly inside [0, ldk) or wholly outside
    uint16_t h[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) h[e] = kk + e < K ? __builtin_bit_cast(uint16_t, (__bf16)tile[kc + e][c]) : (uint16_t)0;
    uint4 o;
    o.x = h[0] | ((unsigned)h[1] << 16); o.y = h[2] | ((unsigned)h[3] << 16);
    o.z = h[4] | ((unsigned)h[5] << 16); o.w = h[6] | ((unsigned)h[7] << 16);
    *reinterpret_cast<uint4*>(lz.wt[layer] + (long long)col * ldk + kk) = o;
  }
}

// ---- host side: one argument check, one lr_t, one gap table ------------------------------------------------------
struct AdamRange {
  int64_t off, len;               // floats [off, off + len) of the arena that a listed layer owns
};

// lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t)   (keras.optimizers.Adam.get_updates)
float adam_lr_t(float lr, float beta1, float beta2, int t) { return radnet_adam_lr_t(lr, beta1, beta2, t); }

// What all four entry points ask of their common arguments; `who` names the entry point in the message.
int adam_check(radnet_ctx* ctx, const char* who, const float* p, const float* g, const float* m, const float* v, int64_t n, int32_t t,
               int64_t bias_off, int64_t bias_len, const float* scale, const float* t0, const float* shift) {
  if (!p || !g || !m || !v) RADNET_FAIL(ctx, RADNET_ERR_ARG, "%s: null arena", who);
  if (shift != nullptr && (!scale || !t0)) RADNET_FAIL(ctx, RADNET_ERR_ARG, "%s: shift without scale / t0", who);
  if ((n % 4) || (bias_off % 4) || (bias_len % 4) || n < 0 || bias_off < 0 || bias_len < 0 || bias_off + bias_len > n)
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "%s: arena length %lld, bias range [%lld, +%lld) must be multiples of 4 inside the arena", who, (long long)n,
                (long long)bias_off, (long long)bias_len);
  if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) RADNET_FAIL(ctx, RADNET_ERR_ARG, "%s: arenas must be 16-byte aligned", who);
  if (shift && (((uintptr_t)scale | (uintptr_t)t0 | (uintptr_t)shift) & 15)) RADNET_FAIL(ctx, RADNET_ERR_ARG, "%s: scale / t0 / shift must be 16-byte aligned", who);
  if (t < 1) RADNET_FAIL(ctx, RADNET_ERR_ARG, "%s: step counter starts at 1", who);
  return RADNET_OK;
}

// The gaps that the nr listed ranges leave in the arena, in arena order, and the sweep's grid over them.  Refuses ranges that
// leave the arena or overlap each other or the bias range [bias_off, +bias_len).  Reorders r.
int adam_gaps(radnet_ctx* ctx, const char* who, AdamRange* r, int nr, int64_t n, int64_t bias_off, int64_t bias_len, AdamArgs& a) {
  std::sort(r, r + nr, [](const AdamRange& x, const AdamRange& y) { return x.off < y.off; });
  long long at4 = 0;
  a.ngap = 0;
  a.pref[0] = 0;
  for (int q = 0; q <= nr; ++q) {
    if (q < nr) {
      if ((r[q].off & 3) || (r[q].len & 3) || r[q].off < 0 || r[q].len <= 0 || r[q].off + r[q].len > n)
        RADNET_FAIL(ctx, RADNET_ERR_ARG, "%s: layer [%lld, +%lld) must be multiples of 4 inside the arena", who, (long long)r[q].off, (long long)r[q].len);
      if (r[q].off / 4 < at4) RADNET_FAIL(ctx, RADNET_ERR_ARG, "%s: the layers at %lld and %lld overlap", who, (long long)r[q - 1].off, (long long)r[q].off);
      if (bias_len > 0 && r[q].off < bias_off + bias_len && bias_off < r[q].off + r[q].len)
        RADNET_FAIL(ctx, RADNET_ERR_ARG, "%s: layer [%lld, +%lld) overlaps the bias range", who, (long long)r[q].off, (long long)r[q].len);
    }
    const long long end4 = q < nr ? r[q].off / 4 : n / 4;
    a.gap0[a.ngap] = at4;
    a.pref[a.ngap + 1] = a.pref[a.ngap] + (end4 - at4);
    ++a.ngap;
    if (q < nr) at4 = end4 + r[q].len / 4;
  }
  a.sweep_blocks = (unsigned)grid_for(std::max<long long>(a.pref[a.ngap], 1), 256, 8192);
  return RADNET_OK;
}

// Checks the common arguments and fills the kernels' parameter block; launches nothing.
int adam_prepare(radnet_ctx* ctx, const char* who, float* p, float* g, float* m, float* v, int64_t n, int32_t t, float lr, float beta1,
                 float beta2, float eps, float grad_scale, int32_t zero_grad, int64_t bias_off, int64_t bias_len, const float* scale,
                 const float* t0, float* shift, AdamRange* r, int nr, AdamArgs& a) {
  if (int rc = adam_check(ctx, who, p, g, m, v, n, t, bias_off, bias_len, scale, t0, shift)) return rc;
  a.p = reinterpret_cast<float4*>(p); a.g = reinterpret_cast<float4*>(g); a.m = reinterpret_cast<float4*>(m); a.v = reinterpret_cast<float4*>(v);
  a.lr_t = adam_lr_t(lr, beta1, beta2, t);
  a.b1 = beta1; a.b2 = beta2; a.eps = eps; a.gs = grad_scale;
  a.zero_grad = (int)zero_grad;
  a.aff_off4 = bias_off / 4;
  a.aff_n4 = shift ? bias_len / 4 : 0;
  a.aff_scale = reinterpret_cast<const float4*>(scale); a.aff_t0 = reinterpret_cast<const float4*>(t0); a.aff_shift = reinterpret_cast<float4*>(shift);
  return adam_gaps(ctx, who, r, nr, n, bias_off, shift ? bias_len : 0, a);
}

int adam_fused(radnet_ctx* ctx, const char* who, float* p, float* g, float* m, float* v, int64_t n, int32_t t, float lr, float beta1,
               float beta2, float eps, float grad_scale, int32_t zero_grad, int64_t bias_off, int64_t bias_len, const float* scale,
               const float* t0, float* shift, const radnet_adam_wino* layers, int32_t n_layers, int64_t sweep_from = 0) {
  if (!ctx) return RADNET_ERR_ARG;
  if (n_layers < 0 || n_layers > kAdamWinoMax || (n_layers > 0 && !layers)) RADNET_FAIL(ctx, RADNET_ERR_ARG, "%s: %d layers (at most %d, in a table)", who, n_layers, kAdamWinoMax);
  AdamWino wz{};
  AdamRange r[kAdamGapMax];
  wz.n = n_layers;
  wz.load_only = sweep_from > 0 ? 1 : 0;
  for (int l = 0; l < n_layers; ++l) {
    const radnet_adam_wino& d = layers[l];
    if (!d.u || d.c <= 0 || d.n <= 0 || (d.n & 3) || ((uintptr_t)d.u & 15) || (int64_t)d.c * d.n / 4 >= (1ll << 28) || ((int64_t)d.c * d.n / 4) % 64)
      RADNET_FAIL(ctx, RADNET_ERR_ARG, "%s: layer %d (offset %lld, c %d, n %d) does not describe a dense [3][3][c][n] kernel with c*n a multiple of 256 and a 16-byte aligned u",
                  who, l, (long long)d.off, d.c, d.n);
    wz.off4[l] = d.off / 4;
    wz.cn4[l] = (int)((int64_t)d.c * d.n / 4);
    wz.u[l] = d.u;
    wz.unit0[l + 1] = wz.unit0[l] + wz.cn4[l] / 64;
    r[l] = {d.off, 9ll * d.c * d.n};
  }
  int nr = n_layers;
  if (sweep_from > 0) {
    // the sweep covers [sweep_from, n) only: what lies in front of it and is no listed layer leaves the sweep as ranges of its own
    // (nobody's workgroups: those weights were updated elsewhere)
    if ((sweep_from & 3) || sweep_from > n) RADNET_FAIL(ctx, RADNET_ERR_ARG, "%s: sweep_from %lld must be a multiple of 4 inside the arena", who, (long long)sweep_from);
    std::sort(r, r + n_layers, [](const AdamRange& x, const AdamRange& y) { return x.off < y.off; });
    int64_t at = 0;
    for (int l = 0; l <= n_layers; ++l) {
      const int64_t end = l < n_layers ? r[l].off : sweep_from;
      if (l < n_layers && (r[l].off < at || r[l].off + r[l].len > sweep_from))
        RADNET_FAIL(ctx, RADNET_ERR_ARG, "%s: layer [%lld, +%lld) overlaps another or reaches past sweep_from", who, (long long)r[l].off, (long long)r[l].len);
      if (end > at) {
        if (nr + 1 >= kAdamGapMax) RADNET_FAIL(ctx, RADNET_ERR_ARG, "%s: too many layers for the gap table", who);
        r[nr++] = {at, end - at};
      }
      if (l < n_layers) at = r[l].off + r[l].len;
    }
  }
  AdamArgs a{};
  if (int rc = adam_prepare(ctx, who, p, g, m, v, n, t, lr, beta1, beta2, eps, grad_scale, zero_grad, bias_off, bias_len, scale, t0, shift, r, nr, a)) return rc;
  hipLaunchKernelGGL(adam_kernel, dim3(a.sweep_blocks + (unsigned)wz.unit0[n_layers]), dim3(256), 0, ctx->stream, a, wz);
  RADNET_CHECK_LAUNCH(ctx, who);
  return RADNET_OK;
}

}  // namespace

extern "C" int radnet_adam_step(radnet_ctx* ctx, float* p, float* g, float* m, float* v, int64_t n, int32_t t, float lr, float beta1,
                                float beta2, float eps, float grad_scale, int32_t zero_grad) {
  return adam_fused(ctx, "adam", p, g, m, v, n, t, lr, beta1, beta2, eps, grad_scale, zero_grad, 0, 0, nullptr, nullptr, nullptr, nullptr, 0);
}

extern "C" int radnet_adam_step_affine(radnet_ctx* ctx, float* p, float* g, float* m, float* v, int64_t n, int32_t t, float lr, float beta1,
                                       float beta2, float eps, float grad_scale, int32_t zero_grad, int64_t bias_off, int64_t bias_len,
                                       const float* scale, const float* t0, float* shift) {
  if (!ctx) return RADNET_ERR_ARG;
  if (!scale || !t0 || !shift) RADNET_FAIL(ctx, RADNET_ERR_ARG, "adam_affine: null scale / t0 / shift");
  return adam_fused(ctx, "adam_affine", p, g, m, v, n, t, lr, beta1, beta2, eps, grad_scale, zero_grad, bias_off, bias_len, scale, t0, shift, nullptr, 0);
}

extern "C" int radnet_adam_step_fused(radnet_ctx* ctx, float* p, float* g, float* m, float* v, int64_t n, int32_t t, float lr, float beta1,
                                      float beta2, float eps, float grad_scale, int32_t zero_grad, int64_t bias_off, int64_t bias_len,
                                      const float* scale, const float* t0, float* shift, const radnet_adam_wino* layers, int32_t n_layers) {
  return adam_fused(ctx, "adam_fused", p, g, m, v, n, t, lr, beta1, beta2, eps, grad_scale, zero_grad, bias_off, bias_len, scale, t0, shift, layers, n_layers);
}

// Adam over the arena's tail [sweep_from, n) and, in the same launch, the Winograd filters of the listed 3x3 layers from weights that are
// ALREADY updated (radnet_conv_wgrad_multi's optimizer epilogue): the layers' workgroups read the weights instead of stepping them.
extern "C" int radnet_adam_step_tail(radnet_ctx* ctx, float* p, float* g, float* m, float* v, int64_t n, int32_t t, float lr, float beta1,
                                     float beta2, float eps, float grad_scale, int32_t zero_grad, int64_t bias_off, int64_t bias_len,
                                     const float* scale, const float* t0, float* shift, const radnet_adam_wino* layers, int32_t n_layers,
                                     int64_t sweep_from) {
  if (!ctx) return RADNET_ERR_ARG;
  if (sweep_from <= 0) RADNET_FAIL(ctx, RADNET_ERR_ARG, "adam_tail: sweep_from must be positive (radnet_adam_step_fused sweeps the whole arena)");
  if (shift != nullptr && bias_off < sweep_from) RADNET_FAIL(ctx, RADNET_ERR_ARG, "adam_tail: the bias range starts in front of the sweep");
  return adam_fused(ctx, "adam_tail", p, g, m, v, n, t, lr, beta1, beta2, eps, grad_scale, zero_grad, bias_off, bias_len, scale, t0, shift, layers, n_layers, sweep_from);
}

extern "C" int radnet_adam_step_bf16(radnet_ctx* ctx, float* p, float* g, float* m, float* v, int64_t n, int32_t t, float lr, float beta1,
                                     float beta2, float eps, float grad_scale, int32_t zero_grad, int64_t bias_off, int64_t bias_len,
                                     const float* scale, const float* t0, float* shift, const radnet_adam_bf16* layers, int32_t n_layers) {
  const char* who = "adam_bf16";
  if (!ctx) return RADNET_ERR_ARG;
  if (n_layers < 0 || n_layers > kAdamBf16Max || (n_layers > 0 && !layers)) RADNET_FAIL(ctx, RADNET_ERR_ARG, "%s: %d layers (at most %d, in a table)", who, n_layers, kAdamBf16Max);
  AdamBf16 lz{};
  AdamRange r[kAdamBf16Max];
  lz.nl = n_layers;
  for (int l = 0; l < n_layers; ++l) {
    const radnet_adam_bf16& d = layers[l];
    if (!d.wt || d.k <= 0 || d.n <= 0 || d.ldw < d.n || (d.ldw & 3) || (d.off & 3) || d.ldk < d.k || (d.ldk & 7) || ((uintptr_t)d.wt & 15) ||
        d.k >= (1 << 24) || d.ldk >= (1 << 24) || d.ldw >= (1 << 20))
      RADNET_FAIL(ctx, RADNET_ERR_ARG, "%s: layer %d (k %d, n %d, ldw %d, ldk %d): needs ldw >= n, ldk >= k, ldw %% 4 == 0, ldk %% 8 == 0, "
                  "offset %% 4 == 0, a 16-byte aligned image", who, l, d.k, d.n, d.ldw, d.ldk);
    lz.off4[l] = d.off / 4;
    lz.k[l] = d.k; lz.n[l] = d.n; lz.ldw4[l] = d.ldw / 4; lz.ldk[l] = d.ldk; lz.wt[l] = d.wt;
    lz.ntn[l] = radnet_cdiv(d.ldw, kAdamBf16Tile);
    lz.unit0[l + 1] = lz.unit0[l] + radnet_cdiv(std::max(d.k, d.ldk), kAdamBf16Tile) * lz.ntn[l];
    r[l] = {d.off, (int64_t)d.k * d.ldw};
  }
  AdamArgs a{};
  if (int rc = adam_prepare(ctx, who, p, g, m, v, n, t, lr, beta1, beta2, eps, grad_scale, zero_grad, bias_off, bias_len, scale, t0, shift, r, n_layers, a)) return rc;
  hipLaunchKernelGGL(adam_bf16_kernel, dim3(a.sweep_blocks + (unsigned)lz.unit0[n_layers]), dim3(256), 0, ctx->stream, a, lz);
  RADNET_CHECK_LAUNCH(ctx, who);
  return RADNET_OK;
}
