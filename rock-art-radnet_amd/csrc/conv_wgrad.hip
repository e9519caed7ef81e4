// Weight gradients on the fp32 matrix cores: the kernels around conv_wgrad_body (conv_wgrad_body.h), the weight + data gradient
// of one layer as one launch, their launch policy (run_wgrad) and the C entry points.
#include "conv_host.h"
#include "conv_igemm_body.h"
#include "conv_wgrad_body.h"
#include "wgrad_multi_plan.h"

namespace {
template <int BMK, int BN>
__global__ void __launch_bounds__(NTHREADS) conv_wgrad_kernel(WgradArgs g) {
  __shared__ __attribute__((aligned(16))) float lds[wgrad_lds_floats<BMK, BN>()];
  if (g.batch > 1 && g.xcd_batch) {             // see conv_igemm_kernel: the tiles of one problem share its two operands
    const unsigned gx = gridDim.x, gy = gridDim.y, total = gx * gy * gridDim.z;
    const unsigned lin = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z), per = total >> 3;
    const unsigned l2 = lin < (per << 3) ? (lin & 7u) * per + (lin >> 3) : lin;
    const unsigned z = l2 / (gx * gy), r = l2 - z * gx * gy, y = r / gx;
    conv_wgrad_body<BMK, BN>(g, lds, r - y * gx, y, z);
    return;
  }
  conv_wgrad_body<BMK, BN>(g, lds, blockIdx.x, blockIdx.y, blockIdx.z);
}

// ---- data gradient and weight gradient of one layer in ONE launch ---------------------------------------------------------
// Both read the same dy and are independent of each other; as two launches on one stream they run one after the other, each
// with its own lockstep prologue / epilogue phases and launch gap.  Here the workgroups of the two problems alternate in the
// grid (even linear id: dgrad, odd: wgrad, the longer one fills the rest), so a CU holds workgroups of both and the phases of
// one hide under the K loops of the other.  64x64 tiles, 4 waves, for both (what the tuner picks for the classifier's layers).

// ABM: rows of the data gradient's output tile (64, or 32 since round 4: M = 980 rows are 31 tiles of 32 with no K slices to reduce)
template <int ABM>
__global__ void __launch_bounds__(NTHREADS) conv_bwd_pair_kernel(GemmArgs ga, WgradArgs gw, PairMap pm) {
  constexpr int kLds = igemm_lds_floats<ABM, 64, 1>() > wgrad_lds_floats<64, 64>() ? igemm_lds_floats<ABM, 64, 1>() : wgrad_lds_floats<64, 64>();
  __shared__ __attribute__((aligned(16))) float lds[kLds];
  const unsigned b = blockIdx.x, both = 2u * (pm.n_a < pm.n_w ? pm.n_a : pm.n_w);
  bool is_a;
  unsigned idx;
  if (b < both) {
    is_a = (b & 1u) == 0u;
    idx = b >> 1;
  } else {
    is_a = pm.n_a > pm.n_w;
    idx = b - both + (both >> 1);
  }
  if (is_a) {
    const unsigned by = idx / pm.ax;
    conv_igemm_body<ABM, 64, 1, false, 4>(ga, lds, idx - by * pm.ax, by, 0u, pm.ax);
  } else {
    const unsigned plane = pm.wx * pm.wy, bz = idx / plane, r = idx - bz * plane, by = r / pm.wx;
    conv_wgrad_body<64, 64>(gw, lds, r - by * pm.wx, by, bz);
  }
}

// ---- the weight gradients of several layers in ONE launch ---------------------------------------------------------------
// Up to kWgradMultiMax problems of one tile shape, each with the grid, the slices and the slice order of its single launch
// (radnet_conv_wgrad_multi lays the table out), one behind the other in a 1-D grid.  A workgroup finds its problem in the prefix
// table -- wave-uniform, once -- copies the problem's arguments out of the device table and runs conv_wgrad_body on them: a layer's
// prologue, tail and ordered reduction run beside the K loops of the layers around it instead of in a launch of their own.
template <int BMK, int BN>
__global__ void __launch_bounds__(NTHREADS) conv_wgrad_multi_kernel(const WgradArgs* __restrict__ tab, WgradMultiMap mp, WgradOptScalars os) {
  __shared__ __attribute__((aligned(16))) float lds[wgrad_lds_floats<BMK, BN>()];
  const unsigned b = blockIdx.x;
  int p = 0;
  for (int q = 1; q < mp.n; ++q)
    if (b >= mp.first[q]) p = q;
  const unsigned idx = b - mp.first[p], wx = mp.wx[p], plane = wx * mp.wy[p], bz = idx / plane, r = idx - bz * plane, by = r / wx;
  WgradArgs g = tab[p];
  g.lr_t = os.lr_t; g.beta1 = os.beta1; g.beta2 = os.beta2; g.eps = os.eps; g.grad_scale = os.grad_scale;
  conv_wgrad_body<BMK, BN, true>(g, lds, r - by * wx, by, bz);
}

// Row table of a convolution geometry for the wgrad kernel: entry m = output pixel (image, oh, ow) holds the byte offset
// of its window origin (image, oh*stride - pad_t, ow*stride - pad_l, channel 0) in x -- negative inside the halo -- and
// the origin's (ih0, iw0) packed into 16 + 16 bits.  Built on the host at the first use of a geometry, cached on the
// context (device memory, freed with it).
const int* get_row_table(radnet_ctx* ctx, const radnet_conv_desc* d) {
  const std::array<int, 11> key{d->nb, d->h, d->w_, d->c, d->oh, d->ow, d->stride, d->pad_t, d->pad_l, d->kh, d->kw};
  auto it = ctx->row_tables->m.find(key);
  if (it != ctx->row_tables->m.end()) return (const int*)it->second;
  const int M = d->nb * d->oh * d->ow, mpad = radnet_cdiv(M, BK) * BK, taps = d->kh * d->kw;
  const int64_t bias = ((int64_t)d->pad_t * d->w_ + d->pad_l) * d->c * 4;
  std::vector<uint32_t> host((size_t)taps * mpad, 0x80000000u);
  for (int kh = 0; kh < d->kh; ++kh)
    for (int kw = 0; kw < d->kw; ++kw) {
      uint32_t* row = host.data() + (size_t)(kh * d->kw + kw) * mpad;
      size_t m = 0;
      for (int img = 0; img < d->nb; ++img)
        for (int oh = 0; oh < d->oh; ++oh)
          for (int ow = 0; ow < d->ow; ++ow, ++m) {
            const int ih = oh * d->stride - d->pad_t + kh, iw = ow * d->stride - d->pad_l + kw;
            if ((unsigned)ih < (unsigned)d->h && (unsigned)iw < (unsigned)d->w_)
              row[m] = (uint32_t)((((int64_t)img * d->h + ih) * d->w_ + iw) * d->c * 4 + bias);
          }
    }
  void* dev = nullptr;
  if (hipMalloc(&dev, host.size() * sizeof(uint32_t)) != hipSuccess) return nullptr;
  if (hipMemcpy(dev, host.data(), host.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
  ctx->row_tables->m.emplace(key, dev);
  return (const int*)dev;
}
}  // namespace

static int run_wgrad(radnet_ctx* ctx, const radnet_conv_desc* d, int batch, long long x_bs, long long dy_bs, long long dw_bs) {
  if (!ctx || !d) return RADNET_ERR_ARG;
  if (!d->x || !d->dy || !d->dw) RADNET_FAIL(ctx, RADNET_ERR_ARG, "conv_wgrad: null tensor");
  WgradArgs g{};
  g.batch = batch; g.x_bstride = x_bs; g.dy_bstride = dy_bs; g.dw_bstride = dw_bs;
  g.x = d->x; g.dy = d->dy; g.gscale = d->gscale; g.dw = d->dw; g.db = nullptr;
  g.H = d->h; g.W = d->w_; g.C = d->c; g.OH = d->oh; g.OW = d->ow; g.KW = d->kw;
  g.stride = d->stride; g.pad_t = d->pad_t; g.pad_l = d->pad_l;
  g.M = d->nb * d->oh * d->ow; g.N = d->n; g.K = d->kh * d->kw * d->c;
  g.ld_dy = d->ld_dy; g.ldw = d->ldw;
  if (g.M >= (1 << 20)) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "conv_wgrad: M=%d exceeds 2^20", g.M);
  if ((g.N & 3) || (g.ld_dy & 3) || (g.ldw & 3)) RADNET_FAIL(ctx, RADNET_ERR_ARG, "conv_wgrad: n, ld_dy, ldw must be multiples of 4");
  if (d->h >= 32768 || d->w_ >= 32768) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "conv_wgrad: input %dx%d exceeds the 16-bit row table", d->h, d->w_);
  g.rowtab = get_row_table(ctx, d);
  if (!g.rowtab) RADNET_FAIL(ctx, RADNET_ERR_HIP, "conv_wgrad: cannot build the row table");
  g.mpad = radnet_cdiv(g.M, BK) * BK;
  g.x_bias = (unsigned)(((int64_t)d->pad_t * d->w_ + d->pad_l) * d->c * 4);
  {
    const uint64_t xb = (uint64_t)d->nb * d->h * d->w_ * d->c * 4ull, db = (uint64_t)g.M * g.ld_dy * 4ull;
    if (xb + g.x_bias >= (1ull << 31) || db >= (1ull << 31)) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "conv_wgrad: tensor larger than 2 GiB");
    g.x_bytes = (unsigned)xb;
    g.dy_bytes = (unsigned)db;
  }
  if (d->c % 64) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "conv_wgrad: channels %d not a multiple of 64", d->c);
  if ((uint64_t)g.K * (uint64_t)g.ldw * 4ull >= (1ull << 31)) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "conv_wgrad: weight tensor larger than 2 GiB");
  const int nmt = radnet_cdiv(g.M, BK);
  uint64_t wgrad_slab_bytes = 0;
  auto launch = [&](int bmk, int bn, int splits) -> int {
    g.xcd_batch = (batch > 1 && splits < 0) ? 1 : 0;      // a batch: -s = the same grid, XCD-contiguous numbering
    if (splits < 0) {
      if (batch <= 1) return RADNET_ERR_UNSUPPORTED;
      splits = -splits;
    }
    wgrad_slab_bytes = 0;
    g.mt_per_split = radnet_cdiv(nmt, splits);
    g.splits = splits;
    // dw_accumulate: 0 = overwrite, 1 = add to existing contents, 2 = destination is pre-zeroed by the caller
    // (plain stores when un-split, atomics without the memset when split)
    g.atomic = (splits > 1 || d->dw_accumulate == 1) ? 1 : 0;
    dim3 grid(radnet_cdiv(g.K, bmk), radnet_cdiv(g.N, bn), splits * (batch > 1 ? batch : 1)), block(NTHREADS);
    g.slabs = nullptr;
    g.counters = nullptr;
    g.tiles_x = (int)grid.x; g.tiles_y = (int)grid.y;
    g.accumulate = d->dw_accumulate == 1;
    if (splits > 1 && ctx->deterministic) {
      // ordered reduction: slabs at the END of the workspace (a dgrad launch paired with this one keeps its split-K slabs at the start)
      const uint64_t tiles = (uint64_t)grid.x * grid.y * (batch > 1 ? batch : 1);
      const uint64_t need = (tiles * splits * (uint64_t)(bmk * bn) + (uint64_t)grid.y * (batch > 1 ? batch : 1) * splits * bn) * sizeof(float);
      if (tiles > kAuxWgradCounterCount || ctx->ws == nullptr || need > ctx->ws_bytes) return RADNET_ERR_UNSUPPORTED;      // candidate skipped
      g.slabs = reinterpret_cast<float*>(reinterpret_cast<char*>(ctx->ws) + ((ctx->ws_bytes - need) & ~(uint64_t)255));
      g.counters = reinterpret_cast<unsigned*>(ctx->aux + kAuxWgradCounters);
      g.atomic = 0;
      wgrad_slab_bytes = need + 256;
    } else if (splits > 1 && d->dw_accumulate == 0) {  // atomics need a zeroed destination
      // a pitched dw (a column block of a wider tensor): only the n columns of each row are this layer's to clear
      if (batch <= 1 && g.ldw != g.N)
        RADNET_CHECK_HIP(ctx, hipMemset2DAsync(d->dw, (size_t)g.ldw * sizeof(float), 0, (size_t)g.N * sizeof(float), (size_t)g.K, ctx->stream));
      else
        RADNET_CHECK_HIP(ctx, hipMemsetAsync(d->dw, 0, (batch > 1 ? (size_t)batch * dw_bs : (size_t)g.K * g.ldw) * sizeof(float), ctx->stream));
    }
    if (ctx->pair_capture != nullptr) {
      PairCapture* pc = (PairCapture*)ctx->pair_capture;
      pc->have_w = true;
      pc->w_ok = bmk == 64 && bn == 64 && batch <= 1;
      pc->gw = g;
      pc->w_slab_bytes = wgrad_slab_bytes;
      pc->w_bmk = bmk; pc->w_bn = bn;
      pc->w_slab_need = wgrad_slab_bytes ? wgrad_slab_bytes - 256 : 0;
      pc->wx = grid.x; pc->wy = grid.y; pc->wz = grid.z;
      pc->flops += 2.0 * g.M * g.N * g.K;
      return RADNET_OK;
    }
    if (bmk == 128 && bn == 128) RADNET_LAUNCH((conv_wgrad_kernel<128, 128>), grid, block, 0, ctx->stream, ctx->arm0, ctx->arm1, g);
    else if (bmk == 128 && bn == 64) RADNET_LAUNCH((conv_wgrad_kernel<128, 64>), grid, block, 0, ctx->stream, ctx->arm0, ctx->arm1, g);
    else if (bmk == 64 && bn == 128) RADNET_LAUNCH((conv_wgrad_kernel<64, 128>), grid, block, 0, ctx->stream, ctx->arm0, ctx->arm1, g);
    else RADNET_LAUNCH((conv_wgrad_kernel<64, 64>), grid, block, 0, ctx->stream, ctx->arm0, ctx->arm1, g);
    RADNET_CHECK_LAUNCH(ctx, "conv_wgrad");
    return RADNET_OK;
  };
  int bmk = (d->c % 128 == 0) ? 128 : 64, bn = g.N > 64 ? 128 : 64, splits = 1;
  const radnet_shape_key key{2 + (d->dw_accumulate == 1 ? 1 : 0) + (batch > 1 ? 16 : 0), g.M, g.N, g.K, g.C, d->kh * d->kw, batch > 1 ? batch : g.stride};
  auto it = ctx->tuned->find(key);
  if (ctx->force_a > 0) {
    bmk = ctx->force_a; bn = ctx->force_b; splits = ctx->force_splits < 1 ? 1 : ctx->force_splits;
    if (bmk < 64) bmk = 64;      // the 32-row tiles are the forward / data-gradient kernel's: a forced 32x64 leaves the weight gradient at 64x64
    if (bn < 64) bn = 64;        // (radnet_conv_bwd then pairs a 32x64 data gradient with a 64x64 weight gradient)
    if (d->c % bmk) RADNET_FAIL(ctx, RADNET_ERR_ARG, "conv_wgrad: forced k tile %d does not divide c=%d", bmk, d->c);
  } else if (it != ctx->tuned->end()) {
    bmk = it->second.a; bn = it->second.b; splits = it->second.splits;
  } else if (const radnet_tuned* nb = (ctx->autotune == 2 && d->dw_accumulate != 1) ? radnet_tuned_neighbour(*ctx->tuned, key) : nullptr;
             nb && (nb->splits <= 1 || (nmt / nb->splits >= 2 && radnet_cdiv(nmt, radnet_cdiv(nmt, nb->splits)) == nb->splits))) {
    bmk = nb->a; bn = nb->b; splits = nb->splits;
    (*ctx->tuned)[key] = *nb;
  } else if (ctx->autotune && d->dw_accumulate != 1) {
    PairPause pause(ctx);                       // trial launches are real launches
    struct WCand { float ms; int bmk, bn, s; };
    std::vector<WCand> seen;
    const bool for_pair = pause.saved != nullptr && batch <= 1 && d->dx != nullptr;      // see run_igemm
    for (int cb = 128; cb >= 64; cb -= 64) {
      if (d->c % cb) continue;
      if (for_pair && cb != 64) continue;
      for (int cn = 128; cn >= 64; cn -= 64) {
        if (cn > 64 && g.N <= 64) continue;
        if (for_pair && cn != 64) continue;
        for (int s0 : {1, 2, 3, 4, 6, 8, 12, 16}) {
          if (s0 > 1 && (nmt / s0 < 2 || radnet_cdiv(nmt, radnet_cdiv(nmt, s0)) != s0)) continue;
          for (int s = s0; s >= (batch > 1 ? -s0 : s0); s -= 2 * s0) {      // a batch: also -s, the XCD-contiguous numbering
            float ms = 0.f;
            int rc = radnet_time_launches(ctx, [&]() { return launch(cb, cn, s); }, 3, &ms);
            if (rc == RADNET_ERR_UNSUPPORTED) continue;      // ordered reduction: slabs larger than the workspace
            if (rc != RADNET_OK) return rc;
            seen.push_back(WCand{ms, cb, cn, s});
          }
        }
      }
    }
    std::sort(seen.begin(), seen.end(), [](const WCand& a, const WCand& b) { return a.ms < b.ms; });
    float best = 1e30f;
    for (size_t i = 0; i < seen.size() && i < 4; ++i) {        // finalists again, longer and twice (see run_igemm)
      float ms = 0.f;
      const int rc = radnet_time_launches_twice(ctx, [&]() { return launch(seen[i].bmk, seen[i].bn, seen[i].s); }, 12, &ms);
      if (rc != RADNET_OK) return rc;
      if (ms < best) { best = ms; bmk = seen[i].bmk; bn = seen[i].bn; splits = seen[i].s; }
    }
    (*ctx->tuned)[key] = radnet_tuned{bmk, bn, splits, best, 4};
    if (getenv("RADNET_TUNE_LOG"))
      fprintf(stderr, "radnet tune: wgrad M=%d N=%d K=%d C=%d -> tile %dx%d slices %d : %.1f us (%.1f TFLOP/s)\n", g.M, g.N, g.K, g.C,
              bmk, bn, splits, best * 1e3, 2.0 * g.M * g.N * g.K / (best * 1e9));
    if (d->dw_accumulate == 2)               // the trial launches added into the pre-zeroed buffer: restore it
      RADNET_CHECK_HIP(ctx, hipMemset2DAsync(d->dw, (size_t)g.ldw * sizeof(float), 0, (size_t)g.N * sizeof(float), (size_t)g.K, ctx->stream));
  } else {
    // accumulate mode reuses the overwrite-mode measurement when there is one
    const radnet_shape_key k0{2, g.M, g.N, g.K, g.C, d->kh * d->kw, g.stride};
    auto it0 = ctx->tuned->find(k0);
    if (it0 != ctx->tuned->end()) {
      bmk = it0->second.a; bn = it0->second.b; splits = it0->second.splits;
    } else {
      long long tiles = (long long)radnet_cdiv(g.K, bmk) * radnet_cdiv(g.N, bn);
      if (tiles < kNumCU && bmk == 128 && bn == 128) {
        bn = 64;
        tiles = (long long)radnet_cdiv(g.K, bmk) * radnet_cdiv(g.N, bn);
      }
      while (tiles * splits < 2 * kNumCU && nmt / (splits * 2) >= 4 && splits < 16) splits *= 2;
    }
  }
  radnet_timing_arm(ctx);
  {
    // bias gradient in the same launch (the measurement launches above ran without it); atomics need zeros to add to
    g.db = d->db;
    if (d->db && d->dw_accumulate == 0) RADNET_CHECK_HIP(ctx, hipMemsetAsync(d->db, 0, (size_t)g.N * sizeof(float), ctx->stream));
    int rc = launch(bmk, bn, splits);
    if (rc == RADNET_ERR_UNSUPPORTED && splits < 0) {      // a loaded / shared choice this launch cannot use as it is
      splits = -splits;
      rc = launch(bmk, bn, splits);
    }
    if (rc == RADNET_ERR_UNSUPPORTED && splits > 1) {      // a forced / shared / loaded choice whose slabs exceed THIS context's workspace
      while (rc == RADNET_ERR_UNSUPPORTED && splits > 1) {
        splits = splits > 2 ? splits / 2 : 1;
        while (splits > 1 && radnet_cdiv(nmt, radnet_cdiv(nmt, splits)) != splits) --splits;      // no empty split
        rc = launch(bmk, bn, splits);
      }
    }
    if (rc == RADNET_ERR_UNSUPPORTED) RADNET_FAIL(ctx, rc, "conv_wgrad: no launch shape fits (tile %dx%d, workspace %llu bytes)", bmk, bn, (unsigned long long)ctx->ws_bytes);
    if (rc != RADNET_OK) return rc;
  }
  RADNET_CHECK_LAUNCH(ctx, "conv_wgrad");
  radnet_timing_end_armed(ctx, 2, 2.0 * g.M * g.N * g.K * (batch > 1 ? batch : 1));
  return RADNET_OK;
}

extern "C" int radnet_conv_wgrad(radnet_ctx* ctx, const radnet_conv_desc* d) { return run_wgrad(ctx, d, 1, 0, 0, 0); }

// Weight gradient and data gradient of one layer (the same descriptor: both read dy) as ONE launch when both problems run as
// 64x64-tile, 4-wave workgroups (conv_bwd_pair_kernel); otherwise -- other tile choices, or RADNET_NO_BWD_PAIR=1 -- the two
// launches in the order wgrad, dgrad.  Results are those of the separate launches (same kernels' code, same launch shapes).
extern "C" int radnet_conv_bwd(radnet_ctx* ctx, const radnet_conv_desc* d) {
  if (!ctx || !d) return RADNET_ERR_ARG;
  static const bool disabled = radnet_env_flag("RADNET_NO_BWD_PAIR");
  if (disabled || ctx->pair_capture != nullptr || !d->dx) {
    int rc = radnet_conv_wgrad(ctx, d);
    return rc != RADNET_OK || !d->dx ? rc : radnet_conv_dgrad(ctx, d);
  }
  PairCapture pc;
  const int timed = ctx->timing;
  ctx->timing = 0;
  ctx->pair_capture = &pc;
  int rc = radnet_conv_wgrad(ctx, d);           // host-side preparation (tables, memsets of overwrite mode) happens here
  if (rc == RADNET_OK) rc = radnet_conv_dgrad(ctx, d);
  ctx->pair_capture = nullptr;
  ctx->timing = timed;
  if (rc != RADNET_OK) return rc;
  if (pc.a_slab_bytes + pc.w_slab_bytes > ctx->ws_bytes) pc.a_ok = false;      // the two problems' slabs would overlap in the workspace
  if (!(pc.have_a && pc.have_w && pc.a_ok && pc.w_ok)) {      // not the fusable shapes: issue them one after the other
    rc = radnet_conv_wgrad(ctx, d);
    return rc != RADNET_OK ? rc : radnet_conv_dgrad(ctx, d);
  }
  PairMap pm{pc.ax * pc.ay, pc.wx * pc.wy * pc.wz, pc.ax, pc.ay, pc.wx, pc.wy};
  radnet_timing_arm(ctx);
  if (pc.a_bm == 32) RADNET_LAUNCH(conv_bwd_pair_kernel<32>, dim3(pm.n_a + pm.n_w), dim3(NTHREADS), 0, ctx->stream, ctx->arm0, ctx->arm1, pc.ga, pc.gw, pm);
  else RADNET_LAUNCH(conv_bwd_pair_kernel<64>, dim3(pm.n_a + pm.n_w), dim3(NTHREADS), 0, ctx->stream, ctx->arm0, ctx->arm1, pc.ga, pc.gw, pm);
  RADNET_CHECK_LAUNCH(ctx, "conv_bwd_pair");
  radnet_timing_end_armed(ctx, 4, pc.flops);
  return RADNET_OK;
}

radnet_ctx::MultiTables::~MultiTables() {
  for (auto& e : v)
    if (e.second) (void)hipFree(e.second);
}

namespace {
// The device copy of a problem table: the one made for the same bytes before, or a new allocation (a table is never rewritten).
const WgradArgs* get_multi_table(radnet_ctx* ctx, const WgradArgs* host, int n) {
  const size_t bytes = sizeof(WgradArgs) * (size_t)n;
  auto& v = ctx->multi_tables.v;
  for (auto& e : v)
    if (e.first.size() == bytes && memcmp(e.first.data(), host, bytes) == 0) return (const WgradArgs*)e.second;
  if (v.size() >= 256) {                     // hipFree waits for the device: no launch reads the table any more
    (void)hipFree(v.front().second);
    v.erase(v.begin());
  }
  void* dev = nullptr;
  if (hipMalloc(&dev, bytes) != hipSuccess) return nullptr;
  if (hipMemcpy(dev, host, bytes, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(dev);
    return nullptr;
  }
  v.emplace_back(std::vector<char>((const char*)host, (const char*)host + bytes), dev);
  return (const WgradArgs*)dev;
}
}  // namespace

// The weight gradients (and bias gradients) of n layers in as few launches as their tile shapes allow: every problem keeps the tile
// shape, the slice count and the slice order of its own radnet_conv_wgrad call -- that call's launch policy chooses them, tuning
// table, forced configuration and autotuner included -- so dw and db hold the bits of the n single calls.  With an optimizer block
// the writer of each tile's final value applies the Adam step to the weights behind that tile instead of storing the gradient.
extern "C" int radnet_conv_wgrad_multi(radnet_ctx* ctx, const radnet_conv_desc* descs, int32_t n, const radnet_wgrad_adam* opt) {
  if (!ctx || n < 0 || (n > 0 && !descs)) return RADNET_ERR_ARG;
  if (n == 0) return RADNET_OK;
  if (ctx->pair_capture != nullptr) RADNET_FAIL(ctx, RADNET_ERR_ARG, "conv_wgrad_multi: called inside radnet_conv_bwd");
  const bool adam = opt != nullptr && opt->p != nullptr;
  if (adam) {
    if (!opt->g || !opt->m || !opt->v || opt->n <= 0) RADNET_FAIL(ctx, RADNET_ERR_ARG, "conv_wgrad_multi: optimizer block with a null arena");
    if (opt->t < 1) RADNET_FAIL(ctx, RADNET_ERR_ARG, "conv_wgrad_multi: step counter starts at 1");
  }
  std::vector<PairCapture> pcs((size_t)n);
  std::vector<WgradMultiItem> items((size_t)n);
  const int timed = ctx->timing;
  for (int i = 0; i < n; ++i) {
    radnet_conv_desc d = descs[i];
    d.dx = nullptr;                            // a weight gradient of its own: the autotuner does not narrow its candidates for a pairing
    if (adam) {
      if (d.dw_accumulate == 1) RADNET_FAIL(ctx, RADNET_ERR_ARG, "conv_wgrad_multi: problem %d adds to its gradient; the optimizer epilogue needs the whole gradient", i);
      const int64_t off = d.dw - opt->g, last = (int64_t)(d.kh * d.kw * d.c - 1) * d.ldw + d.n;
      if (!d.dw || d.dw < opt->g || off + last > opt->n) RADNET_FAIL(ctx, RADNET_ERR_ARG, "conv_wgrad_multi: problem %d's dw lies outside the gradient arena", i);
    }
    ctx->timing = 0;
    ctx->pair_capture = &pcs[i];
    const int rc = radnet_conv_wgrad(ctx, &d);      // host-side preparation (row table, memsets of overwrite mode, autotuning) happens here
    ctx->pair_capture = nullptr;
    ctx->timing = timed;
    if (rc != RADNET_OK) return rc;
    PairCapture& pc = pcs[i];
    if (!pc.have_w) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "conv_wgrad_multi: problem %d produced no launch", i);
    const bool ordered = pc.gw.slabs != nullptr;
    if (adam && !ordered && pc.gw.atomic)
      RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "conv_wgrad_multi: problem %d adds its slices with atomics (no final writer); the optimizer epilogue needs ordered reductions", i);
    items[i] = WgradMultiItem{pc.w_bmk, pc.w_bn, pc.wx, pc.wy, pc.wz, ordered ? pc.w_slab_need : 0, ordered ? pc.wx * pc.wy : 0u};
  }
  std::vector<WgradMultiLaunch> plan((size_t)n);
  const int nl = wgrad_multi_plan(items.data(), n, ctx->ws_bytes, (unsigned)kAuxWgradCounterCount, plan.data(), n);
  if (nl < 0) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "conv_wgrad_multi: the problems do not fit a launch plan (%d)", nl);
  WgradOptScalars os{};
  if (adam) os = WgradOptScalars{radnet_adam_lr_t(opt->lr, opt->beta1, opt->beta2, opt->t), opt->beta1, opt->beta2, opt->eps, opt->grad_scale};
  for (int l = 0; l < nl; ++l) {
    const WgradMultiLaunch& L = plan[l];
    WgradArgs host[kWgradMultiMax];
    memset(host, 0, sizeof(host));
    double flops = 0.0;
    for (int k = 0; k < L.n; ++k) {
      const PairCapture& pc = pcs[L.problem[k]];
      WgradArgs& g = host[k];
      memcpy(&g, &pc.gw, sizeof(g));
      if (g.slabs != nullptr) {
        g.slabs = reinterpret_cast<float*>(reinterpret_cast<char*>(ctx->ws) + L.slab_off[k]);
        g.counters = reinterpret_cast<unsigned*>(ctx->aux + kAuxWgradCounters) + L.counter_off[k];
      }
      g.ow = g.om = g.ov = nullptr;
      g.lr_t = g.beta1 = g.beta2 = g.eps = g.grad_scale = 0.f;      // they arrive as kernel arguments
      g.pad_opt = 0;
      if (adam) {
        const int64_t off = g.dw - opt->g;
        g.ow = opt->p + off; g.om = opt->m + off; g.ov = opt->v + off;
      }
      flops += 2.0 * g.M * g.N * g.K;
    }
    const WgradArgs* tab = get_multi_table(ctx, host, L.n);
    if (!tab) RADNET_FAIL(ctx, RADNET_ERR_HIP, "conv_wgrad_multi: cannot place the problem table on the device");
    const dim3 grid(L.map.first[L.n]), block(NTHREADS);
    radnet_timing_arm(ctx);
    if (L.bmk == 128 && L.bn == 128) RADNET_LAUNCH((conv_wgrad_multi_kernel<128, 128>), grid, block, 0, ctx->stream, ctx->arm0, ctx->arm1, tab, L.map, os);
    else if (L.bmk == 128 && L.bn == 64) RADNET_LAUNCH((conv_wgrad_multi_kernel<128, 64>), grid, block, 0, ctx->stream, ctx->arm0, ctx->arm1, tab, L.map, os);
    else if (L.bmk == 64 && L.bn == 128) RADNET_LAUNCH((conv_wgrad_multi_kernel<64, 128>), grid, block, 0, ctx->stream, ctx->arm0, ctx->arm1, tab, L.map, os);
    else RADNET_LAUNCH((conv_wgrad_multi_kernel<64, 64>), grid, block, 0, ctx->stream, ctx->arm0, ctx->arm1, tab, L.map, os);
    RADNET_CHECK_LAUNCH(ctx, "conv_wgrad_multi");
    radnet_timing_end_armed(ctx, 2, flops);
  }
  return RADNET_OK;
}

extern "C" int radnet_wgrad_batched(radnet_ctx* ctx, const float* a, const float* dy, float* dw, int32_t batch, int32_t m, int32_t k, int32_t n,
                                    int32_t accumulate) {
  if (!ctx || !a || !dy || !dw) return RADNET_ERR_ARG;
  if (batch < 1 || batch > 4096) RADNET_FAIL(ctx, RADNET_ERR_ARG, "wgrad_batched: batch %d", batch);
  radnet_conv_desc d{};
  d.x = a; d.dy = dy; d.dw = dw;
  d.nb = 1; d.h = 1; d.w_ = m; d.c = k; d.oh = 1; d.ow = m;      // a 1x1 convolution over m 'pixels' of k channels
  d.kh = 1; d.kw = 1; d.stride = 1; d.pad_t = 0; d.pad_l = 0; d.n = n;
  d.ldw = n; d.ld_dy = n;
  d.dw_accumulate = accumulate;
  return run_wgrad(ctx, &d, batch, (long long)m * k, (long long)m * n, (long long)k * n);
}
