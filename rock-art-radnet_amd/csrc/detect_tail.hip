// The detection tail of one predict tile on the device: classifier outputs -> detections in source-image pixels
// (RADNet.py:104-154 apply_spatial_pyramid_pooling's decode loop + rpn.py:346-378 apply_regr, RADNet.py:562-575 the per-class
// NMS 0.2, RADNet.py:44-51 get_real_coordinates).  Compiled with -ffp-contract=off: Python and NumPy round every product and
// sum separately, so no FMA contraction is allowed here.
//
//   rois_chunks_kernel   (x1,y1,x2,y2) int64 proposals + device count -> fp32 (x,y,w,h) RoIs for ceil(n/k)*k rows, the padding
//                        rows of a chunk repeating THAT chunk's first row (RADNet.py:110-122).
//   detect_tail_kernel   ONE workgroup of 1024 threads, the whole problem in LDS (<= 1024 rows, <= 32 classes: latency, not
//                        bandwidth):
//                          (1) a thread per row: first maximum, threshold / background test, delta decode in fp64, box in LDS,
//                              a 64-bit key  (class + 1) << 42 | raw order-preserving score bits << 10 | row;
//                          (2) descending bitonic sort of the keys (nms_device.h): every class becomes one run, inside it "stable
//                              ascending, walk from the end" (among equal scores the higher row first) -- nms_kernel's order;
//                          (3) a wave per class walks its run: the liveness of candidate j lives in bit j/64 of lane j%64, a pick
//                              tests the rest of the run 64 candidates at a time with nms_device.h's suppression test;
//                          (4) classes in order of their first surviving row (the insertion order of the Python dicts), picks in
//                              pick order, float floor division by the resize ratio, one compact record array.
//                        No floating-point atomics, plain vector stores, no scratch memory outside LDS.
#include "radnet_internal.h"
#include "nms_device.h"

namespace {

constexpr int kMaxRows = 1024;      // rows of one launch (= threads of the workgroup, bits of the row field in a key)
constexpr int kMaxClasses = 32;
constexpr int kHeader = RADNET_DETECT_HEADER_WORDS;      // int32 words in front of the records: [0] count (-1: malformed box), [1] rows considered
constexpr int kRecord = RADNET_DETECT_RECORD_WORDS;      // int32 words per record: class, x1, y1, x2, y2, prob (fp32 bits)

__global__ void __launch_bounds__(256) rois_chunks_kernel(const long long* __restrict__ R, const int* __restrict__ n_dev, int max_n, int k,
                                                          int rows, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows) return;
  int n = *n_dev;
  n = n < 0 ? 0 : (n > max_n ? max_n : n);
  // i < n: the proposal itself; n <= i < ceil(n/k)*k: padding of the last chunk = that chunk's first row ((i/k)*k < n there);
  // rows past the last chunk are not looked at by the tail: row 0, so that the head computes on a valid RoI
  const int j = i < n ? i : ((i / k) * k < n ? (i / k) * k : 0);
  const long long x1 = R[4 * j], y1 = R[4 * j + 1], x2 = R[4 * j + 2], y2 = R[4 * j + 3];
  out[4 * i] = (float)x1;
  out[4 * i + 1] = (float)y1;
  out[4 * i + 2] = (float)(x2 - x1);
  out[4 * i + 3] = (float)(y2 - y1);
}

// NumPy's / Python's float floor division (npy_divmod: fmod-based, NOT floor(a / b)); b != 0
__device__ __forceinline__ double floor_divide(double a, double b) {
  double mod = fmod(a, b);
  double div = (a - mod) / b;
  if (mod != 0.0 && ((b < 0.0) != (mod < 0.0))) div -= 1.0;
  if (div != 0.0) {
    double fl = floor(div);
    if (div - fl > 0.5) fl += 1.0;
    return fl;
  }
  return copysign(0.0, a / b);
}

__device__ __forceinline__ int to_i32(double v) {      // int(round(v)); beyond int32 the host path has no defined value: saturate
  const double r = rint(v);
  if (!(r > -2147483648.0)) return INT32_MIN;
  if (!(r < 2147483647.0)) return INT32_MAX;
  return (int)r;
}

struct TailArgs {
  const float* p_cls;
  const float* p_regr;
  const float* rois;
  const int* n_dev;
  int rows, nc, k, bg;
  float thr;
  float std0, std1, std2, std3;
  double stride, nms_thr, ratio;
  int max_boxes;
  int* out;
};

__global__ void __launch_bounds__(1024) detect_tail_kernel(TailArgs g) {
  __shared__ double4 s_box[kMaxRows];                    // by row: x1, y1, x2, y2 in resized-image pixels
  __shared__ unsigned long long s_key[kMaxRows];
  __shared__ int s_cnt[kMaxClasses], s_first[kMaxClasses], s_start[kMaxClasses], s_npick[kMaxClasses], s_obase[kMaxClasses];
  __shared__ int s_malformed;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int n = *g.n_dev;
  n = n < 0 ? 0 : n;
  long long m64 = ((long long)n + g.k - 1) / g.k * g.k;  // RADNet.py:110-122: whole chunks of k rows, padding rows included
  const int m = (int)(m64 < (long long)g.rows ? m64 : (long long)g.rows);
  int P = 64;
  while (P < m) P <<= 1;                                 // <= 1024

  if (tid < kMaxClasses) {
    s_cnt[tid] = 0;
    s_first[tid] = kMaxRows;
    s_npick[tid] = 0;
  }
  if (tid == 0) s_malformed = 0;
  __syncthreads();

  // ---- (1) a thread per row -----------------------------------------------------------------------------------------------
  unsigned long long key = 0ull;
  if (tid < m) {
    const float* pc = g.p_cls + (size_t)tid * g.nc;
    // np.argmax / np.max: the FIRST maximum; a NaN wins (first NaN) and is not below the threshold
    int best = 0;
    float smax = pc[0];
    for (int c = 1; c < g.nc; ++c) {
      const float v = pc[c];
      if (!(smax != smax) && (v > smax || v != v)) { smax = v; best = c; }
    }
    if (!(smax < g.thr) && best != g.bg) {
      const double x = (double)g.rois[4 * tid], y = (double)g.rois[4 * tid + 1];
      const double w = (double)g.rois[4 * tid + 2], h = (double)g.rois[4 * tid + 3];
      const float* pr = g.p_regr + (size_t)tid * 4 * (g.nc - 1) + 4 * best;
      // np.float32 / Python float: an fp32 division; everything after it is fp64 (np.float32 * np.int64, math.exp)
      const float tx = pr[0] / g.std0, ty = pr[1] / g.std1, tw = pr[2] / g.std2, th = pr[3] / g.std3;
      const double cx1 = (double)tx * w + (x + w / 2.), cy1 = (double)ty * h + (y + h / 2.);
      const double ew = exp((double)tw), eh = exp((double)th);
      const double w1 = ew * w, h1 = eh * h;
      const double px = cx1 - w1 / 2., py = cy1 - h1 / 2.;
      // math.exp overflows (OverflowError) for a finite argument; round() raises on a NaN (ValueError) or an infinity
      // (OverflowError): rpn.py:376-378 then hands the box back undecoded
      const bool overflow = (isinf(ew) && !isinf((double)tw)) || (isinf(eh) && !isinf((double)th));
      const bool finite = isfinite(px) && isfinite(py) && isfinite(w1) && isfinite(h1);
      double bx = x, by = y, bw = w, bh = h;
      if (!overflow && finite) { bx = rint(px); by = rint(py); bw = rint(w1); bh = rint(h1); }
      const double4 b = make_double4(g.stride * bx, g.stride * by, g.stride * (bx + bw), g.stride * (by + bh));
      s_box[tid] = b;
      if (!(b.x < b.z) || !(b.y < b.w)) s_malformed = 1;              // rpn.py:400-401 asserts (every writer stores 1)
      key = ((unsigned long long)(best + 1) << 42) | ((unsigned long long)sortable_bits(smax) << 10) | (unsigned long long)tid;
      atomicAdd(&s_cnt[best], 1);
      atomicMin(&s_first[best], tid);
    }
  }
  if (tid < P) s_key[tid] = key;
  __syncthreads();
  if (s_malformed) {
    if (tid == 0) { g.out[0] = -1; g.out[1] = m; }
    return;
  }

  // ---- (2) descending bitonic sort of P keys --------------------------------------------------------------------------------
  __builtin_assume(P <= kMaxRows);                       // one trip of the sort's strided loop: the compiler then emits none
  bitonic_sort<true>(s_key, P);
  // runs of the classes in the sorted array: the highest class index first
  if (tid == 0) {
    int at = 0;
    for (int c = g.nc - 1; c >= 0; --c) { s_start[c] = at; at += s_cnt[c]; }
  }
  __syncthreads();

  // ---- (3) greedy NMS, a wave per class ---------------------------------------------------------------------------------------
  // candidate j of the run: lane j % 64, bit j / 64 of `dead` / `picked` (<= 16 bits)
  unsigned int picked_of[2] = {0u, 0u};                  // this wave's classes: wave, wave + 16
  for (int q = 0; q < 2; ++q) {
    const int c = wave + 16 * q;
    if (c >= g.nc) break;
    const int cnt = s_cnt[c], start = s_start[c];
    unsigned int dead = 0u, picked = 0u;
    int np = 0;
    for (int i = 0; i < cnt && np < g.max_boxes; ++i) {
      const unsigned int owner = (unsigned int)__shfl((int)dead, i & 63, 64);
      if ((owner >> (i >> 6)) & 1u) continue;             // uniform over the wave
      if (lane == (i & 63)) picked |= 1u << (i >> 6);
      ++np;
      const double4 pk = s_box[(int)(s_key[start + i] & 1023ull)];
      const double pk_area = (pk.z - pk.x) * (pk.w - pk.y);
      for (int j0 = (i + 1) & ~63; j0 < cnt; j0 += 64) {
        const int j = j0 + lane;
        if (j > i && j < cnt && !((dead >> (j >> 6)) & 1u)) {
          const double4 cb = s_box[(int)(s_key[start + j] & 1023ull)];
          if (suppresses(pk, pk_area, cb, (cb.z - cb.x) * (cb.w - cb.y), g.nms_thr)) dead |= 1u << (j >> 6);
        }
      }
    }
    picked_of[q] = picked;
    if (lane == 0) s_npick[c] = np;
  }
  __syncthreads();

  // ---- (4) classes in order of their first surviving row; records ------------------------------------------------------------
  if (tid == 0) {
    int total = 0;
    unsigned int done = 0u;
    for (int r = 0; r < g.nc; ++r) {                      // selection by first row (distinct for distinct classes)
      int bc = -1, bf = kMaxRows;
      for (int c = 0; c < g.nc; ++c)
        if (!((done >> c) & 1u) && s_cnt[c] > 0 && s_first[c] < bf) { bf = s_first[c]; bc = c; }
      if (bc < 0) break;
      done |= 1u << bc;
      s_obase[bc] = total;
      total += s_npick[bc];
    }
    g.out[0] = total;
    g.out[1] = m;
  }
  __syncthreads();
  for (int q = 0; q < 2; ++q) {
    const int c = wave + 16 * q;
    if (c >= g.nc) break;
    const int cnt = s_cnt[c], start = s_start[c];
    if (cnt == 0) continue;
    int at = s_obase[c];
    const unsigned int picked = picked_of[q];
    for (int s = 0; s * 64 < cnt; ++s) {
      const bool mine = (picked >> s) & 1u;
      const unsigned long long mask = __ballot(mine);
      if (mine) {
        const unsigned long long kq = s_key[start + s * 64 + lane];
        const int row = (int)(kq & 1023ull);
        const double4 b = s_box[row];
        int* o = g.out + kHeader + (size_t)kRecord * (at + __popcll(mask & ((1ull << lane) - 1ull)));
        o[0] = c;
        // boxes[pick].astype('int') of integer-valued boxes, then int(round(v // ratio)) (RADNet.py:44-51)
        o[1] = to_i32(floor_divide(b.x, g.ratio));
        o[2] = to_i32(floor_divide(b.y, g.ratio));
        o[3] = to_i32(floor_divide(b.z, g.ratio));
        o[4] = to_i32(floor_divide(b.w, g.ratio));
        o[5] = (int)__float_as_uint(g.p_cls[(size_t)row * g.nc + c]);
      }
      at += __popcll(mask);
    }
  }
}

int check_desc(radnet_ctx* ctx, const radnet_detect_tail_desc* d) {
  if (!d->p_cls || !d->p_regr || !d->rois || !d->n || !d->out) RADNET_FAIL(ctx, RADNET_ERR_ARG, "detect_tail: null pointer in the descriptor");
  if (d->rows < 1 || d->rows > kMaxRows) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "detect_tail: %d rows (1..%d)", d->rows, kMaxRows);
  if (d->nc < 2 || d->nc > kMaxClasses) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "detect_tail: %d classes (2..%d)", d->nc, kMaxClasses);
  if (d->k < 1) RADNET_FAIL(ctx, RADNET_ERR_ARG, "detect_tail: chunk size k = %d", d->k);
  if (d->max_boxes < 1) RADNET_FAIL(ctx, RADNET_ERR_ARG, "detect_tail: max_boxes = %d", d->max_boxes);
  if (!(d->ratio > 0.0) || !(d->ratio < 1e300)) RADNET_FAIL(ctx, RADNET_ERR_ARG, "detect_tail: resize ratio %g", d->ratio);
  for (int q = 0; q < 4; ++q)
    if (d->regr_std[q] == 0.f) RADNET_FAIL(ctx, RADNET_ERR_ARG, "detect_tail: classifier_regr_std[%d] is 0", q);
  return RADNET_OK;
}

}  // namespace

extern "C" uint64_t radnet_detect_tail_out_bytes(int32_t rows) {
  return rows < 0 ? 0 : (uint64_t)4 * (kHeader + (uint64_t)kRecord * rows);
}

extern "C" int radnet_rois_from_proposals(radnet_ctx* ctx, const int64_t* R, const int32_t* n_dev, int32_t max_n, int32_t k, int32_t rows,
                                          float* rois) {
  if (!ctx) return RADNET_ERR_ARG;
  if (!R || !n_dev || !rois) RADNET_FAIL(ctx, RADNET_ERR_ARG, "rois_from_proposals: null pointer");
  if (max_n < 1 || k < 1 || rows < 1) RADNET_FAIL(ctx, RADNET_ERR_ARG, "rois_from_proposals: max_n %d, k %d, rows %d", max_n, k, rows);
  hipLaunchKernelGGL(rois_chunks_kernel, dim3(radnet_cdiv(rows, 256)), dim3(256), 0, ctx->stream, (const long long*)R, n_dev, max_n, k, rows, rois);
  RADNET_CHECK_LAUNCH(ctx, "rois_chunks");
  return RADNET_OK;
}

extern "C" int radnet_detect_tail(radnet_ctx* ctx, const radnet_detect_tail_desc* d) {
  if (!ctx || !d) return RADNET_ERR_ARG;
  int rc = check_desc(ctx, d);
  if (rc != RADNET_OK) return rc;
  TailArgs g;
  g.p_cls = d->p_cls; g.p_regr = d->p_regr; g.rois = d->rois; g.n_dev = d->n;
  g.rows = d->rows; g.nc = d->nc; g.k = d->k; g.bg = d->bg;
  g.thr = d->bbox_threshold;
  g.std0 = d->regr_std[0]; g.std1 = d->regr_std[1]; g.std2 = d->regr_std[2]; g.std3 = d->regr_std[3];
  g.stride = d->rpn_stride; g.nms_thr = d->nms_thresh; g.ratio = d->ratio;
  g.max_boxes = d->max_boxes;
  g.out = (int*)d->out;
  hipLaunchKernelGGL(detect_tail_kernel, dim3(1), dim3(1024), 0, ctx->stream, g);
  RADNET_CHECK_LAUNCH(ctx, "detect_tail");
  return RADNET_OK;
}

extern "C" int radnet_predict_tile_detect(radnet_ctx* ctx, const radnet_tile_desc* t, const radnet_detect_tail_desc* d) {
  if (!ctx || !t || !d) return RADNET_ERR_ARG;
  if (!t->head) RADNET_FAIL(ctx, RADNET_ERR_ARG, "predict_tile_detect: the tile descriptor has no head");
  const radnet_head_desc& h = *t->head;
  int rc = check_desc(ctx, d);
  if (rc != RADNET_OK) return rc;
  if (d->rows != h.n_rois || d->nc != h.nc || d->p_cls != h.p_cls || d->p_regr != h.p_regr || d->rois != h.rois || d->n != t->Rn)
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "predict_tile_detect: the tail descriptor must name the head's rois / p_cls / p_regr, its row and class "
                                     "counts, and the tile's proposal count");
  if ((int64_t)(t->max_boxes + d->k - 1) / d->k * d->k > h.n_rois)
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "predict_tile_detect: a head of %d rows cannot hold ceil(%d / %d) chunks", h.n_rois, t->max_boxes, d->k);
  radnet_tile_desc front = *t;                            // preprocess .. proposals
  front.head = nullptr;
  rc = radnet_predict_tile(ctx, &front);
  if (rc == RADNET_OK) rc = radnet_rois_from_proposals(ctx, t->R, t->Rn, t->max_boxes, d->k, h.n_rois, const_cast<float*>(h.rois));
  // classifier_layer (resnet50.py:231-281), as radnet_predict_tile runs it
  if (rc == RADNET_OK) rc = radnet_roi_resize_fwd(ctx, h.fmap, h.fh, h.fw, h.fc, h.rois, h.n_rois, h.pool, h.pooled);
  if (rc == RADNET_OK) rc = radnet_program_run(ctx, h.fwd_ops, h.n_fwd);
  if (rc == RADNET_OK)
    rc = radnet_head_tail_fwd(ctx, h.y5, h.n_rois, h.hw, h.feat_c, h.dense_w, h.dense_ld, h.dense_b, h.nc, h.nreg, h.feat, h.p_cls, h.p_regr, nullptr,
                              nullptr, nullptr, nullptr, 1, nullptr, h.tail_scratch);
  if (rc == RADNET_OK) rc = radnet_detect_tail(ctx, d);
  return rc;
}
