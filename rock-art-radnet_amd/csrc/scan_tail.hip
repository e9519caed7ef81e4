// The merge of a scan's tile detections on the device: what RADNet.predict does behind its tile passes (RADNet.py:577-718) --
// the tiles' offsets, RADNet.final_nms (RADNet.py:156-240) per image and class, the NMS 0.4 across the images per class -- bit for
// bit what the host code gives on the same records.  Compiled with -ffp-contract=off: NumPy rounds every product and sum
// separately.  Contract: include/radnet_hip.h.
//
//   final_nms_kernel     a workgroup of 1024 threads per group.  (1) keys  prob bits with signed zeros tied << 32 | row, ascending
//                        bitonic sort (in LDS up to 2048 keys, in the workspace above): "stable ascending, walked from the end";
//                        (2) the clusters by nms_device.h's walk from the top: a round per cluster marks its members with the
//                        cluster's number;  (3) a second sort by (cluster, position) lays every cluster's members side by side
//                        in order position, which is ascending prob: the chosen boxes are a SUFFIX of that run -- the last
//                        n_obj_avg, or those above the threshold;  (4) a thread per cluster: int64 coordinate sums, NumPy's
//                        pairwise fp32 sum, the two means.
//   scan_count / scan_plan / scan_fill   the gather: per tile the records of every class counted, per (image, class) group the
//                        tiles' places inside it and the groups' offsets (prefix sums), then every record copied to its place
//                        with the tile's offset added.
//   class_nms_kernel     a workgroup per class: the clusters of its images in image order, sorted as above (raw prob bits), greedy
//                        NMS from the end: the same walk, a pick per round, with nms_device.h's suppression test.
//   scan_write_kernel    the status, the classes in order of first appearance, the records.
// All per-box state lives in the workspace; LDS holds one sort of up to 2048 keys and a few words.  No floating-point atomics.
#include "radnet_internal.h"
#include "nms_device.h"

namespace {

typedef unsigned long long u64;

constexpr int kThreads = kNmsThreads;
constexpr int kLdsKeys = 2048;      // keys sorted in LDS (16 KB); larger sorts run in the workspace
constexpr int kHeader = RADNET_DETECT_HEADER_WORDS;      // radnet_detect_tail's output: int32 words in front of the records ...
constexpr int kRecord = RADNET_DETECT_RECORD_WORDS;      // ... and per record
constexpr int kMaxClasses = RADNET_SCAN_MAX_CLASSES;
constexpr int kFlagMalformed = 1, kFlagRange = 2, kFlagEmpty = 4;      // final_nms_kernel's findings, by precedence

__host__ __device__ __forceinline__ size_t pad16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

// ---- NumPy's fp32 sum of a contiguous vector (pairwise_sum of loops_utils.h.src, as np.add.reduce and np.mean call it) ------
__device__ float np_block_sum(const float* a, int n) {      // n <= 128
  if (n < 8) {
    float r = 0.f;
    for (int i = 0; i < n; ++i) r += a[i];
    return r;
  }
  float r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
    r0 += a[i]; r1 += a[i + 1]; r2 += a[i + 2]; r3 += a[i + 3];
    r4 += a[i + 4]; r5 += a[i + 5]; r6 += a[i + 6]; r7 += a[i + 7];
  }
  float res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (; i < n; ++i) res += a[i];
  return res;
}

__device__ float np_sum_f32(const float* a, int n) {
  if (n <= 128) return np_block_sum(a, n);
  // the recursion "halves split at n/2 rounded down to a multiple of 8" with its own stack: a level halves the length, so 32
  // frames hold any int32 length
  int off[32], len[32];
  float left[32];
  int state[32];                      // 0: not entered, 1: in its left half, 2: in its right half
  int sp = 1;
  off[0] = 0; len[0] = n; state[0] = 0;
  float v = 0.f;
  bool have = false;                  // v holds the sum of the frame just left
  for (;;) {
    const int f = sp - 1;
    if (!have) {
      if (len[f] <= 128) {
        v = np_block_sum(a + off[f], len[f]);
        have = true;
        --sp;
      } else {
        int n2 = len[f] / 2;
        n2 -= n2 % 8;
        state[f] = 1;
        off[sp] = off[f]; len[sp] = n2; state[sp] = 0;
        ++sp;
      }
    } else {
      if (sp == 0) return v;
      if (state[f] == 1) {
        int n2 = len[f] / 2;
        n2 -= n2 % 8;
        left[f] = v;
        state[f] = 2;
        off[sp] = off[f] + n2; len[sp] = len[f] - n2; state[sp] = 0;
        ++sp;
        have = false;
      } else {
        v = left[f] + v;
        --sp;
      }
    }
  }
}

// ---- RADNet.final_nms ------------------------------------------------------------------------------------------------------
struct FinalArgs {
  const long long* boxes;
  const float* probs;
  const int* offsets;
  int n_groups, capacity;
  double thr;
  float conf;
  int navg;
  long long* out_boxes;
  float* out_probs;
  int* out_count;
  int* out_status;
  // workspace
  u64* keys;         // [2 * capacity]: group at 2 * lo (a group's power of two is below twice its size)
  int4* sbox;        // [capacity] boxes by order position
  float* sprob;      // [capacity] probs by order position
  int* cid;          // [capacity] cluster of an order position, -1 while it is alive
  float* cprob;      // [capacity] probs by (cluster, position)
  int* rstart;       // [capacity + n_groups]: group at lo + its index; first row of every cluster's run, then n
};

struct FinalWs {
  size_t keys, sbox, sprob, cid, cprob, rstart, bytes;
};

__host__ __device__ inline FinalWs final_ws(long long capacity, long long n_groups) {
  FinalWs w;
  size_t at = 0;
  w.keys = at;   at += pad16((size_t)16 * capacity);
  w.sbox = at;   at += pad16((size_t)16 * capacity);
  w.sprob = at;  at += pad16((size_t)4 * capacity);
  w.cid = at;    at += pad16((size_t)4 * capacity);
  w.cprob = at;  at += pad16((size_t)4 * capacity);
  w.rstart = at; at += pad16((size_t)4 * (capacity + n_groups + 1));
  w.bytes = at + 16;
  return w;
}

template <bool kLds>
__device__ void final_group(const FinalArgs& g, int grp, int lo, int n, int P, u64* s_keys, int* s_next, int* s_flags) {
  const int tid = threadIdx.x;
  u64* gkeys = g.keys + 2 * (size_t)lo;
  auto K = [&](int i) -> u64& { return kLds ? s_keys[i] : gkeys[i]; };
  const long long* boxes = g.boxes + 4 * (size_t)lo;
  const float* probs = g.probs + lo;
  int4* sbox = g.sbox + lo;
  float* sprob = g.sprob + lo;
  int* cid = g.cid + lo;
  float* cprob = g.cprob + lo;
  int* rstart = g.rstart + lo + grp;

  // (1) validation, keys, sort
  for (int i = tid; i < P; i += kThreads) {
    u64 key = ~0ull;                                       // padding: behind every key
    if (i < n) {
      const long long x1 = boxes[4 * i], y1 = boxes[4 * i + 1], x2 = boxes[4 * i + 2], y2 = boxes[4 * i + 3];
      const float p = probs[i];
      const long long m = RADNET_SCAN_MAX_COORD;
      if (!(x1 < x2) || !(y1 < y2)) atomicOr(s_flags, kFlagMalformed);      // RADNet.py:171-172 asserts
      if (x1 < -m || y1 < -m || x2 > m || y2 > m || p != p) atomicOr(s_flags, kFlagRange);
      // signed zeros tie, as in np.argsort: the key of p + 0.0f (-0 + 0 = +0, the sum is the identity on every other non-NaN
      // value, and a NaN has raised kFlagRange above, which returns before a key is read)
      key = ((u64)sortable_bits_np(p) << 32) | (unsigned int)i;
    }
    K(i) = key;
  }
  __syncthreads();
  if (*s_flags) {
    if (tid == 0) {
      g.out_count[grp] = 0;
      g.out_status[grp] = (*s_flags & kFlagMalformed) ? RADNET_FINAL_NMS_MALFORMED : RADNET_FINAL_NMS_RANGE;
    }
    return;
  }
  if (kLds) bitonic_sort<false>(s_keys, P); else bitonic_sort<false>(gkeys, P);
  for (int i = tid; i < n; i += kThreads) {
    const int r = (int)(K(i) & 0xFFFFFFFFull);
    sbox[i] = make_int4((int)boxes[4 * r], (int)boxes[4 * r + 1], (int)boxes[4 * r + 2], (int)boxes[4 * r + 3]);
    sprob[i] = probs[r];
    cid[i] = -1;
  }
  __syncthreads();

  // (2) the clusters, a round of the walk each: cid[j] is the per-position state.  The overlap is RADNet.final_nms's own (exact
  // integer areas, the quotient always taken), not suppresses().
  int4 tb;
  long long at;
  const int nclus = walk_from_top(
      n - 1, INT_MAX, s_next,
      [&](int top, int c) {
        tb = sbox[top];
        at = (long long)(tb.z - tb.x) * (long long)(tb.w - tb.y);
        if ((top & (kThreads - 1)) == tid) cid[top] = c;
      },
      [&](int j, int c) {
        if (cid[j] >= 0) return true;
        const int4 b = sbox[j];
        const long long iw = max(0, min(tb.z, b.z) - max(tb.x, b.x)), ih = max(0, min(tb.w, b.w) - max(tb.y, b.y));
        const long long inter = iw * ih;
        const long long ar = (long long)(b.z - b.x) * (long long)(b.w - b.y);
        const double overlap = (double)inter / ((double)(at + ar - inter) + 1e-6);
        if (overlap > g.thr) cid[j] = c;
        return overlap > g.thr;
      });

  // (3) every cluster's members side by side, in order position
  for (int i = tid; i < P; i += kThreads) K(i) = i < n ? (((u64)(unsigned int)cid[i] << 32) | (unsigned int)i) : ~0ull;
  __syncthreads();
  if (kLds) bitonic_sort<false>(s_keys, P); else bitonic_sort<false>(gkeys, P);
  for (int i = tid; i < n; i += kThreads) {
    const u64 k = K(i);
    const int ci = (int)(k >> 32);
    cprob[i] = sprob[(int)(k & 0xFFFFFFFFull)];
    if (i == 0 || (int)(K(i - 1) >> 32) != ci) rstart[ci] = i;
  }
  if (tid == 0) rstart[nclus] = n;
  __syncthreads();

  // (4) a thread per cluster
  for (int cl = tid; cl < nclus; cl += kThreads) {
    const int s = rstart[cl], e = rstart[cl + 1];
    int a;
    if (cprob[e - 1] < g.conf) {                           // the members' maximum is top's prob, the last of the run
      a = (e - s > g.navg) ? e - g.navg : s;
    } else {
      a = e;
      while (a > s && cprob[a - 1] > g.conf) --a;
    }
    if (a == e) {                                          // the maximum equals the threshold: nothing chosen
      atomicOr(s_flags, kFlagEmpty);
      continue;
    }
    long long sx1 = 0, sy1 = 0, sx2 = 0, sy2 = 0;
    for (int k = a; k < e; ++k) {
      const int4 b = sbox[(int)(K(k) & 0xFFFFFFFFull)];
      sx1 += b.x; sy1 += b.y; sx2 += b.z; sy2 += b.w;
    }
    const int cnt = e - a;
    const float ps = 0.f + np_sum_f32(cprob + a, cnt);     // add.reduce starts from its identity
    long long* ob = g.out_boxes + 4 * ((size_t)lo + cl);
    ob[0] = (long long)rint((double)sx1 / (double)cnt);
    ob[1] = (long long)rint((double)sy1 / (double)cnt);
    ob[2] = (long long)rint((double)sx2 / (double)cnt);
    ob[3] = (long long)rint((double)sy2 / (double)cnt);
    g.out_probs[lo + cl] = ps / (float)cnt;
  }
  __syncthreads();
  if (tid == 0) {
    g.out_count[grp] = nclus;
    g.out_status[grp] = (*s_flags & kFlagEmpty) ? RADNET_FINAL_NMS_EMPTY : 0;
  }
}

__global__ void __launch_bounds__(kThreads) final_nms_kernel(FinalArgs g) {
  __shared__ u64 s_keys[kLdsKeys];
  __shared__ int s_next[3];
  __shared__ int s_flags;
  const int grp = blockIdx.x;
  int lo = g.offsets[grp], hi = g.offsets[grp + 1];
  lo = lo < 0 ? 0 : (lo > g.capacity ? g.capacity : lo);
  hi = hi < lo ? lo : (hi > g.capacity ? g.capacity : hi);
  const int n = hi - lo;
  if (threadIdx.x == 0) {
    s_flags = 0;
    s_next[0] = s_next[1] = s_next[2] = -1;
  }
  if (n == 0) {
    if (threadIdx.x == 0) { g.out_count[grp] = 0; g.out_status[grp] = 0; }
    return;
  }
  int P = 1;
  while (P < n) P <<= 1;
  __syncthreads();
  if (P <= kLdsKeys) final_group<true>(g, grp, lo, n, P, s_keys, s_next, &s_flags);
  else final_group<false>(g, grp, lo, n, P, s_keys, s_next, &s_flags);
}

int check_final(radnet_ctx* ctx, const radnet_final_nms_desc* d) {
  if (d->n_groups < 0 || d->capacity < 0) RADNET_FAIL(ctx, RADNET_ERR_ARG, "final_nms: %d groups, capacity %d", d->n_groups, d->capacity);
  if (d->capacity > RADNET_SCAN_MAX_BOXES) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "final_nms: capacity %d (max %d)", d->capacity, RADNET_SCAN_MAX_BOXES);
  if (d->n_obj_avg < 1) RADNET_FAIL(ctx, RADNET_ERR_ARG, "final_nms: n_obj_avg = %d", d->n_obj_avg);
  if (d->obj_avg_threshold != d->obj_avg_threshold || d->obj_confidence_threshold != d->obj_confidence_threshold)
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "final_nms: a NaN threshold");
  if (d->n_groups == 0) return RADNET_OK;
  if (!d->offsets || !d->out_count || !d->out_status || !d->ws) RADNET_FAIL(ctx, RADNET_ERR_ARG, "final_nms: null pointer in the descriptor");
  if (d->capacity > 0 && (!d->boxes || !d->probs || !d->out_boxes || !d->out_probs)) RADNET_FAIL(ctx, RADNET_ERR_ARG, "final_nms: null pointer in the descriptor");
  if ((uintptr_t)d->ws & 15) RADNET_FAIL(ctx, RADNET_ERR_ARG, "final_nms: the workspace must be 16-byte aligned");
  return RADNET_OK;
}

int launch_final(radnet_ctx* ctx, const radnet_final_nms_desc* d) {
  if (d->n_groups == 0) return RADNET_OK;
  const FinalWs w = final_ws(d->capacity, d->n_groups);
  char* ws = (char*)d->ws;
  FinalArgs g;
  g.boxes = (const long long*)d->boxes; g.probs = d->probs; g.offsets = d->offsets;
  g.n_groups = d->n_groups; g.capacity = d->capacity;
  g.thr = d->obj_avg_threshold; g.conf = d->obj_confidence_threshold; g.navg = d->n_obj_avg;
  g.out_boxes = (long long*)d->out_boxes; g.out_probs = d->out_probs; g.out_count = d->out_count; g.out_status = d->out_status;
  g.keys = (u64*)(ws + w.keys); g.sbox = (int4*)(ws + w.sbox); g.sprob = (float*)(ws + w.sprob); g.cid = (int*)(ws + w.cid);
  g.cprob = (float*)(ws + w.cprob); g.rstart = (int*)(ws + w.rstart);
  hipLaunchKernelGGL(final_nms_kernel, dim3(d->n_groups), dim3(kThreads), 0, ctx->stream, g);
  RADNET_CHECK_LAUNCH(ctx, "final_nms");
  return RADNET_OK;
}

// ---- the gather --------------------------------------------------------------------------------------------------------------
struct MergeArgs {
  const int* pool;
  long long pool_words;
  int slot_rows;
  const radnet_scan_tile* tiles;
  int n_tiles, n_images, nc, max_boxes;
  long long capacity;      // n_tiles * slot_rows
  double nms_thr;
  int* out;
  // workspace
  int* tile_n;             // [n_tiles] records of the tile, 0 for a bad slot
  int* tile_bad;           // [n_tiles]
  int* tile_cnt;           // [n_tiles][nc] records of a class
  int* tile_first;         // [n_tiles][nc] its first record
  int* tile_base;          // [n_tiles][nc] where the tile's records of the class start inside their group
  int* goff;               // [n_images * nc + 1] the groups' offsets
  u64* first_key;          // [nc] tile << 32 | record of the class's first appearance, ~0 for none
  int* bad;                // [1] any bad slot
  long long* gboxes;       // [capacity][4]
  float* gprobs;           // [capacity]
  long long* fboxes;       // radnet_final_nms's outputs
  float* fprobs;
  int* fcount;
  int* fstatus;
  u64* ckeys;              // [2 * capacity] class NMS: keys; a class's candidates start at the count of the classes below it
  double4* cbox;           // [capacity] boxes by order position
  int* crow;               // [capacity] row of fboxes of a candidate
  int* srow;               // [capacity] the same by order position
  int* live;               // [capacity]
  int* cls_np;             // [nc] picks of a class
  int* cls_bad;            // [nc] a malformed box among its candidates
  int* pick_row;           // [nc][max_boxes]
};

struct MergeWs {
  size_t tile_n, tile_bad, tile_cnt, tile_first, tile_base, goff, first_key, bad, gboxes, gprobs, fboxes, fprobs, fcount, fstatus, fws, ckeys, cbox,
      crow, srow, live, cls_np, cls_bad, pick_row, bytes;
};

MergeWs merge_ws(long long n_tiles, long long slot_rows, long long n_images, long long nc, long long max_boxes) {
  const long long cap = n_tiles * slot_rows, groups = n_images * nc;
  MergeWs w;
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t here = at; at += pad16(bytes); return here; };
  w.tile_n = take(4 * n_tiles);
  w.tile_bad = take(4 * n_tiles);
  w.tile_cnt = take(4 * n_tiles * nc);
  w.tile_first = take(4 * n_tiles * nc);
  w.tile_base = take(4 * n_tiles * nc);
  w.goff = take(4 * (groups + 1));
  w.first_key = take(8 * nc);
  w.bad = take(4);
  w.gboxes = take(32 * cap);
  w.gprobs = take(4 * cap);
  w.fboxes = take(32 * cap);
  w.fprobs = take(4 * cap);
  w.fcount = take(4 * groups);
  w.fstatus = take(4 * groups);
  w.fws = take(final_ws(cap, groups).bytes);
  w.ckeys = take(16 * cap);
  w.cbox = take(32 * cap);
  w.crow = take(4 * cap);
  w.srow = take(4 * cap);
  w.live = take(4 * cap);
  w.cls_np = take(4 * nc);
  w.cls_bad = take(4 * nc);
  w.pick_row = take(4 * nc * max_boxes);
  w.bytes = at + 32;
  return w;
}

// the records of a tile's slot, or 0 with *bad set for a slot that cannot be read
__device__ __forceinline__ int slot_records(const MergeArgs& g, const radnet_scan_tile& t, bool* bad) {
  const long long slot_words = kHeader + (long long)kRecord * g.slot_rows;
  *bad = t.slot < 0 || (long long)t.slot > g.pool_words - slot_words || t.image < 0 || t.image >= g.n_images;
  if (*bad) return 0;
  const int m = g.pool[t.slot];
  if (m < 0 || m > g.slot_rows) { *bad = true; return 0; }
  return m;
}

__global__ void __launch_bounds__(256) scan_count_kernel(MergeArgs g) {
  __shared__ int s_cnt[kMaxClasses], s_first[kMaxClasses], s_bad;
  const int t = blockIdx.x, tid = threadIdx.x;
  const radnet_scan_tile tile = g.tiles[t];
  bool bad;
  const int m = slot_records(g, tile, &bad);
  if (tid < kMaxClasses) { s_cnt[tid] = 0; s_first[tid] = INT32_MAX; }
  if (tid == 0) s_bad = bad ? 1 : 0;
  __syncthreads();
  const int* rec = g.pool + (bad ? 0 : tile.slot) + kHeader;
  for (int r = tid; r < m; r += 256) {
    const int c = rec[kRecord * r];
    if (c < 0 || c >= g.nc) { s_bad = 1; continue; }      // (every writer stores 1) the record is left out, here and in scan_fill
    atomicAdd(&s_cnt[c], 1);
    atomicMin(&s_first[c], r);
  }
  __syncthreads();
  if (tid < g.nc) {
    g.tile_cnt[(size_t)t * g.nc + tid] = s_cnt[tid];
    g.tile_first[(size_t)t * g.nc + tid] = s_first[tid];
  }
  if (tid == 0) { g.tile_n[t] = m; g.tile_bad[t] = s_bad; }
}

__global__ void __launch_bounds__(256) scan_plan_kernel(MergeArgs g) {
  __shared__ int s_part[256];
  __shared__ int s_bad;
  const int tid = threadIdx.x;
  const int groups = g.n_images * g.nc;
  if (tid == 0) s_bad = 0;
  for (int i = tid; i <= groups; i += 256) g.goff[i] = 0;              // sizes first, offsets below
  __syncthreads();
  for (int t = tid; t < g.n_tiles; t += 256)
    if (g.tile_bad[t]) s_bad = 1;
  if (tid < g.nc) {                                                    // a thread per class walks the tiles in order
    const int c = tid;
    int image = -1, running = 0;
    u64 first = ~0ull;
    for (int t = 0; t < g.n_tiles; ++t) {
      const int im = g.tiles[t].image;
      if (im != image) {
        if (image >= 0 && image < g.n_images) g.goff[image * g.nc + c] = running;
        image = im;
        running = 0;
      }
      const int cnt = g.tile_cnt[(size_t)t * g.nc + c];
      g.tile_base[(size_t)t * g.nc + c] = running;
      running += cnt;
      if (cnt > 0 && first == ~0ull) first = ((u64)(unsigned int)t << 32) | (unsigned int)g.tile_first[(size_t)t * g.nc + c];
    }
    if (image >= 0 && image < g.n_images) g.goff[image * g.nc + c] = running;
    g.first_key[c] = first;
  }
  __syncthreads();
  // exclusive prefix sum of the sizes: a run of groups per thread, the runs' sums through LDS
  const int per = (groups + 255) / 256;
  const int lo = min(groups, tid * per), hi = min(groups, lo + per);
  int sum = 0;
  for (int i = lo; i < hi; ++i) sum += g.goff[i];
  s_part[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    int at = 0;
    for (int i = 0; i < 256; ++i) { const int v = s_part[i]; s_part[i] = at; at += v; }
    g.goff[groups] = at;
    g.bad[0] = s_bad;
  }
  __syncthreads();
  int at = s_part[tid];
  for (int i = lo; i < hi; ++i) { const int v = g.goff[i]; g.goff[i] = at; at += v; }
}

__global__ void __launch_bounds__(kThreads) scan_fill_kernel(MergeArgs g) {
  const int t = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const radnet_scan_tile tile = g.tiles[t];
  const int m = g.tile_n[t];
  if (m == 0) return;
  const int* rec = g.pool + tile.slot + kHeader;                      // m > 0: scan_count read this slot
  for (int c = wave; c < g.nc; c += kThreads / 64) {
    if (g.tile_cnt[(size_t)t * g.nc + c] == 0) continue;
    const long long dst = (long long)g.goff[tile.image * g.nc + c] + g.tile_base[(size_t)t * g.nc + c];
    int run = 0;
    for (int r0 = 0; r0 < m; r0 += 64) {
      const int r = r0 + lane;
      const bool mine = r < m && rec[kRecord * r] == c;
      const u64 mask = __ballot(mine);
      if (mine) {
        const long long d = dst + run + __popcll(mask & ((1ull << lane) - 1ull));
        if (d < g.capacity) {
          const int* q = rec + kRecord * r;
          g.gboxes[4 * d] = (long long)q[1] + tile.ox;
          g.gboxes[4 * d + 1] = (long long)q[2] + tile.oy;
          g.gboxes[4 * d + 2] = (long long)q[3] + tile.ox;
          g.gboxes[4 * d + 3] = (long long)q[4] + tile.oy;
          g.gprobs[d] = __int_as_float(q[5]);
        }
      }
      run += __popcll(mask);
    }
  }
}

// ---- the NMS across the images, a workgroup per class --------------------------------------------------------------------------
template <bool kLds>
__device__ void class_nms(const MergeArgs& g, int c, int start, int M, int P, u64* s_keys, int* s_next, int* s_bad) {
  const int tid = threadIdx.x;
  u64* gkeys = g.ckeys + 2 * (size_t)start;
  auto K = [&](int i) -> u64& { return kLds ? s_keys[i] : gkeys[i]; };
  const int* crow = g.crow + start;
  double4* cbox = g.cbox + start;
  int* srow = g.srow + start;
  int* live = g.live + start;
  for (int i = tid; i < P; i += kThreads) K(i) = i < M ? (((u64)sortable_bits(g.fprobs[crow[i]]) << 32) | (unsigned int)i) : ~0ull;      // raw bits, as detect_tail_kernel's keys
  __syncthreads();
  if (kLds) bitonic_sort<false>(s_keys, P); else bitonic_sort<false>(gkeys, P);
  for (int i = tid; i < M; i += kThreads) {
    const int row = crow[(int)(K(i) & 0xFFFFFFFFull)];
    const long long* b = g.fboxes + 4 * (size_t)row;
    const double4 d = make_double4((double)b[0], (double)b[1], (double)b[2], (double)b[3]);
    if (!(d.x < d.z) || !(d.y < d.w)) *s_bad = 1;                      // rpn.py:400-401 asserts (every writer stores 1)
    cbox[i] = d;
    srow[i] = row;
    live[i] = 1;
  }
  __syncthreads();
  if (*s_bad) {
    if (tid == 0) { g.cls_np[c] = 0; g.cls_bad[c] = 1; }
    return;
  }
  // greedy from the end of the ascending order (among equal probs the higher index first), a pick per round of the walk
  double4 pk;
  double pk_area;
  const int np = walk_from_top(
      M - 1, g.max_boxes, s_next,
      [&](int top, int r) {
        pk = cbox[top];
        pk_area = (pk.z - pk.x) * (pk.w - pk.y);
        if (tid == 0) g.pick_row[(size_t)c * g.max_boxes + r] = srow[top];
      },
      [&](int j, int) {
        if (!live[j]) return true;
        const double4 cb = cbox[j];
        const bool hit = suppresses(pk, pk_area, cb, (cb.z - cb.x) * (cb.w - cb.y), g.nms_thr);
        if (hit) live[j] = 0;
        return hit;
      });
  if (tid == 0) { g.cls_np[c] = np; g.cls_bad[c] = 0; }
}

__global__ void __launch_bounds__(kThreads) class_nms_kernel(MergeArgs g) {
  __shared__ u64 s_keys[kLdsKeys];
  __shared__ int s_next[3];
  __shared__ int s_bad, s_start, s_total;
  const int c = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) {
    s_bad = 0; s_start = 0; s_total = 0;
    s_next[0] = s_next[1] = s_next[2] = -1;
  }
  __syncthreads();
  // candidates of this class, and of the classes below it: where its part of the workspace starts
  const int groups = g.n_images * g.nc;
  int below = 0, mine = 0;
  for (int i = tid; i < groups; i += kThreads) {
    const int cc = i % g.nc, cnt = g.fcount[i];
    if (cc < c) below += cnt; else if (cc == c) mine += cnt;
  }
  if (below) atomicAdd(&s_start, below);
  if (mine) atomicAdd(&s_total, mine);
  __syncthreads();
  const int start = s_start, M = s_total;
  if (M == 0 || (long long)start + M > g.capacity) {
    if (tid == 0) { g.cls_np[c] = 0; g.cls_bad[c] = 0; }
    return;
  }
  int base = 0;
  for (int im = 0; im < g.n_images; ++im) {                             // image order, then cluster order
    const int grp = im * g.nc + c, cnt = g.fcount[grp], off = g.goff[grp];
    for (int i = tid; i < cnt; i += kThreads) g.crow[start + base + i] = off + i;
    base += cnt;
  }
  int P = 1;
  while (P < M) P <<= 1;
  __syncthreads();
  if (P <= kLdsKeys) class_nms<true>(g, c, start, M, P, s_keys, s_next, &s_bad);
  else class_nms<false>(g, c, start, M, P, s_keys, s_next, &s_bad);
}

__global__ void __launch_bounds__(kThreads) scan_write_kernel(MergeArgs g) {
  __shared__ int s_status, s_obase[kMaxClasses];
  const int tid = threadIdx.x;
  if (tid == 0) s_status = g.bad[0] ? RADNET_SCAN_MERGE_BAD_SLOT : 0;
  __syncthreads();
  int st = 0;
  for (int i = tid; i < g.n_images * g.nc; i += kThreads) {
    const int f = g.fstatus[i];
    const int code = f == RADNET_FINAL_NMS_MALFORMED ? RADNET_SCAN_MERGE_MALFORMED
                     : f == RADNET_FINAL_NMS_EMPTY   ? RADNET_SCAN_MERGE_EMPTY
                     : f == RADNET_FINAL_NMS_RANGE   ? RADNET_SCAN_MERGE_RANGE
                                                     : 0;
    st = min(st, code);
  }
  if (st < 0) atomicMin(&s_status, st);
  __syncthreads();
  // a group that failed leaves cluster rows unwritten: what the final NMS made of them says nothing
  const bool nms_box = s_status == 0 && tid < g.nc && g.cls_bad[tid];
  __syncthreads();
  if (nms_box) s_status = RADNET_SCAN_MERGE_NMS_BOX;      // (every writer stores the same)
  __syncthreads();
  const int status = s_status;
  if (tid == 0) {
    int total = 0;
    if (status == 0) {
      unsigned int done = 0u;
      for (int r = 0; r < g.nc; ++r) {                                  // selection by first appearance (distinct for distinct classes)
        int bc = -1;
        u64 bk = ~0ull;
        for (int c = 0; c < g.nc; ++c)
          if (!((done >> c) & 1u) && g.first_key[c] < bk) { bk = g.first_key[c]; bc = c; }
        if (bc < 0) break;
        done |= 1u << bc;
        s_obase[bc] = total;
        total += g.cls_np[bc];
      }
      for (int c = 0; c < g.nc; ++c)
        if (!((done >> c) & 1u)) s_obase[c] = total;                    // no record of the class: nothing to write
    }
    g.out[0] = total;
    g.out[1] = status;
  }
  __syncthreads();
  if (status != 0) return;
  for (int i = tid; i < g.nc * g.max_boxes; i += kThreads) {
    const int c = i / g.max_boxes, p = i - c * g.max_boxes;
    if (g.first_key[c] == ~0ull || p >= g.cls_np[c]) continue;
    const int row = g.pick_row[i];
    const long long* b = g.fboxes + 4 * (size_t)row;
    int* o = g.out + kHeader + (size_t)kRecord * (s_obase[c] + p);
    o[0] = c;
    o[1] = (int)b[0]; o[2] = (int)b[1]; o[3] = (int)b[2]; o[4] = (int)b[3];      // within +-RADNET_SCAN_MAX_COORD: final_nms_kernel saw to it
    o[5] = (int)__float_as_uint(g.fprobs[row]);
  }
}

}  // namespace

extern "C" uint64_t radnet_final_nms_ws_bytes(int32_t capacity, int32_t n_groups) {
  if (capacity < 0 || n_groups < 0) return 0;
  return (uint64_t)final_ws(capacity, n_groups).bytes;
}

extern "C" int radnet_final_nms(radnet_ctx* ctx, const radnet_final_nms_desc* d) {
  if (!ctx || !d) return RADNET_ERR_ARG;
  int rc = check_final(ctx, d);
  if (rc != RADNET_OK) return rc;
  return launch_final(ctx, d);
}

extern "C" uint64_t radnet_scan_merge_out_bytes(int32_t nc, int32_t max_boxes) {
  if (nc < 0 || max_boxes < 0) return 0;
  return (uint64_t)4 * (kHeader + (uint64_t)kRecord * nc * max_boxes);
}

extern "C" uint64_t radnet_scan_merge_ws_bytes(int32_t n_tiles, int32_t slot_rows, int32_t n_images, int32_t nc, int32_t max_boxes) {
  if (n_tiles < 0 || slot_rows < 0 || n_images < 0 || nc < 0 || max_boxes < 0) return 0;
  return (uint64_t)merge_ws(n_tiles, slot_rows, n_images, nc, max_boxes).bytes;
}

extern "C" int radnet_scan_merge(radnet_ctx* ctx, const radnet_scan_merge_desc* d) {
  if (!ctx || !d) return RADNET_ERR_ARG;
  if (d->nc < 1 || d->nc > kMaxClasses) RADNET_FAIL(ctx, RADNET_ERR_ARG, "scan_merge: %d classes (1..%d)", d->nc, kMaxClasses);
  if (d->max_boxes < 1 || d->max_boxes > RADNET_SCAN_MAX_BOXES / kMaxClasses) RADNET_FAIL(ctx, RADNET_ERR_ARG, "scan_merge: max_boxes = %d", d->max_boxes);
  if (d->nms_thresh != d->nms_thresh) RADNET_FAIL(ctx, RADNET_ERR_ARG, "scan_merge: a NaN threshold");
  if (!d->out || !d->ws) RADNET_FAIL(ctx, RADNET_ERR_ARG, "scan_merge: null pointer in the descriptor");
  if ((uintptr_t)d->ws & 31) RADNET_FAIL(ctx, RADNET_ERR_ARG, "scan_merge: the workspace must be 32-byte aligned");
  int32_t n_images = 0, bad_entry = -1;
  char msg[200];
  if (radnet_scan_merge_check(d->tiles_host, d->n_tiles, d->pool_words, d->slot_rows, &n_images, &bad_entry, msg, (int32_t)sizeof(msg)) != RADNET_OK)
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "%s", msg);
  if (d->n_tiles > 0 && (!d->pool || !d->tiles_dev)) RADNET_FAIL(ctx, RADNET_ERR_ARG, "scan_merge: null pointer in the descriptor");
  const MergeWs w = merge_ws(d->n_tiles, d->slot_rows, n_images, d->nc, d->max_boxes);
  char* ws = (char*)d->ws;
  const int groups = n_images * d->nc;

  radnet_final_nms_desc f;
  memset(&f, 0, sizeof(f));
  f.boxes = (const int64_t*)(ws + w.gboxes); f.probs = (const float*)(ws + w.gprobs); f.offsets = (const int32_t*)(ws + w.goff);
  f.n_groups = groups; f.capacity = d->n_tiles * d->slot_rows;
  f.obj_avg_threshold = d->obj_avg_threshold; f.obj_confidence_threshold = d->obj_confidence_threshold; f.n_obj_avg = d->n_obj_avg;
  f.out_boxes = (int64_t*)(ws + w.fboxes); f.out_probs = (float*)(ws + w.fprobs);
  f.out_count = (int32_t*)(ws + w.fcount); f.out_status = (int32_t*)(ws + w.fstatus);
  f.ws = ws + w.fws;
  int rc = check_final(ctx, &f);
  if (rc != RADNET_OK) return rc;

  MergeArgs g;
  g.pool = d->pool; g.pool_words = d->pool_words; g.slot_rows = d->slot_rows; g.tiles = d->tiles_dev;
  g.n_tiles = d->n_tiles; g.n_images = n_images; g.nc = d->nc; g.max_boxes = d->max_boxes;
  g.capacity = (long long)d->n_tiles * d->slot_rows;
  g.nms_thr = d->nms_thresh;
  g.out = (int*)d->out;
  g.tile_n = (int*)(ws + w.tile_n); g.tile_bad = (int*)(ws + w.tile_bad); g.tile_cnt = (int*)(ws + w.tile_cnt);
  g.tile_first = (int*)(ws + w.tile_first); g.tile_base = (int*)(ws + w.tile_base); g.goff = (int*)(ws + w.goff);
  g.first_key = (u64*)(ws + w.first_key); g.bad = (int*)(ws + w.bad);
  g.gboxes = (long long*)(ws + w.gboxes); g.gprobs = (float*)(ws + w.gprobs);
  g.fboxes = (long long*)(ws + w.fboxes); g.fprobs = (float*)(ws + w.fprobs); g.fcount = (int*)(ws + w.fcount); g.fstatus = (int*)(ws + w.fstatus);
  g.ckeys = (u64*)(ws + w.ckeys); g.cbox = (double4*)(ws + w.cbox); g.crow = (int*)(ws + w.crow); g.srow = (int*)(ws + w.srow);
  g.live = (int*)(ws + w.live); g.cls_np = (int*)(ws + w.cls_np); g.cls_bad = (int*)(ws + w.cls_bad); g.pick_row = (int*)(ws + w.pick_row);

  if (d->n_tiles > 0) {
    hipLaunchKernelGGL(scan_count_kernel, dim3(d->n_tiles), dim3(256), 0, ctx->stream, g);
    RADNET_CHECK_LAUNCH(ctx, "scan_count");
  }
  hipLaunchKernelGGL(scan_plan_kernel, dim3(1), dim3(256), 0, ctx->stream, g);
  RADNET_CHECK_LAUNCH(ctx, "scan_plan");
  if (d->n_tiles > 0) {
    hipLaunchKernelGGL(scan_fill_kernel, dim3(d->n_tiles), dim3(kThreads), 0, ctx->stream, g);
    RADNET_CHECK_LAUNCH(ctx, "scan_fill");
  }
  rc = launch_final(ctx, &f);
  if (rc != RADNET_OK) return rc;
  hipLaunchKernelGGL(class_nms_kernel, dim3(d->nc), dim3(kThreads), 0, ctx->stream, g);
  RADNET_CHECK_LAUNCH(ctx, "class_nms");
  hipLaunchKernelGGL(scan_write_kernel, dim3(1), dim3(kThreads), 0, ctx->stream, g);
  RADNET_CHECK_LAUNCH(ctx, "scan_write");
  return RADNET_OK;
}
