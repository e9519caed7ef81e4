// The building blocks of the greedy NMS kernels (proposals.hip: nms_kernel, select_nms_kernel; detect_tail.hip: the per-class NMS
// of a tile; scan_tail.hip: final_nms and the NMS across the images of a scan), each ONE body, so that the units cannot drift apart:
//   keys        sortable_bits / sortable_bits_np: a float's bits in an order that unsigned comparison keeps
//   tests       suppresses (fp64 boxes) / suppresses_int (IBox): the reference's rounded quotient against the threshold
//   sort        bitonic_sort<kDescending>: a workgroup's compare-exchange network over keys in LDS or in global memory
//   chunk scan  chunk_scan<Box trait> + write_picks: greedy NMS over sorted candidates, 64 at a time, picks in LDS
//   walk        walk_from_top: greedy rounds over ascending positions kept in global memory, a barrier per round
// Every workgroup that uses them has kNmsThreads threads.  Units that include this are compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

constexpr int kNmsThreads = 1024;

// ---- keys ---------------------------------------------------------------------------------------------------------------------
// Order-preserving bits of a float: a < b  <=>  sortable_bits(a) < sortable_bits(b), with -0.0 below +0.0 (the raw mapping).
__device__ __forceinline__ unsigned int sortable_bits(float f) {
  const unsigned int u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// The same with signed zeros tied, as NumPy's sort has them (-0.0 == +0.0): one key, so that the caller's tie rule (the index in
// the low bits) decides between them.  Every other value, NaNs included, keeps its raw key.
__device__ __forceinline__ unsigned int sortable_bits_np(float f) {
  return sortable_bits(__float_as_uint(f) == 0x80000000u ? 0.0f : f);
}

// ---- suppression tests --------------------------------------------------------------------------------------------------------
// rpn.py:429-447 with i = the picked box
__device__ __forceinline__ bool suppresses(const double4& pk, double pk_area, const double4& c, double c_area, double thr) {
  const double ww = fmax(0.0, fmin(pk.z, c.z) - fmax(pk.x, c.x));
  const double hh = fmax(0.0, fmin(pk.w, c.w) - fmax(pk.y, c.y));
  const double inter = ww * hh;
  const double uni = pk_area + c_area - inter;
  const double d = uni + 1e-6;
  // The reference compares the ROUNDED quotient with thr.  An fp64 division is a ~40-instruction sequence here and
  // this test runs picks x candidates times, so decide without it whenever the outcome cannot depend on rounding:
  // with d > 0, thr > 0 and |inter - thr*d| beyond a 2^-40 relative margin (the products and the quotient each
  // carry < 2^-52), fl(inter/d) > thr  <=>  inter > thr*d.  Everything inside the margin takes the division.
  if (d > 0.0 && thr > 0.0) {
    const double t = thr * d;
    if (inter > t * (1.0 + 0x1p-40)) return true;
    if (inter < t * (1.0 - 0x1p-40)) return false;
  }
  return inter / d > thr;
}

struct __attribute__((aligned(8))) IBox {      // integer-valued box (after np.round and the clip to the feature map), 8 bytes
  short x1, y1, x2, y2;
};

// rpn.py:429-447 on integer boxes: inter and union are exact integers, the comparison is the reference's
// fl(inter / (union + 1e-6)) > thr (same margin test as `suppresses`, the division only inside the margin)
__device__ __forceinline__ bool suppresses_int(const IBox& pk, int pk_area, const IBox& c, int c_area, double thr) {
  const int iw = min((int)pk.x2, (int)c.x2) - max((int)pk.x1, (int)c.x1);
  const int ih = min((int)pk.y2, (int)c.y2) - max((int)pk.y1, (int)c.y1);
  if (iw <= 0 || ih <= 0) return false;                   // inter = 0: 0 / d > thr is false for thr > 0 (checked by the launcher)
  const int inter_i = iw * ih;
  const double inter = (double)inter_i, d = (double)(pk_area + c_area - inter_i) + 1e-6;
  const double t = thr * d;
  if (inter > t * (1.0 + 0x1p-40)) return true;
  if (inter < t * (1.0 - 0x1p-40)) return false;
  return inter / d > thr;
}

// ---- bitonic sort -------------------------------------------------------------------------------------------------------------
// Sorts the P keys k[0 .. P) (P a power of two; 64-bit, in LDS or in global memory) by every thread of the workgroup; the keys are
// visible to all on entry and on return.  Equal keys (the padding) give the same array whether or not they swap.
template <bool kDescending, typename Keys>
__device__ __forceinline__ void bitonic_sort(Keys k, int P) {
  for (int kk = 2; kk <= P; kk <<= 1) {
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < P; i += kNmsThreads) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const unsigned long long a = k[i], b = k[ixj];
          const bool up = ((i & kk) == 0) != kDescending;
          if (up ? a > b : a < b) { k[i] = b; k[ixj] = a; }
        }
      }
      __syncthreads();
    }
  }
}

// ---- chunk scan ---------------------------------------------------------------------------------------------------------------
// The two box forms the scan runs on: the box and area types, the area, the test, the corners as the reference's astype('int').
struct BoxF64 {
  typedef double4 Box;
  typedef double Area;
  static __device__ __forceinline__ Area area(const Box& b) { return (b.z - b.x) * (b.w - b.y); }
  static __device__ __forceinline__ bool hit(const Box& pk, Area pa, const Box& c, Area ca, double thr) { return suppresses(pk, pa, c, ca, thr); }
  static __device__ __forceinline__ void corners(const Box& b, long long* o) {      // truncation
    o[0] = (long long)b.x; o[1] = (long long)b.y; o[2] = (long long)b.z; o[3] = (long long)b.w;
  }
};

struct BoxI16 {
  typedef IBox Box;
  typedef int Area;
  static __device__ __forceinline__ Area area(const Box& b) { return ((int)b.x2 - (int)b.x1) * ((int)b.y2 - (int)b.y1); }
  static __device__ __forceinline__ bool hit(const Box& pk, Area pa, const Box& c, Area ca, double thr) { return suppresses_int(pk, pa, c, ca, thr); }
  static __device__ __forceinline__ void corners(const Box& b, long long* o) {
    o[0] = (long long)b.x1; o[1] = (long long)b.y1; o[2] = (long long)b.x2; o[3] = (long long)b.y2;
  }
};

constexpr int kMaxPicks = 1024;

// The scan's state, all of it in LDS and declared by the kernel: the picks (kMaxPicks of each), the chunk's 64 candidates,
// sup[2] (candidates suppressed by earlier picks), mat[64] (the intra-chunk matrix) and the number of picks.
template <typename T>
struct ChunkScanLds {
  typename T::Box* pick_box;
  typename T::Area* pick_area;
  int* pick_idx;
  typename T::Box* cand_box;
  typename T::Area* cand_area;
  int* cand_idx;
  unsigned int* sup;
  unsigned long long* mat;
  int* npicks;
};

// Greedy NMS over the n candidates whose keys (box index in the low 32 bits) stand sorted in keys[0 .. n), appending to the picks
// already in `s`; by every thread of the workgroup, *s.npicks visible on entry.  64 candidates at a time:
//   (1) 16 waves test the 64 candidates against all picks so far,
//   (2) each wave builds rows of the 64x64 intra-chunk suppression matrix with __ballot,
//   (3) one lane resolves the chunk sequentially with bit operations and appends picks.
// Work is (#candidates examined) x (#picks), not n^2.  Returns true as soon as max_boxes picks stand.
template <typename T, typename Keys>
__device__ __forceinline__ bool chunk_scan(Keys keys, int n, const typename T::Box* __restrict__ boxes, double thr, int max_boxes,
                                           const ChunkScanLds<T>& s) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // The chunk's candidates come through two dependent reads (sorted key -> box): the reads of chunk c+1 are issued before
  // chunk c is processed and land while its three phases run, instead of ~1.5 us of exposed latency per chunk on a
  // single workgroup.
  int pre_id = 0;
  typename T::Box pre_box = {};
  auto fetch = [&](int base) {
    if (tid < 64 && base + tid < n) {
      pre_id = (int)(keys[base + tid] & 0xFFFFFFFFull);
      pre_box = boxes[pre_id];
    }
  };
  fetch(0);
  for (int base = 0; base < n; base += 64) {
    const int nc = min(64, n - base);
    if (tid < 64) {
      if (tid < nc) {
        s.cand_idx[tid] = pre_id;
        s.cand_box[tid] = pre_box;
        s.cand_area[tid] = T::area(pre_box);
      }
      if (tid < 2) s.sup[tid] = 0u;
    }
    fetch(base + 64);
    __syncthreads();
    const int npicks = *s.npicks;
    // (1) candidates vs existing picks: lane = candidate, wave = slice of the pick list
    {
      bool dead = false;
      if (lane < nc) {
        const typename T::Box c = s.cand_box[lane];
        const typename T::Area ca = s.cand_area[lane];
        for (int p = wave; p < npicks && !dead; p += 16) dead = T::hit(s.pick_box[p], s.pick_area[p], c, ca, thr);
      }
      const unsigned long long m = __ballot(dead);
      if (lane == 0 && m) {
        atomicOr(&s.sup[0], (unsigned int)(m & 0xFFFFFFFFull));
        atomicOr(&s.sup[1], (unsigned int)(m >> 32));
      }
    }
    // (2) intra-chunk matrix: wave handles rows j = wave, wave+16, ...; lane = victim i (> j)
    for (int j = wave; j < 64; j += 16) {
      bool hit = false;
      if (j < nc && lane < nc && lane > j) hit = T::hit(s.cand_box[j], s.cand_area[j], s.cand_box[lane], s.cand_area[lane], thr);
      const unsigned long long m = __ballot(hit);
      if (lane == 0) s.mat[j] = m;
    }
    __syncthreads();
    // (3) sequential resolve of this chunk
    if (tid == 0) {
      unsigned long long alive = ~(((unsigned long long)s.sup[1] << 32) | s.sup[0]);
      if (nc < 64) alive &= (1ull << nc) - 1ull;
      int np = npicks;
      while (alive != 0ull && np < max_boxes) {          // visits the survivors only, in candidate order
        const int j = __ffsll((long long)alive) - 1;
        s.pick_box[np] = s.cand_box[j];
        s.pick_area[np] = s.cand_area[j];
        s.pick_idx[np] = s.cand_idx[j];
        ++np;
        alive &= ~s.mat[j];                               // mat[j] only has bits above j
        alive &= ~(1ull << j);
      }
      *s.npicks = np;
    }
    __syncthreads();
    if (*s.npicks >= max_boxes) return true;
  }
  return false;
}

// The picks to global memory: the count, and whichever of the indices, the boxes and the probs the caller asks for (a prob is
// looked up through the pick's flat index = a*probs_div + pix  ->  probs_src[pix*probs_stride + a]).  *s.npicks visible on entry.
template <typename T>
__device__ __forceinline__ void write_picks(const ChunkScanLds<T>& s, int* __restrict__ out_count, int* __restrict__ out_idx,
                                            long long* __restrict__ out_boxes, float* __restrict__ out_probs,
                                            const float* __restrict__ probs_src, int probs_stride, int probs_div) {
  const int tid = threadIdx.x, np = *s.npicks;
  if (tid == 0) *out_count = np;
  for (int i = tid; i < np; i += blockDim.x) {           // not kNmsThreads: as measured, the constant moves nms_kernel's scan loop and costs it 1 %
    const int id = s.pick_idx[i];
    if (out_idx) out_idx[i] = id;
    if (out_boxes) T::corners(s.pick_box[i], out_boxes + 4 * i);
    if (out_probs) {
      const int a = id / probs_div, pix = id - a * probs_div;
      out_probs[i] = probs_src[(size_t)pix * probs_stride + a];
    }
  }
}

// ---- walk from the top --------------------------------------------------------------------------------------------------------
// Greedy rounds over positions that stand in ascending order in global memory, from `top` down, by every thread of the workgroup:
// a round takes the current `top` (enter(top, r), run by every thread), then a thread visits the positions j = tid, tid + 1024, ..
// below it -- position j belongs to thread j % 1024 alone, so the per-position state needs no ordering between threads -- and
// claimed(j, r) says whether j is out of the running (claimed by this round or an earlier one) or still alive.  The highest position
// left alive is the next `top`: every thread proposes its own (j ascends: the last one left alive is its highest) through an integer
// atomicMax into s_next[r % 3], and ONE barrier per round publishes it.  Three rotating slots (all -1 on entry, the state of the
// first round visible) are enough: thread 0 resets slot r + 1 in round r, whose last readers (round r - 2) passed the barrier of
// round r - 1 before, and whose next writers (round r + 1) come after the barrier of round r.  Ends when nothing is left alive or
// after max_rounds rounds; returns the number of rounds.
template <typename Enter, typename Claimed>
__device__ __forceinline__ int walk_from_top(int top, int max_rounds, int* s_next, Enter enter, Claimed claimed) {
  const int tid = threadIdx.x;
  int r = 0;
  while (top >= 0 && r < max_rounds) {
    enter(top, r);
    if (tid == 0) s_next[(r + 1) % 3] = -1;
    int next = -1;
    for (int j = tid; j < top; j += kNmsThreads)
      if (!claimed(j, r)) next = j;
    if (next >= 0) atomicMax(&s_next[r % 3], next);
    __syncthreads();
    top = s_next[r % 3];
    ++r;
  }
  return r;
}
