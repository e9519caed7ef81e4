// See wgrad_multi_plan.h.
#include "wgrad_multi_plan.h"

#include <string.h>

int wgrad_multi_plan(const WgradMultiItem* items, int n, uint64_t ws_bytes, unsigned counter_cap, WgradMultiLaunch* out, int cap) {
  if (n < 0 || cap < 0 || (n > 0 && !items) || (cap > 0 && !out)) return kWgradMultiErrArg;
  const uint64_t kMaxGrid = 0x7fffffffull;
  for (int i = 0; i < n; ++i) {
    const WgradMultiItem& it = items[i];
    if ((it.bmk != 64 && it.bmk != 128) || (it.bn != 64 && it.bn != 128) || it.wx == 0 || it.wy == 0 || it.wz == 0) return kWgradMultiErrArg;
    if ((uint64_t)it.wx * it.wy * it.wz > kMaxGrid) return kWgradMultiErrFit;
    if (it.slab_bytes > ws_bytes || it.counters > counter_cap) return kWgradMultiErrFit;
  }
  int n_out = 0;
  for (int first = 0; first < n; ++first) {
    const int bmk = items[first].bmk, bn = items[first].bn;
    bool seen = false;                     // a shape is planned where its first problem stands
    for (int j = 0; j < first && !seen; ++j) seen = items[j].bmk == bmk && items[j].bn == bn;
    if (seen) continue;
    WgradMultiLaunch* cur = nullptr;
    uint64_t slab_at = 0, grid = 0;
    unsigned ctr_at = 0;
    for (int i = first; i < n; ++i) {
      const WgradMultiItem& it = items[i];
      if (it.bmk != bmk || it.bn != bn) continue;
      const uint64_t wgs = (uint64_t)it.wx * it.wy * it.wz;
      if (cur != nullptr && (cur->n == kWgradMultiMax || slab_at + it.slab_bytes > ws_bytes || (uint64_t)ctr_at + it.counters > counter_cap ||
                             grid + wgs > kMaxGrid))
        cur = nullptr;
      if (cur == nullptr) {
        if (n_out == cap) return kWgradMultiErrCap;
        cur = &out[n_out++];
        memset(cur, 0, sizeof(*cur));
        cur->bmk = bmk;
        cur->bn = bn;
        slab_at = 0;
        grid = 0;
        ctr_at = 0;
      }
      const int k = cur->n++;
      cur->problem[k] = i;
      cur->slab_off[k] = slab_at;
      cur->counter_off[k] = ctr_at;
      cur->map.first[k] = (unsigned)grid;
      cur->map.wx[k] = it.wx;
      cur->map.wy[k] = it.wy;
      grid += wgs;
      for (int q = k + 1; q <= kWgradMultiMax; ++q) cur->map.first[q] = (unsigned)grid;      // the entries behind the last problem: the grid
      cur->map.n = cur->n;
      slab_at = (slab_at + it.slab_bytes + 255) & ~(uint64_t)255;
      ctr_at += it.counters;
    }
  }
  return n_out;
}
