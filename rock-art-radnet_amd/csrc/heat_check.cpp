// ---- host side of the heat painter (heat.hip): the placement table's validation ------------------------------------------------------
// No device call and no HIP header: compiled by g++, runs without a GPU (contract: include/radnet_hip.h).  radnet_heat_paint_u8
// calls this before it launches; tests/native/heat_check_sanitize.cpp runs it under ASan + UBSan on exactly sized tables.
#include <stdarg.h>
#include <stdio.h>
#include "radnet_hip.h"

namespace {

int refuse(int32_t i, int32_t* bad_entry, char* msg, int32_t msg_cap, const char* fmt, ...) {
  if (bad_entry) *bad_entry = i;
  if (msg && msg_cap > 0) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, (size_t)msg_cap, fmt, ap);
    va_end(ap);
  }
  return RADNET_ERR_ARG;
}

bool beyond(int32_t v) { return v < -RADNET_DRAW_SCENE_MAX_COORD || v > RADNET_DRAW_SCENE_MAX_COORD; }

}  // namespace

extern "C" int radnet_heat_check(const radnet_heat_place* places, int32_t count, int64_t pool_len, int32_t h, int32_t w, int32_t* bad_entry,
                                 char* msg, int32_t msg_cap) {
  if (msg && msg_cap > 0) msg[0] = 0;
  if (count < 0) return refuse(-1, bad_entry, msg, msg_cap, "heat_paint: %d placements", count);
  if (pool_len < 0) return refuse(-1, bad_entry, msg, msg_cap, "heat_paint: a pool of %lld bytes", (long long)pool_len);
  if (h < 1 || w < 1) return refuse(-1, bad_entry, msg, msg_cap, "heat_paint: an image of %d x %d", h, w);
  if (count == 0) return RADNET_OK;
  if (!places) return refuse(-1, bad_entry, msg, msg_cap, "heat_paint: a null table of %d placements", count);
  for (int32_t i = 0; i < count; ++i) {
    const radnet_heat_place& p = places[i];
    if (p.w < 1 || p.w > RADNET_HEAT_MAX_EXTENT) return refuse(i, bad_entry, msg, msg_cap, "heat_paint: entry %d has w = %d, outside 1..%d", i, p.w, RADNET_HEAT_MAX_EXTENT);
    if (p.h < 1 || p.h > RADNET_HEAT_MAX_EXTENT) return refuse(i, bad_entry, msg, msg_cap, "heat_paint: entry %d has h = %d, outside 1..%d", i, p.h, RADNET_HEAT_MAX_EXTENT);
    if (p.mw < 1 || p.mw > RADNET_HEAT_MAX_MAP) return refuse(i, bad_entry, msg, msg_cap, "heat_paint: entry %d has mw = %d, outside 1..%d", i, p.mw, RADNET_HEAT_MAX_MAP);
    if (p.mh < 1 || p.mh > RADNET_HEAT_MAX_MAP) return refuse(i, bad_entry, msg, msg_cap, "heat_paint: entry %d has mh = %d, outside 1..%d", i, p.mh, RADNET_HEAT_MAX_MAP);
    if (beyond(p.x0)) return refuse(i, bad_entry, msg, msg_cap, "heat_paint: entry %d has x0 = %d, beyond +-%d", i, p.x0, RADNET_DRAW_SCENE_MAX_COORD);
    if (beyond(p.y0)) return refuse(i, bad_entry, msg, msg_cap, "heat_paint: entry %d has y0 = %d, beyond +-%d", i, p.y0, RADNET_DRAW_SCENE_MAX_COORD);
    const int64_t cells = (int64_t)p.mw * p.mh;                       // at most 2047^2
    if (p.offset < 0 || p.offset > pool_len - cells)                  // pool_len - cells cannot overflow: both are small against 2^63
      return refuse(i, bad_entry, msg, msg_cap, "heat_paint: entry %d has offset = %lld for a map of %d x %d in a pool of %lld bytes", i, (long long)p.offset,
                    p.mh, p.mw, (long long)pool_len);
  }
  return RADNET_OK;
}
