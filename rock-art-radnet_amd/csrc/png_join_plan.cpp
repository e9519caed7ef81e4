// ---- host side of the IDAT join (png_join.hip): the piece table's validation and the span count ----------------------------------------
// No device call and no HIP header: compiled by g++, runs without a GPU (contract: include/radnet_hip.h).  radnet_png_join_u8 calls
// radnet_png_plan_join before it launches; tests/native/png_join_plan_sanitize.cpp runs it under ASan + UBSan on exactly sized tables.
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

}  // namespace

extern "C" int radnet_png_plan_join(const radnet_png_piece* table, int32_t count, int64_t file_len, int64_t n, int32_t misalign,
                                    radnet_png_join_plan* plan, int32_t* bad_entry, char* msg, int32_t msg_cap) {
  if (msg && msg_cap > 0) msg[0] = 0;
  if (bad_entry) *bad_entry = -1;
  if (!plan) return refuse(-1, bad_entry, msg, msg_cap, "png_join: a null plan");
  if (count < 0) return refuse(-1, bad_entry, msg, msg_cap, "png_join: %d pieces", count);
  if (file_len < 0) return refuse(-1, bad_entry, msg, msg_cap, "png_join: a file of %lld bytes", (long long)file_len);
  if (n < 0) return refuse(-1, bad_entry, msg, msg_cap, "png_join: an output of %lld bytes", (long long)n);
  if (misalign < 0 || misalign >= RADNET_PNG_JOIN_GRAIN)
    return refuse(-1, bad_entry, msg, msg_cap, "png_join: a misalignment of %d (0..%d)", misalign, RADNET_PNG_JOIN_GRAIN - 1);
  if (count > 0 && !table) return refuse(-1, bad_entry, msg, msg_cap, "png_join: a null table of %d pieces", count);
  int64_t at = 0;      // the sum of the lengths so far; 0 <= at <= n, so n - at cannot overflow
  for (int32_t i = 0; i < count; ++i) {
    const radnet_png_piece& p = table[i];
    if (p.src < 0 || p.length < 0 || p.src > file_len || p.length > file_len - p.src)      // file_len - src cannot overflow: 0 <= src <= file_len
      return refuse(i, bad_entry, msg, msg_cap, "png_join: piece %d (%lld bytes at byte %lld) leaves the file of %lld bytes", i, (long long)p.length,
                    (long long)p.src, (long long)file_len);
    if (p.dst != at)
      return refuse(i, bad_entry, msg, msg_cap, "png_join: piece %d stands at %lld of the output, the pieces in front of it hold %lld bytes", i,
                    (long long)p.dst, (long long)at);
    if (p.length > n - at)
      return refuse(i, bad_entry, msg, msg_cap, "png_join: piece %d (%lld bytes at %lld) passes the output's %lld bytes", i, (long long)p.length,
                    (long long)at, (long long)n);
    at += p.length;
  }
  if (at != n) return refuse(-1, bad_entry, msg, msg_cap, "png_join: the pieces hold %lld bytes, the output %lld", (long long)at, (long long)n);
  // misalign + n may leave int64 at its very end, so the grains are counted unsigned
  const uint64_t grains = n ? ((uint64_t)misalign + (uint64_t)n + RADNET_PNG_JOIN_GRAIN - 1) / RADNET_PNG_JOIN_GRAIN : 0;
  const uint64_t spans = (grains + RADNET_PNG_JOIN_SPAN_GRAINS - 1) / RADNET_PNG_JOIN_SPAN_GRAINS;
  if (spans > RADNET_PNG_JOIN_MAX_SPANS) {
    refuse(-1, bad_entry, msg, msg_cap, "png_join: more than %d spans of %d bytes", RADNET_PNG_JOIN_MAX_SPANS, RADNET_PNG_JOIN_GRAIN * RADNET_PNG_JOIN_SPAN_GRAINS);
    return RADNET_ERR_UNSUPPORTED;
  }
  plan->grains = (int64_t)grains;
  plan->spans = (int64_t)spans;
  return RADNET_OK;
}
