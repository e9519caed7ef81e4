// ---- host side of the CRC-32 kernels (crc32.hip): the GF(2) helpers, the segment table's validation and the grain plan ---------------
// No device call and no HIP header: compiled by g++, runs without a GPU (contract: include/radnet_hip.h).  radnet_crc32_segments
// calls radnet_crc32_plan_segments before it launches; tests/native/crc32_plan_sanitize.cpp runs it under ASan + UBSan on exactly
// sized tables.
#include <stdarg.h>
#include <stdio.h>
#include "radnet_hip.h"
#include "crc32_rule.h"

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

extern "C" uint32_t radnet_crc32_shift(int64_t len) { return crc_shift(len); }

extern "C" uint32_t radnet_crc32_combine(uint32_t crc1, uint32_t crc2, int64_t len2) {
  // the init and the final xor of the two sums cancel: what is left of crc1 moves len2 bytes to the front
  return len2 <= 0 ? crc1 : crc_times(crc1, crc_shift(len2)) ^ crc2;
}

extern "C" int radnet_crc32_plan_segments(const radnet_crc32_segment* table, int32_t count, int64_t n, int32_t misalign, radnet_crc32_plan* plan,
                                          int32_t* bad_entry, char* msg, int32_t msg_cap) {
  if (msg && msg_cap > 0) msg[0] = 0;
  if (bad_entry) *bad_entry = -1;
  if (!plan) return refuse(-1, bad_entry, msg, msg_cap, "crc32_segments: a null plan");
  if (count < 0) return refuse(-1, bad_entry, msg, msg_cap, "crc32_segments: %d segments", count);
  if (n < 0) return refuse(-1, bad_entry, msg, msg_cap, "crc32_segments: a buffer of %lld bytes", (long long)n);
  if (misalign < 0 || misalign >= kCrcGrain) return refuse(-1, bad_entry, msg, msg_cap, "crc32_segments: a misalignment of %d (0..%d)", misalign, kCrcGrain - 1);
  if (count > 0 && !table) return refuse(-1, bad_entry, msg, msg_cap, "crc32_segments: a null table of %d segments", count);
  int64_t spans = 0;
  for (int32_t i = 0; i < count; ++i) {
    const radnet_crc32_segment& s = table[i];
    if (s.offset < 0 || s.length < 0 || s.offset > n || s.length > n - s.offset)      // n - offset cannot overflow: 0 <= offset <= n
      return refuse(i, bad_entry, msg, msg_cap, "crc32_segments: segment %d (%lld bytes at offset %lld) leaves the buffer of %lld bytes", i,
                    (long long)s.length, (long long)s.offset, (long long)n);
    // a segment has at most 2^63 / 4096 spans, so the sum passes the bound below long before it could leave 64 bits
    spans += crc_cut_of((uint64_t)misalign + (uint64_t)s.offset, s.length).spans;
    if (spans > RADNET_CRC32_MAX_SPANS) {
      refuse(i, bad_entry, msg, msg_cap, "crc32_segments: more than %d spans of %d bytes up to segment %d", RADNET_CRC32_MAX_SPANS, (int)kCrcSpan, i);
      return RADNET_ERR_UNSUPPORTED;
    }
  }
  plan->spans = spans;
  plan->ws_bytes = 4 * ((int64_t)count + 1 + spans);
  return RADNET_OK;
}
