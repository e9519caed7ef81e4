// ---- host side of the device inflate (inflate.hip): the measured units -> the chain of units that is the stream ------------------
// No device call and no HIP header: compiled by g++, runs without a GPU (contract: include/radnet_hip.h).
#include <cstdio>
#include <thread>
#include <vector>

#include "radnet_hip.h"

namespace {

// CRC-32 as PNG uses it (ISO 3309, polynomial 0xEDB88320 reflected), eight bytes a step
struct CrcTables {
  uint32_t t[8][256];
  CrcTables() {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
      t[0][i] = c;
    }
    for (uint32_t i = 0; i < 256; ++i)
      for (int k = 1; k < 8; ++k) t[k][i] = t[0][t[k - 1][i] & 255] ^ (t[k - 1][i] >> 8);
  }
};

uint32_t crc32_of(const uint8_t* p, int64_t n) {
  static const CrcTables tables;
  const uint32_t(*t)[256] = tables.t;
  uint32_t c = 0xFFFFFFFFu;
  for (; n >= 8; n -= 8, p += 8) {
    const uint32_t a = c ^ ((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
    c = t[7][a & 255] ^ t[6][(a >> 8) & 255] ^ t[5][(a >> 16) & 255] ^ t[4][a >> 24] ^ t[3][p[4]] ^ t[2][p[5]] ^ t[1][p[6]] ^ t[0][p[7]];
  }
  for (; n > 0; --n, ++p) c = t[0][(c ^ *p) & 255] ^ (c >> 8);
  return ~c;
}

// index of the unit that starts at `bit`, or -1: the starts are strictly increasing
template <class Unit>
int32_t find_start(const Unit* units, int32_t count, int64_t bit) {
  int32_t lo = 0, hi = count;
  while (lo < hi) {
    const int32_t mid = lo + (hi - lo) / 2;
    if ((int64_t)units[mid].start_bit < bit) lo = mid + 1; else hi = mid;
  }
  return lo < count && (int64_t)units[lo].start_bit == bit ? lo : -1;
}

}  // namespace

extern "C" int radnet_inflate_chain(const radnet_inflate_unit* units, int32_t count, int64_t first_bit, int64_t n, int64_t expected,
                                    radnet_inflate_link* links, int32_t link_cap, int32_t* link_count, int32_t* false_count, int32_t* bad_unit) {
  if (!units || !links || !link_count || !false_count || !bad_unit || count < 1 || n < 1 || first_bit < 0 || expected < 0 || link_cap < 0)
    return RADNET_ERR_ARG;
  for (int32_t u = 1; u < count; ++u)
    if (units[u].start_bit <= units[u - 1].start_bit) return RADNET_ERR_ARG;
  *link_count = 0;
  *false_count = 0;
  *bad_unit = -1;
  int64_t bit = first_bit, total = 0;
  int32_t from = -1, written = 0;
  bool have_prev = false;
  uint32_t prev = 0;
  for (;;) {
    const int32_t u = find_start(units, count, bit);
    if (u < 0) {
      *bad_unit = from;
      return RADNET_INFLATE_CHAIN_NO_START;
    }
    const radnet_inflate_unit& unit = units[u];
    *bad_unit = u;
    if (unit.status != RADNET_INFLATE_OK) return RADNET_INFLATE_CHAIN_BAD_UNIT;
    if ((unit.flags & RADNET_INFLATE_FLAG_LEAD_MATCH) && !have_prev) return RADNET_INFLATE_CHAIN_LEAD_MATCH;
    if (written >= link_cap) return RADNET_ERR_ARG;
    links[written++] = radnet_inflate_link{total, unit.start_bit, unit.out_bytes, have_prev ? prev : 0u, 0u};
    *link_count = written;
    total += unit.out_bytes;
    if (unit.flags & RADNET_INFLATE_FLAG_LAST_KNOWN) prev = unit.last_byte, have_prev = true;      // else its bytes, if any, repeat prev
    if (unit.flags & RADNET_INFLATE_FLAG_FINAL) {
      if (total != expected) return RADNET_INFLATE_CHAIN_LENGTH;
      if (((int64_t)unit.end_bit + 7) / 8 + 4 != n) return RADNET_INFLATE_CHAIN_TRAILER;
      break;
    }
    if ((int64_t)unit.end_bit <= bit) return RADNET_INFLATE_CHAIN_BAD_UNIT;      // a record no measurement gives: the walk must advance
    from = u;
    bit = unit.end_bit;
  }
  *bad_unit = -1;
  *false_count = count - written;
  return RADNET_INFLATE_CHAIN_OK;
}

extern "C" int radnet_inflate_lz_chain(const radnet_inflate_lz_unit* units, int32_t count, int64_t first_bit, int64_t n, int64_t expected,
                                       radnet_inflate_link* links, int32_t link_cap, int32_t* link_count, int32_t* false_count, int32_t* bad_unit) {
  if (!units || !links || !link_count || !false_count || !bad_unit || count < 1 || n < 1 || first_bit < 0 || expected < 0 || link_cap < 0)
    return RADNET_ERR_ARG;
  for (int32_t u = 1; u < count; ++u)
    if (units[u].start_bit <= units[u - 1].start_bit) return RADNET_ERR_ARG;
  *link_count = 0;
  *false_count = 0;
  *bad_unit = -1;
  int64_t bit = first_bit, total = 0;
  int32_t from = -1, written = 0;
  for (;;) {
    const int32_t u = find_start(units, count, bit);
    if (u < 0) {
      *bad_unit = from;
      return RADNET_INFLATE_CHAIN_NO_START;
    }
    const radnet_inflate_lz_unit& unit = units[u];
    *bad_unit = u;
    if (unit.status != RADNET_INFLATE_OK) return RADNET_INFLATE_CHAIN_BAD_UNIT;
    if ((int64_t)unit.reach > total) return RADNET_INFLATE_CHAIN_REACH;      // the guard: every source emit writes is >= total - reach >= 0
    if (written >= link_cap) return RADNET_ERR_ARG;
    links[written++] = radnet_inflate_link{total, unit.start_bit, unit.out_bytes, 0u, 0u};
    *link_count = written;
    total += unit.out_bytes;
    if (unit.flags & RADNET_INFLATE_FLAG_FINAL) {
      if (total != expected) return RADNET_INFLATE_CHAIN_LENGTH;
      if (((int64_t)unit.end_bit + 7) / 8 + 4 != n) return RADNET_INFLATE_CHAIN_TRAILER;
      break;
    }
    if ((int64_t)unit.end_bit <= bit) return RADNET_INFLATE_CHAIN_BAD_UNIT;      // a record no measurement gives: the walk must advance
    from = u;
    bit = unit.end_bit;
  }
  *bad_unit = -1;
  *false_count = count - written;
  return RADNET_INFLATE_CHAIN_OK;
}

extern "C" int radnet_png_check_crcs(const uint8_t* file, int64_t file_len, const int64_t* at, const int64_t* end, int32_t count, int32_t workers) {
  if (!file || !at || !end || count < 1 || file_len < 0) return RADNET_ERR_ARG;
  for (int32_t k = 0; k < count; ++k)
    if (at[k] < 0 || at[k] + 8 > end[k] || end[k] + 4 > file_len) return RADNET_ERR_ARG;
  crc32_of(file, 0);                              // the tables exist before the threads start
  workers = workers < 1 ? 1 : workers > 16 ? 16 : workers;
  if (workers > count) workers = count;
  std::vector<int32_t> first_bad((size_t)workers, count);
  auto run = [&](int32_t w) {
    const int32_t lo = (int32_t)((int64_t)count * w / workers), hi = (int32_t)((int64_t)count * (w + 1) / workers);
    for (int32_t k = lo; k < hi; ++k) {
      const uint8_t* c = file + end[k];
      const uint32_t stored = (uint32_t)c[0] << 24 | (uint32_t)c[1] << 16 | (uint32_t)c[2] << 8 | (uint32_t)c[3];
      if (crc32_of(file + at[k] + 4, end[k] - at[k] - 4) != stored) {
        first_bad[(size_t)w] = k;
        return;
      }
    }
  };
  std::vector<std::thread> threads;
  for (int32_t w = 1; w < workers; ++w) threads.emplace_back(run, w);
  run(0);
  for (std::thread& t : threads) t.join();
  for (int32_t w = 0; w < workers; ++w)
    if (first_bad[(size_t)w] < count) return first_bad[(size_t)w];
  return count;
}

extern "C" int radnet_inflate_streams_check(const radnet_inflate_stream* streams, int32_t count, int64_t z_len, int64_t out_len, int32_t* bad_stream,
                                            char* msg, int32_t msg_cap) {
  int code = RADNET_ERR_ARG;
  char text[200];
  text[0] = 0;
  int32_t bad = -1;
  auto refuse = [&](int32_t k) {
    if (bad_stream) *bad_stream = k;
    if (msg && msg_cap > 0) std::snprintf(msg, (size_t)msg_cap, "inflate streams: %s", text);
    return code;
  };
  if (!streams || count < 1 || count > RADNET_INFLATE_MANY_MAX_STREAMS || z_len < 0 || out_len < 0) {
    std::snprintf(text, sizeof text, "a null table, %d streams (1..%d), or buffers of %lld and %lld bytes", count, RADNET_INFLATE_MANY_MAX_STREAMS,
                  (long long)z_len, (long long)out_len);
    return refuse(bad);
  }
  if (z_len >= (1ll << 29) || out_len >= (1ll << 31)) {
    code = RADNET_ERR_UNSUPPORTED;
    std::snprintf(text, sizeof text, "%lld compressed bytes (below 2^29: global bit offsets keep 32 bits) or %lld inflated ones (below 2^31)",
                  (long long)z_len, (long long)out_len);
    return refuse(bad);
  }
  for (int32_t k = 0; k < count; ++k) {
    const radnet_inflate_stream& s = streams[k];
    if (s.z_offset < 0 || s.n < 3 || s.out_offset < 0 || s.expected < 0) {
      std::snprintf(text, sizeof text, "stream %d: z_offset %lld, n %lld (3 at least), out_offset %lld, expected %lld", k, (long long)s.z_offset,
                    (long long)s.n, (long long)s.out_offset, (long long)s.expected);
      return refuse(k);
    }
    if (s.n > z_len - s.z_offset || s.expected > out_len - s.out_offset) {      // no sum that could overflow
      std::snprintf(text, sizeof text, "stream %d: [%lld, +%lld) of %lld compressed bytes or [%lld, +%lld) of %lld inflated ones lies outside", k,
                    (long long)s.z_offset, (long long)s.n, (long long)z_len, (long long)s.out_offset, (long long)s.expected, (long long)out_len);
      return refuse(k);
    }
    if (k == 0) continue;
    const radnet_inflate_stream& f = streams[k - 1];      // f lies inside the buffers, so its ends do not overflow
    if (s.z_offset < f.z_offset || s.out_offset < f.out_offset) {
      std::snprintf(text, sizeof text, "stream %d begins in front of stream %d: the table is not sorted", k, k - 1);
      return refuse(k);
    }
    if (s.z_offset < f.z_offset + f.n || s.out_offset < f.out_offset + f.expected) {
      std::snprintf(text, sizeof text, "stream %d overlaps stream %d", k, k - 1);
      return refuse(k);
    }
  }
  if (bad_stream) *bad_stream = -1;
  return RADNET_OK;
}
