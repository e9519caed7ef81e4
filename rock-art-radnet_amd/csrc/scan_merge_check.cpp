// ---- host side of the scan merge (scan_tail.hip): the tile table's validation -----------------------------------------------------------
// No device call and no HIP header: compiled by g++, runs without a GPU (contract: include/radnet_hip.h).  radnet_scan_merge calls
// this before it launches; tests/native/scan_merge_check_sanitize.cpp runs it under ASan + UBSan on exactly sized tables.
#include <stdarg.h>
#include <stdio.h>
#include <algorithm>
#include <vector>
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

bool beyond(int32_t v) { return v < -RADNET_SCAN_MAX_COORD || v > RADNET_SCAN_MAX_COORD; }

}  // namespace

extern "C" int radnet_scan_merge_check(const radnet_scan_tile* tiles, int32_t n_tiles, int64_t pool_words, int32_t slot_rows, int32_t* n_images,
                                       int32_t* bad_entry, char* msg, int32_t msg_cap) {
  if (msg && msg_cap > 0) msg[0] = 0;
  if (n_images) *n_images = 0;
  if (n_tiles < 0 || n_tiles > RADNET_SCAN_MAX_TILES)
    return refuse(-1, bad_entry, msg, msg_cap, "scan_merge: %d tiles, outside 0..%d", n_tiles, RADNET_SCAN_MAX_TILES);
  if (pool_words < 0) return refuse(-1, bad_entry, msg, msg_cap, "scan_merge: a pool of %lld words", (long long)pool_words);
  if (slot_rows < 1 || slot_rows > RADNET_SCAN_MAX_BOXES) return refuse(-1, bad_entry, msg, msg_cap, "scan_merge: slots of %d rows", slot_rows);
  if ((int64_t)n_tiles * slot_rows > RADNET_SCAN_MAX_BOXES)
    return refuse(-1, bad_entry, msg, msg_cap, "scan_merge: %d tiles of %d rows are more than %d boxes", n_tiles, slot_rows, RADNET_SCAN_MAX_BOXES);
  if (n_tiles == 0) return RADNET_OK;
  if (!tiles) return refuse(-1, bad_entry, msg, msg_cap, "scan_merge: a null table of %d tiles", n_tiles);
  const int64_t slot_words = 8 + (int64_t)6 * slot_rows;             // radnet_detect_tail_out_bytes(slot_rows) / 4: below 2^29
  int32_t image = 0;
  for (int32_t i = 0; i < n_tiles; ++i) {
    const radnet_scan_tile& t = tiles[i];
    if (t.slot < 0 || (t.slot & 1) || (int64_t)t.slot > pool_words - slot_words)       // pool_words - slot_words cannot overflow
      return refuse(i, bad_entry, msg, msg_cap, "scan_merge: entry %d has slot = %d (even, a slot of %lld words in a pool of %lld)", i, t.slot,
                    (long long)slot_words, (long long)pool_words);
    if (t.image < 0 || t.image >= RADNET_SCAN_MAX_IMAGES)
      return refuse(i, bad_entry, msg, msg_cap, "scan_merge: entry %d has image = %d, outside 0..%d", i, t.image, RADNET_SCAN_MAX_IMAGES - 1);
    if (t.image < image) return refuse(i, bad_entry, msg, msg_cap, "scan_merge: entry %d has image = %d after %d", i, t.image, image);
    image = t.image;
    if (beyond(t.ox)) return refuse(i, bad_entry, msg, msg_cap, "scan_merge: entry %d has ox = %d, beyond +-%d", i, t.ox, RADNET_SCAN_MAX_COORD);
    if (beyond(t.oy)) return refuse(i, bad_entry, msg, msg_cap, "scan_merge: entry %d has oy = %d, beyond +-%d", i, t.oy, RADNET_SCAN_MAX_COORD);
  }
  // no two slots overlap: by slot start, every slot ends before the next begins; the entry named is the later one of the table
  std::vector<int32_t> by(static_cast<size_t>(n_tiles));
  for (int32_t i = 0; i < n_tiles; ++i) by[(size_t)i] = i;
  std::sort(by.begin(), by.end(), [&](int32_t a, int32_t b) { return tiles[a].slot != tiles[b].slot ? tiles[a].slot < tiles[b].slot : a < b; });
  int32_t bad = -1;
  for (int32_t k = 1; k < n_tiles; ++k) {
    const int32_t a = by[(size_t)k - 1], b = by[(size_t)k];
    if ((int64_t)tiles[a].slot + slot_words > (int64_t)tiles[b].slot) {
      const int32_t later = a > b ? a : b;
      if (bad < 0 || later < bad) bad = later;
    }
  }
  if (bad >= 0) return refuse(bad, bad_entry, msg, msg_cap, "scan_merge: entry %d has slot = %d, which overlaps the slot of an earlier entry", bad, tiles[bad].slot);
  if (n_images) *n_images = image + 1;
  return RADNET_OK;
}
