// Driver for the AddressSanitizer + UBSan build of csrc/scan_merge_check.cpp (tests/test_scan_merge_check_sanitize.py builds and
// runs it): radnet_scan_merge_check on exactly-sized heap tables and message buffers, so a read past the last entry or a write past
// msg_cap is caught; the arithmetic at the ends of int32 and int64 runs under UBSan.
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "radnet_hip.h"

static int failed = 0, checked = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    ++checked;                                                       \
    if (!(cond)) {                                                   \
      ++failed;                                                      \
      printf("FAILED line %d: %s\n", __LINE__, #cond);               \
    }                                                                \
  } while (0)

static const int kMsg = 128;

// the check on a heap copy of exactly `count` entries of the table (count may be below its size: a truncated table)
static int run(const std::vector<radnet_scan_tile>& tiles, int64_t pool_words, int32_t slot_rows, int32_t* n_images, int32_t* bad, int msg_cap = kMsg,
               const char* field = nullptr, int count = -1) {
  const size_t n = count < 0 ? tiles.size() : (size_t)count;
  radnet_scan_tile* table = (radnet_scan_tile*)malloc(sizeof(radnet_scan_tile) * (n ? n : 1));
  char* msg = (char*)malloc((size_t)(msg_cap > 0 ? msg_cap : 1));
  if (n) memcpy(table, tiles.data(), sizeof(radnet_scan_tile) * n);
  *bad = -7;
  *n_images = -7;
  const int rc = radnet_scan_merge_check(n ? table : nullptr, (int32_t)n, pool_words, slot_rows, n_images, bad, msg_cap > 0 ? msg : nullptr, msg_cap);
  if (msg_cap > 0) CHECK(memchr(msg, 0, (size_t)msg_cap) != nullptr);      // always terminated inside its buffer
  if (rc == RADNET_OK && msg_cap > 0) CHECK(msg[0] == 0);
  if (rc != RADNET_OK && field && msg_cap == kMsg) CHECK(strstr(msg, field) != nullptr);
  if (rc != RADNET_OK) CHECK(*n_images == 0);
  free(msg);
  free(table);
  return rc;
}

int main() {
  static_assert(sizeof(radnet_scan_tile) == 16, "radnet_scan_tile is 16 bytes");
  const int M = RADNET_SCAN_MAX_COORD;
  const int rows = 300;
  const int64_t sw = 8 + 6 * rows;                                  // 1808 words per slot
  int32_t bad, ni;
  // the accept table: slots in no particular order, touching but not overlapping; three images, one without a gap, offsets at their bounds
  const std::vector<radnet_scan_tile> good = {{(int32_t)(2 * sw), 0, 0, 0}, {0, 250, 0, 0}, {(int32_t)sw, -M, M, 1}, {(int32_t)(4 * sw), M, -M, 1},
                                              {(int32_t)(3 * sw), 0, 0, 3}};
  const int64_t pool = 5 * sw;
  CHECK(run(good, pool, rows, &ni, &bad) == RADNET_OK && bad == -7 && ni == 4);
  CHECK(run(good, INT64_MAX, rows, &ni, &bad) == RADNET_OK && ni == 4);
  CHECK(run(good, pool, rows, &ni, &bad, 0) == RADNET_OK);                                     // no message buffer at all
  CHECK(run(good, pool, rows, &ni, &bad, kMsg, nullptr, 2) == RADNET_OK && ni == 1);           // a truncated table: two entries read, no more
  CHECK(run({}, 0, 1, &ni, &bad) == RADNET_OK && bad == -7 && ni == 0);                        // no tiles: a valid no-op
  CHECK(radnet_scan_merge_check(nullptr, 0, 0, 1, nullptr, nullptr, nullptr, 0) == RADNET_OK);
  CHECK(radnet_scan_merge_check(good.data(), 5, pool, rows, nullptr, nullptr, nullptr, 0) == RADNET_OK);
  // the arguments themselves
  CHECK(radnet_scan_merge_check(nullptr, 3, pool, rows, &ni, &bad, nullptr, 0) == RADNET_ERR_ARG && bad == -1);
  CHECK(radnet_scan_merge_check(good.data(), -1, pool, rows, &ni, &bad, nullptr, 0) == RADNET_ERR_ARG && bad == -1);
  CHECK(radnet_scan_merge_check(good.data(), INT_MIN, pool, rows, &ni, &bad, nullptr, 0) == RADNET_ERR_ARG && bad == -1);
  CHECK(radnet_scan_merge_check(good.data(), INT_MAX, pool, rows, &ni, &bad, nullptr, 0) == RADNET_ERR_ARG && bad == -1);      // huge counts: refused before
  CHECK(radnet_scan_merge_check(good.data(), RADNET_SCAN_MAX_TILES + 1, pool, rows, &ni, &bad, nullptr, 0) == RADNET_ERR_ARG && bad == -1);   // a read
  CHECK(radnet_scan_merge_check(good.data(), 5, -1, rows, &ni, &bad, nullptr, 0) == RADNET_ERR_ARG && bad == -1);
  CHECK(radnet_scan_merge_check(good.data(), 5, INT64_MIN, rows, &ni, &bad, nullptr, 0) == RADNET_ERR_ARG && bad == -1);
  CHECK(radnet_scan_merge_check(good.data(), 5, pool, 0, &ni, &bad, nullptr, 0) == RADNET_ERR_ARG && bad == -1);
  CHECK(radnet_scan_merge_check(good.data(), 5, pool, INT_MIN, &ni, &bad, nullptr, 0) == RADNET_ERR_ARG && bad == -1);
  CHECK(radnet_scan_merge_check(good.data(), 5, INT64_MAX, INT_MAX, &ni, &bad, nullptr, 0) == RADNET_ERR_ARG && bad == -1);
  CHECK(radnet_scan_merge_check(good.data(), 5, INT64_MAX, RADNET_SCAN_MAX_BOXES / 4, &ni, &bad, nullptr, 0) == RADNET_ERR_ARG && bad == -1);   // 5 tiles of it
  CHECK(run(good, pool - 1, rows, &ni, &bad, kMsg, " slot = ") == RADNET_ERR_ARG && bad == 3);   // the pool one word short: the last slot leaves it
  CHECK(run(good, 0, rows, &ni, &bad, kMsg, " slot = ") == RADNET_ERR_ARG && bad == 0);

  // the refuse tables: one field of one entry of the accept table replaced
  struct Case {
    int entry, field;       // 0 slot, 1 ox, 2 oy, 3 image
    int64_t value;
    int bad;
    const char* name;
  };
  const Case cases[] = {{1, 0, -2, 1, " slot = "},          {1, 0, INT_MIN, 1, " slot = "},   {2, 0, INT_MAX, 2, " slot = "},     {0, 0, 1, 0, " slot = "},
                        {4, 0, pool, 4, " slot = "},        {4, 0, pool - sw + 2, 4, " slot = "},                                  // out of range
                        {1, 0, sw - 2, 2, " overlaps "},    {3, 0, 2 * sw, 3, " overlaps "},  {0, 0, 0, 1, " overlaps "},          // overlapping (the later entry)
                        {4, 0, 2 * sw + 6, 4, " overlaps "},
                        {3, 3, 0, 3, " image = "},          {1, 3, -1, 1, " image = "},       {4, 3, 0, 4, " image = "},           // decreasing / negative
                        {4, 3, RADNET_SCAN_MAX_IMAGES, 4, " image = "},                        {0, 3, INT_MAX, 0, " image = "},    {3, 3, INT_MIN, 3, " image = "},
                        {0, 1, M + 1, 0, " ox = "},         {2, 1, -M - 1, 2, " ox = "},      {3, 1, INT_MAX, 3, " ox = "},        {4, 1, INT_MIN, 4, " ox = "},
                        {0, 2, M + 1, 0, " oy = "},         {2, 2, -M - 1, 2, " oy = "},      {3, 2, INT_MAX, 3, " oy = "},        {1, 2, INT_MIN, 1, " oy = "}};
  for (const Case& c : cases) {
    std::vector<radnet_scan_tile> t = good;
    ((int32_t*)&t[(size_t)c.entry])[c.field] = (int32_t)c.value;
    CHECK(run(t, pool, rows, &ni, &bad, kMsg, c.name) == RADNET_ERR_ARG && bad == c.bad);
    CHECK(run(t, pool, rows, &ni, &bad, 1) == RADNET_ERR_ARG && bad == c.bad);               // a message buffer of one byte
    CHECK(run(t, pool, rows, &ni, &bad, 9) == RADNET_ERR_ARG && bad == c.bad);
    if (failed) printf("  (entry %d, field %d = %lld, named %d)\n", c.entry, c.field, (long long)c.value, bad);
  }
  {                                                                   // a long table: the first bad entry is the one named
    std::vector<radnet_scan_tile> many;
    for (int i = 0; i < 4000; ++i) many.push_back(radnet_scan_tile{(int32_t)(((i * 7919) % 4000) * 20), i, -i, i / 40});
    CHECK(run(many, 4000 * 20, 2, &ni, &bad) == RADNET_OK && ni == 100);
    many[3998].ox = M + 1, many[640].slot = many[12].slot + 10;
    CHECK(run(many, 4000 * 20, 2, &ni, &bad) == RADNET_ERR_ARG && bad == 3998);              // the per-entry checks come first
    many[3998].ox = 0;
    CHECK(run(many, 4000 * 20, 2, &ni, &bad) == RADNET_ERR_ARG && bad == 640);
  }
  printf("%d checks, %d failed\n", checked, failed);
  return failed ? 1 : 0;
}
