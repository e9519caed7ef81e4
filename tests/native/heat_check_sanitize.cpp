// Driver for the AddressSanitizer + UBSan build of csrc/heat_check.cpp (tests/test_heat_check_sanitize.py builds and runs it):
// radnet_heat_check on exactly-sized heap tables and message buffers, so a read past the last entry or a write past msg_cap is caught;
// the arithmetic at the ends of int32 and int64 runs under UBSan.
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

static const int kMsg = 96;

// the check on a heap copy of exactly the table's size; returns its code, *bad the entry it names
static int run(const std::vector<radnet_heat_place>& places, int64_t pool_len, int32_t h, int32_t w, int32_t* bad, int msg_cap = kMsg,
               const char* field = nullptr) {
  radnet_heat_place* table = (radnet_heat_place*)malloc(sizeof(radnet_heat_place) * (places.size() ? places.size() : 1));
  char* msg = (char*)malloc((size_t)(msg_cap > 0 ? msg_cap : 1));
  if (places.size()) memcpy(table, places.data(), sizeof(radnet_heat_place) * places.size());
  *bad = -7;
  const int rc = radnet_heat_check(places.size() ? table : nullptr, (int32_t)places.size(), pool_len, h, w, bad, msg_cap > 0 ? msg : nullptr, msg_cap);
  if (msg_cap > 0) CHECK(memchr(msg, 0, (size_t)msg_cap) != nullptr);      // always terminated inside its buffer
  if (rc == RADNET_OK && msg_cap > 0) CHECK(msg[0] == 0);
  if (rc != RADNET_OK && field && msg_cap == kMsg) CHECK(strstr(msg, field) != nullptr);
  free(msg);
  free(table);
  return rc;
}

static radnet_heat_place place(int x0, int y0, int w, int h, int mw, int mh, int64_t offset) { return radnet_heat_place{x0, y0, w, h, mw, mh, offset}; }

int main() {
  static_assert(sizeof(radnet_heat_place) == 32, "radnet_heat_place is 32 bytes");
  const int M = RADNET_DRAW_SCENE_MAX_COORD, E = RADNET_HEAT_MAX_EXTENT, K = RADNET_HEAT_MAX_MAP;
  int32_t bad;
  // the accept table: ordinary placements, overhangs on every side, one wholly outside, everything at its bound
  const std::vector<radnet_heat_place> good = {place(1, 1, 20, 10, 5, 4, 0),     place(25, 12, 8, 6, 1, 1, 20), place(-7, -3, 15, 9, 3, 2, 21),
                                               place(30, 15, 20, 20, 2047, 1, 27), place(400, 3, 5, 5, 1, 1, 0),  place(M, -M, E, E, K, K, 2074),
                                               place(-M, M, 1, 1, 1, 1, 2074 + (int64_t)K * K - 1)};
  const int64_t pool_len = 2074 + (int64_t)K * K;
  CHECK(run(good, pool_len, 21, 37, &bad) == RADNET_OK && bad == -7);
  CHECK(run(good, pool_len, 1, 1, &bad) == RADNET_OK && bad == -7);
  CHECK(run(good, INT64_MAX, INT_MAX, INT_MAX, &bad) == RADNET_OK);
  CHECK(run({}, 0, 1, 1, &bad) == RADNET_OK && bad == -7);                                    // count 0: a valid no-op
  CHECK(run(good, pool_len, 21, 37, &bad, 0) == RADNET_OK);                                   // no message buffer at all
  CHECK(radnet_heat_check(nullptr, 0, 0, 1, 1, nullptr, nullptr, 0) == RADNET_OK);
  CHECK(radnet_heat_check(nullptr, 3, 10, 1, 1, &bad, nullptr, 0) == RADNET_ERR_ARG && bad == -1);
  CHECK(radnet_heat_check(good.data(), -1, pool_len, 1, 1, &bad, nullptr, 0) == RADNET_ERR_ARG && bad == -1);
  CHECK(radnet_heat_check(good.data(), INT_MIN, pool_len, 1, 1, &bad, nullptr, 0) == RADNET_ERR_ARG && bad == -1);
  CHECK(radnet_heat_check(good.data(), 1, -1, 1, 1, &bad, nullptr, 0) == RADNET_ERR_ARG && bad == -1);
  CHECK(radnet_heat_check(good.data(), 1, INT64_MIN, 1, 1, &bad, nullptr, 0) == RADNET_ERR_ARG && bad == -1);
  CHECK(radnet_heat_check(good.data(), 1, pool_len, 0, 1, &bad, nullptr, 0) == RADNET_ERR_ARG && bad == -1);
  CHECK(radnet_heat_check(good.data(), 1, pool_len, 1, INT_MIN, &bad, nullptr, 0) == RADNET_ERR_ARG && bad == -1);
  CHECK(radnet_heat_check(good.data(), 1, 19, 1, 1, &bad, nullptr, 0) == RADNET_ERR_ARG && bad == 0);      // the first map alone needs 20 bytes
  CHECK(radnet_heat_check(good.data(), 1, 20, 1, 1, nullptr, nullptr, 0) == RADNET_OK);

  // the refuse tables: one field of one entry of the accept table replaced
  struct Case {
    int entry, field;       // field: 0..5 the int32 of that index (x0, y0, w, h, mw, mh), 6 the offset
    int64_t value;
    const char* name;
  };
  const Case cases[] = {{0, 2, 0, " w = "},          {1, 2, -1, " w = "},          {2, 2, E + 1, " w = "},          {3, 2, INT_MAX, " w = "},   {4, 2, INT_MIN, " w = "},
                        {0, 3, 0, " h = "},          {5, 3, E + 1, " h = "},       {6, 3, INT_MIN, " h = "},        {1, 3, INT_MAX, " h = "},
                        {0, 4, 0, " mw = "},         {3, 4, K + 1, " mw = "},      {2, 4, INT_MAX, " mw = "},       {1, 4, INT_MIN, " mw = "},
                        {0, 5, 0, " mh = "},         {5, 5, K + 1, " mh = "},      {4, 5, INT_MAX, " mh = "},       {6, 5, -5, " mh = "},
                        {0, 0, M + 1, " x0 = "},     {5, 0, -M - 1, " x0 = "},     {1, 0, INT_MAX, " x0 = "},       {2, 0, INT_MIN, " x0 = "},
                        {0, 1, M + 1, " y0 = "},     {6, 1, -M - 1, " y0 = "},     {3, 1, INT_MAX, " y0 = "},       {4, 1, INT_MIN, " y0 = "},
                        {0, 6, -1, " offset = "},    {1, 6, pool_len, " offset = "}, {5, 6, 2075, " offset = "},    {6, 6, pool_len, " offset = "},
                        {2, 6, INT64_MAX, " offset = "}, {3, 6, INT64_MIN, " offset = "}, {0, 6, pool_len - 19, " offset = "}};
  for (const Case& c : cases) {
    std::vector<radnet_heat_place> t = good;
    if (c.field < 6)
      ((int32_t*)&t[(size_t)c.entry])[c.field] = (int32_t)c.value;
    else
      t[(size_t)c.entry].offset = c.value;
    CHECK(run(t, pool_len, 21, 37, &bad, kMsg, c.name) == RADNET_ERR_ARG && bad == c.entry);
    CHECK(run(t, pool_len, 21, 37, &bad, 1) == RADNET_ERR_ARG && bad == c.entry);             // a message buffer of one byte
    CHECK(run(t, pool_len, 21, 37, &bad, 9) == RADNET_ERR_ARG && bad == c.entry);
    if (failed) printf("  (entry %d, field %d = %lld)\n", c.entry, c.field, (long long)c.value);
  }
  {                                                                   // a long table: the first bad entry is the one named
    std::vector<radnet_heat_place> many;
    for (int i = 0; i < 1000; ++i) many.push_back(good[(size_t)(i % 5)]);
    CHECK(run(many, pool_len, 21, 37, &bad) == RADNET_OK);
    many[998].w = 0, many[640].mh = 0;
    CHECK(run(many, pool_len, 21, 37, &bad) == RADNET_ERR_ARG && bad == 640);
  }
  printf("%d checks, %d failed\n", checked, failed);
  return failed ? 1 : 0;
}
