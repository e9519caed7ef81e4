// Driver for the AddressSanitizer + UBSan build of radnet_inflate_lz_chain (csrc/inflate_plan.cpp; tests/test_inflate_lz_plan_sanitize.py
// builds and runs it): the chain on exactly-sized heap tables, so a read past the units or a write past the links is caught; an
// accepted table, every refusal code once with the index it names, an unsorted table, a link table too small, and the reach at 0,
// at the unit's offset and one byte beyond it.
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

static radnet_inflate_lz_unit unit(uint32_t start, uint32_t end, uint32_t out, uint32_t reach, uint32_t flags = 0, uint32_t status = RADNET_INFLATE_OK) {
  radnet_inflate_lz_unit u = {start, end, out, out, 1, status, flags, reach, reach > 1 ? 1u : 0u, 0};
  return u;
}

struct Result {
  int rc, links, false_count, bad;
  std::vector<radnet_inflate_link> table;
};

// the chain of `units` in heap tables of exactly units.size() units and link_cap links
static Result run(const std::vector<radnet_inflate_lz_unit>& units, int64_t first_bit, int64_t n, int64_t expected, int link_cap) {
  radnet_inflate_lz_unit* u = (radnet_inflate_lz_unit*)malloc(sizeof(radnet_inflate_lz_unit) * units.size());
  memcpy(u, units.data(), sizeof(radnet_inflate_lz_unit) * units.size());
  radnet_inflate_link* l = (radnet_inflate_link*)malloc(sizeof(radnet_inflate_link) * (link_cap ? link_cap : 1));
  memset(l, 0xEE, sizeof(radnet_inflate_link) * (link_cap ? link_cap : 1));
  Result r;
  int32_t links = -7, false_count = -7, bad = -7;
  r.rc = radnet_inflate_lz_chain(u, (int32_t)units.size(), first_bit, n, expected, l, link_cap, &links, &false_count, &bad);
  r.links = links, r.false_count = false_count, r.bad = bad;
  if (links > 0) r.table.assign(l, l + links);
  free(l);
  free(u);
  return r;
}

int main() {
  const uint32_t F = RADNET_INFLATE_FLAG_FINAL;
  CHECK(sizeof(radnet_inflate_lz_unit) == 40 && sizeof(radnet_inflate_link) == 24);
  // five chained units and a false candidate at bit 40; the reaches are 0, the whole offset (10), below it, 0 for an empty unit, the
  // whole offset again (35)
  std::vector<radnet_inflate_lz_unit> good = {unit(16, 100, 10, 0),  unit(40, 90, 3, 0),   unit(100, 200, 20, 10),
                                              unit(200, 300, 0, 0),  unit(300, 400, 5, 29), unit(400, 795, 8, 35, F)};
  const int64_t n = 100 + 4, total = 43;
  Result r = run(good, 16, n, total, 5);
  CHECK(r.rc == RADNET_INFLATE_CHAIN_OK && r.links == 5 && r.false_count == 1 && r.bad == -1);
  if (r.links == 5) {
    const int64_t offsets[5] = {0, 10, 30, 30, 35};
    const uint32_t starts[5] = {16, 100, 200, 300, 400}, outs[5] = {10, 20, 0, 5, 8};
    for (int i = 0; i < 5; ++i)
      CHECK(r.table[i].out_offset == offsets[i] && r.table[i].prev_byte == 0 && r.table[i].start_bit == starts[i] && r.table[i].out_bytes == outs[i] &&
            r.table[i].reserved == 0);
  }
  CHECK(run(good, 16, n, total, 4).rc == RADNET_ERR_ARG);                  // one link too few: refused, nothing behind the table
  CHECK(run(good, 16, n, total, 0).rc == RADNET_ERR_ARG);
  // the reach: out_offset passes, out_offset + 1 does not, in the first unit (offset 0) and in a later one
  std::vector<radnet_inflate_lz_unit> v = good;
  v[2].reach = 11;
  r = run(v, 16, n, total, 6);
  CHECK(r.rc == RADNET_INFLATE_CHAIN_REACH && r.bad == 2 && r.links == 1);
  v = good;
  v[0].reach = 1;
  r = run(v, 16, n, total, 6);
  CHECK(r.rc == RADNET_INFLATE_CHAIN_REACH && r.bad == 0 && r.links == 0);
  v = good;
  v[5].reach = 36;
  r = run(v, 16, n, total, 6);
  CHECK(r.rc == RADNET_INFLATE_CHAIN_REACH && r.bad == 5);
  v = good;
  v[5].reach = 32768, v[4].out_bytes = 32768 - 30;                         // the largest reach there is, met exactly by the offset
  CHECK(run(v, 16, n, 32768 + 8, 6).rc == RADNET_INFLATE_CHAIN_OK);
  v[4].out_bytes = 32768 - 31;                                             // and missed by one byte
  r = run(v, 16, n, 32768 + 7, 6);
  CHECK(r.rc == RADNET_INFLATE_CHAIN_REACH && r.bad == 5 && r.links == 4);
  v = good;
  v[1].reach = 40000;                                                      // a false candidate's reach is nobody's business
  CHECK(run(v, 16, n, total, 6).rc == RADNET_INFLATE_CHAIN_OK);
  r = run(good, 17, n, total, 6);
  CHECK(r.rc == RADNET_INFLATE_CHAIN_NO_START && r.bad == -1);
  v = good;
  v[2].end_bit = 201;
  r = run(v, 16, n, total, 6);
  CHECK(r.rc == RADNET_INFLATE_CHAIN_NO_START && r.bad == 2);
  v = good;
  v[3].status = RADNET_INFLATE_BAD_CODE;
  r = run(v, 16, n, total, 6);
  CHECK(r.rc == RADNET_INFLATE_CHAIN_BAD_UNIT && r.bad == 3);
  v[3].reach = 99;                                                         // BAD_UNIT comes before REACH
  CHECK(run(v, 16, n, total, 6).rc == RADNET_INFLATE_CHAIN_BAD_UNIT);
  r = run(good, 16, n, total + 1, 6);
  CHECK(r.rc == RADNET_INFLATE_CHAIN_LENGTH && r.bad == 5);
  r = run(good, 16, n + 1, total, 6);
  CHECK(r.rc == RADNET_INFLATE_CHAIN_TRAILER && r.bad == 5);
  v = good;
  v[4].end_bit = 300;                                                      // a unit that does not advance
  CHECK(run(v, 16, n, total, 6).rc == RADNET_INFLATE_CHAIN_BAD_UNIT);
  v = good;
  v[1].start_bit = 100;                                                    // unsorted (equal) starts
  CHECK(run(v, 16, n, total, 6).rc == RADNET_ERR_ARG);
  v = good;
  v[1].start_bit = 150, v[2].start_bit = 120;                              // unsorted (falling) starts
  CHECK(run(v, 16, n, total, 6).rc == RADNET_ERR_ARG);
  std::vector<radnet_inflate_lz_unit> one = {unit(16, 50, 4, 0, F)};
  r = run(one, 16, 7 + 4, 4, 1);
  CHECK(r.rc == RADNET_INFLATE_CHAIN_OK && r.links == 1 && r.false_count == 0);
  int32_t a, b, c;
  radnet_inflate_link l;
  CHECK(radnet_inflate_lz_chain(nullptr, 1, 16, 11, 4, &l, 1, &a, &b, &c) == RADNET_ERR_ARG);
  CHECK(radnet_inflate_lz_chain(one.data(), 0, 16, 11, 4, &l, 1, &a, &b, &c) == RADNET_ERR_ARG);
  CHECK(radnet_inflate_lz_chain(one.data(), 1, -1, 11, 4, &l, 1, &a, &b, &c) == RADNET_ERR_ARG);
  CHECK(radnet_inflate_lz_chain(one.data(), 1, 16, 0, 4, &l, 1, &a, &b, &c) == RADNET_ERR_ARG);
  CHECK(radnet_inflate_lz_chain(one.data(), 1, 16, 11, -1, &l, 1, &a, &b, &c) == RADNET_ERR_ARG);
  CHECK(radnet_inflate_lz_chain(one.data(), 1, 16, 11, 4, nullptr, 1, &a, &b, &c) == RADNET_ERR_ARG);
  CHECK(radnet_inflate_lz_chain(one.data(), 1, 16, 11, 4, &l, -1, &a, &b, &c) == RADNET_ERR_ARG);
  CHECK(radnet_inflate_lz_chain(one.data(), 1, 16, 11, 4, &l, 1, nullptr, &b, &c) == RADNET_ERR_ARG);
  CHECK(radnet_inflate_lz_chain(one.data(), 1, 16, 11, 4, &l, 1, &a, nullptr, &c) == RADNET_ERR_ARG);
  CHECK(radnet_inflate_lz_chain(one.data(), 1, 16, 11, 4, &l, 1, &a, &b, nullptr) == RADNET_ERR_ARG);
  printf("%d checked, %d failed\n", checked, failed);
  return failed ? 1 : 0;
}
