// Driver for the AddressSanitizer + UBSan build of csrc/inflate_plan.cpp (tests/test_inflate_plan_sanitize.py builds and runs it):
// radnet_inflate_chain on exactly-sized heap tables, so a read past the units or a write past the links is caught; every refusal
// code once, with the index it names; radnet_png_check_crcs on an exactly-sized file.
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

static radnet_inflate_unit unit(uint32_t start, uint32_t end, uint32_t out, uint32_t flags, uint32_t last, uint32_t status = RADNET_INFLATE_OK) {
  radnet_inflate_unit u = {start, end, out, out, 1, status, flags, last};
  return u;
}

struct Result {
  int rc, links, false_count, bad;
  std::vector<radnet_inflate_link> table;
};

// the chain of `units` in heap tables of exactly units.size() units and link_cap links
static Result run(const std::vector<radnet_inflate_unit>& units, int64_t first_bit, int64_t n, int64_t expected, int link_cap) {
  radnet_inflate_unit* u = (radnet_inflate_unit*)malloc(sizeof(radnet_inflate_unit) * units.size());
  memcpy(u, units.data(), sizeof(radnet_inflate_unit) * units.size());
  radnet_inflate_link* l = (radnet_inflate_link*)malloc(sizeof(radnet_inflate_link) * (link_cap ? link_cap : 1));
  memset(l, 0xEE, sizeof(radnet_inflate_link) * (link_cap ? link_cap : 1));
  Result r;
  int32_t links = -7, false_count = -7, bad = -7;
  r.rc = radnet_inflate_chain(u, (int32_t)units.size(), first_bit, n, expected, l, link_cap, &links, &false_count, &bad);
  r.links = links, r.false_count = false_count, r.bad = bad;
  if (links > 0) r.table.assign(l, l + links);
  free(l);
  free(u);
  return r;
}

int main() {
  const uint32_t F = RADNET_INFLATE_FLAG_FINAL, M = RADNET_INFLATE_FLAG_LEAD_MATCH, K = RADNET_INFLATE_FLAG_LAST_KNOWN;
  // five units and a false candidate at bit 40: a literal unit, two units of matches alone, an empty one, the final one
  std::vector<radnet_inflate_unit> good = {unit(16, 100, 10, K, 7), unit(40, 90, 3, K, 1), unit(100, 200, 20, M, 0), unit(200, 300, 0, 0, 0),
                                           unit(300, 400, 5, M, 0), unit(400, 795, 8, M | K | F, 9)};
  const int64_t n = 100 + 4, total = 43;
  Result r = run(good, 16, n, total, 5);
  CHECK(r.rc == RADNET_INFLATE_CHAIN_OK && r.links == 5 && r.false_count == 1 && r.bad == -1);
  if (r.links == 5) {
    const int64_t offsets[5] = {0, 10, 30, 30, 35};
    const uint32_t prevs[5] = {0, 7, 7, 7, 7}, starts[5] = {16, 100, 200, 300, 400};
    for (int i = 0; i < 5; ++i)
      CHECK(r.table[i].out_offset == offsets[i] && r.table[i].prev_byte == prevs[i] && r.table[i].start_bit == starts[i] && r.table[i].reserved == 0);
  }
  CHECK(run(good, 16, n, total, 4).rc == RADNET_ERR_ARG);                  // one link too few: refused, nothing behind the table
  CHECK(run(good, 16, n, total, 0).rc == RADNET_ERR_ARG);
  r = run(good, 17, n, total, 6);
  CHECK(r.rc == RADNET_INFLATE_CHAIN_NO_START && r.bad == -1);
  std::vector<radnet_inflate_unit> v = good;
  v[2].end_bit = 201;
  r = run(v, 16, n, total, 6);
  CHECK(r.rc == RADNET_INFLATE_CHAIN_NO_START && r.bad == 2);
  v = good;
  v[3].status = RADNET_INFLATE_NOT_RLE;
  r = run(v, 16, n, total, 6);
  CHECK(r.rc == RADNET_INFLATE_CHAIN_BAD_UNIT && r.bad == 3);
  v = good;
  v[0].flags = M;
  r = run(v, 16, n, total, 6);
  CHECK(r.rc == RADNET_INFLATE_CHAIN_LEAD_MATCH && r.bad == 0);
  v = good;
  v[0] = unit(16, 100, 0, 0, 0);                                           // an empty first unit: the match behind it has nothing in front
  r = run(v, 16, n, total - 10, 6);
  CHECK(r.rc == RADNET_INFLATE_CHAIN_LEAD_MATCH && r.bad == 2);
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
  std::vector<radnet_inflate_unit> one = {unit(16, 50, 4, K | F, 3)};
  r = run(one, 16, 7 + 4, 4, 1);
  CHECK(r.rc == RADNET_INFLATE_CHAIN_OK && r.links == 1 && r.false_count == 0);
  int32_t a, b, c;
  radnet_inflate_link l;
  CHECK(radnet_inflate_chain(nullptr, 1, 16, 11, 4, &l, 1, &a, &b, &c) == RADNET_ERR_ARG);
  CHECK(radnet_inflate_chain(one.data(), 0, 16, 11, 4, &l, 1, &a, &b, &c) == RADNET_ERR_ARG);
  CHECK(radnet_inflate_chain(one.data(), 1, -1, 11, 4, &l, 1, &a, &b, &c) == RADNET_ERR_ARG);
  CHECK(radnet_inflate_chain(one.data(), 1, 16, 11, -1, &l, 1, &a, &b, &c) == RADNET_ERR_ARG);
  CHECK(radnet_inflate_chain(one.data(), 1, 16, 11, 4, nullptr, 1, &a, &b, &c) == RADNET_ERR_ARG);
  CHECK(radnet_inflate_chain(one.data(), 1, 16, 11, 4, &l, 1, nullptr, &b, &c) == RADNET_ERR_ARG);
  // radnet_png_check_crcs on an exactly-sized file of IEND chunks (CRC AE 42 60 82), on one thread and on more threads than chunks
  const int chunks = 37;
  uint8_t* file = (uint8_t*)malloc(12 * chunks);
  std::vector<int64_t> at, end;
  for (int k = 0; k < chunks; ++k) {
    const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
    memcpy(file + 12 * k, iend, 12);
    at.push_back(12 * k), end.push_back(12 * k + 8);
  }
  for (int workers : {1, 3, 16, 64}) CHECK(radnet_png_check_crcs(file, 12 * chunks, at.data(), end.data(), chunks, workers) == chunks);
  file[12 * 20 + 5] ^= 1;
  file[12 * 30 + 11] ^= 1;
  for (int workers : {1, 4, 16}) CHECK(radnet_png_check_crcs(file, 12 * chunks, at.data(), end.data(), chunks, workers) == 20);
  CHECK(radnet_png_check_crcs(file, 12 * chunks, at.data(), end.data(), 20, 5) == 20);
  CHECK(radnet_png_check_crcs(file, 12 * chunks - 1, at.data(), end.data(), chunks, 2) == RADNET_ERR_ARG);      // the last CRC would be read past the file
  CHECK(radnet_png_check_crcs(nullptr, 12 * chunks, at.data(), end.data(), chunks, 2) == RADNET_ERR_ARG);
  CHECK(radnet_png_check_crcs(file, 12 * chunks, at.data(), end.data(), 0, 2) == RADNET_ERR_ARG);
  end[3] = at[3] + 7;
  CHECK(radnet_png_check_crcs(file, 12 * chunks, at.data(), end.data(), chunks, 2) == RADNET_ERR_ARG);
  free(file);
  printf("%d checked, %d failed\n", checked, failed);
  return failed ? 1 : 0;
}
