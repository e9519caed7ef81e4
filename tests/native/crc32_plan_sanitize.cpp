// Stand-alone driver for csrc/crc32_plan.cpp under AddressSanitizer + UBSan (tests/test_crc32_plan_sanitize.py builds and runs it):
// accept tables, one refuse table per bound and the ends of int64, on exactly sized heap tables and message buffers, so that a read or
// a write past either is caught; radnet_crc32_shift and radnet_crc32_combine against a bitwise sum written here.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "radnet_hip.h"

static int failed = 0, passed = 0;

#define CHECK(cond)                                                  \
  do {                                                               \
    if (cond) ++passed;                                              \
    else {                                                           \
      ++failed;                                                      \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
    }                                                                \
  } while (0)

static uint32_t bitwise_crc(const std::vector<uint8_t>& b, uint32_t crc) {
  crc = ~crc;
  for (uint8_t v : b) {
    crc ^= v;
    for (int i = 0; i < 8; ++i) crc = (crc >> 1) ^ (0xEDB88320u & (0u - (crc & 1u)));
  }
  return ~crc;
}

struct Outcome {
  int rc;
  int32_t bad;
  radnet_crc32_plan plan;
  bool spoke;
};

// the table, the plan and the message each live in a heap block of exactly their size
static Outcome run(const std::vector<radnet_crc32_segment>& segs, int32_t count, int64_t n, int32_t misalign, int32_t msg_cap = 200) {
  radnet_crc32_segment* table = segs.empty() ? nullptr : new radnet_crc32_segment[segs.size()];
  for (size_t i = 0; i < segs.size(); ++i) table[i] = segs[i];
  radnet_crc32_plan* plan = new radnet_crc32_plan{-7, -7};
  char* msg = msg_cap > 0 ? new char[msg_cap] : nullptr;
  if (msg) memset(msg, 'x', (size_t)msg_cap);
  int32_t* bad = new int32_t(-2);
  Outcome o;
  o.rc = radnet_crc32_plan_segments(table, count, n, misalign, plan, bad, msg, msg_cap);
  o.bad = *bad;
  o.plan = *plan;
  o.spoke = msg && msg[0] != 0 && memchr(msg, 0, (size_t)msg_cap) != nullptr;
  delete[] table;
  delete plan;
  delete[] msg;
  delete bad;
  return o;
}

int main() {
  const int64_t kMax = INT64_MAX, kMin = INT64_MIN;
  // ---- accept ----
  {
    Outcome o = run({}, 0, 0, 0);
    CHECK(o.rc == RADNET_OK && o.bad == -1 && o.plan.spans == 0 && o.plan.ws_bytes == 4 && !o.spoke);
    o = run({{0, 0, 0, 0}, {10, 0, 0, 0}}, 2, 10, 5);
    CHECK(o.rc == RADNET_OK && o.plan.spans == 0 && o.plan.ws_bytes == 12);
    // 100 bytes from 3 behind a boundary: the body ends at 96, 6 grains, one span; 12288 bytes from 8: 768 grains, 3 spans
    o = run({{0, 100, 0, 0}, {5, 12288, 1, 2}, {100, 0, 3, 4}}, 3, 20000, 3);
    CHECK(o.rc == RADNET_OK && o.plan.spans == 4 && o.plan.ws_bytes == 4 * (3 + 1 + 4));
    o = run({{0, 15, 0, 0}}, 1, 15, 0);                       // no 16-byte boundary inside: all tail
    CHECK(o.rc == RADNET_OK && o.plan.spans == 0);
    o = run({{0, 16, 0, 0}, {0, 4096, 0, 0}, {0, 4097, 0, 0}, {1, 4096, 0, 0}}, 4, 4097, 0);
    CHECK(o.rc == RADNET_OK && o.plan.spans == 1 + 1 + 1 + 1);
    o = run({{0, 4097, 0, 0}}, 1, 4097, 15);                  // 15 + 4097 = 4112 = 257 * 16: 257 grains
    CHECK(o.rc == RADNET_OK && o.plan.spans == 2);
    o = run({{7, 3, 0, 0}, {7, 3, 0, 0}, {0, 10, 0, 0}}, 3, 10, 9);      // overlapping, out of order
    CHECK(o.rc == RADNET_OK);
    o = run({{10, 0, 0, 0}}, 1, 10, 0);                       // an empty segment at the very end
    CHECK(o.rc == RADNET_OK);
    o = run({{0, 0, 0, 0}}, 1, 0, 0, 0);                      // no message buffer
    CHECK(o.rc == RADNET_OK);
  }
  // ---- one refuse table per bound ----
  {
    Outcome o = run({{-1, 1, 0, 0}}, 1, 10, 0);
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == 0 && o.spoke && o.plan.spans == -7);
    o = run({{0, -1, 0, 0}}, 1, 10, 0);
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == 0 && o.spoke);
    o = run({{0, 10, 0, 0}, {11, 0, 0, 0}}, 2, 10, 0);
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == 1 && o.spoke);
    o = run({{0, 10, 0, 0}, {0, 10, 0, 0}, {5, 6, 0, 0}}, 3, 10, 0);
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == 2 && o.spoke);
    o = run({{0, 1, 0, 0}}, -1, 10, 0);
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == -1 && o.spoke);
    o = run({{0, 1, 0, 0}}, 1, -1, 0);
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == -1 && o.spoke);
    o = run({{0, 1, 0, 0}}, 1, 10, 16);
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == -1 && o.spoke);
    o = run({{0, 1, 0, 0}}, 1, 10, -1);
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == -1 && o.spoke);
    o = run({}, 2, 10, 0);                                    // a null table
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == -1 && o.spoke);
    o = run({{0, 11, 0, 0}}, 1, 10, 0, 8);                    // a message buffer shorter than the message
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == 0 && o.spoke);
    o = run({{0, 11, 0, 0}}, 1, 10, 0, 0);                    // none at all
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == 0);
    CHECK(radnet_crc32_plan_segments(nullptr, 0, 0, 0, nullptr, nullptr, nullptr, 0) == RADNET_ERR_ARG);      // a null plan, nothing to write to
  }
  // ---- the ends of int64 ----
  {
    Outcome o = run({{kMax, kMax, 0, 0}}, 1, kMax, 0);         // offset + length leaves 64 bits
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == 0);
    o = run({{kMax, 1, 0, 0}}, 1, kMax, 15);
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == 0);
    o = run({{1, kMax, 0, 0}}, 1, kMax, 0);
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == 0);
    o = run({{kMin, 0, 0, 0}}, 1, kMax, 0);
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == 0);
    o = run({{0, kMin, 0, 0}}, 1, kMax, 0);
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == 0);
    o = run({{kMin, kMin, 0, 0}}, 1, kMax, 0);
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == 0);
    o = run({{0, 0, 0, 0}}, 1, kMin, 0);
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == -1);
    o = run({{kMax, 0, 0xFFFFFFFFu, 0xFFFFFFFFu}}, 1, kMax, 15);      // legal: empty, at the end of the largest buffer
    CHECK(o.rc == RADNET_OK && o.plan.spans == 0);
    o = run({{0, kMax, 0, 0}}, 1, kMax, 15);                  // legal bounds, but 2^51 spans
    CHECK(o.rc == RADNET_ERR_UNSUPPORTED && o.bad == 0 && o.spoke);
    o = run({{0, (int64_t)RADNET_CRC32_MAX_SPANS * 4096, 0, 0}}, 1, kMax, 0);
    CHECK(o.rc == RADNET_OK && o.plan.spans == RADNET_CRC32_MAX_SPANS);
    o = run({{0, (int64_t)RADNET_CRC32_MAX_SPANS * 4096, 0, 0}, {0, 16, 0, 0}}, 2, kMax, 0);
    CHECK(o.rc == RADNET_ERR_UNSUPPORTED && o.bad == 1);
  }
  // ---- the GF(2) helpers ----
  {
    CHECK(radnet_crc32_shift(0) == 0x80000000u && radnet_crc32_shift(-1) == 0x80000000u && radnet_crc32_shift(kMin) == 0x80000000u);
    CHECK(radnet_crc32_shift(1) == 0x00800000u && radnet_crc32_shift(4) == 0xEDB88320u);      // x^32 = P
    (void)radnet_crc32_shift(kMax);
    std::vector<uint8_t> a(1000), b(777), ab;
    uint32_t s = 12345;
    for (auto* v : {&a, &b})
      for (uint8_t& x : *v) x = (uint8_t)((s = s * 1664525u + 1013904223u) >> 24);
    ab = a;
    ab.insert(ab.end(), b.begin(), b.end());
    CHECK(bitwise_crc(std::vector<uint8_t>{'1', '2', '3', '4', '5', '6', '7', '8', '9'}, 0) == 0xCBF43926u);
    CHECK(radnet_crc32_combine(bitwise_crc(a, 0), bitwise_crc(b, 0), (int64_t)b.size()) == bitwise_crc(ab, 0));
    CHECK(radnet_crc32_combine(bitwise_crc(a, 0), 0, 0) == bitwise_crc(a, 0));
    CHECK(radnet_crc32_combine(0x12345678u, 0x9ABCDEF0u, -3) == 0x12345678u && radnet_crc32_combine(0x12345678u, 0x9ABCDEF0u, kMin) == 0x12345678u);
    (void)radnet_crc32_combine(0xFFFFFFFFu, 0xFFFFFFFFu, kMax);
    // zlib.crc32(B, c0) = pure(B) ^ (c0 ^ ~0) * x^(8 |B|) ^ ~0, with the product written as a combine of (c0 ^ ~0) in front of zeros
    const uint32_t c0 = 0x35AF061Eu;
    const std::vector<uint8_t> zeros(b.size(), 0);
    CHECK((bitwise_crc(b, c0) ^ bitwise_crc(b, 0)) == (bitwise_crc(zeros, c0) ^ bitwise_crc(zeros, 0)));
  }
  printf("%d passed, %d failed\n", passed, failed);
  return failed ? 1 : 0;
}
