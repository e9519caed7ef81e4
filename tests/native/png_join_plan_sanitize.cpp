// Stand-alone driver for csrc/png_join_plan.cpp under AddressSanitizer + UBSan (tests/test_png_join_plan_sanitize.py builds and runs
// it): accept tables, one refuse table per reason and the ends of int64, on exactly sized heap tables and message buffers, so that a
// read or a write past either is caught.
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

struct Outcome {
  int rc;
  int32_t bad;
  radnet_png_join_plan plan;
  bool spoke;
};

// the table, the plan and the message each live in a heap block of exactly their size
static Outcome run(const std::vector<radnet_png_piece>& pieces, int32_t count, int64_t file_len, int64_t n, int32_t misalign, int32_t msg_cap = 200) {
  radnet_png_piece* table = pieces.empty() ? nullptr : new radnet_png_piece[pieces.size()];
  for (size_t i = 0; i < pieces.size(); ++i) table[i] = pieces[i];
  radnet_png_join_plan* plan = new radnet_png_join_plan{-7, -7};
  char* msg = msg_cap > 0 ? new char[msg_cap] : nullptr;
  if (msg) memset(msg, 'x', (size_t)msg_cap);
  int32_t* bad = new int32_t(-2);
  Outcome o;
  o.rc = radnet_png_plan_join(table, count, file_len, n, misalign, plan, bad, msg, msg_cap);
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
  static_assert(sizeof(radnet_png_piece) == 24, "the table's record");
  // ---- accept ----
  {
    Outcome o = run({}, 0, 0, 0, 0);
    CHECK(o.rc == RADNET_OK && o.bad == -1 && o.plan.grains == 0 && o.plan.spans == 0 && !o.spoke);
    o = run({{0, 0, 0}, {40, 0, 0}}, 2, 40, 0, 5);                      // empty pieces alone, one at the file's end
    CHECK(o.rc == RADNET_OK && o.plan.grains == 0 && o.plan.spans == 0);
    o = run({{8, 0, 10}, {30, 10, 0}, {30, 10, 7}, {5, 17, 3}}, 4, 40, 20, 0);      // out of order, overlapping
    CHECK(o.rc == RADNET_OK && o.plan.grains == 2 && o.plan.spans == 1);
    o = run({{0, 0, 4096}}, 1, 4096, 4096, 0);
    CHECK(o.rc == RADNET_OK && o.plan.grains == 256 && o.plan.spans == 1);
    o = run({{0, 0, 4096}}, 1, 4096, 4096, 1);                          // one byte behind a boundary: a clipped grain at each end
    CHECK(o.rc == RADNET_OK && o.plan.grains == 257 && o.plan.spans == 2);
    o = run({{0, 0, 1}}, 1, 1, 1, 15);
    CHECK(o.rc == RADNET_OK && o.plan.grains == 1 && o.plan.spans == 1);
    o = run({{0, 0, 2}}, 1, 2, 2, 15);
    CHECK(o.rc == RADNET_OK && o.plan.grains == 2);
    o = run({{3, 0, 1}}, 1, 4, 1, 0, 0);                                // no message buffer
    CHECK(o.rc == RADNET_OK);
  }
  // ---- one refuse table per reason ----
  {
    Outcome o = run({{-1, 0, 1}}, 1, 10, 1, 0);
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == 0 && o.spoke && o.plan.spans == -7 && o.plan.grains == -7);
    o = run({{0, 0, -1}}, 1, 10, 0, 0);
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == 0 && o.spoke);
    o = run({{0, 0, 10}, {11, 10, 0}}, 2, 10, 10, 0);
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == 1 && o.spoke);
    o = run({{0, 0, 10}, {0, 10, 10}, {5, 20, 6}}, 3, 10, 26, 0);
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == 2 && o.spoke);
    o = run({{0, 0, 5}, {0, 4, 5}}, 2, 10, 10, 0);                      // dst is not the sum in front of it
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == 1 && o.spoke);
    o = run({{0, 1, 5}}, 1, 10, 5, 0);
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == 0 && o.spoke);
    o = run({{0, 0, 5}, {0, 5, 5}}, 2, 10, 9, 0);                       // the total above n: the piece that passes it
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == 1 && o.spoke);
    o = run({{0, 0, 5}, {0, 5, 5}}, 2, 10, 11, 0);                      // and below
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == -1 && o.spoke);
    o = run({}, 0, 10, 1, 0);
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == -1 && o.spoke);
    o = run({{0, 0, 1}}, -1, 10, 1, 0);
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == -1 && o.spoke);
    o = run({{0, 0, 1}}, 1, -1, 1, 0);
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == -1 && o.spoke);
    o = run({{0, 0, 1}}, 1, 10, -1, 0);
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == -1 && o.spoke);
    o = run({{0, 0, 1}}, 1, 10, 1, 16);
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == -1 && o.spoke);
    o = run({{0, 0, 1}}, 1, 10, 1, -1);
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == -1 && o.spoke);
    o = run({}, 2, 10, 0, 0);                                           // a null table
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == -1 && o.spoke);
    o = run({{0, 0, 11}}, 1, 10, 11, 0, 8);                             // a message buffer shorter than the message
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == 0 && o.spoke);
    o = run({{0, 0, 11}}, 1, 10, 11, 0, 0);                             // none at all
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == 0);
    CHECK(radnet_png_plan_join(nullptr, 0, 0, 0, 0, nullptr, nullptr, nullptr, 0) == RADNET_ERR_ARG);      // a null plan, nothing to write to
  }
  // ---- the ends of int64 ----
  {
    Outcome o = run({{kMax, 0, kMax}}, 1, kMax, kMax, 0);               // src + length leaves 64 bits
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == 0);
    o = run({{kMax, 0, 1}}, 1, kMax, 1, 15);
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == 0);
    o = run({{1, 0, kMax}}, 1, kMax, kMax, 0);
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == 0);
    o = run({{kMin, 0, 0}}, 1, kMax, 0, 0);
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == 0);
    o = run({{0, 0, kMin}}, 1, kMax, 0, 0);
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == 0);
    o = run({{0, kMin, 0}}, 1, kMax, 0, 0);
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == 0);
    o = run({{0, 0, kMax}, {0, kMax, kMax}}, 2, kMax, kMax, 0);         // overlapping sources whose lengths sum past 64 bits
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == 1);
    o = run({{0, 0, 0}}, 1, kMin, 0, 0);
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == -1);
    o = run({{0, 0, 0}}, 1, 0, kMin, 0);
    CHECK(o.rc == RADNET_ERR_ARG && o.bad == -1);
    o = run({{kMax, 0, 0}}, 1, kMax, 0, 15);                            // legal: empty, at the end of the largest file
    CHECK(o.rc == RADNET_OK && o.plan.spans == 0);
    o = run({{0, 0, kMax}}, 1, kMax, kMax, 15);                         // legal bounds, misalign + n leaves int64, 2^51 spans
    CHECK(o.rc == RADNET_ERR_UNSUPPORTED && o.bad == -1 && o.spoke && o.plan.spans == -7);
    const int64_t most = (int64_t)RADNET_PNG_JOIN_MAX_SPANS * 4096;
    o = run({{0, 0, most}}, 1, kMax, most, 0);
    CHECK(o.rc == RADNET_OK && o.plan.spans == RADNET_PNG_JOIN_MAX_SPANS && o.plan.grains == most / 16);
    o = run({{0, 0, most}}, 1, kMax, most, 1);
    CHECK(o.rc == RADNET_ERR_UNSUPPORTED);
  }
  printf("%d passed, %d failed\n", passed, failed);
  return failed ? 1 : 0;
}
