// Driver for the AddressSanitizer + UBSan build of csrc/png_plan.cpp (tests/test_png_segments_host.py builds and runs it):
// radnet_png_plan_segments on exactly-sized heap buffers, so a read past the last scanline or a write past `cap` entries is caught.
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

// a pass of `rows` scanlines in a buffer of exactly rows * (1 + rowbytes) bytes with the given filter-type column
static uint8_t* make_pass(const std::vector<int>& types, int rowbytes) {
  const size_t pitch = 1 + (size_t)rowbytes;
  uint8_t* p = (uint8_t*)malloc(types.size() * pitch);
  memset(p, 0xEE, types.size() * pitch);          // sample bytes that would be illegal filter types if read as such
  for (size_t r = 0; r < types.size(); ++r) p[r * pitch] = (uint8_t)types[r];
  return p;
}

// the segments tile the rows in order, every first row is a legal cut, the offsets follow
static void check_tiling(const std::vector<int>& types, int rowbytes, int64_t off, const radnet_png_segment* seg, int n) {
  int64_t row = 0;
  for (int i = 0; i < n; ++i) {
    CHECK(seg[i].rows > 0 && seg[i].rowbytes == rowbytes);
    CHECK(seg[i].offset == off + row * (1 + (int64_t)rowbytes));
    CHECK(row == 0 || types[(size_t)row] <= 1);
    row += seg[i].rows;
  }
  CHECK(row == (int64_t)types.size());
}

static int plan(const std::vector<int>& types, int rowbytes, int64_t off, int target, int cap, int expect_min, int expect_max) {
  uint8_t* pass = make_pass(types, rowbytes);
  radnet_png_segment* out = (radnet_png_segment*)malloc(sizeof(radnet_png_segment) * (size_t)cap);      // exactly cap entries
  const int n = radnet_png_plan_segments(pass, off, (int32_t)types.size(), rowbytes, target, out, cap);
  CHECK(n >= expect_min && n <= expect_max && n <= cap);
  if (n > 0) check_tiling(types, rowbytes, off, out, n);
  free(out);
  free(pass);
  return n;
}

int main() {
  static_assert(sizeof(radnet_png_segment) == 16, "radnet_png_segment is 16 bytes");
  std::vector<int> none200(200, 0), paeth200(200, 4), mixed;
  unsigned s = 12345;
  for (int r = 0; r < 777; ++r) {
    s = s * 1664525u + 1013904223u;
    mixed.push_back((int)((s >> 24) % 5));
  }
  plan(std::vector<int>(1, 0), 1, 0, 0, 1, 1, 1);                     // rows = 1
  plan(std::vector<int>(1, 4), 7, 99, 64, 1, 1, 1);                   // rows = 1, Paeth, cap = 1
  plan(none200, 5, 0, 0, 1, 1, 1);                                    // cap = 1: everything merges into one segment
  plan(mixed, 3, 1000, 0, 1, 1, 1);
  plan(none200, 5, 16, 0, 4, 4, 4);                                   // 200 / 64 -> 4 segments: a table exactly at capacity
  plan(none200, 5, 16, 0, 3, 3, 3);                                   // one fewer: merged, never an error
  plan(none200, 5, 16, 1, 200, 200, 200);                             // target 1: one segment per row, exactly at capacity
  plan(paeth200, 9, 0, 0, 8, 1, 1);                                   // no legal cut: one segment
  const int full = plan(mixed, 3, 1000, 16, 777, 2, 777);
  plan(mixed, 3, 1000, 16, full, full, full);                         // exactly at capacity
  plan(mixed, 3, 1000, 16, full - 1, full - 1, full - 1);
  plan(mixed, 3, 1000, 16, 2, 2, 2);
  {                                                                   // errors: nothing is written
    std::vector<int> bad(10, 2);
    bad[9] = 5;
    uint8_t* pass = make_pass(bad, 4);
    radnet_png_segment out[2];
    memset(out, 0x5A, sizeof(out));
    radnet_png_segment before[2];
    memcpy(before, out, sizeof(out));
    CHECK(radnet_png_plan_segments(pass, 0, 10, 4, 0, out, 2) == RADNET_ERR_ARG);
    CHECK(radnet_png_plan_segments(pass, 0, 9, 4, 0, out, 0) == RADNET_ERR_ARG);
    CHECK(radnet_png_plan_segments(pass, -1, 9, 4, 0, out, 2) == RADNET_ERR_ARG);
    CHECK(radnet_png_plan_segments(pass, 0, 0, 4, 0, out, 2) == RADNET_ERR_ARG);
    CHECK(radnet_png_plan_segments(pass, 0, 9, 0, 0, out, 2) == RADNET_ERR_ARG);
    CHECK(radnet_png_plan_segments(pass, 0, 9, 4, -1, out, 2) == RADNET_ERR_ARG);
    CHECK(radnet_png_plan_segments(nullptr, 0, 9, 4, 0, out, 2) == RADNET_ERR_ARG);
    CHECK(radnet_png_plan_segments(pass, 0, 9, 4, 0, nullptr, 2) == RADNET_ERR_ARG);
    CHECK(memcmp(before, out, sizeof(out)) == 0);
    CHECK(radnet_png_plan_segments(pass, 0, 9, 4, 0, out, 2) == 1);   // without the bad row
    free(pass);
  }
  printf("%d checks, %d failed\n", checked, failed);
  return failed ? 1 : 0;
}
