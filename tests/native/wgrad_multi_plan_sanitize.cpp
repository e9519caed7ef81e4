// Driver for the AddressSanitizer + UBSan build of csrc/wgrad_multi_plan.cpp (tests/test_wgrad_multi_plan_sanitize.py builds and runs
// it): the launch plan of radnet_conv_wgrad_multi on exactly-sized heap buffers -- prefix sums, grouping by tile shape, the 16-problem
// cap that spills into a second launch, slabs and counters that do not fit beside each other, and the refusals.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "wgrad_multi_plan.h"

static int failed = 0, checked = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    ++checked;                                                       \
    if (!(cond)) {                                                   \
      ++failed;                                                      \
      printf("FAILED line %d: %s\n", __LINE__, #cond);               \
    }                                                                \
  } while (0)

// runs the plan with the item list and the output in heap blocks of exactly their sizes
static int plan(const std::vector<WgradMultiItem>& items, uint64_t ws, unsigned ctr, std::vector<WgradMultiLaunch>& out, int cap) {
  WgradMultiItem* in = (WgradMultiItem*)malloc(sizeof(WgradMultiItem) * (items.size() ? items.size() : 1));
  if (!items.empty()) memcpy(in, items.data(), sizeof(WgradMultiItem) * items.size());
  WgradMultiLaunch* o = (WgradMultiLaunch*)malloc(sizeof(WgradMultiLaunch) * (cap ? cap : 1));
  memset(o, 0xEE, sizeof(WgradMultiLaunch) * (cap ? cap : 1));
  const int n = wgrad_multi_plan(items.empty() ? nullptr : in, (int)items.size(), ws, ctr, cap ? o : nullptr, cap);
  out.clear();
  for (int i = 0; i < n; ++i) out.push_back(o[i]);
  free(o);
  free(in);
  return n;
}

// what every plan must satisfy: each problem once, in list order inside its launch, prefix sums of its grid, aligned disjoint slabs
static void check_plan(const std::vector<WgradMultiItem>& items, const std::vector<WgradMultiLaunch>& L, uint64_t ws, unsigned ctr) {
  std::vector<int> seen(items.size(), 0);
  for (const WgradMultiLaunch& l : L) {
    CHECK(l.n >= 1 && l.n <= kWgradMultiMax && l.map.n == l.n);
    uint64_t grid = 0, slab_end = 0;
    unsigned ctr_end = 0;
    for (int k = 0; k < l.n; ++k) {
      const int i = l.problem[k];
      CHECK(i >= 0 && i < (int)items.size());
      if (i < 0 || i >= (int)items.size()) continue;
      ++seen[i];
      CHECK(k == 0 || l.problem[k - 1] < i);
      CHECK(items[i].bmk == l.bmk && items[i].bn == l.bn);
      CHECK(l.map.first[k] == grid && l.map.wx[k] == items[i].wx && l.map.wy[k] == items[i].wy);
      grid += (uint64_t)items[i].wx * items[i].wy * items[i].wz;
      CHECK(l.slab_off[k] % 256 == 0 && l.slab_off[k] >= slab_end && l.slab_off[k] + items[i].slab_bytes <= ws);
      slab_end = l.slab_off[k] + items[i].slab_bytes;
      CHECK(l.counter_off[k] == ctr_end && ctr_end + items[i].counters <= ctr);
      ctr_end += items[i].counters;
    }
    for (int k = l.n; k <= kWgradMultiMax; ++k) CHECK(l.map.first[k] == grid);
    CHECK(grid <= 0x7fffffffull);
  }
  for (size_t i = 0; i < items.size(); ++i) CHECK(seen[i] == 1);
}

int main() {
  std::vector<WgradMultiLaunch> L;
  const uint64_t ws = 1 << 20;
  const unsigned ctr = 1000;
  // nothing to do
  CHECK(plan({}, ws, ctr, L, 0) == 0);
  // the classifier's ten layers: two tile shapes interleaved -> two launches, shapes in the order of their first problem
  {
    std::vector<WgradMultiItem> it;
    for (int i = 0; i < 10; ++i) it.push_back(WgradMultiItem{64, i % 3 == 1 ? 128 : 64, 8u + i, 8, i % 2 ? 3u : 1u, i % 2 ? 1000u + 64 * i : 0u, i % 2 ? (8u + i) * 8 : 0u});
    CHECK(plan(it, ws, ctr, L, 10) == 2);
    check_plan(it, L, ws, ctr);
    CHECK(L.size() == 2 && L[0].bn == 64 && L[1].bn == 128 && L[0].n == 7 && L[1].n == 3);
    CHECK(L[0].problem[0] == 0 && L[0].problem[1] == 2 && L[1].problem[0] == 1 && L[1].problem[2] == 7);
    CHECK(L[0].map.first[1] == 8 * 8 * 1 && L[0].map.first[2] == 64 + 10 * 8 * 1);
    CHECK(plan(it, ws, ctr, L, 1) == kWgradMultiErrCap);
  }
  // 16 problems fill a launch, the 17th .. 35th spill: 16 + 16 + 3
  {
    std::vector<WgradMultiItem> it(35, WgradMultiItem{128, 64, 4, 2, 1, 0, 0});
    CHECK(plan(it, ws, ctr, L, 35) == 3);
    check_plan(it, L, ws, ctr);
    CHECK(L.size() == 3 && L[0].n == 16 && L[1].n == 16 && L[2].n == 3 && L[1].problem[0] == 16 && L[2].problem[2] == 34);
    CHECK(L[0].map.first[16] == 16 * 8 && L[2].map.first[3] == 24 && L[2].map.first[16] == 24);
    CHECK(plan(it, ws, ctr, L, 2) == kWgradMultiErrCap);
  }
  // slabs that do not fit beside each other, counters that do not: a new launch each time, offsets start again at 0
  {
    std::vector<WgradMultiItem> it{{64, 64, 2, 2, 2, 600000, 4}, {64, 64, 2, 2, 2, 600000, 4}, {64, 64, 2, 2, 2, 100, 4}, {64, 64, 1, 1, 2, 8, 999}};
    CHECK(plan(it, ws, ctr, L, 4) == 3);
    check_plan(it, L, ws, ctr);
    CHECK(L.size() == 3 && L[0].n == 1 && L[1].n == 2 && L[2].n == 1 && L[1].slab_off[0] == 0 && L[1].slab_off[1] == 600064 && L[2].counter_off[0] == 0);
    CHECK(plan(it, 600000, ctr, L, 4) == 4);      // exactly the workspace: every large one alone
    check_plan(it, L, 600000, ctr);
  }
  // a grid that would pass 2^31 - 1 workgroups closes the launch
  {
    std::vector<WgradMultiItem> it{{64, 64, 32768, 32768, 1, 0, 0}, {64, 64, 32768, 32768, 1, 0, 0}};
    CHECK(plan(it, ws, ctr, L, 2) == 2);
    check_plan(it, L, ws, ctr);
  }
  // refusals
  {
    std::vector<WgradMultiItem> big{{64, 64, 1, 1, 2, ws + 1, 1}}, many{{64, 64, 1, 1, 2, 8, ctr + 1}}, shape{{96, 64, 1, 1, 1, 0, 0}}, empty{{64, 64, 0, 1, 1, 0, 0}},
        huge{{64, 64, 65536, 65536, 1, 0, 0}};
    CHECK(plan(big, ws, ctr, L, 1) == kWgradMultiErrFit);
    CHECK(plan(many, ws, ctr, L, 1) == kWgradMultiErrFit);
    CHECK(plan(huge, ws, ctr, L, 1) == kWgradMultiErrFit);
    CHECK(plan(shape, ws, ctr, L, 1) == kWgradMultiErrArg);
    CHECK(plan(empty, ws, ctr, L, 1) == kWgradMultiErrArg);
    CHECK(wgrad_multi_plan(nullptr, 1, ws, ctr, nullptr, 0) == kWgradMultiErrArg);
    CHECK(wgrad_multi_plan(nullptr, -1, ws, ctr, nullptr, 0) == kWgradMultiErrArg);
  }
  printf("%d checked, %d failed\n", checked, failed);
  return failed ? 1 : 0;
}
