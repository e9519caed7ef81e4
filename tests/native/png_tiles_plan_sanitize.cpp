// Driver for the AddressSanitizer + UBSan build of csrc/png_plan.cpp (tests/test_png_tiles_host.py builds and runs it):
// radnet_png_plan_tiles and radnet_png_tiles_on_sweep with exactly-sized heap buffers, so a write past `cap` pairs is caught, and
// with the largest sizes the entries take, so an overflow in the rule's integer arithmetic is.
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

// every tile of the plan appears once over the sweeps, on sweep block + 2 * band, bands ascending within a sweep
static void walk(int rows, int rowbytes, int bpp) {
  radnet_png_tile_plan plan;
  CHECK(radnet_png_plan_tiles(rows, rowbytes, bpp, &plan) == RADNET_OK);
  const int pixels = rowbytes / bpp, T = RADNET_PNG_TILE_PIXELS;
  CHECK(plan.tile_rows == RADNET_PNG_TILE_ROWS && plan.tile_pixels == T);
  CHECK(plan.bands == (rows - 1) / 64 + 1 && (int64_t)plan.blocks * T >= (int64_t)pixels + 63 && (int64_t)(plan.blocks - 1) * T < (int64_t)pixels + 63);
  CHECK(plan.sweeps == plan.blocks + 2 * (plan.bands - 1));
  if ((int64_t)plan.bands * plan.blocks > 1 << 20) return;          // the large plans: the numbers alone
  std::vector<int> seen((size_t)plan.bands * plan.blocks, 0);
  for (int d = 0; d < plan.sweeps; ++d) {
    const int n = radnet_png_tiles_on_sweep(rows, rowbytes, bpp, d, nullptr, 0);
    CHECK(n >= 0 && n <= plan.bands && (n >= 1 || (plan.blocks == 1 && d % 2 == 1)));      // one block: the even sweeps alone
    if (n < 1) continue;
    int32_t* pairs = (int32_t*)malloc(sizeof(int32_t) * 2 * (size_t)n);      // exactly n pairs
    CHECK(radnet_png_tiles_on_sweep(rows, rowbytes, bpp, d, pairs, n) == n);
    for (int i = 0; i < n; ++i) {
      const int band = pairs[2 * i], block = pairs[2 * i + 1];
      CHECK(band >= 0 && band < plan.bands && block >= 0 && block < plan.blocks && block + 2 * band == d);
      CHECK(i == 0 || band == pairs[2 * i - 2] + 1);
      if (band >= 0 && band < plan.bands && block >= 0 && block < plan.blocks) ++seen[(size_t)band * plan.blocks + block];
    }
    free(pairs);
    if (n > 1) {                                                      // a smaller cap: that many pairs and no more
      int32_t* one = (int32_t*)malloc(sizeof(int32_t) * 2);
      CHECK(radnet_png_tiles_on_sweep(rows, rowbytes, bpp, d, one, 1) == n);
      free(one);
    }
  }
  for (size_t k = 0; k < seen.size(); ++k) CHECK(seen[k] == 1);
}

int main() {
  static_assert(sizeof(radnet_png_tile_plan) == 20, "radnet_png_tile_plan is five int32");
  const int T = RADNET_PNG_TILE_PIXELS;
  const int rows[] = {1, 63, 64, 65, 128, 129, 4000};
  const int pixels[] = {1, 2, 62, 63, 64, 65, T - 63, T - 1, T, T + 1, 2 * T + 1, 4000};
  const int bpps[] = {1, 2, 3, 4, 6, 8};
  for (int r : rows)
    for (int p : pixels)
      for (int b : bpps) walk(r, p * b, b);
  walk(0x7fffffff, 1 << 30, 1);                                       // the largest segment the entries take
  walk(0x7fffffff, 1 << 30, 8);
  walk(1, 1 << 30, 1);
  {                                                                   // refusals: nothing is written
    radnet_png_tile_plan plan;
    memset(&plan, 0x5A, sizeof(plan));
    radnet_png_tile_plan before = plan;
    int32_t pairs[4];
    memset(pairs, 0x5A, sizeof(pairs));
    CHECK(radnet_png_plan_tiles(0, 12, 3, &plan) == RADNET_ERR_ARG);
    CHECK(radnet_png_plan_tiles(5, 0, 3, &plan) == RADNET_ERR_ARG);
    CHECK(radnet_png_plan_tiles(5, 12, 5, &plan) == RADNET_ERR_ARG);
    CHECK(radnet_png_plan_tiles(5, 13, 3, &plan) == RADNET_ERR_ARG);
    CHECK(radnet_png_plan_tiles(5, (1 << 30) + 8, 8, &plan) == RADNET_ERR_ARG);
    CHECK(radnet_png_plan_tiles(5, 12, 3, nullptr) == RADNET_ERR_ARG);
    CHECK(memcmp(&plan, &before, sizeof(plan)) == 0);
    CHECK(radnet_png_tiles_on_sweep(130, 12, 3, -1, pairs, 2) == RADNET_ERR_ARG);
    CHECK(radnet_png_plan_tiles(130, 12, 3, &plan) == RADNET_OK && plan.bands == 3);
    const radnet_png_tile_plan small = plan;
    plan = before;
    CHECK(radnet_png_tiles_on_sweep(130, 12, 3, small.sweeps, pairs, 2) == RADNET_ERR_ARG);
    CHECK(radnet_png_tiles_on_sweep(130, 12, 3, 0, pairs, -1) == RADNET_ERR_ARG);
    CHECK(radnet_png_tiles_on_sweep(130, 12, 3, 0, nullptr, 1) == RADNET_ERR_ARG);
    CHECK(radnet_png_tiles_on_sweep(130, 13, 3, 0, pairs, 2) == RADNET_ERR_ARG);
    for (int k = 0; k < 4; ++k) CHECK(pairs[k] == 0x5A5A5A5A);
    CHECK(radnet_png_tiles_on_sweep(130, 12, 3, small.sweeps - 1, pairs, 2) == 1 && pairs[0] == 2 && pairs[1] == small.blocks - 1 && pairs[2] == 0x5A5A5A5A);
  }
  printf("%d checks, %d failed\n", checked, failed);
  return failed ? 1 : 0;
}
