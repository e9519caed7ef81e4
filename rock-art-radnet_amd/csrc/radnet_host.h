// Host-only helpers with no HIP dependency: radnet_internal.h includes them, chain_plan.cpp (g++) uses them alone.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include "radnet_hip.h"

#define RADNET_FAIL(ctx, code, ...)                         \
  do {                                                      \
    snprintf((ctx)->err, sizeof((ctx)->err), __VA_ARGS__);  \
    return (code);                                          \
  } while (0)

static inline int radnet_cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
// workgroups of a grid-stride launch over `total` work items: cdiv(total, block) clamped to [1, cap]
static inline int grid_for(long long total, int block = 256, int cap = 4096) {
  long long b = (total + block - 1) / block;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (int)b;
}
// exact floor(m / d) for m, d < 2^20 as (m * magic) >> 40  (m*d < 2^40, see conv_device.h: div_magic)
static inline uint64_t radnet_div_magic(uint32_t d) { return ((1ull << 40) + d - 1) / d; }
