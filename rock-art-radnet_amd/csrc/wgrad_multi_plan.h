// Host-side plan of radnet_conv_wgrad_multi (conv_wgrad.hip): which weight-gradient problems share a launch, where each problem's
// workgroups start in the grid, and where its ordered-reduction slabs and arrival counters lie.  No device code and no HIP header: g++
// compiles wgrad_multi_plan.cpp (also under the sanitizers, tests/native/wgrad_multi_plan_sanitize.cpp).
#pragma once
#include <stdint.h>

#include "conv_args.h"

// What the plan needs to know of one problem: the launch shape its single launch would use.
struct WgradMultiItem {
  int bmk, bn;               // output tile (k x n)
  unsigned wx, wy, wz;       // grid of the single launch: k tiles, n tiles, slices
  uint64_t slab_bytes;       // ordered reduction: bytes of partial tiles + bias partials (0: not split, or atomics)
  unsigned counters;         // ordered reduction: arrival counters (one per output tile), else 0
};

struct WgradMultiLaunch {
  int bmk, bn, n;                          // the tile shape all n problems of the launch share
  int problem[kWgradMultiMax];             // index of each in the item list, in list order
  uint64_t slab_off[kWgradMultiMax];       // byte offset of its slabs in the workspace (a multiple of 256)
  unsigned counter_off[kWgradMultiMax];    // its first arrival counter
  WgradMultiMap map;
};

constexpr int kWgradMultiErrArg = -1, kWgradMultiErrFit = -2, kWgradMultiErrCap = -3;

// Problems are grouped by tile shape, shapes in the order of their first problem, problems in list order.  A launch is closed when it
// holds kWgradMultiMax problems, or when the next problem's slabs / counters / workgroups would not fit beside the ones it holds
// (ws_bytes of workspace, counter_cap counters, 2^31 - 1 workgroups); the next launch starts again at offset 0 -- launches of one stream
// run one after the other.  Returns the number of launches written to out[0 .. cap), kWgradMultiErrArg for a malformed list,
// kWgradMultiErrFit when one problem alone does not fit, kWgradMultiErrCap when `cap` launches are not enough.
int wgrad_multi_plan(const WgradMultiItem* items, int n, uint64_t ws_bytes, unsigned counter_cap, WgradMultiLaunch* out, int cap);
