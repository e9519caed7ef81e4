// Host side shared by the launchers of conv_mfma.hip, conv_wgrad.hip and chain.hip.
#pragma once
#include "radnet_internal.h"
#include "conv_args.h"
#include <hip/hip_ext.h>

// One launch, timed from its own dispatch when an event pair is armed (bench.py's roofline leg), plain otherwise.
#define RADNET_LAUNCH(kernel, grid, block, shmem, st, e0, e1, ...)                                                  \
  do {                                                                                                              \
    if (e0) hipExtLaunchKernelGGL(kernel, grid, block, shmem, st, e0, e1, 0, __VA_ARGS__);                          \
    else hipLaunchKernelGGL(kernel, grid, block, shmem, st, __VA_ARGS__);                                           \
  } while (0)

// radnet_conv_bwd: the final launch of run_igemm (dgrad) / run_wgrad lands here instead of on the stream while
// ctx->pair_capture is set; the measuring launches of a first, autotuned call are issued as usual (PairPause).
struct PairCapture {
  bool have_a = false, a_ok = false, have_w = false, w_ok = false;
  int a_bm = 64;
  GemmArgs ga;
  unsigned ax = 0, ay = 0;
  WgradArgs gw;
  unsigned wx = 0, wy = 0, wz = 0;
  uint64_t a_slab_bytes = 0, w_slab_bytes = 0;      // split-K slabs at the start / ordered wgrad slabs at the end of the workspace
  int w_bmk = 64, w_bn = 64;                        // the weight gradient's tile and the exact size of its slabs (radnet_conv_wgrad_multi
  uint64_t w_slab_need = 0;                         // lays the slabs of several problems side by side)
  double flops = 0.0;
};
struct PairPause {
  radnet_ctx* ctx;
  void* saved;
  explicit PairPause(radnet_ctx* c) : ctx(c), saved(c->pair_capture) { c->pair_capture = nullptr; }
  ~PairPause() { ctx->pair_capture = saved; }
};
