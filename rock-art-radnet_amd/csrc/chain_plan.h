// The chain kernel's work-item list as the host plans it (chain_plan.cpp: host code only) and chain.hip uploads it.
#pragma once
#include <stddef.h>
#include <vector>
#include "conv_args.h"
#include "radnet_hip.h"

struct ChainPlan {
  std::vector<ChainStage> stages;
  std::vector<ChainItem> items;
  std::vector<unsigned> need;                   // per counter
  std::vector<int> units;                       // all K-split unit tables, 8 ints per unit
  std::vector<size_t> unit_base;                // per stage: first int of its table (or ~0)
  std::vector<size_t> slab_base;                // per stage (floats)
  size_t slabs_total = 0;
  double flops = 0.0, flops_alg = 0.0;
};
struct ErrSink {                                // RADNET_FAIL needs ->err
  char err[512];
};

// plans the list and checks that it can run in list order; a failure leaves its message in ec.err (library-internal: not exported)
__attribute__((visibility("hidden"))) int radnet_chain_plan(const radnet_op* ops, int32_t n_ops, ChainPlan& pl, ErrSink& ec);
