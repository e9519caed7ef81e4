// Argument structs of the fp32 conv GEMM kernels and the chain kernel: filled on the host, passed to the kernels by value or
// copied to device memory.  No device code and no HIP header: hipcc and g++ (chain_plan.cpp) both read this file, and the
// static_asserts turn a disagreement about a layout into a compile error.
#pragma once

constexpr int BK = 32;          // reduction depth per LDS tile
constexpr int NTHREADS = 256;
constexpr int kNumCU = 256;

struct GemmArgs {
  const float* x;        // gathered activation tensor (NHWC)
  const float* w;        // B operand base
  float* y;              // output [M][ldy]
  const float* scale;    // epilogue per-column scale
  const float* shift;    // epilogue per-column shift
  const float* addend;   // epilogue addend [M][ld_add]
  const float* mask;     // epilogue mask   [M][ld_mask] (zero where <= 0)
  const float* in_scale; // per-gathered-channel factor (C entries) or null
  float* partial;        // split-K partial sums [split][M][N] (null = direct epilogue)
  int H, W, C;           // gathered tensor geometry
  int OH, OW;            // output spatial geometry
  int KW, npos;          // kernel width, kh*kw
  int stride, pad_t, pad_l;
  int M, N, K;           // GEMM sizes, K = npos*C
  int ldw, ldy, ld_add, ld_mask;
  int act, act_cols;
  int flip;              // dgrad: kernel position flipped (npos-1-pos)
  int cin_fwd;           // dgrad B addressing: forward input channels (= N here)
  const int* units;      // work-unit table (8 ints per unit: tile_m, tile_n, kt_begin, kt_end, slot, pad..) or null
  unsigned long long magic_ohow, magic_ow;
  int OHOW;
  unsigned x_bytes, w_bytes;   // extents for the buffer descriptors
  unsigned y_bytes, add_bytes, mask_bytes;
  int batch;                   // > 1: blockIdx.z selects one of `batch` independent GEMMs (plain launches only)
  long long x_bstride, w_bstride, y_bstride;   // floats between consecutive problems of a batch
  unsigned* counters;          // K-split launches: arrival counter per output tile (zero outside a launch)
  unsigned long long* stamps;  // diagnostic build only (RADNET_DIAG_STAMPS): 8 words per workgroup
  int xcd_batch;               // batched launch: workgroups renumbered so that each XCD runs a contiguous run of (problem, tile)s
  int zper;                    // persistent batched launch (PERSIST kernels): consecutive problems one workgroup runs, blockIdx.z = group
};

// fused bottleneck tail (conv_igemm_body.h: bneck_tail)
struct TailArgs {
  const float* w2; const float* sc2; const float* sh2; const float* add; float* y;     // expand: [64][ldw2], columns N2 (multiple of 64)
  const float* w3; const float* sc3; const float* sh3; float* t;                        // next reduce: [N2][ldw3] -> 64 columns, or null
  int N2, ldw2, ldy2, ld_add2, ldw3, ldt;
  unsigned w2_bytes, w3_bytes, y_bytes, add_bytes, t_bytes;
};

struct WgradArgs {
  const float* x;
  const float* dy;
  const float* gscale;
  float* dw;
  float* db;             // bias gradient [N] (atomic adds by the workgroups of the first k tile) or null
  int H, W, C, OH, OW, KW, stride, pad_t, pad_l;
  int M, N, K;
  int ld_dy, ldw;
  int mt_per_split;
  int atomic;
  const int* rowtab;     // [taps][mpad] byte offset of the row's tap in the biased x descriptor, or kOOB; see get_row_table
  int mpad;              // M rounded up to whole 32-row tiles
  int xcd_batch;         // batched launch: XCD-contiguous workgroup numbering (GemmArgs::xcd_batch)
  unsigned x_bias;       // bytes the x descriptor starts ahead of x (halo rows keep non-negative offsets)
  unsigned x_bytes, dy_bytes;
  int batch, splits;     // batch > 1: blockIdx.z = problem * splits + split (radnet_wgrad_batched)
  long long x_bstride, dy_bstride, dw_bstride;   // floats between consecutive problems
  // Ordered reduction of a split launch (radnet_ctx::deterministic): the splits write their partial tiles as slabs, the last
  // one to arrive at a tile sums them in split order -- the forward kernel's in-launch split-K protocol.  slabs == null:
  // fp32 atomics (run-to-run differences in the last bits).
  float* slabs;          // [tile][split][BMK*BN], then the bias partials [n tile][split][BN]
  unsigned* counters;    // arrival counter per tile (zero outside a launch)
  int accumulate;        // ordered form: 1 = add the sum to dw's contents, 0 = store it
  int tiles_x, tiles_y;  // grid.x, grid.y of the launch (the pair kernel has a grid of its own)
  // Optimizer block (conv_wgrad_multi_kernel only; every other kernel ignores it): ow != null -> the writer of a tile's final value
  // applies the Adam update (adam_update.h) to ow / om / ov [K][ldw] at the tile's place and does NOT store the gradient into dw.
  float* ow;
  float* om;
  float* ov;
  float lr_t, beta1, beta2, eps, grad_scale;
  int pad_opt;
};

// conv_wgrad_multi_kernel (conv_wgrad.hip): up to kWgradMultiMax problems of one tile shape in one launch.  first[p] = first workgroup
// of problem p, first[n] = the grid; a problem's workgroups number its (k tile, n tile, slice) grid with the k tile running fastest.
constexpr int kWgradMultiMax = 16;
struct WgradMultiMap {
  unsigned first[kWgradMultiMax + 1];
  unsigned wx[kWgradMultiMax], wy[kWgradMultiMax];
  int n;
};
// the optimizer scalars of a multi launch travel as kernel arguments (they change with every step; the problem table does not)
struct WgradOptScalars {
  float lr_t, beta1, beta2, eps, grad_scale;
};

// conv_bwd_pair_kernel (conv_wgrad.hip): how its grid divides between the two problems
struct PairMap {
  unsigned n_a, n_w;            // workgroups of the dgrad / wgrad problem
  unsigned ax, ay;              // dgrad grid (x, y); z = 1
  unsigned wx, wy;              // wgrad grid (x, y); z = n_w / (wx * wy)
};

// chain kernel (chain.hip; the list is written by chain_plan.cpp)
struct ChainStage {
  GemmArgs g;                                   // type 0: conv tile / tile of a batched GEMM
  const float* t_src;                           // type 1: x [nb][h][w][c] -> V;  type 2: M [36][T][n] -> y
  float* t_dst;
  const float* t_scale;
  const float* t_shift;
  int t_nb, t_h, t_w, t_c, t_th, t_tw, t_act, t_ldy;
  unsigned t_dst_bytes;
  int type;
};
struct ChainItem {
  int stage, bx, by, bz;
  int d0_first, d0_count, d1_first, d1_count;   // counter ranges that must have reached their `need`
  int sig0, sig1, pad0, pad1;                   // counters this item bumps when done (-1: none)
};
struct ChainHeader {
  unsigned next, exited, error, last_error;
  unsigned runs, host_lo, host_hi, pad;       // host_lo/hi: a mapped host word that receives the first error (radnet_chain_error: no sync)
};

// arrival counters sit 64 bytes apart: the counters one item polls, and the ones neighbouring items bump, spread over cache
// lines and memory channels instead of queueing on one
constexpr int kCtrStride = 16;

// the kernels read these bytes as the host wrote them: both compilers must lay them out alike
static_assert(sizeof(GemmArgs) == 264 && sizeof(TailArgs) == 120 && sizeof(WgradArgs) == 248 && sizeof(PairMap) == 24, "kernel argument layout");
static_assert(sizeof(WgradMultiMap) == 200 && sizeof(WgradOptScalars) == 20, "multi-problem weight-gradient launch layout");
static_assert(sizeof(ChainStage) == 336 && sizeof(ChainItem) == 48 && sizeof(ChainHeader) == 32, "chain list layout");
