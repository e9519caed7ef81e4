/*
 * radnet_hip.h -- C ABI of libradnet_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * Faster R-CNN train / predict hot path of rock-art-radnet.
 *
 * The reference has NO native layer: everything below replaces work it hands to the TensorFlow
 * runtime (Keras graph in faster_rcnn/base_models/resnet50.py, rpn.py:12-66, RoiPoolingConv.py,
 * FixedBatchNormalization.py, losses.py, keras Adam) or does in single-threaded NumPy/Python
 * (rpn.py:68-455, utils.py:554-822).  Each entry point cites the reference lines it stands in for.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (e.g. torch-ROCm tensor.data_ptr());
 *     the library never allocates or frees caller-visible memory;
 *   - work is enqueued on the hipStream_t given to radnet_create(); calls return immediately;
 *   - activations are NHWC fp32; conv weights are [K = kh*kw*cin][N = cout] row-major (the Keras
 *     HWIO kernel flattened), dense weights [in][out];
 *   - return value 0 = ok, negative = error; radnet_last_error() gives the message;
 *   - one context per thread / stream (no internal locking).
 */
#ifndef RADNET_HIP_H
#define RADNET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct radnet_ctx radnet_ctx;

#define RADNET_OK 0
#define RADNET_ERR_ARG (-1)
#define RADNET_ERR_HIP (-2)
#define RADNET_ERR_UNSUPPORTED (-3)

/* ---- context ------------------------------------------------------------------------------ */
int radnet_create(int device, void* hip_stream, radnet_ctx** out);
void radnet_destroy(radnet_ctx* ctx);
const char* radnet_last_error(radnet_ctx* ctx);
int radnet_sync(radnet_ctx* ctx);
/* Re-binds the context to another HIP stream (e.g. a stream in capture mode while a sequence of launches is recorded
 * into a hipGraph; the library performs no allocation, host synchronisation or autotuning for shapes it has already
 * run, so a recorded sequence replays as is). */
int radnet_set_stream(radnet_ctx* ctx, void* hip_stream);
int radnet_version(void);
/* Scratch the library may use for split-K partial sums (caller-owned, >= bytes). */
int radnet_set_workspace(radnet_ctx* ctx, void* ws, uint64_t bytes);
/* Autotuning of the conv GEMM launch shape.  While enabled, the FIRST conv_fwd / conv_dgrad / conv_wgrad call of
 * each problem shape times every (output tile, split-K) candidate on the ctx stream (synchronising it) and caches
 * the fastest; later calls of that shape reuse the choice.  Shapes are static per image size, so a warm-up step
 * tunes the whole layer program.  radnet_tuned_shapes() returns the number of cached shapes.
 * enable = 2: as 1, but a new shape first adopts the cached choice of the shape that differs from it in M only, by at most
 * M/4 (nearest M), and is measured only when there is none -- for training on tiles whose size changes from sample to
 * sample (rotation / shear augmentation, augmentation.py:158-271), where every new size would otherwise re-tune every layer. */
int radnet_set_autotune(radnet_ctx* ctx, int enable);
int radnet_tuned_shapes(radnet_ctx* ctx);
/* Persist / restore the measured choices (text, one shape per line).  A context that loaded a table runs no trial
 * launches for the shapes in it: restarts skip the tuning step, and a profiler sees steady-state launches only. */
int radnet_tune_save(radnet_ctx* ctx, const char* path);
/* `ctx` uses (reads and extends) the table of `owner` from now on: the contexts an engine keeps for its concurrent lanes
 * (one per HIP stream) measure every shape once.  All calls on contexts that share a table come from one host thread.
 * The read-only device tables the weight-gradient kernel keeps per conv geometry are shared the same way, so a context can
 * meet a geometry for the first time inside a stream capture (its sibling built the table in an earlier eager run). */
int radnet_share_tuning(radnet_ctx* ctx, radnet_ctx* owner);
int radnet_tune_load(radnet_ctx* ctx, const char* path);
/* Test hook: force every following conv GEMM launch to use output tile (tile_a x tile_b in {64,128}) and `slices` K
 * slices per tile (negative = same slices with the XCD-aware workgroup order); tile_a = 0 switches it off.  Batched launches
 * (radnet_gemm_batched / radnet_wgrad_batched: the Winograd positions) take slices = 1 or -1 only: -1 renumbers the workgroups
 * so that each XCD runs a contiguous run of (problem, tile)s and the tiles that share a problem's operands share an L2 --
 * same results bit for bit, 5-9 % shorter launches for the 36 GEMMs of a Winograd layer at 1000x600. */
int radnet_force_config(radnet_ctx* ctx, int tile_a, int tile_b, int slices);
/* With radnet_force_config active: waves per workgroup of the forward / dgrad kernel (4, or 8 = every K tile halved
 * between two wave grids and summed through LDS); 0 = default (4). */
int radnet_force_waves(radnet_ctx* ctx, int waves);
/* Reproducible reductions (default ON; the environment variable RADNET_DETERMINISTIC=0 sets the default of new contexts to
 * off).  ON: every floating-point reduction that crosses workgroups -- the pixel splits of conv_wgrad / wgrad_batched /
 * conv_bwd and their bias gradients, radnet_colsum's row blocks, radnet_roi_resize_bwd's overlapping RoIs, the loss sums of
 * radnet_rpn_loss -- is handed to ONE workgroup that adds the partial results in index order, so a launch returns the same
 * bits on every run and on every stream (TF's own GPU gradients, train.py:288/393, give no such guarantee; what this buys is
 * that two schedules of the same training step can be compared bit for bit).  OFF: fp32 / fp64 atomics, whose order -- and
 * therefore last bits -- change from run to run.  Split weight-gradient launches then keep their partial tiles in the
 * workspace (radnet_set_workspace), from its end downwards; launch shapes whose partials do not fit are not used. */
int radnet_set_deterministic(radnet_ctx* ctx, int enable);
/* The context's current setting (1 / 0; negative: error) -- what bench.py's `config.reductions` reports. */
int radnet_get_deterministic(radnet_ctx* ctx);
/* Per-launch timing of the conv/GEMM kernel families with HIP events on the ctx stream (bench.py's roofline leg).
 * enable=1 starts recording; radnet_timing_read returns accumulated milliseconds and launch count since the last reset for
 * kernel class `cls`: 0 fwd, 1 dgrad, 2 wgrad, 4 dgrad + wgrad in one launch -- each launch timed from its own dispatch
 * (hipExtLaunchKernelGGL start / stop events: the kernel's begin and end, what rocprofv3 --kernel-trace reports) --, and
 * 3 Winograd 3x3 LAYERS of a program: transforms + batched GEMMs bracketed by two marker events as one unit (that bracket
 * includes the markers' dispatch latency, ~5 us) and credited the layer's algorithmic 2*M*N*9C flops. */
int radnet_timing_enable(radnet_ctx* ctx, int enable);
int radnet_timing_read(radnet_ctx* ctx, int cls, double* ms, int64_t* launches, double* flops);
int radnet_timing_reset(radnet_ctx* ctx);

/* ---- convolution as implicit GEMM on fp32 MFMA ----------------------------------------------
 * Replaces keras Conv2D / TimeDistributed(Conv2D) + FixedBatchNormalization + Add + Activation
 * (resnet50.py:41-147,183-186; rpn.py:41-64; FixedBatchNormalization.py:59-85) and their TF
 * autodiff gradients.  One descriptor describes the FORWARD convolution; dgrad / wgrad reuse it.
 *
 *   forward :  y[m][n] = act( (sum_k im2col(x)[m][k] * w[k][n]) * scale[n] + shift[n] + addend[m][n] )
 *   dgrad   :  dx[p][c] = ( sum_{kh,kw,n} (dy*gscale)[..][n] * w[(kh,kw,c)][n] + addend[p][c] ) masked
 *              by mask[p][c] > 0   (stride 1 only; ReLU backward of the producer fused as the mask)
 *   wgrad   :  dw[k][n] (+)= sum_m im2col(x)[m][k] * (dy*gscale)[m][n];
 *              db[n] (+)= sum_m (dy*gscale)[m][n] in the same launch when db is set (else radnet_colsum)
 */
typedef struct radnet_conv_desc {
  const float* x;        /* forward input  [nb][h][w][c]                                   */
  const float* w;        /* weights        [kh*kw*c][ldw]                                  */
  float* y;              /* forward output [nb*oh*ow][ldy]                                 */
  const float* scale;    /* per-output-channel scale (frozen BN: gamma/sqrt(var+eps)) or 0 */
  const float* shift;    /* per-output-channel shift (bias and BN shift folded) or 0       */
  const float* addend;   /* residual branch [m][ld_add] or 0                               */
  int32_t nb, h, w_, c;  /* input geometry                                                 */
  int32_t oh, ow;        /* output geometry                                                */
  int32_t kh, kw, stride, pad_t, pad_l;
  int32_t n;             /* output channels                                                */
  int32_t ldw, ldy, ld_add;
  int32_t act;           /* 0 none, 1 relu, 2 sigmoid on columns [0,act_cols) / linear rest */
  int32_t act_cols;
  /* backward-only fields */
  const float* dy;       /* gradient w.r.t. y (post-activation mask already applied) [m][ld_dy] */
  const float* gscale;   /* per-output-channel factor applied to dy on load (BN scale) or 0 */
  float* dx;             /* dgrad output [nb*h*w][ld_dx]                                   */
  const float* dx_add;   /* added to dx before masking (residual-path gradient) or 0       */
  const float* dx_mask;  /* dx zeroed where dx_mask <= 0 (producer's ReLU) or 0            */
  float* dw;             /* wgrad output [kh*kw*c][ldw]                                    */
  int32_t ld_dy, ld_dx, ld_dx_add, ld_dx_mask;
  int32_t dw_accumulate; /* 0: overwrite dw; 1: dw += ; 2: dw was zeroed by the caller (no memset, no atomics unless split) */
  float* db;             /* wgrad: bias gradient [n], same accumulate mode as dw, or 0                   */
} radnet_conv_desc;

int radnet_conv_fwd(radnet_ctx* ctx, const radnet_conv_desc* d);
/* Strided-batched fp32 GEMM on the same matrix-core kernel: y[p][m][n] = a[p][m][k] * b[p][k][n], p < batch, all
 * operands dense row-major and contiguous over p; k a multiple of 32, n of 4. */
int radnet_gemm_batched(radnet_ctx* ctx, const float* a, const float* b, float* y, int32_t batch, int32_t m, int32_t n, int32_t k);
/* Winograd F(2x2,3x3) form of a stride-1 'same' 3x3 convolution (same layers as radnet_conv_fwd; 2.25x fewer matrix-core
 * flops): u = filter transform of w [3][3][c][ldw] -> [16][c][n] (once per weight update); v = input transform of
 * x [nb][h][w][c] -> [16][tiles][c], tiles = nb*ceil(h/2)*ceil(w/2); radnet_gemm_batched(v, u, m, 16, tiles, n, c);
 * output transform of m [16][tiles][n] with the conv epilogue: y = act(conv * scale + shift), act 0 none / 1 relu. */
int radnet_winograd_filter(radnet_ctx* ctx, const float* w, int32_t c, int32_t n, int32_t ldw, float* u);
int radnet_winograd_input(radnet_ctx* ctx, const float* x, int32_t nb, int32_t h, int32_t w, int32_t c, float* v);
int radnet_winograd_output(radnet_ctx* ctx, const float* m, int32_t nb, int32_t oh, int32_t ow, int32_t n, const float* scale,
                           const float* shift, int32_t act, float* y, int32_t ldy);
/* Weight gradient of the same layers in the Winograd domain: dz = A dY A^T per tile of the (gscale-scaled) output gradient
 * [nb][oh][ow][ld_dy] -> [16][tiles][n]; radnet_wgrad_batched(v, dz, du, 16, tiles, c, n, 0): du[p][c][n] = sum over tiles of
 * v[p][tile][c] * dz[p][tile][n] with the v of the forward pass; dw [3][3][c][ldw] (+)= G^T du G.  The bias gradient is the
 * plain column sum of dy (radnet_colsum). */
int radnet_winograd_dy(radnet_ctx* ctx, const float* dy, int32_t nb, int32_t oh, int32_t ow, int32_t n, int32_t ld_dy,
                       const float* gscale, float* dz);
int radnet_wgrad_batched(radnet_ctx* ctx, const float* a, const float* dy, float* dw, int32_t batch, int32_t m, int32_t k, int32_t n,
                         int32_t accumulate);
int radnet_winograd_filter_grad(radnet_ctx* ctx, const float* du, int32_t c, int32_t n, int32_t ldw, float* dw, int32_t accumulate);
/* The same five transforms for Winograd F(4x4,3x3): 36 positions instead of 16 (u [36][c][n], v [36][tiles][c], m / dz
 * [36][tiles][n], batch 36 in radnet_gemm_batched / radnet_wgrad_batched) over tiles = nb*ceil(h/4)*ceil(w/4) -- 4x fewer
 * matrix-core flops than the direct 3x3 form, 1.78x fewer than F(2x2), and 0.56x the transform traffic of F(2x2); the fp32
 * result is off by about 2e-5 of the largest activation from the fp64 sum (F(2x2): 1e-6), inside the stated 2e-4. */
int radnet_winograd4_filter(radnet_ctx* ctx, const float* w, int32_t c, int32_t n, int32_t ldw, float* u);
int radnet_winograd4_input(radnet_ctx* ctx, const float* x, int32_t nb, int32_t h, int32_t w, int32_t c, float* v);
int radnet_winograd4_output(radnet_ctx* ctx, const float* m, int32_t nb, int32_t oh, int32_t ow, int32_t n, const float* scale,
                            const float* shift, int32_t act, float* y, int32_t ldy);
int radnet_winograd4_dy(radnet_ctx* ctx, const float* dy, int32_t nb, int32_t oh, int32_t ow, int32_t n, int32_t ld_dy,
                        const float* gscale, float* dz);
int radnet_winograd4_filter_grad(radnet_ctx* ctx, const float* du, int32_t c, int32_t n, int32_t ldw, float* dw, int32_t accumulate);
int radnet_conv_dgrad(radnet_ctx* ctx, const radnet_conv_desc* d);
int radnet_conv_wgrad(radnet_ctx* ctx, const radnet_conv_desc* d);
/* Weight gradient and data gradient of one layer from one descriptor (train.py's backward pass through a Conv2D: both read
 * dy).  Issued as ONE launch whose workgroups alternate between the two problems when both run as 64x64-tile, 4-wave
 * workgroups -- two short launches in a row each pay their own lockstep prologue / epilogue and launch gap, mixed they hide
 * each other's -- and as radnet_conv_wgrad followed by radnet_conv_dgrad otherwise (other launch shapes, d->dx == 0,
 * RADNET_NO_BWD_PAIR=1).  Same results as the two calls.  Timing class 4. */
int radnet_conv_bwd(radnet_ctx* ctx, const radnet_conv_desc* d);
/* The weight gradients (and bias gradients, d->db) of n layers in as few launches as their launch shapes allow: the problems are
 * grouped by the output tile radnet_conv_wgrad would give each of them, up to 16 problems of one tile shape share a launch, and every
 * problem keeps the grid, the slice count and the slice order of its own radnet_conv_wgrad call -- dw and db hold the bits of the n
 * single calls.  d->dx is ignored.  Row tables and problem tables are built on the host at the first call (not inside a stream
 * capture).
 * opt != 0 with opt->p != 0: Adam in the tile epilogue.  Every dw must lie inside the gradient arena opt->g [n]; the workgroup that
 * holds the final value of a dw tile -- the tile's only workgroup, or the last arriver of its ordered slice reduction -- applies the
 * update of radnet_adam_step (step t, grad_scale on the gradient) to the weights and moments at the same offset of opt->p / m / v and
 * does NOT store the gradient: opt->g is neither written nor read, the same bits as radnet_conv_wgrad into a zeroed arena followed by
 * radnet_adam_step over these ranges.  The caller guarantees that nothing in flight reads the weights (all data gradients of the step
 * have run).  Bias gradients still go to d->db.  Refused: dw_accumulate == 1, and split problems on a context whose reductions are
 * not ordered (radnet_set_deterministic 0).  opt == 0 or opt->p == 0: gradients only.
 * A refused call launches no kernel and changes no byte of opt->p / m / v, but the problems are prepared one by one, each with the host
 * side of its own radnet_conv_wgrad call, before the later ones are checked: when problem i is refused, the memsets of write mode 0 --
 * db, and dw where the slices add with atomics -- of problems 0 .. i-1 (and of problem i itself where the refusal comes after its own
 * preparation: atomic slices under an optimizer block) are already enqueued, so exactly those destinations may hold zeros.  With
 * dw_accumulate == 2 throughout, a refused call changes nothing. */
typedef struct radnet_wgrad_adam {
  float* p; float* g; float* m; float* v;   /* the four arenas; dw - g locates a problem's weights and moments */
  int64_t n;                                /* floats per arena */
  int32_t t;                                /* Adam step, from 1 */
  float lr, beta1, beta2, eps, grad_scale;
} radnet_wgrad_adam;
int radnet_conv_wgrad_multi(radnet_ctx* ctx, const radnet_conv_desc* descs, int32_t n, const radnet_wgrad_adam* opt);
/* Two INDEPENDENT forward convolutions with the same output grid and reduction depth -- branch2a and the shortcut conv of a conv_block
 * (resnet50.py:100,111: both read the block's input) -- as ONE launch where that measured faster than the two launches with their own
 * launch shapes (decided once per pair of shapes, kept in the tuning table), as radnet_conv_fwd(d1), radnet_conv_fwd(d2) otherwise
 * (different grids, 4-channel input, forced configs, autotuning off, RADNET_NO_FWD_PAIR=1).  Same results as the two calls. */
int radnet_conv_fwd_pair(radnet_ctx* ctx, const radnet_conv_desc* d1, const radnet_conv_desc* d2);
/* The back of a bottleneck block (resnet50.py:53-71, 104-128) as ONE launch: db = its 3x3 convolution (stride 1, 'same', 64 output
 * channels, ReLU), dc = its 1x1 expand on db's output (dc->x == db->y; + shortcut dc->addend, ReLU), da = the NEXT block's 1x1 reduce on
 * dc's output (da->x == dc->y, 64 output channels, ReLU) or 0.  A workgroup that holds [rows x 64] of the 3x3's output holds all of that
 * layer's channels for its rows and goes on with the pointwise convolutions for the same rows through LDS: db->y is NOT written
 * (frozen layers only -- nothing can be differentiated through the block afterwards), dc->y once, da->x is not read back.  Used where it
 * measured faster than the separate launches (decided once per shape, kept in the tuning table); radnet_conv_fwd(db), (dc), (da) -- which
 * do write db->y -- for every other geometry, forced configs, autotuning off, RADNET_NO_BNECK_FUSE=1.  The separate launches are what
 * this call means: a descriptor has no pitch for x, so they read db->y (and dc->y, with da) as a DENSE matrix whatever ldy it was
 * written with.  The one-launch form is therefore taken only for dense intermediates -- db->ldy == db->n, and dc->ldy == dc->n when da
 * is given (without da, dc->ldy may be any pitch >= n) -- and only while M * max(dc->ldy, dc->ld_add, da->ldy) * 4 < 2^31. */
int radnet_conv_bottleneck(radnet_ctx* ctx, const radnet_conv_desc* db, const radnet_conv_desc* dc, const radnet_conv_desc* da);

/* ---- inference convolution on bf16 matrix cores (csrc/conv_bf16.hip) -----------------------------
 * The forward semantics of radnet_conv_fwd (resnet50.py:41-147,183-186; rpn.py:41-64) with bf16 operands and fp32 accumulation,
 * for frozen weights only (RADNet.predict, RADNet.py:520-600; the reference runs the same graph in fp32):
 *   y[m][n] = act( (sum_k bf16(im2col(x))[m][k] * bf16(w)[k][n]) * scale[n] + shift[n] + addend[m][n] ),  act / act_cols as above.
 * bf16() rounds to nearest, ties to even (v_cvt_pk_bf16_f32); subnormals are kept.  Activations stay fp32 in memory: the gather
 * rounds x on its way to the matrix cores, the epilogue and y are fp32.  No atomics, no split K: two runs give the same bits.
 *
 * radnet_weights_to_bf16: wt[j][i] = bf16(w[i][j]) for i < k, j < n; 0 for k <= i < ldk (w [k][ldw] fp32, wt [n][ldk] bf16 bits).
 *   Made once per weight load.  ldk >= k rounded up to 32 (the kernel's K tile), a multiple of 8.
 * radnet_conv_fwd_bf16: d->w and d->ldw are ignored; wt / ldk are the output of radnet_weights_to_bf16 for this layer's weights
 *   (k = kh*kw*c).  Needs c % 8 == 0 (8 consecutive k are 8 channels of one tap: the 4-channel stem stays on radnet_conv_fwd;
 *   RADNET_ERR_UNSUPPORTED otherwise), 16-byte aligned x and wt.  Any kernel size, stride and padding radnet_conv_fwd takes.
 *   The launch shape (128x128, 128x64 or 64x64 output tiles) is a fixed rule of (M, N): no autotuning, no tuning-table entry. */
int radnet_weights_to_bf16(radnet_ctx* ctx, const float* w, int32_t k, int32_t n, int32_t ldw, uint16_t* wt, int32_t ldk);
int radnet_conv_fwd_bf16(radnet_ctx* ctx, const radnet_conv_desc* d, const uint16_t* wt, int32_t ldk);
/* radnet_conv_fwd_bf16 with its K tiles dealt over `ksplit` slices of one launch (bf16-mixed training: small M, deep K).  Ordered:
 * every slice writes its partial tile to the context's workspace (radnet_set_workspace), the last to arrive sums the slices in
 * slice order and runs the epilogue -- no float atomics, the bits do not depend on arrival order or timing.  ksplit <= 1 is
 * radnet_conv_fwd_bf16 bit for bit; at most 64 and the number of 32-deep K tiles.  The split changes the summation order, so
 * results differ from ksplit = 1 within the rounding of an fp32 sum.
 * radnet_conv_bf16_pick_split: the split the bf16-mixed engine uses, a fixed function of (M = nb*oh*ow, N, K = kh*kw*c): the
 * smallest power of two (at most 16) that gives >= 256 workgroups, doubled only while every slice keeps >= 8 K tiles.
 * radnet_conv_bf16_tile_shape: the output tile *bm x *bn (128x128, 128x64 or 64x64) every bf16 matrix-core conv launch uses for an
 * output of rows x cols, and as return value the number of such tiles (0 and nothing written for an empty output or a null pointer).
 * Forward: (M, n); radnet_conv_dgrad_bf16: (P = nb*h*w, c); radnet_conv_wgrad_bf16: (K = kh*kw*c, n).  Needs no device.  The slabs of
 * a split launch take tiles * slices * bm * bn * 4 bytes of the context's workspace. */
int radnet_conv_fwd_bf16_split(radnet_ctx* ctx, const radnet_conv_desc* d, const uint16_t* wt, int32_t ldk, int32_t ksplit);
int32_t radnet_conv_bf16_pick_split(int64_t m, int32_t n, int32_t k);
int64_t radnet_conv_bf16_tile_shape(int64_t rows, int32_t cols, int32_t* bm, int32_t* bn);

/* ---- convolution backward on bf16 matrix cores (csrc/conv_bf16_bwd.hip; engine precision "bf16-train") ---------------
 * The backward semantics of radnet_conv_dgrad / radnet_conv_wgrad with bf16 operands and fp32 accumulation.  With
 * g[m][n] = dy[m][n] * gscale[n] computed as ONE fp32 multiply (g = dy when gscale is 0) and bf16() as above:
 *   dgrad :  dx[p][c] = mask( (sum_{kh,kw,n} bf16(g)[q(p,kh,kw)][n] * bf16(w)[(kh,kw,c)][n]) + dx_add[p][c] ), stride 1 only;
 *            dx_add and the dx_mask > 0 test are fp32, in the epilogue
 *   wgrad :  dw[k][n] (+)= sum_m bf16(im2col(x))[m][k] * bf16(g)[m][n], any stride / padding / kernel size radnet_conv_wgrad takes;
 *            dw_accumulate 0 overwrites, 1 and 2 add the sum ONCE to what dw holds (2: the zeros the caller wrote);
 *            d->db set: the bias gradient is radnet_colsum of the UNROUNDED dy * gscale (exact fp32, added in index order)
 * Activations and gradients stay fp32 in memory and are rounded on their way to the matrix cores.  bf16 has fp32's exponent
 * range: there is no loss scaling (dy * 2^-40 gives dw * 2^-40 and dx * 2^-40 bit for bit while nothing is subnormal).
 * No float atomics: a split of the reduction is radnet_conv_fwd_bf16_split's ordered in-launch protocol (slabs in the context
 * workspace, arrival counters in the context's aux block, the last arrival adds ALL slices in slice order), so two runs and
 * two contexts give the same bits.  A split whose slabs (output size x slices, rounded up to whole tiles) do not fit the
 * workspace, or whose output has more than 8192 tiles, is halved until it does -- by that rule, never by a timer; the launch shape
 * is radnet_conv_fwd_bf16's fixed rule on (output rows, output columns).  split <= 1: one pass.
 *
 * radnet_weights_to_bf16_dgrad: the dgrad image of a conv kernel w [taps*c][ldw] (taps = kh*kw):
 *   wd[i][t*n8 + j] = bf16(w[t*c + i][j]) for i < c, t < taps, j < n;  0 for every other element of wd [c][ldkd];
 *   n8 = n rounded up to 8, ldkd >= taps*n8 rounded up to 32, a multiple of 8; wd 16-byte aligned.  8 consecutive n of one
 *   (tap, c) are 16 contiguous bytes: the B fragment of the dgrad's MFMA.  Same rounding as radnet_weights_to_bf16.
 * radnet_weights_to_bf16_dgrad_arena: the same for up to 16 kernels that live in one optimizer arena p [n_arena] -- ONE launch
 *   over the registry, issued after the arena's Adam step (radnet_adam_step_bf16 keeps its signature and its 16-layer cap).
 * radnet_conv_dgrad_bf16: d->w / d->ldw are ignored; wd / ldkd are the layer's dgrad image.  Needs stride 1, n and ld_dy multiples
 *   of 4 with ld_dy >= n rounded up to 8 (columns >= n of dy are read but contribute zero: rpn_heads has 60 live columns in a
 *   pitch of 64), 16-byte aligned dy / gscale / wd; RADNET_ERR_UNSUPPORTED otherwise, nothing launched.
 * radnet_conv_wgrad_bf16: needs c and n multiples of 8, ld_dy a multiple of 4, 16-byte aligned x / dy / gscale;
 *   RADNET_ERR_UNSUPPORTED otherwise, nothing launched.  msplit slices of the M = nb*oh*ow pixels.
 * radnet_dgrad_bf16_pick_split(P = nb*h*w, c, kd = kh*kw*n8) / radnet_wgrad_bf16_pick_split(M, n, K = kh*kw*c): the splits the
 *   bf16-train engine uses -- radnet_conv_bf16_pick_split's rule on (output rows, output columns, reduction length): the smallest
 *   power of two (at most 16) that gives >= 256 workgroups, doubled only while every slice keeps >= 8 reduction tiles of 32. */
typedef struct radnet_bf16_dgrad_image {
  int64_t off;           /* float offset of the kernel [taps*c][ldw] in the arena */
  int32_t taps, c, n, ldw;
  uint16_t* wd;          /* dgrad image [c][ldkd] */
  int32_t ldkd;
} radnet_bf16_dgrad_image;
int radnet_weights_to_bf16_dgrad(radnet_ctx* ctx, const float* w, int32_t taps, int32_t c, int32_t n, int32_t ldw, uint16_t* wd, int32_t ldkd);
int radnet_weights_to_bf16_dgrad_arena(radnet_ctx* ctx, const float* p, int64_t n_arena, const radnet_bf16_dgrad_image* layers, int32_t n_layers);
int radnet_conv_dgrad_bf16(radnet_ctx* ctx, const radnet_conv_desc* d, const uint16_t* wd, int32_t ldkd);
int radnet_conv_dgrad_bf16_split(radnet_ctx* ctx, const radnet_conv_desc* d, const uint16_t* wd, int32_t ldkd, int32_t ksplit);
int radnet_conv_wgrad_bf16(radnet_ctx* ctx, const radnet_conv_desc* d, int32_t msplit);
int32_t radnet_dgrad_bf16_pick_split(int64_t p, int32_t c, int32_t kd);
int32_t radnet_wgrad_bf16_pick_split(int64_t m, int32_t n, int32_t k);

/* out[n] (+)= sum_m g[m][n] * gscale[n]   (bias gradients).  g is [m][ld] with ld >= n (columns n..ld are never read); gscale may be
 * null.  accumulate = 0 zeroes out[0..n) first.  RADNET_ERR_ARG, nothing zeroed or launched, for m < 1, n < 1 or ld < n. */
int radnet_colsum(radnet_ctx* ctx, const float* g, int32_t m, int32_t n, int32_t ld, const float* gscale,
                  float* out, int32_t accumulate);

/* ---- pooling / RoI crop-resize ------------------------------------------------------------- */
/* MaxPooling2D k x k / stride s 'valid' (resnet50.py:188: 3,2; VGG16 blocks: 2,2) */
int radnet_maxpool_fwd(radnet_ctx* ctx, const float* x, float* y, int32_t nb, int32_t h, int32_t w, int32_t c,
                       int32_t k, int32_t s);
/* RoiPoolingConv.call (RoiPoolingConv.py:48-88): int-cast RoI, clamped crop, TF1 legacy bilinear
 * resize to ps x ps.  rois: [r][4] fp32 (x,y,w,h) in feature-map units.  y: [r][ps][ps][c]. */
int radnet_roi_resize_fwd(radnet_ctx* ctx, const float* fmap, int32_t h, int32_t w, int32_t c, const float* rois,
                          int32_t r, int32_t ps, float* y);
/* gradient w.r.t. the feature map (scatter-add; dfmap must be zeroed by the caller) */
int radnet_roi_resize_bwd(radnet_ctx* ctx, const float* dy, int32_t h, int32_t w, int32_t c, const float* rois,
                          int32_t r, int32_t ps, float* dfmap);
/* TimeDistributed(AveragePooling2D((7,7))) + Flatten (resnet50.py:260-261): [r][hw][c] -> [r][c] */
int radnet_avgpool_fwd(radnet_ctx* ctx, const float* x, int32_t r, int32_t hw, int32_t c, float* y);
/* dx[r][p][c] = (y_act[r][p][c] > 0) ? dfeat[r][c] / hw : 0  (avg-pool backward fused with the ReLU mask) */
int radnet_avgpool_bwd_relu(radnet_ctx* ctx, const float* dfeat, const float* y_act, int32_t r, int32_t hw, int32_t c,
                            float* dx);

/* ---- classifier dense heads (resnet50.py:263-279) -------------------------------------------
 * w: [k][ldw] with the class columns first then the 4*(nc-1) regression columns; b: [nc+nreg].
 * out_cls = softmax(feat @ w[:, :nc] + b), out_regr = feat @ w[:, nc:] + b. */
int radnet_dense_heads_fwd(radnet_ctx* ctx, const float* feat, int32_t r, int32_t k, const float* w, int32_t ldw,
                           const float* b, int32_t nc, int32_t nreg, float* out_cls, float* out_regr);
/* dz: [r][nc+nreg] gradient w.r.t. the pre-softmax logits / regression outputs.
 * Writes (accumulate=0) or adds to (accumulate=1) dw [k][ldw] and db [ldw]; writes dfeat [r][k]. */
int radnet_dense_heads_bwd(radnet_ctx* ctx, const float* feat, const float* dz, int32_t r, int32_t k, const float* w,
                           int32_t ldw, int32_t nout, float* dw, float* db, float* dfeat, int32_t accumulate);

/* The tail of classifier_layer and its losses in one launch (csrc/head_tail.hip): avg-pool + both dense heads (+ softmax)
 * per RoI and -- with targets (y1 != 0) -- losses.py:69-95 and dz in the same launch.  The r RoIs come in `groups` equal groups, each its own reference step (own normalisers; losses
 * [groups][3] = cls, regr, accuracy); group_live[g] == 0: zero gradient rows, losses untouched.  scratch: device memory of
 * radnet_head_tail_scratch_bytes(r) bytes the caller zeroed ONCE (arrival counters that every launch leaves at zero, the
 * channel slices' partial sums, per-RoI loss terms). */
uint64_t radnet_head_tail_scratch_bytes(int32_t r);
int radnet_head_tail_fwd(radnet_ctx* ctx, const float* y5, int32_t r, int32_t hw, int32_t c, const float* w, int32_t ldw, const float* b,
                         int32_t nc, int32_t nreg, float* feat, float* p_cls, float* p_regr, const float* y1, const float* y2,
                         float* dz, float* losses, int32_t groups, const int32_t* group_live, void* scratch);

/* ---- losses (losses.py) ----------------------------------------------------------------------
 * RPN (losses.py:16-66): pred [m][ld_pred] holds the sigmoid class scores in columns [0,A) and the
 * regression outputs in [A,5A) (the fused head GEMM's layout); y_cls [m][2A], y_regr [m][8A].
 * losses[0..1] = (cls, regr).  dz [m][ld_dz]: gradient w.r.t. the PRE-activation outputs, same
 * column layout (sigmoid' folded in), columns >= 5A zeroed.
 * bce_mode 0: K.binary_crossentropy argument order as executed under Keras 2 (target=y_pred,
 * output=y_true) -- what the reference runs; 1: textbook BCE(y_true, clip(p)). */
int radnet_rpn_loss(radnet_ctx* ctx, const float* pred, int32_t ld_pred, const float* y_cls, const float* y_regr,
                    int32_t m, int32_t a, int32_t bce_mode, float* dz, int32_t ld_dz, float* losses,
                    double* scratch8);
/* Detector (losses.py:69-95): p_cls [r][nc] softmax, p_regr [r][nreg], y1 [r][nc], y2 [r][2*nreg].
 * losses[0..2] = (cls, regr, accuracy).  dz [r][nc+nreg] w.r.t. logits / regression outputs. */
int radnet_det_loss(radnet_ctx* ctx, const float* p_cls, const float* p_regr, const float* y1, const float* y2,
                    int32_t r, int32_t nc, int32_t nreg, float* dz, float* losses);

/* ---- optimizer: keras.optimizers.Adam over one flat arena (train.py:236-252) -----------------
 * zero_grad != 0: the gradient arena is cleared in the same pass (each value is read once and overwritten with 0),
 * so the next step's backward can accumulate into it without a separate memset.
 * All four entry points share one argument check: n a multiple of 4, t >= 1, and p, g, m, v 16-byte aligned (every path reads
 * float4; whole allocations are) -- otherwise a negative code, a message that names the entry point, and nothing is launched. */
int radnet_adam_step(radnet_ctx* ctx, float* p, float* g, float* m, float* v, int64_t n, int32_t t, float lr,
                     float beta1, float beta2, float eps, float grad_scale, int32_t zero_grad);
/* The same step with the folded epilogue shifts of the layers whose biases live in p[bias_off, bias_off + bias_len) refreshed in the
 * same pass: shift[j] = scale[j] * p[bias_off + j] + t0[j] (the radnet_affine_vec call that otherwise follows the update of trainable
 * convs with a frozen FixedBatchNormalization behind them, FixedBatchNormalization.py:59-85).  bias_off, bias_len multiples of 4. */
int radnet_adam_step_affine(radnet_ctx* ctx, float* p, float* g, float* m, float* v, int64_t n, int32_t t, float lr, float beta1, float beta2,
                            float eps, float grad_scale, int32_t zero_grad, int64_t bias_off, int64_t bias_len, const float* scale,
                            const float* t0, float* shift);
/* radnet_adam_step_affine (shift may be 0: no bias re-fold) that ALSO rewrites the Winograd F(4x4,3x3) filter transforms of up to twelve
 * 3x3 kernels that live in the arena -- dense [3][3][c][n] at float offset `off` -- into u [36][c][n], from the weights it has just
 * updated: the arithmetic of radnet_winograd4_filter on the new weights, in the optimizer's pass (the classifier's three 3x3 convs run
 * their training forward on U; a transform launch per layer and update cost the step what the Winograd forward gives). */
typedef struct radnet_adam_wino {
  int64_t off;           /* float offset of the kernel in the arena (multiple of 4) */
  int32_t c, n;          /* input / output channels; the kernel is dense: ldw == n  */
  float* u;              /* [36][c][n]                                              */
} radnet_adam_wino;
int radnet_adam_step_fused(radnet_ctx* ctx, float* p, float* g, float* m, float* v, int64_t n, int32_t t, float lr, float beta1, float beta2,
                           float eps, float grad_scale, int32_t zero_grad, int64_t bias_off, int64_t bias_len, const float* scale,
                           const float* t0, float* shift, const radnet_adam_wino* layers, int32_t n_layers);
/* What is left of that launch behind radnet_conv_wgrad_multi with its optimizer block, which has already stepped the kernels in front of
 * float offset sweep_from (> 0, a multiple of 4): Adam over [sweep_from, n) only -- biases with their folded shifts (the bias range must
 * not start in front of sweep_from), dense heads -- and, in the same launch, the filter transforms of the listed 3x3 kernels (all in
 * front of sweep_from) from the weights as they ARE: their workgroups read the kernels instead of stepping them.  The gradients, moments
 * and weights in front of sweep_from are not touched.  Same bits as radnet_adam_step_affine on the tail followed by
 * radnet_winograd4_filter per layer. */
int radnet_adam_step_tail(radnet_ctx* ctx, float* p, float* g, float* m, float* v, int64_t n, int32_t t, float lr, float beta1, float beta2,
                          float eps, float grad_scale, int32_t zero_grad, int64_t bias_off, int64_t bias_len, const float* scale,
                          const float* t0, float* shift, const radnet_adam_wino* layers, int32_t n_layers, int64_t sweep_from);
/* bf16-mixed training: radnet_adam_step_affine (shift may be 0: no bias re-fold) that ALSO rewrites the bf16 images of up to sixteen
 * conv kernels that live in the arena -- [k][ldw] fp32 at float offset `off` -- from the weights it has just updated:
 * wt[j][i] = bf16(p[off + i*ldw + j]) for i < k, j < n; 0 for k <= i < ldk (radnet_weights_to_bf16's layout and rounding).
 * Bit-identical to radnet_adam_step_affine / radnet_adam_step followed by radnet_weights_to_bf16 for each listed layer.
 * Needs ldw >= n, ldk >= k, ldw and off multiples of 4, ldk a multiple of 8, wt 16-byte aligned; layers inside the arena, not
 * overlapping each other or the bias range; at most 16 layers.  Otherwise a negative code and nothing is launched. */
typedef struct radnet_adam_bf16 {
  int64_t off;           /* float offset of the kernel [k][ldw] in the arena */
  int32_t k, n, ldw;     /* reduction length kh*kw*c, output columns of the image, row pitch of the fp32 kernel */
  uint16_t* wt;          /* bf16 image [n][ldk] */
  int32_t ldk;           /* >= k, a multiple of 8 */
} radnet_adam_bf16;
int radnet_adam_step_bf16(radnet_ctx* ctx, float* p, float* g, float* m, float* v, int64_t n, int32_t t, float lr, float beta1, float beta2,
                          float eps, float grad_scale, int32_t zero_grad, int64_t bias_off, int64_t bias_len, const float* scale,
                          const float* t0, float* shift, const radnet_adam_bf16* layers, int32_t n_layers);

/* ---- proposal decode + greedy NMS (rpn.py:68-172, 299-344, 380-455), fp64 ---------------------
 * pred: fused head output [rows*cols][ld_pred] (scores in [0,A), regression in [A,5A)).
 * anchor_wh: host array [A][2] of anchor (w,h) in feature-map units.
 * out_boxes [max_boxes][4] int64 (x1,y1,x2,y2), out_probs [max_boxes] fp32, out_count[1] int32.
 * ws: device scratch of >= radnet_proposals_ws_bytes(rows*cols*A) bytes. */
uint64_t radnet_proposals_ws_bytes(int64_t n_anchors_total);
int radnet_rpn_to_roi(radnet_ctx* ctx, const float* pred, int32_t ld_pred, int32_t rows, int32_t cols, int32_t a,
                      const double* anchor_wh_host, double std_scaling, int32_t use_regr, double overlap_thresh,
                      int32_t max_boxes, int64_t* out_boxes, float* out_probs, int32_t* out_count, void* ws);
/* Generic greedy NMS on n boxes [n][4] fp64 xyxy + probs fp32 (rpn.py:380-455).  out_idx [max_boxes]
 * indices into the input.  Malformed boxes (x1>=x2 or y1>=y2) set out_count to -1 (the reference asserts). */
int radnet_nms(radnet_ctx* ctx, const double* boxes, const float* probs, int32_t n, double overlap_thresh,
               int32_t max_boxes, int32_t* out_idx, int32_t* out_count, void* ws);

/* ---- anchor targets: utils.calc_region_props before the random subsampling (utils.py:585-766) --
 * gt [g][4] fp64 (x1,y1,x2,y2) in SOURCE-image pixels, gt_is_bg [g].  anchor_sizes host [ns],
 * anchor_ratios host [nr][2].  Outputs (A = ns*nr): valid, overlap uint8 [A][fh][fw] (the NCHW order
 * the host subsampler indexes), regr fp64 [fh][fw][4A], best_anchor int32 [g][4] (jy,ix,ratio,size)
 * or -1, n_for_gt int32 [g].  scratch: >= 8*g bytes. */
int radnet_anchor_targets(radnet_ctx* ctx, const double* gt, const int32_t* gt_is_bg, int32_t g, int32_t width,
                          int32_t height, int32_t rw, int32_t rh, int32_t fw, int32_t fh, const double* anchor_sizes_host,
                          int32_t ns, const double* anchor_ratios_host, int32_t nr, double rpn_stride,
                          double max_overlap, uint8_t* valid, uint8_t* overlap, double* regr, int32_t* best_anchor,
                          int32_t* n_for_gt, void* scratch);
/* utils.py:815-816 + 475-478: y_cls [fh][fw][2A] = [valid || overlap], y_regr [fh][fw][8A] =
 * [repeat(overlap,4) || regr*std_scaling], fp32 NHWC. */
int radnet_anchor_targets_pack(radnet_ctx* ctx, const uint8_t* valid, const uint8_t* overlap, const double* regr,
                               int32_t fw, int32_t fh, int32_t a, double std_scaling, float* y_cls, float* y_regr);

/* ---- RoI labelling: rpn.calc_iou (rpn.py:176-296) ----------------------------------------------
 * rois int64 [n][4] xyxy (feature-map units), gt as above + gt_cls int32 [g] class index.
 * Per RoI: keep (0/1), cls (class index; bg for hard negatives), box int32 [4] (x,y,w,h),
 * t fp64 [4] = (sx*tx, sy*ty, sw*tw, sh*th) (zeros unless foreground), iou fp64. */
int radnet_roi_targets(radnet_ctx* ctx, const int64_t* rois, int32_t n, const double* gt, const int32_t* gt_cls, int32_t g,
                       int32_t width, int32_t height, int32_t rw, int32_t rh, double rpn_stride, double min_overlap,
                       double max_overlap, const double* regr_std_host4, int32_t bg_class, uint8_t* keep, int32_t* cls,
                       int32_t* box, double* t, double* iou, const int32_t* n_dev);
/* ^ cls is -1 for dropped RoIs.  n_dev (optional device int32): only the first min(*n_dev, n) rows are labelled,
 *   so the NMS count never has to travel to the host between the two kernels.
 *   max_overlap must be > 0: the call is refused otherwise (an RoI that overlaps nothing would be foreground without a box). */
/* Build the detector batch for `r` selected RoIs: rois_out fp32 [r][4], y1 [r][nc], y2 [r][8(nc-1)].  r = 0 writes nothing. */
int radnet_roi_batch_pack(radnet_ctx* ctx, const int32_t* sel, int32_t r, const int32_t* cls, const int32_t* box,
                          const double* t, int32_t nc, int32_t bg_class, float* rois_out, float* y1, float* y2);

/* ---- host-only helper (HOST pointers, no GPU work) ------------------------------------------------
 * One round of NumPy's legacy RandomState.choice(n, size, replace=False, p=p) as used by utils.py:797,812.
 * live_p / live_idx [*n_live_io]: the still non-zero probabilities and their indices (increasing); the round does
 * cumsum + normalise over them (bit-identical to NumPy's cumsum over the full p: zeroed entries add 0.0), maps the
 * k uniforms `x` (drawn by the caller with np.random.random_sample, so the global MT19937 stream is consumed
 * exactly as NumPy would) through searchsorted(side='right'), appends first occurrences to found[n_found...] and
 * removes them from the live lists.  Returns the number appended.  cdf: scratch [n] doubles; sel: scratch [n] bytes. */
int64_t radnet_host_choice_round(double* live_p, int64_t* live_idx, int64_t* n_live_io, int64_t* found, int64_t n_found,
                                 const double* x, int64_t k, double* cdf, uint8_t* sel);

/* ---- small utilities ---------------------------------------------------------------------------- */
/* uint8 BGR HWC image -> fp32 NHWC with `cpad` channels (zeros beyond 3), minus the caffe BGR means
 * (RADNet.py:83-87 / utils.py:468-472 with keras 'caffe' preprocess_input).  cpad >= 3; RADNET_ERR_ARG for h < 1 or w < 1. */
int radnet_preprocess_bgr(radnet_ctx* ctx, const uint8_t* img, int32_t h, int32_t w, int32_t cpad, float* out);
/* dst[0..bytes) = src[0..bytes) by a kernel on the context's stream; either side may be pinned host memory (hipHostMalloc /
 * torch pin_memory: mapped into the device's address space).  The step's small transfers between host and device (image panel
 * in, anchor label maps out and back, RoI class codes out: utils.py:777-813, train.py:300-330 run on the host in the reference)
 * go through this instead of hipMemcpyAsync: an asynchronous copy enqueued on a stream with a few layer programs in arrears
 * was measured to block the enqueuing host thread for 7-11 ms (tools/fill_drain_probe.py); a kernel launch never did. */
int radnet_copy_bytes(radnet_ctx* ctx, void* dst, const void* src, uint64_t bytes);
/* cv2.resize(img, (dw, dh), interpolation=INTER_CUBIC) for uint8 HWC images (RADNet.py:72, utils.py:442-446):
 * a = -0.75 bicubic, half-pixel centres, replicated borders, OpenCV's 11-bit fixed-point arithmetic.
 * Parity unpinned (OpenCV absent offline). */
int radnet_resize_bicubic_u8(radnet_ctx* ctx, const uint8_t* src, int32_t sh, int32_t sw, uint8_t* dst, int32_t dh,
                             int32_t dw, int32_t channels);
/* The tile cut and the resize of the predict tile loop in ONE launch, for an image that is already on the device (RADNet.py:545-547:
 * np.copy(img[ty0:ty1, tx0:tx1, :]) then format_img's cv2.resize; RADNet.py:348-350: the full-image pass, the window that covers
 * the image).  dst (dh x dw x channels, contiguous) receives exactly the bytes radnet_resize_bicubic_u8 writes for a contiguous
 * copy of the window src[y0:y0+wh, x0:x0+ww, :] of the sh x sw image: the four taps replicate at the WINDOW's edges, not the
 * image's (a tile from the middle of a scan never sees its neighbours' pixels), the scale factors come from (wh, ww) -> (dh, dw),
 * and with (dh, dw) == (wh, ww) the output is the window's bytes (coefficients exactly 0, 2048, 0, 0).  The kernel never reads
 * outside the window.  RADNET_ERR_ARG, and nothing is launched, when ctx, src or dst is null, any extent is below 1, y0 < 0,
 * x0 < 0, y0 + wh > sh or x0 + ww > sw. */
int radnet_resize_bicubic_window_u8(radnet_ctx* ctx, const uint8_t* src, int32_t sh, int32_t sw, int32_t y0, int32_t x0, int32_t wh,
                                    int32_t ww, uint8_t* dst, int32_t dh, int32_t dw, int32_t channels);
/* cv2.warpAffine(src, M, (dw, dh)) with its defaults (INTER_LINEAR, BORDER_CONSTANT 0) for uint8 HWC tiles: the +-3 degree rotation
 * and the shear of the train-time augmentation (augmentation.py:158-271).  The caller inverts M and passes the inverse map's
 * per-column and per-row terms in 10-bit fixed point, rounded in float64 as OpenCV does: col_tab = {adelta[dw], bdelta[dw]},
 * row_tab = {x0[dh], y0[dh]} (device int32 arrays; faster_rcnn/augmentation.py:warp_tables builds them).  Bit-identical to that
 * module's NumPy restatement; against OpenCV itself unpinned (absent here). */
int radnet_warp_affine_u8(radnet_ctx* ctx, const uint8_t* src, int32_t sh, int32_t sw, int32_t channels, uint8_t* dst, int32_t dh,
                          int32_t dw, const int32_t* col_tab, const int32_t* row_tab);
/* ---- train-time tile augmentation on the device (csrc/augment.hip) -------------------------------------------------------
 * The image operations of faster_rcnn/augmentation.py for a tile that stays on the device from crop to network input
 * (faster_rcnn/augmentation_device.py drives them; the +-3 degree rotation and the shear use radnet_warp_affine_u8, the final
 * resize radnet_resize_bicubic_u8).  All images are uint8 HWC with 3 channels, contiguous, any extent >= 1 x 1.  Integer
 * atomics only: results are reproducible run to run. */
/* dst[y][x][c] = src[map(y, x)][c]: the window [y0, y0 + wh) x [x0, x0 + ww) of the sh x sw source under one of the eight
 * dihedral transforms.  transform: bit 2 transposes the window first, then bit 0 reverses the rows and bit 1 the columns of
 * the result; dst is wh x ww, or ww x wh when bit 2 is set.  0 with a window: the tile crop (utils.py:420) and the strap slice
 * img[row_min:row_max, col_min:col_max] (augmentation.py:209, 262); 1 / 2 / 3: cv2.flip codes 0 / 1 / -1, i.e. vertical_flip
 * (augmentation.py:101-115), horizontal_flip (augmentation.py:85-99) and the 180 degree case; 6 / 5: the 90 / 270 degree cases
 * of ninety_degree_rotation (augmentation.py:117-156: transpose, then flip 1 / 0); 4 the bare transpose, 7 the anti-transpose. */
int radnet_aug_gather_u8(radnet_ctx* ctx, const uint8_t* src, int32_t sh, int32_t sw, int32_t y0, int32_t x0, int32_t wh, int32_t ww,
                         int32_t transform, uint8_t* dst);
/* strap_img (augmentation.py:17-31): out4 = {row_min, row_max, col_min, col_max} (device int32) of the pixels whose channel 1 is
 * non-zero; {INT32_MAX, -1, INT32_MAX, -1} when there is none (the caller raises what the host function raises).  uint8 holds no
 * non-finite value: that branch of the host function has no device form. */
int radnet_aug_extent_u8(radnet_ctx* ctx, const uint8_t* img, int32_t h, int32_t w, int32_t* out4);
/* bins256[v] (device uint32, overwritten) = number of elements equal to v over channel 0 (all_channels = 0) or over all three:
 * per-workgroup bins in LDS, integer adds to global memory.  The host derives from it what brightness (augmentation.py:303-333:
 * sum and count of the non-zero elements -> the foreground mean) and the poisson mode (augmentation.py:443-478 through
 * skimage.util.random_noise: the number of distinct values) decide on; h * w * channels < 2^32. */
int radnet_aug_histogram_u8(radnet_ctx* ctx, const uint8_t* img, int32_t h, int32_t w, int32_t all_channels, uint32_t* bins256);
/* The pointwise modes, one launch each; src == dst is allowed.  Background -- exact zeros of the input, per element, or per pixel of
 * channel 0 when `grey` -- stays zero, as brightness and the shared tail of the noise functions restore it; with `grey`
 * ("grey" in C.img_types[0]; noise modes only) ONE plane computed from channel 0 is written to all three channels.
 *   RADNET_AUG_BRIGHTNESS (augmentation.py:303-333): f = float(v); f -= d (p1 != 0) or f += d (p1 == 0) in fp32 with d = (float)p0,
 *     the host's delta; clip to [0, 255]; truncate.
 *   RADNET_AUG_CONTRAST (augmentation.py:335-351, skimage.exposure.rescale_intensity in fp64): f = clip(v, lo = p0, hi = p1);
 *     f = (f - lo) / (hi - lo) unless lo == hi; truncate f * 255.0.  No background restore (0 maps to 0 for lo >= 0 anyway).
 *   The noise modes (augmentation.py:353-478: skimage.util.random_noise + img_as_ubyte in fp64): x = v / 255.0, the mode, clip
 *     to [0, 1], rint(x * 255) half-to-even.  scikit-image draws the field from a generator the reference never seeds -- only the
 *     distribution is specified -- so the device has a reproducible field of its own, Philox4x32-10 (multipliers 0xD2511F53,
 *     0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85; ten rounds): key = low and high half of `noise_seed`; counter =
 *     (element_index_lo, element_index_hi, field_id, 0), element_index the row-major index in the field's own shape (H x W with
 *     `grey`, H x W x 3 otherwise), field_id the sample's ordinal in the feed.  The output words x0..x3 give two uniforms, in fp64
 *     as written: u_a = ((((x0 << 32) | x1) >> 11) + 0.5) * 2^-53 and u_b likewise from x2, x3.
 *   RADNET_AUG_SALT_PEPPER: hit = u_a <= amount (p0), salt = u_b <= salt_vs_pepper (p1); a hit becomes 1 (salt) or 0.
 *   RADNET_AUG_GAUSSIAN: z = sqrt(-2 ln u_a) * cos(2 pi u_b); x + (mean + sigma * z), p0 = mean, p1 = sigma = sqrt(var) rounded
 *     once on the host.
 *   RADNET_AUG_POISSON: lam = x * v (p0 = v = 2 ** ceil(log2(#distinct values)), 1 <= v <= 256); the CDF is walked in fp64: p = s =
 *     exp(-lam), k = 0, while u_a > s and k < 1023: k += 1, p *= lam / k, s += p; the result is k / v. */
#define RADNET_AUG_BRIGHTNESS 0
#define RADNET_AUG_CONTRAST 1
#define RADNET_AUG_SALT_PEPPER 2
#define RADNET_AUG_GAUSSIAN 3
#define RADNET_AUG_POISSON 4
int radnet_aug_pointwise_u8(radnet_ctx* ctx, const uint8_t* src, uint8_t* dst, int32_t h, int32_t w, int32_t mode, int32_t grey, double p0,
                            double p1, uint64_t noise_seed, uint32_t field_id);
/* ---- PNG images onto the device (csrc/png.hip) ------------------------------------------------------------------------------
 * faster_rcnn/png.py reads the container and inflates the IDAT stream on the host; the per-byte work runs here, on the inflated
 * stream after ONE upload: per pass (one for a non-interlaced file, up to seven for Adam7) a reconstruction launch and an
 * expansion launch.  A pass is pass_h scanlines of 1 + rowbytes bytes: the filter-type byte, then the packed samples.  The result
 * is what cv2.imdecode(buf, cv2.IMREAD_COLOR) returns, uint8 [dst_h][dst_w][3] in B, G, R order; both steps restate the PNG
 * specification and libpng's documented transforms as OpenCV requests them -- against OpenCV itself unpinned (absent here). */
/* Scanline reconstruction (PNG specification, section 9) IN PLACE on one pass: rows x (1 + rowbytes) bytes at `stream`; the filter-type
 * bytes stay, every other byte x becomes Recon(x) = x + predictor modulo 256 with a = the reconstructed byte bpp to the left, b = the
 * one above, c = the one above a (0 left of the row and above row 0): type 0 None 0; 1 Sub a; 2 Up b; 3 Average floor((a + b) / 2)
 * on the 9-bit sum; 4 Paeth p = a + b - c, the first of a, b, c (in that order, compared with <=) nearest to p.
 * bpp = max(1, channels * bit_depth / 8), one of 1, 2, 3, 4, 6, 8, and divides rowbytes.  A filter-type byte above 4 is the CALLER's
 * to refuse (png.py checks the column on the host); the kernel treats it as None.  One workgroup walks the pass in bands of
 * RADNET_PNG_UNFILTER_BAND_ROWS rows, one lane per row, each row one pixel behind the row above, and moves row data between global
 * memory and LDS in chunks of RADNET_PNG_UNFILTER_CHUNK_BYTES per row: the seams tests/test_gpu_png.py straddles.  Nothing waits
 * on another workgroup; the loop bounds depend on (rows, rowbytes, bpp) alone.  One workgroup is one CU: for whole files, and for
 * many at once, radnet_png_unfilter_segments_u8 below spreads the same walk over the device, and radnet_png_unfilter_tiles_u8 (further
 * down) does so for rows of Up / Average / Paeth type, which allow no segment cut. */
#define RADNET_PNG_UNFILTER_BAND_ROWS 512
#define RADNET_PNG_UNFILTER_CHUNK_BYTES 96
int radnet_png_unfilter_u8(radnet_ctx* ctx, uint8_t* stream, int32_t rows, int32_t rowbytes, int32_t bpp);
/* ---- many passes in one launch: segments ----
 * The only bytes a scanline takes from the row above are its b and c, and filter types 0 (None) and 1 (Sub) use neither.  So a row
 * of type 0 or 1 reconstructs to the same bytes whatever stands above it, and the rows from it up to the next such row form a run
 * that can be reconstructed on its own, the row above its first row counting as zeros, exactly as above row 0 of a pass.  A segment
 * is one or more adjacent runs of one pass.  A file whose rows are all Up / Average / Paeth has one segment per pass. */
typedef struct radnet_png_segment {
  int64_t offset;   /* of the filter-type byte of the segment's first scanline in the uploaded buffer */
  int32_t rows;     /* scanlines in the segment */
  int32_t rowbytes; /* of its pass: a scanline is 1 + rowbytes bytes */
} radnet_png_segment;
/* the planner's default target_rows: the reconstruction runs one lane per row, so 64 rows fill one wave */
#define RADNET_PNG_SEGMENT_TARGET_ROWS 64
/* Host only (csrc/png_plan.cpp; no context, no device, like radnet_chain_check): cuts one pass into segments.  `stream` points at
 * the pass's first scanline in HOST memory (rows x (1 + rowbytes) bytes, of which only the filter-type bytes are read);
 * stream_offset is where that byte will stand in the uploaded buffer, so out[0].offset == stream_offset and a segment that starts at
 * row r has offset stream_offset + r * (1 + rowbytes).  A legal cut is in front of row 0 or of a row of type 0 or 1.  Greedy: a
 * segment ends at the last legal cut that keeps it within target_rows rows (0 = RADNET_PNG_SEGMENT_TARGET_ROWS), at the end of the
 * pass if that is within target_rows, else at the next legal cut (or the end of the pass).  The segments tile the pass in row
 * order.  If that makes more than cap segments, adjacent ones are merged, evenly by count, into exactly cap: never an error.
 * Returns the number of segments written, or RADNET_ERR_ARG for a null pointer, rows / rowbytes / cap < 1, a negative
 * stream_offset or target_rows, or a filter-type byte above 4 (nothing is written then). */
int radnet_png_plan_segments(const uint8_t* stream, int64_t stream_offset, int32_t rows, int32_t rowbytes, int32_t target_rows,
                             radnet_png_segment* out, int32_t cap);
/* radnet_png_unfilter_u8 on `count` segments of the buffer base[0 .. base_len) (device), which may come from any passes of any
 * images that share bpp: the same bytes as one radnet_png_unfilter_u8 per pass when every segment starts at a legal cut (the
 * caller's to ensure, with the planner; the filter-type bytes above 4 likewise).  segs_host and segs_dev hold the SAME table, on the
 * host and on the device; the caller uploads it (png.py: behind the streams in the one staging buffer, as the palette) and this
 * entry copies nothing.  The host table is validated before anything is launched: rows > 0, rowbytes > 0, rowbytes % bpp == 0,
 * offset >= 0, offset + rows * (1 + rowbytes) <= base_len; a violation is RADNET_ERR_ARG naming the segment's index and nothing
 * is modified.  Segments must not overlap (not checked; overlapping ones race on bytes inside the buffer).  count == 0 is
 * RADNET_OK without a launch, whatever the pointers.
 * The table may be in any order.  At most two launches, one workgroup per table entry, nothing waits on another workgroup:
 * segments of at most 64 rows run as one wave with a 6.5 KB LDS tile (many per CU), longer ones as the band-sized workgroup of
 * radnet_png_unfilter_u8.  Each launch spans the index range from the first to the last entry of its kind and a workgroup that
 * finds an entry of the other kind returns at once, so a table with the short segments first and the long ones last starts no
 * idle workgroup. */
int radnet_png_unfilter_segments_u8(radnet_ctx* ctx, uint8_t* base, int64_t base_len, const radnet_png_segment* segs_host,
                                    const radnet_png_segment* segs_dev, int32_t count, int32_t bpp);
/* Expansion of one reconstructed pass: pixel (r, c) of the pass_h x pass_w pass goes to dst[y0 + r * dy][x0 + c * dx] (a
 * non-interlaced image: y0 = x0 = 0, dy = dx = 1; Adam7: the pass's origin and spacing).  colour types 0 (grey; depth 1, 2, 4, 8, 16),
 * 2 (RGB; 8, 16), 3 (palette; 1, 2, 4, 8), 4 (grey + alpha; 8, 16), 6 (RGBA; 8, 16).  Sub-byte samples unpack MSB first; grey is
 * replicated to the three channels, depths 1 / 2 / 4 scaled by 255 / 85 / 17; a 16-bit sample keeps its high byte (libpng's
 * strip_16); alpha is dropped, not blended; a palette index selects palette_bgr[index] (device, 256 x 3 bytes in B, G, R order,
 * entries beyond the file's PLTE zero; ignored for the other colour types and may then be null).  No gamma, sBIT, tRNS or
 * background handling.  The pass must lie inside dst and rowbytes must hold pass_w pixels: refused otherwise, never read or
 * written out of bounds. */
int radnet_png_expand_bgr_u8(radnet_ctx* ctx, const uint8_t* stream, int32_t pass_h, int32_t pass_w, int32_t rowbytes, int32_t color_type,
                             int32_t bit_depth, const uint8_t* palette_bgr, uint8_t* dst, int32_t dst_h, int32_t dst_w, int32_t y0,
                             int32_t x0, int32_t dy, int32_t dx);
/* ---- device images out to PNG files: the forward filter (csrc/png.hip) and rectangles (csrc/draw.hip) ------------------------------
 * faster_rcnn/png.py writes the container and deflates on host threads; the per-byte work on the image runs here, where the image
 * already is (RADNet.predict leaves it on the device). */
/* The forward filter of the PNG specification (section 9), from a device image to the scanline stream radnet_png_unfilter_u8 consumes:
 * stream receives h rows of 1 + w * channels bytes, the filter-type byte and then Filt(x) = x - predictor modulo 256 with the
 * predictors stated at radnet_png_unfilter_u8 over the RAW bytes (a = bpp to the left, b = above, c = above-left; 0 left of the row
 * and above row 0), bpp = channels.  img is h rows of pitch_bytes bytes (pitch_bytes >= w * channels; the padding is not read);
 * channels == 3: a B, G, R image whose bytes are written as R, G, B (colour type 2, depth 8); channels == 1: the bytes as they are
 * (colour type 0).  mode 0..4: that type for every row.  mode 5, adaptive: per row the type whose residual bytes v have the smallest
 * sum of min(v, 256 - v); on a tie the lowest type.  The sums are integers; w * channels above 2^24 is RADNET_ERR_UNSUPPORTED so that
 * they fit 32 bits.  `stream` needs no alignment (its rows start at every byte offset anyway) and must not overlap img.  A null
 * pointer, h or w below 1, channels other than 1 and 3, a mode outside 0..5 or a short pitch is RADNET_ERR_ARG and nothing is
 * launched.  One workgroup per row, one launch; every row reads raw bytes only, so rows do not wait for each other. */
int radnet_png_filter_rows_u8(radnet_ctx* ctx, const uint8_t* img, int32_t h, int32_t w, int32_t channels, int64_t pitch_bytes, int32_t mode,
                              uint8_t* stream);
/* ---- deflate of the scanline stream on the device (csrc/deflate.hip, csrc/deflate_plan.cpp): run-length tokens, one Huffman code ---
 * What zlib's Z_RLE strategy does (matches at distance 1 only), restated so that a position's token depends on nothing but the run
 * it sits in.  THE TOKEN RULE: the stream of n bytes is cut into chunks of RADNET_DEFLATE_CHUNK bytes; each chunk becomes one
 * deflate block, one "piece".  Inside a chunk, runs are additionally cut at multiples of RADNET_DEFLATE_TILE bytes (counted from the
 * chunk's start), so a token never needs bytes beyond its tile.  A maximal run of L equal bytes b inside a tile is coded as
 *   the literal b; then floor((L - 1) / 258) matches of length 258 at distance 1; then the rest r = (L - 1) mod 258: one match of
 *   length r at distance 1 if r >= 3, else r literals b.
 * The rule is deterministic: tests/deflate_cases.py states it in Python and the kernels are compared with it byte for byte.
 * A code is a table of 286 literal/length symbols (RFC 1951, 3.2.5): `bits` the canonical code as RFC 1951 3.2.2 numbers it (its most
 * significant bit goes into the stream first), `length` its length in bits, 0 for a symbol that does not occur. */
#define RADNET_DEFLATE_CHUNK 65536
#define RADNET_DEFLATE_TILE 4096
#define RADNET_DEFLATE_SYMBOLS 286
#define RADNET_DEFLATE_HEADER_MAX_BITS 2048
typedef struct radnet_deflate_code {
  uint16_t bits, length;
} radnet_deflate_code; /* 4 bytes */
/* First pass over the stream (device, n bytes): one workgroup per chunk tokenises by the rule above and ADDS the counts of the
 * literal/length symbols, one end-of-block (256) per chunk included, to hist[286] (device, uint32; the caller zeroes it; integer
 * atomics, so the result does not depend on the order).  adler_parts (device, uint64 [chunks][2], 8-byte aligned) receives per chunk
 * of len bytes the two exact sums  sum(byte[i])  and  sum((len - i) * byte[i]),  i counted from the chunk's start: the host combines
 * them into the Adler-32 of the stream without seeing it.  chunks = ceil(n / RADNET_DEFLATE_CHUNK).  A null pointer or n < 1 is
 * RADNET_ERR_ARG, n >= 2^32 (a count could leave 32 bits) RADNET_ERR_UNSUPPORTED; nothing is launched then. */
int radnet_deflate_rle_scan_u8(radnet_ctx* ctx, const uint8_t* stream, int64_t n, uint32_t* hist, uint64_t* adler_parts);
/* Second pass: one workgroup per chunk writes piece c to pieces + c * piece_cap (device) and its size in bytes to sizes[c] (device,
 * uint32).  A piece holds, from its bit 0 on (bits fill a byte from its least significant end, RFC 1951 3.1.1):
 *   header_bits[0 .. header_nbits): the caller's block header -- BFINAL = 0, BTYPE and, for a dynamic block, the code description;
 *   the tokens of the chunk: Huffman codes most significant bit first, a length symbol's extra bits least significant bit first,
 *     and after every match the distance code of distance 1: dist_nbits zero bits (1 for radnet_deflate_build_code's table, 5 for
 *     the fixed code);
 *   end-of-block;
 *   then a sync flush, the empty stored block: 000, zero bits up to the byte, 00 00 FF FF.  The LAST piece instead has BFINAL = 1
 *     (bit 0 of the piece is set) and zero bits up to the byte, no stored block.
 * Bit offsets come from a workgroup prefix sum of per-position bit counts.  Bits no code covers are zero; no byte at or beyond
 * sizes[c] is written.  `code` (286 entries) and header_bits (ceil(header_nbits / 8) bytes) are HOST memory and travel with the
 * launch; the code is data, so the fixed code of RFC 1951 3.2.6 is one more table (header 3 bits, BTYPE 01) and any legal table
 * works.  The caller answers for a table that gives a length to every symbol radnet_deflate_rle_scan_u8 counted.
 * piece_cap must be at least radnet_deflate_piece_cap(code, header_nbits, dist_nbits).  RADNET_ERR_ARG and nothing is launched: a
 * null pointer, n < 1, a code length outside 0..15, bits that do not fit the length, a zero length for end-of-block (256),
 * header_nbits outside 3..RADNET_DEFLATE_HEADER_MAX_BITS, dist_nbits outside 0..15, a short piece_cap; n >= 2^32 is
 * RADNET_ERR_UNSUPPORTED. */
int radnet_deflate_rle_emit_u8(radnet_ctx* ctx, const uint8_t* stream, int64_t n, const radnet_deflate_code* code, const uint8_t* header_bits,
                               int32_t header_nbits, int32_t dist_nbits, uint8_t* pieces, int64_t piece_cap, uint32_t* sizes);
/* Host only (csrc/deflate_plan.cpp; no context, no device): the bound a piece cannot pass,
 *   ceil(header_nbits / 8) + ceil(w * RADNET_DEFLATE_CHUNK / 8) + 16,
 * w = the larger of the longest code length and ceil((longest length-symbol code + 5 extra bits + dist_nbits) / 3): a literal costs
 * at most the first per byte, a match covers three bytes at least; from a longest code of 9 bits on (the fixed code, every code of
 * an image) w is the longest code length.  The 16 hold end-of-block and the sync flush.  Negative (RADNET_ERR_ARG) for the table,
 * header_nbits and dist_nbits that radnet_deflate_rle_emit_u8 refuses. */
int64_t radnet_deflate_piece_cap(const radnet_deflate_code* code, int32_t header_nbits, int32_t dist_nbits);
/* The pieces one behind the other: out[0 .. total) (device) = piece 0, piece 1, ... by an exclusive prefix sum of sizes[0 .. count),
 * and *total (device, uint64) = their sum.  The host reads the 8 bytes of total and then downloads exactly that many.  Nothing is
 * written at or beyond out + out_cap: if *total > out_cap the copy is cut there and the caller sees it from total.  One launch, a
 * workgroup per piece; each sums the sizes in front of its own (count^2 / 2 reads of 4 bytes in all, from the caches).  A null
 * pointer, count < 1, piece_cap < 1 or out_cap < 0 is RADNET_ERR_ARG, count > 65536 (more than n < 2^32 gives) RADNET_ERR_UNSUPPORTED. */
int radnet_deflate_pack(radnet_ctx* ctx, const uint8_t* pieces, int64_t piece_cap, const uint32_t* sizes, int32_t count, uint8_t* out,
                        int64_t out_cap, uint64_t* total);
/* Host only (csrc/deflate_plan.cpp; no context, no device, like radnet_png_plan_segments): from the 286 counts of
 * radnet_deflate_rle_scan_u8 a literal/length code of at most 15 bits per symbol and the dynamic block header that describes it.
 * A symbol with a count gets a length; end-of-block always does; with fewer than two such symbols literal 0 (or 1) joins them, so
 * the code is COMPLETE -- the Kraft sum of 2^-length is exactly 1 -- as zlib's inflate demands.  Lengths are Huffman's, and where
 * the tree is deeper than 15, shortened to 15 and repaired to a Kraft sum of 1; codes are canonical (RFC 1951 3.2.2).
 * header receives ceil(*header_nbits / 8) bytes, unused bits zero: BFINAL 0, BTYPE 10, HLIT 29, HDIST 0, HCLEN 15; the code-length
 * code gives 4 bits to each of its symbols 0..15 and none to 16..18 (complete); then the 286 lengths and the one distance length,
 * 1 for distance symbol 0, four bits each: 1222 bits.  A match's distance code is therefore one zero bit (dist_nbits = 1).
 * A null pointer or header_cap < 153 is RADNET_ERR_ARG and nothing is written. */
int radnet_deflate_build_code(const uint32_t* hist, radnet_deflate_code* code, uint8_t* header, int32_t header_cap, int32_t* header_nbits);
/* ---- deflate with far matches on the device (csrc/deflate_lz.hip, csrc/deflate_plan.cpp): LZ77 tokens, two Huffman codes -------------
 * The section above restated with matches at any distance of deflate's window.  THE LZ TOKEN RULE, constants first: */
#define RADNET_DEFLATE_LZ_GROUP 256
#define RADNET_DEFLATE_LZ_FAR_MIN 10
#define RADNET_DEFLATE_LZ_FAR_MIN2 12
#define RADNET_DEFLATE_LZ_FAR_D 4096
#define RADNET_DEFLATE_DIST_SYMBOLS 30
/* Chunks and tiles: the stream is cut into chunks of RADNET_DEFLATE_CHUNK bytes, one chunk is one deflate block and one piece, as
 *   above.  No match reads in front of its chunk and none crosses a multiple of RADNET_DEFLATE_TILE counted from the chunk's start.
 *   Positions below are counted from the chunk's start.
 * Candidates of position p, up to three: distance 1 (p >= 1); distance `near`, an argument (p >= near; faster_rcnn/png.py passes the
 *   pixel stride, 3 for RGB and 1 for grey; near == 1 is the candidate above); the HASH CANDIDATE: the greatest q that lies in a
 *   GROUP in front of p's own and has H(q) == H(p).  Groups are RADNET_DEFLATE_LZ_GROUP positions; H(x) =
 *   ((the little-endian uint32 at x) * 2654435761 mod 2^32) >> 17, 15 bits, defined only while x + 4 <= the chunk's end (p has no
 *   hash candidate beyond that).  The hash candidate is refused when p - q > 32768.  Only earlier groups are sources, so the table
 *   of greatest positions is kept per group by "read, barrier, integer max, barrier" and needs no sort: 2^15 entries of 16 bits,
 *   64 KiB of LDS beside the 64 KiB of the chunk's bytes, within the 160 KiB of a CU.
 * Length of a candidate: the number of equal bytes byte[p + i] == byte[p + i - distance], i = 0, 1, ..., at most 258 and at most
 *   the bytes left in p's tile; a source that overlaps the position (distance < length) is legal.
 * Acceptance: distances 1 and `near` from 3 bytes; the hash candidate from RADNET_DEFLATE_LZ_FAR_MIN bytes when its distance is at
 *   most RADNET_DEFLATE_LZ_FAR_D, from RADNET_DEFLATE_LZ_FAR_MIN2 bytes beyond.
 * Choice: the longest accepted candidate; on equal length the smaller distance.
 * Parse: greedy from every tile's start -- the token at p is the chosen match, or the literal byte[p] when there is none; the next
 *   token is at p + max(1, length).
 * The rule is deterministic and depends on no launch order: tests/deflate_lz_cases.py states it in Python and the kernels are
 * compared with it byte for byte.  The constants were chosen with that model.
 * THE TOKEN TABLE: one uint32 per stream byte -- 0: the position is covered by a match that starts in front of it; 1 << 31: a
 * literal starts here; 1 << 31 | length << 16 | (distance - 1): a match starts here (length 3..258, distance 1..32768). */
/* First pass (device): one workgroup per chunk finds the candidates and parses the chunk.  tokens (device, uint32 [n], 16-byte
 * aligned) receives the token table; hist_ll[286] and hist_d[30] (device, uint32; the caller zeroes them; integer atomics) have the
 * counts of the literal/length symbols, one end-of-block per chunk included, and of the distance symbols (RFC 1951 3.2.5) ADDED;
 * adler_parts as radnet_deflate_rle_scan_u8 writes them.  near: 1..32768.  A null pointer, n < 1, near outside 1..32768 or a
 * misaligned table is RADNET_ERR_ARG, n >= 2^32 RADNET_ERR_UNSUPPORTED; nothing is launched then. */
int radnet_deflate_lz_scan_u8(radnet_ctx* ctx, const uint8_t* stream, int64_t n, int32_t near, uint32_t* tokens, uint32_t* hist_ll, uint32_t* hist_d,
                              uint64_t* adler_parts);
/* Second pass: the pieces of radnet_deflate_rle_emit_u8 -- its layout, sync flush, BFINAL, bit order and "no byte at or beyond
 * sizes[c]" -- from the token table of the first pass (device, 16-byte aligned; the caller answers for a table that pass wrote for
 * this stream).  A match is its length symbol's code, that symbol's extra bits, the distance symbol's code out of code_d (30
 * entries) and the distance's extra bits, least significant bit first (RFC 1951 3.2.5); a token takes at most 48 bits.  Bit offsets
 * come from a workgroup prefix sum over the token starts.  code_ll, code_d and header_bits are HOST memory.  piece_cap must be at
 * least radnet_deflate_lz_piece_cap(code_ll, code_d, header_nbits).  Refused as radnet_deflate_rle_emit_u8 refuses (code_d's
 * lengths and bits are checked like code_ll's); a misaligned table is RADNET_ERR_ARG. */
int radnet_deflate_lz_emit_u8(radnet_ctx* ctx, const uint8_t* stream, int64_t n, const uint32_t* tokens, const radnet_deflate_code* code_ll,
                              const radnet_deflate_code* code_d, const uint8_t* header_bits, int32_t header_nbits, uint8_t* pieces, int64_t piece_cap,
                              uint32_t* sizes);
/* Host only (csrc/deflate_plan.cpp; no context, no device).  From the counts of radnet_deflate_lz_scan_u8 two complete canonical
 * codes of at most 15 bits (built as radnet_deflate_build_code builds its one; with fewer than two used distance symbols, symbol 0
 * -- or 1 -- joins them) and the dynamic block header: BFINAL 0, BTYPE 10, HLIT 29, HDIST 29, HCLEN 15, the code-length code of
 * radnet_deflate_build_code, then the 286 + 30 lengths, four bits each: 17 + 57 + 316 * 4 = 1338 bits, 168 bytes.  A null pointer
 * or header_cap < 168 is RADNET_ERR_ARG and nothing is written. */
int radnet_deflate_build_codes_lz(const uint32_t* hist_ll, const uint32_t* hist_d, radnet_deflate_code* code_ll, radnet_deflate_code* code_d,
                                  uint8_t* header, int32_t header_cap, int32_t* header_nbits);
/* Host only: the bound an LZ piece cannot pass, ceil(header_nbits / 8) + ceil(w * RADNET_DEFLATE_CHUNK / 8) + 16 with w = the larger
 * of the longest literal/length code and ceil(the most bits a match can take / 3) -- a match covers three bytes at least, and takes
 * its two codes and their symbols' extra bits.  Negative (RADNET_ERR_ARG) for what radnet_deflate_lz_emit_u8 refuses. */
int64_t radnet_deflate_lz_piece_cap(const radnet_deflate_code* code_ll, const radnet_deflate_code* code_d, int32_t header_nbits);
/* Host only: the bits of all block headers, tokens and end-of-blocks that emit writes for these counts and codes over `chunks`
 * pieces -- each symbol's extra bits are fixed, so the counts decide it.  The flush and the zero bits up to a byte are not counted:
 * they depend on where each piece ends and are at most 7 bits a piece more for one rule than for another, which is why
 * png.deflate_device_lz takes the LZ stream only when bits_lz + 7 * chunks < bits_rle.  hist_d and code_d null (both): the
 * run-length rule, every match followed by dist_nbits bits.  Negative (RADNET_ERR_ARG): a null hist_ll or code_ll, one of hist_d and
 * code_d null alone, an illegal code, header_nbits or dist_nbits, chunks outside 1..65536. */
int64_t radnet_deflate_stream_bits(const uint32_t* hist_ll, const uint32_t* hist_d, const radnet_deflate_code* code_ll, const radnet_deflate_code* code_d,
                                   int32_t dist_nbits, int32_t header_nbits, int64_t chunks);
/* ---- inflate of run-length streams on the device (csrc/inflate.hip, csrc/inflate_plan.cpp): speculative block search ----------------
 * The reader's counterpart of the section above, for the streams this project meets: zlib level 1 with Z_RLE (cv2.imwrite's
 * defaults), png.assemble and the device deflate.  Every match of such a stream has distance 1, so a block's output depends on the
 * blocks in front of it through ONE byte, and a dynamic block header can be recognised at any bit offset.  z is the whole zlib
 * stream of n bytes (device; no alignment asked): 2 header bytes, the deflate blocks, the 4 bytes of the Adler-32; bit b of the
 * stream is bit b % 8 of byte b / 8 (RFC 1951 3.1.1) and first_bit is 16 for such a stream.  Nothing here waits on another
 * workgroup or spins; every loop is bounded by the stream's length and by RADNET_INFLATE_UNIT_MAX_SYMBOLS.
 * A UNIT is a run of consecutive deflate blocks: it begins at a given bit with a block of any type, continues while the next block
 * is stored or fixed (their headers cannot be recognised speculatively, so they ride with the block in front of them) and ends
 * before the next dynamic block or behind a block with BFINAL set.
 * THE READING RULE shared by the three kernels and tests/inflate_cases.py: bits beyond the stream read as zero; after every group of
 * bits taken the position is compared with 8 * n and a position beyond it ends the unit with RADNET_INFLATE_PAST_END before the
 * value is looked at; a code word that no symbol has is RADNET_INFLATE_BAD_CODE (PAST_END if fewer than 15 bits were left).
 * RADNET_INFLATE_UNIT_MAX_SYMBOLS is 8 times the largest block zlib emits (32,767 symbols at memLevel 9); it bounds the time a
 * false candidate, or a file made of fixed blocks, can hold a wave. */
#define RADNET_INFLATE_UNIT_MAX_SYMBOLS 262144
#define RADNET_INFLATE_OK 0
/* BTYPE 11, or a dynamic header radnet_inflate_find_blocks would not accept */
#define RADNET_INFLATE_BAD_HEADER 1
/* a code word without a symbol, literal/length symbol 286 / 287, distance symbol 30 / 31 */
#define RADNET_INFLATE_BAD_CODE 2
/* a distance symbol other than 0: not a run-length stream */
#define RADNET_INFLATE_NOT_RLE 3
/* LEN != ~NLEN in a stored block */
#define RADNET_INFLATE_STORED_MISMATCH 4
/* ran past the stream */
#define RADNET_INFLATE_PAST_END 5
/* more than RADNET_INFLATE_UNIT_MAX_SYMBOLS literal/length symbols (end-of-block included) */
#define RADNET_INFLATE_TOO_LONG 6
/* the unit ends behind a block with BFINAL set */
#define RADNET_INFLATE_FLAG_FINAL 1
/* its first output comes from a match: it needs the byte in front of it */
#define RADNET_INFLATE_FLAG_LEAD_MATCH 2
/* it holds a literal or a stored byte, so last_byte does not depend on the predecessor */
#define RADNET_INFLATE_FLAG_LAST_KNOWN 4
typedef struct radnet_inflate_unit {
  uint32_t start_bit;  /* given by the caller */
  uint32_t end_bit;    /* the bit behind the unit: the next dynamic header, or the bit behind the final block (not byte aligned) */
  uint32_t out_bytes, symbols, blocks;
  uint32_t status;     /* RADNET_INFLATE_*; when it is not OK every field but start_bit and status is zero */
  uint32_t flags;      /* RADNET_INFLATE_FLAG_* */
  uint32_t last_byte;  /* the unit's last output byte if LAST_KNOWN, else 0 */
} radnet_inflate_unit; /* 32 bytes */
typedef struct radnet_inflate_link {
  int64_t out_offset;  /* exclusive prefix sum of out_bytes along the chain */
  uint32_t start_bit, out_bytes;
  uint32_t prev_byte;  /* the output byte in front of the unit (0 for the first) */
  uint32_t reserved;
} radnet_inflate_link; /* 24 bytes */
/* Host only (csrc/inflate_plan.cpp; no context, no device): the CRC-32 of `count` PNG chunks of the file in HOST memory, on up to
 * `workers` threads (1..16; a run of consecutive chunks each), so that a map written as thousands of 8 KiB IDAT chunks does not pay a
 * Python call per chunk.  Chunk k's length field stands at file[at[k]], its CRC field at file[end[k]]: the sum covers
 * file[at[k] + 4 .. end[k]), the type and the payload, and is compared with the big-endian word at end[k].  Returns count when
 * every sum matches, else the index of the first chunk whose sum does not; RADNET_ERR_ARG for a null pointer, count < 1, or a chunk
 * that does not lie inside file_len (at[k] + 8 <= end[k], end[k] + 4 <= file_len). */
int radnet_png_check_crcs(const uint8_t* file, int64_t file_len, const int64_t* at, const int64_t* end, int32_t count, int32_t workers);
/* One thread per bit offset p in [first_bit, 8 * n): p is appended to cand exactly when a dynamic block header that zlib's inflate
 * accepts begins there (BFINAL at p, either value).  The rule, in order: BTYPE is 10; 257 + HLIT <= 286 and 1 + HDIST <= 30; the
 * code-length code is complete (Kraft sum exactly 1); no repeat symbol 16 comes first and no repeat runs past the declared count;
 * symbol 256 has a non-zero length; the literal/length code is complete or a single 1-bit code; the distance code is complete, a
 * single 1-bit code, or empty; every bit read lies inside the stream.  The append is unordered: idx = atomicAdd(count, 1) (integer;
 * the caller zeroes *count, device uint32) and cand[idx] = p if idx < cand_cap, so *count may exceed cand_cap and nothing is written
 * beyond the cap; the host sorts.  A null pointer, n < 3, first_bit < 0 or >= 8 * n, cand_cap < 0 is RADNET_ERR_ARG; n >= 2^29,
 * where bit offsets leave 32 bits, RADNET_ERR_UNSUPPORTED; nothing is launched then. */
int radnet_inflate_find_blocks(radnet_ctx* ctx, const uint8_t* z, int64_t n, int64_t first_bit, uint32_t* cand, int32_t cand_cap, uint32_t* count);
/* Decodes the unit that begins at units[u].start_bit (device table, count entries; start_bit below 8 * n is the caller's to ensure,
 * a larger one gives PAST_END) WITHOUT writing output, one wave per unit, and fills the other fields of the record.  The code tables
 * stand in LDS, the compressed bytes pass through an LDS window, one lane decodes.  A unit AT the symbol cap (262,144 fixed-code literals, one wave alone on the device) took 114 to 134 ms when
 * measured (tools/png_inflate_timing.py): that is what a false candidate or a file of fixed blocks can cost.
 * Arguments refused as above; count < 1 is RADNET_ERR_ARG. */
int radnet_inflate_rle_measure(radnet_ctx* ctx, const uint8_t* z, int64_t n, radnet_inflate_unit* units, int32_t count);
/* Host only (csrc/inflate_plan.cpp; no context, no device, like radnet_png_plan_segments).  units: the measured records sorted by
 * start_bit (strictly increasing).  Follows start -> end -> start from first_bit and writes the chained units in order to links
 * (link_cap >= count always suffices) with their exclusive output offsets and the byte in front of each, inherited through units
 * that produced no known byte.  *link_count = the links written; *false_count = count - *link_count, the candidates the chain
 * never visits, when the chain is accepted.  Returns RADNET_INFLATE_CHAIN_OK, RADNET_ERR_ARG (a null pointer, count < 1, n < 1,
 * first_bit < 0, expected < 0, link_cap < the links needed, unsorted starts) or one of the refusals below with *bad_unit = the
 * index in `units` of the offending unit (for NO_START: the unit whose end bit is no measured start, or -1 when first_bit itself is
 * none).  The refusals, checked per unit in this order while walking, LENGTH and TRAILER at the end:
 *   NO_START   a position of the walk that is no measured start;
 *   BAD_UNIT   a unit whose status is not RADNET_INFLATE_OK;
 *   LEAD_MATCH a unit that begins with a match while no output byte stands in front of it (the first unit, or one behind empty ones);
 *   LENGTH     the chain's total differs from `expected`;
 *   TRAILER    the final unit's end, rounded up to a byte, plus 4 (the Adler-32) is not n. */
#define RADNET_INFLATE_CHAIN_OK 0
#define RADNET_INFLATE_CHAIN_NO_START 1
#define RADNET_INFLATE_CHAIN_BAD_UNIT 2
#define RADNET_INFLATE_CHAIN_LEAD_MATCH 3
#define RADNET_INFLATE_CHAIN_LENGTH 4
#define RADNET_INFLATE_CHAIN_TRAILER 5
int radnet_inflate_chain(const radnet_inflate_unit* units, int32_t count, int64_t first_bit, int64_t n, int64_t expected, radnet_inflate_link* links,
                         int32_t link_cap, int32_t* link_count, int32_t* false_count, int32_t* bad_unit);
/* Decodes every chained unit again (links: device table, count entries) and writes its bytes to out[out_offset .. out_offset +
 * out_bytes) (device) and nowhere else: a literal its byte, a stored block its bytes, a match the byte in front of it, which for the
 * unit's first token is prev_byte.  A unit that would give more than its out_bytes, or pass out_len, is cut there; one that fails
 * to decode stops (the caller checks the Adler-32 of `out` against the stream's trailer).  One wave per unit: one lane decodes a
 * batch of tokens into LDS, the wave sums their lengths by prefix and all lanes expand them.  Arguments refused as above;
 * out_len < 0 is RADNET_ERR_ARG. */
int radnet_inflate_rle_emit(radnet_ctx* ctx, const uint8_t* z, int64_t n, const radnet_inflate_link* links, int32_t count, uint8_t* out,
                            int64_t out_len);
/* ---- inflate of ANY stream on the device (csrc/inflate_lz.hip, csrc/inflate_plan.cpp): far matches by pointer jumping ---------------
 * The section above with the distance taken whole.  radnet_inflate_find_blocks recognises a dynamic header whatever the distances
 * are, and a unit's length in bits and in bytes does not depend on the bytes in front of it, so units are measured and chained in
 * the same way.  What a match copies need not stand in its own unit: emit therefore writes, beside the literals, for EVERY output
 * byte the position it is a copy of (src[i] = i for a literal, an earlier position for a byte of a match).  The stream is then a
 * forest of pointers whose roots are the literals; resolve halves every path per round, gather reads each byte from its root.  No
 * 32 KiB window travels from unit to unit, no workgroup waits on another, no loop spins, and the final bytes and the final src do
 * not depend on the order in which anything ran.  The token decoder, the LDS window and THE READING RULE are those above (one
 * kernel body, csrc/inflate_units_body.h); distance symbols 0..29 take their extra bits (RFC 1951 3.2.5) with the PAST_END check
 * behind them as behind every group of bits. */
typedef struct radnet_inflate_lz_unit {
  uint32_t start_bit;   /* given by the caller */
  uint32_t end_bit;     /* as in radnet_inflate_unit */
  uint32_t out_bytes, symbols, blocks;
  uint32_t status;      /* RADNET_INFLATE_* (never NOT_RLE); when it is not OK every field but start_bit and status is zero */
  uint32_t flags;       /* RADNET_INFLATE_FLAG_FINAL only */
  uint32_t reach;       /* max over the unit's matches of distance - bytes the unit produced before that match, floored at 0: how
                           far the unit reads in front of itself, 0..32768 */
  uint32_t far_matches; /* the matches whose distance is not 1 */
  uint32_t reserved;    /* 0 */
} radnet_inflate_lz_unit; /* 40 bytes */
/* radnet_inflate_rle_measure for any stream: the same unit rule (stored and fixed blocks ride along), symbol cap, statuses and
 * refusals; RADNET_INFLATE_NOT_RLE is never returned. */
int radnet_inflate_lz_measure(radnet_ctx* ctx, const uint8_t* z, int64_t n, radnet_inflate_lz_unit* units, int32_t count);
/* a unit whose reach exceeds its out_offset: a match that points in front of the stream (zlib: "invalid distance too far back") */
#define RADNET_INFLATE_CHAIN_REACH 6
/* Host only (csrc/inflate_plan.cpp; no context, no device): radnet_inflate_chain's walk, arguments, results and refusals for
 * radnet_inflate_lz_unit records, without LEAD_MATCH and without the byte in front (every link's prev_byte is 0).  Per unit, in
 * order: NO_START, BAD_UNIT, REACH, then link_cap (RADNET_ERR_ARG); LENGTH and TRAILER at the end.  THE REACH CHECK IS THE GUARD
 * THAT KEEPS EVERY LATER INDEX NON-NEGATIVE: a unit chained at out_offset copies from out_offset - reach at the lowest, so with
 * reach <= out_offset every source radnet_inflate_lz_emit writes lies in [0, position). */
int radnet_inflate_lz_chain(const radnet_inflate_lz_unit* units, int32_t count, int64_t first_bit, int64_t n, int64_t expected,
                            radnet_inflate_link* links, int32_t link_cap, int32_t* link_count, int32_t* false_count, int32_t* bad_unit);
/* Decodes every chained unit again, one wave per unit, batches of tokens through LDS as radnet_inflate_rle_emit does.  buf:
 * uint8[out_len], src: uint32[out_len] (device).  A literal or a stored byte at absolute position i: buf[i] = the byte, src[i] = i.
 * A match of length L and distance D that begins at p: src[p + j] = p - D + (j % D) for j < L, and buf is NOT written there; the
 * % D lets an overlapping match (a run) point in front of itself directly, so the depth of a chain is the number of matches on
 * it, not of bytes.  A source that would be negative (no chain gives one, see REACH) is written as the position itself.  Nothing
 * outside the unit's [out_offset, out_offset + out_bytes) and [0, out_len) is written, in either array.  Arguments refused as
 * radnet_inflate_rle_emit refuses them (src null too); out_len >= 2^31 is RADNET_ERR_UNSUPPORTED; nothing is launched then. */
int radnet_inflate_lz_emit(radnet_ctx* ctx, const uint8_t* z, int64_t n, const radnet_inflate_link* links, int32_t count, uint8_t* buf, uint32_t* src,
                           int64_t out_len);
/* Enqueues `rounds` launches (1..RADNET_INFLATE_LZ_MAX_ROUNDS), one thread per position, IN PLACE:
 *   s = src[i]; if (s < i) { t = src[s]; if (t < s) { src[i] = t; count } }
 * changed: device uint32[rounds], zeroed by the caller; launch r adds the entries it rewrote to changed[r] (an integer atomic, once
 * per workgroup that rewrote any).  An entry with src[i] >= i is a root by definition, so the kernel reads nothing outside
 * src[0 .. out_len) and terminates on ANY content of src.  In place is correct: whatever another thread has stored in src[s]
 * meanwhile is an ancestor of s.  The roots are unique, so the flat src does not depend on timing; the counts may.  At most
 * ceil(log2(max(out_len, 2))) rounds flatten any table radnet_inflate_lz_emit writes: a path of k links has at most ceil(k / 2)
 * after a round, and no path is longer than out_len - 1.  A round that rewrote nothing leaves src flat.  A null pointer,
 * out_len < 0 or rounds outside 1..RADNET_INFLATE_LZ_MAX_ROUNDS is RADNET_ERR_ARG, out_len >= 2^31 RADNET_ERR_UNSUPPORTED;
 * nothing is launched then, nor for out_len = 0. */
#define RADNET_INFLATE_LZ_MAX_ROUNDS 32
int radnet_inflate_lz_resolve(radnet_ctx* ctx, uint32_t* src, int64_t out_len, int32_t rounds, uint32_t* changed);
/* s = src[i]; if (s < i) buf[i] = buf[s], one thread per position, IN PLACE: race-free once src is flat, because a root is never
 * written; memory-safe on any content of src.  Refusals as radnet_inflate_lz_resolve's. */
int radnet_inflate_lz_gather(radnet_ctx* ctx, const uint32_t* src, uint8_t* buf, int64_t out_len);
/* ---- inflate of MANY streams in one pass (csrc/inflate_many.hip, csrc/inflate_plan.cpp) -----------------------------------------
 * The two sections above for a batch of zlib streams that stand in ONE device buffer z[0 .. z_len) and inflate into ONE output
 * out[0 .. out_len): one search, one measure and one emit serve the batch, and radnet_inflate_lz_resolve / radnet_inflate_lz_gather
 * run as they are on the common src / buf.  The stream table says where each stream stands; it lives on the host (validated before
 * any launch) and on the device (the SAME table, uploaded by the caller, 8-byte aligned) like the segment and piece tables.
 * THE BOUNDARY RULE: a bit, a unit or a link belongs to the stream whose bytes [z_offset, z_offset + n) hold its (start) bit, and
 * to no stream when it stands in a gap.  THE READING RULE's 8 * n is that stream's end: bits behind it read as zero and end the
 * header or the unit with PAST_END, whatever stands in the gap or in the next stream.  Bit offsets are GLOBAL, 8 * z_offset + p for
 * bit p of the stream; output positions are absolute in `out`.  Per stream, every result is what the one-stream entry gives for
 * that stream alone, shifted by 8 * z_offset and out_offset.  The host chain stays per stream (radnet_inflate_chain /
 * radnet_inflate_lz_chain on the stream's slice of the sorted records with its bits shifted back; the links are shifted forward).
 * The kernels are the one-stream ones (csrc/inflate_units_body.h); a wave finds its stream by bisection over the table. */
typedef struct radnet_inflate_stream {
  int64_t z_offset;    /* byte of z at which this zlib stream's byte 0 stands */
  int64_t n;           /* its length in bytes, zlib header and Adler-32 included; 3 at least, as for one stream */
  int64_t out_offset;  /* where its inflated bytes begin in the common output */
  int64_t expected;    /* how many there are; 0 is legal */
} radnet_inflate_stream; /* 32 bytes */
#define RADNET_INFLATE_MANY_MAX_STREAMS 4096
/* Host only (csrc/inflate_plan.cpp; no context, no device): the validation every _many entry runs before it launches.  The table
 * must ascend in z_offset and in out_offset with disjoint ranges of both kinds (gaps are allowed: radnet_png_join_u8 writes 16-byte
 * grains, so a caller may align its streams) that lie inside z_len / out_len.  RADNET_ERR_ARG, with the reason in msg (msg_cap
 * bytes; may be null) and the first bad stream's index in *bad_stream (-1 when the arguments themselves are refused; may be null):
 * a null table, count < 1 or > RADNET_INFLATE_MANY_MAX_STREAMS, z_len < 0, out_len < 0; a stream with z_offset < 0, n < 3,
 * out_offset < 0 or expected < 0, or one that passes z_len or out_len (checked without overflow); a stream that begins in front
 * of its predecessor (unsorted) or inside it (overlapping), in z or in the output.  z_len >= 2^29 (a global bit offset could pass
 * 2^32) and out_len >= 2^31 (positions leave 31 bits) are RADNET_ERR_UNSUPPORTED, judged before the streams. */
int radnet_inflate_streams_check(const radnet_inflate_stream* streams, int32_t count, int64_t z_len, int64_t out_len, int32_t* bad_stream,
                                 char* msg, int32_t msg_cap);
/* radnet_inflate_find_blocks over the batch, one thread per bit of z[0 .. z_len): a bit that lies in stream k is appended exactly
 * when radnet_inflate_find_blocks(z + z_offset_k, n_k, first_bit = 16, ...) would append it, as the GLOBAL offset 8 * z_offset_k + p;
 * "every bit read lies inside the stream" means inside stream k.  Bits in a gap are never appended.  A workgroup takes 256 bits:
 * it bisects the device table once for the stream that holds or precedes its first byte, stages the few entries that can touch
 * its 32 bytes in LDS (streams are 3 bytes at least), and each thread bisects those.  The append, cand_cap and *count are as
 * there.  Refusals: radnet_inflate_streams_check's (out_len taken as the end of the last stream's output); a null pointer,
 * cand_cap < 0 or a table_dev that is not 8-byte aligned is RADNET_ERR_ARG; nothing is launched then. */
int radnet_inflate_find_blocks_many(radnet_ctx* ctx, const uint8_t* z, int64_t z_len, const radnet_inflate_stream* streams_host,
                                    const radnet_inflate_stream* streams_dev, int32_t n_streams, uint32_t* cand, int32_t cand_cap, uint32_t* count);
/* radnet_inflate_rle_measure / radnet_inflate_lz_measure over the batch: units[u].start_bit is GLOBAL; the unit's stream is the one
 * that holds that bit, a start in a gap or behind z_len gives PAST_END; end_bit is GLOBAL; every other field is the one-stream
 * entry's for the same unit of the same stream alone.  Refusals as above; count < 1 or a null table is RADNET_ERR_ARG. */
int radnet_inflate_rle_measure_many(radnet_ctx* ctx, const uint8_t* z, int64_t z_len, const radnet_inflate_stream* streams_host,
                                    const radnet_inflate_stream* streams_dev, int32_t n_streams, radnet_inflate_unit* units, int32_t count);
int radnet_inflate_lz_measure_many(radnet_ctx* ctx, const uint8_t* z, int64_t z_len, const radnet_inflate_stream* streams_host,
                                   const radnet_inflate_stream* streams_dev, int32_t n_streams, radnet_inflate_lz_unit* units, int32_t count);
/* radnet_inflate_rle_emit / radnet_inflate_lz_emit over the batch: links[u].start_bit is GLOBAL and links[u].out_offset ABSOLUTE in
 * out (buf) of out_len bytes.  Reading is bounded by the link's own stream (the one that holds its start bit; a link in a gap
 * writes nothing).  Writing is bounded by the link's [out_offset, out_offset + out_bytes) AND by its stream's [out_offset,
 * out_offset + expected): a link that begins outside its stream's output writes nothing.  LZ: src holds ABSOLUTE positions; a
 * source that would fall in front of the stream's own out_offset is written as the position itself (the per-stream chain's REACH
 * check makes that unreachable), so no byte of one stream is ever a copy of another's.  Refusals as above and as the one-stream
 * entries' (streams_check is run against out_len). */
int radnet_inflate_rle_emit_many(radnet_ctx* ctx, const uint8_t* z, int64_t z_len, const radnet_inflate_stream* streams_host,
                                 const radnet_inflate_stream* streams_dev, int32_t n_streams, const radnet_inflate_link* links, int32_t count,
                                 uint8_t* out, int64_t out_len);
int radnet_inflate_lz_emit_many(radnet_ctx* ctx, const uint8_t* z, int64_t z_len, const radnet_inflate_stream* streams_host,
                                const radnet_inflate_stream* streams_dev, int32_t n_streams, const radnet_inflate_link* links, int32_t count,
                                uint8_t* buf, uint32_t* src, int64_t out_len);
/* For a batch, radnet_crc32_segments is ONE launch group over the common z (its table takes any ranges of one buffer), and
 * radnet_png_join_u8 is one launch PER FILE: its pieces tile out[0 .. n) from dst 0 on, so a file joins into z + z_offset. */
/* The filter-type column of an inflated stream on the device: column[k] = stream[offset[p] + r * (1 + rowbytes[p])] for the rows r
 * of the passes p = 0 .. passes - 1 in order (k counts them through), one launch; offsets, rows and rowbytes are HOST arrays of
 * `passes` (1..7) entries that travel with the launch.  The pass must lie inside stream_len.  png.py downloads the column, refuses
 * a type above 4 and plans segments from it (radnet_png_plan_segments_column). */
int radnet_png_gather_column_u8(radnet_ctx* ctx, const uint8_t* stream, int64_t stream_len, const int64_t* offsets, const int32_t* rows,
                                const int32_t* rowbytes, int32_t passes, uint8_t* column);
/* radnet_png_plan_segments for a pass whose filter-type bytes stand one behind the other: column[r] is the type of row r (HOST).
 * Same rule, same result, same refusals. */
int radnet_png_plan_segments_column(const uint8_t* column, int64_t stream_offset, int32_t rows, int32_t rowbytes, int32_t target_rows,
                                    radnet_png_segment* out, int32_t cap);
/* ---- adaptive-filter rows on all CUs: tiles (csrc/png_tiles.hip, csrc/png_tile_rule.h) ----
 * Up, Average and Paeth rows allow no segment cut, but byte (r, x) needs only (r, x - bpp), (r - 1, x) and (r - 1, x - bpp).  A
 * segment of R rows and P = rowbytes / bpp pixels is cut into bands of RADNET_PNG_TILE_ROWS rows (one wave, one lane per row, each
 * row one pixel behind the row above, as in radnet_png_unfilter_u8) and column blocks of T = RADNET_PNG_TILE_PIXELS pixels.  Tiles
 * are SKEWED: tile (band b, block c) holds, of the band's row l (lane l), the pixels [c * T - l, (c + 1) * T - l) clipped to
 * [0, P), so the wave is full through the whole tile.  The tile reads, beside its own bytes, the pixels c * T - l - 1 of its rows
 * l and l - 1 (tile (b, c - 1)) and of the last row of band b - 1 the pixels [c * T - 1, (c + 1) * T) (tiles (b - 1, c) and
 * (b - 1, c + 1), because T >= 64).  So tile (b, c) runs on sweep d = c + 2 * b, tiles of one sweep are independent, and
 *   bands = ceil(R / 64),  blocks = ceil((P + 63) / T),  sweeps = blocks + 2 * (bands - 1).
 * On sweep d the bands lo .. hi have a tile, lo = max(0, ceil((d - blocks + 1) / 2)), hi = min(bands - 1, floor(d / 2)); the
 * tile of blockIdx.x = i is (lo + i, d - 2 * (lo + i)); every sweep has a tile, except the odd sweeps of a segment of one block.  The rule stands once, in csrc/png_tile_rule.h, for the planner below and
 * for the kernel and its launch code.  T = 64, the narrowest block the rule allows, by measurement: of the sweeps, 2 * (bands - 1) do
 * not depend on T and each lasts as long as one tile, so on the 4000 x 4000 RGB panel the stage takes 6.6 ms at 64, 10.3 at 128 and
 * 17.9 at 256 (profiles/png_unfilter_tiles_timing.txt). */
#define RADNET_PNG_TILE_ROWS 64
#define RADNET_PNG_TILE_PIXELS 64
typedef struct radnet_png_tile_plan {
  int32_t bands, blocks, sweeps; /* as above */
  int32_t tile_rows, tile_pixels; /* RADNET_PNG_TILE_ROWS, RADNET_PNG_TILE_PIXELS */
} radnet_png_tile_plan;
/* Host only (csrc/png_plan.cpp; no context, no device): the plan of one segment of `rows` scanlines of `rowbytes` bytes.  RADNET_OK,
 * or RADNET_ERR_ARG (nothing written) for a null `out`, rows or rowbytes < 1, rowbytes above 2^30, a bpp that is not one of 1, 2, 3,
 * 4, 6, 8 or does not divide rowbytes. */
int radnet_png_plan_tiles(int32_t rows, int32_t rowbytes, int32_t bpp, radnet_png_tile_plan* out);
/* Host only: the tiles of sweep `sweep` (0 .. sweeps - 1) in blockIdx.x order.  Returns their number n and writes the first
 * min(n, cap) of them as (band, block) pairs, 2 * min(n, cap) int32, to band_block_pairs, which may be null when cap is 0 (the
 * count alone: what the launch code asks).  RADNET_ERR_ARG (nothing written) for the arguments radnet_png_plan_tiles refuses, a
 * sweep outside the plan, a negative cap, or a null band_block_pairs with cap > 0. */
int radnet_png_tiles_on_sweep(int32_t rows, int32_t rowbytes, int32_t bpp, int32_t sweep, int32_t* band_block_pairs, int32_t cap);
/* radnet_png_unfilter_segments_u8 by tiles, for segments of any length: the same table contract, word for word -- the same table on
 * the host and on the device, uploaded by the caller (this entry copies nothing); the host table validated before anything is
 * launched (rows > 0, rowbytes > 0, rowbytes % bpp == 0, offset >= 0, offset + rows * (1 + rowbytes) <= base_len; a violation is
 * RADNET_ERR_ARG naming the segment's index and nothing is modified); segments must not overlap (not checked); count == 0 is
 * RADNET_OK without a launch, whatever the pointers; the table may be in any order; a whole pass is a table of one entry.  The bytes
 * are those radnet_png_unfilter_u8 defines for each segment on its own: the row above the first row counts as zeros, the
 * filter-type bytes stay, a type above 4 is treated as None.
 * One plain kernel launch per sweep on the context's stream, max over the segments of `sweeps` launches in all (a sweep on which no
 * segment has a tile is passed over), stream order being
 * the only dependency: nothing waits on another workgroup, no flag or counter in memory, every loop bound a function of the
 * arguments.  The grid of sweep d is (the most tiles any segment has on d, count) -- count in slices of 65535, the limit of
 * gridDim.y --, one wave per workgroup and per tile; a workgroup whose segment has no such tile returns.  A tile goes through LDS
 * in chunks of 32 pixels (16 for bpp 6 and 8), the next chunk's loads in flight while the wave works on this one, and every byte
 * goes out with a byte store to a byte the tile owns: tiles of one sweep own neighbouring bytes of one dword. */
int radnet_png_unfilter_tiles_u8(radnet_ctx* ctx, uint8_t* base, int64_t base_len, const radnet_png_segment* segs_host,
                                 const radnet_png_segment* segs_dev, int32_t count, int32_t bpp);
/* The same with the block width given, for the measurement of T (tools/png_unfilter_timing.py): tile_pixels a multiple of 32 from
 * 64 to 4096, else RADNET_ERR_ARG.  The plan of such a call is the rule above with that T; the planner entries describe
 * radnet_png_unfilter_tiles_u8 only. */
int radnet_png_unfilter_tiles_width_u8(radnet_ctx* ctx, uint8_t* base, int64_t base_len, const radnet_png_segment* segs_host,
                                       const radnet_png_segment* segs_dev, int32_t count, int32_t bpp, int32_t tile_pixels);
/* ---- CRC-32 of PNG chunks on the device (csrc/crc32.hip, csrc/crc32_plan.cpp, csrc/crc32_rule.h) ------------------------------------
 * The CRC-32 of zlib and PNG: polynomial 0xEDB88320, reflected (bit 31 of a register is the coefficient of x^0), init and final
 * xor 0xFFFFFFFF.  With pure(B) the register after the bytes B from init 0 without the final xor, and products taken mod P:
 *   pure(A || B) = pure(A) * x^(8 |B|) ^ pure(B);   pure(0^k || B) = pure(B);
 *   zlib.crc32(B, c0) = pure(B) ^ (c0 ^ 0xFFFFFFFF) * x^(8 |B|) ^ 0xFFFFFFFF.
 * So a range of bytes is summed in pieces of any size, on any number of workgroups in any order, and the result is exact. */
typedef struct radnet_crc32_segment {
  int64_t offset;  /* of the segment's first byte in the buffer */
  int64_t length;  /* in bytes; 0 is legal */
  uint32_t init;   /* the running value in front of the segment: 0 for a sum of its own, zlib.crc32(b"IDAT") for a chunk's payload */
  uint32_t expect; /* what the sum is compared with */
} radnet_crc32_segment; /* 24 bytes */
/* THE GRAIN RULE: a lane sums RADNET_CRC32_GRAIN bytes, a workgroup a span of RADNET_CRC32_SPAN_GRAINS grains (4096 bytes).  The
 * last bytes of a segment behind the last 16-byte boundary of device memory inside it (0..15, the tail) are summed one by one; the
 * body in front of them is cut into grains counted BACKWARDS from that boundary, so that every grain is one aligned 16-byte load
 * but the segment's first, which is read byte by byte and padded in front with zeros (free, by the second identity); spans are
 * counted backwards from the same boundary.  A unit that stands i units in front of the end weighs x^(8 * unit * i): constants,
 * generated at compile time (csrc/crc32_rule.h). */
#define RADNET_CRC32_GRAIN 16
#define RADNET_CRC32_SPAN_GRAINS 256
#define RADNET_CRC32_MAX_SPANS 2147483646
typedef struct radnet_crc32_plan {
  int64_t spans;    /* of all segments together: the workgroups of the span launch */
  int64_t ws_bytes; /* of scratch the call takes from the context: 4 * (count + 1 + spans) */
} radnet_crc32_plan;
/* Host only (csrc/crc32_plan.cpp; no context, no device).  x^(8 len) mod P as a register; len <= 0 gives x^0 = 0x80000000. */
uint32_t radnet_crc32_shift(int64_t len);
/* Host only.  zlib's crc32_combine: zlib.crc32(a + b) from crc1 = zlib.crc32(a), crc2 = zlib.crc32(b), len2 = len(b); crc1 for
 * len2 <= 0. */
uint32_t radnet_crc32_combine(uint32_t crc1, uint32_t crc2, int64_t len2);
/* Host only: the validation and the grain plan radnet_crc32_segments runs before it launches.  table: `count` segments in HOST
 * memory for a buffer of n bytes whose first byte stands `misalign` (0..15) bytes behind a 16-byte boundary.  RADNET_ERR_ARG, with
 * the reason in msg (msg_cap bytes; may be null) and the first bad segment's index in *bad_entry (-1 when the arguments
 * themselves are refused; may be null): a null plan, count < 0, n < 0, misalign outside 0..15, a null table with count > 0, a
 * segment with offset < 0, length < 0 or offset + length > n (checked without overflow).  More than RADNET_CRC32_MAX_SPANS spans
 * is RADNET_ERR_UNSUPPORTED.  *plan is written on RADNET_OK only. */
int radnet_crc32_plan_segments(const radnet_crc32_segment* table, int32_t count, int64_t n, int32_t misalign, radnet_crc32_plan* plan,
                               int32_t* bad_entry, char* msg, int32_t msg_cap);
/* crc[k] = zlib.crc32(buf[offset_k : offset_k + length_k], init_k) for the `count` segments of the device buffer buf[0 .. n);
 * result[0] = the smallest k with crc[k] != expect_k, or count when there is none; result[1] = how many such k there are.  The
 * entry initialises result itself (on the stream; nothing is copied or waited for).  count == 0 is legal, gives {0, 0} and may
 * come with null tables and a null crc; n == 0 may come with a null buf.  Segments may overlap, may be empty and may come in any
 * order; buf may stand at any byte address.  table_host and table_dev hold the SAME table on the host and on the device (the
 * caller uploads it, as for radnet_png_unfilter_segments_u8); table_dev is 8-byte aligned, crc (count words) and result (2 words)
 * 4-byte aligned device memory.
 * The host table is validated before anything is launched (radnet_crc32_plan_segments: RADNET_ERR_ARG or RADNET_ERR_UNSUPPORTED
 * with its message; a null ctx, a null result or another null pointer that the counts do not excuse, or a misaligned table_dev,
 * crc or result is RADNET_ERR_ARG too) and nothing is written then.
 * Always three launches, whatever count and the data: (1) one workgroup sets result and sums the segments' span counts into their
 * exclusive prefix, (2) one workgroup per span of the plan -- it finds its segment in the prefix by bisection, a lane sums one
 * grain bitwise and weighs it, the xor over the lanes is the span's sum --, (3) one workgroup per segment joins its spans (beyond
 * 256 of them by Horner's rule per lane), adds the tail, folds init in with x^(8 length), writes crc[k] and compares.  The unit
 * of work is the span, so one segment of tens of MB and thousands of 8 KiB segments both fill the device.  No workgroup waits on
 * another, every loop is bounded by a length or a count, and the only atomics are an integer min and an integer add on result.
 * The prefix and the span sums stand in scratch that belongs to the context (plan.ws_bytes; it only grows, and a call that has to
 * grow it waits for the context's stream first). */
int radnet_crc32_segments(radnet_ctx* ctx, const uint8_t* buf, int64_t n, const radnet_crc32_segment* table_host,
                          const radnet_crc32_segment* table_dev, int32_t count, uint32_t* crc, int32_t* result);
/* ---- A PNG's IDAT payloads joined on the device (csrc/png_join.hip, csrc/png_join_plan.cpp) ------------------------------------------
 * The file's bytes go up as they are; one launch gathers the payloads of its IDAT chunks into the zlib stream the inflate entries
 * take.  Piece k of the table says  out[dst_k + j] = file[src_k + j]  for 0 <= j < length_k.  dst is the exclusive prefix sum of
 * the lengths in table order -- the pieces tile out[0 .. n) without a gap, in order; a length of 0 is legal, anywhere and any number
 * of times in a row; the src ranges may come in any order and may overlap. */
typedef struct radnet_png_piece {
  int64_t src;    /* of the piece's first byte in the file */
  int64_t dst;    /* of the piece's first byte in the joined stream: the sum of the lengths in front of it */
  int64_t length; /* in bytes; 0 is legal */
} radnet_png_piece; /* 24 bytes */
/* THE GRAIN RULE: a lane writes one grain, the RADNET_PNG_JOIN_GRAIN bytes between two 16-byte boundaries of DEVICE MEMORY, clipped
 * to [out, out + n); a workgroup takes a span of RADNET_PNG_JOIN_SPAN_GRAINS grains (4096 bytes).  With out standing `misalign`
 * bytes behind a boundary there are ceil((misalign + n) / 16) grains; only the first and the last can be clipped. */
#define RADNET_PNG_JOIN_GRAIN 16
#define RADNET_PNG_JOIN_SPAN_GRAINS 256
#define RADNET_PNG_JOIN_MAX_SPANS 2147483647
typedef struct radnet_png_join_plan {
  int64_t grains; /* ceil((misalign + n) / RADNET_PNG_JOIN_GRAIN); 0 for n == 0 */
  int64_t spans;  /* ceil(grains / RADNET_PNG_JOIN_SPAN_GRAINS): the workgroups of the launch */
} radnet_png_join_plan;
/* Host only (csrc/png_join_plan.cpp; no context, no device): the validation and the span count radnet_png_join_u8 runs before it
 * launches.  table: `count` pieces in HOST memory of a file of file_len bytes, for an output of n bytes whose first byte stands
 * `misalign` (0..15) bytes behind a 16-byte boundary.  RADNET_ERR_ARG, with the reason in msg (msg_cap bytes; may be null) and the
 * first bad entry's index in *bad_entry (-1 when the arguments themselves are refused, and for a total that is not n; may be null):
 * a null plan, count < 0, file_len < 0, n < 0, misalign outside 0..15, a null table with count > 0; a piece with src < 0, length < 0
 * or src + length > file_len (checked without overflow); a piece whose dst is not the sum of the lengths in front of it, or whose
 * end passes n; a total length other than n.  More than RADNET_PNG_JOIN_MAX_SPANS spans is RADNET_ERR_UNSUPPORTED.  *plan is
 * written on RADNET_OK only. */
int radnet_png_plan_join(const radnet_png_piece* table, int32_t count, int64_t file_len, int64_t n, int32_t misalign,
                         radnet_png_join_plan* plan, int32_t* bad_entry, char* msg, int32_t msg_cap);
/* out[0 .. n) = the pieces of file[0 .. file_len) joined, as above.  file and out are device buffers at any byte address;
 * table_host and table_dev hold the SAME table on the host and on the device (the caller uploads it, as for
 * radnet_crc32_segments); table_dev is 8-byte aligned.
 * The host table is validated before anything is launched (radnet_png_plan_join, with its message); a null ctx, a null pointer that
 * the counts do not excuse (file, out and table_dev with n > 0, table_host with count > 0), a misaligned table_dev, and
 * [out, out + n) overlapping [file, file + file_len) are RADNET_ERR_ARG too.  Nothing is written on a refusal.  n == 0 (with any
 * count of empty pieces) is RADNET_OK without a launch.
 * Otherwise ONE launch of plan.spans workgroups.  A lane finds the piece of its grain's first byte p by bisection over dst -- the
 * last k with dst_k <= p, which steps over empty pieces -- takes that piece's bytes up to the grain's end, and bisects again, from
 * the next entry on, whenever the grain goes on into the next non-empty piece: at most 16 bisections of log2(count) steps and 16
 * bytes per lane, so a run of thousands of empty pieces costs one more bisection and never a walk.  Every byte of out[0 .. n) is
 * written by exactly one lane, and no byte outside is written: a full grain is one aligned 16-byte store, a clipped one (the
 * first, the last) byte stores.  The file is read byte by byte, and no load touches a byte outside file[0 .. file_len).  No scratch
 * memory, no atomics, no flags; no workgroup waits on another. */
int radnet_png_join_u8(radnet_ctx* ctx, const uint8_t* file, int64_t file_len, const radnet_png_piece* table_host,
                       const radnet_png_piece* table_dev, int32_t count, uint8_t* out, int64_t n);
/* Rectangles painted into a uint8 [h][w][3] device image (rows pitch_bytes apart) IN PLACE.  The contract is this package's own:
 *   the corners (x1, y1), (x2, y2) come in either order, as cv2.rectangle takes them, and are normalised to x1 <= x2, y1 <= y2;
 *   thickness < 0 (cv2.FILLED): pixel (x, y) is painted iff x1 <= x <= x2 and y1 <= y <= y2;
 *   thickness t > 0, hw = t / 2 (integer division): painted iff (x, y) lies in [x1 - hw, x2 + hw] x [y1 - hw, y2 + hw] and NOT
 *     strictly inside (x1 + hw, x2 - hw) x (y1 + hw, y2 - hw); t = 1 is the one-pixel outline;
 *   everything is clipped to the image, a rectangle wholly outside paints nothing; a painted pixel becomes (b, g, r).
 * Against OpenCV: FILLED and t = 1 are cv2.rectangle's pixel sets; for t > 1 OpenCV joins four thick edges with round caps, so its
 * outer corners are rounded where these are square.  Parity with cv2 itself is unpinned (absent here, as for the decoder).
 * The result equals painting the rectangles one after the other in list order -- where they overlap the later one wins -- and is
 * deterministic; a pixel no rectangle covers is not written (nor is the pitch padding).  rects_host and rects_dev hold the SAME
 * table on the host and on the device (the caller uploads it; this entry copies nothing), as for radnet_png_unfilter_segments_u8.
 * The host copy is validated before the launch: thickness != 0, b, g, r in 0..255, and pitch_bytes >= 3 * w; a violation is
 * RADNET_ERR_ARG naming the entry's index and nothing is modified.  count == 0 is RADNET_OK without a launch, whatever the pointers.
 * One launch: a workgroup per tile of 32 x 8 pixels, the table streamed through LDS in batches of RADNET_DRAW_RECT_BATCH entries,
 * each batch culled against the tile; no atomics, no floating point. */
typedef struct radnet_rect {
  int32_t x1, y1, x2, y2, thickness, b, g, r;
} radnet_rect; /* 32 bytes */
#define RADNET_DRAW_RECT_BATCH 256
int radnet_draw_rects_u8(radnet_ctx* ctx, uint8_t* img, int32_t h, int32_t w, int64_t pitch_bytes, const radnet_rect* rects_host,
                         const radnet_rect* rects_dev, int32_t count);
/* An ORDERED list of rectangles and text runs painted into the same kind of image in place, in one launch: what one labelled
 * detection needs (outline, label box, label) without a launch per step and with the later entry on top.
 *   kind RADNET_PRIM_RECT: (x1, y1), (x2, y2) the corners, a the thickness, b unused, bgr = b | g << 8 | r << 16.  The pixel set is
 *     exactly radnet_draw_rects_u8's, FILLED (a < 0) included.
 *   kind RADNET_PRIM_TEXT: (x1, y1) the left end of the baseline (cv2.putText's org), x2 = s the integer scale in
 *     1..RADNET_DRAW_TEXT_MAX_SCALE, y2 = 0, a the offset and b the length n of the run in the character pool `chars`, bgr the
 *     colour.  The font is this package's own (csrc/draw_font.h; radnet_draw_glyph_rows): glyphs of 5 columns x 8 rows of dots,
 *     advance 6.  Dot (c, r) of character k covers the pixels x1 + (6k + c) * s .. + s - 1 by y1 - 7s + r * s .. + s - 1: the cap
 *     rows 0..6 lie in [y1 - 7s, y1 - 1], the descender row 7 in [y1, y1 + s - 1].  Only set dots are painted (a glyph's
 *     background and the gap column are transparent); n = 0 paints nothing.  Neither glyphs nor metrics are OpenCV's Hershey
 *     fonts; parity with cv2.putText is unpinned, as for the outlines.
 * Everything is clipped to the image; arithmetic that can leave int32 is done in 64 bits.  The result equals painting the list
 * entry by entry in order -- the later entry wins -- and is deterministic; a pixel no entry covers is not written (nor is the
 * pitch padding).  prims_host / prims_dev and chars_host / chars_dev hold the SAME table and the SAME pool on the host and on the
 * device (the caller uploads them; this entry copies nothing).  The host copies are validated before the launch; a violation is
 * RADNET_ERR_ARG naming the entry's index and nothing is modified: an unknown kind, a rectangle of thickness 0, a scale outside
 * 1..RADNET_DRAW_TEXT_MAX_SCALE, y2 != 0 on a text entry, a negative offset or length, a + b > n_chars, a byte of a referenced
 * run outside 0x20..0x7E, bgr with bits above 24; likewise pitch_bytes < 3 * w.  The pool pointers may be null when n_chars is 0.
 * count == 0 is RADNET_OK without a launch, whatever the pointers.
 * One launch with the scheme of radnet_draw_rects_u8 (tiles of 32 x 8 pixels, batches of RADNET_DRAW_RECT_BATCH entries culled
 * against the tile); a run is one entry whatever its length; no atomics, no floating point. */
typedef struct radnet_prim {
  int32_t kind, x1, y1, x2, y2, a, b, bgr;
} radnet_prim; /* 32 bytes */
#define RADNET_PRIM_RECT 0
#define RADNET_PRIM_TEXT 1
#define RADNET_DRAW_TEXT_MAX_SCALE 64
int radnet_draw_list_u8(radnet_ctx* ctx, uint8_t* img, int32_t h, int32_t w, int64_t pitch_bytes, const radnet_prim* prims_host,
                        const radnet_prim* prims_dev, int32_t count, const uint8_t* chars_host, const uint8_t* chars_dev, int32_t n_chars);
/* Host only (no context, no device, like radnet_png_plan_segments): the 8 row bytes of the glyph of `code`, top row first; the dot
 * of column c is (row >> (4 - c)) & 1.  RADNET_ERR_ARG for a code outside 0x20..0x7E or a null pointer (nothing is written). */
int radnet_draw_glyph_rows(int32_t code, uint8_t rows[8]);
/* A SCENE: radnet_draw_list_u8's ordered list with two more kinds and with transparency, painted in one launch by an instantiation
 * of its own of the painters' kernel body (csrc/draw.hip); what the precision/recall figure and the label views need (faster_rcnn/figures.py).  The arguments
 * and the host / device twin tables are radnet_draw_list_u8's.
 *   kinds RADNET_PRIM_RECT and RADNET_PRIM_TEXT: exactly radnet_draw_list_u8's pixel sets and checks.
 *   kind RADNET_PRIM_LINE: the segment from (x1, y1) to (x2, y2); a = t >= 1 the thickness; b the dash: 0 solid, else
 *     on = b & 0xFFFF and off = (b >> 16) & 0xFFFF, both >= 1.  The line is x-major when |x2 - x1| >= |y2 - y1|, else y-major, and
 *     the endpoints are ordered by the major coordinate first (a -> b, xa <= xb), so the pixel set does not depend on the order
 *     they come in.  x-major, for every x in [xa, xb]:  yc = ya + floor((2 (x - xa)(yb - ya) + (xb - xa)) / (2 (xb - xa)))  -- floor
 *     division, an exact half rounds up; a point (xa = xb) has yc = ya -- and the rows yc - (t - 1) / 2 .. yc + t / 2 are in the
 *     set (integer division: t pixels across the major direction, no caps beyond the endpoints).  y-major mirrors this.  With a
 *     dash a pixel of the set is painted iff floormod(its major coordinate, on + off) < on: the phase is the IMAGE's, so the
 *     pieces of a polyline join without a seam.
 *   kind RADNET_PRIM_DISC: centre (x1, y1), x2 = r >= 0 the radius, y2 = 0, b = 0.  With D(rho) = {dx^2 + dy^2 <= rho^2 + rho}:
 *     a < 0 is the filled disc D(r) (r = 0: one pixel); a = t > 0, hw = t / 2, is the ring D(r + hw) minus D(r - hw - 1) when
 *     r - hw >= 1 and all of D(r + hw) otherwise.
 *   Line endpoints, disc centres and radii lie within +-RADNET_DRAW_SCENE_MAX_COORD, which keeps every product exact in 64 bits.
 * TRANSPARENCY: bits 24..31 of bgr are tau; tau = 0 is opaque, so a table radnet_draw_list_u8 accepts means the same here.  A
 * covered pixel becomes per channel (c * (255 - tau) + d * tau + 127) / 255 in integer division, c the entry's colour and d the
 * pixel's value after the earlier entries: the entries compose in list order.  One thread owns a pixel, loads it at most once
 * (when the first translucent entry hits it and no opaque one did before), and stores it once, only if an entry covered it.
 * Against OpenCV, all unpinned as for the rectangles: cv2.line's thick lines have round caps and its thin ones another rounding;
 * cv2.circle draws midpoint circles; cv2.addWeighted rounds a float where this rounds an integer quotient.
 * The host copies are validated by radnet_draw_scene_check before the launch; a violation is RADNET_ERR_ARG naming the entry's
 * index and nothing is modified: an unknown kind; a line with t < 1, with a dash whose on or off is 0 while b != 0, or with an
 * endpoint beyond the bound; a disc with a = 0, r < 0, y2 != 0, b != 0 or a centre or radius beyond the bound; what
 * radnet_draw_list_u8 refuses for rectangles and text, except that bits 24..31 of bgr are allowed; likewise a null pointer, an empty
 * image and pitch_bytes < 3 * w.  count == 0 is RADNET_OK without a launch, whatever the pointers.
 * One launch with the tile, batch and cull scheme of radnet_draw_rects_u8; a line is culled by the box of its major extent by its
 * minor extent widened by the thickness, a disc by the box of its outer radius; every coverage test is O(1) per pixel and entry.
 * No atomics, no floating point. */
#define RADNET_PRIM_LINE 2
#define RADNET_PRIM_DISC 3
/* 1 << 24 */
#define RADNET_DRAW_SCENE_MAX_COORD 16777216
int radnet_draw_scene_u8(radnet_ctx* ctx, uint8_t* img, int32_t h, int32_t w, int64_t pitch_bytes, const radnet_prim* prims_host,
                         const radnet_prim* prims_dev, int32_t count, const uint8_t* chars_host, const uint8_t* chars_dev, int32_t n_chars);
/* Host only (csrc/draw_scene_check.cpp; no context, no device, like radnet_png_plan_segments): the checks of a scene's table and
 * character pool stated above.  RADNET_OK, or RADNET_ERR_ARG with the index of the first bad entry in *bad_entry (-1 when the
 * arguments themselves are at fault: count < 0, a null table with count > 0, n_chars < 0, a null pool with n_chars > 0) and a
 * sentence naming it in msg (at most msg_cap bytes with the terminator).  bad_entry and msg may be null.  count == 0 is RADNET_OK
 * whatever the pointers.  Reads exactly count entries and, of the pool, only the runs the text entries refer to. */
int radnet_draw_scene_check(const radnet_prim* prims, int32_t count, const uint8_t* chars, int32_t n_chars, int32_t* bad_entry, char* msg,
                            int32_t msg_cap);
/* cv2.cvtColor(BGR2GRAY) followed by GRAY2BGR as one pointwise launch: Y = (1868 B + 9617 G + 4899 R + 8192) >> 14 (OpenCV's
 * published 14-bit coefficients) written to all three channels of dst.  src and dst are uint8 [h][w][3] device images with rows
 * src_pitch and dst_pitch bytes apart (each >= 3 * w; the padding is neither read nor written); src == dst (with equal pitches) is
 * allowed, any other overlap is not.  A null pointer, h or w below 1 or a short pitch is RADNET_ERR_ARG and nothing is launched. */
int radnet_grey3_u8(radnet_ctx* ctx, const uint8_t* src, uint8_t* dst, int32_t h, int32_t w, int64_t src_pitch, int64_t dst_pitch);
/* SCORE MAPS AS PICTURES (csrc/heat.hip): the RPN's objectness over a scan, the imshow + colorbar views of train.py:338-347 and
 * RADNet.py:362-367 (faster_rcnn/figures.py: objectness_view, score_map_figure).
 *
 * radnet_score_levels_u8: fp32 scores to uint8 levels, one level per row of a score matrix (one per feature-map cell of
 * radnet_rpn_forward's `pred`, ld = 64, the anchors' scores in columns [0, A)).  For every row m < M: s = the maximum of
 * pred[m * ld + first .. first + count), NaNs skipped as fmaxf skips them; level = clamp(floor(s * 255.0f + 0.5f), 0, 255), the
 * product and the sum each rounded to fp32 (no FMA); a row of NaNs only gives 0, +inf gives 255, -inf gives 0.  levels[m] is
 * written for every m < M; nothing else is read or written (not the other columns of a row either).  RADNET_ERR_ARG, naming what
 * is wrong, for a null pointer, M < 1, first < 0, count < 1 or ld < first + count; nothing is launched then. */
int radnet_score_levels_u8(radnet_ctx* ctx, const float* pred, int32_t ld, int32_t M, int32_t first, int32_t count, uint8_t* levels);
/* radnet_heat_paint_u8: uint8 maps from a byte pool painted through a colour table into a uint8 [h][w][3] device image (rows
 * pitch_bytes apart) IN PLACE, in one launch.  A placement holds a destination rectangle [x0, x0 + w) x [y0, y0 + h) in image
 * pixels, which may leave the image on any side, and a map of mh rows of mw bytes at pool + offset.  For the pixel (X, Y) of the
 * image: every placement whose rectangle holds it gives the map byte at row ((Y - y0) * mh) / h, column ((X - x0) * mw) / w (floor
 * division, the operands are never negative): nearest cells, no interpolation.  The pixel's level is the MAXIMUM over those
 * placements, which does not depend on their order: overlapping tiles need no ordering and no atomics.  A pixel no placement holds,
 * or whose level is below min_level, is not written (nor is the pitch padding).  Otherwise with c = lut_bgr[3 * level ..] (b, g, r)
 * every channel becomes (c * (255 - tau) + d * tau + 127) / 255, d the pixel's value: radnet_draw_scene_u8's mix; tau = 0 stores c
 * without loading the pixel.  A pixel is loaded at most once and stored at most once.
 * img, pool (pool_len bytes), places_dev and lut_bgr (256 * 3 bytes) are device pointers; places_host holds the SAME table on the
 * host (the caller uploads it; this entry copies nothing) and is validated by radnet_heat_check before the launch.  A violation
 * there, a null pointer, an empty image, pool_len < 0, tau or min_level outside 0..255 or pitch_bytes < 3 * w is RADNET_ERR_ARG
 * naming what is wrong, and nothing is modified.  count == 0 is RADNET_OK without a launch, whatever the pointers.
 * One launch with the tile, batch and cull scheme of radnet_draw_rects_u8 (a workgroup per 32 x 8 pixels, the table through LDS in
 * batches of RADNET_DRAW_RECT_BATCH entries culled against the tile); the colour table sits in LDS; integers only. */
typedef struct radnet_heat_place {
  int32_t x0, y0, w, h; /* the destination rectangle */
  int32_t mw, mh;       /* the map's columns and rows */
  int64_t offset;       /* of the map's first byte in the pool */
} radnet_heat_place;    /* 32 bytes */
/* 1 << 20 */
#define RADNET_HEAT_MAX_EXTENT 1048576
#define RADNET_HEAT_MAX_MAP 2047
int radnet_heat_paint_u8(radnet_ctx* ctx, uint8_t* img, int32_t h, int32_t w, int64_t pitch_bytes, const uint8_t* pool, int64_t pool_len,
                         const radnet_heat_place* places_host, const radnet_heat_place* places_dev, int32_t count, const uint8_t* lut_bgr,
                         int32_t tau, int32_t min_level);
/* Host only (csrc/heat_check.cpp; no context, no device, like radnet_draw_scene_check): the checks of a placement table for an
 * image of h x w pixels and a pool of pool_len bytes.  Per entry 1 <= w, h <= RADNET_HEAT_MAX_EXTENT and 1 <= mw, mh <=
 * RADNET_HEAT_MAX_MAP (every product of the cell formula then fits 31 bits), |x0|, |y0| <= RADNET_DRAW_SCENE_MAX_COORD, offset >= 0
 * and offset + mw * mh <= pool_len.  RADNET_OK, or RADNET_ERR_ARG with the index of the first bad entry in *bad_entry (-1 when the
 * arguments themselves are at fault: count < 0, a null table with count > 0, pool_len < 0, h or w below 1) and a sentence naming
 * the entry and the field in msg (at most msg_cap bytes with the terminator).  bad_entry and msg may be null.  count == 0 with
 * sound arguments is RADNET_OK whatever the table pointer.  Reads exactly count entries. */
int radnet_heat_check(const radnet_heat_place* places, int32_t count, int64_t pool_len, int32_t h, int32_t w, int32_t* bad_entry, char* msg,
                      int32_t msg_cap);
int radnet_fill_zero(radnet_ctx* ctx, void* p, uint64_t bytes);
/* y = x * alpha (n floats); used to average gradients after all-reduce.  n = 0 launches nothing; RADNET_ERR_ARG for n < 0. */
int radnet_scale(radnet_ctx* ctx, float* x, int64_t n, float alpha);
/* out[i] = a[i]*b[i] + c[i]: refreshes the folded epilogue shift (BN scale * conv bias + BN shift,
 * FixedBatchNormalization.py:59-85) of the trainable head convs after an optimizer step.  out may be a, b or c.  n = 0 launches
 * nothing; RADNET_ERR_ARG for n < 0. */
int radnet_affine_vec(radnet_ctx* ctx, float* out, const float* a, const float* b, const float* c, int64_t n);
/* Input gradient of a stride-s 1x1 convolution (resnet50.py:100,111: the first 1x1 and the shortcut of every
 * conv_block).  The GEMM runs on the compact grid -- radnet_conv_dgrad with a descriptor whose input geometry is
 * the OUTPUT grid (h = oh, w = ow, stride 1) -- and this pass places its rows at (oh*s, ow*s) of the full
 * [nb][h][w][c] gradient, zeros elsewhere, then applies the producer's ReLU mask (mask > 0) if given.  Every element of dst is
 * written.  RADNET_ERR_ARG for nb < 1, oh < 1, ow < 1, c < 4, c % 4, stride < 1 or a compact grid that does not fit:
 * (oh - 1) * stride >= h or (ow - 1) * stride >= w; RADNET_ERR_UNSUPPORTED for 2^31 float4 elements or more. */
int radnet_scatter_strided(radnet_ctx* ctx, const float* src, int32_t nb, int32_t oh, int32_t ow, int32_t c, int32_t stride,
                           int32_t h, int32_t w, const float* mask, float* dst);
/* g[i] = act[i] > 0 ? g[i] : 0 -- ReLU backward where it cannot ride a GEMM epilogue (VGG16 head, vgg16.py:98-101).  A NaN
 * activation gives 0.  n = 0 launches nothing; RADNET_ERR_ARG for n < 0. */
int radnet_relu_mask(radnet_ctx* ctx, float* g, const float* act, int64_t n);

/* ==== layer programs and composed entry points (rpn_forward, train_step, predict_tile, allreduce_grads) ====
 * A layer program is a static array of launches the host scheduler builds once per input size from the reference's graph
 * (resnet50.py:150-281 nn_base / classifier_layer, rpn.py:12-66 rpn_layer, and their backward programs); radnet_program_run
 * enqueues it on the context's stream.  No allocation, no synchronisation: running it on a capturing stream records it into
 * a hipGraph.  Argument slots per kind (i = integers, p = device pointers):
 *   CONV_FWD / CONV_DGRAD / CONV_WGRAD   conv
 *   CONV_BWD     conv (radnet_conv_bwd: weight gradient + data gradient of the layer);  NOP: skipped
 *   CONV_FWD_PAIR conv = first convolution, the NEXT op's conv = second (its kind is NOP): radnet_conv_fwd_pair
 *   CONV_BNECK   conv = db, the next op's conv = dc, i[0] = 1: the op after that holds da (both NOP slots): radnet_conv_bottleneck
 *   MAXPOOL      p: x, y                     i: nb, h, w, c, k, s
 *   COLSUM       p: g, gscale|0, out         i: m, n, ld, accumulate
 *   WINO         p: x, v, u, m, scale|0, shift|0, y      i: nb, h, w, c, n, tiles, act, ldy, form   (radnet_winograd_input + 16
 *   WINO_REUSE   same, v already holds this input's transform                             GEMMs + radnet_winograd_output;
 *                                                                         form 4: the radnet_winograd4_* transforms, 36 GEMMs)
 *   WINO_WGRAD   p: dy, v, dz, du, dw, gscale|0   i: nb, h, w, c, n, ld_dy, tiles, ldw, accumulate mode (as radnet_conv_desc), form
 *   SCATTER      p: src, mask|0, dst         i: nb, oh, ow, c, stride, h, w
 *   FILL0        p: dst                      i: bytes (low 32 bits), bytes (high 32 bits)
 *   RELU_MASK    p: g, act                   i: n (low), n (high)
 *   ROI_BWD      p: dy, rois, dfmap          i: h, w, c, r, ps
 *   CHAIN        p: radnet_chain*             (radnet_chain_run: a run of CONV_FWD / WINO ops as one persistent launch)
 *   CONV_FWD_BF16 conv, p[0] = wt (bf16 weights), i[0] = ldk, i[1] = ksplit (0 or 1: one pass; radnet_conv_fwd_bf16_split)
 *                (bf16 predict programs: ksplit 0; bf16-mixed training programs: radnet_conv_bf16_pick_split of the layer)
 *   CONV_DGRAD_BF16 conv, p[0] = wd (the layer's dgrad image), i[0] = ldkd, i[1] = ksplit (radnet_conv_dgrad_bf16_split)
 *   CONV_WGRAD_BF16 conv, i[1] = msplit (radnet_conv_wgrad_bf16)
 *                (bf16-train training programs: radnet_dgrad_bf16_pick_split / radnet_wgrad_bf16_pick_split of the layer) */
enum {
  RADNET_OP_CONV_FWD = 1, RADNET_OP_CONV_DGRAD = 2, RADNET_OP_CONV_WGRAD = 3, RADNET_OP_MAXPOOL = 4, RADNET_OP_COLSUM = 5,
  RADNET_OP_WINO = 6, RADNET_OP_WINO_REUSE = 7, RADNET_OP_WINO_WGRAD = 8, RADNET_OP_SCATTER = 9, RADNET_OP_FILL0 = 10,
  RADNET_OP_RELU_MASK = 11, RADNET_OP_ROI_BWD = 12, RADNET_OP_CONV_BWD = 13, RADNET_OP_CHAIN = 14, RADNET_OP_CONV_FWD_PAIR = 15,
  RADNET_OP_CONV_BNECK = 16, RADNET_OP_CONV_FWD_BF16 = 17, RADNET_OP_CONV_DGRAD_BF16 = 18, RADNET_OP_CONV_WGRAD_BF16 = 19,
  RADNET_OP_NOP = 0
};
typedef struct radnet_op {
  int32_t kind;
  int32_t i[11];
  const void* p[8];
  radnet_conv_desc conv;
} radnet_op;
int radnet_program_run(radnet_ctx* ctx, const radnet_op* ops, int32_t n_ops);

/* ---- a run of dependent layers as ONE persistent launch ("chain"; resnet50.py:150-228 nn_base, stages 2-4) --------------
 * radnet_chain_build turns a list of CONV_FWD (channels a multiple of 32) and WINO (form 4) ops -- the same radnet_op[] that
 * radnet_program_run would launch one by one -- into a list of work items (output tiles, transform blocks) in dependency
 * order plus arrival counters; radnet_chain_run launches `workgroups` persistent workgroups (0: two per CU; at most 4 per CU)
 * among which the items are dealt statically (workgroup b: items b, b + grid, ...) and which start each item as soon as the
 * blocks it reads are complete.  The deal is deadlock-free only while EVERY workgroup of the grid is resident -- of every chain
 * running at the same time: callers that run chains side by side divide the 4 x 256 slots between them (the engine does).  Same kernels' code, same arithmetic per output element
 * as the launches it replaces for the convs (64x64 tiles; K-split layers add their slices in slice order); what goes away
 * is the gap between dependent launches, their lockstep prologue / epilogue phases and their tails.  A narrow
 * grid leaves CU slots to launches on other streams.  RADNET_ERR_UNSUPPORTED for an op the chain cannot run: the caller
 * keeps radnet_program_run.  The chain holds device memory of its own (items, counters, K-split slabs): build it outside
 * stream capture; radnet_chain_run allocates nothing and can be captured.  radnet_chain_status synchronises the stream;
 * last_error != 0: a workgroup waited 1 s for an input block that never completed (1 + item index; the launch still
 * drains, its outputs are INVALID).  The first such error is sticky and also lands in a mapped host word: radnet_chain_error
 * reads it without synchronising (0 = none so far; a launch still in flight may yet fail), and radnet_chain_run refuses
 * (RADNET_ERR_HIP) to launch a chain that has failed before.  Every tensor of the list must be written once and never after it
 * has been read (no buffer re-use inside a chain): radnet_chain_build / radnet_chain_check refuse such a list. */
typedef struct radnet_chain radnet_chain;
int radnet_chain_build(radnet_ctx* ctx, const radnet_op* ops, int32_t n_ops, int32_t workgroups, radnet_chain** out);
int radnet_chain_run(radnet_ctx* ctx, radnet_chain* chain);
int radnet_chain_status(radnet_ctx* ctx, radnet_chain* chain, int32_t* last_error, int32_t* runs, int32_t* n_items, int32_t* n_stages,
                        double* flops_executed, double* flops_algorithmic);
uint32_t radnet_chain_error(radnet_chain* chain);
void radnet_chain_destroy(radnet_chain* chain);
/* Diagnosis while a chain launch runs (uses a stream of its own): out[0..7] = {next item, workgroups gone, error, first
 * error, runs, ...}; with item >= 0, out[8..19] = its record {stage, bx, by, bz, dep0 first, dep0 count, dep1 first, dep1 count,
 * signal 0, signal 1, ..} and out[20 + 2k], out[21 + 2k] = current value / expected value of the k-th counter it waits for.
 * Returns the number of such pairs (or a negative error); out_words >= 148. */
int radnet_chain_peek(radnet_chain* chain, int32_t item, uint32_t* out, int32_t out_words);
/* Host-only (no device, no context): plans the work-item list of `ops` as radnet_chain_build would and checks that it can
 * run in list order -- every item finds its input blocks completed by earlier items, every counter reaches exactly the
 * count its waiters expect -- which is what makes the launch deadlock-free while its workgroups are all resident.  first_bad_item:
 * -1, or the offending item (n_items: a counter that never reaches its count).  The pointers in `ops` are used as
 * identities only.  radnet_chain_build runs the same check and refuses a list that fails it. */
int radnet_chain_check(const radnet_op* ops, int32_t n_ops, int32_t* n_items, int32_t* n_stages, int32_t* n_counters, int32_t* first_bad_item,
                       int32_t* bad_counter, char* err, int32_t err_len);

/* model_rpn.predict (RADNet.py:552; train.py:291): nn_base program, then rpn_layer program (outputs where the programs'
 * descriptors point: the fused head matrix [fh*fw][ld] with the sigmoid scores in columns [0,A), regressions in [A,5A)). */
int radnet_rpn_forward(radnet_ctx* ctx, const radnet_op* base_ops, int32_t n_base, const radnet_op* rpn_ops, int32_t n_rpn);

/* classifier_layer on n_rois RoIs of one feature map (resnet50.py:231-281): RoI crop-resize, stage-5 program, avg-pool,
 * dense heads.  rois [n_rois][4] fp32 (x,y,w,h); outputs p_cls [n_rois][nc] (softmax), p_regr [n_rois][nreg]. */
typedef struct radnet_head_desc {
  const float* fmap; int32_t fh, fw, fc;
  const float* rois; int32_t n_rois, pool; float* pooled;
  const radnet_op* fwd_ops; int32_t n_fwd;
  const float* y5; int32_t hw, feat_c; float* feat;
  const float* dense_w; int32_t dense_ld; const float* dense_b; int32_t nc, nreg;
  float* p_cls; float* p_regr;
  void* tail_scratch;      /* radnet_head_tail_scratch_bytes(n_rois) bytes, zeroed once by the caller */
} radnet_head_desc;

/* One tile of RADNet.predict up to the classifier outputs (RADNet.py:520-600): preprocess (img_u8 != 0: uint8 BGR [h][w][3]
 * -> x fp32 [h][w][4]), base + RPN programs, rpn.rpn_to_roi (decode + NMS, <= max_boxes RoIs in R / Rn), then -- when head is
 * set -- the first head->n_rois proposals (padded with copies of the first, RADNet.py:115-122) through classifier_layer. */
typedef struct radnet_tile_desc {
  const uint8_t* img_u8; int32_t h, w; float* x;
  const radnet_op* base_ops; int32_t n_base;
  const radnet_op* rpn_ops; int32_t n_rpn;
  const float* pred; int32_t ld_pred, fh, fw, a;
  const double* anchor_wh_host; double std_scaling, overlap_thresh; int32_t max_boxes;
  int64_t* R; float* Rp; int32_t* Rn; void* prop_ws;
  const radnet_head_desc* head;
} radnet_tile_desc;
int radnet_predict_tile(radnet_ctx* ctx, const radnet_tile_desc* t);

/* ---- the detection tail of a tile on the device (csrc/detect_tail.hip) ---------------------------------------------------
 * From the classifier outputs to detections in source-image pixels, bit for bit what the reference's host code gives on the
 * same tensors: the decode loop of apply_spatial_pyramid_pooling (RADNet.py:124-154) with rpn.apply_regr (rpn.py:346-378),
 * the per-class NMS 0.2 (RADNet.py:562-575 over rpn.py:380-455) and get_real_coordinates (RADNet.py:44-51).
 *
 * Rows looked at: the first ceil(*n / k) * k (whole chunks of k = n_rois RoIs, padding rows included; never more than `rows`).
 * Per row: best = the FIRST maximum of p_cls; dropped when max < bbox_threshold (an fp32 comparison, as NumPy 2 makes it against
 *   a Python float) or best == bg.  t_q = p_regr[4*best + q] / regr_std[q] is an fp32 division, the rest fp64:
 *   cx = tx*w + (x + w/2), w1 = exp(tw)*w, x1 = round_half_even(cx - w1/2), w1 = round_half_even(w1); where math.exp overflows
 *   or a NaN / infinity reaches round(), the row keeps its undecoded (x, y, w, h).  Box = rpn_stride * (x, y, x+w, y+h).
 *   exp is within 1 ulp of libm's: results can differ only where a value lies within 1 ulp of a half before rounding.
 * Per class: greedy NMS in fp64 with radnet_nms's suppression test and tie rule (among equal scores the higher row first),
 *   at most max_boxes picks.  A surviving box with x1 >= x2 or y1 >= y2 (the reference asserts): count = -1, no records.
 * Per pick: int(round(v // ratio)) with Python's float floor division (fmod-based; not floor(v / ratio)).
 * out: radnet_detect_tail_out_bytes(rows) bytes of int32 words: [0] count, [1] rows looked at, [2..7] reserved, then `count`
 *   records (class, x1, y1, x2, y2, prob as fp32 bits) -- classes in order of their first surviving row (the insertion order of
 *   the reference's dicts), picks of a class in pick order.  Coordinates beyond int32 saturate.
 * One launch of one workgroup; rows <= 1024, nc <= 32; no scratch memory besides `out`. */
/* int32 words of `out` in front of the records, and of a record */
#define RADNET_DETECT_HEADER_WORDS 8
#define RADNET_DETECT_RECORD_WORDS 6
typedef struct radnet_detect_tail_desc {
  const float* p_cls;      /* [rows][nc] softmax                                              */
  const float* p_regr;     /* [rows][4*(nc-1)]                                                */
  const float* rois;       /* [rows][4] (x, y, w, h), integers in feature-map units           */
  const int32_t* n;        /* device: proposal count                                          */
  int32_t rows, nc, k, bg;
  float bbox_threshold;
  float regr_std[4];       /* C.classifier_regr_std                                           */
  double rpn_stride, nms_thresh, ratio;
  int32_t max_boxes;
  void* out;
} radnet_detect_tail_desc;
uint64_t radnet_detect_tail_out_bytes(int32_t rows);
int radnet_detect_tail(radnet_ctx* ctx, const radnet_detect_tail_desc* d);
/* (x1,y1,x2,y2) int64 proposals R + device count (clamped to max_n) -> fp32 (x,y,w,h) RoIs for `rows` rows: row i < n is
 * proposal i; the padding rows of the last chunk of k repeat THAT chunk's first row (RADNet.py:110-122); rows past
 * ceil(n/k)*k, which radnet_detect_tail does not look at, repeat row 0. */
int radnet_rois_from_proposals(radnet_ctx* ctx, const int64_t* R, const int32_t* n_dev, int32_t max_n, int32_t k, int32_t rows,
                               float* rois);
/* radnet_predict_tile followed by the tail: one tile of RADNet.predict up to its detections (RADNet.py:520-575), no host
 * read-back inside the call.  t->head is built for ceil(t->max_boxes / d->k) * d->k rows, its RoIs come from
 * radnet_rois_from_proposals; d names the head's rois / p_cls / p_regr and t->Rn.  The rows the tail looks at equal those of
 * radnet_predict_tile on the same plan bit for bit (a GEMM row does not depend on the other rows of its launch). */
int radnet_predict_tile_detect(radnet_ctx* ctx, const radnet_tile_desc* t, const radnet_detect_tail_desc* d);

/* ---- the merge of a scan's tile detections on the device (csrc/scan_tail.hip) ---------------------------------------------
 * radnet_final_nms: RADNet.final_nms (RADNet.py:156-240) on a batch of groups, bit for bit what the host code returns.  The
 * groups stand one after the other: group g is the rows offsets[g] .. offsets[g + 1] of boxes / probs (offsets on the DEVICE,
 * so that a launch can follow the kernel that made them; every offset is clamped to 0 .. capacity before it is used).
 * Per group, on the STABLE ascending order of the fp32 probs walked from the end (among equal probs the higher row becomes
 * `top` first; -0 and +0 are equal): the members of top's cluster are the live boxes with
 *   overlap = double(inter) / (double(area_top + area - inter) + 1e-6) > obj_avg_threshold     (fp64; areas, inter in int64)
 * in order position, top last.  The members' maximum is top's prob.  Below obj_confidence_threshold (an fp32 comparison, as
 * NumPy 2 makes it against a Python float) the chosen boxes are the last n_obj_avg members; otherwise the members strictly
 * above it.  A cluster becomes (round_half_even(double(sum of the int64 coordinates) / count), fp32 sum / float(count)),
 * the fp32 sum being the one np.mean takes over a contiguous vector: below 8 elements in sequence; up to 128 eight interleaved
 * accumulators over blocks of 8, combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), the remainder in sequence; above 128 the two
 * halves split at n/2 rounded down to a multiple of 8, recursively.
 * Outputs of group g: its clusters in the order they were found at rows offsets[g] .. of out_boxes / out_probs (rows past the
 * cluster count are not written), out_count[g], out_status[g]:
 *   0                         success
 *   RADNET_FINAL_NMS_MALFORMED   a box with x1 >= x2 or y1 >= y2 (the host asserts)
 *   RADNET_FINAL_NMS_EMPTY       a cluster whose maximum equals the threshold, so that nothing is chosen (the host takes
 *                                the mean of an empty slice)
 *   RADNET_FINAL_NMS_RANGE       a coordinate beyond +-RADNET_SCAN_MAX_COORD, or a NaN prob
 * With a negative status the other outputs of that group are unspecified and the caller takes the host path.
 * One launch, a workgroup of 1024 threads per group: a bitonic sort of the group's keys, then per cluster one parallel pass
 * over the positions below top, then a second sort that lays every cluster's members side by side and a thread per cluster
 * for the means.  Bounded by `capacity` alone: all per-box state lives in ws (radnet_final_nms_ws_bytes bytes, no
 * initialisation needed), LDS holds a sort of up to 2048 keys and nothing that grows with the group.  Integer atomics in LDS
 * only; no floating-point atomics.  RADNET_ERR_ARG for a null pointer, n_groups < 0, capacity < 0 or n_obj_avg < 1;
 * n_groups == 0 launches nothing. */
#define RADNET_FINAL_NMS_MALFORMED -1
#define RADNET_FINAL_NMS_EMPTY -2
#define RADNET_FINAL_NMS_RANGE -3
/* 1 << 29: widths, areas and the coordinate sums of a cluster then stay far inside int64 */
#define RADNET_SCAN_MAX_COORD 536870912
typedef struct radnet_final_nms_desc {
  const int64_t* boxes;    /* device [capacity][4] (x1, y1, x2, y2)                            */
  const float* probs;      /* device [capacity]                                               */
  const int32_t* offsets;  /* device [n_groups + 1]                                           */
  int32_t n_groups, capacity;
  double obj_avg_threshold;
  float obj_confidence_threshold;
  int32_t n_obj_avg;
  int64_t* out_boxes;      /* device [capacity][4]                                            */
  float* out_probs;        /* device [capacity]                                               */
  int32_t* out_count;      /* device [n_groups]                                               */
  int32_t* out_status;     /* device [n_groups]                                               */
  void* ws;                /* device, radnet_final_nms_ws_bytes(capacity, n_groups) bytes     */
} radnet_final_nms_desc;
uint64_t radnet_final_nms_ws_bytes(int32_t capacity, int32_t n_groups);
int radnet_final_nms(radnet_ctx* ctx, const radnet_final_nms_desc* d);

/* radnet_scan_merge: the tail of RADNet.predict behind the tile passes (RADNet.py:577-718: the offsets, final_nms per image
 * and class, NMS across the images per class), with no host read-back inside the call.
 * pool: device int32 words; tile t's slot starts at word tiles[t].slot and holds what radnet_detect_tail wrote there for a
 * head of at most slot_rows rows (slot_words = radnet_detect_tail_out_bytes(slot_rows) / 4).  tiles_host / tiles_dev hold the
 * SAME table on the host and on the device (the caller uploads it; this entry copies nothing); the host copy goes through
 * radnet_scan_merge_check first.  Tiles stand in predict's order, image indices do not decrease.
 *   gather     per image and class the records of that class over the image's tiles, in tile order and within a tile in
 *              record order, (ox, oy) added in int64;
 *   cluster    radnet_final_nms on every (image, class) group;
 *   final NMS  per class the clusters of its images in image order, then cluster order: greedy NMS in fp64 with radnet_nms's
 *              suppression test and tie rule at nms_thresh, at most max_boxes picks;
 *   write      out: radnet_scan_merge_out_bytes(nc, max_boxes) bytes of int32 words: [0] count, [1] status, [2..7] reserved
 *              (not written), then `count` records (class, x1, y1, x2, y2, prob as fp32 bits): the classes in the order of
 *              their first appearance over the tiles (the insertion order of the reference's dicts), the picks of a class in
 *              pick order.  Words past the last record are not written.
 * Status: 0, or the smallest of the first four below, or -- when none of them is met -- the fifth:
 *   RADNET_SCAN_MERGE_BAD_SLOT    a slot whose count is -1 (its tile met a malformed box), exceeds slot_rows, or that holds a
 *                                 class outside 0 .. nc - 1
 *   RADNET_SCAN_MERGE_MALFORMED   RADNET_FINAL_NMS_MALFORMED of a group
 *   RADNET_SCAN_MERGE_EMPTY       RADNET_FINAL_NMS_EMPTY of a group
 *   RADNET_SCAN_MERGE_RANGE       RADNET_FINAL_NMS_RANGE of a group (a coordinate beyond +-RADNET_SCAN_MAX_COORD, hence
 *                                 every coordinate beyond int32)
 *   RADNET_SCAN_MERGE_NMS_BOX     a cluster mean with x1 >= x2 or y1 >= y2 at the final NMS (radnet_nms's count -1)
 * and then count = 0 and no record is written: the caller takes the host path on a download of the pool.
 * Six launches on the context's stream (count, plan, fill, radnet_final_nms, a workgroup per class for the final NMS, write);
 * none waits on another but through stream order.  Bounded by n_tiles * slot_rows boxes and n_images * nc groups; all state in
 * ws (radnet_scan_merge_ws_bytes bytes, no initialisation needed).  RADNET_ERR_ARG for a null pointer, a table the check refuses,
 * nc outside 1 .. RADNET_SCAN_MAX_CLASSES, max_boxes < 1 or n_obj_avg < 1.  n_tiles == 0 writes count 0, status 0. */
#define RADNET_SCAN_MERGE_BAD_SLOT -1
#define RADNET_SCAN_MERGE_MALFORMED -2
#define RADNET_SCAN_MERGE_EMPTY -3
#define RADNET_SCAN_MERGE_RANGE -4
#define RADNET_SCAN_MERGE_NMS_BOX -5
#define RADNET_SCAN_MAX_CLASSES 32
#define RADNET_SCAN_MAX_TILES 65536
#define RADNET_SCAN_MAX_IMAGES 4096
/* n_tiles * slot_rows at most (1 << 26) */
#define RADNET_SCAN_MAX_BOXES 67108864
typedef struct radnet_scan_tile {
  int32_t slot;            /* first word of the tile's slot in the pool                       */
  int32_t ox, oy;          /* the tile's offset in its image                                  */
  int32_t image;           /* index of its image in the call                                  */
} radnet_scan_tile;        /* 16 bytes */
typedef struct radnet_scan_merge_desc {
  const int32_t* pool;     /* device                                                          */
  int64_t pool_words;
  int32_t slot_rows;
  const radnet_scan_tile* tiles_host;
  const radnet_scan_tile* tiles_dev;
  int32_t n_tiles, nc;
  double obj_avg_threshold;
  float obj_confidence_threshold;
  int32_t n_obj_avg;
  double nms_thresh;
  int32_t max_boxes;
  void* out;               /* device, radnet_scan_merge_out_bytes(nc, max_boxes) bytes        */
  void* ws;                /* device, radnet_scan_merge_ws_bytes(n_tiles, slot_rows, n_images, nc, max_boxes) bytes */
} radnet_scan_merge_desc;
uint64_t radnet_scan_merge_out_bytes(int32_t nc, int32_t max_boxes);
uint64_t radnet_scan_merge_ws_bytes(int32_t n_tiles, int32_t slot_rows, int32_t n_images, int32_t nc, int32_t max_boxes);
int radnet_scan_merge(radnet_ctx* ctx, const radnet_scan_merge_desc* d);
/* Host only (csrc/scan_merge_check.cpp; no context, no device, like radnet_heat_check): the checks of a tile table for a pool
 * of pool_words int32 words whose slots hold slot_rows rows each.  1 <= slot_rows, 0 <= n_tiles <= RADNET_SCAN_MAX_TILES and
 * n_tiles * slot_rows <= RADNET_SCAN_MAX_BOXES; per entry slot >= 0, even (the slot is 8-byte aligned) and slot + slot_words <=
 * pool_words; no two slots overlap (they may stand in any order); 0 <= image < RADNET_SCAN_MAX_IMAGES, not below the entry
 * before; |ox|, |oy| <= RADNET_SCAN_MAX_COORD, so that ox + any int32 coordinate of a record is an int64 sum that the device
 * forms without overflow and then holds against RADNET_SCAN_MAX_COORD.  RADNET_OK with the number of images (last index + 1; 0
 * for no tiles) in *n_images, or RADNET_ERR_ARG with the index of the first bad entry in *bad_entry (-1 when the arguments
 * themselves are at fault) and a sentence naming the entry and the field in msg (at most msg_cap bytes with the terminator).
 * n_images, bad_entry and msg may be null.  Reads exactly n_tiles entries. */
int radnet_scan_merge_check(const radnet_scan_tile* tiles, int32_t n_tiles, int64_t pool_words, int32_t slot_rows, int32_t* n_images,
                            int32_t* bad_entry, char* msg, int32_t msg_cap);

/* One flat optimizer arena (train.py:236-252: one Adam per model). */
typedef struct radnet_adam_desc {
  float* p; float* g; float* m; float* v; int64_t n; int32_t t; float lr;
} radnet_adam_desc;

/* The two places where a reference iteration draws from NumPy's GLOBAL random stream stay on the host, in the caller's RNG:
 *   subsample_anchors  utils.py:785-813: valid / overlap uint8 [a][fh][fw] (host); edits valid in place; returns n_pos, or < 0
 *                      when the labeller fails as the reference's does (the sample is skipped, utils.py:461-465);
 *   select_rois        train.py:93-129: cls[n] class index per proposal (-1 = dropped by calc_iou); writes n_rois indices into
 *                      the proposal list to sel; returns n_rois, or 0 when no proposal was kept (head step skipped). */
typedef struct radnet_host_hooks {
  void* user;
  int32_t (*subsample_anchors)(void* user, uint8_t* valid, const uint8_t* overlap, int32_t a, int32_t fh, int32_t fw);
  int32_t (*select_rois)(void* user, const int32_t* cls, int32_t n, int32_t* sel, int32_t n_rois);
} radnet_host_hooks;

/* One reference training iteration on one image (train.py:288-402), synchronous, on the context's stream:
 * anchor targets -> base + RPN forward -> [hook] -> RPN losses / backward -> [all-reduce] -> Adam #1 -> re-prediction ->
 * proposals -> RoI labelling -> [hook] -> classifier forward / losses / backward -> [all-reduce] -> Adam #2.  The caller owns
 * every buffer (h_* are pinned host mirrors) and increments the optimizers' t before the call.  world > 1: the gradient
 * arenas are summed over the communicator of radnet_comm_init and the update uses 1/world (one image per rank).
 * losses5 = (rpn_cls, rpn_regr, det_cls, det_regr, det_acc); took_head_step = 1, 0 when the classifier step was skipped
 * (no proposal kept), -1 when the labeller hook dropped the image (nothing was trained, no optimizer step). */
typedef struct radnet_train_desc {
  const uint8_t* img_u8; int32_t h, w; float* x;
  const double* gt; const int32_t* gt_is_bg; const int32_t* gt_cls; int32_t g, width, height;
  const double* anchor_sizes_host; int32_t ns; const double* anchor_ratios_host; int32_t nr;
  double rpn_stride, rpn_max_overlap, std_scaling;
  uint8_t* valid; uint8_t* overlap; double* regr; int32_t* best_anchor; int32_t* n_for_gt; void* at_scratch;
  uint8_t* h_valid; uint8_t* h_overlap; float* y_cls; float* y_regr;
  const radnet_op* base_ops; int32_t n_base;
  const radnet_op* rpn_fwd_ops; int32_t n_rpn_fwd;
  const radnet_op* rpn_bwd_ops; int32_t n_rpn_bwd;
  const radnet_op* rpn_refwd_ops; int32_t n_rpn_refwd;
  float* pred; float* dz; int32_t ld_pred, fh, fw, a, bce_mode; double* loss_scratch8; float* rpn_losses;
  radnet_adam_desc rpn_opt, head_opt; int32_t world;
  const float* wino_w; int32_t wino_c, wino_n, wino_ldw, wino_form; float* wino_u;   /* rpn_conv1 filter re-transform after Adam #1; form 4 = F(4x4) */
  const double* anchor_wh_host; double overlap_thresh; int32_t max_boxes;
  int64_t* R; float* Rp; int32_t* Rn; void* prop_ws;
  int32_t rw, rh; double min_overlap, max_overlap; const double* regr_std_host4; int32_t bg_class;
  uint8_t* keep; int32_t* roi_cls; int32_t* roi_box; double* roi_t; double* roi_iou;
  int32_t* h_roi_cls; int32_t* h_n; int32_t* sel; int32_t* h_sel;
  const radnet_head_desc* head; float* y1; float* y2;
  float* head_dz; float* det_losses; float* dense_dw; float* dense_db; float* dfeat; float* g_last;
  const radnet_op* head_bwd_ops; int32_t n_head_bwd;
  float* head_shift; const float* head_scale; const float* head_bias; const float* head_t0; int64_t head_bias_len;
  void* tail_scratch;      /* unused (the head descriptor carries the scratch); kept for layout stability */
  const radnet_adam_wino* head_wino; int32_t n_head_wino;   /* classifier 3x3 kernels whose training forward runs on Winograd filters: Adam #2 rewrites them (radnet_adam_step_fused) */
} radnet_train_desc;
int radnet_train_step(radnet_ctx* ctx, const radnet_train_desc* d, const radnet_host_hooks* hooks, float* losses5,
                      int32_t* took_head_step);

/* ---- data-parallel gradient exchange over RCCL / xGMI ---------------------------------------------------
 * One communicator per context: rank 0 draws the id (radnet_comm_unique_id) and hands it to the other ranks through whatever
 * rendezvous the job has (torch.distributed's store, a file, MPI); every rank then calls radnet_comm_init.  The collective
 * is enqueued on the context's stream, in place, fp32 sum.  RCCL is bound at run time: RADNET_ERR_UNSUPPORTED without it. */
int radnet_comm_unique_id(char out128[128]);
int radnet_comm_init(radnet_ctx* ctx, int32_t world, int32_t rank, const char id128[128]);
int radnet_comm_destroy(radnet_ctx* ctx);
int radnet_allreduce_grads(radnet_ctx* ctx, float* grads, int64_t count);
/* Exchanges issued on this context so far (calls, fp32 elements): lets a caller check that every rank of a data-parallel job
 * takes part in the same sequence of collectives, whatever path its own image took through radnet_train_step. */
int radnet_comm_stats(radnet_ctx* ctx, int64_t* calls, int64_t* elements);

#ifdef __cplusplus
}
#endif
#endif /* RADNET_HIP_H */
