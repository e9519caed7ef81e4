// =====================================================================================================================
// Chain kernel: a run of dependent layers as ONE persistent launch
// =====================================================================================================================
// nn_base (resnet50.py:150-228) at batch 1 is ~50 dependent launches of 10-25 us.  Each loses 2 us to the gap behind
// the previous launch, 2 + 3 us to prologue / epilogue phases that all of its workgroups pass through together, and a tail in
// which the CUs with one workgroup fewer idle (profiles/r02_workgroup_stamps.txt) -- about half of the 0.95 ms the chain
// takes alone on the chip.  Here the whole run is one launch of `grid` persistent workgroups that draw WORK ITEMS -- one
// output tile of a conv (conv_igemm_body: the same code the layer launches run), or a block of a Winograd transform -- from
// a list the host wrote in dependency order, and start an item as soon as the items it reads from have finished:
//   * every stage (conv, Winograd input transform, batched Winograd GEMM, output transform) owns arrival counters over
//     blocks of its output (64 rows of a conv output, 64 tiles of a transformed operand, one tile row of a Winograd layer's
//     output); a finished item adds 1 to the counters of the blocks it wrote, an item waits until the blocks it reads have
//     reached the count the host computed for them (`need`);
//   * hand-off between workgroups is the split-K protocol of conv_igemm_body: outputs are written through (sc1 stores),
//     the writer drains them (vmcnt(0)) and bumps the counter with a relaxed agent-scope atomic, the reader polls the counter
//     with agent-scope loads.  Consumers read the data with ordinary loads: a line of an activation tensor is complete before
//     any workgroup may touch it (the counters cover whole rows of whole tiles, tensors are not shared, a launch starts with
//     clean caches), so no cache on the reader's side can hold an older copy;
//   * items are DEALT statically (workgroup b runs items b, b + grid, b + 2 grid, ...: a shared queue head cost one same-address
//     atomic per item) and the list is topologically sorted, so the lowest unfinished item belongs to a workgroup whose earlier
//     items are finished -- i.e. it is being run -- PROVIDED EVERY WORKGROUP OF THE GRID IS RESIDENT: the deal is deadlock-free
//     only while grid (x the number of chains running at the same time, plus whatever other launches hold CU slots) fits the
//     chip's 4 workgroups per CU.  radnet_chain_build caps one grid at 4 * 256; the engine divides that by the chains it runs
//     side by side.  A poll that does not see its counters move within 1 s raises `error` and every workgroup leaves (the grid
//     always drains); the launch's outputs are then INVALID and radnet_chain_run of the NEXT launch of that chain returns
//     RADNET_ERR_HIP (the sticky hdr->last_error travels to a mapped host word), as does radnet_chain_status;
//   * the last workgroup to leave zeroes the counters and the queue head: the launch can be replayed (hipGraph).
// A narrow grid (1-2 workgroups per CU) leaves CU slots to the other lanes' launches: the frozen base forward of an announced
// batch is background work in the pipelined step.
#include "chain_plan.h"
#include "conv_host.h"
#include "conv_igemm_body.h"
#include "radnet_wino4.h"

namespace {
// One block (256 units: a unit = one tile x 1 channel: 36 live registers, so the item does not
// raise the register budget of the GEMM items it shares the kernel with) of the F(4x4,3x3) input transform, write-through stores.
__device__ __forceinline__ void chain_wino4_input(const ChainStage& st, unsigned block) {
  typedef float VT;
  const int cv = st.t_c, H = st.t_h, W_ = st.t_w, C = st.t_c, TH = st.t_th, TW = st.t_tw;
  const unsigned T = (unsigned)(st.t_nb * TH * TW), total = T * (unsigned)cv;
  const unsigned i = block * 256u + threadIdx.x;
  if (i >= total) return;
  const unsigned tile = i / (unsigned)cv;
  const int cq = (int)(i - tile * (unsigned)cv);
  const unsigned trow = tile / (unsigned)TW;
  const int tj = (int)(tile - trow * (unsigned)TW);
  const int img = (int)(trow / (unsigned)TH);
  const int ti = (int)(trow - (unsigned)img * (unsigned)TH);
  const float* x = st.t_src;
  VT t[6][6];
#pragma unroll
  for (int b = 0; b < 6; ++b) {
    const int iw = 4 * tj - 1 + b;
    VT col[6], o[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      const int ih = 4 * ti - 1 + a;
      col[a] = ((unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W_)
                   ? *reinterpret_cast<const VT*>(x + (((long long)img * H + ih) * W_ + iw) * C + cq)
                   : vzero<VT>();
    }
    bt6(col, o);
#pragma unroll
    for (int a = 0; a < 6; ++a) t[a][b] = o[a];
  }
  const __amdgpu_buffer_rsrc_t rd = make_rsrc(st.t_dst, st.t_dst_bytes);
  const unsigned off0 = (tile * (unsigned)cv + (unsigned)cq) * 4u, ps = total * 4u;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    VT o[6];
    bt6(t[a], o);
#pragma unroll
    for (int b = 0; b < 6; ++b) buf_store1_sc1(rd, off0 + (unsigned)(6 * a + b) * ps, o[b]);
  }
}

// One block of the output transform (+ folded BN scale / shift, ReLU), write-through stores.
__device__ __forceinline__ void chain_wino4_output(const ChainStage& st, unsigned block) {
  typedef float VT;
  const int N = st.t_c, nv = N, OH = st.t_h, OW = st.t_w, TH = st.t_th, TW = st.t_tw, ldy = st.t_ldy;
  const unsigned T = (unsigned)(st.t_nb * TH * TW), total = T * (unsigned)nv;
  const unsigned i = block * 256u + threadIdx.x;
  if (i >= total) return;
  const unsigned tile = i / (unsigned)nv;
  const int nq = (int)(i - tile * (unsigned)nv);
  const unsigned trow = tile / (unsigned)TW;
  const int tj = (int)(tile - trow * (unsigned)TW);
  const int img = (int)(trow / (unsigned)TH);
  const int ti = (int)(trow - (unsigned)img * (unsigned)TH);
  const VT* src = reinterpret_cast<const VT*>(st.t_src) + tile * (unsigned)nv + nq;
  const size_t ps = total;
  VT t[4][6];
#pragma unroll
  for (int b = 0; b < 6; ++b) {
    VT col[6], o[4];
#pragma unroll
    for (int a = 0; a < 6; ++a) col[a] = src[(size_t)(6 * a + b) * ps];
    at6(col, o);
#pragma unroll
    for (int a = 0; a < 4; ++a) t[a][b] = o[a];
  }
  VT sc = 1.f, sh = 0.f;
  if (st.t_scale) sc = *reinterpret_cast<const VT*>(st.t_scale + nq);
  if (st.t_shift) sh = *reinterpret_cast<const VT*>(st.t_shift + nq);
  const __amdgpu_buffer_rsrc_t rd = make_rsrc(st.t_dst, st.t_dst_bytes);
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int oh = 4 * ti + a;
    VT o[4];
    at6(t[a], o);
    if (oh >= OH) continue;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int ow = 4 * tj + b;
      if (ow >= OW) continue;
      VT v = st.t_scale ? o[b] * sc + sh : o[b] + sh;
      if (st.t_act == 1) v = vmax0(v);
      buf_store1_sc1(rd, (unsigned)((((unsigned)img * OH + oh) * OW + ow) * (unsigned)ldy + nq) * 4u, v);
    }
  }
}

constexpr unsigned long long kChainGiveUpTicks = 100000000ull;      // 1 s of the 100 MHz real-time counter: a workgroup gives up waiting

template <bool COHV, int DBG = 0>
__device__ __forceinline__ void chain_body(ChainHeader* __restrict__ hdr, const ChainStage* __restrict__ stages,
                                                         const ChainItem* __restrict__ items, unsigned* __restrict__ counters,
                                                         const unsigned* __restrict__ need, unsigned n_items, unsigned n_counters,
                                                         unsigned* __restrict__ marks, float* __restrict__ lds, unsigned* __restrict__ s_ctl) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // progress mark of every WAVE (diagnosis, radnet_chain_peek): phase in the low byte, item above it
#define CHAIN_MARK(phase, item) do { if (marks != nullptr && lane == 0) __hip_atomic_store(marks + blockIdx.x * 4 + wave, ((item) << 8) | (phase), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); } while (0)
  // Control flow: every barrier of this loop must be reached by all four waves the same number of times.  The queue draw is
  // one lane's work; it sits at the END of the loop body (and once in front of the loop), not at its head -- a lane-divergent
  // branch at the head of a loop makes the compiler split the loop so that the other lanes of that wave run on to the barrier
  // first and the drawing lane arrives at it a second time (seen as a hang: waves of one workgroup in different phases).
  // The loop's own conditions are wave-uniform scalars (readfirstlane).
  // Static deal: workgroup b runs items b, b + grid, b + 2 grid, ... (a shared queue head costs one same-address atomic per
  // item: 38 720 of them serialised to ~2 ms for a 1000x600 base forward, more than the launches they replace).  Still
  // deadlock-free while every workgroup of the grid is resident (radnet_chain_build caps the grid at the chip's capacity for
  // this kernel): the lowest unfinished item belongs to a workgroup whose earlier items are finished, i.e. it is being run.
  if (threadIdx.x == 0) s_ctl[1] = 0u;
  __syncthreads();
  unsigned idx = blockIdx.x;
  bool gave_up = false;
  for (; idx < n_items; idx += gridDim.x) {
    CHAIN_MARK(1u, idx);
    const ChainItem* ip = items + idx;
    const int it_stage = __builtin_amdgcn_readfirstlane(ip->stage);
    const int it_bx = __builtin_amdgcn_readfirstlane(ip->bx), it_by = __builtin_amdgcn_readfirstlane(ip->by), it_bz = __builtin_amdgcn_readfirstlane(ip->bz);
    const int d0f = __builtin_amdgcn_readfirstlane(ip->d0_first), d0n = __builtin_amdgcn_readfirstlane(ip->d0_count);
    const int d1f = __builtin_amdgcn_readfirstlane(ip->d1_first), d1n = __builtin_amdgcn_readfirstlane(ip->d1_count);
    const int sig0 = __builtin_amdgcn_readfirstlane(ip->sig0), sig1 = __builtin_amdgcn_readfirstlane(ip->sig1);
    // ---- wait until the blocks this item reads are complete: one counter per lane, one round trip per poll
    if (DBG != 2 && wave == 0 && d0n + d1n > 0) {      // DBG 2 (diagnosis): nobody waits -- results are garbage, the time is the items' own
      const int ci = lane < d0n ? d0f + lane : (lane < d0n + d1n ? d1f + (lane - d0n) : -1);
      const unsigned want = ci >= 0 ? need[ci] : 0u;
      const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();      // 100 MHz, constant
      unsigned polls = 0;
      for (;;) {
        const unsigned have = ci >= 0 ? __hip_atomic_load(counters + (size_t)ci * kCtrStride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        if (__all(have >= want)) break;
        if ((++polls & 63u) == 0u) {             // now and then: has somebody given up / have we waited kChainGiveUpTicks
          const bool late = __builtin_amdgcn_s_memrealtime() - t0 > kChainGiveUpTicks;
          if (late || __hip_atomic_load(&hdr->error, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
            if (late && lane == 0) __hip_atomic_store(&hdr->error, idx + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (lane == 0) s_ctl[1] = 1u;
            break;
          }
        }
        // back off: a workgroup that is early for its inputs must not crowd out the atomics that would complete them
        if (polls < 4u) __builtin_amdgcn_s_sleep(16);
        else if (polls < 16u) __builtin_amdgcn_s_sleep(48);
        else __builtin_amdgcn_s_sleep(127);
      }
    }
    __syncthreads();
    gave_up = __builtin_amdgcn_readfirstlane(s_ctl[1]) != 0u;      // some wait of the launch timed out: leave (uniform for the workgroup)
    if (gave_up) break;
    CHAIN_MARK(2u, idx);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");          // compiler-only: the item's loads stay below the poll
    const ChainStage& st = stages[it_stage];
    const int type = __builtin_amdgcn_readfirstlane(st.type);
    if (DBG == 1) {
      // diagnosis: the queue / counter machinery without any item work
    } else if (type == 0) {
      GemmArgs g = st.g;
      conv_igemm_body<64, 64, 0, false, 4, COHV>(g, lds, (unsigned)it_bx, (unsigned)it_by, (unsigned)it_bz, 0u);
    } else if (type == 1) {
      chain_wino4_input(st, (unsigned)it_bx);
    } else {
      chain_wino4_output(st, (unsigned)it_bx);
    }
    // ---- publish: every store of this workgroup has left (write-through), then the counters move
    CHAIN_MARK(3u, idx);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    CHAIN_MARK(4u, idx);
    if (wave == 0) {
      if (lane == 0) {
        if (sig0 >= 0) __hip_atomic_fetch_add(counters + (size_t)sig0 * kCtrStride, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (sig1 >= 0) __hip_atomic_fetch_add(counters + (size_t)sig1 * kCtrStride, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  // ---- the last workgroup to leave restores the initial state (replay), keeping the first error for the host
  CHAIN_MARK(5u, 0u);
  if (wave == 0) {
    if (lane == 0) s_ctl[2] = __hip_atomic_fetch_add(&hdr->exited, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1 ? 1u : 0u;
  }
  __syncthreads();
  if (s_ctl[2] != 0u) {
    // (the K-split tile counters inside the spans reset themselves; after an aborted launch they may not have: clear everything)
    const bool aborted = __hip_atomic_load(&hdr->error, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
    if (aborted)
      for (size_t i = tid; i < (size_t)n_counters * kCtrStride; i += NTHREADS) __hip_atomic_store(counters + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
      for (unsigned i = tid; i < n_counters; i += NTHREADS) __hip_atomic_store(counters + (size_t)i * kCtrStride, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid == 0) {
      const unsigned e = __hip_atomic_load(&hdr->error, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (e != 0u && hdr->last_error == 0u) {
        hdr->last_error = e;
        unsigned* hp = reinterpret_cast<unsigned*>(((unsigned long long)hdr->host_hi << 32) | (unsigned long long)hdr->host_lo);
        if (hp != nullptr) __hip_atomic_store(hp, e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
      hdr->runs += 1u;
      __hip_atomic_store(&hdr->error, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&hdr->next, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&hdr->exited, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}


#define CHAIN_KERNEL(name, attr, coh, dbg)                                                                                         \
  __global__ void __launch_bounds__(NTHREADS) attr name(ChainHeader* __restrict__ hdr, const ChainStage* __restrict__ stages, \
                                                        const ChainItem* __restrict__ items, unsigned* __restrict__ counters,  \
                                                        const unsigned* __restrict__ need, unsigned n_items, unsigned n_counters, \
                                                        unsigned* __restrict__ marks) {                                        \
    __shared__ __attribute__((aligned(16))) float lds[igemm_lds_floats<64, 64, 0>()];                                          \
    __shared__ unsigned s_ctl[4];                                                                                              \
    chain_body<coh, dbg>(hdr, stages, items, counters, need, n_items, n_counters, marks, lds, s_ctl);                          \
  }
CHAIN_KERNEL(chain_kernel, __attribute__((amdgpu_waves_per_eu(4, 4))), true, 0)
CHAIN_KERNEL(chain_kernel_noattr, , true, 1)
CHAIN_KERNEL(chain_kernel_nocoh, __attribute__((amdgpu_waves_per_eu(4, 4))), true, 2)
}  // namespace

struct radnet_chain {
  ChainHeader* d_hdr = nullptr;
  ChainStage* d_stages = nullptr;
  ChainItem* d_items = nullptr;
  unsigned* d_counters = nullptr;
  unsigned* d_need = nullptr;
  int* d_units = nullptr;
  float* d_slabs = nullptr;
  unsigned* d_marks = nullptr;      // RADNET_CHAIN_DEBUG=1: one word per wave (phase, item)
  unsigned* h_err = nullptr;        // mapped host word: first 'gave up waiting' error of any launch (1 + item), sticky
  unsigned n_items = 0, n_counters = 0, n_stages = 0;
  int grid = 0;
  std::vector<ChainItem> h_items;       // host copies for radnet_chain_peek / diagnosis
  std::vector<unsigned> h_need;
  double flops = 0.0;            // executed by the matrix cores
  double flops_algorithmic = 0.0;   // 2 M N K of the layers as direct convolutions (Winograd layers credited 9 C per output)
};

extern "C" void radnet_chain_destroy(radnet_chain* ch) {
  if (!ch) return;
  for (void* p : {(void*)ch->d_hdr, (void*)ch->d_stages, (void*)ch->d_items, (void*)ch->d_counters, (void*)ch->d_need, (void*)ch->d_units, (void*)ch->d_slabs, (void*)ch->d_marks})
    if (p) (void)hipFree(p);
  if (ch->h_err) (void)hipHostFree(ch->h_err);
  delete ch;
}

extern "C" int radnet_chain_build(radnet_ctx* ctx, const radnet_op* ops, int32_t n_ops, int32_t workgroups, radnet_chain** out) {
  if (!ctx || !ops || n_ops <= 0 || !out) return RADNET_ERR_ARG;
  *out = nullptr;
  // every workgroup of the grid must be resident (static deal, see chain_body): 4 per CU is what LDS and registers allow
  const int grid = std::min(workgroups > 0 ? workgroups : 2 * kNumCU, 4 * kNumCU);
  ChainPlan pl;
  {
    ErrSink ec{};
    const int rc = radnet_chain_plan(ops, n_ops, pl, ec);
    if (rc != RADNET_OK) RADNET_FAIL(ctx, rc, "%s", ec.err);
  }
  std::vector<ChainStage>& stages = pl.stages;
  std::vector<ChainItem>& items = pl.items;
  std::vector<unsigned>& need = pl.need;
  std::vector<int>& units = pl.units;
  std::vector<size_t>& unit_base = pl.unit_base;
  std::vector<size_t>& slab_base = pl.slab_base;
  const size_t slabs_total = pl.slabs_total;
  const double flops = pl.flops, flops_alg = pl.flops_alg;

  radnet_chain* ch = new radnet_chain();
  ch->grid = grid;
  ch->n_items = (unsigned)items.size();
  ch->n_counters = (unsigned)need.size();
  ch->n_stages = (unsigned)stages.size();
  ch->flops = flops;
  ch->flops_algorithmic = flops_alg;
  auto fail = [&](const char* what) {
    radnet_chain_destroy(ch);
    snprintf(ctx->err, sizeof(ctx->err), "chain: %s", what);
    return RADNET_ERR_HIP;
  };
  if (hipMalloc((void**)&ch->d_hdr, sizeof(ChainHeader)) != hipSuccess || hipMemset(ch->d_hdr, 0, sizeof(ChainHeader)) != hipSuccess) return fail("header");
  {
    if (hipHostMalloc((void**)&ch->h_err, sizeof(unsigned), hipHostMallocMapped) != hipSuccess) return fail("error word");
    *ch->h_err = 0u;
    ChainHeader h0{};
    h0.host_lo = (unsigned)((unsigned long long)(uintptr_t)ch->h_err & 0xffffffffull);
    h0.host_hi = (unsigned)((unsigned long long)(uintptr_t)ch->h_err >> 32);
    if (hipMemcpy(ch->d_hdr, &h0, sizeof(h0), hipMemcpyHostToDevice) != hipSuccess) return fail("header");
  }
  if (hipMalloc((void**)&ch->d_counters, need.size() * 4 * kCtrStride) != hipSuccess || hipMemset(ch->d_counters, 0, need.size() * 4 * kCtrStride) != hipSuccess) return fail("counters");
  if (hipMalloc((void**)&ch->d_need, need.size() * 4) != hipSuccess || hipMemcpy(ch->d_need, need.data(), need.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return fail("need");
  if (!units.empty() && (hipMalloc((void**)&ch->d_units, units.size() * 4) != hipSuccess || hipMemcpy(ch->d_units, units.data(), units.size() * 4, hipMemcpyHostToDevice) != hipSuccess)) return fail("units");
  if (slabs_total && hipMalloc((void**)&ch->d_slabs, slabs_total * 4) != hipSuccess) return fail("slabs");
  for (size_t s = 0; s < stages.size(); ++s) {
    if (unit_base[s] == ~(size_t)0) continue;
    GemmArgs& g = stages[s].g;
    g.units = ch->d_units + unit_base[s];
    g.partial = ch->d_slabs + slab_base[s];
    g.counters = ch->d_counters + (uintptr_t)g.counters * kCtrStride;      // dense tile counters inside this stage's strided span
  }
  if (hipMalloc((void**)&ch->d_stages, stages.size() * sizeof(ChainStage)) != hipSuccess ||
      hipMemcpy(ch->d_stages, stages.data(), stages.size() * sizeof(ChainStage), hipMemcpyHostToDevice) != hipSuccess) return fail("stages");
  if (hipMalloc((void**)&ch->d_items, items.size() * sizeof(ChainItem)) != hipSuccess ||
      hipMemcpy(ch->d_items, items.data(), items.size() * sizeof(ChainItem), hipMemcpyHostToDevice) != hipSuccess) return fail("items");
  ch->h_items = items;
  ch->h_need = need;
  if (getenv("RADNET_CHAIN_DEBUG") && (hipMalloc((void**)&ch->d_marks, (size_t)grid * 16) != hipSuccess || hipMemset(ch->d_marks, 0, (size_t)grid * 16) != hipSuccess)) return fail("marks");
  *out = ch;
  return RADNET_OK;
}

// Diagnosis WHILE a chain launch is (or seems to be) running: copies the header {next item, workgroups gone, error, first
// error, runs} and, for item `item` (>= 0), its record and the current values / expected values of the counters it waits
// for, through a stream of its own (does not wait for the launch).  out: 8 header words, 12 item words, then up to 64
// (have, need) pairs; returns the number of pairs.
extern "C" int radnet_chain_peek(radnet_chain* ch, int32_t item, uint32_t* out, int32_t out_words) {
  if (!ch || !out || out_words < 20 + 128) return RADNET_ERR_ARG;
  hipStream_t st = nullptr;
  if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return RADNET_ERR_HIP;
  int pairs = 0;
  bool ok = hipMemcpyAsync(out, ch->d_hdr, 8 * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
  if (ok && item >= 0 && (unsigned)item < ch->n_items) {
    const ChainItem& it = ch->h_items[(size_t)item];
    memcpy(out + 8, &it, 12 * 4);
    for (int r = 0; r < 2 && ok; ++r) {
      const int f = r == 0 ? it.d0_first : it.d1_first, n = r == 0 ? it.d0_count : it.d1_count;
      for (int k = 0; k < n && pairs < 64 && ok; ++k, ++pairs) {
        ok = hipMemcpyAsync(out + 20 + 2 * pairs, ch->d_counters + (size_t)(f + k) * kCtrStride, 4, hipMemcpyDeviceToHost, st) == hipSuccess;
        out[20 + 2 * pairs + 1] = ch->h_need[(size_t)f + k];
      }
    }
  }
  ok = ok && hipStreamSynchronize(st) == hipSuccess;
  if (ok && ch->d_marks && item == -2) {        // debug build of the chain: histogram of the waves' phases into out[20..27], a stuck wave's mark in out[28]
    std::vector<unsigned> m((size_t)ch->grid * 4);
    ok = hipMemcpyAsync(m.data(), ch->d_marks, m.size() * 4, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
    for (int k = 0; k < 9; ++k) out[20 + k] = 0;
    for (unsigned v : m) {
      out[20 + std::min(v & 255u, 7u)] += 1;
      if ((v & 255u) >= 1 && (v & 255u) <= 4) out[28] = v;
    }
  }
  (void)hipStreamDestroy(st);
  return ok ? pairs : RADNET_ERR_HIP;
}

extern "C" uint32_t radnet_chain_error(radnet_chain* ch) { return (ch && ch->h_err) ? *(volatile unsigned*)ch->h_err : 0u; }

extern "C" int radnet_chain_run(radnet_ctx* ctx, radnet_chain* ch) {
  if (!ctx || !ch) return RADNET_ERR_ARG;
  if (const uint32_t e = radnet_chain_error(ch))
    RADNET_FAIL(ctx, RADNET_ERR_HIP, "chain: an earlier launch of this chain gave up waiting at item %u (not every workgroup of its grid was resident?): "
                "its outputs were invalid", e - 1u);
  radnet_timing_arm(ctx);
  static const int variant = getenv("RADNET_CHAIN_VARIANT") ? atoi(getenv("RADNET_CHAIN_VARIANT")) : 0;      // diagnosis
  if (variant == 1)
    RADNET_LAUNCH(chain_kernel_noattr, dim3(ch->grid), dim3(NTHREADS), 0, ctx->stream, ctx->arm0, ctx->arm1, ch->d_hdr, ch->d_stages, ch->d_items,
                  ch->d_counters, ch->d_need, ch->n_items, ch->n_counters, ch->d_marks);
  else if (variant == 2)
    RADNET_LAUNCH(chain_kernel_nocoh, dim3(ch->grid), dim3(NTHREADS), 0, ctx->stream, ctx->arm0, ctx->arm1, ch->d_hdr, ch->d_stages, ch->d_items,
                  ch->d_counters, ch->d_need, ch->n_items, ch->n_counters, ch->d_marks);
  else
    RADNET_LAUNCH(chain_kernel, dim3(ch->grid), dim3(NTHREADS), 0, ctx->stream, ctx->arm0, ctx->arm1, ch->d_hdr, ch->d_stages, ch->d_items, ch->d_counters,
                  ch->d_need, ch->n_items, ch->n_counters, ch->d_marks);
  RADNET_CHECK_LAUNCH(ctx, "chain");
  radnet_timing_end_armed(ctx, 0, ch->flops_algorithmic);
  return RADNET_OK;
}

// Synchronises the context's stream.  last_error: 0, or 1 + the index of the first item that gave up waiting (sticky).
extern "C" int radnet_chain_status(radnet_ctx* ctx, radnet_chain* ch, int32_t* last_error, int32_t* runs, int32_t* n_items, int32_t* n_stages,
                                   double* flops_executed, double* flops_algorithmic) {
  if (!ctx || !ch) return RADNET_ERR_ARG;
  RADNET_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ChainHeader h;
  RADNET_CHECK_HIP(ctx, hipMemcpy(&h, ch->d_hdr, sizeof(h), hipMemcpyDeviceToHost));
  if (last_error) *last_error = (int32_t)h.last_error;
  if (runs) *runs = (int32_t)h.runs;
  if (n_items) *n_items = (int32_t)ch->n_items;
  if (n_stages) *n_stages = (int32_t)ch->n_stages;
  if (flops_executed) *flops_executed = ch->flops;
  if (flops_algorithmic) *flops_algorithmic = ch->flops_algorithmic;
  return RADNET_OK;
}
