// ---- host side of the chain kernel (chain.hip): radnet_op[] -> stages, items, counters ---------------------------------
// No device call and no HIP header: compiled by g++, radnet_chain_check runs without a GPU.
#include "chain_plan.h"
#include "radnet_host.h"
#include <algorithm>
#include <map>
#include <set>

namespace {

// where a stage's output can be waited for
struct ChainOut {
  enum Kind { ROWS64, TILES64, TILEROWS } kind = ROWS64;
  int first = 0, count = 0;       // its counters
  int h = 0, w = 0, th = 0, tw = 0;   // TILEROWS: output geometry (pixels, tiles)
};

template <typename E>
int chain_conv_args(E* ctx, const radnet_conv_desc* d, GemmArgs& g) {
  if (!d->x || !d->w || !d->y) RADNET_FAIL(ctx, RADNET_ERR_ARG, "chain: conv with a null tensor");
  g = GemmArgs{};
  g.x = d->x; g.w = d->w; g.y = d->y;
  g.scale = d->scale; g.shift = d->shift; g.addend = d->addend;
  g.H = d->h; g.W = d->w_; g.C = d->c; g.OH = d->oh; g.OW = d->ow;
  g.KW = d->kw; g.npos = d->kh * d->kw; g.stride = d->stride; g.pad_t = d->pad_t; g.pad_l = d->pad_l;
  g.M = d->nb * d->oh * d->ow; g.N = d->n; g.K = g.npos * d->c;
  g.ldw = d->ldw; g.ldy = d->ldy; g.ld_add = d->ld_add;
  g.act = d->act; g.act_cols = d->act_cols;
  g.OHOW = d->oh * d->ow;
  if (g.M <= 0 || g.N <= 0 || g.K <= 0 || g.M >= (1 << 20) || (g.ldw & 3) || (g.N & 3) || (g.C % BK) != 0 || g.npos > 32)
    RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "chain: conv M=%d N=%d K=%d C=%d taps=%d cannot run as chain items", g.M, g.N, g.K, g.C, g.npos);
  if (((uintptr_t)g.x & 15) || ((uintptr_t)g.w & 15)) RADNET_FAIL(ctx, RADNET_ERR_ARG, "chain: x / w must be 16-byte aligned");
  g.magic_ohow = radnet_div_magic((uint32_t)g.OHOW);
  g.magic_ow = radnet_div_magic((uint32_t)g.OW);
  const uint64_t xb = (uint64_t)d->nb * g.H * g.W * g.C * 4ull, wb = (uint64_t)g.K * g.ldw * 4ull;
  const uint64_t halo = ((uint64_t)g.pad_t * g.W + g.pad_l) * g.C * 4ull;
  const uint64_t ld_max = (uint64_t)std::max(g.ldy, g.addend ? g.ld_add : 0);
  if (xb + halo >= (1ull << 31) || wb >= (1ull << 31) || (uint64_t)g.M * ld_max * 4ull >= (1ull << 31))
    RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "chain: tensor larger than 2 GiB");
  if (g.ldy < g.N || (g.addend && g.ld_add < g.N)) RADNET_FAIL(ctx, RADNET_ERR_ARG, "chain: row pitch smaller than n=%d", g.N);
  g.x_bytes = (unsigned)xb;
  g.w_bytes = (unsigned)wb;
  g.y_bytes = (unsigned)(((uint64_t)(g.M - 1) * g.ldy + g.N) * 4ull);
  g.add_bytes = g.addend ? (unsigned)(((uint64_t)(g.M - 1) * g.ld_add + g.N) * 4ull) : 0u;
  return RADNET_OK;
}

}  // namespace

// Host-only: the work-item list of a program (no device call; radnet_chain_check runs it without a GPU).
static int chain_plan(const radnet_op* ops, int32_t n_ops, ChainPlan& pl, ErrSink& ec) {
  std::vector<ChainStage>& stages = pl.stages;
  std::vector<ChainOut> outs;                   // per stage
  std::vector<ChainItem>& items = pl.items;
  std::vector<unsigned>& need = pl.need;
  std::vector<int>& units = pl.units;
  std::vector<size_t>& unit_base = pl.unit_base;
  std::vector<size_t>& slab_base = pl.slab_base;
  std::vector<size_t> slab_floats;              // per stage (floats)
  std::map<const void*, int> producer;          // pixel tensor -> stage that writes it
  size_t& slabs_total = pl.slabs_total;
  double& flops = pl.flops;
  double& flops_alg = pl.flops_alg;

  auto new_counters = [&](int n, unsigned want) {
    const int first = (int)need.size();
    need.insert(need.end(), (size_t)n, want);
    return first;
  };
  // counters of `p` that cover rows [r0, r1] of the pixel tensor it writes -> (first, count)
  auto rows_dep = [&](int p, int r0, int r1, int& first, int& count) {
    const ChainOut& o = outs[p];
    if (o.kind == ChainOut::ROWS64) {
      first = o.first + r0 / 64;
      count = r1 / 64 - r0 / 64 + 1;
    } else {                                    // TILEROWS: one counter per (image, tile row)
      const int y0 = r0 / o.w, y1 = r1 / o.w;   // global pixel row = image * h + oh
      const int t0 = (y0 / o.h) * o.th + (y0 % o.h) / 4, t1 = (y1 / o.h) * o.th + (y1 % o.h) / 4;
      first = o.first + t0;
      count = t1 - t0 + 1;
    }
  };
  auto push_stage = [&](const ChainStage& st, const ChainOut& o) {
    stages.push_back(st);
    outs.push_back(o);
    unit_base.push_back(~(size_t)0);
    slab_base.push_back(0);
    slab_floats.push_back(0);
    return (int)stages.size() - 1;
  };
  // items of one conv / batched-GEMM stage; dep(tm, first, count) gives the counters tile row tm waits for
  auto emit_gemm = [&](int si, int batch, int dep_stage_main, int dep_stage_add, bool batched_dep) -> int {
    GemmArgs& g = stages[si].g;
    const int Mt = radnet_cdiv(g.M, 64), Nt = radnet_cdiv(g.N, 64), nk = radnet_cdiv(g.K, BK);
    int S = 1;
    if (batch <= 1) {
      const long long tiles = (long long)Mt * Nt;
      if (tiles < 384) S = (int)std::min<long long>(std::max(nk / 4, 1), (512 + tiles - 1) / tiles);
      const int kt = radnet_cdiv(nk, S);
      S = radnet_cdiv(nk, kt);
    }
    const int kt = radnet_cdiv(nk, S);
    ChainOut& o = outs[si];
    o.kind = batch > 1 ? ChainOut::TILES64 : ChainOut::ROWS64;
    o.count = Mt;
    o.first = new_counters(Mt, (unsigned)(Nt * S * (batch > 1 ? batch : 1)));
    int split_counters = -1;
    if (S > 1) {
      unit_base[si] = units.size();
      slab_base[si] = slabs_total;
      slab_floats[si] = (size_t)Mt * Nt * S * 4096;
      slabs_total += slab_floats[si];
      split_counters = new_counters(Mt * Nt, 0u);      // arrival counters of the in-launch reduction (never polled)
    }
    for (int tm = 0; tm < Mt; ++tm) {
      int d0f = 0, d0n = 0, d1f = 0, d1n = 0;
      if (batched_dep) {                        // batched Winograd GEMM: tile block tm of the transformed operand
        d0f = outs[dep_stage_main].first + tm;
        d0n = 1;
      } else {
        if (dep_stage_main >= 0) {
          // rows of the producer this tile's windows touch
          int r0 = INT32_MAX, r1 = -1;
          for (int m = tm * 64; m < std::min(g.M, tm * 64 + 64); ++m) {
            const int img = m / g.OHOW, rem = m % g.OHOW, oh = rem / g.OW, ow = rem % g.OW;
            const int ih0 = std::max(oh * g.stride - g.pad_t, 0), iw0 = std::max(ow * g.stride - g.pad_l, 0);
            const int ih1 = std::min(oh * g.stride - g.pad_t + (g.npos / g.KW) - 1, g.H - 1), iw1 = std::min(ow * g.stride - g.pad_l + g.KW - 1, g.W - 1);
            r0 = std::min(r0, (img * g.H + ih0) * g.W + iw0);
            r1 = std::max(r1, (img * g.H + ih1) * g.W + iw1);
          }
          rows_dep(dep_stage_main, r0, r1, d0f, d0n);
        }
        if (dep_stage_add >= 0) rows_dep(dep_stage_add, tm * 64, std::min(g.M, tm * 64 + 64) - 1, d1f, d1n);
      }
      if (d0n + d1n > 64) RADNET_FAIL(&ec, RADNET_ERR_UNSUPPORTED, "chain: an item would wait for %d blocks (64 at most)", d0n + d1n);
      for (int bz = 0; bz < (batch > 1 ? batch : 1); ++bz)
        for (int tn = 0; tn < Nt; ++tn)
          for (int s = 0; s < S; ++s) {
            ChainItem it{};
            it.stage = si;
            it.d0_first = d0f; it.d0_count = d0n; it.d1_first = d1f; it.d1_count = d1n;
            it.sig0 = o.first + tm; it.sig1 = -1;
            if (S > 1) {
              const int tile = tn * Mt + tm;
              const int u[8] = {tm, tn, s * kt, std::min(nk, (s + 1) * kt), tile * S + s, tile * S, S, tile};
              it.bx = (int)((units.size() - unit_base[si]) / 8);
              units.insert(units.end(), u, u + 8);
            } else {
              it.bx = tm; it.by = tn; it.bz = bz;
            }
            items.push_back(it);
          }
    }
    if (S > 1) g.counters = reinterpret_cast<unsigned*>((uintptr_t)split_counters);      // index for now, pointer once allocated
    return RADNET_OK;
  };

  // Every tensor is written ONCE per launch and never after it has been read (consumers use ordinary loads: a cache line is complete
  // before any workgroup touches it; the counters order a reader behind its producer -- RAW -- and nothing else).  A list that
  // re-uses a buffer (ping-pong activations, an output written twice, an output that an earlier op read) has WAR / WAW hazards the
  // counters do not cover: refused here, the caller keeps the launch list.
  std::set<const void*> touched;
  auto claim_output = [&](const void* p, int k, const char* what) -> int {
    if (p != nullptr && touched.count(p)) RADNET_FAIL(&ec, RADNET_ERR_UNSUPPORTED, "chain: op %d writes %s that an earlier op of the list reads or writes (buffer re-use inside a chain)", k, what);
    touched.insert(p);
    return RADNET_OK;
  };
  for (int k = 0; k < n_ops; ++k) {
    const radnet_op& op = ops[k];
    if (op.kind == RADNET_OP_NOP) continue;
    if (op.kind == RADNET_OP_CONV_FWD) {
      ChainStage st{};
      st.type = 0;
      int rc = chain_conv_args(&ec, &op.conv, st.g);
      if (rc != RADNET_OK) return rc;
      touched.insert(op.conv.x);
      if (op.conv.addend) touched.insert(op.conv.addend);
      rc = claim_output(op.conv.y, k, "its output");
      if (rc != RADNET_OK) return rc;
      const int si = push_stage(st, ChainOut{});
      auto pm = producer.find(op.conv.x), pa = op.conv.addend ? producer.find(op.conv.addend) : producer.end();
      rc = emit_gemm(si, 1, pm != producer.end() ? pm->second : -1, pa != producer.end() ? pa->second : -1, false);
      if (rc != RADNET_OK) return rc;
      producer[op.conv.y] = si;
      flops += 2.0 * stages[si].g.M * stages[si].g.N * stages[si].g.K;
      flops_alg += 2.0 * stages[si].g.M * stages[si].g.N * stages[si].g.K;
    } else if (op.kind == RADNET_OP_WINO && op.i[8] == 4) {
      const float* x = (const float*)op.p[0];
      float* V = (float*)op.p[1];
      const float* U = (const float*)op.p[2];
      float* Mw = (float*)op.p[3];
      touched.insert(x);
      for (int q : {1, 3, 6}) {
        const int rcq = claim_output(op.p[q], k, q == 1 ? "its transformed input" : q == 3 ? "its product buffer" : "its output");
        if (rcq != RADNET_OK) return rcq;
      }
      const int nb = op.i[0], h = op.i[1], w = op.i[2], c = op.i[3], n = op.i[4], T = op.i[5], act = op.i[6], ldy = op.i[7];
      const int th = (h + 3) / 4, tw = (w + 3) / 4;
      if (T != nb * th * tw || (c & 63) || (n & 63) || !(256 % c == 0 || c % 256 == 0) || !(256 % n == 0 || n % 256 == 0))
        RADNET_FAIL(&ec, RADNET_ERR_UNSUPPORTED, "chain: Winograd layer c=%d n=%d tiles=%d", c, n, T);
      if ((uint64_t)36 * T * std::max(c, n) * 4ull >= (1ull << 32) || (uint64_t)nb * h * w * ldy * 4ull >= (1ull << 32))
        RADNET_FAIL(&ec, RADNET_ERR_UNSUPPORTED, "chain: Winograd operand larger than 4 GiB");
      auto pm = producer.find(x);
      const int dep_x = pm != producer.end() ? pm->second : -1;
      // (1) input transform: blocks of 256 units (tile, 2 channels); counters per 64 tiles
      ChainStage s1{};
      s1.type = 1;
      s1.t_src = x; s1.t_dst = V; s1.t_nb = nb; s1.t_h = h; s1.t_w = w; s1.t_c = c; s1.t_th = th; s1.t_tw = tw;
      s1.t_dst_bytes = (unsigned)((uint64_t)36 * T * c * 4ull);
      ChainOut o1;
      o1.kind = ChainOut::TILES64;
      o1.count = radnet_cdiv(T, 64);
      const int cv = c;                          // units per tile: one per channel (chain_wino4_input)
      const int n_blk1 = radnet_cdiv((long long)T * cv, 256);
      const int si1 = push_stage(s1, o1);
      outs[si1].first = new_counters(o1.count, 0u);
      for (int b = 0; b < n_blk1; ++b) {
        const int t0 = (int)(((long long)b * 256) / cv), t1 = (int)(std::min<long long>((long long)b * 256 + 255, (long long)T * cv - 1) / cv);
        ChainItem it{};
        it.stage = si1; it.bx = b;
        if (dep_x >= 0) {
          int r0 = INT32_MAX, r1 = -1;
          for (int t = t0; t <= t1; ++t) {
            const int img = t / (th * tw), ti = (t / tw) % th, tj = t % tw;
            const int ih0 = std::max(4 * ti - 1, 0), ih1 = std::min(4 * ti + 4, h - 1), iw0 = std::max(4 * tj - 1, 0), iw1 = std::min(4 * tj + 4, w - 1);
            r0 = std::min(r0, (img * h + ih0) * w + iw0);
            r1 = std::max(r1, (img * h + ih1) * w + iw1);
          }
          rows_dep(dep_x, r0, r1, it.d0_first, it.d0_count);
          if (it.d0_count > 64) RADNET_FAIL(&ec, RADNET_ERR_UNSUPPORTED, "chain: a transform block would wait for %d blocks", it.d0_count);
        }
        it.sig0 = outs[si1].first + t0 / 64;
        it.sig1 = t1 / 64 != t0 / 64 ? outs[si1].first + t1 / 64 : -1;
        if (t1 / 64 > t0 / 64 + 1) RADNET_FAIL(&ec, RADNET_ERR_UNSUPPORTED, "chain: a transform block spans three tile blocks");
        need[(size_t)it.sig0] += 1u;
        if (it.sig1 >= 0) need[(size_t)it.sig1] += 1u;
        items.push_back(it);
      }
      // (2) 36 GEMMs [T x c] . [c x n] as one batched stage
      ChainStage s2{};
      s2.type = 0;
      GemmArgs& g = s2.g;
      g.x = V; g.w = U; g.y = Mw;
      g.H = 1; g.W = T; g.C = c; g.OH = 1; g.OW = T;
      g.KW = 1; g.npos = 1; g.stride = 1;
      g.M = T; g.N = n; g.K = c;
      g.ldw = n; g.ldy = n;
      g.OHOW = T;
      g.batch = 36;
      g.x_bstride = (long long)T * c; g.w_bstride = (long long)c * n; g.y_bstride = (long long)T * n;
      g.magic_ohow = radnet_div_magic((uint32_t)g.OHOW);
      g.magic_ow = radnet_div_magic((uint32_t)g.OW);
      g.x_bytes = (unsigned)((uint64_t)T * c * 4ull);
      g.w_bytes = (unsigned)((uint64_t)c * n * 4ull);
      g.y_bytes = (unsigned)(((uint64_t)(T - 1) * n + n) * 4ull);
      const int si2 = push_stage(s2, ChainOut{});
      int rc = emit_gemm(si2, 36, si1, -1, true);
      if (rc != RADNET_OK) return rc;
      // (3) output transform: counters per (image, tile row)
      ChainStage s3{};
      s3.type = 2;
      s3.t_src = Mw; s3.t_dst = (float*)op.p[6]; s3.t_scale = (const float*)op.p[4]; s3.t_shift = (const float*)op.p[5];
      s3.t_nb = nb; s3.t_h = h; s3.t_w = w; s3.t_c = n; s3.t_th = th; s3.t_tw = tw; s3.t_act = act; s3.t_ldy = ldy;
      s3.t_dst_bytes = (unsigned)((uint64_t)nb * h * w * ldy * 4ull);
      ChainOut o3;
      o3.kind = ChainOut::TILEROWS;
      o3.count = nb * th;
      o3.h = h; o3.w = w; o3.th = th; o3.tw = tw;
      const int si3 = push_stage(s3, o3);
      outs[si3].first = new_counters(o3.count, 0u);
      const int nv = n;
      const int n_blk3 = radnet_cdiv((long long)T * nv, 256);
      for (int b = 0; b < n_blk3; ++b) {
        const int t0 = (int)(((long long)b * 256) / nv), t1 = (int)(std::min<long long>((long long)b * 256 + 255, (long long)T * nv - 1) / nv);
        ChainItem it{};
        it.stage = si3; it.bx = b;
        it.d0_first = outs[si2].first + t0 / 64;
        it.d0_count = t1 / 64 - t0 / 64 + 1;
        const int row0 = t0 / tw, row1 = t1 / tw;         // (image * th + tile row)
        if (row1 > row0 + 1) RADNET_FAIL(&ec, RADNET_ERR_UNSUPPORTED, "chain: a transform block spans three tile rows");
        it.sig0 = outs[si3].first + row0;
        it.sig1 = row1 != row0 ? outs[si3].first + row1 : -1;
        need[(size_t)it.sig0] += 1u;
        if (it.sig1 >= 0) need[(size_t)it.sig1] += 1u;
        items.push_back(it);
      }
      producer[op.p[6]] = si3;
      flops += 2.0 * 36.0 * T * (double)n * c;
      flops_alg += 2.0 * nb * h * w * (double)n * 9.0 * c;
    } else {
      RADNET_FAIL(&ec, RADNET_ERR_UNSUPPORTED, "chain: op kind %d at position %d cannot run as chain items", op.kind, k);
    }
  }
  if (pl.items.empty()) RADNET_FAIL(&ec, RADNET_ERR_ARG, "chain: empty program");
  return RADNET_OK;
}

// In list order, with every earlier item finished, each item must find its input blocks complete: then a single workgroup
// can run the list, and any number of workgroups drawing from it in order cannot deadlock.  Also: every counter reaches
// exactly its `need`.  Returns the first offending item (or -1).
static int chain_first_unrunnable(const ChainPlan& pl, int* bad_counter) {
  std::vector<unsigned> c(pl.need.size(), 0u);
  for (size_t i = 0; i < pl.items.size(); ++i) {
    const ChainItem& it = pl.items[i];
    for (int k = 0; k < it.d0_count; ++k)
      if (c[(size_t)it.d0_first + k] < pl.need[(size_t)it.d0_first + k]) { *bad_counter = it.d0_first + k; return (int)i; }
    for (int k = 0; k < it.d1_count; ++k)
      if (c[(size_t)it.d1_first + k] < pl.need[(size_t)it.d1_first + k]) { *bad_counter = it.d1_first + k; return (int)i; }
    if (it.sig0 >= 0) c[(size_t)it.sig0] += 1u;
    if (it.sig1 >= 0) c[(size_t)it.sig1] += 1u;
  }
  for (size_t k = 0; k < c.size(); ++k)
    if (pl.need[k] != 0u && c[k] != pl.need[k]) { *bad_counter = (int)k; return (int)pl.items.size(); }
  return -1;
}

extern "C" int radnet_chain_check(const radnet_op* ops, int32_t n_ops, int32_t* n_items, int32_t* n_stages, int32_t* n_counters, int32_t* first_bad_item,
                                  int32_t* bad_counter, char* err, int32_t err_len) {
  if (!ops || n_ops <= 0) return RADNET_ERR_ARG;
  ChainPlan pl;
  ErrSink ec{};
  const int rc = chain_plan(ops, n_ops, pl, ec);
  if (err && err_len > 0) snprintf(err, (size_t)err_len, "%s", ec.err);
  if (rc != RADNET_OK) return rc;
  int bc = -1;
  const int bad = chain_first_unrunnable(pl, &bc);
  if (n_items) *n_items = (int32_t)pl.items.size();
  if (n_stages) *n_stages = (int32_t)pl.stages.size();
  if (n_counters) *n_counters = (int32_t)pl.need.size();
  if (first_bad_item) *first_bad_item = bad;
  if (bad_counter) *bad_counter = bc;
  return RADNET_OK;
}

int radnet_chain_plan(const radnet_op* ops, int32_t n_ops, ChainPlan& pl, ErrSink& ec) {
  const int rc = chain_plan(ops, n_ops, pl, ec);
  if (rc != RADNET_OK) return rc;
  int bc = -1;
  const int bad = chain_first_unrunnable(pl, &bc);
  if (bad >= 0) RADNET_FAIL(&ec, RADNET_ERR_UNSUPPORTED, "chain: item %d of %d cannot run in list order (counter %d)", bad, (int)pl.items.size(), bc);
  return RADNET_OK;
}
