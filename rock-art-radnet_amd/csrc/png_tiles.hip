// PNG scanline reconstruction by tiles (radnet_png_unfilter_tiles_u8; the contract and the tile rule: include/radnet_hip.h,
// png_tile_rule.h).  png.hip walks a pass with ONE workgroup, because Up / Average / Paeth rows allow no cut; here the wave lag of
// that walk is lifted to the grid.  A segment is cut into bands of 64 rows and skewed column blocks of T pixels; tile (b, c) needs
// only tiles of the sweeps before d = c + 2 * b, so one plain launch per sweep, in stream order, is the whole dependency: no
// workgroup ever waits on another, no flag, no counter, every loop bound a function of the arguments.
// One wave does one tile (a workgroup is one wave: no __syncthreads, the LDS tile is the wave's own).  Lane l owns row b * 64 + l,
// one pixel behind the row above, `b` by the DPP wave shift, `c` = last step's `b` (png_predict.h), exactly as in png.hip.  The
// tile moves through LDS in chunks of kChunkPixels pixels per row, consecutive lanes on consecutive bytes of a row; the loads of
// the next chunk are in flight (in registers) while the wave computes this one -- a tile's input bytes are written by nobody
// else in its sweep.  A lane's piece leaves LDS as dwords and the unrolled steps run on registers.  Every store is a byte store to a byte the tile owns: two tiles of one sweep own neighbouring bytes of one dword.
// Integer arithmetic only; compiled with -ffp-contract=off like png.hip.
#include "radnet_internal.h"
#include "png_predict.h"
#include "png_tile_rule.h"

namespace {

static_assert(RADNET_PNG_TILE_ROWS == 64, "a band is one wave, one lane per row");
static_assert(RADNET_PNG_TILE_PIXELS >= 64 && RADNET_PNG_TILE_PIXELS % 32 == 0, "the row above a tile lies in two tiles of earlier sweeps; whole chunks");

// what one lane's LDS writes of a phase are to the other lanes' reads of the next: the wave runs in lockstep and its LDS
// instructions complete in order, so the compiler must only keep them in order
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

constexpr int gcd_of(int a, int b) { return b == 0 ? a : gcd_of(b, a % b); }

template <int BPP>
struct TileShape {
  static constexpr int kChunkPixels = BPP <= 4 ? 32 : 16;
  static constexpr int kChunkBytes = kChunkPixels * BPP;                  // 32, 64, 96, 128, 96, 128
  static constexpr int kStride = kChunkBytes + 4;                         // an odd number of dwords: a column of 64 rows hits 64 banks
  // Byte u * 64 + lane of the 64 row pieces of a chunk (u < kChunkBytes: 64 * kChunkBytes bytes, consecutive lanes on consecutive
  // bytes of a piece) repeats with a period of kPeriodSlots slots that cover kPeriodRows whole pieces: 1 / 2, 1 / 1, 3 / 2, 2 / 1
  static constexpr int kPeriodSlots = kChunkBytes / gcd_of(kChunkBytes, 64), kPeriodRows = 64 / gcd_of(kChunkBytes, 64);
  static constexpr int kAboveLoads = (kChunkBytes + 63) / 64;             // slots of the piece of the row above the band
  static constexpr int kLoads = kChunkBytes + kAboveLoads;
  static_assert(kChunkBytes % 8 == 0 && (kStride / 4) % 2 == 1, "bank-conflict-free stride");
  static_assert(kChunkBytes % kPeriodSlots == 0 && kPeriodRows <= 2, "whole periods; a slot touches at most two pieces");
};

// What a lane keeps for slot t of a period, the same in every period, chunk and tile: the piece (0 or 1) and the byte of it that it
// moves, and from them its offsets in the stream (pieces of neighbouring rows stand pitch - BPP bytes apart: each starts one pixel
// to the left of the one above), in the row and in the LDS tile.
template <int BPP>
struct Slots {
  using S = TileShape<BPP>;
  int piece[S::kPeriodSlots], row_pos[S::kPeriodSlots], lds_at[S::kPeriodSlots];
  unsigned stream_at[S::kPeriodSlots];             // below 2^31: one pitch at most
  __device__ __forceinline__ Slots(int lane, int rowbytes) {
#pragma unroll
    for (int t = 0; t < S::kPeriodSlots; ++t) {
      const int idx = t * 64 + lane, dj = idx / S::kChunkBytes, i = idx - dj * S::kChunkBytes;
      piece[t] = dj;
      row_pos[t] = i - dj * BPP;
      lds_at[t] = dj * S::kStride + i;
      stream_at[t] = (unsigned)(dj * (1 + rowbytes - BPP) + i);
    }
  }
};

// One chunk of a tile: lane 0's first pixel is ps0, the piece of the band's row j starts j pixels to the left of it.
template <int BPP>
struct Chunk {
  using S = TileShape<BPP>;
  uint8_t* row0;             // byte 0 of row 0's piece
  long long step;            // from a piece to the one below
  int rows_left, byte0, rowbytes;      // rows of the segment from the band's first on; of row 0's piece in its row

  __device__ __forceinline__ Chunk(uint8_t* stream, int rows, int rowbytes_, int wave_r0, int ps0)
      : row0(stream + (wave_r0 * (1 + (long long)rowbytes_) + 1 + (long long)ps0 * BPP)), step((long long)rowbytes_ + 1 - BPP), rows_left(rows - wave_r0),
        byte0(ps0 * BPP), rowbytes(rowbytes_) {}
  // the address of slot u's byte, or null where the piece leaves the segment: such a byte counts as 0 and is never stored
  __device__ __forceinline__ uint8_t* row_byte(const Slots<BPP>& sl, int u) const {
    const int m = u / S::kPeriodSlots, t = u - m * S::kPeriodSlots;       // constants once unrolled
    const int pos = (byte0 - m * S::kPeriodRows * BPP) + sl.row_pos[t];
    const bool ok = m * S::kPeriodRows + sl.piece[t] < rows_left && (unsigned)pos < (unsigned)rowbytes;
    return ok ? (row0 + m * S::kPeriodRows * step) + sl.stream_at[t] : nullptr;
  }
  // slot v of the piece of the row above the band, at lane 0's pixels; null above row 0 and outside the row
  __device__ __forceinline__ const uint8_t* above_byte(int v, int lane, bool has_above) const {
    const int i = v * 64 + lane, pos = byte0 + i;
    return (has_above && i < S::kChunkBytes && (unsigned)pos < (unsigned)rowbytes) ? row0 - (step + BPP) + i : nullptr;
  }
  __device__ __forceinline__ void load(const Slots<BPP>& sl, uint8_t (&regs)[S::kLoads], int lane, bool has_above) const {
#pragma unroll
    for (int u = 0; u < S::kChunkBytes; ++u) {
      const uint8_t* at = row_byte(sl, u);
      regs[u] = at ? *at : (uint8_t)0;
    }
#pragma unroll
    for (int v = 0; v < S::kAboveLoads; ++v) {
      const uint8_t* at = above_byte(v, lane, has_above);
      regs[S::kChunkBytes + v] = at ? *at : (uint8_t)0;
    }
  }
};

template <int BPP>
__global__ void __launch_bounds__(64) png_unfilter_tiles_kernel(uint8_t* base, const radnet_png_segment* __restrict__ segs, int first, int sweep,
                                                                int tile_pixels) {
  using S = TileShape<BPP>;
  __shared__ __attribute__((aligned(16))) uint8_t lds[65 * S::kStride];
  const radnet_png_segment seg = segs[first + (int)blockIdx.y];
  const int rows = seg.rows, rowbytes = seg.rowbytes, P = rowbytes / BPP;
  const png_tile_grid g = png_tile_grid_of(rows, P, tile_pixels);
  if (sweep >= g.sweeps) return;
  int lo;
  const int on_sweep = png_tiles_on_sweep(g, sweep, &lo);
  if ((int)blockIdx.x >= on_sweep) return;
  const int band = lo + (int)blockIdx.x, block = sweep - 2 * band;

  uint8_t* stream = base + seg.offset;
  const long long pitch = 1 + (long long)rowbytes;
  const int lane = threadIdx.x;
  const int wave_r0 = band * 64, r = wave_r0 + lane;
  const bool valid = r < rows, has_above = band > 0;
  const int ft = valid ? stream[r * pitch] : 0;

  // the state in front of the tile: a = this row's pixel to the left of the lane's first, c = the same pixel of the row above;
  // both were written by tile (band, block - 1), or for lane 0's c by tile (band - 1, block), on earlier sweeps
  int a[BPP], bprev[BPP];
  {
    const int q = block * tile_pixels - lane - 1;
    const bool left = valid && q >= 0 && q < P;
    const long long at = r * pitch + 1 + (long long)q * BPP;
#pragma unroll
    for (int j = 0; j < BPP; ++j) {
      a[j] = left ? stream[at + j] : 0;
      bprev[j] = (left && r > 0) ? stream[at - pitch + j] : 0;
    }
  }

  const Slots<BPP> sl(lane, rowbytes);
  const int n_chunks = tile_pixels / S::kChunkPixels;
  uint8_t next[S::kLoads];
  Chunk<BPP>(stream, rows, rowbytes, wave_r0, block * tile_pixels).load(sl, next, lane, has_above);
  for (int k = 0; k < n_chunks; ++k) {
    const int ps0 = block * tile_pixels + k * S::kChunkPixels;          // lane 0's first pixel of this chunk; lane l's is ps0 - l
    if (ps0 - 63 >= P) break;                                          // uniform: the rest of the tile lies to the right of every row
#pragma unroll
    for (int u = 0; u < S::kChunkBytes; ++u) {
      const int m = u / S::kPeriodSlots, t = u - m * S::kPeriodSlots;
      lds[m * S::kPeriodRows * S::kStride + sl.lds_at[t]] = next[u];
    }
#pragma unroll
    for (int v = 0; v < S::kAboveLoads; ++v)
      if (v * 64 + lane < S::kChunkBytes) lds[64 * S::kStride + v * 64 + lane] = next[S::kChunkBytes + v];
    wave_sync();
    if (k + 1 < n_chunks) Chunk<BPP>(stream, rows, rowbytes, wave_r0, ps0 + S::kChunkPixels).load(sl, next, lane, has_above);
    {
      // the lane's piece and the piece of the row above leave LDS as dwords and the steps run on registers (the loop is unrolled, so
      // every byte is a constant bit field of a register): a step then waits for the step before it and for nothing else
      uint32_t* mine = reinterpret_cast<uint32_t*>(lds + lane * S::kStride);
      const uint32_t* above = reinterpret_cast<const uint32_t*>(lds + 64 * S::kStride);
      uint32_t piece[S::kChunkBytes / 4], up[S::kChunkBytes / 4], done[S::kChunkBytes / 4];
#pragma unroll
      for (int q = 0; q < S::kChunkBytes / 4; ++q) {
        piece[q] = mine[q];
        up[q] = above[q];
        done[q] = 0;
      }
#pragma unroll
      for (int s = 0; s < S::kChunkPixels; ++s) {
        const int p = ps0 - lane + s;
        const bool on = valid && p >= 0 && p < P;
        int b[BPP];
#pragma unroll
        for (int j = 0; j < BPP; ++j) b[j] = from_lane_above(a[j]);
#pragma unroll
        for (int j = 0; j < BPP; ++j) {
          const int at = s * BPP + j, shift = 8 * (at & 3);
          const int x = (piece[at >> 2] >> shift) & 255;
          if (lane == 0) b[j] = (up[at >> 2] >> shift) & 255;
          const int out = (x + predictor(ft, a[j], b[j], bprev[j])) & 255;
          done[at >> 2] |= (uint32_t)(on ? out : x) << shift;
          a[j] = on ? out : 0;                     // left of the row and outside the image count as 0
          bprev[j] = b[j];
        }
      }
#pragma unroll
      for (int q = 0; q < S::kChunkBytes / 4; ++q) mine[q] = done[q];
    }
    wave_sync();
    const Chunk<BPP> chunk(stream, rows, rowbytes, wave_r0, ps0);
#pragma unroll
    for (int u = 0; u < S::kChunkBytes; ++u) {
      const int m = u / S::kPeriodSlots, t = u - m * S::kPeriodSlots;
      uint8_t* at = chunk.row_byte(sl, u);
      if (at) *at = lds[m * S::kPeriodRows * S::kStride + sl.lds_at[t]];      // exactly the bytes this tile owns
    }
    wave_sync();                                   // the next chunk overwrites the LDS tile
  }
}

template <int BPP>
void launch_sweep(radnet_ctx* ctx, uint8_t* base, const radnet_png_segment* segs, int first, int n, int sweep, int most, int tile_pixels) {
  hipLaunchKernelGGL(png_unfilter_tiles_kernel<BPP>, dim3((unsigned)most, (unsigned)n), dim3(64), 0, ctx->stream, base, segs, first, sweep, tile_pixels);
}

constexpr int kMaxGridY = 65535;

}  // namespace

extern "C" int radnet_png_unfilter_tiles_width_u8(radnet_ctx* ctx, uint8_t* base, int64_t base_len, const radnet_png_segment* segs_host,
                                                  const radnet_png_segment* segs_dev, int32_t count, int32_t bpp, int32_t tile_pixels) {
  if (!ctx) return RADNET_ERR_ARG;
  if (count < 0) RADNET_FAIL(ctx, RADNET_ERR_ARG, "png_unfilter_tiles: %d segments", count);
  if (count == 0) return RADNET_OK;
  if (!base || !segs_host || !segs_dev || base_len <= 0)
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "png_unfilter_tiles: null buffer or table (base %p of %lld bytes, host table %p, device table %p)", (void*)base,
                (long long)base_len, (const void*)segs_host, (const void*)segs_dev);
  if (!(bpp == 1 || bpp == 2 || bpp == 3 || bpp == 4 || bpp == 6 || bpp == 8)) RADNET_FAIL(ctx, RADNET_ERR_ARG, "png_unfilter_tiles: %d bytes per pixel", bpp);
  if (tile_pixels < 64 || tile_pixels > 4096 || tile_pixels % 32 != 0)
    RADNET_FAIL(ctx, RADNET_ERR_ARG, "png_unfilter_tiles: blocks of %d pixels (a multiple of 32 from 64 to 4096)", tile_pixels);
  int max_sweeps = 0;
  for (int i = 0; i < count; ++i) {
    const radnet_png_segment& s = segs_host[i];
    if (s.rows <= 0 || s.rowbytes <= 0 || s.rowbytes % bpp != 0)
      RADNET_FAIL(ctx, RADNET_ERR_ARG, "png_unfilter_tiles: segment %d has %d rows of %d bytes at %d bytes per pixel", i, s.rows, s.rowbytes, bpp);
    if (s.rowbytes > (1 << 30)) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "png_unfilter_tiles: segment %d has %d bytes per row", i, s.rowbytes);
    const int64_t bytes = (int64_t)s.rows * (1 + (int64_t)s.rowbytes);       // below 2^62
    if (s.offset < 0 || s.offset > base_len || bytes > base_len - s.offset)
      RADNET_FAIL(ctx, RADNET_ERR_ARG, "png_unfilter_tiles: segment %d (%lld bytes at offset %lld) leaves the buffer of %lld bytes", i, (long long)bytes,
                  (long long)s.offset, (long long)base_len);
    const int sweeps = png_tile_grid_of(s.rows, s.rowbytes / bpp, tile_pixels).sweeps;
    max_sweeps = sweeps > max_sweeps ? sweeps : max_sweeps;
  }
  for (int first = 0; first < count; first += kMaxGridY) {
    const int n = count - first < kMaxGridY ? count - first : kMaxGridY;
    for (int d = 0; d < max_sweeps; ++d) {
      int most = 0;
      for (int i = first; i < first + n; ++i) {
        const png_tile_grid g = png_tile_grid_of(segs_host[i].rows, segs_host[i].rowbytes / bpp, tile_pixels);
        int lo;
        const int here = d < g.sweeps ? png_tiles_on_sweep(g, d, &lo) : 0;
        most = here > most ? here : most;
      }
      if (most == 0) continue;                     // no segment of this slice reaches sweep d
      switch (bpp) {
        case 1: launch_sweep<1>(ctx, base, segs_dev, first, n, d, most, tile_pixels); break;
        case 2: launch_sweep<2>(ctx, base, segs_dev, first, n, d, most, tile_pixels); break;
        case 3: launch_sweep<3>(ctx, base, segs_dev, first, n, d, most, tile_pixels); break;
        case 4: launch_sweep<4>(ctx, base, segs_dev, first, n, d, most, tile_pixels); break;
        case 6: launch_sweep<6>(ctx, base, segs_dev, first, n, d, most, tile_pixels); break;
        default: launch_sweep<8>(ctx, base, segs_dev, first, n, d, most, tile_pixels); break;
      }
      RADNET_CHECK_LAUNCH(ctx, "png_unfilter_tiles_u8");
    }
  }
  return RADNET_OK;
}

extern "C" int radnet_png_unfilter_tiles_u8(radnet_ctx* ctx, uint8_t* base, int64_t base_len, const radnet_png_segment* segs_host,
                                            const radnet_png_segment* segs_dev, int32_t count, int32_t bpp) {
  return radnet_png_unfilter_tiles_width_u8(ctx, base, base_len, segs_host, segs_dev, count, bpp, RADNET_PNG_TILE_PIXELS);
}
