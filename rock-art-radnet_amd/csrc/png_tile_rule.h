// The tile rule of radnet_png_unfilter_tiles_u8 (include/radnet_hip.h states it in words), once: the planner (png_plan.cpp, g++),
// the launch code and the kernel (png_tiles.hip) all read it from here.  No HIP header; integers only.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RADNET_TILE_HD __host__ __device__ __forceinline__
#else
#define RADNET_TILE_HD inline
#endif

struct png_tile_grid {
  int32_t bands, blocks, sweeps;
};

// rows >= 1, 1 <= pixels <= 2^30, 64 <= tile_pixels: bands of 64 rows, skewed blocks of tile_pixels pixels (lane l of block c
// starts at pixel c * tile_pixels - l, so the last block must still reach pixel `pixels - 1` of lane 63)
RADNET_TILE_HD png_tile_grid png_tile_grid_of(int32_t rows, int32_t pixels, int32_t tile_pixels) {
  png_tile_grid g;
  g.bands = (rows - 1) / 64 + 1;
  g.blocks = (pixels + 63 + tile_pixels - 1) / tile_pixels;
  g.sweeps = g.blocks + 2 * (g.bands - 1);
  return g;
}

// the number of tiles on sweep d (0 <= d < sweeps) and *lo, the band of the first: tile i is band lo + i, block d - 2 * (lo + i).
// At least one, but for a segment of one block, whose tiles stand on the even sweeps alone.
RADNET_TILE_HD int32_t png_tiles_on_sweep(const png_tile_grid& g, int32_t d, int32_t* lo) {
  const int32_t first = d >= g.blocks ? (d - g.blocks + 2) / 2 : 0;      // ceil((d - (blocks - 1)) / 2): the block index stays below blocks
  const int32_t last = d / 2 < g.bands - 1 ? d / 2 : g.bands - 1;       // the block index stays at 0 or above
  *lo = first;
  return last - first + 1;
}
