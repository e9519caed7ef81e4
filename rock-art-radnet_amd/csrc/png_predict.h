// What the PNG reconstruction kernels share (png.hip: one workgroup per pass or segment; png_tiles.hip: one wave per tile) and the
// forward filter reads too: the predictor of a filter type and the move of a value to the lane below.
#pragma once

namespace {

// lane l receives lane l - 1's value (DPP wave_shr:1); lane 0 receives 0
__device__ __forceinline__ int from_lane_above(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x138, 0xf, 0xf, false); }

// Recon(x) - x for one byte: the predictor of filter type ft (0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth)
__device__ __forceinline__ int predictor(int ft, int a, int b, int c) {
  const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
  const int paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
  int p = 0;
  p = ft == 1 ? a : p;
  p = ft == 2 ? b : p;
  p = ft == 3 ? ((a + b) >> 1) : p;
  p = ft == 4 ? paeth : p;
  return p;
}

}  // namespace
