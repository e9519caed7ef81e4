// The suppression test of the greedy NMS kernels (proposals.hip: nms_kernel; detect_tail.hip: the per-class NMS of a tile;
// scan_tail.hip: the NMS across the images of a scan): one body, so that the three cannot drift apart.  Units that include it
// are compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

// rpn.py:429-447 with i = the picked box
__device__ __forceinline__ bool suppresses(const double4& pk, double pk_area, const double4& c, double c_area, double thr) {
  const double ww = fmax(0.0, fmin(pk.z, c.z) - fmax(pk.x, c.x));
  const double hh = fmax(0.0, fmin(pk.w, c.w) - fmax(pk.y, c.y));
  const double inter = ww * hh;
  const double uni = pk_area + c_area - inter;
  const double d = uni + 1e-6;
  // The reference compares the ROUNDED quotient with thr.  An fp64 division is a ~40-instruction sequence here and
  // this test runs picks x candidates times, so decide without it whenever the outcome cannot depend on rounding:
  // with d > 0, thr > 0 and |inter - thr*d| beyond a 2^-40 relative margin (the products and the quotient each
  // carry < 2^-52), fl(inter/d) > thr  <=>  inter > thr*d.  Everything inside the margin takes the division.
  if (d > 0.0 && thr > 0.0) {
    const double t = thr * d;
    if (inter > t * (1.0 + 0x1p-40)) return true;
    if (inter < t * (1.0 - 0x1p-40)) return false;
  }
  return inter / d > thr;
}
