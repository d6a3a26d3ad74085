// Pixel-centre arithmetic shared by the point-splat renderer (f3r_render.hip) and the triangle rasteriser (f3r_raster.hip): both decide
// which pixel centres i + 0.5 a window-space interval holds, and both must give the comparison's own answer.
#pragma once

#include "f3r_common.h"

// the smallest integer i with i + 0.5 >= t, clamped to [0, hi].  i + 0.5 is exact for every i the clamp leaves; the two corrections make
// the result the comparison's own answer whatever ceil(t - 0.5) rounded to
__device__ __forceinline__ int first_center_ge(double t, int hi) {
  if (!(t > 0.5)) return 0;  // pixel 0's centre is already >= t
  if (t > (double)hi) return hi;
  double i = ceil(t - 0.5);
  if ((i - 1.0) + 0.5 >= t) i -= 1.0;
  if (i + 0.5 < t) i += 1.0;
  return (int)fmin(fmax(i, 0.0), (double)hi);
}
