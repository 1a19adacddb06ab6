// Grey levels <-> float32 in [0, 1]: the two conversions every kernel that reads or writes integer images shares (io.hip: the
// pages of prediction; data.hip / resize.hip: the resident 16-bit tiles of training and evaluation).
#pragma once
#include "common.h"

// np.float32(min(v, in_max) / float(in_max)): the quotient in double, rounded once more to float32 (util.uint2single /
// uint162single, dlib/utils/utils_image.py:322-331, with a white level).  dmax = (double)in_max.
static __device__ __forceinline__ float unit_of(unsigned v, unsigned in_max, double dmax) {
  return (float)((double)min(v, in_max) / dmax);
}

// round_half_even(clamp(x, 0, 1) * out_max) (util.tensor2uint / single2uint16 / tensor2uint82float, utils_image.py:334-335,
// 362-372): fmaxf / fminf drop a NaN operand, so NaN -> 0, -inf -> 0, +inf -> out_max; ONE float32 product (there is nothing it
// could be contracted with); v_rndne_f32 rounds half to even; the result is an integer in [0, 65535], exact in float32.
static __device__ __forceinline__ unsigned level_of(float x, float out_max) {
  return (unsigned)rintf(__fmul_rn(fminf(fmaxf(x, 0.f), 1.f), out_max));
}

// A pixel of the metrics at L levels (small.hip, ssim.hip: --metric_levels): its level at L, and the 8-bit level the ROI is
// thresholded at.  A float image is quantised by either white level directly; a level v of an image that holds levels goes
// back through np.float32(v / L) (unit_of), so both forms of one image give one ROI.
static __device__ __forceinline__ float metric_level(float v, int is_levels, float fL) {
  return is_levels ? v : (float)level_of(v, fL);
}
static __device__ __forceinline__ float metric_level8(float v, int is_levels, unsigned L) {
  return (float)level_of(is_levels ? unit_of((unsigned)fminf(fmaxf(v, 0.f), (float)L), L, (double)L) : v, 255.f);
}
