// nn.Dropout on the tape (ACT's seven dropouts per fusion block, network_act.py:136-204): masks from a counter-based
// generator, Philox4x32-10 (Salmon et al., SC'11), so that a mask is a pure function of (seed, site, element index) --
// the backward regenerates it with the same launch on the gradient and nothing is stored; a batch slice passes its element
// offset and sees the mask of the whole tensor.  The seed is read from device memory: a launch captured in a hipGraph
// replays with whatever the seed tensor holds then.
#include "common.h"
#include "philox.h"
#include <math.h>

namespace {

// One Philox call per group of four consecutive elements; a thread walks groups q, q + stride, ...  `vec`: x and out are
// 16-byte aligned, so a whole group is one 16-byte load and one 16-byte store.  The last group may hold 1 .. 3 elements.
template <bool VEC>
__global__ __launch_bounds__(256) void k_dropout(const float* x, float* out, long n, long group0, const long long* seed,
                                                 unsigned site, unsigned thr, float scale) {
  // (no __restrict__: out may be x -- every element is read by the thread that writes it, before it writes)
  const unsigned long long s = (unsigned long long)*seed;
  const unsigned k0 = (unsigned)s, k1 = (unsigned)(s >> 32);
  const long ngroups = (n + 3) >> 2;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < ngroups; q += stride) {
    const unsigned long long g = (unsigned long long)(group0 + q);
    const uint4 w = philox4x32_10((unsigned)g, (unsigned)(g >> 32), site, k0, k1);
    const long i = q << 2;
    if (VEC && i + 4 <= n) {
      const f32x4 v = *(const f32x4*)(x + i);
      f32x4 o;
      o.x = w.x >= thr ? v.x * scale : 0.f;
      o.y = w.y >= thr ? v.y * scale : 0.f;
      o.z = w.z >= thr ? v.z * scale : 0.f;
      o.w = w.w >= thr ? v.w * scale : 0.f;
      *(f32x4*)(out + i) = o;
    } else {
      const unsigned ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i + j < n) out[i + j] = ww[j] >= thr ? x[i + j] * scale : 0.f;
    }
  }
}

}  // namespace

extern "C" {

/* out[i] = keep(offset + i) ? x[i] * scale : 0 (include/srhip.h).  out may be x. */
int srhip_dropout(const float* x, float* out, long n, long offset, const long long* seed, int site, unsigned int thr,
                  float scale, void* stream) {
  SR_REQUIRE(x && out && seed && n > 0, "dropout: bad operand");
  SR_REQUIRE(offset >= 0 && offset % 4 == 0, "dropout: offset must be a non-negative multiple of 4 (got %ld)", offset);
  SR_REQUIRE(site >= 0, "dropout: site >= 0 (got %d)", site);
  // scale = 1 / (1 - p): p >= 1 arrives as an infinite (or negative, or NaN) scale, p < 0 as one below 1
  SR_REQUIRE(isfinite(scale) && scale >= 1.0f, "dropout: 0 <= p < 1, that is a finite scale = 1 / (1 - p) >= 1 (got %g)",
             (double)scale);
  SR_REQUIRE(out == x || sr_disjoint(x, n * 4, out, n * 4), "dropout: out is x or does not overlap it");
  const long ngroups = (n + 3) >> 2;
  const long gb = (ngroups + 255) / 256;
  const int grid = (int)(gb < 8192 ? gb : 8192);
  const bool vec = (((uintptr_t)x | (uintptr_t)out) & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(k_dropout<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, out, n, offset >> 2, seed,
                       (unsigned)site, thr, scale);
  else
    hipLaunchKernelGGL(k_dropout<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, out, n, offset >> 2, seed,
                       (unsigned)site, thr, scale);
  SR_LAUNCH_CHECK("dropout");
  return 0;
}

}  // extern "C"
