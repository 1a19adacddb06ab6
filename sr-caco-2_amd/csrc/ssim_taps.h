// The normalised 1-D Gaussian taps (sigma 1.5) of the SSIM windows, made on the host and passed to the kernels by value: one
// definition for ssim.hip (loss and metrics) and msssim.hip, so that every metric kernel filters with the same floats.
#pragma once
#include <math.h>

constexpr int MAXWS = 19;     // largest window (README recipe uses 19)

struct Taps { float g[MAXWS]; };

static inline Taps gaussian_taps(int ws, bool centered_half) {
  // loss: exp(-(i - ws//2)^2 / (2 sigma^2)) (ssim.py:23-27);
  // metric: coords - (ks-1)/2 (utils_image.py:1102-1117) -- identical for odd ws
  Taps t;
  float g[MAXWS];
  float s = 0.f;
  for (int i = 0; i < ws; ++i) {
    const float d = centered_half ? (float)i - (float)(ws - 1) / 2.0f : (float)(i - ws / 2);
    g[i] = expf(-(d * d) / (2.0f * 1.5f * 1.5f));
    s += g[i];
  }
  for (int i = 0; i < MAXWS; ++i) t.g[i] = i < ws ? g[i] / s : 0.f;
  return t;
}
