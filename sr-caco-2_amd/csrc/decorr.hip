// Image decorrelation analysis at L levels, float64 (predict.py --resolution; Descloux, Grussmayer, Radenovic 2019): one
// resolution figure per image, with no second image and no target.  Not a reference call: the definition is the one of
// include/srhip.h (srhip_metrics_decorr_lv).
//
// Three launches.  Images are real, so TWO images of the batch cost ONE complex transform: z = win x_a + i win x_b, and with
// A = Z(k), B = conj Z(-k) the two spectra are Fa = (A + B) / 2, Fb = (A - B) / (2i); B images take ceil(B / 2) transforms, an odd
// tail runs with a zero partner.
//   k_dc_rows   as k_frc_rows: a block quantises, windows and packs 4 rows of both images into LDS, transforms them and writes
//               them TRANSPOSED into the workspace, T[pair][p][y], in 64-byte runs.
//   k_dc_cols   block kx (0 .. S/2) loads column kx and its mirror, transforms both and takes the ring sums of column kx: one
//               thread per ring r >= 2 walks that ring's ky in ascending order and adds |Fa|, |Fa|^2, |Fb|, |Fb|^2 and counts the
//               frequencies.  Column -kx holds the conjugates, the same magnitudes on the same rings, so its share is the factor 2.
//               part[pair][q][kx][r], r >= max(kx, 2); plane 4 is the count, a 64-bit integer.
//   k_dc_fin    one block per image, 10 waves.  Thread r adds part[.][.][0 .. r][r] in ascending kx; wave 0 forms curve 0 and
//               finds its peak; then every wave forms one curve of bank 1 and finds its peak, and then one of bank 2.
// Nothing is accumulated with atomics, in LDS or in memory: two calls give the same bits.
//
// A curve in one wave: lane l owns the c = ceil((S/2 - 1) / 64) <= 16 consecutive rings from 2 + l c.  The running numerator is
// the lane's own sum behind a shuffle scan of the lanes' totals.  The peak search of the header walks m down from S/2 and takes
// the first argmax i of d[2 .. m] each time, which is quadratic as stated; here it is one pass.  i is always a strict record of
// the running maximum, and record i is the argmax exactly for m in [i, j - 1], j the next record (or S/2 + 1).  Within that range
// min(d[i .. m]) only grows as m falls, so the test d[i] - min >= 5e-4 holds somewhere in it iff it holds at m = j - 1, and the
// search stops at the HIGHEST record i > 2 with j - 1 > i whose segment [i, j - 1] passes.  A lane marks the records of its rings
// (a bit each) from the shuffle-scanned maximum before them, takes the minimum of its rings in front of its first record, gets
// from the lanes above it the minimum and length of the part of its last segment that they hold (63 shuffles), and walks its
// rings downwards once.  No lane reads what another lane wrote to LDS.
#include "common.h"
#include "levels.h"
#include "fft_lds.h"

namespace {

constexpr int NCURVE = 21, NBANK = 10, FIN_WAVES = 10;
constexpr double PEAK_DROP = 5e-4, SIGMA_MIN = 0.15;
constexpr double PI2 = 9.869604401089358;     // pi^2, the double next to it

// grid (S / ROWS, ceil(B / 2)).  T[pair][p][y] = the row transform of row y of z = win x_a + i win x_b at position p
__global__ void __launch_bounds__(1024) k_dc_rows(const float* __restrict__ img, double2* __restrict__ T, int B, int H, int W,
                                                  int lg, int L, int in_is_lv) {
  extern __shared__ double2 dc_sm[];
  const int S = 1 << lg, rs = S + RPAD;
  double2* const tw = dc_sm;                  // [S / 2]
  double2* const x = dc_sm + (S >> 1);        // [ROWS][rs]
  const int pr = blockIdx.y, y0 = blockIdx.x * ROWS;
  const int oy = (H - S) / 2, ox = (W - S) / 2;
  const float fL = (float)L;
  const double dL = (double)L;
  const float* const ia = img + (long)(2 * pr) * H * W;
  const bool two = 2 * pr + 1 < B;            // the odd tail has a zero partner
  const float* const ib = ia + (two ? (long)H * W : 0);
  make_twiddles(tw, lg);
  __syncthreads();
  for (int i = threadIdx.x; i < ROWS * S; i += blockDim.x) {
    const int r = i >> lg, c = i & (S - 1);
    const long o = ((long)oy + y0 + r) * W + ox + c;
    const double win = hann(tw, y0 + r, lg) * hann(tw, c, lg);
    x[r * rs + c] = make_double2(win * ((double)metric_level(ia[o], in_is_lv, fL) / dL),
                                 two ? win * ((double)metric_level(ib[o], in_is_lv, fL) / dL) : 0.0);
  }
  __syncthreads();
  fft_rows(x, tw, ROWS, rs, lg);
  for (int i = threadIdx.x; i < ROWS * S; i += blockDim.x) {
    const int r = i & (ROWS - 1), p = i >> 2;
    T[((long)pr * S + p) * S + y0 + r] = x[r * rs + p];
  }
}

// grid (S / 2 + 1, ceil(B / 2)).  part[pair][q][kx][r], q = 0: sum |Fa|, 1: sum |Fa|^2, 2: sum |Fb|, 3: sum |Fb|^2, 4: the number
// of frequencies (long long), over ring r >= 2 of columns +-kx
__global__ void __launch_bounds__(1024) k_dc_cols(const double2* __restrict__ T, double* __restrict__ part, int lg) {
  extern __shared__ double2 dc_sm[];
  const int S = 1 << lg, rs = S + RPAD, nr = (S >> 1) + 1;
  double2* const tw = dc_sm;
  double2* const x = dc_sm + (S >> 1);        // [2][rs]: column kx, column S - kx
  const int pr = blockIdx.y, kx = blockIdx.x;
  const int kxm = (S - kx) & (S - 1);
  const bool pair = kxm != kx;                // kx = 0 and kx = S / 2 are their own mirrors
  make_twiddles(tw, lg);
  const double2* const c0 = T + ((long)pr * S + bitrev(kx, lg)) * S;
  const double2* const c1 = T + ((long)pr * S + bitrev(kxm, lg)) * S;
  for (int i = threadIdx.x; i < S; i += blockDim.x) {
    x[i] = c0[i];
    if (pair) x[rs + i] = c1[i];
  }
  __syncthreads();
  fft_rows(x, tw, pair ? 2 : 1, rs, lg);
  const double2* const xm = pair ? x + rs : x;
  const double mult = pair ? 2.0 : 1.0;
  const long plane = (long)nr * nr;
  for (int r = (kx > 2 ? kx : 2) + threadIdx.x; r < nr; r += blockDim.x) {
    // ring r of this column: (2r - 1)^2 <= 4 (kx^2 + ky^2) < (2r + 1)^2, that is a <= |ky| < e, ky in [-S/2, S/2)
    const int a = half_root_up((2 * r - 1) * (2 * r - 1) - 4 * kx * kx);
    const int e = half_root_up((2 * r + 1) * (2 * r + 1) - 4 * kx * kx);
    double a1 = 0, q1 = 0, a2 = 0, q2 = 0;
    int n = 0;
    auto term = [&](int ky) {
      const double2 A = x[bitrev(ky & (S - 1), lg)], B = xm[bitrev(-ky & (S - 1), lg)];    // Z(k), Z(-k)
      const double f1x = 0.5 * (A.x + B.x), f1y = 0.5 * (A.y - B.y);
      const double f2x = 0.5 * (A.y + B.y), f2y = -0.5 * (A.x - B.x);
      const double m1 = f1x * f1x + f1y * f1y, m2 = f2x * f2x + f2y * f2y;
      a1 += sqrt(m1); q1 += m1;
      a2 += sqrt(m2); q2 += m2;
      ++n;
    };
    const int top = e - 1 < (S >> 1) ? e - 1 : (S >> 1);
    for (int ky = -top; ky <= -(a > 1 ? a : 1); ++ky) term(ky);
    for (int ky = a; ky <= (top < (S >> 1) ? top : (S >> 1) - 1); ++ky) term(ky);
    const long o = (((long)pr * 5) * nr + kx) * nr + r;
    part[o] = mult * a1;
    part[o + plane] = mult * q1;
    part[o + 2 * plane] = mult * a2;
    part[o + 3 * plane] = mult * q2;
    ((long long*)part)[o + 4 * plane] = (pair ? 2 : 1) * (long long)n;
  }
}

struct Peak { int ring; double amp; };

// ONE WAVE: curve d[2 .. M] of the high-pass of width sigma (0: no filter) into dw (LDS, this wave's) and, if given, into gcurve
// (global, [M + 1], rings 0 and 1 are 0), and its peak by step 7 of the header.  sA, sQ: the ring sums; sN: the number of
// frequencies on the rings 2 .. r.  All 64 lanes return the same Peak.
__device__ Peak wave_curve(const double* sA, const double* sQ, const double* sN, double* dw, int M, double sigma, double S,
                           double* gcurve) {
  const int lane = threadIdx.x & 63;
  const int c = (M - 1 + 63) >> 6;
  const int lo = 2 + lane * c, hi = lo + c < M + 1 ? lo + c : M + 1;       // lo >= hi: a lane without rings
  const double INF = __longlong_as_double(0x7ff0000000000000LL);
  const double k = -2.0 * PI2 * sigma * sigma / (S * S);
  // the numerator's terms, this lane's total, the denominator's filter sum
  double s = 0.0, q2 = 0.0;
  for (int r = lo; r < hi; ++r) {
    const double g = sigma > 0.0 ? -expm1(k * ((double)r * (double)r)) : 1.0;
    const double t = g * sA[r];
    dw[r] = t;
    s += t;
    q2 += (g * g) * sQ[r];
  }
  double inc = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const double v = __shfl_up(inc, o, 64); if (lane >= o) inc += v; }
  double run = __shfl_up(inc, 1, 64);
  if (lane == 0) run = 0.0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) q2 += __shfl_xor(q2, o, 64);          // a + b = b + a: the same bits on every lane
  double cm = -INF;
  for (int r = lo; r < hi; ++r) {
    run += dw[r];
    const double den = q2 * sN[r];
    const double d = den > 0.0 ? run / sqrt(den) : 0.0;
    dw[r] = d;
    if (gcurve) gcurve[r] = d;
    cm = fmax(cm, d);
  }
  if (gcurve && lane == 0) gcurve[0] = gcurve[1] = 0.0;
  // the maximum in front of this lane's rings; its records; the minimum and number of its rings in front of its first record
  double pin = cm;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const double v = __shfl_up(pin, o, 64); if (lane >= o) pin = fmax(pin, v); }
  double pm = __shfl_up(pin, 1, 64);
  if (lane == 0) pm = -INF;
  unsigned rec = 0;
  double hm = INF;
  int hc = 0, seen = 0;
  for (int r = lo; r < hi; ++r) {
    const double d = dw[r];
    if (d > pm) { rec |= 1u << (r - lo); pm = d; seen = 1; }
    else if (!seen) { hm = fmin(hm, d); ++hc; }
  }
  // what the lanes above hold of this lane's last segment: up to and with the first lane that has a record
  double mn = INF;
  int cnt = 0, done = 0;
  for (int o = 1; o < 64; ++o) {
    const double v = __shfl_down(hm, o, 64);
    const int n = __shfl_down(hc, o, 64), h = __shfl_down(seen, o, 64);
    if (!done && lane + o < 64) { mn = fmin(mn, v); cnt += n; done = h; }
  }
  int cand = 0;
  for (int r = hi - 1; r >= lo; --r) {
    const double d = dw[r];
    if (rec >> (r - lo) & 1) {
      if (r != 2 && cnt > 0 && d - mn >= PEAK_DROP) { cand = r; break; }
      mn = INF;
      cnt = 0;
    } else {
      mn = fmin(mn, d);
      ++cnt;
    }
  }
  int best = cand;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const int v = __shfl_xor(best, o, 64); best = v > best ? v : best; }
  double amp = best >= lo && best < hi ? dw[best] : 0.0;                   // one lane owns it; d >= 0
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) amp = fmax(amp, __shfl_xor(amp, o, 64));
  return Peak{best, best ? amp : 0.0};
}

// the first of the curves 0 .. n - 1 with the largest peak ring
__device__ __forceinline__ int best_curve(const int* ring, int n) {
  int b = 0;
  for (int j = 1; j < n; ++j) b = ring[j] > ring[b] ? j : b;
  return b;
}

// grid B, FIN_WAVES waves.  out[b][5] = cut, ring, amp, sigma, side; curves[b][21][S/2 + 1] and peaks[b][21] if given
__global__ void __launch_bounds__(FIN_WAVES * 64) k_dc_fin(const double* __restrict__ part, int lg, double* __restrict__ out,
                                                            double* __restrict__ curves, int* __restrict__ peaks) {
  extern __shared__ double dcf_sm[];
  __shared__ int s_ring[NCURVE];
  __shared__ double s_amp[NCURVE], s_sig[NCURVE];
  const int S = 1 << lg, M = S >> 1, nr = M + 1, nrp = (nr + 7) & ~7, b = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double* const sA = dcf_sm;                  // [nrp] each
  double* const sQ = sA + nrp;
  double* const sN = sQ + nrp;
  double* const dw = sN + nrp + wave * nrp;
  const long plane = (long)nr * nr;
  const double* const p = part + (long)(b >> 1) * 5 * plane + (b & 1) * 2 * plane;
  const long long* const pn = (const long long*)(part + (long)(b >> 1) * 5 * plane + 4 * plane);
  for (int r = threadIdx.x; r < nr; r += FIN_WAVES * 64) {
    double a = 0, q = 0;
    long long n = 0;
    if (r >= 2)
      for (int kx = 0; kx <= r; ++kx) {
        const long o = (long)kx * nr + r;
        a += p[o]; q += p[o + plane]; n += pn[o];
      }
    sA[r] = a; sQ[r] = q; sN[r] = (double)n;
  }
  __syncthreads();
  if (wave == 0) {                            // sN[r] <- the number of frequencies on the rings 2 .. r: integers, exact
    const int c = (M - 1 + 63) >> 6;
    const int lo = 2 + lane * c, hi = lo + c < nr ? lo + c : nr;
    double s = 0;
    for (int r = lo; r < hi; ++r) s += sN[r];
    double inc = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const double v = __shfl_up(inc, o, 64); if (lane >= o) inc += v; }
    double run = inc - s;
    for (int r = lo; r < hi; ++r) { run += sN[r]; sN[r] = run; }
  }
  __syncthreads();
  double* const cv = curves ? curves + (long)b * NCURVE * nr : nullptr;
  if (wave == 0) {
    const Peak pk = wave_curve(sA, sQ, sN, dw, M, 0.0, (double)S, cv);
    if (lane == 0) { s_ring[0] = pk.ring; s_amp[0] = pk.amp; s_sig[0] = 0.0; }
  }
  __syncthreads();
  double la = log(s_ring[0] ? (double)S / (double)s_ring[0] : (double)M), lb = log(SIGMA_MIN);
  for (int bank = 0; bank < 2; ++bank) {
    const int j = 1 + bank * NBANK + wave;
    if (bank == 1) {
      const int bj = best_curve(s_ring, 1 + NBANK);
      if (bj == 0) {                          // curve 0 is the best: no bank 2
        if (cv) for (int r = lane; r < nr; r += 64) cv[(long)j * nr + r] = 0.0;
        if (lane == 0) { s_ring[j] = 0; s_amp[j] = 0.0; s_sig[j] = 0.0; }
        continue;
      }
      la = log(s_sig[bj - 1 > 1 ? bj - 1 : 1]);
      lb = log(s_sig[bj + 1 < NBANK ? bj + 1 : NBANK]);
    }
    // np.linspace(la, lb, 10)[wave]: start + wave * step, and the stop itself at the end
    const double sigma = exp(wave == NBANK - 1 ? lb : la + (double)wave * ((lb - la) / (double)(NBANK - 1)));
    const Peak pk = wave_curve(sA, sQ, sN, dw, M, sigma, (double)S, cv ? cv + (long)j * nr : nullptr);
    if (lane == 0) { s_ring[j] = pk.ring; s_amp[j] = pk.amp; s_sig[j] = sigma; }
    __syncthreads();
  }
  __syncthreads();
  if (threadIdx.x < NCURVE && peaks) peaks[b * NCURVE + threadIdx.x] = s_ring[threadIdx.x];
  if (threadIdx.x == 0) {
    const int bj = best_curve(s_ring, NCURVE);
    double* const o = out + (long)b * 5;
    o[0] = (double)s_ring[bj] / (double)M;
    o[1] = (double)s_ring[bj];
    o[2] = s_amp[bj];
    o[3] = s_sig[bj];
    o[4] = (double)S;
  }
}

size_t fin_lds(int S) { return (size_t)(3 + FIN_WAVES) * ((((S >> 1) + 1) + 7) & ~7) * sizeof(double); }
static_assert((3 + FIN_WAVES) * ((((MAXS >> 1) + 1) + 7) & ~7) * 8 <= 160 * 1024, "k_dc_fin: LDS at the largest side");

long ws_doubles(int B, int S) {
  const long nr = (S >> 1) + 1, P = (B + 1) / 2;
  return P * (2L * S * S + 5L * nr * nr);
}

}  // namespace

extern "C" {

long srhip_metrics_decorr_lv_ws(int B, int H, int W) {
  const int lg = side_log2(H, W);
  return B > 0 && lg ? ws_doubles(B, 1 << lg) : 0;
}

int srhip_metrics_decorr_lv(const float* img, int B, int H, int W, int L, int inputs_are_levels, double* workspace,
                            long workspace_doubles, double* out, double* curves, int* peaks, void* stream) {
  SR_REQUIRE(L >= 255 && L <= 65535, "metrics_decorr_lv: the white level is 255 .. 65535 (got %d)", L);
  SR_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0, "metrics_decorr_lv: empty input or more than 65535 images");
  const int lg = side_log2(H, W);
  SR_REQUIRE(lg, "metrics_decorr_lv: both sides must be at least %d (got %d x %d)", MINS, H, W);
  const int S = 1 << lg, P = (B + 1) / 2;
  SR_REQUIRE(img && workspace && out, "metrics_decorr_lv: null pointer");
  const long need = ws_doubles(B, S);
  SR_REQUIRE(workspace_doubles >= need && ((uintptr_t)workspace & 15) == 0,
             "metrics_decorr_lv: the workspace holds %ld doubles, the call needs %ld (srhip_metrics_decorr_lv_ws), 16-byte aligned",
             workspace_doubles, need);
  const size_t lr = rows_lds(S), lc = cols_lds(S), lf = fin_lds(S);
  // above the 64 KiB default the attribute is set at every call, as in srhip_metrics_frc_lv: it belongs to the current device
  constexpr size_t LDS_DEFAULT = 64 * 1024;
  if (lr > LDS_DEFAULT &&
      hipFuncSetAttribute((const void*)k_dc_rows, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lr) != hipSuccess)
    return sr_fail(-5, "metrics_decorr_lv: cannot reserve %zu bytes of LDS", lr);
  if (lc > LDS_DEFAULT &&
      hipFuncSetAttribute((const void*)k_dc_cols, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lc) != hipSuccess)
    return sr_fail(-5, "metrics_decorr_lv: cannot reserve %zu bytes of LDS", lc);
  if (lf > LDS_DEFAULT &&
      hipFuncSetAttribute((const void*)k_dc_fin, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lf) != hipSuccess)
    return sr_fail(-5, "metrics_decorr_lv: cannot reserve %zu bytes of LDS", lf);
  hipStream_t st = (hipStream_t)stream;
  double2* const T = (double2*)workspace;
  double* const part = workspace + 2L * P * S * S;
  const int nt_r = ROWS * S / 2 < 1024 ? ROWS * S / 2 : 1024;      // a butterfly per thread and stage, 64 .. 1024
  const int nt_c = S < 64 ? 64 : (S < 1024 ? S : 1024);
  hipLaunchKernelGGL(k_dc_rows, dim3(S / ROWS, P), dim3(nt_r), lr, st, img, T, B, H, W, lg, L, inputs_are_levels);
  hipLaunchKernelGGL(k_dc_cols, dim3(S / 2 + 1, P), dim3(nt_c), lc, st, (const double2*)T, part, lg);
  hipLaunchKernelGGL(k_dc_fin, dim3(B), dim3(FIN_WAVES * 64), lf, st, (const double*)part, lg, out, curves, peaks);
  SR_LAUNCH_CHECK("metrics_decorr_lv");
  return 0;
}

}  // extern "C"
