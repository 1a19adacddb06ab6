// Input-pipeline row f2: the 'edt', 'edt*roi' and Otsu ('automatic_threshold') styles of the training-crop sampler
// (PatchSampler, dlib/datasets/dataset_dpsr.py:371-457,479-480) on resident tiles.
//   * srhip_edt_sq: the exact squared Euclidean distance transform of img >= threshold, in integers (scipy's
//     distance_transform_edt is exactly its square root);
//   * srhip_hist_u8: the 256-bin histogram Otsu's threshold is computed from;
//   * srhip_origin_rowcum / srhip_origin_sample: inverse CDF of the reference's origin probabilities, fp64, from one
//     uniform per patch.  The weights are recomputed from d2 and the ROI bit; only a row prefix per tile is stored.
#include "common.h"
#include "../../include/srhip.h"

namespace {

constexpr int EDT_MAX_SIDE = 16384;
// "this column holds no background pixel": above every real d2 (<= 2 * 16384^2 = 2^29), and small enough that
// EDT_SENT + (c - c')^2 (<= 2^30 + (16384 + 256)^2 < 2^31) cannot wrap, so pass 2 needs no branch
constexpr int EDT_SENT = 1 << 30;
constexpr int EDT_CHUNK = 4096;          // ints of one row staged in LDS at a time (16 KiB)

// Pass 1, one lane per column: g = distance to the nearest background pixel above or below, stored squared.
__global__ void __launch_bounds__(256) k_edt_cols(const unsigned char* __restrict__ img, int H, int W, int th,
                                                  int* __restrict__ g2) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= W) return;
  int dist = -1;                                            // -1: no background pixel met yet
  for (int r = 0; r < H; ++r) {
    const bool bg = img[(long)r * W + c] < th;
    dist = bg ? 0 : (dist < 0 ? -1 : dist + 1);
    g2[(long)r * W + c] = dist;
  }
  dist = -1;
  for (int r = H - 1; r >= 0; --r) {
    const int down = g2[(long)r * W + c];
    dist = down == 0 ? 0 : (dist < 0 ? -1 : dist + 1);
    const int g = down < 0 ? dist : (dist < 0 ? down : min(down, dist));
    g2[(long)r * W + c] = g < 0 ? EDT_SENT : g * g;
  }
}

// Pass 2, one lane per output pixel of row blockIdx.y: min over c' of (c - c')^2 + g2[c'], the row's g2 read from LDS
// (every lane the same address: a broadcast).  Without any background pixel in the image every column holds the
// sentinel; scipy then measures to a virtual pixel at (-1, 0).
__global__ void __launch_bounds__(256) k_edt_rows(const int* __restrict__ g2, int H, int W, int* __restrict__ d2) {
  __shared__ __attribute__((aligned(16))) int s[EDT_CHUNK];
  const int r = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  const int* row = g2 + (long)r * W;
  int best = 0x7fffffff;
  for (int c0 = 0; c0 < W; c0 += EDT_CHUNK) {
    const int n = min(EDT_CHUNK, W - c0), n4 = (n + 3) & ~3;
    __syncthreads();
    for (int i = threadIdx.x; i < n4; i += 256) s[i] = i < n ? row[c0 + i] : EDT_SENT;
    __syncthreads();
    for (int i = 0; i < n4; i += 4) {
      const int4 v = *reinterpret_cast<const int4*>(&s[i]);
      const int d = c - (c0 + i);
      best = min(best, v.x + __mul24(d, d));
      best = min(best, v.y + __mul24(d - 1, d - 1));
      best = min(best, v.z + __mul24(d - 2, d - 2));
      best = min(best, v.w + __mul24(d - 3, d - 3));
    }
  }
  if (c < W) d2[(long)r * W + c] = best >= EDT_SENT ? (r + 1) * (r + 1) + c * c : best;
}

__global__ void __launch_bounds__(256) k_hist_u8(const unsigned char* __restrict__ img, long n, int* __restrict__ counts) {
  __shared__ int h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) atomicAdd(&h[img[i]], 1);
  __syncthreads();
  if (h[threadIdx.x]) atomicAdd(&counts[threadIdx.x], h[threadIdx.x]);
}

// Unnormalised weight of one candidate origin (proportional to the reference's probability: :343-347,389-392,431-439).
constexpr double ROI_W1 = 149.4131591025766, ROI_W0 = 2.0;      // exp(5) + 1, exp(0) + 1
__device__ __forceinline__ double origin_weight(int style, bool roi, int d2) {
#pragma clang fp contract(off)
  if (style == SRHIP_ORIGIN_ROI) return roi ? ROI_W1 : ROI_W0;
  const double d = sqrt((double)d2);
  if (style == SRHIP_ORIGIN_EDT) return d + 1.0;
  return (roi ? ROI_W1 : ROI_W0) * (exp(d) + 1.0);
}

// One wave walks the candidates of row R in tiles of 64: an inclusive scan inside the tile (fixed tree), the carry is the
// cumulative weight at the tile's last candidate.  SEARCH = false returns the row total; SEARCH = true returns in `col` the
// first candidate with base + cum > target.  Both add the same terms in the same order, so with base + total = the row
// prefix the search always ends inside the row (and is clamped to its last candidate regardless).
template <bool SEARCH>
__device__ __forceinline__ double row_walk(const srhip_origin_tile& T, int R, int lane, double base, double target, int& col) {
#pragma clang fp contract(off)
  const int Wc = T.W - T.P, half = T.P / 2;
  const unsigned char* img = T.img + (long)(R + half) * T.W + half;
  const int* d2 = T.d2 ? T.d2 + (long)(R + half) * T.W + half : nullptr;
  double carry = 0.0;
  for (int c0 = 0; c0 < Wc; c0 += 64) {
    const int c = c0 + lane;
    double w = 0.0;
    if (c < Wc) w = origin_weight(T.style, img[c] >= T.threshold, d2 ? d2[c] : 0);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double up = __shfl_up(w, o, 64);
      if (lane >= o) w += up;
    }
    const double cum = carry + w;
    if (SEARCH) {
      const unsigned long long hit = __ballot(c < Wc && base + cum > target);
      if (hit) { col = c0 + __ffsll((long long)hit) - 1; return cum; }
    }
    carry = __shfl(cum, min(63, Wc - 1 - c0), 64);
  }
  return carry;
}

// one wave per candidate row: rowcum[r] = total weight of row r
__global__ void __launch_bounds__(256) k_origin_rowsum(srhip_origin_tile T, double* __restrict__ rowcum) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= T.H - T.P) return;
  int col;
  const double total = row_walk<false>(T, r, lane, 0.0, 0.0, col);
  if (lane == 0) rowcum[r] = total;
}

// in place, one wave: rowcum[r] = rowcum[r - 1] + rowsum[r], strictly in this order
__global__ void __launch_bounds__(64) k_origin_prefix(double* __restrict__ rowcum, int n) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x;
  double acc = 0.0;
  for (int r0 = 0; r0 < n; r0 += 64) {
    const double v = r0 + lane < n ? rowcum[r0 + lane] : 0.0;
    double out = 0.0;
    for (int l = 0; l < 64; ++l) {
      acc += __shfl(v, l, 64);
      if (lane == l) out = acc;
    }
    if (r0 + lane < n) rowcum[r0 + lane] = out;
  }
}

// one wave per patch: search the row prefix, then walk the chosen row
__global__ void __launch_bounds__(256) k_origin_sample(const srhip_origin_tile* __restrict__ table, int ntiles,
                                                       const int* __restrict__ ids, const double* __restrict__ u, int B,
                                                       int* __restrict__ origin) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= B) return;
  const int id = ids[b];
  int R = -1, C = -1;                                        // an id outside the table: no tile is touched
  if (id >= 0 && id < ntiles) {
    const srhip_origin_tile T = table[id];
    const int Hc = T.H - T.P, Wc = T.W - T.P;
    const double target = u[b] * T.rowcum[Hc - 1];
    int lo = 0, hi = Hc - 1;                                 // first row whose prefix exceeds the target, else the last
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (T.rowcum[mid] > target) hi = mid; else lo = mid + 1;
    }
    R = lo;
    C = Wc - 1;
    row_walk<true>(T, R, lane, R ? T.rowcum[R - 1] : 0.0, target, C);
  }
  if (lane == 0) { origin[2 * b] = R; origin[2 * b + 1] = C; }
}

}  // namespace

extern "C" int srhip_edt_sq(const unsigned char* img, int H, int W, int threshold, int* workspace, int* d2, void* stream) {
  SR_REQUIRE(H > 0 && W > 0 && H <= EDT_MAX_SIDE && W <= EDT_MAX_SIDE,
             "edt_sq: tile %dx%d: sides must lie in 1..%d (d2 stays below 2^31)", H, W, EDT_MAX_SIDE);
  SR_REQUIRE(img && workspace && d2 && workspace != d2, "edt_sq: NULL argument / workspace aliases d2");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_edt_cols, dim3(sr_cdiv(W, 256)), dim3(256), 0, st, img, H, W, threshold, workspace);
  hipLaunchKernelGGL(k_edt_rows, dim3(sr_cdiv(W, 256), H), dim3(256), 0, st, (const int*)workspace, H, W, d2);
  SR_LAUNCH_CHECK("edt_sq");
  return 0;
}

extern "C" int srhip_hist_u8(const unsigned char* img, long n, int* counts, void* stream) {
  SR_REQUIRE(img && counts && n > 0 && n < (1L << 31), "hist_u8: NULL argument / pixel count %ld outside 1..2^31-1", n);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, 256 * sizeof(int), st) != hipSuccess) return sr_fail(-5, "hist_u8: memset failed");
  long g = (n + 256 * 16 - 1) / (256 * 16);
  if (g > 1024) g = 1024;
  hipLaunchKernelGGL(k_hist_u8, dim3((unsigned)g), dim3(256), 0, st, img, n, counts);
  SR_LAUNCH_CHECK("hist_u8");
  return 0;
}

static int origin_tile_check(const char* who, const srhip_origin_tile& T) {
  SR_REQUIRE(T.H > 0 && T.W > 0 && T.H <= EDT_MAX_SIDE && T.W <= EDT_MAX_SIDE,
             "%s: tile %dx%d: sides must lie in 1..%d", who, T.H, T.W, EDT_MAX_SIDE);
  SR_REQUIRE(T.P > 0 && T.H > T.P && T.W > T.P, "%s: tile %dx%d must exceed the patch %d", who, T.H, T.W, T.P);
  SR_REQUIRE(T.style == SRHIP_ORIGIN_ROI || T.style == SRHIP_ORIGIN_EDT || T.style == SRHIP_ORIGIN_EDTXROI,
             "%s: style %d (0 roi, 1 edt, 2 edt*roi)", who, T.style);
  SR_REQUIRE(T.img && T.rowcum && (T.d2 || T.style == SRHIP_ORIGIN_ROI), "%s: NULL image / d2 / row prefix", who);
  return 0;
}

extern "C" int srhip_origin_rowcum(const srhip_origin_tile* tile, void* stream) {
  SR_REQUIRE(tile, "origin_rowcum: NULL tile");
  if (int rc = origin_tile_check("origin_rowcum", *tile)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int Hc = tile->H - tile->P;
  hipLaunchKernelGGL(k_origin_rowsum, dim3(sr_cdiv(Hc, 4)), dim3(256), 0, st, *tile, tile->rowcum);
  hipLaunchKernelGGL(k_origin_prefix, dim3(1), dim3(64), 0, st, tile->rowcum, Hc);
  SR_LAUNCH_CHECK("origin_rowcum");
  return 0;
}

extern "C" int srhip_origin_sample(const srhip_origin_tile* table, int ntiles, const int* ids, const double* uniforms, int B,
                                   int* origins, void* stream) {
  SR_REQUIRE(table && ids && uniforms && origins, "origin_sample: NULL argument");
  SR_REQUIRE(ntiles > 0 && B > 0, "origin_sample: empty table / batch (ntiles=%d B=%d)", ntiles, B);
  hipLaunchKernelGGL(k_origin_sample, dim3(sr_cdiv(B, 4)), dim3(256), 0, (hipStream_t)stream, table, ntiles, ids, uniforms, B,
                     origins);
  SR_LAUNCH_CHECK("origin_sample");
  return 0;
}
