// Resolution-scaled error (predict.py --consistency; Culley et al., Nature Methods 2018): is the net's output E still an image of
// the LR page L that was acquired?  E is degraded back to the acquisition, b_q = bin_s(G_sigma * E) with sigma = q s / 64, the
// blur that explains L best is searched over two banks of 16 candidates, and the Pearson coefficient (RSP), the RMS residual
// (RSE) and the signed residual map of the winner are reported.  include/srhip.h states the measure; tests/consistency_ref.py
// restates it in numpy.
//
// The candidate images never exist in memory.  A block owns (page, candidate, tile of 64 / s LR rows): per strip of 32 LR columns
// it stages eight HR rows with their halo in LDS as float32 (the reflection is resolved there), forms their row correlations in
// float64 into an LDS buffer of at most 64 + 2 * 64 rows, runs the column correlation out of that buffer and folds b, b^2, b l,
// l, l^2 into five running sums per thread.  A tile of 64 HR rows under a radius of 64 recomputes each row correlation three
// times; in exchange every block is independent and nothing but 5 doubles a block leaves the CU.
//
//   k_cons_bank<S, false>   16 candidates x tiles x pages: the block's five sums (wave butterflies, then the four waves in order)
//   k_cons_decide           one wave a page: the tiles' partials in ascending order, the 16 scores, the first largest; after the
//                           coarse bank it writes the fine bank's q list, after the fine bank the page's result
//   k_cons_bank<S, true>    the winner once more: float32(l - (alpha b + beta))
//
// Five launches (four without the map), no atomics, no host synchronisation.  The partition depends on (h, w, s) alone and a
// candidate's arithmetic on (page, q) alone: a page gives the same bits alone or inside any batch, in any slot of a bank.
#include "common.h"
#include <math.h>

// every product and sum below is rounded on its own, as numpy rounds them: a fused multiply-add would move last bits
#pragma clang fp contract(off)

namespace {

constexpr int CN_Q = 128;               // candidates of the table: sigma = q s / 64, q = 0 .. 127
constexpr int CN_MAXR = 64;             // radius of q = 127 at s = 8, srhip_psf_bin's limit
constexpr int CN_PITCH = 2 * CN_MAXR + 8;       // doubles a table row: 2 r + s weights, zeros behind them
constexpr int CN_BANK = 16;             // candidates a bank
constexpr int CN_CW = 32;               // LR columns a strip
constexpr int CN_RG = 8;                // HR rows staged at a time: 8 x 32 outputs, one a thread
constexpr int CN_THREADS = CN_CW * CN_RG;

// scipy's 'reflect' border (d c b a | a b c d | d c b a) for any distance from the line
__device__ __forceinline__ int reflect(int i, int n) {
  if (i >= 0 && i < n) return i;
  int m = i % (2 * n);
  if (m < 0) m += 2 * n;
  return m < n ? m : 2 * n - 1 - m;
}

template <int S>
struct Geo {
  static constexpr int TI = 64 / S;                             // LR rows a tile
  static constexpr int ROWS = TI * S + 2 * CN_MAXR;             // row correlations a tile keeps
  static constexpr int SEG = CN_CW * S + 2 * CN_MAXR;           // HR pixels of a staged row
  // the 32 lanes of a half-wave read pixels S apart (ds_read_b32: 32 banks): an even S gets one pad word every S pixels, so
  // that the lanes are S + 1 words apart
  static constexpr bool PAD = S % 2 == 0;
  static constexpr int SEGP = PAD ? SEG + SEG / S + 1 : SEG;
  __device__ static __forceinline__ int at(int p) { return PAD ? p + p / S : p; }
};

__device__ __forceinline__ int radius_of(int q, int s) { return (q * s + 8) >> 4; }      // int(4 sigma + 0.5), sigma = q s / 64

template <int S, bool RESID>
__global__ void __launch_bounds__(CN_THREADS) k_cons_bank(const float* __restrict__ E, long E_plane, long E_ld,
                                                          const float* __restrict__ L, long L_plane, long L_ld, int h, int w,
                                                          const double* __restrict__ table, const int* __restrict__ qlist,
                                                          double* __restrict__ partials, int ntile,
                                                          const double* __restrict__ result, float* __restrict__ residual) {
  typedef Geo<S> G;
  __shared__ double rbuf[G::ROWS * CN_CW];
  __shared__ float stage[CN_RG * G::SEGP];
  __shared__ double wts[CN_PITCH];
  __shared__ double red[CN_THREADS / SR_WAVE][5];
  const int tid = threadIdx.x, tile = blockIdx.x, slot = blockIdx.y, b = blockIdx.z;
  const int H = h * S, W = w * S;
  int q;
  double alpha = 0.0, beta = 0.0;
  if (RESID) {
    q = (int)result[b * 8L + 5];
    alpha = result[b * 8L + 1];
    beta = result[b * 8L + 2];
  } else {
    q = qlist ? qlist[b * CN_BANK + slot] : 8 * slot;
  }
  q = min(max(q, 0), CN_Q - 1);
  const int r = radius_of(q, S), taps = 2 * r + S;
  if (tid < CN_PITCH) wts[tid] = table[(long)q * CN_PITCH + tid];
  const float* Eb = E + b * E_plane;
  const float* Lb = L + b * L_plane;
  const int i0 = tile * G::TI, ti = min(G::TI, h - i0);
  const int nrows = ti * S + 2 * r, y0 = i0 * S - r;
  double s_b = 0.0, s_bb = 0.0, s_bl = 0.0, s_l = 0.0, s_ll = 0.0;
  for (int j0 = 0; j0 < w; j0 += CN_CW) {
    const int cw = min(CN_CW, w - j0), seg = cw * S + 2 * r, x0 = j0 * S - r;
    for (int g0 = 0; g0 < nrows; g0 += CN_RG) {
      __syncthreads();            // the last readers of stage (and, in a new strip, of rbuf) are done; wts is written
      for (int idx = tid; idx < CN_RG * seg; idx += CN_THREADS) {
        const int rr = idx / seg, p = idx - rr * seg;
        if (g0 + rr < nrows)
          stage[rr * G::SEGP + G::at(p)] = ldg_f(Eb + (long)reflect(y0 + g0 + rr, H) * E_ld + reflect(x0 + p, W));
      }
      __syncthreads();
      const int rr = tid / CN_CW, j = tid % CN_CW;
      if (g0 + rr < nrows && j < cw) {
        const float* row = stage + rr * G::SEGP;
        double acc = 0.0;
        for (int t = 0; t < taps; ++t) acc += wts[t] * (double)row[G::at(j * S + t)];
        rbuf[(g0 + rr) * CN_CW + j] = acc;
      }
    }
    __syncthreads();
    for (int item = tid; item < ti * CN_CW; item += CN_THREADS) {
      const int ii = item / CN_CW, j = item % CN_CW;
      if (j >= cw) continue;
      const double* col = rbuf + ii * S * CN_CW + j;
      double acc = 0.0;
      for (int t = 0; t < taps; ++t) acc += wts[t] * col[t * CN_CW];
      const double l = (double)ldg_f(Lb + (long)(i0 + ii) * L_ld + j0 + j);
      if (RESID) {
        residual[((long)b * h + i0 + ii) * w + j0 + j] = (float)(l - (alpha * acc + beta));
      } else {
        s_b += acc;
        s_bb += acc * acc;
        s_bl += acc * l;
        s_l += l;
        s_ll += l * l;
      }
    }
  }
  if (RESID) return;
  double v[5] = {wave_sum_d(s_b), wave_sum_d(s_bb), wave_sum_d(s_bl), wave_sum_d(s_l), wave_sum_d(s_ll)};
  if ((tid & (SR_WAVE - 1)) == 0)
    for (int k = 0; k < 5; ++k) red[tid / SR_WAVE][k] = v[k];
  __syncthreads();
  if (tid < 5) {
    double t = red[0][tid];
    for (int wv = 1; wv < CN_THREADS / SR_WAVE; ++wv) t += red[wv][tid];
    partials[(((long)b * CN_BANK + slot) * ntile + tile) * 5 + tid] = t;
  }
}

// one wave a page.  fine == 0: the coarse bank (q = 8 c) -> the fine bank's q list; fine == 1: the fine bank -> out[b][8]
__global__ void __launch_bounds__(SR_WAVE) k_cons_decide(const double* __restrict__ partials, int ntile, double n, int s, int fine,
                                                         int* __restrict__ qlist, double* __restrict__ out,
                                                         double* __restrict__ scores, int* __restrict__ qs) {
  __shared__ double sm[CN_BANK][5];
  __shared__ double sc[CN_BANK];
  const int c = threadIdx.x, b = blockIdx.x;
  if (c < CN_BANK) {
    const double* p = partials + ((long)b * CN_BANK + c) * ntile * 5;
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int t = 0; t < ntile; ++t)
      for (int k = 0; k < 5; ++k) v[k] += p[t * 5 + k];
    const double cbb = v[1] - v[0] * v[0] / n, cll = v[4] - v[3] * v[3] / n, cbl = v[2] - v[0] * v[3] / n;
    const double score = (cbb > 0.0 && cll > 0.0) ? cbl * fabs(cbl) / (cbb * cll) : 0.0;
    for (int k = 0; k < 5; ++k) sm[c][k] = v[k];
    sc[c] = score;
    const int q = fine ? qlist[b * CN_BANK + c] : 8 * c;
    if (scores) scores[b * 32L + fine * CN_BANK + c] = score;
    if (qs) qs[b * 32L + fine * CN_BANK + c] = q;
  }
  __syncthreads();
  if (c != 0) return;
  int best = 0;
  for (int k = 1; k < CN_BANK; ++k)
    if (sc[k] > sc[best]) best = k;             // the FIRST index of the largest score
  if (!fine) {
    for (int m = 0; m < CN_BANK; ++m) qlist[b * CN_BANK + m] = max(0, 8 * best + m - 8);
    return;
  }
  const double sb = sm[best][0], sbb = sm[best][1], sbl = sm[best][2], sl = sm[best][3], sll = sm[best][4];
  const double cbb = sbb - sb * sb / n, cll = sll - sl * sl / n, cbl = sbl - sb * sl / n;
  double* o = out + b * 8L;
  if (cbb > 0.0 && cll > 0.0) {
    const int q = qlist[b * CN_BANK + best];
    const double score = sc[best], alpha = cbl / cbb;
    const double root = sqrt(fabs(score));
    o[0] = (double)(q * s) / 64.0;
    o[1] = alpha;
    o[2] = (sl - alpha * sb) / n;
    o[3] = score < 0.0 ? -root : root;
    o[4] = sqrt(fmax(0.0, cll - cbl * cbl / cbb) / n);
    o[5] = (double)q;
  } else {                                      // a constant page, or a constant model: nothing to scale
    o[0] = 0.0;
    o[1] = 0.0;
    o[2] = sl / n;
    o[3] = 0.0;
    o[4] = sqrt(fmax(0.0, cll) / n);
    o[5] = 0.0;
  }
  o[6] = n;
  o[7] = 0.0;
}

inline int tiles_of(int h, int s) { return sr_cdiv(h, 64 / s); }

inline long span_bytes(int B, long plane, long ld, int rows, int cols) {
  return (((long)B - 1) * plane + ((long)rows - 1) * ld + cols) * 4;
}

template <int S>
int run(const float* E, long E_plane, long E_ld, const float* L, long L_plane, long L_ld, int B, int h, int w, const double* table,
        double* ws, double* out, double* scores, int* qs, float* residual, hipStream_t st) {
  const int ntile = tiles_of(h, S);
  double* partials = ws;
  int* qlist = (int*)(ws + (long)B * CN_BANK * ntile * 5);
  const dim3 grid((unsigned)ntile, CN_BANK, (unsigned)B), one((unsigned)ntile, 1, (unsigned)B), blk(CN_THREADS);
  const double n = (double)h * (double)w;
  for (int fine = 0; fine < 2; ++fine) {
    hipLaunchKernelGGL((k_cons_bank<S, false>), grid, blk, 0, st, E, E_plane, E_ld, L, L_plane, L_ld, h, w, table,
                       fine ? (const int*)qlist : (const int*)nullptr, partials, ntile, (const double*)nullptr, (float*)nullptr);
    SR_LAUNCH_CHECK(fine ? "consistency: the fine bank" : "consistency: the coarse bank");
    hipLaunchKernelGGL(k_cons_decide, dim3((unsigned)B), dim3(SR_WAVE), 0, st, (const double*)partials, ntile, n, S, fine, qlist, out,
                       scores, qs);
    SR_LAUNCH_CHECK("consistency: the decision");
  }
  if (residual) {
    hipLaunchKernelGGL((k_cons_bank<S, true>), one, blk, 0, st, E, E_plane, E_ld, L, L_plane, L_ld, h, w, table, (const int*)nullptr,
                       (double*)nullptr, ntile, (const double*)out, residual);
    SR_LAUNCH_CHECK("consistency: the residual map");
  }
  return 0;
}

}  // namespace

extern "C" {

/* doubles of workspace for srhip_consistency (include/srhip.h) */
int srhip_consistency_ws(int B, int h, int w, int s, long* doubles) {
  SR_REQUIRE(doubles, "consistency_ws: null pointer");
  *doubles = 0;
  SR_REQUIRE(s >= 2 && s <= 8, "consistency: the scale s is 2 .. 8 (got %d)", s);
  SR_REQUIRE(B > 0 && h >= 4 && w >= 4, "consistency: B > 0 and both LR sides at least 4 (got %d x %d x %d)", B, h, w);
  *doubles = (long)B * CN_BANK * tiles_of(h, s) * 5 + (long)B * CN_BANK / 2;
  return 0;
}

/* resolution-scaled error of E [B][s h][s w] against L [B][h][w] (include/srhip.h) */
int srhip_consistency(const float* E, long E_plane, long E_ld, const float* L, long L_plane, long L_ld, int B, int h, int w, int s,
                      const double* weights_table, double* workspace, long workspace_doubles, double* out, double* scores, int* qs,
                      float* residual, void* stream) {
  SR_REQUIRE(s >= 2 && s <= 8, "consistency: the scale s is 2 .. 8 (got %d)", s);
  SR_REQUIRE(B > 0 && B <= 65535 && h >= 4 && w >= 4, "consistency: 1 <= B <= 65535 and both LR sides at least 4 (got %d x %d x %d)",
             B, h, w);
  SR_REQUIRE((long)h * s < (1L << 24) && (long)w * s < (1L << 24) && (long)h * w < (1L << 31), "consistency: page too large (%d x %d)",
             h, w);
  SR_REQUIRE(E && L && weights_table && workspace && out, "consistency: null pointer");
  const long sh = (long)h * s, sw = (long)w * s;
  SR_REQUIRE(E_ld >= sw && L_ld >= w, "consistency: a row stride below the row (E_ld %ld for %ld, L_ld %ld for %d)", E_ld, sw, L_ld, w);
  SR_REQUIRE(B == 1 || (E_plane >= (sh - 1) * E_ld + sw && L_plane >= (h - 1L) * L_ld + w),
             "consistency: a plane stride below the page (E_plane %ld, L_plane %ld)", E_plane, L_plane);
  long need = 0;
  if (srhip_consistency_ws(B, h, w, s, &need)) return -22;
  SR_REQUIRE(workspace_doubles >= need, "consistency: the workspace holds %ld doubles, the call needs %ld", workspace_doubles, need);
  SR_REQUIRE(((uintptr_t)E & 3) == 0 && ((uintptr_t)L & 3) == 0 && ((uintptr_t)residual & 3) == 0 && ((uintptr_t)qs & 3) == 0 &&
             ((uintptr_t)weights_table & 7) == 0 && ((uintptr_t)workspace & 7) == 0 && ((uintptr_t)out & 7) == 0 &&
             ((uintptr_t)scores & 7) == 0, "consistency: misaligned pointer");
  const void* buf[8] = {E, L, weights_table, workspace, out, scores, qs, residual};
  const long len[8] = {span_bytes(B, E_plane, E_ld, (int)sh, (int)sw), span_bytes(B, L_plane, L_ld, h, w), CN_Q * CN_PITCH * 8L, need * 8,
                       B * 64L, B * 256L, B * 128L, (long)B * h * w * 4};
  for (int a = 3; a < 8; ++a)             // what the call writes shares no byte with anything else
    for (int c = 0; c < a; ++c)
      SR_REQUIRE(sr_disjoint(buf[a], len[a], buf[c], len[c]), "consistency: buffers %d and %d overlap (E, L, table, workspace, out, "
                 "scores, qs, residual)", c, a);
  const hipStream_t st = (hipStream_t)stream;
#define CN_RUN(S) case S: return run<S>(E, E_plane, E_ld, L, L_plane, L_ld, B, h, w, weights_table, workspace, out, scores, qs, residual, st)
  switch (s) {
    CN_RUN(2); CN_RUN(3); CN_RUN(4); CN_RUN(5); CN_RUN(6); CN_RUN(7); CN_RUN(8);
  }
#undef CN_RUN
  return sr_fail(-22, "consistency: the scale s is 2 .. 8 (got %d)", s);
}

}  // extern "C"
