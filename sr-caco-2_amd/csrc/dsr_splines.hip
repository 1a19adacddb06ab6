// DSR-Splines -- reference DsrSplines.forward / _SplineNet.forward, dlib/models/network_dsr_splines.py:245-260,389-413.
// The reference runs every spline net over the whole interpolated image, multiplies each result by the spline's grey-level
// mask and sums.  With one image channel the masks partition the 256 grey levels, so exactly one spline ("expert") owns a
// pixel; behind the first in_ksz x in_ksz conv every layer is 1x1.  The output at a pixel is therefore a small MLP on the
// pixel's reflect-padded neighbourhood whose weights are chosen by the pixel's own grey level, and that is what runs here:
//
//   k_ds_ids / k_ds_scan / k_ds_scatter   expert id per pixel (uint8(float32(v) * 255.0f) through a 256-entry table) and a
//                                         stable counting sort of the pixel positions by expert (<= 256 keys; the in-tree
//                                         pattern of nlsa.hip's k_bucket_order, spread over blocks).  Segment offsets stay
//                                         on the device; the grids depend on (pixels, n_splines) alone.
//   k_ds_fwd                              one workgroup = 64 pixels of ONE expert (segments are cut into tiles; at most
//                                         n_splines tiles are partly filled): the expert's parameters in LDS, four threads
//                                         per pixel, activations exchanged through LDS.  Nothing per layer goes to HBM.
//   k_ds_bwd / k_ds_grad_reduce           a fixed number of workgroups, dealt to the experts in proportion to their pixels
//                                         (ds_deal), each walking its share of its expert's run in batches of 64 pixels:
//                                         recompute the activations, back-propagate per pixel,
//                                         sum the weight gradients over the batch in pixel order (each element has one owner
//                                         thread) into the workgroup's partial table, then one fixed-order sum over the
//                                         workgroups.  No float atomics: two runs give the same bits.  Experts that own no
//                                         pixel get written zeros.
//
// Parameter table: [n_splines][stride] floats; one expert's block holds its tensors in named_parameters() order (per layer
// conv.weight, conv.bias, then match_sz.weight, match_sz.bias where the layer has them), each padded to a multiple of four
// floats -- the layout of the training step's flat parameter / gradient buffers, which are used in place.
#include "common.h"

namespace {

constexpr int DS_MAXL = 9;        // SPLINEHIDDEN: up to eight hidden widths + the output layer
constexpr int DS_NB = 64;         // pixels per tile / batch
constexpr int DS_AP = 33;         // activation row pitch in LDS (floats): pixels across lanes hit distinct banks
constexpr int DS_T = 256;         // threads: 4 per pixel
constexpr int DS_CH = 4096;       // pixels per block of the sort kernels
constexpr int DS_KEYS = 256;
constexpr int DS_GMAX = 64;

struct DsNet {
  int nl, ks, kk, local, tanh_out, glob, P;
  int ci[DS_MAXL], co[DS_MAXL], w[DS_MAXL], b[DS_MAXL], mw[DS_MAXL], mb[DS_MAXL];
};

inline int ds_pad4(int n) { return (n + 3) / 4 * 4; }

// SPLINEHIDDEN[snet_type{nh}] = [32] * (nh - 1) + [16] (constants.py); layers: in_ksz^2 -> h0, h[i] -> h[i+1], h[-1] -> 1
bool ds_make(DsNet& L, int ksz, int nh, int local, int glob) {
  if (ksz < 1 || ksz > 15 || ksz % 2 == 0 || nh < 1 || nh > 8) return false;
  L.nl = nh + 1; L.ks = ksz; L.kk = ksz * ksz; L.local = local != 0; L.glob = glob != 0; L.tanh_out = glob != 0;
  int off = 0;
  for (int l = 0; l < L.nl; ++l) {
    const int hi = l == 0 ? 1 : (l - 1 == nh - 1 ? 16 : 32), ho = l == L.nl - 1 ? 1 : (l == nh - 1 ? 16 : 32);
    L.ci[l] = hi; L.co[l] = ho;
    L.w[l] = off; off += ds_pad4(ho * hi * (l == 0 ? L.kk : 1));
    L.b[l] = off; off += ds_pad4(ho);
    L.mw[l] = L.mb[l] = -1;
    if (L.local && hi != ho) {
      L.mw[l] = off; off += ds_pad4(ho * hi);
      L.mb[l] = off; off += ds_pad4(ho);
    }
  }
  for (int l = L.nl; l < DS_MAXL; ++l) L.ci[l] = L.co[l] = L.w[l] = L.b[l] = 0, L.mw[l] = L.mb[l] = -1;
  L.P = off;
  return true;
}

__device__ __forceinline__ int ds_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// ---------------------------------------------------------------- expert id and order
// id = lut[clamp(int(float32(v) * 255.0f), 0, 255)] (_SplineNet.get_mask, network_dsr_splines.py:223-226: the product in
// float32, truncated towards zero) and the block's histogram
__global__ void __launch_bounds__(DS_T) k_ds_ids(const float* __restrict__ xi, const int* __restrict__ lut,
                                                 unsigned char* __restrict__ ids, int* __restrict__ bh, long N) {
  __shared__ int h[DS_KEYS];
  __shared__ int slut[DS_KEYS];
  const int tid = threadIdx.x;
  h[tid] = 0;
  slut[tid] = lut[tid];
  __syncthreads();
  const long base = (long)blockIdx.x * DS_CH;
  for (int r = 0; r < DS_CH / DS_T; ++r) {
    const long p = base + r * DS_T + tid;
    if (p < N) {
      const float f = __fmul_rn(xi[p], 255.0f);
      const int u = f >= 0.f ? (f < 256.f ? (int)f : 255) : 0;
      const int id = slut[u];
      ids[p] = (unsigned char)id;
      atomicAdd(&h[id], 1);
    }
  }
  __syncthreads();
  bh[(long)blockIdx.x * DS_KEYS + tid] = h[tid];
}

// bh[b][k] -> first slot of block b's pixels of expert k; meta = seg[257] (segment offsets), ts[257] (first tile of every
// expert), tile_expert[max_tiles] (-1 behind the last tile)
__global__ void __launch_bounds__(DS_T) k_ds_scan(int* __restrict__ bh, int* __restrict__ meta, int nb, int max_tiles) {
  __shared__ int cnt[DS_KEYS];
  __shared__ int seg[DS_KEYS + 1];
  __shared__ int ts[DS_KEYS + 1];
  const int k = threadIdx.x;
  int run = 0;
  for (int b = 0; b < nb; ++b) {
    const int t = bh[(long)b * DS_KEYS + k];
    bh[(long)b * DS_KEYS + k] = run;
    run += t;
  }
  cnt[k] = run;
  __syncthreads();
  if (k == 0) {
    int s = 0, t = 0;
    for (int i = 0; i < DS_KEYS; ++i) {
      seg[i] = s; ts[i] = t;
      s += cnt[i];
      t += (cnt[i] + DS_NB - 1) / DS_NB;
    }
    seg[DS_KEYS] = s; ts[DS_KEYS] = t;
  }
  __syncthreads();
  const int s0 = seg[k];
  for (int b = 0; b < nb; ++b) bh[(long)b * DS_KEYS + k] += s0;
  meta[k] = seg[k];
  meta[DS_KEYS + 1 + k] = ts[k];
  if (k == 0) { meta[DS_KEYS] = seg[DS_KEYS]; meta[2 * DS_KEYS + 1] = ts[DS_KEYS]; }
  int* te = meta + 2 * (DS_KEYS + 1);
  for (int t = k; t < max_tiles; t += DS_T) {
    int e = -1;
    if (t < ts[DS_KEYS]) {                 // the last expert whose first tile is <= t (empty experts share a start: skip them)
      int lo = 0, hi = DS_KEYS - 1;
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (ts[mid] <= t) lo = mid; else hi = mid - 1;
      }
      e = lo;
    }
    te[t] = e;
  }
}

// the pixels of one block in their own order: slot = start of (block, expert) + pixels of that expert in earlier rounds, in
// earlier waves of this round and in lower lanes of the wave (ballot per distinct expert) -- k_bucket_order's scheme
__global__ void __launch_bounds__(DS_T) k_ds_scatter(const unsigned char* __restrict__ ids, const int* __restrict__ bh,
                                                     int* __restrict__ order, long N) {
  constexpr int NW = DS_T / 64;
  __shared__ int base[DS_KEYS];
  __shared__ int wcnt[NW][DS_KEYS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  base[tid] = bh[(long)blockIdx.x * DS_KEYS + tid];
  for (int w = 0; w < NW; ++w) wcnt[w][tid] = 0;
  __syncthreads();
  const long b0 = (long)blockIdx.x * DS_CH;
  for (int r = 0; r < DS_CH / DS_T; ++r) {
    const long p = b0 + r * DS_T + tid;
    const bool live = p < N;
    const int code = live ? (int)ids[p] : -1;
    int rank = 0;
    unsigned long long todo = __ballot(live);
    while (todo) {
      const int c0 = __shfl(code, __ffsll((long long)todo) - 1);
      const unsigned long long same = __ballot(code == c0);
      if (code == c0) rank = __popcll(same & ((1ull << lane) - 1ull));
      if (lane == 0) wcnt[wave][c0] = __popcll(same);
      todo &= ~same;
    }
    __syncthreads();
    if (live) {
      int before = base[code];
      for (int w = 0; w < wave; ++w) before += wcnt[w][code];
      order[before + rank] = (int)p;
    }
    __syncthreads();
    int t = 0;
    for (int w = 0; w < NW; ++w) { t += wcnt[w][tid]; wcnt[w][tid] = 0; }
    base[tid] += t;
    __syncthreads();
  }
}

// ---------------------------------------------------------------- the expert net on 64 pixels
struct DsPix { int* off; int* y; int* x; };     // LDS: image offset, row, column of the batch's pixels

// layer l for pixel px, outputs o = q + 4 j: _Layer.forward (network_dsr_splines.py:84-93).  q is wave-uniform, so every
// weight address is.  in / out: activation rows [px][DS_AP]; cm (backward only): bit o of cm[l * DS_NB + px] = conv output > 0
template <bool MASK>
__device__ __forceinline__ void ds_layer(const DsNet& L, int l, const float* W, const float* __restrict__ xi, int H, int Wd,
                                         const DsPix& P, const float* in, float* out, unsigned* cm, int px, int q) {
  const int ci = L.ci[l], co = L.co[l];
  const bool match = L.local && L.mw[l] >= 0;
  float acc[8], macc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int o = q + 4 * j;
    acc[j] = o < co ? W[L.b[l] + o] : 0.f;
    macc[j] = (match && o < co) ? W[L.mb[l] + o] : 0.f;
  }
  if (l == 0) {
    const int pad = (L.ks - 1) / 2, kk = L.kk;
    const float* img = xi + P.off[px];
    const int y = P.y[px], x = P.x[px];
    const float* w0 = W + L.w[0];
    for (int ky = 0; ky < L.ks; ++ky) {
      const float* row = img + (long)ds_reflect(y + ky - pad, H) * Wd;
      for (int kx = 0; kx < L.ks; ++kx) {
        const float v = row[ds_reflect(x + kx - pad, Wd)];
        const int tap = ky * L.ks + kx;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int o = q + 4 * j;
          if (o < co) acc[j] = fmaf(v, w0[o * kk + tap], acc[j]);
        }
      }
    }
    if (match) {
      const float xc = img[(long)y * Wd + x];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int o = q + 4 * j;
        if (o < co) macc[j] = fmaf(xc, W[L.mw[0] + o], macc[j]);
      }
    }
  } else {
    const float* wl = W + L.w[l];
    const float* wm = W + (match ? L.mw[l] : 0);
    for (int i = 0; i < ci; ++i) {
      const float v = in[px * DS_AP + i];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int o = q + 4 * j;
        if (o < co) {
          acc[j] = fmaf(v, wl[o * ci + i], acc[j]);
          if (match) macc[j] = fmaf(v, wm[o * ci + i], macc[j]);
        }
      }
    }
  }
  const bool th = L.tanh_out && l == L.nl - 1;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int o = q + 4 * j;
    if (o < co) {
      float s = acc[j];
      if (L.local) {
        const float m = match ? macc[j] : in[px * DS_AP + o];       // identity where the widths agree (l > 0 there)
        if (MASK && s > 0.f) atomicOr(&cm[l * DS_NB + px], 1u << o);
        s = fmaxf(s, 0.f) + m;
      }
      // the backward keeps the tanh's ARGUMENT: 1 - tanh^2 from the rounded output loses everything once it saturates
      out[px * DS_AP + o] = th ? (MASK ? s : tanhf(s)) : fmaxf(s, 0.f);
    }
  }
}

__device__ __forceinline__ void ds_load_pix(const int* __restrict__ order, int first, int nv, int H, int Wd, const DsPix& P,
                                            int* pos, int tid) {
  if (tid < DS_NB) {
    const int p = tid < nv ? order[first + tid] : 0;     // idle rows compute on pixel 0 and are never written out
    const int plane = H * Wd, bi = p / plane, rem = p - bi * plane;
    pos[tid] = tid < nv ? p : -1;
    P.off[tid] = bi * plane;
    P.y[tid] = rem / Wd;
    P.x[tid] = rem - (rem / Wd) * Wd;
  }
}

__global__ void __launch_bounds__(DS_T) k_ds_fwd(const float* __restrict__ xi, const float* __restrict__ table, long stride,
                                                 const int* __restrict__ order, const int* __restrict__ meta,
                                                 float* __restrict__ y, int H, int Wd, DsNet L) {
  extern __shared__ float lds[];
  const int* te = meta + 2 * (DS_KEYS + 1);
  const int t = blockIdx.x, k = te[t];
  if (k < 0) return;
  const int tid = threadIdx.x, px = tid & 63, q = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lt = t - meta[DS_KEYS + 1 + k], seg0 = meta[k], cnt = meta[k + 1] - seg0;
  const int first = seg0 + lt * DS_NB, nv = min(DS_NB, cnt - lt * DS_NB);
  float* Wl = lds;
  float* a0 = Wl + L.P;
  float* a1 = a0 + DS_NB * DS_AP;
  int* pos = (int*)(a1 + DS_NB * DS_AP);
  DsPix P{pos + DS_NB, pos + 2 * DS_NB, pos + 3 * DS_NB};
  const float* src = table + (long)k * stride;
  for (int e = tid; e < L.P; e += DS_T) Wl[e] = src[e];
  ds_load_pix(order, first, nv, H, Wd, P, pos, tid);
  __syncthreads();
  float *in = a1, *out = a0;
  for (int l = 0; l < L.nl; ++l) {
    ds_layer<false>(L, l, Wl, xi, H, Wd, P, in, out, nullptr, px, q);
    __syncthreads();
    float* tmp = in; in = out; out = tmp;
  }
  if (tid < nv) {                                        // `in` holds the last layer's single output
    const int p = pos[tid];
    y[p] = in[tid * DS_AP] + (L.glob ? xi[p] : 0.f);     // + x_interp under use_global_residual (:407-411)
  }
}

// The backward's `wgs` workgroups are dealt to the experts in proportion to the pixels they own, one at least to each of the
// n (microscopy images are mostly dark: the first expert may own nearly everything): ws[k] ... ws[k + 1] are expert k's.
// The deal depends on the segment offsets alone, so the backward and the reduction agree on it and two runs repeat it.
__device__ __forceinline__ void ds_deal(const int* __restrict__ meta, int n, int wgs, int* ws) {
  const int k = threadIdx.x;
  const int cnt = meta[k + 1] - meta[k], N = meta[DS_KEYS];
  ws[k + 1] = k < n ? 1 + (int)(((long)(wgs - n) * cnt) / N) : 0;
  if (k == 0) ws[0] = 0;
  __syncthreads();
  for (int d = 1; d < DS_KEYS; d <<= 1) {
    const int v = k >= d ? ws[k + 1 - d] : 0;
    __syncthreads();
    ws[k + 1] += v;
    __syncthreads();
  }
}

// sum over the batch's pixels, in pixel order, of d[px][o] * input(px, i) for the elements this thread owns
__global__ void __launch_bounds__(DS_T) k_ds_bwd(const float* __restrict__ xi, const float* __restrict__ dy,
                                                 const float* __restrict__ table, long stride, const int* __restrict__ order,
                                                 const int* __restrict__ meta, float* __restrict__ part, int n, int H, int Wd,
                                                 DsNet L) {
  extern __shared__ float lds[];
  __shared__ int ws[DS_KEYS + 1];
  __shared__ int mine;
  const int tid = threadIdx.x, px = tid & 63, q = __builtin_amdgcn_readfirstlane(tid >> 6);
  ds_deal(meta, n, gridDim.x, ws);
  if (tid == 0) mine = -1;
  __syncthreads();
  if (ws[tid] <= (int)blockIdx.x && (int)blockIdx.x < ws[tid + 1]) mine = tid;
  __syncthreads();
  const int k = mine;
  if (k < 0) return;                                     // a workgroup the integer deal left over: nobody reads its table
  const int g = blockIdx.x - ws[k], G = ws[k + 1] - ws[k];
  const int seg0 = meta[k], cnt = meta[k + 1] - seg0;
  const int share = ((cnt + G - 1) / G + DS_NB - 1) / DS_NB * DS_NB;
  const int lo = min(cnt, g * share), hi = min(cnt, lo + share);
  float* acts = lds;                                     // [nl][DS_NB][DS_AP]
  float* da = acts + L.nl * DS_NB * DS_AP;
  float* dsb = da + DS_NB * DS_AP;
  float* dcb = dsb + DS_NB * DS_AP;
  unsigned* cm = (unsigned*)(dcb + DS_NB * DS_AP);       // [nl][DS_NB]
  int* pos = (int*)(cm + L.nl * DS_NB);
  DsPix P{pos + DS_NB, pos + 2 * DS_NB, pos + 3 * DS_NB};
  const float* W = table + (long)k * stride;
  float* pt = part + (long)blockIdx.x * L.P;
  for (int e = tid; e < L.P; e += DS_T) pt[e] = 0.f;
  const int pad = (L.ks - 1) / 2;
  for (int b0 = lo; b0 < hi; b0 += DS_NB) {
    const int nv = min(DS_NB, hi - b0);
    __syncthreads();                                     // the previous batch is done with every buffer
    for (int e = tid; e < L.nl * DS_NB; e += DS_T) cm[e] = 0u;
    ds_load_pix(order, seg0 + b0, nv, H, Wd, P, pos, tid);
    __syncthreads();
    for (int l = 0; l < L.nl; ++l) {
      ds_layer<true>(L, l, W, xi, H, Wd, P, l ? acts + (l - 1) * DS_NB * DS_AP : acts, acts + l * DS_NB * DS_AP, cm, px, q);
      __syncthreads();
    }
    if (tid < DS_NB) da[tid * DS_AP] = tid < nv ? dy[pos[tid]] : 0.f;
    __syncthreads();
    for (int l = L.nl - 1; l >= 0; --l) {
      const int ci = L.ci[l], co = L.co[l];
      const float* al = acts + l * DS_NB * DS_AP;
      const float* ap = acts + (l ? l - 1 : 0) * DS_NB * DS_AP;
      const bool th = L.tanh_out && l == L.nl - 1;
      const bool match = L.local && L.mw[l] >= 0;
      // (a) through the output activation and the ReLU in front of the local residual
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int o = q + 4 * j;
        if (o < co) {
          const float a = al[px * DS_AP + o], d = da[px * DS_AP + o];
          float ds;
          if (th) {                                      // a = the tanh's argument: sech^2(a) = 4 e / (1 + e)^2, e = exp(-2 |a|)
            const float e = expf(-2.f * fabsf(a)), r = 1.f + e;
            ds = d * (4.f * e / (r * r));
          } else {
            ds = a > 0.f ? d : 0.f;
          }
          dsb[px * DS_AP + o] = ds;
          dcb[px * DS_AP + o] = (!L.local || ((cm[l * DS_NB + px] >> o) & 1u)) ? ds : 0.f;
        }
      }
      __syncthreads();
      // (b) parameter gradients of this batch: each element has one owner thread and a fixed pixel order
      const int cik = l == 0 ? L.kk : ci;
      for (int e = tid; e < co * cik; e += DS_T) {
        const int o = e / cik, i = e - o * cik;
        float s = 0.f;
        if (l == 0) {
          const int ky = i / L.ks - pad, kx = i - (i / L.ks) * L.ks - pad;
          for (int p = 0; p < nv; ++p) {
            const float v = xi[P.off[p] + (long)ds_reflect(P.y[p] + ky, H) * Wd + ds_reflect(P.x[p] + kx, Wd)];
            s = fmaf(dcb[p * DS_AP + o], v, s);
          }
        } else {
          for (int p = 0; p < nv; ++p) s = fmaf(dcb[p * DS_AP + o], ap[p * DS_AP + i], s);
        }
        pt[L.w[l] + e] += s;
      }
      for (int e = tid; e < co; e += DS_T) {
        float s = 0.f;
        for (int p = 0; p < nv; ++p) s += dcb[p * DS_AP + e];
        pt[L.b[l] + e] += s;
      }
      if (match) {
        for (int e = tid; e < co * ci; e += DS_T) {
          const int o = e / ci, i = e - o * ci;
          float s = 0.f;
          if (l == 0) {
            for (int p = 0; p < nv; ++p) s = fmaf(dsb[p * DS_AP + o], xi[P.off[p] + (long)P.y[p] * Wd + P.x[p]], s);
          } else {
            for (int p = 0; p < nv; ++p) s = fmaf(dsb[p * DS_AP + o], ap[p * DS_AP + i], s);
          }
          pt[L.mw[l] + e] += s;
        }
        for (int e = tid; e < co; e += DS_T) {
          float s = 0.f;
          for (int p = 0; p < nv; ++p) s += dsb[p * DS_AP + e];
          pt[L.mb[l] + e] += s;
        }
      }
      // (c) gradient of the layer's input (da was consumed by (a))
      if (l > 0) {
        const float* wl = W + L.w[l];
        const float* wm = W + (match ? L.mw[l] : 0);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int i = q + 4 * j;
          if (i < ci) {
            float s = 0.f;
            for (int o = 0; o < co; ++o) s = fmaf(wl[o * ci + i], dcb[px * DS_AP + o], s);
            if (match) {
              for (int o = 0; o < co; ++o) s = fmaf(wm[o * ci + i], dsb[px * DS_AP + o], s);
            } else if (L.local) {
              s += dsb[px * DS_AP + i];
            }
            da[px * DS_AP + i] = s;
          }
        }
      }
      __syncthreads();
    }
  }
}

// grad[k][e] = sum over the expert's workgroups in a fixed order: four strided partial sums, then those in order.  One block
// = 64 elements of one expert.
__global__ void __launch_bounds__(DS_T) k_ds_grad_reduce(const float* __restrict__ part, const int* __restrict__ meta,
                                                         float* __restrict__ grad, long gstride, int wgs, int P, int n) {
  __shared__ int ws[DS_KEYS + 1];
  __shared__ float red[4][64];
  ds_deal(meta, n, wgs, ws);
  const int chunks = (P + 63) / 64;
  const int k = blockIdx.x / chunks, e = (blockIdx.x % chunks) * 64 + (threadIdx.x & 63), gl = threadIdx.x >> 6;
  float s = 0.f;
  if (e < P)
    for (int g = ws[k] + gl; g < ws[k + 1]; g += 4) s += part[(long)g * P + e];
  red[gl][threadIdx.x & 63] = s;
  __syncthreads();
  if (gl == 0 && e < P) grad[(long)k * gstride + e] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// the tensors of every expert <-> the table: one block per tensor
struct DsTensors { int T; int off[4 * DS_MAXL], len[4 * DS_MAXL]; };
__global__ void __launch_bounds__(DS_T) k_ds_pack(const long long* __restrict__ ptrs, float* __restrict__ table, long stride,
                                                  DsTensors D, int to_table) {
  const int t = blockIdx.x % D.T, k = blockIdx.x / D.T;
  float* a = (float*)ptrs[blockIdx.x];
  float* b = table + (long)k * stride + D.off[t];
  for (int e = threadIdx.x; e < D.len[t]; e += DS_T) {
    if (to_table) b[e] = a[e]; else a[e] = b[e];
  }
}

size_t ds_fwd_lds(const DsNet& L) { return ((size_t)L.P + 2 * DS_NB * DS_AP + 4 * DS_NB) * 4; }
size_t ds_bwd_lds(const DsNet& L) { return ((size_t)(L.nl + 3) * DS_NB * DS_AP + (size_t)L.nl * DS_NB + 4 * DS_NB) * 4; }

int ds_groups(const DsNet& L, int n, long part_floats) {
  long G = part_floats / ((long)n * L.P);
  return (int)(G > DS_GMAX ? DS_GMAX : G);
}

}  // namespace

extern "C" {

long srhip_dsr_splines_table_floats(int in_ksz, int n_hidden, int local_residual) {
  DsNet L;
  return ds_make(L, in_ksz, n_hidden, local_residual, 0) ? L.P : -1;
}

int srhip_dsr_splines_order_sizes(long pixels, int n_splines, long* meta_ints, long* hist_ints) {
  SR_REQUIRE(pixels > 0 && pixels < (1L << 31) && n_splines >= 1 && n_splines <= DS_KEYS && meta_ints && hist_ints,
             "dsr_splines_order_sizes: pixels = %ld (< 2^31), n_splines = %d (1 ... 256)", pixels, n_splines);
  *meta_ints = 2 * (DS_KEYS + 1) + sr_cdiv(pixels, DS_NB) + n_splines;
  *hist_ints = (long)sr_cdiv(pixels, DS_CH) * DS_KEYS;
  return 0;
}

int srhip_dsr_splines_order(const float* x_interp, long pixels, const int* level_to_expert, int n_splines,
                            unsigned char* expert_id, int* order, int* meta, int* hist, void* stream) {
  SR_REQUIRE(x_interp && level_to_expert && expert_id && order && meta && hist, "dsr_splines_order: null operand");
  SR_REQUIRE(pixels > 0 && pixels < (1L << 31) && n_splines >= 1 && n_splines <= DS_KEYS,
             "dsr_splines_order: pixels = %ld (< 2^31), n_splines = %d (1 ... 256)", pixels, n_splines);
  hipStream_t st = (hipStream_t)stream;
  const int nb = sr_cdiv(pixels, DS_CH), max_tiles = sr_cdiv(pixels, DS_NB) + n_splines;
  hipLaunchKernelGGL(k_ds_ids, dim3(nb), dim3(DS_T), 0, st, x_interp, level_to_expert, expert_id, hist, pixels);
  hipLaunchKernelGGL(k_ds_scan, dim3(1), dim3(DS_T), 0, st, hist, meta, nb, max_tiles);
  hipLaunchKernelGGL(k_ds_scatter, dim3(nb), dim3(DS_T), 0, st, expert_id, hist, order, pixels);
  SR_LAUNCH_CHECK("dsr_splines_order");
  return 0;
}

static int ds_check(DsNet& L, const char* who, int B, int H, int W, int n_splines, int in_ksz, int n_hidden, int local_residual,
                    int global_residual, long stride) {
  SR_REQUIRE(ds_make(L, in_ksz, n_hidden, local_residual, global_residual),
             "%s: in_ksz = %d (odd, 1 ... 15), %d hidden widths (1 ... 8)", who, in_ksz, n_hidden);
  SR_REQUIRE(B > 0 && H > 0 && W > 0 && (long)B * H * W < (1L << 31) && n_splines >= 1 && n_splines <= DS_KEYS,
             "%s: image %d x %d x %d (< 2^31 pixels), n_splines = %d (1 ... 256)", who, B, H, W, n_splines);
  SR_REQUIRE(H > (in_ksz - 1) / 2 && W > (in_ksz - 1) / 2,
             "%s: reflect padding %d needs image sides above it, got %d x %d", who, (in_ksz - 1) / 2, H, W);
  SR_REQUIRE(stride >= L.P, "%s: table stride %ld below the expert's %d floats", who, stride, L.P);
  return 0;
}

int srhip_dsr_splines_fwd(const float* x_interp, const float* table, long stride, const int* order, const int* meta, float* y,
                          int B, int H, int W, int n_splines, int in_ksz, int n_hidden, int local_residual,
                          int global_residual, void* stream) {
  SR_REQUIRE(x_interp && table && order && meta && y, "dsr_splines_fwd: null operand");
  DsNet L;
  if (int rc = ds_check(L, "dsr_splines_fwd", B, H, W, n_splines, in_ksz, n_hidden, local_residual, global_residual, stride))
    return rc;
  const size_t lds = ds_fwd_lds(L);
  SR_REQUIRE(lds <= 160 * 1024, "dsr_splines_fwd: %zu bytes of LDS", lds);
  static size_t reserved = 0;
  if (lds > reserved) {
    if (hipFuncSetAttribute((const void*)k_ds_fwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
      return sr_fail(-5, "dsr_splines_fwd: cannot reserve %zu bytes of LDS", lds);
    reserved = lds;
  }
  const int tiles = sr_cdiv((long)B * H * W, DS_NB) + n_splines;
  hipLaunchKernelGGL(k_ds_fwd, dim3(tiles), dim3(DS_T), lds, (hipStream_t)stream, x_interp, table, stride, order, meta, y, H, W,
                     L);
  SR_LAUNCH_CHECK("dsr_splines_fwd");
  return 0;
}

long srhip_dsr_splines_bwd_ws(int n_splines, int in_ksz, int n_hidden, int local_residual) {
  DsNet L;
  if (!ds_make(L, in_ksz, n_hidden, local_residual, 0) || n_splines < 1 || n_splines > DS_KEYS) return -1;
  // enough workgroups to fill the device (about 1024) while the partial tables stay within 32 MiB
  long G = 1024 / n_splines;
  const long cap = (8L << 20) / ((long)n_splines * L.P);
  if (G > cap) G = cap;
  if (G > DS_GMAX) G = DS_GMAX;
  if (G < 1) G = 1;
  return G * n_splines * L.P;
}

int srhip_dsr_splines_bwd(const float* x_interp, const float* dy, const float* table, long stride, const int* order,
                          const int* meta, float* grad_table, long grad_stride, float* workspace, long workspace_floats,
                          int B, int H, int W, int n_splines, int in_ksz, int n_hidden, int local_residual,
                          int global_residual, void* stream) {
  SR_REQUIRE(x_interp && dy && table && order && meta && grad_table && workspace, "dsr_splines_bwd: null operand");
  DsNet L;
  if (int rc = ds_check(L, "dsr_splines_bwd", B, H, W, n_splines, in_ksz, n_hidden, local_residual, global_residual, stride))
    return rc;
  SR_REQUIRE(grad_stride >= L.P, "dsr_splines_bwd: gradient table stride %ld below the expert's %d floats", grad_stride, L.P);
  const int G = ds_groups(L, n_splines, workspace_floats);
  SR_REQUIRE(G >= 1, "dsr_splines_bwd: workspace of %ld floats, need srhip_dsr_splines_bwd_ws()", workspace_floats);
  const size_t lds = ds_bwd_lds(L);
  SR_REQUIRE(lds <= 160 * 1024, "dsr_splines_bwd: %zu bytes of LDS", lds);
  static size_t reserved = 0;
  if (lds > reserved) {
    if (hipFuncSetAttribute((const void*)k_ds_bwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
      return sr_fail(-5, "dsr_splines_bwd: cannot reserve %zu bytes of LDS", lds);
    reserved = lds;
  }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_ds_bwd, dim3(n_splines * G), dim3(DS_T), lds, st, x_interp, dy, table, stride, order, meta, workspace,
                     n_splines, H, W, L);
  hipLaunchKernelGGL(k_ds_grad_reduce, dim3(n_splines * sr_cdiv(L.P, 64)), dim3(DS_T), 0, st, workspace, meta, grad_table,
                     grad_stride, n_splines * G, L.P, n_splines);
  SR_LAUNCH_CHECK("dsr_splines_bwd");
  return 0;
}

int srhip_dsr_splines_pack(const long long* tensor_ptrs, float* table, long stride, int n_splines, int in_ksz, int n_hidden,
                           int local_residual, int to_table, void* stream) {
  SR_REQUIRE(tensor_ptrs && table, "dsr_splines_pack: null operand");
  DsNet L;
  SR_REQUIRE(ds_make(L, in_ksz, n_hidden, local_residual, 0) && n_splines >= 1 && n_splines <= DS_KEYS && stride >= L.P,
             "dsr_splines_pack: in_ksz = %d, %d hidden widths, n_splines = %d, stride = %ld", in_ksz, n_hidden, n_splines, stride);
  DsTensors D;
  D.T = 0;
  for (int l = 0; l < L.nl; ++l) {
    D.off[D.T] = L.w[l]; D.len[D.T++] = L.co[l] * L.ci[l] * (l == 0 ? L.kk : 1);
    D.off[D.T] = L.b[l]; D.len[D.T++] = L.co[l];
    if (L.mw[l] >= 0) {
      D.off[D.T] = L.mw[l]; D.len[D.T++] = L.co[l] * L.ci[l];
      D.off[D.T] = L.mb[l]; D.len[D.T++] = L.co[l];
    }
  }
  hipLaunchKernelGGL(k_ds_pack, dim3(n_splines * D.T), dim3(DS_T), 0, (hipStream_t)stream, tensor_ptrs, table, stride, D,
                     to_table);
  SR_LAUNCH_CHECK("dsr_splines_pack");
  return 0;
}

}  // extern "C"
