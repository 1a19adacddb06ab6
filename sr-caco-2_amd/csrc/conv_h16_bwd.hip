// fp16 STORAGE training path of the plain conv family (EDSR under --amp: the reference's autocast + GradScaler step,
// model_plain.py:318-363): the weight and bias gradients of 3x3 convs from fp16 activations and fp16 activation gradients,
// ONE v_mfma_f32_16x16x32_f16 product, f32 accumulate; the 1-channel ends; the fp16 long-skip add; the GradScaler's unscale
// + overflow check.  The data gradients of the body run on k_conv3x3_h16 (conv_h16.hip) with the data-gradient pack.
//
//   k_wgrad_h16        dW[co][ci][t] = sum_p dY[p][co] X[p + d_t][ci], db[co] = sum_p dY[p][co]: a block = one problem x a
//                      64-wide slice of Cout x a 64-wide slice of Cin x a run of 4-row x 32-pixel tiles; the tile's dY rows
//                      and X's halo go straight from global memory into LDS pixel-major (16-byte copies, no split, no
//                      exponent), and both MFMA operands are read back transposed (ds_read_b64_tr_b16): lane (c, g) gets
//                      channel c of the pixels 16 h + 4 g + 0..3 (h = 0, 1) of a 32-pixel row -- for X at the tap's shift.
//                      Wave w owns the 16 input channels 16 w .. of the slice: 4 Cout tiles x 9 taps of accumulators; wave 0
//                      also sums dY against a ones operand (the bias).  Partial sums per run; k_wgrad_h16_reduce adds the
//                      runs in a fixed order (deterministic) into the torch layouts.  ps2: dY is the gradient of the
//                      PixelShuffle(2) OUTPUT [B][2H][2W][Cout/4] (the EDSR upsampler, network_nlsn.py:100-118): kernel
//                      channel sp * (Cout/4) + c = torch channel c * 4 + sp, gathered from the four sub-pixels.
//   k_cin1_wgrad_h16   the 1-channel ends: dW[c][t] = sum_p img[p + d_t] feat[p][c] (+ db[c] = sum_p feat[p][c]) of an f32
//                      image and fp16 features -- the head's weight gradient (image = input, feat = dY) and, with the taps
//                      mirrored, the tail's (image = dy, feat = the tail's input)
//                      accumulate: the reducer ADDS into dW / db (DRRN's weights shared by its U residual units: one launch per
//                      unit, the units in a fixed order -- srhip_conv3x3_wgrad_shared_h16)
//   k_axpby_h16        y = a y + b x on fp16 (f32 arithmetic): the long skip's gradient add
//   k_amp_unscale      g *= inv_scale over the flat gradient; a flag when any |g| >= 65520 (an fp16 gradient of the
//                      reference would be inf) or non-finite before the unscale
#include "common.h"
#include "kernels.h"

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((__vector_size__(4 * sizeof(short))));

namespace {

constexpr int WG_TR = 4;                          // dY rows of a tile
constexpr int WG_TC = 32;                         // dY pixels of a tile row (= one MFMA k step)
constexpr int WG_PP = 160;                        // LDS bytes per pixel: 64 channels (128 B) + 32 pad -> 40 dwords: eight
                                                  // consecutive pixels of a 32-lane half cover the 64 banks once
constexpr int WG_XC = WG_TC + 2;                  // halo pixels of an X row
constexpr int WG_DY_PIX = WG_TR * WG_TC;          // 128
constexpr int WG_X_PIX = (WG_TR + 2) * WG_XC;     // 204
constexpr int WG_DY_IT = WG_DY_PIX * 8 / 256;     // 4 slots of 16 bytes per thread
constexpr int WG_X_IT = (WG_X_PIX * 8 + 255) / 256;   // 7 (the last one partial)
constexpr int WG_LDS = (WG_DY_PIX + WG_X_PIX) * WG_PP;

struct WgradH16Args {
  const _Float16* dY[40];
  const _Float16* X[40];
  float* dW[40];
  float* db[40];
  long lddy, ldx;
  int B, H, W, Cout, Cin, ps2;
  int S, ntiles, tiles_x, tiles_y;
  float* part;                        // [item][S][Cout][9 * Cin + 1]
  long pitem;                         // floats per item
  int accumulate;                     // 1: the reducer adds into dW / db
};

__device__ __forceinline__ f32x4 mfma16(u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h16x8, a), __builtin_bit_cast(h16x8, b), c, 0, 0, 0);
}

// transposed fragment: lane (c, g) gets channel ch0 + c of the pixels pix(16 h + 4 g + q), q = 0..3, h = 0, 1.  Lane 4 q + p of
// a 16-lane group supplies the address of pixel q of its group's four, channels ch0 + 4 p .. + 3
__device__ __forceinline__ u32x4 tr_frag(const unsigned char* img, int pix0, int pix1, int ch0, int p) {
  unsigned r[4];
  const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) s16x4*)(img + pix0 * WG_PP + (ch0 + 4 * p) * 2));
  const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) s16x4*)(img + pix1 * WG_PP + (ch0 + 4 * p) * 2));
  const sr_u32x2 u0 = __builtin_bit_cast(sr_u32x2, v0), u1 = __builtin_bit_cast(sr_u32x2, v1);
  r[0] = u0.x; r[1] = u0.y; r[2] = u1.x; r[3] = u1.y;
  return u32x4{r[0], r[1], r[2], r[3]};
}

__global__ void __launch_bounds__(256, 2) k_wgrad_h16(WgradH16Args p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* const dys = smem;                                  // [128 pixels][WG_PP]
  unsigned char* const xs = smem + WG_DY_PIX * WG_PP;               // [6 rows][34 pixels][WG_PP]
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, g = lane >> 4, q = c >> 2, pq = c & 3;
  const int s = blockIdx.x, item = blockIdx.z;
  const int nco = p.Cout >> 6;
  const int co0 = (blockIdx.y % nco) * 64, ci0 = (blockIdx.y / nco) * 64;
  const _Float16* const dY = p.dY[item];
  const _Float16* const X = p.X[item];
  const int t0 = (int)((long)s * p.ntiles / p.S), t1 = (int)((long)(s + 1) * p.ntiles / p.S);
  // dY channels of the slice: plain co0 .. co0 + 63; ps2: sub-pixel sp of the shuffled image, its channels cc0 ..
  const int fs = p.Cout >> 2, sp = co0 / fs, cc0 = co0 - sp * fs;

  auto tile_geo = [&](int t, int& img, int& y0, int& x0) {
    x0 = (t % p.tiles_x) * WG_TC; t /= p.tiles_x;
    y0 = (t % p.tiles_y) * WG_TR;
    img = t / p.tiles_y;
  };
  u32x4 rd[WG_DY_IT], rx[WG_X_IT];
  auto load = [&](int t) {
    int img, y0, x0;
    tile_geo(t, img, y0, x0);
#pragma unroll
    for (int it = 0; it < WG_DY_IT; ++it) {
      const int idx = tid + it * 256, px = idx >> 3, c8 = idx & 7;
      const int y = y0 + px / WG_TC, x = x0 + px % WG_TC;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (y < p.H && x < p.W) {
        const long off = p.ps2 ? (((long)img * 2 * p.H + 2 * y + (sp >> 1)) * (2 * p.W) + 2 * x + (sp & 1)) * p.lddy + cc0
                               : (((long)img * p.H + y) * p.W + x) * p.lddy + co0;
        v = *(const u32x4*)(dY + off + c8 * 8);
      }
      rd[it] = v;
    }
#pragma unroll
    for (int it = 0; it < WG_X_IT; ++it) {
      const int idx = tid + it * 256, px = idx >> 3, c8 = idx & 7;
      const int y = y0 - 1 + px / WG_XC, x = x0 - 1 + px % WG_XC;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (px < WG_X_PIX && y >= 0 && y < p.H && x >= 0 && x < p.W)
        v = *(const u32x4*)(X + (((long)img * p.H + y) * p.W + x) * p.ldx + ci0 + c8 * 8);
      rx[it] = v;
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int it = 0; it < WG_DY_IT; ++it) {
      const int idx = tid + it * 256;
      *(u32x4*)(dys + (idx >> 3) * WG_PP + (idx & 7) * 16) = rd[it];
    }
#pragma unroll
    for (int it = 0; it < WG_X_IT; ++it) {
      const int idx = tid + it * 256;
      if (idx < WG_X_PIX * 8) *(u32x4*)(xs + (idx >> 3) * WG_PP + (idx & 7) * 16) = rx[it];
    }
  };

  f32x4 acc[4][9], accb[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    accb[m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const _Float16 one = (_Float16)1.f;
  const u32x4 ones = __builtin_bit_cast(u32x4, h16x8{one, one, one, one, one, one, one, one});
  // the lane's pixels of a 32-pixel row: 4 g + q and 16 + 4 g + q
  const int pa = 4 * g + q, pb = 16 + 4 * g + q;
  if (t0 < t1) load(t0);
  for (int t = t0; t < t1; ++t) {
    __syncthreads();                              // the previous tile's images are read
    store();
    __syncthreads();
    if (t + 1 < t1) load(t + 1);                  // travels during the tile's MFMAs
#pragma unroll 1
    for (int r = 0; r < WG_TR; ++r) {
      u32x4 fa[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) fa[m] = tr_frag(dys, r * WG_TC + pa, r * WG_TC + pb, 16 * m, pq);
      if (w == 0) {
#pragma unroll
        for (int m = 0; m < 4; ++m) accb[m] = mfma16(fa[m], ones, accb[m]);
      }
#pragma unroll
      for (int ty = 0; ty < 3; ++ty)
#pragma unroll
        for (int tx = 0; tx < 3; ++tx) {
          const int hb = (r + ty) * WG_XC + tx;
          const u32x4 fb = tr_frag(xs, hb + pa, hb + pb, 16 * w, pq);
#pragma unroll
          for (int m = 0; m < 4; ++m) acc[m][3 * ty + tx] = mfma16(fa[m], fb, acc[m][3 * ty + tx]);
        }
    }
  }
  // partial sums of the run: rows co (kernel order), [9][Cin] then the bias column; acc[m][t][e] = (co 16 m + 4 g + e, ci 16 w + c)
  float* const part = p.part + (long)item * p.pitem + (long)s * p.Cout * (9 * p.Cin + 1);
  const int ld = 9 * p.Cin + 1;
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float* const row = part + (long)(co0 + 16 * m + 4 * g + e) * ld;
#pragma unroll
      for (int t = 0; t < 9; ++t) row[t * p.Cin + ci0 + 16 * w + c] = acc[m][t][e];
      if (w == 0 && c == 0 && ci0 == 0) row[9 * p.Cin] = accb[m][e];
    }
}

// dW[co][ci][t] (torch) = sum over the runs s = 0 .. S-1 in order; db[co] the same over the bias column.  ps2: kernel row
// sp * (Cout/4) + c is torch channel c * 4 + sp.
__global__ void __launch_bounds__(256) k_wgrad_h16_reduce(WgradH16Args p) {
  const int item = blockIdx.y;
  const long ld = 9L * p.Cin + 1, n = (long)p.Cout * ld;
  const float* const part = p.part + (long)item * p.pitem;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int row = (int)(i / ld), k = (int)(i - (long)row * ld);
    float v = 0.f;
    for (int s = 0; s < p.S; ++s) v += part[(long)s * n + i];
    int co = row;
    if (p.ps2) { const int fs = p.Cout >> 2, sp = row / fs; co = (row - sp * fs) * 4 + sp; }
    float* dst = nullptr;
    if (k == 9 * p.Cin) {
      if (p.db[item]) dst = p.db[item] + co;
    } else {
      const int t = k / p.Cin, ci = k - t * p.Cin;
      dst = p.dW[item] + ((long)co * p.Cin + ci) * 9 + t;
    }
    if (dst) *dst = p.accumulate ? *dst + v : v;
  }
}

// 1-channel ends: a block = a run of pixels; a thread = (pixel lane, 8-channel group), 10 x 8 sums in registers, reduced over
// the wave's pixel lanes by shuffles and over the four waves through LDS; partials [block][10][C] (taps 0..8, then the feature
// sum), k_cin1_wgrad_h16_reduce adds the blocks in order.
__global__ void __launch_bounds__(256) k_cin1_wgrad_h16(const float* __restrict__ img, const _Float16* __restrict__ feat,
                                                         long ldf, int B, int H, int W, int C, int flip,
                                                         float* __restrict__ part) {
  extern __shared__ float red[];                  // [4 waves][10][C]
  const int G = C >> 3;                           // 8-channel groups: a power of two <= 32 (C in 8, 16, .., 256)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int gq = lane % G, pl = wv * (64 / G) + lane / G, npl = 4 * (64 / G);
  const long n = (long)B * H * W;
  float a[10][8];
#pragma unroll
  for (int t = 0; t < 10; ++t)
#pragma unroll
    for (int e = 0; e < 8; ++e) a[t][e] = 0.f;
  for (long pix = (long)blockIdx.x * npl + pl; pix < n; pix += (long)gridDim.x * npl) {
    const int xx = (int)(pix % W);
    const long rr = pix / W;
    const int yy = (int)(rr % H);
    const long b = rr / H;
    const h16x8 f = *(const h16x8*)(feat + pix * ldf + gq * 8);
    float fv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { fv[e] = (float)f[e]; a[9][e] += fv[e]; }
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int tt = flip ? 8 - t : t;
      const int sy = yy + tt / 3 - 1, sx = xx + tt % 3 - 1;
      const float iv = (sy >= 0 && sy < H && sx >= 0 && sx < W) ? img[(b * H + sy) * W + sx] : 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) a[t][e] += iv * fv[e];
    }
  }
#pragma unroll
  for (int t = 0; t < 10; ++t)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float v = a[t][e];
      for (int o = G; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
      if (lane < G) red[(wv * 10 + t) * C + gq * 8 + e] = v;
    }
  __syncthreads();
  for (int i = threadIdx.x; i < 10 * C; i += 256)
    part[(long)blockIdx.x * 10 * C + i] = red[i] + red[10 * C + i] + red[20 * C + i] + red[30 * C + i];
}

__global__ void __launch_bounds__(256) k_cin1_wgrad_h16_reduce(const float* __restrict__ part, int nblk, int C, int flip,
                                                                float* __restrict__ dw, float* __restrict__ db) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 10 * C) return;
  float v = 0.f;
  for (int b = 0; b < nblk; ++b) v += part[(long)b * 10 * C + i];
  const int t = i / C, ch = i - t * C;
  if (t == 9) { if (db) db[ch] = v; }
  else dw[ch * 9 + t] = v;                        // [C][1][3][3] or [1][C][3][3]: the same bytes
  (void)flip;
}

__global__ void __launch_bounds__(256) k_axpby_h16(_Float16* __restrict__ y, const _Float16* __restrict__ x, long n8, float a,
                                                    float b) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
    h16x8 yv = *(const h16x8*)(y + i * 8);
    const h16x8 xv = *(const h16x8*)(x + i * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) yv[e] = (_Float16)(a * (float)yv[e] + b * (float)xv[e]);
    *(h16x8*)(y + i * 8) = yv;
  }
}

__global__ void __launch_bounds__(256) k_amp_unscale(float* __restrict__ g, long n, float inv_scale, int* __restrict__ flag) {
  bool bad = false;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float v = g[i];
    bad |= !(fabsf(v) < 65520.f);                 // NaN fails the comparison too
    g[i] = v * inv_scale;
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

}  // namespace

int srhip_conv3x3_wgrad_h16_plan(int n, int B, int H, int W, int Cout, int Cin, int ps2, int* S, long* part_floats_per_item) {
  SR_REQUIRE(n >= 1 && n <= 40, "conv3x3_wgrad_h16_plan: 1..40 problems (got %d)", n);
  SR_REQUIRE(B > 0 && H > 0 && W > 0 && Cout % 64 == 0 && Cin % 64 == 0 && Cout <= 4096 && Cin <= 4096 &&
             (!ps2 || Cout % 256 == 0),
             "conv3x3_wgrad_h16_plan: Cout = %d, Cin = %d (multiples of 64; ps2: Cout of 256)", Cout, Cin);
  const long ntiles = (long)B * sr_cdiv(H, WG_TR) * sr_cdiv(W, WG_TC);
  const long slices = (long)n * (Cout / 64) * (Cin / 64);
  // ~4 blocks per CU over the 256 CUs, at least two tiles a run, at most 16 runs: every run is a partial tile of
  // Cout x (9 Cin + 1) floats written and read back (one run per block for the upsampler's 256 x 64 problem was 151 MB and a
  // 0.5-ms reducer of the x8 step's 5.5 ms)
  long s = (1024 + slices - 1) / slices;
  if (s > ntiles / 2) s = ntiles / 2;
  if (s > 16) s = 16;
  if (s < 1) s = 1;
  *S = (int)s;
  *part_floats_per_item = s * Cout * (9L * Cin + 1);
  return 0;
}

static int sr_wgrad_h16_launch(const srhip_conv_wgrad_h16_item* items, int n, long lddy, long ldx, int B, int H, int W,
                               int Cout, int Cin, int ps2, float* part, int S, int accumulate, hipStream_t st);

int srhip_conv3x3_wgrad_h16(const srhip_conv_wgrad_h16_item* items, int n, long lddy, long ldx, int B, int H, int W, int Cout,
                            int Cin, int ps2, float* part, int S, void* stream) {
  return sr_wgrad_h16_launch(items, n, lddy, ldx, B, H, W, Cout, Cin, ps2, part, S, 0, (hipStream_t)stream);
}

static int sr_wgrad_h16_launch(const srhip_conv_wgrad_h16_item* items, int n, long lddy, long ldx, int B, int H, int W,
                               int Cout, int Cin, int ps2, float* part, int S, int accumulate, hipStream_t st) {
  SR_REQUIRE(n >= 1 && n <= 40 && items && part && S >= 1, "conv3x3_wgrad_h16: 1..40 problems, workspace, S >= 1");
  SR_REQUIRE(B > 0 && H > 0 && W > 0 && Cout % 64 == 0 && Cin % 64 == 0 && Cout <= 4096 && Cin <= 4096 &&
             (!ps2 || Cout % 256 == 0),
             "conv3x3_wgrad_h16: Cout = %d, Cin = %d (multiples of 64; ps2: Cout of 256)", Cout, Cin);
  SR_REQUIRE(lddy % 8 == 0 && ldx % 8 == 0 && lddy >= (ps2 ? Cout / 4 : Cout) && ldx >= Cin,
             "conv3x3_wgrad_h16: pixel pitches (multiples of 8 halves, >= the channels)");
  WgradH16Args p;
  memset(&p, 0, sizeof(p));
  for (int k = 0; k < n; ++k) {
    SR_REQUIRE(items[k].dY && items[k].X && items[k].dW, "conv3x3_wgrad_h16: item %d has a NULL pointer", k);
    p.dY[k] = (const _Float16*)items[k].dY; p.X[k] = (const _Float16*)items[k].X; p.dW[k] = items[k].dW; p.db[k] = items[k].db;
  }
  p.lddy = lddy; p.ldx = ldx; p.B = B; p.H = H; p.W = W; p.Cout = Cout; p.Cin = Cin; p.ps2 = ps2 ? 1 : 0;
  p.tiles_x = sr_cdiv(W, WG_TC); p.tiles_y = sr_cdiv(H, WG_TR);
  p.ntiles = B * p.tiles_y * p.tiles_x;
  p.S = S; p.part = part;
  p.pitem = (long)S * Cout * (9L * Cin + 1);
  p.accumulate = accumulate;
  hipLaunchKernelGGL(k_wgrad_h16, dim3(S, (Cout / 64) * (Cin / 64), n), dim3(256), WG_LDS, st, p);
  SR_LAUNCH_CHECK("k_wgrad_h16");
  const long outs = (long)Cout * (9L * Cin + 1);
  const int gx = (int)((outs + 255) / 256);
  hipLaunchKernelGGL(k_wgrad_h16_reduce, dim3(gx, n), dim3(256), 0, st, p);
  SR_LAUNCH_CHECK("k_wgrad_h16_reduce");
  return 0;
}

long srhip_conv3x3_cin1_wgrad_h16_ws(int C) { return 256L * 10 * C; }

int srhip_conv3x3_cin1_wgrad_h16(const float* img, const void* feat, long ldf, float* dw, float* db, float* ws, int B, int H,
                                 int W, int C, int flip, void* stream) {
  SR_REQUIRE(img && feat && dw && ws, "conv3x3_cin1_wgrad_h16: null operand");
  SR_REQUIRE(C % 8 == 0 && C >= 8 && C <= 256 && ((C / 8) & (C / 8 - 1)) == 0 && ldf % 8 == 0, "conv3x3_cin1_wgrad_h16: C = %d (8 times a power of two, <= 256)", C);
  const long n = (long)B * H * W;
  SR_REQUIRE(n > 0, "conv3x3_cin1_wgrad_h16: empty image");
  const int npl = 4 * (64 / (C / 8));
  const int nblk = (int)((n + npl - 1) / npl < 256 ? (n + npl - 1) / npl : 256);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_cin1_wgrad_h16, dim3(nblk), dim3(256), (size_t)4 * 10 * C * 4, st, img, (const _Float16*)feat, ldf, B,
                     H, W, C, flip, ws);
  SR_LAUNCH_CHECK("k_cin1_wgrad_h16");
  hipLaunchKernelGGL(k_cin1_wgrad_h16_reduce, dim3(sr_cdiv(10L * C, 256)), dim3(256), 0, st, ws, nblk, C, flip, dw, db);
  SR_LAUNCH_CHECK("k_cin1_wgrad_h16_reduce");
  return 0;
}

int srhip_conv3x3_cin1_h16_flip(const float* x, const float* w, void* y, long ldy, int B, int H, int W, int Co, void* stream) {
  return sr_conv_cin1_h16(x, w, nullptr, y, ldy, B, H, W, Co, 0, 0.f, (hipStream_t)stream, 1);
}

int srhip_axpby_h16(void* y, const void* x, long n, float a, float b, void* stream) {
  SR_REQUIRE(y && x && n % 8 == 0, "axpby_h16: null operand or n = %ld not a multiple of 8", n);
  if (n == 0) return 0;
  const long n8 = n / 8;
  const int grid = (int)(n8 / 256 + 1 < 4096 ? n8 / 256 + 1 : 4096);
  hipLaunchKernelGGL(k_axpby_h16, dim3(grid), dim3(256), 0, (hipStream_t)stream, (_Float16*)y, (const _Float16*)x, n8, a, b);
  SR_LAUNCH_CHECK("k_axpby_h16");
  return 0;
}

int srhip_amp_unscale_check(float* g, long n, float inv_scale, int* overflow_flag, void* stream) {
  SR_REQUIRE(g && overflow_flag && n >= 0, "amp_unscale_check: null operand");
  if (n == 0) return 0;
  const int grid = (int)(n / 1024 + 1 < 2048 ? n / 1024 + 1 : 2048);
  hipLaunchKernelGGL(k_amp_unscale, dim3(grid), dim3(256), 0, (hipStream_t)stream, g, n, inv_scale, overflow_flag);
  SR_LAUNCH_CHECK("k_amp_unscale");
  return 0;
}

int srhip_conv3x3_ps2_bwd_data_h16(const void* dYup, long lddy, const void* Wht, void* dX, long ldx, int B, int H, int W,
                                   int Cout, int Cin, void* stream) {
  ConvH16Args p;
  memset(&p, 0, sizeof(p));
  p.X = (const _Float16*)dYup; p.ldx = lddy; p.Wb = (const unsigned short*)Wht; p.Y = (_Float16*)dX; p.ldy = ldx;
  p.B = B; p.H = H; p.Wd = W; p.K = Cout; p.N = Cin; p.ps_in = 1; p.alpha = 1.f;
  return sr_conv3x3_h16(p, (hipStream_t)stream);
}

// ---- DRRN under --amp: the recursion's shared weights and its identity gradient (network_drrn.py:22-126 under autocast,
// model_plain.py:322-348)

int srhip_conv3x3_wgrad_shared_h16_plan(int n, int B, int H, int W, int Cout, int Cin, int* S, long* part_floats_per_item) {
  SR_REQUIRE(n >= 1 && n <= 40 && S && part_floats_per_item, "conv3x3_wgrad_shared_h16_plan: 1..40 problems (got %d)", n);
  SR_REQUIRE(B > 0 && H > 0 && W > 0 && Cout % 64 == 0 && Cin % 64 == 0 && Cout <= 4096 && Cin <= 4096,
             "conv3x3_wgrad_shared_h16_plan: Cout = %d, Cin = %d (multiples of 64)", Cout, Cin);
  // a launch is ONE application (two problems for DRRN's unit: 2 x 2 x 2 slices of 128 x 128): the runs alone fill the
  // GPU -- ~2 blocks per CU (k_wgrad_h16 fits two), at least two tiles a run, at most 64 runs
  const long ntiles = (long)B * sr_cdiv(H, WG_TR) * sr_cdiv(W, WG_TC);
  const long slices = (long)n * (Cout / 64) * (Cin / 64);
  long s = (512 + slices - 1) / slices;
  if (s > ntiles / 2) s = ntiles / 2;
  if (s > 64) s = 64;
  if (s < 1) s = 1;
  *S = (int)s;
  *part_floats_per_item = s * Cout * (9L * Cin + 1);
  return 0;
}

int srhip_conv3x3_wgrad_shared_h16(const srhip_conv_wgrad_h16_item* items, int n, long lddy, long ldx, int B, int H, int W,
                                   int Cout, int Cin, float* part, int S, int accumulate, void* stream) {
  SR_REQUIRE(n >= 1 && n <= 40 && items && part && S >= 1 && S <= 64, "conv3x3_wgrad_shared_h16: 1..40 problems, workspace, S 1..64");
  SR_REQUIRE(B > 0 && H > 0 && W > 0 && Cout % 64 == 0 && Cin % 64 == 0 && Cout <= 4096 && Cin <= 4096,
             "conv3x3_wgrad_shared_h16: Cout = %d, Cin = %d (multiples of 64)", Cout, Cin);
  SR_REQUIRE(lddy % 8 == 0 && ldx % 8 == 0 && lddy >= Cout && ldx >= Cin,
             "conv3x3_wgrad_shared_h16: pixel pitches (multiples of 8 halves, >= the channels)");
  // the reducers of a launch run concurrently and read the operands of every problem: no output may overlap another output,
  // an operand or the workspace (ranges, not base pointers)
  const long pix = (long)B * H * W;
  const long bw = (long)Cout * Cin * 9 * 4, bb = (long)Cout * 4;
  const long bpart = (long)n * S * Cout * (9L * Cin + 1) * 4;
  for (int k = 0; k < n; ++k) {
    SR_REQUIRE(items[k].dY && items[k].X && items[k].dW, "conv3x3_wgrad_shared_h16: item %d has a NULL pointer", k);
    SR_REQUIRE(sr_disjoint(items[k].dW, bw, items[k].db, bb), "conv3x3_wgrad_shared_h16: item %d: dW overlaps db", k);
    SR_REQUIRE(sr_disjoint(items[k].dW, bw, part, bpart) && sr_disjoint(items[k].db, bb, part, bpart),
               "conv3x3_wgrad_shared_h16: item %d: an output overlaps the workspace", k);
    for (int j = 0; j < n; ++j) {
      const long by = sr_map_bytes(pix, lddy, Cout, 2), bx = sr_map_bytes(pix, ldx, Cin, 2);
      SR_REQUIRE(sr_disjoint(items[k].dW, bw, items[j].dY, by) && sr_disjoint(items[k].dW, bw, items[j].X, bx) &&
                 sr_disjoint(items[k].db, bb, items[j].dY, by) && sr_disjoint(items[k].db, bb, items[j].X, bx),
                 "conv3x3_wgrad_shared_h16: an output of item %d overlaps an operand of item %d", k, j);
      if (j != k)
        SR_REQUIRE(sr_disjoint(items[k].dW, bw, items[j].dW, bw) && sr_disjoint(items[k].dW, bw, items[j].db, bb) &&
                   sr_disjoint(items[k].db, bb, items[j].db, bb),
                   "conv3x3_wgrad_shared_h16: items %d and %d share an output (one launch per application)", k, j);
    }
  }
  return sr_wgrad_h16_launch(items, n, lddy, ldx, B, H, W, Cout, Cin, 0, part, S, accumulate ? 1 : 0, (hipStream_t)stream);
}

int srhip_conv3x3_dgrad_relu_acc_h16(const void* dY, long lddy, const void* Wht, const void* R, long ldr, void* dX, long lddx,
                                     float* G, long ldg, int B, int H, int W, int Cout, int Cin, int mode, void* stream) {
  SR_REQUIRE(dY && Wht && R && dX && G, "conv3x3_dgrad_relu_acc_h16: null operand");
  SR_REQUIRE(mode == 0 || mode == 1, "conv3x3_dgrad_relu_acc_h16: mode %d (0 accumulate into G, 1 add G)", mode);
  SR_REQUIRE(B > 0 && H > 0 && W > 0 && lddy >= Cout && ldr >= Cin && lddx >= Cin && ldg >= Cin,
             "conv3x3_dgrad_relu_acc_h16: shape / pitches");
  // dX is written while other tiles still read dY's halo and the epilogue reads R and G; G is read-modify-written
  const long pix = (long)B * H * W;
  const long by = sr_map_bytes(pix, lddy, Cout, 2), br = sr_map_bytes(pix, ldr, Cin, 2);
  const long bx = sr_map_bytes(pix, lddx, Cin, 2), bg = sr_map_bytes(pix, ldg, Cin, 4);
  SR_REQUIRE(sr_disjoint(dX, bx, dY, by) && sr_disjoint(dX, bx, R, br) && sr_disjoint(dX, bx, G, bg),
             "conv3x3_dgrad_relu_acc_h16: dX overlaps dY, R or G");
  SR_REQUIRE(sr_disjoint(G, bg, dY, by) && sr_disjoint(G, bg, R, br), "conv3x3_dgrad_relu_acc_h16: G overlaps dY or R");
  ConvH16Args p;
  memset(&p, 0, sizeof(p));
  p.X = (const _Float16*)dY; p.ldx = lddy; p.Wb = (const unsigned short*)Wht; p.Y = (_Float16*)dX; p.ldy = lddx;
  p.R = (const _Float16*)R; p.ldr = ldr; p.G = G; p.ldg = ldg; p.epi = mode ? 11 : 10; p.alpha = 1.f;
  p.B = B; p.H = H; p.Wd = W; p.K = Cout; p.N = Cin;
  return sr_conv3x3_h16(p, (hipStream_t)stream);
}

int srhip_conv3x3_cin1_h16_flip_mask(const float* x, const float* w, const void* R, long ldr, void* y, long ldy, float* G,
                                     long ldg, int B, int H, int W, int Co, void* stream) {
  SR_REQUIRE(x && w && R && y, "conv3x3_cin1_h16_flip_mask: null operand");
  SR_REQUIRE(B > 0 && H > 0 && W > 0 && ldr >= Co && ldy >= Co && (!G || ldg >= Co),
             "conv3x3_cin1_h16_flip_mask: shape / pitches (>= the %d channels)", Co);
  const long pix = (long)B * H * W;
  const long by = sr_map_bytes(pix, ldy, Co, 2), br = sr_map_bytes(pix, ldr, Co, 2), bg = sr_map_bytes(pix, ldg, Co, 4);
  const long bxi = pix * 4, bw = 9L * Co * 4;
  SR_REQUIRE(sr_disjoint(y, by, R, br) && sr_disjoint(y, by, x, bxi) && sr_disjoint(y, by, w, bw) && sr_disjoint(y, by, G, bg),
             "conv3x3_cin1_h16_flip_mask: y overlaps an input or G");
  SR_REQUIRE(sr_disjoint(G, bg, R, br) && sr_disjoint(G, bg, x, bxi) && sr_disjoint(G, bg, w, bw),
             "conv3x3_cin1_h16_flip_mask: G overlaps an input");
  return sr_conv_cin1_h16(x, w, nullptr, y, ldy, B, H, W, Co, 0, 0.f, (hipStream_t)stream, 1, (const _Float16*)R, ldr, G,
                          ldg);
}
