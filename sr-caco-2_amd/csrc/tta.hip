// The test modes of dlib/utils/utils_model.py:51-214 (test_pad, test_split, test_x8, test_split_x8) as two launches around
// batched forwards.  The reference slices, rotates, pads and stitches on the host around one forward per view or tile;
// here
//   * srhip_view_gather makes every tile of one output shape in one launch: rectangle -> dihedral view (augment_img_tensor4,
//     dlib/utils/utils_image.py:490-508) -> replicate padding right / bottom (ReplicationPad2d((0, pr, 0, pb)) of test_pad),
//   * srhip_view_merge builds the result in one launch, pull form: one thread per destination pixel walks the K views in
//     the order 0 .. K-1, maps the pixel into each view's frame, descends the split's quadtree to the one tile that owns it
//     (the hard crops of test_split_fn, :160-163) and adds that tile's pixel.  No atomics, no reductions across threads.
// Both are index arithmetic plus copies (and, in the merge, K f32 additions in a fixed order and one multiplication).
#include "common.h"

namespace {

constexpr int VT = 64;          // a block makes a VT x VT tile of the output
constexpr int VLD = VT + 1;     // LDS leading dimension: padded by one b32 access, so that the column read of the transposing
                                // views is conflict-free (leading dimension 64: 64 cycles per wave read; 65: 2)

// Source position inside an h x w rectangle R for position (i, j) of view m of it, V = augment_img_tensor4(R, m)
// (torch.rot90 turns counter-clockwise; flip([2]) reverses the rows).  Views 1, 3, 5, 7 are w x h.
//   0 R[i][j]        1 R[j][i]        2 R[h-1-i][j]       3 R[h-1-j][i]
//   4 R[i][w-1-j]    5 R[j][w-1-i]    6 R[h-1-i][w-1-j]   7 R[h-1-j][w-1-i]
__device__ __forceinline__ void view_src(int m, int i, int j, int h, int w, int& si, int& sj) {
  const int a = (m & 1) ? j : i, b = (m & 1) ? i : j;          // a walks R's rows, b its columns
  si = (m == 2 || m == 3 || m == 6 || m == 7) ? h - 1 - a : a;
  sj = (m >= 4) ? w - 1 - b : b;
}

// VEC: out is 16-byte aligned and tw a multiple of 4, so that four consecutive output pixels are one 16-byte store.
template <bool VEC>
__global__ __launch_bounds__(256) void k_view_gather(const float* __restrict__ src, int H, int W,
                                                     const srhip_view_job* __restrict__ jobs, float* __restrict__ out,
                                                     int th, int tw) {
  __shared__ float tile[VT * VLD];
  const srhip_view_job J = jobs[blockIdx.z];
  // the host checked its copy of the table; a table that differs from it must not send a load outside the image
  if (J.y0 < 0 || J.x0 < 0 || J.h <= 0 || J.w <= 0 || J.y0 + J.h > H || J.x0 + J.w > W || (unsigned)J.mode > 7u) return;
  const int n = blockIdx.y, N = gridDim.y;
  const int tiles_j = (tw + VT - 1) / VT;
  const int i0 = (blockIdx.x / tiles_j) * VT, j0 = (blockIdx.x % tiles_j) * VT;
  const float* R = src + ((long)n * H + J.y0) * W + J.x0;       // the rectangle's first pixel; rows W apart
  float* o = out + ((long)blockIdx.z * N + n) * th * tw;
  const int m = J.mode, h = J.h, w = J.w;
  const int vh = (m & 1) ? w : h, vw = (m & 1) ? h : w;         // the view's size; beyond it: replicate its last row / column
  const int t = threadIdx.x;
  if (vh > th || vw > tw) return;

  if (m & 1) {
    // transposing views: output (i, j) reads R[a(j)][b(i)].  Load with the lanes along R's columns (= the output's rows),
    // one source row per wave and step, into tile[jj][ii]; then read column-wise with the lanes along the output's columns.
    const int lane = t & 63, wv = t >> 6;
    const int ic = min(i0 + lane, vh - 1);
    for (int jj = wv; jj < VT; jj += 4) {
      if (j0 + jj >= tw) break;
      const int jc = min(j0 + jj, vw - 1);
      int si, sj;
      view_src(m, ic, jc, h, w, si, sj);
      tile[jj * VLD + lane] = ldg_f(R + (long)si * W + sj);
    }
    __syncthreads();
    for (int ii = wv; ii < VT; ii += 4) {
      const int i = i0 + ii, j = j0 + lane;
      if (i < th && j < tw) o[(long)i * tw + j] = tile[lane * VLD + ii];
    }
    return;
  }

  // views 0, 2, 4, 6: row copies, forwards or backwards
  if (VEC) {
    const int jq = j0 + (t & 15) * 4;                            // four consecutive output columns
    for (int ii = t >> 4; ii < VT; ii += 16) {
      const int i = i0 + ii;
      if (i >= th || jq >= tw) break;
      int si, s0, s3;
      view_src(m, min(i, vh - 1), min(jq, vw - 1), h, w, si, s0);
      view_src(m, min(i, vh - 1), min(jq + 3, vw - 1), h, w, si, s3);
      const float* row = R + (long)si * W;
      f32x4 v;
      if (jq + 3 < vw && (((uintptr_t)(row + min(s0, s3))) & 15) == 0) {       // the widest aligned access there is
        const f32x4 u = ldg_f4(row + min(s0, s3));
        v = s0 <= s3 ? u : f32x4{u.w, u.z, u.y, u.x};
      } else {
        int s1, s2;
        view_src(m, min(i, vh - 1), min(jq + 1, vw - 1), h, w, si, s1);
        view_src(m, min(i, vh - 1), min(jq + 2, vw - 1), h, w, si, s2);
        v = f32x4{ldg_f(row + s0), ldg_f(row + s1), ldg_f(row + s2), ldg_f(row + s3)};
      }
      *(f32x4*)(o + (long)i * tw + jq) = v;
    }
  } else {
    const int j = j0 + (t & 63);
    for (int ii = t >> 6; ii < VT; ii += 4) {
      const int i = i0 + ii;
      if (i >= th || j >= tw) break;
      int si, sj;
      view_src(m, min(i, vh - 1), min(j, vw - 1), h, w, si, sj);
      o[(long)i * tw + j] = ldg_f(R + (long)si * W + sj);
    }
  }
}

// One thread per destination pixel, 16 x 16 pixels per block: a transposing view reads its tiles along the other axis, and a
// square block gives both kinds of view 64-byte runs.
__global__ __launch_bounds__(256) void k_view_merge(const srhip_view_desc* __restrict__ views, int K, float* __restrict__ dst,
                                                    int N, int H, int W, int sf, float inv_k) {
  const int X = blockIdx.x * 16 + (threadIdx.x & 15), Y = blockIdx.y * 16 + (threadIdx.x >> 4);
  const int n = blockIdx.z;
  const int HS = H * sf, WS = W * sf;
  if (X >= WS || Y >= HS) return;
  float acc = 0.f;
  for (int k = 0; k < K; ++k) {
    const srhip_view_desc& V = views[k];
    const int m = V.mode;
    const int inv = m == 3 ? 5 : m == 5 ? 3 : m;               // test_x8: mode = 8 - i for i = 3, 5; the others are involutions
    // result = augment_img_tensor4(E_k, inv): the h x w "rectangle" is view k's assembled output, the "view" the destination
    int y, x;
    view_src(inv, Y, X, V.h[0] * sf, V.w[0] * sf, y, x);
    long idx = 0;
    for (int l = 0; l < V.depth; ++l) {                        // test_split_fn :146-163: top / left own [0, side // 2)
      const int hl = V.h[l], wl = V.w[l], qh = V.h[l + 1], qw = V.w[l + 1];
      int q = 0;
      if (y >= (hl / 2) * sf) { y -= (hl - qh) * sf; q = 2; }
      if (x >= (wl / 2) * sf) { x -= (wl - qw) * sf; q |= 1; }
      idx = idx * 4 + q;
    }
    const long ths = (long)V.th * sf, tws = (long)V.tw * sf;
    acc += ldg_f(V.tiles + ((idx * N + n) * ths + y) * tws + x);
  }
  dst[((long)n * HS + Y) * WS + X] = acc * inv_k;
}

// the pointer names device (or managed) memory
bool on_device(const void* p) {
  hipPointerAttribute_t a;
  memset(&a, 0, sizeof(a));
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();                                    // a plain host pointer: not an error of a later launch
    return false;
  }
  return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

}  // namespace

extern "C" {

/* out[job][n][th][tw] = pad(view_mode(src[n][y0 : y0 + h][x0 : x0 + w])) (include/srhip.h) */
int srhip_view_gather(const float* src, int N, int H, int W, const srhip_view_job* jobs_dev, const srhip_view_job* jobs_host,
                      int njobs, float* out, int th, int tw, void* stream) {
  SR_REQUIRE(src && jobs_dev && jobs_host && out, "view_gather: NULL argument");
  SR_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0, "view_gather: 1 <= planes <= 65535, H, W > 0 (got %d, %d, %d)", N, H, W);
  SR_REQUIRE(njobs > 0 && njobs <= 65535, "view_gather: 1 <= jobs <= 65535 (got %d)", njobs);
  SR_REQUIRE(th > 0 && tw > 0, "view_gather: th, tw > 0 (got %d, %d)", th, tw);
  SR_REQUIRE(on_device(jobs_dev), "view_gather: the job table must be on the device");
  for (int q = 0; q < njobs; ++q) {
    const srhip_view_job& j = jobs_host[q];
    SR_REQUIRE(j.mode >= 0 && j.mode <= 7, "view_gather: job %d: mode 0..7 (got %d)", q, j.mode);
    SR_REQUIRE(j.h > 0 && j.w > 0 && j.y0 >= 0 && j.x0 >= 0 && (long)j.y0 + j.h <= H && (long)j.x0 + j.w <= W,
               "view_gather: job %d: rectangle (%d, %d) + (%d, %d) leaves the %d x %d image", q, j.y0, j.x0, j.h, j.w, H, W);
    const int vh = (j.mode & 1) ? j.w : j.h, vw = (j.mode & 1) ? j.h : j.w;
    SR_REQUIRE(th >= vh && tw >= vw, "view_gather: job %d: its view is %d x %d, larger than the tile %d x %d", q, vh, vw, th, tw);
  }
  const long tiles = (long)sr_cdiv(th, VT) * sr_cdiv(tw, VT);
  SR_REQUIRE(tiles <= 0x7fffffffL, "view_gather: tile too large (%d x %d)", th, tw);
  SR_REQUIRE(sr_disjoint(src, (long)N * H * W * 4, out, (long)njobs * N * th * tw * 4), "view_gather: out overlaps src");
  const dim3 grid((unsigned)tiles, (unsigned)N, (unsigned)njobs);
  const bool vec = (((uintptr_t)out) & 15) == 0 && tw % 4 == 0;
  if (vec)
    hipLaunchKernelGGL(k_view_gather<true>, grid, dim3(256), 0, (hipStream_t)stream, src, H, W, jobs_dev, out, th, tw);
  else
    hipLaunchKernelGGL(k_view_gather<false>, grid, dim3(256), 0, (hipStream_t)stream, src, H, W, jobs_dev, out, th, tw);
  SR_LAUNCH_CHECK("view_gather");
  return 0;
}

/* dst[n][sf H][sf W] = (1 / K) sum_k inverse_view_k(assembled tiles of view k) (include/srhip.h) */
int srhip_view_merge(const srhip_view_desc* views_dev, const srhip_view_desc* views_host, int K, float* dst, int N, int H,
                     int W, int sf, void* stream) {
  SR_REQUIRE(views_dev && views_host && dst, "view_merge: NULL argument");
  SR_REQUIRE(K >= 1 && K <= 8, "view_merge: 1 <= K <= 8 views (got %d)", K);
  SR_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0 && sf >= 1, "view_merge: 1 <= planes <= 65535, H, W > 0, sf >= 1");
  SR_REQUIRE((long)H * sf <= 0x7fffffffL / 2 && (long)W * sf <= 0x7fffffffL / 2, "view_merge: image too large");
  SR_REQUIRE(on_device(views_dev), "view_merge: the view table must be on the device");
  const long dst_bytes = (long)N * H * sf * W * sf * 4;
  for (int k = 0; k < K; ++k) {
    const srhip_view_desc& v = views_host[k];
    SR_REQUIRE(v.tiles, "view_merge: view %d: NULL tiles", k);
    SR_REQUIRE(v.mode >= 0 && v.mode <= 7, "view_merge: view %d: mode 0..7 (got %d)", k, v.mode);
    SR_REQUIRE(v.depth >= 0 && v.depth <= 8, "view_merge: view %d: depth 0..8 (got %d)", k, v.depth);
    const int fh = (v.mode & 1) ? W : H, fw = (v.mode & 1) ? H : W;
    SR_REQUIRE(v.h[0] == fh && v.w[0] == fw, "view_merge: view %d (mode %d): its frame is %d x %d, the image's view %d x %d", k,
               v.mode, v.h[0], v.w[0], fh, fw);
    for (int l = 0; l < v.depth; ++l) {
      // a quadrant lies inside its level and reaches the half it owns: no owned pixel falls outside a tile
      SR_REQUIRE(v.h[l + 1] > 0 && v.h[l + 1] <= v.h[l] && v.h[l + 1] >= v.h[l] - v.h[l] / 2 && v.w[l + 1] > 0 &&
                     v.w[l + 1] <= v.w[l] && v.w[l + 1] >= v.w[l] - v.w[l] / 2,
                 "view_merge: view %d: level %d quadrants %d x %d do not cover the halves of %d x %d", k, l, v.h[l + 1],
                 v.w[l + 1], v.h[l], v.w[l]);
    }
    SR_REQUIRE(v.th >= v.h[v.depth] && v.tw >= v.w[v.depth], "view_merge: view %d: tile %d x %d smaller than its leaf %d x %d", k,
               v.th, v.tw, v.h[v.depth], v.w[v.depth]);
    const long tile_bytes = ((long)N << (2 * v.depth)) * v.th * sf * v.tw * sf * 4;
    SR_REQUIRE(sr_disjoint(dst, dst_bytes, v.tiles, tile_bytes), "view_merge: dst overlaps the tiles of view %d", k);
  }
  const dim3 grid((unsigned)sr_cdiv((long)W * sf, 16), (unsigned)sr_cdiv((long)H * sf, 16), (unsigned)N);
  SR_REQUIRE(grid.y <= 65535u, "view_merge: more than 65535 * 16 rows");
  hipLaunchKernelGGL(k_view_merge, grid, dim3(256), 0, (hipStream_t)stream, views_dev, K, dst, N, H, W, sf, 1.0f / (float)K);
  SR_LAUNCH_CHECK("view_merge");
  return 0;
}

}  // extern "C"
