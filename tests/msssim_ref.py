"""The statement and the inputs of the multi-scale SSIM tests (srhip_metrics_msssim_lv, dlib.metrics.sweep(msssim=...), --msssim).

tests/test_cpu_msssim.py checks the statement itself; tests/test_gpu_msssim.py gates the kernel against it.  Both import it from here.

The statement (include/srhip.h carries the same text; nothing in the reference computes it).  a, b: [B, 1, H, W] images at L, float
tensors that hold the integer levels 0 .. L (deep_metric_cases.q_levels makes them); M scales, 1 .. 5.
  1. crop by border on every side; x = level / L
  2. scale 1 is that pair; scale j + 1 = F.avg_pool2d(scale j, 2, padding=(h % 2, w % 2)): an odd extent gets one zero row / column
     in front, the zero counts in the divisor 4, the new extent is ceil(h / 2)
  3. every scale: the 11 x 11 sigma 1.5 window of deep_metric_cases.ssim_map at valid positions, C1 = 1e-4, C2 = 9e-4,
     cs = (2 sxy + C2) / (sxx + syy + C2), ss = (2 mx my + C1) / (mx^2 + my^2 + C1) * cs; v_j = mean(cs) for j < M, v_M = mean(ss)
  4. MS-SSIM = prod_j max(v_j, 0)^w_j, 0^w = 0, w the first M of WEIGHTS (Wang, Simoncelli, Bovik 2003), divided by their sum if M < 5
  5. both cropped sides are at least min_side(M) = 10 * 2^(M - 1) + 1
msssim(..., dtype) runs every operation in ``dtype``: float64 is the reference of the gates, float32 the plain float32 statement
whose distance from it scales them."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import sr_oracle as O
import step_kernel_cases as C
import deep_metric_cases as D

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
C1, C2 = 0.01 ** 2, 0.03 ** 2


def weights(M):
    assert 1 <= M <= 5, M
    w = WEIGHTS[:M]
    return w if M == 5 else tuple(v / sum(w) for v in w)


def min_side(M, border=0):
    return 10 * 2 ** (M - 1) + 1 + 2 * border


def pool(x):
    """the next scale of [B, 1, h, w]"""
    h, w = x.shape[-2:]
    return F.avg_pool2d(x, 2, padding=(h % 2, w % 2))


def cs_ss_maps(x, y, k):
    """(cs_map, ss_map) [B, 1, h - 10, w - 10] of one scale; k the [1, 1, 11, 11] window in the dtype of x"""
    blur = lambda t: F.conv2d(t, k)
    mx, my = blur(x), blur(y)
    sxx, syy, sxy = blur(x ** 2) - mx ** 2, blur(y ** 2) - my ** 2, blur(x * y) - mx * my
    cs = (2.0 * sxy + C2) / (sxx + syy + C2)
    return cs, ((2.0 * mx * my + C1) / (mx ** 2 + my ** 2 + C1)) * cs


def window(dtype, as_kernel=False):
    """the statement's window: the reference's float32 2-D Gaussian normalised in 2-D (deep_metric_cases.ssim_map); as_kernel:
    the outer product of the kernel's separable float32 taps, which differs from it in the eighth digit"""
    if as_kernel:
        g = torch.from_numpy(D.kernel_taps().astype(np.float64))
        return (g[:, None] * g[None, :])[None, None].to(dtype)
    return O.gaussian_window_2d_metric()[None, None].to(dtype)


def msssim(a, b, L, border=0, M=5, dtype=torch.float64, as_kernel=False):
    """[B, 1 + M] in ``dtype``: MS-SSIM, then the unclamped v_1 .. v_M"""
    x, y = O._crop(a, border).to(dtype) / float(L), O._crop(b, border).to(dtype) / float(L)
    h, w = x.shape[-2:]
    if min(h, w) < min_side(M):
        raise ValueError(f"msssim: {M} scales need both cropped sides to be at least {min_side(M)} (got {h} x {w})")
    k = window(dtype, as_kernel)
    n = x.shape[0]
    v = []
    for j in range(M):
        cs, ss = cs_ss_maps(x, y, k)
        v.append((ss if j == M - 1 else cs).reshape(n, -1).mean(-1))
        if j < M - 1:
            x, y = pool(x), pool(y)
    v = torch.stack(v, 1)
    wt = torch.tensor(weights(M), dtype=dtype)
    return torch.cat([torch.pow(v.clamp(min=0.0), wt).prod(1, keepdim=True), v], 1)


# ------------------------------------------------------------------ inputs
# (B, h, w, border, M, L), h x w after the crop: the smallest shapes at which the kernel can go wrong
CASES = ((3, 161, 163, 0, 5, 255),        # the minimum size; odd extents at scales 1 - 4; several tiles
         (2, 177, 179, 8, 5, 65535),      # border crop; full depth
         (3, 21, 24, 0, 2, 255),          # a small image, two scales
         (2, 45, 47, 2, 3, 4095),         # border crop, three scales
         (2, 11, 11, 0, 1, 255))          # one map pixel


def smooth_field(n, H, W, g):
    """a uniform field under a 5 x 5 box mean, [n, 1, H, W] float32 in [0, 1]"""
    return F.avg_pool2d(torch.rand(n, 1, H + 4, W + 4, generator=g), 5, stride=1)


@functools.lru_cache(maxsize=None)
def inputs(B, h, w, border, L):
    """(E, Hf, a, b) [B, 1, h + 2 border, w + 2 border]: the target a 5 x 5-smoothed uniform field, the prediction the target plus
    N(0, 0.05); image 0 is identical to its target; where B = 3, image 2 is 1 - H.  a = Q_L(prediction), b = Q_L(target) hold the
    levels; E = unit(a), Hf = unit(b) are the float images on the L grid, whose levels are a and b again."""
    H, W = h + 2 * border, w + 2 * border
    g = C.gen(2003 + 7 * h + w + border + L % 1000)
    t = smooth_field(B, H, W, g)
    p = t + 0.05 * torch.randn(B, 1, H, W, generator=g)
    p[0] = t[0]
    if B == 3:
        p[2] = 1.0 - t[2]
    a, b = D.t_q(p, L), D.t_q(t, L)
    E, Hf = D.t_unit(a, L), D.t_unit(b, L)
    assert torch.equal(D.t_q(E, L), a) and torch.equal(D.t_q(Hf, L), b)
    return E, Hf, a, b


@functools.lru_cache(maxsize=None)
def constant_pair(h, w, border, L):
    """(a, b) at L, B = 2: both images one constant (the same, then two different ones): every variance is 0, cs = 1"""
    H, W = h + 2 * border, w + 2 * border
    a = torch.stack([torch.full((1, H, W), 0.25), torch.full((1, H, W), 0.75)])
    b = torch.stack([torch.full((1, H, W), 0.25), torch.full((1, H, W), 0.5)])
    return D.t_q(a, L), D.t_q(b, L)


@functools.lru_cache(maxsize=None)
def expect(B, h, w, border, M, L):
    """(ref64, ref32) [B, 1 + M] of inputs(B, h, w, border, L)"""
    _, _, a, b = inputs(B, h, w, border, L)
    return msssim(a, b, L, border, M, torch.float64), msssim(a, b, L, border, M, torch.float32)
