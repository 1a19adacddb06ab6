"""Statements and inputs of the full-depth metric tests (srhip_tensor2levels, srhip_metrics_psnr_family_lv,
srhip_metrics_ssim_lv, dlib.metrics.sweep(levels=...), --metric_levels).

tests/test_cpu_deep_metrics.py checks the statements themselves (at L = 255 they are the oracle's metrics) and the arithmetic the
SSIM kernel uses; tests/test_gpu_deep_metrics.py gates the kernels against the same statements.  Both import them from here.

L is the number of the white level, 255 .. 65535.  An image `at L` is a float tensor that holds the integer levels 0 .. L.
  Q_L(x)   = clamp(rint_half_even(float32(clamp(x, 0, 1)) * float32(L)), 0, L), ONE float32 product (q_levels)
  unit(v)  = np.float32(v / L), the quotient in double, rounded once (unit_of_levels' rule)
  ROI of threshold th = Q_255(unit(target level)) >= th: defined at the 8-bit levels whatever L is (level8)
  metrics  = float64 arithmetic on the integer levels: MSE in levels^2, PSNR = 20 log10(L / sqrt(max(mse, 1e-45))), PSNR_Y on
             L * clamp((219 v / L + 16) / 255, 0, 1), NRMSE with the reference's ymax / lo / den == 0 -> 1 rules, SSIM on v / L with
             the reference's 11 x 11 window, C1 = 1e-4, C2 = 9e-4."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import sr_oracle as O
import step_kernel_cases as C

LEVELS = (4095, 65535)
ROUND_TRIP_LEVELS = (255, 257, 1023, 4095, 12345, 65534, 65535)
LEVELS_N = C.CAP + 77                              # past the grid cap of the element-wise kernels


# ------------------------------------------------------------------ Q_L, unit, the 8-bit level
def q_levels(x, L):
    """Q_L of a float array, in numpy: float32 [same shape] holding the levels"""
    c = np.clip(np.asarray(x, dtype=np.float32), np.float32(0), np.float32(1))
    p = c * np.float32(L)
    assert p.dtype == np.float32
    return np.clip(np.rint(p), 0, L).astype(np.float32)          # np.rint rounds half to even


def unit(v, L):
    """np.float32(v / L): the float image of an image at L"""
    return np.float32(np.asarray(v, dtype=np.float64) / float(L))


def level8(v, L):
    """the 8-bit level of a level at L"""
    return q_levels(unit(v, L), 255)


def t_q(x, L):
    return torch.from_numpy(q_levels(x.numpy(), L))


def t_unit(v, L):
    return torch.from_numpy(unit(v.numpy(), L))


def t_level8(v, L):
    return torch.from_numpy(level8(v.numpy(), L))


@functools.lru_cache(maxsize=None)
def levels_inputs(L):
    """(x [LEVELS_N], number of ties): values below 0 and above 1, -0.0, exact half-way products, then generic values in
    [-0.1, 1.1].  float32((k + 0.5) / L) * L need not round to k + 0.5, so a tie is looked for among that float and its two
    neighbours, for the first 600 k and 600 more spread up to L: those whose float32 product with L IS k + 0.5 are kept."""
    g = C.gen(1500 + L % 1000)
    x = (torch.rand(LEVELS_N, generator=g) * 1.2 - 0.1).numpy()
    special = [-0.0, -0.3, 1.7, 0.0, 1.0, -1e-9, 1 + 1e-6]
    ks = np.unique(np.concatenate([np.arange(0, min(L, 600)), np.linspace(0, L - 1, 600).astype(np.int64)]))
    ties = []
    for k in ks:
        c = np.float32((k + 0.5) / L)
        for cand in (np.nextafter(c, np.float32(0)), c, np.nextafter(c, np.float32(2))):
            if np.float32(cand) * np.float32(L) == np.float32(k + 0.5):
                ties.append(float(cand))
    sp = np.array(special + ties, dtype=np.float32)
    x[:sp.size] = sp
    return torch.from_numpy(x), len(ties)


# ------------------------------------------------------------------ the four metrics at L, float64
def roi_of(b, L, th, dtype=torch.float64):
    return (t_level8(b, L) >= th).to(dtype)


def _masked_mse(a, b, border, roi):
    a, b, roi = O._crop(a, border).double(), O._crop(b, border).double(), O._crop(roi, border)
    n = a.shape[0]
    if roi is None:
        return ((a - b) ** 2).reshape(n, -1).mean(-1)
    cnt = roi.reshape(n, -1).sum(-1)
    cnt[cnt == 0] = 1.0
    return (((a - b) * roi) ** 2).reshape(n, -1).sum(-1) / cnt


def mse_lv(a, b, L, border=0, th=None):
    """MSE in levels^2; [B] float64"""
    return _masked_mse(a, b, border, None if th is None else roi_of(b, L, th))


def _psnr(mse, L):
    mse = torch.where(mse < 1e-45, torch.full_like(mse, 1e-45), mse)
    return 20.0 * torch.log10(float(L) / torch.sqrt(mse))


def psnr_lv(a, b, L, border=0, th=None):
    return _psnr(mse_lv(a, b, L, border, th), L)


def y_lv(v, L):
    """the reference's Y of a grey image (65.481 + 128.553 + 24.966 = 219), in levels: L * clamp((219 v / L + 16) / 255, 0, 1)"""
    return float(L) * ((219.0 * v.double() / float(L) + 16.0) / 255.0).clamp(0.0, 1.0)


def psnr_y_lv(a, b, L, border=0, th=None):
    return _psnr(_masked_mse(y_lv(a, L), y_lv(b, L), border, None if th is None else roi_of(b, L, th)), L)


def nrmse_lv(a, b, L, border=0, th=None):
    mse = mse_lv(a, b, L, border, th)
    y = O._crop(b, border).double()
    n = y.shape[0]
    if th is None:
        yy = y.reshape(n, -1)
        lo = yy.min(-1)[0]
    else:
        yy = (y * O._crop(roi_of(b, L, th), border)).reshape(n, -1)
        lo = torch.maximum(y.reshape(n, -1).min(-1)[0], yy.min(-1)[0])
    den = yy.max(-1)[0] - lo
    den[den == 0] = 1.0
    return torch.sqrt(mse) / den


def ssim_map(a, b, L, border=0, dtype=torch.float64):
    """the SSIM map [B, 1, h - 10, w - 10] of the cropped images, every operation in ``dtype`` (float32: the plain float32
    statement, sigma^2 = E[x^2] - E[x]^2 as the 8-bit kernel and the reference compute it)"""
    x, y = O._crop(a, border).to(dtype) / float(L), O._crop(b, border).to(dtype) / float(L)
    k = O.gaussian_window_2d_metric()[None, None].to(dtype)
    blur = lambda t: F.conv2d(t, k)
    mx, my = blur(x), blur(y)
    sxx, syy, sxy = blur(x ** 2) - mx ** 2, blur(y ** 2) - my ** 2, blur(x * y) - mx * my
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    return ((2.0 * mx * my + c1) / (mx ** 2 + my ** 2 + c1)) * ((2.0 * sxy + c2) / (sxx + syy + c2))


def _mean_of_map(ss, b, L, border, th):
    n = ss.shape[0]
    if th is None:
        return ss.reshape(n, -1).mean(-1)
    r = O._crop(roi_of(b, L, th, ss.dtype), border)
    r = r[:, :, 5:r.shape[2] - 5, 5:r.shape[3] - 5]
    cnt = r.reshape(n, -1).sum(-1)
    cnt[cnt == 0] = 1.0
    return (ss * r).reshape(n, -1).sum(-1) / cnt


def ssim_lv(a, b, L, border=0, th=None, dtype=torch.float64):
    """[B] in ``dtype``: the per-image mean of ssim_map (over the ROI cropped by the border, then by 5; an empty ROI: 0 / 1)"""
    return _mean_of_map(ssim_map(a, b, L, border, dtype), b, L, border, th)


def kernel_taps():
    """gaussian_taps(11, true) of ssim.hip: float32 exp, float32 sum in index order, float32 quotient"""
    d = np.arange(11, dtype=np.float32) - np.float32(5)
    g = np.exp(-(d * d) / np.float32(2 * 1.5 * 1.5)).astype(np.float32)
    s = np.float32(0)
    for v in g:
        s = np.float32(s + v)
    return (g / s).astype(np.float32)


def ssim_map_as_kernel(a, b, L, border=0):
    """what k_ssim_metric_lv computes, in numpy: float64 throughout on the integer levels, but with the SEPARABLE float32 taps
    of the 8-bit kernel (rows first), and the moments scaled by 1 / L and 1 / L^2 after the two passes.  It differs from
    ssim_map(float64) by the window alone: the reference's window is the float32 2-D Gaussian normalised in 2-D."""
    x, y = O._crop(a, border).double().numpy()[:, 0], O._crop(b, border).double().numpy()[:, 0]
    g = kernel_taps().astype(np.float64)

    def blur(t):
        w = t.shape[2] - 10
        hp = sum(g[k] * t[:, :, k:k + w] for k in range(11))
        h = t.shape[1] - 10
        return sum(g[k] * hp[:, k:k + h] for k in range(11))
    iL = 1.0 / float(L)
    mx, my = blur(x) * iL, blur(y) * iL
    exx, eyy, exy = blur(x * x) * (iL * iL), blur(y * y) * (iL * iL), blur(x * y) * (iL * iL)
    sxx, syy, sxy = exx - mx * mx, eyy - my * my, exy - mx * my
    c1, c2 = 0.01 * 0.01, 0.03 * 0.03
    ss = ((2.0 * mx * my + c1) / (mx * mx + my * my + c1)) * ((2.0 * sxy + c2) / (sxx + syy + c2))
    return torch.from_numpy(ss)[:, None]


def ssim_as_kernel(a, b, L, border=0, th=None):
    return _mean_of_map(ssim_map_as_kernel(a, b, L, border), b, L, border, th)


# ------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def psnr_inputs(H, W, border, L):
    """the images of step_kernel_cases.metric_psnr_inputs at L levels: (pr, hr_f, a, b) with pr the float prediction as it is
    (off the grid, beyond [0, 1]), b = Q_L(hr) the target at L, hr_f = unit(b) the float target ON the L grid (so the float and
    the levels form of the target have one ROI), a = Q_L(pr).  The 8-bit level of b is the 8-bit target of the 8-bit cases, so
    they survive: image 1 is pred == target, image 2 is constant with its 8-bit level at 64."""
    pr, hr, _, b8 = C.metric_psnr_inputs(H, W, border)
    b = t_q(hr, L)
    assert torch.equal(t_level8(b, L), b8)
    return pr, t_unit(b, L), t_q(pr, L), b


# The 11 x 11 case is ONE output pixel and the float32 statement's error there a sample of one: of the bases 1700 .. 1759 this is
# the first at which that sample is above 1.5e-4 under every border and L of the tests (test_cpu_deep_metrics.py asserts > 5e-5).
BRIGHT_SEED = 1703


def bright_smooth(h, w, border, L, seed):
    """(a, b) at L, [1, 1, H, W]: the target is 0.97 + 0.02 x / W plus 0.002 N(0, 1), the prediction the target plus
    0.004 N(0, 1), both clamped and quantised to L: the variances are 1e-5 beside means of 0.98, which float32 cannot subtract"""
    H, W = h + 2 * border, w + 2 * border
    g = C.gen(seed)
    t = 0.97 + 0.02 * torch.arange(W).float()[None, None, None, :] / W + 0.002 * torch.randn(1, 1, H, W, generator=g)
    p = t + 0.004 * torch.randn(1, 1, H, W, generator=g)
    return t_q(p, L), t_q(t, L)


@functools.lru_cache(maxsize=None)
def ssim_inputs(h, w, border, L):
    """B = 4 at L: the three step targets of step_kernel_cases.metric_ssim_inputs under their noisy predictions, rescaled to L
    levels, then one bright-smooth pair.  (E, Hf, a, b): E = unit(a), Hf = unit(b) the float images on the L grid."""
    pr, hr, _, b8 = C.metric_ssim_inputs(h, w, border)
    a3, b3 = t_q(pr, L), t_q(hr, L)
    assert torch.equal(t_level8(b3, L), b8)
    a1, b1 = bright_smooth(h, w, border, L, BRIGHT_SEED + h * w + border)
    a, b = torch.cat([a3, a1]), torch.cat([b3, b1])
    return t_unit(a, L), t_unit(b, L), a, b


def ssim_expect(h, w, border, L):
    """(ref64, ref32) [4, 1 + 8]: slot 0 no ROI, then METRIC_SSIM_THS, the statement in float64 and in plain float32"""
    _, _, a, b = ssim_inputs(h, w, border, L)
    cols = [[ssim_lv(a, b, L, border, th, dt) for th in (None,) + C.METRIC_SSIM_THS] for dt in (torch.float64, torch.float32)]
    return torch.stack(cols[0], 1), torch.stack(cols[1], 1)


def psnr_expect(H, W, border, nth, L):
    """[4, 1 + nth, 4] float64 = PSNR, PSNR_Y, MSE, NRMSE at L"""
    _, _, a, b = psnr_inputs(H, W, border, L)
    out = torch.empty(4, 1 + nth, 4, dtype=torch.float64)
    for k, th in enumerate((None,) + C.METRIC_PSNR_THS[:nth]):
        out[:, k, 0], out[:, k, 1] = psnr_lv(a, b, L, border, th), psnr_y_lv(a, b, L, border, th)
        out[:, k, 2], out[:, k, 3] = mse_lv(a, b, L, border, th), nrmse_lv(a, b, L, border, th)
    return out
