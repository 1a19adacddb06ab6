"""Metric entry points under their reference module path
(dlib/utils/utils_image.py); implementation in dlib.metrics."""
from dlib.metrics import (tensor2uint82float, mbatch_gpu_calculate_psnr,  # noqa: F401
                          mbatch_gpu_calculate_mse, mbatch_gpu_calculate_nrmse,
                          mbatch_gpu_calculate_ssim)


# ----------------------------------------------------------------------------------------------
# MATLAB-style bicubic imresize (the reference's utils_image.py:1358-1422 cubic / calculate_weights_indices,
# :1505-1578 imresize_np): the low-resolution image of a pair that has a high-resolution tile only
# (dataset_dpsr.py:798-824).  Our own numpy restatement; the CPU path of EvalPairs and the yardstick of
# srhip_imresize_aa, which evaluates the very same expressions in the same order.
# ----------------------------------------------------------------------------------------------
import math

import numpy as np


def _cubic(x: np.ndarray) -> np.ndarray:
    """Keys' cubic convolution kernel, a = -0.5, support [-2, 2]."""
    a = np.abs(x)
    a2 = a * a
    a3 = a2 * a
    near = 1.5 * a3 - 2.5 * a2 + 1.0
    far = -0.5 * a3 + 2.5 * a2 - 4.0 * a + 2.0
    return np.where(a <= 1.0, near, np.where(a <= 2.0, far, 0.0))


def imresize_weights(n_in: int, n_out: int, scale: float, antialiasing: bool = True):
    """Per output pixel of one axis: normalised float64 weights [n_out, P] and the 0-based source indices [n_out, P] of
    its taps, mirrored about the borders with the edge pixel repeated.  An index outside [0, n_in) belongs to a tap that
    lies more than n_in pixels beyond a border; imresize_np refuses it unless its weight is zero."""
    scale = float(scale)
    shrink = scale < 1 and antialiasing
    width = 4.0 / scale if shrink else 4.0
    x = np.arange(1, n_out + 1, dtype=np.float64)
    u = x / scale + 0.5 * (1.0 - 1.0 / scale)           # 1-based input coordinate of every output pixel
    left = np.floor(u - width / 2.0)
    taps = math.ceil(width) + 2
    idx = left[:, None] + np.arange(taps, dtype=np.float64)[None, :]        # 1-based
    dist = u[:, None] - idx
    w = scale * _cubic(dist * scale) if shrink else _cubic(dist)
    total = np.zeros(n_out, dtype=np.float64)
    for k in range(taps):                               # the sum in tap order, as the device kernel forms it
        total = total + w[:, k]
    w = w / total[:, None]
    j = idx.astype(np.int64) - 1
    j = np.where(j < 0, -j - 1, np.where(j >= n_in, 2 * n_in - 1 - j, j))
    return w, j


def _resample_axis0(img: np.ndarray, w: np.ndarray, j: np.ndarray) -> np.ndarray:
    """out[o] = sum_k w[o, k] * img[j[o, k]] in float64, taps in order, rounded once to float32."""
    n_in = img.shape[0]
    live = w != 0.0
    if np.any(live & ((j < 0) | (j >= n_in))):
        raise ValueError(f'imresize_np: {n_in} pixels are too few for this scale: a tap would mirror past the opposite border')
    j = np.clip(j, 0, n_in - 1)
    acc = np.zeros((w.shape[0],) + img.shape[1:], dtype=np.float64)
    tail = (1,) * (img.ndim - 1)
    for k in range(w.shape[1]):
        acc = acc + w[:, k].reshape((-1,) + tail) * np.where(live[:, k].reshape((-1,) + tail), img[j[:, k]].astype(np.float64), 0.0)
    return acc.astype(np.float32)


def imresize_np(img: np.ndarray, scale: float, antialiasing: bool = True) -> np.ndarray:
    """The reference's ``util.imresize_np``: img float HW or HWC in [0, 1] -> float32 (ceil(H * scale), ceil(W * scale)[, C]),
    not rounded to grey levels and not clipped (a sharp edge overshoots [0, 1]).  Rows first, then columns, the image in
    between rounded to float32 as the reference stores it; weights, coordinates and sums in float64 (the reference forms
    them in float32: its outputs sit within one float32 ulp of these, golden g51)."""
    img = np.asarray(img)
    assert img.ndim in (2, 3), img.shape
    x = img.astype(np.float32)
    h, w = x.shape[:2]
    oh, ow = math.ceil(h * scale), math.ceil(w * scale)
    wy, jy = imresize_weights(h, oh, scale, antialiasing)
    wx, jx = imresize_weights(w, ow, scale, antialiasing)
    rows = _resample_axis0(x, wy, jy)                                   # (oh, W[, C]) float32
    cols = _resample_axis0(np.swapaxes(rows, 0, 1), wx, jx)             # (ow, oh[, C])
    return np.ascontiguousarray(np.swapaxes(cols, 0, 1))
