"""The low-resolution side of the reference's dataset items (dlib/datasets/dataset_dpsr.py): what surrounds the
patch-level hot path on the data side.

Host functions -- numpy / torch on the CPU, run once per tile at dataset construction or per sample on patches of a few
hundred pixels, with the reference's own random-number streams so that a seeded run draws what the reference draws:
  interpolate_torch       :684-710   LR = uint8(clamp(F.interpolate(HR, 1/s, bicubic)))  (the synthesised LR of sets
                                      without true LR tiles)
  simulate_low_res        :713-744   + seeded Gaussian noise inside the cells' region (CACO-2)
  per_color_weights       :592-645   --ppiw: one loss weight per grey level from the HR histogram of the split
  da_blur / da_dot_bin_noise / da_add_gaus_noise   :1071-1180   the LR-only augmentations on a random block
  otsu_threshold                     skimage.filters.threshold_otsu on a uint8 image (the 'automatic_threshold' ROI style;
                                      skimage is not in this image: restated, parity unpinned)
  otsu_from_counts                   the same from a histogram (srhip_hist_u8's counts of a resident tile)
  (the LR image of an HR-only pair -- :798-824, util.imresize_np -- is dlib.utils.utils_image.imresize_np on the host and
   srhip_imresize_aa on the device; it stays float32: EvalPairs.low_res_f32, ResidentTrainSet)
  psf_bin_weights / psf_bin_np / photon_noise_np   --lr_synth psf (not a reference option): the camera model of the LR image of
                                      an HR-only pair in numpy, the statement of srhip_psf_bin / srhip_photon_noise and the
                                      host path of EvalPairs.low_res_f32
Device functions (libsrhip):
  l_to_h                  :659-683   cv2.resize(INTER_CUBIC) of the LR image to the HR size: srhip_resize_cubic
  per_pixel_weight        :1037-1056 weight image of an HR patch: a lookup of the per-colour table
"""
import math

import numpy as np
import torch
import torch.nn.functional as F


def is_caco2(path: str) -> bool:
    """utils_image.py:202-208"""
    return ('caco2' in path) and any(c in path for c in ('CELL0', 'CELL1', 'CELL2'))


def interpolate_torch(x: np.ndarray, scale: float, mode: str = 'bicubic', min_v: float = 0.0, max_v: float = 255.) -> np.ndarray:
    """dataset_dpsr.py:684-710: x uint8 HWC -> uint8 (int(H*scale), int(W*scale), C); the float result is clamped and
    TRUNCATED by astype (not rounded)."""
    assert isinstance(x, np.ndarray) and x.dtype == np.uint8 and x.ndim == 3 and x.shape[-1] in (1, 3), (x.dtype, x.shape)
    v = torch.from_numpy(x).float().permute(2, 0, 1)
    c, h, w = v.shape
    out = F.interpolate(v.unsqueeze(0), size=(int(h * scale), int(w * scale)), mode=mode).squeeze(0)
    out = torch.clamp(out, min=min_v, max=max_v)
    return out.permute(1, 2, 0).numpy().astype(x.dtype)


def simulate_low_res(x: np.ndarray, seed: int, th: float, sigma: float, min_v: float = 0.0, max_v: float = 255.) -> np.ndarray:
    """dataset_dpsr.py:713-744: Gaussian noise N(v, sigma) on the pixels >= th (the cells), seeded per image index with the
    reference's set_seed (utils_reproducibility.py:89-115)."""
    assert sigma >= 0.0 and isinstance(sigma, float) and th >= 0 and isinstance(th, float)
    assert isinstance(x, np.ndarray) and x.ndim == 3 and x.shape[-1] in (1, 3)
    v = torch.from_numpy(x).float()
    roi = (v >= th).float()
    # The reference runs this inside a DataLoader worker and re-seeds the worker's GLOBAL generators (torch, numpy, random)
    # with the item index; here the call happens in the main process (resident sets are built up front), where that would
    # leave every rank's numpy / random streams at the last tile's index and perturb whatever is drawn next (patch
    # samplers, LR augmentations, DropPath).  The only draw below is torch.normal: a private generator seeded with the
    # index yields the very stream the re-seeded default generator would (golden g31), and touches nothing global.
    gen = torch.Generator()
    gen.manual_seed(seed)
    new_low = torch.normal(mean=v, std=sigma, generator=gen)
    new_low = torch.clamp(new_low, 0.0, 255.)
    new_low = new_low * roi + (1 - roi) * v
    new_low = torch.clamp(new_low, min=min_v, max=max_v)
    return new_low.numpy().astype(x.dtype)


def per_color_weights(hr_images, color_min: int, color_max: int, min_w: float) -> np.ndarray:
    """dataset_dpsr.py:592-645: hr_images = iterable of uint8 [H, W] tiles of the training split -> (nbr_colors,) weights in
    [min_w, 1], rarest grey level heaviest."""
    nbr = len(list(range(color_min, color_max))) + 1
    full = 1.
    for img in hr_images:
        full = np.histogram(img, bins=nbr, range=(color_min, color_max), density=False)[0] + full
    full = nbr * full / float(full.sum())
    w = 1. / full
    w = w / w.sum()
    w += 1e-8
    lo, hi = w.min(), w.max()
    return ((1. - min_w) * (w - lo) / (hi - lo) + min_w).flatten()


def per_pixel_weight(h_patch: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """dataset_dpsr.py:1037-1056 on the device: h_patch float [B, 1, P, P] in [0, 1] (= uint8 / 255) -> the weight of every
    pixel's grey level, float32 of the same shape (a table lookup: index plumbing, no arithmetic)."""
    idx = (h_patch * 255.).to(torch.uint8).long()        # (img_h * 255.).type(torch.uint8): truncation, as the reference
    return table.to(h_patch.device, torch.float32)[idx]


def random_block(h: int, w: int, area: float):
    """get_random_coordinates_block (:1060-1070): np.random draws in the reference's order."""
    assert 0. <= area <= 1., area
    ratio = np.random.randn() * 0.01 + area
    bh, bw = np.int64(h * ratio), np.int64(w * ratio)
    ch = np.random.randint(0, h - bh + 1)
    cw = np.random.randint(0, w - bw + 1)
    return ch, cw, bh, bw


def da_blur(img: np.ndarray, prob: float, area: float, sigma: float) -> np.ndarray:
    """np_blur (:1071-1108): a Gaussian blur (scipy.ndimage.gaussian_filter over all three axes of the HWC array) inside
    or -- with probability 0.98 -- outside a random block."""
    from scipy.ndimage import gaussian_filter
    assert img.ndim == 3
    if area == 0 or np.random.rand(1) >= prob:
        return img
    h, w, c = img.shape
    ch, cw, bh, bw = random_block(h, w, area)
    blurred = gaussian_filter(input=img, sigma=sigma)
    if np.random.rand(1) >= 0.98:
        img[ch:ch + bh, cw:cw + bw, :] = blurred[ch:ch + bh, cw:cw + bw, :]
    else:
        im = np.copy(blurred)
        im[ch:ch + bh, cw:cw + bw, :] = img[ch:ch + bh, cw:cw + bw, :]
        img = im
    return img


def da_dot_bin_noise(img: np.ndarray, prob: float, area: float, p: float) -> np.ndarray:
    """np_prod_binary_noise (:1111-1144): a Bernoulli(1 - p) mask on a random block."""
    assert img.ndim == 3
    if area == 0 or np.random.rand(1) >= prob:
        return img
    h, w, c = img.shape
    ch, cw, bh, bw = random_block(h, w, area)
    mask = np.random.binomial(n=1, p=1. - p, size=(bh, bw, 1)).astype(np.float32)
    img[ch:ch + bh, cw:cw + bw, :] = img[ch:ch + bh, cw:cw + bw, :] * mask
    return img


def da_add_gaus_noise(img: np.ndarray, prob: float, area: float, std: float) -> np.ndarray:
    """np_add_gaussian_noise (:1147-1180): N(0, std) on a random block."""
    assert img.ndim == 3
    if area == 0 or np.random.rand(1) >= prob:
        return img
    h, w, c = img.shape
    ch, cw, bh, bw = random_block(h, w, area)
    noise = np.random.normal(loc=0.0, scale=std, size=(bh, bw, c))
    img[ch:ch + bh, cw:cw + bw, :] = img[ch:ch + bh, cw:cw + bw, :] + noise
    return img


def apply_lr_augmentations(img_l: np.ndarray, args) -> np.ndarray:
    """The LR-only block of DatasetDPSR.__getitem__ (:899-905) in its order: blur, dot-binary noise, additive Gaussian."""
    if getattr(args, 'da_blur', False):
        img_l = da_blur(img_l, args.da_blur_prob, args.da_blur_area, args.da_blur_sigma)
    if getattr(args, 'da_dot_bin_noise', False):
        img_l = da_dot_bin_noise(img_l, args.da_dot_bin_noise_prob, args.da_dot_bin_noise_area, args.da_dot_bin_noise_p)
    if getattr(args, 'da_add_gaus_noise', False):
        img_l = da_add_gaus_noise(img_l, args.da_add_gaus_noise_prob, args.da_add_gaus_noise_area, args.da_add_gaus_noise_std)
    return img_l


# ---------------------------------------------------------------------------------------------------------------------------
# --lr_synth psf (not a reference option): the camera model of the LR image of an HR-only pair, stated in numpy.
#   clean = bin_s(G_sigma * HR)                      psf_bin_np        (srhip_psf_bin)
#   LR = float32((Poisson(photons * clean) + read_std * z) / photons)   photon_noise_np   (srhip_photon_noise)
# Same weights, tap order, roundings and draws as the kernels (include/srhip.h); the host path of EvalPairs.low_res_f32.
LR_BLUR_MAX_RADIUS = 64                 # srhip.ops.LR_BLUR_MAX_RADIUS
LR_SYNTH_MAX_PHOTONS = 1e6
NEAR_INVERSION, NEAR_PTRS = 1e-12, 1e-8     # photon_noise_np marks decisions closer than this to their boundary
_M32 = np.uint64(0xFFFFFFFF)


def psf_bin_weights(sigma: float, s: int) -> np.ndarray:
    """float64 [2 r + s]: box_s (*) gaussian, r = int(4 sigma + 0.5) -- scipy's normalised Gaussian weights
    (scipy.ndimage._filters._gaussian_kernel1d; sigma = 0: the single weight 1) summed over the s pixels of a bin in ascending
    order and divided by s."""
    sigma, s = float(sigma), int(s)
    if not (0. <= sigma < math.inf):
        raise ValueError(f"psf_bin_weights: sigma must be a finite number >= 0 (got {sigma})")
    if not 2 <= s <= 16:
        raise ValueError(f"psf_bin_weights: the bin side s is 2 .. 16 (got {s})")
    r = int(4.0 * sigma + 0.5)
    if r > LR_BLUR_MAX_RADIUS:
        raise ValueError(f"psf_bin_weights: sigma {sigma} gives a blur radius of {r}, above {LR_BLUR_MAX_RADIUS}")
    if r == 0:
        g = np.ones(1, dtype=np.float64)
    else:
        k = np.arange(-r, r + 1)
        phi = np.exp(-0.5 / (sigma * sigma) * k ** 2)
        g = phi / phi.sum()
    w = np.zeros(2 * r + s, dtype=np.float64)
    for j in range(s):
        w[j:j + 2 * r + 1] += g
    return w / float(s)


def _reflect(i: np.ndarray, n: int) -> np.ndarray:
    """scipy's 'reflect' border (d c b a | a b c d | d c b a) for any distance from the line"""
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def psf_bin_np(img: np.ndarray, sigma: float, s: int, in_max=None) -> np.ndarray:
    """bin_s(G_sigma * img) as srhip_psf_bin computes it: img [..., H, W] float32, uint8 (read as np.float32(v / 255.)) or
    uint16 (np.float32(min(v, in_max) / float(in_max))), H and W multiples of s -> float32 [..., H / s, W / s].  Per axis -- the
    last one first -- one strided correlation with psf_bin_weights over the reflected source, float64 sums in ascending tap
    order, one rounding to float32."""
    if img.dtype == np.uint8:
        img = np.float32(img / 255.)
    elif img.dtype == np.uint16:
        m = 65535 if in_max is None else int(in_max)
        img = np.float32(np.minimum(img, m) / float(m))
    assert img.dtype == np.float32 and img.ndim >= 2, (img.dtype, img.shape)
    H, W = img.shape[-2:]
    if H % s or W % s:
        raise ValueError(f"psf_bin_np: {H} x {W} is no multiple of s = {s}")
    w = psf_bin_weights(sigma, s)
    r = (w.size - s) // 2

    def one_axis(a, axis):
        n = a.shape[axis]
        first = np.arange(n // s) * s - r
        acc = np.zeros(a.shape[:axis] + (n // s,) + a.shape[axis + 1:], dtype=np.float64)
        for k in range(w.size):
            acc += w[k] * np.take(a, _reflect(first + k, n), axis=axis).astype(np.float64)
        return acc.astype(np.float32)
    return one_axis(one_axis(img, img.ndim - 1), img.ndim - 2)


def _philox4x32_10(c0, c1, c2, seed: int):
    """Philox4x32-10 (Salmon et al., SC'11; csrc/philox.h, tests/philox_ref.py) of the counters (c0, c1, c2, 0) under the key
    (low, high 32 bits of seed): the four output words, uint64 arrays holding 32-bit values"""
    c0, c1, c2 = (np.asarray(c, dtype=np.uint64) & _M32 for c in (c0, c1, c2))
    c3 = np.zeros(c0.shape, dtype=np.uint64)
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    sh = np.uint64(32)
    for _ in range(10):
        p0, p1 = c0 * np.uint64(0xD2511F53), c2 * np.uint64(0xCD9E8D57)
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ np.uint64(k0), p1 & _M32, (p0 >> sh) ^ c3 ^ np.uint64(k1), p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def _u01(w: np.ndarray) -> np.ndarray:
    """a 32-bit word as a double strictly inside (0, 1)"""
    return (w.astype(np.float64) + 0.5) * (1.0 / 4294967296.0)


def photon_noise_np(x: np.ndarray, seed: int, photons: float, read_std: float = 0., on=None, first_sample: int = 0, info=None):
    """srhip_photon_noise in numpy: x float32 [B, 1, h, w] -> (LR float32 of the same shape, marked bool of the same shape).
    Sample b of x is sample first_sample + b of the call (its Philox counter); ``on``: B flags, None = all.  ``marked``: the pixels
    whose Poisson decision lies so near a boundary that another libm may decide otherwise -- the inversion's uniform within
    1e-12 of a cumulated probability, or the two sides of a PTRS log comparison within 1e-8 of each other.  ``info`` (a dict)
    receives 'counts' (float64, the Poisson draws) and 'attempts' (0: no draw or inversion; t: PTRS accepted at its t-th
    attempt; 17: sixteen rejections, rint(lambda))."""
    from scipy.special import gammaln
    photons, read_std = float(photons), float(read_std)
    if not 0. < photons <= LR_SYNTH_MAX_PHOTONS:
        raise ValueError(f"photon_noise_np: photons lies in (0, 1e6] (got {photons})")
    if not 0. <= read_std < math.inf:
        raise ValueError(f"photon_noise_np: read_std is a finite number >= 0 (got {read_std})")
    assert x.dtype == np.float32 and x.ndim == 4 and x.shape[1] == 1, (x.dtype, x.shape)
    B, _, h, w = x.shape
    hw = h * w
    flat = x.reshape(B, hw)
    i = np.broadcast_to(np.arange(hw, dtype=np.uint64), (B, hw)).reshape(-1)
    b = np.repeat(np.arange(first_sample, first_sample + B, dtype=np.uint64), hw)
    lam = photons * flat.reshape(-1).astype(np.float64)
    n = np.zeros(lam.shape, dtype=np.float64)
    marked = np.zeros(lam.shape, dtype=bool)
    attempts = np.zeros(lam.shape, dtype=np.int64)
    c = _philox4x32_10(i, b, np.zeros_like(i), seed)
    with np.errstate(all='ignore'):
        # 0 < lambda < 30: inversion by sequential search from one uniform
        inv = np.flatnonzero((lam > 0.) & (lam < 30.))
        if inv.size:
            la, u = lam[inv], _u01(c[0][inv])
            p = np.exp(-la)
            cum = p.copy()
            k = np.zeros(la.shape, dtype=np.float64)
            near = np.abs(u - cum) <= NEAR_INVERSION
            go = u > cum
            for _ in range(255):
                if not go.any():
                    break
                k[go] += 1.
                p[go] = p[go] * la[go] / k[go]
                cum[go] += p[go]
                near |= go & (np.abs(u - cum) <= NEAR_INVERSION)
                go &= u > cum
            n[inv], marked[inv] = k, near
        # lambda >= 30: Hoermann's PTRS, attempt t from words (2 t % 4, 2 t % 4 + 1) of counter (i, b, t // 2)
        todo = np.flatnonzero(lam >= 30.)
        if todo.size:
            attempts[todo] = 17
            n[todo] = np.rint(lam[todo])
        for t in range(16):
            if not todo.size:
                break
            if t & 1 == 0:
                cw = c if t == 0 else _philox4x32_10(i[todo], b[todo], np.full(todo.shape, t >> 1, dtype=np.uint64), seed)
                cw = [v[todo] for v in cw] if t == 0 else list(cw)
            la = lam[todo]
            slam, loglam = np.sqrt(la), np.log(la)
            bb = 0.931 + 2.53 * slam
            a = -0.059 + 0.02483 * bb
            invalpha = 1.1239 + 1.1328 / (bb - 3.4)
            vr = 0.9277 - 3.6224 / (bb - 2.0)
            U = _u01(cw[2] if t & 1 else cw[0]) - 0.5
            V = _u01(cw[3] if t & 1 else cw[1])
            us = 0.5 - np.abs(U)
            k = np.floor((2.0 * a / us + bb) * U + la + 0.43)
            quick = (us >= 0.07) & (V <= vr)
            skip = ~quick & ((k < 0.) | ((us < 0.013) & (V > us)))
            test = ~quick & ~skip
            lhs = np.log(V) + np.log(invalpha) - np.log(a / (us * us) + bb)
            rhs = -la + k * loglam - gammaln(np.where(test, k, 0.) + 1.0)
            marked[todo[test & (np.abs(lhs - rhs) <= NEAR_PTRS)]] = True
            accept = quick | (test & (lhs <= rhs))
            n[todo[accept]] = k[accept]
            attempts[todo[accept]] = t + 1
            if t & 1 == 0:
                cw = [v[~accept] for v in cw]
            todo = todo[~accept]
        val = n
        if read_std != 0.:
            g = _philox4x32_10(i, b, np.full(i.shape, 0x80000000, dtype=np.uint64), seed)
            z = np.sqrt(-2.0 * np.log(_u01(g[0]))) * np.cos(6.283185307179586 * _u01(g[1]))
            val = n + read_std * z
        out = (val / photons).astype(np.float32).reshape(B, hw)
    if on is not None:
        off = ~np.asarray(on, dtype=bool)
        assert off.shape == (B,), off.shape
        out[off] = flat[off]
        marked.reshape(B, hw)[off] = False
    if info is not None:
        info['counts'], info['attempts'] = n.reshape(x.shape), attempts.reshape(x.shape)
    return out.reshape(x.shape), marked.reshape(x.shape)


def otsu_threshold(img: np.ndarray, nbins: int = 256):
    """skimage.filters.threshold_otsu(image, nbins) for an integer image (the sampler's 'automatic_threshold' style,
    dataset_dpsr.py:479-480).  skimage is not in this image: restated from its published algorithm -- for integer images
    the histogram has one bin per grey level between the image's min and max (nbins is ignored), and the threshold is the
    bin centre that maximises the between-class variance.  PARITY UNPINNED against skimage."""
    assert np.issubdtype(img.dtype, np.integer), img.dtype
    flat = img.reshape(-1)
    lo, hi = int(flat.min()), int(flat.max())
    if lo == hi:
        return lo
    return otsu_from_counts(np.bincount(flat.astype(np.int64) - lo, minlength=hi - lo + 1), first=lo)


def otsu_from_counts(counts, first: int = 0):
    """otsu_threshold from the image's histogram: counts[k] = number of pixels of grey level first + k (e.g. the 256 bins of
    srhip_hist_u8 with first = 0).  Empty bins below the image's min and above its max are dropped, as skimage's histogram
    of an integer image spans min..max only; a constant image returns its grey level."""
    counts = np.asarray(counts)
    nz = np.flatnonzero(counts)
    assert nz.size, "otsu_from_counts: empty histogram"
    lo, hi = int(nz[0]), int(nz[-1])
    if lo == hi:
        return first + lo
    counts = counts[lo:hi + 1].astype(np.float64)
    centers = np.arange(first + lo, first + hi + 1).astype(np.float64)
    w1 = np.cumsum(counts)
    w2 = np.cumsum(counts[::-1])[::-1]
    m1 = np.cumsum(counts * centers) / w1
    m2 = (np.cumsum((counts * centers)[::-1]) / w2[::-1])[::-1]
    var12 = w1[:-1] * w2[1:] * (m1[:-1] - m2[1:]) ** 2
    return centers[int(np.argmax(var12))]


def l_to_h(img_l: torch.Tensor, size_hw) -> torch.Tensor:
    """_resize_low_to_scale (:659-683) on the device: img_l [B, h, w] uint8 or float32 CUDA -> [B, H, W] of the same dtype."""
    from srhip import ops
    return ops.resize_cubic(img_l.contiguous(), size_hw)
