"""numpy statement of srhip_lr_augment (include/srhip.h): the reference's three LR-only augmentations -- np_blur,
np_prod_binary_noise, np_add_gaussian_noise on a random block, dataset_dpsr.py:899-905,1060-1180 -- with the library's draws.

Stage s = 0 blur, 1 dot noise, 2 Gaussian noise, in that order; stage s of sample b is skipped when it is off, its area is 0
or u_apply >= prob.  All draws are Philox4x32-10 (philox_ref) under key = (low, high 32 bits of the seed), c3 = 0; a word w is
the double u = (w + 0.5) 2^-32, a normal is sqrt(-2 ln u1) cos(2 pi u2) in float64.
  per (sample, stage)  counter (b, 0xFFFFFFFF, s) -> w0..w3, counter (b, 0xFFFFFFFE, s) -> w4..w7; u_apply = u(w0),
                       z = normal(w1, w2), u_ch = u(w3), u_cw = u(w4), u_side = u(w5); ratio = z * 0.01 + area,
                       bh = clamp(trunc(h ratio), 0, h), ch = min(floor(u_ch (h - bh + 1)), h - bh), bw / cw likewise from w;
                       the blur goes inside the block iff u_side >= 0.98
  per pixel            e = (b h + y) w + x: word e % 4 of counter (low, high 32 bits of e / 4, site) -- philox_ref.words; site 1
                       the Bernoulli mask (kept iff word >= round(p 2^32)), sites 2 and 3 u1 and u2 of the pixel's normal
  blur                 scipy.ndimage.gaussian_filter(img_hwc, sigma)

Also here: the cases the CPU and the GPU test files share, and their seeds."""
import functools

import numpy as np

import philox_ref as PR

STAGES = ("blur", "dot", "gaus")
OFF = (False, 0.0, 0.0, 0.0)
SIDE_INSIDE = 0.98


def u01(w):
    return (np.asarray(w, dtype=np.float64) + 0.5) * 2.0 ** -32


def normal01(w1, w2):
    return np.sqrt(-2.0 * np.log(u01(w1))) * np.cos(2.0 * np.pi * u01(w2))


def block_draws(seed, b, s):
    """the eight words of (sample b, stage s) as Python ints"""
    k0, k1 = int(seed) & PR.MASK32, (int(seed) >> 32) & PR.MASK32
    a = PR.philox4x32_10(b, 0xFFFFFFFF, s, 0, k0, k1)
    c = PR.philox4x32_10(b, 0xFFFFFFFE, s, 0, k0, k1)
    return [int(v) for v in a] + [int(v) for v in c]


def decide(seed, b, s, h, w, prob, area):
    """(decision, raw): decision = (applied, ch, cw, bh, bw, inside); raw holds the quantities the decision was cut from --
    what the case selection measures its margins on -- and the normal z."""
    d = block_draws(seed, b, s)
    u_apply = float(u01(d[0]))
    raw = {"u_apply": u_apply, "prob": prob}
    if area == 0 or u_apply >= prob:
        return (False, 0, 0, 0, 0, False), raw
    z = float(normal01(d[1], d[2]))
    ratio = z * 0.01 + area
    bh = min(max(int(np.trunc(h * ratio)), 0), h)
    bw = min(max(int(np.trunc(w * ratio)), 0), w)
    u_ch, u_cw, u_side = float(u01(d[3])), float(u01(d[4])), float(u01(d[5]))
    ch = min(int(np.floor(u_ch * (h - bh + 1))), h - bh)
    cw = min(int(np.floor(u_cw * (w - bw + 1))), w - bw)
    raw.update(z=z, ratio=ratio, u_side=u_side,
               cuts=[h * ratio, w * ratio, u_ch * (h - bh + 1), u_cw * (w - bw + 1)])
    return (True, ch, cw, bh, bw, u_side >= SIDE_INSIDE), raw


def margin(raw, with_side):
    """the smallest distance of a cut quantity from the value at which its decision flips"""
    m = abs(raw["u_apply"] - raw["prob"])
    for v in raw.get("cuts", ()):
        m = min(m, abs(v - np.rint(v)))
    if with_side and "u_side" in raw:
        m = min(m, abs(raw["u_side"] - SIDE_INSIDE))
    return m


def pixel_draws(seed, b, h, w, s, ch, cw, bh, bw, value):
    """what stage s (1: the float32 mask, 2: the float64 noise) draws for the pixels of its block, [bh, bw]"""
    rows = (np.arange(ch, ch + bh)[:, None] * w + np.arange(cw, cw + bw)[None, :]).reshape(-1)
    if s == 1:
        keep = PR.words(seed, 1, b * h * w, h * w)[rows] >= np.uint64(PR.threshold(value)[0])
        return keep.astype(np.float32).reshape(bh, bw)
    w1, w2 = PR.words(seed, 2, b * h * w, h * w)[rows], PR.words(seed, 3, b * h * w, h * w)[rows]
    return (np.float64(value) * normal01(w1, w2)).reshape(bh, bw)


def blur_weights(sigma):
    """scipy's normalised Gaussian weights [2 r + 1], r = int(4 sigma + 0.5) (what ops.lr_blur_weights uploads)"""
    r = int(4.0 * float(sigma) + 0.5)
    k = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * k ** 2)
    return phi / phi.sum()


def blur_passes(img, sigma):
    """gaussian_filter(img[:, :, None], sigma)[:, :, 0] restated pass by pass in the order the kernel computes it: the rows
    axis, the columns axis, the channel axis of length 1; 'reflect' folds i by m = i mod 2 n, m >= n -> 2 n - 1 - m; each pass
    sums in float64 -- the centre tap, then the pairs from the farthest inwards -- and stores float32."""
    wt = blur_weights(sigma)
    r = len(wt) // 2

    def fold(i, n):
        m = np.mod(i, 2 * n)
        return np.where(m >= n, 2 * n - 1 - m, m)

    def one(a, axis):
        a = np.moveaxis(a, axis, 0).astype(np.float64)
        n = a.shape[0]
        pos = np.arange(n)
        acc = a * wt[r]
        for jj in range(-r, 0):
            acc = acc + (a[fold(pos + jj, n)] + a[fold(pos - jj, n)]) * wt[r + jj]
        return np.moveaxis(acc.astype(np.float32), 0, axis)
    out = one(one(np.asarray(img, dtype=np.float32), 0), 1)
    return one(out[:, :, None], 2)[:, :, 0]


def augment_sample(img, seed, b, params):
    """img: float32 [h, w], sample b of a batch under ``seed``; params = ((on, prob, area, sigma), (on, prob, area, p),
    (on, prob, area, std)).  Returns (float32 [h, w], [decision of stage 0, 1, 2], [raw of stage 0, 1, 2])."""
    from scipy.ndimage import gaussian_filter
    img = np.array(img, dtype=np.float32, copy=True)
    h, w = img.shape
    decisions, raws = [], []
    for s, (on, prob, area, value) in enumerate(params):
        if not on:
            decisions.append((False, 0, 0, 0, 0, False))
            raws.append({})
            continue
        dec, raw = decide(seed, b, s, h, w, prob, area)
        decisions.append(dec)
        raws.append(raw)
        applied, ch, cw, bh, bw, inside = dec
        if not applied:
            continue
        blk = (slice(ch, ch + bh), slice(cw, cw + bw))
        if s == 0:
            blurred = gaussian_filter(input=img[:, :, None], sigma=value)[:, :, 0]
            if inside:
                img[blk] = blurred[blk]
            else:
                blurred[blk] = img[blk]
                img = blurred
        elif s == 1:
            img[blk] = img[blk] * pixel_draws(seed, b, h, w, 1, ch, cw, bh, bw, value)
        else:
            img[blk] = img[blk] + pixel_draws(seed, b, h, w, 2, ch, cw, bh, bw, value)
    return img, decisions, raws


def augment_batch(x, seed, params):
    """x: float32 [B, 1, h, w] -> (augmented copy, decisions [B][3])"""
    out, decs = np.empty_like(x), []
    for b in range(x.shape[0]):
        out[b, 0], d, _ = augment_sample(x[b, 0], seed, b, params)
        decs.append(d)
    return out, decs


# ---- the cases of tests/test_lr_augment.py (CPU) and tests/test_gpu_lr_augment.py --------------------------------------------
# (B, h, w, sigma): radius 4; radius 8 >= n; radius 12 > 2 n with h w no multiple of 4 (Philox groups straddle samples); rows
# that are no multiple of a 16-byte group; the x8 workload's LR patch; the x2 workload's
SHAPES = ((3, 8, 8, 1.0), (3, 8, 8, 2.0), (3, 5, 7, 3.0), (3, 16, 12, 1.0), (2, 64, 64, 1.0), (1, 256, 256, 1.0))
# (prob, area, p, std)
VALUES = ((1.0, 0.3, 0.5, 0.05), (1.0, 1.0, 0.5, 0.05), (1.0, 0.0, 0.5, 0.05), (0.0, 0.3, 0.5, 0.05), (1.0, 0.3, 0.0, 0.0),
          (1.0, 0.3, 0.999, 0.05), (1.0, 1.0, 0.999, 0.0))
MODES = ("blur", "dot", "gaus", "all")


def make_params(mode, sigma, prob, area, p, std):
    on = [mode in (name, "all") for name in STAGES]
    return tuple((o, prob, area, v) if o else OFF for o, v in zip(on, (sigma, p, std)))


def cases():
    """[(name, B, h, w, params, seed)]: every stage alone and all three, crossed with VALUES, at every shape.  The seed of
    case k is a fixed 63-bit number with both halves set."""
    out = []
    for (B, h, w, sigma) in SHAPES:
        for mode in MODES:
            for vals in VALUES:
                k = len(out)
                seed = ((k + 1) * 0x9E3779B97F4A7C15) & 0x7FFFFFFFFFFFFFFF
                out.append((f"{B}x{h}x{w}-s{sigma:g}-{mode}-" + "-".join(f"{v:g}" for v in vals), B, h, w,
                            make_params(mode, sigma, *vals), seed))
    return out


def case_input(B, h, w):
    """float32 [B, 1, h, w] in [0, 1], with exact zeros and ones among the values"""
    x = np.random.default_rng(1000 * B + 10 * h + w).random((B, 1, h, w), dtype=np.float32)
    x.reshape(-1)[::7] = 0.0
    x.reshape(-1)[3::11] = 1.0
    return x


@functools.lru_cache(maxsize=None)
def case_reference(k):
    """(input, expected, decisions, smallest margin) of case k, computed once"""
    name, B, h, w, params, seed = cases()[k]
    x = case_input(B, h, w)
    want, decs, m = np.empty_like(x), [], 1.0
    for b in range(B):
        want[b, 0], d, raws = augment_sample(x[b, 0], seed, b, params)
        decs.append(d)
        for s, raw in enumerate(raws):
            if raw:
                m = min(m, margin(raw, with_side=(s == 0)))
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want, decs, m
