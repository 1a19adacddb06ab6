"""Statements and inputs of the 16-bit tile tests (srhip_patch_gather_u16, srhip_imresize_aa_u16, srhip_levels_u16_to_u8 and the
data sets built on them).

tests/test_cpu_deep_tiles.py checks the statements themselves; tests/test_gpu_deep_tiles.py gates the kernels and the sets,
bit for bit, against the same statements.  Both import them from here.

R1 (value): a 16-bit grey level v with white level in_max is np.float32(min(v, in_max) / float(in_max)) -- predict_cases'
ingest_value, the rule of srhip_ingest_pad.  R2 (8-bit reduction): tensor2uint82float of that value,
round_half_even(clamp(x, 0, 1) * 255) with ONE float32 product."""
import os

import numpy as np

from predict_cases import ingest_value

IN_MAXES = (65535, 4095)


def unit(v, in_max):
    """R1"""
    return ingest_value(np.asarray(v), in_max)


def level8(v, in_max):
    """R2: uint8 levels of uint16 levels"""
    x = unit(v, in_max)
    assert x.dtype == np.float32
    c = np.clip(x, np.float32(0), np.float32(1))
    p = c * np.float32(255)
    assert p.dtype == np.float32
    return np.rint(p).astype(np.uint8)          # np.rint rounds half to even


def augment_img(img, mode):
    """util.augment_img (utils_image.py:469-487)"""
    return [img, np.flipud(np.rot90(img)), np.flipud(img), np.rot90(img, k=3), np.flipud(np.rot90(img, k=2)), np.rot90(img),
            np.rot90(img, k=2), np.flipud(np.rot90(img, k=3))][mode]


def tile_u16(h, w, in_max, seed):
    """random uint16 tile: half of the pixels over the whole uint16 range (above a white level below 65535 too), half in
    0 .. in_max; the extremes and both sides of the white level are present"""
    rng = np.random.RandomState(seed)
    a = np.where(rng.rand(h, w) < 0.5, rng.randint(0, 65536, size=(h, w)), rng.randint(0, in_max + 1, size=(h, w)))
    a.reshape(-1)[:4] = (0, 65535, in_max, min(in_max + 1, 65535))
    return a.astype(np.uint16)


def tile_u8(h, w, seed):
    """a smooth blob on noise: an ROI exists at every threshold the sampler tests use, and Otsu's threshold is well defined"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    blob = 150. * np.exp(-((yy - 0.4 * h) ** 2 + (xx - 0.6 * w) ** 2) / (2. * (0.2 * min(h, w)) ** 2))
    return np.clip(blob + rng.randint(0, 40, size=(h, w)), 0, 255).astype(np.uint8)


def down_u8(img, sf):
    """a plausible true LR tile of a uint8 HR tile: block means, rounded"""
    h, w = img.shape
    return np.rint(img.reshape(h // sf, sf, w // sf, sf).astype(np.float64).mean(axis=(1, 3))).astype(np.uint8)


def write_fold(root, ds, hr, lr=None, ext="tif"):
    """<root>/data/biosr/<ds>/{h,l}_<i>.<ext> (PIL: uint8 -> L, uint16 -> I;16) and <root>/folds/<ds>/{h_l,l_h}.txt; lr None:
    an HR-only fold ('None_<i>' keys).  A biosr... name: the tiles are not CACO-2 tiles."""
    from PIL import Image
    assert ds.startswith("biosr")
    d = os.path.join(root, "data", "biosr", ds)
    f = os.path.join(root, "folds", ds)
    os.makedirs(d, exist_ok=True)
    os.makedirs(f, exist_ok=True)
    pairs = []
    for i, h in enumerate(hr):
        hk = f"{ds}/h_{i}.{ext}"
        Image.fromarray(h).save(os.path.join(d, f"h_{i}.{ext}"))
        if lr is None:
            lk = f"None_{i}"
        else:
            lk = f"{ds}/l_{i}.{ext}"
            Image.fromarray(lr[i]).save(os.path.join(d, f"l_{i}.{ext}"))
        pairs.append((hk, lk))
    with open(os.path.join(f, "h_l.txt"), "w") as fh:
        fh.write("".join(f"{a},{b}\n" for a, b in pairs))
    with open(os.path.join(f, "l_h.txt"), "w") as fh:
        fh.write("".join(f"{b},{a}\n" for a, b in pairs))
    return os.path.join(root, "data"), os.path.join(root, "folds")
