"""Images of the decorrelation analysis tests (tests/test_cpu_decorr.py, tests/test_gpu_decorr.py) and their float64 statement,
computed once a process.

Three kinds of image take turns inside a case: the cell-like target of tests/frc_cases.py, its blurred noisy prediction, and
sparse dots under a Gaussian point spread function with shot noise, the image the method was published for.  The shapes are
those of the Fourier ring correlation cases, because the two transform passes fail in the same places.  Seeds are fixed;
test_cpu_decorr.py asserts the condition the cases must satisfy (no image is marked)."""
import functools

import numpy as np

import decorr_ref as D
import frc_cases as F
import frc_ref as R


def dots(h, w, seed, sigma=2.0, photons=300.0):
    """point emitters on a dark ground through a Gaussian PSF of width ``sigma`` pixels, Poisson noise at ``photons`` in the peak"""
    rng = np.random.default_rng(seed)
    img = np.zeros((h, w))
    n = max(6, h * w // 120)
    img[rng.integers(0, h, n), rng.integers(0, w, n)] = rng.uniform(0.5, 1.0, n)
    img = F.blur(img, sigma)
    img = np.maximum(img, 0.0) / img.max()
    return np.clip(rng.poisson(photons * (0.02 + img)) / (1.25 * photons), 0.0, 1.0)


def image(kind, h, w, seed):
    if kind == 0:
        return F.target(h, w, seed)
    if kind == 1:
        return F.prediction(F.target(h, w, seed), seed)
    return dots(h, w, seed)


# name: (B, h, w, levels, inputs_are_levels, seed); image i of a case is of kind (seed + i) % 3
CASES = {
    "32x32": (1, 32, 32, 255, False, 11),
    "37x45": (1, 37, 45, 255, False, 12),
    "3x70x151": (3, 70, 151, 255, False, 13),                   # odd B: the zero-partner tail
    "128x128_65535": (1, 128, 128, 65535, False, 14),
    "128x128_65535_levels": (1, 128, 128, 65535, True, 14),
    "512x512": (1, 512, 512, 255, False, 15),
    "8x512x512": (8, 512, 512, 255, False, 18),
    "2x2048x2048": (2, 2048, 2048, 255, False, 16),
    "2100x2050": (1, 2100, 2050, 255, False, 17),
}
SMALL = tuple(k for k, v in CASES.items() if R.side(v[1], v[2]) <= 128)       # where the direct longdouble DFT is affordable


@functools.lru_cache(maxsize=None)
def images(name):
    """float32 (B, 1, h, w): floats in [0, 1], or the levels 0 .. N of the same images for an inputs_are_levels case"""
    B, h, w, N, lv, seed = CASES[name]
    X = np.stack([image((seed + i) % 3, h, w, seed + 100 * i) for i in range(B)]).astype(np.float32)[:, None]
    if lv:
        X = R.levels(X, N)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def expect(name):
    """the per-image dicts of decorr_ref.decorr_one: the float64 statement, computed once"""
    _, _, _, N, lv, _ = CASES[name]
    return D.decorr(images(name), N, lv)


@functools.lru_cache(maxsize=None)
def e_ref():
    """the reference's own rounding: the largest difference over all 21 curves between the statement through np.fft.fft2
    (pocketfft, float64) and through a direct DFT with np.longdouble sums, over the cases with S <= 128"""
    worst = 0.0
    for name in SMALL:
        _, _, _, N, lv, _ = CASES[name]
        for x, o in zip(images(name)[:, 0], expect(name)):
            c = D.curves_longdouble(x, o["sigmas"], N, lv)
            worst = max(worst, float(np.abs(c - o["curves"].astype(np.longdouble)).max()))
    return worst


def bound():
    """the gate of the kernel's curves: 64 e_ref, the rule of tests/frc_cases.py::bound and its reasoning (butterfly order,
    twiddle source and the order of the ring sums are each a few eps a stage; 64 covers S = 2048 against the S <= 128 of e_ref);
    the running sums over the rings add terms of one sign, so they lose nothing to cancellation"""
    return 64.0 * e_ref()
