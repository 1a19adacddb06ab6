"""Image pairs of the Fourier ring correlation tests (tests/test_cpu_frc.py, tests/test_gpu_frc.py) and their float64 statement,
computed once a process.

A target H is cell-like: a pedestal, a smooth random field, sparse dots blurred to a pixel or so, and a little white texture, so
that it has power up to Nyquist.  The prediction is E = G_sigma * H + noise: correlated with H at low frequencies, noise at high
ones, so the curve starts at 1 and crosses 1/7 inside the band.  An image and its noise-free blurred copy would give FRC = 1 on
every ring: the pairs need the noise.  Seeds are fixed; test_cpu_frc.py asserts the conditions the cases must satisfy."""
import functools

import numpy as np

import frc_ref as R


def blur(img, sigma):
    """periodic Gaussian blur through the real FFT"""
    h, w = img.shape
    fy, fx = np.fft.fftfreq(h)[:, None], np.fft.rfftfreq(w)[None, :]
    g = np.exp(-2.0 * (np.pi * sigma) ** 2 * (fy ** 2 + fx ** 2))
    return np.fft.irfft2(np.fft.rfft2(img) * g, s=(h, w))


def target(h, w, seed):
    rng = np.random.default_rng(seed)
    smooth = blur(rng.standard_normal((h, w)), 6.0)
    smooth /= np.abs(smooth).max()
    dots = np.zeros((h, w))
    n = max(4, h * w // 150)
    dots[rng.integers(0, h, n), rng.integers(0, w, n)] = rng.uniform(0.5, 1.0, n)
    dots = blur(dots, 0.8)
    dots /= dots.max()
    return np.clip(0.15 + 0.15 * smooth + 0.5 * dots + 0.02 * rng.standard_normal((h, w)), 0.0, 1.0)


def prediction(H, seed, sigma=1.0, noise=0.01):
    rng = np.random.default_rng(seed + 1000)
    return np.clip(blur(H, sigma) + noise * rng.standard_normal(H.shape), 0.0, 1.0)


# name: (B, h, w, levels, inputs_are_levels, seed)
CASES = {
    "32x32": (1, 32, 32, 255, False, 11),
    "37x45": (1, 37, 45, 255, False, 12),
    "3x70x151": (3, 70, 151, 255, False, 13),
    "128x128_65535": (1, 128, 128, 65535, False, 14),
    "128x128_65535_levels": (1, 128, 128, 65535, True, 14),
    "512x512": (1, 512, 512, 255, False, 15),
    "8x512x512": (8, 512, 512, 255, False, 18),               # (not in the issue's list) one evaluation batch
    "2x2048x2048": (2, 2048, 2048, 255, False, 16),
    "2100x2050": (1, 2100, 2050, 255, False, 17),
}
SMALL = tuple(k for k, v in CASES.items() if R.side(v[1], v[2]) <= 128)       # where the direct longdouble DFT is affordable


@functools.lru_cache(maxsize=None)
def images(name):
    """(E, H) float32 (B, 1, h, w): floats in [0, 1], or the levels 0 .. N of the same images for an inputs_are_levels case"""
    B, h, w, N, lv, seed = CASES[name]
    Hs = [target(h, w, seed + 100 * i) for i in range(B)]
    Es = [prediction(t, seed + 100 * i) for i, t in enumerate(Hs)]
    E, H = (np.stack(v).astype(np.float32)[:, None] for v in (Es, Hs))
    if lv:
        E, H = R.levels(E, N), R.levels(H, N)
    E.setflags(write=False)
    H.setflags(write=False)
    return E, H


@functools.lru_cache(maxsize=None)
def expect(name):
    """(curve (B, S/2 + 1), cut (B,), the per-image dicts of frc_ref.frc_one): the float64 statement, computed once"""
    _, _, _, N, lv, _ = CASES[name]
    E, H = images(name)
    curve, cut, each = R.frc(E, H, N, R.T_DEFAULT, lv)
    curve.setflags(write=False)
    cut.setflags(write=False)
    return curve, cut, each


@functools.lru_cache(maxsize=None)
def e_ref():
    """the reference's own rounding: the largest curve difference between the statement through np.fft.fft2 (pocketfft, float64)
    and through a direct DFT in np.longdouble, over the cases with S <= 128"""
    worst = 0.0
    for name in SMALL:
        _, _, _, N, lv, _ = CASES[name]
        E, H = images(name)
        for e, h, o in zip(E[:, 0], H[:, 0], expect(name)[2]):
            a, b = R.windowed(e, N, lv), R.windowed(h, N, lv)
            c = R.curve_of(R.dft2_longdouble(a), R.dft2_longdouble(b))[0]
            worst = max(worst, float(np.abs(c - o["curve"].astype(np.longdouble)).max()))
    return worst


def bound():
    """the gate of the kernel's curve: 64 e_ref (butterfly order, twiddle source and ring-sum order are each a few eps a stage;
    64 covers S = 2048 against the S <= 128 of e_ref, and rings of up to ~6 S terms)"""
    return 64.0 * e_ref()
