"""Cases of the resolution-scaled error tests (tests/test_cpu_consistency.py, tests/test_gpu_consistency.py) and their float64
statement, computed once a process.

An output E is the cell-like target of tests/frc_cases.py at the HR size, float32.  Its LR page is planted: L = float32(a b_q0(E)
+ c + noise), b_q0 the statement's own model image at the blur q0, so that the search has a known answer (noise-free: q == q0,
alpha == a, beta == c up to the float32 rounding of L).  Seeds are fixed; test_cpu_consistency.py asserts the condition the cases
must satisfy (every bank of every page is decided by at least 1e-9).

A blur of 0.125 HR pixels is the identity to 1e-14: its outer Gaussian weights are exp(-32).  So the candidates up to q = 1 at
s = 8 (q = 2 at s = 4, q = 4 at s = 2) are one model to the last bits, and a noise-free plant at q0 = 0 is decided between them
by the float32 rounding of L, by 1e-15, under any seed.  The pages with q0 = 0 therefore carry noise, which gives their search
an optimum of its own, and their seeds are chosen so that it is decided by 1e-9 like every other."""
import functools

import numpy as np

import consistency_ref as C
import frc_cases as F

# name: (B, h, w, s, q0 per page, noise (one figure, or one per page), seed, (padded HR side, padded LR side) or None)
CASES = {
    "5x7_s8": (1, 5, 7, 8, (40,), 0.0, 31, None),             # radius up to 64 against 40 HR rows: the reflection folds twice
    "16x16_s2": (1, 16, 16, 2, (24,), 0.0, 32, None),         # the smallest scale
    "3x21x37_s4": (3, 21, 37, 4, (37, 0, 90), (0.0, 0.02, 0.0), 36, None),         # odd sizes, odd batch, two column strips, two row tiles
    "33x20_s8_q127": (1, 33, 20, 8, (127,), 0.0, 34, None),   # the last table entry, radius 64; five row tiles
    "2x64x64_s8": (2, 64, 64, 8, (72, 0), 0.02, 35, None),    # the predict shape
    "8x64x64_s8_strided": (8, 64, 64, 8, (72, 0, 16, 33, 50, 90, 110, 127), 0.02, 38, (576, 72)),     # views of padded tensors
}
SMALL = tuple(k for k, v in CASES.items() if v[1] * v[2] * v[3] ** 2 <= 2 ** 16)        # where the longdouble chain is affordable


def noise_of(name, i):
    v = CASES[name][5]
    return float(v[i]) if isinstance(v, tuple) else float(v)


NOISE_FREE = tuple((k, i) for k, v in CASES.items() for i in range(v[0]) if noise_of(k, i) == 0.0)        # (case, page)
MIN_MARGIN = 1e-9
QUANTITIES = ("score", "alpha", "beta", "rse")


def gain(i):
    """the planted linear rescaling of page i: (a, c)"""
    return 0.7 + 0.1 * (i % 3), 0.03 + 0.01 * (i % 4)


@functools.lru_cache(maxsize=None)
def tensors(name):
    """(E [B, 1, s h, s w], L [B, 1, h, w]) float32.  In a strided case both are views of padded arrays whose padding holds other
    numbers: reading past a row or a page shows."""
    B, h, w, s, q0s, noise, seed, padded = CASES[name]
    rng = np.random.default_rng(seed + 5000)
    Es = np.stack([F.target(s * h, s * w, seed + 100 * i) for i in range(B)]).astype(np.float32)
    Ls = []
    for i in range(B):
        a, c = gain(i)
        b = C.model(Es[i], q0s[i], s)
        Ls.append((a * b + c + noise_of(name, i) * rng.standard_normal((h, w))).astype(np.float32))
    Ls = np.stack(Ls)
    if padded is None:
        E, L = Es[:, None], Ls[:, None]
    else:
        PE, PL = padded
        big_e = rng.random((B, 1, PE, PE), dtype=np.float32)
        big_l = rng.random((B, 1, PL, PL), dtype=np.float32)
        big_e[:, 0, :s * h, :s * w] = Es
        big_l[:, 0, :h, :w] = Ls
        E, L = big_e[:, :, :s * h, :s * w], big_l[:, :, :h, :w]
    E.setflags(write=False)
    L.setflags(write=False)
    return E, L


@functools.lru_cache(maxsize=None)
def expect(name):
    """the per-page dicts of consistency_ref.consistency: the float64 statement, computed once"""
    E, L = tensors(name)
    return C.consistency(E[:, 0], L[:, 0], CASES[name][3])


@functools.lru_cache(maxsize=None)
def e_ref():
    """the statement's own rounding per output quantity: the largest difference between the float64 chain and the np.longdouble
    chain (correlations, sums, score, alpha, beta, rse on the float64 statement's q lists) over the cases with h w s^2 <= 2^16.
    'score' runs over all 32 slots."""
    worst = dict.fromkeys(QUANTITIES, 0.0)
    for name in SMALL:
        E, L = tensors(name)
        s = CASES[name][3]
        for e, l, o in zip(E[:, 0], L[:, 0], expect(name)):
            x = C.consistency_one(e, l, s, np.longdouble, qs=o["qs"])
            worst["score"] = max(worst["score"], float(np.abs(x["scores"] - o["scores"].astype(np.longdouble)).max()))
            for k in ("alpha", "beta", "rse"):
                worst[k] = max(worst[k], float(abs(x[k] - np.longdouble(o[k]))))
    return worst


def bound(quantity):
    """the gate of the kernel against the statement: 64 e_ref of that quantity, the rule of tests/frc_cases.py::bound.  The model
    images have the statement's bits (same weights, same tap order, no contraction); what differs is the order of the five sums
    over the pixels -- thread, wave, block and tile order against numpy's pairwise sum, each a few eps of the sum -- and the
    cancellation in C_xy = Sxy - Sx Sy / n carries that into the figures exactly as it carries the statement's own rounding into
    e_ref.  64 covers 8 x 64^2 terms against the small cases of e_ref."""
    return 64.0 * e_ref()[quantity]


BLOB = (203, 314, 3.0, 0.5)         # a structure the acquisition does not hold: HR row, HR column, sigma (HR pixels), height


def with_blob(E):
    """E [sh, sw] plus a Gaussian blob at BLOB, float32"""
    y0, x0, sigma, height = BLOB
    y, x = np.mgrid[:E.shape[0], :E.shape[1]]
    return (E.astype(np.float64) + height * np.exp(-((y - y0) ** 2 + (x - x0) ** 2) / (2.0 * sigma * sigma))).astype(np.float32)
