"""The Fourier ring correlation of include/srhip.h (srhip_metrics_frc_lv) stated in numpy float64, the rule that marks an image
whose cutoff is ill-conditioned, and the same statement through a direct DFT in np.longdouble (the reference's own rounding).

Steps as the header numbers them: Q_N levels, x = level / N; the centred S x S square, S the largest power of two not above
min(h, w), at most 2048, at least 32, NO border crop; the separable periodic Hann window; two unnormalised FFT2; integer rings
(2r - 1)^2 <= 4 |k|^2 < (2r + 1)^2 kept for r = 0 .. S/2; FRC[r] = C_r / sqrt(P1_r P2_r), 0 where the product is 0; the first
ring from 1 on under T, linear interpolation, cut = x / (S/2); no smoothing."""
import functools

import numpy as np

T_DEFAULT = 1.0 / 7.0
MIN_SIDE, MAX_SIDE = 32, 2048
MARK = 1e-6              # an image with a curve value this close to T, up to its crossing ring, is marked: its cutoff may jump


def side(h, w):
    m = min(int(h), int(w))
    if m < MIN_SIDE:
        raise ValueError(f"frc: both sides must be at least {MIN_SIDE} (got {h} x {w})")
    S = MIN_SIDE
    while 2 * S <= m and 2 * S <= MAX_SIDE:
        S *= 2
    return S


def levels(x, N):
    """Q_N, the rule of srhip_tensor2levels: round_half_even(clip(x, 0, 1) * N) with ONE float32 product"""
    x = np.clip(np.asarray(x, dtype=np.float32), np.float32(0), np.float32(1))
    return np.rint(x * np.float32(N)).astype(np.float32)


def hann(S):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(S, dtype=np.float64) / S)


@functools.lru_cache(maxsize=None)
def ring_index(S):
    """(S, S) int: the ring of every frequency in FFT order by the integer rule, -1 beyond ring S/2"""
    k = np.arange(S, dtype=np.int64)
    k = np.where(k < S // 2, k, k - S)                           # signed, in [-S/2, S/2)
    q = 4 * (k[:, None] ** 2 + k[None, :] ** 2)                   # 4 |k|^2
    r = (np.floor(np.sqrt(q.astype(np.float64))).astype(np.int64) + 1) // 2       # a first guess, then the rule itself
    r = np.where((2 * r - 1) ** 2 > q, r - 1, r)
    r = np.where((2 * r + 1) ** 2 <= q, r + 1, r)
    r = np.where(q == 0, 0, r)
    assert bool(((q == 0) | (((2 * r - 1) ** 2 <= q) & (q < (2 * r + 1) ** 2))).all())
    return np.where(r <= S // 2, r, -1)


@functools.lru_cache(maxsize=None)
def _ring_order(S):
    ring = ring_index(S).ravel()
    order = np.argsort(ring, kind="stable")
    order = order[ring[order] >= 0]
    starts = np.searchsorted(ring[order], np.arange(S // 2 + 1))
    return order, starts


def ring_sums(v):
    """v (S, S) real, any float dtype -> (S/2 + 1,) sums over the kept rings, in the dtype of v"""
    order, starts = _ring_order(v.shape[-1])
    return np.add.reduceat(v.ravel()[order], starts)


def windowed(img, N, inputs_are_levels=False):
    """(h, w) -> the S x S float64 image win * level / N of steps 1 - 3"""
    h, w = img.shape
    S = side(h, w)
    lv = np.asarray(img, dtype=np.float32) if inputs_are_levels else levels(img, N)
    oy, ox = (h - S) // 2, (w - S) // 2
    x = lv[oy:oy + S, ox:ox + S].astype(np.float64) / float(N)
    win = hann(S)
    return (win[:, None] * win[None, :]) * x


def dft2_longdouble(x):
    """direct 2-D DFT in np.longdouble, the twiddles from the exactly reduced index j k mod S"""
    S = x.shape[0]
    jk = (np.arange(S, dtype=np.int64)[:, None] * np.arange(S, dtype=np.int64)[None, :]) % S
    pi = np.longdouble(4) * np.arctan(np.longdouble(1))           # (np.pi is a double)
    ang = np.longdouble(2) * pi * jk.astype(np.longdouble) / np.longdouble(S)
    Wm = np.cos(ang) - 1j * np.sin(ang)                           # clongdouble
    return Wm @ x.astype(np.longdouble) @ Wm.T


def curve_of(F1, F2):
    c = ring_sums((F1 * np.conj(F2)).real)
    p1 = ring_sums(F1.real ** 2 + F1.imag ** 2)
    p2 = ring_sums(F2.real ** 2 + F2.imag ** 2)
    den = p1 * p2
    ok = den > 0
    return np.where(ok, c / np.sqrt(np.where(ok, den, 1)), 0), p1, p2


def cutoff(curve, T=T_DEFAULT):
    """step 7 -> dict(cut, r: the crossing ring or None, p, q: FRC[r - 1], FRC[r], marked)"""
    curve = np.asarray(curve, dtype=np.float64)
    half = len(curve) - 1
    below = np.nonzero(curve[1:] < T)[0]
    if len(below) == 0:
        return dict(cut=1.0, r=None, p=None, q=None, marked=bool((np.abs(curve - T) < MARK).any()))
    r = int(below[0]) + 1
    p, q = float(curve[r - 1]), float(curve[r])
    x = 0.0 if p < T else (r - 1) + (p - T) / (p - q)
    return dict(cut=x / half, r=r, p=p, q=q, marked=bool((np.abs(curve[:r + 1] - T) < MARK).any()))


def frc_one(E, H, N=255, T=T_DEFAULT, inputs_are_levels=False, fft2=np.fft.fft2):
    """one pair of (h, w) images -> dict(curve, cut, side, p1, p2, r, p, q, marked)"""
    if not 0.0 < T < 1.0:
        raise ValueError(f"frc: the threshold lies in (0, 1) (got {T})")
    a, b = windowed(E, N, inputs_are_levels), windowed(H, N, inputs_are_levels)
    curve, p1, p2 = curve_of(fft2(a), fft2(b))
    out = cutoff(curve, T)
    out.update(curve=curve, side=a.shape[0], p1=p1, p2=p2)
    return out


def frc(E, H, N=255, T=T_DEFAULT, inputs_are_levels=False):
    """(B, h, w) or (B, 1, h, w) arrays -> (curve (B, S/2 + 1) float64, cut (B,) float64, the per-image dicts)"""
    E, H = (np.asarray(t).reshape(-1, *np.asarray(t).shape[-2:]) for t in (E, H))
    each = [frc_one(e, h, N, T, inputs_are_levels) for e, h in zip(E, H)]
    return np.stack([o["curve"] for o in each]), np.array([o["cut"] for o in each]), each


def cut_bound(o, bound, T=T_DEFAULT):
    """the curve bound propagated through step 7: 2 bound / ((p - FRC[r]) S/2) plus one spacing; 0 where nothing crosses (the
    cutoff is 1.0) and where ring 0 is already under T (it is 0.0): the marking rule keeps the curve off T there"""
    if o["r"] is None or o["p"] < T:
        return 0.0
    return 2.0 * bound / ((o["p"] - o["q"]) * (o["side"] // 2)) + float(np.spacing(o["cut"]))
