"""The image decorrelation analysis of include/srhip.h (srhip_metrics_decorr_lv) stated in numpy float64, the same statement
through a direct DFT in np.longdouble (the reference's own rounding), and the rule that marks an image whose result hangs on a
decision taken by a hair.

Steps as the header numbers them.  1 - 3: Q_N levels, x = level / N, the centred S x S square, the separable periodic Hann
window, one unnormalised FFT2 (tests/frc_ref.py: ``windowed``).  4: no mean subtraction, every sum runs over the rings 2 .. S/2.
5: A_q = sum |F|, Q_q = sum |F|^2, n_q over the FRC's integer rings.  6: d_sigma(r) = sum_{q<=r} g A_q / sqrt((sum_q g^2 Q_q)
sum_{q<=r} n_q) with g_sigma(q) = -expm1(-2 pi^2 sigma^2 q^2 / S^2).  7: the peak search, written here exactly as the header words
it, one argmax per m (quadratic; the kernel does it in one pass).  8: curve 0, bank 1 from sigma_max = S / q0 down to 0.15, bank 2
around the best of bank 1.  9: ring, cut = ring / (S/2), amp, sigma."""
import numpy as np

import frc_ref as R

PEAK_DROP = 5e-4
SIGMA_MIN = 0.15
NBANK = 10
NCURVE = 1 + 2 * NBANK
MARK = 1e-10             # an image with a decision of steps 7 - 8 taken by less than this is marked: its rings may jump


def ring_stats(F):
    """F (S, S) complex -> A, Q in the real dtype of F, n int64, each (S/2 + 1,)"""
    m2 = F.real ** 2 + F.imag ** 2
    ring = R.ring_index(F.shape[-1])
    return R.ring_sums(np.sqrt(m2)), R.ring_sums(m2), np.bincount(ring[ring >= 0], minlength=F.shape[-1] // 2 + 1)


def highpass(sigma, S, dtype=np.float64):
    """g_sigma on the rings 0 .. S/2; sigma = 0: no filter"""
    q = np.arange(S // 2 + 1).astype(dtype)
    if sigma == 0:
        return np.ones_like(q)
    pi = np.pi if dtype == np.float64 else dtype(4) * np.arctan(dtype(1))
    return -np.expm1(-2 * pi ** 2 * dtype(sigma) ** 2 * q ** 2 / dtype(S) ** 2)


def curve_of(A, Q, n, sigma):
    """step 6 -> (S/2 + 1,) in the dtype of A; rings 0 and 1 are 0"""
    S = 2 * (len(A) - 1)
    g = highpass(sigma, S, A.dtype.type)
    num = np.cumsum((g * A)[2:])
    den = np.sum((g * g * Q)[2:]) * np.cumsum(n[2:]).astype(A.dtype)
    ok = den > 0
    d = np.zeros(len(A), dtype=A.dtype)
    d[2:] = np.where(ok, num / np.sqrt(np.where(ok, den, 1)), 0)
    return d


def peak(d):
    """step 7 -> (ring, amp, the smallest margin of a decision taken on the way)"""
    d = np.asarray(d, dtype=np.float64)
    m, margin = len(d) - 1, np.inf
    while True:
        seg = d[2:m + 1]
        i = int(np.argmax(seg)) + 2                               # the first one
        if len(seg) > 1:
            margin = min(margin, float(d[i] - np.delete(seg, i - 2).max()))
        if i == 2:
            return 0, 0.0, margin
        if i == m:
            m -= 1
            continue
        drop = float(d[i] - d[i:m + 1].min())
        margin = min(margin, abs(drop - PEAK_DROP))
        if drop >= PEAK_DROP:
            return i, float(d[i]), margin
        m -= 1


def bank(s_from, s_to):
    return np.exp(np.linspace(np.log(s_from), np.log(s_to), NBANK))


def analyse(A, Q, n):
    """steps 6 - 9 on the ring statistics -> dict(ring, cut, amp, sigma, best, curves (21, S/2 + 1), peaks (21,), amps, sigmas,
    margin, marked)"""
    A, Q = np.asarray(A, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    half = len(A) - 1
    S = 2 * half
    curves, peaks = np.zeros((NCURVE, half + 1)), np.zeros(NCURVE, dtype=np.int64)
    amps, sigmas, margin = np.zeros(NCURVE), np.zeros(NCURVE), np.inf

    def run(j, sigma):
        nonlocal margin
        curves[j] = curve_of(A, Q, n, sigma)
        peaks[j], amps[j], mg = peak(curves[j])
        sigmas[j] = sigma
        margin = min(margin, mg)
    run(0, 0.0)
    s_max = S / peaks[0] if peaks[0] else S / 2
    for k, s in enumerate(bank(s_max, SIGMA_MIN)):
        run(1 + k, s)
    best = int(np.argmax(peaks[:1 + NBANK]))                      # the largest ring, the lowest index among equals: exact
    if best >= 1:
        for k, s in enumerate(bank(sigmas[max(best - 1, 1)], sigmas[min(best + 1, NBANK)])):
            run(1 + NBANK + k, s)
    best = int(np.argmax(peaks))
    return dict(ring=int(peaks[best]), cut=peaks[best] / half, amp=amps[best], sigma=sigmas[best], best=best, side=S, curves=curves,
                peaks=peaks, amps=amps, sigmas=sigmas, margin=margin, marked=bool(margin < MARK))


def decorr_one(img, N=255, inputs_are_levels=False, fft2=np.fft.fft2):
    """one (h, w) image -> the dict of ``analyse`` plus A, Q, n"""
    A, Q, n = ring_stats(fft2(R.windowed(img, N, inputs_are_levels)))
    out = analyse(A, Q, n)
    out.update(A=A, Q=Q, n=n)
    return out


def decorr(X, N=255, inputs_are_levels=False):
    """(B, h, w) or (B, 1, h, w) -> the per-image dicts"""
    X = np.asarray(X)
    return [decorr_one(x, N, inputs_are_levels) for x in X.reshape(-1, *X.shape[-2:])]


def curves_longdouble(img, sigmas, N=255, inputs_are_levels=False):
    """the 21 curves of given widths (``analyse``'s 'sigmas'; 0 behind curve 0: there was no bank 2, the curve is 0) through the
    direct np.longdouble DFT, ring sums, filters and quotients in np.longdouble"""
    A, Q, n = ring_stats(R.dft2_longdouble(R.windowed(img, N, inputs_are_levels)))
    return np.stack([curve_of(A, Q, n, s) if j == 0 or s > 0 else np.zeros(len(A), dtype=A.dtype) for j, s in enumerate(sigmas)])
