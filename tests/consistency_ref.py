"""numpy statement of srhip_consistency (include/srhip.h): the resolution-scaled error of NanoJ-SQUIRREL (Culley et al. 2018) on
the fixed two-bank grid of Gaussian blurs.

  weights   candidate q blurs with sigma = q s / 64 HR pixels: dlib.datasets.lowres.psf_bin_weights(q s / 64, s), 2 r + s float64
            weights, r = int(4 sigma + 0.5); they are data, the same bits in the float64 and in the longdouble chain
  model     b_q[i][j] = sum_t w[t] R[reflect(i s - r + t)][j],  R[y][j] = sum_t w[t] E[y][reflect(j s - r + t)]: taps ascending,
            every product and sum rounded on its own, no float32 in between
  sums      Sb, Sbb, Sbl, Sl, Sll over the n = h w pixels (np.sum: the order of a sum is not part of the statement)
  score     C_bl |C_bl| / (C_bb C_ll), C_xy = Sxy - Sx Sy / n; 0 when C_bb <= 0 or C_ll <= 0
  search    coarse q = 8 k, fine q = max(0, q_coarse + m - 8); a winner is the FIRST index of the largest score
  result    sigma, alpha = C_bl / C_bb, beta = (Sl - alpha Sb) / n, rsp = sign(score) sqrt(|score|),
            rse = sqrt(max(0, C_ll - C_bl^2 / C_bb) / n), q, n; residual = float32(double(L) - (alpha b + beta))

``dtype=np.longdouble`` runs the whole chain (correlations, sums, score, alpha, beta, rse) in extended precision on a given q
list: the statement's own rounding, e_ref of tests/consistency_cases.py."""
import numpy as np

from dlib.datasets import lowres

NQ, BANK = 128, 16


def sigma_of(q, s):
    return q * s / 64.0


def weights(q, s):
    return lowres.psf_bin_weights(sigma_of(q, s), s)


def reflect(i, n):
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def model(E, q, s, dtype=np.float64):
    """b_q of one page: E [s h, s w] -> [h, w] in ``dtype``"""
    w = weights(q, s).astype(dtype)
    r = (w.size - s) // 2

    def one_axis(a, axis):
        n = a.shape[axis]
        first = np.arange(n // s) * s - r
        acc = np.zeros(a.shape[:axis] + (n // s,) + a.shape[axis + 1:], dtype=dtype)
        for k in range(w.size):
            acc += w[k] * np.take(a, reflect(first + k, n), axis=axis)
        return acc
    return one_axis(one_axis(E.astype(dtype), 1), 0)


def sums(b, l):
    return b.sum(), (b * b).sum(), (b * l).sum(), l.sum(), (l * l).sum()


def figures(sm, n):
    """(score, alpha, beta, rsp, rse, degenerate) from the five sums, in their dtype"""
    sb, sbb, sbl, sl, sll = sm
    zero = sb * 0
    cbb, cll, cbl = sbb - sb * sb / n, sll - sl * sl / n, sbl - sb * sl / n
    if not (cbb > 0 and cll > 0):
        return zero, zero, sl / n, zero, np.sqrt(np.maximum(zero, cll) / n), True
    score = cbl * np.abs(cbl) / (cbb * cll)
    alpha = cbl / cbb
    root = np.sqrt(np.abs(score))
    return score, alpha, (sl - alpha * sb) / n, (-root if score < 0 else root), np.sqrt(np.maximum(zero, cll - cbl * cbl / cbb) / n), False


def first_largest(v):
    best = 0
    for k in range(1, len(v)):
        if v[k] > v[best]:
            best = k
    return best


def gap(v, qs, s):
    """by how much a bank was decided: the largest score minus the largest score of a DISTINCT candidate, one whose weights are
    not the winner's bit for bit (inf: there is none).  Duplicate q = 0 slots, and q = 1 beside q = 0 where both have the radius
    0, are the same candidate.  This asks more than a gap between distinct score VALUES would: two different candidates whose
    scores happen to agree in every bit give 0."""
    k = first_largest(v)
    wk = weights(int(qs[k]), s)
    rest = [float(v[j]) for j in range(len(v)) if not np.array_equal(weights(int(qs[j]), s), wk)]
    return float(v[k]) - max(rest) if rest else float("inf")


def consistency_one(E, L, s, dtype=np.float64, qs=None):
    """one page.  E float32 [s h, s w], L float32 [h, w].  ``qs``: run the 32 slots on this q list instead of searching (the
    longdouble chain on the float64 statement's decisions).  Returns a dict: qs (32,), scores (32,), q, sigma, alpha, beta, rsp,
    rse, n, degenerate, margin (coarse, fine), b (the winner's model image), residual (float32)."""
    h, w = L.shape
    assert E.shape == (s * h, s * w) and E.dtype == np.float32 and L.dtype == np.float32
    n = dtype(h * w)
    l = L.astype(dtype)
    cache = {}

    def slot(q):
        if q not in cache:
            b = model(E, q, s, dtype)
            sm = sums(b, l)
            cache[q] = (b, sm, figures(sm, n))
        return cache[q]
    coarse = [8 * k for k in range(BANK)]
    sc_c = [slot(q)[2][0] for q in (coarse if qs is None else qs[:BANK])]
    kc = first_largest(sc_c)
    fine = [max(0, coarse[kc] + m - 8) for m in range(BANK)] if qs is None else [int(q) for q in qs[BANK:]]
    sc_f = [slot(q)[2][0] for q in fine]
    kf = first_largest(sc_f)
    b, sm, (score, alpha, beta, rsp, rse, deg) = slot(fine[kf])
    q = 0 if deg else fine[kf]
    if deg:
        b = slot(0)[0]
    resid = (l - (alpha * b + beta)).astype(np.float32)
    return {"qs": np.array((coarse if qs is None else list(qs[:BANK])) + fine, dtype=np.int32), "scores": np.array(sc_c + sc_f, dtype=dtype),
            "q": q, "sigma": sigma_of(q, s), "alpha": alpha, "beta": beta, "rsp": rsp, "rse": rse, "n": h * w, "degenerate": deg,
            "margin": (gap(sc_c, coarse if qs is None else qs[:BANK], s), gap(sc_f, fine, s)), "b": b, "residual": resid, "sums": sm}


def consistency(E, L, s, dtype=np.float64):
    """a batch: E [B, s h, s w], L [B, h, w] -> the per-page dicts"""
    return [consistency_one(e, l, s, dtype) for e, l in zip(E, L)]


def margin(each):
    """per bank, the smallest ``gap`` over the pages"""
    return tuple(min(o["margin"][k] for o in each) for k in (0, 1))
