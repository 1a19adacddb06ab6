"""numpy restatement of the dropout masks of srhip_dropout (include/srhip.h), and a torch stand-in for ops.dropout built on it.

keep(e) for the element with global index e, under a 64-bit seed and a site number:
    counter = (low 32 bits of e // 4, high 32 bits of e // 4, site, 0), key = (low, high 32 bits of the seed),
    word = output word e % 4 of Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11:
    multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten rounds),
    keep iff word >= thr, thr = round(p 2^32).
KAT: the known-answer vectors of Philox4x32-10 (Random123's kat_vectors), (counter, key, output)."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF

KAT = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK32,) * 4, (MASK32,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays (or scalars) of 32-bit words held in uint64: the four output words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & np.uint64(MASK32) for c in (c0, c1, c2, c3))
    k0, k1 = int(k0) & MASK32, int(k1) & MASK32
    sh, m32 = np.uint64(32), np.uint64(MASK32)
    for _ in range(10):
        p0, p1 = c0 * np.uint64(M0), c2 * np.uint64(M1)                  # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> sh) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c0, c1, c2, c3


def threshold(p):
    """thr = round(p 2^32) (kept below 2^32) and scale = 1 / (1 - p) as the host passes them"""
    assert 0.0 <= p < 1.0, p
    return min(int(round(p * 4294967296.0)), MASK32), 1.0 / (1.0 - p)


def words(seed, site, offset, n):
    """the 32-bit word of each of the n elements offset .. offset + n - 1 (uint64 array)"""
    e = np.arange(int(offset), int(offset) + int(n), dtype=np.uint64)
    g = e >> np.uint64(2)
    w = philox4x32_10(g & np.uint64(MASK32), g >> np.uint64(32), np.full(g.shape, int(site), dtype=np.uint64),
                      np.zeros(g.shape, dtype=np.uint64), int(seed) & MASK32, (int(seed) >> 32) & MASK32)
    lane = (e & np.uint64(3)).astype(np.int64)
    return np.choose(lane, w)


def mask(seed, site, offset, n, p):
    """bool [n]: which of the elements offset .. offset + n - 1 are kept"""
    return words(seed, site, offset, n) >= np.uint64(threshold(p)[0])


def dropout_standin(x, out, seed, site, p, offset=0):
    """ops.dropout on torch tensors of any device, in float32 arithmetic: out = keep ? x * scale : 0 (out may be x)"""
    import torch
    thr, scale = threshold(p)
    m = torch.from_numpy(mask(int(seed.item()) if hasattr(seed, "item") else int(seed), site, offset, x.numel(), p))
    xs = x.reshape(-1) * torch.tensor(scale, dtype=torch.float32).to(x.device)
    out.reshape(-1).copy_(torch.where(m.to(x.device), xs, torch.zeros_like(xs)))
    return out
