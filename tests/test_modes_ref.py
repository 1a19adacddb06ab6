"""Test infrastructure for the test modes (dlib/utils/utils_model.py, csrc/tta.hip): a toy model that is exact in
float32 and a plain-torch restatement of the five modes, one forward per view or tile, the way the reference runs them
(utils_model.py:51-214).  tools/make_golden_test_modes.py checks the restatement against the reference bit for bit and
writes tests/golden/g54_test_modes.npz; the CPU and GPU tests read the .npz and this module, nothing else.

The toy model, y = up(x) + up(x) shifted down / 2 + up(x) shifted right / 4 + a ramp in the coordinates of what it was given:
  * works for any batch and channel count (every plane on its own),
  * is not equivariant under any of the seven non-identity views (the shifts go down and right only, with different weights,
    and the ramp has a different slope per axis),
  * reads a neighbour along each axis with zero fill, and its ramp restarts in every tile: a tile's border rows differ from
    the whole image's, so the overlap of the split and the crops matter,
  * is exact: inputs are multiples of 2^-8 in [0, 1), the weights powers of two, the ramp multiples of 2^-12 below 1 -- every
    value is a multiple of 2^-12 below 4, the sum of eight of them a multiple of 2^-12 below 32 (17 bits), and so is its
    eighth.  Any summation order, CPU or GPU, gives the same bits."""
import numpy as np
import torch

GOLDEN = "g54_test_modes.npz"

# name: (shape of L, refield, min_size, sf, modulo)
CASES = {
    "A": ((2, 1, 21, 27), 4, 8, 2, 1),      # two split levels, 8 x 12 leaves
    "B": ((1, 1, 45, 53), 4, 8, 2, 1),      # three levels, 12 x 12 leaves
    "C": ((1, 2, 5, 9), 4, 8, 3, 4),        # no split, padded to 8 x 12 (12 x 8 under the turning views), two planes per image
    "D": ((2, 1, 7, 6), 4, 8, 2, 4),        # h w <= min_size^2: the padded base case of the split, 8 x 8
    "E": ((1, 1, 16, 16), 4, 8, 2, 1),      # square: all eight views share a shape; one level, 12 x 12 leaves
}


def make_input(name):
    shape = CASES[name][0]
    g = torch.Generator().manual_seed(5400 + ord(name))
    return torch.randint(0, 256, shape, generator=g).to(torch.float32) / 256.0


def toy_model(sf):
    def model(x):
        h, w = x.shape[-2:]
        u = x.repeat_interleave(sf, dim=-2).repeat_interleave(sf, dim=-1)
        down, right = torch.zeros_like(u), torch.zeros_like(u)
        down[..., 1:, :] = u[..., :-1, :]
        right[..., :, 1:] = u[..., :, :-1]
        yy = torch.arange(h * sf, device=x.device, dtype=torch.float32)[:, None] * 2.0 ** -10
        xx = torch.arange(w * sf, device=x.device, dtype=torch.float32)[None, :] * 2.0 ** -12
        return u + 0.5 * down + 0.25 * right + (yy + xx)
    return model


# ---- the five modes, one forward per view / tile ---------------------------------------------------------------------
def view(x, m):
    """dihedral view m of the last two axes (the reference's augment_img_tensor4, utils_image.py:490-508)"""
    turns, flip = {0: (0, False), 1: (1, True), 2: (0, True), 3: (3, False), 4: (2, True), 5: (1, False), 6: (2, False),
                   7: (3, True)}[m]
    y = torch.rot90(x, turns, dims=(-2, -1)) if turns else x
    return torch.flip(y, dims=(-2,)) if flip else y


INVERSE = {0: 0, 1: 1, 2: 2, 3: 5, 4: 4, 5: 3, 6: 6, 7: 7}


def pad_to(x, modulo):
    h, w = x.shape[-2:]
    return torch.nn.functional.pad(x, (0, -w % modulo, 0, -h % modulo), mode="replicate")


def ref_pad(model, L, modulo, sf):
    h, w = L.shape[-2:]
    return model(pad_to(L, modulo))[..., :h * sf, :w * sf]


def ref_split(model, L, refield, min_size, sf, modulo):
    h, w = L.shape[-2:]
    if h * w <= min_size ** 2:
        return ref_pad(model, L, modulo, sf)
    qh, qw = (h // 2 // refield + 1) * refield, (w // 2 // refield + 1) * refield
    assert qh <= h and qw <= w, "a quadrant longer than the side"
    direct = h * w <= 4 * min_size ** 2
    rows = []
    for y0, keep_y in ((0, slice(0, h // 2 * sf)), (h - qh, slice((qh - (h - h // 2)) * sf, qh * sf))):
        parts = []
        for x0, keep_x in ((0, slice(0, w // 2 * sf)), (w - qw, slice((qw - (w - w // 2)) * sf, qw * sf))):
            q = L[..., y0:y0 + qh, x0:x0 + qw]
            e = model(q) if direct else ref_split(model, q, refield, min_size, sf, modulo)
            parts.append(e[..., keep_y, keep_x])
        rows.append(torch.cat(parts, dim=-1))
    return torch.cat(rows, dim=-2)


def ref_ensemble(one, L, inverse=INVERSE):
    outs = [view(one(view(L, m)), inverse[m]) for m in range(8)]
    return torch.stack(outs, dim=0).mean(dim=0)


def ref_test_mode(model, L, mode, refield=32, min_size=256, sf=1, modulo=1, inverse=INVERSE):
    if mode == 0:
        return model(L)
    if mode == 1:
        return ref_pad(model, L, modulo, sf)
    if mode == 2:
        return ref_split(model, L, refield, min_size, sf, modulo)
    if mode == 3:
        return ref_ensemble(lambda v: ref_pad(model, v, modulo, sf), L, inverse)
    if mode == 4:
        return ref_ensemble(lambda v: ref_split(model, v, refield, min_size, sf, modulo), L, inverse)
    raise ValueError(mode)


def load_golden(path):
    z = np.load(path)
    return {name: {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")} for name in CASES}
