"""The test modes of the reference's ``dlib/utils/utils_model.py`` (:51-214) -- padding to a modulus, splitting an image
too large for one forward into overlapping quadrants, the x8 geometric self-ensemble, and both -- on the libsrhip path.

Same names, signatures and results as the reference: ``test_mode(model, L, mode, refield, min_size, sf, modulo)``,
``test``, ``test_pad``, ``test_split``, ``test_x8``, ``test_split_x8``.  ``model`` is any callable ``[B, C, h, w] ->
[B, C, sf h, sf w]`` on the GPU.  The reference makes one forward per view or tile (8, 4^depth, 8 * 4^depth) and slices,
rotates and stitches on the host in between; here

  * ``split_plan`` flattens the recursion of ``test_split_fn`` (:127-164) into its 4^depth leaves (pure host arithmetic),
  * one ``srhip_view_gather`` launch per tile shape cuts, turns and pads every tile of every view (at most two shapes:
    the views that swap the axes and those that do not),
  * the tiles run through ``model`` in batches of at most ``max_batch`` tile-images (an extra keyword, default 8: the batch
    the engines are tested at), all batches of one shape before the other,
  * one ``srhip_view_merge`` launch undoes the views, crops every tile to what it owns and averages in a fixed order.

Everything runs under ``torch.no_grad()``; a CPU tensor raises (GPU only, as everywhere in this package)."""
import torch

__all__ = ["test_mode", "test", "test_pad", "test_split", "test_x8", "test_split_x8", "split_plan", "split_levels"]


def _ceil_to(v, modulo):
    return -(-v // modulo) * modulo


def split_levels(h, w, refield=32, min_size=256, modulo=1):
    """The shapes of ``test_split_fn``'s recursion on an h x w image: ``(levels, (th, tw))``.  ``levels[l]`` is the (h, w) of
    the image a call at depth l sees -- all four quadrants of a level have one shape, so a depth has one -- and the last
    entry is the leaf; (th, tw) is what the model receives for a leaf.  The reference's asymmetry is kept: a level with
    h w <= 4 min_size^2 hands its quadrants to the model as they are, only an image with h w <= min_size^2 (the recursion's
    base case) is padded to ``modulo``.

    Raises ValueError where the reference's slices would run off the image: a side shorter than its quadrant length
    (side // 2 // refield + 1) * refield at a level that splits (the reference's negative slice start wraps around there)."""
    h, w, refield, min_size, modulo = int(h), int(w), int(refield), int(min_size), int(modulo)
    if h < 1 or w < 1 or refield < 1 or min_size < 1 or modulo < 1:
        raise ValueError(f"split: h, w, refield, min_size, modulo must be positive (got {h}, {w}, {refield}, {min_size}, {modulo})")
    levels = [(h, w)]
    while True:
        if h * w <= min_size ** 2:
            return levels, (_ceil_to(h, modulo), _ceil_to(w, modulo))
        qh, qw = (h // 2 // refield + 1) * refield, (w // 2 // refield + 1) * refield
        if qh > h:
            raise ValueError(f"split: the height {h} of a level is shorter than its quadrants ({qh} = (height // 2 // refield + 1)"
                             f" * refield, refield {refield}): choose a smaller refield or a larger min_size")
        if qw > w:
            raise ValueError(f"split: the width {w} of a level is shorter than its quadrants ({qw} = (width // 2 // refield + 1)"
                             f" * refield, refield {refield}): choose a smaller refield or a larger min_size")
        last = h * w <= 4 * min_size ** 2
        h, w = qh, qw
        levels.append((h, w))
        if len(levels) > 9:
            raise ValueError("split: more than 8 levels (4^8 tiles per view); choose a larger min_size")
        if last:
            return levels, (h, w)


def split_plan(h, w, refield=32, min_size=256, modulo=1):
    """``test_split_fn`` flattened: one record per leaf, in the order the reference's recursion reaches them (top-left,
    top-right, bottom-left, bottom-right, depth first): ``{"src": (y0, x0, h, w), "pad": (th, tw), "dst": (y0, x0, h, w)}``
    in low-resolution pixels -- the rectangle of the image the leaf is cut from, the size the model receives it in, and
    the rectangle of the result it owns (inside ``src``; times sf in the output).  4^depth leaves of one shape."""
    levels, pad = split_levels(h, w, refield, min_size, modulo)
    leaves = [dict(src=(0, 0) + levels[0], pad=pad, dst=(0, 0) + levels[0])]
    for (hl, wl), (qh, qw) in zip(levels[:-1], levels[1:]):
        nxt = []
        for leaf in leaves:
            sy, sx = leaf["src"][:2]
            dy0, dx0, dh, dw = leaf["dst"]
            for by in (0, 1):
                for bx in (0, 1):
                    # the quadrant's rectangle, and the half of the level it owns, both in image coordinates
                    qy, qx = sy + by * (hl - qh), sx + bx * (wl - qw)
                    oy0, oy1 = (sy, sy + hl // 2) if by == 0 else (sy + hl // 2, sy + hl)
                    ox0, ox1 = (sx, sx + wl // 2) if bx == 0 else (sx + wl // 2, sx + wl)
                    y0, y1 = max(oy0, dy0), min(oy1, dy0 + dh)
                    x0, x1 = max(ox0, dx0), min(ox1, dx0 + dw)
                    nxt.append(dict(src=(qy, qx, qh, qw), pad=pad, dst=(y0, x0, max(y1 - y0, 0), max(x1 - x0, 0))))
        leaves = nxt
    return leaves


def _view_rect(mode, rect, H, W):
    """The rectangle of the H x W image that rectangle ``rect`` of its view ``mode`` shows: view(L)[rect] is
    view(L[that rectangle])."""
    y0, x0, h, w = rect
    if mode & 1:
        a0, a1, b0, b1 = x0, x0 + w, y0, y0 + h            # the view's columns walk the image's rows
    else:
        a0, a1, b0, b1 = y0, y0 + h, x0, x0 + w
    if mode in (2, 3, 6, 7):
        a0, a1 = H - a1, H - a0
    if mode >= 4:
        b0, b1 = W - b1, W - b0
    return a0, b0, a1 - a0, b1 - b0


def _run(model, L, modes, split, refield, min_size, sf, modulo, max_batch):
    """views ``modes`` of L, each split (``split``) or whole, through ``model`` in batches; the mean of the inverse views"""
    from srhip import ops
    if not (torch.is_tensor(L) and L.is_cuda):
        raise RuntimeError("test modes (libsrhip) run on the GPU only: move the model and the input to cuda; there is no "
                           "CPU fallback")
    if L.dim() != 4 or L.dtype != torch.float32:
        raise ValueError(f"test modes: L is a float32 image batch [B, C, h, w] (got {L.dtype}, {tuple(L.shape)})")
    sf, max_batch = int(sf), int(max_batch)
    if sf < 1 or max_batch < 1:
        raise ValueError(f"test modes: sf >= 1 and max_batch >= 1 (got {sf}, {max_batch})")
    B, C, H, W = L.shape
    N = B * C
    with torch.no_grad():
        src = L.detach().contiguous()
        groups, views = {}, []                               # tile shape -> jobs;  per view: (shape, first job, levels)
        for m in modes:
            fh, fw = (W, H) if m & 1 else (H, W)
            if split:
                levels, pad = split_levels(fh, fw, refield, min_size, modulo)
                rects = [leaf["src"] for leaf in split_plan(fh, fw, refield, min_size, modulo)]
            else:
                levels, pad = [(fh, fw)], (_ceil_to(fh, int(modulo)), _ceil_to(fw, int(modulo)))
                rects = [(0, 0, fh, fw)]
            jobs = groups.setdefault(pad, [])
            views.append((pad, len(jobs), levels, m))
            jobs.extend(_view_rect(m, r, H, W) + (m,) for r in rects)
        outs = {}
        for (th, tw), jobs in groups.items():                # every batch of one shape before the next shape
            tiles = ops.view_gather(src.view(N, H, W), jobs, th, tw).view(len(jobs) * B, C, th, tw)
            E = torch.empty(len(jobs) * B, C, th * sf, tw * sf, dtype=torch.float32, device=L.device)
            for i in range(0, len(jobs) * B, max_batch):
                x = tiles[i:i + max_batch]
                y = model(x)
                if y.numel() != x.shape[0] * C * th * sf * tw * sf:
                    raise ValueError(f"test modes: the model turned {tuple(x.shape)} into {tuple(y.shape)}, not into "
                                     f"[{x.shape[0]}, {C}, {th * sf}, {tw * sf}] (sf {sf})")
                E[i:i + max_batch].copy_(y.reshape(x.shape[0], C, th * sf, tw * sf))
            outs[(th, tw)] = E.view(len(jobs), N, th * sf, tw * sf)
        descs = []
        for pad, first, levels, m in views:
            n_leaves = 4 ** (len(levels) - 1)
            descs.append((outs[pad][first:first + n_leaves], m, pad[0], pad[1], levels))
        return ops.view_merge(descs, N, H, W, sf).view(B, C, H * sf, W * sf)


def test_mode(model, L, mode=0, refield=32, min_size=256, sf=1, modulo=1, max_batch=8):
    """(0) normal  (1) pad to ``modulo``  (2) split  (3) x8 self-ensemble  (4) split and x8 -- utils_model.py:51-88.
    refield: receptive field of the net, the overlap of the split's quadrants is a multiple of it; min_size: images of up
    to min_size^2 pixels go through the model whole (modes 2, 4); sf: scale factor of the model; modulo: 1 when splitting."""
    if mode == 0:
        return test(model, L)
    if mode == 1:
        return test_pad(model, L, modulo, sf, max_batch=max_batch)
    if mode == 2:
        return test_split(model, L, refield, min_size, sf, modulo, max_batch=max_batch)
    if mode == 3:
        return test_x8(model, L, modulo, sf, max_batch=max_batch)
    if mode == 4:
        return test_split_x8(model, L, refield, min_size, sf, modulo, max_batch=max_batch)
    raise ValueError(f"test_mode: mode 0..4 (got {mode!r})")


def test(model, L):
    """normal (0): utils_model.py:98-100"""
    if not (torch.is_tensor(L) and L.is_cuda):
        raise RuntimeError("test modes (libsrhip) run on the GPU only: move the model and the input to cuda; there is no "
                           "CPU fallback")
    with torch.no_grad():
        return model(L)


def test_pad(model, L, modulo=16, sf=1, max_batch=8):
    """pad (1): replicate-pad right / bottom to a multiple of ``modulo``, crop the output (utils_model.py:110-117)"""
    return _run(model, L, (0,), False, 1, 1, sf, modulo, max_batch)


def test_split(model, L, refield=32, min_size=256, sf=1, modulo=1, max_batch=8):
    """split (2): utils_model.py:127-176"""
    return _run(model, L, (0,), True, refield, min_size, sf, modulo, max_batch)


def test_x8(model, L, modulo=1, sf=1, max_batch=8):
    """x8 (3): the mean over the eight flips / rotations of the input of the output turned back (utils_model.py:186-195)"""
    return _run(model, L, range(8), False, 1, 1, sf, modulo, max_batch)


def test_split_x8(model, L, refield=32, min_size=256, sf=1, modulo=1, max_batch=8):
    """split and x8 (4): utils_model.py:205-214"""
    return _run(model, L, range(8), True, refield, min_size, sf, modulo, max_batch)
