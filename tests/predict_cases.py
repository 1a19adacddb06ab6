"""Statements and inputs of the prediction I/O tests (srhip_ingest_pad, srhip_emit_uint, srhip/predict.py).

tests/test_cpu_predict.py checks the statements against hand-computed values and the inputs for the properties the GPU
tests rely on; tests/test_gpu_predict.py gates the kernels, bit for bit, against the same statements.  Both import them from
here, so the GPU tests cannot drift from what was checked."""
import numpy as np
import torch


# ---------------------------------------------------------------- ingest
def ingest_value(v, in_max):
    """the reference's uint2single / uint162single with a white level: the quotient in double, rounded to float32"""
    return np.float32(np.minimum(v, in_max) / float(in_max))


def ingest_pad_ref(pages, in_max, Hp, Wp):
    """pages [B, H, W] uint8 / uint16 (numpy) -> float32 tensor [B, Hp, Wp]: ingest_value, then the cat + flip lines of
    _forward_with_padding (rows, then the columns of the row-padded image)"""
    B, H, W = pages.shape
    im = torch.from_numpy(ingest_value(pages, in_max))[:, None]
    h_pad, w_pad = Hp - H, Wp - W
    assert 0 <= h_pad <= H and 0 <= w_pad <= W
    im = torch.cat([im, torch.flip(im[:, :, H - h_pad:, :], [2])], 2)
    im = torch.cat([im, torch.flip(im[:, :, :, W - w_pad:], [3])], 3)
    return im[:, 0].contiguous()


# (H, W) -> (Hp, Wp): a whole extra window in one axis and 7 columns in the other; an odd height; the pad equal to the size
# (the limit); no pad with an odd row length
INGEST_SHAPES = (((16, 17), (24, 24)), ((9, 8), (16, 16)), ((8, 8), (16, 16)), ((16, 17), (16, 17)))
INGEST_TOO_SMALL = ((7, 8), (16, 16))
# (dtype, in_max): the two defaults, and 12-bit data in a 16-bit container
INGEST_RANGES = ((np.uint8, 255), (np.uint16, 65535), (np.uint16, 4095))


def ingest_pages(dtype, in_max, B, H, W, seed=0):
    """random pages over the whole range of the dtype; every other pixel is drawn from 0 .. in_max, so that both sides of a
    white level below the dtype's range are well populated; the extremes are present"""
    rng = np.random.RandomState(seed)
    top = np.iinfo(dtype).max
    a = rng.randint(0, top + 1, size=(B, H, W))
    low = rng.randint(0, in_max + 1, size=(B, H, W))
    a = np.where(rng.rand(B, H, W) < 0.5, a, low)
    a.reshape(-1)[:4] = (0, top, in_max, min(in_max + 1, top))
    return a.astype(dtype)


# ---------------------------------------------------------------- emit
def emit_value(x, out_max):
    """the reference's tensor2uint / single2uint16 in numpy: clip, ONE float32 product, round half to even"""
    x = np.asarray(x, dtype=np.float32)
    c = np.where(np.isnan(x), np.float32(0), np.clip(x, np.float32(0), np.float32(1))).astype(np.float32)
    return np.rint(c * np.float32(out_max)).astype(np.int64)


def emit_ref(x, out_max):
    """the same in torch on the CPU, as the reference writes it (finite inputs)"""
    return (x.clamp(0, 1) * out_max).round()


EMIT_B, EMIT_HS, EMIT_WS, EMIT_HO, EMIT_WO = 2, 24, 40, 19, 33


def halfway_values():
    """np.float32((k + 0.5) / m) and its two float32 neighbours for every k in 0 .. 255 (m = 255) and for 64 values of k
    spread over 0 .. 65534 (m = 65535): the product with m lands on or beside a rounding boundary, which is where a fused or
    a double-precision product would round to another integer than one float32 product"""
    out = []
    for m, ks in ((255, range(256)), (65535, np.linspace(0, 65534, 64).astype(np.int64))):
        for k in ks:
            c = np.float32((int(k) + 0.5) / m)
            out += [np.nextafter(c, np.float32(-1)), c, np.nextafter(c, np.float32(2))]
    return np.asarray(out, dtype=np.float32)


EMIT_SPECIALS = np.asarray([-0.0, 0.0, -1e-30, -0.25, -3.0, 1.0, 1.0000001, 1.5, 1e30, 0.5, 0.25, 0.99999994],
                           dtype=np.float32)


def emit_input(seed=0):
    """float32 [B, Hs, Ws], all finite: random values in (-0.25, 1.25) with the halfway values and the specials at positions
    inside the Ho x Wo crop.  Returns (x, positions): flat indices of the placed values."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(EMIT_B, EMIT_HS, EMIT_WS, generator=g) * 1.5 - 0.25
    placed = torch.from_numpy(np.concatenate([halfway_values(), EMIT_SPECIALS]))
    inside = torch.zeros(EMIT_B, EMIT_HS, EMIT_WS, dtype=torch.bool)
    inside[:, :EMIT_HO, :EMIT_WO] = True
    pos = inside.view(-1).nonzero()[:, 0]
    assert len(placed) < len(pos)
    pos = pos[torch.randperm(len(pos), generator=g)[:len(placed)]]
    x.view(-1)[pos] = placed
    return x, pos
