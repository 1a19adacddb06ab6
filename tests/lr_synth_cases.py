"""The cases that test_lr_synth.py (the numpy statement against scipy) and test_gpu_lr_synth.py (the kernels against the
statement) share: sources of srhip_psf_bin and the ramp of srhip_photon_noise."""
import numpy as np

# (source kind, B, H, W, s, sigma[, in_max])
PSF_CASES = (("float32", 1, 16, 24, 2, 0.0),
             ("uint8", 3, 24, 40, 4, 1.5),
             ("float32", 2, 64, 64, 8, 3.4),             # radius 14
             ("float32", 1, 8, 8, 2, 4.0),               # radius 16 > 8: repeated reflection
             ("uint16", 2, 40, 72, 4, 0.8, 4095),        # values above in_max present
             ("float32", 1, 6, 10, 2, 1.0))              # rows of 5 floats, no multiple of 4: the scalar path
PSF_IDS = [f"{c[0]}-{c[1]}x{c[2]}x{c[3]}-s{c[4]}-sigma{c[5]:g}" for c in PSF_CASES]


def psf_source(case):
    kind, B, H, W = case[:4]
    rng = np.random.default_rng(7 * H + W)
    if kind == "float32":
        x = rng.random((B, H, W), dtype=np.float32)
        x.reshape(-1)[:2] = (0.0, 1.0)
        return x
    if kind == "uint8":
        return rng.integers(0, 256, (B, H, W), dtype=np.uint8)
    x = rng.integers(0, 6000, (B, H, W)).astype(np.uint16)
    x.reshape(-1)[:3] = (0, 4095, 65535)
    return x


def noise_ramp(B, h, w):
    """float32 [B, 1, h, w] in [0, 1]: a cubic ramp -- a dark region of many small values, a bright one -- shifted per sample,
    with exact 0 and 1 in every sample"""
    n = h * w
    t = np.linspace(0.0, 1.0, n)
    x = np.stack([np.roll(t ** 3, 3 * b) for b in range(B)]).astype(np.float32)
    x[:, 0], x[:, n - 1] = 0.0, 1.0
    return x.reshape(B, 1, h, w)
