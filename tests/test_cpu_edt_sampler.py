"""Host side of the device 'edt' / 'edt*roi' / Otsu crop sampler (dlib/datasets/dataset_dpsr.py: origin_weights,
check_origin_total; dlib/datasets/lowres.py: otsu_from_counts).

The weight formula the HIP kernels evaluate is stated once in numpy (origin_weights); normalised, it is the probability
vector the REFERENCE handed to np.random.multinomial (g32).  The counts-based Otsu function is otsu_threshold on the
image's histogram.  A tile whose total weight is not finite is refused by name."""
import math
import os
import subprocess

import numpy as np
import pytest

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def candidates(img, th, P):
    """(d2, roi) at the pixel every candidate origin looks at: exact integer squared distances from scipy's float EDT"""
    from scipy.ndimage import distance_transform_edt
    h, w = img.shape
    lo, hi = P // 2, math.ceil(P / 2)
    roi = img >= th
    d2 = np.rint(distance_transform_edt(roi) ** 2).astype(np.int64)
    return d2[lo:h - hi, lo:w - hi], roi[lo:h - hi, lo:w - hi]


def test_origin_weights_normalised_are_the_reference_probabilities():
    from dlib.datasets.dataset_dpsr import origin_weights
    g = np.load(os.path.join(G, "g32_patch_sampler_edt.npz"))
    for name in ("a", "b"):
        img = g[f"{name}/img"]
        P, th = (int(v) for v in g[f"{name}/cfg"])
        d2, roi = candidates(img, th, P)
        for style, tag in (("edt", "edt"), ("edt*roi", "edtxroi")):
            w = origin_weights(d2, roi, style)
            assert w.dtype == np.float64 and w.shape == (img.shape[0] - P, img.shape[1] - P)
            p = (w / w.sum()).reshape(-1)
            want = g[f"{name}/{tag}_pvals"]
            print(name, style, "max relative difference", (np.abs(p - want) / want).max())
            assert (np.abs(p - want) <= 1e-14 * want).all(), (name, style)
        # 'roi' with a per-tile threshold: the weights of roi_probabilities
        from dlib.datasets.dataset_dpsr import roi_probabilities
        w = origin_weights(d2, roi, "roi")
        want = roi_probabilities(img, float(th), P)
        assert (np.abs(w / w.sum() - want) <= 1e-14 * want).all()


def test_otsu_from_counts_is_otsu_threshold():
    from dlib.datasets.lowres import otsu_from_counts, otsu_threshold
    rng = np.random.RandomState(0)
    img = np.where(rng.rand(64, 64) < 0.3, rng.randint(150, 200, (64, 64)), rng.randint(5, 40, (64, 64))).astype(np.uint8)
    th = otsu_threshold(img, 256)
    got = otsu_from_counts(np.bincount(img.reshape(-1), minlength=256))
    assert got == th and type(got) is type(th) and 39 <= got < 150
    const = np.full((9, 7), 37, np.uint8)
    assert otsu_from_counts(np.bincount(const.reshape(-1), minlength=256)) == otsu_threshold(const, 256) == 37
    # two grey levels at the ends of the range, int32 counts as the device histogram returns them
    two = np.zeros((4, 4), np.uint8)
    two[2:] = 255
    assert otsu_from_counts(np.bincount(two.reshape(-1), minlength=256).astype(np.int32)) == otsu_threshold(two, 256)


def test_int_threshold_is_the_float_comparison_on_uint8():
    from dlib.datasets.dataset_dpsr import int_threshold
    v = np.arange(256, dtype=np.uint8)
    for th in (0., 6.5, 7., 7.000001, 254.5, 255., 300., -3.2):
        assert np.array_equal(v >= th, v.astype(np.int64) >= int_threshold(th)), th


def test_non_finite_total_is_refused_by_tile_name():
    from dlib.datasets.dataset_dpsr import origin_weights, check_origin_total
    d2 = np.full((4, 6), 9, np.int64)
    d2[2, 3] = 800 ** 2                                   # exp(800) overflows fp64
    roi = np.ones((4, 6), bool)
    w = origin_weights(d2, roi, "edt*roi")
    assert not np.isfinite(w.sum())
    with pytest.raises(ValueError, match="t/h_7.tif"):
        check_origin_total(w.sum(), "t/h_7.tif", "edt*roi")
    # the same distances are fine for 'edt' (no exponential)
    assert check_origin_total(origin_weights(d2, roi, "edt").sum(), "t/h_7.tif", "edt") == 801 + 23 * 4


def test_origin_tile_struct_mirrors_the_header(tmp_path):
    """srhip_origin_tile as ops.py uploads it to the device table: sizeof and the offset of every field, asked of the C
    compiler on the plain-C header"""
    import ctypes
    from srhip import ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [f[0] for f in ops._OriginTile._fields_]
    body = '  printf("%zu\\n", sizeof(srhip_origin_tile));\n' + "".join(
        f'  printf("%zu\\n", offsetof(srhip_origin_tile, {f}));\n' for f in fields)
    src = tmp_path / "tile.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "srhip.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(tmp_path / "tile")], check=True)
    out = [int(v) for v in subprocess.run([str(tmp_path / "tile")], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(ops._OriginTile)
    assert out[1:] == [getattr(ops._OriginTile, f).offset for f in fields]
    assert ops.ORIGIN_STYLES == {"roi": 0, "edt": 1, "edt*roi": 2}
