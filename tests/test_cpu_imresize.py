"""HR-only image sets, host side: ``dlib.utils.utils_image.imresize_np`` (the MATLAB-style antialiased bicubic down-scaling
behind the low-resolution image of a pair that has a high-resolution tile only, dataset_dpsr.py:798-824) against the
REFERENCE's own outputs (tests/golden/g51_imresize.npz, written by tools/make_golden_imresize.py), and the data sets
built on it.

Gate of the host function against g51: 2.4e-7 -- the reference forms weights and sums in float32, this restatement in
float64 with the same float32 image between the two passes; measured on random tiles the two sit one float32 ulp below 1
apart (1.19e-7), plus one for a different summation order."""
import os
import subprocess
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
HX = os.path.join(G, "hr_only_exp")
SIZES = [(40, 56), (64, 64), (72, 88), (36, 50), (37, 50), (33, 47), (16, 24), (24, 40)]
TOL_G51 = 2.4e-7
TOL_DEVICE = 1.2e-7      # device kernel against the host function: the two f64 sums may round apart by one f32 ulp


@pytest.fixture(scope="module")
def g51():
    return np.load(os.path.join(G, "g51_imresize.npz"))


def _unit(x):
    return np.float32(x / 255.) if x.dtype == np.uint8 else x


def test_imresize_np_against_the_reference_outputs(g51):
    from dlib.utils.utils_image import imresize_np
    n = 0
    for kind in ("u8", "f32"):
        for h, w in SIZES:
            x = _unit(g51[f"{kind}_{h}x{w}"])
            for s in (2, 4, 8):
                want = g51[f"{kind}_{h}x{w}_s{s}"]
                got = imresize_np(x, 1 / s, True)
                assert got.dtype == np.float32 and got.shape == want.shape == (-(-h // s), -(-w // s))
                err = np.abs(got.astype(np.float64) - want).max()
                assert err <= TOL_G51, (kind, h, w, s, err)
                assert 0.0 <= want.min() and want.max() <= 1.0          # the fixtures never leave the range
                n += 1
    assert n == 48


def test_imresize_np_takes_hw_and_hwc_and_sizes_that_do_not_divide(g51):
    from dlib.utils.utils_image import imresize_np
    x = g51["f32_40x56x3"]
    got = imresize_np(x, 1 / 2)
    assert got.shape == (20, 28, 3) and got.dtype == np.float32
    assert np.abs(got.astype(np.float64) - g51["f32_40x56x3_s2"]).max() <= TOL_G51
    for c in range(3):                                                  # a channel of an HWC image is that HW image
        assert np.array_equal(got[:, :, c], imresize_np(np.ascontiguousarray(x[:, :, c]), 1 / 2))
    assert np.array_equal(imresize_np(x[:, :, :1], 1 / 2)[:, :, 0], got[:, :, 0])
    y = imresize_np(g51["f32_37x50"], 1 / 4)
    assert y.shape == (10, 13)                                          # ceil(37 / 4) x ceil(50 / 4)
    assert np.abs(y.astype(np.float64) - g51["f32_37x50_s4"]).max() <= TOL_G51
    # float64 input is read as float32, as the reference's copy into a FloatTensor does
    assert np.array_equal(imresize_np(g51["f32_37x50"].astype(np.float64), 1 / 4), y)
    # a constant image stays constant (weights normalised per output pixel), a sharp edge overshoots: nothing is clipped
    assert np.abs(imresize_np(np.full((24, 40), 0.25, np.float32), 1 / 4) - 0.25).max() <= 6e-8
    edge = np.zeros((32, 32), np.float32)
    edge[:, 16:] = 1.0
    e = imresize_np(edge, 1 / 2)
    assert e.min() < 0.0 and e.max() > 1.0
    # an image so small that a live tap would mirror past the opposite border is refused
    with pytest.raises(ValueError):
        imresize_np(np.zeros((8, 8), np.float32), 1 / 8)


def test_weights_are_normalised_and_mirror_with_the_edge_repeated():
    from dlib.utils.utils_image import imresize_weights
    for n_in, s in ((16, 8), (37, 4), (50, 2)):
        n_out = -(-n_in // s)
        w, j = imresize_weights(n_in, n_out, 1 / s)
        assert w.shape == j.shape == (n_out, 4 * s + 2) and w.dtype == np.float64
        assert np.abs(w.sum(1) - 1.0).max() < 1e-15
        live = w != 0.0
        assert j[live].min() >= 0 and j[live].max() < n_in
    w, j = imresize_weights(16, 2, 1 / 8)
    # output pixel 0 sits at 1-based input coordinate 4.5: its taps start 12 pixels left of the image and mirror back
    assert j[0, :14].tolist() == [12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0, 0] and w[0, 0] == 0.0


def _hr_only_pairs(tmp_path, h=97, w=131):
    from PIL import Image
    d = tmp_path / "biosr" / "t"
    d.mkdir(parents=True)
    rng = np.random.RandomState(7)
    img = rng.randint(30, 200, size=(h, w)).astype(np.uint8)
    Image.fromarray(img, mode="L").save(d / "h_0.tif")
    pairs_h = {"t/h_0.tif": {"abs_path": str(d / "h_0.tif"), "low_path_key": "None_0"}}
    pairs_l = {"None_0": {"abs_path": "None_0", "high_path_key": "t/h_0.tif"}}
    return img, pairs_h, pairs_l


def test_eval_pairs_on_an_hr_only_set(tmp_path):
    """The refusal this build had ('... imresize_np, outside this build') is gone: l_im = imresize_np of the MOD-CROPPED
    tile / 255 in float32, l_path = h_path."""
    from dlib.utils.utils_dataloaders import EvalPairs, get_eval_loader
    from dlib.utils.utils_image import imresize_np
    img, pairs_h, pairs_l = _hr_only_pairs(tmp_path)
    ev = EvalPairs(types.SimpleNamespace(scale=2), pairs_h, pairs_l)
    assert ev.is_hr_only(0)
    it = ev[0]
    want = imresize_np(np.float32(img[:96, :130] / 255.), 1 / 2)
    assert it["l_im"].dtype == torch.float32 and tuple(it["l_im"].shape) == (1, 48, 65)
    assert tuple(it["h_im"].shape) == (1, 96, 130)
    assert torch.equal(it["h_im"][0], torch.from_numpy(np.float32(img[:96, :130] / 255.)))
    if torch.cuda.is_available():       # the device kernel made it
        assert np.abs(it["l_im"][0].numpy().astype(np.float64) - want).max() <= TOL_DEVICE
    else:
        assert np.array_equal(it["l_im"][0].numpy(), want)
    assert it["l_path"] == it["h_path"] == pairs_h["t/h_0.tif"]["abs_path"]
    assert it["l_id"] == "None_0" and it["h_id"] == "t/h_0.tif"
    # the committed folds: biosr... names resolve to data/biosr, 'None_<i>' keys to no file
    a = types.SimpleNamespace(scale=2, splits_root=os.path.join(HX, "folds"), data_root=os.path.join(HX, "data"), eval_bsize=2)
    ld = get_eval_loader(a, "biosrv1-ccps-test-X-2")
    batches = list(ld)
    assert len(ld.dataset) == 3 and [tuple(b["l_im"].shape) for b in batches] == [(2, 1, 48, 64), (1, 1, 48, 64)]
    assert batches[0]["l_path"] == batches[0]["h_path"] and batches[0]["l_id"] == ["None_0", "None_1"]
    lo = torch.cat([b["l_im"] for b in batches])
    assert 0.0 < lo.min() and lo.max() < 1.0            # smooth tiles: the uint8 source of l_to_h_img needs no clamp


def test_a_synthesised_caco2_item_is_unchanged(tmp_path):
    """A CACO-2 tile without a true LR tile keeps the reference's CACO-2 synthesis (bicubic + seeded noise), uint8."""
    import shutil
    from dlib.datasets import lowres as L
    from dlib.utils.utils_dataloaders import EvalPairs, imread_gray_uint8
    hp = os.path.join(G, "eval_exp", "data", "caco2", "t", "h_0.tif")
    d = tmp_path / "caco2" / "CELL0"
    d.mkdir(parents=True)
    shutil.copy(hp, d / "h_0.tif")
    pairs_h = {"CELL0/h_0.tif": {"abs_path": str(d / "h_0.tif"), "low_path_key": "None_0"}}
    ev = EvalPairs(types.SimpleNamespace(scale=8), pairs_h, {"None_0": {"abs_path": "None_0"}})
    assert not ev.is_hr_only(0)
    it = ev[0]
    want = L.simulate_low_res(np.clip(L.interpolate_torch(imread_gray_uint8(hp), 1. / 8), 0, 255), seed=0, th=7., sigma=6.)
    assert torch.equal(it["l_im"], torch.from_numpy(np.float32(want / 255.)).permute(2, 0, 1))
    assert it["l_path"] == str(d / "h_0.tif")


def test_hr_only_pairs_are_cropped_uniformly_only():
    """dataset_dpsr.py:863-864 asserts sample_tr_patch == 'uniform' for such pairs: so does the resident set, before it
    reads a tile or touches a device."""
    from dlib.utils.utils_dataloaders import get_train_set
    a = types.SimpleNamespace(scale=2, splits_root=os.path.join(HX, "folds"), data_root=os.path.join(HX, "data"),
                              train_dsets="biosrv1-ccps-train-X-2", h_size=32, batch_size=2, myseed=0,
                              sample_tr_patch="roi", sample_tr_patch_th_style="fix_threshold", sample_tr_patch_th=7)
    with pytest.raises(AssertionError, match="^roi"):
        get_train_set(a, "cuda")


def test_float_patch_job_mirrors_the_header(tmp_path):
    import ctypes
    from srhip import ops
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "srhip.h"\nint main(void) {\n'
                   '  printf("%zu %zu\\n", sizeof(srhip_patch_job_f32), offsetof(srhip_patch_job_f32, mode));\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, off = map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert (size, off) == (ctypes.sizeof(ops._PatchJobF32), ops._PatchJobF32.mode.offset)
