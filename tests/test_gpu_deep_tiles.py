"""16-bit tiles on the device: srhip_patch_gather_u16, srhip_imresize_aa_u16 and srhip_levels_u16_to_u8 against the numpy
statements of tests/deep_tile_cases.py, the resident training set and the evaluation pairs built on them, and main.py /
eval.py / the Predictor on a 16-bit fold.  Every comparison is bit for bit.

The equivalence the set tests lean on: 257 v / 65535 and v / 255 are the same real number, so a fold whose tiles are
257 * (an 8-bit fold's tiles) computes, under the same seeds, what the 8-bit fold computes."""
import os
import pickle
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest
import torch
import yaml
from PIL import Image

import deep_tile_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sr-caco-2_amd")

pytestmark = pytest.mark.gpu


def _x257(t):
    return (257 * t.astype(np.int64)).astype(np.uint16)


def _zeros_u16(*shape):
    return torch.from_numpy(np.zeros(shape, np.uint16)).cuda()


def _shifted_by_2_bytes(a):
    """a copy of a uint16 CUDA tensor that starts 2 bytes into an allocation"""
    raw = torch.empty(2 * a.numel() + 2, dtype=torch.uint8, device="cuda")
    raw[2:].copy_(a.contiguous().view(torch.uint8).view(-1))
    return raw[2:].view(torch.uint16).view(a.shape)


# ---------------------------------------------------------------- srhip_patch_gather_u16
def _gather_jobs(tiles, P):
    """every mode at every corner of both tiles (64 jobs), then random origins"""
    rng = np.random.RandomState(P)
    ids, y0, x0, modes = [], [], [], []
    for i, t in enumerate(tiles):
        for m in range(8):
            for (cy, cx) in ((0, 0), (0, 1), (1, 0), (1, 1)):
                ids.append(i), modes.append(m), y0.append(cy * (t.shape[0] - P)), x0.append(cx * (t.shape[1] - P))
    for _ in range(8):
        i = int(rng.randint(len(tiles)))
        ids.append(i), modes.append(int(rng.randint(8)))
        y0.append(int(rng.randint(0, tiles[i].shape[0] - P + 1))), x0.append(int(rng.randint(0, tiles[i].shape[1] - P + 1)))
    return ids, y0, x0, modes


@pytest.mark.parametrize("in_max", D.IN_MAXES)
@pytest.mark.parametrize("P", [8, 5])
def test_patch_gather_u16_is_the_numpy_crop_augmentation_and_value_rule(P, in_max):
    from srhip import ops
    tiles = [D.tile_u16(19, 23, in_max, seed=1), D.tile_u16(16, 16, in_max, seed=2)]
    assert in_max == 65535 or max(int(t.max()) for t in tiles) > in_max          # values above the white level are present
    dev = [torch.from_numpy(t).cuda() for t in tiles]
    ids, y0, x0, modes = _gather_jobs(tiles, P)
    got = ops.patch_gather_u16(dev, ids, y0, x0, modes, P, in_max=in_max)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(ids), 1, P, P)          # 72 jobs: two launches of <= 64
    for b in range(len(ids)):
        crop = tiles[ids[b]][y0[b]:y0[b] + P, x0[b]:x0[b] + P]
        want = np.ascontiguousarray(D.augment_img(D.unit(crop, in_max), modes[b]))
        assert np.array_equal(got[b, 0].cpu().numpy(), want), (b, modes[b], y0[b], x0[b])
    if in_max == 65535:                                                                  # the default white level
        assert torch.equal(ops.patch_gather_u16(dev, ids, y0, x0, modes, P), got)


@pytest.mark.parametrize("P", [8, 5])
def test_patch_gather_u16_on_a_scaled_8_bit_tile_gives_patch_gather_s_bits(P):
    from srhip import ops
    t8 = [D.tile_u8(19, 23, seed=3), np.arange(256, dtype=np.uint8).reshape(16, 16)]            # every 8-bit level
    ids, y0, x0, modes = _gather_jobs(t8, P)
    want = ops.patch_gather([torch.from_numpy(t).cuda() for t in t8], ids, y0, x0, modes, P)
    got = ops.patch_gather_u16([torch.from_numpy(_x257(t)).cuda() for t in t8], ids, y0, x0, modes, P, in_max=65535)
    assert torch.equal(got, want)


def test_patch_gather_u16_refuses_what_patch_gather_refuses():
    from srhip import ops
    from srhip._lib import SrhipError
    t = torch.from_numpy(D.tile_u16(19, 23, 65535, seed=4)).cuda()
    with pytest.raises(SrhipError, match="outside"):
        ops.patch_gather_u16([t], [0], [19 - 8 + 1], [0], [0], 8)
    with pytest.raises(SrhipError, match="outside"):
        ops.patch_gather_u16([t], [0], [0], [-1], [0], 8)
    with pytest.raises(SrhipError, match="mode"):
        ops.patch_gather_u16([t], [0], [0], [0], [8], 8)
    with pytest.raises(ValueError, match="uint16"):
        ops.patch_gather_u16([torch.zeros(19, 23, dtype=torch.uint8, device="cuda")], [0], [0], [0], [0], 8)
    with pytest.raises(ValueError, match="in_max"):
        ops.patch_gather_u16([t], [0], [0], [0], [0], 8, in_max=65536)


# ---------------------------------------------------------------- srhip_imresize_aa_u16
# widths that are multiples of 8 (16-byte loads of 8 pixels) and one odd width per scale (the scalar row path)
RESIZE_CASES = [(40, 48, 2), (64, 72, 4), (128, 136, 8), (41, 47, 2), (65, 71, 4), (129, 131, 8)]


@pytest.mark.parametrize("in_max", D.IN_MAXES)
@pytest.mark.parametrize("h,w,s", RESIZE_CASES)
def test_imresize_aa_u16_is_imresize_np_of_the_full_depth_image(h, w, s, in_max):
    from srhip import ops
    from dlib.utils.utils_image import imresize_np
    a = np.stack([D.tile_u16(h, w, in_max, seed=10 + s), D.tile_u16(h, w, in_max, seed=20 + s)])
    got = ops.imresize_aa(torch.from_numpy(a).cuda(), 1 / s, in_max=in_max)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, -(-h // s), -(-w // s))
    worst = 0.0
    for b in range(2):
        want = imresize_np(D.unit(a[b], in_max), 1 / s, True)
        worst = max(worst, float(np.abs(got[b].cpu().numpy().astype(np.float64) - want).max()))
    print(f"imresize_aa_u16 {h}x{w} 1/{s} in_max {in_max}: max |device - imresize_np| = {worst:.3g}")
    for b in range(2):
        assert np.array_equal(got[b].cpu().numpy(), imresize_np(D.unit(a[b], in_max), 1 / s, True)), (b, worst)


@pytest.mark.parametrize("h,w,s", RESIZE_CASES)
def test_imresize_aa_u16_on_a_scaled_8_bit_image_gives_the_uint8_kernel_s_bits(h, w, s):
    from srhip import ops
    a = np.stack([D.tile_u8(h, w, seed=s), np.random.RandomState(s).randint(0, 256, size=(h, w)).astype(np.uint8)])
    want = ops.imresize_aa(torch.from_numpy(a).cuda(), 1 / s)
    got = ops.imresize_aa(torch.from_numpy(_x257(a)).cuda(), 1 / s, in_max=65535)
    assert torch.equal(got, want)
    assert torch.equal(ops.imresize_aa(torch.from_numpy(_x257(a)).cuda(), 1 / s), want)          # the default white level


def test_imresize_aa_u16_on_a_source_aligned_to_2_bytes_only():
    """rows of whole 8-pixel runs on a source that starts 2 bytes into an allocation: the scalar path, the same bits"""
    from srhip import ops
    a = torch.from_numpy(np.stack([D.tile_u16(40, 48, 4095, seed=5)] * 2)).cuda()
    shifted = _shifted_by_2_bytes(a)
    assert a.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 2
    assert torch.equal(ops.imresize_aa(shifted, 1 / 2, in_max=4095), ops.imresize_aa(a, 1 / 2, in_max=4095))


def test_imresize_aa_u16_refuses_an_image_too_small_for_the_scale():
    from srhip import ops
    from srhip._lib import SrhipError
    small = _zeros_u16(1, 8, 8)
    with pytest.raises(SrhipError, match="too small"):
        ops.imresize_aa(small, 1 / 8)
    with pytest.raises(SrhipError, match="too small"):                  # as the uint8 entry point refuses it
        ops.imresize_aa(torch.zeros(1, 8, 8, dtype=torch.uint8, device="cuda"), 1 / 8)
    with pytest.raises(SrhipError):
        ops.imresize_aa(_zeros_u16(1, 16, 16), 2.0)
    with pytest.raises(ValueError, match="in_max"):
        ops.imresize_aa(_zeros_u16(1, 16, 24), 1 / 2, in_max=0)
    assert tuple(ops.imresize_aa(_zeros_u16(1, 16, 24), 1 / 8).shape) == (1, 2, 3)


# ---------------------------------------------------------------- srhip_levels_u16_to_u8
@pytest.mark.parametrize("in_max", (65535, 4095, 1))
def test_levels_u16_to_u8_is_the_numpy_statement(in_max):
    from srhip import ops
    allv = np.arange(65536, dtype=np.uint16)
    rng = np.random.RandomState(in_max)
    for n in (1, 255, 1022, 65536):                      # 1022: no multiple of 4; 65536: every level
        v = allv if n == 65536 else rng.randint(0, 65536, size=n).astype(np.uint16)
        got = ops.levels_u16_to_u8(torch.from_numpy(v).cuda(), in_max)
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), D.level8(v, in_max)), (n, in_max)
    # a source 2 bytes into an allocation (pixel by pixel) and a 2-D tile keep their shape and bits
    odd = _shifted_by_2_bytes(torch.from_numpy(allv[5000:6022].copy()).cuda())
    assert odd.data_ptr() % 8 == 2
    assert np.array_equal(ops.levels_u16_to_u8(odd, in_max).cpu().numpy(), D.level8(allv[5000:6022], in_max))
    t = D.tile_u16(19, 23, in_max, seed=6)
    got = ops.levels_u16_to_u8(torch.from_numpy(t).cuda(), in_max)
    assert tuple(got.shape) == (19, 23) and np.array_equal(got.cpu().numpy(), D.level8(t, in_max))
    with pytest.raises(ValueError):
        ops.levels_u16_to_u8(torch.zeros(4, dtype=torch.uint8, device="cuda"))


def test_levels_u16_to_u8_of_a_scaled_8_bit_tile_is_that_tile():
    from srhip import ops
    b = np.arange(256, dtype=np.uint8)
    assert np.array_equal(ops.levels_u16_to_u8(torch.from_numpy(_x257(b)).cuda()).cpu().numpy(), b)


# ---------------------------------------------------------------- ResidentTrainSet.epoch
def _args(data, folds, ds, **kw):
    a = types.SimpleNamespace(scale=2, splits_root=folds, data_root=data, train_dsets=ds, h_size=16, batch_size=2, myseed=3,
                              sample_tr_patch="uniform", sample_tr_patch_th_style="fix_threshold", sample_tr_patch_th=60,
                              netG={"net_type": "swinir"}, net_type="swinir")
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.fixture(scope="module")
def folds(tmp_path_factory):
    """three 40 x 48 tiles (scale 2): a paired and an HR-only 8-bit fold, and the same folds with every tile times 257"""
    root = str(tmp_path_factory.mktemp("deep"))
    hr = [D.tile_u8(40, 48, seed=30 + i) for i in range(3)]
    lr = [D.down_u8(t, 2) for t in hr]
    out = {"hr": hr, "lr": lr}
    out["data"], out["folds"] = D.write_fold(root, "biosrp8-train-X-2", hr, lr)
    D.write_fold(root, "biosrp16-train-X-2", [_x257(t) for t in hr], [_x257(t) for t in lr])
    D.write_fold(root, "biosrh8-train-X-2", hr)
    D.write_fold(root, "biosrh16-train-X-2", [_x257(t) for t in hr])
    return out


ARMS = {"paired-uniform": ("p", {}),
        "paired-roi-fixed": ("p", {"sample_tr_patch": "roi"}),
        "paired-edt-otsu": ("p", {"sample_tr_patch": "edt", "sample_tr_patch_th_style": "automatic_threshold"}),
        "hr-only-uniform": ("h", {})}


@pytest.mark.parametrize("arm", list(ARMS))
def test_a_scaled_fold_gives_the_8_bit_fold_s_batches(folds, arm):
    from dlib.utils.utils_dataloaders import get_train_set
    kind, kw = ARMS[arm]
    sets = [get_train_set(_args(folds["data"], folds["folds"], f"biosr{kind}{bits}-train-X-2", **kw), "cuda") for bits in (8, 16)]
    assert [t.dtype for t in sets[0].hr] == [torch.uint8] * 3 and [t.dtype for t in sets[1].hr] == [torch.uint16] * 3
    if kind == "p":
        assert [t.dtype for t in sets[1].lr] == [torch.uint16] * 3
        if kw:      # the samplers threshold the same 8-bit image
            assert all(torch.equal(a, b) for a, b in zip(sets[0].roi_src, sets[1].roi_src))
    else:
        assert [t.dtype for t in sets[1].lr] == [torch.float32] * 3
        assert all(torch.equal(a, b) for a, b in zip(sets[0].lr, sets[1].lr))
    b8, b16 = list(sets[0].epoch(0)), list(sets[1].epoch(0))
    assert len(b8) == len(b16) == 1
    for x, y in zip(b8, b16):
        assert x["origin"] == y["origin"] and x["mode"] == y["mode"] and x["h_id"][0][-7:] == y["h_id"][0][-7:]
        for k in ("l_im", "h_im", "l_to_h_img"):
            assert tuple(x[k].shape)[:2] == (2, 1) and torch.equal(x[k], y[k]), k


def test_a_16_bit_fold_is_read_at_full_depth(tmp_path):
    """random uint16 tiles, white level 4095: h_im and l_im are the statement at the batch's own origin and mode"""
    from dlib.utils.utils_dataloaders import get_train_set
    hr = [D.tile_u16(40, 48, 4095, seed=40 + i) for i in range(3)]
    lr = [D.tile_u16(20, 24, 4095, seed=50 + i) for i in range(3)]
    ds = "biosrq-train-X-2"
    data, fo = D.write_fold(str(tmp_path), ds, hr, lr)
    ts = get_train_set(_args(data, fo, ds, in_max=4095), "cuda")
    n = 0
    for epoch in range(2):
        for b in ts.epoch(epoch):
            for k in range(2):
                i = int(b["h_id"][k].split("_")[-1].split(".")[0])
                (r0, c0), m = b["origin"][k], b["mode"][k]
                want_h = D.augment_img(D.unit(hr[i][r0:r0 + 16, c0:c0 + 16], 4095), m)
                want_l = D.augment_img(D.unit(lr[i][r0 // 2:r0 // 2 + 8, c0 // 2:c0 // 2 + 8], 4095), m)
                assert np.array_equal(b["h_im"][k, 0].cpu().numpy(), want_h)
                assert np.array_equal(b["l_im"][k, 0].cpu().numpy(), want_l)
                n += 1
    assert n == 4


def test_one_set_mixes_depths_and_each_sample_comes_from_its_own_gather(tmp_path):
    """an 8-bit pair, a 16-bit pair and a pair with an 8-bit LR and a 16-bit HR tile in one set, batches of three"""
    from dlib.datasets.dataset_dpsr import ResidentTrainSet
    h8, h16, hm = D.tile_u8(40, 48, seed=60), D.tile_u16(40, 48, 65535, seed=61), D.tile_u16(40, 48, 65535, seed=62)
    l8, l16, lm = D.down_u8(h8, 2), D.tile_u16(20, 24, 65535, seed=63), D.tile_u8(20, 24, seed=64)
    d = tmp_path / "biosr"
    d.mkdir()
    pairs_h, pairs_l, raw = {}, {}, {}
    for name, h, l in (("a", h8, l8), ("b", h16, l16), ("c", hm, lm)):
        Image.fromarray(h).save(str(d / f"h_{name}.tif"))
        Image.fromarray(l).save(str(d / f"l_{name}.tif"))
        pairs_h[f"h_{name}.tif"] = {"abs_path": str(d / f"h_{name}.tif"), "low_path_key": f"l_{name}.tif"}
        pairs_l[f"l_{name}.tif"] = {"abs_path": str(d / f"l_{name}.tif")}
        raw[f"h_{name}.tif"] = (h, l)
    ts = ResidentTrainSet(_args("", "", "", batch_size=3), pairs_h, pairs_l, "cuda")
    assert [t.dtype for t in ts.hr] == [torch.uint8, torch.uint16, torch.uint16]
    assert [t.dtype for t in ts.lr] == [torch.uint8, torch.uint16, torch.uint8]
    (b,) = list(ts.epoch(0))
    assert sorted(b["h_id"]) == sorted(raw)
    unit = lambda a: D.unit(a, 65535) if a.dtype == np.uint16 else np.float32(a / 255.)
    for k in range(3):
        h, l = raw[b["h_id"][k]]
        (r0, c0), m = b["origin"][k], b["mode"][k]
        assert np.array_equal(b["h_im"][k, 0].cpu().numpy(), D.augment_img(unit(h[r0:r0 + 16, c0:c0 + 16]), m))
        assert np.array_equal(b["l_im"][k, 0].cpu().numpy(), D.augment_img(unit(l[r0 // 2:r0 // 2 + 8, c0 // 2:c0 // 2 + 8]), m))


def test_eval_pairs_on_a_16_bit_fold(folds, tmp_path):
    from dlib.utils.utils_dataloaders import get_eval_loader
    from dlib.utils.utils_image import imresize_np
    from srhip import ops
    ev = lambda ds, **kw: list(get_eval_loader(types.SimpleNamespace(scale=2, splits_root=folds["folds"], data_root=folds["data"],
                                                                    eval_bsize=3, **kw), ds))[0]
    p8, p16 = ev("biosrp8-train-X-2"), ev("biosrp16-train-X-2")
    assert p8["h_bits"] == [8] * 3 and p16["h_bits"] == [16] * 3
    assert torch.equal(p8["h_im"], p16["h_im"]) and torch.equal(p8["l_im"], p16["l_im"])
    # l_to_h_img of a 16-bit pair: cv2's FLOAT cubic of l_im, clipped (an 8-bit pair keeps the fixed-point path)
    want = ops.clip01_(ops.resize_cubic(p16["l_im"][:, 0].cuda().contiguous(), (40, 48)))
    assert torch.equal(p16["l_to_h_img"][:, 0], want)
    h8, h16 = ev("biosrh8-train-X-2"), ev("biosrh16-train-X-2")
    assert torch.equal(h8["l_im"], h16["l_im"]) and torch.equal(h8["h_im"], h16["h_im"])
    # a genuinely 16-bit HR-only pair with a white level: imresize_np of the full-depth image
    a = D.tile_u16(40, 48, 4095, seed=70)
    data, fo = D.write_fold(str(tmp_path), "biosrz-test-X-2", [a])
    it = list(get_eval_loader(types.SimpleNamespace(scale=2, splits_root=fo, data_root=data, eval_bsize=1, in_max=4095),
                              "biosrz-test-X-2"))[0]
    assert np.array_equal(it["h_im"][0, 0].numpy(), D.unit(a, 4095))
    assert np.array_equal(it["l_im"][0, 0].numpy(), imresize_np(D.unit(a, 4095), 1 / 2, True))


# ---------------------------------------------------------------- main.py, eval.py, Predictor
TINY = ("--task super-resolution --scale 2 --method SWINIR --net_type swinir --n_channels 1 --h_size 32 --batch_size 1 "
        "--swinir_depths 2+2 --swinir_embed_dim 60 --swinir_num_heads 6+6 --swinir_mlp_ratio 2 "
        "--swinir_upsampler pixelshuffledirect --l1 True --G_scheduler_type MyStepLR --G_scheduler_step_size 3 "
        "--G_scheduler_gamma 0.5 --G_scheduler_min_lr 1e-6 --G_optimizer_lr 1e-3 --max_epochs 1 --max_iters 2 "
        "--checkpoint_eval 2 --checkpoint_save 2 --eval_bsize 1 --myseed 0").split()


def _main(folds, ds, outd, extra=()):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = TINY + ["--train_dsets", ds, "--valid_dsets", ds, "--test_dsets", ds, "--data_root", folds["data"],
                  "--splits_root", folds["folds"], "--outd", outd] + list(extra)
    p = subprocess.run([sys.executable, os.path.join(PKG, "main.py")] + cmd, capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]


def _numbers(tr):
    """every number of a tracker, in a fixed order"""
    out = []

    def walk(path, v):
        if isinstance(v, dict):
            for k in sorted(v, key=str):
                walk(path + (str(k),), v[k])
        elif isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                walk(path + (str(i),), x)
        elif isinstance(v, (int, float, np.floating, np.integer)):
            out.append(("/".join(path), float(v)))
    walk((), tr)
    return out


def test_main_trains_on_a_16_bit_fold_and_eval_and_predict_read_the_folder(folds, tmp_path):
    """two iterations on the 8-bit paired fold and on the same fold times 257 (--in_max 65535 given): the same weights and the
    same tracker values, bit for bit; I;16 previews; in_max in config_model.yml of the run that passed it only; eval.py
    reproduces the test score; the Predictor takes the recorded white level for 16-bit pages"""
    o8, o16 = str(tmp_path / "e8"), str(tmp_path / "e16")
    ds8, ds16 = "biosrp8-train-X-2", "biosrp16-train-X-2"
    _main(folds, ds8, o8)
    _main(folds, ds16, o16, ["--in_max", "65535"])
    sd8 = torch.load(os.path.join(o8, "models", "2_G.pth"), map_location="cpu")
    sd16 = torch.load(os.path.join(o16, "models", "2_G.pth"), map_location="cpu")
    assert list(sd8) == list(sd16) and all(torch.equal(sd8[k], sd16[k]) for k in sd8)
    best8 = torch.load(os.path.join(o8, "best-models", "G-model.pth"), map_location="cpu")
    best16 = torch.load(os.path.join(o16, "best-models", "G-model.pth"), map_location="cpu")
    assert all(torch.equal(best8[k], best16[k]) for k in best8)
    trs = []
    for o in (o8, o16):
        with open(os.path.join(o, "tracker.pkl"), "rb") as f:
            trs.append(pickle.load(f))
    n8 = _numbers(trs[0])
    n16 = [(k.replace(ds16, ds8), v) for k, v in _numbers(trs[1])]
    assert len(n8) > 10 and n8 == n16
    assert len(trs[1]["train"]["period_iter"]["master_loss"]["vals"]) == 2
    # previews: I;16 for the 16-bit fold, L for the 8-bit one
    for o, ds, mode in ((o8, ds8, "L"), (o16, ds16, "I;16")):
        seen = 0
        for dirpath, _, files in os.walk(os.path.join(o, "imgs")):
            for f in files:
                if f.endswith(".png"):
                    with Image.open(os.path.join(dirpath, f)) as im:
                        assert im.mode == mode and im.size == (48, 40), (dirpath, f, im.mode)
                    seen += 1
        assert seen >= 3
    with open(os.path.join(o8, "config_model.yml")) as f:
        assert "in_max" not in yaml.safe_load(f)
    with open(os.path.join(o16, "config_model.yml")) as f:
        assert yaml.safe_load(f)["in_max"] == 65535
    # eval.py on the 16-bit folder
    import eval as E
    tr, _ = E.evaluate_pretrained(["--cudaid", "0", "--exp_path", o16, "--data_root", folds["data"], "--splits_root", folds["folds"]])
    assert abs(tr["test"][ds16]["psnr"]["vals"][0] - trs[1]["test"][ds16]["psnr"]["vals"][0]) <= 1e-9
    # the Predictor: a folder that recorded 4095 reads 16-bit pages by 4095 unless told otherwise
    from srhip.predict import Predictor
    o12 = str(tmp_path / "e12")
    os.makedirs(os.path.join(o12, "best-models"))
    shutil.copy(os.path.join(o16, "best-models", "G-model.pth"), os.path.join(o12, "best-models", "G-model.pth"))
    with open(os.path.join(o16, "config_model.yml")) as f:
        cfg = yaml.safe_load(f)
    cfg["in_max"] = 4095
    with open(os.path.join(o12, "config_model.yml"), "w") as f:
        yaml.safe_dump(cfg, f)
    pages = np.stack([D.tile_u16(16, 24, 4095, seed=80)])
    p12, p16 = Predictor(o12), Predictor(o16)
    rec, dflt = p12.run(pages), p16.run(pages)
    assert rec.dtype == np.uint16 and not np.array_equal(rec, dflt)
    p16.in_max, p12.in_max = 4095, 65535             # the user's own white level wins over the recorded one
    assert np.array_equal(p16.run(pages), rec) and np.array_equal(p12.run(pages), dflt)
