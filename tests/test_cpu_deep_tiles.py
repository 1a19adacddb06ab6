"""16-bit tiles, host side: the reader, the two value rules in numpy, the --in_max flag of main.py / eval.py / predict.py, and
what a set with a 16-bit tile refuses -- all before any device is touched."""
import os
import types

import numpy as np
import pytest
import torch
import yaml
from PIL import Image

import deep_tile_cases as D
import predict_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the reader
@pytest.mark.parametrize("ext", ["tif", "png"])
def test_reader_keeps_16_bit_files_at_full_depth(tmp_path, ext):
    from dlib.utils.utils_dataloaders import imread_gray
    a = D.tile_u16(19, 23, 65535, seed=1)
    p = str(tmp_path / f"a.{ext}")
    Image.fromarray(a).save(p)
    with Image.open(p) as im:
        assert im.mode == "I;16"
    got = imread_gray(p)
    assert got.dtype == np.uint16 and got.shape == (19, 23, 1) and np.array_equal(got[:, :, 0], a)
    assert got.dtype.isnative and got.flags["C_CONTIGUOUS"]


def test_reader_brings_byte_swapped_files_to_native_order(tmp_path):
    from dlib.utils.utils_dataloaders import imread_gray
    a = D.tile_u16(9, 11, 65535, seed=2)
    p = str(tmp_path / "be.tif")
    Image.frombytes("I;16B", (11, 9), a.astype(">u2").tobytes()).save(p)
    with Image.open(p) as im:
        assert im.mode == "I;16B"
    got = imread_gray(p)
    assert got.dtype == np.uint16 and got.dtype.isnative and np.array_equal(got[:, :, 0], a)


def test_reader_keeps_8_bit_files_and_refuses_the_rest_by_name(tmp_path):
    from dlib.utils.utils_dataloaders import imread_gray, imread_gray_uint8
    a = D.tile_u8(12, 16, seed=3)
    p = str(tmp_path / "l.tif")
    Image.fromarray(a).save(p)
    got = imread_gray(p)
    assert got.dtype == np.uint8 and np.array_equal(got, imread_gray_uint8(p)) and np.array_equal(got[:, :, 0], a)
    for name, im in (("F", Image.fromarray(np.zeros((4, 4), np.float32))), ("I", Image.fromarray(np.zeros((4, 4), np.int32))),
                     ("RGB", Image.fromarray(np.zeros((4, 4, 3), np.uint8)))):
        q = str(tmp_path / f"m_{name}.tif")
        im.save(q)
        with pytest.raises(NotImplementedError, match=f"m_{name}.tif.*'{name}'"):
            imread_gray(q)
    # the 8-bit reader is what it was: a 16-bit file is still not its business
    p16 = str(tmp_path / "d.tif")
    Image.fromarray(D.tile_u16(4, 4, 65535, seed=4)).save(p16)
    with pytest.raises(NotImplementedError, match="the reference reads 8-bit tiles"):
        imread_gray_uint8(p16)


# ---------------------------------------------------------------- R1, R2 in numpy
def test_value_rule_is_the_ingest_rule():
    from dlib.utils.utils_dataloaders import unit_of_levels
    v = np.arange(65536, dtype=np.uint16)
    for in_max in (65535, 4095, 1):
        want = C.ingest_value(v, in_max)
        assert want.dtype == np.float32
        assert np.array_equal(D.unit(v, in_max), want) and np.array_equal(unit_of_levels(v, in_max), want)
        assert want[0] == 0.0 and want[in_max] == 1.0 and (want[in_max:] == 1.0).all() and (np.diff(want[:in_max + 1]) > 0).all()
    assert np.array_equal(unit_of_levels(v), C.ingest_value(v, 65535))                 # the default white level
    b = np.arange(256, dtype=np.uint8)
    assert np.array_equal(unit_of_levels(b, 4095), np.float32(b / 255.))                # no effect on 8-bit tiles
    # R4: 257 v / 65535 and v / 255 are the same real number, and the same float32
    assert np.array_equal(D.unit((257 * b.astype(np.int64)).astype(np.uint16), 65535), np.float32(b / 255.))


@pytest.mark.parametrize("in_max", [65535, 4095, 1])
def test_reduction_rule_over_all_levels(in_max):
    v = np.arange(65536, dtype=np.uint16)
    got = D.level8(v, in_max)
    assert got.dtype == np.uint8 and got[0] == 0 and (got[in_max:] == 255).all() and (np.diff(got.astype(int)) >= 0).all()
    # the metric's rule on the same float: torch's (x.clamp(0, 1) * 255).round() of tensor2uint82float
    x = torch.from_numpy(D.unit(v, in_max))
    assert np.array_equal(got, (x.clamp(0, 1) * 255.).round().numpy().astype(np.uint8))
    # exact rounding of the exact quotient wherever that is no tie and not within float32's reach of one
    exact = 255.0 * np.minimum(v, in_max).astype(np.float64) / in_max
    far = np.abs(exact - np.floor(exact) - 0.5) > 1e-4
    assert np.array_equal(got[far], np.rint(exact[far]).astype(np.uint8))


def test_reduction_of_a_scaled_8_bit_tile_is_that_tile():
    b = np.arange(256)
    assert np.array_equal(D.level8((257 * b).astype(np.uint16), 65535), b.astype(np.uint8))


# ---------------------------------------------------------------- --in_max
def _stub_exp(tmp_path, name, **top):
    d = tmp_path / name
    d.mkdir()
    cfg = dict({"scale": 2, "method": "EDSR_LIIF", "myseed": 0, "amp": False, "splits_root": "folds", "test_dsets": "biosrx-test-X-2",
                "netG": {"net_type": "EDSR_LIIF"}}, **top)
    (d / "config_model.yml").write_text(yaml.safe_dump(cfg))
    return str(d)


def test_in_max_reaches_main_and_eval_and_predict(tmp_path, capsys):
    import main as M
    import eval as E
    from srhip import predict as P
    base = "--net_type swinir --method SWINIR --scale 2".split()
    a = M.parse_input(base + ["--in_max", "4095"])
    assert a.in_max == 4095 and dict(a)["in_max"] == 4095
    assert "in_max" not in M.parse_input(base)                       # absent unless given: such a folder behaves as before
    for bad in ("0", "70000", "-3"):
        with pytest.raises(SystemExit) as ei:
            M.parse_input(base + ["--in_max", bad])
        assert ei.value.code == 2 and "--in_max" in capsys.readouterr().err
    plain, rec = _stub_exp(tmp_path, "plain"), _stub_exp(tmp_path, "rec", in_max=4095)
    argv = ["--data_root", str(tmp_path)]
    assert "in_max" not in E.load_args(["--exp_path", plain] + argv)[1]
    assert E.load_args(["--exp_path", rec] + argv)[1].in_max == 4095              # read back from the folder
    assert E.load_args(["--exp_path", rec, "--in_max", "1023"] + argv)[1].in_max == 1023
    for bad in ("0", "70000"):
        with pytest.raises(SystemExit) as ei:
            E.load_args(["--exp_path", rec, "--in_max", bad] + argv)
        assert ei.value.code == 2 and "--in_max" in capsys.readouterr().err
    # predict: the recorded white level is the default of 16-bit pages; the user's own wins; 8-bit pages keep 255
    assert P.check_request(P.load_config(rec), np.uint16, 16, 16) == (4095, "uint16")
    assert P.check_request(P.load_config(rec), np.uint16, 16, 16, in_max=1023) == (1023, "uint16")
    assert P.check_request(P.load_config(rec), np.uint8, 16, 16) == (255, "uint8")
    assert P.check_request(P.load_config(plain), np.uint16, 16, 16) == (65535, "uint16")


# ---------------------------------------------------------------- refusals, when the set is built
def _args(data, folds, ds, **kw):
    a = types.SimpleNamespace(scale=2, splits_root=folds, data_root=data, train_dsets=ds, h_size=16, batch_size=2, myseed=0,
                              sample_tr_patch="uniform", netG={"net_type": "swinir"}, net_type="swinir")
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_a_set_with_a_16_bit_tile_says_what_it_cannot_do(tmp_path):
    from dlib.utils import constants
    from dlib.utils.utils_dataloaders import get_train_set, EvalPairs
    hr8 = [D.tile_u8(40, 48, seed=i) for i in range(2)]
    hr16 = [(257 * t.astype(np.int64)).astype(np.uint16) for t in hr8]
    ds = "biosrd-train-X-2"
    data, folds = D.write_fold(str(tmp_path), ds, hr16, [D.down_u8(t, 2) for t in hr8])       # 16-bit HR, 8-bit LR
    with pytest.raises(NotImplementedError, match="--ppiw"):
        get_train_set(_args(data, folds, ds, ppiw=True), "cuda")
    for net in (constants.SRCNN, constants.DSRSPLINES):
        with pytest.raises(NotImplementedError, match=net):
            get_train_set(_args(data, folds, ds, netG={"net_type": net}, net_type=net), "cuda")
    for bad in (0, 70000):
        with pytest.raises(ValueError, match="--in_max"):
            get_train_set(_args(data, folds, ds, in_max=bad), "cuda")
    # a 16-bit LR tile of an 8-bit HR tile is a 16-bit tile of the set too
    ds2 = "biosre-train-X-2"
    data2, folds2 = D.write_fold(str(tmp_path / "two"), ds2, hr8, [(257 * D.down_u8(t, 2).astype(np.int64)).astype(np.uint16)
                                                                  for t in hr8])
    with pytest.raises(NotImplementedError, match="--ppiw"):
        get_train_set(_args(data2, folds2, ds2, ppiw=True), "cuda")
    # a 16-bit CACO-2 tile without a true LR tile: the reference's synthesis is defined on uint8
    d = tmp_path / "caco2" / "CELL0"
    d.mkdir(parents=True)
    Image.fromarray(hr16[0]).save(str(d / "h_0.tif"))
    pairs_h = {"CELL0/h_0.tif": {"abs_path": str(d / "h_0.tif"), "low_path_key": "None_0"}}
    ev = EvalPairs(types.SimpleNamespace(scale=2), pairs_h, {"None_0": {"abs_path": "None_0"}})
    with pytest.raises(NotImplementedError, match="CACO-2.*uint8"):
        ev.low_res_u8(0, np.asarray(hr16[0])[:, :, None], str(d / "h_0.tif"))
    from dlib.datasets.dataset_dpsr import ResidentTrainSet
    with pytest.raises(NotImplementedError, match="CACO-2.*uint8"):
        ResidentTrainSet(_args("", "", ""), pairs_h, {"None_0": {"abs_path": "None_0"}}, "cuda")


def test_eval_pairs_read_a_16_bit_hr_only_pair(tmp_path):
    """the LR image of a 16-bit HR-only pair is imresize_np of R1; h_im is R1 of the mod-cropped tile"""
    from dlib.utils.utils_dataloaders import EvalPairs
    from dlib.utils.utils_image import imresize_np
    a = D.tile_u16(41, 48, 4095, seed=9)
    d = tmp_path / "biosr" / "t"
    d.mkdir(parents=True)
    Image.fromarray(a).save(str(d / "h_0.tif"))
    pairs_h = {"t/h_0.tif": {"abs_path": str(d / "h_0.tif"), "low_path_key": "None_0"}}
    ev = EvalPairs(types.SimpleNamespace(scale=2, in_max=4095), pairs_h, {"None_0": {"abs_path": "None_0"}})
    assert ev.is_hr_only(0)
    want_h = D.unit(a[:40], 4095)
    it = ev[0]          # where there is a GPU, srhip_imresize_aa_u16 makes l_im: the same bits
    assert it["h_bits"] == 16 and np.array_equal(it["h_im"][0].numpy(), want_h)
    assert np.array_equal(it["l_im"][0].numpy(), imresize_np(want_h, 1 / 2, True))
