"""Host side of prediction on images without an HR partner: the plan of sr-caco-2_amd/predict.py, its PIL reading and writing,
the refusals of srhip/predict.py (from a stub config, without a device) and the numpy statements of the two value rules that
tests/test_gpu_predict.py gates the kernels against (tests/predict_cases.py)."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import yaml
from PIL import Image

import predict_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = os.path.join(ROOT, "tests", "golden", "eval_exp")


def _cli():
    spec = importlib.util.spec_from_file_location("srhip_predict_cli", os.path.join(ROOT, "sr-caco-2_amd", "predict.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _stub_exp(tmp_path, net_type, **netg):
    """an experiment folder that holds a configuration only: enough for every check that comes before the device"""
    d = tmp_path / f"exp_{net_type}"
    d.mkdir()
    cfg = {"scale": 2, "method": net_type.upper(), "myseed": 0, "amp": False,
           "netG": dict({"net_type": net_type}, **netg)}
    (d / "config_model.yml").write_text(yaml.safe_dump(cfg))
    return str(d)


# ---------------------------------------------------------------- the plan
def test_plan_orders_by_name_and_groups_consecutive_equal_pages():
    cli = _cli()
    u8, u16 = ("uint8", 16, 17), ("uint16", 16, 17)
    files = [("/in/c.tif", [u16] * 5), ("/in/a.png", [u8]), ("/in/b.tiff", [u8, u8, ("uint8", 9, 8), u8])]
    p = cli.plan(files, batch=3, scale=8, out_dir="/out")
    assert p["order"] == ["/in/a.png", "/in/b.tiff", "/in/c.tif"]
    # a.png and the first two pages of b.tiff are equal and consecutive: one group across the file boundary; the 9 x 8 page
    # separates the last page of b.tiff from them; c.tif's five pages are cut at the cap of 3
    assert p["groups"] == [[(0, 0), (1, 0), (1, 1)], [(1, 2)], [(1, 3)], [(2, 0), (2, 1), (2, 2)], [(2, 3), (2, 4)]]
    assert p["outputs"] == ["/out/a_x8.png", "/out/b_x8.tiff", "/out/c_x8.tif"]
    # every page exactly once, in order
    assert [q for g in p["groups"] for q in g] == [(fi, pi) for fi, f in enumerate(sorted(files)) for pi in range(len(f[1]))]
    # the cap alone
    q = cli.plan([("x.tif", [u8] * 7)], batch=2, scale=2, out_dir="o")
    assert [len(g) for g in q["groups"]] == [2, 2, 2, 1] and q["outputs"] == [os.path.join("o", "x_x2.tif")]
    # equal shape, other dtype: not batched together
    r = cli.plan([("x.tif", [u8, u16, u16, u8])], batch=8, scale=2, out_dir="o")
    assert r["groups"] == [[(0, 0)], [(0, 1), (0, 2)], [(0, 3)]]
    # float32 pages cannot live in a PNG: TIFF mode F
    f = cli.plan(files, batch=3, scale=8, out_dir="/out", out_dtype="float32")
    assert f["outputs"] == ["/out/a_x8.tif", "/out/b_x8.tiff", "/out/c_x8.tif"]
    with pytest.raises(cli.PredictError):
        cli.plan([("/p/a.png", [u8]), ("/q/a.png", [u8])], batch=3, scale=8, out_dir="/out")


# ---------------------------------------------------------------- reading and writing
def test_pages_read_and_written_with_pil(tmp_path):
    cli = _cli()
    rng = np.random.RandomState(3)
    stack = rng.randint(0, 65536, size=(3, 6, 7)).astype(np.uint16)
    stack[0, 0, :2] = (0, 65535)
    tif = str(tmp_path / "s.tif")
    ims = [Image.fromarray(p) for p in stack]
    assert ims[0].mode == "I;16"
    ims[0].save(tif, save_all=True, append_images=ims[1:])
    one = rng.randint(0, 256, size=(5, 4)).astype(np.uint8)
    png = str(tmp_path / "o.png")
    Image.fromarray(one).save(png)
    got = cli.read_pages(tif)
    assert len(got) == 3 and all(g.dtype == np.uint16 for g in got) and np.array_equal(np.stack(got), stack)
    assert cli.read_meta(tif) == [("uint16", 6, 7)] * 3
    got = cli.read_pages(png)
    assert len(got) == 1 and got[0].dtype == np.uint8 and np.array_equal(got[0], one)
    assert cli.read_meta(png) == [("uint8", 5, 4)]
    assert sorted(os.path.basename(f) for f in cli.list_inputs(str(tmp_path))) == ["o.png", "s.tif"]
    # a grey palette is an 8-bit grey image: the palette's levels, not the indices
    pal = Image.fromarray(one).convert("P")
    pal.putpalette([v for i in range(256) for v in (255 - i,) * 3])
    pal.save(str(tmp_path / "p.png"))
    assert np.array_equal(cli.read_pages(str(tmp_path / "p.png"))[0], 255 - one)
    # written pages come back: same container, page count, order and bits
    out = str(tmp_path / "w.tif")
    cli.write_pages(out, list(stack))
    with Image.open(out) as im:
        assert im.n_frames == 3 and im.mode == "I;16"
    assert np.array_equal(np.stack(cli.read_pages(out)), stack)
    cli.write_pages(str(tmp_path / "w.png"), [one])
    assert np.array_equal(cli.read_pages(str(tmp_path / "w.png"))[0], one)
    cli.write_pages(str(tmp_path / "w16.png"), [stack[1]])
    assert np.array_equal(cli.read_pages(str(tmp_path / "w16.png"))[0], stack[1])
    fl = rng.rand(2, 6, 7).astype(np.float32)
    cli.write_pages(str(tmp_path / "f.tif"), list(fl))
    with Image.open(str(tmp_path / "f.tif")) as im:
        assert im.n_frames == 2 and im.mode == "F"
        im.seek(1)
        assert np.array_equal(np.asarray(im), fl[1])


def test_other_modes_are_refused_naming_file_and_mode(tmp_path):
    cli = _cli()
    rgb = str(tmp_path / "colour.png")
    Image.fromarray(np.zeros((4, 4, 3), np.uint8)).save(rgb)
    with pytest.raises(cli.PredictError, match=r"colour\.png.*'RGB'"):
        cli.read_pages(rgb)
    with pytest.raises(cli.PredictError, match=r"colour\.png.*'RGB'"):
        cli.read_meta(rgb)
    fl = str(tmp_path / "float.tif")
    Image.fromarray(np.zeros((4, 4), np.float32)).save(fl)
    with pytest.raises(cli.PredictError, match=r"float\.tif.*'F'"):
        cli.read_meta(fl)
    i32 = str(tmp_path / "int.tif")
    Image.fromarray(np.zeros((4, 4), np.int32)).save(i32)
    with pytest.raises(cli.PredictError, match=r"int\.tif.*'I'"):
        cli.read_pages(i32)
    pal = Image.fromarray(np.zeros((4, 4), np.uint8)).convert("P")
    pal.putpalette([v for i in range(256) for v in (i, 0, 255 - i)])
    pal.save(str(tmp_path / "pal.png"))
    with pytest.raises(cli.PredictError, match=r"pal\.png.*'P'"):
        cli.read_pages(str(tmp_path / "pal.png"))


# ---------------------------------------------------------------- the refusals, before any device use
def test_refusals_from_a_stub_config(tmp_path, monkeypatch):
    from srhip import predict as P
    from dlib.utils import constants

    def no_device(*a, **k):
        raise AssertionError("the refusal must come before the model is built")
    monkeypatch.setattr("dlib.models.select_model.define_model", no_device)
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    u16 = np.zeros((2, 16, 16), np.uint16)
    u8 = np.zeros((2, 16, 16), np.uint8)
    with pytest.raises(P.PredictError, match="SRCNN"):
        P.Predictor(_stub_exp(tmp_path, constants.SRCNN, SRCNN_in_chans=1)).run(u16)
    with pytest.raises(P.PredictError, match="DSR-Splines"):
        P.Predictor(_stub_exp(tmp_path, constants.DSRSPLINES)).run(u16)
    swin = _stub_exp(tmp_path, constants.SWINIR, swinir_window_size=8)
    with pytest.raises(P.PredictError, match="in_max 70000"):
        P.Predictor(swin, in_max=70000)
    with pytest.raises(P.PredictError, match="in_max 4095"):       # fine for 16-bit pages, above the range of 8-bit ones
        P.Predictor(swin, in_max=4095).run(u8)
    with pytest.raises(P.PredictError, match="too small"):         # 7 rows -> 8: fine; 3 columns -> 8 flips 5 of 3
        P.Predictor(swin).run(np.zeros((1, 7, 3), np.uint8))
    with pytest.raises(P.PredictError, match="uint8 or uint16"):
        P.Predictor(swin).run(np.zeros((1, 16, 16), np.float32))
    with pytest.raises(P.PredictError, match="out_dtype"):
        P.Predictor(swin, out_dtype="int8")
    # what is asked of the device for the requests that pass
    args = P.load_config(swin)
    assert P.padded_size(args, 64, 64) == (72, 72) and P.padded_size(args, 16, 17) == (24, 24)       # a whole extra window
    assert P.padded_size(args, 9, 8) == (16, 16) and P.padded_size(args, 4, 7) == (8, 8)
    assert P.check_request(args, np.uint16, 16, 17, None, "same") == (65535, "uint16")
    assert P.check_request(args, np.uint16, 16, 17, 4095, "uint8") == (4095, "uint8")
    assert P.check_request(args, np.uint8, 4, 4, None, "float32") == (255, "float32")            # pad 4 of 4: the limit
    with pytest.raises(P.PredictError, match="too small"):
        P.check_request(args, np.uint8, 3, 8)
    edsr = P.load_config(_stub_exp(tmp_path, constants.EDSR_LIIF))
    assert P.padded_size(edsr, 9, 13) == (9, 13) and P.check_request(edsr, np.uint8, 1, 1) == (255, "uint8")
    # 8-bit pages pass with the two nets that refuse 16-bit ones
    for net in (constants.SRCNN, constants.DSRSPLINES):
        assert P.check_request(P.load_config(str(tmp_path / f"exp_{net}")), np.uint8, 16, 16) == (255, "uint8")
    # the real fixture's configuration is read as eval.py reads it
    real = P.load_config(os.path.join(FX, "exp"))
    assert real.scale == 8 and real.netG["checkpoint_path_netG"].endswith("best-models/G-model.pth") and not real.is_train


def test_command_line_skips_a_file_whose_output_is_not_finite(tmp_path, monkeypatch):
    """the bookkeeping of the command line around a stand-in for the device work: a group that raises NonFiniteError costs the
    files it holds pages of, the others are written, the log names both kinds and the status is 1"""
    cli = _cli()
    from srhip import predict as P
    from dlib.utils import constants
    exp = _stub_exp(tmp_path, constants.EDSR_LIIF)
    src = tmp_path / "in"
    src.mkdir()
    rng = np.random.RandomState(0)
    good = rng.randint(1, 65536, size=(3, 4, 5)).astype(np.uint16)
    ims = [Image.fromarray(p) for p in good]
    ims[0].save(str(src / "a.tif"), save_all=True, append_images=ims[1:])
    bad = rng.randint(1, 256, size=(4, 5)).astype(np.uint8)
    bad[0, 0] = 0                                                  # the stand-in's trigger
    Image.fromarray(bad).save(str(src / "b.png"))
    last = rng.randint(1, 256, size=(6, 5)).astype(np.uint8)
    Image.fromarray(last).save(str(src / "c.png"))
    seen = []

    def fake_run(self, pages):
        seen.append(pages.shape)
        if (pages == 0).any():
            raise P.NonFiniteError(range(len(pages)))
        return np.repeat(np.repeat(pages, 2, axis=1), 2, axis=2)
    monkeypatch.setattr(P.Predictor, "run", fake_run)
    rc = cli.predict(["--exp_path", exp, "--input", str(src), "--batch", "2"])
    out = os.path.join(exp, "predict", "in")                      # the default output directory
    assert rc == 1 and sorted(os.listdir(out)) == ["a_x2.tif", "c_x2.png", "log.json", "log.txt"]
    assert seen == [(2, 4, 5), (1, 4, 5), (1, 4, 5), (1, 6, 5)]    # a.tif at a cap of 2, then b.png, then c.png
    assert np.array_equal(np.stack(cli.read_pages(os.path.join(out, "a_x2.tif"))), np.repeat(np.repeat(good, 2, 1), 2, 2))
    assert np.array_equal(cli.read_pages(os.path.join(out, "c_x2.png"))[0], np.repeat(np.repeat(last, 2, 0), 2, 1))
    log = open(os.path.join(out, "log.txt")).read()
    assert "b.png: 4 x 5 uint8, 1 page(s)" in log and "NOT WRITTEN" in log.split("b.png:")[1].splitlines()[0]
    assert "a.tif: 4 x 5 uint16, 3 page(s)" in log and "-> a_x2.tif" in log and "1 of 3 file(s) not written" in log
    # a mode the command line does not read stops it before anything is run or written
    Image.fromarray(np.zeros((4, 4, 3), np.uint8)).save(str(src / "d.png"))
    seen.clear()
    with pytest.raises(cli.PredictError, match=r"d\.png.*'RGB'"):
        cli.predict(["--exp_path", exp, "--input", str(src), "--output", str(tmp_path / "o2")])
    assert not seen and not os.path.exists(str(tmp_path / "o2"))


# ---------------------------------------------------------------- the statements of the two value rules
def _bits(x):
    return int(np.float32(x).view(np.uint32))


def test_ingest_statement_against_hand_computed_values():
    # 1 / 255 = 0x1.010101...p-8: 24 bits are 0x808080|8 -> round up: 0x3B808081; 128 / 255 is that times 2^7
    assert _bits(C.ingest_value(np.uint8(1), 255)) == 0x3B808081 and _bits(C.ingest_value(np.uint8(128), 255)) == 0x3F008081
    assert C.ingest_value(np.uint8(0), 255) == 0.0 and C.ingest_value(np.uint8(255), 255) == 1.0
    assert C.ingest_value(np.uint16(65535), 65535) == 1.0 and _bits(C.ingest_value(np.uint16(257), 65535)) == 0x3B808081
    # 1 / 65535 = 0x1.00010001...p-16 -> 0x37800080
    assert _bits(C.ingest_value(np.uint16(1), 65535)) == 0x37800080
    # a white level below the container's range saturates
    v = np.asarray([0, 4095, 4096, 5000, 65535], np.uint16)
    assert C.ingest_value(v, 4095).tolist() == [0.0, 1.0, 1.0, 1.0, 1.0] and C.ingest_value(v, 4095).dtype == np.float32
    # 1 / 4095 = 0x1.001001001...p-12 -> 0x39800801
    assert _bits(C.ingest_value(np.uint16(1), 4095)) == 0x39800801
    # 257 v / 65535 and v / 255 are the same real number: the 16-bit path sees the 8-bit image exactly
    a = np.arange(256)
    assert np.array_equal(C.ingest_value((a * 257).astype(np.uint16), 65535), C.ingest_value(a.astype(np.uint8), 255))
    # the padding: rows first, then columns of the row-padded image; the corner is flipped both ways
    p = np.arange(12, dtype=np.uint8).reshape(1, 3, 4)
    got = (C.ingest_pad_ref(p, 255, 5, 6) * 255).round().to(torch.int64)[0].tolist()
    assert got == [[0, 1, 2, 3, 3, 2], [4, 5, 6, 7, 7, 6], [8, 9, 10, 11, 11, 10], [8, 9, 10, 11, 11, 10], [4, 5, 6, 7, 7, 6]]
    for (H, W), (Hp, Wp) in C.INGEST_SHAPES:
        for dtype, m in C.INGEST_RANGES:
            pages = C.ingest_pages(dtype, m, 3, H, W)
            assert pages.dtype == dtype and (pages > m).any() == (m < np.iinfo(dtype).max) and (pages == m).any()
            assert tuple(C.ingest_pad_ref(pages, m, Hp, Wp).shape) == (3, Hp, Wp)
    (H, W), (Hp, Wp) = C.INGEST_TOO_SMALL
    assert Hp - H > H


def test_emit_statement_against_hand_computed_values():
    x = np.asarray([-0.0, -3.0, 2.0, 0.5, 1.0, 0.25, 0.75, np.nan, np.inf, -np.inf], np.float32)
    # 127.5 -> 128 and 63.75 -> 64, 191.25 -> 191; NaN -> 0; the infinities: what the clamp gives
    assert C.emit_value(x, 255).tolist() == [0, 0, 255, 128, 255, 64, 191, 0, 255, 0]
    # 32767.5 -> 32768 (even), 16383.75 -> 16384, 49151.25 -> 49151
    assert C.emit_value(x, 65535).tolist() == [0, 0, 65535, 32768, 65535, 16384, 49151, 0, 65535, 0]
    # half to even in both directions: where the float32 product of float32((k + 0.5) / 255) is exactly k + 0.5, an even k
    # stays and an odd k goes up; both kinds occur
    k = np.arange(255)                                             # (255 + 0.5) / 255 is above 1: clamped
    c = np.float32((k + 0.5) / 255)
    tie = (c * np.float32(255)) == (k + 0.5)
    assert (tie & (k % 2 == 0)).any() and (tie & (k % 2 == 1)).any()
    assert np.array_equal(C.emit_value(c, 255)[tie], (k + k % 2)[tie])
    # the torch statement the GPU test compares with says the same on every finite test input
    xin, pos = C.emit_input()
    assert torch.isfinite(xin).all() and len(pos) == len(C.halfway_values()) + len(C.EMIT_SPECIALS)
    inside = torch.zeros_like(xin, dtype=torch.bool)
    inside[:, :C.EMIT_HO, :C.EMIT_WO] = True
    assert inside.view(-1)[pos].all() and len(set(pos.tolist())) == len(pos)
    for m in (255, 65535):
        assert np.array_equal(C.emit_ref(xin, m).to(torch.int64).numpy(), C.emit_value(xin.numpy(), m))
    # the halfway values are where the kind of product matters: among them are inputs that a double-precision product (or
    # a product fused with anything) rounds to another integer than the single float32 product of the rule
    h = C.halfway_values()
    assert len(h) == 3 * (256 + 64)
    for m in (255, 65535):
        one_f32 = C.emit_value(h, m)
        in_double = np.rint(np.clip(h.astype(np.float64), 0, 1) * m).astype(np.int64)
        assert (one_f32 != in_double).any(), m
