"""Prediction on images without an HR partner, on the device: srhip_ingest_pad and srhip_emit_uint against the numpy / torch
statements of tests/predict_cases.py, then srhip/predict.py's Predictor and the sr-caco-2_amd/predict.py command line against
compositions of what was there before (``_forward_with_padding``, ``tensor2uint82float``).

Every comparison is bit-exact: the ingest is one correctly rounded conversion, the emit one float32 product and a rounding to
an integer below 2^24, and the pipeline checks run the same kernels on the same inputs at the same batch."""
import importlib.util
import os

import numpy as np
import pytest
import torch
from PIL import Image

import predict_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = os.path.join(ROOT, "tests", "golden", "eval_exp")
EXP = os.path.join(FX, "exp")


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _cli():
    spec = importlib.util.spec_from_file_location("srhip_predict_cli", os.path.join(ROOT, "sr-caco-2_amd", "predict.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---------------------------------------------------------------- srhip_ingest_pad
@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("dtype,in_max", C.INGEST_RANGES, ids=lambda v: getattr(v, "__name__", str(v)))
def test_ingest_pad_is_the_statement(dtype, in_max, B):
    from srhip import ops
    for (H, W), (Hp, Wp) in C.INGEST_SHAPES:
        pages = C.ingest_pages(dtype, in_max, B, H, W, seed=H * 100 + W + B)
        want = C.ingest_pad_ref(pages, in_max, Hp, Wp)
        got = ops.ingest_pad(torch.from_numpy(pages).cuda(), in_max, Hp, Wp)
        assert got.dtype == torch.float32 and tuple(got.shape) == (B, Hp, Wp)
        assert torch.equal(got.cpu(), want), (dtype, in_max, B, (H, W), (Hp, Wp))


def test_ingest_pad_off_alignment_and_inside_its_buffers():
    """source and destination one element past an aligned address (heads and tails everywhere), between guard values"""
    from srhip import ops
    for dtype, in_max in C.INGEST_RANGES:
        tdt = torch.uint8 if dtype == np.uint8 else torch.uint16
        for (H, W), (Hp, Wp) in C.INGEST_SHAPES:
            pages = C.ingest_pages(dtype, in_max, 2, H, W, seed=7)
            sbuf = torch.empty(2 * H * W + 1, dtype=tdt, device="cuda")
            src = sbuf[1:].view(2, H, W)
            src.copy_(torch.from_numpy(pages))
            n = 2 * Hp * Wp
            dbuf = torch.full((n + 9,), -7.0, device="cuda")
            out = dbuf[5:5 + n].view(2, Hp, Wp)
            assert ops.ingest_pad(src, in_max, Hp, Wp, out=out).data_ptr() == out.data_ptr()
            host = dbuf.cpu()
            assert torch.equal(host[5:5 + n].view(2, Hp, Wp), C.ingest_pad_ref(pages, in_max, Hp, Wp))
            assert (host[:5] == -7).all() and (host[5 + n:] == -7).all()


def test_ingest_pad_refuses():
    from srhip import ops
    from srhip._lib import SrhipError
    (H, W), (Hp, Wp) = C.INGEST_TOO_SMALL
    with pytest.raises(SrhipError, match="pad exceeds the page"):          # 7 rows cannot give 9 flipped ones
        ops.ingest_pad(torch.zeros(1, H, W, dtype=torch.uint8, device="cuda"), 255, Hp, Wp)
    with pytest.raises(SrhipError, match="pad exceeds the page"):
        ops.ingest_pad(torch.empty(1, W, H, dtype=torch.uint16, device="cuda"), 65535, Wp, Hp)
    with pytest.raises(SrhipError, match="smaller than the page"):
        ops.ingest_pad(torch.zeros(1, 8, 8, dtype=torch.uint8, device="cuda"), 255, 8, 7)
    with pytest.raises(SrhipError, match="in_max"):
        ops.ingest_pad(torch.zeros(1, 8, 8, dtype=torch.uint8, device="cuda"), 4095, 8, 8)
    with pytest.raises(SrhipError, match="GPU only"):
        ops.ingest_pad(torch.zeros(1, 8, 8, dtype=torch.uint8), 255, 8, 8)
    with pytest.raises(SrhipError, match="uint8 / uint16"):
        ops.ingest_pad(torch.zeros(1, 8, 8, device="cuda"), 255, 8, 8)


# ---------------------------------------------------------------- srhip_emit_uint
@pytest.fixture(scope="module")
def emit_x():
    return C.emit_input()[0]


@pytest.mark.parametrize("bits", (8, 16))
def test_emit_uint_is_the_statement(emit_x, bits):
    from srhip import ops
    m = 2 ** bits - 1
    want = C.emit_ref(emit_x, m)[:, :C.EMIT_HO, :C.EMIT_WO].to(torch.int64)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = ops.emit_uint(emit_x.cuda(), bits, C.EMIT_HO, C.EMIT_WO, flag=flag)
    assert got.dtype == (torch.uint8 if bits == 8 else torch.uint16) and tuple(got.shape) == (C.EMIT_B, C.EMIT_HO, C.EMIT_WO)
    assert torch.equal(got.cpu().to(torch.int64), want)
    assert flag.item() == 0
    # the numpy statement says the same (it is what the CPU test checks by hand)
    assert np.array_equal(got.cpu().to(torch.int64).numpy(), C.emit_value(emit_x.numpy(), m)[:, :C.EMIT_HO, :C.EMIT_WO])
    # without a flag
    assert torch.equal(ops.emit_uint(emit_x.cuda(), bits, C.EMIT_HO, C.EMIT_WO), got)


@pytest.mark.parametrize("bits", (8, 16))
def test_emit_uint_flags_what_is_not_finite_inside_the_crop(emit_x, bits):
    from srhip import ops
    m = 2 ** bits - 1
    want = C.emit_ref(emit_x, m)[:, :C.EMIT_HO, :C.EMIT_WO].to(torch.int64)

    def run(x):
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        return ops.emit_uint(x.cuda(), bits, C.EMIT_HO, C.EMIT_WO, flag=flag).cpu().to(torch.int64), flag.item()
    # outside the crop (below it, right of it, in the last plane's corner): not looked at
    x = emit_x.clone()
    x[0, C.EMIT_HO, 0] = float("nan")
    x[1, 0, C.EMIT_WO] = float("inf")
    x[1, -1, -1] = float("-inf")
    got, flag = run(x)
    assert flag == 0 and torch.equal(got, want)
    # inside: NaN stores 0, +inf what the clamp gives, -inf 0; each sets the flag, the other pixels are untouched
    for pos, val, stored in (((1, C.EMIT_HO - 1, C.EMIT_WO - 1), float("nan"), 0), ((0, 3, 5), float("nan"), 0),
                             ((0, 0, 0), float("inf"), m), ((1, 7, 32), float("-inf"), 0)):
        x = emit_x.clone()
        x[pos] = val
        got, flag = run(x)
        exp = want.clone()
        exp[pos] = stored
        assert flag == 1 and torch.equal(got, exp), (pos, val)


def test_emit_uint_off_alignment_and_inside_its_buffers(emit_x):
    from srhip import ops
    from srhip._lib import SrhipError
    n_in = emit_x.numel()
    for bits, tdt in ((8, torch.uint8), (16, torch.uint16)):
        m = 2 ** bits - 1
        xbuf = torch.zeros(n_in + 1, device="cuda")
        x = xbuf[1:].view(emit_x.shape)
        x.copy_(emit_x)
        n = C.EMIT_B * C.EMIT_HO * C.EMIT_WO
        dbuf = torch.full((n + 8,), 77, dtype=torch.uint8 if bits == 8 else torch.int16, device="cuda").view(tdt)
        out = dbuf[3:3 + n].view(C.EMIT_B, C.EMIT_HO, C.EMIT_WO)
        ops.emit_uint(x, bits, C.EMIT_HO, C.EMIT_WO, out=out)
        host = dbuf.cpu().to(torch.int64)
        assert torch.equal(host[3:3 + n].view(out.shape), C.emit_ref(emit_x, m)[:, :C.EMIT_HO, :C.EMIT_WO].to(torch.int64))
        assert (host[:3] == 77).all() and (host[3 + n:] == 77).all()
    with pytest.raises(SrhipError, match="not inside the image"):
        ops.emit_uint(emit_x.cuda(), 8, C.EMIT_HS + 1, C.EMIT_WO)
    with pytest.raises(SrhipError, match="bits 8 or 16"):
        ops.emit_uint(emit_x.cuda(), 12, C.EMIT_HO, C.EMIT_WO)
    with pytest.raises(SrhipError, match="GPU only"):
        ops.emit_uint(emit_x, 8, C.EMIT_HO, C.EMIT_WO)


# ---------------------------------------------------------------- the pipeline
def _lr_pages():
    return np.stack([np.asarray(Image.open(os.path.join(FX, "data", "caco2", "t", f"l_{i}.tif"))) for i in range(3)])


@pytest.fixture(scope="module")
def composed():
    """What was there before this path, computed once: the three LR tiles of the fixture / 255 as one batch of 3 through
    _forward_with_padding, plain and in test mode 2 (refield 8, min_size 64).  {mode: float32 E [3, 128, 136] on the CPU}"""
    if not torch.cuda.is_available():
        return None
    from srhip.predict import load_config
    from dlib.models.select_model import define_model
    from dlib.utils.utils_trainer import _forward_with_padding
    pages = _lr_pages()
    assert pages.dtype == np.uint8 and pages.shape == (3, 16, 17)
    out = {}
    args = load_config(EXP)
    torch.cuda.set_device(0)
    model = define_model(args)
    model.load()
    model.netG.eval()
    for mode in (0, 2):
        if mode:
            args.test_mode, args.test_refield, args.test_min_size = mode, 8, 64
        data = {"l_im": torch.from_numpy(np.float32(pages / 255.))[:, None], "h_im": torch.zeros(3, 1, 128, 136)}
        model = _forward_with_padding(data, model, args)
        out[mode] = model.E.detach().float().contiguous().cpu()[:, 0]
        assert tuple(out[mode].shape) == (3, 128, 136) and torch.isfinite(out[mode]).all()
    return out


def _u8_of(E):
    from dlib.metrics import tensor2uint82float
    return tensor2uint82float(E.cuda().contiguous()).to(torch.uint8).cpu().numpy()


@pytest.mark.parametrize("mode", (0, 2))
def test_predictor_is_forward_with_padding_and_tensor2uint(composed, mode):
    from srhip.predict import Predictor
    pred = Predictor(EXP, batch=3, test_mode=mode, test_refield=8, test_min_size=64)
    got = pred.run(_lr_pages())
    assert got.dtype == np.uint8 and got.shape == (3, 128, 136)
    assert np.array_equal(got, _u8_of(composed[mode]))
    pred.out_dtype = "float32"
    assert np.array_equal(pred.run(_lr_pages()), composed[mode].numpy())


def test_16_bit_pages_give_what_the_8_bit_pages_give(composed):
    """257 v / 65535 and v / 255 are the same real number: the uint16 stack gives the 8-bit run's float output, and its
    uint16 pages are that output clamped, times 65535, rounded"""
    from srhip.predict import Predictor
    p16 = (_lr_pages().astype(np.uint16) * 257)
    pred = Predictor(EXP, batch=3, out_dtype="float32")
    E = pred.run(p16)
    assert E.dtype == np.float32 and np.array_equal(E, composed[0].numpy())
    pred.out_dtype = "same"
    got = pred.run(p16)
    assert got.dtype == np.uint16
    assert np.array_equal(got.astype(np.int64), (composed[0].clamp(0, 1) * 65535).round().to(torch.int64).numpy())
    # groups smaller than the stack: the pages come back in order (each group a batch of its own)
    pred.batch = 2
    again = pred.run(p16)
    assert again.shape == got.shape and np.array_equal(again[2], Predictor(EXP, batch=1).run(p16[2:])[0])


def test_command_line_writes_what_the_predictor_returns(tmp_path, composed):
    from srhip.predict import Predictor
    cli = _cli()
    src = tmp_path / "in"
    src.mkdir()
    p16 = (_lr_pages().astype(np.uint16) * 257)
    ims = [Image.fromarray(p) for p in p16]
    ims[0].save(str(src / "a_stack.tif"), save_all=True, append_images=ims[1:])
    one = np.random.RandomState(5).randint(0, 256, size=(1, 12, 10)).astype(np.uint8)
    Image.fromarray(one[0]).save(str(src / "b_single.png"))
    out = tmp_path / "out"
    rc = cli.predict(["--exp_path", EXP, "--input", str(src), "--output", str(out), "--batch", "3"])
    assert rc == 0
    assert sorted(os.listdir(out)) == ["a_stack_x8.tif", "b_single_x8.png", "log.json", "log.txt"]
    pred = Predictor(EXP, batch=3)
    with Image.open(str(out / "a_stack_x8.tif")) as im:
        assert im.n_frames == 3 and im.mode == "I;16"
    assert np.array_equal(np.stack(cli.read_pages(str(out / "a_stack_x8.tif"))), pred.run(p16))
    with Image.open(str(out / "b_single_x8.png")) as im:
        assert getattr(im, "n_frames", 1) == 1 and im.mode == "L" and im.size == (80, 96)
    assert np.array_equal(cli.read_pages(str(out / "b_single_x8.png"))[0], pred.run(one)[0])
    log = (out / "log.txt").read_text()
    assert "a_stack.tif: 16 x 17 uint16, 3 page(s)" in log and "b_single.png: 12 x 10 uint8, 1 page(s)" in log


@pytest.mark.parametrize("net,method", (("EDSR_LIIF", "EDSR_LIIF"), ("SRCNN", "SRCNN"), ("DSR-Splines", "DSR-SPLINES")))
def test_other_nets_run_without_padding(tmp_path, net, method):
    """Nets other than SwinIR on 8-bit pages: no padding, an odd 9 x 13 page, x2.  A tiny EDSR (1 block, 16 features); SRCNN,
    whose input is the page brought to the target size by the cv2-style cubic of the existing lowres.l_to_h path; the
    registry's DSR-Splines.  The composition is uint8 / 255 -> feed_data -> test() -> tensor2uint82float."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "sr-caco-2_amd"))
    import main as M
    from dlib.datasets import lowres
    from dlib.models.select_model import define_model
    from dlib.utils.utils_config import save_config
    from srhip import ops
    from srhip.predict import Predictor
    args = M.parse_input(f"--net_type {net} --method {method} --scale 2".split())
    if net == "EDSR_LIIF":
        args.netG["EDSR_LIIF_n_resblocks"], args.netG["EDSR_LIIF_n_feats"] = 1, 16
    exp = tmp_path / "exp"
    (exp / "best-models").mkdir(parents=True)
    save_config(args, str(exp), "config_model.yml")
    torch.manual_seed(0)
    torch.cuda.set_device(0)
    model = define_model(args)
    torch.save(model.netG.state_dict(), str(exp / "best-models" / "G-model.pth"))
    pages = np.random.RandomState(1).randint(0, 256, size=(2, 9, 13)).astype(np.uint8)
    data = {"l_im": torch.from_numpy(np.float32(pages / 255.))[:, None]}
    if net == "SRCNN":
        data["l_to_h_img"] = ops.u8_to_unit(lowres.l_to_h(torch.from_numpy(pages).cuda(), (18, 26)))[:, None]
    model.feed_data(data, need_H=False)
    model.test()
    E = model.E.detach().float().contiguous().cpu()[:, 0]
    assert tuple(E.shape) == (2, 18, 26)
    got = Predictor(str(exp)).run(pages)
    assert got.dtype == np.uint8 and np.array_equal(got, _u8_of(E))
    # the float output as well: an image, not a constant (a randomly initialised SRCNN lies below 0, its pages are all 0)
    assert E.std() > 0 and np.array_equal(Predictor(str(exp), out_dtype="float32").run(pages), E.numpy())
    if net == "EDSR_LIIF":
        # weights that are not finite: the group's flag comes back set and nothing is returned for its pages
        from srhip.predict import NonFiniteError
        sd = torch.load(str(exp / "best-models" / "G-model.pth"), map_location="cpu")
        first = next(k for k, v in sd.items() if v.dtype == torch.float32 and v.dim() == 4)
        sd[first] = torch.full_like(sd[first], float("nan"))
        torch.save(sd, str(exp / "best-models" / "G-model.pth"))
        for out_dtype in ("same", "float32"):
            with pytest.raises(NonFiniteError) as e:
                Predictor(str(exp), out_dtype=out_dtype).run(pages)
            assert e.value.pages == [0, 1]
