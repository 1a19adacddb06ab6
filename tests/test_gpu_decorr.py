"""Image decorrelation analysis on the device: srhip_metrics_decorr_lv against the float64 statement of tests/decorr_ref.py on
the images of tests/decorr_cases.py, dlib.metrics.decorr, and predict.py --resolution True on the experiment fixture.

Gates.  The 21 curves: 64 e_ref, e_ref the statement's own rounding (np.fft.fft2 against a direct DFT with np.longdouble sums over
the cases with S <= 128, tests/decorr_cases.py::e_ref; 5.2e-16, so the gate is 3.3e-14), the rule and the reasoning of the Fourier
ring correlation tests.  The amplitude is a curve value: the same gate.  Rings are integers: the best ring, the index of the best
curve and all 21 peak rings are EQUAL; test_cpu_decorr.py asserts that no image is marked (no decision of the peak search or of
the banks was taken by less than 1e-10, far above the gate), so they cannot differ for rounding.  sigma: the widths come through
log, linspace and exp, at most four roundings of an ulp in the log domain, where |ln sigma| <= ln 1024 = 6.9: 64 eps relative."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

import decorr_cases as K  # noqa: E402
import decorr_ref as D  # noqa: E402
import frc_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXP = os.path.join(ROOT, "tests", "golden", "eval_exp", "exp")
NAN = float("nan")
EPS = float(np.finfo(np.float64).eps)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from srhip import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits64(t):
    return t.contiguous().view(torch.int64).cpu()


def _call(ops, X, L=255, lv=False, ws=None, curves=True):
    """the raw call: a NaN workspace of the declared size with a NaN guard behind it, NaN outputs with guards of their own"""
    B, (H, W) = X.shape[0], X.shape[-2:]
    need = ops.lib.srhip_metrics_decorr_lv_ws(B, H, W)
    ws = need if ws is None else ws
    guard = 16
    buf = torch.full((max(ws, 1) + guard,), NAN, dtype=torch.float64, device="cuda")
    nr = max(ops.frc_side(H, W), 2) // 2 + 1
    out = torch.full((B * 5 + guard,), NAN, dtype=torch.float64, device="cuda")
    cv = torch.full((B * 21 * nr + guard,), NAN, dtype=torch.float64, device="cuda")
    pk = torch.full((B * 21 + guard,), -7, dtype=torch.int32, device="cuda")
    ops.call("srhip_metrics_decorr_lv", X.data_ptr(), B, H, W, L, int(lv), buf.data_ptr(), ws, out.data_ptr(),
             cv.data_ptr() if curves else None, pk.data_ptr() if curves else None, ops._st())
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[max(ws, 1):]).all()), "the guard behind the workspace was written"
    assert bool(torch.isnan(out[B * 5:]).all()) and bool(torch.isnan(cv[B * 21 * nr:]).all()) and bool((pk[B * 21:] == -7).all())
    if not curves:
        assert bool(torch.isnan(cv).all()) and bool((pk == -7).all())
    return out[:B * 5].view(B, 5).cpu(), cv[:B * 21 * nr].view(B, 21, nr).cpu(), pk[:B * 21].view(B, 21).cpu()


def _against_statement(tag, out, cv, pk, each, bound):
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(cv).all())
    worst = 0.0
    for i, o in enumerate(each):
        e_curve = float(np.abs(cv[i].numpy() - o["curves"]).max())
        e_amp = abs(out[i, 2].item() - o["amp"])
        worst = max(worst, e_curve)
        print(f"[decorr] {tag}[{i}]: curves {e_curve:.3e} amp {e_amp:.3e} (gate {bound:.3e})   ring {int(out[i, 1])} cut "
              f"{out[i, 0].item():.6f} amp {out[i, 2].item():.4f} sigma {out[i, 3].item():.4f}   statement: ring {o['ring']} best "
              f"{o['best']} margin {o['margin']:.2e}")
        assert e_curve <= bound, f"curves: {e_curve:.3e} above {bound:.3e}"
        assert e_amp <= bound, f"amp: {e_amp:.3e} above {bound:.3e}"
        assert pk[i].tolist() == o["peaks"].tolist(), "peak rings"
        assert int(out[i, 1].item()) == o["ring"] and out[i, 1].item() == float(o["ring"])
        assert int(np.argmax(pk[i].numpy())) == o["best"], "the index of the best curve"
        assert out[i, 0].item() == o["ring"] / (o["side"] // 2) and out[i, 4].item() == float(o["side"])
        assert abs(out[i, 3].item() - o["sigma"]) <= 64 * EPS * o["sigma"], "sigma"
    return worst


@pytest.mark.parametrize("name", list(K.CASES))
def test_metrics_decorr_lv(ops, name):
    """kernel against statement: curves, amplitude, rings; two calls give the same bits; without the optional pointers the same
    result; the wrapper is the raw call"""
    B, h, w, N, lv, _ = K.CASES[name]
    X = dev(K.images(name))
    out, cv, pk = _call(ops, X, N, lv)
    assert cv.shape == (B, 21, R.side(h, w) // 2 + 1)
    _against_statement(name, out, cv, pk, K.expect(name), K.bound())
    out2, cv2, pk2 = _call(ops, X, N, lv)
    assert torch.equal(bits64(out2), bits64(out)) and torch.equal(bits64(cv2), bits64(cv)) and torch.equal(pk2, pk), "two calls"
    assert torch.equal(bits64(_call(ops, X, N, lv, curves=False)[0]), bits64(out)), "without curves and peaks: other bits"
    wo, wc, wp = ops.metrics_decorr_lv(X, N, lv, curves=True)
    assert torch.equal(bits64(wo), bits64(out)) and torch.equal(bits64(wc), bits64(cv)) and torch.equal(wp.cpu(), pk)
    assert torch.equal(bits64(ops.metrics_decorr_lv(X, N, lv)), bits64(out)), "the wrapper: other bits"


@pytest.mark.parametrize("N", (255, 65535))
def test_levels_in_give_the_same_bits(ops, N):
    """a float input and its own tensor2levels output under inputs_are_levels"""
    X = dev(K.images("3x70x151"))
    lv = ops.tensor2levels(X, N)
    a, b = _call(ops, X, N, False), _call(ops, lv, N, True)
    assert all(torch.equal(bits64(u.double()), bits64(v.double())) for u, v in zip(a, b))


def test_odd_and_even_batches_agree_image_by_image(ops):
    """an image beside a zero partner (the tail of an odd batch), beside another image, and as either half of its pair: the
    spectra come out of different complex transforms, so the curves agree within the gate, and every ring is the same"""
    X = K.images("3x70x151")
    each, bound = K.expect("3x70x151"), K.bound()
    odd = _call(ops, dev(X))
    even = _call(ops, dev(np.concatenate([X, X[:1]])))
    swapped = _call(ops, dev(X[[1, 0, 2, 2]]))
    alone = [_call(ops, dev(X[i:i + 1])) for i in range(3)]
    _against_statement("B=4", even[0][:3], even[1][:3], even[2][:3], each, bound)
    _against_statement("B=4[3]", even[0][3:], even[1][3:], even[2][3:], each[:1], bound)
    _against_statement("swapped", *(t[[1, 0, 2]] for t in swapped), each, bound)
    _against_statement("swapped[3]", *(t[3:] for t in swapped), each[2:], bound)
    for i in range(3):
        _against_statement(f"B=1 image {i}", *alone[i], each[i:i + 1], bound)
        assert torch.equal(odd[2][i], even[2][i]) and torch.equal(odd[2][i], alone[i][2][0])
        assert (odd[1][i] - even[1][i]).abs().max().item() <= 2 * bound and (odd[1][i] - alone[i][1][0]).abs().max().item() <= 2 * bound
    # the first pair of B = 3 and of B = 4 is the same transform
    assert torch.equal(bits64(odd[1][:2]), bits64(even[1][:2])) and torch.equal(bits64(odd[0][:2]), bits64(even[0][:2]))


def test_the_entry_point_refuses(ops):
    """a short workspace, a side below 32, a white level below 255: refused before any launch; empty images give cut 0"""
    x = torch.zeros(3, 1, 64, 80, device="cuda")
    need = ops.lib.srhip_metrics_decorr_lv_ws(3, 64, 80)
    assert need == 2 * (2 * 64 * 64 + 5 * 33 * 33)
    with pytest.raises(ops.SrhipError, match=f"holds {need - 1} doubles, the call needs {need}"):
        _call(ops, x, ws=need - 1)
    for shape in ((31, 64), (64, 31)):
        y = x[:, :, :shape[0], :shape[1]].contiguous()
        assert ops.lib.srhip_metrics_decorr_lv_ws(3, *shape) == 0
        with pytest.raises(ops.SrhipError, match="at least 32"):
            _call(ops, y, ws=1 << 16)
        with pytest.raises(ops.SrhipError, match="at least 32"):
            ops.metrics_decorr_lv(y)
    with pytest.raises(ValueError, match="255 .. 65535"):
        ops.metrics_decorr_lv(x, 254)
    with pytest.raises(ops.SrhipError, match="255 .. 65535"):
        _call(ops, x, L=254)
    out, cv, pk = _call(ops, x)                    # empty images: every denominator is 0, every curve is 0, no peak, no NaN
    assert cv.abs().max().item() == 0.0 and pk.abs().max().item() == 0
    assert out.tolist() == [[0.0, 0.0, 0.0, 0.0, 64.0]] * 3


def test_metrics_surface(ops):
    from dlib import metrics
    name = "3x70x151"
    B, h, w, N, _, _ = K.CASES[name]
    X = dev(K.images(name))
    out, cv, pk = _call(ops, X, N)
    d = metrics.decorr(X)
    assert list(d) == ["cut", "ring", "amp", "sigma", "side"] and d["side"] == 64
    assert all(d[k].shape == (B,) and d[k].is_cuda for k in ("cut", "ring", "amp", "sigma"))
    assert d["cut"].dtype == d["amp"].dtype == d["sigma"].dtype == torch.float64 and d["ring"].dtype == torch.int64
    for k, col in (("cut", 0), ("amp", 2), ("sigma", 3)):
        assert torch.equal(bits64(d[k]), bits64(out[:, col]))
    assert d["ring"].tolist() == [o["ring"] for o in K.expect(name)]
    full = metrics.decorr(X, curves=True)
    assert list(full) == ["cut", "ring", "amp", "sigma", "side", "curves", "peaks"]
    assert torch.equal(bits64(full["curves"]), bits64(cv)) and torch.equal(full["peaks"].cpu(), pk) and full["peaks"].dtype == torch.int32
    lv = metrics.decorr(metrics.tensor2levels(X, 4095), levels=4095, inputs_are_levels=True)
    fl = metrics.decorr(X, levels=4095)
    assert all(torch.equal(lv[k], fl[k]) for k in ("cut", "ring", "amp", "sigma"))
    with pytest.raises(RuntimeError, match="GPU only"):
        metrics.decorr(X.cpu())
    assert "decorr" in metrics.__all__


# ------------------------------------------------------------------ predict.py --resolution True
def _pages():
    """three 8-bit LR pages of 40 x 45: emitters under a PSF, the smallest side the option takes and more"""
    return np.stack([np.rint(255.0 * K.dots(40, 45, 40 + i, sigma=1.2)).astype(np.uint8) for i in range(3)])


def _by_hand(ops, pred, pages, in_max, out_levels):
    """dlib.metrics.decorr on the tensors the run saw, group by group: the ingested pages without their padding, and the float
    output of the same groups (out_dtype float32) cropped to the page"""
    from dlib import metrics
    from srhip.predict import Predictor, padded_size, resolution_record
    H, W = pages.shape[-2:]
    Hp, Wp = padded_size(pred.args, H, W)
    flt = Predictor(EXP, batch=pred.batch, in_max=pred.in_max, out_dtype="float32").run(pages)
    want = []
    for g0 in range(0, len(pages), pred.batch):
        grp = pages[g0:g0 + pred.batch]
        lr = ops.ingest_pad(dev(grp), in_max, Hp, Wp).view(len(grp), 1, Hp, Wp)[:, :, :H, :W].contiguous()
        r_in = metrics.decorr(lr, levels=in_max)
        r_out = metrics.decorr(dev(flt[g0:g0 + pred.batch])[:, None], levels=out_levels)
        for i in range(len(grp)):
            want.append(resolution_record(pred.scale, *({"side": r["side"], "cut": r["cut"][i].item(), "amp": r["amp"][i].item()}
                                                        for r in (r_in, r_out))))
    return want


@pytest.mark.parametrize("dtype,in_max,out_levels", (("uint8", 255, 255), ("uint16", 65535, 65535)))
def test_predictor_with_resolution(ops, dtype, in_max, out_levels):
    """run(pages, resolution=True): the pages of a run without the option, bit for bit; last_resolution is metrics.decorr by hand"""
    from srhip.predict import Predictor
    pages = _pages().astype(dtype) * (1 if dtype == "uint8" else 257)
    pred = Predictor(EXP, batch=2)
    plain = pred.run(pages)
    assert pred.last_resolution is None
    got = pred.run(pages, resolution=True)
    assert got.dtype == plain.dtype and np.array_equal(got, plain)
    recs = pred.last_resolution
    assert len(recs) == 3 and all(list(r) == ["in", "out", "gain"] for r in recs)
    assert recs == _by_hand(ops, pred, pages, in_max, out_levels)
    for r in recs:
        assert r["in"]["side"] == 32 and r["out"]["side"] == 256 and list(r["in"]) == ["side", "cut", "res_px", "amp"]
        for side in ("in", "out"):
            assert (r[side]["res_px"] is None) == (r[side]["cut"] == 0.0)
            if r[side]["cut"]:
                assert r[side]["res_px"] == 2.0 / r[side]["cut"]
        if r["gain"] is not None:
            assert r["gain"] == (r["in"]["res_px"] * 8) / r["out"]["res_px"]
    print(f"[decorr] predictor {dtype}: {recs}")
    assert np.array_equal(pred.run(pages), plain) and pred.last_resolution is None


def test_command_line_with_resolution(tmp_path):
    """predict.py --resolution True: the output files of a run without the flag, byte for byte, plus resolution.yml with what
    the Predictor reports and one more log line per file"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from PIL import Image
    from srhip.predict import Predictor
    spec = importlib.util.spec_from_file_location("srhip_predict_cli_res", os.path.join(ROOT, "sr-caco-2_amd", "predict.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    src = tmp_path / "in"
    src.mkdir()
    pages = _pages()
    ims = [Image.fromarray(p) for p in pages[:2]]
    ims[0].save(str(src / "a_stack.tif"), save_all=True, append_images=ims[1:])
    Image.fromarray(pages[2]).save(str(src / "b_single.png"))
    outs = {}
    for name, flags in (("plain", []), ("res", ["--resolution", "True"])):
        outs[name] = tmp_path / name
        assert cli.predict(["--exp_path", EXP, "--input", str(src), "--output", str(outs[name]), "--batch", "2"] + flags) == 0
    files = ["a_stack_x8.tif", "b_single_x8.png", "log.json", "log.txt"]
    assert sorted(os.listdir(outs["plain"])) == files and sorted(os.listdir(outs["res"])) == sorted(files + ["resolution.yml"])
    for f in files[:2]:
        assert open(outs["plain"] / f, "rb").read() == open(outs["res"] / f, "rb").read(), f
    rep = yaml.safe_load(open(outs["res"] / "resolution.yml"))
    pred = Predictor(EXP, batch=2)
    pred.run(pages[:2], resolution=True)
    want = {"a_stack.tif": [{"page": k, **r} for k, r in enumerate(pred.last_resolution)]}
    pred.run(pages[2:], resolution=True)
    want["b_single.png"] = [{"page": 0, **pred.last_resolution[0]}]
    assert rep == want and list(rep) == ["a_stack.tif", "b_single.png"]
    log, log0 = (outs["res"] / "log.txt").read_text(), (outs["plain"] / "log.txt").read_text()
    assert log.count(": resolution ") == 2 and "resolution" not in log0
    # a page below 32 pixels: refused by file and page before the device is used
    Image.fromarray(pages[0][:31]).save(str(src / "c_small.png"))
    with pytest.raises(cli.PredictError, match=r"c_small\.png, page 0: --resolution True: a 31 x 45 page is too small.*at least 32"):
        cli.predict(["--exp_path", EXP, "--input", str(src), "--output", str(tmp_path / "no"), "--resolution", "True"])
    assert not os.path.exists(tmp_path / "no")
