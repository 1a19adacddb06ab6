"""Fourier ring correlation on the device: srhip_metrics_frc_lv against the float64 statement of tests/frc_ref.py on the pairs of
tests/frc_cases.py, dlib.metrics.frc / mbatch_gpu_calculate_frc, metrics.sweep beside it, and eval.py --frc True on the
experiment fixture.

Gates.  The curve: 64 e_ref, e_ref the statement's own rounding (np.fft.fft2 against a direct DFT in np.longdouble over the cases
with S <= 128, tests/frc_cases.py::e_ref; 9.4e-16, so the gate is 6.0e-14).  The kernel differs from pocketfft in butterfly
order, twiddle source and ring-sum order, each a few eps a stage; the factor covers S = 2048 and rings of ~6 S terms.  The
cutoff: that bound through the interpolation, 2 bound / ((p - FRC[r]) S/2) plus one spacing.  test_cpu_frc.py asserts that no
case is marked (no curve value within 1e-6 of T up to the crossing ring), so the crossing ring itself cannot differ."""
import os
import pickle
import shutil

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

import frc_cases as K  # noqa: E402
import frc_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = os.path.join(ROOT, "tests", "golden", "eval_exp")
DS = "caco2_test_X_8_in_64_out_512_cell_CELL0"
MTRS = ("psnr", "mse", "nrmse", "ssim", "psnr_y")
NAN = float("nan")
T = R.T_DEFAULT


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


def _call(ops, E, Hh, L=255, lv=False, thr=T, ws=None):
    """the raw call: a NaN workspace of the declared size with a NaN guard behind it, NaN outputs"""
    B, (H, W) = E.shape[0], E.shape[-2:]
    need = ops.lib.srhip_metrics_frc_lv_ws(B, H, W)
    ws = need if ws is None else ws
    guard = 16
    buf = torch.full((max(ws, 1) + guard,), NAN, dtype=torch.float64, device="cuda")
    nr = max(ops.frc_side(H, W), 2) // 2 + 1
    curve = torch.full((B, nr), NAN, dtype=torch.float64, device="cuda")
    cut = torch.full((B,), NAN, dtype=torch.float64, device="cuda")
    ops.call("srhip_metrics_frc_lv", E.data_ptr(), Hh.data_ptr(), B, H, W, L, int(lv), thr, buf.data_ptr(), ws, curve.data_ptr(),
             cut.data_ptr(), ops._st())
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[max(ws, 1):]).all()), "the guard behind the workspace was written"
    return curve.cpu(), cut.cpu()


@pytest.mark.parametrize("name", list(K.CASES))
def test_metrics_frc_lv(ops, name):
    """kernel against statement, curve and cutoff; two calls give the same bits; the wrapper is the raw call"""
    B, h, w, N, lv, _ = K.CASES[name]
    E, H = (dev(t) for t in K.images(name))
    want_curve, want_cut, each = K.expect(name)
    bound = K.bound()
    curve, cut = _call(ops, E, H, N, lv)
    assert curve.shape == want_curve.shape and bool(torch.isfinite(curve).all()) and bool(torch.isfinite(cut).all())
    e_curve = np.abs(curve.numpy() - want_curve).max()
    e_cut = np.abs(cut.numpy() - want_cut)
    gates = np.array([R.cut_bound(o, bound) for o in each])
    print(f"[frc] {name}: curve {e_curve:.3e} (gate {bound:.3e})   cut {e_cut.max():.3e} (gate {gates[e_cut.argmax()]:.3e})   "
          f"cut = {cut.tolist()}")
    assert e_curve <= bound, f"curve: {e_curve:.3e} above {bound:.3e}"
    assert bool((e_cut <= gates).all()), f"cut: {e_cut.tolist()} above {gates.tolist()}"
    curve2, cut2 = _call(ops, E, H, N, lv)
    assert torch.equal(bits64(curve2), bits64(curve)) and torch.equal(bits64(cut2), bits64(cut)), "two calls: other bits"
    wc, wk = ops.metrics_frc_lv(E, H, N, T, lv)
    assert torch.equal(bits64(wc), bits64(curve)) and torch.equal(bits64(wk), bits64(cut)), "the wrapper: other bits"


@pytest.mark.parametrize("h,w,N", ((32, 32, 255), (70, 151, 255), (128, 128, 65535), (512, 512, 255)))
def test_identical_images(ops, h, w, N):
    """E = H: every ring within the bound of 1, and nothing crosses: the cutoff is exactly 1.0"""
    H = dev(np.stack([K.target(h, w, 21), K.target(h, w, 22)]).astype(np.float32)[:, None])
    curve, cut = _call(ops, H, H, N)
    e = (curve - 1.0).abs().max().item()
    print(f"[frc] E = H {h}x{w} N={N}: {e:.3e} from 1")
    assert e <= K.bound() and cut.tolist() == [1.0, 1.0]


def test_more_noise_never_raises_the_cutoff(ops):
    Hn = K.target(256, 256, 31)
    Es = np.stack([K.prediction(Hn, 31, noise=n) for n in (0.003, 0.01, 0.03, 0.1)]).astype(np.float32)[:, None]
    Hs = np.repeat(Hn.astype(np.float32)[None, None], 4, axis=0)
    _, cut = _call(ops, dev(Es), dev(Hs))
    want = R.frc(Es, Hs)[1]
    print(f"[frc] noise 0.003 .. 0.1: cut {cut.tolist()}   statement {want.tolist()}")
    c = cut.tolist()
    assert all(a >= b for a, b in zip(c, c[1:])) and c[0] > c[-1] and 0.0 <= c[-1] and c[0] <= 1.0


@pytest.mark.parametrize("N", (255, 65535))
def test_levels_in_give_the_same_bits(ops, N):
    """a float input and its own tensor2levels output under inputs_are_levels"""
    E, H = (dev(t) for t in K.images("3x70x151"))
    a, b = ops.tensor2levels(E, N), ops.tensor2levels(H, N)
    assert torch.equal(a.cpu(), torch.from_numpy(R.levels(K.images("3x70x151")[0], N)))
    c0, k0 = _call(ops, E, H, N, False)
    c1, k1 = _call(ops, a, b, N, True)
    assert torch.equal(bits64(c0), bits64(c1)) and torch.equal(bits64(k0), bits64(k1))


def test_another_threshold(ops):
    E, H = (dev(t) for t in K.images("512x512"))
    N = K.CASES["512x512"][3]
    curve, cut = _call(ops, E, H, N, thr=0.5)
    o = R.cutoff(K.expect("512x512")[0][0], 0.5)
    assert not o["marked"] and torch.equal(bits64(curve), bits64(_call(ops, E, H, N)[0]))
    o["side"] = 512
    assert abs(cut[0].item() - o["cut"]) <= R.cut_bound(o, K.bound(), 0.5) and cut[0].item() < K.expect("512x512")[1][0]


def test_the_entry_point_refuses(ops):
    """a short workspace, a side below 32, a threshold outside (0, 1): refused before any launch"""
    x = torch.zeros(2, 1, 64, 80, device="cuda")
    need = ops.lib.srhip_metrics_frc_lv_ws(2, 64, 80)
    assert need == 2 * (2 * 64 * 64 + 3 * 33 * 33)
    with pytest.raises(ops.SrhipError, match=f"holds {need - 1} doubles, the call needs {need}"):
        _call(ops, x, x, ws=need - 1)
    for shape in ((31, 64), (64, 31)):
        y = x[:, :, :shape[0], :shape[1]].contiguous()
        assert ops.lib.srhip_metrics_frc_lv_ws(2, *shape) == 0
        with pytest.raises(ops.SrhipError, match="at least 32"):
            _call(ops, y, y, ws=1 << 16)
        with pytest.raises(ops.SrhipError, match="at least 32"):
            ops.metrics_frc_lv(y, y)
    for thr in (0.0, 1.0, -0.5, 1.5):
        with pytest.raises(ops.SrhipError, match=r"\(0, 1\)"):
            _call(ops, x, x, thr=thr)
        with pytest.raises(ValueError, match=r"\(0, 1\)"):
            ops.metrics_frc_lv(x, x, 255, thr)
    with pytest.raises(ValueError, match="255 .. 65535"):
        ops.metrics_frc_lv(x, x, 254)
    curve, cut = _call(ops, x, x)                  # two empty images: every product is 0, the curve is 0 and ring 0 is under T
    assert curve.abs().max().item() == 0.0 and cut.tolist() == [0.0, 0.0]


def test_metrics_surface_and_the_sweep_beside_it(ops):
    """metrics.frc and mbatch_gpu_calculate_frc: shapes, dtypes, the raw call's bits; metrics.sweep has the same keys and the
    same bits before and after FRC calls in this process"""
    from dlib import metrics
    name = "3x70x151"
    B, h, w, N, _, _ = K.CASES[name]
    E, H = (dev(t) for t in K.images(name))
    ths = (10, 50)
    before = metrics.sweep(E, H, border=8, thresholds=ths)
    curve, cut = _call(ops, E, H, N)
    out = metrics.frc(E, H)
    assert list(out) == ["curve", "cut", "side"] and out["side"] == 64
    assert out["curve"].shape == (B, 33) and out["cut"].shape == (B,) and out["curve"].dtype == out["cut"].dtype == torch.float64
    assert out["curve"].is_cuda and torch.equal(bits64(out["curve"]), bits64(curve)) and torch.equal(bits64(out["cut"]), bits64(cut))
    a, b = metrics.tensor2levels(E, 4095), metrics.tensor2levels(H, 4095)
    lv = metrics.frc(a, b, levels=4095, threshold=0.5, inputs_are_u8=True)
    fl = metrics.frc(E, H, levels=4095, threshold=0.5)
    assert torch.equal(bits64(lv["curve"]), bits64(fl["curve"])) and torch.equal(bits64(lv["cut"]), bits64(fl["cut"]))
    mb = metrics.mbatch_gpu_calculate_frc(a, b, levels=4095, threshold=0.5)
    assert mb.shape == (B,) and mb.dtype == torch.float64 and torch.equal(bits64(mb), bits64(lv["cut"]))
    with pytest.raises(RuntimeError, match="GPU only"):
        metrics.frc(E.cpu(), H.cpu())
    after = metrics.sweep(E, H, border=8, thresholds=ths)
    assert list(after) == list(before) == ["psnr", "psnr_y", "mse", "nrmse", "ssim"]
    assert all(after[k].dtype == before[k].dtype and torch.equal(after[k], before[k]) for k in before)


# ------------------------------------------------------------------ eval.py --frc True
def _eval_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("srhip_eval_frc", os.path.join(ROOT, "sr-caco-2_amd", "eval.py"))
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)
    return ev


def test_eval_py_with_frc(ops, tmp_path):
    """eval.py on two copies of the experiment fixture, with --frc True and without.  With the flag: frc_<ds>.yml for the net and
    for the bicubic row with threshold, mean_cut, images {side, cut, res_px} and mean_curve {128: 65 floats}; its cutoffs are
    the 'frc_cut' of details_*.yml and what metrics.frc gives on the same tensors.  Every other file is the one of the run
    without the flag, value for value (which tests/test_eval_fixture.py pins to expected/), and so are both trackers."""
    from dlib import metrics
    from dlib.models.select_model import define_model
    from dlib.utils.utils_dataloaders import get_all_eval_loaders
    from dlib.utils.utils_trainer import Interpolate, _forward_with_padding
    ev = _eval_module()
    runs = {}
    for name, flags in (("plain", []), ("frc", ["--frc", "True"])):
        exp = tmp_path / name
        shutil.copytree(os.path.join(FX, "exp"), exp)
        argv = ["--cudaid", "0", "--exp_path", str(exp), "--data_root", os.path.join(FX, "data"), "--splits_root",
                os.path.join(FX, "folds")] + flags
        runs[name] = (exp, argv, ev.evaluate_pretrained(argv))
    exp, argv, (tracker, roi) = runs["frc"]
    plain, _, (tracker0, roi0) = runs["plain"]
    assert tracker == tracker0 and roi == roi0
    out = exp / f"eval_test_{DS}"
    assert pickle.load(open(out / "tracker.pkl", "rb")) == tracker0 and pickle.load(open(out / "roi_tracker.pkl", "rb")) == roi0
    # what metrics.frc gives on the same tensors
    _, args = ev.load_args(argv)
    args.outd = args.outd_backup = str(exp)
    args.is_train, args.is_master = False, True
    args.netG['checkpoint_path_netG'] = os.path.join(str(exp), 'best-models/G-model.pth')
    model = define_model(args)
    model.load()
    model.netG.eval()
    base = Interpolate(task=args.task, scale=args.scale, scale_mode=args.basic_interpolation)
    want = {DS: {}, f"{DS}_bicubic": {}}
    for batch in get_all_eval_loaders(args, args.test_dsets, n=-1)[DS]:
        model = _forward_with_padding(batch, model, args)
        base.feed_data(batch)
        base.test()
        for row, m in ((DS, model), (f"{DS}_bicubic", base)):
            vis = m.current_visuals()
            fr = metrics.frc(vis['E'], vis['H'])
            assert fr["side"] == 128
            for i, img in enumerate(batch['h_id']):
                want[row][img] = (fr["cut"][i].item(), fr["curve"][i].cpu())
    names = sorted(os.listdir(plain / "best-models"))
    assert sorted(os.listdir(exp / "best-models")) == sorted(names + [f"frc_{DS}.yml", f"frc_{DS}_bicubic.yml"])
    for row in (DS, f"{DS}_bicubic"):
        rep = yaml.safe_load(open(exp / "best-models" / f"frc_{row}.yml"))
        det = yaml.safe_load(open(exp / "best-models" / f"details_{row}.yml"))
        det0 = yaml.safe_load(open(plain / "best-models" / f"details_{row}.yml"))
        assert sorted(rep) == ["images", "mean_curve", "mean_cut", "threshold"] and rep["threshold"] == T
        assert list(rep["images"]) == list(det) == list(det0) == ["t/h_0.tif", "t/h_1.tif", "t/h_2.tif"]
        for img in det:
            assert set(det[img]) == set(MTRS) | {"frc_cut"} and set(det0[img]) == set(MTRS)
            assert all(det[img][m] == det0[img][m] for m in MTRS)
            cut = want[row][img][0]
            assert det[img]["frc_cut"] == cut and 0.0 < cut <= 1.0
            assert rep["images"][img] == {"side": 128, "cut": cut, "res_px": 2.0 / cut}
        assert abs(rep["mean_cut"] - sum(want[row][img][0] for img in det) / 3.0) <= 1e-15
        assert list(rep["mean_curve"]) == [128] and len(rep["mean_curve"][128]) == 65
        mean = torch.stack([want[row][img][1] for img in det]).sum(0) / 3.0
        assert (torch.tensor(rep["mean_curve"][128], dtype=torch.float64) - mean).abs().max().item() <= 1e-15
        for f in (f"roi_details_{row}.yml", f"{row}.yaml", f"roi-{row}.yaml"):
            assert yaml.safe_load(open(exp / "best-models" / f)) == yaml.safe_load(open(plain / "best-models" / f)), f
    for row in (DS, f"{DS}_bicubic"):             # the previews of the first images, as without the flag
        previews = sorted(os.listdir(plain / "images" / "test" / row))
        assert "t_h_0.tif.png" in previews and sorted(os.listdir(exp / "images" / "test" / row)) == previews
    log, log0 = open(out / "log.txt").read(), open(plain / f"eval_test_{DS}" / "log.txt").read()
    assert log.count("frc_cut: ") == 2 and "frc" not in log0
    # the plain run's details are the reference's, under the tolerances of tests/test_eval_fixture.py
    for row in (DS, f"{DS}_bicubic"):
        det = yaml.safe_load(open(exp / "best-models" / f"details_{row}.yml"))
        ref = yaml.safe_load(open(os.path.join(FX, "expected", "best-models", f"details_{row}.yml")))
        for img in ref:
            for m in MTRS:
                tol = 0.01 if m in ("psnr", "psnr_y") else 5e-5 if m == "ssim" else 1e-4 * max(1.0, abs(ref[img][m]))
                assert abs(det[img][m] - ref[img][m]) <= tol, (row, img, m)
    # an image below 32 pixels: refused by set name, image id and the minimum when the first sweep meets it
    from dlib.utils import constants
    from dlib.utils.utils_trainer import fast_eval
    from dlib.utils.utils_tracker import init_tracker

    class Small:
        def __iter__(self):
            for b in get_all_eval_loaders(args, args.test_dsets, n=-1)[DS]:
                yield {**b, 'l_im': b['l_im'][..., :3, :], 'h_im': b['h_im'][..., :24, :]}
    with pytest.raises(ValueError, match=rf"--frc True: image t/h_0\.tif of {DS}_bicubic is 24 x 136.*at least 32"):
        fast_eval(base, Small(), f"{DS}_bicubic", constants.TESTSET, init_tracker(args), init_tracker(args, roi=True), args, -1, -1,
                  nbr_to_plot=0)
