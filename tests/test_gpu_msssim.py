"""Multi-scale SSIM on the device: srhip_metrics_msssim_lv against the float64 statement of tests/msssim_ref.py, dlib.metrics.sweep
(msssim=M) beside today's sweep, and eval.py --msssim True on the experiment fixture.

Gates: out[:, 0] and out[:, 1:] each by the suite's Gates rule at scale 1, e <= min(METRIC_SSIM = 5e-5, 3 e32), e32 the float32
statement's own distance from the float64 one (floored at 2^-24).  The kernel is float64 throughout, but it filters with the
separable float32 taps of srhip_metrics_ssim_lv while the statement has the reference's 2-D float32 window; the two windows' sums
differ from 1 by 1e-7, which sigma^2 = E[x^2] - E[x]^2 turns into up to 2e-5 of cs on a strongly (anti)correlated pair.  That is
the kernel's distance from the statement.  Its distance from the statement under the numpy form of its taps is printed beside it,
not gated: the taps are made on the host with expf, and one ulp in a tap moves the window's sum, and with it cs, as much again.

The 1 - H image: the issue expected every v_j below 0.  By the definition itself that cannot hold at five scales on these inputs:
a 5 x 5-smoothed uniform field has a variance of 2e-4 at scale 5, below C2 / 2 = 4.5e-4, so cs is positive there and the float64
statement gives v_5 = +0.61 (v_1 .. v_4 = -0.55, -0.61, -0.56, -0.23).  The test therefore asserts that the product is exactly
0.0, that v_1 is below 0, and that every v_j has the sign the float64 statement gives it; at two scales both are below 0."""
import os
import pickle
import shutil

import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

import step_kernel_cases as C  # noqa: E402
import msssim_ref as R  # noqa: E402
from test_gpu_tape_op_kernels import Gates, NAN  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = os.path.join(ROOT, "tests", "golden", "eval_exp")
DS = "caco2_test_X_8_in_64_out_512_cell_CELL0"
MTRS = ("psnr", "mse", "nrmse", "ssim", "psnr_y")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from srhip import ops as _ops
    return _ops


def dev(t):
    return t.cuda().contiguous()


def bits64(t):
    return t.contiguous().view(torch.int64).cpu()


def _call(ops, E, Hh, border, L, lv, M, ws=None, weights=None):
    """the raw call: a NaN workspace of the declared size with a NaN guard behind it, a NaN output"""
    import ctypes
    B, (H, W) = E.shape[0], E.shape[-2:]
    need = ops.lib.srhip_metrics_msssim_lv_ws(B, H, W, border, M)
    ws = need if ws is None else ws
    guard = 16
    buf = torch.full((max(ws, 1) + guard,), NAN, dtype=torch.float64, device="cuda")
    out = torch.full((B, max(M, 0) + 1), NAN, dtype=torch.float64, device="cuda")
    w = None if weights is None else ctypes.cast((ctypes.c_double * len(weights))(*weights), ctypes.c_void_p)
    ops.call("srhip_metrics_msssim_lv", E.data_ptr(), Hh.data_ptr(), B, H, W, border, L, int(lv), M, w, buf.data_ptr(), ws,
             out.data_ptr(), ops._st())
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[max(ws, 1):]).all()), "the guard behind the workspace was written"
    return out.cpu()


@pytest.mark.parametrize("B,h,w,border,M,L", R.CASES)
def test_metrics_msssim_lv(ops, B, h, w, border, M, L):
    E, Hf, a, b = (dev(t) for t in R.inputs(B, h, w, border, L))
    ref64, ref32 = R.expect(B, h, w, border, M, L)
    refk = R.msssim(a.cpu(), b.cpu(), L, border, M, as_kernel=True)
    with Gates(f"metrics_msssim_lv B={B} {h}x{w} border={border} M={M} L={L}") as G:
        out = _call(ops, E, Hf, border, L, False, M)
        G.true(out.shape == ref64.shape and bool(torch.isfinite(out).all()), "a slot was not written")
        for i in range(B):
            print(f"[v] {G.name} image {i}: msssim {out[i, 0]:.12f} v {[f'{v:+.9f}' for v in out[i, 1:].tolist()]}")
        print(f"[own window] {G.name}: {(out - refk).abs().max().item():.3e}")
        G(out[:, 0], ref64[:, 0], ref32[:, 0], C.METRIC_SSIM, "out[:, 0]", scale=1.0)
        G(out[:, 1:], ref64[:, 1:], ref32[:, 1:], C.METRIC_SSIM, "out[:, 1:]", scale=1.0)
        G.true((out[0] - 1.0).abs().max().item() <= 1e-12, f"identical images: {(out[0] - 1.0).abs().max().item():.3e} from 1")
        if B == 3:
            G.true(out[2, 0].item() == 0.0 and out[2, 1].item() < 0, f"1 - H: {out[2].tolist()}")
            G.true(torch.equal(out[2, 1:] < 0, ref64[2, 1:] < 0), "1 - H: a v_j has another sign than the float64 statement's")
            if M == 2:
                G.true(bool((out[2, 1:] < 0).all()), "1 - H at two scales: every v_j is below 0")
        # the definition's weights are the default; passing them is the same call
        G.true(torch.equal(bits64(_call(ops, E, Hf, border, L, False, M, weights=R.weights(M))), bits64(out)), "weights given: other bits")
        G.true(torch.equal(bits64(_call(ops, E, Hf, border, L, False, M)), bits64(out)), "two calls: other bits")
        G.true(torch.equal(bits64(_call(ops, a, b, border, L, True, M)), bits64(out)), "inputs_are_levels: other bits")
        G.true(torch.equal(bits64(ops.metrics_msssim_lv(E, Hf, border, L, M)), bits64(out)), "the wrapper: other bits")
        # an input pitched past w: the wrapper makes it contiguous
        wide = torch.full((2, B, 1, E.shape[2], E.shape[3] + 5), NAN, device="cuda")
        wide[0, ..., :E.shape[3]], wide[1, ..., :E.shape[3]] = E, Hf
        G.true(not wide[0, ..., :E.shape[3]].is_contiguous(), "the pitched view is contiguous")
        G.true(torch.equal(bits64(ops.metrics_msssim_lv(wide[0, ..., :E.shape[3]], wide[1, ..., :E.shape[3]], border, L, M)), bits64(out)),
               "a pitched input: other bits")
        # the constant pair
        ca, cb = (dev(t) for t in R.constant_pair(h, w, border, L))
        c64, c32 = R.msssim(ca.cpu(), cb.cpu(), L, border, M), R.msssim(ca.cpu(), cb.cpu(), L, border, M, torch.float32)
        cout = _call(ops, ca, cb, border, L, True, M)
        G(cout[:, 0], c64[:, 0], c32[:, 0], C.METRIC_SSIM, "constant pair out[:, 0]", scale=1.0)
        G(cout[:, 1:], c64[:, 1:], c32[:, 1:], C.METRIC_SSIM, "constant pair out[:, 1:]", scale=1.0)
        G.true((cout[0] - 1.0).abs().max().item() <= 1e-12, "the constant pair of equal images")


@pytest.mark.parametrize("L", (255, 4095))
@pytest.mark.parametrize("h,w,border", ((11, 11, 0), (43, 44, 3)))
def test_one_scale_is_srhip_metrics_ssim_lv(ops, h, w, border, L):
    """M = 1: out[:, 0] is slot 0 of srhip_metrics_ssim_lv on the same inputs (max(v, 0): the inputs have no negative mean)"""
    E, Hf, _, _ = (dev(t) for t in R.inputs(2, h, w, border, L))
    out = _call(ops, E, Hf, border, L, False, 1)
    y = ops.metrics_ssim_lv(E, Hf, border, (), L).cpu()[:, 0]
    e = ((out[:, 0] - y).abs() / y.abs().clamp(min=1.0)).max().item()
    print(f"[M=1] {h}x{w} border={border} L={L}: {e:.3e}")
    assert e <= 1e-12


def test_the_entry_point_refuses_by_number(ops):
    """argument checks that return before any launch: the size rule, M, L, a short workspace"""
    x = torch.zeros(1, 1, 177, 177, device="cuda")
    for shape, border, M, L, ws, text in (((160, 161), 0, 5, 255, None, "161"), ((161, 160), 0, 5, 255, None, "161"),
                                          ((176, 177), 8, 5, 255, None, "161"), ((161, 161), 0, 0, 255, None, "got 0"),
                                          ((161, 161), 0, 6, 255, None, "got 6"), ((161, 161), 0, 5, 254, None, "254")):
        with pytest.raises(ops.SrhipError, match=text):
            _call(ops, x[:, :, :shape[0], :shape[1]].contiguous(), x[:, :, :shape[0], :shape[1]].contiguous(), border, L, False, M, ws)
    need = ops.lib.srhip_metrics_msssim_lv_ws(1, 177, 177, 0, 5)
    with pytest.raises(ops.SrhipError, match=f"holds {need - 1} doubles, the call needs {need}"):
        _call(ops, x, x, 0, 255, False, 5, ws=need - 1)
    with pytest.raises(ops.SrhipError, match="161"):
        ops.metrics_msssim_lv(x[:, :, :160], x[:, :, :160], 0, 255, 5)
    with pytest.raises(ValueError, match="255 .. 65535"):
        ops.metrics_msssim_lv(x, x, 0, 254, 5)
    with pytest.raises(ValueError, match="1 .. 5"):
        ops.metrics_msssim_lv(x, x, 0, 255, 6)
    assert _call(ops, x, x, 0, 255, False, 5)[0].tolist() == [1.0] * 6


@pytest.mark.parametrize("B,h,w,border,M,L", R.CASES[1:4])
def test_sweep_with_msssim(ops, B, h, w, border, M, L):
    """sweep(msssim=M): today's five tensors with the bits of msssim=0, and 'msssim' = out[:, 0]; the float and the levels form;
    mbatch_gpu_calculate_msssim on the levels"""
    from dlib import metrics
    E, Hf, a, b = (dev(t) for t in R.inputs(B, h, w, border, L))
    ths = C.METRIC_SSIM_THS
    out = ops.metrics_msssim_lv(E, Hf, border, L, M)
    for args, lv in (((E, Hf), False), ((a, b), True)):
        s0, s = metrics.sweep(*args, border, ths, lv, levels=L), metrics.sweep(*args, border, ths, lv, levels=L, msssim=M)
        assert list(s0) == ["psnr", "psnr_y", "mse", "nrmse", "ssim"] and list(s) == list(s0) + ["msssim"]
        assert all(s[k].dtype == s0[k].dtype and torch.equal(s[k], s0[k]) for k in s0)
        assert s["msssim"].shape == (B,) and s["msssim"].dtype == torch.float64 and torch.equal(s["msssim"], out[:, 0])
    assert torch.equal(metrics.mbatch_gpu_calculate_msssim(a, b, border, L, M), out[:, 0])
    if L == 255:
        assert list(metrics.sweep(E, Hf, border, ths)) == ["psnr", "psnr_y", "mse", "nrmse", "ssim"]


# ------------------------------------------------------------------ eval.py --msssim True
def _eval_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("srhip_eval_msssim", os.path.join(ROOT, "sr-caco-2_amd", "eval.py"))
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)
    return ev


def test_eval_py_with_msssim(ops, tmp_path):
    """eval.py on two copies of the experiment fixture, with --msssim True --msssim_scales 4 and without.  The fixture's images
    are 128 x 136 under a border of 8, 112 x 120 after the crop: four scales need 81, five would need 161 (177 with the border)
    and are refused by name, image id and that number.  With the flag: details_*.yml of the net and of the bicubic row carry
    'msssim' per image, equal to metrics.sweep on the same tensors; tracker.pkl and the summary yaml have the key; roi_tracker.pkl,
    roi_details_* and roi-*.yaml do not; the other five values are those of the run without the flag, bit for bit."""
    from dlib import metrics
    from dlib.utils import constants
    from dlib.models.select_model import define_model
    from dlib.utils.utils_dataloaders import get_all_eval_loaders
    from dlib.utils.utils_trainer import Interpolate, _forward_with_padding
    ev = _eval_module()
    runs = {}
    for name, flags in (("plain", []), ("ms", ["--msssim", "True", "--msssim_scales", "4"])):
        exp = tmp_path / name
        shutil.copytree(os.path.join(FX, "exp"), exp)
        argv = ["--cudaid", "0", "--exp_path", str(exp), "--data_root", os.path.join(FX, "data"), "--splits_root",
                os.path.join(FX, "folds")] + flags
        runs[name] = (exp, argv, ev.evaluate_pretrained(argv))
    exp, argv, (tracker, roi) = runs["ms"]
    plain = runs["plain"][0]
    out = exp / f"eval_test_{DS}"
    assert pickle.load(open(out / "tracker.pkl", "rb")) == tracker and pickle.load(open(out / "roi_tracker.pkl", "rb")) == roi
    # what the sweep gives on the same tensors
    _, args = ev.load_args(argv)
    args.outd = args.outd_backup = str(exp)
    args.is_train, args.is_master = False, True
    args.netG['checkpoint_path_netG'] = os.path.join(str(exp), 'best-models/G-model.pth')
    model = define_model(args)
    model.load()
    model.netG.eval()
    base = Interpolate(task=args.task, scale=args.scale, scale_mode=args.basic_interpolation)
    want = {DS: {}, f"{DS}_bicubic": {}}
    ths = tuple(int(t) for t in args.eval_over_roi_also_ths)
    for batch in get_all_eval_loaders(args, args.test_dsets, n=-1)[DS]:
        model = _forward_with_padding(batch, model, args)
        base.feed_data(batch)
        base.test()
        for row, m in ((DS, model), (f"{DS}_bicubic", base)):
            vis = m.current_visuals()
            sw = metrics.sweep(vis['E'], vis['H'], border=args.scale, thresholds=ths, msssim=4)
            for i, img in enumerate(batch['h_id']):
                want[row][img] = sw["msssim"][i].item()
    for row in (DS, f"{DS}_bicubic"):
        det = yaml.safe_load(open(exp / "best-models" / f"details_{row}.yml"))
        det0 = yaml.safe_load(open(plain / "best-models" / f"details_{row}.yml"))
        assert list(det) == ["t/h_0.tif", "t/h_1.tif", "t/h_2.tif"]
        for img in det:
            assert set(det[img]) == set(MTRS) | {"msssim"} and set(det0[img]) == set(MTRS)
            assert det[img]["msssim"] == want[row][img] and 0.0 < det[img]["msssim"] < 1.0
            assert all(det[img][m] == det0[img][m] for m in MTRS)
        assert (yaml.safe_load(open(exp / "best-models" / f"roi_details_{row}.yml"))
                == yaml.safe_load(open(plain / "best-models" / f"roi_details_{row}.yml")))
        node, node0 = tracker["test"][row], runs["plain"][2][0]["test"][row]
        assert list(node) == constants.METRICS + ["msssim"] and list(node0) == constants.METRICS
        mean = sum(det[img]["msssim"] for img in det) / 3.0
        assert len(node["msssim"]["vals"]) == 1 and abs(node["msssim"]["vals"][0] - mean) <= 1e-15
        assert all(node[m] == node0[m] for m in constants.METRICS)
        assert list(roi["test"][row]) == constants.METRICS and roi["test"][row] == runs["plain"][2][1]["test"][row]
        summary = yaml.safe_load(open(exp / "best-models" / f"{row}.yaml"))
        assert summary["last_msssim"] == node["msssim"]["vals"][0] and summary["best_msssim"] == node["msssim"]["best_val"]
        assert not any("msssim" in k for k in yaml.safe_load(open(exp / "best-models" / f"roi-{row}.yaml")))
    assert "msssim: " in open(out / "log.txt").read() and "msssim" not in open(plain / f"eval_test_{DS}" / "log.txt").read()
    # five scales (the default): the set's images are too small, and the first sweep says so
    from dlib.utils.utils_trainer import fast_eval
    from dlib.utils.utils_tracker import init_tracker
    args.msssim_scales = None
    with pytest.raises(ValueError, match=r"--msssim True.*t/h_0\.tif.*at least 177"):
        fast_eval(base, get_all_eval_loaders(args, args.test_dsets, n=-1)[DS], f"{DS}_bicubic", constants.TESTSET, init_tracker(args),
                  init_tracker(args, roi=True), args, -1, -1, nbr_to_plot=0)
