"""Multi-scale SSIM without a GPU: the statement of tests/msssim_ref.py itself, the host side of the entry points (size rule,
workspace size, the refusals, which return before any launch), the --msssim / --msssim_scales options of main.py and eval.py, and
the tracker keys."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import deep_metric_cases as D
import msssim_ref as R
from dlib.utils.constants import MSSSIM_MTR          # (the parent of this feature has none of it)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sr-caco-2_amd")
FX = os.path.join(ROOT, "tests", "golden", "eval_exp")


def close12(x, y):
    return bool(((x - y).abs() <= 1e-12 * y.abs().clamp(min=1.0)).all())


# ------------------------------------------------------------------ the statement
@pytest.mark.parametrize("L", (255, 4095, 65535))
@pytest.mark.parametrize("border", (0, 3))
def test_one_scale_is_the_single_scale_ssim(border, L):
    """M = 1: MS-SSIM = max(mean(ss), 0)^1, the float64 SSIM of deep_metric_cases.ssim_lv without a threshold"""
    _, _, a, b = R.inputs(3, 21, 24, border, L)
    got, want = R.msssim(a, b, L, border, 1), D.ssim_lv(a, b, L, border)
    assert got.shape == (3, 2) and close12(got[:, 1], want)
    assert close12(got[:, 0], want.clamp(min=0.0))
    assert want[2] < 0 and got[2, 0] == 0.0                  # image 2 is 1 - H


@pytest.mark.parametrize("B,h,w,border,M,L", R.CASES)
def test_identical_images_give_one_and_inverted_ones_zero(B, h, w, border, M, L):
    """image 0 is its target: every v_j and the product are 1 within 1e-12.  Image 2 (B = 3) is 1 - H on a smooth H: cs is
    negative wherever the local variance is above C2 / 2, the mean of at least the first scale is below 0, and the product is
    exactly 0.0 (0^w = 0), not a NaN of a negative base.  The constant pair: variances 0, cs = 1 at scale 1."""
    ref64, ref32 = R.expect(B, h, w, border, M, L)
    assert ref64.dtype == torch.float64 and ref32.dtype == torch.float32 and ref64.shape == (B, 1 + M)
    assert (ref64[0] - 1.0).abs().max().item() <= 1e-12
    assert 0.0 < ref64[1, 0].item() < 1.0
    if B == 3:
        assert ref64[2, 0].item() == 0.0 and ref64[2, 1].item() < 0 and ref32[2, 0].item() == 0.0
    a, b = R.constant_pair(h, w, border, L)
    c = R.msssim(a, b, L, border, M)
    assert (c[0] - 1.0).abs().max().item() <= 1e-12
    if M > 1:                   # scale 1: cs = C2 / C2 up to the window's float32 sum; below it the zeros in front are an edge
        assert abs(c[1, 1].item() - 1.0) <= 1e-4
    assert 0.9 < c[1, 0].item() < 1.0                                          # the luminance term of 0.75 against 0.5


def test_weights():
    assert R.weights(5) == R.WEIGHTS == (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)       # as published: they sum to 1.0001
    for M in (1, 2, 3, 4):
        w = R.weights(M)
        assert len(w) == M and abs(sum(w) - 1.0) < 1e-15 and abs(w[0] / w[-1] - R.WEIGHTS[0] / R.WEIGHTS[M - 1]) < 1e-12
    from srhip import ops
    assert all(ops.msssim_weights(M) == R.weights(M) for M in range(1, 6))
    for bad in (0, 6, True, 2.5):
        with pytest.raises(ValueError, match="1 .. 5"):
            ops.msssim_weights(bad)


def test_the_zero_goes_in_front():
    """a 1 x 5 row pools to [x0 / 2, (x1 + x2) / 2, (x3 + x4) / 2] along its odd axis, and the single row is halved once more
    by the zero row in front of it; the same for a column; an even extent gets no zero; a 5 x 4 image written out by hand"""
    x = torch.tensor([1.0, 2.0, 4.0, 8.0, 16.0], dtype=torch.float64)
    axis = torch.stack([x[0] / 2, (x[1] + x[2]) / 2, (x[3] + x[4]) / 2])
    assert torch.equal(R.pool(x.view(1, 1, 1, 5)), (axis / 2).view(1, 1, 1, 3))
    assert torch.equal(R.pool(x.view(1, 1, 5, 1)), (axis / 2).view(1, 1, 3, 1))
    assert torch.equal(R.pool(x[:4].view(1, 1, 1, 4)), (torch.stack([x[0] + x[1], x[2] + x[3]]) / 4).view(1, 1, 1, 2))
    img = torch.arange(1.0, 21.0, dtype=torch.float64).view(1, 1, 5, 4)
    front = F.pad(img, (0, 0, 1, 0))                                    # one zero row in front, none behind: 6 x 4
    want = front.view(1, 1, 3, 2, 2, 2).sum((3, 5)) / 4.0
    assert torch.equal(R.pool(img), want) and R.pool(img).shape == (1, 1, 3, 2)
    assert R.pool(torch.zeros(1, 1, 161, 163)).shape == (1, 1, 81, 82)


# ------------------------------------------------------------------ the size rule, on the host
def test_size_rule_at_160_and_161():
    from srhip import ops
    assert [R.min_side(M) for M in range(1, 6)] == [11, 21, 41, 81, 161] and R.min_side(5, 8) == 177
    assert all(ops.msssim_min_side(M, b) == R.min_side(M, b) for M in range(1, 6) for b in (0, 8))
    _, _, a, b = R.inputs(2, 161, 161, 0, 255)
    assert R.msssim(a, b, 255, 0, 5).shape == (2, 6)
    for crop in ((slice(0, 160), slice(0, 161)), (slice(0, 161), slice(0, 160))):
        with pytest.raises(ValueError, match="161"):
            R.msssim(a[:, :, crop[0], crop[1]], b[:, :, crop[0], crop[1]], 255, 0, 5)
    assert R.msssim(a[:, :, :160, :160], b[:, :, :160, :160], 255, 0, 4).shape == (2, 5)
    ws = ops.lib.srhip_metrics_msssim_lv_ws
    assert ws(1, 160, 161, 0, 5) == 0 and ws(1, 161, 160, 0, 5) == 0 and ws(1, 176, 177, 8, 5) == 0
    assert ws(1, 161, 161, 0, 0) == 0 and ws(1, 161, 161, 0, 6) == 0 and ws(0, 161, 161, 0, 5) == 0
    # 161 -> 81 -> 41 -> 21 -> 11: tiles of 32 x 16 map pixels, two sums a tile; then the four uint32 pairs, counted in doubles
    tiles = 5 * 10 + 3 * 5 + 1 * 2 + 1 * 1 + 1 * 1
    assert ws(1, 161, 161, 0, 5) == ws(1, 177, 177, 8, 5) == 2 * tiles + (81 ** 2 + 41 ** 2 + 21 ** 2 + 11 ** 2)
    assert ws(3, 11, 11, 0, 1) == 2 * 3


def test_the_entry_point_refuses_by_number_before_any_launch():
    """the argument checks of srhip_metrics_msssim_lv come before its first use of a pointer or of the device"""
    from srhip import ops

    def call(H, W, border, L, M, ws_doubles=1 << 20):
        ops.call("srhip_metrics_msssim_lv", None, None, 1, H, W, border, L, 0, M, None, None, ws_doubles, None, None)
    for args, text in (((160, 161, 0, 255, 5), "161"), ((161, 160, 0, 255, 5), "161"), ((176, 177, 8, 255, 5), "161"),
                       ((40, 41, 0, 255, 3), "41"), ((161, 161, 0, 255, 0), "got 0"), ((161, 161, 0, 255, 6), "got 6"),
                       ((161, 161, 0, 254, 5), "254"), ((161, 161, 0, 65536, 5), "65536")):
        with pytest.raises(ops.SrhipError, match=text):
            call(*args)


# ------------------------------------------------------------------ the command line
def _main(*flags):
    import main
    return main.parse_input(["--net_type", "swinir", "--method", "SWINIR", *flags])


def test_main_cli_accepts():
    for flags in ((), ("--msssim", "False")):
        a = _main(*flags)
        assert "msssim_scales" not in a and not a.msssim and ("msssim" in a) == bool(flags)
    a = _main("--msssim", "True")
    assert a.msssim is True and "msssim_scales" not in a
    a = _main("--msssim", "True", "--msssim_scales", "3", "--model_select_mtr", MSSSIM_MTR)
    assert a.msssim is True and a.msssim_scales == 3 and a.model_select_mtr == "msssim"
    a = _main("--msssim", "True", "--model_select_mtr", MSSSIM_MTR, "--eval_over_roi_also", "True")
    assert a.eval_over_roi_also and not a.eval_over_roi_also_model_select
    from dlib.utils.own_options import check_msssim
    assert check_msssim(_main()) == 0 and check_msssim(_main("--msssim", "True")) == 5
    assert check_msssim(_main("--msssim", "True", "--msssim_scales", "1")) == 1


REFUSED = ((("--msssim_scales", "3"), "--msssim_scales"),
           (("--msssim", "False", "--msssim_scales", "3"), "--msssim_scales"),
           (("--msssim", "True", "--msssim_scales", "0"), "--msssim_scales"),
           (("--msssim", "True", "--msssim_scales", "6"), "--msssim_scales"),
           (("--model_select_mtr", "msssim"), "--model_select_mtr msssim"),
           (("--msssim", "True", "--model_select_mtr", "msssim", "--eval_over_roi_also", "True",
             "--eval_over_roi_also_model_select", "True"), "--model_select_mtr msssim"))


@pytest.mark.parametrize("flags,named", REFUSED)
def test_main_cli_refuses_by_name(flags, named, capsys):
    with pytest.raises(SystemExit) as e:
        _main(*flags)
    assert e.value.code == 2 and named in capsys.readouterr().err


def _eval_args(*flags):
    import importlib.util
    spec = importlib.util.spec_from_file_location("srhip_eval_cli", os.path.join(PKG, "eval.py"))
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)
    return ev.load_args(["--exp_path", os.path.join(FX, "exp"), "--data_root", os.path.join(FX, "data"), *flags])[1]


def test_eval_cli(capsys):
    a = _eval_args()
    assert "msssim" not in a and "msssim_scales" not in a
    a = _eval_args("--msssim", "True", "--msssim_scales", "4")
    assert a.msssim is True and a.msssim_scales == 4
    for flags, named in ((("--msssim_scales", "4"), "--msssim_scales"), (("--msssim", "True", "--msssim_scales", "7"), "--msssim_scales")):
        with pytest.raises(SystemExit) as e:
            _eval_args(*flags)
        assert e.value.code == 2 and named in capsys.readouterr().err


def test_the_exit_code_of_the_program():
    """main.py as a program: exit code 2 and the flag in stderr, before any use of the device"""
    r = subprocess.run([sys.executable, os.path.join(PKG, "main.py"), "--net_type", "swinir", "--method", "SWINIR", "--msssim_scales", "3"],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "--msssim_scales 3 needs --msssim True" in r.stderr


def test_a_folder_recorded_at_another_value_is_not_resumed(tmp_path):
    import yaml
    import main
    for recorded, flags, old, want in (({}, ("--msssim", "True"), 0, 5), ({"msssim": True}, (), 5, 0),
                                       ({"msssim": True, "msssim_scales": 3}, ("--msssim", "True"), 3, 5)):
        a = _main("--outd", str(tmp_path), *flags)
        a.outd_backup = a.outd
        with open(tmp_path / "config_model.yml", "w") as f:
            yaml.dump({"net_type": "swinir", "scale": a.scale, **recorded}, f)
        with pytest.raises(SystemExit, match=f"msssim_scales = {old} .*asks for {want}"):
            main._resume_point(a)
    a = _main("--outd", str(tmp_path), "--msssim", "True", "--msssim_scales", "3")
    a.outd_backup = a.outd
    assert main._resume_point(a) == 0                   # the same value: the folder is this run's


# ------------------------------------------------------------------ constants and trackers
def test_metrics_and_tracker_keys():
    from dlib.utils import constants, utils_tracker as T
    from dlib.utils.tools import Dict2Obj
    assert constants.METRICS == ["psnr", "ssim", "mse", "nrmse", "psnr_y", "ssim_y"] and MSSSIM_MTR == "msssim"
    assert set(constants.BEST_MTR) == set(constants.METRICS)
    assert constants.EXTRA_METRICS == ["msssim"] and constants.EXTRA_BEST_MTR == {"msssim": max}
    base = dict(valid_dsets="v", test_dsets="t", basic_interpolation="bicubic", model_select_mtr="psnr")
    plain, on = Dict2Obj(base), Dict2Obj(dict(base, msssim=True, model_select_mtr="msssim"))
    for a in (plain, Dict2Obj(dict(base, msssim=False))):
        for tr in (T.init_tracker(a), T.init_tracker(a, roi=True)):
            assert all(list(node) == constants.METRICS for split in ("val", "test") for node in tr[split].values())
    tr, roi = T.init_tracker(on), T.init_tracker(on, roi=True)
    assert all(list(node) == constants.METRICS + ["msssim"] for split in ("val", "test") for node in tr[split].values())
    assert all(list(node) == constants.METRICS for split in ("val", "test") for node in roi[split].values())
    # higher is better, the others follow its best evaluation; a reset test row keeps the key
    from dlib.utils.utils_trainer import _fast_update_tracker
    for ms, mse in ((0.5, 3.0), (0.75, 4.0), (0.625, 1.0)):
        tr, best = _fast_update_tracker(on, tr, {"msssim": ms, "mse": mse}, "val", "v")
        roi, _ = _fast_update_tracker(on, roi, {"mse": 2 * mse}, "val", "v", best)
    assert tr["val"]["v"]["msssim"] == {"vals": [0.5, 0.75, 0.625], "best_val": 0.75} and best == 1
    assert tr["val"]["v"]["mse"]["best_val"] == 4.0 and roi["val"]["v"]["mse"]["best_val"] == 8.0 and "msssim" not in roi["val"]["v"]
    assert not T.is_last_perf_best_perf(tr, roi, True, False, "val", "v", "msssim")
    T.reset_tracker_eval(T.update_tracker_eval(tr, "test", "t", "msssim", 0.5)[0], "test", "t")
    assert tr["test"]["t"]["msssim"] == {"vals": [], "best_val": 0.0}
    T.reset_tracker_eval(roi, "test", "t")
    assert list(roi["test"]["t"]) == constants.METRICS
    status = T.write_current_perf_eval(tr, "val", "v", None, None, 7, 1)
    roi_status = T.write_current_perf_eval(roi, "val", "v", None, None, 7, 1)
    assert status["last_msssim"] == 0.625 and status["best_msssim"] == 0.75 and "last_msssim" not in roi_status
    msg = T.current_perf_to_str(status, roi_status, "msssim", False)
    assert "msssim: 0.750000 [BEST] | 0.6250 [LAST] ---> MASTER" in msg and "mse: 4.000000* (ROI: 8.000000)" in msg
