"""The full-depth metrics without a GPU: the float64 statements of tests/deep_metric_cases.py against the oracle at L = 255, the
round trips of Q_L, the arithmetic of the SSIM kernel on the bright-smooth case, and --metric_levels in main.py / eval.py."""
import numpy as np
import pytest
import torch
import yaml

import sr_oracle as O
import step_kernel_cases as C
import deep_metric_cases as M


# ---------------------------------------------------------------- the statements at L = 255 are the oracle's metrics
@pytest.mark.parametrize("H,W,border", C.METRIC_PSNR_SHAPES)
def test_the_psnr_family_at_255_is_the_oracle_s(H, W, border):
    _, _, a, b = C.metric_psnr_inputs(H, W, border)
    ya, yb = O.gray_to_y(a / 255.0) * 255.0, O.gray_to_y(b / 255.0) * 255.0
    for th in (None,) + C.METRIC_PSNR_THS:
        roi = None if th is None else C.roi_of(b, th, torch.float32)
        assert torch.equal(M.mse_lv(a, b, 255, border, th), O.metric_mse(a, b, border, roi)), th
        assert torch.equal(M.psnr_lv(a, b, 255, border, th), O.metric_psnr(a, b, border, roi)), th
        assert torch.equal(M.nrmse_lv(a, b, 255, border, th), O.metric_nrmse(a, b, border, roi)), th
        e = (M.psnr_y_lv(a, b, 255, border, th) - O.metric_psnr(ya, yb, border, roi)).abs().max().item()
        assert e < 1e-4, (th, e)


@pytest.mark.parametrize("border", C.METRIC_SSIM_BORDERS)
@pytest.mark.parametrize("h,w", C.METRIC_SSIM_SIZES)
def test_ssim_at_255_is_the_oracle_s_in_float64(h, w, border):
    _, _, a, b = C.metric_ssim_inputs(h, w, border)
    for th in (None,) + C.METRIC_SSIM_THS:
        roi = None if th is None else C.roi_of(b, th, torch.float64)
        e = (M.ssim_lv(a, b, 255, border, th) - O.metric_ssim(a.double(), b.double(), border, roi)).abs().max().item()
        assert e <= 1e-12, (th, e)


def test_the_level_inputs_survive_the_rescaling():
    """the 8-bit cases of the psnr inputs at L: image 1 is pred == target, image 2 is constant with its 8-bit level at 64"""
    for L in M.LEVELS:
        for H, W, border in C.METRIC_PSNR_SHAPES:
            pr, hf, a, b = M.psnr_inputs(H, W, border, L)
            assert torch.equal(a[1], b[1]) and torch.equal(M.t_q(hf, L), b) and torch.equal(M.t_q(pr, L), a)
            assert bool((M.t_level8(b[2], L) == 64).all()) and b[2].unique().numel() == 1
            assert bool((pr < 0).any()) and bool((pr > 1).any())
            assert torch.equal(M.t_q(hf, 255), M.t_level8(b, L))          # the float form and the levels form: one ROI


# ---------------------------------------------------------------- Q_L
@pytest.mark.parametrize("L", M.ROUND_TRIP_LEVELS)
def test_q_levels_round_trip(L):
    v = np.arange(L + 1)
    assert np.array_equal(M.q_levels(M.unit(v, L), L), v)


def test_q_levels_between_the_depths():
    v = np.arange(256)
    assert np.array_equal(M.q_levels(np.float32(v / 255.), 65535), 257 * v)
    for L in (4095, 65535):
        v = np.arange(L + 1)
        exact = (2 * v * 255 + L) // (2 * L)              # round(v 255 / L); an odd L has no tie
        assert L % 2 == 1 and np.array_equal(M.level8(v, L), exact)


def test_the_tie_inputs_are_ties():
    for L in (255,) + M.LEVELS:
        x, nties = M.levels_inputs(L)
        assert x.numel() == M.LEVELS_N and nties >= 200
        p = x.numpy() * np.float32(L)
        assert bool((p[7:7 + nties] % 1 == 0.5).all())
        assert bool((x < 0).any()) and bool((x > 1).any()) and bool(torch.isfinite(x).all())
    assert torch.equal(M.t_q(M.levels_inputs(255)[0], 255), O.tensor2uint82float(M.levels_inputs(255)[0]))


# ---------------------------------------------------------------- the SSIM kernel's arithmetic, before any GPU run
@pytest.mark.parametrize("L", M.LEVELS)
@pytest.mark.parametrize("border", C.METRIC_SSIM_BORDERS)
@pytest.mark.parametrize("h,w", C.METRIC_SSIM_SIZES)
def test_the_ssim_kernel_s_arithmetic_meets_the_gate_and_plain_float32_does_not(h, w, border, L):
    """k_ssim_metric_lv is float64 throughout; what it does NOT share with the statement is the window (the separable float32
    taps of the 8-bit kernel against the reference's float32 2-D window).  Its arithmetic, stated in numpy
    (deep_metric_cases.ssim_map_as_kernel), meets the suite's gate -- min(5e-5, 3 x the float32 statement's distance), scale 1,
    the [B, 9] buffer as one comparison -- on the step images and the bright-smooth one.  The plain float32 statement is printed
    beside it; on the 11 x 11 case, one output pixel of the bright-smooth image, it is above the ceiling: the case has teeth."""
    _, _, a, b = M.ssim_inputs(h, w, border, L)
    ref64, ref32 = M.ssim_expect(h, w, border, L)
    got = torch.stack([M.ssim_as_kernel(a, b, L, border, th) for th in (None,) + C.METRIC_SSIM_THS], 1)
    e = (got - ref64).abs().max().item()
    e32 = max((ref32.double() - ref64).abs().max().item(), C.F32_ROUNDING)
    e32_bright = (ref32[3].double() - ref64[3]).abs().max().item()
    pix = (M.ssim_map(a[3:], b[3:], L, border, torch.float32).double() - M.ssim_map(a[3:], b[3:], L, border)).abs().max().item()
    print(f"[ssim_lv arithmetic] {h}x{w} border={border} L={L}: as the kernel {e:.3e}; float32 statement {e32:.3e} "
          f"(bright-smooth image {e32_bright:.3e}, its worst map pixel {pix:.3e})")
    assert e <= min(C.METRIC_SSIM, 3 * e32), (e, e32)
    assert torch.equal(got[:, 1 + C.METRIC_SSIM_THS.index(300)], torch.zeros(4, dtype=torch.float64))
    if (h, w) == (11, 11):
        assert e32_bright > C.METRIC_SSIM, e32_bright


# ---------------------------------------------------------------- --metric_levels
def _stub_exp(tmp_path, name, **top):
    d = tmp_path / name
    d.mkdir()
    cfg = dict({"scale": 2, "method": "SWINIR", "net_type": "swinir", "myseed": 0, "amp": False, "splits_root": "folds",
                "test_dsets": "biosrx-test-X-2", "netG": {"net_type": "swinir"}}, **top)
    (d / "config_model.yml").write_text(yaml.safe_dump(cfg))
    return str(d)


def test_metric_levels_reaches_main_and_eval(tmp_path, capsys):
    import main as Mn
    import eval as E
    base = "--net_type swinir --method SWINIR --scale 2".split()
    a = Mn.parse_input(base + ["--metric_levels", "4095"])
    assert a.metric_levels == 4095 and dict(a)["metric_levels"] == 4095
    assert "metric_levels" not in Mn.parse_input(base)            # absent unless given: such a run is today's run
    for bad in ("100", "70000"):
        with pytest.raises(SystemExit) as ei:
            Mn.parse_input(base + ["--metric_levels", bad])
        err = capsys.readouterr().err
        assert ei.value.code == 2 and "--metric_levels" in err and "255 .. 65535" in err
    plain, rec = _stub_exp(tmp_path, "plain"), _stub_exp(tmp_path, "rec", metric_levels=4095)
    argv = ["--data_root", str(tmp_path)]
    assert "metric_levels" not in E.load_args(["--exp_path", plain] + argv)[1]
    assert E.load_args(["--exp_path", rec] + argv)[1].metric_levels == 4095              # read back from the folder
    assert E.load_args(["--exp_path", rec, "--metric_levels", "65535"] + argv)[1].metric_levels == 65535
    for bad in ("100", "70000"):
        with pytest.raises(SystemExit) as ei:
            E.load_args(["--exp_path", rec, "--metric_levels", bad] + argv)
        err = capsys.readouterr().err
        assert ei.value.code == 2 and "--metric_levels" in err and "255 .. 65535" in err


def test_a_run_does_not_resume_a_folder_with_other_metric_levels(tmp_path):
    import main as Mn
    base = "--net_type swinir --method SWINIR --scale 2".split()

    def resume(folder, extra=()):
        args = Mn.parse_input(base + ["--outd", folder] + list(extra))
        args.outd_backup = args.outd
        return Mn._resume_point(args)
    rec, plain = _stub_exp(tmp_path, "rec", metric_levels=4095), _stub_exp(tmp_path, "plain")
    assert resume(rec, ["--metric_levels", "4095"]) == 0 and resume(plain) == 0
    for folder, extra, old, new in ((rec, ["--metric_levels", "65535"], "4095", "65535"), (rec, [], "4095", "255"),
                                    (plain, ["--metric_levels", "4095"], "255", "4095")):
        with pytest.raises(SystemExit) as ei:
            resume(folder, extra)
        msg = str(ei.value)
        assert "metric_levels" in msg and old in msg and new in msg, msg


def test_check_metric_levels():
    from dlib.utils.own_options import check_metric_levels
    assert check_metric_levels(None) == 255 and check_metric_levels(255) == 255 and check_metric_levels(65535) == 65535
    for bad in (254, 65536, 4095.5, True):
        with pytest.raises(ValueError, match="255 .. 65535"):
            check_metric_levels(bad)
