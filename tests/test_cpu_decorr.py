"""Image decorrelation analysis without a GPU: the condition the images of tests/decorr_cases.py must satisfy (none is marked),
the statement's own rounding e_ref (64 e_ref is the gate of tests/test_gpu_decorr.py), the peak rule and the one-pass form of it
that the kernel uses, what the figure means on images of known blur, the header's two prototypes, and the host side of
predict.py --resolution True: records, resolution.yml, the log line, the refusals.

e_ref measured here: 5.2e-16 (np.fft.fft2 against a direct DFT with np.longdouble sums over the five cases with S <= 128, all 21
curves).  The smallest decision margin of a case: 5.9e-8 among the cases up to 8x512x512; test_case_conditions prints each."""
import importlib.util
import os

import numpy as np
import pytest
import yaml

import decorr_cases as K
import decorr_ref as D
import frc_cases as F
import frc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sr-caco-2_amd")
EXP = os.path.join(ROOT, "tests", "golden", "eval_exp", "exp")


# ------------------------------------------------------------------ the cases and the bound
@pytest.mark.parametrize("name", list(K.CASES))
def test_case_conditions(name):
    """NO image is marked: every decision of steps 7 - 8 on every one of its 21 curves (each argmax against the runner-up of the
    searched segment, each test against 5e-4) was taken by at least 1e-10; every image has a resolution"""
    B, h, w, N, lv, _ = K.CASES[name]
    X, each = K.images(name), K.expect(name)
    S = R.side(h, w)
    assert X.shape == (B, 1, h, w) and X.dtype == np.float32 and len(each) == B
    for i, o in enumerate(each):
        print(f"[case] {name}[{i}] S={o['side']} ring={o['ring']} cut={o['cut']:.6f} amp={o['amp']:.4f} sigma={o['sigma']:.4f} "
              f"best={o['best']} peaks={o['peaks'].tolist()} margin={o['margin']:.2e}")
        assert o["side"] == S and o["curves"].shape == (D.NCURVE, S // 2 + 1) and o["curves"].dtype == np.float64
        assert not o["marked"] and o["margin"] >= D.MARK
        assert 2 < o["ring"] <= S // 2 and 0.0 < o["cut"] <= 1.0 and 0.0 < o["amp"] <= 1.0
        assert np.isfinite(o["curves"]).all() and o["curves"].min() >= 0.0 and (o["curves"][:, :2] == 0).all()
        assert o["ring"] == o["peaks"].max() and o["best"] == int(np.argmax(o["peaks"])) and o["sigma"] == o["sigmas"][o["best"]]
        assert int(o["n"].sum()) == int((R.ring_index(S) >= 0).sum()) and o["n"][1] == 8
    if lv:
        assert X.max() > 255 and np.array_equal(X, np.rint(X))         # levels 0 .. N


def test_levels_case_is_the_float_case():
    a, b = K.expect("128x128_65535")[0], K.expect("128x128_65535_levels")[0]
    assert np.array_equal(a["curves"], b["curves"]) and np.array_equal(a["peaks"], b["peaks"]) and a["sigma"] == b["sigma"]


def test_e_ref():
    """the statement's own rounding over all 21 curves, the unit of the GPU gate; a few 1e-16 .. 1e-14 by the precision of float64"""
    e = K.e_ref()
    print(f"[e_ref] {e:.3e}   gate 64 e_ref = {K.bound():.3e}")
    assert 1e-17 < e < 1e-12


# ------------------------------------------------------------------ the peak rule
def one_pass_peak(d):
    """the kernel's form of step 7 (decorr.hip): the records of the running maximum from the top down; record i is the argmax for
    m in [i, j - 1], j the next record, and the 5e-4 test holds somewhere in that range iff it holds at m = j - 1"""
    m = len(d) - 1
    rec = [r for r in range(2, m + 1) if r == 2 or d[r] > d[2:r].max()]
    for k in range(len(rec) - 1, -1, -1):
        i, top = rec[k], (rec[k + 1] - 1 if k + 1 < len(rec) else m)
        if i == 2:
            return 0, 0.0
        if top > i and d[i] - d[i:top + 1].min() >= D.PEAK_DROP:
            return i, float(d[i])
    return 0, 0.0


def test_peak_rule():
    z = [0.0, 0.0]
    assert D.peak(np.array(z + [0.1, 0.2, 0.3, 0.2, 0.1]))[:2] == (4, 0.3)
    assert D.peak(np.array(z + [0.1, 0.2, 0.3, 0.4, 0.5]))[:2] == (0, 0.0)                  # rising to the end: i == m all the way
    assert D.peak(np.array(z + [0.5, 0.4, 0.3, 0.2, 0.1]))[:2] == (0, 0.0)                  # falling from ring 2
    assert D.peak(np.array(z + [0.1, 0.3, 0.2999, 0.2998, 0.4]))[:2] == (0, 0.0)            # a dip under 5e-4 is no peak
    assert D.peak(np.array(z + [0.1, 0.3, 0.2994, 0.35, 0.4]))[:2] == (3, 0.3)              # 6e-4 is one
    assert D.peak(np.array(z + [0.1, 0.3, 0.3, 0.2, 0.4]))[:2] == (3, 0.3)                  # the FIRST argmax
    assert D.peak(np.array(z + [0.1, 0.3, 0.1, 0.5, 0.2]))[:2] == (5, 0.5)                  # the highest peak that has a drop
    assert D.peak(np.zeros(17))[:2] == (0, 0.0)
    assert D.peak(np.array(z + [0.1, 0.3, 0.2995 - 1e-12, 0.4]))[2] < D.MARK               # the 5e-4 test by a hair: marked
    assert D.peak(np.array(z + [0.1, 0.3, 0.3 - 1e-12, 0.2, 0.4]))[2] < D.MARK             # the argmax by a hair: marked
    assert D.peak(np.array(z + [0.1, 0.3, 0.2, 0.1, 0.05]))[2] >= 5e-4 - 1e-15


def test_the_one_pass_search_is_the_rule():
    """random curves of every character: smooth with a few maxima, plateaus of equal values, steps of about 5e-4, white noise"""
    rng = np.random.default_rng(3)
    n_found = 0
    for k in range(400):
        m = int(rng.integers(3, 90))
        kind = k % 4
        if kind == 0:
            d = np.cumsum(rng.standard_normal(m)) * 1e-3
        elif kind == 1:
            d = np.round(rng.random(m), 1)
        elif kind == 2:
            d = 0.5 + np.cumsum(rng.choice([-5e-4, 5e-4, -2.5e-4, 2.5e-4, 1e-3], m))
        else:
            d = rng.random(m)
        d = np.concatenate([[0.0, 0.0], d - d.min()])
        assert one_pass_peak(d) == D.peak(d)[:2], (k, d.tolist())
        n_found += D.peak(d)[0] > 0
    assert 100 < n_found < 400


# ------------------------------------------------------------------ what the figure means
@pytest.mark.parametrize("sigma", (1.0, 2.0, 4.0))
def test_psf_width_is_found(sigma):
    """emitters under a Gaussian PSF of width sigma with shot noise at 128 x 128: 2 / cut within a factor 1.5 of the PSF's full
    width at half maximum, 2.355 sigma"""
    for seed in (1, 2):
        o = D.decorr_one(K.dots(128, 128, seed, sigma=sigma).astype(np.float32))
        res = 2.0 / o["cut"]
        print(f"[psf] sigma {sigma} seed {seed}: ring {o['ring']} res_px {res:.2f} (FWHM {2.355 * sigma:.2f}) amp {o['amp']:.3f}")
        assert 2.355 * sigma / 1.5 <= res <= 2.355 * sigma * 1.5


@pytest.mark.parametrize("name", list(F.CASES)[:list(F.CASES).index("512x512") + 1])
def test_the_sharp_image_has_the_larger_cut(name):
    """the pairs of the Fourier ring correlation tests, from 32x32 to 512x512 in the order of their table: the target H against
    E = blurred H + noise.  This is an observation about these images, not a theorem: where the white texture of a target carries
    every high-passed curve up to Nyquist without a maximum, only the bump of its smooth field is found.  Of the eight pairs of
    the evaluation batch that follows in the table (8x512x512), seven go the same way and the last does not: cut(H) 0.1406
    against cut(E) 0.5898."""
    _, _, _, N, lv, _ = F.CASES[name]
    E, H = F.images(name)
    for e, h in zip(E[:, 0], H[:, 0]):
        ce, ch = D.decorr_one(e, N, lv)["cut"], D.decorr_one(h, N, lv)["cut"]
        print(f"[pair] {name}: cut(H) {ch:.4f} cut(E) {ce:.4f}")
        assert ch > ce > 0.0


def test_a_constant_image():
    """an empty image: every spectrum value is 0, every denominator too, every curve is 0 and nothing is found, without a NaN.
    A grey image: the window's spectrum is exactly the rings 0 and 1, which the sums leave out, so what they see is the rounding
    of the transform, 1e-16 of the pedestal; the curves are finite, and what a normalised curve of rounding noise reports is
    not pinned (the statement finds nothing for 0.3 and ring 6 of 32 for 1.0 at 64 x 64)"""
    o = D.decorr_one(np.zeros((64, 64), np.float32))
    assert o["cut"] == 0.0 and o["ring"] == 0 and o["amp"] == 0.0 and o["sigma"] == 0.0 and o["best"] == 0
    assert (o["curves"] == 0).all() and (o["peaks"] == 0).all()
    for c in (0.3, 128 / 255, 1.0):
        o = D.decorr_one(np.full((64, 64), c, np.float32))
        assert np.isfinite(o["curves"]).all() and np.isfinite([o["cut"], o["amp"], o["sigma"]]).all()
        assert o["A"][2:].max() <= 1e-12 * o["A"][0]


def test_banks():
    b = D.bank(64.0, D.SIGMA_MIN)
    assert len(b) == 10 and b[0] == pytest.approx(64.0, rel=1e-15) and b[-1] == pytest.approx(0.15, rel=1e-15)
    assert np.allclose(b[1:] / b[:-1], (0.15 / 64.0) ** (1 / 9), rtol=1e-13)
    g = D.highpass(2.0, 64)
    assert g[0] == 0.0 and np.all(np.diff(g) > 0) and g[-1] < 1.0 and (D.highpass(0, 64) == 1).all()
    assert g[3] == -np.expm1(-2 * np.pi ** 2 * 4.0 * 9 / 64 ** 2)
    # curve 0 is the best of its image: no bank 2, the curves 11 .. 20 are 0 and report ring 0
    o = K.expect("37x45")[0]
    assert o["best"] == 0 and (o["peaks"][11:] == 0).all() and (o["curves"][11:] == 0).all() and (o["sigmas"][11:] == 0).all()
    # bank 2 lies between the neighbours of the best of bank 1
    o = K.expect("32x32")[0]
    j = int(np.argmax(o["peaks"][:11]))
    assert j >= 1 and o["sigmas"][11] == pytest.approx(o["sigmas"][max(j - 1, 1)], rel=1e-15)
    assert o["sigmas"][20] == pytest.approx(o["sigmas"][min(j + 1, 10)], rel=1e-15)


# ------------------------------------------------------------------ the library's host side
def test_header_carries_both_prototypes():
    from srhip import _lib, ops
    protos = _lib.parse_header()
    assert protos["srhip_metrics_decorr_lv_ws"] == ("l", "iii")
    # img, B, H, W, L, inputs_are_levels, workspace, workspace_doubles, out, curves, peaks, stream
    assert protos["srhip_metrics_decorr_lv"] == ("i", "piiiiiplpppp")
    ws = ops.lib.srhip_metrics_decorr_lv_ws
    assert ws(1, 31, 64) == 0 and ws(1, 64, 31) == 0 and ws(0, 64, 64) == 0
    assert ws(1, 32, 32) == ws(2, 32, 32) == 2 * 32 * 32 + 5 * 17 * 17                  # two images share a transform
    assert ws(3, 70, 151) == 2 * (2 * 64 * 64 + 5 * 33 * 33)
    assert ws(8, 2100, 2050) == 4 * (2 * 2048 * 2048 + 5 * 1025 * 1025)
    assert ws(80, 2048, 2048) * 8 > 2 ** 31 and ws(80, 2048, 2048) == 40 * ws(1, 2048, 2048)          # long, not int
    assert ops.DECORR_CURVES == D.NCURVE == 21
    text = open(_lib.HEADER).read()
    for words in ("Descloux", "Hann window instead of a cosine apodisation", "integer rings of the FRC instead of 50 sampled radii",
                  "filters constant on a ring", "no refinement of the", "comparable with another figure from this code"):
        assert words in text, words


def test_the_entry_point_refuses_by_number_before_any_launch():
    """the argument checks of srhip_metrics_decorr_lv come before its first use of a pointer or of the device"""
    from srhip import ops

    def call(H, W, L=255, B=1, ws_doubles=1 << 24):
        ops.call("srhip_metrics_decorr_lv", None, B, H, W, L, 0, None, ws_doubles, None, None, None, None)
    for kw, text in ((dict(H=31, W=64), "at least 32"), (dict(H=64, W=31), "at least 32"), (dict(H=64, W=64, L=254), "254"),
                     (dict(H=64, W=64, L=65536), "65536"), (dict(H=64, W=64, B=0), "empty input"),
                     (dict(H=64, W=64), "null pointer")):
        with pytest.raises(ops.SrhipError, match=text):
            call(**kw)


# ------------------------------------------------------------------ predict.py --resolution True
def _cli():
    spec = importlib.util.spec_from_file_location("srhip_predict_cli_decorr", os.path.join(PKG, "predict.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_resolution_record():
    from srhip.predict import resolution_record
    r = resolution_record(8, {"side": 32, "cut": 0.5, "amp": 0.7}, {"side": 256, "cut": 0.25, "amp": 0.4})
    assert r == {"in": {"side": 32, "cut": 0.5, "res_px": 4.0, "amp": 0.7}, "out": {"side": 256, "cut": 0.25, "res_px": 8.0, "amp": 0.4},
                 "gain": 4.0}                                          # 4 LR pixels are 32 HR pixels; the output resolves 8
    assert list(r) == ["in", "out", "gain"] and list(r["in"]) == ["side", "cut", "res_px", "amp"]
    for a, b in ((0.0, 0.25), (0.5, 0.0), (0.0, 0.0)):
        r = resolution_record(8, {"side": 32, "cut": a, "amp": 0.0}, {"side": 256, "cut": b, "amp": 0.0})
        assert r["gain"] is None and (r["in"]["res_px"] is None) == (a == 0) and (r["out"]["res_px"] is None) == (b == 0)


def test_resolution_file_and_log_line(tmp_path):
    from srhip.predict import resolution_record
    cli = _cli()
    recs = {1: resolution_record(8, {"side": 32, "cut": 0.5, "amp": 0.7}, {"side": 256, "cut": 0.25, "amp": 0.4}),
            0: resolution_record(8, {"side": 32, "cut": 0.25, "amp": 0.6}, {"side": 256, "cut": 0.125, "amp": 0.3}),
            2: resolution_record(8, {"side": 32, "cut": 0.0, "amp": 0.0}, {"side": 256, "cut": 0.5, "amp": 0.2})}
    rows = cli.resolution_rows(recs)
    assert [r["page"] for r in rows] == [0, 1, 2] and list(rows[0]) == ["page", "in", "out", "gain"] and rows[1]["gain"] == 4.0
    assert cli.resolution_means(rows) == (6.0, (16.0 + 8.0 + 4.0) / 3, 4.0)
    line = cli.resolution_line("a.tif", rows)
    assert line.startswith("a.tif: resolution 6.00 px in -> 9.33 px out") and "3 page(s)" in line and line.endswith("gain x4.00")
    none = cli.resolution_rows({0: recs[2] | {"out": recs[2]["in"]}})
    assert cli.resolution_means(none) == (None, None, None)
    assert "resolution none found in -> none found out" in cli.resolution_line("b.png", none) and "gain" not in cli.resolution_line("b.png", none)
    report = {"a.tif": rows, "b.png": none}
    cli.write_resolution(str(tmp_path), report)
    back = yaml.safe_load(open(tmp_path / "resolution.yml"))
    assert back == report and list(back) == ["a.tif", "b.png"] and back["a.tif"][2]["in"]["res_px"] is None and back["a.tif"][2]["gain"] is None


def test_the_option_refuses_by_name_before_the_device(tmp_path):
    from PIL import Image
    from srhip.predict import Predictor, PredictError, check_request, load_config
    args = load_config(EXP)
    assert check_request(args, "uint8", 31, 64) == (255, "uint8") and check_request(args, "uint8", 32, 32, resolution=True) == (255, "uint8")
    for H, W in ((31, 64), (64, 31), (16, 17)):
        with pytest.raises(PredictError, match=rf"--resolution True: a {H} x {W} page is too small.*at least 32"):
            check_request(args, "uint8", H, W, resolution=True)
    assert check_request(args, "uint16", 40, 40, in_max=100) == (100, "uint16")
    with pytest.raises(PredictError, match="--resolution True: in_max 100 is below 255"):
        check_request(args, "uint16", 40, 40, in_max=100, resolution=True)
    assert check_request(args, "uint16", 40, 40, in_max=4095, resolution=True) == (4095, "uint16")
    pred = Predictor(EXP)
    assert pred.last_resolution is None
    with pytest.raises(PredictError, match="--resolution True: a 16 x 17 page is too small"):
        pred.run(np.zeros((2, 16, 17), np.uint8), resolution=True)
    assert pred._model is None                                         # nothing was built or moved to the device
    # the command line: default off; a small page is refused by file and page, and nothing is written
    cli = _cli()
    src = tmp_path / "in"
    src.mkdir()
    Image.fromarray(np.zeros((40, 45), np.uint8)).save(str(src / "a_fine.png"))
    Image.fromarray(np.zeros((31, 45), np.uint8)).save(str(src / "b_small.png"))
    with pytest.raises(PredictError, match=r"b_small\.png, page 0: --resolution True: a 31 x 45 page is too small.*at least 32"):
        cli.predict(["--exp_path", EXP, "--input", str(src), "--output", str(tmp_path / "out"), "--resolution", "True"])
    assert not os.path.exists(tmp_path / "out")
    with pytest.raises(SystemExit):
        cli.predict(["--exp_path", EXP, "--input", str(src), "--resolution", "perhaps"])
    import inspect
    assert inspect.signature(Predictor.run).parameters["resolution"].default is False
