"""--lr_synth psf without a GPU: the numpy statement of the camera model (dlib/datasets/lowres.py: psf_bin_np, photon_noise_np)
against scipy and against the distributions it claims, the parser, config_model.yml and the refusals.

Bounds, from the arithmetic:
  psf_bin_np against scipy.ndimage.gaussian_filter + reshape-mean in float64: 2^-24 for images in [0, 1] -- the statement
      rounds to float32 once per pass, each rounding at most 2^-25 on a value in [0, 1], and the second pass is a convex
      combination (the weights are positive and sum to 1) that does not amplify the first one's; the float64 sums differ from
      scipy's by their order only, some 1e-15;
  the sampler: mean within 5 standard errors sqrt(lambda / N) of lambda, variance within 5 of its standard error
      sqrt((mu4 - var^2) / N) with Poisson's mu4 = lambda + 3 lambda^2; the read noise likewise with the normal's mu4 = 3 var^2."""
import math
import os

import numpy as np
import pytest

import lr_synth_cases as C
from dlib.datasets import lowres

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N = 25000
LAMBDAS = (0.05, 1, 7.3, 29.9, 30, 100, 1000, 65535)


@pytest.mark.parametrize("case", C.PSF_CASES, ids=C.PSF_IDS)
def test_psf_bin_np_against_scipy(case):
    from scipy.ndimage import gaussian_filter
    kind, B, H, W, s, sigma = case[:6]
    in_max = case[6] if len(case) > 6 else None
    src = C.psf_source(case)
    if kind == "uint16":
        assert (src > in_max).any()
    got = lowres.psf_bin_np(src, sigma, s, in_max)
    assert got.dtype == np.float32 and got.shape == (B, H // s, W // s)
    unit = {"float32": lambda a: a, "uint8": lambda a: np.float32(a / 255.),
            "uint16": lambda a: np.float32(np.minimum(a, in_max) / float(in_max))}[kind](src).astype(np.float64)
    worst = 0.0
    for b in range(B):
        blurred = gaussian_filter(unit[b], sigma, mode="reflect") if sigma > 0 else unit[b]
        want = blurred.reshape(H // s, s, W // s, s).mean(axis=(1, 3))
        worst = max(worst, float(np.abs(got[b].astype(np.float64) - want).max()))
    print(f"psf_bin_np {case}: max |statement - scipy| = {worst:.3e} (bound {2.0 ** -24:.3e})")
    assert worst <= 2.0 ** -24


def test_psf_bin_weights_are_the_box_of_scipys_gaussian():
    from scipy.ndimage._filters import _gaussian_kernel1d
    for sigma, s in ((0.0, 2), (0.8, 4), (1.5, 4), (3.4, 8), (4.0, 2), (16.1, 16)):
        w = lowres.psf_bin_weights(sigma, s)
        r = int(4.0 * sigma + 0.5)
        assert w.dtype == np.float64 and w.size == 2 * r + s and (w > 0).all() and abs(w.sum() - 1.0) <= 1e-15
        g = _gaussian_kernel1d(sigma, 0, r) if r else np.ones(1)
        assert np.abs(w - np.convolve(g, np.full(s, 1.0 / s))).max() <= 1e-16
    from srhip import ops
    assert np.array_equal(ops.psf_bin_weights(1.5, 4, "cpu").numpy(), lowres.psf_bin_weights(1.5, 4))
    assert ops.LR_BLUR_MAX_RADIUS == lowres.LR_BLUR_MAX_RADIUS and ops.LR_SYNTH_MAX_PHOTONS == lowres.LR_SYNTH_MAX_PHOTONS
    for bad in ((-1.0, 2), (1.0, 1), (1.0, 17), (16.2, 2), (float("nan"), 2)):
        with pytest.raises(ValueError):
            lowres.psf_bin_weights(*bad)
        with pytest.raises(ops.SrhipError):
            ops.psf_bin_weights(*bad, "cpu")


def test_the_statements_philox_is_philox_ref():
    import philox_ref as PR
    for ctr, key, out in PR.KAT:
        if ctr[3] == 0:
            got = lowres._philox4x32_10(ctr[0], ctr[1], ctr[2], key[0] | (key[1] << 32))
            assert tuple(int(v) for v in got) == out
    c = np.arange(50, dtype=np.uint64)
    seed = 0x1234567890ABCDEF
    a = lowres._philox4x32_10(c, c * np.uint64(3), c + np.uint64(0x80000000), seed)
    b = PR.philox4x32_10(c, c * np.uint64(3), c + np.uint64(0x80000000), np.zeros(50, dtype=np.uint64), seed & PR.MASK32,
                         seed >> 32)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("lam", LAMBDAS)
def test_photon_noise_np_samples_a_poisson_law(lam):
    x = np.ones((1, 1, 100, N // 100), dtype=np.float32)          # photons = lambda, x = 1: lambda exactly
    info = {}
    out, marked = lowres.photon_noise_np(x, 0xC0FFEE + int(lam * 100), lam, 0.0, info=info)
    n, att = info["counts"].reshape(-1), info["attempts"].reshape(-1)
    assert out.dtype == np.float32 and out.shape == x.shape and marked.shape == x.shape
    assert np.array_equal(n, np.rint(n)) and (n >= 0).all()
    assert np.array_equal(np.rint(out.reshape(-1).astype(np.float64) * lam), n)       # the counts can be read off the image
    share = float(marked.mean())
    print(f"lambda {lam}: marked {int(marked.sum())} of {n.size}, most attempts {int(att.max())}, mean {n.mean():.6g}, "
          f"var {n.var():.6g}")
    assert share <= 1e-4
    assert att.max() <= 16 and ((att == 0).all() if lam < 30 else (att >= 1).all())
    assert abs(n.mean() - lam) <= 5.0 * math.sqrt(lam / n.size)
    var_se = math.sqrt((lam + 3.0 * lam * lam - lam * lam) / n.size)
    assert abs(n.var() - lam) <= 5.0 * var_se


def test_photon_noise_np_read_noise_and_edges():
    x = np.zeros((1, 1, 100, N // 100), dtype=np.float32)
    out, marked = lowres.photon_noise_np(x, 77, 100.0, 2.5)
    v = out.reshape(-1).astype(np.float64)
    var = (2.5 / 100.0) ** 2
    assert not marked.any()
    assert abs(v.mean()) <= 5.0 * math.sqrt(var / v.size)
    assert abs(v.var() - var) <= 5.0 * math.sqrt(2.0 * var * var / v.size)
    # lambda = 0 gives 0 and a negative pixel records no photon; no read noise: exact zeros
    x = np.array([0.0, -0.25, 1.0], dtype=np.float32).reshape(1, 1, 1, 3)
    out, _ = lowres.photon_noise_np(x, 5, 200.0, 0.0)
    assert out[0, 0, 0, 0] == 0.0 and out[0, 0, 0, 1] == 0.0 and out[0, 0, 0, 2] > 0.5
    # the off samples keep their bits, the on samples do not depend on the batch they sit in
    x = np.random.default_rng(3).random((3, 1, 5, 7), dtype=np.float32)
    whole, _ = lowres.photon_noise_np(x, 9, 200.0, 2.5, on=[1, 0, 1])
    assert np.array_equal(whole[1], x[1]) and not np.array_equal(whole[0], x[0])
    alone, _ = lowres.photon_noise_np(x[2:], 9, 200.0, 2.5, first_sample=2)
    assert np.array_equal(alone[0], whole[2])
    other, _ = lowres.photon_noise_np(x, 10, 200.0, 2.5, on=[1, 0, 1])
    assert not np.array_equal(other[0], whole[0])
    for bad in ((0.0, 0.0), (-1.0, 0.0), (2e6, 0.0), (10.0, -1.0), (10.0, float("inf"))):
        with pytest.raises(ValueError):
            lowres.photon_noise_np(x, 1, *bad)


BASE = ["--net_type", "swinir"]
PSF = ["--lr_synth", "psf", "--lr_synth_psf_sigma", "1.2", "--lr_synth_photons", "150", "--lr_synth_read_std", "1.5"]
KEYS = ("lr_synth", "lr_synth_psf_sigma", "lr_synth_photons", "lr_synth_read_std")


def test_main_parses_lr_synth_and_config_model_has_the_keys_only_when_given(tmp_path):
    import yaml
    import main as M
    from dlib.utils.utils_config import save_config
    from dlib.utils.own_options import check_lr_synth
    plain = M.parse_input(BASE)
    assert all(k not in dict(plain) for k in KEYS) and check_lr_synth(plain) is None
    cfg = M.parse_input(BASE + PSF)
    assert [cfg[k] for k in KEYS] == ["psf", 1.2, 150.0, 1.5] and check_lr_synth(cfg) == (1.2, 150.0, 1.5)
    bare = M.parse_input(BASE + ["--lr_synth", "psf"])
    assert [bare[k] for k in KEYS] == ["psf", 0.0, 0.0, 0.0] and check_lr_synth(bare) == (0.0, 0.0, 0.0)
    bic = M.parse_input(BASE + ["--lr_synth", "bicubic"])
    assert bic["lr_synth"] == "bicubic" and check_lr_synth(bic) is None
    for c, name in ((plain, "plain"), (cfg, "psf")):
        save_config(c, str(tmp_path / name), "config_model.yml")
        back = yaml.safe_load(open(tmp_path / name / "config_model.yml"))
        if name == "plain":
            assert all(k not in back for k in KEYS)
        else:
            assert [back[k] for k in KEYS] == ["psf", 1.2, 150.0, 1.5]


@pytest.mark.parametrize("argv, name", [
    (["--lr_synth", "psf", "--lr_synth_read_std", "1.5"], "lr_synth_read_std"),
    (["--lr_synth", "psf", "--lr_synth_psf_sigma", "-0.5"], "lr_synth_psf_sigma"),
    (["--lr_synth", "psf", "--lr_synth_photons", "-3"], "lr_synth_photons"),
    (["--lr_synth", "psf", "--lr_synth_photons", "10", "--lr_synth_read_std", "-1"], "lr_synth_read_std"),
    (["--lr_synth", "psf", "--lr_synth_psf_sigma", "16.2"], "lr_synth_psf_sigma"),
    (["--lr_synth", "psf", "--lr_synth_photons", "2e6"], "lr_synth_photons"),
    (["--lr_synth", "lanczos"], "lr_synth lanczos"),
    (["--lr_synth_photons", "10"], "lr_synth_photons"),
    (["--lr_synth", "bicubic", "--lr_synth_photons", "10"], "lr_synth psf"),
])
def test_main_refuses_by_option_name(argv, name, capsys):
    import main as M
    with pytest.raises(SystemExit):
        M.parse_input(BASE + argv)
    assert f"--{name}" in capsys.readouterr().err


def _caco2_args(**kw):
    import yaml
    from dlib.utils.tools import Dict2Obj
    fx = os.path.join(G, "eval_exp")
    a = Dict2Obj(yaml.safe_load(open(os.path.join(fx, "exp", "config_model.yml"))))
    a.train_dsets, a.data_root, a.splits_root = a.test_dsets, os.path.join(fx, "data"), os.path.join(fx, "folds")
    a.h_size, a.batch_size, a.myseed = 64, 2, 3
    a.sample_tr_patch = "uniform"
    for k, v in kw.items():
        a[k] = v
    return a


def test_a_set_without_an_hr_only_pair_refuses_lr_synth_psf():
    from dlib.utils.utils_dataloaders import get_train_set
    from dlib.utils.own_options import check_lr_synth
    with pytest.raises(ValueError, match="--lr_synth psf: the set has no HR-only pair"):
        get_train_set(_caco2_args(lr_synth="psf", lr_synth_psf_sigma=1.2, lr_synth_photons=150.0), "cpu")
    # the same values are refused by name when a set is built from a configuration that never saw the parser
    for kw, name in ((dict(lr_synth="psf", lr_synth_read_std=1.0), "--lr_synth_read_std"),
                     (dict(lr_synth="psf", lr_synth_photons=-1.0), "--lr_synth_photons"),
                     (dict(lr_synth="gauss"), "--lr_synth gauss")):
        with pytest.raises(ValueError, match=name):
            check_lr_synth(_caco2_args(**kw))


def test_eval_pairs_host_path_is_the_statement():
    """EvalPairs.low_res_f32(device=None) under --lr_synth psf: psf_bin_np, then photon_noise_np once per tile as a batch of
    one under LR_SYNTH_EVAL_SALT + index; the training set's clean tile without an index"""
    import types
    from dlib.utils.utils_dataloaders import EvalPairs, LR_SYNTH_EVAL_SALT
    a = types.SimpleNamespace(scale=2, lr_synth="psf", lr_synth_psf_sigma=1.2, lr_synth_photons=150.0, lr_synth_read_std=1.5)
    ev = EvalPairs(a, {}, {})
    img = np.random.default_rng(1).integers(0, 256, (12, 20, 1), dtype=np.uint8)
    clean = lowres.psf_bin_np(img[:, :, 0], 1.2, 2)
    got = ev.low_res_f32(img)
    assert got.shape == (6, 10, 1) and got.dtype == np.float32 and np.array_equal(got[:, :, 0], clean)
    noisy = ev.low_res_f32(img, None, 4)
    want, _ = lowres.photon_noise_np(clean[None, None], LR_SYNTH_EVAL_SALT + 4, 150.0, 1.5)
    assert np.array_equal(noisy[:, :, 0], want[0, 0]) and np.array_equal(noisy, ev.low_res_f32(img, None, 4))
    assert not np.array_equal(noisy, ev.low_res_f32(img, None, 5))
    a.lr_synth_photons = a.lr_synth_read_std = 0.0
    assert np.array_equal(EvalPairs(a, {}, {}).low_res_f32(img, None, 4)[:, :, 0], clean)
