"""Fourier ring correlation without a GPU: the conditions the image pairs of tests/frc_cases.py must satisfy, the reference's own
rounding e_ref (64 e_ref is the gate of tests/test_gpu_frc.py), the integer ring rule, the packing identity the kernel rests on,
the --frc / --frc_threshold options of main.py and eval.py, the constants and tracker keys, and the header's two prototypes.

e_ref measured here: 9.4e-16 (np.fft.fft2 against a direct DFT in np.longdouble over the five cases with S <= 128)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import frc_cases as K
import frc_ref as R
from dlib.utils.constants import FRC_CUT             # (the parent of this feature has none of it)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sr-caco-2_amd")
FX = os.path.join(ROOT, "tests", "golden", "eval_exp")


# ------------------------------------------------------------------ the cases and the bound
@pytest.mark.parametrize("name", list(K.CASES))
def test_case_conditions(name):
    """every kept ring of both images holds at least 1e-7 of the mean ring power; up to and including the crossing ring no
    FRC[r] lies within 1e-6 of T (no case is marked); at the crossing p - FRC[r] >= 1e-3; the curve starts at 1"""
    B, h, w, N, lv, _ = K.CASES[name]
    curve, cut, each = K.expect(name)
    S = R.side(h, w)
    assert curve.shape == (B, S // 2 + 1) and cut.shape == (B,) and curve.dtype == cut.dtype == np.float64
    for i, o in enumerate(each):
        weakest = min((o["p1"] / o["p1"].mean()).min(), (o["p2"] / o["p2"].mean()).min())
        upto = o["curve"] if o["r"] is None else o["curve"][:o["r"] + 1]
        print(f"[case] {name}[{i}] S={o['side']} cut={o['cut']:.6f} r={o['r']} p-q={o['p'] - o['q']:.3e} "
              f"weakest ring={weakest:.2e} nearest to T={np.abs(upto - R.T_DEFAULT).min():.2e}")
        assert o["side"] == S and weakest >= 1e-7
        assert not o["marked"] and np.abs(upto - R.T_DEFAULT).min() >= R.MARK
        assert o["r"] is not None and o["p"] - o["q"] >= 1e-3
        assert 0.0 < o["cut"] < 1.0 and o["curve"][0] == pytest.approx(1.0, abs=1e-12) and o["curve"][1] > 0.99
    if B > 1:
        assert len({round(float(c), 9) for c in cut}) == B            # different images
    E, H = K.images(name)
    assert E.shape == (B, 1, h, w) and E.dtype == np.float32
    if lv:
        assert E.max() > 255 and np.array_equal(E, np.rint(E))         # levels 0 .. N


def test_levels_case_is_the_float_case():
    a, b = K.expect("128x128_65535"), K.expect("128x128_65535_levels")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_e_ref():
    """the reference's own rounding, the unit of the GPU gate; a few 1e-16 .. 1e-14 by the precision of float64"""
    e = K.e_ref()
    print(f"[e_ref] {e:.3e}   gate 64 e_ref = {K.bound():.3e}")
    assert 1e-17 < e < 1e-12


def test_marking_rule_and_cutoff():
    T = R.T_DEFAULT
    c = np.array([1.0, 0.9, 0.5, 0.1, 0.3, 0.05])
    o = R.cutoff(c, T)
    assert o["r"] == 3 and o["cut"] == pytest.approx((2 + (0.5 - T) / 0.4) / 5) and not o["marked"]
    assert R.cutoff(np.array([1.0, 0.9, T + 5e-7, 0.1]), T)["marked"]
    assert not R.cutoff(np.array([1.0, 0.9, 0.1, T + 5e-7]), T)["marked"]          # behind the crossing ring
    o = R.cutoff(np.array([1.0, 0.9, 0.5, 0.3]), T)
    assert o["r"] is None and o["cut"] == 1.0
    assert R.cutoff(np.array([0.1, 0.05, 0.9]), T)["cut"] == 0.0                    # ring 0 already under T
    assert R.cutoff(np.array([0.1, 0.9, 0.05]), T)["r"] == 2                        # the search starts at r = 1
    assert R.cut_bound(dict(r=3, p=0.5, q=0.1, side=64, cut=0.5), 1e-13) == 2e-13 / (0.4 * 32) + np.spacing(0.5)
    with pytest.raises(ValueError, match="at least 32"):
        R.side(31, 64)
    assert [R.side(*s) for s in ((32, 32), (37, 45), (70, 151), (63, 64), (2100, 2050), (4096, 4096))] == [32, 32, 64, 32, 2048, 2048]


# ------------------------------------------------------------------ the ring rule
@pytest.mark.parametrize("S", (32, 64, 128, 256, 512, 1024, 2048))
def test_ring_rule_is_the_rounded_radius(S):
    """(2r - 1)^2 <= 4 |k|^2 < (2r + 1)^2 is rint(|k|): |k| = r + 1/2 has no integer solution, so rint meets no tie"""
    ring = R.ring_index(S)
    k = np.fft.fftfreq(S, 1.0 / S)
    want = np.rint(np.hypot(k[:, None], k[None, :])).astype(np.int64)
    assert ring.shape == (S, S) and ring[0, 0] == 0 and ring[0, S // 2] == S // 2 and ring[S // 2, S // 2] == -1
    assert np.array_equal(ring, np.where(want <= S // 2, want, -1))
    counts = np.bincount(ring[ring >= 0], minlength=S // 2 + 1)
    assert counts[0] == 1 and counts[1] == 8 and counts.min() >= 1 and counts.sum() < S * S
    q = 4 * (k[:, None] ** 2 + k[None, :] ** 2)
    assert not np.any(np.sqrt(q) % 2 == 1)                            # 2 |k| is never an odd integer


# ------------------------------------------------------------------ the packing identity
@pytest.mark.parametrize("S", (32, 64))
def test_two_real_spectra_from_one_complex_transform(S):
    """z = a + i b, A = Z(k), B = conj Z(-k): F1 = (A + B) / 2, F2 = (A - B) / (2i); and the three ring terms of -k are those of
    k, which is why the kernel takes the columns kx and S - kx in one block and doubles"""
    rng = np.random.default_rng(S)
    a, b = rng.standard_normal((2, S, S))
    Z = np.fft.fft2(a + 1j * b)
    idx = (-np.arange(S)) % S
    Bm = np.conj(Z[idx][:, idx])
    F1, F2 = np.fft.fft2(a), np.fft.fft2(b)
    scale = np.abs(Z).max()
    assert np.abs((Z + Bm) / 2 - F1).max() <= 1e-14 * scale and np.abs((Z - Bm) / 2j - F2).max() <= 1e-14 * scale
    for term in ((F1 * np.conj(F2)).real, np.abs(F1) ** 2, np.abs(F2) ** 2):
        assert np.abs(term[idx][:, idx] - term).max() <= 1e-12 * np.abs(term).max()
    ring = R.ring_index(S)
    assert np.array_equal(ring[idx][:, idx], ring)


def test_statement_properties():
    """E = H: every ring 1 within rounding and the cutoff exactly 1.0; a noise-free blurred copy also gives 1 on every ring
    (the pairs need their noise); more noise on one H never raises the cutoff"""
    H = K.target(64, 64, 5)
    o = R.frc_one(H, H)
    assert np.abs(o["curve"] - 1.0).max() <= 1e-12 and o["cut"] == 1.0 and o["r"] is None
    assert np.abs(R.frc_one(np.clip(K.blur(H, 1.0), 0, 1), H, 65535)["curve"] - 1.0).max() < 0.05
    cuts = [R.frc_one(K.prediction(H, 5, noise=n), H)["cut"] for n in (0.003, 0.01, 0.03, 0.1)]
    assert all(a >= b for a, b in zip(cuts, cuts[1:])) and cuts[0] > cuts[-1]
    with pytest.raises(ValueError, match=r"\(0, 1\)"):
        R.frc_one(H, H, T=1.0)


# ------------------------------------------------------------------ the library's host side
def test_header_carries_both_prototypes():
    from srhip import _lib, ops
    protos = _lib.parse_header()
    assert protos["srhip_metrics_frc_lv_ws"] == ("l", "iii")
    # E, Hh, B, H, W, L, inputs_are_levels, threshold, workspace, workspace_doubles, curve, cut, stream
    assert protos["srhip_metrics_frc_lv"] == ("i", "ppiiiiidplppp")
    ws = ops.lib.srhip_metrics_frc_lv_ws
    assert ws(1, 31, 64) == 0 and ws(1, 64, 31) == 0 and ws(0, 64, 64) == 0
    assert ws(1, 32, 32) == 2 * 32 * 32 + 3 * 17 * 17 and ws(3, 70, 151) == 3 * (2 * 64 * 64 + 3 * 33 * 33)
    assert ws(8, 2100, 2050) == 8 * (2 * 2048 * 2048 + 3 * 1025 * 1025)
    assert ws(40, 2048, 2048) * 8 > 2 ** 31 and ws(40, 2048, 2048) == 40 * ws(1, 2048, 2048)          # long, not int
    assert [ops.frc_side(*s) for s in ((31, 64), (32, 32), (37, 45), (70, 151), (2100, 2050), (5000, 4096))] == [0, 32, 32, 64, 2048, 2048]
    assert all(ops.frc_side(h, w) == R.side(h, w) for h, w in ((32, 33), (127, 128), (128, 127), (1023, 2000), (2047, 2049)))
    assert ops.FRC_THRESHOLD == R.T_DEFAULT == 1.0 / 7.0


def test_the_entry_point_refuses_by_number_before_any_launch():
    """the argument checks of srhip_metrics_frc_lv come before its first use of a pointer or of the device"""
    from srhip import ops

    def call(H, W, L=255, thr=1.0 / 7.0, ws_doubles=1 << 24):
        ops.call("srhip_metrics_frc_lv", None, None, 1, H, W, L, 0, thr, None, ws_doubles, None, None, None)
    for kw, text in ((dict(H=31, W=64), "at least 32"), (dict(H=64, W=31), "at least 32"), (dict(H=64, W=64, thr=0.0), r"\(0, 1\)"),
                     (dict(H=64, W=64, thr=1.0), r"\(0, 1\)"), (dict(H=64, W=64, thr=float("nan")), r"\(0, 1\)"),
                     (dict(H=64, W=64, L=254), "254"), (dict(H=64, W=64, L=65536), "65536")):
        with pytest.raises(ops.SrhipError, match=text):
            call(**kw)
    for bad in (0.0, 1.0, -0.1, True, "0.5", None):
        with pytest.raises(ValueError, match=r"\(0, 1\)"):
            ops.frc_threshold(bad)


# ------------------------------------------------------------------ the command line
def _main(*flags):
    import main
    return main.parse_input(["--net_type", "swinir", "--method", "SWINIR", *flags])


def test_main_cli_accepts():
    from dlib.utils.own_options import check_frc
    for flags in ((), ("--frc", "False")):
        a = _main(*flags)
        assert "frc_threshold" not in a and not a.frc and ("frc" in a) == bool(flags) and check_frc(a) == 0
    a = _main("--frc", "True")
    assert a.frc is True and "frc_threshold" not in a and check_frc(a) == 1.0 / 7.0
    a = _main("--frc", "True", "--frc_threshold", "0.5")
    assert a.frc is True and a.frc_threshold == 0.5 and check_frc(a) == 0.5


REFUSED = ((("--frc_threshold", "0.5"), "--frc_threshold 0.5 needs --frc True"),
           (("--frc", "False", "--frc_threshold", "0.5"), "--frc_threshold"),
           (("--frc", "True", "--frc_threshold", "0"), "--frc_threshold"),
           (("--frc", "True", "--frc_threshold", "1.0"), "--frc_threshold"),
           (("--model_select_mtr", "frc_cut"), "--model_select_mtr frc_cut"),
           (("--frc", "True", "--model_select_mtr", "frc_cut"), "--model_select_mtr frc_cut"))


@pytest.mark.parametrize("flags,named", REFUSED)
def test_main_cli_refuses_by_name(flags, named, capsys):
    with pytest.raises(SystemExit) as e:
        _main(*flags)
    assert e.value.code == 2 and named in capsys.readouterr().err


def _eval_module_cli():
    import importlib.util
    spec = importlib.util.spec_from_file_location("srhip_eval_frc_cli", os.path.join(PKG, "eval.py"))
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)
    return ev


def _eval_args(*flags):
    ev = _eval_module_cli()
    return ev.load_args(["--exp_path", os.path.join(FX, "exp"), "--data_root", os.path.join(FX, "data"), *flags])[1]


def test_eval_cli(capsys):
    a = _eval_args()
    assert "frc" not in a and "frc_threshold" not in a
    a = _eval_args("--frc", "True")
    assert a.frc is True and "frc_threshold" not in a
    a = _eval_args("--frc", "True", "--frc_threshold", "0.25")
    assert a.frc is True and a.frc_threshold == 0.25
    for flags, named in ((("--frc_threshold", "0.25"), "--frc_threshold"), (("--frc", "True", "--frc_threshold", "1.5"), "--frc_threshold")):
        with pytest.raises(SystemExit) as e:
            _eval_args(*flags)
        assert e.value.code == 2 and named in capsys.readouterr().err


def test_eval_frc_false_turns_off_a_recorded_run(tmp_path, capsys):
    """an experiment whose config_model.yml recorded frc and frc_threshold: eval.py reads both back; --frc False alone turns it
    off (the inherited threshold goes with it); --frc False with a threshold given on the command line is still refused"""
    import shutil
    import yaml
    from dlib.utils.own_options import check_frc
    exp = tmp_path / "exp"
    os.makedirs(exp)
    cfg = yaml.safe_load(open(os.path.join(FX, "exp", "config_model.yml")))
    cfg.update(frc=True, frc_threshold=0.25)
    yaml.dump(cfg, open(exp / "config_model.yml", "w"))
    lead = ["--exp_path", str(exp), "--data_root", os.path.join(FX, "data")]
    ev = _eval_module_cli()
    a = ev.load_args(lead)[1]
    assert a.frc is True and a.frc_threshold == 0.25 and check_frc(a) == 0.25
    a = ev.load_args(lead + ["--frc_threshold", "0.5"])[1]
    assert a.frc is True and check_frc(a) == 0.5
    a = ev.load_args(lead + ["--frc", "False"])[1]
    assert a.frc is False and "frc_threshold" not in a and check_frc(a) == 0
    with pytest.raises(SystemExit) as e:
        ev.load_args(lead + ["--frc", "False", "--frc_threshold", "0.5"])
    assert e.value.code == 2 and "--frc_threshold 0.5 needs --frc True" in capsys.readouterr().err


def test_the_rate_tool_states_the_definition():
    """tools/frc_rate.py's torch arm on the CPU: its gather-and-sum ring sums give the statement's curve, every kept frequency
    is gathered once and the padding points at the appended zero"""
    import importlib.util
    import torch
    spec = importlib.util.spec_from_file_location("srhip_frc_rate", os.path.join(ROOT, "tools", "frc_rate.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    for S in (32, 64, 512):
        idx = tool.ring_gather(S, "cpu").numpy()
        ring = R.ring_index(S).ravel()
        assert idx.shape[0] == S // 2 + 1 and idx.min() >= 0 and idx.max() == S * S
        for r in (0, 1, S // 4, S // 2):
            got = idx[r][idx[r] < S * S]
            assert np.array_equal(np.sort(got), np.nonzero(ring == r)[0])
        assert (idx < S * S).sum() == (ring >= 0).sum()
    E, H = K.images("3x70x151")
    fn = tool.torch_statement(64, 255, torch.device("cpu"))
    c = fn(torch.from_numpy(E.copy()), torch.from_numpy(H.copy())).numpy()
    assert np.abs(c - K.expect("3x70x151")[0]).max() <= 64 * K.e_ref()


@pytest.mark.parametrize("prog,lead", (("main.py", ("--net_type", "swinir", "--method", "SWINIR")),
                                       ("eval.py", ("--exp_path", os.path.join(FX, "exp"), "--data_root", os.path.join(FX, "data")))))
def test_the_exit_code_of_the_programs(prog, lead):
    """main.py and eval.py as programs: exit code 2 and the flag in stderr for both refusals, before any use of the device"""
    for flags, text in ((("--frc_threshold", "0.5"), "--frc_threshold 0.5 needs --frc True"),
                        (("--frc", "True", "--frc_threshold", "2"), "--frc_threshold 2.0: the threshold is a number in (0, 1)")):
        r = subprocess.run([sys.executable, os.path.join(PKG, prog), *lead, *flags], capture_output=True, text=True)
        assert r.returncode == 2 and text in r.stderr, (r.returncode, r.stderr[-400:])


# ------------------------------------------------------------------ constants and trackers
def test_a_report_metric_not_a_tracker_metric():
    from dlib.utils import constants, utils_tracker as T
    from dlib.utils.tools import Dict2Obj
    assert FRC_CUT == "frc_cut" and constants.REPORT_METRICS == ["frc_cut"]
    assert constants.METRICS == ["psnr", "ssim", "mse", "nrmse", "psnr_y", "ssim_y"] and constants.EXTRA_METRICS == ["msssim"]
    assert "frc_cut" not in constants.BEST_MTR and "frc_cut" not in constants.EXTRA_BEST_MTR
    base = dict(valid_dsets="v", test_dsets="t", basic_interpolation="bicubic", model_select_mtr="psnr")
    for extra, keys in ((dict(frc=True), constants.METRICS), (dict(frc=True, frc_threshold=0.5), constants.METRICS),
                        (dict(frc=True, msssim=True), constants.METRICS + ["msssim"])):
        a, plain = Dict2Obj(dict(base, **extra)), Dict2Obj(dict(base, **{k: v for k, v in extra.items() if k == "msssim"}))
        assert T.extra_metrics(a) == T.extra_metrics(plain) and T.extra_metrics(a, roi=True) == []
        assert T.init_tracker(a) == T.init_tracker(plain) and T.init_tracker(a, roi=True) == T.init_tracker(plain, roi=True)
        assert all(list(node) == keys for split in ("val", "test") for node in T.init_tracker(a)[split].values())
        assert all(list(node) == constants.METRICS for split in ("val", "test") for node in T.init_tracker(a, roi=True)[split].values())
    with pytest.raises(AssertionError):
        T.update_tracker_eval(T.init_tracker(Dict2Obj(dict(base, frc=True))), "val", "v", "frc_cut", 0.5)


def test_the_report_file():
    from dlib.utils.utils_trainer import _frc_report
    import torch
    def det():
        return {"a": {"psnr": 30.0, "frc_cut": 0.5, "_frc_side": 64.0}, "b": {"psnr": 31.0, "frc_cut": 0.0, "_frc_side": 32.0}}
    curves = {64: [torch.full((33,), 1.5, dtype=torch.float64), 3], 32: [torch.ones(17, dtype=torch.float64), 1]}
    d = det()
    rep = _frc_report(1.0 / 7.0, 0.25, d, curves)
    assert d == {"a": {"psnr": 30.0, "frc_cut": 0.5}, "b": {"psnr": 31.0, "frc_cut": 0.0}}          # the side left the details
    assert list(rep) == ["threshold", "mean_cut", "images", "mean_curve"] and rep["threshold"] == 1.0 / 7.0 and rep["mean_cut"] == 0.25
    assert rep["images"] == {"a": {"side": 64, "cut": 0.5, "res_px": 4.0}, "b": {"side": 32, "cut": 0.0, "res_px": None}}
    assert list(rep["mean_curve"]) == [32, 64] and rep["mean_curve"][64] == [0.5] * 33 and rep["mean_curve"][32] == [1.0] * 17
    sharded = _frc_report(0.5, 0.25, det(), None)
    assert sharded["mean_curve"] is None and "rank-sharded" in sharded["mean_curve_note"] and sharded["images"] == rep["images"]
    import yaml
    assert yaml.safe_load(yaml.dump(rep)) == rep


def test_fast_eval_wiring_with_stand_in_metrics(tmp_path, monkeypatch):
    """evaluate_single_ds with dlib.metrics replaced by CPU stand-ins (the statement for frc, ones for the sweep): without the
    option the files, keys and previews of today; with it 'frc_cut' in the details, frc_<ds>.yml over two side lengths, the mean
    in the log, the same previews, and trackers equal to those of the run without it"""
    import torch
    import yaml
    import dlib.utils.utils_trainer as U
    from dlib import metrics
    from dlib.utils.tools import Dict2Obj
    from dlib.utils.utils_tracker import init_tracker

    class Model:
        def set_eval_mode(self):
            pass

        def set_train_mode(self):
            pass

        def current_visuals(self):
            return self.v

    def forward(batch, model, args):
        model.v = {'E': batch['e'], 'H': batch['h_im']}
        return model

    def sweep(E, H, border=0, thresholds=(), **kw):
        return {m: torch.ones(E.shape[0], 1 + len(thresholds)) for m in ('psnr', 'psnr_y', 'mse', 'nrmse', 'ssim')}

    def frc(E, H, levels=255, threshold=1.0 / 7.0, inputs_are_u8=False):
        c, k, _ = R.frc(E.numpy(), H.numpy(), levels, threshold)
        return {'curve': torch.from_numpy(c), 'cut': torch.from_numpy(k), 'side': R.side(*E.shape[-2:])}
    logged = []
    monkeypatch.setattr(U, "_forward_with_padding", forward)
    monkeypatch.setattr(metrics, "sweep", sweep)
    monkeypatch.setattr(metrics, "frc", frc)
    monkeypatch.setattr(metrics, "tensor2uint82float", lambda x: (x.clamp(0, 1) * 255).round())
    monkeypatch.setattr(U.DLLogger, "log", lambda msg, *a, **k: logged.append(str(msg)))
    batches = []
    for j, (name, n) in enumerate((("128x128_65535", 1), ("3x70x151", 3))):
        E, H = (torch.from_numpy(t.copy()) for t in K.images(name))
        batches.append({'h_im': H, 'e': E, 'l_im': H[..., ::8, ::8], 'h_id': [f't/h_{j}_{i}.tif' for i in range(n)]})
    out = {}
    for key, extra in (("plain", {}), ("frc", {"frc": True})):
        d = str(tmp_path / key)
        a = Dict2Obj(dict(valid_dsets='v', test_dsets='t', basic_interpolation='bicubic', model_select_mtr='psnr', scale=8,
                          eval_over_roi_also=True, eval_over_roi_also_ths=[10, 20], eval_over_roi_also_model_select=False, outd=d,
                          outd_backup=d, save_dir_imgs='images', is_master=True, distributed=False, eval_bsize=1, **extra))
        out[key] = U.evaluate_single_ds(a, Model(), batches, 't', init_tracker(a), init_tracker(a, roi=True), -1, -1, 'test')
    assert out["plain"] == out["frc"]
    plain, on = tmp_path / "plain", tmp_path / "frc"
    names = ['details_t.yml', 'roi-t.yaml', 'roi_details_t.yml', 't.yaml']
    assert sorted(os.listdir(plain / "best-models")) == names and sorted(os.listdir(on / "best-models")) == sorted(names + ['frc_t.yml'])
    previews = sorted(os.listdir(plain / "images" / "test" / "t"))
    assert previews == ['t_h_0_0.tif.png', 't_h_1_0.tif.png', 't_h_1_1.tif.png', 't_h_1_2.tif.png']
    assert sorted(os.listdir(on / "images" / "test" / "t")) == previews
    for f in names[1:]:
        assert yaml.safe_load(open(plain / "best-models" / f)) == yaml.safe_load(open(on / "best-models" / f))
    det0, det = (yaml.safe_load(open(p / "best-models" / "details_t.yml")) for p in (plain, on))
    rep = yaml.safe_load(open(on / "best-models" / "frc_t.yml"))
    cuts = {'t/h_0_0.tif': K.expect("128x128_65535")[1][0], **{f't/h_1_{i}.tif': K.expect("3x70x151")[1][i] for i in range(3)}}
    assert list(det) == list(det0) == list(cuts) == list(rep["images"])
    for img, cut in cuts.items():
        assert set(det0[img]) == {'psnr', 'psnr_y', 'mse', 'nrmse', 'ssim'} and set(det[img]) == set(det0[img]) | {'frc_cut'}
        # (the first pair is quantised at 255 here, not at the case's 65535: only the batch of three is compared in value)
        if img.startswith('t/h_1_'):
            assert det[img]['frc_cut'] == cut and rep["images"][img] == {'side': 64, 'cut': cut, 'res_px': 2.0 / cut}
    assert rep["images"]['t/h_0_0.tif']['side'] == 128 and rep["threshold"] == 1.0 / 7.0
    assert abs(rep["mean_cut"] - sum(det[i]['frc_cut'] for i in det) / 4.0) <= 1e-15
    assert list(rep["mean_curve"]) == [64, 128] and [len(v) for v in rep["mean_curve"].values()] == [33, 65]
    assert np.abs(np.array(rep["mean_curve"][64]) - K.expect("3x70x151")[0].mean(0)).max() <= 1e-15
    assert sum("frc_cut: " in m for m in logged) == 1
