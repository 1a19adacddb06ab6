"""The resolution-scaled error without a GPU: the numpy statement (tests/consistency_ref.py) against scipy, what it finds on planted
pages, the condition the cases of tests/consistency_cases.py must satisfy (every bank of every page is decided by at least 1e-9),
the statement's own rounding e_ref (64 e_ref is the gate of tests/test_gpu_consistency.py), the weight table, the header's two
prototypes and their refusals, and the host side of predict.py --consistency True: records, consistency.yml, the log line, the
refusals.

Measured here: e_ref = 7.7e-14 (score, all 32 slots), 1.6e-14 (alpha), 2.3e-15 (beta), 4.1e-10 (rse: on a noise-free plant the
radicand C_ll - C_bl^2 / C_bb is what float32 left of L, 1e-15 of C_ll, so its float64 rounding is a fraction of it); bank margins
between 4.7e-7 and 7.3e-3."""
import importlib.util
import inspect
import os

import numpy as np
import pytest
import yaml

import consistency_cases as K
import consistency_ref as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sr-caco-2_amd")
EXP = os.path.join(ROOT, "tests", "golden", "eval_exp", "exp")
U = 2.0 ** -53


# ------------------------------------------------------------------ the statement
@pytest.mark.parametrize("h,w,s,q", ((16, 16, 2, 24), (21, 37, 4, 37), (9, 11, 3, 100), (12, 10, 5, 1), (5, 7, 8, 40), (33, 20, 8, 127),
                                     (8, 8, 8, 0), (10, 6, 7, 64), (7, 9, 6, 90)))
def test_model_image_against_scipy(h, w, s, q):
    """b_q against scipy.ndimage.gaussian_filter(float64, sigma, 'reflect') followed by the s x s mean.  The gate is the float64
    rounding of the two compositions, first order in u = 2^-53, on values in [0, 1] under non-negative weights that sum to 1
    (every partial sum is at most 1, so an operation rounds by at most u): the statement does 2 r + s multiply-adds a pass, two
    passes, and each of its weights is a sum of up to s Gaussian weights (s u relative, a pass): 2 (2 r + s) + 2 s roundings;
    scipy does 2 r + 1 multiply-adds a pass, two passes, then a mean of s^2 terms and one division: 2 (2 r + 1) + s^2 + 1.  Both
    start from the same Gaussian weights, bit for bit (tests/test_lr_synth.py).  n roundings are bounded by n u / (1 - n u)."""
    from scipy.ndimage import gaussian_filter
    E = np.random.default_rng(1000 * s + q).random((s * h, s * w), dtype=np.float32)
    sigma = C.sigma_of(q, s)
    r = int(4.0 * sigma + 0.5)
    assert C.weights(q, s).size == 2 * r + s
    got = C.model(E, q, s)
    assert got.dtype == np.float64 and got.shape == (h, w)
    blurred = gaussian_filter(E.astype(np.float64), sigma, mode="reflect") if sigma > 0 else E.astype(np.float64)
    want = blurred.reshape(h, s, w, s).mean(axis=(1, 3))
    n = 2 * (2 * r + s) + 2 * s + 2 * (2 * r + 1) + s * s + 1
    gate = n * U / (1.0 - n * U)
    worst = float(np.abs(got - want).max())
    print(f"[model] {h}x{w} s={s} q={q} sigma={sigma:.4f} r={r}: max |statement - scipy| = {worst:.3e} (gate {gate:.3e})")
    assert worst <= gate


def test_candidates_and_radius():
    """sigma = q s / 64; the largest radius is 64, at q = 127 and s = 8; the radius is (q s + 8) >> 4 in integers (the kernel's form)"""
    for s in range(2, 9):
        for q in range(C.NQ):
            assert int(4.0 * C.sigma_of(q, s) + 0.5) == (q * s + 8) >> 4
    assert C.sigma_of(127, 8) == 15.875 and (127 * 8 + 8) >> 4 == 64


def test_a_reflection_that_folds_more_than_once():
    o = K.expect("5x7_s8")[0]
    assert (C.weights(int(o["qs"].max()), 8).size - 8) // 2 > 40          # a radius above the 40 HR rows of the page


# ------------------------------------------------------------------ the cases and the bound
@pytest.mark.parametrize("name", list(K.CASES))
def test_case_conditions(name):
    """every bank of every page is decided by at least 1e-9 (consistency_ref.gap: against every candidate with other weights)"""
    B, h, w, s, q0s, _, _, padded = K.CASES[name]
    E, L = K.tensors(name)
    each = K.expect(name)
    assert E.shape == (B, 1, s * h, s * w) and L.shape == (B, 1, h, w) and E.dtype == L.dtype == np.float32 and len(each) == B
    assert (padded is not None) == (not E[0].flags["C_CONTIGUOUS"])
    for i, o in enumerate(each):
        print(f"[case] {name}[{i}] q0={q0s[i]} q={o['q']} sigma={o['sigma']:.4f} alpha={float(o['alpha']):.6f} beta={float(o['beta']):.6f} "
              f"rsp={float(o['rsp']):.6f} rse={float(o['rse']):.3e} margins coarse {o['margin'][0]:.2e} fine {o['margin'][1]:.2e}")
        assert not o["degenerate"] and o["n"] == h * w
        assert o["margin"][0] >= K.MIN_MARGIN and o["margin"][1] >= K.MIN_MARGIN
        assert o["qs"][:16].tolist() == list(range(0, 128, 8)) and 0 <= o["qs"].min() and o["qs"].max() <= 127
        assert o["qs"][16:].tolist() == [max(0, int(o["qs"][int(np.argmax(o["scores"][:16]))]) + m - 8) for m in range(16)]
        assert abs(o["q"] - q0s[i]) <= 8 and 0.0 < float(o["rsp"]) <= 1.0 + 1e-12
    assert C.margin(each) == tuple(min(o["margin"][k] for o in each) for k in (0, 1))


def test_gap_counts_candidates_not_values():
    """two slots of one candidate are no runner-up; two candidates with one score are (gap 0)"""
    qs = [0] * 9 + list(range(1, 8))
    v = [0.5] * 9 + [0.4, 0.3, 0.2, 0.1, 0.0, -0.1, -0.2]
    assert C.gap(v, qs, 8) == pytest.approx(0.1)
    v[9] = 0.5
    assert C.gap(v, qs, 8) == 0.0
    assert np.array_equal(C.weights(0, 4), C.weights(1, 4)) and C.gap([0.5, 0.5], [0, 1], 4) == float("inf")


def test_e_ref():
    """the statement's own rounding, per quantity: the unit of the GPU gate"""
    e = K.e_ref()
    print("[e_ref] " + "  ".join(f"{k} {e[k]:.3e} (gate {K.bound(k):.3e})" for k in K.QUANTITIES))
    assert set(e) == set(K.QUANTITIES) and len(K.SMALL) == 4
    assert all(1e-17 < e[k] < 1e-11 for k in ("score", "alpha", "beta")) and 1e-17 < e["rse"] < 1e-7


@pytest.mark.parametrize("name,i", K.NOISE_FREE)
def test_noise_free_plants_are_recovered(name, i):
    """q == q0, and alpha, beta, rsp within what the float32 rounding of L allows.  L = a b + c + delta with |delta| <= d, d one
    float32 spacing at max |L|.  Least squares: alpha - a = C_b,delta / C_bb, and |C_b,delta| <= sqrt(C_bb) sqrt(n) d
    (Cauchy-Schwarz), so |alpha - a| <= d sqrt(n / C_bb); beta - c = mean(delta) - (alpha - a) mean(b), so |beta - c| <= d +
    |alpha - a| |mean(b)|; 1 - r^2 = (residual sum of squares) / C_ll <= n d^2 / C_ll, and 1 - rsp <= 1 - r^2.  The float64
    rounding of the statement comes on top: 64 e_ref of the quantity."""
    B, h, w, s, q0s, _, _, _ = K.CASES[name]
    o = K.expect(name)[i]
    L = K.tensors(name)[1][i, 0]
    a, c = K.gain(i)
    n = h * w
    sb, sbb, sbl, sl, sll = (float(v) for v in o["sums"])
    cbb, cll = sbb - sb * sb / n, sll - sl * sl / n
    d = float(np.spacing(np.float32(np.abs(L).max())))
    g_alpha = d * np.sqrt(n / cbb)
    g_beta = d + g_alpha * abs(sb / n)
    g_rsp = n * d * d / cll
    da, db, dr = abs(float(o["alpha"]) - a), abs(float(o["beta"]) - c), 1.0 - float(o["rsp"])
    print(f"[plant] {name}[{i}] q {o['q']} (q0 {q0s[i]})  |alpha - a| {da:.3e} (gate {g_alpha:.3e})  |beta - c| {db:.3e} (gate {g_beta:.3e})  "
          f"1 - rsp {dr:.3e} (gate {g_rsp:.3e} + {K.bound('score'):.1e})")
    assert o["q"] == q0s[i] and o["sigma"] == q0s[i] * s / 64.0
    assert da <= g_alpha + K.bound("alpha") and db <= g_beta + K.bound("beta")
    assert -K.bound("score") <= dr <= g_rsp + K.bound("score")
    assert float(o["rse"]) <= d + K.bound("rse")


def test_scaling_the_page_scales_the_fit():
    """L -> float32(2 L + 0.1), one more float32 rounding delta of at most d, a spacing at max |2 L + 0.1|: the same q, and by the
    least-squares argument of the plant test alpha -> 2 alpha within d sqrt(n / C_bb), beta -> 2 beta + 0.1 within d + that
    times |mean(b)|"""
    E, L = K.tensors("3x21x37_s4")
    o = K.expect("3x21x37_s4")[2]
    L2 = (2.0 * L[2, 0].astype(np.float64) + 0.1).astype(np.float32)
    p = C.consistency_one(E[2, 0], L2, 4)
    assert p["q"] == o["q"] and p["qs"].tolist() == o["qs"].tolist()
    n = 21 * 37
    sb, sbb = float(o["sums"][0]), float(o["sums"][1])
    d = float(np.spacing(np.float32(np.abs(L2).max())))
    g_alpha = d * np.sqrt(n / (sbb - sb * sb / n))
    assert abs(float(p["alpha"]) - 2 * float(o["alpha"])) <= g_alpha + K.bound("alpha")
    assert abs(float(p["beta"]) - (2 * float(o["beta"]) + 0.1)) <= d + g_alpha * abs(sb / n) + K.bound("beta")


def test_degenerate_pages():
    """a constant page, or a constant output: sigma = alpha = rsp = 0, beta the mean of L, rse its standard deviation"""
    E, L = K.tensors("16x16_s2")
    flat = C.consistency_one(E[0, 0], np.full((16, 16), 0.5, np.float32), 2)
    assert flat["degenerate"] and (flat["q"], flat["sigma"], float(flat["alpha"]), float(flat["rsp"]), float(flat["rse"])) == (0, 0.0, 0.0, 0.0, 0.0)
    assert float(flat["beta"]) == 0.5 and not flat["residual"].any() and flat["scores"].tolist() == [0.0] * 32
    dark = C.consistency_one(np.zeros((32, 32), np.float32), L[0, 0], 2)
    l = L[0, 0].astype(np.float64)
    assert dark["degenerate"] and float(dark["alpha"]) == 0.0 and float(dark["beta"]) == l.sum() / 256
    assert float(dark["rse"]) == pytest.approx(l.std(), rel=1e-12)
    assert np.array_equal(dark["residual"], (l - l.sum() / 256).astype(np.float32))


# ------------------------------------------------------------------ the library's host side
def test_weight_table_is_psf_bin_weights_row_by_row():
    from dlib.datasets import lowres
    from srhip import ops
    assert (ops.CONSISTENCY_Q, ops.CONSISTENCY_PITCH) == (128, 136)
    for s in range(2, 9):
        tab = ops.consistency_table(s)
        assert tab.shape == (128, 136) and tab.dtype == np.float64 and tab.flags["C_CONTIGUOUS"]
        for q in range(128):
            w = lowres.psf_bin_weights(q * s / 64.0, s)
            assert w.size == 2 * ((q * s + 8) >> 4) + s <= 136
            assert np.array_equal(tab[q, :w.size], w) and not tab[q, w.size:].any(), (s, q)
            assert np.array_equal(w, C.weights(q, s))
    for bad in (1, 9, 2.0, True, None):
        with pytest.raises(ops.SrhipError, match="the scale s is an integer 2 .. 8"):
            ops.consistency_table(bad)


def test_header_carries_both_prototypes():
    import ctypes
    from srhip import _lib, ops
    protos = _lib.parse_header()
    assert protos["srhip_consistency_ws"] == ("i", "iiiip")
    # E, E_plane, E_ld, L, L_plane, L_ld, B, h, w, s, weights_table, workspace, workspace_doubles, out, scores, qs, residual, stream
    assert protos["srhip_consistency"] == ("i", "pllplliiiipplppppp")

    def ws(B, h, w, s):
        n = ctypes.c_long(-1)
        ops.call("srhip_consistency_ws", B, h, w, s, ctypes.addressof(n))
        return n.value
    assert ws(1, 64, 64, 8) == 16 * 8 * 5 + 8 and ws(8, 64, 64, 8) == 8 * ws(1, 64, 64, 8)          # tiles of 64 / s LR rows
    assert ws(3, 21, 37, 4) == 3 * (16 * 2 * 5 + 8) and ws(1, 5, 7, 8) == 16 * 5 + 8 and ws(1, 33, 20, 8) == 16 * 5 * 5 + 8
    assert ws(1, 16, 16, 2) == 16 * 5 + 8 and ws(1, 22, 4, 3) == 16 * 2 * 5 + 8
    for args, text in (((1, 64, 64, 9), "2 .. 8"), ((1, 64, 64, 1), "2 .. 8"), ((1, 3, 64, 8), "at least 4"), ((1, 64, 3, 8), "at least 4"),
                       ((0, 64, 64, 8), "B > 0")):
        with pytest.raises(ops.SrhipError, match=text):
            ws(*args)
    text = open(_lib.HEADER).read()
    for words in ("Culley", "NanoJ-SQUIRREL", "a fixed two-bank grid instead of particle-swarm optimisation",
                  "a Gaussian\n * resolution-scaling function only", "no sub-pixel registration", "a signed map", "'reflect' borders",
                  "comparable with another figure from this code", "NO rounding to float32 in between"):
        assert words in text, words


def test_the_entry_point_refuses_by_number_before_any_launch():
    """the argument checks of srhip_consistency come before its first use of a pointer or of the device: every call below passes
    made-up addresses"""
    from srhip import ops
    base = dict(E=0x100000, E_plane=512 * 512, E_ld=512, L=0x900000, L_plane=64 * 64, L_ld=64, B=2, h=64, w=64, s=8, table=0xA00000,
                ws=0xB00000, ws_n=2 * (16 * 8 * 5 + 8), out=0xC00000, scores=None, qs=None, residual=None)

    def call(**kw):
        a = {**base, **kw}
        ops.call("srhip_consistency", a["E"], a["E_plane"], a["E_ld"], a["L"], a["L_plane"], a["L_ld"], a["B"], a["h"], a["w"], a["s"],
                 a["table"], a["ws"], a["ws_n"], a["out"], a["scores"], a["qs"], a["residual"], None)
    for kw, text in ((dict(s=9), "2 .. 8 .got 9"), (dict(s=1), "2 .. 8 .got 1"), (dict(h=3), "at least 4"), (dict(w=3), "at least 4"),
                     (dict(B=0), "1 <= B"), (dict(E=None), "null pointer"), (dict(L=None), "null pointer"), (dict(table=None), "null pointer"),
                     (dict(ws=None), "null pointer"), (dict(out=None), "null pointer"),
                     (dict(E_ld=511), "row stride below the row"), (dict(L_ld=63), "row stride below the row"),
                     (dict(E_plane=512 * 512 - 1), "plane stride below the page"), (dict(L_plane=64 * 64 - 1), "plane stride below the page"),
                     (dict(ws_n=base["ws_n"] - 1), f"holds {base['ws_n'] - 1} doubles, the call needs {base['ws_n']}"),
                     (dict(E=0x100002), "misaligned"), (dict(out=0xC00004), "misaligned"),
                     (dict(out=0xB00000 + 64), "overlap"), (dict(residual=0x900000 + 4096), "overlap"), (dict(scores=0xC00000), "overlap"),
                     (dict(qs=0x100000 + 1024), "overlap"), (dict(ws=0xA00000 + 8), "overlap")):
        with pytest.raises(ops.SrhipError, match=text):
            call(**kw)


def test_ops_wrapper_needs_device_tensors():
    import torch
    from srhip import ops
    with pytest.raises(ops.SrhipError, match="no CPU fallback"):
        ops.consistency(torch.zeros(1, 1, 32, 32), torch.zeros(1, 1, 16, 16), 2)
    with pytest.raises(ops.SrhipError, match="the scale s is an integer 2 .. 8"):
        ops.consistency(torch.zeros(1, 1, 32, 32), torch.zeros(1, 1, 16, 16), 16)


# ------------------------------------------------------------------ predict.py --consistency True
def _cli():
    spec = importlib.util.spec_from_file_location("srhip_predict_cli_consistency", os.path.join(PKG, "predict.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_consistency_record():
    from srhip.predict import consistency_record
    r = consistency_record(8, 4095, [4.5, 0.8, 0.05, 0.9, 0.01, 36.0, 4096.0, 0.0])
    assert r == {"sigma_px": 4.5, "sigma_lr": 0.5625, "alpha": 0.8, "beta": 0.05, "rsp": 0.9, "rse": 0.01, "rse_levels": 40.95}
    assert list(r) == ["sigma_px", "sigma_lr", "alpha", "beta", "rsp", "rse", "rse_levels"] and all(type(v) is float for v in r.values())


def test_consistency_file_and_log_line(tmp_path):
    from srhip.predict import consistency_record
    cli = _cli()
    recs = {1: consistency_record(8, 255, [4.0, 0.8, 0.05, 0.9, 0.02, 32, 4096, 0]),
            0: consistency_record(8, 255, [2.0, 0.7, 0.04, 0.7, 0.04, 16, 4096, 0])}
    rows = cli.consistency_rows(recs)
    assert [r["page"] for r in rows] == [0, 1] and rows[1]["sigma_lr"] == 0.5
    assert list(rows[0]) == ["page", "sigma_px", "sigma_lr", "alpha", "beta", "rsp", "rse", "rse_levels"]
    rsp, rse, lv = cli.consistency_means(rows)
    assert rsp == pytest.approx(0.8) and rse == pytest.approx(0.03) and lv == pytest.approx(7.65)
    line = cli.consistency_line("a.tif", rows)
    assert line.startswith("a.tif: consistency RSP 0.8000, RSE 0.03000 of the white level = 7.65 grey level(s)") and "2 page(s)" in line
    report = {"a.tif": rows, "b.png": cli.consistency_rows({0: recs[1]})}
    cli.write_consistency(str(tmp_path), report)
    back = yaml.safe_load(open(tmp_path / "consistency.yml"))
    assert back == report and list(back) == ["a.tif", "b.png"] and back["b.png"][0]["page"] == 0
    assert cli.residual_path("/x/out/a_stack_x8.tif") == "/x/out/a_stack_x8_residual.tif"
    assert cli.residual_path("/x/out/b_x8.png") == "/x/out/b_x8_residual.tif"


def test_the_option_refuses_by_name_before_the_device(tmp_path):
    import copy
    from PIL import Image
    from dlib.utils import constants
    from srhip.predict import Predictor, PredictError, check_request, load_config
    args = load_config(EXP)
    assert int(args.scale) == 8 and check_request(args, "uint8", 8, 8, consistency=True) == (255, "uint8")
    # a scale above 8: the largest blur of the table would need a radius above 64
    big = load_config(EXP)
    big.scale = 16
    assert check_request(big, "uint8", 40, 40) == (255, "uint8")
    with pytest.raises(PredictError, match=r"--consistency True: scale 16 is outside 2 \.\. 8"):
        check_request(big, "uint8", 40, 40, consistency=True)
    # a side below 4 (a net without the window padding, which refuses such a page for a reason of its own)
    conv = load_config(EXP)
    conv.netG = copy.deepcopy(dict(conv.netG))
    conv.netG["net_type"] = constants.VDSR
    assert check_request(conv, "uint8", 3, 64) == (255, "uint8")
    for H, W in ((3, 64), (64, 3), (2, 2)):
        with pytest.raises(PredictError, match=rf"--consistency True: a {H} x {W} page is too small.*at least 4"):
            check_request(conv, "uint8", H, W, consistency=True)
    pred = Predictor(EXP)
    assert pred.last_consistency is None and pred.last_residuals is None
    with pytest.raises(PredictError, match="consistency_maps=True needs consistency=True"):
        pred.run(np.zeros((2, 40, 40), np.uint8), consistency_maps=True)
    assert pred._model is None                                         # nothing was built or moved to the device
    sig = inspect.signature(Predictor.run).parameters
    assert sig["consistency"].default is False and sig["consistency_maps"].default is False
    # the command line: --consistency_maps True alone is refused by name, and nothing is written
    cli = _cli()
    src = tmp_path / "in"
    src.mkdir()
    Image.fromarray(np.zeros((40, 45), np.uint8)).save(str(src / "a_fine.png"))
    with pytest.raises(PredictError, match="--consistency_maps True needs --consistency True"):
        cli.predict(["--exp_path", EXP, "--input", str(src), "--output", str(tmp_path / "out"), "--consistency_maps", "True"])
    assert not os.path.exists(tmp_path / "out")
    with pytest.raises(SystemExit):
        cli.predict(["--exp_path", EXP, "--input", str(src), "--consistency", "perhaps"])
