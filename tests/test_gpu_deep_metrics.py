"""The full-depth metrics on the device: srhip_tensor2levels, srhip_metrics_psnr_family_lv and srhip_metrics_ssim_lv against the
float64 statements of tests/deep_metric_cases.py, dlib.metrics.sweep(levels=...) beside the 8-bit sweep, and fast_eval with
--metric_levels on an 8-bit fold and its 257 v twin.

Bounds: Q_L and MSE (a sum of integers in double) bit for bit; PSNR 1e-9, NRMSE 1e-12 and -- the kernel being float64, with no
float32 path to mimic -- PSNR_Y 1e-9; SSIM by the suite's Gates rule at scale 1 under the ceiling METRIC_SSIM = 5e-5, the [B, 9]
buffer as one comparison (tests/test_gpu_step_kernels.py: test_metrics_ssim)."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import step_kernel_cases as C  # noqa: E402
import deep_metric_cases as M  # noqa: E402
import deep_tile_cases as D  # noqa: E402
from test_gpu_tape_op_kernels import Gates, NAN  # noqa: E402


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


# ------------------------------------------------------------------ srhip_tensor2levels
@pytest.mark.parametrize("L", (255,) + M.LEVELS)
def test_tensor2levels(ops, L):
    """srhip_tensor2levels bit for bit against the numpy statement of Q_L: values below 0 and above 1, -0.0, hundreds of exact
    half-way products (round half to even); n = 2048 * 256 + 77, past the grid cap"""
    from dlib import metrics
    x, _ = M.levels_inputs(L)
    out = torch.full((M.LEVELS_N,), NAN, device="cuda")
    ops.call("srhip_tensor2levels", dev(x).data_ptr(), out.data_ptr(), M.LEVELS_N, L, ops._st())
    with Gates(f"tensor2levels L={L}") as G:
        G.equal(out, M.t_q(x, L), "Q_L")
        G.equal(ops.tensor2levels(dev(x), L), out, "the wrapper")
        G.equal(metrics.tensor2levels(dev(x), L), out, "dlib.metrics")
        if L == 255:
            G.equal(ops.tensor2uint82float(dev(x)), out, "tensor2uint82float")


def test_the_entry_points_refuse_what_they_cannot_do(ops):
    x = torch.zeros(1, 1, 32, 32, device="cuda")
    for bad in (254, 65536):
        with pytest.raises(ValueError, match="255 .. 65535"):
            ops.tensor2levels(x, bad)
        for name in ("srhip_metrics_psnr_family_lv", "srhip_metrics_ssim_lv"):
            with pytest.raises(ops.SrhipError, match="255 .. 65535"):
                _call_lv(ops, name, x, x, 0, (), bad, False)
        with pytest.raises(ops.SrhipError, match="255 .. 65535"):
            ops.call("srhip_tensor2levels", x.data_ptr(), x.data_ptr(), x.numel(), bad, ops._st())
    for name in ("srhip_metrics_psnr_family_lv", "srhip_metrics_ssim_lv"):
        with pytest.raises(ops.SrhipError, match="at most 8"):
            _call_lv(ops, name, x, x, 0, tuple(range(9)), 4095, False, ws=1 << 16)
    with pytest.raises(ops.SrhipError, match="11x11"):
        _call_lv(ops, "srhip_metrics_ssim_lv", x, x, 11, (), 4095, False, ws=64)      # 10 x 10 after the crop
    with pytest.raises(ops.SrhipError, match="empty image"):
        _call_lv(ops, "srhip_metrics_psnr_family_lv", x, x, 16, (), 4095, False)
    assert ops.lib.srhip_metrics_ssim_lv_ws(1, 32, 32, 11, 0) == 0
    assert ops.lib.srhip_metrics_ssim_lv_ws(3, 43 + 10, 44 + 10, 0, 8) == 2 * 3 * 9 * 2 * 3   # 43 x 44 outputs: 2 x 3 tiles of 32 x 16


# ------------------------------------------------------------------ the raw calls: NaN workspace of the declared size, NaN output
def _call_lv(ops, name, E, Hh, border, ths, L, lv, ws=None):
    B, (H, W) = E.shape[0], E.shape[-2:]
    nth = len(ths)
    th = torch.tensor(list(ths) or [0], dtype=torch.int32, device="cuda")
    if ws is None:
        ws = (ops.lib.srhip_metrics_ws(B, nth) if name.endswith("family_lv") else ops.lib.srhip_metrics_ssim_lv_ws(B, H, W, border, nth))
    guard = 16
    buf = torch.full((ws + guard,), NAN, dtype=torch.float64, device="cuda")
    out = torch.full((B, nth + 1, 4) if name.endswith("family_lv") else (B, nth + 1), NAN, dtype=torch.float64, device="cuda")
    ops.call(name, E.data_ptr(), Hh.data_ptr(), B, H, W, border, th.data_ptr(), nth, L, int(lv), buf.data_ptr(), out.data_ptr(), ops._st())
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[ws:]).all()), "the guard behind the workspace was written"
    return out.cpu()


# ------------------------------------------------------------------ srhip_metrics_psnr_family_lv
@pytest.mark.parametrize("L", M.LEVELS)
@pytest.mark.parametrize("nth", (0, 8))
@pytest.mark.parametrize("H,W,border", C.METRIC_PSNR_SHAPES)
def test_metrics_psnr_family_lv(ops, H, W, border, nth, L):
    """srhip_metrics_psnr_family_lv against the float64 statements, on the cases of the 8-bit test at L levels (1 pixel after
    the crop; whole blocks without a pixel; image 1 pred == target: the 1e-45 floor; image 2 constant with its 8-bit level at 64:
    `>= 64` all of it -- cnt == npix, den == 0 -> 1 --, `>= 65` none of it).  The ROI is thresholded at the 8-bit levels.  The
    float form (a prediction off the grid and beyond [0, 1], the target on the L grid) and the levels form give the same bits."""
    pr, hf, a, b = (dev(t) for t in M.psnr_inputs(H, W, border, L))
    ths = C.METRIC_PSNR_THS[:nth]
    ref = M.psnr_expect(H, W, border, nth, L)
    out = _call_lv(ops, "srhip_metrics_psnr_family_lv", pr, hf, border, ths, L, False)
    with Gates(f"metrics_psnr_family_lv {H}x{W} border={border} nth={nth} L={L}") as G:
        G.true(out.shape == ref.shape and bool(torch.isfinite(out).all()), "a slot was not written")
        for k, th in enumerate((None,) + ths):
            e = (out[:, k] - ref[:, k]).abs().max(0)[0]
            print(f"[metric] {G.name} th {th}: psnr {e[0]:.3e} psnr_y {e[1]:.3e} mse {e[2]:.3e} nrmse {e[3]:.3e}")
            G.equal(out[:, k, 2], ref[:, k, 2], f"mse th={th}")                 # integer sums: exact
            G.true(e[0].item() < 1e-9, f"psnr th={th}: {e[0]:.3e}")
            G.true(e[3].item() < 1e-12, f"nrmse th={th}: {e[3]:.3e}")
            G.true(e[1].item() < 1e-9, f"psnr_y th={th}: {e[1]:.3e}")
        floor = 20 * np.log10(L) + 450                                          # 20 log10(L / sqrt(1e-45))
        G.true(abs(out[1, 0, 0].item() - floor) < 1e-9, "pred == target: the PSNR of the 1e-45 floor")
        lv = _call_lv(ops, "srhip_metrics_psnr_family_lv", a, b, border, ths, L, True)
        G.true(torch.equal(bits64(lv), bits64(out)), "inputs_are_levels: other bits")
        G.true(torch.equal(bits64(ops.metrics_psnr_family_lv(pr, hf, border, ths, L)), bits64(out)), "the wrapper: other bits")


# ------------------------------------------------------------------ srhip_metrics_ssim_lv
@pytest.mark.parametrize("L", M.LEVELS)
@pytest.mark.parametrize("border", C.METRIC_SSIM_BORDERS)
@pytest.mark.parametrize("h,w", C.METRIC_SSIM_SIZES)
def test_metrics_ssim_lv(ops, h, w, border, L):
    """srhip_metrics_ssim_lv against the float64 statement, B = 4: the three step targets of the 8-bit test at L levels and one
    bright-smooth image (0.97 + 0.02 x / W, noise of 0.002 and 0.004), on which sigma^2 = E[x^2] - E[x]^2 in float32 is 1e-3 a
    pixel off.  Cropped sizes 11x11 (one output pixel: the gate is per pixel, and the plain float32 statement is above the
    ceiling there -- tests/test_cpu_deep_metrics.py), 12x43, 42x42, 43x44 (tiles of 32 x 16 outputs: slivers both ways), borders
    0, 3, 8.  The ROI at the window centre, thresholded at the 8-bit levels: 0 the whole image, 300 nothing (exactly 0 / 1).
    nth = 0 is slot 0.  Two calls give the same bits; the levels form gives the bits of the float form."""
    E, Hf, a, b = (dev(t) for t in M.ssim_inputs(h, w, border, L))
    ref64, ref32 = M.ssim_expect(h, w, border, L)
    with Gates(f"metrics_ssim_lv {h}x{w} border={border} L={L}") as G:
        out = _call_lv(ops, "srhip_metrics_ssim_lv", E, Hf, border, C.METRIC_SSIM_THS, L, False)
        for k in range(9):                                                # slot by slot, for the record
            print(f"[slot] {G.name} slot {k}: kernel {(out[:, k] - ref64[:, k]).abs().max():.3e} "
                  f"fp32 {(ref32[:, k].double() - ref64[:, k]).abs().max():.3e}")
        print(f"[bright-smooth] {G.name}: kernel {(out[3] - ref64[3]).abs().max():.3e} fp32 {(ref32[3].double() - ref64[3]).abs().max():.3e}")
        G(out, ref64, ref32, C.METRIC_SSIM, "[B, 9]", scale=1.0)
        empty = C.METRIC_SSIM_THS.index(300) + 1
        G.equal(out[:, empty], torch.zeros(4, dtype=torch.float64), "the empty ROI is 0 / 1")
        again = _call_lv(ops, "srhip_metrics_ssim_lv", E, Hf, border, C.METRIC_SSIM_THS, L, False)
        G.true(torch.equal(bits64(again), bits64(out)), "two calls: other bits")
        lv = _call_lv(ops, "srhip_metrics_ssim_lv", a, b, border, C.METRIC_SSIM_THS, L, True)
        G.true(torch.equal(bits64(lv), bits64(out)), "inputs_are_levels: other bits")
        out0 = _call_lv(ops, "srhip_metrics_ssim_lv", E, Hf, border, (), L, False)
        G.true(out0.shape == (4, 1), "nth = 0: one slot")
        G.true(torch.equal(bits64(out0[:, 0]), bits64(out[:, 0])), "nth = 0 is not slot 0 of nth = 8")
        G.true(torch.equal(bits64(ops.metrics_ssim_lv(E, Hf, border, C.METRIC_SSIM_THS, L)), bits64(out)), "the wrapper: other bits")


# ------------------------------------------------------------------ dlib.metrics.sweep(levels=...)
@pytest.fixture(scope="module")
def grid8():
    """prediction and target on the 8-bit grid, v / 255 with integer v: the 43 x 44 step images under border 3"""
    _, _, a, b = C.metric_ssim_inputs(43, 44, 3)
    return a, b, dev(a / 255), dev(b / 255)


def test_sweep_at_65535_is_comparable_with_the_8_bit_sweep(ops, grid8):
    """both images on the 8-bit grid: the levels at 65535 are 257 v, so MSE is exactly 257^2 times the 8-bit MSE, PSNR and
    NRMSE agree (1e-9, 1e-12; PSNR not where the MSE is 0: the floor 1e-45 is in levels^2 at either L, and 20 log10(L) + 450
    depends on L), PSNR_Y within the 8-bit kernel's float32 Y (the suite's 1e-4), SSIM within the 8-bit kernel's own distance from
    float64 (5e-5).  The ROI counts are identical: read from pairs with a constant difference (a non-empty ROI's masked MSE is
    that constant squared, an empty one's 0) and from a pair that differs by one level at the target's brightest pixel, which
    lies in every non-empty ROI (masked MSE = 1 / count)."""
    from dlib import metrics
    a, b, E, H = grid8
    ths = C.METRIC_SSIM_THS
    s8, s16 = metrics.sweep(E, H, 3, ths), metrics.sweep(E, H, 3, ths, levels=65535)
    with Gates("sweep levels=65535 against levels=255") as G:
        G.true(s16["ssim"].dtype == torch.float64 and all(s16[k].shape == s8[k].shape == (3, 9) for k in s8), "dtypes and shapes")
        crop = b[:, :, 3:-3, 3:-3]
        want = torch.stack([(crop >= th).reshape(3, -1).sum(-1) for th in ths], 1).double()     # the ROI counts
        n = torch.cat([torch.full((3, 1), float(crop[0].numel()), dtype=torch.float64), want.clamp(min=1)], 1)
        sse8, sse16 = (s8["mse"].cpu() * n).round(), (s16["mse"].cpu() * n).round()              # integers, far below 2^51
        G.true(((s8["mse"].cpu() * n - sse8).abs().max() < 1e-6) and ((s16["mse"].cpu() * n - sse16).abs().max() < 1e-3), "sums of squares")
        G.equal(sse16, sse8 * 257.0 ** 2, "mse: not 257^2 times the 8-bit one")
        some = (s8["mse"] > 0).cpu()
        G.true(bool(some[:, :8].all()) and not bool(some[:, 8].any()), "slots 0 .. 7 have pixels, slot 8 has none")
        for k, bound in (("psnr", 1e-9), ("nrmse", 1e-12), ("psnr_y", 1e-4), ("ssim", C.METRIC_SSIM)):
            e = (s16[k].double() - s8[k].double()).abs().cpu()
            e = e[some] if k.startswith("psnr") else e
            print(f"[comparable] {k}: {e.max().item():.3e}")
            G.true(e.max().item() <= bound, f"{k}: {e.max().item():.3e} > {bound:g}")
        G.true((s16["psnr"][:, 8].cpu() - (20 * np.log10(65535.) + 450)).abs().max().item() < 1e-9, "the floor of an empty ROI")
        # the ROI counts
        Ec = dev(torch.where(b < 2, b + 2, b - 2) / 255)        # a constant difference of two 8-bit levels
        c8, c16 = metrics.sweep(Ec, H, 3, ths)["mse"].cpu(), metrics.sweep(Ec, H, 3, ths, levels=65535)["mse"].cpu()
        G.equal(c8[:, 1:], 4.0 * (want > 0).double(), "constant difference, 8-bit")
        G.equal(c16[:, 1:], 4.0 * 257 ** 2 * (want > 0).double(), "constant difference, 65535")
        E1 = H.clone()
        for i in range(3):
            flat = crop[i, 0].reshape(-1).argmax().item()
            y, x = 3 + flat // crop.shape[3], 3 + flat % crop.shape[3]
            E1[i, 0, y, x] = (b[i, 0, y, x].item() - 1) / 255
        o8, o16 = metrics.sweep(E1, H, 3, ths)["mse"].cpu(), metrics.sweep(E1, H, 3, ths, levels=65535)["mse"].cpu()
        cnt8 = torch.where(o8[:, 1:] > 0, 1.0 / o8[:, 1:], torch.zeros(3, 8, dtype=torch.float64))
        cnt16 = torch.where(o16[:, 1:] > 0, 257.0 ** 2 / o16[:, 1:], torch.zeros(3, 8, dtype=torch.float64))
        G.true((cnt8 - want).abs().max().item() < 1e-6 and (cnt16 - want).abs().max().item() < 1e-6, "the ROI counts")


def test_sweep_at_255_is_the_untouched_sweep(ops, grid8):
    """levels = 255 takes the two 8-bit launches: the bits of sweep() without the argument and of the entry points themselves;
    the four mbatch functions likewise, and at L levels they are the sweep's slots"""
    from dlib import metrics
    a, b, E, H = grid8
    ths = C.METRIC_SSIM_THS
    for args, u8 in (((E, H), False), ((dev(a), dev(b)), True)):
        s, s255 = metrics.sweep(*args, 3, ths, u8), metrics.sweep(*args, 3, ths, u8, levels=255)
        fam = ops.metrics_psnr_family(*args, 3, ths, u8)
        assert s255["ssim"].dtype == torch.float32
        assert all(torch.equal(s[k], s255[k]) for k in s)
        assert torch.equal(s255["ssim"], ops.metrics_ssim(*args, 3, ths, u8))
        assert all(torch.equal(s255[k], fam[:, :, i]) for i, k in enumerate(("psnr", "psnr_y", "mse", "nrmse")))
    L = 4095
    aL, bL = dev(M.t_q(a / 255, L)), dev(M.t_q(b / 255, L))
    sL = metrics.sweep(aL, bL, 3, (150,), True, levels=L)
    roi = (dev(M.t_level8(bL.cpu(), L)) >= 150).float()
    for name, fn in (("psnr", metrics.mbatch_gpu_calculate_psnr), ("mse", metrics.mbatch_gpu_calculate_mse),
                     ("nrmse", metrics.mbatch_gpu_calculate_nrmse), ("ssim", metrics.mbatch_gpu_calculate_ssim)):
        assert torch.equal(fn(dev(a), dev(b), 3), metrics.sweep(dev(a), dev(b), 3, (), True)[name][:, 0]), name
        assert torch.equal(fn(aL, bL, 3, None, L), sL[name][:, 0]), name
        assert torch.equal(fn(aL, bL, 3, roi, L), sL[name][:, 1]), name


# ------------------------------------------------------------------ fast_eval with --metric_levels
class Args(dict):
    __getattr__ = dict.get
    __setattr__ = dict.__setitem__


def test_fast_eval_at_65535_on_an_8_bit_fold_and_its_scaled_twin(ops, tmp_path):
    """the 8-bit paired fold of the 16-bit tile tests and the same fold times 257, through fast_eval with metric_levels = 65535 on
    a small SwinIR: the net's inputs are bit-equal between the folds and the targets are the levels 257 v either way, so every
    tracker value and every entry of the details is equal; the values are the statements' on the net's own output."""
    from dlib.utils import constants
    from dlib.models.select_model import define_model
    from dlib.utils.utils_dataloaders import get_eval_loader as _loader
    from dlib.utils.utils_tracker import init_tracker
    from dlib.utils.utils_trainer import fast_eval, _forward_with_padding
    hr = [D.tile_u8(40, 48, seed=30 + i) for i in range(3)]
    lr = [D.down_u8(t, 2) for t in hr]
    x257 = lambda t: (257 * t.astype(np.int64)).astype(np.uint16)
    ds8, ds16 = "biosrp8-test-X-2", "biosrp16-test-X-2"
    data, folds = D.write_fold(str(tmp_path), ds8, hr, lr)
    D.write_fold(str(tmp_path), ds16, [x257(t) for t in hr], [x257(t) for t in lr])
    netG = {'net_type': constants.SWINIR, 'swinir_upscale': 2, 'swinir_in_chans': 1, 'swinir_img_size': 16,
            'swinir_window_size': 8, 'swinir_img_range': 1.0, 'swinir_depths': [2], 'swinir_embed_dim': 60,
            'swinir_num_heads': [6], 'swinir_mlp_ratio': 2, 'swinir_upsampler': constants.US_PIXEL_SHUFFLE_DIRECT,
            'swinir_resi_connection': constants.R_CONNECTION_1CONV}
    ths = [20, 100]
    args = Args(netG=netG, train={}, is_train=False, scale=2, outd=str(tmp_path), data_root=data, splits_root=folds, eval_bsize=3,
                eval_over_roi_also=True, eval_over_roi_also_ths=ths, eval_over_roi_also_model_select=False,
                model_select_mtr=constants.PSNR_MTR, valid_dsets=ds8, test_dsets=ds8 + constants.SEP + ds16,
                basic_interpolation="bicubic", is_master=True, metric_levels=65535)
    get_eval_loader = lambda _, ds: _loader(types.SimpleNamespace(scale=2, splits_root=folds, data_root=data, eval_bsize=3), ds)
    torch.manual_seed(5)
    model = define_model(args)
    model.netG.eval()
    got = {}
    for ds in (ds8, ds16):
        tr, det, roi_tr, roi_det = fast_eval(model, get_eval_loader(args, ds), ds, constants.TESTSET, init_tracker(args),
                                             init_tracker(args), args, -1, -1, nbr_to_plot=0)
        got[ds] = (tr[constants.TESTSET][ds], roi_tr[constants.TESTSET][ds], [det[k] for k in sorted(det)],
                   [roi_det[k] for k in sorted(roi_det)])
    assert len(got[ds8][2]) == 3 and set(got[ds8][2][0]) == {"psnr", "mse", "nrmse", "ssim", "psnr_y"}
    assert got[ds8] == got[ds16]
    # the values are those of the statements at 65535 on the net's output
    batch = next(iter(get_eval_loader(args, ds8)))
    E = _forward_with_padding(batch, model, args).current_visuals()['E'].cpu()
    tile = [int(k.split("_")[-1].split(".")[0]) for k in batch['h_id']]
    a, b = M.t_q(E, 65535), torch.from_numpy(np.stack([257. * hr[t] for t in tile])[:, None]).float()
    close = lambda x, y: abs(x - y) <= 1e-12 * max(abs(y), 1.0)
    for j, i in enumerate(sorted(range(3), key=lambda i: batch['h_id'][i])):
        d, rd = got[ds8][2][j], got[ds8][3][j]
        assert d["mse"] == M.mse_lv(a, b, 65535, 2)[i].item()
        assert abs(d["psnr"] - M.psnr_lv(a, b, 65535, 2)[i].item()) < 1e-9
        assert abs(d["ssim"] - M.ssim_lv(a, b, 65535, 2)[i].item()) <= C.METRIC_SSIM
        assert close(rd["mse"], np.mean([M.mse_lv(a, b, 65535, 2, th)[i].item() for th in ths]))
    assert len(got[ds8][0]["mse"]["vals"]) == 1 and close(got[ds8][0]["mse"]["vals"][0], np.sum([d["mse"] for d in got[ds8][2]]) / 3.0)
    # without the flag the same fold is measured at 256 levels, in other units
    args.metric_levels = None
    tr, det, _, _ = fast_eval(model, get_eval_loader(args, ds8), ds8, constants.TESTSET, init_tracker(args), init_tracker(args),
                              args, -1, -1, nbr_to_plot=0)
    assert all(det[k]["mse"] < 0.01 * got[ds8][2][j]["mse"] for j, k in enumerate(sorted(det)))
