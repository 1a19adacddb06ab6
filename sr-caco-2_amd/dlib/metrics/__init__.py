"""SR evaluation metrics on libsrhip.

The reference keeps them in ``dlib/utils/utils_image.py`` (843-1198, 369-372,
618-653) and calls them from ``utils_trainer._compute_metrics`` (:961-1032);
``north_star`` names the surface ``dlib.metrics``.  Same function names,
arguments ``(img1, img2, border=0, roi=None)`` and ``(B,)`` results.  The ROI is
given as the reference builds it, ``roi = (H_img >= th).float()``; because the
kernels take thresholds, a mask is mapped back to its threshold when it has
that form and rejected otherwise (``sweep`` is the fast fused entry point: all
five metrics x all thresholds in two passes over the images).

``levels`` (not a reference argument; ``--metric_levels``): the number of the white level the images are quantised to,
255 .. 65535.  255 is the reference's metric, bit for bit.  Any other value takes the float64 kernels: MSE is then in
levels^2, PSNR is 20 log10(levels / sqrt(mse)), SSIM is on level / levels with float64 window moments, and ``inputs_are_u8``
/ the inputs of ``mbatch_gpu_calculate_*`` mean the levels 0 .. ``levels``.  The ROI stays ``Q_255(H) >= th``, the pixel set
of the 8-bit metrics, whatever ``levels`` is.

``msssim`` (not a reference argument; ``--msssim``): the number of scales, 1 .. 5, of the multi-scale SSIM of Wang, Simoncelli and
Bovik (2003) that ``sweep`` adds under 'msssim'; include/srhip.h (srhip_metrics_msssim_lv) states it.  It is float64 at either
white level, a whole-image metric without ROI slots, and needs both cropped sides to be at least 10 * 2^(scales - 1) + 1.

``frc`` / ``mbatch_gpu_calculate_frc`` (not reference functions; ``--frc``): the Fourier ring correlation of prediction against
target and its cutoff, the resolution figure of the light-microscopy literature; include/srhip.h (srhip_metrics_frc_lv) states it.
A call of its own, never part of ``sweep``: a report metric, not a tracker metric.  No border crop (a Hann window instead), the
centred power-of-two square, float64; both sides at least 32.

``decorr`` (not a reference function; ``predict.py --resolution``): image decorrelation analysis (Descloux, Grussmayer, Radenovic
2019), the resolution of ONE image with no target and no second acquisition; include/srhip.h (srhip_metrics_decorr_lv) states it.
The square, the window and the rings are the FRC's; a call of its own, never part of ``sweep``.

``consistency`` (not a reference function; ``predict.py --consistency``): the resolution-scaled error of NanoJ-SQUIRREL (Culley et
al. 2018), how well a super-resolved image, blurred, binned and rescaled, explains the LR page it was made from -- RSP, RSE and
the signed error map, with no target; include/srhip.h (srhip_consistency) states it.  A call of its own, never part of ``sweep``.
"""
import torch

from srhip import ops

__all__ = ['tensor2uint82float', 'tensor2levels', 'mbatch_gpu_calculate_psnr', 'mbatch_gpu_calculate_mse',
           'mbatch_gpu_calculate_nrmse', 'mbatch_gpu_calculate_ssim', 'mbatch_gpu_calculate_msssim', 'sweep',
           'frc', 'mbatch_gpu_calculate_frc', 'decorr', 'consistency']


def _need_cuda(t):
    if not t.is_cuda:
        raise RuntimeError("dlib.metrics (libsrhip) runs on the GPU only; there is no CPU fallback")


def tensor2uint82float(img):
    """(img.clamp(0,1)*255).round().clamp(0,255); utils_image.py:369-372."""
    _need_cuda(img)
    return ops.tensor2uint82float(img)


def tensor2levels(img, levels):
    """(img.clamp(0,1)*levels).round().clamp(0,levels): tensor2uint82float at the white level ``levels``."""
    _need_cuda(img)
    return ops.tensor2levels(img, levels)


def _threshold_of(roi, img2, levels=255):
    """roi == (img2 >= th) for an integer th in [0,256]?  Returns th or raises.  img2 holds the levels 0 .. ``levels``; the
    threshold is one of its 8-bit levels, Q_255(float32(v / levels))."""
    if roi is None:
        return None
    assert roi.ndim == 4 and roi.shape[1] == 1 and roi.shape[0] == img2.shape[0]
    on = roi > 0
    if not bool(on.any()):
        return 256                      # empty ROI: nothing reaches the threshold
    if levels != 255:
        img2 = ops.tensor2uint82float((img2.double() / levels).float())
    th = int(img2[on].min().item())
    if not torch.equal(on, img2 >= th):
        raise NotImplementedError("libsrhip metrics take ROIs of the form (H >= threshold) "
                                  "(utils_trainer.py:983-988)")
    return th


def sweep(E, H, border=0, thresholds=(), inputs_are_u8=False, levels=255, msssim=0):
    """All metrics in two fused passes.  E, H: (B,1,h,w) in [0,1] (or already
    u8-valued floats; with ``levels``, floats that hold the levels 0 .. levels).  Returns dict name ->
    (B, 1+len(thresholds)) tensors; column 0 is 'no ROI', column k the ROI H_u8 >= thresholds[k-1].  ``levels`` other than
    255: the float64 kernels at that white level (module docstring); 'ssim' is then float64.  ``msssim`` = M > 0: the dict gains
    'msssim', the (B,) float64 multi-scale SSIM over M scales at ``levels``; the five other tensors are those of ``msssim=0``."""
    _need_cuda(E)
    assert E.shape == H.shape and E.ndim == 4 and E.shape[1] == 1, "1-channel images"
    E, H = E.float().contiguous(), H.float().contiguous()
    if levels == 255:
        fam = ops.metrics_psnr_family(E, H, border, tuple(thresholds), inputs_are_u8)
        ssim = ops.metrics_ssim(E, H, border, tuple(thresholds), inputs_are_u8)
    else:
        fam = ops.metrics_psnr_family_lv(E, H, border, tuple(thresholds), levels, inputs_are_u8)
        ssim = ops.metrics_ssim_lv(E, H, border, tuple(thresholds), levels, inputs_are_u8)
    out = {"psnr": fam[:, :, 0], "psnr_y": fam[:, :, 1], "mse": fam[:, :, 2],
           "nrmse": fam[:, :, 3], "ssim": ssim}
    if msssim:
        out["msssim"] = ops.metrics_msssim_lv(E, H, border, levels, msssim, inputs_are_u8)[:, 0].contiguous()
    return out


def _one(name, img1, img2, border, roi, levels=255):
    _need_cuda(img1)
    assert img1.ndim == 4 and img1.shape == img2.shape
    th = _threshold_of(roi, img2, levels)
    out = sweep(img1, img2, border, () if th is None else (th,), inputs_are_u8=True, levels=levels)[name]
    return out[:, 0 if th is None else 1].contiguous()


def mbatch_gpu_calculate_psnr(img1, img2, border=0, roi=None, levels=255):
    """utils_image.py:843-891; inputs in [0,255]; fp64 result."""
    return _one("psnr", img1, img2, border, roi, levels)


def mbatch_gpu_calculate_mse(img1, img2, border=0, roi=None, levels=255):
    """utils_image.py:894-934."""
    return _one("mse", img1, img2, border, roi, levels)


def mbatch_gpu_calculate_nrmse(img, y, border=0, roi=None, levels=255):
    """utils_image.py:937-1007."""
    return _one("nrmse", img, y, border, roi, levels)


def mbatch_gpu_calculate_ssim(x, y, border=0, roi=None, levels=255):
    """utils_image.py:1120-1198; fp32 result."""
    return _one("ssim", x, y, border, roi, levels)


def mbatch_gpu_calculate_msssim(x, y, border=0, levels=255, scales=5):
    """(not a reference function) multi-scale SSIM over ``scales`` scales; inputs hold the levels 0 .. ``levels``; fp64 (B,)."""
    _need_cuda(x)
    assert x.ndim == 4 and x.shape == y.shape and x.shape[1] == 1, "1-channel images"
    return ops.metrics_msssim_lv(x, y, border, levels, scales, True)[:, 0].contiguous()


def frc(E, H, levels=255, threshold=ops.FRC_THRESHOLD, inputs_are_u8=False):
    """(not a reference function) Fourier ring correlation of E against H, (B,1,h,w) in [0,1] (or, with ``inputs_are_u8``, floats
    that hold the levels 0 .. ``levels``).  Returns {'curve': (B, S/2 + 1) float64 over the rings 0 .. S/2, 'cut': (B,) float64,
    the first crossing of ``threshold`` as a fraction of Nyquist (2 / cut is the resolution in pixels), 'side': S}."""
    _need_cuda(E)
    assert E.shape == H.shape and E.ndim == 4 and E.shape[1] == 1, "1-channel images"
    curve, cut = ops.metrics_frc_lv(E, H, levels, threshold, inputs_are_u8)
    return {"curve": curve, "cut": cut, "side": ops.frc_side(*E.shape[-2:])}


def mbatch_gpu_calculate_frc(x, y, levels=255, threshold=ops.FRC_THRESHOLD):
    """(not a reference function) the cutoff of the Fourier ring correlation; inputs hold the levels 0 .. ``levels``; fp64 (B,)."""
    _need_cuda(x)
    assert x.ndim == 4 and x.shape == y.shape and x.shape[1] == 1, "1-channel images"
    return ops.metrics_frc_lv(x, y, levels, threshold, True)[1]


def decorr(X, levels=255, inputs_are_levels=False, curves=False):
    """(not a reference function) image decorrelation analysis of every image of X, (B,1,h,w) in [0,1] (or, with
    ``inputs_are_levels``, floats that hold the levels 0 .. ``levels``): no target is needed.  Returns {'cut': (B,) float64, the
    resolution as a fraction of Nyquist (2 / cut is the resolution in pixels; 0: none was found), 'ring': (B,) int64, 'amp': (B,)
    float64, the height of the peak, 'sigma': (B,) float64, the width of the high-pass that gave it (0: none), 'side': S}; with
    ``curves`` also 'curves': (B, 21, S/2 + 1) float64 and 'peaks': (B, 21) int32, the peak ring of every curve."""
    _need_cuda(X)
    assert X.ndim == 4 and X.shape[1] == 1, "1-channel images"
    res = ops.metrics_decorr_lv(X, levels, inputs_are_levels, curves)
    out = res[0] if curves else res
    d = {"cut": out[:, 0].contiguous(), "ring": out[:, 1].to(torch.int64), "amp": out[:, 2].contiguous(),
         "sigma": out[:, 3].contiguous(), "side": ops.frc_side(*X.shape[-2:])}
    if curves:
        d["curves"], d["peaks"] = res[1], res[2]
    return d


def consistency(E, L, scale, scores=False, residual=False):
    """(not a reference function) resolution-scaled error of the outputs E, (B,1,scale h,scale w), against the LR pages L,
    (B,1,h,w), both float32 in units of the white level, strided views welcome; scale 2 .. 8.  Returns {'sigma': (B,) float64, the
    blur in HR pixels under which E explains L best, 'alpha', 'beta': (B,) float64, the linear intensity rescaling, 'rsp': (B,)
    float64, the Pearson coefficient of the degraded E with L, 'rse': (B,) float64, the RMS residual in units of the white level,
    'q': (B,) int64, sigma = q scale / 64}; with ``scores`` also 'scores': (B, 32) float64 and 'qs': (B, 32) int32, the signed r^2
    of the coarse and the fine bank and their q; with ``residual`` also 'residual': (B, h, w) float32, L minus the rescaled
    degraded E, positive where the acquisition is brighter than the output explains."""
    _need_cuda(E)
    _need_cuda(L)
    res = ops.consistency(E, L, scale, scores, residual)
    res = res if isinstance(res, tuple) else (res,)
    out = res[0]
    d = {"sigma": out[:, 0].contiguous(), "alpha": out[:, 1].contiguous(), "beta": out[:, 2].contiguous(),
         "rsp": out[:, 3].contiguous(), "rse": out[:, 4].contiguous(), "q": out[:, 5].to(torch.int64)}
    if scores:
        d["scores"], d["qs"] = res[1], res[2]
    if residual:
        d["residual"] = res[-1]
    return d
