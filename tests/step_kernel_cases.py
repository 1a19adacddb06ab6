"""Cases, inputs and float64 / float32 statements of the training-step kernel tests (the loss, metric, optimizer and
element-wise kernels every net's step ends in).

tests/test_gpu_step_kernels.py runs the kernels on what this module builds and gates them against what it states;
tests/test_cpu_step_kernel_inputs.py checks, on the statements alone, that the inputs have the properties the GPU tests
rely on.  Both import the builders from here, so the GPU tests cannot drift from what was checked.

The statements are the oracle's own functions (oracle/sr_oracle.py: loss_*, metric_*, tensor2uint82float), torch.optim and
F.interpolate; gradients are autograd of the statement in its own dtype.  Every `*_expect` function returns a list of Exp:
one gated comparison each, with the statement evaluated in float64 (the reference) and in float32 (the yardstick)."""
import functools
import math
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

import sr_oracle as O

F32_ROUNDING = 2.0 ** -24          # the least e32 the gate reckons with (Gates, tests/test_gpu_tape_op_kernels.py)
CAP = 2048 * 256                   # elements one pass of the largest element-wise grid covers; beyond it the grid strides

POINTWISE, SSIM_VALUE, SSIM_GRAD, STENCIL, BOUNDED, HIST_VALUE, HIST_GRAD, ELEMENTWISE = (
    1e-6, 1e-4, 2e-4, 2e-6, 5e-6, 2e-5, 5e-4, 2e-6)
METRIC_SSIM = 5e-5


class Exp(NamedTuple):
    what: str
    ref64: torch.Tensor
    ref32: torch.Tensor
    ceiling: float
    scale: Optional[float] = None      # None: the float64 result's largest entry


def e32_of(x):
    """the float32 statement's distance from float64 as Gates reckons it"""
    s = (x.ref64.abs().max().item() if x.scale is None else x.scale) + 1e-300
    return max((x.ref32.double() - x.ref64.double()).abs().max().item() / s, F32_ROUNDING)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def value_and_grad(stmt, pred, dtype):
    """stmt(dtype)(pred) -> scalar loss; returns (value [1], d value / d pred), both in dtype"""
    p = pred.to(dtype).clone().requires_grad_(True)
    v = stmt(dtype)(p)
    g = torch.autograd.grad(v, p, allow_unused=True)[0] if v.requires_grad else None
    return v.detach().reshape(1).clone(), (torch.zeros_like(p) if g is None else g).detach()


class LossRef(NamedTuple):
    v64: torch.Tensor
    g64: torch.Tensor
    v32: torch.Tensor
    g32: torch.Tensor


def loss_ref(stmt, pred):
    v64, g64 = value_and_grad(stmt, pred, torch.float64)
    v32, g32 = value_and_grad(stmt, pred, torch.float32)
    return LossRef(v64, g64, v32, g32)


def accum_buffers(r, seed=5):
    """non-zero float32 buffers of the result's own size for the accumulate flags"""
    g0 = ((torch.rand(r.g64.shape, generator=gen(seed)) - 0.5) * 2 * max(r.g64.abs().max().item(), 1e-3)).float()
    v0 = torch.tensor([0.75 * max(r.v64.abs().item(), 1e-3)], dtype=torch.float32)
    return g0, v0


VARIANTS = ("plain", "nograd", "accum")


def loss_exps(r, variant, cv, cg, sv=None, sg=None):
    """plain: value and gradient; nograd: the value alone (grad = NULL); accum: both added onto accum_buffers(r)"""
    if variant == "nograd":
        return [Exp("value", r.v64, r.v32, cv, sv)]
    if variant == "plain":
        return [Exp("value", r.v64, r.v32, cv, sv), Exp("grad", r.g64, r.g32, cg, sg)]
    g0, v0 = accum_buffers(r)
    return [Exp("value", v0.double() + r.v64, v0 + r.v32, cv, sv),
            Exp("grad", g0.double() + r.g64, g0.reshape(r.g32.shape) + r.g32, cg, sg)]


# ------------------------------------------------------------------ loss_l1l2 / loss_pointwise
POINTWISE_KINDS = {            # name: (mode, eps, weighted); loss_l1l2 takes modes 0 and 1 only
    "l1": (0, None, False), "l1w": (0, None, True), "l2": (1, None, False),
    "charbonnier_1e-9": (2, 1e-9, False), "charbonnier_1e-3": (2, 1e-3, False), "l2sum": (3, None, False)}
POINTWISE_N = (1, 255, 256, 257, CAP + 77)
POINTWISE_LAM = 2.0


@functools.lru_cache(maxsize=None)
def pointwise_inputs(n):
    """pred, target, weight; a stretch of pred == target (sign(0) = 0) wherever there is room for one"""
    g = gen(100 + n % 1000)
    pred, target, weight = torch.rand(n, generator=g), torch.rand(n, generator=g), torch.rand(n, generator=g) * 2
    if n >= 8:
        target[n // 3:n // 2] = pred[n // 3:n // 2]
    return pred, target, weight


@functools.lru_cache(maxsize=None)
def pointwise_ref(kind, n):
    mode, eps, weighted = POINTWISE_KINDS[kind]
    pred, target, weight = pointwise_inputs(n)

    def stmt(dt):
        t, w = target.to(dt), weight.to(dt)
        if mode == 0:
            return lambda p: O.loss_l1(p, t, POINTWISE_LAM, w if weighted else None)
        if mode == 1:
            return lambda p: O.loss_l2(p, t, POINTWISE_LAM)
        if mode == 2:
            return lambda p: O.loss_charbonnier(p, t, POINTWISE_LAM, eps)
        return lambda p: O.loss_l2sum(p, t, POINTWISE_LAM)
    return loss_ref(stmt, pred)


def pointwise_expect(kind, n, variant):
    return loss_exps(pointwise_ref(kind, n), variant, POINTWISE, POINTWISE)


# ------------------------------------------------------------------ loss_bounded
BOUNDED_T = (1.0, O.elb_t_after(40), 10.0)
BOUNDED_CASES = [(t, scale, eps, 1000) for t in BOUNDED_T for scale in (1.0, 255.0) for eps in (0.0, 0.01)] + [
    (O.elb_t_after(40), 255.0, 0.01, CAP + 77)]
BOUNDED_LAM = 0.5


@functools.lru_cache(maxsize=None)
def bounded_inputs(t, scale, eps, n):
    """generic pairs at least 0.05 apart, then by hand: z_r and z_l on the branch point z == -1 / t^2 (exactly so for scale
    1, eps 0; the barrier and its derivative are continuous there, so a neighbouring float lands on the same value), elements
    inside the band |pred - target| <= eps, and elements far outside it on either side.  (A generic pair closer than 0.05
    at scale 255 has z = 255 pred - 255 target - eps a float32 cancellation, 1.5e-5 off, and just past the branch point the
    gradient 1 / (t z) of the float32 STATEMENT is then 4.6e-6 of the largest entry off float64: no yardstick.)"""
    g = gen(200 + n % 1000)
    target = torch.rand(n, generator=g)
    pred = target + (0.05 + 0.5 * torch.rand(n, generator=g)) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1)
    ct = float(1.0 / torch.tensor(t, dtype=torch.float32) ** 2)
    d = max(ct - eps, 0.0) / scale
    pred[0], target[0] = 0.0, d                # z_r = pred * scale - (target * scale + eps) = -ct
    pred[1], target[1] = d, 0.0                # z_l = -ct
    pred[2], target[2] = 0.0, 0.0              # inside the band (small values: target * scale + eps rounds finely)
    pred[3], target[3] = eps / (2 * scale), 0.0
    pred[4], target[4] = 1.9, 0.05             # far outside: past the branch point of one term even at t = 1, scale 1, so
    pred[5], target[5] = -0.9, 0.95            # the gradient's largest entry is of the order of t whatever t and scale
    return pred, target


@functools.lru_cache(maxsize=None)
def bounded_ref(t, scale, eps, n):
    pred, target = bounded_inputs(t, scale, eps, n)

    def stmt(dt):
        tg = target.to(dt)
        return lambda p: O.loss_bounded_prediction(p, tg, BOUNDED_LAM, eps, t, scale != 1.0, scale)
    return loss_ref(stmt, pred)


def bounded_expect(t, scale, eps, n, variant):
    return loss_exps(bounded_ref(t, scale, eps, n), variant, BOUNDED, BOUNDED)


# ------------------------------------------------------------------ l1_sparsity
SPARSITY_N = (1000, CAP + 77)
SPARSITY_LAM = 0.3


@functools.lru_cache(maxsize=None)
def sparsity_inputs(n):
    w = torch.randn(n, generator=gen(300 + n % 1000))
    w[::7] = 0.0
    w[3] = -0.0
    return w


@functools.lru_cache(maxsize=None)
def sparsity_ref(n):
    w = sparsity_inputs(n)
    return loss_ref(lambda dt: (lambda p: O.loss_weights_sparsity([p], SPARSITY_LAM)), w)


def sparsity_expect(n, variant):
    """the kernel always ADDS its gradient: `plain` and `accum` both start from accum_buffers' gradient buffer, `accum` adds the value too"""
    r = sparsity_ref(n)
    g0, v0 = accum_buffers(r)
    val = Exp("value", v0.double() + r.v64, v0 + r.v32, POINTWISE) if variant == "accum" else Exp("value", r.v64, r.v32, POINTWISE)
    return [val] if variant == "nograd" else [val, Exp("grad", g0.double() + r.g64, g0 + r.g32, POINTWISE)]


# ------------------------------------------------------------------ sum_into
SUM_N = (1, 257, CAP + 77)


@functools.lru_cache(maxsize=None)
def sum_inputs(n):
    """values around 1e4: a float32 running sum of half a million of them has lost its low bits long before the end"""
    return 1e4 + torch.randn(n, generator=gen(400 + n % 1000))


def sum_expect(n):
    x = sum_inputs(n)
    return [Exp("sum", x.double().sum().reshape(1), x.sum().reshape(1), POINTWISE)]


# ------------------------------------------------------------------ tensor2uint82float
U8_N = (1, 257, CAP + 77)


@functools.lru_cache(maxsize=None)
def u8_inputs(n):
    """every (k + 0.5) / 255 tie, values below 0 and above 1, -0.0, then generic values in [-0.1, 1.1]"""
    special = torch.cat([torch.tensor([-0.0, -0.3, 1.7, 0.0, 1.0, -1e-9, 1 + 1e-6]), (torch.arange(255).float() + 0.5) / 255])
    x = torch.rand(n, generator=gen(500 + n % 1000)) * 1.2 - 0.1
    if n == 1:
        return torch.tensor([2.5 / 255])
    k = min(n, special.numel())
    x[:k] = special[:k]
    return x


# ------------------------------------------------------------------ ssim_loss
SSIM_WS = (3, 5, 11, 19)
SSIM_SHAPES = ((1, 1, 1), (1, 7, 5), (2, 33, 31), (1, 65, 40), (3, 32, 64))
SSIM_VARIANT_SHAPES = ((2, 33, 31), (3, 32, 64))
SSIM_KINDS = ("generic", "flat", "equal")
SSIM_LAM = 5.0


@functools.lru_cache(maxsize=None)
def ssim_inputs(shape, kind):
    """generic: target uniform, pred = target + noise (a trained net's regime); flat: pred constant (its variance and
    covariance are pure float32 cancellation; with BOTH images flat the denominator is c2 = 9e-4 plus that cancellation and the
    float32 statement itself is 1e-4 off float64: no yardstick); equal: pred == target (SSIM 1, gradient 0 in exact arithmetic)"""
    B, H, W = shape
    g = gen(600 + H * W)
    target = torch.rand(B, 1, H, W, generator=g)
    pred = target + 0.1 * torch.randn(B, 1, H, W, generator=g)
    if kind == "flat":
        pred = torch.full_like(pred, 0.4)
    elif kind == "equal":
        pred = target.clone()
    return pred, target


@functools.lru_cache(maxsize=None)
def ssim_ref(ws, shape, kind):
    pred, target = ssim_inputs(shape, kind)
    return loss_ref(lambda dt: (lambda p: O.loss_neg_ssim(p, target.to(dt), SSIM_LAM, ws)), pred)


def ssim_expect(ws, shape, kind, variant="plain"):
    """flat / equal: gated at the scale of the generic case of the same shape and window"""
    r = ssim_ref(ws, shape, kind)
    if kind == "generic":
        return loss_exps(r, variant, SSIM_VALUE, SSIM_GRAD)
    gr = ssim_ref(ws, shape, "generic")
    return loss_exps(r, variant, SSIM_VALUE, SSIM_GRAD, max(gr.v64.abs().item(), r.v64.abs().item()), gr.g64.abs().max().item())


# ------------------------------------------------------------------ metrics
METRIC_SSIM_SIZES = ((11, 11), (12, 43), (42, 42), (43, 44))     # after the border crop; valid output 1x1, 2x33, 32x32, 33x34
METRIC_SSIM_BORDERS = (0, 3, 8)
METRIC_SSIM_THS = (0, 20, 30, 100, 150, 210, 240, 300)           # 0: the whole image; 300: above every pixel
METRIC_PSNR_SHAPES = ((9, 9, 4), (5, 7, 0), (9, 11, 2), (17, 130, 0), (21, 134, 2), (96, 112, 0), (112, 128, 8))   # H, W, border
METRIC_PSNR_THS = (0, 20, 30, 64, 65, 150, 240, 300)             # image 2 is constant 64: `>= 64` all of it, `>= 65` none


def _step_target(B, H, W, border, g):
    """u8 targets with a sharp step through the middle of the cropped image: low 0..39 on one side, high 200..255 on the other
    (image 0: left | right, 1: top | bottom, 2: across the diagonal, 3 on: left | right again)"""
    h, w = H - 2 * border, W - 2 * border
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    masks = [xx >= border + w // 2, yy >= border + h // 2, (yy - border) * w >= (xx - border) * h]
    low = torch.randint(0, 40, (B, 1, H, W), generator=g)
    high = torch.randint(200, 256, (B, 1, H, W), generator=g)
    mask = torch.stack([masks[b if b < 3 else 0] for b in range(B)])[:, None]
    return torch.where(mask, high, low).float()


@functools.lru_cache(maxsize=None)
def metric_ssim_inputs(h, w, border):
    """B = 3 float images in [0, 1] (pred noisy, values beyond [0, 1] included) and their u8-ised forms"""
    H, W = h + 2 * border, w + 2 * border
    g = gen(700 + H * W + border)
    hr = _step_target(3, H, W, border, g) / 255
    pr = hr + 0.05 * torch.randn(3, 1, H, W, generator=g)
    return pr, hr, O.tensor2uint82float(pr), O.tensor2uint82float(hr)


def roi_of(b_u8, th, dtype):
    return (b_u8 >= th).to(dtype)


def metric_ssim_roi_counts(h, w, border):
    """[B, nth] ROI pixels under the valid output (the ROI cropped by the border, then by 5)"""
    _, _, _, b = metric_ssim_inputs(h, w, border)
    c = O._crop(b, border)[:, :, 5:h - 5, 5:w - 5]
    return torch.stack([(c >= th).reshape(3, -1).sum(-1) for th in METRIC_SSIM_THS], 1)


@functools.lru_cache(maxsize=None)
def metric_ssim_expect(h, w, border):
    """one Exp per slot: slot 0 no ROI, then METRIC_SSIM_THS; [B] each.  SSIM lies in [-1, 1]: gated at scale 1, the
    suite's absolute 5e-5"""
    _, _, a, b = metric_ssim_inputs(h, w, border)
    out = []
    for k, th in enumerate((None,) + METRIC_SSIM_THS):
        r64, r32 = [O.metric_ssim(a.to(dt), b.to(dt), border, None if th is None else roi_of(b, th, dt))
                    for dt in (torch.float64, torch.float32)]
        out.append(Exp(f"slot {k} (th {th})", r64, r32, METRIC_SSIM, 1.0))
    return out


@functools.lru_cache(maxsize=None)
def metric_psnr_inputs(H, W, border):
    """B = 4: 0 a step target under a noisy pred; 1 pred == target (the 1e-45 floor); 2 a constant target (den == 0 -> 1);
    3 a uniform random target"""
    g = gen(800 + H * W + border)
    hr = _step_target(4, H, W, border, g) / 255
    hr[2] = 64.0 / 255
    hr[3] = torch.randint(0, 256, (1, H, W), generator=g).float() / 255
    pr = hr + 0.05 * torch.randn(4, 1, H, W, generator=g)
    pr[1] = hr[1]
    return pr, hr, O.tensor2uint82float(pr), O.tensor2uint82float(hr)


def metric_psnr_roi_counts(H, W, border):
    _, _, _, b = metric_psnr_inputs(H, W, border)
    c = O._crop(b, border)
    return torch.stack([(c >= th).reshape(4, -1).sum(-1) for th in METRIC_PSNR_THS], 1)


@functools.lru_cache(maxsize=None)
def metric_psnr_expect(H, W, border, nth):
    """[B, 1 + nth, 4] float64 = PSNR, PSNR_Y, MSE, NRMSE as the oracle states them on the u8-ised images"""
    _, _, a, b = metric_psnr_inputs(H, W, border)
    ya, yb = O.gray_to_y(a / 255.0) * 255.0, O.gray_to_y(b / 255.0) * 255.0
    out = torch.empty(4, 1 + nth, 4, dtype=torch.float64)
    for k, th in enumerate((None,) + METRIC_PSNR_THS[:nth]):
        roi = None if th is None else roi_of(b, th, torch.float32)
        out[:, k, 0] = O.metric_psnr(a, b, border, roi)
        out[:, k, 1] = O.metric_psnr(ya, yb, border, roi)
        out[:, k, 2] = O.metric_mse(a, b, border, roi)
        out[:, k, 3] = O.metric_nrmse(a, b, border, roi)
    return out


# ------------------------------------------------------------------ loss_stencil
STENCIL_OPS = {"grad": ("grad", 3), "laplace": ("laplace", 3), "lv3": ("lv", 3), "lv5": ("lv", 5), "lv7": ("lv", 7)}
STENCIL_SHAPES = ((1, 38, 54), (2, 37, 53), (1, 1, 1), (1, 2, 9), (1, 3, 3), (1, 16, 16))
STENCIL_ACCUM_SHAPE = (2, 37, 53)
STENCIL_COMBOS = tuple((norm, cn) for norm in (1, 2) for cn in (False, True))
STENCIL_LAM = 1.5


@functools.lru_cache(maxsize=None)
def stencil_inputs(shape):
    """multiples of 1/256: every stencil sum and sum of squares is exact in float32 and float64 alike, so NORM1's sign
    agrees.  From 16 x 16 up: a flat 6 x 6 block of pred in the top-left corner (operator norm 0 -> coefficient 0) and a
    6 x 6 block of pred == target in the bottom-right one; from 32 rows up one more of each inside the tiles at (16, 16) and
    (16, 32), the interior tiles of 38 x 54"""
    B, H, W = shape
    g = gen(900 + H * W)
    pred = torch.randint(0, 257, (B, 1, H, W), generator=g).float() / 256
    target = torch.randint(0, 257, (B, 1, H, W), generator=g).float() / 256
    if H >= 16 and W >= 16:
        pred[:, :, :6, :6] = 0.5
        pred[:, :, H - 6:, W - 6:] = target[:, :, H - 6:, W - 6:]
    if H >= 32 and W >= 48:
        pred[:, :, 18:24, 20:26] = 0.25
        pred[:, :, 24:30, 36:44] = target[:, :, 24:30, 36:44]
    return pred, target


@functools.lru_cache(maxsize=None)
def stencil_ref(op, shape, norm, cn):
    kind, ksz = STENCIL_OPS[op]
    pred, target = stencil_inputs(shape)
    return loss_ref(lambda dt: (lambda p: O.loss_local_variation(p, target.to(dt), kind, STENCIL_LAM, norm, ksz, cn)), pred)


def stencil_expect(op, shape, norm, cn, variant="plain"):
    return loss_exps(stencil_ref(op, shape, norm, cn), variant, STENCIL, STENCIL)


# ------------------------------------------------------------------ loss_local_moments
MOMENTS_SHAPES = ((1, 2, 2), (1, 2, 17), (2, 17, 2), (2, 33, 31))
MOMENTS_ACCUM_SHAPE = (2, 33, 31)
MOMENTS_LAM = 0.7


@functools.lru_cache(maxsize=None)
def moments_inputs(shape):
    """targets on the 1/255 grid with flat blocks touching each border and each corner (2 x 2: the whole image, every
    reflected patch holds all four pixels); pred generic (2 x 2: three times as wide, or the mean of four KL terms, each what
    is left of 0.5 - 0.5, is a float32 sample no better than 7e-7)"""
    B, H, W = shape
    g = gen(1000 + H * W)
    pred = torch.rand(B, 1, H, W, generator=g) * (3 if H * W == 4 else 1)
    t = torch.randint(0, 256, (B, 1, H, W), generator=g).float()
    if H == 2 and W == 2:
        t[:] = 77
    elif H == 2:
        t[..., :5], t[..., W - 5:] = 10, 200
    elif W == 2:
        t[..., :5, :], t[..., H - 5:, :] = 10, 200
    else:
        t[..., :5, :5], t[..., :5, W - 5:], t[..., H - 5:, :5], t[..., H - 5:, W - 5:] = 10, 60, 110, 255
        t[..., :5, 12:18], t[..., H - 5:, 12:18], t[..., 14:20, :5], t[..., 14:20, W - 5:] = 0, 33, 128, 201
    return pred, t / 255


@functools.lru_cache(maxsize=None)
def moments_ref(shape):
    pred, target = moments_inputs(shape)
    return loss_ref(lambda dt: (lambda p: O.loss_local_moments(p, target.to(dt), MOMENTS_LAM)), pred)


def moments_expect(shape, variant="plain"):
    return loss_exps(moments_ref(shape), variant, STENCIL, STENCIL)


# ------------------------------------------------------------------ loss_hist / loss_kde
HIST_CASES = ((3, 37, 37, 300.0), (2, 117, 2, 20.0), (2, 117, 255, 5e3), (3, 37, 256, 1e5))          # B, n, bins, sigma
HIST_NORMS = ((1, 1.0), (2, 1.0), (3, 1.0), (4, 1.0), (4, O.elb_t_after(30)))                        # norm, elb_t
KDE_CASES = ((3, 37, 256, 1.0 / 255 ** 2), (2, 117, 2, 0.05), (2, 117, 37, 1e-3))                    # B, n, bins, kde_bw
KDE_NORMS = ((1, 1.0), (2, 1.0), (4, 1.0), (4, O.elb_t_after(30)))
HIST_LAM = 3.0


@functools.lru_cache(maxsize=None)
def hist_inputs(B, n):
    """target uniform; pred darker and noisy: histograms that differ in every bin (between near-equal histograms the KL value
    is a difference of near-equal logarithms, which float32 does not resolve)"""
    g = gen(1100 + B * n)
    target = torch.rand(B, 1, 1, n, generator=g)
    return (0.7 * target + 0.05 * torch.randn(B, 1, 1, n, generator=g)).clamp(0, 1), target


@functools.lru_cache(maxsize=None)
def hist_ref(B, n, bins, sigma, norm, elb_t):
    pred, target = hist_inputs(B, n)
    return loss_ref(lambda dt: (lambda p: O.loss_histogram_match(p, target.to(dt), HIST_LAM, norm, sigma, bins, elb_t)), pred)


def hist_expect(B, n, bins, sigma, norm, elb_t, variant="plain"):
    return loss_exps(hist_ref(B, n, bins, sigma, norm, elb_t), variant, HIST_VALUE, HIST_GRAD)


@functools.lru_cache(maxsize=None)
def kde_ref(B, n, bins, bw, norm, elb_t):
    pred, target = hist_inputs(B, n)
    return loss_ref(lambda dt: (lambda p: O.loss_kde_match(p, target.to(dt), HIST_LAM, norm, bw, bins, elb_t)), pred)


def kde_expect(B, n, bins, bw, norm, elb_t, variant="plain"):
    return loss_exps(kde_ref(B, n, bins, bw, norm, elb_t), variant, HIST_VALUE, HIST_GRAD)


# ------------------------------------------------------------------ optimizers
OPTIM_CONFIGS = {
    "adam": dict(kind="adam", lr0=1e-2, wd=0.0),
    "adam_wd": dict(kind="adam", lr0=1e-2, wd=1e-4),
    "sgd_m0": dict(kind="sgd", lr0=0.05, momentum=0.0, nesterov=False, wd=0.0),
    "sgd_m9": dict(kind="sgd", lr0=0.05, momentum=0.9, nesterov=False, wd=0.0),
    "sgd_m9_nesterov": dict(kind="sgd", lr0=0.05, momentum=0.9, nesterov=True, wd=0.0),
    "sgd_m9_nesterov_wd": dict(kind="sgd", lr0=0.05, momentum=0.9, nesterov=True, wd=1e-4),
}
OPTIM_N = (1, 257, CAP + 5)
OPTIM_GSCALES = (1.0, 0.25)
OPTIM_STEPS = 20
OPTIM_SKIPPED = frozenset((1, 2, 11))      # 1-based steps whose skip flag is set
OPTIM_GATED = (3, 4, 12, 20)               # gated after these steps: the first applied one, the next, the one after a skip, the last
OPTIM_HOST_LR = 123.0                      # the host lr handed to the _dc forms next to lr_dev: must be ignored


def optim_lr(cfg, step):
    """a MultiStepLR with milestones 8 and 15, gamma 0.5"""
    return cfg["lr0"] * (0.5 if step > 8 else 1.0) * (0.5 if step > 15 else 1.0)


@functools.lru_cache(maxsize=None)
def optim_inputs(n):
    """p0 [n], g [steps, n] with zeros in g"""
    g = gen(1200 + n % 1000)
    p0, gs = torch.randn(n, generator=g), torch.randn(OPTIM_STEPS, n, generator=g)
    gs[gs.abs() < 0.3] = 0.0
    return p0, gs


def optim_reference(name, n, gscale, dtype, skipped=OPTIM_SKIPPED, steps=OPTIM_STEPS):
    """torch.optim on tensors of dtype, stepping only on the steps that are not skipped; {step: {"p", "m", "v" | "buf"}} at
    the gated steps"""
    cfg = OPTIM_CONFIGS[name]
    p0, gs = optim_inputs(n)
    P = p0.to(dtype).clone().requires_grad_(True)
    if cfg["kind"] == "adam":
        opt = torch.optim.Adam([P], lr=cfg["lr0"], betas=(0.9, 0.999), eps=1e-8, weight_decay=cfg["wd"])
    else:
        opt = torch.optim.SGD([P], lr=cfg["lr0"], momentum=cfg["momentum"], nesterov=cfg["nesterov"], weight_decay=cfg["wd"])
    snaps = {}
    for s in range(1, steps + 1):
        if s not in skipped:
            opt.param_groups[0]["lr"] = optim_lr(cfg, s)
            P.grad = (gs[s - 1] * gscale).to(dtype)
            opt.step()
        if s in OPTIM_GATED or s == steps:
            st = opt.state[P]
            snap = {"p": P.detach().clone()}
            if cfg["kind"] == "adam":
                snap["m"], snap["v"] = st["exp_avg"].clone(), st["exp_avg_sq"].clone()
            elif cfg["momentum"]:
                snap["buf"] = st["momentum_buffer"].clone()
            snaps[s] = snap
    return snaps


def optim_expect(name, n, gscale, skipped=OPTIM_SKIPPED, steps=OPTIM_STEPS):
    """{step: [Exp]} (not cached: half a million elements a tensor at the largest n)"""
    r64 = optim_reference(name, n, gscale, torch.float64, skipped, steps)
    r32 = optim_reference(name, n, gscale, torch.float32, skipped, steps)
    return {s: [Exp(f"step {s} {k}", r64[s][k], r32[s][k], ELEMENTWISE) for k in r64[s]] for s in r64}


# ------------------------------------------------------------------ grad_norm_clip
CLIP_N = (1, 5, 4097)


@functools.lru_cache(maxsize=None)
def clip_inputs(n):
    return torch.randn(n, generator=gen(1300 + n)) * 0.01 + 0.02


def clip_expect(n, max_norm):
    """[norm, coef] and the scaled gradient, torch's clip_grad_norm_ as the oracle states it"""
    out = []
    for dt in (torch.float64, torch.float32):
        g = [clip_inputs(n).to(dt).clone()]
        total, coef = O.clip_grad_norm(g, max_norm)
        out.append((torch.stack([total, coef]), g[0]))
    return [Exp("norm, coef", out[0][0], out[1][0], ELEMENTWISE), Exp("g", out[0][1], out[1][1], ELEMENTWISE)]


# ------------------------------------------------------------------ element-wise kernels
ELEMENTWISE_N = (1, 257, CAP + 77)
LEAKY_ALPHAS = (0.2, 0.01)


@functools.lru_cache(maxsize=None)
def elementwise_inputs(n):
    """g generic; a generic with 0, -0.0 (and, for relu_mask, NaN) among its first entries; x for axpby"""
    gg = gen(1400 + n % 1000)
    g, a, x = torch.randn(n, generator=gg), torch.randn(n, generator=gg), torch.randn(n, generator=gg)
    if n == 1:
        a[0] = -0.0
    else:
        a[0], a[1], a[n - 1] = 0.0, -0.0, 0.0
    return g, a, x


def leaky_expect(n, alpha):
    _, a, _ = elementwise_inputs(n)
    return [Exp("leaky_relu", F.leaky_relu(a.double(), alpha), F.leaky_relu(a, alpha), ELEMENTWISE)]


def axpby_expect(n, a, b):
    """y = a * x + b * y; with b == 0 the y read is an uninitialised buffer's: it does not count (the BLAS rule, as axpby2d has it)"""
    g, _, x = elementwise_inputs(n)
    if b == 0:
        return [Exp(f"axpby a={a} b=0", a * x.double(), a * x, ELEMENTWISE)]
    return [Exp(f"axpby a={a} b={b}", a * x.double() + b * g.double(), a * x + b * g, ELEMENTWISE)]


NEAREST_CASES = ((1, 1, 1, 4), (2, 3, 5, 60), (1, 7, 2, 64))       # B, h, w, C


def nearest_up2(lo):
    """NHWC [B, h, w, C] -> [B, 2h, 2w, C], F.interpolate(mode='nearest')"""
    return F.interpolate(lo.permute(0, 3, 1, 2), scale_factor=2, mode="nearest").permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def nearest_inputs(B, h, w, C):
    g = gen(1500 + h * w * C)
    return torch.randn(B, h, w, C, generator=g), torch.randn(B, 2 * h, 2 * w, C, generator=g)


def nearest_adjoint_expect(B, h, w, C):
    lo, hi = nearest_inputs(B, h, w, C)
    out = []
    for dt in (torch.float64, torch.float32):
        x = lo.to(dt).clone().requires_grad_(True)
        out.append(torch.autograd.grad(nearest_up2(x), x, hi.to(dt))[0])
    return [Exp("adjoint", out[0], out[1], ELEMENTWISE)]
