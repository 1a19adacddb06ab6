"""What tests/test_gpu_step_kernels.py relies on in its inputs, checked on the statements alone (no GPU): the builders of
tests/step_kernel_cases.py are the ones the GPU tests run.

For every gated case the float32 statement's distance e32 from float64 is finite and below the case's ceiling / 3, so the
`3 x e32` arm of the gate, not the ceiling, is the binding one.  A case that breaks a condition here gets other inputs, never
a wider gate (tests/step_kernel_cases.py says at each builder which inputs were turned down and why)."""
import math

import numpy as np
import pytest
import torch

import sr_oracle as O
import step_kernel_cases as C


def conditioned(exps, name):
    bad = []
    for x in exps:
        assert x.ref64.dtype == torch.float64 and x.ref32.dtype == torch.float32, (name, x.what)
        assert x.ref64.shape == x.ref32.shape, (name, x.what)
        e32 = C.e32_of(x)
        if not math.isfinite(e32) or not bool(torch.isfinite(x.ref64).all()):
            bad.append(f"{name} {x.what}: e32 {e32}")
        elif not e32 < x.ceiling / 3:
            bad.append(f"{name} {x.what}: e32 {e32:.3e} >= {x.ceiling:g} / 3")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("kind", list(C.POINTWISE_KINDS))
def test_pointwise_cases(kind):
    for n in C.POINTWISE_N:
        pred, target, _ = C.pointwise_inputs(n)
        assert n < 8 or bool((pred == target).any()) and bool((pred != target).any())
        for variant in C.VARIANTS:
            conditioned(C.pointwise_expect(kind, n, variant), f"{kind} n={n} {variant}")


@pytest.mark.parametrize("t,scale,eps,n", C.BOUNDED_CASES)
def test_bounded_cases(t, scale, eps, n):
    """both branches of both barrier terms are taken, and with scale 1, eps 0 the first two elements sit exactly on the branch point"""
    pred, target = C.bounded_inputs(t, scale, eps, n)
    ct = -(1.0 / torch.tensor(t, dtype=torch.float32) ** 2)
    zr, zl = pred * scale - (target * scale + eps), target * scale - eps - pred * scale
    for z in (zr, zl):
        assert bool((z <= ct).any()) and bool((z > ct).any())
    if scale == 1.0 and eps == 0.0:
        assert zr[0] == ct and zl[1] == ct
        assert pred.double()[0] - target.double()[0] == ct.double()
    for variant in C.VARIANTS:
        conditioned(C.bounded_expect(t, scale, eps, n, variant), f"bounded {variant}")


def test_sparsity_sum_and_u8_cases():
    for n in C.SPARSITY_N:
        w = C.sparsity_inputs(n)
        assert bool((w == 0).any()) and bool((w > 0).any()) and bool((w < 0).any())
        for variant in C.VARIANTS:
            conditioned(C.sparsity_expect(n, variant), f"l1_sparsity n={n} {variant}")
    for n in C.SUM_N:
        conditioned(C.sum_expect(n), f"sum n={n}")
    x = C.sum_inputs(C.CAP + 77)
    run = float(np.cumsum(x.numpy(), dtype=np.float32)[-1])          # a float32 running sum does lose bits
    assert abs(run - float(x.double().sum())) > 1e-6 * float(x.double().sum())
    for n in C.U8_N:
        x = C.u8_inputs(n)
        assert x.numel() == n
        if n > 1:
            v = x.double() * 255
            assert bool((x < 0).any()) and bool((x > 1).any()) and bool(((v - v.floor() - 0.5).abs() < 1e-4).any())
            assert math.copysign(1.0, x[0].item()) == -1.0 and x[0] == 0              # -0.0


@pytest.mark.parametrize("ws", C.SSIM_WS)
def test_ssim_loss_cases(ws):
    for shape in C.SSIM_SHAPES:
        conditioned(C.ssim_expect(ws, shape, "generic"), f"ssim{ws} {shape}")
    for shape in C.SSIM_VARIANT_SHAPES:
        for kind in C.SSIM_KINDS:
            conditioned(C.ssim_expect(ws, shape, kind), f"ssim{ws} {shape} {kind}")
        for variant in C.VARIANTS:
            conditioned(C.ssim_expect(ws, shape, "generic", variant), f"ssim{ws} {shape} {variant}")


@pytest.mark.parametrize("border", C.METRIC_SSIM_BORDERS)
@pytest.mark.parametrize("h,w", C.METRIC_SSIM_SIZES)
def test_metric_ssim_cases(h, w, border):
    """threshold 0 takes every output pixel, 300 none, 100 some but not all wherever there is more than one"""
    cnt = C.metric_ssim_roi_counts(h, w, border)
    npix = (h - 10) * (w - 10)
    ths = C.METRIC_SSIM_THS
    assert bool((cnt[:, ths.index(0)] == npix).all()) and bool((cnt[:, ths.index(300)] == 0).all())
    if npix > 1:
        mid = cnt[:, ths.index(100)]
        assert bool(((mid > 0) & (mid < npix)).all()), mid
    conditioned(C.metric_ssim_expect(h, w, border), f"metric ssim {h}x{w} border {border}")


@pytest.mark.parametrize("H,W,border", C.METRIC_PSNR_SHAPES)
def test_metric_psnr_cases(H, W, border):
    """ROI counts: all of the image at 0 (and at 64 on the constant image), none at 300 (and at 65 on the constant image),
    in between at 150 on the step images"""
    cnt = C.metric_psnr_roi_counts(H, W, border)
    npix = (H - 2 * border) * (W - 2 * border)
    ths = C.METRIC_PSNR_THS
    assert bool((cnt[:, ths.index(0)] == npix).all()) and bool((cnt[:, ths.index(300)] == 0).all())
    assert cnt[2, ths.index(64)] == npix and cnt[2, ths.index(65)] == 0
    if npix > 1:
        assert 0 < cnt[0, ths.index(150)] < npix
    pr, hr, a, b = C.metric_psnr_inputs(H, W, border)
    assert torch.equal(a[1], b[1]) and bool((O._crop(b, border)[2] == 64).all())
    assert bool(torch.isfinite(C.metric_psnr_expect(H, W, border, 8)).all())
    assert torch.equal(C.metric_psnr_expect(H, W, border, 0)[:, 0], C.metric_psnr_expect(H, W, border, 8)[:, 0])


@pytest.mark.parametrize("shape", C.STENCIL_SHAPES)
@pytest.mark.parametrize("op", list(C.STENCIL_OPS))
def test_stencil_cases(op, shape):
    """the float32 and float64 statements agree in the gradient within 1e-5 of its largest entry"""
    for norm, cn in C.STENCIL_COMBOS:
        r = C.stencil_ref(op, shape, norm, cn)
        s = r.g64.abs().max().item() + 1e-300
        assert (r.g32.double() - r.g64).abs().max().item() / s <= 1e-5, (op, shape, norm, cn)
        conditioned(C.stencil_expect(op, shape, norm, cn), f"{op} {shape} norm {norm} cn {cn}")
        if shape == C.STENCIL_ACCUM_SHAPE:
            conditioned(C.stencil_expect(op, shape, norm, cn, "accum"), f"{op} {shape} norm {norm} cn {cn} accum")


def test_stencil_inputs_hold_a_flat_and_an_equal_block():
    pred, target = C.stencil_inputs((1, 38, 54))
    assert bool((pred * 256 == (pred * 256).round()).all()) and bool((target * 256 == (target * 256).round()).all())
    assert bool((pred[:, :, 18:24, 20:26] == 0.25).all()) and torch.equal(pred[:, :, 24:30, 36:44], target[:, :, 24:30, 36:44])
    assert bool((pred[:, :, :6, :6] == 0.5).all()) and torch.equal(pred[:, :, -6:, -6:], target[:, :, -6:, -6:])
    assert not torch.equal(pred, target)


@pytest.mark.parametrize("shape", C.MOMENTS_SHAPES)
def test_local_moments_cases(shape):
    """the set `tv == 0` is the same in float32 and float64 and is non-empty"""
    pred, target = C.moments_inputs(shape)
    assert bool(((target * 255).round() / 255 == target).all())
    flat32 = O.patch_moments(target)[1] == 0
    flat64 = O.patch_moments(target.double())[1] == 0
    assert torch.equal(flat32, flat64) and bool(flat32.any())
    if shape[1] > 2 and shape[2] > 2:
        assert not bool(flat32.all())
        m = flat32.reshape(shape)
        for corner in (m[:, 0, 0], m[:, 0, -1], m[:, -1, 0], m[:, -1, -1], m[:, 0, 14], m[:, -1, 14], m[:, 16, 0], m[:, 16, -1]):
            assert bool(corner.all())
    for variant in (C.VARIANTS if shape == C.MOMENTS_ACCUM_SHAPE else ("plain",)):
        conditioned(C.moments_expect(shape, variant), f"local_moments {shape} {variant}")


@pytest.mark.parametrize("B,n,bins,sigma", C.HIST_CASES)
def test_hist_cases(B, n, bins, sigma):
    for norm, elb_t in C.HIST_NORMS:
        conditioned(C.hist_expect(B, n, bins, sigma, norm, elb_t), f"hist norm {norm} t {elb_t}")
    conditioned(C.hist_expect(B, n, bins, sigma, 2, 1.0, "accum"), "hist accum")


@pytest.mark.parametrize("B,n,bins,bw", C.KDE_CASES)
def test_kde_cases(B, n, bins, bw):
    for norm, elb_t in C.KDE_NORMS:
        conditioned(C.kde_expect(B, n, bins, bw, norm, elb_t), f"kde norm {norm} t {elb_t}")
    conditioned(C.kde_expect(B, n, bins, bw, 2, 1.0, "accum"), "kde accum")


@pytest.mark.parametrize("name", list(C.OPTIM_CONFIGS))
def test_optimizer_cases(name):
    for n in C.OPTIM_N:
        p0, gs = C.optim_inputs(n)
        assert bool((gs == 0).any()) and bool((gs != 0).any())
        for gscale in C.OPTIM_GSCALES:
            for step, exps in C.optim_expect(name, n, gscale).items():
                conditioned(exps, f"{name} n={n} gscale={gscale}")
    cfg = C.OPTIM_CONFIGS[name]
    assert len({C.optim_lr(cfg, s) for s in range(1, C.OPTIM_STEPS + 1)}) == 3
    conditioned([x for exps in C.optim_expect(name, 257, 1.0, frozenset(), 5).values() for x in exps], f"{name} no flag")


def test_clip_and_elementwise_cases():
    for n in C.CLIP_N:
        total = float(C.clip_inputs(n).double().norm())
        conditioned(C.clip_expect(n, 0.5 * total), f"clip n={n}")               # clipped
        exps = C.clip_expect(n, 2.0 * total)                                    # under max_norm: coefficient 1
        assert exps[0].ref64[1] == 1.0 and torch.equal(exps[1].ref32, C.clip_inputs(n))
    for n in C.ELEMENTWISE_N:
        g, a, x = C.elementwise_inputs(n)
        assert bool((a == 0).any()) and math.copysign(1.0, a[min(1, n - 1)].item()) == -1.0
        for alpha in C.LEAKY_ALPHAS:
            conditioned(C.leaky_expect(n, alpha), f"leaky n={n}")
        conditioned(C.axpby_expect(n, 1.5, 0.0) + C.axpby_expect(n, 0.75, -1.25), f"axpby n={n}")
    for case in C.NEAREST_CASES:
        conditioned(C.nearest_adjoint_expect(*case), f"nearest_up2 {case}")
