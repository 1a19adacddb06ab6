"""GPU parity tests of the kernels every net's training step and evaluation end in, one entry point at a time: the loss
values and dL/dpred (misc.hip, ssim.hip, loss_ext.hip), the optimizer updates driven by the device-side step counter and the
element-wise helpers (misc.hip), the PSNR-family and SSIM metrics (small.hip, ssim.hip).  Called through srhip.ops (ops.call
on the C-ABI where a wrapper allocates the output itself), every output buffer NaN before the call, against the oracle's own
statements (oracle/sr_oracle.py), torch.optim and F.interpolate evaluated in float64 on the CPU; gradients are float64 autograd
of the statement.  tests/step_kernel_cases.py builds every input and reference; tests/test_cpu_step_kernel_inputs.py checks
the input conditions the gates below rely on.

Gate (class Gates of tests/test_gpu_tape_op_kernels.py): with e the kernel's and e32 the float32 statement's largest distance
from float64, both relative to the float64 result's largest entry and e32 floored at 2 ** -24, a test asserts
e <= min(ceiling, 3 x e32).  Ceilings are the suite's existing ones for the same kernel (tests/test_gpu_kernels.py,
tests/test_gpu_multiscale_loss.py): 1e-6 L1 / L2 / point-wise and sums, 1e-4 / 2e-4 SSIM loss value / gradient, 2e-6 stencil
and local moments, 5e-6 bounded, 2e-5 / 5e-4 hist and kde value / gradient, 2e-6 optimizers and element-wise kernels; the
metrics keep test_metrics' absolute bounds (MSE bit-equal, PSNR 1e-9, NRMSE 1e-12, PSNR_Y 1e-4, SSIM 5e-5 gated at scale 1).
Copies and index operations (tensor2uint82float, relu_mask, leaky_relu_mask, nearest_up2 forward, an unclipped
grad_norm_clip) are torch.equal.  Where the float64 result is zero or nearly so (pred == target, a flat pred under SSIM) the
scale is that of the generic case of the same shape.

Branches no earlier test reached, by entry point (each test's docstring says which case reaches which):
  loss_l1l2 / loss_pointwise  n = 1 .. 257 around one block; the grid-stride loop's second turn; sign(0); grad = NULL; Charbonnier, L2Sum directly
  loss_bounded, l1_sparsity   first direct calls: both branches of both barrier terms and the branch point; scale 255; the added gradient
  sum, tensor2uint82float     first direct calls; the rounding ties, clamps and -0.0; past the grid cap
  ssim_loss                   windows 3 and 5; images smaller than the window; ragged and exact tiles; B = 3 (`plane`); caller's workspace
  metrics_ssim                one output pixel; an exact 32x32 tile; sliver tiles; nth = 0; count 0 -> 0 / 1; the ROI at the window centre on a step
  metrics_psnr_family         blocks of k_metrics_pass with no pixel; 1 pixel; nth = 0; cnt == 0; cnt == npix (min_masked); den == 0 -> 1
  loss_stencil                the interior fast path for R = 1, 2, 3 against the oracle over the whole gradient; src_range clamped on both
                              sides; norm_lv ksz 7; norm_laplace NORM1; coefficient 0 on a flat block; sign(0) on pred == target
  loss_local_moments          2x2, 2xN, Nx2; flat target patches on every border and corner; both accumulate flags
  loss_hist / loss_kde        bins < 256 (masked lanes of k_hist_finalize); n < 64 (blocks whose slice starts past the end); B x bins odd
  optim_tick, *_step_dc       first direct calls: the skip flag, the counter after a skipped first step, first = (counter == 1), the bias
                              correction from the counter, lr_dev over the host lr, skip_flag = NULL, bit-equality with the host-count forms
  grad_norm_clip              blocks of k_sumsq_partials past the end; the unclipped gradient bit-unchanged
  relu_mask, leaky_relu(_mask), nearest_up2, axpby (b = 0), nonfinite_flag   first or second direct calls; NaN / 0 / -0.0 / +-inf placements

Factor 3 is the suite's convention for a different summation order.  Four groups exceed it for a reason of order or of a
sample of one, read as correct, and are gated at factor 10 (each stated again where it is applied):
  ssim_loss value, flat pred: one number, all of it E[x^2] - mu^2 cancellation; 5.1e-7 against 9.4e-8, ratio 5.4 (ws 19, 2x33x31)
  loss_stencil gradient at 1x1x1, 1x2x9, 1x3x3: the gather's running sum of up to 48 taps x 9 clamped sources; ratio 4.8 (lv7)
  loss_hist / loss_kde value: one number from two near-equal histograms of float32 atomic sums; ratio 7.2 (bins 2, sigma 20)
  optimizers at n = 1: one number after up to 17 updates, e32 at the floor; ratio 3.7 (adam_wd v after step 20)

Three faults these tests found are fixed with them: k_axpby computed 0 * y for b = 0, so a NaN in an uninitialised y survived
(srhip_axpby2d already skipped the read; every caller in the tree passes y = x there, so no net was hit); bin_center of the
soft histogram was fused into the subtraction x - centre, using the unrounded product where the reference's centres are
float32 values (the gradient of loss_hist was sigma x 1e-8 of its largest entry off: 4.9e-5 at sigma 5e3, 3.0e-6 at 300; at
the reference's default 1e5 the same shift is 1e-3 in the sigmoid's argument for a pixel on a bin edge); srhip_loss_hist_ws was one float short when B x bins is odd
(the last per-image double of the loss ended 4 bytes past the workspace).

Deliberate breaks tried against this file, one at a time, on a scratch build (none committed):
  src_range: `hi = n - 2` at the far border             -> 25 of the 30 test_loss_stencil cases fail
  first = (counter == 0) in k_sgd_dc                    -> every momentum case of test_optimizer_dc_steps fails (the NaN buffer)
  plane = (gridDim.z - 1) * H * W in k_ssim_loss_fwd    -> all 28 ssim_loss cases fail
  ROI centre at r + 4 in k_ssim_metric                  -> all 12 test_metrics_ssim cases fail
  interior with R in place of 2 * R                     -> nothing fails, and nothing can: tiles start at multiples of 16 >= 2 * R,
      and ty0 + 16 + R <= H already keeps every source q - off inside the image and the border row out of the tile, so the fast
      path gives the gather's sums (2 * R is merely cautious).  A real break of the predicate, `ty0 >= 0` for its lower bound,
      fails 10 cases: the 38x54 and 37x53 shapes of every operator.

Measured on an MI355X, the worst over every case of a kernel (e and e32 relative to the float64 result's largest entry, or to
the stated scale; e / e32 with e32 floored as above).  The metrics' absolute figures: PSNR 7.1e-15, PSNR_Y 3.1e-5, MSE and
NRMSE bit-equal to the oracle's.

    kernel                                         worst e worst e32 worst e / e32
    loss_pointwise / l1l2 value                    5.3e-08   1.1e-07          0.89
    loss_pointwise / l1l2 grad                     1.8e-07   1.9e-07          1.15
    loss_bounded value                             7.7e-08   9.5e-08          1.29
    loss_bounded grad                              1.9e-07   1.7e-07          1.27
    l1_sparsity value                              2.5e-08   6.0e-08          0.42
    l1_sparsity grad                               7.0e-08   7.0e-08          1.00
    sum_into                                       2.2e-08   6.0e-08          0.37
    ssim_loss value                                5.5e-07   4.9e-07          5.44
    ssim_loss grad                                 4.8e-06   9.8e-06          2.99
    metrics_ssim                                   4.5e-06   1.4e-05          2.45
    loss_stencil value                             1.1e-07   1.7e-07          1.90
    loss_stencil grad                              7.1e-07   3.1e-07          4.80
    loss_local_moments value                       1.6e-07   3.4e-07          1.26
    loss_local_moments grad                        1.5e-07   1.3e-07          1.49
    loss_hist value                                1.7e-06   1.5e-06          7.22
    loss_hist grad                                 8.0e-07   6.7e-07          2.32
    loss_kde value                                 3.0e-07   3.2e-07          5.05
    loss_kde grad                                  4.8e-07   3.0e-07          1.94
    adam_step_dc p                                 4.0e-07   4.0e-07          1.00
    adam_step_dc m                                 2.0e-07   1.9e-07          2.24
    adam_step_dc v                                 3.1e-07   3.8e-07          3.66
    sgd_step_dc p                                  3.3e-07   3.3e-07          1.00
    sgd_step_dc buf                                2.6e-07   2.7e-07          1.28
    grad_norm_clip coef                            4.1e-08   2.1e-07          0.69
    grad_norm_clip g                               8.9e-08   2.4e-07          1.00
    leaky_relu                                     7.8e-09   6.0e-08          0.13
    axpby                                          5.5e-08   7.8e-08          0.92
    nearest_up2                                    6.5e-08   6.1e-08          1.09
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import sr_oracle as O  # noqa: E402
import step_kernel_cases as C  # noqa: E402
from test_gpu_tape_op_kernels import Gates, NAN  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from srhip import ops as _ops
    return _ops


def dev(t):
    return t.cuda().contiguous()


def nan_like(t):
    return torch.full(t.shape, NAN, device="cuda")


def bits_equal(a, b):
    """bit for bit, NaN included"""
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def gate_all(G, got, exps, prefix="", factor=3):
    for x in exps:
        G(got[x.what], x.ref64, x.ref32, x.ceiling, prefix + x.what, factor=factor, scale=x.scale)


def run_loss(launch, r, variant):
    """launch(grad, loss_out, grad_accum, loss_accum) under the three variants of step_kernel_cases.loss_exps; grad and
    loss_out are NaN before a call that overwrites them"""
    if variant == "accum":
        g0, v0 = C.accum_buffers(r)
        grad, val = dev(g0.reshape(r.g64.shape)), dev(v0)
        launch(grad, val, True, True)
    else:
        grad = None if variant == "nograd" else nan_like(r.g64)
        val = torch.full((1,), NAN, device="cuda")
        launch(grad, val, False, False)
    torch.cuda.synchronize()
    return {"value": val, "grad": grad}


# ------------------------------------------------------------------ srhip_loss_l1l2, srhip_loss_pointwise
@pytest.mark.parametrize("n", C.POINTWISE_N)
@pytest.mark.parametrize("kind", list(C.POINTWISE_KINDS))
def test_loss_pointwise_and_l1l2(ops, kind, n):
    """srhip_loss_pointwise (every mode) and srhip_loss_l1l2 (L1, weighted L1, L2) against O.loss_l1 / loss_l2 /
    loss_charbonnier / loss_l2sum.  n = 1, 255, 256, 257: one block, partly filled / full / one element into a second; n =
    2048 * 256 + 77: past the grid cap, so the grid-stride loop takes a second turn in 77 threads.  A stretch of pred == target
    (sign(0) = 0); grad = NULL; both accumulate flags onto non-zero buffers."""
    mode, eps, weighted = C.POINTWISE_KINDS[kind]
    pred, target, weight = (dev(t) for t in C.pointwise_inputs(n))
    w = weight if weighted else None
    r = C.pointwise_ref(kind, n)
    entries = [("pointwise", lambda g, v, ga, la: ops.loss_pointwise(pred, target, mode, C.POINTWISE_LAM, eps or 1e-9, w, g, v, ga, la))]
    if mode <= 1:
        entries.append(("l1l2", lambda g, v, ga, la: ops.loss_l1l2(pred, target, mode, C.POINTWISE_LAM, w, g, v, ga, la)))
    with Gates(f"loss_{kind} n={n}") as G:
        for name, launch in entries:
            for variant in C.VARIANTS:
                gate_all(G, run_loss(launch, r, variant), C.pointwise_expect(kind, n, variant), f"{name} {variant} ")


# ------------------------------------------------------------------ srhip_loss_bounded
@pytest.mark.parametrize("t,scale,eps,n", C.BOUNDED_CASES)
def test_loss_bounded(ops, t, scale, eps, n):
    """srhip_loss_bounded against O.loss_bounded_prediction: t = 1, the value after 40 updates and the cap 10; scale 1 and 255
    (restore_range); eps 0 and 0.01; elements on the branch point z == -1 / t^2 of either barrier term, inside the band and far
    outside it (both branches of both terms are taken: tests/test_cpu_step_kernel_inputs.py); n past the grid cap once."""
    pred, target = (dev(x) for x in C.bounded_inputs(t, scale, eps, n))
    r = C.bounded_ref(t, scale, eps, n)
    with Gates(f"loss_bounded t={t:.4g} scale={scale:g} eps={eps:g} n={n}") as G:
        for variant in C.VARIANTS:
            got = run_loss(lambda g, v, ga, la: ops.loss_bounded(pred, target, C.BOUNDED_LAM, eps, t, scale, g, v, ga, la), r, variant)
            gate_all(G, got, C.bounded_expect(t, scale, eps, n, variant), variant + " ")


# ------------------------------------------------------------------ srhip_l1_sparsity
@pytest.mark.parametrize("n", C.SPARSITY_N)
def test_l1_sparsity(ops, n):
    """srhip_l1_sparsity against O.loss_weights_sparsity: zeros and -0.0 in w (sign 0); the gradient is ADDED to a non-zero
    buffer in every call; loss_accum; grad = NULL"""
    w = dev(C.sparsity_inputs(n))
    r = C.sparsity_ref(n)
    g0, v0 = C.accum_buffers(r)
    with Gates(f"l1_sparsity n={n}") as G:
        for variant in C.VARIANTS:
            grad = None if variant == "nograd" else dev(g0)
            val = dev(v0) if variant == "accum" else torch.full((1,), NAN, device="cuda")
            ops.l1_sparsity(w, C.SPARSITY_LAM, grad, val, loss_accum=variant == "accum")
            gate_all(G, {"value": val, "grad": grad}, C.sparsity_expect(n, variant), variant + " ")


# ------------------------------------------------------------------ srhip_sum
@pytest.mark.parametrize("n", C.SUM_N)
def test_sum_into(ops, n):
    """srhip_sum sums in double: values around 1e4, whose float32 running sum has lost its low bits long before the end"""
    out = torch.full((1,), NAN, device="cuda")
    ops.sum_into(dev(C.sum_inputs(n)), out)
    with Gates(f"sum_into n={n}") as G:
        gate_all(G, {"sum": out}, C.sum_expect(n))


# ------------------------------------------------------------------ srhip_tensor2uint82float
@pytest.mark.parametrize("n", C.U8_N)
def test_tensor2uint82float(ops, n):
    """srhip_tensor2uint82float bit for bit against O.tensor2uint82float: the (k + 0.5) / 255 ties (round half to even),
    values below 0 and above 1, -0.0; n past the grid cap"""
    x = C.u8_inputs(n)
    out = torch.full((n,), NAN, device="cuda")
    ops.call("srhip_tensor2uint82float", dev(x).data_ptr(), out.data_ptr(), n, ops._st())
    with Gates(f"tensor2uint82float n={n}") as G:
        G.equal(out, O.tensor2uint82float(x), "u8")
        G.equal(ops.tensor2uint82float(dev(x)), out, "the wrapper")


# ------------------------------------------------------------------ srhip_ssim_loss
def _ssim_launch(ops, pred, target, ws, workspace=None):
    return lambda g, v, ga, la: ops.ssim_loss(pred, target, ws, C.SSIM_LAM, g, v, ga, la, workspace)


@pytest.mark.parametrize("shape", C.SSIM_SHAPES)
@pytest.mark.parametrize("ws", C.SSIM_WS)
def test_ssim_loss(ops, ws, shape):
    """srhip_ssim_loss against O.loss_neg_ssim at windows 3, 5, 11, 19: 1x1x1; 1x7x5 (smaller than the larger windows: every
    tap row meets the zero padding); 2x33x31 and 1x65x40 (one past / one short of a 32-pixel tile edge: a tile of one row, a
    tile 8 wide); 3x32x64 (exact tiles; B = 3: the `plane` stride of the three gradient maps)"""
    pred, target = (dev(t) for t in C.ssim_inputs(shape, "generic"))
    with Gates(f"ssim_loss ws={ws} {shape}") as G:
        got = run_loss(_ssim_launch(ops, pred, target, ws), C.ssim_ref(ws, shape, "generic"), "plain")
        gate_all(G, got, C.ssim_expect(ws, shape, "generic"))


@pytest.mark.parametrize("shape", C.SSIM_VARIANT_SHAPES)
@pytest.mark.parametrize("ws", C.SSIM_WS)
def test_ssim_loss_flat_equal_and_flags(ops, ws, shape):
    """srhip_ssim_loss: a flat pred and pred == target, gated at the generic case's scale; grad = NULL; both accumulate flags
    onto non-zero buffers; a caller-owned workspace of exactly srhip_ssim_loss_ws elements, the NaN guard behind it untouched"""
    B, H, W = shape
    with Gates(f"ssim_loss ws={ws} {shape}") as G:
        for kind in ("flat", "equal"):
            pred, target = (dev(t) for t in C.ssim_inputs(shape, kind))
            got = run_loss(_ssim_launch(ops, pred, target, ws), C.ssim_ref(ws, shape, kind), "plain")
            exps = C.ssim_expect(ws, shape, kind)
            # the value is ONE number: with a flat pred it is all cancellation, and the float32 statement's distance is a sample
            # of one (9.4e-8 at ws 19, 2x33x31, where the kernel's separable 19 + 19 taps give 5.1e-7: ratio 5.4) -- factor 10
            gate_all(G, got, exps[:1], kind + " ", factor=10 if kind == "flat" else 3)
            gate_all(G, got, exps[1:], kind + " ")
        pred, target = (dev(t) for t in C.ssim_inputs(shape, "generic"))
        r = C.ssim_ref(ws, shape, "generic")
        for variant in ("nograd", "accum"):
            gate_all(G, run_loss(_ssim_launch(ops, pred, target, ws), r, variant), C.ssim_expect(ws, shape, "generic", variant), variant + " ")
        nws = ops.lib.srhip_ssim_loss_ws(B, H, W)
        buf = torch.full((nws + 64,), NAN, device="cuda")
        got = run_loss(_ssim_launch(ops, pred, target, ws, buf[:nws]), r, "plain")
        gate_all(G, got, C.ssim_expect(ws, shape, "generic"), "own workspace ")
        G.true(bool(torch.isnan(buf[nws:]).all()), "the guard behind the workspace was written")


# ------------------------------------------------------------------ srhip_metrics_ssim
def _call_metrics_ssim(ops, E, Hh, border, ths, u8):
    B, (H, W) = E.shape[0], E.shape[-2:]
    nth = len(ths)
    th = torch.tensor(list(ths) or [0], dtype=torch.int32, device="cuda")
    ws = torch.full((2 * B * (nth + 1),), NAN, dtype=torch.float64, device="cuda")
    out = torch.full((B, nth + 1), NAN, device="cuda")
    ops.call("srhip_metrics_ssim", E.data_ptr(), Hh.data_ptr(), B, H, W, border, th.data_ptr(), nth, int(u8), ws.data_ptr(),
             out.data_ptr(), ops._st())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("border", C.METRIC_SSIM_BORDERS)
@pytest.mark.parametrize("h,w", C.METRIC_SSIM_SIZES)
def test_metrics_ssim(ops, h, w, border):
    """srhip_metrics_ssim against O.metric_ssim, B = 3.  Cropped sizes 11x11 (one output pixel), 12x43 (2x33: a tile of one
    column), 42x42 (32x32: exactly one tile), 43x44 (33x34: four tiles, three of them slivers), each under border 0, 3, 8.
    Eight thresholds: 0 takes the whole image, 300 nothing (count 0 -> the 0 / 1 rule), the others cut the target's sharp step,
    so a ROI read one pixel off the window centre moves the masked mean; nth = 0; inputs_are_u8 both ways.  The output buffer
    [B, 1 + nth] is ONE comparison: a slot is a mean over as few as one pixel of a map whose float32 error is 1e-5 a pixel
    (E[x^2] - mu^2 on the bright side of the step), so the float32 statement's distance in a single slot of three images is a
    sample -- at 12x43, border 0 it is 1.1e-7 in the slot next to one where it is 1.4e-5."""
    pr, hr, a, b = (dev(t) for t in C.metric_ssim_inputs(h, w, border))
    exps = C.metric_ssim_expect(h, w, border)
    ref64, ref32 = torch.stack([x.ref64 for x in exps], 1), torch.stack([x.ref32 for x in exps], 1)
    with Gates(f"metrics_ssim {h}x{w} border={border}") as G:
        for name, E, Hh, u8 in (("float", pr, hr, False), ("u8", a, b, True)):
            out = _call_metrics_ssim(ops, E, Hh, border, C.METRIC_SSIM_THS, u8)
            for k, x in enumerate(exps):                              # slot by slot, for the record
                print(f"[slot] {G.name} {name} {x.what}: kernel {(out[:, k].double().cpu() - x.ref64).abs().max():.3e} "
                      f"fp32 {(x.ref32.double() - x.ref64).abs().max():.3e}")
            G(out, ref64, ref32, C.METRIC_SSIM, name + " [B, 9]", scale=1.0)
            empty = C.METRIC_SSIM_THS.index(300) + 1
            G.equal(out[:, empty], torch.zeros(3), name + ": the empty ROI is 0 / 1")
        # nth = 0: the one slot stands in the place of slot 0 of the nine above (the same double sums in another order)
        out0 = _call_metrics_ssim(ops, pr, hr, border, (), False)
        G.true(out0.shape == (3, 1), "nth = 0: one slot")
        G(torch.cat([out0, out[:, 1:]], 1), ref64, ref32, C.METRIC_SSIM, "nth = 0 [B, 1] in place of slot 0", scale=1.0)
        G.true((out0[:, 0] - out[:, 0]).abs().max().item() <= 2.0 ** -23, "nth = 0 differs from slot 0 of nth = 8 by more than a rounding")


# ------------------------------------------------------------------ srhip_metrics_psnr_family
def _call_metrics_psnr(ops, E, Hh, border, ths, u8):
    B, (H, W) = E.shape[0], E.shape[-2:]
    nth = len(ths)
    th = torch.tensor(list(ths) or [0], dtype=torch.int32, device="cuda")
    ws = torch.full((ops.lib.srhip_metrics_ws(B, nth),), NAN, dtype=torch.float64, device="cuda")
    out = torch.full((B, nth + 1, 4), NAN, dtype=torch.float64, device="cuda")
    ops.call("srhip_metrics_psnr_family", E.data_ptr(), Hh.data_ptr(), B, H, W, border, th.data_ptr(), nth, int(u8), ws.data_ptr(),
             out.data_ptr(), ops._st())
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("nth", (0, 8))
@pytest.mark.parametrize("H,W,border", C.METRIC_PSNR_SHAPES)
def test_metrics_psnr_family(ops, H, W, border, nth):
    """srhip_metrics_psnr_family against O.metric_psnr / metric_mse / metric_nrmse (PSNR_Y through O.gray_to_y): 1 pixel after
    the crop (9x9, border 4), 5x7 with and without a border, 17x130, 96x112 -- all but the last have fewer pixels than the 64 x
    256 threads of k_metrics_pass, so whole blocks see no pixel.  Image 1 is pred == target (the 1e-45 floor), image 2 a
    constant target (den == 0 -> 1; `>= 64` covers it all: cnt == npix takes the other min_masked branch of k_metrics_fin; `>=
    65` is an empty ROI).  Already-u8 inputs give the same bits."""
    pr, hr, a, b = (dev(t) for t in C.metric_psnr_inputs(H, W, border))
    ths = C.METRIC_PSNR_THS[:nth]
    ref = C.metric_psnr_expect(H, W, border, nth)
    out = _call_metrics_psnr(ops, pr, hr, border, ths, False)
    with Gates(f"metrics_psnr_family {H}x{W} border={border} nth={nth}") as G:
        G.true(out.shape == ref.shape and bool(torch.isfinite(out).all()), "a slot was not written")
        for k, th in enumerate((None,) + ths):
            e = (out[:, k] - ref[:, k]).abs().max(0)[0]
            print(f"[metric] {G.name} th {th}: psnr {e[0]:.3e} psnr_y {e[1]:.3e} mse {e[2]:.3e} nrmse {e[3]:.3e}")
            G.equal(out[:, k, 2], ref[:, k, 2], f"mse th={th}")                 # integer sums: exact
            G.true(e[0].item() < 1e-9, f"psnr th={th}: {e[0]:.3e}")
            G.true(e[3].item() < 1e-12, f"nrmse th={th}: {e[3]:.3e}")
            G.true(e[1].item() < 1e-4, f"psnr_y th={th}: {e[1]:.3e}")
        G.true(abs(out[1, 0, 0].item() - 498.1308) < 1e-3, "pred == target: the PSNR of the 1e-45 floor")
        G.equal(_call_metrics_psnr(ops, a, b, border, ths, True), out, "already-u8 inputs")


# ------------------------------------------------------------------ srhip_loss_stencil
@pytest.mark.parametrize("shape", C.STENCIL_SHAPES)
@pytest.mark.parametrize("op", list(C.STENCIL_OPS))
def test_loss_stencil(ops, op, shape):
    """srhip_loss_stencil against O.loss_local_variation, the WHOLE gradient, for NORM1 / NORM2 x plain / channel-norm.  Tiles
    are 16 x 16; a tile is `interior` (the compile-time fast path) when 2R <= ty0 and ty0 + 16 + 2R <= H, likewise in x.
    1x38x54: the tiles at (16, 16) and (16, 32) are interior for every R up to 3 (lv7); 2x37x53: none for R = 3, the one at (16,
    16) and (16, 32) for R = 1 and R = 2 (lv5: 16 + 16 + 4 <= 37), and an image border inside the batch; 1x1x1, 1x2x9, 1x3x3:
    narrower than the radius, src_range clamps on both sides at once; 1x16x16: one tile, no halo tile.  Inputs are multiples of
    1/256 with a flat block of pred (operator norm 0 -> coefficient 0) and a block of pred == target (NORM1's sign(0)); at
    2x37x53 also both accumulate flags.  Factor 10 at the three shapes narrower than the radius: there a pixel's gradient is
    the gather's running float32 sum of up to 48 taps x 9 clamped sources, signed and cancelling, where autograd adds channel
    by channel; measured e / e32 = 4.8 (lv7, 1x3x3, channel-norm NORM2: 5.9e-7 against 1.2e-7), 3.1 at lv5."""
    kind, ksz = C.STENCIL_OPS[op]
    pred, target = (dev(t) for t in C.stencil_inputs(shape))
    with Gates(f"loss_stencil {op} {shape}") as G:
        for norm, cn in C.STENCIL_COMBOS:
            r = C.stencil_ref(op, shape, norm, cn)
            for variant in (("plain", "accum") if shape == C.STENCIL_ACCUM_SHAPE else ("plain",)):
                got = run_loss(lambda g, v, ga, la: ops.loss_stencil(pred, target, kind, C.STENCIL_LAM, norm, ksz, cn, g, v, ga, la), r, variant)
                gate_all(G, got, C.stencil_expect(op, shape, norm, cn, variant), f"norm{norm} {'chan-norm ' if cn else ''}{variant} ",
                         factor=10 if shape[1] < 16 else 3)


# ------------------------------------------------------------------ srhip_loss_local_moments
@pytest.mark.parametrize("shape", C.MOMENTS_SHAPES)
def test_loss_local_moments(ops, shape):
    """srhip_loss_local_moments against O.loss_local_moments, the whole gradient: 1x2x2 (every patch is the whole image
    reflected), 1x2x17 and 2x17x2 (one dimension reflects on both sides of every pixel), 2x33x31 (tiles of one row / 15
    columns).  Targets on the 1/255 grid with flat blocks touching each border and each corner: only those patches count."""
    pred, target = (dev(t) for t in C.moments_inputs(shape))
    r = C.moments_ref(shape)
    with Gates(f"loss_local_moments {shape}") as G:
        for variant in (C.VARIANTS if shape == C.MOMENTS_ACCUM_SHAPE else ("plain",)):
            got = run_loss(lambda g, v, ga, la: ops.loss_local_moments(pred, target, C.MOMENTS_LAM, g, v, ga, la), r, variant)
            gate_all(G, got, C.moments_expect(shape, variant), variant + " ")


# ------------------------------------------------------------------ srhip_loss_hist, srhip_loss_kde
# The VALUE of either loss is one number, a norm of the difference of two near-equal histograms whose bins are float32 atomic sums
# in arrival order; the float32 statement's distance from float64 is a sample of one and sits at the 2 ** -24 floor where the
# kernel's is a few roundings: measured e / e32 = 7.2 (hist, bins 2, sigma 20, NORM2 accumulated), 5.1 (kde, bins 2).  Order alone: factor 10 for the value, 3 for every gradient.
VALUE_FACTOR = 10


@pytest.mark.parametrize("norm,elb_t", C.HIST_NORMS)
@pytest.mark.parametrize("B,n,bins,sigma", C.HIST_CASES)
def test_loss_hist(ops, B, n, bins, sigma, norm, elb_t):
    """srhip_loss_hist against O.loss_histogram_match.  bins 37, 2, 255 < 256: lanes k >= bins of k_hist_finalize are masked;
    n = 37 < 64 blocks per image: per = 1, the slices of blocks 37 .. 63 of k_soft_hist start past the end; n = 117: per = 2,
    blocks 59 .. 63 likewise; sigma 300 .. 5e3: every pixel reaches several bins; sigma 1e5 (the reference's own): only the
    neighbours.  The cases at sigma 300 and 5e3 are the ones that caught the bin centres' fused multiply-add (bin_center in
    loss_ext.hip): the gradient was sigma x 1e-8 of its largest entry off, 4.9e-5 at 5e3 against a float32 statement at 4e-7.
    With B x bins odd (3 x 37) the last per-image double must still end inside srhip_loss_hist_ws floats."""
    pred, target = (dev(t) for t in C.hist_inputs(B, n))
    r = C.hist_ref(B, n, bins, sigma, norm, elb_t)
    with Gates(f"loss_hist B={B} n={n} bins={bins} sigma={sigma:g} norm={norm} t={elb_t:.4g}") as G:
        for variant in (C.VARIANTS if norm == 2 else ("plain",)):
            got = run_loss(lambda g, v, ga, la: ops.loss_hist(pred, target, C.HIST_LAM, norm, sigma, bins, g, v, ga, la, elb_t), r, variant)
            exps = C.hist_expect(B, n, bins, sigma, norm, elb_t, variant)
            gate_all(G, got, exps[:1], variant + " ", factor=VALUE_FACTOR)
            gate_all(G, got, exps[1:], variant + " ")
        # a caller-owned workspace of exactly srhip_loss_hist_ws floats: with B * bins odd (3 x 37) the per-image doubles sit one
        # float further back, and the last of them must still end inside it
        nws = ops.lib.srhip_loss_hist_ws(B, bins)
        buf = torch.full((nws + 64,), NAN, device="cuda")
        grad, val = nan_like(r.g64), torch.full((1,), NAN, device="cuda")
        ops.call("srhip_loss_hist", pred.data_ptr(), target.data_ptr(), grad.data_ptr(), val.data_ptr(), buf.data_ptr(), B, n, bins,
                 float(sigma), norm, C.HIST_LAM, 0, 0, float(elb_t), ops._st())
        torch.cuda.synchronize()
        exps = C.hist_expect(B, n, bins, sigma, norm, elb_t)
        gate_all(G, {"value": val}, exps[:1], "own workspace ", factor=VALUE_FACTOR)
        gate_all(G, {"grad": grad}, exps[1:], "own workspace ")
        G.true(bool(torch.isnan(buf[nws:]).all()), "the guard behind the workspace was written")


@pytest.mark.parametrize("norm,elb_t", C.KDE_NORMS)
@pytest.mark.parametrize("B,n,bins,bw", C.KDE_CASES)
def test_loss_kde(ops, B, n, bins, bw, norm, elb_t):
    """srhip_loss_kde against O.loss_kde_match: the reference's own bandwidth 1 / 255^2 at 256 bins, and 2 and 37 bins under
    bandwidths at which every pixel reaches every bin; n = 37 and 117 as in test_loss_hist"""
    pred, target = (dev(t) for t in C.hist_inputs(B, n))
    r = C.kde_ref(B, n, bins, bw, norm, elb_t)
    with Gates(f"loss_kde B={B} n={n} bins={bins} bw={bw:.3g} norm={norm} t={elb_t:.4g}") as G:
        for variant in (C.VARIANTS if norm == 2 else ("plain",)):
            got = run_loss(lambda g, v, ga, la: ops.loss_kde(pred, target, C.HIST_LAM, norm, bw, bins, g, v, ga, la, elb_t), r, variant)
            exps = C.kde_expect(B, n, bins, bw, norm, elb_t, variant)
            gate_all(G, got, exps[:1], variant + " ", factor=VALUE_FACTOR)
            gate_all(G, got, exps[1:], variant + " ")


# ------------------------------------------------------------------ srhip_optim_tick, srhip_adam_step_dc, srhip_sgd_step_dc
class _OptimRun:
    """device state of one optimizer run: the _dc form on (p, m, v | buf) and the host-count form on a twin"""

    def __init__(self, ops, name, n, gscale, use_flag):
        self.ops, self.cfg, self.gscale, self.use_flag = ops, C.OPTIM_CONFIGS[name], gscale, use_flag
        p0, self.gs = C.optim_inputs(n)
        adam = self.cfg["kind"] == "adam"
        # Adam's moments start at 0; SGD's buffer is NaN until the first APPLIED step initialises it
        self.state = [dev(p0)] + ([torch.zeros(n).cuda(), torch.zeros(n).cuda()] if adam else [torch.full((n,), NAN, device="cuda")])
        self.twin = [t.clone() for t in self.state]
        self.counter = torch.zeros(1, dtype=torch.int32).cuda()
        self.flag = torch.zeros(1, dtype=torch.int32).cuda() if use_flag else None
        self.lr_dev = torch.zeros(1).cuda()
        self.applied = 0

    def step(self, s, skip):
        ops, cfg = self.ops, self.cfg
        if self.use_flag:
            self.flag.fill_(int(skip))
        lr = C.optim_lr(cfg, s)
        self.lr_dev.fill_(lr)
        g = dev(self.gs[s - 1])
        self.applied += not skip
        ops.optim_tick(self.flag, self.counter)
        if cfg["kind"] == "adam":
            ops.adam_step_dc(*self.state[:1], g, *self.state[1:], self.counter, C.OPTIM_HOST_LR, wd=cfg["wd"], gscale=self.gscale,
                             skip_flag=self.flag, lr_dev=self.lr_dev)
            ops.adam_step(*self.twin[:1], g, *self.twin[1:], max(self.applied, 1), lr, wd=cfg["wd"], gscale=self.gscale,
                          skip_flag=self.flag)
        else:
            ops.sgd_step_dc(self.state[0], g, self.state[1], self.counter, C.OPTIM_HOST_LR, cfg["momentum"], cfg["wd"],
                            cfg["nesterov"], self.gscale, self.flag, self.lr_dev)
            ops.sgd_step(self.twin[0], g, self.twin[1], lr, cfg["momentum"], cfg["wd"], cfg["nesterov"], self.applied == 1,
                         self.gscale, self.flag)
        torch.cuda.synchronize()

    def got(self, s):
        names = ("p", "m", "v") if self.cfg["kind"] == "adam" else ("p", "buf")
        return {f"step {s} {k}": t for k, t in zip(names, self.state)}


@pytest.mark.parametrize("gscale", C.OPTIM_GSCALES)
@pytest.mark.parametrize("n", C.OPTIM_N)
@pytest.mark.parametrize("name", list(C.OPTIM_CONFIGS))
def test_optimizer_dc_steps(ops, name, n, gscale):
    """srhip_optim_tick + srhip_adam_step_dc / srhip_sgd_step_dc over 20 steps against torch.optim.Adam / SGD stepping only on
    the steps that are not skipped (float64 tensors the reference, float32 tensors the yardstick): p and m, v / buf gated after
    steps 3, 4, 12 and 20.  Steps 1, 2 and 11 carry a set skip flag: p, m, v / buf and the counter stay bit-unchanged, so step 3
    is the first applied one -- the counter is 1 there, Adam's bias correction is that of step 1 and SGD's momentum buffer, NaN
    until then, is initialised (first = (counter == 1)).  The learning rate is read from lr_dev, which halves after steps 8 and
    15; the host value passed beside it is 123 and must be ignored.  Zeros in g; gscale 1 and 0.25; n = 1, 257 and past the grid
    cap.  At every step the _dc form is bit-equal to srhip_adam_step / srhip_sgd_step given the applied-step count, `first` and
    the learning rate from the host."""
    run = _OptimRun(ops, name, n, gscale, True)
    expect = C.optim_expect(name, n, gscale)
    with Gates(f"{name} n={n} gscale={gscale:g}") as G:
        for s in range(1, C.OPTIM_STEPS + 1):
            skip = s in C.OPTIM_SKIPPED
            before = [t.clone() for t in run.state] if skip else None
            run.step(s, skip)
            G.true(run.counter.item() == run.applied, f"step {s}: counter {run.counter.item()} after {run.applied} applied steps")
            for k, (a, b) in enumerate(zip(run.state, run.twin)):
                G.true(bits_equal(a, b), f"step {s}: the _dc form differs from the host-count form in buffer {k}")
            if skip:
                for k, (a, b) in enumerate(zip(run.state, before)):
                    G.true(bits_equal(a, b), f"skipped step {s} changed buffer {k}")
            if s in expect:
                got = run.got(s)
                if "step %d buf" % s in got and not C.OPTIM_CONFIGS[name]["momentum"]:
                    G.true(bool(torch.isnan(got.pop(f"step {s} buf")).all()), "momentum 0 touched the buffer")
                # n = 1: one number after up to 17 updates, each a rounding or two; the float32 statement's distance is a sample of
                # one (0 in places).  Measured e / e32 = 3.7 (adam_wd, gscale 0.25, v after step 20: 2.2e-7): factor 10 there
                gate_all(G, got, expect[s], factor=10 if n == 1 else 3)


@pytest.mark.parametrize("name", list(C.OPTIM_CONFIGS))
def test_optimizer_dc_steps_without_a_flag(ops, name):
    """skip_flag = NULL: optim_tick counts every step and the _dc forms apply every one"""
    run = _OptimRun(ops, name, 257, 1.0, False)
    expect = C.optim_expect(name, 257, 1.0, frozenset(), 5)
    with Gates(f"{name} no flag") as G:
        for s in range(1, 6):
            run.step(s, False)
            G.true(run.counter.item() == s, f"step {s}: counter {run.counter.item()}")
            for k, (a, b) in enumerate(zip(run.state, run.twin)):
                G.true(bits_equal(a, b), f"step {s}: the _dc form differs from the host-count form in buffer {k}")
            if s in expect:
                got = run.got(s)
                if not C.OPTIM_CONFIGS[name].get("momentum", 1):
                    got.pop(f"step {s} buf")
                gate_all(G, got, expect[s])


# ------------------------------------------------------------------ srhip_grad_norm_clip
@pytest.mark.parametrize("n", C.CLIP_N)
def test_grad_norm_clip_small(ops, n):
    """srhip_grad_norm_clip where test_grad_norm_clip_and_ema_kernels does not go: n = 1 and 5 (every block of k_sumsq_partials
    but the first two starts past the end), 4097 (slices of 8: blocks 513 .. 1023 do).  A gradient under max_norm comes back
    bit-unchanged with coefficient exactly 1."""
    g0 = C.clip_inputs(n)
    total = float(g0.double().norm())
    with Gates(f"grad_norm_clip n={n}") as G:
        g, nc = dev(g0), torch.full((2,), NAN, device="cuda")
        ops.grad_norm_clip(g, 1.0, 0.5 * total, nc)
        gate_all(G, {"norm, coef": nc, "g": g}, C.clip_expect(n, 0.5 * total), "clipped ")
        g, nc = dev(g0), torch.full((2,), NAN, device="cuda")
        ops.grad_norm_clip(g, 1.0, 2.0 * total, nc)
        exps = C.clip_expect(n, 2.0 * total)
        G(nc, exps[0].ref64, exps[0].ref32, exps[0].ceiling, "unclipped norm, coef")
        G.true(nc[1].item() == 1.0, "unclipped: coefficient not exactly 1")
        G.equal(g, g0, "unclipped: the gradient changed")


# ------------------------------------------------------------------ element-wise kernels
@pytest.mark.parametrize("n", C.ELEMENTWISE_N)
def test_relu_and_leaky_kernels(ops, n):
    """srhip_relu_mask (a holds 0, -0.0 and NaN: all masked, as g * (a > 0) would), srhip_leaky_relu_mask (bit-equal to the
    float32 product) and srhip_leaky_relu at alpha 0.2 and 0.01; n past the grid cap"""
    g, a, _ = C.elementwise_inputs(n)
    with Gates(f"relu / leaky n={n}") as G:
        an = a.clone()
        an[n // 2] = NAN
        zero = torch.zeros(())
        G.equal(ops.relu_mask(dev(g), dev(an)), torch.where(an > 0, g, zero), "relu_mask")
        for alpha in C.LEAKY_ALPHAS:
            fa = torch.tensor(alpha, dtype=torch.float32)
            G.equal(ops.leaky_relu_mask(dev(g), dev(a), alpha), torch.where(a > 0, g, g * fa), f"leaky_relu_mask {alpha}")
            gate_all(G, {"leaky_relu": ops.leaky_relu_(dev(a), alpha)}, C.leaky_expect(n, alpha), f"alpha {alpha} ")


@pytest.mark.parametrize("n", C.ELEMENTWISE_N)
def test_axpby(ops, n):
    """srhip_axpby: y = a x + b y; with b = 0 a NaN-filled y does not count (y is then an output only, as srhip_axpby2d has it)"""
    g, _, x = C.elementwise_inputs(n)
    with Gates(f"axpby n={n}") as G:
        y = torch.full((n,), NAN, device="cuda")
        ops.axpby(y, dev(x), 1.5, 0.0)
        gate_all(G, {"axpby a=1.5 b=0": y}, C.axpby_expect(n, 1.5, 0.0))
        y = dev(g)
        ops.axpby(y, dev(x), 0.75, -1.25)
        gate_all(G, {"axpby a=0.75 b=-1.25": y}, C.axpby_expect(n, 0.75, -1.25))


@pytest.mark.parametrize("n", C.ELEMENTWISE_N)
def test_nonfinite_flag(ops, n):
    """srhip_nonfinite_flag: +inf, -inf and NaN each as the only bad value, at the first and at the last element; a clean
    input leaves a 0 flag 0 and a flag that is already 1 at 1"""
    g, _, _ = C.elementwise_inputs(n)
    with Gates(f"nonfinite_flag n={n}") as G:
        flag = torch.zeros(1, dtype=torch.int32).cuda()
        ops.nonfinite_flag(dev(g), flag)
        G.true(flag.item() == 0, "clean input raised the flag")
        for bad in (math.inf, -math.inf, NAN):
            for at in (0, n - 1):
                x = g.clone()
                x[at] = bad
                flag.zero_()
                ops.nonfinite_flag(dev(x), flag)
                G.true(flag.item() == 1, f"{bad} at {at} not flagged")
        ops.nonfinite_flag(dev(g), flag)
        G.true(flag.item() == 1, "a clean input cleared a flag that was 1")


@pytest.mark.parametrize("B,h,w,C_", C.NEAREST_CASES)
def test_nearest_up2(ops, B, h, w, C_):
    """srhip_nearest_up2_nhwc: forward bit-equal to F.interpolate(mode='nearest'); the adjoint (four values added in a fixed
    order) gated against float64 autograd of the same statement"""
    lo, hi = C.nearest_inputs(B, h, w, C_)
    with Gates(f"nearest_up2 {(B, h, w, C_)}") as G:
        G.equal(ops.nearest_up2(dev(lo), nan_like(hi)), C.nearest_up2(lo), "forward")
        out = nan_like(lo)
        ops.nearest_up2(out, dev(hi), adjoint=True)
        gate_all(G, {"adjoint": out}, C.nearest_adjoint_expect(B, h, w, C_))
