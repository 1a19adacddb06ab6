"""The fp16-storage conv kernels (conv_h16.hip, conv_h16_bwd.hip) at the tile forms real launches take, one entry point at a
time against float64 on the SAME fp16-exact operands: the 8-row tile (RW = 4) of k_conv3x3_h16 / k_conv1x1_h16 with every
epilogue, the PixelShuffle(2) store and read, the BatchNorm-ReLU prologue, two column slices, partly empty last tiles, two
images and pitched views; the 1x1 form's stage edges (1, 2, 3 and 3 + 2 chunks); k_wgrad_h16 with runs of unequal length, a
single run and half-empty tile rows (batched, ps2, shared); the head / tail convs and the 1-channel weight gradient past
their grid caps (the grid-stride form).  tests/test_gpu_conv_h16.py and the kernel tests of test_gpu_amp_train*.py cover the
small forms (RW = 2, equal runs, one pass).

The arm is asserted: rw_of() restates sr_conv3x3_h16's tile rule, the weight-gradient cases ask the library's own plan for S,
the capped cases restate the grid rule -- a case whose shape stops reaching its arm fails instead of testing the other one.

Reference: float64 on the device, a 3x3 conv as nine shifted matmuls (conv_ref), the weight gradient as an im2col GEMM
(_wgrad_ref).  Gates are the suite's own: check_h16 (|ref| 2^-10 + refabs 2^-20 + 2^-24) for fp16 outputs, check_f32
(refabs 2^-18) for G / dW / db, relative 1e-5 for the tail conv.  Every gate prints its figure (worst error / tolerance)
before it asserts.

The in_bn prologue is relu((x - mean) k + beta) in f32, rounded to fp16.  Its operands here lie on grids (x, mean, beta
multiples of 2^-8, k of 2^-4) on which that expression is exact in f32 however the compiler contracts it, so the fp16 value
the kernel stages and the one the reference rounds are the same number and the gate keeps its width.

Two counts differ from the hand-worked ones the cases were planned with, and the cases say so where they assert:
  * srhip_conv3x3_wgrad_shared_h16_plan allows 64 runs, not 16: at (3, 22, 50), 2 problems of 128 x 128 it returns S = 18 over
    36 tiles (equal runs).  That shape runs with the plan's S and, through the C-ABI, with S = 16 (runs of 2 and 3); a third
    shape, (3, 18, 70) -> 45 tiles, S = 22, gets unequal runs from the plan itself.
  * 728 x 728 IS a multiple of 32, so the tail conv's last group of that image is whole; 727 x 729 (16562 blocks wanted,
    odd pixel count) adds the partial last group in a strided pass.

sr_conv_cout1_h16 at Cin = 1024 asks for 67,584 bytes of dynamic LDS (above 64 KiB) without a hipFuncSetAttribute call: on
an MI355X (160 KiB of LDS per CU) the runtime takes that launch as it is and the result matches float64 (table below), so the
entry point's `Cin <= 1024` stands and test_cout1_h16_cin_1024 keeps the case.

Measured on an MI355X, worst error as a fraction of the gate over every comparison of a kernel and arm:

    kernel, arm                                                       gate                  worst / gate
    k_conv3x3_h16<4>  epilogues 0, 1, 2, 8, 6 (2 x 250 x 250)         check_h16             0.498
    k_conv3x3_h16<4>  epilogue 2 on pitched views                     check_h16             0.498
    k_conv3x3_h16<4>  in_bn prologue + bias                           check_h16             0.497
    k_conv3x3_h16<4>  epilogue 9, two column slices                   check_h16             0.496
    k_conv3x3_h16<4>  epilogue 10 (mode 0) out / G                    check_h16 / _f32      0.494 / 0.016
    k_conv3x3_h16<4>  epilogue 11 (mode 1) out                        check_h16             0.495
    k_conv3x3_h16<4>  PixelShuffle(2) store + bias                    check_h16             0.496
    k_conv3x3_h16<4>  PixelShuffle(2) read, K = 256                   check_h16             0.492
    k_conv1x1_h16<4>  5 chunks, with / without in_bn                  check_h16             0.498 / 0.497
    k_conv1x1_h16<2>  Cin 32, 64, 96, 160, with / without in_bn       check_h16             0.496 / 0.498
    k_wgrad_h16  S = 1 of 1 tile, dW / db                             check_f32             0.032 / 0.000
    k_wgrad_h16  S = 4 of 9 tiles, dW / db                            check_f32             0.021 / 0.000
    k_wgrad_h16  ps2, S = 4 of 9 tiles, dW / db                       check_f32             0.016 / 0.000
    k_wgrad_h16  S = 16 of 36 tiles, 3 problems, dW / db              check_f32             0.009 / 0.002
    k_wgrad_h16  shared, S = 18 / 16 of 36, 22 of 45 tiles, dW / db   check_f32             0.006 / 0.001
    k_cin1_h16  capped: bias + ReLU, LeakyReLU, flip, flip + mask     check_h16             0.499
    k_cin1_h16  Co = 8 / Co = 1024                                    check_h16             0.481 / 0.497
    k_cout1_h16  capped, 728 x 728 / 727 x 729, bias + add            1e-5 relative         0.018 / 0.016
    k_cout1_h16  capped, 728 x 728 / 727 x 729, in_bn                 1e-5 relative         0.017 / 0.016
    k_cout1_h16  Cin = 1024, bias + add / in_bn                       1e-5 relative         0.031 / 0.060
    k_cin1_wgrad_h16  capped, C = 64 / 8 / 256, dW                    check_f32             0.010 / 0.002 / 0.017
    k_cin1_wgrad_h16  capped, C = 64 / 8 / 256, db                    check_f32             0.004 / 0.001 / 0.004

(0.5 of check_h16 is the final rounding to fp16 alone.)  No case needed the float32-statement fallback: the widest
contractions (K = 256 x 9, Cin = 160, Cin = 1024) stay where the narrow ones are.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def h(t):
    """fp16-exact f32 copy (operands both sides share)."""
    return t.half().float()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def packs(w, ps2=False):
    """fp16x2 forward / data-gradient packs of a conv weight [Co,Ci,3,3] (leading plane = what the h16 kernels read)."""
    from srhip import ops
    Co, Ci = w.shape[:2]
    ws = ops.WeightSet()
    tb = ops.PrepTable()
    tb.conv(w, ws.planes("wp", 9 * Co, Ci, w.device), ps2=ps2, force_f16=True)
    tb.conv(w, ws.planes("wpt", 9 * Ci, Co, w.device), data_grad=True, ps2=ps2, force_f16=True)
    tb.build(w.device).run()
    return ws["wp"], ws["wpt"], tb


def pack_fwd(w):
    """the forward pack alone (Cin no multiple of 64: the data-gradient pack of such a weight does not exist)"""
    from srhip import ops
    Co, Ci = w.shape[:2]
    ws = ops.WeightSet()
    tb = ops.PrepTable()
    tb.conv(w, ws.planes("wp", 9 * Co, Ci, w.device), force_f16=True)
    tb.build(w.device).run()
    return ws["wp"], tb


def check_h16(out, ref, refabs):
    """fp16 output within one fp16 rounding of the float64 result (+ the f32 accumulation's share)."""
    err = (out.double() - ref).abs()
    tol = ref.abs() * 2.0 ** -10 + refabs * 2.0 ** -20 + 2.0 ** -24
    assert bool((err <= tol).all()), f"max excess {(err - tol).max().item():.3e}"


def check_f32(out, ref, refabs):
    """f32 results of an f32 accumulation of exact fp16 products: within a few f32 ulps of the sum of magnitudes."""
    err = (out.double() - ref).abs()
    tol = refabs * 2.0 ** -18 + 1e-30
    assert bool((err <= tol).all()), f"max excess {(err - tol).max().item():.3e} (max err {err.max().item():.3e})"


def gate_h16(tag, out, ref, refabs):
    """check_h16, with the figure printed first: the worst error as a fraction of its tolerance"""
    err = (out.double() - ref).abs()
    tol = ref.abs() * 2.0 ** -10 + refabs * 2.0 ** -20 + 2.0 ** -24
    print(f"MEAS {tag}: {(err / tol).max().item():.3f} of check_h16")
    check_h16(out, ref, refabs)


def gate_f32(tag, out, ref, refabs):
    err = (out.double() - ref).abs()
    tol = refabs * 2.0 ** -18 + 1e-30
    print(f"MEAS {tag}: {(err / tol).max().item():.3f} of check_f32")
    check_f32(out, ref, refabs)


def gate_tail(tag, y, ref):
    """the tail conv's gate (tests/test_gpu_conv_h16.py): 1e-5 of the largest result"""
    rel = ((y.double() - ref).abs().max() / ref.abs().max()).item()
    print(f"MEAS {tag}: {rel / 1e-5:.3f} of 1e-5 relative")
    assert rel < 1e-5, rel


def cdiv(a, b):
    return (a + b - 1) // b


def rw_of(B, H, W, Cout):
    """sr_conv3x3_h16's tile rule: 8-row tiles (RW = 4) from 1024 of them on, 4-row tiles (RW = 2) below"""
    return 4 if cdiv(W, 16) * cdiv(H, 8) * B * (Cout // 64) >= 1024 else 2


def f32v(a):
    """the float the kernel gets for a Python scalar, as a float64"""
    return torch.tensor(a, dtype=torch.float32).double().item()


def leaky_scale(v, a):
    """what a LeakyReLU multiplies its argument (and that argument's error) by"""
    return torch.where(v > 0, torch.ones_like(v), torch.full_like(v, a))


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def randn(g, *shape):
    return torch.randn(*shape, device="cuda", generator=g)


def conv_ref(x, w, center_only=False):
    """3x3 conv, stride 1, zero padding, float64 NHWC: x [B,H,W,Ci], w [Co,Ci,3,3] -> the result and the same contraction of
    the magnitudes, [B,H,W,Co] each.  Nine shifted matmuls (aten's float64 conv is the slow step at these sizes)."""
    x, w = x.double(), w.double()
    B, H, W, Ci = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    xa = xp.abs()
    out = torch.zeros(B, H, W, w.shape[0], dtype=torch.float64, device=x.device)
    outabs = torch.zeros_like(out)
    for ky in range(3):
        for kx in range(3):
            if center_only and (ky, kx) != (1, 1):
                continue
            wt = w[:, :, ky, kx].t().contiguous()
            out += xp[:, ky:ky + H, kx:kx + W, :] @ wt
            outabs += xa[:, ky:ky + H, kx:kx + W, :] @ wt.abs()
    return out, outabs


def dgrad_w(w):
    """the weight of the data gradient as a forward conv: taps mirrored, channels transposed"""
    return w.double().flip(2, 3).transpose(0, 1)


def _wgrad_ref(dY, X):
    """dW [Co,Ci,3,3], db [Co] and their magnitude sums in float64 (im2col GEMM on the GPU)."""
    B, Ci, H, W = X.shape
    Co = dY.shape[1]
    cols = F.unfold(X.double(), 3, padding=1)                      # [B, Ci*9, H*W]
    dy = dY.double().reshape(B, Co, H * W)
    dw = torch.einsum("bok,bck->oc", dy, cols).reshape(Co, Ci, 3, 3)
    dwa = torch.einsum("bok,bck->oc", dy.abs(), cols.abs()).reshape(Co, Ci, 3, 3)
    return dw, dy.sum((0, 2)), dwa, dy.abs().sum((0, 2))


def bn_operands(g, shape, Cin):
    """x and the prologue's coefficient rows [mean, rstd, k, beta] on grids that make relu((x - mean) k + beta) exact in f32
    (module docstring), and that activation rounded to fp16 as the kernel stages it"""
    x = (torch.round(randn(g, *shape, Cin) * 256.0) / 256.0).clamp(-7.5, 7.5)
    mean = torch.round(randn(g, Cin) * 0.3 * 256.0) / 256.0
    k = torch.randint(8, 32, (Cin,), device="cuda", generator=g).float() / 16.0
    beta = torch.round(randn(g, Cin) * 0.2 * 256.0) / 256.0
    coef = torch.stack([mean, torch.ones_like(k), k, beta]).contiguous()
    assert torch.equal(x.half().float(), x)
    act = torch.relu((x - coef[0]) * coef[2] + coef[3])
    assert torch.equal(act.double(), torch.relu((x.double() - mean.double()) * k.double() + beta.double()))
    return x.half(), coef, act.half()


# ------------------------------------------------------------------------------ A. srhip_conv3x3_nhwc_h16 at RW = 4
def test_conv3x3_rw4_epilogues_two_images_partial_last_tiles_and_pitched_views():
    """2 x 250 x 250, 64 -> 64: 16 x 32 x 2 = 1024 tiles of 8 x 16; the last tile column has 10 of 16 pixels, the last tile
    row 2 of 8: block row 31 ends image 0 on two rows and the next one begins image 1."""
    from srhip import ops
    B, H, W, Cin, Cout = 2, 250, 250, 64, 64
    assert rw_of(B, H, W, Cout) == 4 and H % 8 == 2 and W % 16 == 10
    g = gen(101)
    x = randn(g, B, H, W, Cin).half()
    w = h(randn(g, Cout, Cin, 3, 3) * 0.05)
    b = randn(g, Cout) * 0.1
    r = randn(g, B, H, W, Cout).half()
    wp, _, _keep = packs(w)
    pre, preabs = conv_ref(x, w)
    bd, rd = b.double(), r.double()
    gate_h16("conv3x3 RW=4 epi 0", ops.conv3x3_h16(x, wp, None, Cout), pre, preabs)
    gate_h16("conv3x3 RW=4 epi 1 + bias", ops.conv3x3_h16(x, wp, b, Cout, epi=1), torch.relu(pre + bd), preabs + bd.abs())
    a1 = f32v(0.1)
    ref2, ref2abs = rd + a1 * (pre + bd), rd.abs() + a1 * (preabs + bd.abs())
    gate_h16("conv3x3 RW=4 epi 2 + bias", ops.conv3x3_h16(x, wp, b, Cout, epi=2, R=r, alpha=0.1), ref2, ref2abs)
    gate_h16("conv3x3 RW=4 epi 8", ops.conv3x3_h16(x, wp, None, Cout, epi=8, R=r), torch.relu(rd + pre), rd.abs() + preabs)
    a2 = f32v(0.2)
    v = pre + bd
    gate_h16("conv3x3 RW=4 epi 6 + bias", ops.conv3x3_h16(x, wp, b, Cout, epi=6, alpha=0.2), torch.where(v > 0, v, a2 * v),
             leaky_scale(v, a2) * (preabs + bd.abs()))
    # pitched views: 8 spare halves per pixel in X, R and out; the kernel writes none of the output's
    xb = torch.full((B, H, W, Cin + 8), 77.0, device="cuda", dtype=torch.float16)
    rb = torch.full((B, H, W, Cout + 8), 77.0, device="cuda", dtype=torch.float16)
    ob = torch.full((B, H, W, Cout + 8), float("nan"), device="cuda", dtype=torch.float16)
    xb[..., :Cin] = x
    rb[..., :Cout] = r
    out = ops.conv3x3_h16(xb[..., :Cin], wp, b, Cout, out=ob[..., :Cout], epi=2, R=rb[..., :Cout], alpha=0.1)
    assert out.data_ptr() == ob.data_ptr() and out.stride(2) == Cout + 8
    gate_h16("conv3x3 RW=4 epi 2, pitched", ob[..., :Cout], ref2, ref2abs)
    assert bool(torch.isnan(ob[..., Cout:]).all())


def test_conv3x3_rw4_bn_prologue():
    from srhip import ops
    B, H, W, Cin, Cout = 2, 250, 250, 64, 64
    assert rw_of(B, H, W, Cout) == 4
    g = gen(102)
    x, coef, act = bn_operands(g, (B, H, W), Cin)
    w = h(randn(g, Cout, Cin, 3, 3) * 0.05)
    b = randn(g, Cout) * 0.1
    wp, _, _keep = packs(w)
    pre, preabs = conv_ref(act, w)
    gate_h16("conv3x3 RW=4 in_bn + bias", ops.conv3x3_h16(x, wp, b, Cout, in_bn=coef), pre + b.double(), preabs + b.double().abs())


def test_conv3x3_rw4_two_column_slices_and_the_masked_data_gradients_with_G():
    """DRRN's width, 1 x 250 x 250, 128 -> 128: 16 x 32 x 2 column slices = 1024 blocks (the block index walks the slices
    first), four chunks.  Epilogue 9, then srhip_conv3x3_dgrad_relu_acc_h16 mode 0 (twice: every element belongs to one
    thread, a difference between two runs is a race) and mode 1, G read, modified and written in f32."""
    from srhip import ops
    B, H, W, C = 1, 250, 250, 128
    assert rw_of(B, H, W, C) == 4
    g = gen(103)
    w = h(randn(g, C, C, 3, 3) * 0.03)
    _, wpt, _keep = packs(w)
    gy = randn(g, B, H, W, C).half()
    R = torch.relu(randn(g, B, H, W, C)).half()
    G0 = randn(g, B, H, W, C)
    ref, refabs = conv_ref(gy, dgrad_w(w))
    m = (R > 0).double()
    a = f32v(0.1)
    gate_h16("conv3x3 RW=4 epi 9, 2 slices", ops.conv3x3_h16(gy, wpt, None, C, epi=9, R=R, alpha=0.1), ref * m * a, refabs * a)
    runs = []
    for _ in range(2):
        G = G0.clone()
        out = torch.full((B, H, W, C), float("nan"), device="cuda", dtype=torch.float16)
        ops.conv3x3_dgrad_relu_acc_h16(gy, wpt, R, out, G, mode=0)
        runs.append((out, G))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    out, G = runs[0]
    gate_h16("conv3x3 RW=4 epi 10 out", out, ref * m, refabs)
    gate_f32("conv3x3 RW=4 epi 10 G", G, G0.double() + out.double(), G0.double().abs() + out.double().abs())
    G = G0.clone()
    out = torch.full((B, H, W, C), float("nan"), device="cuda", dtype=torch.float16)
    ops.conv3x3_dgrad_relu_acc_h16(gy, wpt, R, out, G, mode=1)
    gate_h16("conv3x3 RW=4 epi 11 out", out, (ref + G0.double()) * m, refabs + G0.double().abs())
    assert torch.equal(G, G0)                                      # mode 1 only reads G


def test_conv3x3_rw4_pixelshuffle2_store_with_bias():
    """1 x 125 x 250, 64 -> 256 through PixelShuffle(2): 16 x 16 x 4 column slices = 1024 blocks; kernel column
    sp (N / 4) + cc takes bias[(cc) 4 + sp] and goes to sub-pixel sp of [1, 250, 500, 64]."""
    from srhip import ops
    B, H, W, Cin, Cout = 1, 125, 250, 64, 256
    assert rw_of(B, H, W, Cout) == 4
    g = gen(104)
    x = randn(g, B, H, W, Cin).half()
    w = h(randn(g, Cout, Cin, 3, 3) * 0.05)
    b = randn(g, Cout) * 0.1
    wp, _, _keep = packs(w, ps2=True)
    pre, preabs = conv_ref(x, w)

    def shuffle(t):
        return F.pixel_shuffle(t.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    out = ops.conv3x3_h16(x, wp, b, Cout, ps2=True)
    assert tuple(out.shape) == (B, 2 * H, 2 * W, Cout // 4)
    gate_h16("conv3x3 RW=4 ps store + bias", out, shuffle(pre + b.double()), shuffle(preabs + b.double().abs()))


def test_conv3x3_rw4_pixelshuffle2_read():
    """The upsampler's data gradient (srhip_conv3x3_ps2_bwd_data_h16): out 1 x 256 x 500, K = 4 x 64 -> 64, 32 x 32 = 1024
    blocks, read from the shuffled gradient [1, 512, 1000, 64]; the last tile column has 4 of 16 pixels."""
    from srhip import ops
    B, H, W, Fc = 1, 256, 500, 64
    assert rw_of(B, H, W, Fc) == 4 and W % 16 == 4
    g = gen(105)
    w = h(randn(g, 4 * Fc, Fc, 3, 3) * 0.05)
    _, wpt, _keep = packs(w, ps2=True)
    dup = randn(g, B, 2 * H, 2 * W, Fc).half()
    dc = F.pixel_unshuffle(dup.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)      # gradient of the conv's output, torch channel order
    ref, refabs = conv_ref(dc, dgrad_w(w))
    out = torch.full((B, H, W, Fc), float("nan"), device="cuda", dtype=torch.float16)
    ops.conv3x3_ps2_bwd_data_h16(dup, wpt, out)
    gate_h16("conv3x3 RW=4 ps_in (K = 256)", out, ref, refabs)


def _center_weight(g, Cout, Cin):
    w1 = torch.zeros(Cout, Cin, 3, 3, device="cuda")
    w1[:, :, 1, 1] = h(randn(g, Cout, Cin) / Cin ** 0.5)
    return w1


def test_conv1x1_rw4_five_chunks():
    """k_conv1x1_h16<4>: 2 x 250 x 250, 160 -> 64 = 1024 blocks, five 32-channel chunks (one full stage of three, then two)."""
    from srhip import ops
    B, H, W, Cin, Cout = 2, 250, 250, 160, 64
    assert rw_of(B, H, W, Cout) == 4
    g = gen(106)
    x, coef, act = bn_operands(g, (B, H, W), Cin)
    w1 = _center_weight(g, Cout, Cin)
    wp, _keep = pack_fwd(w1)
    ref, refabs = conv_ref(act, w1, center_only=True)
    gate_h16("conv1x1 RW=4 in_bn, 5 chunks", ops.conv3x3_h16(x, wp, None, Cout, in_bn=coef, center_only=True), ref, refabs)
    ref, refabs = conv_ref(x, w1, center_only=True)
    gate_h16("conv1x1 RW=4, 5 chunks", ops.conv3x3_h16(x, wp, None, Cout, center_only=True), ref, refabs)


@pytest.mark.parametrize("Cin", [32, 64, 96, 160])
def test_conv1x1_rw2_stage_edges(Cin):
    """one chunk, two, three exactly (a full stage) and 3 + 2, with and without the prologue"""
    from srhip import ops
    B, H, W, Cout = 2, 18, 20, 64
    assert rw_of(B, H, W, Cout) == 2
    g = gen(200 + Cin)
    x, coef, act = bn_operands(g, (B, H, W), Cin)
    w1 = _center_weight(g, Cout, Cin)
    b = randn(g, Cout) * 0.1
    wp, _keep = pack_fwd(w1)
    ref, refabs = conv_ref(act, w1, center_only=True)
    gate_h16(f"conv1x1 RW=2 in_bn, Cin {Cin}", ops.conv3x3_h16(x, wp, b, Cout, in_bn=coef, center_only=True),
             ref + b.double(), refabs + b.double().abs())
    ref, refabs = conv_ref(x, w1, center_only=True)
    gate_h16(f"conv1x1 RW=2, Cin {Cin}", ops.conv3x3_h16(x, wp, b, Cout, center_only=True), ref + b.double(), refabs + b.double().abs())


# ------------------------------------------------------------------------------ B. the fp16 weight gradients
def _plan(n, B, H, W, Cout, Cin, ps2=False, shared=False):
    from srhip import ops
    S, per = ctypes.c_int(0), ctypes.c_long(0)
    if shared:
        ops.call("srhip_conv3x3_wgrad_shared_h16_plan", n, B, H, W, Cout, Cin, ctypes.addressof(S), ctypes.addressof(per))
    else:
        ops.call("srhip_conv3x3_wgrad_h16_plan", n, B, H, W, Cout, Cin, int(ps2), ctypes.addressof(S), ctypes.addressof(per))
    assert per.value == S.value * Cout * (9 * Cin + 1)
    return S.value, B * cdiv(H, 4) * cdiv(W, 32)


@pytest.mark.parametrize("B,H,W,n,Cout,Cin,ps2,S,ntiles", [
    (1, 4, 32, 1, 64, 64, False, 1, 1),            # the floor of the plan: one tile, one run
    (1, 10, 72, 1, 64, 64, False, 4, 9),           # runs of 2, 2, 2, 3; last tile row half empty, last tile column 8 of 32
    (1, 10, 72, 1, 256, 64, True, 4, 9),           # the same through the shuffled dY [1, 20, 144, 64]
    (3, 22, 50, 3, 128, 64, False, 16, 36),        # runs of 2 and 3, image borders inside runs
])
def test_wgrad_h16_unequal_runs(B, H, W, n, Cout, Cin, ps2, S, ntiles):
    from srhip import ops
    assert _plan(n, B, H, W, Cout, Cin, ps2=ps2) == (S, ntiles)
    assert S == 1 or ntiles % S != 0
    assert ntiles == 1 or (H % 4 != 0 and W % 32 != 0)
    g = gen(300 + W + Cout + n)
    items, refs = [], []
    for _ in range(n):
        X = h(torch.relu(randn(g, B, Cin, H, W)))
        if ps2:
            dup = h(randn(g, B, Cout // 4, 2 * H, 2 * W) * 0.01)
            dY, dYk = F.pixel_unshuffle(dup, 2), nhwc(dup).half()
        else:
            dY = h(randn(g, B, Cout, H, W) * 0.01)
            dYk = nhwc(dY).half()
        dW = torch.full((Cout, Cin, 3, 3), float("nan"), device="cuda")
        db = torch.full((Cout,), float("nan"), device="cuda")
        items.append((dYk, nhwc(X).half(), dW, db))
        refs.append(_wgrad_ref(dY, X))
    ops.conv3x3_wgrad_h16(items, ps2=ps2)
    tag = f"wgrad_h16{' ps2' if ps2 else ''} S={S} of {ntiles} tiles"
    for (_, _, dW, db), (rw, rb, rwa, rba) in zip(items, refs):
        gate_f32(tag + " dW", dW, rw, rwa)
        gate_f32(tag + " db", db, rb, rba)


@pytest.mark.parametrize("B,H,W,S_plan,ntiles,S_forced,equal_runs", [
    (3, 22, 50, 18, 36, None, True),     # the plan's own S here: 18 equal runs of two tiles (the shared plan allows 64 runs)
    (3, 22, 50, 18, 36, 16, False),      # ... and S = 16 through the C-ABI: runs of 2 and 3, image borders inside runs
    (3, 18, 70, 22, 45, None, False),    # unequal runs from the plan itself: 21 of 2 and one of 3; 6 of 32 in the last column
])
def test_wgrad_shared_h16_three_applications(B, H, W, S_plan, ntiles, S_forced, equal_runs):
    """two problems of 128 x 128 per launch; the first application overwrites (dW, db prefilled with NaN), two add; the
    reference is the float64 sum over the three"""
    from srhip import ops
    n, C = 2, 128
    assert _plan(n, B, H, W, C, C, shared=True) == (S_plan, ntiles)
    S = S_forced or S_plan
    assert (ntiles % S == 0) == equal_runs
    assert H % 4 != 0 and W % 32 != 0
    g = gen(400 + W + S)
    dWs = [torch.full((C, C, 3, 3), float("nan"), device="cuda") for _ in range(n)]
    dbs = [torch.full((C,), float("nan"), device="cuda") for _ in range(n)]
    acc = [[torch.zeros(s, dtype=torch.float64, device="cuda") for s in ((C, C, 3, 3), (C,), (C, C, 3, 3), (C,))] for _ in range(n)]
    part = torch.empty(n * S * C * (9 * C + 1), device="cuda") if S_forced else None
    for k in range(3):
        items = []
        for j in range(n):
            X = h(torch.relu(randn(g, B, C, H, W)))
            dY = h(randn(g, B, C, H, W) * 0.01)
            items.append((nhwc(dY).half(), nhwc(X).half(), dWs[j], dbs[j]))
            for a, r in zip(acc[j], _wgrad_ref(dY, X)):
                a += r
        if S_forced:
            arr = (ops._ConvWgradH16Item * n)()
            for j, (dY, X, dW, db) in enumerate(items):
                arr[j].dY, arr[j].X, arr[j].dW, arr[j].db = dY.data_ptr(), X.data_ptr(), dW.data_ptr(), db.data_ptr()
            ops.call("srhip_conv3x3_wgrad_shared_h16", ctypes.addressof(arr), n, C, C, B, H, W, C, C, part.data_ptr(), S, int(k > 0),
                     torch.cuda.current_stream().cuda_stream)
        else:
            ops.conv3x3_wgrad_shared_h16(items, accumulate=k > 0)
    tag = f"wgrad_shared_h16 S={S} of {ntiles} tiles"
    for j in range(n):
        gate_f32(tag + " dW", dWs[j], acc[j][0], acc[j][2])
        gate_f32(tag + " db", dbs[j], acc[j][1], acc[j][3])


# ------------------------------------------------------------------------------ C. head and tail at their grid caps
def _cin1_blocks(B, H, W, Co):
    return B * H * W * (Co // 8) // 256 + 1


def _head_ref(x, w, b=None):
    """1 -> Co conv of the f32 image x [B,H,W] in float64, NHWC, and its magnitude sum"""
    ref, refabs = conv_ref(x[..., None], w)
    if b is not None:
        ref, refabs = ref + b.double(), refabs + b.double().abs()
    return ref, refabs


def test_cin1_h16_past_the_grid_cap():
    """1 x 520 x 512, Co = 64: 8321 blocks wanted, 8192 launched -- the last 129 blocks' pixels come in a second pass"""
    from srhip import ops
    B, H, W, Co = 1, 520, 512, 64
    assert _cin1_blocks(B, H, W, Co) == 8321 > 8192
    g = gen(501)
    x = torch.rand(B, H, W, device="cuda", generator=g)
    w = randn(g, Co, 1, 3, 3) / 3.0
    b = randn(g, Co) * 0.1
    ref, refabs = _head_ref(x, w, b)
    gate_h16("cin1_h16 capped, bias + ReLU", ops.conv3x3_cin1_h16(x, w, b, Co, relu=True), torch.relu(ref), refabs)
    ref, refabs = _head_ref(x, w)
    a = f32v(0.2)
    gate_h16("cin1_h16 capped, LeakyReLU", ops.conv3x3_cin1_h16(x, w, None, Co, leaky=0.2), torch.where(ref > 0, ref, a * ref),
             leaky_scale(ref, a) * refabs)
    # the tail's data gradient: f32 dy through the mirrored taps of w [1,Co,3,3]
    dy = randn(g, B, H, W) * 100.0
    wt = randn(g, 1, Co, 3, 3) * 0.05
    ref, refabs = conv_ref(dy[..., None], dgrad_w(wt))
    gate_h16("cin1_h16 capped, flip", ops.conv3x3_cin1_h16_flip(dy, wt, Co), ref, refabs)
    R = torch.relu(randn(g, B, H, W, Co)).half()
    out = torch.full((B, H, W, Co), float("nan"), device="cuda", dtype=torch.float16)
    G = torch.full((B, H, W, Co), float("nan"), device="cuda")
    ops.conv3x3_cin1_h16_flip_mask(dy, wt, R, out, G)
    gate_h16("cin1_h16 capped, flip + mask", out, ref * (R > 0).double(), refabs)
    assert torch.equal(G, out.float())


@pytest.mark.parametrize("Co", [8, 1024])
def test_cin1_h16_ends_of_the_accepted_widths(Co):
    from srhip import ops
    g = gen(510 + Co)
    x = torch.rand(2, 11, 13, device="cuda", generator=g)
    w = randn(g, Co, 1, 3, 3) / 3.0
    b = randn(g, Co) * 0.1
    ref, refabs = _head_ref(x, w, b)
    gate_h16(f"cin1_h16 Co = {Co}", ops.conv3x3_cin1_h16(x, w, b, Co, relu=True), torch.relu(ref), refabs)


def _tail_case(g, B, H, W, Ci):
    x = randn(g, B, H, W, Ci).half()
    w = h(randn(g, 1, Ci, 3, 3) / (3.0 * Ci ** 0.5))
    b = torch.tensor([0.05], device="cuda")
    add = torch.rand(B, H, W, device="cuda", generator=g)
    return x, w, b, add


@pytest.mark.parametrize("H,W,blocks", [(728, 728, 16563), (727, 729, 16562)])
def test_cout1_h16_past_the_grid_cap(H, W, blocks):
    """16384 blocks launched for more wanted: the rest of the pixels come in a second pass.  728 x 728 ends on a whole group
    of 32 pixels, 727 x 729 on a partial one (the `pix < n + 31` loop keeps its eight-lane groups together)."""
    from srhip import ops
    B, Ci = 1, 64
    n = B * H * W
    assert n // 32 + 1 == blocks > 16384 and (n % 32 != 0) == (H == 727)
    g = gen(520 + H)
    x, w, b, add = _tail_case(g, B, H, W, Ci)
    ref, _ = conv_ref(x, w)
    gate_tail(f"cout1_h16 capped {H}x{W}, bias + add", ops.conv3x3_cout1_h16(x, w, b, add=add), ref[..., 0] + b.double() + add.double())
    xq, coef, _ = bn_operands(g, (B, H, W), Ci)
    act = torch.relu((xq.double() - coef[0].double()) * coef[2].double() + coef[3].double())      # not rounded: the tail keeps f32
    ref, _ = conv_ref(act, w)
    gate_tail(f"cout1_h16 capped {H}x{W}, in_bn", ops.conv3x3_cout1_h16(xq, w, None, in_bn=coef), ref[..., 0])


def test_cout1_h16_cin_1024():
    """The widest Cin the entry point accepts: 12 Cin 4 + 9 Cin 2 = 67,584 bytes of dynamic LDS."""
    from srhip import ops
    B, H, W, Ci = 2, 11, 13, 1024
    assert 12 * Ci * 4 + 9 * Ci * 2 == 67584 > 65536
    g = gen(530)
    x, w, b, add = _tail_case(g, B, H, W, Ci)
    ref, _ = conv_ref(x, w)
    gate_tail("cout1_h16 Cin = 1024, bias + add", ops.conv3x3_cout1_h16(x, w, b, add=add), ref[..., 0] + b.double() + add.double())
    xq, coef, _ = bn_operands(g, (B, H, W), Ci)
    act = torch.relu((xq.double() - coef[0].double()) * coef[2].double() + coef[3].double())
    ref, _ = conv_ref(act, w)
    gate_tail("cout1_h16 Cin = 1024, in_bn", ops.conv3x3_cout1_h16(xq, w, None, in_bn=coef), ref[..., 0])


@pytest.mark.parametrize("C,H,W", [(64, 91, 91), (8, 257, 256), (256, 46, 45)])
@pytest.mark.parametrize("flip", [False, True])
def test_cin1_wgrad_h16_past_the_block_cap(C, H, W, flip):
    """sr_conv_cin1_wgrad_h16 gives a block npl = 4 * (64 / (C / 8)) pixels per pass and at most 256 blocks: the smallest
    images past the cap for C = 64 (8 channel groups: npl = 32), C = 8 (one group: every shuffle step) and C = 256 (32 groups)."""
    from srhip import ops
    B = 1
    npl = 4 * (64 // (C // 8))
    assert 256 < cdiv(B * H * W, npl) <= 260
    g = gen(540 + C + int(flip))
    img = torch.rand(B, 1, H, W, device="cuda", generator=g) if not flip else randn(g, B, 1, H, W) * 0.01
    feat = h(randn(g, B, C, H, W) * (1.0 if flip else 0.01))
    dw = torch.full((1, C, 3, 3) if flip else (C, 1, 3, 3), float("nan"), device="cuda")
    db = None if flip else torch.full((C,), float("nan"), device="cuda")
    ops.conv3x3_cin1_wgrad_h16(img[:, 0].contiguous(), nhwc(feat).half(), dw, db, flip=flip)
    tag = f"cin1_wgrad_h16 capped C = {C} flip = {int(flip)}"
    if flip:                                        # the tail: dW[0][c][t] = sum_p dy[p] feat[p + d_t][c]
        rw, _, rwa, _ = _wgrad_ref(img, feat)
        gate_f32(tag + " dW", dw, rw, rwa)
    else:                                           # the head: dW[c][0][t] = sum_p feat[p][c] img[p + d_t], db[c] = sum_p feat[p][c]
        rw, rb, rwa, rba = _wgrad_ref(feat, img)
        gate_f32(tag + " dW", dw, rw, rwa)
        gate_f32(tag + " db", db, rb, rba)
