"""Cases for tests/test_gpu_amp_arms.py: operands on which the single-product (--amp) arm of a contraction kernel must return
the float64 result BIT FOR BIT, and the routing rules that say which kernel instantiation a case reaches.

Why equality is the right gate.  Every operand value is an integer in [-15, 15] (four bits), or such an integer times a power
of two where a caller-supplied LayerNorm statistic asks for it.  Then

  * the leading bf16 plane (8 bits, RNE) holds the value exactly, and so does the leading fp16 plane (11 bits) after ANY
    power-of-two block scale that keeps the row's largest magnitude below 65504 -- whichever binade the scale rule lands in;
  * every lower plane is zero, every product is an integer multiple of one fixed power of two (`unit`);
  * with sum |a| |w| (+ bias, residual, alpha, row scale) below 2^24 units, float32 accumulation is exact in any order, with
    or without fused multiply-adds, and so is every epilogue step.

tests/test_cpu_amp_arm_cases.py proves these three conditions for every case here, without a GPU.  The same case therefore has
to come out bit-exact in the f32-grade mode 0 as well (all lower-plane products are zero).

The routing functions restate sr_gemm_ntb / sr_gemm_ntp / sr_gemm_ntw (GEMMs) and dispatch_ntb<true> / sr_conv3x3_nhcw2
(convs) of the product build, where no C-side switch is live."""
import zlib

import torch
import torch.nn.functional as F

import lead_plane_ref as LP

VMAX = 15
LIMIT = float(2 ** 24)


def gen_for(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def ints(g, *shape, vmax=VMAX):
    return torch.randint(-vmax, vmax + 1, shape, generator=g).float()


# ---------------------------------------------------------------------------------------------------------------- routing
def f16_linear_ok(N, K):
    """what srhip_gemm_nt_f16x2 takes: widths that run on 192-column tiles, K within the preparation kernel's row"""
    return (N % 180 == 0 or (N > 128 and N % 128 != 0)) and K <= 1024


def gemm_arm(N, fmt, amp, epi=0):
    """the kernel instantiation a Linear GEMM reaches (sr_gemm_ntb -> sr_gemm_ntp -> sr_gemm_ntw); None for the f32-grade bf16x3
    arms, which are not this file's subject"""
    if fmt == 1:
        return "k_nth2<true>" if amp and epi != 5 else "k_nth2<false>"
    if not amp or epi == 5:
        return None
    if N % 180 == 0:
        return "k_ntw<false,true>"
    if N <= 64:
        return "k_ntp<1,true>"
    if N <= 128 or N % 128 == 0:
        return "k_ntp<2,true>"
    return "k_ntw<false,true>"


def conv_arm(B, H, W, Cin, Cout, fmt, ps=0, amp=True):
    """the kernel instantiation a 3x3 conv reaches under mode 1 (dispatch_ntb<true>).  Cin / Cout: the kernel's reduce and
    output sides (for the PixelShuffle forms: ps 1 -> Cout = 4 F, ps 2 -> Cin = 4 F, the grid counts LOW-resolution pixels)."""
    a = "true" if amp else "false"
    if Cout % 180 == 0:
        wn, nt = 3, 180
    elif Cout <= 64:
        wn, nt = 1, 64
    elif Cout <= 128 or Cout % 128 == 0:
        wn, nt = 2, 128
    else:
        wn, nt = 3, 192
    blocks128 = -(-W // 16) * -(-H // 8) * B * -(-Cout // nt)
    wm = 2 if blocks128 >= 1024 else 1
    if fmt == 1:
        if wn == 3 and Cout % 64 != 0 and ps == 0:
            return f"k_nhcw<{a}>"
        return f"k_nhcw2<{4 if wm == 2 else 2},{a}>"
    if wm == 1 and wn == 3 and ps == 0:
        return f"k_ntcw<{a}>"
    if wm == 2 and wn in (1, 2):
        return f"k_ntcw2<4,{a}>"
    if wm == 1 and wn == 1:
        return f"k_ntcw2<2,{a}>"
    return f"k_ntb<{wm},{wn},true,{a}>"


# Every AMP instantiation the product build can launch.  Left out, because only a C-side switch of the experiments build
# reaches them: k_ntb<1,1 | 2,1 | 2,2, true, true> (SRHIP_NTCW2* = 0), k_ntb<1,3,true,true> without a PixelShuffle
# (SRHIP_NTCW = 0), k_ntp<3,true> (SRHIP_NTW = 0) and k_nth under SRHIP_F16X2_PASSES = 0.
GEMM_ARMS = {"k_ntp<1,true>", "k_ntp<2,true>", "k_ntw<false,true>", "k_nth2<true>"}
CONV_ARMS = {"k_ntcw<true>", "k_nhcw<true>", "k_ntcw2<2,true>", "k_nhcw2<2,true>", "k_ntcw2<4,true>", "k_nhcw2<4,true>",
             "k_ntb<1,2,true,true>", "k_ntb<2,3,true,true>"}


# ------------------------------------------------------------------------------------------------------------ GEMM cases
# (M, N, K): bf16x3 planes.  Rows: one, 63 / 65 around the 64-row tile, fewer than a tile, several tiles.  Columns: a ragged last
# tile (196, 200 on 192-column tiles; 48, 120 inside one tile; 724 = 3 x 192 + 148).  K: 20, 84, 100, 212 are no multiple of 32
# and leave half an 8-k octet (K % 8 == 4); 32 / 64 / 96 / 160 / 212 are one / two / three / five / seven 32-k stages.
# N = 62, 126, 198 are no multiple of 4: no 16-byte epilogue whatever the alignment.
GEMM_BF16 = [(1, 64, 64), (63, 48, 20), (65, 60, 84), (130, 64, 160), (40, 62, 64),         # k_ntp<1,true>
             (65, 128, 100), (40, 120, 212), (130, 256, 64), (1, 100, 32), (63, 384, 96), (33, 126, 100),   # k_ntp<2,true>
             (1, 180, 32), (63, 180, 64), (65, 196, 96), (40, 200, 84), (257, 360, 212),    # k_ntw<false,true>
             (130, 448, 100), (70, 724, 20), (300, 540, 180), (65, 198, 84)]
# fp16x2 planes (k_nth2): K = 64, 180 are one 192-k pass; 212 is a pass and one stage (the three-deep W prefetch of stages 3 - 5
# reaches into the next pass); 360 / 416 two passes (12 and 13 stages); 540 three (17 stages); 1024 six, the last of two stages.
GEMM_F16 = [(1, 180, 64), (63, 180, 180), (65, 196, 212), (130, 200, 360), (40, 360, 416), (257, 180, 540), (70, 196, 1024),
            (64, 540, 180), (130, 180, 1024), (65, 198, 212)]
# the epilogue families run on these (format, M, N, K): one per single-product GEMM kernel, two for k_nth2
GEMM_EPI = [(0, 70, 64, 64), (0, 77, 128, 84), (0, 130, 196, 100), (1, 130, 180, 360), (1, 77, 196, 212)]
RPS = (64, 50)          # rows per row-scale entry: a multiple of the 64-row tile (one scale a block) and not (looked up per row)


def gemm_case_id(fmt, M, N, K):
    return f"{'f16' if fmt else 'bf16'}-{M}x{N}x{K}"


def gemm_operands(fmt, M, N, K, a_mode=0):
    """dict(A, W, b, R, stats, unit): float32 CPU tensors.  fmt 1: the rows of A cycle through four magnitude profiles over the
    192-k passes -- dense; RISING (|a| <= 1 in k < 192, 15 in every later pass: the accumulators must be rescaled by 2^-4);
    zero in the first pass(es), 15 afterwards; all zero.  Rows of W: every fourth row small (|w| <= 1), row 5 all zero.
    a_mode 1: statistics {mean, rstd} with an integer mean in [-3, 3] and rstd in {1, 1/2, 1/4}: xhat is a multiple of 1/4."""
    g = gen_for(f"gemm-{fmt}-{M}-{N}-{K}-{a_mode}")
    A, W = ints(g, M, K), ints(g, N, K)
    W[::4] = ints(g, W[::4].shape[0], K, vmax=1)
    if N > 5:
        W[5] = 0
    if fmt == 1:
        P = LP.PASS_K
        for r in range(M):
            kind = r % 4
            if kind == 1:
                A[r, :P] = ints(g, min(P, K), vmax=1)
                A[r, 0] = 1
                for p0 in range(P, K, P):
                    A[r, p0] = 15
            elif kind == 2:
                z = P if K <= 2 * P else 2 * P
                A[r, :z] = 0
                if K > z:
                    A[r, K - 1] = -15
            elif kind == 3:
                A[r] = 0
    b, R = ints(g, N), ints(g, M, N)
    stats, unit = None, 1.0
    if a_mode == 1:
        mean = torch.randint(-3, 4, (M,), generator=g).float()
        rstd = torch.tensor([1.0, 0.5, 0.25])[torch.randint(0, 3, (M,), generator=g)]
        stats = torch.stack([mean, rstd], 1).contiguous()
        unit = 0.25
    return dict(A=A, W=W, b=b, R=R, stats=stats, unit=unit)


ROWSCALES = torch.tensor([1.0, 0.0, 2.0, 4.0])
ALPHA = 2.0


def rowscale_for(M, rows_per_scale):
    n = -(-M // rows_per_scale)
    return ROWSCALES.repeat(-(-n // len(ROWSCALES)))[:n].contiguous()


def gemm_reference(op, epi=0, alpha=1.0, rowscale=None, rows_per_scale=1, bias=True):
    """float64 statement of srhip_gemm_nt_bx3 / _f16x2 on the operands `op`: (result, bound) where bound is the largest value
    any partial sum of any evaluation order can reach (sum of magnitudes)."""
    A, W = op["A"].double(), op["W"].double()
    if op["stats"] is not None:
        A = (A - op["stats"][:, :1].double()) * op["stats"][:, 1:].double()
    y = A @ W.t()
    bound = A.abs() @ W.abs().t()
    if bias:
        y = y + op["b"].double()
        bound = bound + op["b"].abs().double()
    if epi == 1:
        y = y.clamp_min(0)
    elif epi == 2:
        s = torch.full((A.shape[0],), float(alpha), dtype=torch.float64)
        if rowscale is not None:
            s = s * rowscale.double().repeat_interleave(rows_per_scale)[:A.shape[0]]
        y = op["R"].double() + s[:, None] * y
        bound = op["R"].abs().double() + s.abs()[:, None].clamp_min(1.0) * bound
    elif epi == 4:
        y = y * (op["R"] > 0)
    return y, bound.max().item()


# ------------------------------------------------------------------------------------------------------------ conv cases
# (name, kind, B, H, W, Cin, Cout): kind "conv" -> ops.conv3x3; "ps2" -> ops.conv3x3_ps2 (Cout = 4 F channels before the
# shuffle); "ps2_bwd" -> ops.conv3x3_ps2_bwd_data (the conv's Cout = 4 F is the kernel's reduce side, its Cin the output side).
# Image sizes leave partly empty 4- / 8-row x 16-pixel tiles in both directions: 9 x 7, 24 x 40, 13 x 21.
CONV_SMALL = [("c180", "conv", 2, 9, 7, 180, 180), ("c64to180", "conv", 1, 24, 40, 64, 180), ("c64", "conv", 2, 13, 21, 64, 64),
              ("c128to64", "conv", 1, 9, 7, 128, 64), ("c256to64", "conv", 1, 24, 40, 256, 64), ("c64to96", "conv", 2, 9, 7, 64, 96),
              ("c64to256", "conv", 1, 13, 21, 64, 256), ("c128to128", "conv", 1, 24, 40, 128, 128),
              ("ps2", "ps2", 2, 9, 7, 64, 256), ("ps2_bwd", "ps2_bwd", 1, 13, 21, 64, 256)]
# the 128-pixel tiles need 1024 blocks: one 256 x 512 image at 64 -> 64 (and 64 -> 180 for k_ntb<2,3>), 128 x 512 at 64 -> 256
CONV_LARGE = [("big64", "conv", 1, 256, 512, 64, 64), ("big256", "conv", 1, 128, 512, 64, 256), ("big180", "conv", 1, 256, 512, 64, 180),
              ("bigps2", "ps2", 1, 128, 512, 64, 256)]
CONV_CASES = {c[0]: c for c in CONV_SMALL + CONV_LARGE}
CONV_SHARE = {"bigps2": "big256"}      # same operands, hence one reference convolution for both


def conv_kernel_sides(kind, Cin, Cout):
    """(reduce side, output side, ps) as dispatch_ntb sees them"""
    return {"conv": (Cin, Cout, 0), "ps2": (Cin, Cout, 1), "ps2_bwd": (Cout, Cin, 2)}[kind]


def conv_formats(name):
    """the plane formats a case runs in: format 1 where PrepTable.conv's routing rule gives it, format 0 always except for
    big180's twin (180 columns at format 1 is k_nhcw whatever the grid: c180 / c64to180 cover it)"""
    _, kind, B, H, W, Cin, Cout = CONV_CASES[name]
    K, N, ps = conv_kernel_sides(kind, Cin, Cout)
    f16 = (N % 64 == 0 and 64 <= K) or (ps == 0 and N % 180 == 0 and 64 <= K <= 256)
    if name == "big180" or not f16:
        return (0,)
    return (0, 1)


def conv_arm_of(name, fmt):
    _, kind, B, H, W, Cin, Cout = CONV_CASES[name]
    K, N, ps = conv_kernel_sides(kind, Cin, Cout)
    return conv_arm(B, H, W, K, N, fmt, ps)


def conv_operands(name):
    """dict(x [B,Cin,H,W], w [Cout,Cin,3,3], b, R): float32 integers.  Channels: the last 32-channel chunk of the reduce side
    holds +-15, the chunks before it only {-1, 0, 1} (the fp16x2 kernels' running halo-tile scale has to drop at the last
    chunk); every third output channel of w is small as well, channel 1 all zero.  For ps2_bwd `x` is the gradient of the
    SHUFFLED output [B, F, 2H, 2W]."""
    _, kind, B, H, W, Cin, Cout = CONV_CASES[name]
    g = gen_for("conv-" + CONV_SHARE.get(name, name))
    w = ints(g, Cout, Cin, 3, 3)
    w[::3] = ints(g, w[::3].shape[0], Cin, 3, 3, vmax=1)
    w[1] = 0
    if kind == "ps2_bwd":
        Fo = Cout // 4
        x = ints(g, B, Fo, 2 * H, 2 * W, vmax=1)      # the kernel's reduce index is sub-pixel major, sp * F + c: its last 32
        x[:, Fo - 32:, 1::2, 1::2] = ints(g, B, 32, H, W)      # are sub-pixel 3 (odd row, odd column) of the last 32 channels
        R = ints(g, B, Cin, H, W)
    else:
        x = ints(g, B, Cin, H, W)
        if Cin > 32:
            x[:, :Cin - 32] = ints(g, B, Cin - 32, H, W, vmax=1)
        R = ints(g, B, Cout, H, W)
    return dict(x=x, w=w, b=ints(g, Cout), R=R)


def conv_reference(name, op, dtype=torch.float64):
    """the plain convolution (bias included; none for ps2_bwd) as NCHW `dtype`: ps2 -> PixelShuffle(2) of it, ps2_bwd -> the
    data gradient read from the shuffled gradient.  float32 is exact on these operands (module docstring) and is what the
    256 x 512 cases use: float64 aten convs of that size take tens of seconds."""
    kind = CONV_CASES[name][1]
    x, w, b = op["x"].to(dtype), op["w"].to(dtype), op["b"].to(dtype)
    if kind == "ps2_bwd":
        return F.conv_transpose2d(F.pixel_unshuffle(x, 2), w, padding=1)
    y = F.conv2d(x, w, b, padding=1)
    return F.pixel_shuffle(y, 2) if kind == "ps2" else y


IN_BN = ("c64", "c128to64")      # format-1 cases that also run with the BatchNorm-ReLU input prologue


def conv_in_bn(name):
    """coefficients [4, Cin] of the in_bn prologue relu((x - mean) k + beta) with an integer mean in [-2, 2], k in {1, 2} and an
    integer beta in [-3, 3]: the prologue's output is an integer in [0, 37].  (Row 1 is not read by the conv kernels.)"""
    Cin = CONV_CASES[name][5]
    g = gen_for("in_bn-" + name)
    mean = torch.randint(-2, 3, (Cin,), generator=g).float()
    k = torch.tensor([1.0, 2.0])[torch.randint(0, 2, (Cin,), generator=g)]
    beta = torch.randint(-3, 4, (Cin,), generator=g).float()
    return torch.stack([mean, torch.ones(Cin), k, beta]).contiguous()


def in_bn_apply(x, coef):
    """the prologue on NCHW x, in x's dtype"""
    c = coef.to(x.dtype)
    return ((x - c[0][None, :, None, None]) * c[2][None, :, None, None] + c[3][None, :, None, None]).clamp_min(0)


IN_BN_VMAX = (VMAX + 2) * 2 + 3


def conv_bound(name, vmax=VMAX):
    """largest magnitude any partial sum can reach: nine taps x reduce side x 15 x 15, the bias, then alpha = 2 times the largest
    row scale and the residual"""
    _, kind, B, H, W, Cin, Cout = CONV_CASES[name]
    K = conv_kernel_sides(kind, Cin, Cout)[0]
    return (9 * K * vmax * VMAX + VMAX) * ALPHA * ROWSCALES.max().item() + VMAX
