"""The single-product (--amp, srhip_set_matmul_mode(1)) arm of every contraction kernel, arm by arm.

Under mode 1 the Linear GEMMs, the 3x3 convs and the two fused SwinIR kernels run SEPARATE template instantiations that stage,
load and multiply only the leading plane of each operand.  Three kinds of check:

1. Exactly representable operands (tests/amp_arm_cases.py; the conditions are proved on the CPU by
   tests/test_cpu_amp_arm_cases.py): the kernel must return the float64 result bit for bit, in mode 1 and in mode 0, into a
   NaN-filled buffer wider than the result whose frame must stay NaN.  No tolerance, no knowledge of tile geometry.  The convs'
   references are float32 CPU convolutions for the 256 x 512 images (exact on these operands, as the CPU file checks on the
   small cases; a float64 aten conv of that size takes tens of seconds), float64 for the small ones.
2. Random operands: the leading plane is the ROUNDED one (RNE bf16; fp16 under a power-of-two block scale).  The emulation of
   tests/lead_plane_ref.py is first pinned bit for bit against the planes the device writes, then the mode-1 GEMM / conv must
   match float64 on the emulated operands to the project's f32-grade gate, 2e-6 of the largest entry (products of rounded
   operands are exact in f32, only the accumulation differs), and its distance from the UNROUNDED float64 result must be at
   least 100 x that of mode 0: the arm under test really is the single product.  Where an f32 ulp or the tile geometry decides a
   rounding (GELU prologue; the fp16x2 convs' halo-tile scales) the gate is instead: at most 2 x the emulation's own distance
   from the unrounded result (an operand may sit one binade coarser than the emulation assumes).
3. ops.mlp_fwd_f16 / ops.wmsa_fwd_f16 under mode 1 against a float64 emulation of the chain that rounds every contraction
   input to its leading fp16 plane, the same 2 x gate, plus a bound derived from the 0.01-dB PSNR gate of test_gpu_amp.py.

Kernel instantiation reached, per test (routing: amp_arm_cases.gemm_arm / conv_arm, restating sr_gemm_ntb, sr_gemm_ntp,
sr_gemm_ntw, dispatch_ntb<true>, sr_conv3x3_nhcw2):

    test_exact_gemm[bf16-*]                       k_ntp<1,true> (N <= 64), k_ntp<2,true> (N <= 128 or N % 128 == 0),
                                                  k_ntw<false,true> (N % 180 == 0, other N > 128); mode 0: their f32-grade twins
    test_exact_gemm[f16-*]                        k_nth2<true>; mode 0: k_nth2<false>
    test_exact_gemm_epilogues                     the same four, epilogues 0 / 1 / 2 / 4, 16-byte and scalar stores
    test_gemm_aux_and_row_statistics              the same four: epilogue 3 + aux, stats_out
    test_lnbwd_form_keeps_all_planes_in_mode_1    k_nth2<false> (format 1), k_ntw<false,false> (format 0): epilogue 5 has no AMP arm
    test_exact_conv[name-fmt]                     c180, c64to180: k_ntcw<true> / k_nhcw<true>; c64, c128to64, c256to64:
                                                  k_ntcw2<2,true> / k_nhcw2<2,true>; c64to96: k_ntb<1,2,true,true>; c64to256,
                                                  c128to128, ps2: k_ntb<1,2,true,true> / k_nhcw2<2,true>; ps2_bwd:
                                                  k_ntcw2<2,true> / k_nhcw2<2,true> (ps = 2); big64, big256, bigps2:
                                                  k_ntcw2<4,true> / k_nhcw2<4,true>; big180: k_ntb<2,3,true,true>
    test_random_gemm_*, test_random_conv_*        one shape per instantiation above except the 128-pixel conv tiles
    test_mlp_f16_under_mode_1                     k_mlp_f16<false,true>
    test_wmsa_f16_under_mode_1                    k_wmsa_f16h<30 | 32, 2, true> (6 / 5 heads)

Left out -- only a C-side switch of the experiments build reaches them: k_ntb<1,1 | 2,1 | 2,2, true, true> (SRHIP_NTCW2 = 0,
SRHIP_NTCW2_SMALL = 0, SRHIP_NTCW2_WIDE = 0), k_ntb<1,3,true,true> without a PixelShuffle (SRHIP_NTCW = 0), k_ntp<3,true>
(SRHIP_NTW = 0), k_nth (SRHIP_F16X2_PASSES = 0).  The four-wave k_wmsa_f16<D,4,1> (other head counts) has no AMP arm.

Measured on an MI355X (the tests print every figure; the whole file runs in five seconds):

    every equality gate of section 1 holds, in both modes; epilogue 3 at most 1.3e-7, aux 8.2e-8, stats_out 8.2e-8 (gate 1e-5),
    the lnbwd form 3.5e-7 .. 5.9e-7 in either mode (gate 2e-6)
    GEMM, mode 1 against the emulated leading planes (gate 2e-6)      bf16x3 6.1e-8 .. 1.6e-7      fp16x2 8.4e-8 .. 4.4e-7
    GEMM, mode 1 / mode 0 distance from the unrounded result (>= 100) bf16x3 5300 .. 11700         fp16x2 420 .. 1700
    GEMM with the GELU prologue, kernel / emulation (gate 2)          1.00 on all eight shapes (mode 1 / mode 0: 670 .. 20000)
    conv, bf16x3, mode 1 against the leading planes (gate 2e-6)       2.3e-7 .. 6.8e-7             mode 1 / mode 0 1400 .. 3900
    conv, fp16x2, kernel / per-pixel emulation (gate 2)               1.00 on all seven cases      mode 1 / mode 0 250 .. 770
    ops.mlp_fwd_f16, kernel / emulation (gate 2)                      1.00 on all four shapes; rms error 9.5e-5 .. 3.4e-4
    ops.wmsa_fwd_f16, kernel / emulation (gate 2)                     0.82, 0.91, 1.03, 0.82;   rms error 8.5e-5 .. 5.1e-4
    (rms error of the fused kernels: relative to the rms of the output rows; bound 1.9e-3, see PSNR_RMS_BOUND)"""
import contextlib
import functools

import pytest
import torch
import torch.nn.functional as F

import amp_arm_cases as C
import lead_plane_ref as LP
import sr_oracle as O

pytestmark = pytest.mark.gpu
NAN = float("nan")

@pytest.fixture(scope="module")
def ops():
    from srhip import ops as o
    return o


def recorded(monkeypatch, ops):
    """the names of the library calls the wrappers make from here on"""
    calls = []
    monkeypatch.setattr(ops, "call", lambda name, *a, _f=ops.call: (calls.append(name), _f(name, *a))[1])
    return calls


def modes(ops):
    """(mode, context): the f32-grade mode, then inference under --amp"""
    from srhip._lib import lib

    @contextlib.contextmanager
    def amp():
        with ops.amp_inference():
            assert lib.srhip_get_matmul_mode() == 1
            yield
        assert lib.srhip_get_matmul_mode() == 0
    return ((0, contextlib.nullcontext()), (1, amp()))


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def lin_planes(ops, W, fmt):
    Wc = W.cuda().contiguous()
    if fmt == 0:
        return ops.split_bf16x3(Wc)
    out = ops.Bx3(W.shape[0], W.shape[1], "cuda")
    tb = ops.PrepTable()
    tb.linear(Wc, out, f16=True)
    tb.build("cuda").run()
    torch.cuda.synchronize()
    assert out.fmt == 1
    return out


def conv_planes(ops, monkeypatch, w, fmt, kind="conv"):
    """the forward pack of w [Co,Ci,3,3] (kind conv / ps2) or its data-gradient twin (ps2_bwd) in plane format `fmt`"""
    monkeypatch.setattr(ops, "F16X2_CONV", fmt == 1)
    Co, Ci = w.shape[:2]
    rows, kd = (Ci, Co) if kind == "ps2_bwd" else (Co, Ci)
    out = ops.Bx3(9 * rows, kd, "cuda")
    wc = w.cuda().contiguous()
    tb = ops.PrepTable()
    tb.conv(wc, out, data_grad=kind == "ps2_bwd", ps2=kind != "conv")
    tb.build("cuda").run()
    torch.cuda.synchronize()
    assert out.fmt == fmt, (out.fmt, fmt)
    return out


class Frame:
    """a NaN-filled [rows + 2, ld] buffer and the [rows, N] window at row 1, column c0 that a kernel may write.  c0 = 4 keeps the
    window 16-byte aligned (ld is a multiple of 4), an odd c0 does not."""

    def __init__(self, rows, N, c0):
        self.rows, self.N, self.c0 = rows, N, c0
        ld = (N + c0 + 8 + 3) // 4 * 4
        self.buf = torch.full((rows + 2, ld), NAN, device="cuda")
        self.view = self.buf[1:rows + 1, c0:c0 + N]

    def check(self, expect, what):
        got = self.view
        if not torch.equal(got, expect):
            bad = (got != expect) | torch.isnan(got)
            idx = bad.nonzero()[0].tolist()
            raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} entries differ, first at {idx}: "
                                 f"{got[tuple(idx)].item()} instead of {expect[tuple(idx)].item()}")
        outside = torch.ones_like(self.buf, dtype=torch.bool)
        outside[1:self.rows + 1, self.c0:self.c0 + self.N] = False
        assert torch.isnan(self.buf[outside]).all(), f"{what}: written outside its [{self.rows}, {self.N}] window"


def sliced(t, c0):
    """t [M, N] on the device as a column slice, starting at column c0, of a wider NaN-filled buffer"""
    M, N = t.shape
    wide = torch.full((M, (N + c0 + 4 + 3) // 4 * 4), NAN, device="cuda")
    wide[:, c0:c0 + N] = t.cuda()
    return wide[:, c0:c0 + N]


# =============================================================================================== 1. exact operands: GEMMs
GEMM_IDS = [(0,) + c for c in C.GEMM_BF16] + [(1,) + c for c in C.GEMM_F16]
# the LayerNorm prologue of k_nth2 scales by 2^floor(log2(16384 / sqrt(K))) with the device's rsqrtf: at K = 64, 1024 the
# quotient IS a power of two and the binade is the approximation's to choose, with xhat up to 18 the finer one overflows fp16
A_MODE1_K = (180, 212, 360, 540)


@pytest.mark.parametrize("fmt,M,N,K", GEMM_IDS, ids=[C.gemm_case_id(*c) for c in GEMM_IDS])
def test_exact_gemm(ops, monkeypatch, fmt, M, N, K):
    """bias epilogue, plain and behind the LayerNorm prologue with exact statistics, through the 16-byte and the scalar stores"""
    calls = recorded(monkeypatch, ops)
    entry = "srhip_gemm_nt_f16x2" if fmt else "srhip_gemm_nt_bx3"
    n = 0
    for a_mode in (0, 1):
        if a_mode == 1 and fmt == 1 and K not in A_MODE1_K:
            continue
        op = C.gemm_operands(fmt, M, N, K, a_mode)
        ref = C.gemm_reference(op)[0].float().cuda()
        Wb = lin_planes(ops, op["W"], fmt)
        A, b = op["A"].cuda(), op["b"].cuda()
        st = None if op["stats"] is None else op["stats"].cuda()
        for c0 in (4, 3):
            for mode, ctx in modes(ops):
                fr = Frame(M, N, c0)
                with ctx:
                    ops.gemm_nt(A, Wb, b, out=fr.view, a_mode=a_mode, ln_stats=st)
                n += 1
                fr.check(ref, f"{C.gemm_arm(N, fmt, mode)} mode {mode} a_mode {a_mode} c0 {c0}")
    assert [c for c in calls if "gemm" in c] == [entry] * n and "srhip_set_matmul_mode" in calls


@pytest.mark.parametrize("fmt,M,N,K", C.GEMM_EPI, ids=[C.gemm_case_id(*c) for c in C.GEMM_EPI])
@pytest.mark.parametrize("c0", [4, 3], ids=["wide", "scalar"])
def test_exact_gemm_epilogues(ops, fmt, M, N, K, c0):
    """epilogues 1, 2 (alpha = 2, row scales {1, 0, 2, 4} per 64 and per 50 rows), 4; A, R and out as column slices of wider
    buffers.  c0 = 4: everything 16-byte aligned (wide_epi); c0 = 3: out starts at an odd column.  One more scalar-store form
    with out aligned and only R at an odd column."""
    op = C.gemm_operands(fmt, M, N, K)
    Wb = lin_planes(ops, op["W"], fmt)
    A, b = sliced(op["A"], 4), op["b"].cuda()
    forms = [(1, {}, c0), (4, {}, c0)]
    forms += [(2, dict(alpha=C.ALPHA, rowscale=C.rowscale_for(M, r), rows_per_scale=r), c0) for r in C.RPS]
    forms += [(2, dict(alpha=C.ALPHA), (4, 1))]
    for epi, kw, where in forms:
        oc, rc = where if isinstance(where, tuple) else (where, where)
        ref = C.gemm_reference(op, epi, **kw)[0].float().cuda()
        R = sliced(op["R"], rc)
        dkw = dict(kw)
        if kw.get("rowscale") is not None:
            dkw["rowscale"] = kw["rowscale"].cuda()
        for mode, ctx in modes(ops):
            fr = Frame(M, N, oc)
            with ctx:
                ops.gemm_nt(A, Wb, b, out=fr.view, epi=epi, R=R, **dkw)
            fr.check(ref, f"{C.gemm_arm(N, fmt, mode)} mode {mode} epi {epi} {sorted(kw)} out@{oc} R@{rc}")


@pytest.mark.parametrize("fmt,M,N,K", C.GEMM_EPI, ids=[C.gemm_case_id(*c) for c in C.GEMM_EPI])
def test_gemm_aux_and_row_statistics(ops, fmt, M, N, K):
    """Not exact, on exact operands: epilogue 3 (out = s (A W^T) gelu'(R), aux = gelu(R), an A&S 7.1.26 erf) at the f32-grade
    2e-6, and stats_out against the float64 statistics of the exact result at the existing 1e-5; in both modes the same
    gates, with and without aux, wide and scalar stores."""
    op = C.gemm_operands(fmt, M, N, K)
    Wb = lin_planes(ops, op["W"], fmt)
    A, b = op["A"].cuda(), op["b"].cuda()
    Rs = op["R"] / 4.0                                   # gelu' varies over [-3.75, 3.75]
    Rg = Rs.double().clone().requires_grad_(True)
    F.gelu(Rg).sum().backward()
    rs = C.rowscale_for(M, 50)
    ref3 = rs.double().repeat_interleave(50)[:M, None] * (op["A"].double() @ op["W"].double().t()) * Rg.grad
    ref2, _ = C.gemm_reference(op, 2, alpha=C.ALPHA)
    mean, rstd = ref2.mean(1), (ref2.var(1, unbiased=False) + 1e-5).rsqrt()
    for c0 in (4, 3):
        R = sliced(Rs, c0)
        for mode, ctx in modes(ops):
            fr, fa, fp = Frame(M, N, c0), Frame(M, N, c0), Frame(M, N, c0)
            with ctx:
                ops.gemm_nt(A, Wb, None, out=fp.view, epi=3, R=R, rowscale=rs.cuda(), rows_per_scale=50)
                ops.gemm_nt(A, Wb, None, out=fr.view, epi=3, R=R, rowscale=rs.cuda(), rows_per_scale=50, aux=fa.view)
            fp.check(fr.view, "epilogue 3 with / without aux")
            e3, ea = relerr(fr.view, ref3), relerr(fa.view, F.gelu(Rs.double()))
            print(f"gemm {C.gemm_case_id(fmt, M, N, K)} mode {mode} c0 {c0}: epi 3 {e3:.2e}, aux {ea:.2e}")
            assert e3 < 2e-6 and ea < 2e-6
            fa.check(fa.view.clone(), "aux frame")
        if N <= 192:
            for mode, ctx in modes(ops):
                fr = Frame(M, N, c0)
                st = torch.full((M + 1, 2), NAN, device="cuda")
                with ctx:
                    ops.gemm_nt(A, Wb, b, out=fr.view, epi=2, R=sliced(op["R"], c0), alpha=C.ALPHA, stats_out=st[:M])
                fr.check(ref2.float().cuda(), f"stats_out form, mode {mode}")
                em, er = relerr(st[:M, 0], mean), relerr(st[:M, 1], rstd)
                print(f"gemm {C.gemm_case_id(fmt, M, N, K)} mode {mode} c0 {c0}: stats mean {em:.2e} rstd {er:.2e}")
                assert em < 1e-5 and er < 1e-5 and torch.isnan(st[M]).all()


@pytest.mark.parametrize("fmt", [0, 1], ids=["bf16", "f16"])
@pytest.mark.parametrize("M,N,K", [(130, 180, 360), (77, 180, 540), (65, 192, 212)])
def test_lnbwd_form_keeps_all_planes_in_mode_1(ops, fmt, M, N, K):
    """gemm_nt_lnbwd (epilogue 5) has no single-product arm: under mode 1 it must stay f32-grade, 2e-6 of the largest entry
    against float64 on random operands (a single product would sit at 1e-4 .. 1e-3), and give the bits of mode 0."""
    g = C.gen_for(f"lnbwd-{M}-{N}-{K}")
    rnd = lambda *s: torch.randn(*s, generator=g)
    A, W, x, res = rnd(M, K), rnd(N, K) * 0.1, rnd(M, N), rnd(M, N)
    xd = x.double().requires_grad_(True)
    F.layer_norm(xd, (N,), eps=1e-5).backward(A.double() @ W.double().t())
    ref = res.double() + xd.grad
    Wb = lin_planes(ops, W, fmt)
    stats = torch.empty(M, 2).cuda()
    ops.layernorm_fwd(x.cuda(), stats)
    outs = []
    for mode, ctx in modes(ops):
        fr = Frame(M, N, 4)
        with ctx:
            ops.gemm_nt_lnbwd(A.cuda(), Wb, x.cuda(), stats, res.cuda(), fr.view)
        e = relerr(fr.view, ref)
        print(f"lnbwd fmt {fmt} {M}x{N}x{K} mode {mode}: {e:.2e}")
        assert e < 2e-6
        fr.check(fr.view.clone(), "lnbwd frame")
        outs.append(fr.view.clone())
    assert torch.equal(outs[0], outs[1])


# =============================================================================================== 1. exact operands: convs
@functools.lru_cache(maxsize=None)
def conv_case(key):
    """operands and the NHWC reference of a conv case, computed once (bigps2 shares big256's convolution)"""
    op = C.conv_operands(key)
    big = key in {c[0] for c in C.CONV_LARGE}
    kind = C.CONV_CASES[key][1]
    y = C.conv_reference(key, op, torch.float32 if big else torch.float64)
    if big and kind == "conv":
        return op, y.permute(0, 2, 3, 1).contiguous()
    return op, y.float().permute(0, 2, 3, 1).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


CONV_IDS = [(name, fmt) for name in C.CONV_CASES for fmt in C.conv_formats(name)]


@pytest.mark.parametrize("name,fmt", CONV_IDS, ids=[f"{n}-{'f16' if f else 'bf16'}" for n, f in CONV_IDS])
def test_exact_conv(ops, monkeypatch, name, fmt):
    """bias epilogue into an aligned and an odd-column channel slice of a wider NaN buffer, then epilogues 1, 2 (alpha = 2, one
    row scale per image), 4 where the entry point takes them; mode 0 and mode 1."""
    _, kind, B, H, W, Cin, Cout = C.CONV_CASES[name]
    big = name in {c[0] for c in C.CONV_LARGE}
    if name in C.CONV_SHARE:
        op, base = conv_case(C.CONV_SHARE[name])
        y = nhwc(F.pixel_shuffle(base.permute(0, 3, 1, 2), 2))
    else:
        op, y = conv_case(name)
    arm = C.conv_arm_of(name, fmt)
    calls = recorded(monkeypatch, ops)
    Wb = conv_planes(ops, monkeypatch, op["w"], fmt, kind)
    X, b = nhwc(op["x"]).cuda(), op["b"].cuda()
    y = y.cuda()
    Bo, Ho, Wo, No = y.shape
    Rn = nhwc(op["R"]).cuda()
    rs = C.rowscale_for(B, 1)[:B] if B > 1 else torch.tensor([2.0])
    forms = [(0, 4), (0, 3)] if not big else [(0, 4)]
    if not big:
        forms += {"conv": [(1, 4), (2, 4), (4, 3)], "ps2": [(1, 4)], "ps2_bwd": [(4, 4)]}[kind]
    n = 0
    for epi, c0 in forms:
        if epi == 0 or kind == "ps2_bwd":
            ref = y if epi == 0 else y * (Rn > 0)
        elif epi == 1:
            ref = y.clamp_min(0)
        elif epi == 2:
            ref = Rn + C.ALPHA * rs.cuda()[:, None, None, None] * y
        else:
            ref = y * (Rn > 0)
        ref2 = ref.reshape(-1, No)
        for mode, ctx in modes(ops):
            fr = Frame(Bo * Ho * Wo, No, c0)
            out = fr.view.unflatten(0, (Bo, Ho, Wo))
            with ctx:
                if kind == "conv":
                    ops.conv3x3(X, Wb, b, Cout, out=out, epi=epi, R=Rn if epi in (2, 4) else None,
                                rowscale=rs.cuda() if epi == 2 else None, alpha=C.ALPHA if epi == 2 else 1.0)
                elif kind == "ps2":
                    ops.conv3x3_ps2(X, Wb, b, out, epi=epi)
                else:
                    ops.conv3x3_ps2_bwd_data(X, Wb, out, epi=epi, R=Rn if epi == 4 else None)
            n += 1
            fr.check(ref2, f"{name} fmt {fmt} {arm if mode else 'mode 0'} epi {epi} c0 {c0}")
    entry = {"conv": "srhip_conv3x3_nhwc", "ps2": "srhip_conv3x3_ps2", "ps2_bwd": "srhip_conv3x3_ps2_bwd_data"}[kind] \
        + ("_f16x2" if fmt else "_bx3")
    assert [c for c in calls if "conv3x3" in c] == [entry] * n


@pytest.mark.parametrize("name", C.IN_BN)
def test_exact_conv_in_bn_prologue(ops, monkeypatch, name):
    """the BatchNorm-ReLU input prologue relu((x - mean) k + beta) of the 64-column fp16x2 kernel with exact coefficients: the
    zero padding applies BEHIND the prologue (a border pixel's neighbours are 0, not relu(beta - mean k))"""
    _, kind, B, H, W, Cin, Cout = C.CONV_CASES[name]
    op = C.conv_operands(name)
    coef = C.conv_in_bn(name)
    ref = F.conv2d(C.in_bn_apply(op["x"].double(), coef), op["w"].double(), op["b"].double(), padding=1)
    assert ref.abs().max().item() < C.LIMIT
    ref2 = nhwc(ref.float()).reshape(-1, Cout).cuda()
    Wb = conv_planes(ops, monkeypatch, op["w"], 1)
    X = nhwc(op["x"]).cuda()
    for c0 in (4, 3):
        for mode, ctx in modes(ops):
            fr = Frame(B * H * W, Cout, c0)
            with ctx:
                ops.conv3x3(X, Wb, op["b"].cuda(), Cout, out=fr.view.unflatten(0, (B, H, W)), in_bn=coef.cuda())
            fr.check(ref2, f"{name} in_bn mode {mode} c0 {c0}")


# ======================================================================================= 2. random operands: the planes
def plant_row_maxima(W, exps):
    """W [rows, K] with every row rescaled so that its largest magnitude is exactly 1.5 * 2^exps[row]: a third of a binade
    away from a power of two, the scale rule's log2 cannot round into another binade"""
    W = W.clone()
    top = 1.5 * torch.exp2(exps.float())
    mx, at = W.abs().max(1)
    W = W * (top / mx)[:, None]
    r = torch.arange(W.shape[0])
    sign = torch.where(W[r, at] < 0, -1.0, 1.0)
    W = torch.maximum(torch.minimum(W, top[:, None]), -top[:, None])
    W[r, at] = sign * top
    return W


def plant_pass_maxima(A, exps):
    """the same for every 192-k pass of every row of A; exps [M, npass]"""
    A = A.clone()
    for p in range(exps.shape[1]):
        sl = slice(p * LP.PASS_K, (p + 1) * LP.PASS_K)
        A[:, sl] = plant_row_maxima(A[:, sl], exps[:, p])
    return A


def pass_exponents(M, K):
    """rows alternate between maxima that fall from pass to pass (the first pass's scale serves all) and maxima that RISE (the
    scale drops at every pass, the accumulators are rescaled by 2^-3 each time)"""
    npass = -(-K // LP.PASS_K)
    p = torch.arange(npass)
    return torch.where((torch.arange(M) % 2 == 0)[:, None], 3 - 2 * p[None], -4 + 3 * p[None]).float()


def test_planes_match_the_emulation_bit_for_bit(ops, monkeypatch):
    """plane 0 (and, format 1, the trailing 2^-s) of split_bf16x3, PrepTable.linear(f16=True), PrepTable.conv (forward pack and
    data-gradient twin) against tests/lead_plane_ref.py, on weights whose rows are decades apart (2^-20 .. 2^19)"""
    g = C.gen_for("planes")
    N, K = 200, 212
    W = plant_row_maxima(torch.randn(N, K, generator=g), (torch.arange(N) % 40 - 20).float())
    kp = ops.lib.srhip_bf16x3_kp(K)
    bx = lin_planes(ops, W, 0)
    p0, _ = LP.decode_planes(bx.planes.cpu(), N, K, kp, 0)
    assert torch.equal(p0, LP.lead_bf16(W).double())
    hx = lin_planes(ops, W, 1)
    p0, inv = LP.decode_planes(hx.planes.cpu(), N, K, kp, 1)
    q, s = LP.lead_f16_rows(W)
    assert torch.equal(inv[:N].double(), torch.exp2(-s.double()))
    assert torch.equal(p0 * inv[:N, None].double(), q)
    Co, Ci = 64, 128
    w = torch.randn(Co, Ci, 3, 3, generator=g)
    w = plant_row_maxima(w.reshape(Co, -1), (torch.arange(Co) % 30 - 15).float()).reshape(Co, Ci, 3, 3)
    for kind in ("conv", "ps2_bwd"):
        cx = conv_planes(ops, monkeypatch, w, 1, kind)
        if kind == "conv":       # rows t * Co + co hold w[co, :, t]
            rows, kd, wq = Co, Ci, w
        else:                    # rows t * Ci + ci hold w[:, ci, 8 - t] in sub-pixel-major order sp * (Co / 4) + c <- channel 4 c + sp
            rows, kd = Ci, Co
            wq = w.reshape(Co // 4, 4, Ci, 3, 3).transpose(0, 1).reshape(Co, Ci, 3, 3).transpose(0, 1).flip(2, 3)
        q, s = LP.lead_f16_conv(wq)
        p0, inv = LP.decode_planes(cx.planes.cpu(), 9 * rows, kd, ops.lib.srhip_bf16x3_kp(kd), 1)
        assert torch.equal(inv[:rows].double(), torch.exp2(-s.double())), kind
        want = q.reshape(rows, kd, 9).permute(2, 0, 1).reshape(9 * rows, kd)
        assert torch.equal(p0 * inv[:rows].double().repeat(9)[:, None], want), kind


# ======================================================================================= 2. random operands: the GEMMs
RANDOM_GEMMS = [(0, 70, 64, 64), (0, 77, 128, 84), (0, 130, 196, 100), (0, 300, 540, 180),
                (1, 130, 180, 360), (1, 77, 196, 212), (1, 65, 180, 540), (1, 64, 360, 1024)]


def random_gemm(fmt, M, N, K):
    g = C.gen_for(f"rgemm-{fmt}-{M}-{N}-{K}")
    A = plant_pass_maxima(torch.randn(M, K, generator=g), pass_exponents(M, K))
    W = plant_row_maxima(torch.randn(N, K, generator=g), (torch.arange(N) % 7 - 5).float())
    return A, W, torch.randn(N, generator=g)


def lead_w(W, fmt):
    return LP.lead_f16_rows(W)[0] if fmt else LP.lead_bf16(W).double()


def lead_a(A, fmt, a_mode=0):
    return LP.lead_f16_passes(A, a_mode) if fmt else LP.lead_bf16(A).double()


@pytest.mark.parametrize("fmt,M,N,K", RANDOM_GEMMS, ids=[C.gemm_case_id(*c) for c in RANDOM_GEMMS])
def test_random_gemm_multiplies_the_rounded_leading_planes(ops, fmt, M, N, K):
    """a_mode 0 and 1: mode 1 == float64 on the emulated leading planes to 2e-6 of the largest entry, and at least 100 x
    further from the unrounded result than mode 0"""
    A, W, b = random_gemm(fmt, M, N, K)
    Wb = lin_planes(ops, W, fmt)
    for a_mode in (0, 1):
        if a_mode == 1 and fmt == 1 and K not in A_MODE1_K:
            continue
        st = None
        Apro = A
        if a_mode == 1:
            st = torch.stack([A.mean(1), 1 / torch.sqrt(A.var(1, unbiased=False) + 1e-5)], 1).contiguous()
            Apro = LP.layernorm_prologue(A, st)
        full = F.linear((A.double() - st[:, :1].double()) * st[:, 1:].double() if a_mode else A.double(), W.double(), b.double())
        emul = F.linear(lead_a(Apro, fmt, a_mode), lead_w(W, fmt), b.double())
        y0 = ops.gemm_nt(A.cuda(), Wb, b.cuda(), a_mode=a_mode, ln_stats=None if st is None else st.cuda())
        with ops.amp_inference():
            y1 = ops.gemm_nt(A.cuda(), Wb, b.cuda(), a_mode=a_mode, ln_stats=None if st is None else st.cuda())
        e_emul, e1, e0 = relerr(y1, emul), relerr(y1, full), relerr(y0, full)
        print(f"gemm {C.gemm_case_id(fmt, M, N, K)} a_mode {a_mode}: mode 1 vs leading planes {e_emul:.2e}; vs unrounded: "
              f"mode 1 {e1:.2e}, mode 0 {e0:.2e}, ratio {e1 / e0:.0f}")
        assert e_emul < 2e-6
        assert e1 >= 100 * e0


@pytest.mark.parametrize("fmt,M,N,K", RANDOM_GEMMS, ids=[C.gemm_case_id(*c) for c in RANDOM_GEMMS])
def test_random_gemm_gelu_prologue_within_twice_the_emulation(ops, fmt, M, N, K):
    """a_mode 2: an f32 ulp of gelu can flip a rounding or a binade, so the gate is the distance from the unrounded float64
    result: at most 2 x that of the emulation (leading plane of float32(gelu(A)), per-row running scale)"""
    A, W, b = random_gemm(fmt, M, N, K)
    Wb = lin_planes(ops, W, fmt)
    gA = F.gelu(A.double())
    full = F.linear(gA, W.double(), b.double())
    emul = F.linear(lead_a(gA.float(), fmt), lead_w(W, fmt), b.double())
    y0 = ops.gemm_nt(A.cuda(), Wb, b.cuda(), a_mode=2)
    with ops.amp_inference():
        y1 = ops.gemm_nt(A.cuda(), Wb, b.cuda(), a_mode=2)
    e_k, e_e, e0 = relerr(y1, full), relerr(emul, full), relerr(y0, full)
    print(f"gemm gelu {C.gemm_case_id(fmt, M, N, K)}: kernel {e_k:.2e}, emulation {e_e:.2e}, ratio {e_k / e_e:.2f}; "
          f"mode 0 {e0:.2e}, mode 1 / mode 0 {e_k / e0:.0f}")
    assert e_k <= 2 * e_e
    assert e_k >= 100 * e0


# ======================================================================================= 2. random operands: the convs
RANDOM_CONVS = ["c180", "c64to180", "c64", "c128to64", "c64to96", "c128to128", "ps2", "ps2_bwd"]
RCONV_IDS = [(n, f) for n in RANDOM_CONVS for f in C.conv_formats(n)]


@pytest.mark.parametrize("name,fmt", RCONV_IDS, ids=[f"{n}-{'f16' if f else 'bf16'}" for n, f in RCONV_IDS])
def test_random_conv_multiplies_the_rounded_leading_planes(ops, monkeypatch, name, fmt):
    """bf16x3 planes: both operands' leading planes are plain RNE roundings, 2e-6 against float64 on them.  fp16x2 planes: the
    activation's scale belongs to a halo tile and a running channel chunk, so the gate is 2 x the distance of an emulation with
    one scale per PIXEL from the unrounded result.  Both: mode 1 at least 100 x further from the unrounded result than mode 0."""
    _, kind, B, H, W, Cin, Cout = C.CONV_CASES[name]
    g = C.gen_for("rconv-" + name)
    w = torch.randn(Cout, Cin, 3, 3, generator=g)
    w = plant_row_maxima(w.reshape(Cout, -1), (torch.arange(Cout) % 5 - 6).float()).reshape(Cout, Cin, 3, 3)
    b = torch.randn(Cout, generator=g) * 0.1
    if kind == "ps2_bwd":
        x = torch.randn(B, Cout // 4, 2 * H, 2 * W, generator=g)
        xk = F.pixel_unshuffle(x, 2)                      # the kernel's pixels: 4 F channels each
    else:
        x = xk = torch.randn(B, Cin, H, W, generator=g)

    def conv(xx, ww):
        if kind == "ps2_bwd":
            return F.conv_transpose2d(xx, ww, padding=1)
        y = F.conv2d(xx, ww, b.double(), padding=1)
        return F.pixel_shuffle(y, 2) if kind == "ps2" else y
    full = conv(xk.double(), w.double())
    if fmt == 0:
        xq, wq = LP.lead_bf16(xk).double(), LP.lead_bf16(w).double()
    else:
        xq = LP.lead_f16_rows(xk.permute(0, 2, 3, 1))[0].permute(0, 3, 1, 2)
        wq = LP.lead_f16_conv(w)[0] if kind != "ps2_bwd" else LP.lead_f16_conv(w.transpose(0, 1))[0].transpose(0, 1)
    emul = conv(xq, wq)
    Wb = conv_planes(ops, monkeypatch, w, fmt, kind)
    X = nhwc(x).cuda()

    def run():
        if kind == "conv":
            return ops.conv3x3(X, Wb, b.cuda(), Cout)
        if kind == "ps2":
            return ops.conv3x3_ps2(X, Wb, b.cuda(), torch.empty(B, 2 * H, 2 * W, Cout // 4, device="cuda"))
        return ops.conv3x3_ps2_bwd_data(X, Wb, torch.empty(B, H, W, Cin, device="cuda"))
    y0 = run().permute(0, 3, 1, 2)
    with ops.amp_inference():
        y1 = run().permute(0, 3, 1, 2)
    e_emul, e_k, e_e, e0 = relerr(y1, emul), relerr(y1, full), relerr(emul, full), relerr(y0, full)
    print(f"conv {name} fmt {fmt} ({C.conv_arm_of(name, fmt)}): mode 1 vs leading planes {e_emul:.2e}; vs unrounded: kernel "
          f"{e_k:.2e}, emulation {e_e:.2e}, ratio {e_k / e_e:.2f}; mode 0 {e0:.2e}, mode 1 / mode 0 {e_k / e0:.0f}")
    if fmt == 0:
        assert e_emul < 2e-6
    else:
        assert e_k <= 2 * e_e
    assert e_k >= 100 * e0


# ======================================================================================= 3. the fused SwinIR kernels
# What the 0.01-dB PSNR gate of tests/test_gpu_amp.py implies for ONE fused kernel.
#   * PSNR = -10 log10(MSE): 0.01 dB is a factor 10^0.001 - 1 = 2.3e-3 on the MSE.  A perturbation d of the network's output that
#     is uncorrelated with its error e adds its mean square to the MSE (the cross term 2 <e, d> has a standard deviation of
#     2 rms(e) rms(d) / sqrt(pixels), 0.4 % of rms(e) rms(d) on a 512 x 512 image), so the gate allows rms(d) <= 0.048 rms(e).
#   * rms(e) in that gate: its HR images are uniform noise on [0, 1] (standard deviation 0.289) and the network sees a x8
#     bicubic reduction, 1 / 64 of the degrees of freedom; what no function of the LR image can explain is 63 / 64 of the
#     variance: rms(e) >= 0.289 sqrt(63 / 64) = 0.286, whatever the weights.  Hence rms(d) <= 0.0137 of the image range.
#   * SwinIR runs 24 Swin blocks = 48 fused kernels, each adding its rounding error to the residual stream, where it stays; taken
#     as independent, of equal relative size r and carried to the image at that relative size (the image's rms is at most its
#     range), they add in quadrature: r sqrt(48) <= 0.0137, r <= 1.9e-3 of the rms of a kernel's output rows.
# The bound belongs to THAT gate.  On a trained network at 30 dB (rms(e) = 0.0316) the same reasoning allows r <= 2.2e-4, which an
# 11-bit leading plane cannot meet under this worst-case propagation model (measured: up to 5.1e-4, i.e. up to 0.05 dB there);
# the figure is printed with every case.
PSNR_RMS_BOUND = 1.9e-3
PSNR_RMS_BOUND_30DB = 2.2e-4


def rms_rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()


def mlp_chain(x, gamma, beta, w1, b1, w2, b2, s, rps, lead):
    """float64 out = x + s (gelu(LN(x) W1f^T + b1f) W2^T + b2) with the LayerNorm affine folded into the first Linear, as the
    kernel's operands are; lead: round every contraction input to its leading fp16 plane (LayerNorm output at k_nth2's a-priori
    scale, gelu(h) per hidden row, weights per row)"""
    M, Cc = x.shape
    xd = x.double()
    xn = F.layer_norm(xd, (Cc,), eps=1e-5)
    w1f = (w1 * gamma[None, :]).double() if not lead else LP.lead_f16_rows(w1 * gamma[None, :])[0]
    b1f = b1.double() + w1.double() @ beta.double()
    if lead:
        xn = LP.round_f16_at(xn.float(), LP.nth2_apriori_exponent(Cc))
    gh = F.gelu(xn @ w1f.t() + b1f)
    w2d = w2.double()
    if lead:
        gh, w2d = LP.lead_f16_rows(gh.float())[0], LP.lead_f16_rows(w2)[0]
    y = gh @ w2d.t() + b2.double()
    if s is not None:
        y = y * s.double().repeat_interleave(rps)[:M, None]
    return xd + y


@pytest.mark.parametrize("M,C_,hidden,nsamp", [(64, 180, 360, 1), (77, 64, 196, 1), (333, 96, 256, 3), (333, 180, 360, 0)])
def test_mlp_f16_under_mode_1(ops, M, C_, hidden, nsamp):
    g = C.gen_for(f"mlp-{M}-{C_}-{hidden}")
    rnd = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale
    x = rnd(M, C_) * 1.5 + rnd(M, 1)
    w1, b1, w2, b2 = rnd(hidden, C_, scale=0.1), rnd(hidden, scale=0.3), rnd(C_, hidden, scale=0.1), rnd(C_, scale=0.3)
    gamma, beta = 1 + rnd(C_, scale=0.2), rnd(C_, scale=0.2)
    s = torch.rand(nsamp, generator=g) + 0.5 if nsamp else None
    rps = -(-M // nsamp) if nsamp else 1
    d = {k: v.cuda() for k, v in dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, gamma=gamma, beta=beta).items()}
    P1, P2 = ops.Bx3(hidden, C_, "cuda"), ops.Bx3(C_, hidden, "cuda")
    b1f = torch.empty(hidden, device="cuda")
    tb = ops.PrepTable()
    tb.linear(d["w1"], P1, gamma=d["gamma"], f16=True)
    tb.linear(d["w2"], P2, f16=True)
    tb.fold_bias(d["w1"], d["b1"], d["beta"], b1f)
    tb.build("cuda").run()
    st = torch.empty(M, 2, device="cuda")
    ops.layernorm_fwd(d["x"], st)
    sd = None if s is None else s.cuda()
    full = mlp_chain(x, gamma, beta, w1, b1, w2, b2, s, rps, False)
    emul = mlp_chain(x, gamma, beta, w1, b1, w2, b2, s, rps, True)
    y0 = Frame(M, C_, 4)
    ops.mlp_fwd_f16(d["x"], st, P1, b1f, P2, d["b2"], y0.view, rowscale=sd, rows_per_scale=rps)
    with ops.amp_inference():
        fr, fs = Frame(M, C_, 4), Frame(M, C_, 4)
        sto = torch.full((M + 1, 2), NAN, device="cuda")
        ops.mlp_fwd_f16(d["x"], st, P1, b1f, P2, d["b2"], fr.view, rowscale=sd, rows_per_scale=rps)
        ops.mlp_fwd_f16(d["x"], st, P1, b1f, P2, d["b2"], fs.view, rowscale=sd, rows_per_scale=rps, stats_out=sto[:M])
        # the forms mode 1 refuses: the saved gate / gelu(h), every backward entry point
        hbuf = torch.empty(M, hidden, device="cuda")
        with pytest.raises(ops.SrhipError):
            ops.mlp_fwd_f16(d["x"], st, P1, b1f, P2, d["b2"], torch.empty(M, C_, device="cuda"), gate=hbuf,
                            gh=torch.empty_like(hbuf))
        P1T, P2T = ops.Bx3(C_, hidden, "cuda"), ops.Bx3(hidden, C_, "cuda")
        P1T.fmt = P2T.fmt = 1
        with pytest.raises(ops.SrhipError):
            ops.mlp_bwd_f16(torch.zeros(M, C_, device="cuda"), P2T, P1T, hbuf, torch.empty_like(hbuf), None, d["x"], st,
                            torch.empty(M, C_, device="cuda"))
        with pytest.raises(ops.SrhipError):
            ops.mlp_bwd_f16(torch.zeros(M, C_, device="cuda"), P2T, P1T, None, torch.empty_like(hbuf), None, d["x"], st,
                            torch.empty(M, C_, device="cuda"), gate=hbuf)
    assert not torch.isnan(fr.view).any()
    fr.check(fr.view.clone(), "mlp frame")
    fs.check(fr.view, "mlp with / without stats_out")
    od = fr.view.double()                                  # the statistics of the rows the kernel wrote, at the existing 1e-5
    assert torch.isnan(sto[M]).all()
    assert relerr(sto[:M, 0], od.mean(1)) < 1e-5 and relerr(sto[:M, 1], (od.var(1, unbiased=False) + 1e-5).rsqrt()) < 1e-5
    e_k, e_e, e0 = relerr(fr.view, full), relerr(emul, full), relerr(y0.view, full)
    r_k = rms_rel(fr.view, full)
    print(f"mlp {M}x{C_}x{hidden}: kernel {e_k:.2e}, emulation {e_e:.2e}, ratio {e_k / e_e:.2f}; mode 0 {e0:.2e}; "
          f"rms {r_k:.2e} (bound {PSNR_RMS_BOUND:.1e}; at 30 dB {PSNR_RMS_BOUND_30DB:.1e})")
    assert e0 < 2e-6
    assert e_k <= 2 * e_e
    assert r_k <= PSNR_RMS_BOUND


def wmsa_chain(x, gamma, beta, wq, bq, wp, bp, table, s, B, H, W, heads, shift, lead):
    """float64 out of the W-MSA half (test_gpu_wmsa_f16.ref_wmsa) with the LayerNorm affine folded into the qkv Linear; lead:
    every contraction input rounded to its leading fp16 plane -- xn at the a-priori scale, Wqkv / Wproj per row, q and k per
    (token, head) row, P per query row, v per head-dim COLUMN of the window, the attention output per token row."""
    T, Cc = x.shape
    D = Cc // heads
    r = (lambda t: LP.lead_f16_rows(t.float())[0]) if lead else (lambda t: t)
    xd = x.double()
    xn = F.layer_norm(xd, (Cc,), eps=1e-5)
    wqf = (wq * gamma[None, :])
    bqf = bq.double() + wq.double() @ beta.double()
    if lead:
        xn = LP.round_f16_at(xn.float(), LP.nth2_apriori_exponent(Cc))
    qkv = xn @ r(wqf).double().t() + bqf
    t = qkv.reshape(B, H, W, 3 * Cc)
    if shift:
        t = torch.roll(t, shifts=(-shift, -shift), dims=(1, 2))
    xw = O.window_partition(t, 8).reshape(-1, 64, 3, heads, D).permute(2, 0, 3, 1, 4)      # [3][win][head][64][D]
    q, k, v = xw[0] * D ** -0.5, xw[1], xw[2]
    if lead:
        q, k = r(q), r(k)
        v = r(v.transpose(-2, -1)).transpose(-2, -1)
    att = q @ k.transpose(-2, -1)
    rpi = O.relative_position_index(8)
    att = att + table.double()[rpi.reshape(-1)].reshape(64, 64, heads).permute(2, 0, 1)[None]
    if shift:
        m = O.shifted_window_mask(H, W, 8, shift).to(att.dtype)
        att = (att.reshape(B, m.shape[0], heads, 64, 64) + m[None, :, None]).reshape(-1, heads, 64, 64)
    P = r(att.softmax(-1))
    o = (P @ v).transpose(1, 2).reshape(-1, 8, 8, Cc)
    o = O.window_reverse(o, 8, H, W)
    if shift:
        o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    a = r(o.reshape(T, Cc))
    y = a @ r(wp).double().t() + bp.double()
    if s is not None:
        y = y * s.double().repeat_interleave(H * W)[:, None]
    return xd + y


@pytest.mark.parametrize("B,H,W,C_,heads,shift,drop", [(1, 8, 8, 180, 6, 0, False), (2, 16, 24, 180, 6, 4, True),
                                                       (1, 16, 24, 60, 6, 4, False), (1, 16, 16, 160, 5, 4, True)])
def test_wmsa_f16_under_mode_1(ops, B, H, W, C_, heads, shift, drop):
    assert ops.wattn_f16_ok(C_, heads)
    T = B * H * W
    g = C.gen_for(f"wmsa-{B}-{H}-{W}-{C_}-{heads}-{shift}")
    rnd = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale
    x = rnd(T, C_) * 1.5 + rnd(T, 1)
    gamma, beta = 1 + rnd(C_, scale=0.2), rnd(C_, scale=0.2)
    wq, bq, wp, bp = rnd(3 * C_, C_, scale=0.12), rnd(3 * C_, scale=0.3), rnd(C_, C_, scale=0.1), rnd(C_, scale=0.3)
    table = rnd(225, heads, scale=0.5)
    s = torch.rand(B, generator=g) + 0.5 if drop else None
    d = {k: v.cuda() for k, v in dict(x=x, gamma=gamma, beta=beta, wq=wq, bq=bq, wp=wp, bp=bp, table=table).items()}
    sd = None if s is None else s.cuda()
    Pq, Pp = ops.Bx3(3 * C_, C_, "cuda"), ops.Bx3(C_, C_, "cuda")
    bqf = torch.empty(3 * C_, device="cuda")
    biasF, biasG = torch.empty(heads, 64, 64).cuda(), torch.empty(heads, 64, 64).cuda()
    tb = ops.PrepTable()
    tb.linear(d["wq"], Pq, gamma=d["gamma"], f16=True)
    tb.linear(d["wp"], Pp, f16=True)
    tb.fold_bias(d["wq"], d["bq"], d["beta"], bqf)
    tb.build("cuda").run()
    ops.bias_expand_f16(d["table"], biasF, biasG)
    st = torch.empty(T, 2, device="cuda")
    ops.layernorm_fwd(d["x"], st)
    full = wmsa_chain(x, gamma, beta, wq, bq, wp, bp, table, s, B, H, W, heads, shift, False)
    emul = wmsa_chain(x, gamma, beta, wq, bq, wp, bp, table, s, B, H, W, heads, shift, True)
    y0, a0 = torch.empty(T, C_, device="cuda"), torch.empty(T, C_, device="cuda")
    ops.wmsa_fwd_f16(d["x"], st, Pq, bqf, Pp, d["bp"], biasF, None, a0, y0, B, H, W, heads, shift, rowscale=sd)
    with ops.amp_inference():
        outs = []
        for with_qkv, with_stats in ((False, False), (True, False), (False, True)):
            fo = torch.full((T + 2, C_), NAN, device="cuda")
            fa = torch.full((T + 2, C_), NAN, device="cuda")
            fq = torch.full((T + 2, 3 * C_), NAN, device="cuda")
            sto = torch.full((T + 1, 2), NAN, device="cuda")
            ops.wmsa_fwd_f16(d["x"], st, Pq, bqf, Pp, d["bp"], biasF, fq[1:T + 1] if with_qkv else None, fa[1:T + 1],
                             fo[1:T + 1], B, H, W, heads, shift, rowscale=sd, stats_out=sto[:T] if with_stats else None)
            for f in (fo, fa) + ((fq,) if with_qkv else ()):          # every row written, nothing outside
                assert not torch.isnan(f[1:T + 1]).any() and torch.isnan(f[0]).all() and torch.isnan(f[T + 1]).all()
            if with_stats:        # the statistics of the rows the kernel wrote, at the existing 1e-5
                assert torch.isnan(sto[T]).all()
                od = fo[1:T + 1].double()
                assert relerr(sto[:T, 0], od.mean(1)) < 1e-5 and relerr(sto[:T, 1], (od.var(1, unbiased=False) + 1e-5).rsqrt()) < 1e-5
            outs.append((fo[1:T + 1], fa[1:T + 1]))
    for o, a in outs[1:]:
        assert torch.equal(o, outs[0][0]) and torch.equal(a, outs[0][1])
    y1 = outs[0][0]
    e_k, e_e, e0 = relerr(y1, full), relerr(emul, full), relerr(y0, full)
    r_k = rms_rel(y1, full)
    print(f"wmsa {B}x{H}x{W}x{C_} heads {heads} shift {shift}: kernel {e_k:.2e}, emulation {e_e:.2e}, ratio {e_k / e_e:.2f}; "
          f"mode 0 {e0:.2e}; rms {r_k:.2e} (bound {PSNR_RMS_BOUND:.1e}; at 30 dB {PSNR_RMS_BOUND_30DB:.1e})")
    assert e0 < 2e-6
    assert e_k <= 2 * e_e
    assert r_k <= PSNR_RMS_BOUND
