"""GPU parity tests of the tape-net op kernels, one entry point at a time: nlsa.hip, tape_ops.hip, act_ops.hip,
omni_ops.hip and dfca.hip, called through srhip.ops (ops.call on the C-ABI where a wrapper hides an argument), against the
plain statements of tests/tape_op_refs.py evaluated in float64 on the CPU (backward: float64 autograd of the forward
statement).  tests/test_cpu_tape_op_refs.py pins those statements.

Gate (class Gates): every comparison also evaluates the same statement in float32 on the same inputs; with e the kernel's
and e32 the float32 statement's largest distance from float64, both relative to the float64 result's largest entry, the
test asserts e <= min(ceiling, factor * e32) and prints both.  Ceilings are the suite's existing ones: 2e-5 for
contractions (tests/test_gpu_kernels.py), 2e-6 for element-wise and row-normalisation kernels
(test_layernorm_rows_backward_kernel).  factor is 3, the suite's convention for a different summation order.  The index
kernel and the copies (reflection padding, crop, axpby2d with b = 0) are torch.equal.

The least e32 the gate reckons with is 2 ** -24 (half an ulp of the largest entry): where the float32 statement happens to be
exact -- a one-column softmax, a row of equal values, F.normalize of a one-column row -- or is a sample of one value, its own
distance from float64 is 0 or luck, and a float32 kernel that rounds once more cannot be nearer than its own rounding.  Every
such case measured here (softmax n = 64 R = 1, softmax_rows_bwd n = 1, rowdot n = 441 R = 1, l2norm C = 1) sits within 2.5
roundings; 3 x 2 ** -24 = 1.8e-7 is a tenth of the tighter ceiling, so the floor widens nothing a ceiling does not already
bound ten times wider.
rowdot's factor is 10: measured e / e32 = 3.9 (n = 4096, R = 5, where e32 is the worst of five sums).  The cause is order alone:
the kernel adds 64 sequential lane sums by a butterfly, aten's sum is a vectorised pairwise cascade; its e stays below 2.4e-7
of the largest dot wherever the dots do not cancel.

Measured on an MI355X, the worst over every case of a kernel (e and e32 relative to the float64 result's largest entry;
e / e32 with e32 floored as above):

    kernel                                         worst e worst e32 worst e / e32
    nlsa_attention (mfma) ret                      1.8e-06   1.7e-06          1.64
    nlsa_attention (mfma) score                    4.1e-07   4.0e-07          1.62
    nlsa_attention (mfma) out                      5.8e-07   3.2e-07          2.09
    nlsa_attention (scalar) ret                    6.6e-07   1.0e-06          0.82
    nlsa_attention (scalar) score                  2.1e-07   3.0e-07          1.58
    nlsa_attention (scalar) out                    2.3e-07   3.2e-07          1.00
    softmax_rows / _lse P                          1.0e-07   1.1e-07          1.00
    softmax_rows / _lse lse                        4.6e-08   6.0e-08          0.77
    softmax_rows_bwd                               3.1e-07   4.0e-07          2.47
    rowdot                                         8.8e-06   1.1e-05          3.92
    l2norm_rows_train factors                      1.7e-07   2.1e-07          1.01
    l2norm_rows (clamped rows)                     6.8e-08   1.0e-07          1.00
    l2norm_rows_bwd (clamped rows)                 7.5e-08   1.3e-07          0.72
    l2norm_rows (near eps)                         7.5e-08   1.1e-07          1.07
    l2norm_rows_bwd (near eps)                     1.5e-07   1.3e-07          2.51
    l2norm_rows                                    1.6e-07   1.5e-07          2.24
    l2norm_rows_bwd                                1.6e-07   1.8e-07          1.37
    performer_features                             2.9e-07   3.4e-07          0.85
    performer_features_bwd                         3.2e-07   2.5e-07          2.71
    performer chain features                       1.2e-06   2.7e-06          1.00
    performer chain dx                             1.1e-06   2.2e-06          0.98
    enlca_finish                                   4.6e-08   6.0e-08          0.78
    enlca_finish_bwd                               1.3e-07   1.7e-07          1.22
    layernorm_rows                                 1.2e-07   1.3e-07          1.18
    layernorm_rows_res                             1.2e-07   1.1e-07          1.32
    layernorm_rows (two-pass form)                 9.9e-08   1.2e-07          0.81
    unary gelu                                     3.7e-08   9.8e-08          0.38
    unary gelu_bwd                                 9.2e-08   1.6e-07          0.56
    unary sigmoid                                  8.9e-08   8.9e-08          1.00
    unary sigmoid_bwd                              3.2e-07   3.2e-07          1.00
    fft2_mag_pow_shift                             1.4e-07   2.4e-07          0.88
    fft2_mag_pow_shift_bwd                         2.2e-07   1.5e-06          0.41
    channel_gate (one block)                       2.7e-07   1.7e-07          2.34
    channel_gate (64 partial blocks)               3.4e-07   2.3e-07          2.68
    dwconv3x3 (v4)                                 1.9e-07   1.6e-07          1.33
    dwconv3x3 (scalar)                             1.0e-07   1.0e-07          1.06
    group_attention                                4.6e-07   4.6e-07          1.19
    channel_attention (staged)                     2.3e-07   1.8e-07          1.24
    channel_attention (multi-pass)                 2.3e-07   2.2e-07          1.25
    gelu_gate                                      4.7e-08   6.0e-08          0.79
    mul_sigmoid                                    8.1e-08   9.9e-08          0.92
    bilinear_resize                                9.6e-07   9.6e-07          1.25
    prelu_bwd dx                                   0.0e+00   6.0e-08          0.00
    prelu_bwd dalpha                               3.6e-08   2.3e-07          0.60
    axpby2d                                        9.4e-08   9.4e-08          1.00
    pad_reflect1 adjoint                           8.1e-08   1.6e-07          1.05
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import tape_op_refs as R  # noqa: E402

CONTRACTION, ELEMENTWISE = 2e-5, 2e-6
F32_ROUNDING = 2.0 ** -24          # half an ulp of the largest entry: the least e32 the gate reckons with (module docstring)
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from srhip import ops as _ops
    return _ops


def gen(seed):
    return torch.Generator().manual_seed(seed)


def f64(*ts):
    return [None if t is None else t.detach().double().cpu() for t in ts]


def f32(*ts):
    return [None if t is None else t.detach().float().cpu() for t in ts]


def pitched(t, ld):
    """[R, ld] device buffer full of NaN whose first t.shape[1] columns hold t; returns (buffer, view)"""
    buf = torch.full((t.shape[0], ld), NAN, device="cuda")
    buf[:, :t.shape[1]] = t.cuda()
    return buf, buf[:, :t.shape[1]]


def nan_tail(buf, n):
    return buf.shape[1] == n or bool(torch.isnan(buf[:, n:]).all())


class Gates:
    """collects the comparisons of one test, prints every figure, and fails at the end with all that missed"""

    def __init__(self, name):
        self.name, self.bad = name, []

    def __enter__(self):
        return self

    def __call__(self, got, ref64, ref32, ceiling, what, factor=3, scale=None):
        got, ref64, ref32 = f64(got, ref64, ref32)
        assert got.shape == ref64.shape == ref32.shape, (what, got.shape, ref64.shape)
        s = (ref64.abs().max().item() if scale is None else scale) + 1e-300
        e = (got - ref64).abs().max().item() / s
        e32 = max((ref32 - ref64).abs().max().item() / s, F32_ROUNDING)
        print(f"[gate] {self.name} {what}: kernel {e:.3e} fp32 {e32:.3e} ratio {e / e32:.2f}")
        if not e <= min(ceiling, factor * e32):                # (a NaN fails)
            self.bad.append(f"{what}: kernel {e:.3e} > min({ceiling:g}, {factor} x {e32:.3e})")

    def equal(self, a, b, what):
        if not torch.equal(a.cpu(), b.cpu()):
            self.bad.append(f"{what}: not bit-equal")

    def true(self, cond, what):
        if not cond:
            self.bad.append(what)

    def __exit__(self, et, ev, tb):
        if et is None:
            assert not self.bad, self.name + ":\n  " + "\n  ".join(self.bad)
        return False


# ------------------------------------------------------------------ srhip_nlsa_order
def _call_order(ops, rotated, ld, N, L, nh, hb):
    buf, view = pitched(rotated, ld)
    keys = torch.full((N * nh * L,), -1, dtype=torch.int64, device="cuda")
    order = torch.full((N, nh, L), -1, dtype=torch.int64, device="cuda")
    ws = torch.zeros(16, device="cuda")
    ops.call("srhip_nlsa_order", buf.data_ptr(), buf.stride(0), keys.data_ptr(), order.data_ptr(), ws.data_ptr(), 64, N, L, nh, hb,
             ops._st())
    torch.cuda.synchronize()
    return order


def _rotated(kind, N, L, nh, hb, g):
    """values on multiples of 1/8: the argmax is the same on CPU and GPU bit for bit, and exact ties exist by construction"""
    hbh = hb // 2
    if kind == "uniform":
        r = torch.randint(-16, 17, (N * L, nh * hbh), generator=g).float() / 8
        r[0] = 0.0                                             # an all-zero row: code 0
        if hbh > 1:
            r[1] = 0.0; r[1, 0] = 0.5; r[1, 1] = -0.5          # r_0 ties -r_1: the r half wins
            r[2] = 0.0; r[2, 0] = -0.5; r[2, 1] = 0.5          # r_1 ties -r_0
            r[3] = 2.0                                         # every r equal
            r[4] = -2.0                                        # every -r equal
        return r
    r = torch.zeros(N * L, nh, hbh)
    if kind == "one_code":
        r[:, :, hbh - 1] = -1.0                                # every token: code hb - 1
    else:                                                      # "descending": the code falls as the token index rises
        tokn = torch.arange(N * L) % L
        code = hb - 1 - (tokn * hb) // L
        idx = (code % hbh).view(-1, 1, 1).expand(-1, nh, 1)
        r.scatter_(2, idx, torch.where(code < hbh, 1.0, -1.0).view(-1, 1, 1).expand(-1, nh, 1).contiguous())
    return r.reshape(N * L, nh * hbh)


@pytest.mark.parametrize("N,nh", [(1, 1), (2, 4)])
@pytest.mark.parametrize("hb", [2, 28, 128])
@pytest.mark.parametrize("L", [100, 1024, 1025, 4096, 5000])
def test_nlsa_order(ops, L, hb, N, nh):
    """srhip_nlsa_order (k_lsh_keys + k_bucket_order) against lsh_order, the whole int64 order bit for bit, no case
    excluded.  L = 100 / 1024: one tile of BO_T = 1024 tokens (partial / full); 1025: a full first tile and one token in
    the last; 4096 (the bench patch), 5000: four / five tiles, so the `tokens of that code in earlier tiles` and `earlier
    waves` terms carry.  Histograms: uniform random codes with an all-zero row, r and -r tying and all-equal rows; every
    token in one code (one bucket of L, 127 empty); codes descending in token order (the sort reverses the blocks)."""
    with Gates(f"nlsa_order L={L} hb={hb} N*nh={N * nh}") as G:
        for kind in ("uniform", "one_code", "descending"):
            rot = _rotated(kind, N, L, nh, hb, gen(L + hb))
            ref = R.lsh_order(rot, N, L, nh, hb)
            got = _call_order(ops, rot, rot.shape[1] + 3, N, L, nh, hb)
            G.equal(got, ref, kind)
            G.equal(_call_order(ops, rot, rot.shape[1], N, L, nh, hb), got, kind + " (second call, contiguous)")


def test_nlsa_order_errors(ops):
    """`hash_buckets >= 2 && hash_buckets % 2 == 0 && hash_buckets <= BO_HB` (128) and `L < (1 << TOK_BITS)`: refused before
    any launch"""
    buf = torch.zeros(4 * 128, device="cuda")
    for L, hb in ((4, 3), (4, 130), (4, 0), (1 << 20, 2)):
        with pytest.raises(ops.SrhipError):
            ops.call("srhip_nlsa_order", buf.data_ptr(), 128, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 64, 1, L, 1, hb,
                     ops._st())


# ------------------------------------------------------------------ srhip_nlsa_attention
def _call_nlsa(ops, xe, ye, order, x, N, L, cs, res_scale):
    Ce, Cy, nh = xe.shape[1], ye.shape[1], order.shape[1]
    ret = torch.full((N, nh, L, Cy), NAN, device="cuda")
    score = torch.full((N, nh, L), NAN, device="cuda")
    out = torch.full((N * L, Cy), NAN, device="cuda")
    ops.call("srhip_nlsa_attention", xe.data_ptr(), ye.data_ptr(), order.data_ptr(), ret.data_ptr(), score.data_ptr(), x.data_ptr(),
             out.data_ptr(), N, L, Ce, Cy, nh, cs, float(res_scale), ops._st())
    torch.cuda.synchronize()
    return out, ret, score


MFMA = "mfma"      # Cy % 32 == 0 && Cy <= 256 && cs % 8 == 0 && Ce % 4 == 0
SCALAR = "scalar"  # anything else
NLSA_CASES = [
    # (N, L, Ce, Cy, nh, cs, embedding scale, arm)
    (2, 720, 16, 64, 4, 144, 1.0, MFMA),       # the narrow golden width, five chunks, no padding
    (1, 4096, 64, 256, 4, 144, 1.0, MFMA),     # the bench patch: 29 chunks, padding 80, all eight waves live in P V
    (1, 144, 64, 256, 4, 144, 1.0, MFMA),      # nchunks 1: own = back = forward
    (1, 288, 64, 64, 2, 144, 1.0, MFMA),       # nchunks 2: back = forward
    (2, 150, 8, 32, 2, 144, 1.0, MFMA),        # padding 138; Cy = 32: one wave live in P V; Ce = 8: one group of 8
    (1, 210, 16, 64, 2, 40, 1.0, MFMA),        # cs = 40: a partial 32-column tile, NG = 15 (not a multiple of 4)
    (1, 60, 4, 32, 2, 8, 1.0, MFMA),           # cs = 8: nq = 8 < MQ, NG = 3; Ce = 4: half a group of 8
    (1, 300, 60, 96, 2, 40, 1.0, MFMA),        # Ce = 60: not a multiple of 8; three waves live
    (2, 720, 16, 64, 4, 144, 1e-6, MFMA),      # every key norm below 5e-5: the clamped normalise
    (2, 720, 16, 64, 4, 144, 3.0, MFMA),       # sharp softmax
    (2, 720, 16, 64, 4, 144, "mixed", MFMA),   # key norms 2e-5 (clamped), 2e-4 (just above eps) and 4 in turn
    (1, 300, 16, 33, 2, 40, 1.0, SCALAR),      # Cy = 33
    (1, 200, 16, 288, 2, 40, 1.0, SCALAR),     # Cy = 288 > 256: two passes of the channel loop
    (2, 100, 8, 64, 2, 36, 1.0, SCALAR),       # cs = 36: QT = 48 > cs, K3 = 108, K3 % 8 == 4 tail
    (1, 130, 7, 64, 2, 52, 1.0, SCALAR),       # cs = 52: a second query tile of 4 rows; Ce = 7
    (1, 300, 64, 40, 2, 144, 1.0, SCALAR),     # Ce = 64, cs = 144: 136 KB of LDS, the reservation path
    (1, 300, 16, 33, 2, 40, 1e-6, SCALAR),
    (1, 300, 16, 33, 2, 40, 3.0, SCALAR),
    (1, 300, 16, 33, 2, 40, "mixed", SCALAR),
]


@pytest.mark.parametrize("N,L,Ce,Cy,nh,cs,escale,arm", NLSA_CASES)
def test_nlsa_attention(ops, N, L, Ce, Cy, nh, cs, escale, arm):
    """srhip_nlsa_attention: ret, score and out against nlsa_core in float64 under a random permutation per round as the
    order.  Arms: `Cy % 32 == 0 && Cy <= 32 * MW && chunk_size % 8 == 0 && Ce % 4 == 0` takes k_nlsa_attention_mfma, anything
    else k_nlsa_attention (the scalar form); see NLSA_CASES for what each shape reaches.  Embedding scale 1e-6: every key norm is
    below eps = 5e-5; 3: a sharp softmax; "mixed": row norms on both sides of eps under queries large enough for the clamp to show.  ret / score / out are NaN before the
    call (padded rows are never written twice, unpadded ones exactly once); two calls give the same bits."""
    assert (arm == MFMA) == (Cy % 32 == 0 and Cy <= 256 and cs % 8 == 0 and Ce % 4 == 0)
    g = gen(L * 7 + Ce + Cy + cs)
    xe = torch.randn(N * L, Ce, generator=g)
    if escale == "mixed":       # with every row tiny the scores vanish whatever eps is; large queries against tiny keys show it
        norms = torch.tensor([2e-5, 2e-4, 4.0]).repeat(N * L // 3 + 1)[:N * L]
        xe = (xe.double() / xe.double().norm(dim=1, keepdim=True) * norms[:, None].double()).float()
    else:
        xe = xe * escale
    ye, x = torch.randn(N * L, Cy, generator=g), torch.randn(N * L, Cy, generator=g)
    tok = torch.stack([torch.stack([torch.randperm(L, generator=g) for _ in range(nh)]) for _ in range(N)])
    grp = (torch.arange(N).view(N, 1, 1) * nh + torch.arange(nh).view(1, nh, 1)) * 128 + 5
    order = ((grp << R.TOK_BITS) | tok).cuda()
    res_scale = 0.5
    out, ret, score = _call_nlsa(ops, xe.cuda(), ye.cuda(), order, x.cuda(), N, L, cs, res_scale)
    out2, ret2, score2 = _call_nlsa(ops, xe.cuda(), ye.cuda(), order, x.cuda(), N, L, cs, res_scale)

    def ref(dt):
        return R.nlsa_core(xe.to(dt).view(N, L, Ce), ye.to(dt).view(N, L, Cy), tok, x.to(dt).view(N, L, Cy), cs, res_scale)
    (o64, r64, s64), (o32, r32, s32) = ref(torch.float64), ref(torch.float32)
    with Gates(f"nlsa_attention[{arm}] {(N, L, Ce, Cy, nh, cs)} x{escale}") as G:
        G.true(torch.equal(out, out2) and torch.equal(ret, ret2) and torch.equal(score, score2), "two calls differ")
        G(ret, r64, r32, CONTRACTION, "ret")
        G(score, s64, s32, CONTRACTION, "score")
        G(out.view(N, L, Cy), o64, o32, CONTRACTION, "out")


def test_nlsa_attention_errors(ops):
    """`chunk_size % 4 == 0`, `Ce <= CE_MAX` (64), `L >= chunk_size`"""
    for L, Ce, cs in ((64, 8, 6), (64, 68, 8), (16, 8, 32)):
        xe, ye = torch.zeros(L, Ce, device="cuda"), torch.zeros(L, 32, device="cuda")
        order = torch.arange(L, device="cuda").view(1, 1, L)
        with pytest.raises(ops.SrhipError):
            _call_nlsa(ops, xe, ye, order, ye, 1, L, cs, 1.0)


# ------------------------------------------------------------------ softmax_rows, softmax_rows_lse, softmax_rows_bwd, rowdot
def _logits(Rr, n, g):
    x = torch.randn(Rr, n, generator=g) * 3
    if Rr == 1:
        x *= 1e4 / 3                                           # a softmax without the max subtraction overflows
    else:
        x[1] = 2.5                                             # a row of equal values
        x[2] *= 1e4 / 3
    return x


@pytest.mark.parametrize("Rr", [1, 5, 1003])
@pytest.mark.parametrize("n,ld", [(1, 4), (3, 3), (63, 66), (64, 64), (65, 68), (432, 435), (441, 444), (4096, 4099)])
def test_softmax_rows_and_lse(ops, n, ld, Rr):
    """srhip_softmax_rows / srhip_softmax_rows_lse (one wave per row, four rows per block: R = 1, 5, 1003 leave waves idle;
    n on both sides of 64; pitch ld > n with NaN padding that must stay NaN) against softmax / logsumexp(scale x), scale
    0.37; a row of equal values, rows of magnitude 1e4."""
    x = _logits(Rr, n, gen(n * 13 + Rr))
    scale = 0.37
    b1, v1 = pitched(x, ld)
    ops.softmax_rows_(v1, scale)
    b2, v2 = pitched(x, ld)
    lse = torch.full((Rr,), NAN, device="cuda")
    ops.softmax_rows_lse_(v2, lse, scale)
    p64, l64 = R.softmax_rows_lse(x.double(), scale)
    p32, l32 = R.softmax_rows_lse(x, scale)
    with Gates(f"softmax_rows n={n} R={Rr}") as G:
        G.true(nan_tail(b1, n) and nan_tail(b2, n), "padding columns overwritten")
        G(v1, p64, p32, ELEMENTWISE, "softmax_rows")
        G(v2, p64, p32, ELEMENTWISE, "softmax_rows_lse P")
        G(lse, l64, l32, ELEMENTWISE, "softmax_rows_lse lse")
        G.equal(v1, v2, "softmax_rows vs softmax_rows_lse bits")


@pytest.mark.parametrize("Rr", [1, 5, 1003])
@pytest.mark.parametrize("n,ld", [(1, 4), (3, 3), (63, 66), (64, 64), (65, 68), (432, 435), (441, 444), (4096, 4099)])
def test_softmax_rows_bwd_and_rowdot(ops, n, ld, Rr):
    """srhip_softmax_rows_bwd with and without dlse against float64 autograd of (softmax, logsumexp)(x); srhip_rowdot on the
    same pitched operands against sum_c a b.  P given to the kernel is the float32 statement's softmax."""
    g = gen(n * 17 + Rr)
    x = torch.randn(Rr, n, generator=g) * 2
    dP, dlse = torch.randn(Rr, n, generator=g), torch.randn(Rr, generator=g)
    P = torch.softmax(x, dim=-1)
    with Gates(f"softmax_rows_bwd n={n} R={Rr}") as G:
        for with_lse in (True, False):
            bP, vP = pitched(P, ld)
            bD, vD = pitched(dP, ld)
            ops.softmax_rows_bwd_(vP, vD, dlse.cuda() if with_lse else None)

            def ref(dt):
                gl = dlse.to(dt) if with_lse else torch.zeros(Rr, dtype=dt)
                return R.vjp(lambda t: R.softmax_rows_lse(t), (x.to(dt),), (dP.to(dt), gl))[0]
            G.true(nan_tail(bD, n), "padding columns overwritten")
            G(vD, ref(torch.float64), ref(torch.float32), ELEMENTWISE, f"ds (dlse {with_lse})")
        bA, vA = pitched(x, ld)
        bB, vB = pitched(dP, ld + 4)
        out = torch.full((Rr,), NAN, device="cuda")
        ops.rowdot(vA, vB, out)
        G(out, R.rowdot(x.double(), dP.double()), R.rowdot(x, dP), CONTRACTION, "rowdot", factor=10)


# ------------------------------------------------------------------ l2norm_rows, l2norm_rows_train, l2norm_rows_bwd
EPS = 5e-5


def _l2_rows(T, C, g):
    """row 0 zero, row 1 of norm eps / 2 (clamped); rows 2, 3 of norm eps (1 + 1e-3), 2 eps (just above); the rest ordinary"""
    x = torch.randn(T, C, generator=g)
    x[0] = 0.0
    for r, nrm in ((1, 0.5 * EPS), (2, EPS * (1 + 1e-3)), (3, 2 * EPS)):
        x[r] = (x[r].double() / x[r].double().norm() * nrm).float()
    return x


L2_GROUPS = (("clamped", slice(0, 2)), ("near eps", slice(2, 4)), ("ordinary", slice(4, None)))


@pytest.mark.parametrize("k", [1.0, math.sqrt(6)])
@pytest.mark.parametrize("C", [1, 16, 63, 64, 65, 256])
def test_l2norm_rows_forward_and_backward(ops, C, k):
    """srhip_l2norm_rows / _train / _bwd against k * F.normalize(x, eps = 5e-5) and its float64 autograd; T = 1003 rows (not
    a multiple of 4), pitch C + 3 with NaN padding.  Gated per group of rows, because the clamped rows' gradient k / eps
    is 1e4 times the ordinary rows': zero and below-eps rows (`f < k / eps` false: dx = f dy), rows just above eps and
    ordinary rows (the projection).  C == 1: the true gradient of an unclamped row is zero, so the backward's scale there is
    the unprojected gradient |f dy| instead of the output's largest entry."""
    T = 1003
    g = gen(C * 3 + int(k * 10))
    x = _l2_rows(T, C, g)
    dy = torch.randn(T, C, generator=g)
    ld = C + 3
    b1, v1 = pitched(x, ld)
    ops.l2norm_rows_(v1, k, EPS)
    b2, v2 = pitched(x, ld)
    fac = torch.full((T,), NAN, device="cuda")
    ops.l2norm_rows_train_(v2, fac, k, EPS)
    bD, vD = pitched(dy, ld + 4)
    ops.l2norm_rows_bwd_(vD, v2, fac, k, EPS)
    y64, y32 = R.l2norm_rows(x.double(), k, EPS), R.l2norm_rows(x, k, EPS)
    f64_ = k / x.double().norm(dim=1).clamp_min(EPS)
    f32_ = k / x.norm(dim=1).clamp_min(EPS)
    d64 = R.vjp(lambda t: R.l2norm_rows(t, k, EPS), (x.double(),), dy.double())[0]
    d32 = R.vjp(lambda t: R.l2norm_rows(t, k, EPS), (x,), dy)[0]
    with Gates(f"l2norm_rows C={C} k={k:.3f}") as G:
        G.true(nan_tail(b1, C) and nan_tail(b2, C) and nan_tail(bD, C), "padding columns overwritten")
        G.equal(v1, v2, "l2norm_rows vs l2norm_rows_train bits")
        G(fac.cpu().double() / f64_, torch.ones(T, dtype=torch.float64), f32_.double() / f64_, ELEMENTWISE, "factors (ratio)")
        for name, rows in L2_GROUPS:
            G(v1[rows], y64[rows], y32[rows], ELEMENTWISE, f"forward, {name} rows")
            sc = (f64_[rows, None] * dy[rows].double()).abs().max().item() if C == 1 else None
            G(vD[rows], d64[rows], d32[rows], ELEMENTWISE, f"backward, {name} rows", scale=sc)


# ------------------------------------------------------------------ performer_features, performer_features_bwd
@pytest.mark.parametrize("Fn,T", [(5, 1004), (128, 1003), (200, 1003)])
def test_performer_features_and_bwd(ops, Fn, T):
    """srhip_performer_features against ratio (exp(dash - |data|^2 / 2) + eps), ratio = F^-1/2, on pitched dash / data (one wave
    per row, F on both sides of 64); srhip_performer_features_bwd alone against float64 autograd with respect to `dash`."""
    C = 40
    g = gen(Fn)
    data = R.l2norm_rows(torch.randn(T, C, generator=g), math.sqrt(6))
    dash = torch.randn(T, Fn, generator=g) * 1.5
    gr = torch.randn(T, Fn, generator=g)
    bD, vD = pitched(dash, Fn + 3)
    bX, vX = pitched(data, C + 4)
    ops.performer_features_(vD, vX)
    f64_, f32_ = R.performer_features(dash.double(), data.double()), R.performer_features(dash, data)
    gd = gr.cuda().clone()
    fk = vD.contiguous()
    ops.performer_features_bwd_(gd, fk)
    d64 = R.vjp(lambda t: R.performer_features(t, data.double()), (dash.double(),), gr.double())[0]
    d32 = R.vjp(lambda t: R.performer_features(t, data), (dash,), gr)[0]
    with Gates(f"performer_features F={Fn}") as G:
        G.true(nan_tail(bD, Fn), "padding columns overwritten")
        G(vD, f64_, f32_, ELEMENTWISE, "forward")
        G(gd, d64, d32, ELEMENTWISE, "backward with respect to dash")


@pytest.mark.parametrize("C,Fn", [(40, 128), (64, 200)])
def test_performer_chain_backward(ops, C, Fn):
    """l2norm_rows_train -> gemm -> performer_features -> performer_features_bwd -> gemm -> l2norm_rows_bwd against float64
    autograd of the whole composite with respect to the UN-normalised rows (unclamped): holds k_performer_features_bwd's
    claim that the |data|^2 / 2 path needs no gradient because the normalisation in front projects it out."""
    T, k = 1003, math.sqrt(6)
    g = gen(C + Fn)
    x = torch.randn(T, C, generator=g) * 0.7
    proj = torch.randn(Fn, C, generator=g)
    gr = torch.randn(T, Fn, generator=g)
    y = x.cuda().clone()
    fac = torch.empty(T, device="cuda")
    ops.l2norm_rows_train_(y, fac, k, EPS)
    dash = ops.mm(y, proj.cuda(), tb=True)
    f = ops.performer_features_(dash, y)
    gd = ops.performer_features_bwd_(gr.cuda().clone(), f)
    dx = ops.l2norm_rows_bwd_(ops.mm(gd, proj.cuda()), y, fac, k, EPS)
    f64_, f32_ = R.performer_chain(x.double(), proj.double(), k), R.performer_chain(x, proj, k)
    d64 = R.vjp(lambda t: R.performer_chain(t, proj.double(), k), (x.double(),), gr.double())[0]
    d32 = R.vjp(lambda t: R.performer_chain(t, proj, k), (x,), gr)[0]
    with Gates(f"performer chain C={C} F={Fn}") as G:
        G(f, f64_, f32_, CONTRACTION, "features")
        G(dx, d64, d32, CONTRACTION, "gradient of the un-normalised rows")


# ------------------------------------------------------------------ enlca_finish, enlca_finish_bwd
@pytest.mark.parametrize("extra", [1, 4])
@pytest.mark.parametrize("Cy", [40, 64, 256])
def test_enlca_finish_and_bwd(ops, Cy, extra):
    """srhip_enlca_finish / _bwd against x + res_scale num[:, :Cy] / num[:, Cy] and its float64 autograd with respect to num;
    ldn = Cy + 1 and Cy + 4 (the extra columns of num hold NaN going in -- never read -- and dnum must hold zero there)."""
    T, rs = 1003, 0.1
    g = gen(Cy + extra)
    num = torch.randn(T, Cy + extra, generator=g)
    num[:, Cy] = torch.rand(T, generator=g) + 0.5
    x, dout = torch.randn(T, Cy, generator=g), torch.randn(T, Cy, generator=g)
    numk = num.clone()
    numk[:, Cy + 1:] = NAN
    out = torch.full((T, Cy), NAN, device="cuda")
    ops.enlca_finish(numk.cuda(), x.cuda(), out, rs)
    dnum = torch.full((T, Cy + extra), NAN, device="cuda")
    ops.enlca_finish_bwd(dout.cuda(), numk.cuda(), dnum, rs)
    d64 = R.vjp(lambda t: R.enlca_finish(t, x.double(), rs), (num.double(),), dout.double())[0]
    d32 = R.vjp(lambda t: R.enlca_finish(t, x, rs), (num,), dout)[0]
    with Gates(f"enlca_finish Cy={Cy} ldn=Cy+{extra}") as G:
        G(out, R.enlca_finish(num.double(), x.double(), rs), R.enlca_finish(num, x, rs), ELEMENTWISE, "forward")
        G.true(bool((dnum[:, Cy + 1:] == 0).all()), "extra columns of dnum not zero")
        G(dnum[:, :Cy], d64[:, :Cy], d32[:, :Cy], ELEMENTWISE, "dnum[:, :Cy]")
        G(dnum[:, Cy], d64[:, Cy], d32[:, Cy], CONTRACTION, "dnum[:, Cy] (a row dot)")


# ------------------------------------------------------------------ layernorm_rows, layernorm_rows_res
@pytest.mark.parametrize("C", [1, 60, 64, 180, 255, 256, 257])
def test_layernorm_rows_and_res(ops, C):
    """srhip_layernorm_rows: `C <= 256` takes k_layernorm_rows_reg (the row in registers), 257 takes k_layernorm_rows (two
    passes over the row); srhip_layernorm_rows_res (k_layernorm_rows_reg with a residual) up to 256 and its `C <= 256`
    error.  M = 1003 rows, pitched x / res / out with NaN padding, out aliasing x and aliasing res."""
    M = 1003
    g = gen(C)
    x = torch.randn(M, C, generator=g) * 2 + 0.5
    res = torch.randn(M, C, generator=g)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    y64, y32 = R.layernorm_rows(x.double(), gamma.double(), beta.double()), R.layernorm_rows(x, gamma, beta)
    r64 = R.layernorm_rows(x.double(), gamma.double(), beta.double(), res=res.double())
    r32 = R.layernorm_rows(x, gamma, beta, res=res)
    gm, bt = gamma.cuda(), beta.cuda()
    with Gates(f"layernorm_rows C={C}") as G:
        bx, vx = pitched(x, C + 3)
        bo, vo = pitched(torch.full((M, C), NAN), C + 5)
        ops.layernorm_rows(vx, gm, bt, vo)
        G.true(nan_tail(bo, C), "padding columns overwritten")
        G(vo, y64, y32, ELEMENTWISE, "out")
        ops.layernorm_rows(vx, gm, bt, vx)
        G.true(nan_tail(bx, C), "padding columns overwritten (in place)")
        G.equal(vx, vo, "out aliasing x")
        if C > 256:
            with pytest.raises(ops.SrhipError):
                ops.layernorm_rows_res(vo, vo, gm, bt, vo)
            return
        for alias in ("none", "x", "res"):
            bx, vx = pitched(x, C + 3)
            br, vr = pitched(res, C + 1)
            bo, vo = pitched(torch.full((M, C), NAN), C + 5)
            dst = {"none": vo, "x": vx, "res": vr}[alias]
            ops.layernorm_rows_res(vx, vr, gm, bt, dst)
            G.true(nan_tail(bx, C) and nan_tail(br, C) and nan_tail(bo, C), f"padding columns overwritten (alias {alias})")
            G(dst, r64, r32, ELEMENTWISE, f"res form, out aliasing {alias}")


# ------------------------------------------------------------------ unary, unary_bwd
@pytest.mark.parametrize("kind", ["gelu", "sigmoid"])
def test_unary_and_bwd(ops, kind):
    """srhip_unary / srhip_unary_bwd (GELU from the op's input, sigmoid from its output) over [-12, 12] with +-0 and the far
    negative tail; 2 100 003 elements: past ew_blocks' 8192 blocks of 256, so the grid-stride loop runs again; in place
    (out = x, dx = g)."""
    n = 2_100_003
    g = gen(3)
    x = torch.cat([torch.linspace(-12, 12, n - 6), torch.tensor([0.0, -0.0, -12.0, 12.0, -8.5, 1e-20])])
    gr = torch.randn(n, generator=g)
    xk = x.cuda()
    out = ops.unary(xk, torch.full((n,), NAN, device="cuda"), kind)
    y32 = R.unary(x, kind)
    dx = ops.unary_bwd(xk if kind == "gelu" else y32.cuda(), gr.cuda(), torch.full((n,), NAN, device="cuda"), kind)
    ga = gr.cuda().clone()
    ops.unary_bwd(xk if kind == "gelu" else y32.cuda(), ga, ga, kind)
    d64 = R.vjp(lambda t: R.unary(t, kind), (x.double(),), gr.double())[0]
    d32 = R.vjp(lambda t: R.unary(t, kind), (x,), gr)[0]
    with Gates(f"unary {kind}") as G:
        G(out, R.unary(x.double(), kind), y32, ELEMENTWISE, "forward")
        xi = xk.clone()
        G.equal(ops.unary(xi, xi, kind), out, "in place")
        G(dx, d64, d32, ELEMENTWISE, "backward")
        G.equal(ga, dx, "backward in place on g")
        G.true(bool(torch.isfinite(out).all() and torch.isfinite(dx).all()), "non-finite value")


# ------------------------------------------------------------------ fft2_mag_pow_shift_bwd
@pytest.mark.parametrize("B,H,W,C", [(2, 16, 12, 64), (1, 15, 9, 64), (1, 7, 256, 8), (1, 40, 33, 70), (1, 256, 64, 64)])
def test_fft2_mag_pow_shift_bwd(ops, B, H, W, C):
    """srhip_fft2_mag_pow_shift_bwd against float64 autograd of fftshift2d((|fftn(x)| + 1e-8) ** 0.8): both dimensions odd
    (the quadrant swap at h // 2), W = 256 (the LDS limit), C = 70 (a second, partial group of 64 channels), H = 256.  Channel
    1 is constant: its spectrum is zero off the DC term, where the reference is singular, so forward and backward must be
    finite there (the `|F| = 0` branch) and the value gate covers the other channels.  Twice the same bits."""
    g = gen(H * W + C)
    x = torch.randn(B, H, W, C, generator=g)
    x[..., 1] = 1.5
    gr = torch.randn(B, H, W, C, generator=g)
    xk, gk = x.cuda(), gr.cuda()
    fwd = ops.fft2_mag_pow_shift(xk, torch.full_like(xk, NAN))
    dx = ops.fft2_mag_pow_shift_bwd(xk, gk, torch.full_like(xk, NAN))
    dx2 = ops.fft2_mag_pow_shift_bwd(xk, gk, torch.full_like(xk, NAN))
    keep = [c for c in range(C) if c != 1]
    d64 = R.vjp(R.fft2_mag_pow_shift, (x.double(),), gr.double())[0]
    d32 = R.vjp(R.fft2_mag_pow_shift, (x,), gr)[0]
    with Gates(f"fft2_mag_pow_shift_bwd {(B, H, W, C)}") as G:
        G.true(bool(torch.isfinite(fwd).all()), "forward not finite")
        G.true(bool(torch.isfinite(dx).all()), "backward not finite")
        G.equal(dx, dx2, "two calls")
        G(fwd[..., keep], R.fft2_mag_pow_shift(x.double())[..., keep], R.fft2_mag_pow_shift(x)[..., keep], CONTRACTION, "forward")
        G(dx[..., keep], d64[..., keep], d32[..., keep], CONTRACTION, "dx")


# ------------------------------------------------------------------ channel_gate
@pytest.mark.parametrize("C,Cm", [(20, 4), (64, 64), (256, 4)])
@pytest.mark.parametrize("H,W", [(7, 9), (63, 65), (64, 64), (128, 128)])
def test_channel_gate(ops, H, W, C, Cm):
    """srhip_channel_gate: `P < 4096` pools each sample in one block (P = 63, 4095), otherwise in 64 partial blocks (P =
    4096, 16384: k_pool_partial's p0 / p1 split); C = 20 / 64 / 256 (one partial, one and four groups of 64 channels); both
    mid_act (0 ReLU, 1 SiLU); x0 present and absent; biases present and absent."""
    B = 2
    g = gen(H * W + C + Cm)
    feat = torch.randn(B, H, W, C, generator=g) + 0.3
    x0, x1 = torch.randn(B, H, W, C, generator=g), torch.randn(B, H, W, C, generator=g)
    w1, w2 = torch.randn(Cm, C, generator=g) * C ** -0.5 * 3, torch.randn(C, Cm, generator=g) * Cm ** -0.5 * 2
    b1, b2 = torch.randn(Cm, generator=g), torch.randn(C, generator=g)
    with Gates(f"channel_gate P={H * W} C={C} Cm={Cm}") as G:
        for act, has_x0, has_b in (("relu", True, True), ("silu", False, True), ("silu", True, False), ("relu", False, False)):
            a = [feat, w1, b1 if has_b else None, w2, b2 if has_b else None, x0 if has_x0 else None, x1]
            out = torch.full((B, H, W, C), NAN, device="cuda")
            ops.channel_gate(*[None if t is None else t.cuda() for t in a], out, mid_act=act)
            G(out, R.channel_gate(*f64(*a), mid_act=act), R.channel_gate(*a, mid_act=act), ELEMENTWISE,
              f"{act} x0={has_x0} bias={has_b}")


# ------------------------------------------------------------------ dwconv3x3
def _dw_case(name):
    # (B, H, W, C, x channels, x offset, out channels, out offset, bias)
    return {"v4 C=64": (2, 9, 7, 64, 64, 0, 64, 0, True),
            "v4 ldx!=ldo": (1, 5, 6, 8, 24, 4, 16, 8, True),
            "v4 no bias": (1, 6, 5, 16, 16, 0, 16, 0, False),
            "v4 past the grid cap": (1, 520, 512, 64, 64, 0, 64, 0, True),
            "scalar C=6": (2, 9, 7, 6, 6, 0, 6, 0, True),
            "scalar slice at 2": (1, 7, 9, 8, 16, 2, 12, 2, True),
            "scalar no bias": (1, 4, 4, 6, 7, 1, 6, 0, False),
            "H=1": (1, 1, 9, 8, 8, 0, 8, 0, True), "W=1": (1, 9, 1, 6, 6, 0, 6, 0, True),
            "H=2": (1, 2, 5, 8, 8, 0, 8, 0, True), "W=2": (2, 5, 2, 6, 6, 0, 6, 0, True), "1x1": (1, 1, 1, 8, 8, 0, 8, 0, True)}[name]


@pytest.mark.parametrize("name", ["v4 C=64", "v4 ldx!=ldo", "v4 no bias", "v4 past the grid cap", "scalar C=6",
                                  "scalar slice at 2", "scalar no bias", "H=1", "W=1", "H=2", "W=2", "1x1"])
def test_dwconv3x3(ops, name):
    """srhip_dwconv3x3: `C % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && (x | out | bias) % 16 == 0` takes k_dwconv3x3_v4,
    anything else k_dwconv3x3 (scalar): C = 6, and a C = 8 channel slice starting at channel 2 of a wider tensor (an 8-byte
    aligned pointer).  ldx != ldo, H or W of 1 and 2, no bias; 520 x 512 x 64: past ew_blocks' 16384 blocks.  The channels
    of `out` outside the slice hold NaN before and after."""
    B, H, W, C, Cx, ox, Co, oo, has_b = _dw_case(name)
    g = gen(H * W + C)
    xfull = torch.randn(B, H, W, Cx, generator=g)
    w, bias = torch.randn(C, 1, 3, 3, generator=g), (torch.randn(C, generator=g) if has_b else None)
    xk = xfull.cuda()
    ofull = torch.full((B, H, W, Co), NAN, device="cuda")
    xs, os_ = xk[..., ox:ox + C], ofull[..., oo:oo + C]
    v4 = C % 4 == 0 and Cx % 4 == 0 and Co % 4 == 0 and (xs.data_ptr() | os_.data_ptr()) % 16 == 0
    assert v4 == name.startswith(("v4", "H=1", "H=2", "1x1"))
    ops.dwconv3x3(xs, w.cuda(), None if bias is None else bias.cuda(), os_)
    x = xfull[..., ox:ox + C]
    r64 = R.dwconv3x3(x.double(), w.double(), None if bias is None else bias.double())
    with Gates(f"dwconv3x3 {name}") as G:
        G(os_, r64, R.dwconv3x3(x, w, bias), CONTRACTION, "out")
        rest = torch.cat([ofull[..., :oo], ofull[..., oo + C:]], dim=-1)
        G.true(bool(torch.isnan(rest).all()), "channels outside the slice written")


# ------------------------------------------------------------------ group_attention
@pytest.mark.parametrize("n,dh,heads,groups,has_bias", [(1, 5, 1, 7, True), (16, 8, 4, 5000, True), (49, 32, 4, 9, False),
                                                        (64, 8, 1, 9, True), (64, 32, 4, 5, True), (49, 5, 4, 11, False),
                                                        (16, 32, 1, 3, True), (1, 8, 4, 3, False)])
def test_group_attention(ops, n, dh, heads, groups, has_bias):
    """srhip_group_attention against softmax(scale q k^T + bias) v per (n consecutive rows, head): n = 1, 16, 49, 64 (the 4 x 4
    tiles walk all 64 rows; rows n .. 63 are zero), dh = 5, 8, 32, heads 1 and 4, with and without bias, 5000 groups."""
    C = heads * dh
    g = gen(n + dh + heads)
    qkv = torch.randn(groups * n, 3 * C, generator=g)
    bias = torch.randn(heads, n, n, generator=g) if has_bias else None
    scale = dh ** -0.5
    out = torch.full((groups * n, C), NAN, device="cuda")
    ops.group_attention(qkv.cuda(), None if bias is None else bias.cuda(), out, n, heads, scale)
    with Gates(f"group_attention n={n} dh={dh} heads={heads}") as G:
        G(out, R.group_attention(qkv.double(), None if bias is None else bias.double(), n, heads, scale),
          R.group_attention(qkv, bias, n, heads, scale), CONTRACTION, "out")


# ------------------------------------------------------------------ channel_attention
@pytest.mark.parametrize("H,W,ps,grid,d,arm", [(16, 24, 8, False, 8, "staged"), (24, 32, 8, True, 16, "staged"),
                                               (72, 72, 8, True, 8, "multi-pass"), (128, 128, 8, True, 5, "multi-pass"),
                                               (24, 36, 12, False, 16, "multi-pass"), (16, 16, 8, False, 5, "staged")])
def test_channel_attention(ops, H, W, ps, grid, d, arm):
    """srhip_channel_attention, window and grid form, d = 5, 8, 16.  `L <= CA_L` (64) keeps the group's q / k / v staged in
    LDS (an 8 x 8 window: L = 64; grid form on 24 x 32: L = 12); `L > CA_L` stages them 64 at a time for the Gram matrix and
    reads the values again from global memory (grid form on 72 x 72: L = 81 = 64 + 17; on 128 x 128: L = 256; window form
    with ps = 12: L = 144).  One q channel is all zero (the 1e-12 clamp of F.normalize)."""
    B, heads = 2, 4
    C = heads * d
    L = (H // ps) * (W // ps) if grid else ps * ps
    assert (arm == "staged") == (L <= 64)
    g = gen(H + W + d)
    qkv = torch.randn(B, H, W, 3 * C, generator=g)
    qkv[..., d + 1] = 0.0                                     # q channel 1 of head 1
    temp = torch.rand(heads, generator=g) * 2 + 0.5
    out = torch.full((B, H, W, C), NAN, device="cuda")
    ops.channel_attention(qkv.cuda(), temp.cuda(), out, heads, ps, grid)
    with Gates(f"channel_attention[{arm}] {H}x{W} ps={ps} grid={grid} d={d}") as G:
        G(out, R.channel_attention(qkv.double(), temp.double(), heads, ps, grid), R.channel_attention(qkv, temp, heads, ps, grid),
          CONTRACTION, "out")


# ------------------------------------------------------------------ gelu_gate, mul_sigmoid, bilinear_resize
@pytest.mark.parametrize("T,C", [(1003, 60), (16400, 257)])
def test_gelu_gate_and_mul_sigmoid(ops, T, C):
    """srhip_gelu_gate (gelu(x[:, :C]) * x[:, C:]) and srhip_mul_sigmoid (out may alias x); 16400 x 257 elements: past
    ew_blocks' 16384 blocks of 256"""
    g = gen(T + C)
    x = torch.randn(T, 2 * C, generator=g) * 3
    out = torch.full((T, C), NAN, device="cuda")
    ops.gelu_gate(x.cuda(), out)
    a, b = x[:, :C].contiguous(), x[:, C:].contiguous() * 3
    o2 = ops.mul_sigmoid(a.cuda(), b.cuda(), torch.full((T, C), NAN, device="cuda"))
    ak = a.cuda()
    ops.mul_sigmoid(ak, b.cuda(), ak)
    with Gates(f"gelu_gate / mul_sigmoid {T}x{C}") as G:
        G(out, R.gelu_gate(x.double()), R.gelu_gate(x), ELEMENTWISE, "gelu_gate")
        G(o2, R.mul_sigmoid(a.double(), b.double()), R.mul_sigmoid(a, b), ELEMENTWISE, "mul_sigmoid")
        G.equal(ak, o2, "mul_sigmoid in place")


@pytest.mark.parametrize("H,W,Ho,Wo", [(7, 15, 15, 7), (64, 1, 16, 5), (15, 64, 7, 16), (1, 7, 5, 15)])
def test_bilinear_resize(ops, H, W, Ho, Wo):
    """srhip_bilinear_resize against F.interpolate(mode='bilinear', align_corners=False): 7 -> 15, 15 -> 7, 64 -> 16 and 1 -> 5
    in each dimension"""
    g = gen(H + W)
    x = torch.randn(2, H, W, 6, generator=g)
    out = ops.bilinear_resize(x.cuda(), Ho, Wo)
    with Gates(f"bilinear_resize {H}x{W} -> {Ho}x{Wo}") as G:
        G(out, R.bilinear_resize(x.double(), Ho, Wo), R.bilinear_resize(x, Ho, Wo), ELEMENTWISE, "out")


# ------------------------------------------------------------------ prelu_bwd
@pytest.mark.parametrize("n", [4, 4096 * 256 * 4 + 4012])
def test_prelu_bwd(ops, n):
    """srhip_prelu_bwd: dx and the fp64-summed dalpha against float64 autograd of F.prelu, accumulate 0 and 1 (dalpha holds
    0.75 before); 4 elements and past the 4096 blocks x 256 threads x 4 elements of one grid pass; dx aliasing g; twice the
    same bits (partials summed in block order)."""
    g = gen(n % 1000)
    x, gr = torch.randn(n, generator=g), torch.randn(n, generator=g)
    alpha = torch.tensor([0.25])
    xk, gk, ak = x.cuda(), gr.cuda(), alpha.cuda()
    ws = torch.zeros(4096, dtype=torch.float64, device="cuda")

    def run(accumulate, alias=False):
        g_in = gk.clone()
        dx = g_in if alias else torch.full((n,), NAN, device="cuda")
        da = torch.tensor([0.75 if accumulate else NAN], device="cuda")
        ops.call("srhip_prelu_bwd", g_in.data_ptr(), xk.data_ptr(), ak.data_ptr(), dx.data_ptr(), da.data_ptr(), ws.data_ptr(), n,
                 accumulate, ops._st())
        torch.cuda.synchronize()
        return dx, da
    dx, da = run(0)
    dx2, da2 = run(0)
    _, da_acc = run(1)
    dxa, _ = run(0, alias=True)
    dx64, da64 = R.vjp(R.prelu, (x.double(), alpha.double()), gr.double())
    dx32, da32 = R.vjp(R.prelu, (x, alpha), gr)
    with Gates(f"prelu_bwd n={n}") as G:
        G.true(torch.equal(dx, dx2) and torch.equal(da, da2), "two calls differ")
        G(dx, dx64, dx32, ELEMENTWISE, "dx")
        G(da, da64, da32, ELEMENTWISE, "dalpha")
        G(da_acc, da64 + 0.75, da32 + 0.75, ELEMENTWISE, "dalpha, accumulate")
        G.equal(dxa, dx, "dx aliasing g")


# ------------------------------------------------------------------ axpby2d
def test_axpby2d(ops):
    """srhip_axpby2d on channel slices of wider row-major tensors.  b = 0: y holds NaN before the call and is not read --
    the slice becomes a x exactly, the other channels stay NaN.  b != 0 against a x + b y.  70000 rows x 64 columns: past the
    4096 blocks of one grid pass."""
    g = gen(8)
    with Gates("axpby2d") as G:
        for rows, cols, ldx, ox, ldy, oy in ((1003, 8, 12, 4, 20, 8), (5, 4, 4, 0, 4, 0), (70000, 64, 64, 0, 72, 4)):
            xf = torch.randn(rows, ldx, generator=g)
            yf = torch.randn(rows, ldy, generator=g)
            xk = xf.cuda()
            for a in (1.0, -1.75):
                yk = torch.full((rows, ldy), NAN, device="cuda")
                ops.call("srhip_axpby2d", yk.data_ptr() + 4 * oy, ldy, xk.data_ptr() + 4 * ox, ldx, rows, cols, a, 0.0, ops._st())
                G.equal(yk[:, oy:oy + cols], a * xf[:, ox:ox + cols], f"b = 0, a = {a}, {rows}x{cols}")
                rest = torch.cat([yk[:, :oy], yk[:, oy + cols:]], dim=1)
                G.true(bool(torch.isnan(rest).all()), "columns outside the slice written")
            yk = yf.cuda()
            ops.call("srhip_axpby2d", yk.data_ptr() + 4 * oy, ldy, xk.data_ptr() + 4 * ox, ldx, rows, cols, 0.6, -1.3, ops._st())
            xs, ys = xf[:, ox:ox + cols], yf[:, oy:oy + cols]
            G(yk[:, oy:oy + cols], R.axpby2d(ys.double(), xs.double(), 0.6, -1.3), R.axpby2d(ys, xs, 0.6, -1.3), ELEMENTWISE,
              f"b != 0, {rows}x{cols}")
            G.equal(torch.cat([yk[:, :oy], yk[:, oy + cols:]], dim=1), torch.cat([yf[:, :oy], yf[:, oy + cols:]], dim=1),
                    "columns outside the slice changed")
        with pytest.raises(ops.SrhipError):
            ops.call("srhip_axpby2d", yk.data_ptr(), 6, xk.data_ptr(), 4, 4, 4, 1.0, 0.0, ops._st())


# ------------------------------------------------------------------ pad_reflect1, crop1
def _pad_crop(ops, name, src, shape_out, B, H, W, C, adjoint):
    out = torch.full(shape_out, NAN, device="cuda")
    ops.call(name, src.data_ptr(), out.data_ptr(), B, H, W, C, adjoint, ops._st())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("W", [2, 3, 5, 17])
@pytest.mark.parametrize("H", [2, 3, 5, 17])
def test_pad_reflect1_and_crop1(ops, H, W):
    """srhip_pad_reflect1 / srhip_crop1, forward and adjoint = 1, against F.pad(mode='reflect'), the crop and their autograd.
    H, W = 2: a row is both `y == 1` and `y == H - 2`'s neighbour; 3: row 1 receives both mirrors; 5, 17: interior rows.  The
    copies are bit-equal; the padding's adjoint sums up to nine terms and is gated."""
    B, C = 2, 8
    g = gen(H * 20 + W)
    x = torch.randn(B, H, W, C, generator=g)
    gp = torch.randn(B, H + 2, W + 2, C, generator=g)
    with Gates(f"pad_reflect1 / crop1 {H}x{W}") as G:
        G.equal(_pad_crop(ops, "srhip_pad_reflect1", x.cuda(), (B, H + 2, W + 2, C), B, H, W, C, 0), R.pad_reflect1(x), "pad")
        adj = _pad_crop(ops, "srhip_pad_reflect1", gp.cuda(), (B, H, W, C), B, H, W, C, 1)
        G(adj, R.vjp(R.pad_reflect1, (x.double(),), gp.double())[0], R.vjp(R.pad_reflect1, (x,), gp)[0], ELEMENTWISE, "pad adjoint")
        G.equal(_pad_crop(ops, "srhip_crop1", gp.cuda(), (B, H, W, C), B, H, W, C, 0), R.crop1(gp), "crop")
        G.equal(_pad_crop(ops, "srhip_crop1", x.cuda(), (B, H + 2, W + 2, C), B, H, W, C, 1), R.vjp(R.crop1, (gp,), x)[0],
                "crop adjoint")


def test_pad_reflect1_and_crop1_past_grid_cap(ops):
    """300 x 300 x 64: 1.44 M 16-byte items and more, past the 4096 x 256 of one grid pass, forward and adjoint of both"""
    B, H, W, C = 1, 300, 300, 64
    g = gen(2)
    x = torch.randn(B, H, W, C, generator=g)
    gp = torch.randn(B, H + 2, W + 2, C, generator=g)
    with Gates("pad_reflect1 / crop1 300x300x64") as G:
        G.equal(_pad_crop(ops, "srhip_pad_reflect1", x.cuda(), (B, H + 2, W + 2, C), B, H, W, C, 0), R.pad_reflect1(x), "pad")
        adj = _pad_crop(ops, "srhip_pad_reflect1", gp.cuda(), (B, H, W, C), B, H, W, C, 1)
        G(adj, R.vjp(R.pad_reflect1, (x.double(),), gp.double())[0], R.vjp(R.pad_reflect1, (x,), gp)[0], ELEMENTWISE, "pad adjoint")
        G.equal(_pad_crop(ops, "srhip_crop1", gp.cuda(), (B, H, W, C), B, H, W, C, 0), R.crop1(gp), "crop")
        G.equal(_pad_crop(ops, "srhip_crop1", x.cuda(), (B, H + 2, W + 2, C), B, H, W, C, 1), R.vjp(R.crop1, (gp,), x)[0],
                "crop adjoint")
