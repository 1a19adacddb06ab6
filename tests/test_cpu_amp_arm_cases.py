"""The condition that makes `torch.equal` the right gate in tests/test_gpu_amp_arms.py, proved without a GPU for every case of
tests/amp_arm_cases.py: the leading plane holds every operand value exactly (bf16, and fp16 at every block scale the rule can
choose, one binade of slack in either direction), the float64 result is an integer number of `unit`s, and no partial sum of any
evaluation order reaches 2^24 units.  Also: the case lists reach every single-product instantiation the product build can
launch (the routing rules of amp_arm_cases.py), the float32 convolution used as the reference of the 256 x 512 cases is exact
on such operands, and the emulation of tests/lead_plane_ref.py agrees with a scalar statement of the rounding rules."""
import math
import struct

import pytest
import torch

import amp_arm_cases as C
import lead_plane_ref as LP

A_MODE1 = [c for c in C.GEMM_F16 if c[2] in (180, 212, 360, 540)]      # see test_gpu_amp_arms.py: K where sqrt(K) is no power of two


def exact_at(x, s):
    """x * 2^s survives fp16 for s - 1, s, s + 1 (s: per-row float tensor broadcastable to x)"""
    for d in (-1.0, 0.0, 1.0):
        if not torch.equal(LP.round_f16_at(x, s + d), x.double()):
            return False
    return True


def check_result(ref, bound, unit):
    q = ref / unit
    assert torch.equal(q, q.round()), "the float64 result is not a whole number of units"
    assert bound / unit < C.LIMIT and q.abs().max().item() < C.LIMIT
    assert torch.equal(ref.float().double(), ref)


EPIS = [(0, {}), (1, {}), (4, {})] + [(2, dict(alpha=C.ALPHA, rows_per_scale=r)) for r in C.RPS]


def epilogues(M):
    for epi, kw in EPIS:
        if epi == 2:
            kw = dict(kw, rowscale=C.rowscale_for(M, kw["rows_per_scale"]))
        yield epi, kw


@pytest.mark.parametrize("M,N,K", C.GEMM_BF16 + [c[1:] for c in C.GEMM_EPI if c[0] == 0])
def test_bf16_gemm_cases_are_exact(M, N, K):
    assert K % 4 == 0
    for a_mode in (0, 1):
        op = C.gemm_operands(0, M, N, K, a_mode)
        A = op["A"] if a_mode == 0 else LP.layernorm_prologue(op["A"], op["stats"])
        assert torch.equal(LP.lead_bf16(A), A) and torch.equal(LP.lead_bf16(op["W"]), op["W"])
        for epi, kw in epilogues(M):
            check_result(*C.gemm_reference(op, epi, **kw), op["unit"])


@pytest.mark.parametrize("M,N,K", C.GEMM_F16 + [c[1:] for c in C.GEMM_EPI if c[0] == 1])
def test_f16_gemm_cases_are_exact(M, N, K):
    assert C.f16_linear_ok(N, K) and K % 4 == 0
    for a_mode in (0, 1) if (M, N, K) in A_MODE1 else (0,):
        op = C.gemm_operands(1, M, N, K, a_mode)
        A = op["A"] if a_mode == 0 else LP.layernorm_prologue(op["A"], op["stats"])
        s = LP.nth2_pass_exponents(A, a_mode).repeat_interleave(LP.PASS_K, 1)[:, :K]
        assert exact_at(A, s)
        assert exact_at(op["W"], LP.f16_exponent(op["W"].abs().amax(1))[:, None])
        for epi, kw in epilogues(M):
            check_result(*C.gemm_reference(op, epi, **kw), op["unit"])
    if K > LP.PASS_K and M >= 4:      # the profiles are what they claim: a rising row drops its scale by 2^-4, zero rows stay at 0
        s = LP.nth2_pass_exponents(C.gemm_operands(1, M, N, K)["A"])
        assert s[1, 0] == 14 and s[1, 1] == 10 and s[2, 0] == 0 and (s[3] == 0).all()


def test_gemm_cases_reach_every_single_product_instantiation():
    arms = {C.gemm_arm(N, 0, True) for _, N, _ in C.GEMM_BF16} | {C.gemm_arm(N, 1, True) for _, N, _ in C.GEMM_F16}
    assert arms == C.GEMM_ARMS
    assert C.gemm_arm(180, 1, True, epi=5) == "k_nth2<false>" and C.gemm_arm(180, 0, True, epi=5) is None
    # stage counts of the bf16 kernels (32 k a stage): one, two, three, an odd count above three
    for arm in ("k_ntp<1,true>", "k_ntp<2,true>", "k_ntw<false,true>"):
        ks = {K for _, N, K in C.GEMM_BF16 if C.gemm_arm(N, 0, True) == arm}
        assert any(k % 8 == 4 for k in ks), arm                 # half an octet at the K tail
        assert any(-(-k // 32) % 2 == 1 for k in ks) and any(-(-k // 32) % 2 == 0 for k in ks), arm
    # k_nth2: one, two, three and six passes; a stage count that is one past a pass
    assert {-(-K // LP.PASS_K) for _, _, K in C.GEMM_F16} >= {1, 2, 3, 6}
    assert any(-(-K // 32) % 6 == 1 for _, _, K in C.GEMM_F16)


@pytest.mark.parametrize("name", [c[0] for c in C.CONV_SMALL + C.CONV_LARGE])
def test_conv_cases_are_exact(name):
    _, kind, B, H, W, Cin, Cout = C.CONV_CASES[name]
    op = C.conv_operands(name)
    for t in (op["x"], op["w"], op["b"], op["R"]):
        assert torch.equal(t, t.round()) and t.abs().max().item() <= C.VMAX
    assert torch.equal(LP.lead_bf16(op["x"]), op["x"]) and torch.equal(LP.lead_bf16(op["w"]), op["w"])
    # fp16: a block (halo tile, output channel) of largest magnitude m <= 15 is scaled to m 2^s in [8192, 16384], one binade of
    # slack: every member at every such s, i.e. every value at every s that keeps it within 32768
    for t in (op["x"], op["w"]):
        for s in range(9, 16):
            ok = t.abs() * 2.0 ** s <= 32768.0
            v = torch.where(ok, t, torch.zeros_like(t))
            assert torch.equal(LP.round_f16_at(v, torch.tensor(float(s))), v.double())
    assert C.conv_bound(name) < C.LIMIT
    if name in C.IN_BN:
        assert C.conv_formats(name) == (0, 1) and Cout % 64 == 0
        v = C.in_bn_apply(op["x"], C.conv_in_bn(name))
        assert torch.equal(v, v.round()) and 0 <= v.min().item() and v.max().item() <= C.IN_BN_VMAX
        for s in range(8, 16):
            u = torch.where(v * 2.0 ** s <= 32768.0, v, torch.zeros_like(v))
            assert torch.equal(LP.round_f16_at(u, torch.tensor(float(s))), u.double())
        assert C.conv_bound(name, C.IN_BN_VMAX) < C.LIMIT
    wq, s = LP.lead_f16_conv(op["w"] if kind != "ps2_bwd" else op["w"].transpose(0, 1))
    assert torch.equal(wq.float(), (op["w"] if kind != "ps2_bwd" else op["w"].transpose(0, 1)))
    if name in {c[0] for c in C.CONV_SMALL}:
        ref = C.conv_reference(name, op)
        assert torch.equal(ref, ref.round()) and ref.abs().max().item() < C.LIMIT
        # the float32 convolution the large cases are compared with is exact on such operands
        assert torch.equal(C.conv_reference(name, op, torch.float32).double(), ref)


def test_conv_cases_reach_every_single_product_instantiation():
    arms = {C.conv_arm_of(name, fmt) for name in C.CONV_CASES for fmt in C.conv_formats(name)}
    assert arms == C.CONV_ARMS
    # the PixelShuffle forms on both formats, and both tile heights of the 64-column kernels
    for name in ("ps2", "ps2_bwd", "bigps2"):
        assert C.conv_formats(name) == (0, 1)
    assert C.conv_arm_of("ps2", 0) == "k_ntb<1,2,true,true>" and C.conv_arm_of("bigps2", 0) == "k_ntcw2<4,true>"
    assert C.conv_arm_of("ps2_bwd", 0) == "k_ntcw2<2,true>" and C.conv_arm_of("big180", 0) == "k_ntb<2,3,true,true>"


# ---------------------------------------------------------------------------------------------- the emulation itself
def _bf16_scalar(v):
    """RNE to bf16 on the bit pattern"""
    u = struct.unpack("<I", struct.pack("<f", v))[0]
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return struct.unpack("<f", struct.pack("<I", u))[0]


def test_lead_plane_emulation_against_scalar_statements():
    g = torch.Generator().manual_seed(7)
    x = torch.randn(64, 40, generator=g) * torch.exp(torch.randn(64, 1, generator=g) * 4)
    got = LP.lead_bf16(x)
    for v, w in zip(x.flatten().tolist()[:500], got.flatten().tolist()[:500]):
        assert _bf16_scalar(v) == w
    assert LP.lead_bf16(torch.tensor([1.0 + 2.0 ** -8])).item() == 1.0            # a tie goes to the even neighbour
    assert LP.lead_bf16(torch.tensor([1.0 + 3 * 2.0 ** -8])).item() == 1.0 + 2.0 ** -6
    # fp16 rows: the scaled maximum lies in [8192, 16384], the rounded values are multiples of 2^-s x the fp16 spacing
    q, s = LP.lead_f16_rows(x)
    top = x.abs().amax(1).double() * torch.exp2(s.double())
    assert (top > 8192).all() and (top <= 16384).all()
    for r in range(0, 64, 7):
        sc = 2.0 ** s[r].item()
        for v, w in zip(x[r].tolist(), q[r].tolist()):
            h = struct.unpack("<e", struct.pack("<e", v * sc))[0]                   # struct rounds to nearest even
            assert h / sc == w
    assert LP.f16_exponent(torch.tensor([0.0, 1.0, 15.0, 16384.0, 1e-30])).tolist() == [0.0, 14.0, 10.0, 0.0, 100.0]
    # running scale over 192-k passes: non-increasing, an all-zero pass asks for nothing
    A = torch.zeros(3, 600)
    A[0, 5], A[0, 200], A[0, 400] = 1.5, 1.5 * 2 ** 5, 1.5 * 2 ** 2
    A[1, 390] = 3.0
    s = LP.nth2_pass_exponents(A)
    assert s[0].tolist() == [13.0, 8.0, 8.0, 8.0] and s[1].tolist() == [0.0, 0.0, 12.0, 12.0] and s[2].tolist() == [0.0] * 4
    assert LP.nth2_apriori_exponent(180).item() == math.floor(math.log2(16384 / math.sqrt(180))) == 10
    w = torch.randn(6, 5, 3, 3, generator=g) * torch.tensor([1e-3, 1.0, 50.0, 0.0, 7.0, 1e4])[:, None, None, None]
    wq, sw = LP.lead_f16_conv(w)
    assert torch.equal(sw, LP.f16_exponent(w.abs().amax((1, 2, 3)))) and wq[3].abs().max() == 0
    assert ((wq - w.double()).abs().amax((1, 2, 3)) <= w.abs().amax((1, 2, 3)).double() * 2.0 ** -11).all()
