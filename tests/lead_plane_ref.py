"""What the single-product (--amp, srhip_set_matmul_mode(1)) arms of the contraction kernels multiply: the LEADING plane of
each operand, stated in plain torch on the CPU.

    bf16x3 planes (split3_pair, gemm_ntb.hip)        leading plane = the value rounded to bf16, round to nearest even
    fp16x2 planes, prep kind 3 (prep.hip)            v * 2^s rounded to fp16 (RNE), s = min(floor(log2(16384 / rowmax)), 100)
                                                     per ROW of the weight, 2^-s kept as a float behind the planes
    fp16x2 planes, prep kind 4 (prep.hip)            the same with one s per OUTPUT CHANNEL of the conv weight (its nine tap rows)
    A rows of k_nth2 (gemm_ntw.hip)                  the same rule per row as a RUNNING scale over passes of 192 k: a pass is
                                                     rounded at the smallest scale any pass so far asked for; behind the
                                                     LayerNorm prologue the scale is a priori, floor(log2(16384 / sqrt(K)))

The scale arithmetic is done in float32 as on the device (16384 / max, log2, floor).  Where a row maximum sits at 1.5 * 2^e the
quotient is a third of a binade away from a power of two and the device's log2f cannot land in another binade than this
file's; tests/test_gpu_amp_arms.py pins the emulation bit for bit against the planes the device writes."""
import torch

PASS_K = 192            # k per pass of k_nth2
F16_TOP = 16384.0       # a scaled row's largest magnitude lies in [8192, 16384]
S_MAX = 100.0


def lead_bf16(x):
    """the leading bf16 plane of x (round to nearest even), as float32"""
    return x.float().to(torch.bfloat16).float()


def f16_exponent(mx):
    """s of the block scale 2^s for a row whose largest magnitude is mx (float32 tensor); 0 for an all-zero row, which the
    preparation kernels scale by 1"""
    mx = mx.float()
    s = torch.clamp(torch.floor(torch.log2(torch.tensor(F16_TOP) / mx.clamp_min(1e-45))), max=S_MAX)
    return torch.where(mx > 0, s, torch.zeros_like(s))


def round_f16_at(x, s):
    """x * 2^s rounded to fp16 (RNE) and unscaled again; s broadcasts against x.  Returned as float64: 2^-s times an fp16
    value is exact there, and in float32 too wherever the device holds it"""
    sc = torch.exp2(s.double())
    return (x.double() * sc).float().to(torch.float16).double() / sc


def lead_f16_rows(x):
    """leading fp16 plane of a Linear weight [rows, K] (prep kind 3): one scale per row -> (rounded values, s per row)"""
    s = f16_exponent(x.abs().amax(-1))
    return round_f16_at(x, s[..., None]), s


def lead_f16_conv(w):
    """leading fp16 plane of a conv weight [Co, Ci, 3, 3] (prep kind 4): one scale per output channel.  For the data-gradient
    twin pass w.transpose(0, 1): its output channels are the conv's input channels."""
    s = f16_exponent(w.abs().amax((1, 2, 3)))
    return round_f16_at(w, s[:, None, None, None]), s


def nth2_apriori_exponent(K):
    """the scale k_nth2 uses behind the LayerNorm prologue: |xhat| <= sqrt(K)"""
    return torch.floor(torch.log2(torch.tensor(F16_TOP) * torch.rsqrt(torch.tensor(float(K)))))


def nth2_pass_exponents(A, a_mode=0):
    """s of every (row, 192-k pass) of k_nth2's A operand [M, K] -> [M, npass] float32.  a_mode 0 / 2 (A is what the prologue
    returns): the running minimum of what the passes so far need, an all-zero pass asking for nothing; a row that is zero so
    far is staged at scale 1 (s = 0).  a_mode 1: the a-priori scale everywhere."""
    M, K = A.shape
    npass = -(-K // PASS_K)
    if a_mode == 1:
        return nth2_apriori_exponent(K).expand(M, npass).clone()
    out = torch.empty(M, npass)
    run = torch.full((M,), float("inf"))
    for p in range(npass):
        mx = A[:, p * PASS_K:(p + 1) * PASS_K].abs().amax(1).float()
        need = torch.where(mx > 0, f16_exponent(mx), torch.full_like(mx, float("inf")))
        run = torch.minimum(run, need)
        out[:, p] = torch.where(torch.isinf(run), torch.zeros_like(run), run)
    return out


def lead_f16_passes(A, a_mode=0):
    """leading fp16 plane of k_nth2's A operand (A: the prologue's output, float32) -> float64 [M, K]"""
    s = nth2_pass_exponents(A, a_mode)
    return round_f16_at(A, s.repeat_interleave(PASS_K, 1)[:, :A.shape[1]])


def layernorm_prologue(A, stats):
    """(A - mean) * rstd in float32, as the GEMM prologues compute it (a_mode 1); stats [M, 2] = {mean, rstd}"""
    return (A.float() - stats[:, :1].float()) * stats[:, 1:].float()


def decode_planes(planes, rows, K, kp, fmt):
    """plane 0 of a Bx3's storage as float64 [rows, K], and for fmt 1 the floats 2^-s behind the two planes (all of them:
    `rows` for prep kind 3, rows / 9 for kind 4).  planes: the int16 tensor [3, rows, kp] copied to the CPU; storage is 16-k
    sub-chunk major [plane][kp / 16][rows][16]."""
    flat = planes.reshape(-1)
    p0 = flat[:rows * kp]
    if fmt == 0:
        v = (p0.to(torch.int32) << 16).view(torch.float32).double()
    else:
        v = p0.view(torch.float16).double()
    v = v.reshape(kp // 16, rows, 16).permute(1, 0, 2).reshape(rows, kp)
    assert v[:, K:].abs().max().item() == 0 if kp > K else True
    inv = None
    if fmt == 1:
        inv = flat[2 * rows * kp:2 * rows * kp + 2 * rows].contiguous().view(torch.float32)
    return v[:, :K], inv
