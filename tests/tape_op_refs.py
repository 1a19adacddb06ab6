"""Plain statements of the tape-net ops (nlsa.hip, tape_ops.hip, act_ops.hip, omni_ops.hip, dfca.hip), torch primitives only.

Every function takes tensors of any float dtype and computes in that dtype, so the same function is the float64
reference and the float32 yardstick of tests/test_gpu_tape_op_kernels.py.  Backward references are autograd of the
forward statement (``vjp``), never a hand-derived formula.  The statements themselves are pinned by
tests/test_cpu_tape_op_refs.py.  Spatial ops take channels-last [B, H, W, C] tensors, as the kernels do; the line numbers
cited are those of the reference files the kernels' own comments cite."""
import torch
import torch.nn.functional as F

import sr_oracle as O

TOK_BITS = 20


def vjp(fn, inputs, grads):
    """Gradients of fn(*inputs) (a tensor or a tuple of tensors) with respect to every input, for the output gradients
    `grads`, by autograd in the inputs' own dtype."""
    xs = [t.detach().clone().requires_grad_(True) for t in inputs]
    out = fn(*xs)
    outs = out if isinstance(out, (tuple, list)) else (out,)
    gs = grads if isinstance(grads, (tuple, list)) else (grads,)
    return torch.autograd.grad(outs, xs, gs, allow_unused=True)


# ------------------------------------------------------------------ NLSN (network_nlsn.py:131-268)
def lsh_order(rotated, N, L, n_hashes, hash_buckets):
    """rotated [N * L, n_hashes * hash_buckets // 2] (round-major columns) -> int64 keys [N, n_hashes, L]: the code of a
    token is argmax(cat([r, -r])) with torch's first-maximum rule (:145-170), the tokens of a (sample, round) are put in
    order of their code by a STABLE sort (:199-207), and a key is ((n * n_hashes + h) * hash_buckets + code) << 20 | token."""
    hbh = hash_buckets // 2
    r = rotated[:, :n_hashes * hbh].reshape(N, L, n_hashes, hbh).permute(0, 2, 1, 3)
    codes = torch.argmax(torch.cat([r, -r], dim=-1), dim=-1)                   # [N, nh, L]
    codes_sorted, tok = torch.sort(codes, dim=-1, stable=True)
    grp = (torch.arange(N).view(N, 1, 1) * n_hashes + torch.arange(n_hashes).view(1, -1, 1)) * hash_buckets
    return ((grp + codes_sorted) << TOK_BITS) | tok


def nlsa_core(x_embed, y_embed, tok, x, chunk_size, res_scale):
    """Lines 872-909 of oracle/sr_oracle.py::_nlsa (network_nlsn.py:209-266) with the convs removed and the order given.
    x_embed [N, L, Ce], y_embed [N, L, Cy], x [N, L, Cy], tok int64 [N, nh, L] = the token at every sorted position of
    every round.  Returns (out [N, L, Cy], ret [N, nh, L, Cy], score [N, nh, L]), all in token positions."""
    N, L, C = x_embed.shape
    Cy = y_embed.shape[-1]
    nh = tok.shape[1]
    idx = tok.reshape(N, nh * L)

    def bsel(values, i):
        return values.gather(1, i[:, :, None].expand(-1, -1, values.shape[-1]))
    xs, ys = bsel(x_embed, idx), bsel(y_embed, idx)
    padding = chunk_size - L % chunk_size if L % chunk_size != 0 else 0
    xb = torch.reshape(xs, (N, nh, -1, C))
    yb = torch.reshape(ys, (N, nh, -1, Cy))
    if padding:                                     # the last `padding` sorted positions, repeated
        xb = torch.cat([xb, xb[:, :, -padding:, :]], dim=2)
        yb = torch.cat([yb, yb[:, :, -padding:, :]], dim=2)
    xb = torch.reshape(xb, (N, nh, -1, chunk_size, C))
    yb = torch.reshape(yb, (N, nh, -1, chunk_size, Cy))
    xm = F.normalize(xb, p=2, dim=-1, eps=5e-5)

    def adj(t):                                     # keys: own | previous | next chunk
        back = torch.cat([t[:, :, -1:, ...], t[:, :, :-1, ...]], dim=2)
        fwd = torch.cat([t[:, :, 1:, ...], t[:, :, :1, ...]], dim=2)
        return torch.cat([t, back, fwd], dim=3)
    xm, yb = adj(xm), adj(yb)
    raw = torch.einsum('bhkie,bhkje->bhkij', xb, xm)
    lse = torch.logsumexp(raw, dim=-1, keepdim=True)
    prob = torch.exp(raw - lse)
    ret = torch.einsum('bukij,bukje->bukie', prob, yb).reshape(N, nh, -1, Cy)[:, :, :L]
    lse = lse.reshape(N, nh, -1)[:, :, :L]
    undo = torch.argsort(tok, dim=-1)               # token -> its sorted position
    ret = ret.gather(2, undo[..., None].expand(-1, -1, -1, Cy))
    score = lse.gather(2, undo)
    out = torch.sum(ret * F.softmax(score, dim=1)[..., None], dim=1) * res_scale + x
    return out, ret, score


# ------------------------------------------------------------------ ENLCN (network_enlcn.py:207-366)
def l2norm_rows(x, k=1.0, eps=5e-5):
    """k * F.normalize(x, p=2, dim=channel, eps) on token rows (:341-342)"""
    return k * F.normalize(x, p=2, dim=-1, eps=eps)


def performer_features(dash, data, eps=1e-4):
    """softmax_kernel (:207-240): F^-1/2 (exp(dash - |data|^2 / 2) + eps), F = dash.shape[1]"""
    diag = (torch.sum(data ** 2, dim=-1) / 2.0).unsqueeze(-1)
    return dash.shape[-1] ** -0.5 * (torch.exp(dash - diag) + eps)


def performer_chain(x, proj, k, eps_norm=5e-5, eps_feat=1e-4):
    """un-normalised rows -> normalise -> project -> features: the composite whose backward the engine splits into
    performer_features_bwd, a GEMM and l2norm_rows_bwd (:341-342, :207-240)"""
    y = l2norm_rows(x, k, eps_norm)
    return performer_features(y @ proj.t(), y, eps_feat)


def enlca_finish(num, x, res_scale):
    """linear_attention's division and ENLCA's residual (:243-257, :366): x + res_scale num[:, :Cy] / num[:, Cy]"""
    Cy = x.shape[1]
    return x + res_scale * num[:, :Cy] / num[:, Cy:Cy + 1]


# ------------------------------------------------------------------ ACT / GRL row ops (network_act.py:115-133,176,215)
def softmax_rows(x, scale=1.0):
    return torch.softmax(x * scale, dim=-1)


def softmax_rows_lse(x, scale=1.0):
    return torch.softmax(x * scale, dim=-1), torch.logsumexp(x * scale, dim=-1)


def rowdot(a, b):
    return (a * b).sum(dim=-1)


def layernorm_rows(x, gamma, beta, eps=1e-5, res=None):
    """nn.LayerNorm over the rows (network_act.py:115-133); res: the post-norm residual of GRL (network_grl.py:1061-1076)"""
    y = F.layer_norm(x, (x.shape[-1],), gamma, beta, eps)
    return y if res is None else res + y


def unary(x, kind):
    """nn.GELU() (exact erf) / sigmoid"""
    return F.gelu(x) if kind == "gelu" else torch.sigmoid(x)


# ------------------------------------------------------------------ DFCAN (network_dfcan.py:27-36, 39-70)
def fft2_mag_pow_shift(x, gamma=0.8, eps=1e-8):
    """fftshift2d((|fftn(x, dim=(H, W))| + eps) ** gamma) on channels-last x (:27-36, :60-64)"""
    s = torch.fft.fftn(x.permute(0, 3, 1, 2), dim=(2, 3))
    s = torch.pow(torch.abs(s) + eps, gamma)
    return O._dfcan_fftshift2d(s).permute(0, 2, 3, 1)


def channel_gate(feat, w1, b1, w2, b2, x0, x1, mid_act="relu"):
    """x0 + x1 * sigmoid(W2 act(W1 mean_pixels(feat) + b1) + b2) (:65-70); act ReLU (DFCAN, ACT) or SiLU (OmniSR's SE)"""
    mean = feat.mean(dim=(1, 2))
    mid = F.linear(mean, w1, b1)
    mid = F.silu(mid) if mid_act == "silu" else F.relu(mid)
    g = torch.sigmoid(F.linear(mid, w2, b2))[:, None, None, :]
    return x1 * g if x0 is None else x0 + x1 * g


# ------------------------------------------------------------------ OmniSR (network_omni_sr.py)
def dwconv3x3(x, w, bias):
    """nn.Conv2d(C, C, 3, padding=1, groups=C) on channels-last x (:178, :318, :348); w [C, 1, 3, 3]"""
    C = x.shape[-1]
    return F.conv2d(x.permute(0, 3, 1, 2), w.reshape(C, 1, 3, 3), bias, padding=1, groups=C).permute(0, 2, 3, 1)


def group_attention(qkv, bias, n, heads, scale):
    """Attention.forward (:258-306): softmax(scale q k^T + bias) v per (n consecutive rows, head); qkv [G * n, 3C] = q | k | v
    with head-major channels, bias [heads, n, n] or None -> [G * n, C]"""
    T, C3 = qkv.shape
    C = C3 // 3
    q, k, v = (t.reshape(T // n, n, heads, C // heads).permute(0, 2, 1, 3) for t in qkv.split(C, dim=1))
    s = (q * scale) @ k.transpose(-1, -2)
    if bias is not None:
        s = s + bias
    return (s.softmax(dim=-1) @ v).permute(0, 2, 1, 3).reshape(T, C)


def channel_attention(qkv, temperature, heads, ps, grid):
    """Channel_Attention(_grid).forward (:353-428): per (sample, group, head) the d x d attention between L2-normalised
    channel vectors times temperature[head]; window form: group = ps x ps window, vector = its pixels; grid form: group =
    in-window position, vector = the windows.  qkv [B, H, W, 3C] -> [B, H, W, C]"""
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    d, hy, wx = C // heads, H // ps, W // ps

    def split(t):                                   # [B, H, W, C] -> [B, group, head, d, L]
        t = t.reshape(B, hy, ps, wx, ps, heads, d)
        if grid:
            return t.permute(0, 2, 4, 5, 6, 1, 3).reshape(B, ps * ps, heads, d, hy * wx)
        return t.permute(0, 1, 3, 5, 6, 2, 4).reshape(B, hy * wx, heads, d, ps * ps)
    q, k, v = (split(t) for t in qkv.split(C, dim=-1))
    q, k = F.normalize(q, dim=-1), F.normalize(k, dim=-1)
    attn = ((q @ k.transpose(-2, -1)) * temperature.reshape(1, 1, heads, 1, 1)).softmax(dim=-1)
    o = attn @ v
    if grid:
        o = o.reshape(B, ps, ps, heads, d, hy, wx).permute(0, 5, 1, 6, 2, 3, 4)
    else:
        o = o.reshape(B, hy, wx, heads, d, ps, ps).permute(0, 1, 5, 2, 6, 3, 4)
    return o.reshape(B, H, W, C)


def gelu_gate(x):
    """Gated_Conv_FeedForward (:325-326): gelu(x[:, :C]) * x[:, C:]"""
    a, b = x.chunk(2, dim=-1)
    return F.gelu(a) * b


def mul_sigmoid(x, g):
    """ESA (:113-114)"""
    return x * torch.sigmoid(g)


def bilinear_resize(x, Ho, Wo):
    """F.interpolate(mode='bilinear', align_corners=False) on channels-last x (ESA :110)"""
    return F.interpolate(x.permute(0, 3, 1, 2), size=(Ho, Wo), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)


# ------------------------------------------------------------------ DBPN / SRFBN / ProSR helpers
def prelu(x, alpha):
    """nn.PReLU(num_parameters=1) (network_dbpn.py:85, network_srfbn.py:44)"""
    return F.prelu(x, alpha)


def axpby2d(y, x, a, b):
    return a * x if b == 0 else a * x + b * y


def pad_reflect1(x):
    """nn.ReflectionPad2d(1) on channels-last x (network_prosr.py:44-86)"""
    return F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="reflect").permute(0, 2, 3, 1)


def crop1(x):
    return x[:, 1:-1, 1:-1, :]
