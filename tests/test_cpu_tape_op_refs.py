"""Pins the plain references of tests/tape_op_refs.py, so that a wrong reference cannot pass a wrong kernel: nlsa_core and
lsh_order against the oracle's own _nlsa (itself pinned against the reference's goldens) and against a per-token loop,
channel_attention against the oracle's einops statement, the adjoint pairs by <A x, g> == <x, A^T g>, and every statement
whose autograd serves as a backward reference by torch.autograd.gradcheck at a tiny size.  float64 throughout, no GPU."""
import math

import pytest
import torch
import torch.nn.functional as F

import sr_oracle as O
import tape_op_refs as R

D = torch.float64


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _perm_tok(N, nh, L, gen):
    return torch.stack([torch.stack([torch.randperm(L, generator=gen) for _ in range(nh)]) for _ in range(N)])


# (H, W, chunk_size): nchunks 4 with padding 2; nchunks 1; nchunks 2; nchunks 2 with padding 12; nchunks 3
NLSA_CASES = [(6, 5, 8), (4, 4, 16), (8, 4, 16), (5, 4, 16), (6, 6, 12)]


@pytest.mark.parametrize("H,W,cs", NLSA_CASES)
@pytest.mark.parametrize("nh", [1, 3])
def test_nlsa_core_matches_oracle(H, W, cs, nh):
    """nlsa_core against O._nlsa: conv_match = a delta kernel that selects the first Ce channels, conv_assembly = identity,
    the same order fed to both as `indices`; agreement to float64 rounding, with and without padding, nchunks 1 and 2."""
    N, C, Ce, L = 2, 6, 4, H * W
    gen = _gen(H * 100 + W * 10 + nh)
    x = torch.randn(N, C, H, W, generator=gen, dtype=D)
    wm = torch.zeros(Ce, C, 3, 3, dtype=D)
    for e in range(Ce):
        wm[e, e, 1, 1] = 1.0
    sd = {"a.conv_match.0.weight": wm, "a.conv_match.0.bias": torch.zeros(Ce, dtype=D),
          "a.conv_assembly.0.weight": torch.eye(C, dtype=D).reshape(C, C, 1, 1), "a.conv_assembly.0.bias": torch.zeros(C, dtype=D)}
    tok = _perm_tok(N, nh, L, gen)
    indices = (tok + torch.arange(nh).view(1, nh, 1) * L).reshape(N, nh * L)
    ref = O._nlsa(sd, "a", x, nh, cs, 0.3, rotations=torch.zeros(1, Ce, nh, 1, dtype=D), indices=indices)
    rows = x.reshape(N, C, L).permute(0, 2, 1)
    out, ret, score = R.nlsa_core(rows[..., :Ce], rows, tok, rows, cs, 0.3)
    got = out.permute(0, 2, 1).reshape(N, C, H, W)
    assert (got - ref).abs().max().item() <= 1e-13 * ref.abs().max().item()
    # ret and score one by one, from the definition: the query at sorted position p of chunk k against the keys of chunks
    # k, k - 1, k + 1 (cyclic) of the padded order
    padding = cs - L % cs if L % cs else 0
    for n in range(N):
        for h in range(nh):
            order = tok[n, h].tolist()
            order = order + order[L - padding:] if padding else order
            nch = len(order) // cs
            for p in range(L):
                k = p // cs
                keys = [order[c * cs + j] for c in (k, (k - 1) % nch, (k + 1) % nch) for j in range(cs)]
                xk = rows[n, keys, :Ce]
                xk = xk / xk.norm(dim=-1, keepdim=True).clamp_min(5e-5)
                s = xk @ rows[n, order[p], :Ce]
                assert abs(torch.logsumexp(s, 0).item() - score[n, h, order[p]].item()) <= 1e-12
                r = torch.softmax(s, 0) @ rows[n, keys]
                assert (r - ret[n, h, order[p]]).abs().max().item() <= 1e-12


def test_nlsa_core_clamped_keys():
    """embeddings scaled by 1e-6: every key norm is below eps = 5e-5, so the keys are divided by eps, not by their norm"""
    gen = _gen(3)
    N, L, Ce, Cy, cs = 1, 24, 4, 5, 8
    xe = torch.randn(N, L, Ce, generator=gen, dtype=D) * 1e-6
    ye, x = torch.randn(N, L, Cy, generator=gen, dtype=D), torch.randn(N, L, Cy, generator=gen, dtype=D)
    tok = _perm_tok(N, 2, L, gen)
    _, _, score = R.nlsa_core(xe, ye, tok, x, cs, 1.0)
    s = (xe[0] @ xe[0].t()) / 5e-5
    assert (score - math.log(3 * cs)).abs().max().item() <= 2 * s.abs().max().item() + 1e-12


def test_lsh_order_matches_oracle_codes_and_indices():
    """lsh_order against the codes / indices O._nlsa taps (random rotations: no ties in the argmax).  The oracle's sort is
    torch's unstable one, so the indices are compared as (code, token) pairs: the same codes at the same sorted positions,
    the same tokens per code, and lsh_order's own tokens ascending within a code (the stable rule)."""
    N, C, Ce, H, W, nh, cs = 2, 6, 4, 12, 10, 3, 8
    L = H * W
    gen = _gen(11)
    x = torch.randn(N, C, H, W, generator=gen, dtype=D)
    wm = torch.zeros(Ce, C, 3, 3, dtype=D)
    for e in range(Ce):
        wm[e, e, 1, 1] = 1.0
    sd = {"a.conv_match.0.weight": wm, "a.conv_match.0.bias": torch.zeros(Ce, dtype=D),
          "a.conv_assembly.0.weight": torch.eye(C, dtype=D).reshape(C, C, 1, 1), "a.conv_assembly.0.bias": torch.zeros(C, dtype=D)}
    hb = min(L // cs + (L // cs) % 2, 128)
    rot = torch.randn(1, Ce, nh, hb // 2, generator=gen, dtype=D)
    taps = {}
    O._nlsa(sd, "a", x, nh, cs, 0.1, rotations=rot, taps=taps)
    assert taps["hash_buckets"] == hb
    rows = x.reshape(N, C, L).permute(0, 2, 1)[..., :Ce].reshape(N * L, Ce)
    rotated = rows @ rot[0].reshape(Ce, nh * (hb // 2))
    keys = R.lsh_order(rotated, N, L, nh, hb)
    tok = keys & ((1 << R.TOK_BITS) - 1)
    grp = keys >> R.TOK_BITS
    n_idx = torch.arange(N).view(N, 1, 1)
    h_idx = torch.arange(nh).view(1, nh, 1)
    code = grp - (n_idx * nh + h_idx) * hb
    assert code.min() >= 0 and code.max() < hb
    ocodes = taps["codes"].reshape(N, nh, L)                       # in token positions, offset by h * hb
    assert torch.equal(ocodes.gather(2, tok), code + h_idx * hb)   # lsh_order's code of a token is the oracle's
    oidx = taps["indices"].reshape(N, nh, L)
    assert torch.equal(oidx // L, h_idx.expand(N, nh, L))
    otok = oidx % L
    ocode = ocodes.gather(2, otok) - h_idx * hb
    assert torch.equal(ocode, code)                                # the same code at every sorted position
    pair = code * L + tok
    assert torch.equal(pair, pair.sort(dim=-1).values)             # by code, tokens ascending within a code
    assert torch.equal((ocode * L + otok).sort(dim=-1).values, pair)   # the same tokens per code as the oracle


def test_lsh_order_ties_first_maximum_and_stable():
    """the tie rules stated by hand: an all-zero row takes code 0, r and -r tying takes the r half, equal maxima take the
    first, and equal codes keep token order"""
    rotated = torch.tensor([[0., 0.], [0.5, -0.5], [-0.5, 0.5], [0.25, 0.25], [-1., 1.], [0., 0.]], dtype=D)
    keys = R.lsh_order(rotated, 1, 6, 1, 4)
    # codes: 0 (all equal), 0 (r0 = 0.5 ties -r1 = 0.5: first), 1 (r1 = 0.5 ties -r0), 0, 1 (r1 = 1 ties -r0 = 1), 0
    assert keys.tolist() == [[[(0 << 20) | 0, (0 << 20) | 1, (0 << 20) | 3, (0 << 20) | 5, (1 << 20) | 2, (1 << 20) | 4]]]


@pytest.mark.parametrize("grid", [False, True])
def test_channel_attention_matches_oracle(grid):
    """channel_attention (view / permute) against the einops statement of O._omni_channel_attention, on a non-square map"""
    from einops import rearrange
    gen = _gen(5)
    B, H, W, heads, d, ps = 2, 8, 12, 4, 3, 4
    C = heads * d
    qkv = torch.randn(B, 3 * C, H, W, generator=gen, dtype=D)
    temp = torch.rand(heads, 1, 1, generator=gen, dtype=D) + 0.5
    pat = ('b (head d) (h ph) (w pw) -> b (ph pw) head d (h w)' if grid else
           'b (head d) (h ph) (w pw) -> b (h w) head d (ph pw)')
    q, k, v = (rearrange(t, pat, ph=ps, pw=ps, head=heads) for t in qkv.chunk(3, dim=1))
    q, k = F.normalize(q, dim=-1), F.normalize(k, dim=-1)
    out = ((q @ k.transpose(-2, -1)) * temp).softmax(dim=-1) @ v
    back = ('b (ph pw) head d (h w) -> b (head d) (h ph) (w pw)' if grid else
            'b (h w) head d (ph pw) -> b (head d) (h ph) (w pw)')
    ref = rearrange(out, back, h=H // ps, w=W // ps, ph=ps, pw=ps, head=heads)
    got = R.channel_attention(qkv.permute(0, 2, 3, 1), temp.reshape(heads), heads, ps, grid).permute(0, 3, 1, 2)
    assert (got - ref).abs().max().item() <= 1e-14


def test_group_attention_matches_loop():
    gen = _gen(6)
    G, n, heads, dh = 3, 5, 2, 3
    C = heads * dh
    qkv = torch.randn(G * n, 3 * C, generator=gen, dtype=D)
    bias = torch.randn(heads, n, n, generator=gen, dtype=D)
    got = R.group_attention(qkv, bias, n, heads, 0.7)
    for g in range(G):
        rows = qkv[g * n:(g + 1) * n]
        for h in range(heads):
            q, k, v = (rows[:, o * C + h * dh:o * C + (h + 1) * dh] for o in range(3))
            ref = torch.softmax(0.7 * q @ k.t() + bias[h], dim=-1) @ v
            assert (got[g * n:(g + 1) * n, h * dh:(h + 1) * dh] - ref).abs().max().item() <= 1e-14


def test_fft2_statement_matches_oracle_lines_and_odd_shift():
    """fft2_mag_pow_shift against a direct DFT sum at an odd size: out[i][j] = spectrum[(i + H // 2) % H][(j + W // 2) % W]"""
    gen = _gen(7)
    B, H, W, C = 1, 5, 3, 2
    x = torch.randn(B, H, W, C, generator=gen, dtype=D)
    got = R.fft2_mag_pow_shift(x, 0.8, 1e-8)
    u, v = torch.arange(H, dtype=D), torch.arange(W, dtype=D)
    for i in range(H):
        for j in range(W):
            uu, vv = (i + H // 2) % H, (j + W // 2) % W
            ph = -2 * math.pi * (uu * u[:, None] / H + vv * v[None, :] / W)
            re = (x[0] * torch.cos(ph)[..., None]).sum(dim=(0, 1))
            im = (x[0] * torch.sin(ph)[..., None]).sum(dim=(0, 1))
            ref = ((re * re + im * im).sqrt() + 1e-8) ** 0.8
            assert (got[0, i, j] - ref).abs().max().item() <= 1e-12


@pytest.mark.parametrize("H,W", [(2, 2), (3, 3), (2, 5), (3, 17), (5, 4)])
def test_pad_crop_adjoint_pairs(H, W):
    """<A x, g> == <x, A^T g> with A^T from autograd, for the reflection padding, the crop and the bilinear resize; the
    H == 3 padding puts both mirrors on row 1"""
    gen = _gen(H * 31 + W)
    x = torch.randn(2, H, W, 4, generator=gen, dtype=D)
    g = torch.randn(2, H + 2, W + 2, 4, generator=gen, dtype=D)
    (at,) = R.vjp(R.pad_reflect1, (x,), g)
    assert abs((R.pad_reflect1(x) * g).sum().item() - (x * at).sum().item()) <= 1e-12
    if H == 3 and W >= 5:                           # column 2 is interior: padded column 3 only
        assert (at[:, 1, 2] - (g[:, 2, 3] + g[:, 0, 3] + g[:, 4, 3])).abs().max().item() <= 1e-14
    xp = torch.randn(2, H + 2, W + 2, 4, generator=gen, dtype=D)
    gc = torch.randn(2, H, W, 4, generator=gen, dtype=D)
    (ct,) = R.vjp(R.crop1, (xp,), gc)
    assert abs((R.crop1(xp) * gc).sum().item() - (xp * ct).sum().item()) <= 1e-12
    assert ct[:, 0].abs().max().item() == 0 and ct[:, :, -1].abs().max().item() == 0
    gb = torch.randn(2, 7, 3, 4, generator=gen, dtype=D)
    (bt,) = R.vjp(lambda t: R.bilinear_resize(t, 7, 3), (x,), gb)
    assert abs((R.bilinear_resize(x, 7, 3) * gb).sum().item() - (x * bt).sum().item()) <= 1e-12


def test_pad_reflect_mirrors_by_hand():
    """padded row 0 is source row 1 and padded row H + 1 is source row H - 2 (and the same for columns)"""
    x = torch.arange(2 * 4 * 5 * 1, dtype=D).reshape(2, 4, 5, 1)
    p = R.pad_reflect1(x)
    assert torch.equal(p[:, 0, 1:-1], x[:, 1]) and torch.equal(p[:, -1, 1:-1], x[:, -2])
    assert torch.equal(p[:, 1:-1, 0], x[:, :, 1]) and torch.equal(p[:, 1:-1, -1], x[:, :, -2])
    assert torch.equal(p[:, 0, 0], x[:, 1, 1]) and torch.equal(R.crop1(p), x)


def _gc(fn, *inputs):
    xs = [t.clone().requires_grad_(True) for t in inputs]
    assert torch.autograd.gradcheck(fn, xs, eps=1e-6, atol=1e-6, rtol=1e-5)


def test_backward_references_gradcheck():
    """every statement whose autograd is a backward reference of the GPU module, at a tiny size"""
    gen = _gen(9)

    def r(*s):
        return torch.randn(*s, generator=gen, dtype=D)
    _gc(lambda x: R.softmax_rows_lse(x, 0.7)[0], r(3, 5))
    _gc(lambda x: R.softmax_rows_lse(x, 0.7)[1], r(3, 5))
    _gc(lambda x: R.l2norm_rows(x, math.sqrt(6), 5e-5), r(3, 4))
    _gc(lambda x: R.l2norm_rows(x, 1.0, 5e-5), r(3, 4) * 1e-6)                  # clamped rows
    _gc(lambda a, b: R.performer_features(a, b), r(3, 5), r(3, 4))
    _gc(lambda x, p: R.performer_chain(x, p, math.sqrt(6)), r(3, 4), r(5, 4))
    _gc(lambda n, x: R.enlca_finish(n, x, 0.1), torch.cat([r(3, 4), r(3, 1).abs() + 1.0], 1), r(3, 4))
    _gc(lambda x, g, b: R.layernorm_rows(x, g, b), r(3, 6), r(6), r(6))
    _gc(lambda x: R.unary(x, "gelu"), r(7))
    _gc(lambda x: R.unary(x, "sigmoid"), r(7))
    _gc(lambda x: R.fft2_mag_pow_shift(x), r(1, 3, 4, 2))
    _gc(lambda x, a: R.prelu(x, a), r(9) + 0.05, torch.tensor([0.25], dtype=D))
    _gc(R.pad_reflect1, r(1, 3, 2, 1))
    _gc(R.crop1, r(1, 4, 5, 1))


def test_performer_diag_path_is_projected_out():
    """the claim k_performer_features_bwd rests on: behind k * F.normalize (unclamped rows) |data|^2 / 2 is the constant
    k^2 / 2, so the chain's gradient equals the one through `dash` alone"""
    gen = _gen(10)
    x, proj, g = (torch.randn(*s, generator=gen, dtype=D) for s in ((4, 6), (5, 6), (4, 5)))
    k = math.sqrt(6)
    (full,) = R.vjp(lambda t: R.performer_chain(t, proj, k), (x,), g)

    def dash_only(t):
        y = R.l2norm_rows(t, k)
        return R.performer_features(y @ proj.t(), y.detach())
    (part,) = R.vjp(dash_only, (x,), g)
    assert (full - part).abs().max().item() <= 1e-12 * full.abs().max().item()
