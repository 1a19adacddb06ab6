"""DRRN trained under --amp on fp16 storage (conv_h16_bwd.hip, DRRNEngine.forward_h16(save=True) / backward_h16,
TrainStep(amp=True)) against the reference's autocast + GradScaler step (model_plain.py:318-395 with network_drrn.py:22-126):
the shared-weight weight gradient, the unit's masked data-gradient chain with the identity gradient into x0 and the tail's
masked input gradient against float64 on the same fp16 operands; one step and five Adam steps against the oracle's DRRN run
under torch.autocast + a fresh GradScaler per step, with the oracle's float64 autograd as the truth; the GradScaler's skip
rules; graph against eager, one-rank DDP, run-to-run identity; and main.py with DRRN and --amp True."""
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import sr_oracle as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CH = 128


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


def packs(w):
    """fp16x2 forward / data-gradient packs of a conv weight [Co,Ci,3,3] (leading plane = what the h16 kernels read)."""
    from srhip import ops
    Co, Ci = w.shape[:2]
    ws = ops.WeightSet()
    tb = ops.PrepTable()
    tb.conv(w, ws.planes("wp", 9 * Co, Ci, w.device), force_f16=True)
    tb.conv(w, ws.planes("wpt", 9 * Ci, Co, w.device), data_grad=True, force_f16=True)
    tb.build(w.device).run()
    return ws["wp"], ws["wpt"], tb


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


def _dgrad_ref(dY, w):
    """conv_transpose-style data gradient of a 3x3 conv (stride 1, padding 1) and its magnitude sum, float64, NCHW."""
    wd = w.double().flip(2, 3).transpose(0, 1)
    return F.conv2d(dY.double(), wd, padding=1), F.conv2d(dY.double().abs(), wd.abs(), padding=1)


def _wgrad_ref(dY, X):
    """dW [Co,Ci,3,3] and its magnitude sum in float64 (im2col GEMM on the GPU)."""
    B, Ci, H, W = X.shape
    Co = dY.shape[1]
    cols = F.unfold(X.double(), 3, padding=1)
    dy = dY.double().reshape(B, Co, H * W)
    dw = torch.einsum("bok,bck->oc", dy, cols).reshape(Co, Ci, 3, 3)
    dwa = torch.einsum("bok,bck->oc", dy.abs(), cols.abs()).reshape(Co, Ci, 3, 3)
    return dw, dwa


SHAPES = [(8, 64, 64), (2, 24, 40)]


# ---------------------------------------------------------------------------------------------------- 1. kernels
@pytest.mark.parametrize("U", [1, 3, 25])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_shared_weight_gradient_sums_every_application(B, H, W, U):
    """Two shared weights, one launch per application (as DRRN's unit: two problems), the first overwriting, the rest adding:
    within check_f32's bound of the float64 sum over all applications."""
    from srhip import ops
    g = torch.Generator().manual_seed(U * 7 + H)
    dWa = torch.full((CH, CH, 3, 3), float("nan"), device="cuda")
    dWb = torch.full((CH, CH, 3, 3), float("nan"), device="cuda")
    ra = torch.zeros(CH, CH, 3, 3, dtype=torch.float64, device="cuda")
    rb, raa, rba = ra.clone(), ra.clone(), ra.clone()
    for k in range(U):
        Xa = h(torch.relu(torch.randn(B, CH, H, W, generator=g))).cuda()
        Xb = h(torch.relu(torch.randn(B, CH, H, W, generator=g))).cuda()
        dYa = h(torch.randn(B, CH, H, W, generator=g) * 0.01).cuda()
        dYb = h(torch.randn(B, CH, H, W, generator=g) * 0.01).cuda()
        ops.conv3x3_wgrad_shared_h16([(nhwc(dYb).half(), nhwc(Xb).half(), dWb, None),
                                      (nhwc(dYa).half(), nhwc(Xa).half(), dWa, None)], accumulate=k > 0)
        for (dY, X, r, rabs) in ((dYa, Xa, ra, raa), (dYb, Xb, rb, rba)):
            w, wa = _wgrad_ref(dY, X)
            r += w
            rabs += wa
    check_f32(dWa, ra, raa)
    check_f32(dWb, rb, rba)


def test_shared_weight_gradient_is_deterministic_and_leaves_the_batched_one_alone():
    from srhip import ops
    g = torch.Generator().manual_seed(3)
    B, H, W = 2, 24, 40
    maps = [h(torch.randn(B, CH, H, W, generator=g)).cuda() for _ in range(6)]
    items = [(nhwc(maps[2 * k]).half(), nhwc(maps[2 * k + 1]).half()) for k in range(3)]
    outs = []
    for _ in range(2):
        dW = torch.empty(CH, CH, 3, 3, device="cuda")
        for k, (dY, X) in enumerate(items):
            ops.conv3x3_wgrad_shared_h16([(dY, X, dW, None)], accumulate=k > 0)
        outs.append(dW)
    assert torch.equal(outs[0], outs[1])
    # one application alone = the batched (overwriting) weight gradient's value within its bound
    one = torch.empty(CH, CH, 3, 3, device="cuda")
    ops.conv3x3_wgrad_shared_h16([(items[0][0], items[0][1], one, None)], accumulate=False)
    ref = torch.empty(CH, CH, 3, 3, device="cuda")
    ops.conv3x3_wgrad_h16([(items[0][0], items[0][1], ref, None)])
    w, wa = _wgrad_ref(maps[0], maps[1])
    check_f32(one, w, wa)
    check_f32(ref, w, wa)


def test_shared_weight_gradient_refuses_overlapping_outputs():
    from srhip import ops
    from srhip._lib import SrhipError
    g = torch.Generator().manual_seed(4)
    dY = nhwc(h(torch.randn(1, CH, 8, 32, generator=g))).half().cuda()
    X = nhwc(h(torch.randn(1, CH, 8, 32, generator=g))).half().cuda()
    big = torch.zeros(2 * CH * CH * 9, device="cuda")
    a = big[:CH * CH * 9].view(CH, CH, 3, 3)
    b = big[CH * CH * 9 // 2:CH * CH * 9 // 2 + CH * CH * 9].view(CH, CH, 3, 3)     # overlaps a; another base pointer
    with pytest.raises(SrhipError, match="share an output"):
        ops.conv3x3_wgrad_shared_h16([(dY, X, a, None), (dY, X, b, None)], accumulate=False)


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_unit_data_gradient_chain_with_the_identity_gradient(B, H, W):
    """Three units of the backward on fp16: ga = (a > 0) conv_b^T(gu) (epi 9), gu' = (r > 0) conv_a^T(ga) with G += gu'
    (mode 0), the last unit (r_0 = x0) = (x0 > 0) (conv_a^T(ga) + G) (mode 1); G starts as the tail's gu.  Every step
    against float64 on the fp16 operands it was given."""
    from srhip import ops
    g = torch.Generator().manual_seed(B * 3 + W)
    wa = h(torch.randn(CH, CH, 3, 3, generator=g) * 0.03).cuda()
    wb = h(torch.randn(CH, CH, 3, 3, generator=g) * 0.03).cuda()
    _, wat, _ka = packs(wa)
    _, wbt, _kb = packs(wb)
    U = 3
    rs = [h(torch.relu(torch.randn(B, CH, H, W, generator=g))).cuda() for _ in range(U)]      # r_0 = x0, r_1, r_2
    as_ = [h(torch.relu(torch.randn(B, CH, H, W, generator=g))).cuda() for _ in range(U)]
    gu = nhwc(h(torch.randn(B, CH, H, W, generator=g))).half().cuda()
    G = gu.float().clone()
    ga = torch.empty_like(gu)
    gus = [torch.empty_like(gu), torch.empty_like(gu)]
    for k in reversed(range(U)):
        ops.conv3x3_h16(gu, wbt, None, CH, out=ga, epi=9, R=nhwc(as_[k]).half(), alpha=1.0)
        ref, refabs = _dgrad_ref(nchw(gu.float()), wb)
        m = (as_[k] > 0).double()
        check_h16(nchw(ga.float()), ref * m, refabs)
        ref, refabs = _dgrad_ref(nchw(ga.float()), wa)
        m = (rs[k] > 0).double()
        G0 = nchw(G).double()
        out = gus[k % 2]
        ops.conv3x3_dgrad_relu_acc_h16(ga, wat, nhwc(rs[k]).half(), out, G, mode=0 if k else 1)
        if k:
            check_h16(nchw(out.float()), ref * m, refabs)
            gref = G0 + nchw(out.float()).double()
            check_f32(nchw(G), gref, G0.abs() + nchw(out.float()).double().abs())
        else:
            check_h16(nchw(out.float()), (ref + G0) * m, refabs + G0.abs())
            assert torch.equal(nchw(G).double(), G0)                   # mode 1 only reads G
        gu = out


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_tail_masked_input_gradient(B, H, W):
    from srhip import ops
    g = torch.Generator().manual_seed(11 + H)
    dy = (torch.randn(B, 1, H, W, generator=g) * 100).cuda()
    w2 = (torch.randn(1, CH, 3, 3, generator=g) * 0.05).cuda()
    r = h(torch.relu(torch.randn(B, CH, H, W, generator=g))).cuda()
    out = torch.empty(B, H, W, CH, device="cuda", dtype=torch.float16)
    G = torch.full((B, H, W, CH), float("nan"), device="cuda")
    ops.conv3x3_cin1_h16_flip_mask(dy[:, 0].contiguous(), w2, nhwc(r).half(), out, G)
    ref, refabs = _dgrad_ref(dy, w2)
    check_h16(nchw(out.float()), ref * (r > 0).double(), refabs)
    assert torch.equal(G, out.float())
    # the weight gradient of the tail: the 1-channel form, taps mirrored, no bias
    dW2 = torch.empty(1, CH, 3, 3, device="cuda")
    ops.conv3x3_cin1_wgrad_h16(dy[:, 0].contiguous(), nhwc(r).half(), dW2, None, flip=True)
    rw, rwa = _wgrad_ref(dy, r)
    check_f32(dW2, rw, rwa)


def test_masked_data_gradient_refuses_overlapping_ranges():
    """dX interleaved with the mask R in one buffer: different base pointers, overlapping byte ranges."""
    from srhip import ops
    from srhip._lib import SrhipError
    B, H, W = 1, 8, 16
    _, wat, _k = packs(h(torch.randn(CH, CH, 3, 3) * 0.03).cuda())
    dY = torch.zeros(B, H, W, CH, device="cuda", dtype=torch.float16)
    both = torch.zeros(B, H, W, 2 * CH, device="cuda", dtype=torch.float16)
    G = torch.zeros(B, H, W, CH, device="cuda")
    with pytest.raises(SrhipError, match="overlaps"):
        ops.conv3x3_dgrad_relu_acc_h16(dY, wat, both[..., :CH], both[..., CH:], G, mode=0)


# ---------------------------------------------------------------------------------------------------- 2. one step
SHARED = ("trunk.residual_unit.1.weight", "trunk.residual_unit.3.weight")


def _sd(U, seed):
    """The reference's init (kaiming fan_out).  A 25-unit recursion at that init amplifies the gradient so much that its
    scaled shared-weight gradients pass 65504 (the reference's GradScaler skips such a step, and so does this one: the skip
    tests); 0.7 x the shared weights keeps the comparisons with deep recursions in range."""
    sd = O.drrn_init_state_dict(1, seed=seed)
    if U >= 25:
        for k in SHARED:
            sd[k] = sd[k] * 0.7
    return sd


def _near(sd, x, scale, U, g, noise=0.05, offset=0.01):
    """A target near the net's output (the regime of a net in training) and a little below it: the scaled gradient sums
    stay inside fp16 at the reference's init (a far target overflows conv1's, for the reference too), and a systematic
    part keeps the gradients from being pure cancellation noise."""
    with torch.no_grad():
        y = O.drrn_forward({k: v.cuda() for k, v in sd.items()}, x.cuda(), scale, U).cpu()
    return y + noise * torch.randn(y.shape, generator=g) - offset


def _net(U, scale, sd):
    from dlib.models.network_drrn import DRRN
    net = DRRN(upscale=scale, in_chans=1, num_residual_units=U)
    net.load_state_dict(sd, strict=True)
    net = net.cuda()
    net.amp = True
    return net


def _autocast_grads(sd, x, tgt, scale, U, loss="l1"):
    """The reference's --amp step: autocast forward + loss, a fresh GradScaler, scale(loss).backward(), unscaled grads."""
    p = {k: v.clone().cuda().requires_grad_(True) for k, v in sd.items()}
    scaler = torch.amp.GradScaler("cuda")
    with torch.autocast("cuda", torch.float16):
        y = O.drrn_forward(p, x.cuda(), scale, U)
        lv = F.l1_loss(y, tgt.cuda()) if loss == "l1" else F.mse_loss(y, tgt.cuda())
    scaler.scale(lv).backward()
    inv = 1.0 / scaler.get_scale()
    return {k: (v.grad * inv).cpu().double() for k, v in p.items()}, lv.item()


def _truth_grads(sd, x, tgt, scale, U):
    p = {k: v.double().cuda().clone().requires_grad_(True) for k, v in sd.items()}
    lv = F.l1_loss(O.drrn_forward(p, x.double().cuda(), scale, U), tgt.double().cuda())
    lv.backward()
    return {k: v.grad.cpu() for k, v in p.items()}, lv.item()


def _rel(a, b):
    return ((a.double() - b).norm() / b.norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("U,scale,B,P", [(1, 2, 2, 16), (3, 8, 2, 8), (25, 2, 2, 16), (3, 2, 2, 20), (25, 8, 8, 8)])
def test_one_step_against_autocast(U, scale, B, P):
    from srhip.train import Optimizer, TrainStep
    sd = _sd(U, 11 + U)
    g = torch.Generator().manual_seed(3 + scale)
    x = torch.rand(B, 1, P, P, generator=g)
    tgt = _near(sd, x, scale, U, g)
    truth, l64 = _truth_grads(sd, x, tgt, scale, U)
    ac, lac = _autocast_grads(sd, x, tgt, scale, U)
    net = _net(U, scale, sd)
    st = TrainStep(net, [("l1", 1.0)], amp=True)
    st.opt = Optimizer(st.fp, "adam", lr=0.0)
    st.step(x.cuda(), tgt.cuda())
    torch.cuda.synchronize()
    lours = st.loss_values()[0]
    assert abs(lours - l64) <= 4 * abs(lac - l64) + 1e-4 * l64, (lours, lac, l64)
    assert st.overflow.item() == 0 and st.flag.item() == 0
    worst = []
    for k, gt in truth.items():
        ours = st.fp.gviews[k].detach().cpu()
        eo, ea = _rel(ours, gt), _rel(ac[k], gt)
        worst.append((eo / max(ea, 1e-3), k, eo, ea))
        assert eo <= 1.25 * ea + 1e-3, (k, eo, ea)
    print("worst ratio", max(worst))


def test_five_adam_steps_against_autocast():
    from srhip.train import Optimizer, TrainStep
    U, scale = 3, 2
    sd = _sd(U, 5)
    g = torch.Generator().manual_seed(4)
    xs = [torch.rand(2, 1, 16, 16, generator=g) for _ in range(5)]
    batches = [(x, _near(sd, x, scale, U, g)) for x in xs]
    lr = 1e-3
    p64 = {k: v.double().cuda().clone().requires_grad_(True) for k, v in sd.items()}
    o64 = torch.optim.Adam(p64.values(), lr=lr)
    pac = {k: v.clone().cuda().requires_grad_(True) for k, v in sd.items()}
    oac = torch.optim.Adam(pac.values(), lr=lr)
    net = _net(U, scale, sd)
    st = TrainStep(net, [("l1", 1.0)], amp=True)
    st.opt = Optimizer(st.fp, "adam", lr=lr)
    for x, t in batches:
        o64.zero_grad()
        F.l1_loss(O.drrn_forward(p64, x.double().cuda(), scale, U), t.double().cuda()).backward()
        o64.step()
        oac.zero_grad()
        scaler = torch.amp.GradScaler("cuda")
        with torch.autocast("cuda", torch.float16):
            lv = F.l1_loss(O.drrn_forward(pac, x.cuda(), scale, U), t.cuda())
        scaler.scale(lv).backward()
        scaler.step(oac)
        st.step(x.cuda(), t.cuda())
    torch.cuda.synchronize()
    sdo = net.state_dict()
    for k in sd:
        p = p64[k].detach().cpu()
        do = (sdo[k].cpu().double() - p).norm().item()
        da = (pac[k].detach().cpu().double() - p).norm().item()
        ref = (p - sd[k].double()).norm().item()
        assert do <= 1.25 * da + 1e-3 * ref, (k, do, da, ref)


def test_two_runs_from_one_state_are_bit_identical():
    from srhip.train import Optimizer, TrainStep
    sd = _sd(4, 21)
    g = torch.Generator().manual_seed(22)
    xs = [torch.rand(2, 1, 12, 12, generator=g) for _ in range(3)]
    batches = [(x.cuda(), _near(sd, x, 4, 4, g).cuda()) for x in xs]
    out = []
    for _ in range(2):
        net = _net(4, 4, sd)
        st = TrainStep(net, [("l1", 1.0)], amp=True)
        # Adam's first steps move every weight by ~lr at once: tiny ones keep the targets near the output (no overflow)
        st.opt = Optimizer(st.fp, "adam", lr=1e-7)
        for x, t in batches:
            st.step(x, t)
        torch.cuda.synchronize()
        assert st.opt.applied.item() == 3
        out.append((st.fp.flat.clone(), st.fp.grad.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


# ---------------------------------------------------------------------------------------------------- 3. skip rules
def _skip_setup(ema=0.0, clip=0.0, U=3):
    from srhip.train import Optimizer, TrainStep
    sd = O.drrn_init_state_dict(1, seed=6)
    net = _net(U, 2, sd)
    st = TrainStep(net, [("l2", 1.0)], amp=True, ema_decay=ema, clipgrad=clip)
    st.opt = Optimizer(st.fp, "adam", lr=1e-3, scheduler={"type": "MyStepLR", "step_size": 1, "gamma": 0.5, "min_lr": 1e-6})
    return sd, net, st


def test_overflow_skips_the_update_but_not_the_ema_or_the_schedule():
    sd, net, st = _skip_setup(ema=0.9)
    U = 3
    g = torch.Generator().manual_seed(8)
    x = torch.rand(2, 1, 32, 32, generator=g)
    t = O.drrn_forward(sd, x, 2, U).detach() + 0.01 * torch.randn(2, 1, 64, 64, generator=g)
    st.step(x.cuda(), t.cuda())
    torch.cuda.synchronize()
    assert st.opt.applied.item() == 1 and st.overflow.item() == 0
    big = torch.full((2, 1, 64, 64), 1e4)
    # the reference skips this step: the scaled output gradient overflows fp16
    pac = {k: v.clone().cuda().requires_grad_(True) for k, v in sd.items()}
    opt = torch.optim.SGD(pac.values(), lr=1.0)
    sc = torch.amp.GradScaler("cuda")
    with torch.autocast("cuda", torch.float16):
        lv = F.mse_loss(O.drrn_forward(pac, x.cuda(), 2, U), big.cuda())
    sc.scale(lv).backward()
    before_ref = {k: v.detach().clone() for k, v in pac.items()}
    sc.step(opt)
    assert all(torch.equal(before_ref[k], pac[k].detach()) for k in pac), "torch's GradScaler did not skip"
    flat0, m0, v0 = st.fp.flat.clone(), st.opt.m.clone(), st.opt.v.clone()
    e0 = st.ema_flat.clone()
    lr0, sc0 = st.opt.lr, st.opt.sched_count
    st.step(x.cuda(), big.cuda())
    torch.cuda.synchronize()
    assert st.overflow.item() == 1 and st.flag.item() == 0
    assert torch.equal(st.fp.flat, flat0) and torch.equal(st.opt.m, m0) and torch.equal(st.opt.v, v0)
    assert st.opt.applied.item() == 1
    assert st.opt.sched_count == sc0 + 1 and st.opt.lr != lr0
    assert torch.allclose(st.ema_flat, e0 * 0.9 + flat0 * 0.1, rtol=1e-6, atol=1e-7)
    assert not torch.equal(st.ema_flat, e0)
    assert int(st.sticky.item()) == 0
    assert math.isfinite(st.loss_values()[0])


def test_nonfinite_input_keeps_the_full_skip():
    sd, net, st = _skip_setup(ema=0.9)
    g = torch.Generator().manual_seed(9)
    x, t = torch.rand(2, 1, 32, 32, generator=g), torch.rand(2, 1, 64, 64, generator=g)
    x[0, 0, 3, 3] = float("nan")
    flat0, e0 = st.fp.flat.clone(), st.ema_flat.clone()
    st.step(x.cuda(), t.cuda())
    torch.cuda.synchronize()
    assert st.flag.item() == 1
    assert torch.equal(st.fp.flat, flat0) and torch.equal(st.ema_flat, e0) and st.opt.applied.item() == 0
    assert int(st.sticky.item()) == 1


def test_clipping_sees_the_unscaled_gradient():
    sd, net, st = _skip_setup(clip=1e-6)
    g = torch.Generator().manual_seed(10)
    x = torch.rand(2, 1, 32, 32, generator=g)
    t = _near(sd, x, 2, 3, g, noise=0.01, offset=0.05)       # MSE: a systematic gradient, not cancellation noise
    p = {k: v.clone().cuda().requires_grad_(True) for k, v in sd.items()}
    sc = torch.amp.GradScaler("cuda")
    with torch.autocast("cuda", torch.float16):
        lv = F.mse_loss(O.drrn_forward(p, x.cuda(), 2, 3), t.cuda())
    sc.scale(lv).backward()
    sc.unscale_(torch.optim.SGD(p.values(), lr=0.0))
    ref = torch.norm(torch.stack([v.grad.norm() for v in p.values()])).item()
    assert math.isfinite(ref)
    st.step(x.cuda(), t.cuda())
    torch.cuda.synchronize()
    assert st.overflow.item() == 0
    norm = st.clip_state[0].item()
    assert abs(norm - ref) <= 0.01 * ref, (norm, ref)


# ---------------------------------------------------------------------------------------------------- 4. ModelPlain, ranks, CLI
class Args(dict):
    __getattr__ = dict.get


def drrn_args(tmp_path, amp=True):
    from dlib.utils import constants
    nt = constants.DRRN
    netG = {'net_type': nt, f'{nt}_in_chans': 1, f'{nt}_upscale': 2, f'{nt}_num_residual_units': 3}
    train = {'l1': True, 'G_optimizer_type': 'adam', 'G_optimizer_lr': 1e-7, 'G_optimizer_wd': 0.0,
             'G_scheduler_type': 'MyStepLR', 'G_scheduler_step_size': 30, 'G_scheduler_gamma': 0.5,
             'G_scheduler_min_lr': 1e-9}
    return Args(netG=netG, train=train, is_train=True, amp=amp, outd=str(tmp_path), method=nt)


def _run_model(tmp_path, graph, steps=3):
    from dlib.models.select_model import define_model
    os.environ["SRHIP_TRAIN_GRAPH"] = "1" if graph else "0"
    try:
        model = define_model(drrn_args(tmp_path))
        assert model.netG.trunk.num_residual_unit == 3
        sd = O.drrn_init_state_dict(1, seed=12)
        model.netG.load_state_dict(sd, strict=True)
        model.init_train()
        assert model.step_fn.amp
        g = torch.Generator().manual_seed(13)
        for i in range(steps):
            x = torch.rand(2, 1, 16, 16, generator=g)
            model.feed_data({'l_im': x, 'h_im': _near(sd, x, 2, 3, g)})
            model.optimize_parameters(0, i)
        torch.cuda.synchronize()
        assert model.step_fn.opt.applied.item() == steps
        return {k: v.detach().cpu().clone() for k, v in model.netG.state_dict().items()}, model
    finally:
        os.environ.pop("SRHIP_TRAIN_GRAPH", None)


def test_model_plain_drrn_amp_graph_equals_eager(tmp_path):
    sd_e, _ = _run_model(tmp_path, graph=False)
    sd_g, m = _run_model(tmp_path, graph=True)
    assert m.step_fn._graph is not None and m.step_fn._graph["g"] is not None
    for k in sd_e:
        assert torch.equal(sd_e[k], sd_g[k]), k
    assert m.check_finite()


DDP_WORKER = r'''
import os, sys, torch, torch.distributed as dist
root = sys.argv[1]
for p in (os.path.join(root, "sr-caco-2_amd"), os.path.join(root, "oracle"), root):
    sys.path.insert(0, p)
import sr_oracle as O
from dlib.models.network_drrn import DRRN
from srhip.train import Optimizer, TrainStep
dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{sys.argv[2]}", rank=0, world_size=1,
                        device_id=torch.device("cuda", 0))
sd = O.drrn_init_state_dict(1, seed=14)
gen = torch.Generator().manual_seed(15)
xs = [torch.rand(2, 1, 16, 16, generator=gen) for _ in range(2)]
with torch.no_grad():                            # targets near the output: the first two steps apply
    batches = [(x.cuda(), (O.drrn_forward(sd, x, 2, 3) + 0.05 * torch.randn(2, 1, 32, 32, generator=gen) - 0.01).cuda())
               for x in xs]
batches.append((batches[0][0], torch.full((2, 1, 32, 32), 1e4, device="cuda")))      # an overflowing step
out = {}
for mode in ("plain", "ddp"):
    os.environ["SRHIP_FORCE_DDP"] = "1" if mode == "ddp" else "0"
    net = DRRN(upscale=2, in_chans=1, num_residual_units=3)
    net.load_state_dict(sd, strict=True)
    net = net.cuda()
    net.amp = True
    ts = TrainStep(net, [("l2", 1.0)], process_group=dist.group.WORLD if mode == "ddp" else None, world_size=1, amp=True)
    ts.opt = Optimizer(ts.fp, "adam", lr=1e-7)
    assert ts.ddp == (mode == "ddp")
    for lr_img, hr_img in batches:
        ts.step(lr_img, hr_img)
    torch.cuda.synchronize()
    assert ts.overflow.item() == 1 and ts.opt.applied.item() == 2
    out[mode] = (ts.fp.flat.clone(), ts.loss_buf.clone())
assert torch.equal(out["plain"][0], out["ddp"][0]) and torch.equal(out["plain"][1], out["ddp"][1])
dist.destroy_process_group()
print("ddp amp ok")
'''


def test_one_rank_ddp_amp_step_matches_the_plain_one(tmp_path):
    """SRHIP_FORCE_DDP=1 with a one-rank nccl group: the DRRN amp steps (one of them overflowing: the flag goes through the
    MAX-reduce) equal the plain ones bit for bit."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = tmp_path / "ddp_amp_drrn_worker.py"
    script.write_text(DDP_WORKER)
    p = subprocess.run([sys.executable, str(script), ROOT, str(port)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert p.returncode == 0 and "ddp amp ok" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]


def test_other_nets_still_refuse_and_name_the_nets_that_train(tmp_path):
    from dlib.models.model_plain import ModelPlain
    from dlib.models.select_model import define_model
    from dlib.utils import constants
    assert ModelPlain.AMP_TRAIN_NETS == ("EDSR_LIIF", "DRRN")
    nt = constants.VDSR
    a = drrn_args(tmp_path)
    a['netG'] = {'net_type': nt, f'{nt}_in_chans': 1, f'{nt}_upscale': 2}
    a['method'] = nt
    model = define_model(a)
    model.init_train()
    model.feed_data({'l_im': torch.rand(2, 1, 16, 16), 'h_im': torch.rand(2, 1, 32, 32)})
    with pytest.raises(NotImplementedError, match="EDSR_LIIF, DRRN"):
        model.optimize_parameters(0, 0)


def test_main_cli_trains_drrn_under_amp(tmp_path):
    """`main.py --net_type DRRN --method DRRN --amp True`: two iterations of the fp16-storage step to a finite loss."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "sr-caco-2_amd", "main.py"), "--net_type", "DRRN", "--method", "DRRN",
                        "--task", "super-resolution", "--scale", "2", "--n_channels", "1", "--h_size", "64", "--batch_size", "2",
                        "--max_iters", "2", "--DRRN_num_residual_units", "3", "--amp", "True", "--outd", str(tmp_path)],
                       capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    losses = [float(l.split("G_loss")[1].split()[0]) for l in p.stdout.splitlines() if "G_loss" in l]
    assert len(losses) == 1 and math.isfinite(losses[0]), p.stdout[-2000:]
