"""EDSR trained under --amp on fp16 storage (conv_h16_bwd.hip, EDSREngine.forward_h16(save=True) / backward_h16,
TrainStep(amp=True)) against the reference's autocast + GradScaler step (model_plain.py:318-395, tools.py:55):
the kernels against float64 on the same fp16 operands, the unscale / overflow check, one step and five Adam steps against
the oracle's EDSR run under torch.autocast + a fresh GradScaler per step (the reference's --amp) with the oracle's float64
autograd as the truth, the GradScaler's skip rules, and ModelPlain / main.py with EDSR_LIIF and --amp True."""
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
PKG = os.path.join(ROOT, "sr-caco-2_amd")


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


SHAPES = [(8, 64, 64), (2, 24, 40)]


# ---------------------------------------------------------------------------------------------------- 1. kernels
@pytest.mark.parametrize("B,H,W", SHAPES + [(8, 128, 128)])
def test_data_gradient_convs_with_the_training_epilogues(B, H, W):
    from srhip import ops
    g = torch.Generator().manual_seed(B + H)
    Fc = 64
    w = h(torch.randn(Fc, Fc, 3, 3, generator=g) * 0.05).cuda()
    _, wpt, _keep = packs(w)
    gy = h(torch.randn(B, Fc, H, W, generator=g)).cuda()
    a = h(torch.relu(torch.randn(B, Fc, H, W, generator=g))).cuda()
    R = h(torch.randn(B, Fc, H, W, generator=g)).cuda()
    wd = w.double().flip(2, 3).transpose(0, 1)
    ref = F.conv2d(gy.double(), wd, padding=1)
    refabs = F.conv2d(gy.double().abs(), wd.abs(), padding=1)
    gyh = nhwc(gy).half()
    rs = 0.1
    # epi 9: ReLU mask of the kept activation times res_scale
    out = ops.conv3x3_h16(gyh, wpt, None, Fc, epi=9, R=nhwc(a).half(), alpha=rs)
    m = (a > 0).double()
    check_h16(nchw(out.float()), ref * m * rs, refabs * rs)
    # epi 2: + the skip gradient
    out = ops.conv3x3_h16(gyh, wpt, None, Fc, epi=2, R=nhwc(R).half())
    check_h16(nchw(out.float()), ref + R.double(), refabs + R.double().abs())


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_ps2_data_gradient(B, H, W):
    from srhip import ops
    g = torch.Generator().manual_seed(7 + W)
    Fc = 64
    w = h(torch.randn(4 * Fc, Fc, 3, 3, generator=g) * 0.05).cuda()
    _, wpt, _keep = packs(w, ps2=True)
    dup = h(torch.randn(B, Fc, 2 * H, 2 * W, generator=g)).cuda()
    dc = F.pixel_unshuffle(dup.double(), 2)                       # gradient of the conv's output (torch channel order)
    wd = w.double().flip(2, 3).transpose(0, 1)
    ref = F.conv2d(dc, wd, padding=1)
    refabs = F.conv2d(dc.abs(), wd.abs(), padding=1)
    out = torch.empty(B, H, W, Fc, device="cuda", dtype=torch.float16)
    ops.conv3x3_ps2_bwd_data_h16(nhwc(dup).half(), wpt, out)
    check_h16(nchw(out.float()), ref, refabs)


def _wgrad_ref(dY, X):
    """dW [Co,Ci,3,3], db [Co] and their magnitude sums in float64 (im2col GEMM on the GPU)."""
    B, Ci, H, W = X.shape
    Co = dY.shape[1]
    cols = F.unfold(X.double(), 3, padding=1)                      # [B, Ci*9, H*W]
    dy = dY.double().reshape(B, Co, H * W)
    dw = torch.einsum("bok,bck->oc", dy, cols).reshape(Co, Ci, 3, 3)
    dwa = torch.einsum("bok,bck->oc", dy.abs(), cols.abs()).reshape(Co, Ci, 3, 3)
    return dw, dy.sum((0, 2)), dwa, dy.abs().sum((0, 2))


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_batched_weight_gradients_33_items(B, H, W):
    from srhip import ops
    g = torch.Generator().manual_seed(33 + H)
    Fc, n = 64, 33
    Xs = [h(torch.relu(torch.randn(B, Fc, H, W, generator=g))).cuda() for _ in range(n)]
    dYs = [h(torch.randn(B, Fc, H, W, generator=g) * 0.01).cuda() for _ in range(n)]
    dWs = [torch.full((Fc, Fc, 3, 3), float("nan"), device="cuda") for _ in range(n)]
    dbs = [torch.full((Fc,), float("nan"), device="cuda") for _ in range(n)]
    ops.conv3x3_wgrad_h16([(nhwc(dY).half(), nhwc(X).half(), dW, db) for dY, X, dW, db in zip(dYs, Xs, dWs, dbs)])
    for k in range(n):
        rw, rb, rwa, rba = _wgrad_ref(dYs[k], Xs[k])
        check_f32(dWs[k], rw, rwa)
        check_f32(dbs[k], rb, rba)


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_ps2_weight_gradient(B, H, W):
    from srhip import ops
    g = torch.Generator().manual_seed(5 + H)
    Fc = 64
    X = h(torch.randn(B, Fc, H, W, generator=g)).cuda()
    dup = h(torch.randn(B, Fc, 2 * H, 2 * W, generator=g) * 0.01).cuda()
    dW = torch.empty(4 * Fc, Fc, 3, 3, device="cuda")
    db = torch.empty(4 * Fc, device="cuda")
    ops.conv3x3_wgrad_h16([(nhwc(dup).half(), nhwc(X).half(), dW, db)], ps2=True)
    rw, rb, rwa, rba = _wgrad_ref(F.pixel_unshuffle(dup, 2), X)
    check_f32(dW, rw, rwa)
    check_f32(db, rb, rba)


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_head_and_tail_gradients(B, H, W):
    from srhip import ops
    g = torch.Generator().manual_seed(9 + W)
    Fc = 64
    x = torch.rand(B, 1, H, W, generator=g).cuda()
    dY = h(torch.randn(B, Fc, H, W, generator=g) * 0.01).cuda()
    # head: f32 image with fp16 dY
    dW = torch.empty(Fc, 1, 3, 3, device="cuda")
    db = torch.empty(Fc, device="cuda")
    ops.conv3x3_cin1_wgrad_h16(x[:, 0].contiguous(), nhwc(dY).half(), dW, db)
    rw, rb, rwa, rba = _wgrad_ref(dY, x)
    check_f32(dW, rw, rwa)
    check_f32(db, rb, rba)
    # tail: fp16 U with f32 dy -> dW [1, F, 3, 3]
    U = h(torch.randn(B, Fc, H, W, generator=g)).cuda()
    dy = torch.randn(B, 1, H, W, generator=g).cuda() * 0.01
    dWt = torch.empty(1, Fc, 3, 3, device="cuda")
    ops.conv3x3_cin1_wgrad_h16(dy[:, 0].contiguous(), nhwc(U).half(), dWt, None, flip=True)
    rw, _, rwa, _ = _wgrad_ref(dy, U)
    check_f32(dWt, rw, rwa)
    # tail data gradient: f32 dy through the mirrored taps into fp16
    wt = (torch.randn(1, Fc, 3, 3, generator=g) * 0.05).cuda()
    out = ops.conv3x3_cin1_h16_flip(dy[:, 0].contiguous(), wt, Fc)
    wd = wt.double().flip(2, 3).transpose(0, 1)
    check_h16(nchw(out.float()), F.conv2d(dy.double(), wd, padding=1), F.conv2d(dy.double().abs(), wd.abs(), padding=1))
    # long-skip add on fp16
    a16, b16 = nhwc(U).half(), nhwc(dY).half()
    ref = a16.double() + b16.double()
    ops.axpby_h16(a16, b16, 1.0, 1.0)
    assert torch.equal(a16, ref.half())


# ---------------------------------------------------------------------------------------------------- 2. unscale
def test_amp_unscale_check():
    from srhip import ops
    g = torch.Generator().manual_seed(2)
    v = torch.randn(100003, generator=g).cuda() * 1000
    v[17] = 65504.0
    v[99] = -65504.0
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    ref = v * 2.0 ** -16
    ops.amp_unscale_check(v, 2.0 ** -16, flag)
    assert torch.equal(v, ref) and flag.item() == 0
    for bad in (float("inf"), float("-inf"), float("nan"), 65520.0, -65520.0):
        x = torch.randn(5000, generator=g).cuda()
        x[4321] = bad
        flag.zero_()
        ops.amp_unscale_check(x, 2.0 ** -16, flag)
        assert flag.item() == 1, bad


# ---------------------------------------------------------------------------------------------------- 3. one step
def _net(cfg, sd):
    from dlib.models.network_edsr_liif import EDSR_LIIF
    net = EDSR_LIIF(scale=cfg["upscale"], n_resblocks=cfg["n_resblocks"], n_feats=cfg["n_feats"], res_scale=cfg["res_scale"])
    net.load_state_dict(sd, strict=True)
    net = net.cuda()
    net.amp = True
    return net


def _autocast_grads(sd, x, tgt, cfg, loss="l1"):
    """The reference's --amp step: autocast forward + loss, a fresh GradScaler, scale(loss).backward(), unscaled grads."""
    p = {k: v.clone().cuda().requires_grad_(True) for k, v in sd.items()}
    scaler = torch.amp.GradScaler("cuda")
    with torch.autocast("cuda", torch.float16):
        y = O.edsr_forward(p, x.cuda(), cfg)
        lv = F.l1_loss(y, tgt.cuda()) if loss == "l1" else F.mse_loss(y, tgt.cuda())
    scaler.scale(lv).backward()
    inv = 1.0 / scaler.get_scale()
    return {k: (v.grad * inv).cpu().double() for k, v in p.items()}, lv.item(), scaler


def _truth_grads(sd, x, tgt, cfg):
    p = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    lv = F.l1_loss(O.edsr_forward(p, x.double(), cfg), tgt.double())
    lv.backward()
    return {k: v.grad for k, v in p.items()}, lv.item()


def _rel(a, b):
    return ((a.double() - b).norm() / b.norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("nb,scale,B,P", [(2, 2, 2, 32), (16, 8, 8, 64)])
def test_one_step_against_autocast(nb, scale, B, P):
    from srhip.train import Optimizer, TrainStep
    cfg = O.edsr_config(upscale=scale, n_feats=64, n_resblocks=nb)
    sd = O.edsr_init_state_dict(cfg, seed=11)
    g = torch.Generator().manual_seed(3)
    x = torch.rand(B, 1, P, P, generator=g)
    tgt = torch.rand(B, 1, P * scale, P * scale, generator=g)
    truth, l64 = _truth_grads(sd, x, tgt, cfg)
    ac, lac, _ = _autocast_grads(sd, x, tgt, cfg)
    net = _net(cfg, sd)
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
    cfg = O.edsr_config(upscale=2, n_feats=64, n_resblocks=2)
    sd = O.edsr_init_state_dict(cfg, seed=5)
    g = torch.Generator().manual_seed(4)
    batches = [(torch.rand(2, 1, 32, 32, generator=g), torch.rand(2, 1, 64, 64, generator=g)) for _ in range(5)]
    lr = 1e-3
    p64 = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    o64 = torch.optim.Adam(p64.values(), lr=lr)
    pac = {k: v.clone().cuda().requires_grad_(True) for k, v in sd.items()}
    oac = torch.optim.Adam(pac.values(), lr=lr)
    net = _net(cfg, sd)
    st = TrainStep(net, [("l1", 1.0)], amp=True)
    st.opt = Optimizer(st.fp, "adam", lr=lr)
    for x, t in batches:
        o64.zero_grad()
        F.l1_loss(O.edsr_forward(p64, x.double(), cfg), t.double()).backward()
        o64.step()
        oac.zero_grad()
        scaler = torch.amp.GradScaler("cuda")
        with torch.autocast("cuda", torch.float16):
            lv = F.l1_loss(O.edsr_forward(pac, x.cuda(), cfg), t.cuda())
        scaler.scale(lv).backward()
        scaler.step(oac)
        st.step(x.cuda(), t.cuda())
    torch.cuda.synchronize()
    sdo = net.state_dict()
    for k in sd:
        do = (sdo[k].cpu().double() - p64[k].detach()).norm().item()
        da = (pac[k].detach().cpu().double() - p64[k].detach()).norm().item()
        ref = (p64[k].detach() - sd[k].double()).norm().item()
        assert do <= 1.25 * da + 1e-3 * ref, (k, do, da, ref)


# ---------------------------------------------------------------------------------------------------- 4. skip rules
def _skip_setup(ema=0.0, clip=0.0):
    from srhip.train import Optimizer, TrainStep
    cfg = O.edsr_config(upscale=2, n_feats=64, n_resblocks=2)
    sd = O.edsr_init_state_dict(cfg, seed=6)
    net = _net(cfg, sd)
    st = TrainStep(net, [("l2", 1.0)], amp=True, ema_decay=ema, clipgrad=clip)
    st.opt = Optimizer(st.fp, "adam", lr=1e-3, scheduler={"type": "MyStepLR", "step_size": 1, "gamma": 0.5, "min_lr": 1e-6})
    return cfg, sd, net, st


def test_overflow_skips_the_update_but_not_the_ema_or_the_schedule():
    cfg, sd, net, st = _skip_setup(ema=0.9)
    g = torch.Generator().manual_seed(8)
    x = torch.rand(2, 1, 32, 32, generator=g)
    # one applied step (moments and EMA non-trivial) against a target near the output: a far one overflows the scaled
    # tail-bias gradient (sum of dy * 2^16) -- the reference skips such a step too
    t = O.edsr_forward(sd, x, cfg).detach() + 0.01 * torch.randn(2, 1, 64, 64, generator=g)
    st.step(x.cuda(), t.cuda())
    torch.cuda.synchronize()
    assert st.opt.applied.item() == 1
    big = torch.full((2, 1, 64, 64), 1e4)
    # the reference skips this step: the scaled output gradient overflows fp16
    pac = {k: v.clone().cuda().requires_grad_(True) for k, v in sd.items()}
    opt = torch.optim.SGD(pac.values(), lr=1.0)
    sc = torch.amp.GradScaler("cuda")
    with torch.autocast("cuda", torch.float16):
        lv = F.mse_loss(O.edsr_forward(pac, x.cuda(), cfg), big.cuda())
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
    assert torch.equal(st.ema_flat, e0 * 0.9 + flat0 * (1 - 0.9)) or \
        torch.allclose(st.ema_flat, e0 * 0.9 + flat0 * 0.1, rtol=0, atol=1e-7)
    assert int(st.sticky.item()) == 0                            # check_finite() stays True
    assert math.isfinite(st.loss_values()[0])


def test_nonfinite_input_keeps_the_full_skip():
    cfg, sd, net, st = _skip_setup(ema=0.9)
    g = torch.Generator().manual_seed(9)
    x, t = torch.rand(2, 1, 32, 32, generator=g), torch.rand(2, 1, 64, 64, generator=g)
    x[0, 0, 3, 3] = float("nan")
    flat0, e0 = st.fp.flat.clone(), st.ema_flat.clone()
    st.step(x.cuda(), t.cuda())
    torch.cuda.synchronize()
    assert st.flag.item() == 1
    assert torch.equal(st.fp.flat, flat0) and torch.equal(st.ema_flat, e0) and st.opt.applied.item() == 0
    assert int(st.sticky.item()) == 1                            # check_finite() False


def test_clipping_sees_the_unscaled_gradient():
    cfg, sd, net, st = _skip_setup(clip=1e-6)
    g = torch.Generator().manual_seed(10)
    x, t = torch.rand(2, 1, 32, 32, generator=g), torch.rand(2, 1, 64, 64, generator=g)
    p = {k: v.clone().cuda().requires_grad_(True) for k, v in sd.items()}
    sc = torch.amp.GradScaler("cuda")
    with torch.autocast("cuda", torch.float16):
        lv = F.mse_loss(O.edsr_forward(p, x.cuda(), cfg), t.cuda())
    sc.scale(lv).backward()
    sc.unscale_(torch.optim.SGD(p.values(), lr=0.0))
    ref = torch.norm(torch.stack([v.grad.norm() for v in p.values()])).item()
    st.step(x.cuda(), t.cuda())
    torch.cuda.synchronize()
    norm = st.clip_state[0].item()
    assert abs(norm - ref) <= 0.01 * ref, (norm, ref)


# ---------------------------------------------------------------------------------------------------- 5. ModelPlain
class Args(dict):
    __getattr__ = dict.get


def edsr_args(tmp_path, amp=True):
    from dlib.utils import constants
    nt = constants.EDSR_LIIF
    netG = {'net_type': nt, f'{nt}_in_chans': 1, f'{nt}_n_resblocks': 2, f'{nt}_n_feats': 64, f'{nt}_upscale': 2,
            f'{nt}_img_range': 1.0}
    train = {'l1': True, 'G_optimizer_type': 'adam', 'G_optimizer_lr': 2e-4, 'G_optimizer_wd': 0.0,
             'G_scheduler_type': 'MyStepLR', 'G_scheduler_step_size': 30, 'G_scheduler_gamma': 0.5,
             'G_scheduler_min_lr': 1e-4}
    return Args(netG=netG, train=train, is_train=True, amp=amp, outd=str(tmp_path), method=nt)


def _run_model(tmp_path, graph, steps=3):
    from dlib.models.select_model import define_model
    os.environ["SRHIP_TRAIN_GRAPH"] = "1" if graph else "0"
    try:
        model = define_model(edsr_args(tmp_path))
        cfg = O.edsr_config(upscale=2, n_feats=64, n_resblocks=2)
        model.netG.load_state_dict(O.edsr_init_state_dict(cfg, seed=12), strict=True)
        model.init_train()
        assert model.step_fn.amp
        g = torch.Generator().manual_seed(13)
        for i in range(steps):
            model.feed_data({'l_im': torch.rand(2, 1, 32, 32, generator=g), 'h_im': torch.rand(2, 1, 64, 64, generator=g)})
            model.optimize_parameters(0, i)
        torch.cuda.synchronize()
        return {k: v.detach().cpu().clone() for k, v in model.netG.state_dict().items()}, model
    finally:
        os.environ.pop("SRHIP_TRAIN_GRAPH", None)


def test_model_plain_edsr_amp_graph_equals_eager(tmp_path):
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
from dlib.models.network_edsr_liif import EDSR_LIIF
from srhip.train import Optimizer, TrainStep
dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{sys.argv[2]}", rank=0, world_size=1,
                        device_id=torch.device("cuda", 0))
cfg = O.edsr_config(upscale=2, n_feats=64, n_resblocks=2)
sd = O.edsr_init_state_dict(cfg, seed=14)
gen = torch.Generator().manual_seed(15)
batches = [(torch.rand(2, 1, 32, 32, generator=gen).cuda(), torch.rand(2, 1, 64, 64, generator=gen).cuda()) for _ in range(2)]
batches.append((batches[0][0], torch.full((2, 1, 64, 64), 1e4, device="cuda")))      # an overflowing step
out = {}
for mode in ("plain", "ddp"):
    os.environ["SRHIP_FORCE_DDP"] = "1" if mode == "ddp" else "0"
    net = EDSR_LIIF(scale=2, n_resblocks=2, n_feats=64)
    net.load_state_dict(sd, strict=True)
    net = net.cuda()
    net.amp = True
    ts = TrainStep(net, [("l2", 1.0)], process_group=dist.group.WORLD if mode == "ddp" else None, world_size=1, amp=True)
    ts.opt = Optimizer(ts.fp, "adam", lr=1e-3)
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
    """SRHIP_FORCE_DDP=1 with a one-rank nccl group: the amp steps (one of them overflowing: the flag goes through the
    MAX-reduce) equal the plain ones bit for bit."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = tmp_path / "ddp_amp_worker.py"
    script.write_text(DDP_WORKER)
    p = subprocess.run([sys.executable, str(script), ROOT, str(port)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert p.returncode == 0 and "ddp amp ok" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]


def test_vdsr_amp_training_still_raises(tmp_path):
    from dlib.models.select_model import define_model
    from dlib.utils import constants
    nt = constants.VDSR
    a = edsr_args(tmp_path)
    a['netG'] = {'net_type': nt, f'{nt}_in_chans': 1, f'{nt}_upscale': 2}
    a['method'] = nt
    model = define_model(a)
    model.init_train()
    model.feed_data({'l_im': torch.rand(2, 1, 16, 16), 'h_im': torch.rand(2, 1, 32, 32)})
    with pytest.raises(NotImplementedError, match="EDSR_LIIF"):
        model.optimize_parameters(0, 0)
