"""The multi-image training losses of MSLapSRN / ProSR / SRFBN with every MasterLoss term (srhip/train.py:
TrainStep.multiscale_loss_and_grad) and the one-launch target pyramid (csrc/resize.hip:
srhip_resize_bicubic_ac_pyramid), against the three rules of the reference's trainer (model_plain.py:202-314) composed
HERE from the oracle's single-image MasterLoss, in float64.

Gates: the loss kernels are held to the gates of their single-image tests (tests/test_gpu_kernels.py::test_losses: L1 / L2
value and gradient 1e-6 of the largest entry, SSIM 1e-4 / 2e-4, the L2 + 5 SSIM sum 1e-4 / 2e-4;
tests/test_gpu_edsr_api.py: Charbonnier and the stencil terms 2e-6 x max(1, |ref|), the sparsity value 1e-6); the fused
steps to the form of tests/test_gpu_mslapsrn.py::test_fused_train_step_x8_vs_oracle (per parameter, the max-abs error
against the float64 oracle relative to the gradient's maximum, <= max(5e-5, 3 x what the float32 oracle gets); the loss
against the float32 oracle's at 1e-4 relative, the SSIM value gate)."""
import ctypes
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import sr_oracle as O  # noqa: E402
from test_gpu_kernels import check, relerr  # noqa: E402  (the gates' own helper)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
README_LOSS = [("l2", 1.0), ("ssim", 5.0, 19)]


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def resized(target, size):
    """the level target of loss_prosr / loss_mslaprs (model_plain.py:257-264,298-305), in the dtype of ``target``"""
    return torch.clamp(F.interpolate(target, size=tuple(size), mode="bicubic", align_corners=True), 0.0, 1.0)


def ms_rule(outs, target, terms, weight=None, params=None):
    """loss_mslaprs / loss_prosr / loss_srfbn(use_cl): self.loss_fn (the WHOLE MasterLoss, the parameter-space sparsity term
    included, as the reference adds it at every call) of every image against the target brought to its size, summed and
    divided by the number of images.  outs[0] is the network's output."""
    img_terms = [t for t in terms if t[0] != "w_sparsity"]
    total = 0.0
    for o in outs:
        tg = target if o.shape[-2:] == target.shape[-2:] else resized(target, o.shape[-2:])
        if img_terms:
            total = total + O.master_loss(o, tg, img_terms, weight)[0]
        for t in terms:
            if t[0] == "w_sparsity":
                total = total + O.loss_weights_sparsity(params, t[1])
    return total / float(len(outs))


# ------------------------------------------------------------------ 1. the pyramid kernel
def level_sets(H, W):
    return [[(H // 2, W // 2), (H // 4, W // 4)], [(H // 2, W // 2)], [(17, 23)], [(1, 1)]]


@pytest.mark.parametrize("B,H,W", [(2, 32, 32), (3, 40, 56), (8, 512, 512)])
def test_pyramid_kernel_vs_torch_float64(B, H, W):
    """One launch per level set against F.interpolate(bicubic, align_corners=True) + clamp on the CPU in float64.  Bound:
    twice the distance torch's own float32 CPU result keeps from that float64 result on the same input, plus 2^-23."""
    from srhip import ops
    gen = torch.Generator().manual_seed(1000 * B + H)
    x = torch.rand(B, 1, H, W, generator=gen) * 1.2 - 0.1
    xd = x.cuda()
    for shapes in level_sets(H, W):
        outs = ops.resize_bicubic_ac_pyramid(xd, shapes)
        again = ops.resize_bicubic_ac_pyramid(xd, shapes)
        assert len(outs) == len(shapes)
        for s, o, o2 in zip(shapes, outs, again):
            assert tuple(o.shape) == (B, 1) + tuple(s) and o.data_ptr() != o2.data_ptr()
            assert torch.equal(o, o2), "not bit-identical on a second run"
            raw64 = F.interpolate(x.double(), size=s, mode="bicubic", align_corners=True)
            r64 = raw64.clamp(0.0, 1.0)
            r32 = resized(x, s)
            if s != (1, 1):
                assert int((raw64 < 0).sum()) >= 1 and int((raw64 > 1).sum()) >= 1, "the clamp is not exercised"
            d_torch = (r32.double() - r64).abs().max().item()
            d_ours = (o.cpu().double() - r64).abs().max().item()
            print(f"  {B}x{H}x{W} -> {s}: torch float32 vs float64 {d_torch:.3e}, libsrhip vs float64 {d_ours:.3e}")
            assert d_ours <= 2.0 * d_torch + 2.0 ** -23, \
                f"{(B, H, W)} -> {s}: libsrhip {d_ours:.3e} from float64, torch's float32 kernel {d_torch:.3e}"
            assert float(o.min()) >= 0.0 and float(o.max()) <= 1.0
    # without the clamp, and on [B, H, W] input
    o = ops.resize_bicubic_ac_pyramid(xd[:, 0].contiguous(), [(H // 2, W // 2)], clamp=False)[0]
    raw64 = F.interpolate(x.double(), size=(H // 2, W // 2), mode="bicubic", align_corners=True)[:, 0]
    raw32 = F.interpolate(x, size=(H // 2, W // 2), mode="bicubic", align_corners=True)[:, 0]
    assert (o.cpu().double() - raw64).abs().max().item() <= 2.0 * (raw32.double() - raw64).abs().max().item() + 2.0 ** -23
    assert float(o.min()) < 0.0 and float(o.max()) > 1.0


def test_pyramid_same_size_levels_make_no_launch_and_overlap_is_refused(monkeypatch):
    from srhip import ops
    x = torch.rand(2, 1, 16, 24).cuda()
    calls = []
    monkeypatch.setattr(ops, "call", lambda name, *a, _f=ops.call: (calls.append(name), _f(name, *a))[1])
    outs = ops.resize_bicubic_ac_pyramid(x, [(16, 24), (16, 24)])
    assert calls == [] and all(o is x for o in outs)            # SRFBN: every image has the target's size
    outs = ops.resize_bicubic_ac_pyramid(x, [(16, 24), (8, 12), (4, 6)])
    assert calls == ["srhip_resize_bicubic_ac_pyramid"] and outs[0] is x     # the two resized levels: ONE launch
    # a level inside the source, two levels on top of each other
    buf = torch.zeros(2 * 16 * 24 + 2 * 8 * 12, device="cuda")
    src = buf[:2 * 16 * 24].view(2, 1, 16, 24)
    inside = buf[2 * 8 * 12:2 * 8 * 12 * 2].view(2, 1, 8, 12)
    with pytest.raises(ops.SrhipError, match="overlaps the source"):
        ops.resize_bicubic_ac_pyramid(src, [(8, 12)], out=[inside])
    lvl = torch.zeros(2, 1, 8, 12, device="cuda")
    with pytest.raises(ops.SrhipError, match="overlap"):
        ops.resize_bicubic_ac_pyramid(x, [(8, 12), (8, 12)], out=[lvl, lvl])
    nine = (ops._PyrLevel * 9)()
    with pytest.raises(ops.SrhipError, match="9 levels"):       # more than one launch takes: refused before anything is read
        ops.call("srhip_resize_bicubic_ac_pyramid", x.data_ptr(), 2, 16, 24, ctypes.addressof(nine), 9, 1, None)


# ------------------------------------------------------------------ 2. loss and gradient, kernel level
def image_sets():
    """(name, B, target (H, W), sizes of [output] + intermediate images)"""
    return [("mslapsrn_x8_p8", 2, (64, 64), [(64, 64), (16, 16), (32, 32)]),
            ("mslapsrn_x8_p16", 2, (128, 128), [(128, 128), (32, 32), (64, 64)]),
            ("prosr_x4_p8", 2, (32, 32), [(32, 32), (16, 16)]),
            ("srfbn_4passes", 2, (24, 40), [(24, 40)] * 4)]


TERM_SETS = {
    "l1": [("l1", 1.0)],
    "l2": [("l2", 1.0)],
    "readme": README_LOSS,
    "l1_ssim11": [("l1", 1.0), ("ssim", 1.0, 11)],
    "charbonnier": [("charbonnier", 0.7, 1e-3)],
    "lv3_l2": [("lv", 1.0, 2, 3)],
    "l1_w_sparsity": [("l1", 1.0), ("w_sparsity", 1e-4)],
}


def tiny_train_step(terms):
    """a TrainStep over a real (small) network: the loss layer under test needs its term list, value buffer and -- for the
    sparsity term -- its flat parameters"""
    from dlib.models.network_mslapsr import MSLapSRN
    from srhip.train import TrainStep
    net = MSLapSRN(upscale=2, in_chans=1)
    net.load_state_dict(O.mslapsrn_init_state_dict(2, seed=3), strict=True)
    return TrainStep(net.cuda().train(), terms)


def near(target64, sizes, gen):
    """outputs near the (float64) level targets: 0.02 .. 0.12 away, either side -- |y - t| is never within rounding of 0,
    where the sign of an L1 gradient would be decided by the last bit of the resized target"""
    outs = []
    for s in sizes:
        tg = target64 if tuple(s) == tuple(target64.shape[-2:]) else resized(target64, s)
        sign = torch.where(torch.rand(tg.shape, generator=gen) < 0.5, -1.0, 1.0)
        outs.append((tg + sign * (0.02 + 0.1 * torch.rand(tg.shape, generator=gen))).float())
    return outs


@pytest.mark.parametrize("tname", list(TERM_SETS))
@pytest.mark.parametrize("iset", image_sets(), ids=lambda s: s[0])
def test_multiscale_loss_and_gradient_vs_float64_rule(iset, tname):
    name, B, hw, sizes = iset
    terms = TERM_SETS[tname]
    ts = tiny_train_step(terms)
    gen = torch.Generator().manual_seed(len(name) * 131 + len(tname))
    target = torch.rand(B, 1, *hw, generator=gen)
    outs = near(target.double(), sizes, gen)
    dev = [o.cuda() for o in outs]
    dy, d_inter = ts.multiscale_loss_and_grad(dev[0], dev[1:], target.cuda())
    torch.cuda.synchronize()
    got_d = [dy] + list(d_inter)
    vals = ts.loss_buf[1:].cpu().double()
    o64 = [o.double().requires_grad_(True) for o in outs]
    params = [ts.fp.flat.detach().cpu().double()]
    ref = ms_rule(o64, target.double(), terms, params=params)
    ref.backward()
    ref_parts = []
    for t in terms:         # the per-term values (loss_buf[1 + i]): the same rule with that term alone
        with torch.no_grad():
            ref_parts.append(ms_rule([o.detach() for o in o64], target.double(), [t], params=params))
    total = vals.sum().reshape(1)
    kinds = {t[0] for t in terms}
    if "ssim" in kinds:
        vgate, ggate = 1e-4, 2e-4
    elif kinds <= {"l1", "l2", "w_sparsity"}:
        vgate, ggate = 1e-6, 1e-6
    else:
        vgate = ggate = None                # Charbonnier / stencil: 2e-6 x max(1, |ref|), the form of their own test
    print(f"  {name} {tname}: value {total.item():.8f} vs {ref.item():.8f}; gradient rel. errors "
          f"{[f'{relerr(g, o.grad):.2e}' for g, o in zip(got_d, o64)]}")
    if vgate is not None:
        check(total, ref.detach().reshape(1), vgate, f"{name} {tname} value")
        for j, (g, o) in enumerate(zip(got_d, o64)):
            assert g.shape == outs[j].shape
            check(g, o.grad, ggate, f"{name} {tname} dy[{j}] {tuple(o.shape)}")
    else:
        assert abs(total.item() - ref.item()) <= 2e-6 * max(1.0, abs(ref.item())), (total.item(), ref.item())
        for j, (g, o) in enumerate(zip(got_d, o64)):
            err = (g.cpu().double() - o.grad).abs().max().item()
            assert err <= 2e-6 * max(1.0, o.grad.abs().max().item()), (j, err)
    for i, t in enumerate(terms):
        r = ref_parts[i].item()
        if t[0] == "ssim":
            assert abs(vals[i].item() - r) <= 1e-4 * abs(r), (t, vals[i].item(), r)
        elif t[0] in ("l1", "l2"):
            assert abs(vals[i].item() - r) <= 1e-6 * abs(r), (t, vals[i].item(), r)
        elif t[0] == "w_sparsity":
            # ONCE with its full lambda: lam * sum|w| -- not n times, not lam / n
            full = 1e-4 * params[0].abs().sum().item()
            assert abs(r - full) <= 1e-12 * full
            assert abs(vals[i].item() - full) <= 1e-6 * max(1.0, full), (vals[i].item(), full)


def test_multiscale_buffers_persist_and_match_the_single_image_kernels():
    """The second call allocates nothing new (same gradient / target / workspace buffers), and an image of the multi-image
    path carries exactly what the single-image kernels give for lam / n on that image and its level target."""
    from srhip import ops
    ts = tiny_train_step(README_LOSS)
    gen = torch.Generator().manual_seed(5)
    target = torch.rand(2, 1, 64, 64, generator=gen).cuda()
    outs = [o.cuda() for o in near(target.cpu().double(), [(64, 64), (16, 16), (32, 32)], gen)]
    dy, di = ts.multiscale_loss_and_grad(outs[0], outs[1:], target)
    first = [dy.clone()] + [d.clone() for d in di]
    ptrs = [t.data_ptr() for t in ts._ms["dy"]] + [t.data_ptr() for t in ts._ms["tgt"] if t is not None] \
        + [t.data_ptr() for t in ts._ms["ssim_ws"]]
    assert ts._ms["tgt"][0] is None and [tuple(t.shape[-2:]) for t in ts._ms["tgt"][1:]] == [(16, 16), (32, 32)]
    assert [w.numel() for w in ts._ms["ssim_ws"]] == [ops.lib.srhip_ssim_loss_ws(2, *o.shape[-2:]) for o in outs]
    dy, di = ts.multiscale_loss_and_grad(outs[0], outs[1:], target)
    assert ptrs == [t.data_ptr() for t in ts._ms["dy"]] + [t.data_ptr() for t in ts._ms["tgt"] if t is not None] \
        + [t.data_ptr() for t in ts._ms["ssim_ws"]]
    for a, b in zip(first, [dy] + list(di)):
        assert torch.equal(a, b)
    tgts = ops.resize_bicubic_ac_pyramid(target, [o.shape[-2:] for o in outs])
    for j, o in enumerate(outs):
        g = torch.empty_like(o)
        v = ops.loss_l1l2(o, tgts[j], 1, 1.0 / 3.0, None, g)
        ops.ssim_loss(o, tgts[j], 19, 5.0 / 3.0, g, v, grad_accum=True, loss_accum=True)
        assert torch.equal(g, first[j]), j
        assert abs(float(v) - float(ts._ms["parts"][j].sum())) <= 1e-6 * abs(float(v))


# ------------------------------------------------------------------ 3. one fused step per net, README loss
def _grad_check(ts, sd, o32, o64, tgt, names=None, slope_rule=False):
    """loss and every parameter gradient of the step ``ts`` just made, against the oracle outputs o32 / o64 (lists, the
    network's output FIRST) built on leaf dicts sd32 / sd64 = o32[1] / o64[1]"""
    (outs32, sd32), (outs64, sd64) = o32, o64
    loss32 = ms_rule(outs32, tgt, README_LOSS)
    loss32.backward()
    loss64 = ms_rule(outs64, tgt.double(), README_LOSS)
    loss64.backward()
    got = ts.loss_values()[0]
    print(f"  loss {got:.8f}, float32 oracle {loss32.item():.8f}, float64 oracle {loss64.item():.8f}")
    assert abs(got - loss32.item()) <= 1e-4 * max(1.0, abs(loss32.item())), (got, loss32.item())
    worst = ("", 0.0, 0.0)
    smax = max([abs(sd64[k].grad.item()) for k in ts.fp.names if sd64[k].grad is not None and sd64[k].grad.numel() == 1]
               + [0.0])
    for k in ts.fp.names:
        ref = sd64[k].grad
        gh = ts.fp.gviews[k].detach().cpu().double()
        if ref is None:                         # a parameter without a gradient path (ProSR: the other scales' init convs)
            assert float(gh.abs().max()) == 0.0, k
            continue
        if slope_rule and ref.numel() == 1:
            # a PReLU slope: one cancelling sum over whole feature maps (tests/test_gpu_tape_nets.py, same rule)
            assert abs(gh.item() - ref.item()) <= 2e-4 * abs(ref.item()) + 1e-3 * smax, (k, gh.item(), ref.item(), smax)
            continue
        den = ref.abs().max().item() + 1e-12
        e = (gh - ref).abs().max().item() / den
        e32 = (sd32[k].grad.double() - ref).abs().max().item() / den
        if e > worst[1]:
            worst = (k, e, e32)
        assert e <= max(5e-5, 3.0 * e32), (k, e, e32)
    print("  worst gradient vs the fp64 oracle (name, libsrhip, fp32 oracle)", worst)


def _adam_check(ts, x, tgt):
    """one real Adam step from the same state (the lr-0 step moved nothing): the parameters against the oracle's float64
    Adam update on the step's own gradient"""
    from srhip.train import Optimizer
    p0 = {k: ts.fp.flat[ts.fp.offsets[k]:ts.fp.offsets[k] + ts.fp.gviews[k].numel()].view_as(ts.fp.gviews[k]).cpu().clone()
          for k in ts.fp.names}
    ts.opt = Optimizer(ts.fp, "adam", lr=2e-4)
    ts.step(x.cuda(), tgt.cuda())
    torch.cuda.synchronize()
    for k in ts.fp.names:
        g = ts.fp.gviews[k].detach().cpu().double()
        po = p0[k].double()
        O.adam_step(po, g, torch.zeros_like(po), torch.zeros_like(po), 1, 2e-4)
        now = ts.fp.flat[ts.fp.offsets[k]:ts.fp.offsets[k] + g.numel()].view_as(g).cpu().double()
        assert (now - po).abs().max().item() <= 2e-6, k
        if float(g.abs().max()) > 0:
            assert not torch.equal(now.float(), p0[k]), k       # and it moved


def _sgd0(ts):
    from srhip.train import Optimizer
    ts.opt = Optimizer(ts.fp, "sgd", lr=0.0, momentum=0.0, nesterov=False, wd=0.0)    # lr 0: the gradients stay readable


@pytest.mark.parametrize("scale", [2, 8])
def test_fused_step_mslapsrn_readme_loss_vs_oracle(scale):
    from dlib.models.network_mslapsr import MSLapSRN
    from srhip.train import TrainStep
    sd = O.mslapsrn_init_state_dict(scale, seed=5)
    net = MSLapSRN(upscale=scale, in_chans=1)
    net.load_state_dict(sd, strict=True)
    net = net.cuda().train()
    gen = torch.Generator().manual_seed(11)
    # x8 at the size of test_gpu_mslapsrn.py's fused step (32 -> 256): the entry-wise gate needs maps on which ONE LeakyReLU
    # decision that flips under f32 rounding is one pixel of tens of thousands (that file's header; at 8 x 8 -> 64 x 64 a
    # single bias gradient sat at 8.3e-5 with the float32 oracle at 4e-7).  Levels smaller than the 19-pixel SSIM window are
    # covered at kernel level above (16 x 16).
    p, B = (32, 1) if scale == 8 else (24, 2)
    x, tgt = torch.rand(B, 1, p, p, generator=gen), torch.rand(B, 1, p * scale, p * scale, generator=gen)
    ts = TrainStep(net, README_LOSS)
    _sgd0(ts)
    ts.step(x.cuda(), tgt.cuda())
    torch.cuda.synchronize()
    sd32 = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    y32, i32 = O.mslapsrn_forward(sd32, x, scale)
    sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    y64, i64 = O.mslapsrn_forward(sd64, x.double(), scale)
    assert len(i64) == int(math.log2(scale)) - 1
    _grad_check(ts, sd, ([y32] + list(i32), sd32), ([y64] + list(i64), sd64), tgt)
    _adam_check(ts, x, tgt)


def test_fused_step_prosr_readme_loss_vs_oracle():
    """the registry's ProSR (160 features, growth 40, the x4 level configuration) at an 8 x 8 patch"""
    from dlib.models.network_prosr import ProSR
    from srhip.train import TrainStep
    scale = 4
    cfg = O.prosr_config(upscale=scale)
    sd = O.prosr_init_state_dict(cfg, seed=7, bias_std=0.05)
    net = ProSR(upscale=scale, in_chans=1, level_config=cfg["level_config"])
    net.load_state_dict(sd, strict=True)
    net = net.cuda().train()
    gen = torch.Generator().manual_seed(12)
    x, tgt = torch.rand(2, 1, 8, 8, generator=gen), torch.rand(2, 1, 32, 32, generator=gen)
    ts = TrainStep(net, README_LOSS)
    _sgd0(ts)
    ts.step(x.cuda(), tgt.cuda())
    torch.cuda.synchronize()
    sd32 = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    o32 = O.prosr_forward(sd32, x, cfg)
    sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    o64 = O.prosr_forward(sd64, x.double(), cfg)
    assert len(o64) == 2
    _grad_check(ts, sd, (o32[::-1], sd32), (o64[::-1], sd64), tgt)
    _adam_check(ts, x, tgt)


def test_fused_step_srfbn_readme_loss_vs_oracle():
    """SRFBN's curriculum rule (use_cl: every one of the 4 passes against the same target) at the registry's widths, PReLU
    slopes 1 (the entry-wise gate needs a network without slope decisions within rounding of 0:
    tests/test_gpu_tape_nets.py::test_default_width_train_step_vs_oracle documents the effect)"""
    from dlib.models.network_srfbn import SRFBN
    from srhip.train import TrainStep
    scale = 4
    sd = O.srfbn_init_state_dict(scale, 1, seed=12)
    for k in sd:
        if k.endswith("act.weight") or (k.endswith(".1.weight") and sd[k].numel() == 1):
            sd[k] = torch.ones(1)
    net = SRFBN(upscale=scale, in_chans=1)
    net.load_state_dict(sd, strict=True)
    net = net.cuda().train()
    torch.manual_seed(3)
    x, tgt = torch.rand(2, 1, 16, 16), torch.rand(2, 1, 64, 64)
    ts = TrainStep(net, README_LOSS)
    _sgd0(ts)
    ts.step(x.cuda(), tgt.cuda())
    torch.cuda.synchronize()
    fixed = ("sub_mean", "add_mean")
    sd32 = {k: (v.clone().requires_grad_(True) if not k.startswith(fixed) else v.clone()) for k, v in sd.items()}
    o32 = O.srfbn_forward(sd32, x, scale, 4, 6)
    sd64 = {k: (v.double().requires_grad_(True) if not k.startswith(fixed) else v.double()) for k, v in sd.items()}
    o64 = O.srfbn_forward(sd64, x.double(), scale, 4, 6)
    assert len(o64) == 4
    _grad_check(ts, sd, (o32[::-1], sd32), (o64[::-1], sd64), tgt, slope_rule=True)
    _adam_check(ts, x, tgt)


# ------------------------------------------------------------------ 4. replay
def test_step_graph_mslapsrn_x8_readme_loss_replays_bit_identically():
    """eager, capture, replay on a new batch each step; every step equals an eager step of a second TrainStep that starts
    from the same parameters and optimizer state, bit for bit (pattern of tests/test_gpu_bench_shapes.py)."""
    from dlib.models.network_mslapsr import MSLapSRN
    from srhip import ops
    from srhip.train import TrainStep
    from test_gpu_bench_shapes import load_state, snapshot, graph_state

    def make():
        net = MSLapSRN(upscale=8, in_chans=1)
        net.load_state_dict(O.mslapsrn_init_state_dict(8, seed=5), strict=True)
        return TrainStep(net.cuda().train(), README_LOSS)
    ts, twin = make(), make()
    graph = None
    for step in (1, 2, 3):
        gen = torch.Generator().manual_seed(40 + step)
        x, tgt = torch.rand(2, 1, 16, 16, generator=gen).cuda(), torch.rand(2, 1, 128, 128, generator=gen).cuda()
        before = snapshot(ts)
        ts.step_graph(x, tgt)
        torch.cuda.synchronize()
        graph = graph_state(ts, step, graph)
        load_state(twin, *before)
        twin.step(x, tgt)
        torch.cuda.synchronize()
        assert math.isfinite(ts.loss_values()[0])
        assert torch.equal(twin.loss_buf, ts.loss_buf), step
        assert torch.equal(twin.fp.grad, ts.fp.grad), step
        assert torch.equal(twin.fp.flat, ts.fp.flat) and torch.equal(twin.opt.m, ts.opt.m) \
            and torch.equal(twin.opt.v, ts.opt.v), step
    assert int(ts.opt.applied.item()) == 3
    assert ops.realloc_generation() == ts._graph["gen"]


# ------------------------------------------------------------------ 5. per-pixel weights
def test_srfbn_per_pixel_weights_vs_float64_rule_and_mslapsrn_refusal():
    ts = tiny_train_step([("l1", 1.0)])
    gen = torch.Generator().manual_seed(9)
    target = torch.rand(2, 1, 24, 40, generator=gen)
    weight = torch.rand(2, 1, 24, 40, generator=gen) * 3        # mean 1.5: the weighted loss is not the plain one
    outs = near(target.double(), [(24, 40)] * 4, gen)
    dev = [o.cuda() for o in outs]
    dy, di = ts.multiscale_loss_and_grad(dev[0], dev[1:], target.cuda(), weight.cuda())
    o64 = [o.double().requires_grad_(True) for o in outs]
    ref = ms_rule(o64, target.double(), [("l1", 1.0)], weight=weight.double())
    ref.backward()
    check(ts.loss_buf[1:2], ref.detach().reshape(1), 1e-6, "weighted l1 value")
    for j, (g, o) in enumerate(zip([dy] + list(di), o64)):
        check(g, o.grad, 1e-6, f"weighted l1 dy[{j}]")
    # and it IS the weighted rule
    plain = ms_rule([o.detach() for o in o64], target.double(), [("l1", 1.0)])
    assert abs(plain.item() - ref.item()) > 1e-3
    # smaller images than the weight map: the reference itself fails on the shape mismatch
    small = near(target.double(), [(24, 40), (12, 20)], gen)
    with pytest.raises(NotImplementedError, match="shape mismatch"):
        ts.multiscale_loss_and_grad(small[0].cuda(), [small[1].cuda()], target.cuda(), weight.cuda())


def test_fused_step_refuses_per_pixel_weights_for_mslapsrn_and_takes_them_for_srfbn():
    from dlib.models.network_mslapsr import MSLapSRN
    from dlib.models.network_srfbn import SRFBN
    from srhip.train import TrainStep
    net = MSLapSRN(upscale=4, in_chans=1)
    net.load_state_dict(O.mslapsrn_init_state_dict(4, seed=5), strict=True)
    ts = TrainStep(net.cuda().train(), [("l1", 1.0)])
    x, tgt, w = torch.rand(2, 1, 8, 8).cuda(), torch.rand(2, 1, 32, 32).cuda(), torch.rand(2, 1, 32, 32).cuda()
    with pytest.raises(NotImplementedError, match="reference itself fails there on the shape mismatch"):
        ts.step(x, tgt, weight=w)
    cfg = dict(num_features=16, num_steps=3, num_groups=3)
    sd = O.srfbn_init_state_dict(2, 1, cfg["num_features"], cfg["num_groups"], seed=4)
    net = SRFBN(upscale=2, in_chans=1, **cfg)
    net.load_state_dict(sd, strict=True)
    ts = TrainStep(net.cuda().train(), [("l1", 1.0)])
    _sgd0(ts)
    x, tgt, w = torch.rand(2, 1, 12, 12), torch.rand(2, 1, 24, 24), torch.rand(2, 1, 24, 24) * 2
    ts.step(x.cuda(), tgt.cuda(), weight=w.cuda())
    sd64 = {k: (v.double().requires_grad_(True) if not k.startswith(("sub_mean", "add_mean")) else v.double())
            for k, v in sd.items()}
    o64 = O.srfbn_forward(sd64, x.double(), 2, 3, 3)
    ref = ms_rule(o64[::-1], tgt.double(), [("l1", 1.0)], weight=w.double())
    assert abs(ts.loss_values()[0] - ref.item()) <= 2e-6 * max(1.0, abs(ref.item()))


# ------------------------------------------------------------------ 6. CLI
@pytest.mark.parametrize("net_type,method,scale", [("MSLapSRN", "MSLAPSR", 8), ("SRFBN", "SRFBN", 4)])
def test_main_cli_trains_with_the_readme_loss(tmp_path, net_type, method, scale):
    """`main.py --net_type MSLapSRN | SRFBN ... --l1 False --l2 True --ssim True --ssim_lambda 5.0 --ssim_window_s 19`: two
    iterations to a finite loss (pattern of test_main_cli_trains_drrn_under_amp)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "sr-caco-2_amd", "main.py"), "--net_type", net_type, "--method", method,
                        "--task", "super-resolution", "--scale", str(scale), "--n_channels", "1", "--h_size", "64",
                        "--batch_size", "2", "--max_iters", "2", "--l1", "False", "--l2", "True", "--ssim", "True",
                        "--ssim_lambda", "5.0", "--ssim_window_s", "19", "--outd", str(tmp_path)],
                       capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    losses = [float(l.split("G_loss")[1].split()[0]) for l in p.stdout.splitlines() if "G_loss" in l]
    assert len(losses) == 1 and math.isfinite(losses[0]), p.stdout[-2000:]
