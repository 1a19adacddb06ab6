"""GPU parity at the shapes bench.py times: B = 8 patches, several optimisation steps through TrainStep.step_graph (step 1
eager, step 2 captured and replayed, step 3 replayed), as the timed steps of the benchmark run.

EDSR-baseline x8 / x4 / x2 (16 ResBlocks x 64 features, LR (512/s)^2 -> HR 512^2, Adam): every step against the fp32 and
fp64 oracles, Adam's update and moments against the oracle's Adam carried from step 1, and every step bit-identical to an
eager step of a second TrainStep loaded with the same parameters and optimizer state.  SwinIR README workload (DropPath
0.1, SGD-Nesterov with MyStepLR): DropPath masks are drawn on the device inside the graph, so the replayed steps are held
to an eager step of a second TrainStep under the same per-step seed, and the SGD update to the oracle's.

Gates are those of test_gpu_fullsize.py (none looser).  The fp64 oracles run on the GPU through PyTorch's own float64
convolutions (im2col + rocBLAS dgemm: none of this project's kernels), the fp32 oracle -- the reference's own arithmetic --
on the host cores.  Every test prints its worst errors per step, the arm it took and its wall time (-s)."""
import os
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import sr_oracle as O  # noqa: E402
from test_gpu_fullsize import GRAD_GATE, psnr_gap, readme_net, synth, worst_grad, worst_l2  # noqa: E402

BATCH = 8                 # bench.py --batch (README --batch_size 8)
STEPS = 3                 # eager, capture + replay, replay


def cpu_threads():
    """the fp32 oracle's host threads: the process's budget (OMP_NUM_THREADS, else torch's own setting)."""
    env = os.environ.get("OMP_NUM_THREADS", "")
    n = int(env) if env.isdigit() and int(env) > 0 else torch.get_num_threads()
    return max(1, min(32, n))


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.set_num_threads(cpu_threads())


def views(flat, fp):
    """{name: view of a flat buffer laid out as fp.flat}"""
    return {k: flat[fp.offsets[k]:fp.offsets[k] + fp.gviews[k].numel()].view_as(fp.gviews[k]) for k in fp.names}


def load_state(dst, flat, m, v, applied, step_count, sched_count):
    """a TrainStep's parameters and optimizer state set to the given ones (device copies, no host round trip)."""
    dst.fp.flat.copy_(flat)
    dst.opt.m.copy_(m)
    if v is not None:
        dst.opt.v.copy_(v)
    dst.opt.applied.copy_(applied)
    dst.opt.step_count, dst.opt.sched_count = step_count, sched_count
    dst.net.weights_changed()


def snapshot(ts):
    o = ts.opt
    return (ts.fp.flat.clone(), o.m.clone(), None if o.v is None else o.v.clone(), o.applied.clone(), o.step_count,
            o.sched_count)


def graph_state(ts, step, seen):
    """step 1 runs eagerly and leaves no graph; step 2 captures; step 3 replays THAT graph (a re-capture -- a persistent
    buffer replaced in between -- would make step 3 an eager step and the test would not cover a replay)."""
    from srhip import ops
    st = ts._graph
    if step == 1:
        assert st is not None and st["g"] is None
        return None
    assert st["g"] is not None and st["gen"] == ops.realloc_generation(), "no captured graph behind this step"
    if seen is not None:
        assert st["g"] is seen, "the step was re-captured instead of replayed"
    return st["g"]


def max_rel(a, ref):
    ref = ref.double()
    return ((a.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


# ------------------------------------------------------------------ EDSR
def edsr_arm(net, scale):
    """the engine's own choice for the bench shape: (fused one-launch ResBlocks, batched strip-form weight gradient)."""
    from srhip import ops
    eng = net.engine
    pix = BATCH * (512 // scale) ** 2
    fused = bool(eng.fuse_rb and not ops.lib.srhip_get_matmul_mode() and pix <= eng.fuse_rb_maxpix
                 and ops.resblock64_fusable(64))
    batched = bool(ops.bx3_for(64, 64) and eng.nb > 0)
    return fused, batched, pix, eng.fuse_rb_maxpix


@pytest.mark.parametrize("scale,loss", [(8, "l1"), (8, "l2ssim"), (4, "l1"), (2, "l1")])
def test_edsr_bench_shape_replayed_steps_vs_oracle(scale, loss, monkeypatch):
    """EDSR-baseline as bench.py --workload edsr_x{8,4,2} trains it: B = 8, LR (512/s)^2 -> HR 512^2, Adam lr 2e-4 wd 1e-4,
    three steps through step_graph on a new batch each step (a replay that read a stale input would show).

    Arms: x8 (8 x 64^2 = 32768 pixels <= fuse_rb_maxpix) runs the fused one-launch ResBlock in both directions; x4 / x2
    (8 x 128^2, 8 x 256^2) run the two-launch ResBlock.  Every scale runs the body's weight gradients as ONE batched
    strip-form contraction (k_tnb9s: image widths 64 / 128 / 256, multiples of 64; at these shapes slices cross image
    borders and hundreds of blocks hold exponent words for the second pass).  The arm is asserted from the engine's own
    decision and from the launches it made, so a moved threshold fails here instead of covering another arm.

    Per step: output MAE <= 1e-5 and PSNR gap <= 0.01 dB against the fp32 oracle at the parameters the step started
    from, the loss within 1e-5 relative; every gradient entry within GRAD_GATE of the fp64 oracle run under the HIP run's
    own ReLU decisions (or, where the reference's own fp32 result under those decisions is noisier than that, within 3x its
    distance: test_gpu_fullsize.py's SwinIR gate), tensor-wise relative L2 <= 1e-4 against the free-running fp64 oracle
    (likewise, or within 3x the fp32 oracle's own); parameters (2e-6 absolute) and Adam's m / v (1e-6 of the tensor's max) against the oracle's fp64 Adam on the HIP gradients, its state carried
    from step 1 (bias correction at t = 1, 2, 3: the device-side counter under replay); gradients, loss, parameters and
    moments bit-identical to one eager step of a second TrainStep loaded with the same parameters and optimizer state."""
    from dlib.models.network_edsr_liif import EDSR_LIIF
    from srhip import ops
    from srhip.train import Optimizer, TrainStep
    t_start = time.perf_counter()
    cfg = O.edsr_config(upscale=scale)
    sd0 = O.edsr_init_state_dict(cfg, seed=150 + scale)
    terms = [("l1", 1.0)] if loss == "l1" else [("l2", 1.0), ("ssim", 5.0, 19)]

    def make():
        net = EDSR_LIIF(scale=scale)
        net.load_state_dict(sd0, strict=True)
        net = net.cuda().train()
        ts = TrainStep(net, terms)
        ts.opt = Optimizer(ts.fp, "adam", lr=2e-4, wd=1e-4)
        return ts

    ts, twin = make(), make()
    net = ts.net
    fused, batched, pix, maxpix = edsr_arm(net, scale)
    print(f"\nEDSR x{scale} {loss} B={BATCH}: B*H*W = {pix}, fuse_rb_maxpix = {maxpix} -> "
          f"{'fused one-launch' if fused else 'two-launch'} ResBlock, batched strip-form weight gradient {batched}")
    assert fused == (scale == 8), "the ResBlock arm of this bench shape moved: re-point the test before relaxing it"
    assert batched

    calls = {"resblock64_fwd": 0, "resblock64_bwd": 0, "conv3x3_wgrad_batched": []}
    for name in ("resblock64_fwd", "resblock64_bwd"):
        def counted(*a, _f=getattr(ops, name), _n=name, **k):
            calls[_n] += 1
            return _f(*a, **k)
        monkeypatch.setattr(ops, name, counted)

    def batched_counted(items, _f=ops.conv3x3_wgrad_batched):
        calls["conv3x3_wgrad_batched"].append((len(items), tuple(items[0][1].shape)))
        return _f(items)
    monkeypatch.setattr(ops, "conv3x3_wgrad_batched", batched_counted)

    names = ts.fp.names
    m_ref = {k: torch.zeros(ts.fp.gviews[k].shape, dtype=torch.float64) for k in names}
    v_ref = {k: torch.zeros(ts.fp.gviews[k].shape, dtype=torch.float64) for k in names}
    graph = None
    for step in range(1, STEPS + 1):
        t_step = time.perf_counter()
        lr_img, hr_img = synth(BATCH, scale, seed=160 + 10 * scale + step)
        before = snapshot(ts)
        for k in calls:
            calls[k] = [] if k == "conv3x3_wgrad_batched" else 0
        ts.step_graph(lr_img.cuda(), hr_img.cuda())
        torch.cuda.synchronize()
        graph = graph_state(ts, step, graph)
        if step <= 2:       # the eager step and the capture made their launches through the Python entry points
            nb = cfg["n_resblocks"]
            assert calls["resblock64_fwd"] == (nb if fused else 0) and calls["resblock64_bwd"] == (nb if fused else 0), calls
            assert calls["conv3x3_wgrad_batched"] == [(2 * nb + 1, (BATCH, 512 // scale, 512 // scale, 64))], calls
        else:               # a replay makes none
            assert calls["resblock64_fwd"] == 0 and not calls["conv3x3_wgrad_batched"], calls
        y = net.engine.bufs.d["t.y"].detach().reshape(BATCH, 1, 512, 512).cpu()
        lv = ts.loss_values()
        loss_buf = ts.loss_buf.clone()
        grads = {k: v.detach().clone() for k, v in ts.fp.gviews.items()}
        gcpu = {k: v.cpu() for k, v in grads.items()}
        masks = [(net.engine.saved["blocks"][kb][1].permute(0, 3, 1, 2) > 0) for kb in range(cfg["n_resblocks"])]
        p_start = {k: v.detach().cpu().clone() for k, v in views(before[0], ts.fp).items()}

        # the fp32 oracle (the reference's arithmetic) at the parameters the step started from: output and loss
        with torch.no_grad():
            yo = O.edsr_forward(p_start, lr_img, cfg)
            tot, _ = O.master_loss(yo, hr_img, terms)
        mae = (y - yo).abs().mean().item()
        gap = psnr_gap(y, yo, hr_img, scale)
        del yo

        def oracle64(masks_=None):
            sd = {k: v.double().cuda().requires_grad_(True) for k, v in p_start.items()}
            yd = O.edsr_forward(sd, lr_img.double().cuda(), cfg, relu_masks=masks_)
            O.master_loss(yd, hr_img.double().cuda(), terms)[0].backward()
            return {k: v.grad.cpu() for k, v in sd.items()}

        g64 = oracle64()
        kl, el = worst_l2(gcpu, g64)
        eo_l2 = 0.0
        if el > 1e-4:
            # ReLU decisions within rounding of zero move whole pixels in or out of a sum; the same 3x rule as below, tensor-wise
            sd = {k: v.clone().requires_grad_(True) for k, v in p_start.items()}
            O.master_loss(O.edsr_forward(sd, lr_img, cfg), hr_img, terms)[0].backward()
            ko, eo_l2 = worst_l2({k: v.grad for k, v in sd.items()}, g64)
            print(f"  step {step}: the fp32 oracle's own worst tensor-wise L2 vs the free-running fp64 one: {ko} {eo_l2:.2e}")
            del sd
        del g64
        gm = {k: v.float() for k, v in oracle64(masks).items()}
        km, em = worst_grad(gcpu, gm)
        eo = 0.0
        if em > GRAD_GATE:
            # test_gpu_fullsize.py's gate for sums where fp32 itself is noisier than GRAD_GATE (here: 8 x 512^2 pixels):
            # no further from the exact value than 3x the reference's own fp32 result under the same ReLU decisions is
            sd = {k: v.clone().requires_grad_(True) for k, v in p_start.items()}
            O.master_loss(O.edsr_forward(sd, lr_img, cfg, relu_masks=[mk.cpu() for mk in masks]), hr_img,
                          terms)[0].backward()
            ko, eo = worst_grad({k: v.grad for k, v in sd.items()}, gm)
            print(f"  step {step}: the fp32 oracle's own worst entry vs fp64 (same ReLU decisions): {ko} {eo:.2e}")
            del sd
        del gm

        # Adam: the oracle's fp64 update on the HIP gradients, m / v carried from step 1
        wp = wm = wv = 0.0
        pv, mv, vv = views(ts.fp.flat, ts.fp), views(ts.opt.m, ts.fp), views(ts.opt.v, ts.fp)
        for k in names:
            po = p_start[k].double()
            O.adam_step(po, gcpu[k].double(), m_ref[k], v_ref[k], step, 2e-4, wd=1e-4)
            wp = max(wp, (pv[k].detach().cpu().double() - po).abs().max().item())
            wm = max(wm, max_rel(mv[k].cpu(), m_ref[k]))
            wv = max(wv, max_rel(vv[k].cpu(), v_ref[k]))

        # the same step, eagerly, on a second TrainStep holding the same parameters and optimizer state
        load_state(twin, *before)
        twin.step(lr_img.cuda(), hr_img.cuda())
        torch.cuda.synchronize()
        same = (torch.equal(twin.loss_buf, loss_buf) and all(torch.equal(twin.fp.gviews[k], grads[k]) for k in names)
                and torch.equal(twin.fp.flat, ts.fp.flat) and torch.equal(twin.opt.m, ts.opt.m)
                and torch.equal(twin.opt.v, ts.opt.v))
        print(f"  step {step} ({'eager' if step == 1 else 'captured + replayed' if step == 2 else 'replayed'}): "
              f"MAE {mae:.2e}, PSNR gap {gap:.2e} dB, loss {lv[0]:.6f} vs {tot.item():.6f}; worst grad entry vs fp64 "
              f"(HIP ReLU decisions) {km} {em:.2e}; worst L2 vs free fp64 {kl} {el:.2e}; Adam: param {wp:.2e}, "
              f"m {wm:.2e}, v {wv:.2e}; bit-identical to an eager step: {same}; {time.perf_counter() - t_step:.1f} s")
        assert mae <= 1e-5 and gap <= 0.01, (step, mae, gap)
        assert abs(lv[0] - tot.item()) <= 1e-5 * max(1.0, abs(tot.item())), (step, lv[0], tot.item())
        assert em <= max(GRAD_GATE, 3.0 * eo), (step, km, em, eo)
        assert el <= max(1e-4, 3.0 * eo_l2), (step, kl, el, eo_l2)
        assert wp <= 2e-6 and wm <= 1e-6 and wv <= 1e-6, (step, wp, wm, wv)
        assert same, f"step {step}: the step_graph step differs from an eager step on the same state"
    assert int(ts.opt.applied.item()) == STEPS
    print(f"  wall time {time.perf_counter() - t_start:.1f} s")


# ------------------------------------------------------------------ SwinIR
def test_swinir_readme_bench_shape_replayed_steps():
    """The headline workload as bench.py trains it: SwinIR README configuration, drop_path_rate 0.1, B = 8, LR 64^2 ->
    HR 512^2, L1, SGD-Nesterov 0.01 / 0.9 with MyStepLR (step 30, gamma 0.5, min 1e-4), three step_graph steps on a new
    batch each, re-seeded before every step as the trainer does.  Step 1 is gated against fp64 in test_gpu_fullsize.py;
    the DropPath masks of a replay are drawn inside the graph, so here:
    (a) every step's loss and gradients (and the update) are bit-identical to one eager step of a second TrainStep holding
        the same parameters, momentum and per-step seed;
    (b) parameters and momentum buffers after every step are within 2e-6 of the oracle's SGD-Nesterov on the HIP
        gradients, its momentum carried from step 1, at the learning rate of O.mysteplr;
    (c) with SRHIP_SWIN_SIDE_WGRAD=0 (the in-order weight gradients) step 1's gradients are bit-identical too."""
    from srhip.train import Optimizer, TrainStep
    t_start = time.perf_counter()
    cfg = O.swinir_config(drop_path_rate=0.1)
    sd0 = O.swinir_init_state_dict(cfg, seed=170)
    sched = {"type": "MyStepLR", "step_size": 30, "gamma": 0.5, "min_lr": 1e-4}

    def make():
        net = readme_net(0.1)
        net.load_state_dict(sd0, strict=True)
        net = net.cuda().train()
        ts = TrainStep(net, [("l1", 1.0)])
        ts.opt = Optimizer(ts.fp, "sgd", lr=0.01, momentum=0.9, nesterov=True, wd=0.0, scheduler=dict(sched))
        return ts

    ts, twin = make(), make()
    assert max(b.drop_prob for b in ts.net.swin_blocks()) > 0
    names = ts.fp.names
    buf_ref = {k: torch.zeros(ts.fp.gviews[k].shape, dtype=torch.float64) for k in names}
    graph, first = None, None
    print()
    for step in range(1, STEPS + 1):
        t_step = time.perf_counter()
        lr_img, hr_img = synth(BATCH, 8, seed=180 + step)
        lr_img, hr_img = lr_img.cuda(), hr_img.cuda()
        seed = 1234 + step
        before = snapshot(ts)
        lr_now = O.mysteplr(0.01, ts.opt.sched_count, sched["step_size"], sched["gamma"], sched["min_lr"])
        torch.manual_seed(seed)
        ts.step_graph(lr_img, hr_img)
        torch.cuda.synchronize()
        graph = graph_state(ts, step, graph)
        loss_buf = ts.loss_buf.clone()
        grads = {k: v.detach().clone() for k, v in ts.fp.gviews.items()}
        if step == 1:
            first = (before, seed, lr_img, hr_img, grads)
        # (b) the oracle's SGD-Nesterov on the HIP gradients
        pv, mv = views(ts.fp.flat, ts.fp), views(ts.opt.m, ts.fp)
        p_start = views(before[0], ts.fp)
        wp = wm = 0.0
        for k in names:
            po = p_start[k].detach().cpu().double()
            O.sgd_nesterov_step(po, grads[k].cpu().double(), buf_ref[k], step == 1, lr_now)
            wp = max(wp, (pv[k].detach().cpu().double() - po).abs().max().item())
            wm = max(wm, (mv[k].cpu().double() - buf_ref[k]).abs().max().item())
        # (a) the same step, eagerly, on the twin under the same seed
        load_state(twin, *before)
        torch.manual_seed(seed)
        twin.step(lr_img, hr_img)
        torch.cuda.synchronize()
        diff = [k for k in names if not torch.equal(twin.fp.gviews[k], grads[k])]
        same_loss = torch.equal(twin.loss_buf, loss_buf)
        same_state = torch.equal(twin.fp.flat, ts.fp.flat) and torch.equal(twin.opt.m, ts.opt.m)
        print(f"SwinIR README B={BATCH} step {step} ({'eager' if step == 1 else 'captured + replayed' if step == 2 else 'replayed'}): "
              f"loss {loss_buf[1].item():.6f}, lr {lr_now:g}; SGD-Nesterov vs oracle: param {wp:.2e}, momentum {wm:.2e}; "
              f"gradients differing from an eager step: {len(diff)}, loss {'same' if same_loss else 'differs'}; "
              f"{time.perf_counter() - t_step:.1f} s")
        assert same_loss and not diff and same_state, (step, diff[:4], same_loss, same_state)
        assert wp <= 2e-6 and wm <= 2e-6, (step, wp, wm)
    assert int(ts.opt.applied.item()) == STEPS and ts.opt.sched_count == STEPS
    # (c) step 1 with the weight gradients in order on one stream
    before, seed, lr_img, hr_img, grads = first
    old = os.environ.get("SRHIP_SWIN_SIDE_WGRAD")
    os.environ["SRHIP_SWIN_SIDE_WGRAD"] = "0"
    try:
        load_state(twin, *before)
        torch.manual_seed(seed)
        twin.step(lr_img, hr_img)
        torch.cuda.synchronize()
    finally:
        if old is None:
            os.environ.pop("SRHIP_SWIN_SIDE_WGRAD", None)
        else:
            os.environ["SRHIP_SWIN_SIDE_WGRAD"] = old
    diff = [k for k in names if not torch.equal(twin.fp.gviews[k], grads[k])]
    print(f"  SRHIP_SWIN_SIDE_WGRAD=0, step 1: gradients differing from the side-stream form: {len(diff)}; "
          f"wall time {time.perf_counter() - t_start:.1f} s")
    assert not diff, diff[:4]
