"""MemNet on libsrhip (dlib.models.network_memnet, srhip/memnet_engine.py, csrc/bn.hip): the BatchNorm kernels against
float64 aten, the network against the fixture generated from the reference class (g26_memnet.npz: eval / train outputs,
gradients, running statistics after the step) and against the oracle through the fused training step."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import sr_oracle as O  # noqa: E402

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# Gradient gates of the tiny fixture: relative L2 per tensor, as for MSLapSRN (tests/test_gpu_mslapsrn.py) -- a ReLU
# decision that falls differently under f32 rounding moves a gradient by a discrete step; the oracle itself sits at
# 9e-6 / 4.4e-5 relative L2 from the reference class on these two fixtures (oracle/make_goldens.py g_memnet).
L2_GATE = 1e-3
# The BatchNorm on the 1-channel image has ONE weight and ONE bias: their gradients are sums of signed per-pixel terms that
# cancel to ~1/40 of the sum of magnitudes (0.128 against 5.7 on the fused-step case), so the same per-pixel noise shows 40x
# larger on them -- measured up to 5e-3 with one build of the conv kernels, 1.4e-3 with another
SCALAR_GATE = 3e-2


# ... and the per-channel BatchNorm weight / bias gradients (sums over all pixels of one channel) sit in between: 1.25e-3 seen
VECTOR_GATE = 5e-3


def gate(p):
    return SCALAR_GATE if p.numel() == 1 else (VECTOR_GATE if p.dim() == 1 else L2_GATE)


def load(name):
    z = np.load(os.path.join(G, name + ".npz"), allow_pickle=False)
    return {k: (torch.from_numpy(z[k]) if z[k].dtype.kind in "fiu" else z[k]) for k in z.files}


from bn_float64 import check_batchnorm_vs_float64, rel  # noqa: E402  (the flow tests/test_gpu_launch_plans.py runs too)


@pytest.mark.parametrize("shape,C", [((2, 24, 20), 64), ((1, 7, 9), 128), ((3, 16, 16), 1), ((1, 5, 13), 1),
                                     ((2, 33, 31), 448)])
def test_batchnorm_kernels_vs_float64(shape, C):
    """srhip_bn_stats / _apply / _bwd on channels-last data against nn.functional.batch_norm in float64 (training mode:
    batch statistics, running-statistics update, ReLU, gradients of x, gamma, beta with a skip gradient added)."""
    check_batchnorm_vs_float64(shape, C)


def test_batchnorm_rejects_unsupported_channel_counts():
    from srhip import ops
    from srhip._lib import SrhipError
    x = torch.randn(4, 4, 48, device="cuda")
    with pytest.raises(SrhipError):
        ops.bn_apply(x, torch.zeros(4, 48, device="cuda"))


@pytest.mark.parametrize("tag", ["a", "b"])
def test_eval_train_gradients_and_running_stats_vs_reference_golden(tag):
    from dlib.models.network_memnet import MemNet
    g = {k[len(tag) + 1:]: v for k, v in load("g26_memnet").items() if k.startswith(tag + "/")}
    scale, M, R, seed = (int(v) for v in g["cfg"])
    sd = O.memnet_init_state_dict(M, R, 1, seed=seed)
    net = MemNet(in_chans=1, upscale=scale, num_memory_blocks=M, num_residual_blocks=R)
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == [(k, tuple(v.shape)) for k, v in sd.items()]
    net.load_state_dict(sd, strict=True)
    net = net.cuda().eval()
    x = g["x"].cuda()
    with torch.no_grad():
        ye = net(x)
    mag = max(1.0, g["y_eval"].abs().max().item())
    assert (ye.cpu() - g["y_eval"]).abs().max().item() <= 1e-5 * mag
    assert torch.equal(net.state_dict()["reconstructor.0.running_mean"].cpu(), sd["reconstructor.0.running_mean"])
    net.train()
    y = net(x)
    assert (y.detach().cpu() - g["y_train"]).abs().max().item() <= 1e-5 * mag
    (y - g["target"].cuda()).abs().mean().backward()
    sums = g["grad_sums"].numpy()
    for i, (k, p) in enumerate(net.named_parameters()):
        gk = p.grad.double().cpu()
        if "grad/" + k in g:
            ref = g["grad/" + k].double()
            assert ((gk - ref).norm() / ref.norm()).item() <= gate(p), k
        assert abs(gk.abs().sum().item() - sums[i][1]) <= 2e-4 * max(sums[i][1], 1e-6), (k, gk.abs().sum().item(), sums[i][1])
    after = net.state_dict()
    for k, v in g.items():
        if k.startswith("after/"):
            got = after[k[len("after/"):]].cpu()
            if v.dtype.is_floating_point:
                assert rel(got, v) < 2e-6, k
            else:
                assert int(got) == int(v), k


def test_fused_train_step_vs_oracle():
    """One fused optimisation step (forward + L1 + backward + SGD) at 24 -> 96, x4, 2 memory blocks of 2 units: loss,
    gradients (relative L2 per tensor against the float64 oracle, the float32 oracle's own distance as the yardstick) and
    the applied update."""
    from dlib.models.network_memnet import MemNet
    from srhip.train import TrainStep, Optimizer
    scale, M, R = 4, 2, 2
    sd = O.memnet_init_state_dict(M, R, 1, seed=17)
    net = MemNet(in_chans=1, upscale=scale, num_memory_blocks=M, num_residual_blocks=R)
    net.load_state_dict(sd, strict=True)
    net = net.cuda().train()
    gen = torch.Generator().manual_seed(23)
    x, tgt = torch.rand(2, 1, 24, 24, generator=gen), torch.rand(2, 1, 96, 96, generator=gen)
    step = TrainStep(net, [("l1", 1.0)])
    lr = 1e-2
    step.opt = Optimizer(step.fp, "sgd", lr=lr, momentum=0.0, nesterov=False, wd=0.0)
    step.step(x.cuda(), tgt.cuda())

    def run(dt):
        s = {k: (v.to(dt).clone().requires_grad_(True) if v.is_floating_point() and "running" not in k else v.clone())
             for k, v in sd.items()}
        stats = {}
        yo = O.memnet_forward(s, x.to(dt), scale, M, R, training=True, stats=stats)
        loss = (yo - tgt.to(dt)).abs().mean()
        loss.backward()
        return s, loss, stats
    s32, loss, stats = run(torch.float32)
    s64, _, _ = run(torch.float64)
    assert abs(step.loss_values()[0] - loss.item()) <= 2e-6 * max(1.0, abs(loss.item()))
    worst = ("", 0.0, 0.0)
    for k, p in net.named_parameters():
        ref = s64[k].grad
        den = ref.abs().max().item() + 1e-12
        gh = step.fp.gviews[k].detach().cpu()
        e = ((gh.double() - ref).norm() / ref.norm()).item()
        e32 = ((s32[k].grad.double() - ref).norm() / ref.norm()).item()     # what float32 autograd on the CPU gets
        if e > worst[1]:
            worst = (k, e, e32)
        # 18 k pixels, 16 ReLUs deep: a handful of ReLU decisions fall differently under f32 rounding in ANY f32
        # evaluation (the f32 oracle is 2e-4 entry-wise from the f64 one on a mid-net conv) -- relative L2 per tensor
        assert e <= max(gate(p), 3.0 * e32), (k, e, e32)
        del den
        assert (p.detach().cpu() - (sd[k] - lr * gh)).abs().max() <= 1e-7 * max(1.0, sd[k].abs().max().item()), k
    after = net.state_dict()
    for k, v in stats.items():
        if v.is_floating_point():
            assert rel(after[k], v) < 5e-6, k
        else:
            assert int(after[k]) == int(v), k
    print("worst gradient vs the fp64 oracle (name, libsrhip, fp32 oracle)", worst)


def test_registry_and_model_plain_eval():
    import main as M
    from dlib.models.select_model import define_model
    args = M.parse_input(["--net_type", "MemNet", "--method", "MemNet", "--task", "super-resolution", "--scale", "4",
                          "--n_channels", "1", "--h_size", "64", "--batch_size", "2", "--MemNet_num_memory_blocks", "2",
                          "--MemNet_num_residual_blocks", "2"])
    model = define_model(args)
    assert len(model.netG.dense_memory_blocks) == 2
    model.init_train()
    batch = M.synth_batch(2, 4, 64, model.device, 3)
    model.feed_data(batch)
    model.test()
    assert tuple(model.E.shape) == (2, 1, 64, 64) and torch.isfinite(model.E).all()
    model.optimize_parameters(0, 1)
    assert model.check_finite() and tuple(model.E.shape) == (2, 1, 64, 64)
