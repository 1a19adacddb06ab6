"""ACT's dropout on the GPU: srhip_dropout against the numpy restatement of its generator bit for bit (tests/philox_ref.py),
Tape.dropout in a small graph against float64 torch under the restatement's masks, the ACT training step against the
REFERENCE's autograd under the same masks (tests/golden/g52_act_dropout.npz, tools/make_golden_act_dropout.py), evaluation mode,
the per-iteration seed under hipGraph replay, and the command line.  The wiring with torch stand-ins for the kernels:
tests/test_cpu_act_dropout.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import philox_ref as PR  # noqa: E402
import sr_oracle as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(n_feats=16, n_resgroups=4, n_resblocks=2, reduction=4, n_heads=4, n_layers=8, n_fusionblocks=4)
OFFSETS = (0, 4096, (1 << 34) + 8)
RATES = (0.0, 0.25, 0.9)
SEED = 20260101


def _golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "g52_act_dropout.npz"))
    return {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("x2/")}


def _act(rate, seed=502):
    from dlib.models.network_act import ACT
    net = ACT(upscale=2, in_chans=1, dropout_rate=rate, **CFG)
    sd = O.seeded_state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()], seed)
    net.load_state_dict(sd, strict=True)
    return net.cuda()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("n", [1, 3, 4, 1023, (1 << 20) + 5])
def test_kernel_equals_the_restatement_bit_for_bit(n):
    """out = where(mask, x * scale, 0) in float32, for every offset, rate, in place and out of place, on 16-byte aligned
    operands (one 16-byte load and store per Philox call; n % 4 tail elements one by one) and on operands one float off the
    alignment (the element-wise form).  Cells outside [0, n) keep their NaN."""
    from srhip import ops
    x = torch.randn(n, generator=torch.Generator().manual_seed(n))
    x[0] = -0.0 if n > 1 else x[0]
    seed = torch.tensor([SEED], dtype=torch.int64, device="cuda")
    words = {offset: PR.words(SEED, 5, offset, n) for offset in OFFSETS}
    for shift in (0, 1):                                  # first element at a 16-byte boundary / 4 bytes past one
        xb = torch.full((n + 8,), float("nan"), device="cuda")
        xs = xb[4 + shift:4 + shift + n]
        assert xs.data_ptr() % 16 == 4 * shift
        for offset in OFFSETS:
            for p in RATES:
                thr, scale = PR.threshold(p)
                m = torch.from_numpy(words[offset] >= np.uint64(thr))
                ref = torch.where(m, x * torch.tensor(scale, dtype=torch.float32), torch.zeros(n))
                ob = torch.full((n + 8,), float("nan"), device="cuda")
                os_ = ob[4 + shift:4 + shift + n]
                xs.copy_(x)
                ops.dropout(xs, os_, seed, 5, p, offset=offset)
                assert torch.equal(_bits(os_), _bits(ref)), (n, shift, offset, p, "out of place")
                assert torch.equal(_bits(xs), _bits(x)), "the input is left alone"
                ops.dropout(xs, xs, seed, 5, p, offset=offset)
                assert torch.equal(_bits(xs), _bits(ref)), (n, shift, offset, p, "in place")
                for buf in (xb, ob):
                    assert bool(torch.isnan(buf[:4 + shift]).all()) and bool(torch.isnan(buf[4 + shift + n:]).all())
                if p == 0.0:
                    assert torch.equal(_bits(os_), _bits(x))
    # another site, another seed: other masks
    a, b, c = (torch.empty(n, device="cuda") for _ in range(3))
    one = torch.ones(n, device="cuda")
    ops.dropout(one, a, seed, 0, 0.25)
    ops.dropout(one, b, seed, 1, 0.25)
    ops.dropout(one, c, seed + 1, 0, 0.25)
    for got, (s, site) in ((a, (SEED, 0)), (b, (SEED, 1)), (c, (SEED + 1, 0))):
        assert np.array_equal(got.cpu().numpy() != 0, PR.mask(s, site, 0, n, 0.25))


def test_kernel_refuses_bad_arguments_and_launches_nothing():
    from srhip import ops
    from srhip._lib import lib
    x = torch.ones(64, device="cuda")
    out = torch.full((64,), float("nan"), device="cuda")
    seed = torch.tensor([SEED], dtype=torch.int64, device="cuda")
    for kw, what in ((dict(p=0.25, offset=1), "offset"), (dict(p=0.25, offset=6), "offset"), (dict(p=0.25, offset=-4), "offset"),
                     (dict(p=1.0), "p < 1"), (dict(p=1.5), "p < 1"), (dict(p=-0.1), "p < 1")):
        with pytest.raises(ops.SrhipError, match=what):
            ops.dropout(x, out, seed, 0, **kw)
        assert what in lib.srhip_last_error().decode()
    with pytest.raises(ops.SrhipError):
        ops.dropout(x[:60], x[4:], seed, 0, 0.25)         # partial overlap
    with pytest.raises(ops.SrhipError):
        ops.dropout(x, out, seed.cpu(), 0, 0.25)          # the seed lives on the device
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool((x == 1).all())


# ------------------------------------------------------------------ Tape.dropout
def test_tape_dropout_in_a_small_graph_vs_float64():
    """y = x + drop(W2 drop(gelu(W1 x + b1)) + b2) on 2 x 20 rows of 144 (sites 0 and 1): forward and every parameter
    gradient against float64 torch under the restatement's masks, at 2e-5 of the tensor's largest entry -- the gate of the
    Linear's GEMM (tests/test_gpu_kernels.py: gemm_nt; CONTRACTION of tests/test_gpu_tape_op_kernels.py).  A second run of the
    graph, and a second launch of a site's backward, reproduce the first bit for bit: masks are regenerated, not consumed."""
    from srhip import ops
    from srhip.engine import Bufs
    from srhip.tape import Tape, WeightBank
    p, M = 0.25, 40
    gen = torch.Generator().manual_seed(17)
    x = torch.randn(M, 144, generator=gen)
    W1, b1 = torch.randn(576, 144, generator=gen) / 12, 0.1 * torch.randn(576, generator=gen)
    W2, b2 = torch.randn(144, 576, generator=gen) / 24, 0.1 * torch.randn(144, generator=gen)
    dy = torch.randn(M, 144, generator=gen)
    par = {k: torch.nn.Parameter(v.cuda()) for k, v in (("W1", W1), ("b1", b1), ("W2", W2), ("b2", b2))}
    seed = torch.tensor([SEED], dtype=torch.int64, device="cuda")
    bufs, bank = Bufs(), WeightBank()

    def run():
        t = Tape(bufs, bank, True, torch.device("cuda"))
        t.seed = seed
        xv = t.var(x.cuda(), need=False)
        h = t.dropout(t.unary(t.linear(xv, par["W1"], par["b1"], "W1", "b1"), "gelu"), p)
        out = t.axpby(xv, t.dropout(t.linear(h, par["W2"], par["b2"], "W2", "b2"), p))
        y = out.t.clone()
        grads = {k: torch.full_like(v, float("nan")) for k, v in par.items()}
        t.backward(out, dy.cuda(), grads)
        torch.cuda.synchronize()
        return y, grads
    y, grads = run()
    # float64 statement
    s = 1.0 / (1.0 - p)
    m0 = torch.from_numpy(PR.mask(SEED, 0, 0, M * 576, p)).view(M, 576).double() * s
    m1 = torch.from_numpy(PR.mask(SEED, 1, 0, M * 144, p)).view(M, 144).double() * s
    r = {k: v.double().requires_grad_(True) for k, v in (("W1", W1), ("b1", b1), ("W2", W2), ("b2", b2))}
    F = torch.nn.functional
    y64 = x.double() + F.linear(F.gelu(F.linear(x.double(), r["W1"], r["b1"])) * m0, r["W2"], r["b2"]) * m1
    y64.backward(dy.double())

    def rel(a, b):
        return ((a.double().cpu() - b).abs().max() / b.abs().max()).item()
    errs = {"y": rel(y, y64.detach())}
    errs.update({k: rel(grads[k], r[k].grad) for k in par})
    print("tape dropout graph, error relative to the largest entry:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(e <= 2e-5 for e in errs.values()), errs
    y2, grads2 = run()
    assert torch.equal(y2, y) and all(torch.equal(grads2[k], grads[k]) for k in par)
    g = dy.cuda()
    o1, o2 = torch.empty_like(g), torch.empty_like(g)
    ops.dropout(g, o1, seed, 1, p)
    ops.dropout(g, o2, seed, 1, p)
    keep = torch.from_numpy(PR.mask(SEED, 1, 0, M * 144, p)).view(M, 144)
    assert torch.equal(o1, o2) and torch.equal(o1.cpu(), torch.where(keep, dy * torch.tensor(s, dtype=torch.float32), torch.zeros(())))


def test_tape_dropout_mask_does_not_depend_on_the_slicing(monkeypatch):
    """Tape._dropout walks a tensor LIMIT elements at a time and passes each slice's offset: with the limit lowered to 1000
    (slices of 1000 elements: multiples of 4) the output is the one launch's"""
    from srhip import tape as T
    from srhip.engine import Bufs
    seed = torch.tensor([SEED], dtype=torch.int64, device="cuda")
    x = torch.randn(37, 144, generator=torch.Generator().manual_seed(3)).cuda()
    outs = []
    for limit in (T.LIMIT, 1003):
        monkeypatch.setattr(T, "LIMIT", limit)
        t = T.Tape(Bufs(), T.WeightBank(), False, torch.device("cuda"))
        t.seed = seed
        outs.append(t.dropout(t.var(x, need=False), 0.25).t.clone())
    assert torch.equal(outs[0], outs[1])
    assert np.array_equal(outs[0].cpu().numpy().reshape(-1) != 0, PR.mask(SEED, 0, 0, x.numel(), 0.25))


# ------------------------------------------------------------------ the net
def test_act_dropout_training_step_gradients_vs_reference_golden():
    """TrainStep.step(..., dp=seed) on the g45 configuration with dropout_rate 0.25 against the reference's autograd under
    the same masks (g52_act_dropout.npz), as tests/test_gpu_tape_nets.py::test_act_training_step_gradients_vs_reference_golden
    does for g45: loss within 2e-5, every gradient within max(2e-5, 3 e32) of the tensor's largest entry, e32 the golden's own
    float32-against-float64 distance (grad64 / gslice64)."""
    from srhip.train import TrainStep, Optimizer
    g = _golden()
    net = _act(float(g["p"]), int(g["seed"])).train()
    ts = TrainStep(net, [("l1", 1.0)])
    ts.opt = Optimizer(ts.fp, "sgd", lr=0.0, momentum=0.0, nesterov=False, wd=0.0)
    seed = torch.tensor([int(g["drop_seed"])], dtype=torch.int64, device="cuda")
    ts.step(g["x"].cuda(), g["tgt"].cuda(), dp=seed)
    loss = ts.loss_values()[0]
    print(f"loss {loss:.7f} golden {float(g['loss']):.7f}")
    assert abs(loss - float(g["loss"])) <= 2e-5 * max(1.0, float(g["loss"]))
    worst, n = ("", 0.0, 0.0), 0
    for k in ts.fp.names:
        got = ts.fp.gviews[k].double().cpu()
        if "grad/" + k in g:
            ref, r64 = g["grad/" + k].double(), g["grad64/" + k].double()
            den = ref.abs().max().clamp_min(1e-30)
            e = ((got - ref).abs().max() / den).item()
        elif "gslice/" + k in g:
            ref, r64, sums = g["gslice/" + k].double(), g["gslice64/" + k].double(), g["gsum/" + k].double()
            den = sums[2].clamp_min(1e-30)
            e = ((got[:2] - ref).abs().max() / den).item()
            assert abs(got.sum().item() - sums[0].item()) <= 1e-4 * sums[1].item(), k
            assert abs(got.abs().sum().item() - sums[1].item()) <= 1e-4 * sums[1].item(), k
        else:                                   # blocks past n_fusionblocks: the forward does not reach them
            assert float(got.abs().max()) == 0.0, k
            continue
        e32 = ((ref - r64).abs().max() / den).item()
        worst, n = max(worst, (k, e, e32), key=lambda t: t[1]), n + 1
        assert e <= max(2e-5, 3.0 * e32), (k, e, e32)
    assert n == int(g["n_grads"])
    print(f"ACT x2 dropout training step: worst gradient error {worst[1]:.2e} (e32 {worst[2]:.2e}, {worst[0]}) of a tensor's largest entry")


def test_evaluation_ignores_the_rate_and_training_mode_does_not():
    g = _golden()
    x = g["x"].cuda()
    drop, plain = _act(0.25), _act(0.0)
    with torch.no_grad():
        y0 = plain.eval()(x)
        ye = drop.eval()(x)
        assert torch.equal(ye, y0)                        # evaluation: bit-identical to dropout_rate = 0
        assert drop.sample_drop_path(2, x.device) is None
        drop.train()
        torch.manual_seed(5)
        y1 = drop(x).clone()
        torch.manual_seed(5)
        y2 = drop(x).clone()
        torch.manual_seed(6)
        y3 = drop(x).clone()
    assert torch.equal(y1, y2)                            # one seed, one output
    assert (y1 - y0).abs().max() > 1e-3 * y0.abs().max()  # nn.Dropout follows module.training, not the grad mode
    assert not torch.equal(y3, y1)
    # with autograd recording: the same masks under the same seed
    torch.manual_seed(5)
    y4 = drop(x)
    assert y4.requires_grad and torch.equal(y4.detach(), y1)
    # a training-mode net without dropout still evaluates on the eager path under no_grad
    with torch.no_grad():
        assert torch.equal(plain.train()(x), y0)


def test_step_graph_with_dropout_follows_the_per_step_seed():
    """The trainer re-seeds before every iteration and ModelPlain replays the step from a hipGraph: the captured torch.randint of
    sample_drop_path must draw from the CURRENT seed at every replay (tests/test_gpu_swinir.py::
    test_step_graph_with_droppath_follows_the_per_step_seed for DropPath).  Eight steps on one batch: eager and replayed
    trajectories bit-identical, and consecutive losses differ by more than 1e-3 of their size (a repeated mask would repeat the
    loss up to the small weight change)."""
    from srhip.train import TrainStep, Optimizer
    g = _golden()
    batch = (g["x"].cuda(), g["tgt"].cuda())
    runs = []
    for mode in ("eager", "graph"):
        net = _act(0.25).train()
        ts = TrainStep(net, [("l1", 1.0)])
        # a learning rate at which eight steps move the loss by less than the 1e-3 gate below: what moves it is the masks
        ts.opt = Optimizer(ts.fp, "sgd", lr=1e-7, momentum=0.9, nesterov=True, wd=0.0)
        losses = []
        for it in range(8):
            torch.manual_seed(1000 + it)                     # the trainer's per-iteration seed
            (ts.step if mode == "eager" else ts.step_graph)(*batch)
            losses.append(ts.loss_buf.clone())
        torch.cuda.synchronize()
        runs.append((torch.stack(losses).cpu(), ts.fp.flat.clone().cpu()))
    assert bool(torch.isfinite(runs[0][0]).all()) and bool(torch.isfinite(runs[0][1]).all())
    assert torch.equal(runs[0][0], runs[1][0]), (runs[0][0][:, 1] - runs[1][0][:, 1]).abs().max()
    assert torch.equal(runs[0][1], runs[1][1])
    l = runs[1][0][:, 1]                                  # (loss_buf = [total (host-side), term 1, ...])
    print("losses", l.tolist())
    assert (l[1:] - l[:-1]).abs().max() > 1e-3 * l.abs().max(), l


def test_main_cli_trains_act_with_dropout_and_the_folder_evaluates(tmp_path):
    """`main.py --net_type ACT --ACT_dropout_rate 0.1`: two iterations of the registry net, a finite loss; define_model on the
    config_model.yml the run wrote (the rate is in it) followed by model.test() runs."""
    import yaml
    pkg = os.path.join(ROOT, "sr-caco-2_amd")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(pkg, "main.py"), "--net_type", "ACT", "--method", "ACT", "--scale", "4",
                        "--h_size", "96", "--batch_size", "2", "--max_iters", "2", "--ACT_dropout_rate", "0.1",
                        "--outd", str(tmp_path)], capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    losses = [float(l.split("G_loss")[1].split()[0]) for l in p.stdout.splitlines() if "G_loss" in l]
    assert len(losses) == 1 and np.isfinite(losses[0]), losses
    from dlib.models.select_model import define_model
    from dlib.utils.tools import Dict2Obj
    import main as M
    with open(os.path.join(str(tmp_path), "config_model.yml")) as f:
        args = Dict2Obj(yaml.safe_load(f))
    assert args.netG["ACT_dropout_rate"] == 0.1
    args.distributed, args.is_train = False, False
    args.netG["checkpoint_path_netG"] = os.path.join(str(tmp_path), args.save_dir_models, "2_G.pth")
    assert os.path.isfile(args.netG["checkpoint_path_netG"])
    model = define_model(args)
    model.load()
    assert model.netG.dropout_rate == 0.1
    model.feed_data(M.synth_batch(2, 4, 96, model.device, 3))
    model.test()
    e = model.current_visuals()["E"]
    assert e.shape == (2, 1, 96, 96) and bool(torch.isfinite(e).all())
