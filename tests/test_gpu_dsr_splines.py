"""DSR-Splines on the GPU (csrc/dsr_splines.hip, srhip/dsr_splines_engine.py, dlib/models/network_dsr_splines.py) against the
reference's own numbers (tests/golden/g53_dsr_splines.npz) and the float64 restatement (tests/dsr_splines_ref.py).

Gates (the project's): forward max abs <= 1e-5, gradients <= 2e-5 of the tensor's largest entry (+ 1e-12, as the other
gradient checks floor the denominator), expert ids / order / offsets bit-exact, TrainStep parameters within 2e-6 as for
SRCNN, graph replay and repeated backward runs bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dsr_splines_ref as R  # noqa: E402
from test_cpu_dsr_splines import load_case, grad_err  # noqa: E402

pytestmark = pytest.mark.gpu
FWD, GRAD = 1e-5, 2e-5


def pack(sd, lay, n):
    """the kernels' table [n, P] on the host: an expert's tensors in order, each padded to four floats"""
    T = len(lay) // n
    P = sum((int(np.prod(s)) + 3) // 4 * 4 for _, s in lay[:T])
    tab = torch.zeros(n, P)
    for k in range(n):
        off = 0
        for key, shape in lay[k * T:(k + 1) * T]:
            m = int(np.prod(shape))
            tab[k, off:off + m] = sd[key].reshape(-1)
            off += (m + 3) // 4 * 4
    return tab


def unpack(tab, lay, n):
    T = len(lay) // n
    out, pads = {}, []
    for k in range(n):
        off = 0
        for key, shape in lay[k * T:(k + 1) * T]:
            m = int(np.prod(shape))
            out[key] = tab[k, off:off + m].reshape(shape)
            pads.append(tab[k, off + m:off + (m + 3) // 4 * 4])
            off += (m + 3) // 4 * 4
    return out, torch.cat(pads)


def make_net(cfg, sd=None):
    from dlib.models.select_network import define_G
    nt = "DSR_Splines"
    netG = {'net_type': 'DSR-Splines', f'{nt}_upscale': cfg["scale"], f'{nt}_in_planes': 1, f'{nt}_in_ksz': cfg["in_ksz"],
            f'{nt}_splinenet_type': cfg["snet"], f'{nt}_n_splines_per_color': cfg["n"],
            f'{nt}_use_local_residual': cfg["local"], f'{nt}_use_global_residual': cfg["glob"], f'{nt}_color_min': 0,
            f'{nt}_color_max': 255}
    net = define_G(type("A", (), {"netG": netG}))
    if sd is not None:
        net.load_state_dict(sd, strict=True)
    return net.cuda()


def config(in_ksz, nh, n, local, glob, scale=2):
    return dict(in_ksz=in_ksz, nh=nh, n=n, local=local, glob=glob, scale=scale, hidden=R.HIDDEN[f"snet_type{nh}"],
                snet=f"snet_type{nh}")


@pytest.mark.parametrize("n", [1, 7, 16, 256])
def test_expert_id_and_order(n):
    """every k / 255, its float32 neighbours on both sides, 0.0 and 1.0: the product is float32, truncated -- bit-exact"""
    from srhip import ops
    k = (np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float32)
    v = np.concatenate([k, np.nextafter(k, np.float32(-1)), np.nextafter(k, np.float32(2)), np.float32([0.0, 1.0])])
    v = np.resize(v.astype(np.float32), (1, 10, 77)).copy()
    want = R.expert_ids(v, n)
    lut = ops.dsr_splines_level_table(n).cuda()
    ids, order, meta = ops.dsr_splines_order(torch.from_numpy(v).cuda(), lut, n)
    ids, order, seg = ids.cpu().numpy(), order.cpu().numpy(), meta[:257].cpu().numpy()
    assert ids.dtype == np.uint8 and np.array_equal(ids.astype(np.int64), want)
    flat = want.reshape(-1)
    assert np.array_equal(order, np.argsort(flat, kind="stable"))                 # a stable permutation
    assert seg[0] == 0 and np.array_equal(np.diff(seg), np.bincount(flat, minlength=256))
    # more than one block of the sort, a size that is no multiple of anything
    g = torch.Generator().manual_seed(n)
    big = torch.rand(3, 67, 131, generator=g)
    ids, order, meta = ops.dsr_splines_order(big.cuda(), lut, n)
    flat = R.expert_ids(big.numpy(), n).reshape(-1)
    assert np.array_equal(ids.cpu().numpy().reshape(-1).astype(np.int64), flat)
    assert np.array_equal(order.cpu().numpy(), np.argsort(flat, kind="stable"))
    assert np.array_equal(np.diff(meta[:257].cpu().numpy()), np.bincount(flat, minlength=256))


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_ops_against_the_golden(name):
    from srhip import ops
    cfg, a, sd, lay = load_case(name)
    n = cfg["n"]
    xi = torch.from_numpy(a["x_interp"])[:, 0].contiguous().cuda()
    tab = pack(sd, lay, n).cuda()
    assert tab.shape[1] == ops.dsr_splines_table_floats(cfg["in_ksz"], cfg["nh"], cfg["local"])
    lut = ops.dsr_splines_level_table(n).cuda()
    ids, order, meta = ops.dsr_splines_order(xi, lut, n)
    assert np.array_equal(ids.cpu().numpy(), a["ids"])
    y = torch.full_like(xi, float("nan"))
    args = (n, cfg["in_ksz"], cfg["nh"], cfg["local"], cfg["glob"])
    ops.dsr_splines_fwd(xi, tab, order, meta, y, *args)
    ey = (y.cpu() - torch.from_numpy(a["y"])[:, 0]).abs().max().item()
    print(f"{name}: forward {ey:.3g}")
    assert ey <= FWD
    tgt = torch.from_numpy(a["tgt"])[:, 0].cuda()
    dy = torch.sign(y - tgt) / y.numel()
    gt = torch.full_like(tab, float("nan"))
    ops.dsr_splines_bwd(xi, dy, tab, order, meta, gt, *args)
    grads, pads = unpack(gt.cpu(), lay, n)
    assert not pads.any()
    owners = set(np.unique(a["ids"]).tolist())
    worst = 0.0
    for k, _ in lay:
        if int(k.split(".")[1]) not in owners:
            assert bool((grads[k] == 0).all()), k                   # written zeros, not the NaN the buffer held
        worst = max(worst, grad_err(grads[k], a["grad/" + k]), grad_err(grads[k], a["grad64/" + k]))
        assert grad_err(grads[k], a["grad/" + k]) <= GRAD and grad_err(grads[k], a["grad64/" + k]) <= GRAD, k
    print(f"{name}: gradients {worst:.3g}")


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_module_from_the_low_resolution_input(name):
    cfg, a, sd, lay = load_case(name)
    net = make_net(cfg, sd).train()
    x, tgt = torch.from_numpy(a["x"]).cuda(), torch.from_numpy(a["tgt"]).cuda()
    y = net(x)
    assert np.array_equal(net.engine.last_ids.cpu().numpy(), a["ids"])
    assert (y.detach().cpu() - torch.from_numpy(a["y"])).abs().max().item() <= FWD
    loss = (y - tgt).abs().mean()
    assert abs(loss.item() - float(a["loss"])) <= 1e-6
    loss.backward()
    for k, p in net.named_parameters():
        assert grad_err(p.grad.cpu(), a["grad/" + k]) <= GRAD, k
    net.eval()
    with torch.no_grad():
        ye = net(x)
    assert (ye.cpu() - torch.from_numpy(a["y"])).abs().max().item() <= FWD
    net.amp = True                                                   # --amp evaluation: the same float32 kernels
    with torch.no_grad():
        assert torch.equal(net(x), ye)


SHAPES = [
    ("17x33", config(5, 3, 7, True, True), (1, 17, 33)),            # no multiple of the 64-pixel tile, 7 uneven bins
    ("pad+1", config(7, 2, 5, True, False), (2, 4, 9)),             # a side one larger than the reflect pad
    ("one spline", config(3, 2, 1, False, True), (2, 12, 10)),      # one segment holds everything
    ("LDS corner", config(15, 8, 256, True, True), (1, 8, 10)),     # the largest expert, 256 of them
]


@pytest.mark.parametrize("tag,cfg,shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_shapes_against_the_float64_restatement(tag, cfg, shape):
    import sr_oracle as O
    lay = R.layout(cfg["in_ksz"], cfg["hidden"], cfg["n"], cfg["local"])
    sd = O.seeded_state_dict(lay, 5317)
    net = make_net(cfg, sd).train()
    g = torch.Generator().manual_seed(29)
    xi = (torch.rand(shape, generator=g) * 1.2 - 0.1).clamp(0, 1)
    # the loss is sum(y * dy) with a normal dy: an L1 loss hands every pixel +-1/N, and a one-entry tensor (the last bias)
    # of an expert with as many +s as -s is then exactly zero in float64 and a rounding residue in any float32 sum -- the
    # gate is relative to the tensor's largest entry, so such a fixture measures nothing
    dy = torch.randn(shape, generator=g) / xi.numel()
    eng = net.engine
    y = eng.forward_interp(xi.cuda(), save=True)[:, 0]
    ids = eng.last_ids.cpu().numpy().astype(np.int64)
    assert np.array_equal(ids, R.expert_ids(xi.numpy(), cfg["n"]))
    grads = {k: torch.full_like(p, float("nan")) for k, p in net.named_parameters()}
    eng.backward(dy.cuda(), grads)
    args = (cfg["hidden"], cfg["in_ksz"], cfg["local"], cfg["glob"])
    y64, _, g64 = R.loss_and_grads(sd, xi[:, None], ids, None, *args, torch.float64, dy=dy[:, None])
    ey = (y.cpu().double() - y64[:, 0]).abs().max().item()
    worst = max(grad_err(grads[k].cpu(), g64[k]) for k in g64)
    print(f"{tag}: forward {ey:.3g}, gradients {worst:.3g}")
    assert ey <= FWD
    for k in g64:
        assert grad_err(grads[k].cpu(), g64[k]) <= GRAD, k


def test_sides_within_the_pad_raise_by_name():
    net = make_net(config(7, 1, 4, False, False)).eval()
    with pytest.raises(ValueError, match="reflect-pads by 3"):
        net.engine.forward_interp(torch.rand(1, 3, 9).cuda(), save=False)
    with pytest.raises(AssertionError, match="no gradient through the bicubic"):
        net.train()
        net.engine.forward_interp(torch.rand(1, 8, 9).cuda(), save=True)
        net.engine.backward(torch.zeros(1, 8, 9).cuda(), {k: torch.empty_like(p) for k, p in net.named_parameters()}, need_dx=True)


def test_backward_is_deterministic():
    import sr_oracle as O
    cfg = config(5, 3, 7, True, True)
    lay = R.layout(5, cfg["hidden"], 7, True)
    net = make_net(cfg, O.seeded_state_dict(lay, 11)).train()
    g = torch.Generator().manual_seed(12)
    xi, dy = torch.rand(2, 70, 90, generator=g).cuda(), torch.randn(2, 70, 90, generator=g).cuda()
    runs = []
    for _ in range(2):
        net.engine.forward_interp(xi, save=True)
        grads = {k: torch.full_like(p, float("nan")) for k, p in net.named_parameters()}
        net.engine.backward(dy, grads)
        runs.append(torch.cat([grads[k].reshape(-1) for k in grads]))
    assert bool(torch.isfinite(runs[0]).all()) and torch.equal(runs[0], runs[1])


def test_train_step_and_graph_replay():
    """One L1 + SGD-Nesterov step at case A's shape against the restatement's autograd + the oracle's optimizer; the flat
    parameter and gradient buffers are the kernels' tables, in place; a captured step replays bit for bit."""
    import sr_oracle as O
    from srhip.train import TrainStep, Optimizer
    cfg, a, sd, lay = load_case("A")
    x, tgt = torch.from_numpy(a["x"]).cuda(), torch.from_numpy(a["tgt"]).cuda()

    def trainer():
        net = make_net(cfg, sd).train()
        ts = TrainStep(net, [("l1", 1.0)])
        ts.opt = Optimizer(ts.fp, "sgd", lr=0.01, momentum=0.9, nesterov=True, wd=0.0)
        return net, ts
    net, ts = trainer()
    ts.step(x, tgt)
    assert net.engine.table.data_ptr() == ts.fp.flat.data_ptr()      # used in place: nothing packed
    xi = torch.from_numpy(a["x_interp"])
    y32, l32, g32 = R.loss_and_grads(sd, xi, a["ids"].astype(np.int64), torch.from_numpy(a["tgt"]), cfg["hidden"],
                                     cfg["in_ksz"], cfg["local"], cfg["glob"], torch.float32)
    assert abs(ts.loss_values()[0] - l32.item()) <= 1e-5
    for k, p in net.named_parameters():
        w = sd[k].clone()
        O.sgd_nesterov_step(w, g32[k], torch.zeros_like(w), True, 0.01)
        assert (p.detach().cpu() - w).abs().max().item() <= 2e-6, k
    ts.step(x, tgt)
    ts.step(x, tgt)
    net2, ts2 = trainer()
    for _ in range(3):                                               # eager, capture + replay, replay
        ts2.step_graph(x, tgt)
    assert ts2._graph["g"] is not None
    torch.cuda.synchronize()
    assert torch.equal(ts.fp.flat, ts2.fp.flat) and torch.equal(ts.loss_buf, ts2.loss_buf)
    with pytest.raises(NotImplementedError):
        TrainStep(make_net(cfg, sd).train(), [("l1", 1.0)], amp=True)


def test_evaluation_forward_replays_from_a_graph():
    """no host read between the interpolation and the output: the forward is captured once and replayed on other pixels
    (other experts, other segment offsets) bit for bit"""
    cfg, a, sd, lay = load_case("B")
    net = make_net(cfg, sd).eval()
    g = torch.Generator().manual_seed(5)
    x1, x2 = torch.rand(2, 1, 5, 7, generator=g).cuda(), (torch.rand(2, 1, 5, 7, generator=g) * 0.3).cuda()
    with torch.no_grad():
        want1, want2 = net(x1).clone(), net(x2).clone()
        xs = x1.clone()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = net(xs)
        for x, want in ((x2, want2), (x1, want1)):
            xs.copy_(x)
            graph.replay()
            assert torch.equal(y, want)
    assert not torch.equal(want1, want2)


def test_main_trains_it_and_eval_loads_the_folder(tmp_path):
    """main.py --net_type DSR-Splines over the fixture folds (ModelPlain's step, validation, best model, test score), then
    eval.py builds the same net from the experiment folder and reproduces the test score"""
    import pickle
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fx = os.path.join(root, "tests", "golden", "eval_exp")
    ds = "caco2_test_X_8_in_64_out_512_cell_CELL0"
    outd = str(tmp_path / "exp")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = ("--task super-resolution --scale 8 --method DSR-SPLINES --net_type DSR-Splines --n_channels 1 --h_size 64 "
           "--batch_size 1 --DSR_Splines_in_ksz 5 --DSR_Splines_splinenet_type snet_type2 --DSR_Splines_n_splines_per_color 7 "
           "--DSR_Splines_use_local_residual True --DSR_Splines_use_global_residual True --l1 True --max_epochs 2 "
           "--checkpoint_eval 2 --checkpoint_save 3 --G_optimizer_lr 1e-3 --eval_bsize 2").split()
    cmd += ["--train_dsets", ds, "--valid_dsets", ds, "--test_dsets", ds, "--data_root", os.path.join(fx, "data"),
            "--splits_root", os.path.join(fx, "folds"), "--outd", outd]
    p = subprocess.run([sys.executable, os.path.join(root, "sr-caco-2_amd", "main.py")] + cmd, capture_output=True, text=True,
                       timeout=600, env=env)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    with open(os.path.join(outd, "tracker.pkl"), "rb") as f:
        tr = pickle.load(f)
    losses = tr["train"]["period_iter"]["master_loss"]["vals"]
    assert len(losses) == 6 and all(np.isfinite(losses))
    test_psnr = tr["test"][ds]["psnr"]["vals"][0]
    sd = torch.load(os.path.join(outd, "best-models", "G-model.pth"), map_location="cpu")
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == R.layout(5, [32, 16], 7, True)
    import eval as E
    tr2, _ = E.evaluate_pretrained(["--cudaid", "0", "--exp_path", outd, "--data_root", os.path.join(fx, "data"),
                                    "--splits_root", os.path.join(fx, "folds")])
    assert abs(tr2["test"][ds]["psnr"]["vals"][0] - test_psnr) <= 1e-9


def test_full_size_forward():
    """registry default, x8, 1 x 1 x 64 x 64 -> 512 x 512 against the float32 restatement: MAE <= 1e-5, PSNR within 0.01 dB"""
    import sr_oracle as O
    cfg = config(3, 1, 16, False, False, scale=8)
    lay = R.layout(3, [16], 16, False)
    sd = O.seeded_state_dict(lay, 5308, bias_std=0.1)
    net = make_net(cfg, sd).eval()
    g = torch.Generator().manual_seed(8)
    x, tgt = torch.rand(1, 1, 64, 64, generator=g), torch.rand(1, 1, 512, 512, generator=g)
    with torch.no_grad():
        y = net(x.cuda()).cpu()
        xi = net.engine.interpolate(x.cuda()).cpu()
    ids = net.engine.last_ids.cpu().numpy().astype(np.int64)
    assert np.array_equal(ids, R.expert_ids(xi.numpy(), 16))
    with torch.no_grad():
        yo = R.forward(sd, xi[:, None], ids, [16], 3, False, False)
    assert float(yo.abs().max()) > 0
    assert (y - yo).abs().mean().item() <= 1e-5
    ps = lambda t: O.metric_psnr(O.tensor2uint82float(t), O.tensor2uint82float(tgt), 8)
    assert (ps(y) - ps(yo)).abs().max().item() <= 0.01
