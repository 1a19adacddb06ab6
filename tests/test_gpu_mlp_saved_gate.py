"""The saved form of the fused MLP kernels (srhip_mlp_fwd_save_f16x2 / srhip_mlp_bwd_gate_f16x2, mlp_f16.hip): the forward
writes gate = Phi(h) + h phi(h) and gelu(h) beside (or instead of) h, the backward multiplies by that gate and neither
evaluates the GELU nor stores gelu(h).  Everything is compared with the h form on the same inputs -- the values are the
same function of the same h bits, so the project's rounding bound (2e-6 of the tensor's maximum, the bound of
test_recompute_gelu_in_the_weight_gradient_matches_the_stored_form) holds with room -- and the training step with
SRHIP_MLP_SAVE_GATE=1 with the step that saves h (SRHIP_MLP_SAVE_GATE=0)."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

G = torch.Generator().manual_seed(13579)
BOUND = 2e-6


def rnd(*shape, scale=1.0):
    return torch.randn(*shape, generator=G) * scale


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


@pytest.fixture(scope="module")
def ops():
    from srhip import ops as o
    return o


def _problem(ops, M, C, hidden, nsamp):
    x = rnd(M, C) * 1.5 + rnd(M, 1)
    w1, b1 = rnd(hidden, C, scale=0.1), rnd(hidden, scale=0.3)
    w2, b2 = rnd(C, hidden, scale=0.1), rnd(C, scale=0.3)
    gamma, beta = 1 + rnd(C, scale=0.2), rnd(C, scale=0.2)
    K0 = 3 * C
    w0, w3 = rnd(C, K0, scale=0.08), rnd(C, C, scale=0.1)
    dev = {k: v.cuda() for k, v in dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, gamma=gamma, beta=beta, dy=rnd(M, C),
                                        X0=rnd(M, K0), x0=rnd(M, C) * 1.3 + rnd(M, 1), res0=rnd(M, C)).items()}
    dev["s"] = (torch.rand(nsamp, generator=G) + 0.5).cuda() if nsamp else None
    dev["s3"] = (torch.rand(nsamp, generator=G) + 0.5).cuda() if nsamp else None
    P = {k: ops.Bx3(*shape, "cuda") for k, shape in dict(w1=(hidden, C), w2=(C, hidden), w1T=(C, hidden), w2T=(hidden, C),
                                                         w0=(C, K0), w3=(C, C)).items()}
    b1f = torch.empty(hidden, device="cuda")
    tb = ops.PrepTable()
    tb.linear(dev["w1"], P["w1"], gamma=dev["gamma"], f16=True)
    tb.linear(dev["w1"], P["w1T"], gamma=dev["gamma"], transpose=True, f16=True)
    tb.linear(dev["w2"], P["w2"], f16=True)
    tb.linear(dev["w2"], P["w2T"], transpose=True, f16=True)
    tb.linear(w0.cuda(), P["w0"], f16=True)
    tb.linear(w3.cuda(), P["w3"], f16=True)
    tb.fold_bias(dev["w1"], dev["b1"], dev["beta"], b1f)
    tb.build("cuda").run()
    st, st0 = torch.empty(M, 2, device="cuda"), torch.empty(M, 2, device="cuda")
    ops.layernorm_fwd(dev["x"], st)
    ops.layernorm_fwd(dev["x0"], st0)
    return dev, P, b1f, st, st0


def _kernel_gate_and_gelu(h):
    """float64 statement of gelu_gate2 (mlp_f16.hip): Phi by Abramowitz & Stegun 7.1.26, gate = Phi + h phi, gl = h Phi"""
    x = h.double().cpu()
    t = 1.0 / (1.0 + 0.3275911 * x.abs() * math.sqrt(0.5))
    poly = t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429))))
    e1 = torch.exp(-0.5 * x * x)
    cdf = 0.5 * (1.0 + torch.sign(x) * (1.0 - poly * e1))
    return cdf + x * 0.39894228040143267794 * e1, x * cdf


# (C, hidden): one 192-unit half | a second half of 4 units | two full halves at the README width
# M: a ragged second block | a third block of two rows;  nsamp = 3: rows_per_scale 24 / 44, neither divides the 64-row block
@pytest.mark.parametrize("nsamp", [0, 3])
@pytest.mark.parametrize("M", [70, 130])
@pytest.mark.parametrize("C,hidden", [(132, 132), (180, 196), (180, 360)])
def test_saved_gate_forward_and_the_three_backward_forms_match_the_h_form(ops, C, hidden, M, nsamp):
    assert ops.mlp_f16_fusable(C, hidden)
    dev, P, b1f, st, st0 = _problem(ops, M, C, hidden, nsamp)
    rps = -(-M // nsamp) if nsamp else 1
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")      # noqa: E731
    kw = dict(rowscale=dev["s"], rows_per_scale=rps)

    # ---- forward: h, gate and gelu(h) in one call; out, the statistics and h are the h form's bits
    out_old, h_old, so_old = nan(M, C), nan(M, hidden), nan(M, 2)
    ops.mlp_fwd_f16(dev["x"], st, P["w1"], b1f, P["w2"], dev["b2"], out_old, h=h_old, stats_out=so_old, **kw)
    out, h, gate, gh, so = nan(M, C), nan(M, hidden), nan(M, hidden), nan(M, hidden), nan(M, 2)
    ops.mlp_fwd_f16(dev["x"], st, P["w1"], b1f, P["w2"], dev["b2"], out, h=h, stats_out=so, gate=gate, gh=gh, **kw)
    assert torch.equal(out, out_old) and torch.equal(h, h_old) and torch.equal(so, so_old)
    # ... and what the training step asks for: gate and gelu(h), no h
    out2, gate2, gh2 = nan(M, C), nan(M, hidden), nan(M, hidden)
    ops.mlp_fwd_f16(dev["x"], st, P["w1"], b1f, P["w2"], dev["b2"], out2, gate=gate2, gh=gh2, **kw)
    assert torch.equal(out2, out) and torch.equal(gate2, gate) and torch.equal(gh2, gh)
    gate_ref, gl_ref = _kernel_gate_and_gelu(h)
    e_gate, e_gl = relerr(gate, gate_ref), relerr(gh, gl_ref)
    print(f"gate vs float64 {e_gate:.2e}  gelu(h) vs float64 {e_gl:.2e}")
    assert e_gate <= BOUND and e_gl <= BOUND

    # ---- backward, h form against gate form: plain | chain | front + chain
    front = (dev["X0"], P["w0"], dev["x0"], st0, dev["res0"])

    def run(form, saved):
        dy = nan(M, C) if form == "front" else dev["dy"].clone()
        dh, gh_b, dx, o3 = nan(M, hidden), nan(M, hidden), nan(M, C), nan(M, C)
        ops.mlp_bwd_f16(dy, P["w2T"], P["w1T"], None if saved else h, dh, None if saved else gh_b, dev["x"], st, dx,
                        chain=None if form == "plain" else (P["w3"], o3, dev["s3"]),
                        front=front if form == "front" else None, gate=gate if saved else None, **kw)
        return dict(dy=dy, dh=dh, dx=dx, gh=gh_b, out3=None if form == "plain" else o3)
    for form in ("plain", "chain", "front"):
        old, new = run(form, False), run(form, True)
        if form == "plain":
            e = relerr(gh, old["gh"])                # the forward's gelu(h) against the one the h-form backward stores
            print(f"gelu(h), forward vs backward {e:.2e}")
            assert e <= BOUND
        assert torch.isnan(new["gh"]).all()          # the gate form writes no gelu(h)
        for k in ("dy", "dh", "dx", "out3"):
            if old[k] is not None:
                e = relerr(new[k], old[k])
                print(f"{form} {k} {e:.2e}")
                assert e <= BOUND, (form, k, e)


def test_saved_gate_entry_points_refuse_what_they_cannot_do(ops):
    M, C, hidden = 64, 180, 360
    dev, P, b1f, st, _ = _problem(ops, M, C, hidden, 0)
    out, gate, dh, dx = (torch.empty(M, n, device="cuda") for n in (C, hidden, hidden, C))
    L, p = ops.lib, lambda t: None if t is None else t.data_ptr()      # noqa: E731
    # neither gate nor gelu(h): that is srhip_mlp_fwd_f16x2
    assert L.srhip_mlp_fwd_save_f16x2(p(dev["x"]), C, p(st), p(P["w1"].planes), p(b1f), p(P["w2"].planes), p(dev["b2"]), None,
                                      None, None, hidden, p(out), C, M, C, hidden, None, 1, None, None) != 0
    # a pitch shorter than the row
    assert L.srhip_mlp_fwd_save_f16x2(p(dev["x"]), C, p(st), p(P["w1"].planes), p(b1f), p(P["w2"].planes), p(dev["b2"]), None,
                                      p(gate), None, hidden - 4, p(out), C, M, C, hidden, None, 1, None, None) != 0
    # the backward without a gate
    assert L.srhip_mlp_bwd_gate_f16x2(None, 0, 0, None, None, 0, None, None, 0, p(dev["dy"]), C, p(P["w2T"].planes),
                                      p(P["w1T"].planes), None, hidden, p(dh), p(dev["x"]), C, p(st), p(dx), C, M, C, hidden,
                                      None, 1, None, None, 0, None, None) != 0
    torch.cuda.synchronize()


def _step(SwinIR, kw, dpr, save_gate, graph=False):
    from srhip.train import TrainStep, Optimizer
    os.environ["SRHIP_MLP_SAVE_GATE"] = save_gate
    try:
        torch.manual_seed(11)
        net = SwinIR(upscale=8, in_chans=1, img_size=16, window_size=8, mlp_ratio=2, upsampler="pixelshuffledirect",
                     drop_path_rate=dpr, **kw).cuda().train()
        ts = TrainStep(net, [("l1", 1.0)])
        ts.opt = Optimizer(ts.fp, "sgd", lr=0.0, momentum=0.0, nesterov=False, wd=0.0)
        gen = torch.Generator().manual_seed(3)
        lr_img, hr_img = torch.rand(2, 1, 16, 16, generator=gen).cuda(), torch.rand(2, 1, 128, 128, generator=gen).cuda()
        torch.manual_seed(77)                      # the same DropPath masks in every run
        if graph:
            for _ in range(3):
                ts.step_graph(lr_img, hr_img)
        else:
            ts.step(lr_img, hr_img)
        torch.cuda.synchronize()
        saved = [(b[6] is not None, b[7] is not None, b[8] is not None) for b in net.engine.saved["blocks"]]     # h, gate, gelu(h)
        return {k: ts.fp.gviews[k].clone() for k in ts.fp.names}, ts.loss_values()[0], saved
    finally:
        os.environ.pop("SRHIP_MLP_SAVE_GATE", None)


@pytest.fixture(scope="module")
def SwinIR():
    from dlib.models.network_swinir import SwinIR as cls
    return cls


@pytest.mark.parametrize("kw,dpr", [(dict(depths=[2, 2], embed_dim=60, num_heads=[6, 6]), 0.0),
                                    (dict(depths=[2], embed_dim=180, num_heads=[6]), 0.3)])
def test_training_step_with_the_saved_gate_matches_the_step_that_saves_h(SwinIR, kw, dpr):
    """embed 60 takes the separate Linear launches (the switch must not touch it), embed 180 with DropPath the fused kernels"""
    g0, l0, sv0 = _step(SwinIR, kw, dpr, "0")
    g1, l1, sv1 = _step(SwinIR, kw, dpr, "1")
    fused = kw["embed_dim"] == 180
    assert set(sv0) == {(True, False, False)} and set(sv1) == {(False, True, True) if fused else (True, False, False)}
    print(f"loss {l0!r} {l1!r}")
    assert abs(l1 - l0) <= 1e-6
    assert any("fc2.weight" in k for k in g0)
    for k in g0:
        e = (g1[k] - g0[k]).abs().max().item()
        assert e <= BOUND * max(g0[k].abs().max().item(), 1e-12), (k, e)


def test_graph_replay_of_the_saved_gate_step_is_its_eager_step(SwinIR):
    kw = dict(depths=[2, 2], embed_dim=180, num_heads=[6, 6])
    eager, _, _ = _step(SwinIR, kw, 0.0, "1")
    replay, _, _ = _step(SwinIR, kw, 0.0, "1", graph=True)
    for k in eager:
        assert torch.equal(replay[k], eager[k]), k
