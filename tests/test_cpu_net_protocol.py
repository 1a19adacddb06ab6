"""What every net mirror owes its callers (dlib/models/engine_net.py: EngineNet, NetFn), for the seventeen registry nets, on
the CPU with a stub engine: the reference's state_dict keys (tests/golden/mirror_state_keys.json, recorded before the mirrors
shared a base class), the lazy engine and its invalidation, the GPU-only message, and how the one autograd node hands
parameters, gradients, the input gradient, MSLapSRN's extra outputs, DSR-Splines' gradient table and --amp to the engine."""
import json
import os

import pytest
import torch

import net_protocol_cases as C

from srhip._lib import lib

NAMES = list(C.NETS)
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mirror_state_keys.json")) as f:
    KEYS = json.load(f)


class StubEngine:
    """Records what the mirror asks of it.  forward: the input repeated `upscale` times; backward: the number i into the
    gradient of parameter i, and sevens as the input gradient when it is asked for."""

    def __init__(self, net):
        self.net, self.calls, self.modes, self.backward_kw, self.grads = net, [], [], None, None
        self.intermediate_outs = self.all_outs = []

    def invalidate(self):
        self.calls.append("invalidate")

    def forward(self, x, dp=None, save=True):
        self.calls.append(("forward", dp, save))
        self.modes.append(lib.srhip_get_matmul_mode())
        s = self.net.upscale
        y = x.detach()[:, None].repeat_interleave(s, 2).repeat_interleave(s, 3).clone()
        if type(self.net).__name__ == "MSLapSRN":
            self.intermediate_outs = [y[:, :, ::2, ::2] * 2, y * 3]
        self.x = x
        return y

    def backward(self, dy, grads, **kw):
        self.calls.append("backward")
        self.dy, self.grads, self.backward_kw = dy, grads, kw
        for i, k in enumerate(grads):
            grads[k].fill_(i)
        return torch.full_like(self.x, 7.0) if kw.get("need_dx") else None


def stubbed(name):
    """the net with StubEngine behind _make_engine, and the list of the engines made"""
    net = C.build(name)
    made = []

    def make():
        made.append(StubEngine(net))
        return made[-1]
    net._make_engine = make
    return net, made


def apply_node(net, x, dp, need_grad):
    from dlib.models.engine_net import NetFn
    return NetFn.apply(x, net, dp, need_grad, *[p for _, p in net.named_parameters()])


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_keys_and_parameter_order(name):
    net = C.build(name)
    assert sorted([k, list(v.shape)] for k, v in net.state_dict().items()) == KEYS[name]["state_dict"]
    assert [k for k, _ in net.named_parameters()] == KEYS[name]["named_parameters"]


@pytest.mark.parametrize("name", NAMES)
def test_engine_is_lazy_dropped_by_apply_and_invalidated(name):
    net, made = stubbed(name)
    sd = net.state_dict()
    assert net._engine is None and not made
    net.load_state_dict(sd)                     # no engine yet: nothing to invalidate, none made
    net.weights_changed()
    assert net._engine is None and not made
    eng = net.engine
    assert net.engine is eng and net._engine is eng and len(made) == 1
    net.load_state_dict(sd)
    assert eng.calls == ["invalidate"]
    net.weights_changed()
    assert eng.calls == ["invalidate"] * 2
    net.float()
    assert net._engine is None
    assert net.engine is made[1] and len(made) == 2
    net.to("cpu")
    assert net._engine is None and net.engine is made[2] and len(made) == 3


@pytest.mark.parametrize("name", NAMES)
def test_cpu_tensor_raises_with_the_nets_name(name):
    net, _ = stubbed(name)
    with pytest.raises(RuntimeError, match=rf"^{C.NETS[name][3]} \(libsrhip\) runs on the GPU only.*no CPU fallback"):
        net(torch.zeros(1, 1, 16, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.eval()(torch.zeros(1, 1, 16, 16))


@pytest.mark.parametrize("x_grad", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_netfn_hands_gradients_back_in_parameter_order(name, x_grad):
    net, made = stubbed(name)
    named = list(net.named_parameters())
    x = torch.rand(2, 8, 8, requires_grad=x_grad)
    dp = torch.ones(1)
    out = apply_node(net, x, dp, True)
    eng = made[0]
    assert eng.calls == [("forward", dp, True)] and len(made) == 1
    if name == "MSLapSRN":
        y, *inter = out
        assert len(inter) == 2 and all(torch.equal(a, b) and a is not b for a, b in zip(inter, eng.intermediate_outs))
        loss = (y * 2).sum() + (inter[1] * 5).sum()             # inter[0] stays without a gradient
    else:
        assert isinstance(out, torch.Tensor)                     # ProSR, SRFBN: one tensor on the module path
        y, loss = out, (out * 2).sum()
    assert y.shape == (2, 1, 8 * net.upscale, 8 * net.upscale)
    wanted = [(i, p) for i, (_, p) in enumerate(named) if p.requires_grad]
    got = torch.autograd.grad(loss, [p for _, p in wanted] + ([x] if x_grad else []), allow_unused=True)
    assert eng.calls[1:] == ["backward"]
    assert list(eng.grads) == [k for k, _ in named]
    assert all(eng.grads[k].shape == p.shape for k, p in named)
    for (i, p), g in zip(wanted, got):
        assert g.shape == p.shape and bool((g == i).all()), named[i][0]
    assert eng.dy.is_contiguous() and bool((eng.dy == 2).all())
    # the input gradient: asked of the two engines that compute one, and only when the input wants it
    if name in C.INPUT_GRAD:
        assert eng.backward_kw == {"need_dx": x_grad}
        if x_grad:
            assert bool((got[-1] == 7).all())
    else:
        assert "need_dx" not in eng.backward_kw
        if x_grad:
            assert got[-1] is None
    if name == "MSLapSRN":
        d_inter = eng.backward_kw.pop("d_inter")
        assert len(d_inter) == 2 and bool((d_inter[1] == 5).all()) and d_inter[1].is_contiguous()
        assert d_inter[0] is None or not d_inter[0].any()
    if name not in C.INPUT_GRAD:
        assert eng.backward_kw == {}                             # no other keyword reaches an engine


def test_dsr_splines_gradients_are_views_of_one_table():
    """the kernels' table layout: tensors in named_parameters() order, each padded to four floats, one buffer"""
    net, made = stubbed("DsrSplines")
    y = apply_node(net, torch.rand(1, 8, 8), None, True)
    y.sum().backward()
    grads, off = made[0].grads, 0
    base = next(iter(grads.values()))
    for k, p in net.named_parameters():
        g = grads[k]
        assert g.untyped_storage().data_ptr() == base.untyped_storage().data_ptr() and g.is_contiguous()
        assert g.storage_offset() == off and off % 4 == 0
        off += (p.numel() + 3) // 4 * 4
    assert base.untyped_storage().nbytes() == 4 * off
    other, made = stubbed("VDSR")
    apply_node(other, torch.rand(1, 8, 8), None, True).sum().backward()
    ptrs = {g.untyped_storage().data_ptr() for g in made[0].grads.values()}
    assert len(ptrs) == len(made[0].grads)                      # everyone else: a tensor of its own per parameter


@pytest.mark.parametrize("name", NAMES)
def test_amp_is_entered_for_inference_only(name):
    net, made = stubbed(name)
    x = torch.rand(1, 8, 8)
    assert lib.srhip_get_matmul_mode() == 0
    for amp, need_grad in ((True, False), (True, True), (False, False)):
        net.amp = amp
        with torch.no_grad():
            apply_node(net, x, None, need_grad)
        assert lib.srhip_get_matmul_mode() == 0
    assert [c[2] for c in made[0].calls] == [False, True, False]                # save = need_grad
    assert made[0].modes == [int(name != "DsrSplines"), 0, 0]


def test_base_class_registers_nothing():
    from dlib.models.engine_net import EngineNet
    assert all(isinstance(C.build(name), EngineNet) for name in NAMES)
    base = EngineNet()
    assert not list(base.state_dict()) and not list(base.children()) and not list(base.buffers())
