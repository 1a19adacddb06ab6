"""The module path of the seventeen net mirrors (dlib/models/engine_net.py) adds nothing to the engine's arithmetic: at
B = 2, 16 x 16 LR patches, x2, ``net(x)`` / ``.backward()`` in training mode, the --amp evaluation forward and the forward
behind a stock torch.optim step carry the same bits as the engine driven directly.  The engines' reductions run in a fixed
order, so the gate is equality; there is no tolerance.  Both runs of a pair see the same inputs: NLSN draws its hash
rotations with torch.randn at every forward, so the generator is seeded in front of each; OmniSR and GRL sum the gradients of
their bias tables with torch's index_add_, which adds with atomics unless torch's deterministic algorithms are on -- they are
on for the length of a test."""
import pytest
import torch

import net_protocol_cases as C

pytestmark = pytest.mark.gpu

# engine.last_eval_path behind the --amp evaluation forward (None: the engine does not say)
# (recorded at these configurations before the mirrors shared a base class)
LAST_EVAL_PATH = dict.fromkeys(C.NETS)
LAST_EVAL_PATH.update(dict.fromkeys(("VDSR", "DRRN", "SRCNN", "MSLapSRN", "MemNet"), "fp16 storage"))
LAST_EVAL_PATH["ENLCN"] = "fp16 storage (attention blocks f32)"


@pytest.fixture(autouse=True)
def deterministic_torch_ops():
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    yield
    torch.use_deterministic_algorithms(was, warn_only=warn)


def seeded(fn, *a, **k):
    torch.manual_seed(11)
    return fn(*a, **k)


def on_gpu(name, state=None):
    net = C.build(name)
    if state is not None:
        net.load_state_dict(state)
    return net.cuda()


@pytest.mark.parametrize("name", list(C.NETS))
def test_module_path_carries_the_engines_bits(name):
    from srhip import ops
    gen = torch.Generator().manual_seed(7)
    x = torch.rand(2, 1, 16, 16, generator=gen).cuda()
    net = on_gpu(name).train()
    ref = on_gpu(name, net.state_dict()).train()
    named = list(net.named_parameters())
    want_dx = name in C.INPUT_GRAD

    # training mode: forward and backward
    x.requires_grad_(want_dx)
    y = seeded(net, x)
    g = torch.rand(y.shape, generator=gen).cuda()
    (y * g).sum().backward()
    xi = ref.prepare_input(x.detach())[0]
    yd = seeded(ref.engine.forward, xi, None, save=True)
    assert torch.equal(y, yd), f"{name}: training forward"
    grads = {k: torch.empty_like(p) for k, p in named}
    dx = ref.engine.backward(g, grads, need_dx=True) if want_dx else ref.engine.backward(g, grads)
    for k, p in named:
        if p.requires_grad:
            assert torch.equal(p.grad, grads[k]), f"{name}: gradient of {k}"
    if want_dx:
        assert torch.equal(x.grad, dx.view_as(x)), f"{name}: input gradient"
    x = x.detach()

    # --amp evaluation
    net.eval().amp = True
    ref.eval()
    with torch.no_grad():
        ya = seeded(net, x)
        with ops.amp_inference(True):
            yd = seeded(ref.engine.forward, xi, None, save=False)
    print(f"last_eval_path {name!r}: {getattr(net.engine, 'last_eval_path', None)!r}")
    assert torch.equal(ya, yd), f"{name}: --amp evaluation forward"
    assert getattr(net.engine, "last_eval_path", None) == LAST_EVAL_PATH[name]
    net.train().amp = False

    # a stock optimizer writes the weights (no entry moves by more than 0.01): the next forward sees them
    trained = [p for _, p in named if p.requires_grad]
    lr = 0.01 / max(p.grad.abs().max().item() for p in trained)
    torch.optim.SGD(trained, lr=lr).step()
    fresh = on_gpu(name, net.state_dict()).train()
    with torch.no_grad():
        y2 = seeded(net, x)
        yf = seeded(fresh.engine.forward, xi, None, save=False)
    assert bool(torch.isfinite(y2).all()) and not torch.equal(y2, y), f"{name}: the step changed nothing, or too much"
    assert torch.equal(y2, yf), f"{name}: forward behind optimizer.step()"
