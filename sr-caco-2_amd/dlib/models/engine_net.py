"""What every net mirror shares.  A mirror is an ``nn.Module`` that holds the reference's parameters under the reference's
names and hands the arithmetic to an engine of ``srhip/``: ``EngineNet`` carries that protocol once, ``NetFn`` is the one
autograd node of the module path (the training loop in ModelPlain drives the engines directly: srhip/train.py)."""
import torch
import torch.nn as nn

from srhip.module_path import refresh_if_params_changed

__all__ = ['EngineNet', 'TapeNet', 'NetFn']


class NetFn(torch.autograd.Function):
    """The whole network as one node: ``(x, net, dp, need_grad, *params)``.  What differs between the nets -- the input
    gradient, extra outputs, the gradients' storage, --amp -- is asked of the mirror (EngineNet's hooks).

    --amp (net.amp) is inference only; training stays f32-accurate.  Under it the convs run ONE product of the operands'
    leading fp16 planes (11 significant bits under the block exponents), the plain conv family on fp16 storage -- PSNR within
    0.003 dB of the f32-accurate forward on the seeded-weights check (gate 0.01 dB, tests/test_gpu_amp.py; with one bf16
    product, round 2, VDSR was 0.023 dB off)."""

    @staticmethod
    def forward(ctx, x, net, dp, need_grad, *params):
        ctx.net = net
        ctx.need_dx = net.input_grad and x.requires_grad
        y = net.engine_forward(x, dp, need_grad)
        extra = net.extra_outputs()
        ctx.has_extra = extra is not None
        if need_grad:
            y = y.clone()
        return y if extra is None else (y, *extra)

    @staticmethod
    def backward(ctx, dy, *d_extra):
        net = ctx.net
        grads = net.grad_buffers()
        kw = {}
        if net.input_grad:
            kw["need_dx"] = ctx.need_dx
        if ctx.has_extra:
            kw["d_inter"] = [None if g is None else g.contiguous() for g in d_extra]
        dx = net.engine.backward(dy.contiguous(), grads, **kw)
        return (dx if net.input_grad else None, None, None, None) + tuple(grads[k] for k, _ in net.named_parameters())


class EngineNet(nn.Module):
    """Lazy engine, its invalidation, and the forward of the module path.  A subclass adds its parameter holders, its
    constructor checks and ``_make_engine``; it registers nothing of its own here.

    What train.py, model_plain.py, predict.py and bench.py read
      from a mirror: ``amp`` (--amp: reduced-precision evaluation forwards), ``amp_takes_effect`` (False where --amp changes
        nothing), ``eval_graph_default`` (evaluation replays a hipGraph unless told otherwise), ``forward_divides_by_img_range``,
        ``intermediate_outs`` (the multi-scale losses), ``mean``, ``img_range``; ``engine`` / ``_engine``, ``weights_changed``,
        ``sample_drop_path``, ``prepare_input``, ``flush``;
      from an engine: what the docstring of ``Engine`` states (srhip/engine.py).

    Hooks of NetFn (each with the one or two nets that override it): ``input_grad`` (SwinIR, EDSR: the engine returns dx),
    ``extra_outputs`` (MSLapSRN), ``grad_buffers`` and ``engine_forward`` (DSR-Splines)."""
    display_name = None         # the net's name in the GPU-only message where it is not the class name
    amp = False
    input_grad = False

    def __init__(self):
        super().__init__()
        self._engine = None

    @property
    def engine(self):
        if self._engine is None:
            self._engine = self._make_engine()
        return self._engine

    def _apply(self, fn, *a, **k):   # .cuda() / .to(): parameter storage moves
        out = super()._apply(fn, *a, **k)
        self._engine = None
        return out

    def load_state_dict(self, *a, **k):
        out = super().load_state_dict(*a, **k)
        if self._engine is not None:
            self._engine.invalidate()
        return out

    def weights_changed(self):
        """Call after parameters were modified in place (optimizer step)."""
        if self._engine is not None:
            self._engine.invalidate()

    def sample_drop_path(self, batch, device):
        return None

    def flush(self):
        pass

    def check_input(self, x):
        if not x.is_cuda:
            raise RuntimeError(f"{self.display_name or type(self).__name__} (libsrhip) runs on the GPU only: move the model "
                               f"and the input to cuda; there is no CPU fallback")
        assert x.dim() == 4 and x.shape[1] == self.in_chans, f'c: {x.shape}, img-nc: {self.in_chans}'

    def prepare_input(self, x):
        self.check_input(x)
        return x.float().contiguous()[:, 0], x.shape[2], x.shape[3]

    def forward(self, x):
        self.flush()
        return self.run(self.prepare_input(x)[0])

    def run(self, xi, dp=None):
        """NetFn over a prepared input"""
        params = [p for _, p in self.named_parameters()]
        need_grad = self.need_grad(xi, params)
        refresh_if_params_changed(self, params)   # stock torch.optim wrote the weights?
        return NetFn.apply(xi, self, dp, need_grad, *params)

    def need_grad(self, xi, params):
        return torch.is_grad_enabled() and ((self.input_grad and xi.requires_grad) or any(p.requires_grad for p in params))

    # -- NetFn's hooks
    def engine_forward(self, xi, dp, need_grad):
        from srhip import ops
        with ops.amp_inference(self.amp and not need_grad):
            return self.engine.forward(xi, dp, save=need_grad)

    def extra_outputs(self):
        """further outputs of the node (their gradients reach engine.backward as d_inter), or None"""
        return None

    def grad_buffers(self):
        return {k: torch.empty_like(p) for k, p in self.named_parameters()}


class TapeNet(EngineNet):
    """The tape-engine mirrors (srhip/tape.py): one channel, one scale."""

    def _init_protocol(self, upscale, in_chans):
        if in_chans != 1:
            raise NotImplementedError(f"{type(self).__name__} on libsrhip: 1-channel microscopy patches only")
        self.upscale, self.scale, self.in_chans = upscale, upscale, in_chans
