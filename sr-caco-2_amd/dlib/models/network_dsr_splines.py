"""DSR-Splines on libsrhip (reference dlib/models/network_dsr_splines.py:283-413; registry select_network.py):
same constructor, ``forward((B,1,h,w) in [0,1]) -> (B,1,s*h,s*w)``, state_dict keys in the reference's order
(``splines.{k}.model.{i}.conv.weight|bias``, then ``...match_sz.weight|bias`` where use_local_residual gives the layer a
1x1 conv) and torch's default Conv2d initialisation; the compute is ``srhip.dsr_splines_engine.DsrSplinesEngine``
(one spline net per pixel, chosen by the pixel's grey level).  1-channel inputs; GPU only (CPU tensors raise)."""
import numpy as np
import torch
import torch.nn as nn

from dlib.utils import constants
from srhip.module_path import refresh_if_params_changed

__all__ = ['DsrSplines']


class _Layer(nn.Module):
    """Parameter holder of the reference's _Layer (:40-93): conv, and match_sz (a biased 1x1 conv where the widths differ,
    the identity where they agree) under use_local_residual.  nn.Conv2d supplies the keys, shapes and initialisation."""

    def __init__(self, in_planes, out_planes, ksz, use_local_residual):
        super().__init__()
        self.conv = nn.Conv2d(in_planes, out_planes, ksz, padding=(ksz - 1) // 2, bias=True, padding_mode='reflect')
        if use_local_residual:
            self.match_sz = nn.Conv2d(in_planes, out_planes, 1, bias=True) if in_planes != out_planes else nn.Identity()
        else:
            self.match_sz = None


class _SplineNet(nn.Module):
    def __init__(self, in_planes, h_layers, in_ksz, knots, use_local_residual):
        super().__init__()
        self.knots = knots
        widths = [in_planes] + list(h_layers) + [in_planes]
        self.model = nn.Sequential(*[_Layer(widths[i], widths[i + 1], in_ksz if i == 0 else 1, use_local_residual)
                                     for i in range(len(widths) - 1)])


class _NetFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, net, need_grad, *params):
        ctx.net = net
        y = net.engine.forward(x, None, save=need_grad)      # --amp evaluation runs the same float32 kernels
        return y.clone() if need_grad else y

    @staticmethod
    def backward(ctx, dy):
        net = ctx.net
        eng = net.engine
        # the gradients as views of one buffer in the kernels' table layout: written in place by one launch
        flat = torch.empty(eng.n * eng.P, device=dy.device)
        grads, off = {}, 0
        for k, p in net.named_parameters():
            grads[k] = flat[off:off + p.numel()].view_as(p)
            off += (p.numel() + 3) // 4 * 4
        eng.backward(dy.contiguous(), grads)
        return (None, None, None) + tuple(grads[k] for k in eng.names)


class DsrSplines(nn.Module):
    def __init__(self, upscale: int, in_planes: int, in_ksz: int, splinenet_type: str, n_splines_per_color: int,
                 use_global_residual: bool, use_local_residual: bool, color_min: int = 0, color_max: int = 255) -> None:
        super().__init__()
        assert isinstance(upscale, int) and upscale > 0, upscale
        assert isinstance(in_planes, int) and in_planes > 0, in_planes
        assert isinstance(in_ksz, int) and in_ksz > 0 and in_ksz % 2 == 1, in_ksz
        assert splinenet_type in constants.SPLINE_NET_TYPES, splinenet_type
        assert isinstance(n_splines_per_color, int) and n_splines_per_color > 0, n_splines_per_color
        assert isinstance(use_global_residual, bool) and isinstance(use_local_residual, bool)
        if in_planes != 1:
            raise NotImplementedError("DSR-Splines on libsrhip: 1-channel microscopy patches only")
        if (color_min, color_max) != (0, 255):
            raise NotImplementedError("DSR-Splines on libsrhip: grey levels 0 ... 255 only")
        if in_ksz > 15:
            raise NotImplementedError(f"DSR-Splines on libsrhip: in_ksz {in_ksz} (odd, 1 ... 15)")
        assert n_splines_per_color <= 256, n_splines_per_color
        self.upscale, self.scale, self.in_planes, self.in_chans = upscale, upscale, in_planes, in_planes
        self.in_ksz, self.splinenet_type = in_ksz, splinenet_type
        self.n_splines_per_color = n_splines_per_color
        self.use_global_residual, self.use_local_residual = use_global_residual, use_local_residual
        self.color_min, self.color_max = color_min, color_max
        self.h_layers = list(constants.SPLINEHIDDEN[splinenet_type])
        # the bins of the grey levels (network_dsr_splines.py:342-360): one spline each
        splits = np.array_split(np.arange(color_min, color_max + 1), n_splines_per_color)
        self.knots = [[(int(s.min()), int(s.max()))] for s in splits]
        self.splines = nn.ModuleList([_SplineNet(in_planes, self.h_layers, in_ksz, kn, use_local_residual)
                                      for kn in self.knots])
        self.n_splines = len(self.knots)
        self.global_residual = None
        self.x_interp = None
        self._engine = None

    def flush(self):
        """The reference's save path calls it (it drops the masks and predictions kept by the forward): nothing is kept here."""
        self.global_residual = None
        self.x_interp = None

    @property
    def engine(self):
        if self._engine is None:
            from srhip.dsr_splines_engine import DsrSplinesEngine
            self._engine = DsrSplinesEngine(self)
        return self._engine

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self._engine = None
        return out

    def load_state_dict(self, *a, **k):
        out = super().load_state_dict(*a, **k)
        if self._engine is not None:
            self._engine.invalidate()
        return out

    def weights_changed(self):
        if self._engine is not None:
            self._engine.invalidate()

    def sample_drop_path(self, batch, device):
        return None

    def prepare_input(self, x):
        if not x.is_cuda:
            raise RuntimeError("DSR-Splines (libsrhip) runs on the GPU only: move the model and the input to cuda; "
                               "there is no CPU fallback")
        assert x.dim() == 4 and x.shape[1] == self.in_planes, f'c: {x.shape}, img-nc: {self.in_planes}'
        return x.float().contiguous()[:, 0], x.shape[2], x.shape[3]

    def forward(self, x):
        self.flush()
        xi, h, w = self.prepare_input(x)
        params = [p for _, p in self.named_parameters()]
        need_grad = torch.is_grad_enabled() and any(p.requires_grad for p in params)
        refresh_if_params_changed(self, params)   # stock torch.optim wrote the weights?
        return _NetFn.apply(xi, self, need_grad, *params)
