"""DSR-Splines on libsrhip (reference dlib/models/network_dsr_splines.py:283-413; registry select_network.py):
same constructor, ``forward((B,1,h,w) in [0,1]) -> (B,1,s*h,s*w)``, state_dict keys in the reference's order
(``splines.{k}.model.{i}.conv.weight|bias``, then ``...match_sz.weight|bias`` where use_local_residual gives the layer a
1x1 conv) and torch's default Conv2d initialisation; the compute is ``srhip.dsr_splines_engine.DsrSplinesEngine``
(one spline net per pixel, chosen by the pixel's grey level).  1-channel inputs; GPU only (CPU tensors raise)."""
import numpy as np
import torch
import torch.nn as nn

from dlib.utils import constants
from dlib.models.engine_net import EngineNet

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


class DsrSplines(EngineNet):
    display_name = "DSR-Splines"

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

    def flush(self):
        """The reference's save path calls it (it drops the masks and predictions kept by the forward): nothing is kept here."""
        self.global_residual = None
        self.x_interp = None

    def _make_engine(self):
        from srhip.dsr_splines_engine import DsrSplinesEngine
        return DsrSplinesEngine(self)

    def engine_forward(self, xi, dp, need_grad):
        return self.engine.forward(xi, dp, save=need_grad)      # --amp evaluation runs the same float32 kernels

    def grad_buffers(self):
        """The gradients as views of one buffer in the kernels' table layout (each tensor padded to four floats): written in
        place by one launch."""
        named = list(self.named_parameters())
        flat = torch.empty(sum((p.numel() + 3) // 4 * 4 for _, p in named), device=named[0][1].device)
        grads, off = {}, 0
        for k, p in named:
            grads[k] = flat[off:off + p.numel()].view_as(p)
            off += (p.numel() + 3) // 4 * 4
        return grads
