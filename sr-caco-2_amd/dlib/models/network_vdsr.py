"""VDSR on libsrhip (reference dlib/models/network_vdsr.py:24-126; registry select_network.py:200-205):
same constructor, ``forward((B,1,h,w) in [0,1]) -> (B,1,s*h,s*w)``, state_dict keys ``conv1.0.weight``,
``trunk.{k}.conv.weight`` (18), ``conv2.weight`` and the reference's weight initialisation; the compute is
``srhip.vdsr_engine.VDSREngine``.  1-channel inputs; GPU only (CPU tensors raise)."""
from math import sqrt

import torch
import torch.nn as nn

from dlib.models.engine_net import EngineNet

__all__ = ['VDSR']


class _Conv(nn.Module):
    def __init__(self, co, ci):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(co, ci, 3, 3))


class ConvReLU(nn.Module):
    def __init__(self, channels):
        super().__init__()
        self.conv = _Conv(channels, channels)


class VDSR(EngineNet):
    def __init__(self, in_chans: int, upscale: int) -> None:
        super().__init__()
        assert isinstance(upscale, int) and upscale > 0, upscale
        assert isinstance(in_chans, int) and in_chans > 0, in_chans
        if in_chans != 1:
            raise NotImplementedError("VDSR on libsrhip: 1-channel microscopy patches only")
        self.upscale, self.scale, self.in_chans = upscale, upscale, in_chans
        self.global_residual = None
        self.x_interp = None
        self.conv1 = nn.ModuleList([_Conv(64, in_chans)])            # + ReLU (network_vdsr.py:57-60)
        self.trunk = nn.ModuleList([ConvReLU(64) for _ in range(18)])
        self.conv2 = _Conv(in_chans, 64)
        self._initialize_weights()

    def _initialize_weights(self):                                    # network_vdsr.py:121-126
        for m in self.modules():
            if isinstance(m, _Conv):
                m.weight.data.normal_(0.0, sqrt(2 / (3 * 3 * m.weight.shape[0])))

    def flush(self):
        self.global_residual = None
        self.x_interp = None

    def _make_engine(self):
        from srhip.vdsr_engine import VDSREngine
        return VDSREngine(self)
