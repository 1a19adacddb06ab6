"""SRCNN on libsrhip.

Drop-in for the reference's registered ``dlib.models.network_srcnn.SRCNN`` (network_srcnn.py:23-69,
select_network.py:207-210): ctor ``(in_chans)``, ``forward(x)`` on an input that is already at the
target resolution, ``state_dict`` keys ``features.0 / map.0 / reconstruction`` (+ ``.weight/.bias``), the
reference's initialisation law.  The module holds parameters only; ``forward`` runs
srhip/srcnn_engine.py (GEMMs on the bf16x3 kernels); CPU tensors raise."""
import math

import torch
import torch.nn as nn

from dlib.models.engine_net import EngineNet

__all__ = ['SRCNN']


class _Conv(nn.Module):
    def __init__(self, co, ci, k):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(co, ci, k, k))
        self.bias = nn.Parameter(torch.zeros(co))


class SRCNN(EngineNet):
    def __init__(self, in_chans: int) -> None:
        super().__init__()
        assert isinstance(in_chans, int) and in_chans > 0, in_chans
        if in_chans != 1:
            raise NotImplementedError("SRCNN on libsrhip: 1-channel microscopy patches only")
        self.in_chans, self.scale, self.upscale, self.img_range = in_chans, 1, 1, 1.
        self.features = nn.ModuleList([_Conv(1024, in_chans, 5)])        # + ReLU
        self.map = nn.ModuleList([_Conv(128, 1024, 1)])                  # + ReLU
        self.reconstruction = _Conv(in_chans, 128, 1)
        self._initialize_weights()

    def _initialize_weights(self):                                       # network_srcnn.py:63-72
        for m in (self.features[0], self.map[0], self.reconstruction):
            co, k2 = m.weight.shape[0], m.weight.shape[2] * m.weight.shape[3]
            nn.init.normal_(m.weight.data, 0.0, math.sqrt(2 / (co * k2)))
            nn.init.zeros_(m.bias.data)
        nn.init.normal_(self.reconstruction.weight.data, 0.0, 0.001)
        nn.init.zeros_(self.reconstruction.bias.data)

    def _make_engine(self):
        from srhip.srcnn_engine import SRCNNEngine
        return SRCNNEngine(self)
