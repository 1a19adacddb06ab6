"""DRRN on libsrhip (reference dlib/models/network_drrn.py:22-126; registry select_network.py:192-198):
same constructor, ``forward((B,1,h,w) in [0,1]) -> (B,1,s*h,s*w)``, state_dict keys ``conv1.1.weight``,
``trunk.residual_unit.{1,3}.weight``, ``conv2.1.weight`` and the reference's Kaiming (fan_out, relu)
initialisation; the compute is ``srhip.drrn_engine.DRRNEngine``.  1-channel inputs; GPU only."""
import torch
import torch.nn as nn

from dlib.models.engine_net import EngineNet

__all__ = ['DRRN']


class _Conv(nn.Module):
    def __init__(self, co, ci):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(co, ci, 3, 3))


class RecursiveBlock(nn.Module):
    def __init__(self, num_channels, num_residual_unit):
        super().__init__()
        self.num_residual_unit = num_residual_unit
        # indices as in the reference's nn.Sequential(ReLU, Conv, ReLU, Conv)
        self.residual_unit = nn.ModuleList([nn.Identity(), _Conv(num_channels, num_channels), nn.Identity(),
                                            _Conv(num_channels, num_channels)])


class DRRN(EngineNet):
    def __init__(self, in_chans: int, upscale: int, num_residual_units: int):
        super().__init__()
        assert isinstance(upscale, int) and upscale > 0, upscale
        assert isinstance(in_chans, int) and in_chans > 0, in_chans
        if in_chans != 1:
            raise NotImplementedError("DRRN on libsrhip: 1-channel microscopy patches only")
        self.upscale, self.scale, self.in_chans = upscale, upscale, in_chans
        self.global_residual = None
        self.x_interp = None
        self.conv1 = nn.ModuleList([nn.Identity(), _Conv(128, in_chans)])
        self.trunk = RecursiveBlock(128, num_residual_units)
        self.conv2 = nn.ModuleList([nn.Identity(), _Conv(in_chans, 128)])
        self._initialize_weights()

    def _initialize_weights(self):                                    # network_drrn.py:128-136
        for m in self.modules():
            if isinstance(m, _Conv):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")

    def flush(self):
        self.global_residual = None
        self.x_interp = None

    def _make_engine(self):
        from srhip.drrn_engine import DRRNEngine
        return DRRNEngine(self)
