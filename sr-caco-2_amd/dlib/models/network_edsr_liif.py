"""EDSR-baseline on libsrhip, registered as ``EDSR_LIIF``.

The reference's ``network_edsr_liif.py`` is absent from its tree
(select_network.py:39-50 imports a missing file; SURVEY.md section "Five facts",
item 2), so this network follows the EDSR building blocks the reference does
ship (default_conv / ResBlock / Upsampler, network_nlsn.py:38-128) wired as
NLSN.forward without the attention modules (:355-369), with the EDSR-baseline
sizes of utils_init_default_args.py:37-50 (64 feats, 16 blocks, res_scale 1).
The LIIF implicit decoder has no reference source and no test: it is NOT
reproduced (parity unpinned); the tail is the pixel-shuffle Upsampler.
state_dict keys: head.0, body.{k}.body.{0,2}, body.{N}, tail.0.{0,2,..}, tail.1.
GPU only; CPU tensors raise.
"""
import math

import torch
import torch.nn as nn

from dlib.models.engine_net import EngineNet

__all__ = ['EDSR_LIIF', 'EDSR']


class _Box(nn.Module):
    pass


def _conv3(co, ci):
    m = _Box()
    bound = 1.0 / math.sqrt(ci * 9)
    m.weight = nn.Parameter((torch.rand(co, ci, 3, 3) * 2 - 1) * bound)
    m.bias = nn.Parameter((torch.rand(co) * 2 - 1) * bound)
    return m


class EDSR_LIIF(EngineNet):
    display_name = "EDSR"
    input_grad = True           # the engine hands back dx

    def __init__(self, in_chans=1, n_resblocks=16, n_feats=64, scale=2, rgb_range=1.,
                 local_ensemble=True, feat_unfold=True, cell_decode=True, res_scale=1., **kwargs):
        super().__init__()
        if in_chans != 1:
            raise NotImplementedError("EDSR on libsrhip: 1-channel microscopy patches only")
        if scale & (scale - 1) or scale < 2:
            raise NotImplementedError("EDSR on libsrhip: scale must be a power of two")
        if n_feats % 4 or n_feats > 256:
            raise NotImplementedError("EDSR on libsrhip: n_feats must be a multiple of 4, <= 256")
        self.in_chans, self.n_resblocks, self.n_feats = in_chans, n_resblocks, n_feats
        self.scale, self.upscale, self.res_scale, self.img_range = scale, scale, res_scale, rgb_range
        self.head = nn.ModuleList([_conv3(n_feats, in_chans)])
        body = []
        for _ in range(n_resblocks):
            rb = _Box()
            rb.body = nn.ModuleList([_conv3(n_feats, n_feats), nn.Identity(), _conv3(n_feats, n_feats)])
            body.append(rb)
        body.append(_conv3(n_feats, n_feats))
        self.body = nn.ModuleList(body)
        up = []
        for _ in range(int(math.log2(scale))):
            up += [_conv3(4 * n_feats, n_feats), nn.Identity()]
        self.tail = nn.ModuleList([nn.ModuleList(up), _conv3(in_chans, n_feats)])

    def _make_engine(self):
        from srhip.edsr_engine import EDSREngine
        return EDSREngine(self)


EDSR = EDSR_LIIF
