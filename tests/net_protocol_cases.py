"""The seventeen registry nets at the smallest configurations the suite builds elsewhere (x2 where a net has a scale,
drop-path and dropout rates 0), shared by tests/test_cpu_net_protocol.py and tests/test_gpu_net_protocol.py."""

GRL_KW = dict(in_chans=1, window_size=8, mlp_ratio=2, qkv_proj_type="linear", anchor_proj_type="avgpool",
              anchor_window_down_factor=2, out_proj_type="linear", conv_type="1conv", upsampler="pixelshuffle",
              local_connection=True)

# name: (module, class, constructor keywords, the name in the "no CPU fallback" message)
NETS = {
    "SwinIR": ("network_swinir", "SwinIR", dict(upscale=2, in_chans=1, img_size=16, window_size=8, depths=[2], embed_dim=60,
                                                 num_heads=[6], mlp_ratio=2, upsampler="pixelshuffledirect", drop_path_rate=0.0),
               "SwinIR"),
    "EDSR_LIIF": ("network_edsr_liif", "EDSR_LIIF", dict(scale=2, n_resblocks=1, n_feats=16), "EDSR"),
    "VDSR": ("network_vdsr", "VDSR", dict(in_chans=1, upscale=2), "VDSR"),
    "DRRN": ("network_drrn", "DRRN", dict(in_chans=1, upscale=2, num_residual_units=2), "DRRN"),
    "SRCNN": ("network_srcnn", "SRCNN", dict(in_chans=1), "SRCNN"),
    "MSLapSRN": ("network_mslapsr", "MSLapSRN", dict(upscale=2, in_chans=1), "MSLapSRN"),
    "MemNet": ("network_memnet", "MemNet", dict(in_chans=1, upscale=2, num_memory_blocks=1, num_residual_blocks=1), "MemNet"),
    "DBPN": ("network_dbpn", "DBPN", dict(upscale=2, in_chans=1, base_filter=16, feat=32, num_stages=2), "DBPN"),
    "SRFBN": ("network_srfbn", "SRFBN", dict(upscale=2, in_chans=1, num_features=16, num_steps=3, num_groups=3), "SRFBN"),
    "ProSR": ("network_prosr", "ProSR", dict(upscale=2, in_chans=1, num_init_features=32, bn_size=2, growth_rate=8,
                                             level_config=[[3, 2]]), "ProSR"),
    "ENLCN": ("network_enlcn", "ENLCN", dict(upscale=2, in_chans=1, n_resblock=8, n_feats=64), "ENLCN"),
    "NLSN": ("network_nlsn", "NLSN", dict(upscale=2, in_chans=1, n_resblocks=8, n_feats=64), "NLSN"),
    "DFCAN": ("network_dfcan", "DFCAN", dict(input_shape=1, upscale=2), "DFCAN"),
    "ACT": ("network_act", "ACT", dict(upscale=2, in_chans=1, n_feats=16, n_resgroups=4, n_resblocks=2, reduction=4, n_heads=4,
                                       n_layers=8, n_fusionblocks=4), "ACT"),
    "OmniSR": ("network_omni_sr", "OmniSR", dict(input_shape=1, upscale=2, num_feat=16, res_num=2, block_num=1), "OmniSR"),
    "GRL": ("network_grl", "GRL", dict(upscale=2, img_size=16, depths=[2, 2], embed_dim=36, num_heads_window=[3, 3],
                                       num_heads_stripe=[3, 3], drop_path_rate=0.0, **GRL_KW), "GRL"),
    "DsrSplines": ("network_dsr_splines", "DsrSplines", dict(upscale=2, in_planes=1, in_ksz=5, splinenet_type="snet_type2",
                                                             n_splines_per_color=2, use_global_residual=True,
                                                             use_local_residual=True), "DSR-Splines"),
}
INPUT_GRAD = ("SwinIR", "EDSR_LIIF")         # the engines that hand back the gradient of the input


def build(name, seed=0):
    import importlib

    import torch
    mod, cls, kw, _ = NETS[name]
    torch.manual_seed(seed)
    return getattr(importlib.import_module(f"dlib.models.{mod}"), cls)(**kw)
