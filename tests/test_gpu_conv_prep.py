"""prepare() of the six conv engines: every 3x3 conv's forward pack (``name.wp``) and data-gradient twin (``name.wpt``) in
the engine's WeightSet against the same pack stated on its own -- a PrepTable of one job into fresh planes, or
ops.pack_conv_weight into fresh tensors on the exact-f32 kernels -- plus the key set and the rule of the cached job table:
rebuilt when a parameter moved, only re-run when its values changed.  prepare() alone: no image goes through a net."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BLOCK_KEYS = ("wq", "wqT", "wproj", "wpT", "w1", "w1T", "w2", "w2T")


def _edsr(nf):
    def make():
        from dlib.models.network_edsr_liif import EDSR_LIIF
        return EDSR_LIIF(scale=2, n_resblocks=1, n_feats=nf)

    def convs(net, eng):
        out = [("b0.0", net.body[0].body[0].weight.data, False), ("b0.2", net.body[0].body[2].weight.data, False),
               ("bend", net.body[1].weight.data, False), ("up0", net.tail[0][0].weight.data, eng.fuse_ps)]
        return out, set()
    return make, convs


def _vdsr():
    from dlib.models.network_vdsr import VDSR
    return VDSR(in_chans=1, upscale=2)


def _vdsr_convs(net, eng):
    return [(f"t{k}", net.trunk[k].conv.weight.data, False) for k in range(len(net.trunk))], set()


def _drrn():
    from dlib.models.network_drrn import DRRN
    return DRRN(in_chans=1, upscale=2, num_residual_units=2)


def _drrn_convs(net, eng):
    ru = net.trunk.residual_unit
    return [("wa", ru[1].weight.data, False), ("wb", ru[3].weight.data, False)], set()


def _mslapsrn():
    from dlib.models.network_mslapsr import MSLapSRN
    return MSLapSRN(upscale=2, in_chans=1)


def _mslapsrn_convs(net, eng):
    # the transposed conv behind the ten convs runs as a dense 3x3 conv + PixelShuffle(2): its weight is the derived "o0.wc"
    out = [(f"o0.c{k}", net.laplacian_pyramid_conv1[k].cl[0].weight.data, False) for k in range(10)]
    return out + [("o0.up", eng.derived.d["o0.wc"], True)], set()


def _memnet():
    from dlib.models.network_memnet import MemNet
    return MemNet(in_chans=1, upscale=2, num_memory_blocks=1, num_residual_blocks=1)


def _memnet_convs(net, eng):
    seq = net.dense_memory_blocks[0].recursive_unit[0].residual_block
    return [("m0.u0.c0", seq[2].weight.data, False), ("m0.u0.c1", seq[5].weight.data, False)], {"m0.gw", "m0.gwt"}


def _swinir(dim, **kw):
    def make():
        from dlib.models.network_swinir import SwinIR
        return SwinIR(upscale=2, in_chans=1, img_size=16, window_size=8, depths=[2], embed_dim=dim, num_heads=[6], mlp_ratio=2,
                      upsampler="pixelshuffledirect", **kw)

    def convs(net, eng):
        other = {f"{i}.{k}" for i in range(2) for k in BLOCK_KEYS}
        up = ("up", net.upsample[0].weight.data, False)
        if not kw:
            return [("l0", net.layers[0].conv.weight.data, False), ("cab", net.conv_after_body.weight.data, False), up], other
        # '3conv': the outer convs of each residual connection, their C/4 channels zero-padded in the derived set
        D = eng.derived.d
        out = [(f"{n}.{j}", D[f"{n}.w{j}p"], False) for n in ("l0", "cab") for j in (0, 4)]
        return out + [up], other | {f"{n}.1.{k}" for n in ("l0", "cab") for k in ("w", "wT")}
    return make, convs


# id: (net, its convs as (name, weight, ps2) + the other keys of the WeightSet, SRHIP_MM, planes?)
CONFIGS = {
    "edsr16": (*_edsr(16), None, False),            # 16 < BX3_MIN_CHANNELS_NT: the exact-f32 packs
    "edsr64": (*_edsr(64), None, True),             # planes, the upsampler conv with the PixelShuffle fused
    "vdsr": (_vdsr, _vdsr_convs, None, True),
    "vdsr-f32": (_vdsr, _vdsr_convs, "f32", False),
    "drrn": (_drrn, _drrn_convs, None, True),
    "drrn-f32": (_drrn, _drrn_convs, "f32", False),
    "mslapsrn": (_mslapsrn, _mslapsrn_convs, None, True),
    "memnet": (_memnet, _memnet_convs, None, True),
    "swinir60": (*_swinir(60), None, True),
    "swinir60-f32": (*_swinir(60), "f32", False),
    "swinir180-3conv": (*_swinir(180, resi_connection="3conv"), None, True),
}
LITERAL_KEYS = {
    "drrn": {"wa.wp", "wa.wpt", "wb.wp", "wb.wpt"},
    "drrn-f32": {"wa.wp", "wa.wpt", "wb.wp", "wb.wpt"},
    "edsr16": {"b0.0.wp", "b0.0.wpt", "b0.2.wp", "b0.2.wpt", "bend.wp", "bend.wpt", "up0.wp", "up0.wpt"},
    "edsr64": {"b0.0.wp", "b0.0.wpt", "b0.2.wp", "b0.2.wpt", "bend.wp", "bend.wpt", "up0.wp", "up0.wpt"},
}


def _written(bx):
    """The int16 words of a Bx3 that the preparation writes: three bf16 planes (fmt 0), or two fp16 planes and, behind them,
    one f32 scale per weight output channel (fmt 1, prep.hip kind 4) -- the rest of that allocation is never read."""
    flat = bx.planes.view(-1)
    return flat if bx.fmt == 0 else flat[:2 * bx.rows * bx.planes.shape[2] + 2 * (bx.rows // 9)]


def _check_packs(ops, eng, convs, planes):
    dev = convs[0][1].device
    for name, w, ps2 in convs:
        co, ci = w.shape[:2]
        for key, data_grad, (rows, kd) in ((name + ".wp", False, (co, ci)), (name + ".wpt", True, (ci, co))):
            got = eng.ws[key]
            if planes:
                ref = ops.Bx3(9 * rows, kd, dev)
                tb = ops.PrepTable()
                tb.conv(w, ref, data_grad=data_grad, ps2=ps2)
                tb.build(dev).run()
                assert isinstance(got, ops.Bx3) and (got.rows, got.K, got.fmt) == (ref.rows, ref.K, ref.fmt), key
                assert torch.equal(_written(got), _written(ref)), key
            else:
                wp, wpt = torch.empty(9, co, ci, device=dev), torch.empty(9, ci, co, device=dev)
                ops.pack_conv_weight(w, wp, wpt)
                ref = wpt if data_grad else wp
                assert torch.is_tensor(got) and got.shape == ref.shape, key
                assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), key


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_conv_packs_keys_and_table_reuse(cfg, monkeypatch):
    from srhip import ops
    make, conv_list, mm, planes = CONFIGS[cfg]
    if mm is None:
        monkeypatch.delenv("SRHIP_MM", raising=False)
    else:
        monkeypatch.setenv("SRHIP_MM", mm)
    builds = []
    build = ops.PrepTable.build
    monkeypatch.setattr(ops.PrepTable, "build", lambda self, device: builds.append(1) or build(self, device))
    torch.manual_seed(11)
    net = make().cuda()
    eng = net.engine
    assert eng.ws.use_bx3 == planes
    if cfg == "edsr64":
        assert eng.fuse_ps

    def prepare_builds():
        """the job tables one prepare() builds (the statements of _check_packs build their own)"""
        del builds[:]
        eng.prepare()
        return len(builds)

    assert prepare_builds() == int(planes) and eng.prepared
    convs, other = conv_list(net, eng)
    # 1. every pack; 2. the key set
    _check_packs(ops, eng, convs, planes)
    keys = {n + s for n, _, _ in convs for s in (".wp", ".wpt")}
    assert {k for k in eng.ws.d if k.endswith((".wp", ".wpt"))} == keys
    assert set(eng.ws.d) == keys | other
    if cfg in LITERAL_KEYS:
        assert set(eng.ws.d) == LITERAL_KEYS[cfg]

    # 3. new values in the same storage: the table is kept, the packs follow
    for p in net.parameters():
        p.data.mul_(2)
    eng.invalidate()
    assert not eng.prepared
    assert prepare_builds() == 0 and eng.prepared
    _check_packs(ops, eng, conv_list(net, eng)[0], planes)

    # 4. one conv weight in new storage: exactly one new table
    p = [q for q in net.parameters() if q.dim() == 4 and tuple(q.shape[2:]) == (3, 3) and q.shape[1] > 1][-1]
    p.data = p.data.clone()
    eng.invalidate()
    assert prepare_builds() == int(planes)
    _check_packs(ops, eng, conv_list(net, eng)[0], planes)
    torch.cuda.synchronize()
