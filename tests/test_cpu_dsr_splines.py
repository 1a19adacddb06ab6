"""DSR-Splines without a GPU: the one-expert-per-pixel restatement (tests/dsr_splines_ref.py) against the reference's own
numbers (tests/golden/g53_dsr_splines.npz, tools/make_golden_dsr_splines.py), the module's state_dict layout, the registry,
the command line, the grey-level table and the library's exports.

Gates (the project's): forward <= 1e-5, gradients <= 2e-5 of the tensor's largest entry (+ 1e-12), index operations
bit-exact; the float64 restatement reproduces the reference's float64 run to 1e-12 relative."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dsr_splines_ref as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "g53_dsr_splines.npz")
CASES = ("A", "B", "C", "D")
_CACHE = {}


def load_case(name):
    """(cfg dict, arrays dict, state dict) of one golden case; computed once and shared."""
    if name not in _CACHE:
        import sr_oracle as O
        z = np.load(GOLDEN)
        pre = name + "/"
        a = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
        ksz, nh, n, local, glob, scale = (int(v) for v in a["cfg"])
        cfg = dict(in_ksz=ksz, nh=nh, n=n, local=bool(local), glob=bool(glob), scale=scale,
                   hidden=R.HIDDEN[f"snet_type{nh}"], snet=f"snet_type{nh}")
        # the reference's state_dict layout as stored, and the end-to-end gradient arrays cut along it
        lay = [(str(k), tuple(int(v) for v in s[:d])) for k, s, d in zip(a["keys"], a["shapes"], a["ndim"])]
        off = 0
        for k, shape in lay:
            m = int(np.prod(shape))
            a["grad/" + k], a["grad64/" + k] = a["grad"][off:off + m].reshape(shape), a["grad64"][off:off + m].reshape(shape)
            off += m
        assert off == a["grad"].size == a["grad64"].size
        _CACHE[name] = (cfg, a, O.seeded_state_dict(lay, int(a["seed"])), lay)
    return _CACHE[name]


def grad_err(g, ref):
    ref = torch.as_tensor(ref).double()
    return ((torch.as_tensor(g).double() - ref).abs().max() / (ref.abs().max() + 1e-12)).item()


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(name):
    cfg, a, sd, lay = load_case(name)
    x, xi, tgt = (torch.from_numpy(a[k]) for k in ("x", "x_interp", "tgt"))
    if name != "D":           # the edge margin makes the experts independent of the interpolation's last bits; D stores x_interp
        assert torch.equal(R.interpolate(x, cfg["scale"]), xi)
    ids = R.expert_ids(a["x_interp"], cfg["n"])[:, 0]
    assert np.array_equal(ids, a["ids"].astype(np.int64))
    args = (cfg["hidden"], cfg["in_ksz"], cfg["local"], cfg["glob"])
    y64, loss64, g64 = R.loss_and_grads(sd, xi, ids, tgt, *args, torch.float64)
    assert y64.dtype == torch.float64 and a["y64"].dtype == np.float64
    assert grad_err(y64, a["y64"]) <= 1e-12 and abs(loss64.item() - float(a["loss64"])) <= 1e-12 * abs(float(a["loss64"]))
    y32, loss32, g32 = R.loss_and_grads(sd, xi, ids, tgt, *args, torch.float32)
    assert (y32 - torch.from_numpy(a["y"])).abs().max().item() <= 1e-5
    assert abs(loss32.item() - float(a["loss"])) <= 1e-6
    owners = set(np.unique(ids).tolist())
    assert lay == R.layout(cfg["in_ksz"], cfg["hidden"], cfg["n"], cfg["local"])
    assert len(g64) == len(lay) == sum(k.startswith("grad64/") for k in a)
    for k, shape in lay:
        assert a["grad64/" + k].dtype == np.float64 and tuple(g64[k].shape) == shape
        assert grad_err(g64[k], a["grad64/" + k]) <= 1e-12, k
        assert grad_err(g32[k], a["grad/" + k]) <= 2e-5, k
        if int(k.split(".")[1]) not in owners:                      # an expert without pixels: exactly zero
            assert not a["grad/" + k].any() and not g32[k].any() and not g64[k].any(), k
        else:
            assert a["grad/" + k].any(), k
    if name in ("A", "D"):
        assert len(owners) < cfg["n"]


@pytest.mark.parametrize("name", CASES)
def test_module_state_dict_is_the_goldens_layout(name):
    from dlib.models.network_dsr_splines import DsrSplines
    cfg, a, sd, lay = load_case(name)
    net = DsrSplines(upscale=cfg["scale"], in_planes=1, in_ksz=cfg["in_ksz"], splinenet_type=cfg["snet"],
                     n_splines_per_color=cfg["n"], use_global_residual=cfg["glob"], use_local_residual=cfg["local"])
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == lay
    assert [k for k, _ in net.named_parameters()] == [k for k, _ in lay]
    net.load_state_dict(sd, strict=True)
    net.flush()                                                      # the reference's save path calls it
    with pytest.raises(RuntimeError, match="GPU only"):
        net(torch.zeros(1, 1, 4, 4))


def test_default_init_follows_conv2d():
    """torch's default Conv2d law: weights and biases within 1 / sqrt(fan_in), the same draws as nn.Conv2d makes."""
    from dlib.models.network_dsr_splines import DsrSplines
    torch.manual_seed(3)
    net = DsrSplines(2, 1, 5, "snet_type2", 2, True, True)
    torch.manual_seed(3)
    first = torch.nn.Conv2d(1, 32, 5, padding=2, padding_mode='reflect')
    assert torch.equal(net.splines[0].model[0].conv.weight, first.weight) and torch.equal(net.splines[0].model[0].conv.bias, first.bias)
    for k, p in net.named_parameters():
        fan_in = p[0].numel() if p.dim() > 1 else dict(net.named_parameters())[k[:-4] + "weight"][0].numel()
        assert p.abs().max().item() <= fan_in ** -0.5 + 1e-7, k


def test_registry_builds_the_default_net():
    from dlib.models.select_network import define_G
    from dlib.utils import constants
    from dlib.utils.utils_init_default_args import init_net_g
    assert constants.DSRSPLINES == 'DSR-Splines' and constants.DSRSPLINES_MTH == 'DSR-SPLINES'
    assert constants.DSRSPLINES in constants.MODELS and constants.NETTYPE_METHOD[constants.DSRSPLINES] == 'DSR-SPLINES'
    assert constants.SPLINEHIDDEN == R.HIDDEN and list(R.HIDDEN) == constants.SPLINE_NET_TYPES
    g = init_net_g({'net_type': constants.DSRSPLINES}, {'scale': 8, 'n_channels': 1, 'h_size': 512})
    assert (g['DSR_Splines_in_ksz'], g['DSR_Splines_splinenet_type'], g['DSR_Splines_n_splines_per_color']) == (3, 'snet_type1', 16)
    assert g['DSR_Splines_use_local_residual'] is False and g['DSR_Splines_use_global_residual'] is False
    assert (g['DSR_Splines_color_min'], g['DSR_Splines_color_max'], g['DSR_Splines_upscale'], g['DSR_Splines_in_planes']) == (0, 255, 8, 1)

    class A:
        netG = g
    net = define_G(A)
    assert type(net).__name__ == 'DsrSplines' and net.upscale == 8 and net.n_splines == 16
    assert sum(p.numel() for p in net.parameters()) == 16 * (16 * 9 + 16 + 16 + 1)
    assert [k for k, _ in net.named_parameters()] == [k for k, _ in R.layout(3, [16], 16, False)]
    g3 = dict(g, DSR_Splines_in_planes=3)
    with pytest.raises(NotImplementedError):
        define_G(type("B", (), {"netG": g3}))
    with pytest.raises(NotImplementedError):                         # CSR-CNN stays out
        define_G(type("C", (), {"netG": {'net_type': 'CSR-CNN'}}))


def test_command_line(capsys):
    sys.path.insert(0, os.path.join(ROOT, "sr-caco-2_amd"))
    import main as M
    a = M.parse_input("--net_type DSR-Splines --method DSR-SPLINES --scale 8 --h_size 512 --DSR_Splines_in_ksz 5 "
                      "--DSR_Splines_splinenet_type snet_type3 --DSR_Splines_n_splines_per_color 7 "
                      "--DSR_Splines_use_local_residual True --DSR_Splines_use_global_residual True".split())
    g = a.netG
    assert g['net_type'] == 'DSR-Splines' and a.method == 'DSR-SPLINES'
    assert (g['DSR_Splines_upscale'], g['DSR_Splines_in_ksz'], g['DSR_Splines_splinenet_type']) == (8, 5, 'snet_type3')
    assert g['DSR_Splines_n_splines_per_color'] == 7 and g['DSR_Splines_use_local_residual'] is True
    assert g['DSR_Splines_use_global_residual'] is True
    d = M.parse_input("--net_type DSR-Splines --method DSR-SPLINES --scale 2".split()).netG
    assert (d['DSR_Splines_in_ksz'], d['DSR_Splines_n_splines_per_color'], d['DSR_Splines_upscale']) == (3, 16, 2)
    with pytest.raises(ValueError):
        M.parse_input("--net_type DSR-Splines --method VDSR".split())
    with pytest.raises(SystemExit):                                  # another net's flag is still unknown
        M.parse_input("--net_type VDSR --method VDSR --DSR_Splines_in_ksz 5".split())
    with pytest.raises(SystemExit):
        M.parse_input("--net_type DSR-Splines --method DSR-SPLINES --swinir_embed_dim 60".split())
    capsys.readouterr()
    with pytest.raises(NotImplementedError):
        M.parse_input("--net_type CSR-CNN --method CSR-CNN".split())


@pytest.mark.parametrize("n", [1, 7, 16, 255, 256])
def test_level_table_is_array_splits_bins(n):
    from srhip import ops
    lut = ops.dsr_splines_level_table(n).numpy()
    assert lut.dtype == np.int32 and lut.shape == (256,)
    for k, s in enumerate(np.array_split(range(0, 256), n)):
        assert (lut[np.asarray(s, dtype=np.int64)] == k).all()
    assert np.array_equal(lut, R.level_table(n))
    assert (np.diff(lut) >= 0).all() and lut[0] == 0 and lut[-1] == n - 1


def test_library_exports_the_entry_points():
    import ctypes
    from srhip import _lib, ops
    protos = _lib.parse_header()
    want = {"srhip_dsr_splines_table_floats": ("l", "iii"), "srhip_dsr_splines_pack": ("i", "ppliiiiip"),
            "srhip_dsr_splines_order_sizes": ("i", "lipp"), "srhip_dsr_splines_order": ("i", "plpippppp"),
            "srhip_dsr_splines_fwd": ("i", "pplpppiiiiiiiip"), "srhip_dsr_splines_bwd_ws": ("l", "iiii"),
            "srhip_dsr_splines_bwd": ("i", "ppplppplpliiiiiiiip")}
    for name, sig in want.items():
        assert protos[name] == sig, (name, protos[name])
        assert hasattr(_lib.lib, name)
    # an expert's floats in the table: every tensor padded to four (the largest supported expert: 14,722 floats unpadded)
    for ksz, nh, local in ((3, 1, False), (5, 3, True), (15, 8, True), (1, 2, True)):
        lay = R.layout(ksz, R.HIDDEN[f"snet_type{nh}"], 1, local)
        assert ops.dsr_splines_table_floats(ksz, nh, local) == sum((int(np.prod(s)) + 3) // 4 * 4 for _, s in lay)
    assert sum(int(np.prod(s)) for _, s in R.layout(15, R.HIDDEN["snet_type8"], 1, True)) == 14722
    for bad in ((4, 1), (17, 1), (3, 9), (3, 0)):
        with pytest.raises(_lib.SrhipError):
            ops.dsr_splines_table_floats(bad[0], bad[1], False)
    # argument checks run on the host, in front of any launch
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    with pytest.raises(_lib.SrhipError, match="reflect padding"):
        _lib.call("srhip_dsr_splines_fwd", p, p, 14728, p, p, p, 1, 7, 10, 3, 15, 8, 1, 1, None)
    with pytest.raises(_lib.SrhipError, match="n_splines"):
        _lib.call("srhip_dsr_splines_fwd", p, p, 180, p, p, p, 1, 8, 8, 257, 3, 1, 0, 0, None)
