"""CPU-side tests (no GPU): the C-ABI library loads and exports every symbol
include/srhip.h declares, host logic (flat parameters, LR rules, registry,
state_dict layout, loud failure without a GPU) and the data-parallel gradient
path on world_size-2 gloo."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def test_library_exports_every_declared_symbol():
    from srhip import _lib
    protos = _lib.parse_header()
    assert len(protos) >= 38
    for name in protos:
        assert hasattr(_lib.lib, name), name
    assert _lib.lib.srhip_abi_version() >= 3
    assert isinstance(_lib.lib.srhip_last_error(), bytes)
    # the entry-point count README.md / DESIGN.md quote is the header's (the docs lagged the header)
    import re
    for doc in ("README.md", "DESIGN.md"):
        m = re.search(r'(\d+) `extern "C"` entry points', open(os.path.join(ROOT, doc)).read())
        assert m and int(m.group(1)) == len(protos), (doc, m and m.group(1), len(protos))
    # the C-ABI is the ONLY thing the shipped library exports (built with -fvisibility=hidden; VERDICT r5: ~50 mangled C++
    # symbols leaked): nm -D's defined functions == the header's prototypes, nothing else
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    funcs = sorted(line.split()[-1] for line in out.splitlines() if len(line.split()) == 3 and line.split()[1] in "TtWw")
    if os.path.basename(_lib.LIB_PATH) == "libsrhip.so":
        assert funcs == sorted(protos), (sorted(set(funcs) ^ set(protos)))


def test_ctypes_structs_mirror_the_header(tmp_path):
    """The structs ops.py passes by address are laid out as include/srhip.h declares them: sizeof and the offset of the
    last field, asked of the C compiler (gcc on the plain-C header) -- a field added on one side only would otherwise
    show up as a rejected call on the GPU box."""
    import ctypes
    from srhip import ops
    pairs = {"srhip_prep_entry": (ops._PrepEntry, "mode"), "srhip_tn_problem": (ops._TnProblem, "part_colsum"),
             "srhip_reduce_problem": (ops._ReduceProblem, "ln_ws"), "srhip_conv_wgrad_item": (ops._ConvWgradItem, "db"),
             "srhip_patch_job": (ops._PatchJob, "mode")}
    src = tmp_path / "sizes.c"
    body = "".join(f'  printf("{n} %zu %zu\\n", sizeof({n}), offsetof({n}, {last}));\n' for n, (_, last) in pairs.items())
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "srhip.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    for line in out.strip().splitlines():
        name, size, off = line.split()
        cls, last = pairs[name]
        assert ctypes.sizeof(cls) == int(size), (name, ctypes.sizeof(cls), size)
        assert getattr(cls, last).offset == int(off), (name, last)


HEADER_STRUCTS = ["srhip_prep_entry", "srhip_conv_wgrad_h16_item", "srhip_tn_problem", "srhip_reduce_problem", "srhip_pyr_level",
                  "srhip_patch_job", "srhip_patch_job_f32", "srhip_origin_tile", "srhip_conv_wgrad_item", "srhip_view_job",
                  "srhip_view_desc"]


def test_every_struct_parsed_from_the_header_has_the_compilers_layout(tmp_path):
    """_lib.parse_structs: as many structs as the header has ``typedef struct``, and of each one sizeof and the offsetof of
    EVERY field as gcc reports them for the plain-C header."""
    import ctypes
    import re
    from srhip import _lib, ops
    structs = _lib.parse_structs()
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "srhip.h")).read(), flags=re.S)
    assert len(structs) == len(re.findall(r"\btypedef\s+struct\b", text)) >= 11
    assert set(HEADER_STRUCTS) <= set(structs)
    assert all(_lib.struct(n)._fields_ == structs[n]._fields_ for n in structs)
    assert ops._OriginTile is _lib.struct("srhip_origin_tile") and ops._TnProblem is _lib.struct("srhip_tn_problem")
    body = "".join(f'  printf("{n} %zu", sizeof({n}));\n'
                   + "".join(f'  printf(" %zu", offsetof({n}, {f[0]}));\n' for f in cls._fields_) + '  printf("\\n");\n'
                   for n, cls in structs.items())
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "srhip.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], check=True)
    lines = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.strip().splitlines()
    assert [line.split()[0] for line in lines] == list(structs)
    for line in lines:
        name, size, *offs = line.split()
        cls = structs[name]
        assert ctypes.sizeof(cls) == int(size), (name, ctypes.sizeof(cls), size)
        assert [getattr(cls, f[0]).offset for f in cls._fields_] == [int(o) for o in offs], name
    # what the parser reads beyond scalars: a pointer whatever it points to, an array, a comma list that shares the base type
    assert dict(structs["srhip_view_desc"]._fields_)["h"] is ctypes.c_int * 9
    assert dict(structs["srhip_patch_job"]._fields_) == dict(img=ctypes.c_void_p, H=ctypes.c_int, W=ctypes.c_int, y0=ctypes.c_int,
                                                              x0=ctypes.c_int, mode=ctypes.c_int)
    assert _lib.parse_structs("typedef struct { float *a, b; long n; } srhip_t;")["srhip_t"]._fields_ == \
        [("a", ctypes.c_void_p), ("b", ctypes.c_float), ("n", ctypes.c_long)]


@pytest.mark.parametrize("decl", ["unsigned long long x;", "struct { int a; float b; } s;", "int a : 3;", "void (*f)(int);"])
def test_struct_parser_refuses_what_it_does_not_read(decl):
    from srhip import _lib
    with pytest.raises(ValueError, match="srhip_odd"):
        _lib.parse_structs("typedef struct { int n; /* then */ " + decl + " float* p; } srhip_odd;\n")
    assert list(_lib.parse_structs("typedef struct { int n; float* p; } srhip_odd;\n")) == ["srhip_odd"]


# (S, part_floats) of the bx3 planners, recorded before the weight-gradient kernel forms were chosen in one place:
# srhip_tn_plan_bx3 (M, NI, NJ, conv) at SwinIR's Linears and 180 -> 180 conv, EDSR's 64 -> 64 and 64 -> 256 (PixelShuffle)
# convs at 8 x 64^2 / 128^2 / 256^2, DRRN's 128 -> 128 and ragged / narrow widths; srhip_conv3x3_wgrad_batched_plan
# (n, B, H, W, Cout, Cin)
TN_PLAN_BX3 = {
    (32768, 180, 180, 0): (256, 8294400),
    (32768, 180, 180, 1): (28, 8245440),
    (32768, 540, 180, 0): (85, 8262000),
    (32768, 540, 180, 1): (9, 7950960),
    (32768, 360, 180, 0): (128, 8294400),
    (32768, 360, 180, 1): (14, 8245440),
    (32768, 180, 360, 0): (128, 8294400),
    (32768, 180, 360, 1): (14, 8245440),
    (32768, 64, 64, 0): (256, 1048576),
    (32768, 64, 64, 1): (256, 9519104),
    (131072, 64, 64, 0): (256, 1048576),
    (131072, 64, 64, 1): (256, 9519104),
    (524288, 64, 64, 0): (256, 1048576),
    (524288, 64, 64, 1): (256, 9519104),
    (32768, 256, 64, 0): (192, 3145728),
    (32768, 256, 64, 1): (64, 9519104),
    (131072, 256, 64, 0): (192, 3145728),
    (131072, 256, 64, 1): (64, 9519104),
    (524288, 256, 64, 0): (192, 3145728),
    (524288, 256, 64, 1): (64, 9519104),
    (32768, 128, 128, 0): (256, 4194304),
    (32768, 128, 128, 1): (64, 9519104),
    (2097152, 128, 128, 0): (256, 4194304),
    (2097152, 128, 128, 1): (64, 9519104),
    (4096, 96, 96, 0): (32, 294912),
    (4096, 96, 96, 1): (32, 2695168),
    (4096, 184, 184, 0): (32, 1083392),
    (4096, 184, 184, 1): (28, 8612352),
    (4096, 200, 200, 0): (32, 1280000),
    (4096, 200, 200, 1): (16, 5841920),
    (4096, 64, 96, 0): (32, 196608),
    (4096, 64, 96, 1): (32, 1789952),
    (4096, 96, 64, 0): (32, 196608),
    (4096, 96, 64, 1): (32, 1789952),
}
CONV_WGRAD_BATCHED_PLAN = {
    (33, 8, 64, 64, 64, 64): (23, 855232),
    (33, 8, 128, 128, 64, 64): (23, 855232),
    (33, 8, 256, 256, 64, 64): (23, 855232),
    (1, 8, 64, 64, 180, 180): (28, 8245440),
    (2, 8, 64, 64, 256, 64): (32, 4759552),
    (4, 8, 64, 64, 128, 128): (16, 2379776),
    (5, 2, 24, 40, 96, 96): (1, 84224),
    (3, 1, 9, 7, 184, 184): (1, 307584),
    (3, 2, 16, 16, 200, 200): (1, 365120),
    (7, 2, 16, 16, 64, 96): (1, 55936),
}


def test_plan_queries_need_no_gpu():
    import ctypes
    from srhip import ops
    S, n = ops.tn_plan(32768, 180, 180)
    assert S >= 1 and n == S * 180 * 180
    S9, n9 = ops.tn_plan(32768, 180, 180, conv=True)
    # the nine taps' partial sums + the strip-form kernel's per-block words (320 floats for each of the 3 x 3 64-column tiles)
    assert n9 == S9 * 9 * 180 * 180 + S9 * 9 * 320
    for (M, NI, NJ, conv), want in TN_PLAN_BX3.items():
        assert ops.tn_plan(M, NI, NJ, conv=bool(conv), bx=True) == want, (M, NI, NJ, conv)
    for (k, B, H, W, Co, Ci), want in CONV_WGRAD_BATCHED_PLAN.items():
        S, per = ctypes.c_int(0), ctypes.c_long(0)
        ops.call("srhip_conv3x3_wgrad_batched_plan", k, B, H, W, Co, Ci, ctypes.addressof(S), ctypes.addressof(per))
        assert (S.value, per.value) == want, (k, B, H, W, Co, Ci)
    # the grouped Linear weight gradient: tile counts by pick_tile's classes (180 | <= 64 | <= 128 or a multiple of 128 | 192),
    # the README layer group (six blocks of 3 + 2 + 2 + 1 tiles) at S = 5 on the bf16x3 launch, the workspace of the
    # LayerNorm-folded reducers (four rows per row block, two K-vectors each), and the refusals that precede any launch
    tiles = {(540, 180): 3, (180, 360): 2, (360, 180): 2, (180, 180): 1, (180, 60): 1, (60, 120): 1, (384, 128): 3,
             (128, 256): 2, (64, 64): 1, (48, 20): 1, (184, 180): 1, (180, 200): 2, (200, 68): 2, (360, 184): 2, (400, 68): 3}
    for (NI, NJ), want in tiles.items():
        assert ops.lib.srhip_tn_tiles(NI, NJ) == want, (NI, NJ)
    layer = 6 * sum(tiles[k] for k in ((540, 180), (180, 360), (360, 180), (180, 180)))
    assert layer == 48
    for (M, nt, sfx), want in {(32768, 48, "_bx3"): 5, (2077, 48, "_bx3"): 5, (2077, 47, "_bx3"): 5, (2077, 8, "_bx3"): 17,
                               (2077, 3, "_bx3"): 17, (100, 48, "_bx3"): 1, (32768, 1, "_bx3"): 256, (32768, 8, ""): 64,
                               (2077, 8, ""): 17, (32768, 600, ""): 1}.items():
        S = ctypes.c_int(0)
        ops.call("srhip_tn_group_plan" + sfx, M, nt, ctypes.addressof(S))
        assert S.value == want, (M, nt, sfx)
    for N, K in ((180, 180), (540, 180), (60, 120), (20, 48), (4, 4), (6, 5)):
        assert ops.lib.srhip_ln_affine_ws(N, K) == -(-N // 4) * 2 * K >= -(-N // 16) * 2 * K
    tn, red = (ops._TnProblem * 25)(), (ops._ReduceProblem * 25)()
    for name, arr, n, S in (("srhip_gemm_tn_grouped_bx3", tn, 25, 2), ("srhip_gemm_tn_grouped", tn, 5, 2),
                            ("srhip_gemm_tn_grouped_bx3", tn, 0, 2), ("srhip_gemm_tn_grouped_bx3", tn, 1, 0),
                            ("srhip_reduce_wgrad_grouped", red, 25, 2), ("srhip_reduce_wgrad_grouped", red, 1, 0),
                            ("srhip_reduce_wgrad_grouped", red, 1, 2)):      # (the last: a problem without buffers)
        with pytest.raises(ops.SrhipError):
            ops.call(name, ctypes.addressof(arr), n, 64, S, None) if arr is tn else ops.call(name, ctypes.addressof(arr), n, S, None)
    tn[0].b_mode = 3
    with pytest.raises(ops.SrhipError, match="b_mode 3"):
        ops.call("srhip_gemm_tn_grouped_bx3", ctypes.addressof(tn), 1, 64, 2, None)
    tn[0].b_mode = 1
    with pytest.raises(ops.SrhipError, match="without stats"):
        ops.call("srhip_gemm_tn_grouped", ctypes.addressof(tn), 1, 64, 2, None)


def test_cpu_tensors_fail_loudly():
    from srhip import ops
    from dlib.models.network_swinir import SwinIR
    from dlib.models.network_edsr_liif import EDSR_LIIF
    from dlib import loss, metrics
    with pytest.raises(RuntimeError):
        ops.gemm_nt(torch.zeros(8, 8), torch.zeros(8, 8))
    net = SwinIR(upscale=8, in_chans=1, img_size=16, window_size=8, depths=[2], embed_dim=60,
                 num_heads=[6], mlp_ratio=2, upsampler="pixelshuffledirect")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(torch.rand(1, 1, 16, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        EDSR_LIIF(scale=2, n_resblocks=1, n_feats=16)(torch.rand(1, 1, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss.L1(cuda_id="cpu")(epoch=0, y_pred=torch.rand(1, 1, 8, 8), y_target=torch.rand(1, 1, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.mbatch_gpu_calculate_psnr(torch.rand(1, 1, 32, 32), torch.rand(1, 1, 32, 32))
    with pytest.raises(NotImplementedError):                    # heads have to divide the embedding (a multiple of 4)
        SwinIR(upscale=4, in_chans=1, img_size=64, window_size=7, upsampler="pixelshuffle", embed_dim=90, num_heads=[4], depths=[2])
    with pytest.raises(NotImplementedError):
        SwinIR(upscale=4, in_chans=5, img_size=64, window_size=8, upsampler="pixelshuffle")
    assert SwinIR(upscale=4, in_chans=1, img_size=64, window_size=4, upsampler="pixelshuffle", embed_dim=60, depths=[2],
                  num_heads=[6]).use_tape
    # dropout rates: accepted (evaluation is the identity), a training-mode forward refuses
    nd = SwinIR(upscale=2, in_chans=1, img_size=16, window_size=8, depths=[2], embed_dim=60, num_heads=[6], mlp_ratio=2,
                upsampler="pixelshuffledirect", drop_rate=0.1, attn_drop_rate=0.1)
    assert nd.eval().sample_drop_path(2, "cpu") is None
    with pytest.raises(NotImplementedError, match="drop_rate"):
        nd.train().sample_drop_path(2, "cpu")
    # RGB and the absolute position embedding: the reference's parameter names, order and shapes (goldens g42 / g44)
    for name, kw in (("g42_swinir_ape", dict(in_chans=1, depths=[2, 2], num_heads=[6, 6], upsampler="pixelshuffledirect", ape=True)),
                     ("g44_swinir_rgb_pixelshuffle", dict(in_chans=3, depths=[2], num_heads=[6], upsampler="pixelshuffle", img_range=2.0))):
        z = np.load(os.path.join(G, name + ".npz"))
        ref = {k[3:]: z[k].shape for k in z.files if k.startswith("sd/")}
        net = SwinIR(upscale=2, img_size=16, window_size=8, embed_dim=60, mlp_ratio=2, **kw)
        assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == list(ref.items())
    assert torch.equal(net.mean.flatten(), torch.tensor([0.4488, 0.4371, 0.4040]))


def test_state_dict_layouts_match_reference():
    from dlib.models.network_swinir import SwinIR
    from dlib.models.network_edsr_liif import EDSR_LIIF
    z = np.load(os.path.join(G, "g4_swinir_readme.npz"))
    net = SwinIR(upscale=8, in_chans=1, img_size=64, window_size=8, depths=[6, 6, 6, 6], embed_dim=180,
                 num_heads=[6, 6, 6, 6], mlp_ratio=2, upsampler="pixelshuffledirect")
    sd = net.state_dict()
    assert list(sd.keys()) == list(z["keys"]) and len(sd) == 366
    assert [str(tuple(v.shape)) for v in sd.values()] == list(z["shapes"])
    e = np.load(os.path.join(G, "g2_edsr_x4.npz"))
    ref_keys = [k[3:] for k in e.files if k.startswith("sd/")]
    s, nb, nf = [int(v) for v in e["cfg"]]
    assert list(EDSR_LIIF(scale=s, n_resblocks=nb, n_feats=nf).state_dict().keys()) == ref_keys


def test_registry_and_factories():
    from dlib.models.select_network import define_G
    from dlib.utils import constants
    from dlib.utils.utils_init_default_args import init_net_g
    from dlib.utils.utils_instance import define_loss, optimizer_config

    class A(dict):
        __getattr__ = dict.get
    netG = init_net_g({'net_type': constants.SWINIR}, {'scale': 8, 'n_channels': 1, 'h_size': 512})
    netG.update(swinir_depths=[6, 6, 6, 6], swinir_num_heads=[6, 6, 6, 6],
                swinir_upsampler=constants.US_PIXEL_SHUFFLE_DIRECT)
    args = A(netG=netG, train={'l2': True, 'ssim': True, 'ssim_lambda': 5.0, 'ssim_window_s': 19,
                               'G_optimizer_type': 'sgd', 'G_optimizer_lr': 0.01,
                               'G_scheduler_type': 'MyStepLR', 'G_scheduler_step_size': 30,
                               'G_scheduler_gamma': 0.5})
    net = define_G(args)
    assert sum(p.numel() for p in net.parameters()) == 7865884
    m = define_loss(args)
    assert m.n_holder == ['master_loss', 'l2', 'negative_ssim']
    assert m.terms() == [('l2', 1.0), ('ssim', 5.0, 19)]
    cfg = optimizer_config(args)
    assert cfg['kind'] == 'sgd' and cfg['scheduler']['type'] == 'MyStepLR'
    e = init_net_g({'net_type': constants.EDSR_LIIF}, {'scale': 4, 'n_channels': 1, 'h_size': 512})
    assert define_G(A(netG=e)).n_resblocks == 16
    with pytest.raises(NotImplementedError):
        define_G(A(netG={'net_type': 'CSRCNN'}))
    assert constants.NETTYPE_METHOD[constants.SWINIR] == 'SWINIR'


def test_enlcn_mirror_layout_and_oracle_vs_reference_golden():
    """ENLCN: the registry's default net carries the reference's state_dict keys in the reference's order
    (frozen MeanShift convs and the projection-matrix buffers included); the oracle restatement reproduces the reference's
    outputs stored in g33_enlcn.npz."""
    from dlib.models.network_enlcn import ENLCN
    from oracle import sr_oracle as O
    g = np.load(os.path.join(ROOT, "tests", "golden", "g33_enlcn.npz"))
    assert list(ENLCN(upscale=2, in_chans=1).state_dict().keys()) == [str(k) for k in g["state_dict_keys_default"]]
    with pytest.raises(NotImplementedError):
        ENLCN(upscale=3, in_chans=1)
    for scale in (2, 4, 8):
        sd = O.enlcn_init_state_dict(scale, 1, 8, 64, seed=int(g[f"x{scale}/seed"]))
        net = ENLCN(upscale=scale, in_chans=1, n_resblock=8, n_feats=64)
        assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == [(k, tuple(v.shape)) for k, v in sd.items()]
        net.load_state_dict(sd, strict=True)
        y = O.enlcn_forward(sd, torch.from_numpy(g[f"x{scale}/x"]), scale, 8, 0.1)
        assert (y - torch.from_numpy(g[f"x{scale}/y"])).abs().max().item() <= 2e-6


def test_nlsn_mirror_layout_and_oracle_vs_reference_golden():
    """NLSN: state_dict keys in the reference's order; the oracle, given the rotations the reference drew and
    the order its sort produced (both in g34_nlsn.npz), reproduces the reference's output exactly."""
    from dlib.models.network_nlsn import NLSN
    from oracle import sr_oracle as O
    g = np.load(os.path.join(ROOT, "tests", "golden", "g34_nlsn.npz"))
    assert list(NLSN(upscale=2, in_chans=1).state_dict().keys()) == [str(k) for k in g["state_dict_keys_default"]]
    for scale in (2, 4, 8):
        sd = O.nlsn_init_state_dict(scale, 1, 8, 64, seed=int(g[f"x{scale}/seed"]))
        net = NLSN(upscale=scale, in_chans=1, n_resblocks=8, n_feats=64)
        assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == [(k, tuple(v.shape)) for k, v in sd.items()]
        rots = [torch.from_numpy(g[f"x{scale}/rot{a}"]) for a in range(2)]
        idx = [torch.from_numpy(g[f"x{scale}/indices{a}"]) for a in range(2)]
        taps = []
        y = O.nlsn_forward(sd, torch.from_numpy(g[f"x{scale}/x"]), scale, 8, 4, 144, 0.1, rotations=rots, indices=idx, taps=taps)
        assert (y - torch.from_numpy(g[f"x{scale}/y"])).abs().max().item() <= 2e-6
        for a in range(2):
            assert torch.equal(taps[a]["codes"], torch.from_numpy(g[f"x{scale}/codes{a}"]))


def test_dfcan_mirror_layout_and_oracle_vs_reference_golden():
    """DFCAN: state_dict keys in the reference's order; the oracle reproduces the reference's outputs of
    g35_dfcan.npz (even and odd image sizes: the quadrant swap splits at h // 2)."""
    from dlib.models.network_dfcan import DFCAN
    from oracle import sr_oracle as O
    g = np.load(os.path.join(ROOT, "tests", "golden", "g35_dfcan.npz"))
    assert list(DFCAN(input_shape=1, upscale=2).state_dict().keys()) == [str(k) for k in g["state_dict_keys_default"]]
    with pytest.raises(NotImplementedError):
        DFCAN(input_shape=3, upscale=2)
    for scale in (2, 4, 8):
        sd = O.dfcan_init_state_dict(scale, 1, seed=int(g[f"x{scale}/seed"]))
        net = DFCAN(input_shape=1, upscale=scale)
        assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == [(k, tuple(v.shape)) for k, v in sd.items()]
        y = O.dfcan_forward(sd, torch.from_numpy(g[f"x{scale}/x"]), scale)
        assert (y - torch.from_numpy(g[f"x{scale}/y"])).abs().max().item() <= 2e-6


def test_act_mirror_layout_and_oracle_vs_reference_golden():
    """ACT: the 660 state_dict entries of the registry's net in the reference's order and shapes; the oracle
    reproduces the reference's outputs of g36_act.npz (image sizes that are and are not multiples of the token size)."""
    from dlib.models.network_act import ACT
    from oracle import sr_oracle as O
    g = np.load(os.path.join(ROOT, "tests", "golden", "g36_act.npz"))
    sd0 = ACT(upscale=2, in_chans=1).state_dict()
    assert list(sd0.keys()) == [str(k) for k in g["state_dict_keys_default"]]
    assert [str(tuple(v.shape)) for v in sd0.values()] == [str(k) for k in g["state_dict_shapes_default"]]
    cfg = dict(n_feats=16, n_resgroups=4, n_resblocks=2, reduction=4, n_heads=4, n_layers=8, n_fusionblocks=4)
    for scale in (2, 4, 8):
        net = ACT(upscale=scale, in_chans=1, **cfg)
        layout = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
        assert [k for k, _ in layout] == [str(k) for k in g[f"x{scale}/layout_keys"]]
        sd = O.seeded_state_dict(layout, int(g[f"x{scale}/seed"]))
        y = O.act_forward(sd, torch.from_numpy(g[f"x{scale}/x"]), scale, n_feats=16, n_resblocks=2, n_heads=4)
        assert (y - torch.from_numpy(g[f"x{scale}/y"])).abs().max().item() <= 2e-6


def test_omnisr_mirror_layout_and_oracle_vs_reference_golden():
    """OmniSR: the 1066 state_dict entries of the registry's net in the reference's order and shapes; the oracle
    reproduces the reference's outputs of g37_omnisr.npz (sizes that are and are not multiples of the window)."""
    from dlib.models.network_omni_sr import OmniSR
    from oracle import sr_oracle as O
    g = np.load(os.path.join(ROOT, "tests", "golden", "g37_omnisr.npz"))
    sd0 = OmniSR(input_shape=1, upscale=2).state_dict()
    assert list(sd0.keys()) == [str(k) for k in g["state_dict_keys_default"]]
    assert [str(tuple(v.shape)) for v in sd0.values()] == [str(k) for k in g["state_dict_shapes_default"]]
    for scale in (2, 4, 8):
        net = OmniSR(input_shape=1, upscale=scale, num_feat=16, res_num=2, block_num=1)
        layout = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
        assert [k for k, _ in layout] == [str(k) for k in g[f"x{scale}/layout_keys"]]
        sd = O.seeded_state_dict(layout, int(g[f"x{scale}/seed"]))
        y = O.omnisr_forward(sd, torch.from_numpy(g[f"x{scale}/x"]), scale, res_num=2, block_num=1)
        assert (y - torch.from_numpy(g[f"x{scale}/y"])).abs().max().item() <= 2e-6


def test_grl_mirror_layout_buffers_and_oracle_vs_reference_golden():
    """GRL: the state_dict entries of the registry's net ("Big": 180 channels, 40 blocks) in the reference's
    order and shapes, the 13 registered tables / indices / masks equal to the reference's (64 x 64 and a 16 x 24 input), and
    the oracle reproducing the reference's outputs of g38_grl.npz (reflect-padded and recomputed-mask sizes)."""
    from dlib.models.network_grl import GRL, table_index_mask
    from oracle import sr_oracle as O
    g = np.load(os.path.join(ROOT, "tests", "golden", "g38_grl.npz"))
    kw = dict(in_chans=1, window_size=8, mlp_ratio=2, qkv_proj_type="linear", anchor_proj_type="avgpool",
              anchor_window_down_factor=2, out_proj_type="linear", conv_type="1conv", upsampler="pixelshuffle",
              local_connection=True)
    net = GRL(upscale=2, img_size=64, depths=[4, 4, 8, 8, 8, 4, 4], embed_dim=180, num_heads_window=[3] * 7,
              num_heads_stripe=[3] * 7, **kw)
    sd0 = net.state_dict()
    assert list(sd0.keys()) == [str(k) for k in g["state_dict_keys_default"]]
    assert [str(tuple(v.shape)) for v in sd0.values()] == [str(k) for k in g["state_dict_shapes_default"]]
    for k, v in O.grl_buffers((64, 64)).items():
        assert torch.equal(sd0[k], v) and sd0[k].dtype == v.dtype, k
    b = table_index_mask((16, 24), (8, 8), [8, 8], 2)
    bo = O.grl_buffers((16, 24))
    for k in ("table_sh", "index_sh_a2w", "index_sv_w2a", "mask_w", "mask_sh_a2w"):
        ref = torch.from_numpy(g["buf_16x24/" + k])
        assert torch.equal(b[k], ref) and torch.equal(bo[k], ref), k
    for scale in (2, 4, 8):
        net = GRL(upscale=scale, img_size=16, depths=[2, 2], embed_dim=36, num_heads_window=[3, 3], num_heads_stripe=[3, 3], **kw)
        layout = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
        assert [k for k, _ in layout] == [str(k) for k in g[f"x{scale}/layout_keys"]]
        assert [str(s) for _, s in layout] == [str(k) for k in g[f"x{scale}/layout_shapes"]]
        sd = O.grl_state_dict(layout, int(g[f"x{scale}/seed"]), 16)
        net.load_state_dict(sd, strict=True)
        y = O.grl_forward(sd, torch.from_numpy(g[f"x{scale}/x"]), scale, depths=(2, 2))
        assert (y - torch.from_numpy(g[f"x{scale}/y"])).abs().max().item() <= 2e-6
    with pytest.raises(NotImplementedError):
        GRL(upscale=2, in_chans=1, upsampler="nearest+conv")


def test_tape_net_mirrors_have_the_reference_state_dict_layout():
    """DBPN / SRFBN mirrors: the registry's default nets carry the reference's state_dict keys (SRFBN: in the
    reference's ORDER, frozen MeanShift convs included) and the re-layout maps of the strided / transposed convs are exact."""
    import torch.nn.functional as F
    from dlib.models.network_dbpn import DBPN
    from dlib.models.network_srfbn import SRFBN
    from srhip import tape as T
    gd = np.load(os.path.join(ROOT, "tests", "golden", "g28_dbpn.npz"))
    gs = np.load(os.path.join(ROOT, "tests", "golden", "g29_srfbn.npz"))
    assert sorted(DBPN(upscale=4, in_chans=1).state_dict().keys()) == sorted(str(k) for k in gd["state_dict_keys_default"])
    assert list(SRFBN(upscale=4, in_chans=1).state_dict().keys()) == [str(k) for k in gs["state_dict_keys_default"]]
    with pytest.raises(NotImplementedError):
        DBPN(upscale=4, in_chans=3)
    torch.manual_seed(0)
    for s, k in ((2, 6), (3, 7), (4, 8), (8, 12)):
        wt, b, x = torch.randn(3, 5, k, k), torch.randn(5), torch.randn(2, 3, 5, 6)
        ref = F.conv_transpose2d(x, wt, b, stride=s, padding=2)
        y = F.pixel_shuffle(F.conv2d(x, T.expand_deconv(wt, s, 2), b.repeat_interleave(s * s), padding=1), s)
        assert (ref - y).abs().max() < 1e-4
        w, xh = torch.randn(5, 3, k, k), torch.randn(2, 3, 5 * s, 6 * s)
        ref = F.conv2d(xh, w, b, stride=s, padding=2)
        y = F.conv2d(F.pixel_unshuffle(xh, s), T.expand_down(w, s, 2), b, padding=1)
        assert (ref - y).abs().max() < 2e-4
        d = torch.randn(5 * s * s, 3, 3, 3)          # collapse_* is the adjoint of expand_*
        assert abs(((T.expand_deconv(wt, s, 2) * d).sum() - (wt * T.collapse_deconv(d, 3, 5, s, k, 2)).sum()).item()) < 1e-3


def test_flat_params_and_lr_rules():
    from srhip.train import FlatParams, Optimizer
    from dlib.learning.lr_scheduler import MyStepLR
    net = torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.Linear(3, 7))
    before = [p.detach().clone() for p in net.parameters()]
    fp = FlatParams(net)
    for p, b in zip(net.parameters(), before):
        assert torch.equal(p, b) and p.data_ptr() >= fp.flat.data_ptr()
        assert p.grad is not None and p.grad.shape == p.shape
    assert fp.total % 4 == 0 and all(o % 4 == 0 for o in fp.offsets.values())
    lo, hi = fp.range_of(["1."])
    assert lo == fp.offsets["1.weight"] and hi == fp.total
    g = np.load(os.path.join(G, "g8_optim.npz"))
    opt = Optimizer(fp, "sgd", lr=0.01, scheduler={"type": "MyStepLR", "step_size": 30, "gamma": 0.5,
                                                  "min_lr": 1e-4})
    tp = torch.nn.Parameter(torch.zeros(1))
    topt = torch.optim.SGD([tp], lr=0.01)
    sch = MyStepLR(topt, step_size=30, gamma=0.5, min_lr=1e-4)
    for it in range(300):
        opt.scheduler_step()
        topt.step()
        sch.step()
        assert abs(opt.lr - g["mysteplr"][it]) < 1e-15
        assert abs(topt.param_groups[0]["lr"] - g["mysteplr"][it]) < 1e-15


WORKER = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, os.path.join(sys.argv[1], "sr-caco-2_amd"))
from srhip.train import FlatParams, allreduce_range
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo")
torch.manual_seed(0)
net = torch.nn.Sequential(torch.nn.Linear(6, 4), torch.nn.Linear(4, 4), torch.nn.Linear(4, 2))
fp = FlatParams(net)
buckets = [fp.range_of(["2."]), fp.range_of(["1."]), fp.range_of(["0."])]   # backward order
x = torch.randn(8, 6, generator=torch.Generator().manual_seed(100 + rank))
full = torch.cat([torch.randn(8, 6, generator=torch.Generator().manual_seed(100 + r)) for r in range(world)])
net(x).pow(2).mean().backward()                       # autograd writes into the flat views
assert all(p.grad.data_ptr() == fp.gviews[k].data_ptr() for k, p in net.named_parameters())
for lo, hi in buckets:
    allreduce_range(fp.grad, lo, hi)
fp.grad.mul_(1.0 / world)                              # the optimizer's gscale
ref = torch.nn.Sequential(torch.nn.Linear(6, 4), torch.nn.Linear(4, 4), torch.nn.Linear(4, 2))
ref.load_state_dict(net.state_dict())
ref(full).pow(2).mean().backward()                    # 1-rank large batch
for (k, p), q in zip(net.named_parameters(), ref.parameters()):
    assert torch.allclose(fp.gviews[k], q.grad, atol=1e-6), k
covered = sorted(buckets)
assert covered[0][0] == 0 and covered[-1][1] == fp.total
assert all(a[1] == b[0] for a, b in zip(covered, covered[1:]))
dist.barrier()
dist.destroy_process_group()
print("rank", rank, "ok")
'''


def test_data_parallel_gradient_path_gloo_world2(tmp_path):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="2",
               OMP_NUM_THREADS="1")
    procs = [subprocess.Popen([sys.executable, str(script), ROOT], env=dict(env, RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(2)]
    outs = [p.communicate(timeout=240)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} failed:\n{o}"
        assert f"rank {r} ok" in o


def test_main_cli_contract():
    sys.path.insert(0, os.path.join(ROOT, "sr-caco-2_amd"))
    import main as M
    a = M.parse_input("--task super-resolution --scale 8 --method SWINIR --net_type swinir --n_channels 1 "
                      "--h_size 512 --batch_size 8 --G_optimizer_type sgd --G_optimizer_lr 0.01 "
                      "--swinir_depths 6+6+6+6 --swinir_embed_dim 180 --swinir_num_heads 6+6+6+6 "
                      "--swinir_mlp_ratio 2 --swinir_upsampler pixelshuffledirect --l1 False --l2 True "
                      "--ssim True --ssim_lambda 5.0 --ssim_window_s 19 --valid_n_samples 128".split())
    assert a.netG['swinir_depths'] == [6, 6, 6, 6] and a.netG['swinir_img_size'] == 64
    assert a.train['ssim_window_s'] == 19 and a.train['G_optimizer_type'] == 'sgd' and not a.train['l1']
    with pytest.raises(ValueError):
        M.parse_input("--net_type swinir --method EDSR_LIIF".split())
    with pytest.raises(NotImplementedError):
        M.parse_input("--net_type CSRCNN --method CSRCNN".split())
    e = M.parse_input("--net_type EDSR_LIIF --method EDSR_LIIF --scale 4 --h_size 512".split())
    assert e.netG['EDSR_LIIF_n_resblocks'] == 16 and e.netG['EDSR_LIIF_upscale'] == 4


def test_main_cli_says_no_instead_of_ignoring(capsys):
    """VERDICT r5 item 4 (reference: argparse.parse_args + 'key not found' ValueError, utils_parser.py:884,900-923): a flag
    that changes what a run computes is implemented, or an error -- never skipped.  Flags that only name folders / logging /
    launcher plumbing pass without effect; implemented ones land in the configuration."""
    sys.path.insert(0, os.path.join(ROOT, "sr-caco-2_amd"))
    import main as M
    base = "--net_type swinir --method SWINIR --scale 8".split()
    a = M.parse_input(base + "--G_optimizer_clipgrad 1.0 --E_decay 0.999 --E_param_strict False --ppiw True --da_blur True "
                             "--da_blur_sigma 2.0 --use_interpolated_low True --inter_low_sigma 5.0 --exp_id run7 --verbose True "
                             "--num_workers 4 --local_rank 0 --swinir_init_type init_w_default --G_regularizer_orthstep 0 "
                             "--l1_use_residuals False --init_pretrained_path /x/y.pth".split())
    assert a.train['G_optimizer_clipgrad'] == 1.0 and a.train['E_decay'] == 0.999 and a.train['E_param_strict'] is False
    assert a.ppiw is True and a.da_blur is True and a.da_blur_sigma == 2.0 and a.da_blur_prob == 0.5
    assert a.use_interpolated_low is True and a.inter_low_sigma == 5.0 and a.inter_low_th == 7.0
    assert a.netG['init_pretrained_path'] == '/x/y.pth'
    for bad in ("--G_regularizer_orthstep 1", "--G_regularizer_clipstep 2", "--G_optimizer_amsgrad True",
                "--swinir_init_type init_w_normal", "--swinir_init_gain 0.2", "--l1_use_residuals True", "--ce True",
                "--augment True", "--reconstruct_type high_res", "--train_n 0.5", "--no_such_flag 1",
                "--EDSR_LIIF_n_feats 32"):          # (another network's option)
        with pytest.raises(SystemExit) as ei:
            M.parse_input(base + bad.split())
        assert ei.value.code == 2, bad
        assert bad.split()[0] in capsys.readouterr().err
    # the same through the command line: a non-zero exit before anything touches a GPU
    r = subprocess.run([sys.executable, os.path.join(ROOT, "sr-caco-2_amd", "main.py")] + base + ["--G_regularizer_orthstep", "1"],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "G_regularizer_orthstep" in r.stderr
    # every flag of the reference's parser is known to this one (names as of utils_parser.py:33-880; per-net options apart)
    ref_flags = ("cudaid myseed debug_subfolder task reconstruct_type reconstruct_input method is_train n_channels train_dsets "
                 "valid_dsets test_dsets h_size valid_n_samples scale train_n batch_size eval_bsize num_workers exp_id verbose "
                 "fd_exp save_dir_models save_dir_imgs init_pretrained_path basic_interpolation use_interpolated_low inter_low_th "
                 "inter_low_sigma E_decay G_optimizer_type G_optimizer_lr G_optimizer_wd G_optimizer_clipgrad G_optimizer_reuse "
                 "G_optimizer_momentum G_optimizer_nesterov G_optimizer_beta1 G_optimizer_beta2 G_optimizer_eps_adam "
                 "G_optimizer_amsgrad G_scheduler_type G_scheduler_gamma G_scheduler_min_lr G_scheduler_step_size "
                 "G_regularizer_orthstep G_regularizer_clipstep G_param_strict E_param_strict checkpoint_eval checkpoint_save "
                 "test_epoch_freq plot_epoch_freq synch_scratch_epoch_freq max_epochs ppiw ppiw_min_per_col_w sample_tr_patch "
                 "sample_tr_patch_th_style sample_tr_patch_th w_sparsity w_sparsity_lambda net_type net_task elb_init_t elb_max_t "
                 "elb_mulcoef l1 l1_use_residuals l1_lambda l2 l2_use_residuals l2_lambda l2sum l2sum_use_residuals l2sum_lambda "
                 "ssim ssim_lambda ssim_window_s charbonnier charbonnier_use_residuals charbonnier_lambda charbonnier_eps boundpred "
                 "boundpred_use_residuals boundpred_lambda boundpred_eps boundpred_restore_range local_moments "
                 "local_moments_use_residuals local_moments_lambda local_moments_ksz img_grad img_grad_use_residuals img_grad_lambda "
                 "img_grad_norm norm_img_grad norm_img_grad_use_residuals norm_img_grad_lambda norm_img_grad_type laplace "
                 "laplace_use_residuals laplace_lambda laplace_norm norm_laplace norm_laplace_use_residuals norm_laplace_lambda "
                 "norm_laplace_type loc_var loc_var_ksz loc_var_use_residuals loc_var_lambda loc_var_norm norm_loc_var "
                 "norm_loc_var_ksz norm_loc_var_use_residuals norm_loc_var_lambda norm_loc_var_type hist hist_lambda hist_sigma "
                 "hist_metric kde kde_lambda kde_nbins kde_kde_bw kde_metric ce ce_lambda amp amp_eval distributed local_rank "
                 "local_world_size init_method dist_backend world_size model_select_mtr augment augment_nbr_steps augment_use_roi "
                 "eval_over_roi_also eval_over_roi_also_model_select da_blur da_blur_prob da_blur_area da_blur_sigma da_dot_bin_noise "
                 "da_dot_bin_noise_prob da_dot_bin_noise_area da_dot_bin_noise_p da_add_gaus_noise da_add_gaus_noise_prob "
                 "da_add_gaus_noise_area da_add_gaus_noise_std").split()
    import argparse
    known = set()
    orig = argparse.ArgumentParser.add_argument

    def spy(self, *names, **kw):
        known.update(n[2:] for n in names if n.startswith('--'))
        return orig(self, *names, **kw)
    argparse.ArgumentParser.add_argument = spy
    try:
        M.parse_input(base)
    finally:
        argparse.ArgumentParser.add_argument = orig
    assert not [f for f in ref_flags if f not in known], [f for f in ref_flags if f not in known]


def test_sharded_sampler_matches_torch_distributed_sampler():
    """utils_dataloaders.py:138-148 / utils_trainer.py:325-326,382-386: same index lists as torch's
    DistributedSampler for shuffle+seed+drop_last+set_epoch (train) and the unshuffled padded eval form."""
    from torch.utils.data.distributed import DistributedSampler
    from dlib.utils.utils_dataloaders import ShardedSampler, train_sampler, eval_sampler
    for n in (1, 7, 64, 101, 1000):
        ds = list(range(n))
        for world in (1, 2, 3, 8):
            for rank in range(world):
                for drop_last in (True, False):
                    for shuffle in (True, False):
                        if drop_last and n < world:
                            continue
                        ref = DistributedSampler(ds, num_replicas=world, rank=rank, shuffle=shuffle, seed=17,
                                                 drop_last=drop_last)
                        mine = ShardedSampler(n, world, rank, shuffle=shuffle, seed=17, drop_last=drop_last)
                        for epoch in (0, 1, 5):
                            ref.set_epoch(epoch)
                            mine.set_epoch(epoch)
                            assert list(ref) == list(mine), (n, world, rank, drop_last, shuffle, epoch)
                            assert len(ref) == len(mine)
    s = train_sampler(100, 8, 3, seed=0)
    s.set_epoch(2)
    b = s.batches(4)
    assert len(b) == 3 and all(len(x) == 4 for x in b) and sum(b, []) == s.indices()[:12]
    # all ranks together cover every sample exactly once per epoch (drop_last trims the tail)
    cover = sorted(sum((train_sampler(96, 8, r, 5).indices() for r in range(8)), []))
    assert cover == list(range(96))
    assert sorted(sum((eval_sampler(10, 4, r).indices() for r in range(4)), [])) == sorted(list(range(10)) + [0, 1])


def test_modelplain_checkpoint_protocol_signatures():
    """The trainer's call sites (utils_trainer.py:230 save_best(_dir, p_name_file='model.pth'), :1208
    save_current(save_dir=...), :1289 load_current(save_dir=...)) bind against these signatures and the
    file names are the reference's (model_plain.py:103-137)."""
    import inspect
    from dlib.models.model_plain import ModelPlain
    assert list(inspect.signature(ModelPlain.save_best).parameters) == ['self', 'save_dir', 'p_name_file']
    assert list(inspect.signature(ModelPlain.save_current).parameters) == ['self', 'save_dir']
    assert list(inspect.signature(ModelPlain.load_current).parameters) == ['self', 'save_dir']
    assert list(inspect.signature(ModelPlain.load_network).parameters) == \
        ['self', 'load_path', 'network', 'strict', 'param_key']
    inspect.signature(ModelPlain.save_best).bind(None, '/tmp/x', p_name_file='model.pth')
    inspect.signature(ModelPlain.save_current).bind(None, save_dir='/tmp/x')
    inspect.signature(ModelPlain.load_current).bind(None, save_dir='/tmp/x')
    src = inspect.getsource(ModelPlain)
    assert "f'G-{p_name_file}'" in src and "'G-current_model.pth'" in src


WORKER_REDUCER = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, os.path.join(sys.argv[1], "sr-caco-2_amd"))
from srhip.train import FlatParams, GradReducer, broadcast_replica_state
from dlib.utils.utils_parallel import (sync_tensor_across_gpus, sync_non_tensor_value_across_gpus,
                                       sync_dict_across_gpus, sync_metric_sums)
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo")


class StubEngine:
    """Fills the flat gradient views layer by layer in backward order, the way the HIP engines do,
    and announces buckets through on_layer_done -- `announce` picks which ones: the SwinIR engine
    announces every bucket but the last, EDSR none, and an engine that announces its only (= last)
    bucket must not get it reduced twice."""
    def __init__(self, net, prefixes, announce):
        self.net, self.prefixes, self.announce = net, prefixes, announce
    def bucket_prefixes(self):
        return self.prefixes
    def backward(self, x, fp, on_layer_done):
        loss = self.net(x).pow(2).mean()
        grads = torch.autograd.grad(loss, list(self.net.parameters()))
        named = dict(zip([k for k, _ in self.net.named_parameters()], grads))
        for bi, pf in enumerate(self.prefixes):            # backward-completion order
            for k, g in named.items():
                if any(k.startswith(p) for p in pf):
                    fp.gviews[k].copy_(g)
            if on_layer_done is not None and bi in self.announce:
                on_layer_done(bi)


def run(prefixes, announce):
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(6, 4), torch.nn.Linear(4, 4), torch.nn.Linear(4, 2))
    ref = torch.nn.Sequential(torch.nn.Linear(6, 4), torch.nn.Linear(4, 4), torch.nn.Linear(4, 2))
    ref.load_state_dict(net.state_dict())
    fp = FlatParams(net)
    eng = StubEngine(net, prefixes, announce)
    red = GradReducer(fp.grad, [fp.range_of(pf) for pf in eng.bucket_prefixes()])
    x = torch.randn(8, 6, generator=torch.Generator().manual_seed(100 + rank))
    full = torch.cat([torch.randn(8, 6, generator=torch.Generator().manual_seed(100 + r)) for r in range(world)])
    for step in range(2):                                   # begin() must re-arm every step
        fp.grad.zero_()
        red.begin()
        eng.backward(x, fp, red.bucket_done)
        flag = torch.tensor([1 if (rank == 1 and step == 1) else 0], dtype=torch.int32)
        red.finish(flag)
        assert sorted(red.log) == list(range(len(prefixes))) and len(red.log) == len(prefixes), red.log
        assert red.log[:len(announce)] == sorted(announce), (red.log, announce)   # hook order = backward order
        assert int(flag) == (1 if step == 1 else 0)        # MAX over ranks: every replica skips together
        fp.grad.mul_(1.0 / world)                           # the optimizer's gscale
        for p in ref.parameters():
            p.grad = None
        ref(full).pow(2).mean().backward()                  # the rank-MEAN gradient = 1-rank large batch
        for (k, p), q in zip(net.named_parameters(), ref.parameters()):
            assert torch.allclose(fp.gviews[k], q.grad, atol=1e-6), (k, prefixes, announce)


run([["2."], ["1."], ["0."]], announce=[0, 1])      # SwinIR style: all but the last
run([["2."], ["1."], ["0."]], announce=[])          # EDSR style: none announced
run([["2."], ["1."], ["0."]], announce=[0, 1, 2])   # all announced
run([["0.", "1.", "2."]], announce=[0])             # one bucket, announced (old VDSR / DRRN engines)
run([["0.", "1.", "2."]], announce=[])              # one bucket, not announced

# replica initialisation (model_base.py:135-142: DDP broadcasts rank 0's parameters and buffers): replicas that
# START DIFFERENT -- another seed, BatchNorm running statistics that drifted apart, an integer step counter -- end equal,
# and stay equal through reduced steps
def replicas_that_start_different_end_equal():
    torch.manual_seed(10 + rank)                            # a different initialisation on every rank
    net = torch.nn.Sequential(torch.nn.Linear(6, 4), torch.nn.BatchNorm1d(4), torch.nn.Linear(4, 2))
    with torch.no_grad():
        net[1].running_mean.add_(rank + 1.0)
        net[1].num_batches_tracked.add_(7 * rank + 3)
    fp = FlatParams(net)
    def gathered(t):
        out = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(out, t.contiguous())
        return out
    assert not torch.equal(*gathered(fp.flat))              # they do start different
    broadcast_replica_state(fp.flat, list(net.buffers()))
    a, b = gathered(fp.flat)
    assert torch.equal(a, b)
    assert torch.equal(net[0].weight.data, fp.flat[:24].view(4, 6))      # parameters are still views of the flat buffer
    for buf in net.buffers():
        a, b = gathered(buf.detach().to(torch.float64))
        assert torch.equal(a, b), buf
    assert net[1].num_batches_tracked.dtype == torch.int64 and int(net[1].num_batches_tracked) == 3   # rank 0's
    assert float(net[1].running_mean[0]) == 1.0
    # two reduced SGD steps on rank-local batches (BatchNorm in training mode: running statistics drift per rank),
    # with the per-step buffer broadcast TrainStep._enqueue does -> parameters AND buffers equal afterwards
    red = GradReducer(fp.grad, [(0, fp.total)])
    live = [b for k, b in net.named_buffers() if "running_" in k or "num_batches_tracked" in k]
    for step in range(2):
        broadcast_replica_state(None, live)
        x = torch.randn(8, 6, generator=torch.Generator().manual_seed(500 + 10 * step + rank))
        grads = torch.autograd.grad(net(x).pow(2).mean(), list(net.parameters()))
        for (k, _), g in zip(net.named_parameters(), grads):
            fp.gviews[k].copy_(g)
        red.begin()
        red.finish()
        fp.flat.add_(fp.grad, alpha=-0.1 / world)
    broadcast_replica_state(None, live)                      # what distributed evaluation sees
    a, b = gathered(fp.flat)
    assert torch.equal(a, b)
    for buf in net.buffers():
        a, b = gathered(buf.detach().to(torch.float64))
        assert torch.equal(a, b)


replicas_that_start_different_end_equal()

# eval-side collectives (utils_parallel.py:13-64 as used at utils_trainer.py:653-674)
t = torch.tensor([float(rank + 1)], dtype=torch.float64)
assert sync_tensor_across_gpus(t).tolist() == [1.0, 2.0]
assert sync_tensor_across_gpus(None) is None
assert sync_non_tensor_value_across_gpus(3.0 + rank) == 7.0
d = sync_dict_across_gpus({float(10 * rank): torch.tensor(0.5 + rank), float(10 * rank + 1): torch.tensor(2.5 + rank)})
assert {k: float(v) for k, v in d.items()} == {0.0: 0.5, 1.0: 2.5, 10.0: 1.5, 11.0: 3.5}
sums = {"psnr": torch.tensor(30.0 + rank, dtype=torch.float64), "ssim": torch.tensor(0.5 * (rank + 1), dtype=torch.float64)}
tot, n = sync_metric_sums(sums, 4 + rank)
assert float(tot["psnr"]) == 61.0 and float(tot["ssim"]) == 1.5 and n == 9.0
dist.barrier()
dist.destroy_process_group()
print("rank", rank, "ok")
'''


def test_grad_reducer_hook_order_and_eval_collectives_gloo_world2(tmp_path):
    """a20 / SURVEY 8e on CPU: the real GradReducer (the object TrainStep hands to engine.backward as
    on_layer_done) driven by stub engines with every announce pattern the HIP engines use -- each bucket
    is reduced exactly once per step and the result is the rank-mean gradient; the per-step non-finite
    flag is MAX-reduced; the eval metric gathers match the reference's semantics."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = tmp_path / "worker_reducer.py"
    script.write_text(WORKER_REDUCER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="2",
               OMP_NUM_THREADS="1")
    procs = [subprocess.Popen([sys.executable, str(script), ROOT], env=dict(env, RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(2)]
    outs = [p.communicate(timeout=240)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} failed:\n{o}"
        assert f"rank {r} ok" in o


def test_bench_self_launch_relays_worker_failure():
    """`python bench.py --gpus N` is ONE command: outside torchrun the parent starts the N workers under
    torch.distributed.run as child processes (it never touches the GPU itself and never execs), relays
    rank 0's JSON line and propagates failure.  Here there is no GPU: the workers fail, the parent must
    exit non-zero without printing a result line (no fallback, no hang)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1",
                        "--warmup", "0", "--no-cpu-baseline"], capture_output=True, text=True, timeout=300, env=env)
    if torch.cuda.is_available() and torch.cuda.device_count() >= 2:
        assert p.returncode == 0 and '"n_ranks_seen": 2' in p.stdout
    else:
        assert p.returncode != 0
        assert '{"metric"' not in p.stdout
        assert "worker launch failed" in p.stderr


def test_bench_plain_run_and_output_dump(tmp_path):
    """A plain `bench.py` run is the headline and nothing else: the eager rates, roofline, forward-only figures, secondary
    workloads and baselines run only with --full.  --dump-outputs writes float32 .npy files; a vector above the per-array
    cap becomes a sample at the same seeded indices from run to run, so that two builds compare output for output."""
    import bench
    a = bench.parse_args(["--steps", "7"])
    assert a.steps == 7 and not a.full and a.train_only and a.no_roofline and a.dump_outputs is None
    a = bench.parse_args(["--full", "--dump-outputs", str(tmp_path)])
    assert a.full and not a.train_only and not a.no_roofline and not a.no_cpu_baseline and a.dump_outputs == str(tmp_path)
    n = bench.DUMP_MAX_ELEMS + 1000
    big = torch.arange(n, dtype=torch.float64)
    for d in ("a", "b"):
        bench.write_outputs(str(tmp_path / d), {"loss": torch.tensor([0.5, 0.25]), "params": big})
    loss, params = np.load(tmp_path / "a" / "loss.npy"), np.load(tmp_path / "a" / "params.npy")
    assert loss.dtype == np.float32 and loss.tolist() == [0.5, 0.25]
    assert params.dtype == np.float32 and params.shape == (bench.DUMP_MAX_ELEMS,)
    assert np.all(np.diff(params) > 0) and params[-1] < n                  # distinct sorted elements of the vector
    assert np.array_equal(params, np.load(tmp_path / "b" / "params.npy"))
    # what the headline workload dumps (parameters + gradients of SwinIR x8, 7.9 M each) stays under 64 MB
    assert 2 * bench.DUMP_MAX_ELEMS * 4 < 64e6
