"""GPU side of the test modes: the two kernels of csrc/tta.hip alone, dlib/utils/utils_model.py against the reference's
outputs on the exact toy model (tests/golden/g54_test_modes.npz), against the one-forward-per-tile composition on real
nets, and through ModelPlain and eval.py."""
import os
import shutil

import numpy as np
import pytest
import torch
import yaml

import test_modes_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = R.load_golden(os.path.join(ROOT, "tests", "golden", R.GOLDEN))
FX = os.path.join(ROOT, "tests", "golden", "eval_exp")


def _planes(shape, seed, misalign=False):
    """random float32 planes on the GPU; misalign: the first element sits 4 bytes behind a 16-byte boundary"""
    g = torch.Generator().manual_seed(seed)
    n = int(np.prod(shape))
    buf = torch.empty(n + 4, dtype=torch.float32, device="cuda")
    x = buf[1:n + 1] if misalign else buf[:n]
    x.copy_(torch.rand(n, generator=g) * 2.0)
    assert x.data_ptr() % 16 == (4 if misalign else 0)
    return x.view(shape)


def _want_tile(src, job, th, tw):
    y0, x0, h, w, m = job
    v = R.view(src[..., y0:y0 + h, x0:x0 + w], m)
    return torch.nn.ReplicationPad2d((0, tw - v.shape[-1], 0, th - v.shape[-2]))(v)


# ---- the kernels alone -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("misalign", [False, True])
def test_gather_every_view_padded(misalign):
    from srhip import ops
    src = _planes((2, 5, 9), 1, misalign)
    for turning, (th, tw) in ((0, (8, 12)), (1, (12, 8))):
        jobs = [(0, 0, 5, 9, m) for m in range(8) if m & 1 == turning]
        out = None
        if misalign:
            out = _planes((len(jobs), 2, th, tw), 2, True)
        got = ops.view_gather(src, jobs, th, tw, out=out)
        assert got.shape == (len(jobs), 2, th, tw)
        for q, job in enumerate(jobs):
            assert torch.equal(got[q], _want_tile(src, job, th, tw)), job


@pytest.mark.parametrize("th,tw", [(72, 132), (71, 133), (132, 72), (131, 75)])
def test_gather_rectangles_over_several_blocks(th, tw):
    """sub-rectangles at odd origins, tiles of more than one 64 x 64 block, widths that are and are not multiples of 4, and
    views of both kinds in one launch where they fit"""
    from srhip import ops
    src = _planes((3, 75, 140), 3)
    rects = [(3, 5, 70, 131), (0, 0, 64, 128), (5, 9, 1, 1), (10, 7, 65, 129)]
    jobs = [r + (m,) for r in rects for m in range(8)
            if (r[3] if m & 1 else r[2]) <= th and (r[2] if m & 1 else r[3]) <= tw]
    assert len(jobs) >= 12
    got = ops.view_gather(src, jobs, th, tw)
    for q, job in enumerate(jobs):
        assert torch.equal(got[q], _want_tile(src, job, th, tw)), job


def test_merge_of_one_view_is_a_crop():
    from srhip import ops
    tiles = _planes((1, 2, 8 * 3, 12 * 3), 4)
    got = ops.view_merge([(tiles, 0, 8, 12, [(5, 9)])], 2, 5, 9, 3)
    assert torch.equal(got, tiles[0, :, :15, :27])


def _eight_views(N, H, W, sf, th, tw, seed):
    views = []
    for m in range(8):
        fh, fw = (W, H) if m & 1 else (H, W)
        t = (tw, th) if m & 1 else (th, tw)
        views.append((_planes((1, N, t[0] * sf, t[1] * sf), seed + m), m, t[0], t[1], [(fh, fw)]))
    return views


def test_merge_of_eight_views_is_their_mean_and_repeats_bit_for_bit():
    from srhip import ops
    N, H, W, sf = 2, 5, 9, 2
    views = _eight_views(N, H, W, sf, 8, 12, 10)
    got = ops.view_merge(views, N, H, W, sf)
    terms = [R.view(t[0][..., :lv[0][0] * sf, :lv[0][1] * sf], R.INVERSE[m]) for t, m, _, _, lv in views]
    want = torch.stack(terms, dim=0).mean(dim=0)
    err = (got - want).abs().max().item()
    print(f"merge K=8: max |kernel - stack().mean()| = {err:.3g}")
    # eight f32 terms below 2: two summation orders differ by at most 7 * 2^-24 * 16 = 6.7e-6 before the division by 8
    assert err <= 1e-6
    # the kernel's own order, k = 0 .. 7, restated: bit for bit
    acc = torch.zeros_like(terms[0])
    for t in terms:
        acc = acc + t
    assert torch.equal(got, acc * 0.125)
    assert torch.equal(ops.view_merge(views, N, H, W, sf), got)


def test_merge_descends_the_quadtree():
    """two levels of a 21 x 27 split under view 5, against the assembly by slices"""
    from srhip import ops
    from dlib.utils import utils_model as um
    N, H, W, sf, m = 2, 27, 21, 2, 5                   # the view's frame is 21 x 27
    levels, (th, tw) = um.split_levels(21, 27, 4, 8, 1)
    tiles = _planes((16, N, th * sf, tw * sf), 20)
    plan = um.split_plan(21, 27, 4, 8, 1)
    E = torch.zeros(N, 21 * sf, 27 * sf, device="cuda")
    for leaf, t in zip(plan, tiles):
        (sy, sx, _, _), (y0, x0, h, w) = leaf["src"], leaf["dst"]
        E[:, y0 * sf:(y0 + h) * sf, x0 * sf:(x0 + w) * sf] = t[:, (y0 - sy) * sf:(y0 - sy + h) * sf, (x0 - sx) * sf:(x0 - sx + w) * sf]
    got = ops.view_merge([(tiles, m, th, tw, levels)], N, H, W, sf)
    assert torch.equal(got, R.view(E, R.INVERSE[m]))


def test_argument_checks_raise():
    from srhip import ops
    from srhip._lib import call
    import ctypes
    src = _planes((2, 5, 9), 30)
    for jobs, th, tw in (([(0, 0, 5, 9, 8)], 8, 12), ([(0, 0, 5, 9, -1)], 8, 12), ([(1, 0, 5, 9, 0)], 8, 12),
                         ([(0, 1, 5, 9, 0)], 8, 12), ([(-1, 0, 5, 9, 0)], 8, 12), ([(0, 0, 0, 9, 0)], 8, 12),
                         ([(0, 0, 5, 9, 0)], 4, 12), ([(0, 0, 5, 9, 0)], 8, 8), ([(0, 0, 5, 9, 1)], 8, 12)):
        with pytest.raises(ops.SrhipError):
            ops.view_gather(src, jobs, th, tw)
    with pytest.raises(ops.SrhipError):                 # out overlaps src
        ops.view_gather(src, [(0, 0, 5, 9, 0)], 5, 9, out=src)
    host = (ops._ViewJob * 1)(ops._ViewJob(0, 0, 5, 9, 0))
    out = torch.empty(1, 2, 8, 12, device="cuda")
    with pytest.raises(ops.SrhipError, match="on the device"):      # the job table on the host
        call("srhip_view_gather", src.data_ptr(), 2, 5, 9, ctypes.addressof(host), ctypes.addressof(host), 1, out.data_ptr(), 8,
             12, torch.cuda.current_stream().cuda_stream)
    tiles = _planes((1, 2, 8, 12), 31)
    ok = (tiles, 0, 8, 12, [(5, 9)])
    assert ops.view_merge([ok], 2, 5, 9, 1).shape == (2, 5, 9)
    for bad in ((tiles, 8, 8, 12, [(5, 9)]), (tiles, 1, 8, 12, [(5, 9)]), (tiles, 0, 8, 12, [(9, 5)]),
                (_planes((1, 2, 4, 12), 32), 0, 4, 12, [(5, 9)])):
        with pytest.raises(ops.SrhipError):
            ops.view_merge([bad], 2, 5, 9, 1)
    with pytest.raises(ops.SrhipError):                 # a quadrant that does not reach the half it owns
        ops.view_merge([(_planes((4, 2, 8, 12), 33), 0, 8, 12, [(21, 27), (8, 12)])], 2, 21, 27, 1)
    with pytest.raises(ops.SrhipError):                 # dst inside the tiles
        ops.view_merge([ok], 2, 5, 9, 1, out=tiles.view(-1)[:90].view(2, 5, 9))
    with pytest.raises(ops.SrhipError):
        ops.view_merge([ok] * 9, 2, 5, 9, 1)


# ---- the modes on the exact toy model: the reference's bits ----------------------------------------------------------
@pytest.mark.parametrize("max_batch", [8, 1, 3])
@pytest.mark.parametrize("name", list(R.CASES))
def test_modes_reproduce_the_reference_on_the_toy_model(name, max_batch):
    from dlib.utils import utils_model as um
    _, refield, min_size, sf, modulo = R.CASES[name]
    L = torch.from_numpy(GOLD[name]["L"]).cuda()
    seen = []

    def model(x):
        seen.append(x.shape[0])
        return R.toy_model(sf)(x)
    for mode in range(5):
        del seen[:]
        E = um.test_mode(model, L, mode, refield=refield, min_size=min_size, sf=sf, modulo=modulo, max_batch=max_batch)
        assert E.shape == GOLD[name][f"E{mode}"].shape
        assert torch.equal(E.cpu(), torch.from_numpy(GOLD[name][f"E{mode}"])), (name, mode)
        if mode:
            assert max(seen) <= max_batch
    # mode 4 of the last loop: every tile-image went through the model once
    n_tiles = len(GOLD[name]["tiles"]) * 8 * L.shape[0]
    assert sum(seen) == n_tiles


# ---- real nets: batched tiles against one forward per tile -----------------------------------------------------------
def _swinir():
    from dlib.models.network_swinir import SwinIR
    torch.manual_seed(3)
    net = SwinIR(upscale=2, in_chans=1, img_size=16, window_size=8, depths=[2], embed_dim=60, num_heads=[6], mlp_ratio=2,
                 upsampler="pixelshuffledirect")
    return net.cuda().eval()


def _edsr():
    from dlib.models.network_edsr_liif import EDSR_LIIF
    torch.manual_seed(4)
    return EDSR_LIIF(scale=2, n_resblocks=1, n_feats=16, res_scale=1.0).cuda().eval()


@pytest.mark.parametrize("make", [_swinir, _edsr], ids=["swinir", "edsr"])
def test_real_nets_match_the_sequential_composition(make):
    """test_x8 on 2 x 1 x 16 x 24 (two tile shapes) and test_split_x8 on 1 x 1 x 40 x 56 (refield 8, min_size 16: two levels,
    16 x 24 leaves).  The composition is the restatement: net() and torch ops, one forward per view or tile.  Gate: mean
    absolute difference <= 1e-5, the project's parity tolerance (a batched and a single forward may pick different block
    exponents: bit equality is not asked); the maximum is printed."""
    from dlib.utils import utils_model as um
    net = make()
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for shape, mode, kw in (((2, 1, 16, 24), 3, dict(modulo=1)), ((1, 1, 40, 56), 4, dict(refield=8, min_size=16, modulo=1))):
            L = torch.rand(shape, generator=g).cuda()
            got = um.test_mode(net, L, mode, sf=2, **kw)
            want = R.ref_test_mode(lambda x: net(x.contiguous()).clone(), L, mode, sf=2, **kw)
            assert got.shape == want.shape == (shape[0], 1, 2 * shape[2], 2 * shape[3])
            d = (got - want).abs()
            print(f"{make.__name__[1:]} mode {mode} {shape}: mean |batched - sequential| = {d.mean().item():.3g}, max "
                  f"{d.max().item():.3g}, mean |output| = {want.abs().mean().item():.3g}")
            assert torch.isfinite(got).all() and d.mean().item() <= 1e-5
            plain = net(L)
            assert not torch.equal(got, plain.reshape(got.shape))


# ---- ModelPlain and eval.py ------------------------------------------------------------------------------------------
class Args(dict):
    __getattr__ = dict.get


def test_model_plain_testx8(tmp_path):
    from dlib.utils import constants
    from dlib.models.select_model import define_model
    netG = {'net_type': constants.SWINIR, 'swinir_upscale': 8, 'swinir_in_chans': 1, 'swinir_img_size': 16,
            'swinir_window_size': 8, 'swinir_img_range': 1.0, 'swinir_depths': [2], 'swinir_embed_dim': 60,
            'swinir_num_heads': [6], 'swinir_mlp_ratio': 2, 'swinir_upsampler': constants.US_PIXEL_SHUFFLE_DIRECT,
            'swinir_resi_connection': constants.R_CONNECTION_1CONV}
    args = Args(netG=netG, train={}, is_train=False, scale=8, outd=str(tmp_path))
    torch.manual_seed(5)
    model = define_model(args)
    model.netG.train()
    g = torch.Generator().manual_seed(6)
    model.feed_data({'l_im': torch.rand(2, 1, 16, 24, generator=g), 'h_im': torch.rand(2, 1, 128, 192, generator=g)})
    model.testx8()
    assert model.netG.training
    e8 = model.E.clone()
    assert e8.shape == (2, 1, 128, 192) and torch.isfinite(e8).all()
    model.test_tta(3)
    assert model.netG.training and torch.equal(model.E, e8)
    model.test()
    plain = model.E.clone()
    assert plain.shape == e8.shape and not torch.equal(plain, e8)
    model.test_tta(0)
    assert torch.equal(model.E, plain)
    assert set(model.current_visuals()) == {'L', 'E', 'H'}


def test_eval_py_test_mode_3_runs_on_the_fixture(tmp_path, monkeypatch):
    """eval.py --test_mode 3 on the evaluation fixture: runs through, every batch of the model row goes through
    ModelPlain.test_tta(3), the metrics written are finite, and the bicubic row is what it was (the flag does not touch it)."""
    import importlib.util
    from dlib.models.model_plain import ModelPlain
    calls, inner = [], ModelPlain.test_tta

    def counted(self, mode, **kw):
        calls.append((mode, kw))
        return inner(self, mode, **kw)
    monkeypatch.setattr(ModelPlain, "test_tta", counted)
    exp = tmp_path / "exp"
    shutil.copytree(os.path.join(FX, "exp"), exp)
    spec = importlib.util.spec_from_file_location("srhip_eval_tta", os.path.join(ROOT, "sr-caco-2_amd", "eval.py"))
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)
    ev.evaluate_pretrained(["--cudaid", "0", "--exp_path", str(exp), "--data_root", os.path.join(FX, "data"), "--splits_root",
                            os.path.join(FX, "folds"), "--test_mode", "3"])
    ds = "caco2_test_X_8_in_64_out_512_cell_CELL0"
    assert "test mode 3" in open(exp / f"eval_test_{ds}" / "log.txt").read()
    assert calls == [(3, dict(refield=32, min_size=256))] * 2             # the loader's two batches
    want = os.path.join(FX, "expected", "best-models")
    for name, same in ((ds, False), (f"{ds}_bicubic", True)):
        got = yaml.safe_load(open(exp / "best-models" / f"details_{name}.yml"))
        ref = yaml.safe_load(open(os.path.join(want, f"details_{name}.yml")))
        assert list(got) == list(ref)
        for img in ref:
            assert all(np.isfinite(got[img][m]) for m in ("psnr", "mse", "nrmse", "ssim", "psnr_y"))
            if same:
                assert abs(got[img]["psnr"] - ref[img]["psnr"]) <= 0.01, (name, img, got[img]["psnr"], ref[img]["psnr"])
