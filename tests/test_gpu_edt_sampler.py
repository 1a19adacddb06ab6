"""The 'edt' / 'edt*roi' / Otsu styles of the training-crop sampler on the device (csrc/edt.hip; DeviceWeightedSampler and
ResidentTrainSet in dlib/datasets/dataset_dpsr.py).

EDT: integers, so the gate is equality with rint(scipy_edt ** 2).  Draws: every origin returned for a uniform u brackets u
in the CDF of the probabilities the host PatchSampler hands to np.random.multinomial (g32 pins those against the
reference), within tol = 4 N 2^-53 for N candidates: two summation orders of N positive fp64 terms differ by at most
(N - 1) 2^-53 relative on each side, one-ulp exp / sqrt differences add 2^-52 -- derived, not measured."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import sr_oracle as O

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FX = os.path.join(G, "eval_exp")


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def g32():
    g = np.load(os.path.join(G, "g32_patch_sampler_edt.npz"))
    return {n: (g[f"{n}/img"], int(g[f"{n}/cfg"][0]), int(g[f"{n}/cfg"][1]), g[f"{n}/edt_pvals"], g[f"{n}/edtxroi_pvals"])
            for n in ("a", "b")}


def fixture_tile(i=0):
    from PIL import Image
    return np.array(Image.open(os.path.join(FX, "data", "caco2", "t", f"h_{i}.tif")))


def scipy_d2(fg):
    from scipy.ndimage import distance_transform_edt
    return np.rint(distance_transform_edt(fg) ** 2).astype(np.int32)


EDT_SHAPES = [(1, 1), (1, 17), (17, 1), (7, 5), (33, 29), (40, 52), (128, 136), (300, 257)]


def foregrounds(H, W, rng):
    corner = np.ones((H, W), bool)
    corner[H - 1, 0] = False
    column = np.ones((H, W), bool)
    column[H // 3:, W // 2] = False
    return {"density 0.5": rng.rand(H, W) < 0.5, "density 0.98": rng.rand(H, W) < 0.98, "one corner pixel": corner,
            "one column": column, "all foreground": np.ones((H, W), bool), "all background": np.zeros((H, W), bool)}


@pytest.mark.parametrize("shape", EDT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_edt_sq_equals_scipy(shape):
    from srhip import ops
    H, W = shape
    rng = np.random.RandomState(H * 1000 + W)
    th = 100
    for name, fg in foregrounds(H, W, rng).items():
        img = np.where(fg, rng.randint(th, 256, (H, W)), rng.randint(0, th, (H, W))).astype(np.uint8)
        assert np.array_equal(img >= th, fg)
        buf = torch.full((H * W + 131,), -1, dtype=torch.int32, device="cuda")       # a larger buffer: the tail stays
        out = ops.edt_sq(torch.from_numpy(img).cuda(), th, out=buf)
        assert out is buf
        got = buf.cpu().numpy()
        assert np.array_equal(got[:H * W].reshape(H, W), scipy_d2(fg)), (shape, name)
        assert (got[H * W:] == -1).all(), (shape, name)
    # the images the sampler thresholds: g32 and the fixture tile themselves
    for img, th in [(g32()["a"][0], g32()["a"][2]), (g32()["b"][0], g32()["b"][2]), (fixture_tile(), 12)]:
        if img.shape == shape:
            got = ops.edt_sq(torch.from_numpy(img).cuda(), th).cpu().numpy()
            assert got.dtype == np.int32 and np.array_equal(got, scipy_d2(img >= th))
            assert np.array_equal(ops.edt_sq(torch.from_numpy(img).cuda(), 0).cpu().numpy(), scipy_d2(img >= 0))


def host_cdf(img, th, P, style, th_style="fix_threshold"):
    from dlib.datasets.dataset_dpsr import PatchSampler
    p = PatchSampler(style, P, 256, th_style, float(th)).origin_probabilities(img, th)
    return np.cumsum(p.reshape(-1)), p.reshape(-1)


def uniforms(n, seed):
    u = torch.rand(n, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))
    u[:3] = torch.tensor([0.0, 0.5, 1.0 - 2.0 ** -53], dtype=torch.float64)
    return u


def assert_brackets(org, u, cdf, H, W, P, tag):
    Hc, Wc = H - P, W - P
    N = Hc * Wc
    assert org.shape == (u.size, 2) and (org >= 0).all() and (org[:, 0] < Hc).all() and (org[:, 1] < Wc).all(), tag
    i = org[:, 0].astype(np.int64) * Wc + org[:, 1]
    below = np.where(i > 0, cdf[np.maximum(i - 1, 0)], 0.0)
    tol = 4 * N * 2.0 ** -53
    worst = max((below - u).max(), (u - cdf[i]).max())
    print(tag, "N", N, "tol", tol, "worst excess over the bracket (<= 0: inside)", worst)
    assert (below - tol <= u).all() and (u <= cdf[i] + tol).all(), (tag, worst, tol)


DRAW_TILES = ["a", "b", "fixture"]


def draw_tile(name):
    if name == "fixture":
        return fixture_tile(), 64, 12
    img, P, th, _, _ = g32()[name]
    return img, P, th


@pytest.mark.parametrize("name", DRAW_TILES)
@pytest.mark.parametrize("style", ["edt", "edt*roi"])
def test_origin_draws_bracket_the_host_cdf(name, style):
    from srhip import ops
    from dlib.datasets.dataset_dpsr import DeviceWeightedSampler
    img, P, th = draw_tile(name)
    s = DeviceWeightedSampler([torch.from_numpy(img).cuda()], P, style, thresholds=float(th), seed=1)
    u = uniforms(4096, 5)
    org = ops.origin_sample(s.table, torch.zeros(4096, dtype=torch.int32, device="cuda"), u).cpu().numpy()
    cdf, _ = host_cdf(img, float(th), P, style)
    assert_brackets(org, u.cpu().numpy(), cdf, img.shape[0], img.shape[1], P, f"{name} {style}")
    again = ops.origin_sample(s.table, torch.zeros(4096, dtype=torch.int32, device="cuda"), u).cpu().numpy()
    assert np.array_equal(org, again)                         # no atomics: identical run to run


def test_threshold_zero_draws_as_the_reference():
    """every pixel foreground: scipy's virtual-pixel distances are the ones the reference's probabilities hold"""
    from srhip import ops
    from dlib.datasets.dataset_dpsr import DeviceWeightedSampler
    img, P, _ = draw_tile("b")
    for style in ("edt", "edt*roi"):
        s = DeviceWeightedSampler([torch.from_numpy(img).cuda()], P, style, thresholds=0., seed=1)
        u = uniforms(4096, 6)
        org = ops.origin_sample(s.table, torch.zeros(4096, dtype=torch.int32, device="cuda"), u).cpu().numpy()
        cdf, _ = host_cdf(img, 0., P, style)
        assert_brackets(org, u.cpu().numpy(), cdf, img.shape[0], img.shape[1], P, f"b th 0 {style}")


@pytest.mark.parametrize("style,k", [("edt", 3), ("edt*roi", 4)])
def test_origin_distribution_is_the_reference(style, k):
    from srhip import ops
    from dlib.datasets.dataset_dpsr import DeviceWeightedSampler
    img, P, th = draw_tile("b")
    p = g32()["b"][k]
    s = DeviceWeightedSampler([torch.from_numpy(img).cuda()], P, style, thresholds=float(th), seed=2)
    n = 200000
    org, u = s.sample(torch.zeros(n, dtype=torch.int32, device="cuda"))
    org = org.cpu().numpy()
    freq = np.bincount(org[:, 0].astype(np.int64) * (img.shape[1] - P) + org[:, 1], minlength=p.size) / n
    print(style, "max |freq - p|", np.abs(freq - p).max(), "gate", 6.0 * np.sqrt(p.max() / n))
    assert np.abs(freq - p).max() <= 6.0 * np.sqrt(p.max() / n)      # 6 sigma of the largest cell


def test_hist_u8_and_otsu_roi_on_a_mixed_batch():
    from srhip import ops
    from dlib.datasets.lowres import otsu_threshold
    from dlib.datasets.dataset_dpsr import DeviceWeightedSampler, int_threshold
    rng = np.random.RandomState(3)
    bimodal = np.where(rng.rand(300, 257) < 0.3, rng.randint(150, 200, (300, 257)), rng.randint(5, 40, (300, 257))).astype(np.uint8)
    imgs = [g32()["a"][0], g32()["b"][0], fixture_tile(), bimodal]
    for img in imgs + [np.full((5, 3), 255, np.uint8), np.zeros((1, 1), np.uint8)]:
        got = ops.hist_u8(torch.from_numpy(img).cuda()).cpu().numpy()
        assert got.dtype == np.int32 and np.array_equal(got, np.bincount(img.reshape(-1), minlength=256))
    P = 8
    tiles = [torch.from_numpy(i).cuda() for i in imgs]
    s = DeviceWeightedSampler(tiles, P, "roi", thresholds=None, seed=4)
    ths = [otsu_threshold(i, 256) for i in imgs]
    assert s.thresholds == [int_threshold(t) for t in ths] and len(set(s.thresholds)) > 1, s.thresholds
    ids = [(7 * b) % 4 for b in range(4096)]                  # the four tiles interleaved in one launch
    u = uniforms(4096, 7)
    org = ops.origin_sample(s.table, torch.tensor(ids, dtype=torch.int32).cuda(), u).cpu().numpy()
    ids, u = np.array(ids), u.cpu().numpy()
    for k, (img, th) in enumerate(zip(imgs, ths)):
        cdf, _ = host_cdf(img, th, P, "roi", "automatic_threshold")
        assert_brackets(org[ids == k], u[ids == k], cdf, img.shape[0], img.shape[1], P, f"otsu roi tile {k}")
    # through the object: ids as a list, seeded uniforms returned
    org, u = s.sample([3, 0, 2, 1, 1])
    assert org.shape == (5, 2) and u.shape == (5,) and org.dtype == torch.int32 and org.is_cuda


def _args(style, th_style):
    import yaml
    from dlib.utils.tools import Dict2Obj
    a = Dict2Obj(yaml.safe_load(open(os.path.join(FX, "exp", "config_model.yml"))))
    a.train_dsets, a.data_root, a.splits_root = a.test_dsets, os.path.join(FX, "data"), os.path.join(FX, "folds")
    a.h_size, a.batch_size, a.myseed = 64, 2, 3
    a.sample_tr_patch, a.sample_tr_patch_th_style, a.sample_tr_patch_th = style, th_style, 12
    return a


@pytest.mark.parametrize("style,th_style", [("edt", "fix_threshold"), ("edt*roi", "fix_threshold"),
                                            ("roi", "automatic_threshold")])
def test_resident_train_set_draws_on_the_device(style, th_style, monkeypatch):
    from PIL import Image
    from dlib.utils.utils_dataloaders import get_train_set
    from dlib.datasets.dataset_dpsr import PatchSampler
    monkeypatch.delenv("SRHIP_HOST_SAMPLER", raising=False)
    a = _args(style, th_style)
    raw_h = [fixture_tile(i) for i in range(3)]
    raw_l = [np.asarray(Image.open(os.path.join(FX, "data", "caco2", "t", f"l_{i}.tif"))) for i in range(3)]
    ts = get_train_set(a, "cuda")
    assert ts.host_sampler is None and ts.device_weighted and len(ts.weighted.thresholds) == 3
    if th_style == "fix_threshold":
        assert ts.weighted.thresholds == [12, 12, 12]
    origins, seen = [], set()
    for epoch in range(3):
        for b in ts.epoch(epoch):
            assert b["h_im"].shape == (2, 1, 64, 64) and b["l_im"].shape == (2, 1, 8, 8)
            for k in range(2):
                i = int(b["h_id"][k].split("_")[1].split(".")[0])
                (r0, c0), mode = b["origin"][k], b["mode"][k]
                assert 0 <= r0 < 128 - 64 and 0 <= c0 < 136 - 64 and 0 <= mode <= 7
                want_h = O.patch_batch([torch.from_numpy(raw_h[i].copy())], [0], [r0], [c0], [mode], 64)
                want_l = O.patch_batch([torch.from_numpy(raw_l[i].copy())], [0], [r0 // 8], [c0 // 8], [mode], 8)
                assert torch.equal(b["h_im"][k:k + 1].cpu(), want_h) and torch.equal(b["l_im"][k:k + 1].cpu(), want_l)
                seen.add(i)
            origins.append(b["origin"])
    assert seen == {0, 1, 2}
    same = get_train_set(a, "cuda")
    assert [b["origin"] for e in range(3) for b in same.epoch(e)] == origins           # same seed, same origins
    # generator seeding myseed + rank: two ranks of a 2-replica run (one sample each per epoch) draw different origins
    # for the SAME tiles, two sets of one rank the same
    a.batch_size = 1
    ranks = [get_train_set(a, "cuda", rank=r, world=2) for r in (0, 1, 1)]
    assert all(t.host_sampler is None and len(t) == 1 for t in ranks)
    draws = [t.weighted.sample([0, 1, 2] * 8)[0].cpu().tolist() for t in ranks]
    assert draws[1] == draws[2] and draws[0] != draws[1]
    a.batch_size = 2
    monkeypatch.setenv("SRHIP_HOST_SAMPLER", "1")
    host = get_train_set(a, "cuda")
    assert isinstance(host.host_sampler, PatchSampler) and not host.device_weighted
    b = next(iter(host.epoch(0)))
    assert b["h_im"].shape == (2, 1, 64, 64)


def test_non_finite_total_names_the_tile():
    """a 1500-pixel-wide foreground band: exp(distance) overflows on its axis, as in the reference (NaN probabilities)"""
    from dlib.datasets.dataset_dpsr import DeviceWeightedSampler
    img = np.full((24, 1500), 200, np.uint8)
    img[:, 0] = 0
    t = torch.from_numpy(img).cuda()
    with pytest.raises(ValueError, match="wide_tile"):
        DeviceWeightedSampler([t], 8, "edt*roi", thresholds=100., names=["wide_tile"])
    DeviceWeightedSampler([t], 8, "edt", thresholds=100., names=["wide_tile"])          # no exponential: fine


def test_bad_arguments_are_refused_before_any_launch():
    from srhip._lib import lib
    from srhip.ops import _OriginTile
    img = torch.zeros(8, 8, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(64, dtype=torch.int32, device="cuda")
    d2 = torch.full((64,), -7, dtype=torch.int32, device="cuda")
    rowcum = torch.full((8,), -7.0, dtype=torch.float64, device="cuda")
    org = torch.full((4, 2), -7, dtype=torch.int32, device="cuda")
    ids = torch.zeros(4, dtype=torch.int32, device="cuda")
    u = torch.zeros(4, dtype=torch.float64, device="cuda")
    p = lambda t: t.data_ptr()

    def refused(rc, word):
        assert rc < 0 and word in lib.srhip_last_error().decode(), (rc, lib.srhip_last_error())

    # a side above 16384, by shape only (the buffers are 8 x 8: nothing may be launched)
    refused(lib.srhip_edt_sq(p(img), 16385, 8, 1, p(ws), p(d2), None), "16384")
    refused(lib.srhip_edt_sq(p(img), 8, 20000, 1, p(ws), p(d2), None), "16384")
    refused(lib.srhip_edt_sq(p(img), 0, 8, 1, p(ws), p(d2), None), "16384")
    refused(lib.srhip_edt_sq(None, 8, 8, 1, p(ws), p(d2), None), "NULL")
    refused(lib.srhip_edt_sq(p(img), 8, 8, 1, None, p(d2), None), "NULL")
    refused(lib.srhip_edt_sq(p(img), 8, 8, 1, p(ws), None, None), "NULL")
    refused(lib.srhip_edt_sq(p(img), 8, 8, 1, p(d2), p(d2), None), "aliases")
    refused(lib.srhip_hist_u8(None, 64, p(ws), None), "NULL")
    refused(lib.srhip_hist_u8(p(img), 64, None, None), "NULL")
    refused(lib.srhip_hist_u8(p(img), 0, p(ws), None), "pixel count")

    def tile(**kw):
        f = dict(img=p(img), d2=p(d2), rowcum=p(rowcum), H=8, W=8, threshold=1, P=4, style=1, pad_=0)
        f.update(kw)
        return _OriginTile(**f)

    for bad, word in ((tile(P=8), "exceed the patch"), (tile(P=9), "exceed the patch"), (tile(P=0), "exceed the patch"),
                      (tile(H=16385), "16384"), (tile(style=3), "style"), (tile(img=None), "NULL"),
                      (tile(d2=None), "NULL"), (tile(rowcum=None), "NULL")):
        refused(lib.srhip_origin_rowcum(ctypes.addressof(bad), None), word)
    refused(lib.srhip_origin_rowcum(None, None), "NULL")
    table = torch.zeros(48, dtype=torch.uint8, device="cuda")
    refused(lib.srhip_origin_sample(None, 1, p(ids), p(u), 4, p(org), None), "NULL")
    refused(lib.srhip_origin_sample(p(table), 1, None, p(u), 4, p(org), None), "NULL")
    refused(lib.srhip_origin_sample(p(table), 1, p(ids), None, 4, p(org), None), "NULL")
    refused(lib.srhip_origin_sample(p(table), 1, p(ids), p(u), 4, None, None), "NULL")
    refused(lib.srhip_origin_sample(p(table), 0, p(ids), p(u), 4, p(org), None), "empty")
    refused(lib.srhip_origin_sample(p(table), 1, p(ids), p(u), 0, p(org), None), "empty")
    torch.cuda.synchronize()
    assert (d2 == -7).all() and (rowcum == -7.0).all() and (org == -7).all() and (ws == 0).all()    # nothing ran
