"""--da_device on the GPU: ops.lr_augment (srhip_lr_augment, csrc/augment.hip) against its numpy statement
(lr_augment_ref.py: the reference's three LR-only augmentations with the library's draws), stage by stage and all three, and
ResidentTrainSet with the option on.

Bounds, per pixel, from the arithmetic -- not from what the kernels give:
  decisions  exact: the cases keep every cut 1e-9 away from its threshold (test_lr_augment.py asserts it), so the device's
             log / cos cannot move one;
  dot        bit-equal: a float32 product with 0 or 1;
  blur       2 * 2^-24: each of the two image passes is a convex combination of values in [0, 1] summed in float64 and rounded
             once to float32, at most one float32 spacing at 1.0 per pass and none amplified (the order of the sums is scipy's,
             so 0 is expected: the maximum is printed);
  noise      one float32 spacing of the expected value: a float64 libm difference can only move the one final rounding a step;
  all three  the sum of the two."""
import os

import numpy as np
import pytest
import torch

import lr_augment_ref as R

pytestmark = pytest.mark.gpu
BLUR_BOUND = 2.0 * 2.0 ** -24
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def run(x, seed, params, weights=None):
    from srhip import ops
    xd = torch.from_numpy(np.array(x, copy=True)).cuda()
    sd = torch.tensor([seed], dtype=torch.int64).cuda()
    return ops.lr_augment(xd, sd, params, weights).cpu().numpy()


def bound_of(params, want):
    b_on, d_on, g_on = (p[0] for p in params)
    tol = np.zeros(want.shape, dtype=np.float64)
    if b_on:
        tol += BLUR_BOUND
    if g_on:
        tol += np.spacing(np.abs(want)).astype(np.float64)
    return tol


def block_mask(h, w, dec):
    m = np.zeros((h, w), dtype=bool)
    m[dec[1]:dec[1] + dec[3], dec[2]:dec[2] + dec[4]] = True
    return m


@pytest.mark.parametrize("shape", range(len(R.SHAPES)), ids=[f"{B}x{h}x{w}-s{s:g}" for B, h, w, s in R.SHAPES])
def test_lr_augment_equals_the_statement_stage_by_stage_and_together(shape):
    B0, h0, w0, s0 = R.SHAPES[shape]
    worst = {"blur": 0.0, "dot": 0.0, "gaus": 0.0, "all": 0.0}
    n = 0
    for k, (name, B, h, w, params, seed) in enumerate(R.cases()):
        if not name.startswith(f"{B0}x{h0}x{w0}-s{s0:g}-"):
            continue
        mode = name.split("-")[2]
        x, want, decs, margin = R.case_reference(k)
        got = run(x, seed, params)
        d = np.abs(got.astype(np.float64) - want.astype(np.float64))
        worst[mode] = max(worst[mode], float(d.max()))
        assert np.all(d <= bound_of(params, want)), (name, float(d.max()))
        if mode == "dot":
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name                 # bit-equal
        # decisions, exactly: the pixels a stage touched are the statement's
        assert np.array_equal(got != x, want != x), name
        for b in range(B):
            applied = [dec[0] for dec in decs[b]]
            if not any(applied):                          # stage off, area 0 or prob 0: the sample keeps its bits
                assert np.array_equal(got[b].view(np.uint32), x[b].view(np.uint32)), (name, b)
            if mode == "all":
                continue
            dec = decs[b][R.MODES.index(mode)]
            if not dec[0]:
                continue
            blk = block_mask(h, w, dec)
            same = got[b, 0].view(np.uint32) == x[b, 0].view(np.uint32)
            if mode == "blur":                            # inside: only the block moves; outside: the block keeps its bits
                assert np.all(same[~blk]) if dec[5] else np.all(same[blk]), (name, b)
            else:
                assert np.all(same[~blk]), (name, b)
                value = params[R.MODES.index(mode)][3]
                if value == 0:                            # p = 0 keeps every pixel, std = 0 leaves the block bit-identical
                    assert np.all(same), (name, b)
                elif mode == "gaus":                      # std > 0: every pixel of the block that the statement moves, moves
                    assert np.array_equal(~same, want[b, 0] != x[b, 0]), (name, b)
        n += 1
    assert n == len(R.MODES) * len(R.VALUES)
    print(f"lr_augment {B0}x{h0}x{w0} sigma {s0:g}: max |got - statement| per mode {worst} "
          f"(blur bound {BLUR_BOUND:.3e}, {n} cases)")


def test_lr_augment_all_stages_off_and_batch_independence():
    from srhip import ops
    k = next(i for i, c in enumerate(R.cases()) if c[0].startswith("3x5x7-s3-all-1-0.3-0.5-0.05"))
    name, B, h, w, params, seed = R.cases()[k]
    x, want, decs, _ = R.case_reference(k)
    off = run(x, seed, (R.OFF, R.OFF, R.OFF))
    assert np.array_equal(off.view(np.uint32), x.view(np.uint32))
    # sample 0 alone (a batch of 1) has the bits it has in the batch of 3: nothing depends on B
    whole, alone = run(x, seed, params), run(x[:1], seed, params)
    assert np.array_equal(whole[:1].view(np.uint32), alone.view(np.uint32))
    # x at an address that is no multiple of 16 bytes (the scalar form of the compose launch): the same bits
    buf = torch.zeros(x.size + 1, dtype=torch.float32).cuda()
    view = buf[1:].view(B, 1, h, w)
    view.copy_(torch.from_numpy(np.array(x)).cuda())
    assert view.data_ptr() % 16 == 4
    ops.lr_augment(view, torch.tensor([seed], dtype=torch.int64).cuda(), params)
    assert np.array_equal(view.cpu().numpy().view(np.uint32), whole.view(np.uint32)) and buf[0].item() == 0.0
    # weights built once by the caller give what the call builds itself
    wts = ops.lr_blur_weights(params[0][3], "cuda")
    assert np.array_equal(wts.cpu().numpy(), R.blur_weights(params[0][3]))
    assert np.array_equal(run(x, seed, params, wts).view(np.uint32), whole.view(np.uint32))


def test_lr_augment_refuses_what_it_cannot_run():
    from srhip import ops
    x = torch.rand(1, 1, 8, 8).cuda()
    sd = torch.tensor([1], dtype=torch.int64).cuda()
    on = (True, 1.0, 0.3, 1.0)
    for params, what in ((((True, 1.0, 0.3, 16.2), R.OFF, R.OFF), "radius"), (((True, 1.5, 0.3, 1.0), R.OFF, R.OFF), "prob"),
                         ((R.OFF, (True, 1.0, -0.1, 0.5), R.OFF), "area"), ((R.OFF, (True, 1.0, 0.3, 1.0), R.OFF), "p < 1"),
                         ((R.OFF, R.OFF, (True, 1.0, 0.3, -0.05)), "std")):
        keep = x.clone()
        with pytest.raises((ops.SrhipError, ValueError), match=what):
            ops.lr_augment(x, sd, params)
        assert torch.equal(x, keep)
    with pytest.raises(ops.SrhipError, match="seed"):
        ops.lr_augment(x, sd.int(), (on, R.OFF, R.OFF))
    with pytest.raises(ops.SrhipError, match="contiguous float32"):
        ops.lr_augment(x[:, :, :, ::2], sd, (on, R.OFF, R.OFF))
    with pytest.raises(ops.SrhipError, match="blur_weights"):
        ops.lr_augment(x, sd, (on, R.OFF, R.OFF), ops.lr_blur_weights(2.0, "cuda"))


def test_lr_augment_captured_launches_read_the_seed_at_replay():
    """the launches of one call, captured on one stream; after the seed tensor is overwritten a replay gives the statement's
    result for the new seed"""
    from srhip import ops
    k = next(i for i, c in enumerate(R.cases()) if c[0].startswith("3x16x12-s1-all-1-0.3-0.5-0.05"))
    name, B, h, w, params, seed = R.cases()[k]
    x, want, _, _ = R.case_reference(k)
    x0 = torch.from_numpy(np.array(x)).cuda()
    xs, sd = x0.clone(), torch.tensor([seed], dtype=torch.int64).cuda()
    wts = ops.lr_blur_weights(params[0][3], "cuda")
    ops.lr_augment(xs.clone(), sd, params, wts)                   # the workspace exists before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.lr_augment(xs, sd, params, wts)
    other = seed ^ 0x5DEECE66D1234567
    want_other, _ = R.augment_batch(x, other, params)
    assert not np.array_equal(want_other, want)
    for s, w_ in ((other, want_other), (seed, want)):
        xs.copy_(x0)
        sd.fill_(s)
        graph.replay()
        d = np.abs(xs.cpu().numpy().astype(np.float64) - w_.astype(np.float64))
        assert np.all(d <= bound_of(params, w_)), (s, float(d.max()))


def _fixture_args(**kw):
    import yaml
    from dlib.utils.tools import Dict2Obj
    fx = os.path.join(G, "eval_exp")
    a = Dict2Obj(yaml.safe_load(open(os.path.join(fx, "exp", "config_model.yml"))))
    a.train_dsets, a.data_root, a.splits_root = a.test_dsets, os.path.join(fx, "data"), os.path.join(fx, "folds")
    a.h_size, a.batch_size, a.myseed = 64, 2, 3
    a.sample_tr_patch = "uniform"
    for k, v in kw.items():
        a[k] = v
    return a


DA_ON = dict(da_device=True, da_blur=True, da_blur_prob=1.0, da_blur_area=0.3, da_blur_sigma=1.0,
             da_dot_bin_noise=True, da_dot_bin_noise_prob=1.0, da_dot_bin_noise_area=0.4, da_dot_bin_noise_p=0.3,
             da_add_gaus_noise=True, da_add_gaus_noise_prob=1.0, da_add_gaus_noise_area=0.5, da_add_gaus_noise_std=0.05)


def test_resident_train_set_with_da_device():
    from cv2_cubic import resize_cubic
    from dlib.utils.utils_dataloaders import get_train_set
    plain = get_train_set(_fixture_args(), "cuda")
    dev, again = get_train_set(_fixture_args(**DA_ON), "cuda"), get_train_set(_fixture_args(**DA_ON), "cuda")
    assert dev.da_device and not plain.da_device and dev.da_weights.dtype == torch.float64
    params = ((True, 1.0, 0.3, 1.0), (True, 1.0, 0.4, 0.3), (True, 1.0, 0.5, 0.05))
    assert dev.da_params == params
    n, seeds = 0, []
    for pb, nb, ab in zip(plain.epoch(0), dev.epoch(0), again.epoch(0)):
        assert pb["origin"] == nb["origin"] and pb["mode"] == nb["mode"]          # the crop stream did not move
        assert torch.equal(pb["h_im"], nb["h_im"]) and "da_seed" not in pb
        seed = int(nb["da_seed"].item())
        assert nb["da_seed"].is_cuda and nb["da_seed"].dtype == torch.int64 and nb["da_seed"].numel() == 1
        base = pb["l_im"].cpu().numpy()
        want, decs = R.augment_batch(base, seed, params)
        got = nb["l_im"].cpu().numpy()
        assert all(d[0] for per in decs for d in per) and not np.array_equal(got, base)
        d = np.abs(got.astype(np.float64) - want.astype(np.float64))
        assert np.all(d <= bound_of(params, want)), float(d.max())
        for k in range(got.shape[0]):
            up = np.clip(resize_cubic(got[k, 0], (64, 64)), 0., 1.)
            assert np.abs(nb["l_to_h_img"][k, 0].cpu().numpy() - up).max() < 1e-6
        assert nb["l_to_h_img_aug"] is nb["l_to_h_img"]
        # one myseed: the same seed and the same bits
        assert torch.equal(nb["da_seed"], ab["da_seed"]) and torch.equal(nb["l_im"], ab["l_im"])
        assert torch.equal(nb["l_to_h_img"], ab["l_to_h_img"])
        seeds.append(seed)
        n += 1
    assert n == len(plain) >= 1
    # da_device without a da_* stage changes nothing; ranks draw different seeds
    idle = get_train_set(_fixture_args(da_device=True), "cuda")
    fresh = get_train_set(_fixture_args(), "cuda")
    assert not idle.da_device and torch.equal(next(iter(idle.epoch(0)))["l_im"], next(iter(fresh.epoch(0)))["l_im"])
    r0, r1 = (get_train_set(_fixture_args(batch_size=1, **DA_ON), "cuda", rank=r, world=2) for r in (0, 1))
    s0, s1 = (int(next(iter(t.epoch(0)))["da_seed"].item()) for t in (r0, r1))
    assert s0 != s1
