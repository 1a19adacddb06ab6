"""--lr_synth psf on the GPU: ops.psf_bin (srhip_psf_bin) and ops.photon_noise (srhip_photon_noise, csrc/lr_synth.hip) against
their numpy statements (dlib/datasets/lowres.py: psf_bin_np, photon_noise_np), and ResidentTrainSet / EvalPairs with the
option on, on the HR-only fixture tests/golden/hr_only_exp.

Bounds, from the arithmetic -- not from what the kernels give:
  psf_bin   one float32 spacing of the statement's value: both sum the same products of at most 144 taps in float64 in the
            same order without fused multiply-adds, so the sums agree to about 2e-14 and only a rounding tie could differ
            (0 is expected; the largest difference is printed);
  counts    exact outside the pixels the statement marks (a decision within 1e-12 / 1e-8 of its boundary, where another
            libm's exp / log / lgamma may decide otherwise), and at most 1e-4 of the pixels are marked;
  read noise  one float32 spacing of the statement's value outside marked pixels: the device's log / cos differ from numpy's
            by float64 roundings, which can move the one final rounding to float32 by a step."""
import os
import types

import numpy as np
import pytest
import torch

import lr_synth_cases as C
from deep_tile_cases import augment_img
from dlib.datasets import lowres

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HX = os.path.join(G, "hr_only_exp")
DS = "biosrv1-ccps-{}-X-2"


def _psf(src, sigma, s, in_max=None):
    from srhip import ops
    return ops.psf_bin(torch.from_numpy(np.array(src, copy=True)).cuda(), ops.psf_bin_weights(sigma, s), s, in_max=in_max)


@pytest.mark.parametrize("case", C.PSF_CASES, ids=C.PSF_IDS)
def test_psf_bin_equals_the_statement(case):
    kind, B, H, W, s, sigma = case[:6]
    in_max = case[6] if len(case) > 6 else None
    src = C.psf_source(case)
    want = lowres.psf_bin_np(src, sigma, s, in_max)
    one, two = _psf(src, sigma, s, in_max), _psf(src, sigma, s, in_max)
    got = one.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print(f"psf_bin {case}: max |got - statement| = {float(d.max()):.3e}")
    assert np.all(d <= np.spacing(np.abs(want)).astype(np.float64)), float(d.max())
    assert torch.equal(one.view(torch.int32), two.view(torch.int32))            # the same bits on every run


def test_psf_bin_refuses_what_it_cannot_run():
    from srhip import ops
    from srhip._lib import call
    x = torch.rand(1, 8, 8).cuda()
    w2 = ops.psf_bin_weights(1.0, 2)
    st = torch.cuda.current_stream().cuda_stream
    tmp, dst = torch.empty(8 * 4).cuda(), torch.empty(1, 4, 4).cuda()
    for args, what in (((None, 0, 0, w2.data_ptr(), w2.numel(), tmp.data_ptr(), dst.data_ptr(), 1, 8, 8, 2, st), "NULL"),
                       ((x.data_ptr(), 0, 0, None, w2.numel(), tmp.data_ptr(), dst.data_ptr(), 1, 8, 8, 2, st), "NULL"),
                       ((x.data_ptr(), 0, 0, w2.data_ptr(), w2.numel(), None, dst.data_ptr(), 1, 8, 8, 2, st), "NULL"),
                       ((x.data_ptr(), 0, 0, w2.data_ptr(), w2.numel(), tmp.data_ptr(), None, 1, 8, 8, 2, st), "NULL"),
                       ((x.data_ptr(), 0, 0, w2.data_ptr(), w2.numel(), tmp.data_ptr(), dst.data_ptr(), 1, 7, 8, 2, st), "multiples"),
                       ((x.data_ptr(), 0, 0, w2.data_ptr(), 2 * 65 + 2, tmp.data_ptr(), dst.data_ptr(), 1, 8, 8, 2, st), "radius"),
                       ((x.data_ptr(), 0, 0, w2.data_ptr(), w2.numel(), tmp.data_ptr(), x.data_ptr(), 1, 8, 8, 2, st), "overlap"),
                       ((x.data_ptr(), 0, 0, w2.data_ptr(), w2.numel(), x.data_ptr(), dst.data_ptr(), 1, 8, 8, 2, st), "overlap")):
        with pytest.raises(ops.SrhipError, match=what):
            call("srhip_psf_bin", *args)
    # and through the wrapper
    with pytest.raises(ops.SrhipError, match="multiples of s"):
        ops.psf_bin(torch.rand(1, 9, 8).cuda(), w2, 2)
    with pytest.raises(ops.SrhipError, match="radius"):
        ops.psf_bin(x, torch.ones(2 * 65 + 2, dtype=torch.float64).cuda(), 2)
    with pytest.raises(ops.SrhipError, match="radius"):
        ops.psf_bin_weights(16.2, 2)
    with pytest.raises(ops.SrhipError, match="overlap"):
        ops.psf_bin(x, w2, 2, out=x.view(-1)[:16].view(1, 4, 4))
    with pytest.raises(ops.SrhipError, match="2 .. 16"):
        ops.psf_bin(x, w2, 1)
    with pytest.raises(ops.SrhipError, match="weights"):
        ops.psf_bin(x, w2.float(), 2)
    with pytest.raises(ops.SrhipError, match="CUDA/HIP"):
        ops.psf_bin(x.cpu(), w2, 2)


def _noise(x, seed, photons, read_std, on=None):
    from srhip import ops
    xd = torch.from_numpy(np.array(x, copy=True)).cuda()
    sd = torch.tensor([seed], dtype=torch.int64).cuda()
    return ops.photon_noise(xd, sd, photons, read_std, on).cpu().numpy()


def check_noise(got, x, seed, photons, read_std, on=None, first_sample=0):
    """got against the statement on x within the bounds of this file's docstring; returns (marked pixels, largest difference,
    the statement's counts and attempts)"""
    info = {}
    want, marked = lowres.photon_noise_np(x, seed, photons, read_std, on=on, first_sample=first_sample, info=info)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert marked.mean() <= 1e-4, int(marked.sum())
    ok = ~marked
    if read_std == 0:
        counts = np.rint(got.astype(np.float64) * photons)
        touched = np.ones(x.shape, dtype=bool) if on is None else np.broadcast_to(np.asarray(on, bool)[:, None, None, None], x.shape)
        assert np.array_equal(counts[ok & touched], info["counts"][ok & touched])
        assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32))     # one float64 quotient, rounded once
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert np.all(d[ok] <= np.spacing(np.abs(want[ok])).astype(np.float64)), float(d[ok].max())
    if on is not None:
        for b, flag in enumerate(on):
            if not flag:
                assert np.array_equal(got[b].view(np.uint32), x[b].view(np.uint32)), b      # bit-equal to its input
    return int(marked.sum()), float(d[ok].max()), info


@pytest.mark.parametrize("read_std", [0.0, 2.5])
@pytest.mark.parametrize("photons", [0.5, 200.0, 60000.0])
@pytest.mark.parametrize("shape", [(1, 1, 5, 7), (3, 1, 16, 16), (8, 1, 64, 64)], ids=lambda s: "x".join(map(str, s)))
def test_photon_noise_equals_the_statement(shape, photons, read_std):
    B, _, h, w = shape
    x = C.noise_ramp(B, h, w)
    assert x.min() == 0.0 and x.max() == 1.0
    seed = 0x5EED0000 + int(photons) * 7 + B
    got = _noise(x, seed, photons, read_std)
    marked, worst, info = check_noise(got, x, seed, photons, read_std)
    if photons == 200.0:          # both sampler branches occur in one image
        lam = photons * x.astype(np.float64)
        assert ((lam > 0) & (lam < 30)).any() and (lam >= 30).any() and (info["attempts"] > 0).any()
    assert info["attempts"].max() <= 16
    print(f"photon_noise {shape} photons {photons:g} read_std {read_std:g}: marked {marked}, max |got - statement| = {worst:.3e}")
    if B == 3:
        on = [1, 0, 1]
        check_noise(_noise(x, seed, photons, read_std, on), x, seed, photons, read_std, on=on)
        # sample 1 of the batch of 3 is what the statement gives for b = 1 alone: nothing depends on B
        check_noise(got[1:2], x[1:2], seed, photons, read_std, first_sample=1)
        assert np.array_equal(_noise(x, seed, photons, read_std, [0, 1, 0])[1].view(np.uint32), got[1].view(np.uint32))


def test_photon_noise_refuses_what_it_cannot_run():
    from srhip import ops
    from srhip._lib import call
    x = torch.rand(2, 1, 8, 8).cuda()
    sd = torch.tensor([1], dtype=torch.int64).cuda()
    st = torch.cuda.current_stream().cuda_stream
    keep = x.clone()
    for args, what in (((None, 2, 8, 8, sd.data_ptr(), None, 10.0, 0.0, st), "NULL"),
                       ((x.data_ptr(), 2, 8, 8, None, None, 10.0, 0.0, st), "NULL"),
                       ((x.data_ptr(), 2, 8, 8, sd.data_ptr(), None, 0.0, 0.0, st), "photons"),
                       ((x.data_ptr(), 2, 8, 8, sd.data_ptr(), None, 2e6, 0.0, st), "photons"),
                       ((x.data_ptr(), 2, 8, 8, sd.data_ptr(), None, float("nan"), 0.0, st), "photons"),
                       ((x.data_ptr(), 2, 8, 8, sd.data_ptr(), None, 10.0, -1.0, st), "read_std"),
                       ((x.data_ptr(), 2, 8, 8, sd.data_ptr(), None, 10.0, float("inf"), st), "read_std")):
        with pytest.raises(ops.SrhipError, match=what):
            call("srhip_photon_noise", *args)
    for kw, what in ((dict(photons=0.0), "photons"), (dict(photons=-5.0), "photons"), (dict(photons=10.0, read_std=-1.0), "read_std"),
                     (dict(photons=10.0, on=[1]), "one flag per sample")):
        with pytest.raises(ops.SrhipError, match=what):
            ops.photon_noise(x, sd, **kw)
    with pytest.raises(ops.SrhipError, match="seed"):
        ops.photon_noise(x, sd.int(), 10.0)
    with pytest.raises(ops.SrhipError, match="contiguous float32"):
        ops.photon_noise(x[:, :, :, ::2], sd, 10.0)
    torch.cuda.synchronize()
    assert torch.equal(x, keep)


def test_photon_noise_captured_launch_reads_the_seed_at_replay():
    from srhip import ops
    x = C.noise_ramp(3, 16, 16)
    x0 = torch.from_numpy(x).cuda()
    seed, other = 0x1234ABCD5678, 0x1234ABCD5678 ^ 0x5DEECE66D1234567
    xs, sd = x0.clone(), torch.tensor([seed], dtype=torch.int64).cuda()
    ops.photon_noise(xs.clone(), sd, 200.0, 2.5, [1, 0, 1])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.photon_noise(xs, sd, 200.0, 2.5, [1, 0, 1])
    outs = []
    for s in (other, seed):
        xs.copy_(x0)
        sd.fill_(s)
        graph.replay()
        outs.append(xs.cpu().numpy())
        check_noise(outs[-1], x, s, 200.0, 2.5, on=[1, 0, 1])
    assert not np.array_equal(outs[0], outs[1])


PSF_ON = dict(lr_synth="psf", lr_synth_psf_sigma=1.2, lr_synth_photons=150.0, lr_synth_read_std=1.5)


def _train_args(**kw):
    a = types.SimpleNamespace(scale=2, splits_root=os.path.join(HX, "folds"), data_root=os.path.join(HX, "data"),
                              train_dsets=DS.format("train"), h_size=32, batch_size=2, myseed=5, sample_tr_patch="uniform")
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _raw(i):
    from PIL import Image
    return np.asarray(Image.open(os.path.join(HX, "data", "biosr", "t", f"h_{i}.tif")))


def _tile_no(h_id):
    return int(h_id.split("_")[1].split(".")[0])


def test_resident_train_set_with_lr_synth_psf():
    from dlib.utils.utils_dataloaders import get_train_set
    plain, psf = get_train_set(_train_args(), "cuda"), get_train_set(_train_args(**PSF_ON), "cuda")
    quiet = get_train_set(_train_args(**dict(PSF_ON, lr_synth_photons=0.0, lr_synth_read_std=0.0)), "cuda")
    assert plain.lr_synth is None and psf.lr_synth == (1.2, 150.0, 1.5) and psf.hr_only == [True] * 3
    clean = [lowres.psf_bin_np(_raw(i), 1.2, 2) for i in range(3)]
    for i in range(3):          # the resident float tile is the statement's clean tile (same bound as ops.psf_bin's)
        got = psf.lr[i].cpu().numpy()
        assert psf.lr[i].dtype == torch.float32 and got.shape == (48, 64)
        assert np.all(np.abs(got.astype(np.float64) - clean[i]) <= np.spacing(clean[i]).astype(np.float64))
        assert torch.equal(psf.lr[i], quiet.lr[i])
    n, first = 0, {}
    for epoch in range(2):
        for pb, nb, qb in zip(plain.epoch(epoch), psf.epoch(epoch), quiet.epoch(epoch)):
            assert pb["origin"] == nb["origin"] == qb["origin"] and pb["mode"] == nb["mode"] == qb["mode"]   # gen did not move
            assert torch.equal(pb["h_im"], nb["h_im"]) and "lr_synth_seed" not in pb
            sd = nb["lr_synth_seed"]
            assert sd.is_cuda and sd.dtype == torch.int64 and sd.numel() == 1 and torch.equal(sd, qb["lr_synth_seed"])
            crops = []
            for k in range(2):
                i, (r0, c0) = _tile_no(nb["h_id"][k]), nb["origin"][k]
                crops.append(np.ascontiguousarray(augment_img(clean[i][r0 // 2:r0 // 2 + 16, c0 // 2:c0 // 2 + 16], nb["mode"][k])))
                # photons = 0: the crop of the resident clean tile, bit for bit
                res = quiet.lr[i].cpu().numpy()[r0 // 2:r0 // 2 + 16, c0 // 2:c0 // 2 + 16]
                assert np.array_equal(qb["l_im"][k, 0].cpu().numpy(), augment_img(res, nb["mode"][k]))
            base = np.stack(crops)[:, None]
            assert np.all(np.abs(qb["l_im"].cpu().numpy().astype(np.float64) - base) <= np.spacing(base).astype(np.float64))
            # the statement applied to the crop of the statement's clean tile, under the batch's seed
            got = nb["l_im"].cpu().numpy()
            check_noise(got, base, int(sd.item()), 150.0, 1.5)
            assert not np.array_equal(got, qb["l_im"].cpu().numpy())
            up = torch.clamp(nb["l_to_h_img"], 0, 1)
            assert torch.equal(up, nb["l_to_h_img"]) and not torch.equal(nb["l_to_h_img"], qb["l_to_h_img"])   # made from the noisy l_im
            first.setdefault(epoch, (int(sd.item()), got))
            n += 1
    assert n == 2 * len(plain) >= 2
    assert first[0][0] != first[1][0]           # two epochs: another seed, other noise on the same tiles
    # one myseed: the same seeds and the same bits; another rank: other seeds
    again = next(iter(get_train_set(_train_args(**PSF_ON), "cuda").epoch(0)))
    assert int(again["lr_synth_seed"].item()) == first[0][0] and np.array_equal(again["l_im"].cpu().numpy(), first[0][1])
    r1 = get_train_set(_train_args(batch_size=1, **PSF_ON), "cuda", rank=1, world=2)
    r0 = get_train_set(_train_args(batch_size=1, **PSF_ON), "cuda", rank=0, world=2)
    assert int(next(iter(r0.epoch(0)))["lr_synth_seed"].item()) != int(next(iter(r1.epoch(0)))["lr_synth_seed"].item())


def test_same_tile_gets_other_noise_under_another_seed():
    """the same clean crop under the seeds of two batches: different noise"""
    x = C.noise_ramp(2, 16, 16)
    a, b = _noise(x, 11, 150.0, 1.5), _noise(x, 12, 150.0, 1.5)
    assert not np.array_equal(a, b) and np.array_equal(a, _noise(x, 11, 150.0, 1.5))


def test_eval_pairs_with_lr_synth_psf_are_reproducible():
    from dlib.utils.utils_dataloaders import get_eval_loader, LR_SYNTH_EVAL_SALT

    def items():
        a = types.SimpleNamespace(scale=2, splits_root=os.path.join(HX, "folds"), data_root=os.path.join(HX, "data"), eval_bsize=1,
                                  **PSF_ON)
        ds = get_eval_loader(a, DS.format("test")).dataset
        return [ds[i] for i in range(len(ds))]
    one, two = items(), items()
    assert len(one) == 3
    for i, (p, q) in enumerate(zip(one, two)):
        assert torch.equal(p["l_im"], q["l_im"]) and torch.equal(p["l_to_h_img"], q["l_to_h_img"])
        assert p["l_im"].dtype == torch.float32 and tuple(p["l_im"].shape) == (1, 48, 64)
        clean = lowres.psf_bin_np(_raw(i), 1.2, 2)
        # the whole tile as a batch of one under the salt plus the item index
        check_noise(p["l_im"].numpy()[None], clean[None, None], LR_SYNTH_EVAL_SALT + i, 150.0, 1.5)
    assert not torch.equal(one[0]["l_im"], one[1]["l_im"])


def test_main_trains_with_lr_synth_psf_and_eval_reads_the_keys_back(tmp_path):
    """main.py over the HR-only folds with the camera model on: a finite loss, the four keys in config_model.yml, and eval.py --
    which takes them from there -- reproduces the test score on the same noisy LR images."""
    import pickle
    import subprocess
    import sys
    import yaml
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sr-caco-2_amd")
    outd = str(tmp_path / "exp")
    cmd = [sys.executable, os.path.join(pkg, "main.py"), "--net_type", "EDSR_LIIF", "--method", "EDSR_LIIF", "--scale", "2",
           "--h_size", "32", "--batch_size", "2", "--max_iters", "2", "--max_epochs", "2", "--checkpoint_eval", "1",
           "--train_dsets", DS.format("train"), "--valid_dsets", DS.format("val"), "--test_dsets", DS.format("test"),
           "--data_root", os.path.join(HX, "data"), "--splits_root", os.path.join(HX, "folds"), "--eval_bsize", "2",
           "--outd", outd, "--lr_synth", "psf", "--lr_synth_psf_sigma", "1.2", "--lr_synth_photons", "150",
           "--lr_synth_read_std", "1.5"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    with open(os.path.join(outd, "config_model.yml")) as f:
        cfg = yaml.safe_load(f)
    assert [cfg[k] for k in ("lr_synth", "lr_synth_psf_sigma", "lr_synth_photons", "lr_synth_read_std")] == ["psf", 1.2, 150.0, 1.5]
    with open(os.path.join(outd, "tracker.pkl"), "rb") as f:
        tr = pickle.load(f)
    losses = tr["train"]["period_iter"]["master_loss"]["vals"]
    assert len(losses) == 2 and all(np.isfinite(v) and v > 0 for v in losses), losses
    test = DS.format("test")
    psnr = tr["test"][test]["psnr"]["vals"]
    assert len(psnr) == 1 and np.isfinite(psnr[0])
    import eval as E
    tr2, _ = E.evaluate_pretrained(["--cudaid", "0", "--exp_path", outd, "--data_root", os.path.join(HX, "data"),
                                    "--splits_root", os.path.join(HX, "folds")])
    assert abs(tr2["test"][test]["psnr"]["vals"][0] - psnr[0]) <= 1e-9
