#!/usr/bin/env python
"""What --lr_synth psf costs beside the antialiased bicubic LR image of an HR-only pair (csrc/lr_synth.hip against
csrc/resize.hip), at scale 2 and scale 8.  Both arms of each comparison run in this process, alternating; the figure of an arm is
the median of --rounds timed windows after a warm-up.

  tile     one --size^2 uint8 tile through ops.psf_bin (sigma --sigma) against ops.imresize_aa: once per tile, when a set is
           built; microseconds per call by device events over --calls calls
  batches  whole ResidentTrainSet.epoch batches (batch --batch, patch --patch, uniform crops) of an HR-only set of --tiles
           synthetic tiles under --lr_synth psf: with the noise launch (photons --photons, read noise --read-std) against
           without it (photons 0), batches per second; and the noise launch alone on a batch of that shape by device events

    python tools/lr_synth_rate.py --out profiles/lr_synth_rate.json
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sr-caco-2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from sampler_rate import blob_tile, rate  # noqa: E402


def write_hr_only_set(root, n, size):
    from PIL import Image
    pairs_h, pairs_l = {}, {}
    for i in range(n):
        hp = os.path.join(root, f"h_{i}.tif")
        Image.fromarray(blob_tile(size, i)).save(hp)
        pairs_h[f"h_{i}.tif"] = {"low_path_key": f"None_{i}", "abs_path": hp}
        pairs_l[f"None_{i}"] = {"abs_path": f"None_{i}"}
    return pairs_h, pairs_l


def events_us(fn, calls):
    """microseconds per call of fn's launches, by device events over ``calls`` calls after a warm-up"""
    import torch
    for _ in range(10):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=16)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--patch", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--batches", type=int, default=1000)
    ap.add_argument("--sigma", type=float, default=1.2)
    ap.add_argument("--photons", type=float, default=150.)
    ap.add_argument("--read-std", type=float, default=1.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lr_synth_rate.json"))
    o = ap.parse_args()
    import torch
    from dlib.datasets.dataset_dpsr import ResidentTrainSet
    from srhip import ops
    assert torch.cuda.is_available(), "lr_synth_rate needs a GPU"
    res = {"tool": "tools/lr_synth_rate.py", "device": torch.cuda.get_device_name(0), "tiles": o.tiles, "tile": [o.size, o.size],
           "patch": o.patch, "batch": o.batch, "rounds": o.rounds, "sigma": o.sigma, "photons": o.photons, "read_std": o.read_std,
           "scales": {}}
    tile = torch.from_numpy(blob_tile(o.size, 0).copy())[None].cuda()
    for sf in (2, 8):
        row = {}
        # one tile: the camera model's clean image against the antialiased bicubic down-scaling
        wts = ops.psf_bin_weights(o.sigma, sf)
        lo = torch.empty(1, o.size // sf, o.size // sf, device="cuda")
        arms = {"psf_bin": lambda: ops.psf_bin(tile, wts, sf, out=lo), "imresize_aa": lambda: ops.imresize_aa(tile, 1 / sf, out=lo)}
        runs = {k: [] for k in arms}
        for _ in range(o.rounds):                            # the arms alternate
            for k, fn in arms.items():
                runs[k].append(events_us(fn, o.calls))
        for k in arms:
            row[f"{k}_us"] = round(statistics.median(runs[k]), 2)
            row[f"{k}_us_runs"] = [round(v, 2) for v in runs[k]]
        row["psf_bin_taps"] = int(wts.numel())
        row["psf_bin_over_imresize_aa"] = round(row["psf_bin_us"] / row["imresize_aa_us"], 2)
        # whole batches: with and without the noise launch
        with tempfile.TemporaryDirectory() as root:
            pairs_h, pairs_l = write_hr_only_set(root, o.tiles, o.size)
            sets = {}
            for arm, photons, read_std in (("clean", 0., 0.), ("noise", o.photons, o.read_std)):
                args = types.SimpleNamespace(scale=sf, h_size=o.patch, batch_size=o.batch, myseed=0, sample_tr_patch="uniform",
                                             color_max=255, lr_synth="psf", lr_synth_psf_sigma=o.sigma, lr_synth_photons=photons,
                                             lr_synth_read_std=read_std)
                sets[arm] = ResidentTrainSet(args, pairs_h, pairs_l, "cuda")
                assert all(sets[arm].hr_only) and sets[arm].lr_synth == (o.sigma, photons, read_std)
        for arm in sets:
            rate(sets[arm], 4)                               # warm-up
        runs = {arm: [] for arm in sets}
        for _ in range(o.rounds):
            for arm in sets:
                runs[arm].append(rate(sets[arm], o.batches))
        lp = o.patch // sf
        row["lr_patch"] = [lp, lp]
        for arm in runs:
            row[f"{arm}_batches_per_s"] = round(statistics.median(runs[arm]), 1)
            row[f"{arm}_batches_per_s_runs"] = [round(v, 1) for v in runs[arm]]
        row["batches_timed"] = o.batches
        row["noise_over_clean"] = round(row["noise_batches_per_s"] / row["clean_batches_per_s"], 3)
        x0 = torch.rand(o.batch, 1, lp, lp, device="cuda")
        x, seed = x0.clone(), torch.tensor([12345], dtype=torch.int64, device="cuda")

        def noise():          # on a fresh copy each call: the kernel works in place and its time depends on the values
            x.copy_(x0)
            ops.photon_noise(x, seed, o.photons, o.read_std)
        us = [events_us(noise, o.calls) for _ in range(o.rounds)]
        cp = [events_us(lambda: x.copy_(x0), o.calls) for _ in range(o.rounds)]
        row["photon_noise_launch_us"] = round(statistics.median(us) - statistics.median(cp), 2)
        row["photon_noise_with_copy_us_runs"] = [round(v, 2) for v in us]
        row["copy_us_runs"] = [round(v, 2) for v in cp]
        res["scales"][f"x{sf}"] = row
        print(f"x{sf}", row, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
    with open(o.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
