#!/usr/bin/env python
"""Batches per second of ResidentTrainSet.epoch with the three LR-only augmentations on (--da_blur, --da_dot_bin_noise,
--da_add_gaus_noise at the configuration's defaults): through the host path (download, scipy / numpy per sample, upload -- the
default) and with --da_device (one ops.lr_augment call on the gathered l_im, csrc/augment.hip).  Both arms run in this process,
alternating, on the same synthetic set; the figure of an arm is the median of --rounds timed windows after a warm-up.

Synthetic set as tools/sampler_rate.py: --tiles Gaussian-blob HR tiles of --size^2 with their true LR tiles, batch --batch, patch
--patch, uniform crops; once at scale 8 (64^2 LR patches) and once at scale 2 (256^2).  Also timed, by device events: the
launches of one ops.lr_augment call alone on a batch of that shape.

    python tools/lr_augment_rate.py --out profiles/lr_augment_rate.json
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sr-caco-2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from sampler_rate import rate, write_set  # noqa: E402


def launches_us(ts, lp, batch, calls):
    """microseconds of one ops.lr_augment call's launches on [batch, 1, lp, lp], by device events over ``calls`` calls"""
    import torch
    from srhip import ops
    x = torch.rand(batch, 1, lp, lp, device="cuda")
    seed = torch.tensor([12345], dtype=torch.int64, device="cuda")
    for _ in range(10):
        ops.lr_augment(x, seed, ts.da_params, ts.da_weights)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(calls):
        ops.lr_augment(x, seed, ts.da_params, ts.da_weights)
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
    ap.add_argument("--device-batches", type=int, default=2000)
    ap.add_argument("--host-batches", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lr_augment_rate.json"))
    o = ap.parse_args()
    import torch
    from dlib.datasets.dataset_dpsr import ResidentTrainSet
    assert torch.cuda.is_available(), "lr_augment_rate needs a GPU"
    da = dict(da_blur=True, da_blur_prob=0.5, da_blur_area=0.3, da_blur_sigma=1.,
              da_dot_bin_noise=True, da_dot_bin_noise_prob=0.5, da_dot_bin_noise_area=0.3, da_dot_bin_noise_p=0.5,
              da_add_gaus_noise=True, da_add_gaus_noise_prob=0.5, da_add_gaus_noise_area=0.3, da_add_gaus_noise_std=0.03)
    res = {"tool": "tools/lr_augment_rate.py", "device": torch.cuda.get_device_name(0), "tiles": o.tiles,
           "tile": [o.size, o.size], "patch": o.patch, "batch": o.batch, "rounds": o.rounds, "stages": da, "scales": {}}
    for sf in (8, 2):
        with tempfile.TemporaryDirectory() as root:
            pairs_h, pairs_l = write_set(root, o.tiles, o.size, sf)
            sets = {}
            for arm, on in (("host", False), ("device", True)):
                args = types.SimpleNamespace(scale=sf, h_size=o.patch, batch_size=o.batch, myseed=0, sample_tr_patch="uniform",
                                             sample_tr_patch_th_style="fix_threshold", sample_tr_patch_th=12, color_max=255,
                                             da_device=on, **da)
                sets[arm] = ResidentTrainSet(args, pairs_h, pairs_l, "cuda")
                assert sets[arm].da and sets[arm].da_device == on
        nb = {"host": o.host_batches, "device": o.device_batches}
        np.random.seed(0)
        for arm in sets:
            rate(sets[arm], 4)                               # warm-up: library load, allocator, scipy's import
        runs = {"host": [], "device": []}
        for _ in range(o.rounds):                            # the arms alternate
            for arm in ("host", "device"):
                runs[arm].append(rate(sets[arm], nb[arm]))
        lp = o.patch // sf
        row = {"lr_patch": [lp, lp]}
        for arm in runs:
            row[f"{arm}_batches_per_s"] = round(statistics.median(runs[arm]), 1)
            row[f"{arm}_batches_per_s_runs"] = [round(v, 1) for v in runs[arm]]
            row[f"{arm}_batches_timed"] = nb[arm]
        row["device_over_host"] = round(row["device_batches_per_s"] / row["host_batches_per_s"], 2)
        us = [launches_us(sets["device"], lp, o.batch, 200) for _ in range(o.rounds)]
        row["lr_augment_launches_us"] = round(statistics.median(us), 2)
        row["lr_augment_launches_us_runs"] = [round(v, 2) for v in us]
        res["scales"][f"x{sf}"] = row
        print(f"x{sf}", row, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
    with open(o.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
