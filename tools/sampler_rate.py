#!/usr/bin/env python
"""Batches per second of ResidentTrainSet.epoch under the 'edt', 'edt*roi' and 'roi' + Otsu crop samplers: on the device
(DeviceWeightedSampler, csrc/edt.hip) and, with SRHIP_HOST_SAMPLER=1, on the host PatchSampler (scipy's distance transform
and a multinomial over every candidate, per sample) -- both in this process, in the same order, on the same box.

Synthetic set: --tiles Gaussian-blob HR tiles of --size^2 with their true LR tiles (scale 8), written to a temporary
directory; batch --batch, patch --patch.  Also timed: the one-time cost per tile of building the device sampler (threshold,
distance transform, row prefix).

    python tools/sampler_rate.py --out profiles/sampler_rate.json
"""
import argparse
import json
import os
import sys
import tempfile
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sr-caco-2_amd"))


def blob_tile(size, seed):
    """cells on a dark background: Gaussian blobs of sigma 8..40 pixels, so exp(distance) stays far from overflow"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float32)
    img = np.zeros((size, size), np.float32)
    for _ in range(max(4, size * size // 60000)):
        cy, cx, s = rng.uniform(0, size), rng.uniform(0, size), rng.uniform(8, 40)
        img += rng.uniform(30, 120) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    img += rng.uniform(0, 6, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def write_set(root, n, size, sf):
    from PIL import Image
    pairs_h, pairs_l = {}, {}
    for i in range(n):
        h = blob_tile(size, i)
        l = np.asarray(Image.fromarray(h).resize((size // sf, size // sf), Image.BICUBIC))
        hp, lp = os.path.join(root, f"h_{i}.tif"), os.path.join(root, f"l_{i}.tif")
        Image.fromarray(h).save(hp)
        Image.fromarray(l).save(lp)
        pairs_h[f"h_{i}.tif"] = {"low_path_key": f"l_{i}.tif", "abs_path": hp}
        pairs_l[f"l_{i}.tif"] = {"abs_path": lp}
    return pairs_h, pairs_l


def rate(ts, batches):
    import torch
    done, epoch = 0, 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while done < batches:
        for _ in ts.epoch(epoch):
            done += 1
            if done == batches:
                break
        epoch += 1
    torch.cuda.synchronize()
    return done / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=16)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--patch", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--device-batches", type=int, default=100)
    ap.add_argument("--host-batches", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampler_rate.json"))
    o = ap.parse_args()
    import torch
    from dlib.datasets.dataset_dpsr import ResidentTrainSet, DeviceWeightedSampler
    assert torch.cuda.is_available(), "sampler_rate needs a GPU"
    res = {"tool": "tools/sampler_rate.py", "device": torch.cuda.get_device_name(0), "tiles": o.tiles, "tile": [o.size, o.size],
           "patch": o.patch, "batch": o.batch, "scale": 8, "styles": {}}
    with tempfile.TemporaryDirectory() as root:
        pairs_h, pairs_l = write_set(root, o.tiles, o.size, 8)
        for name, style, th_style in (("edt", "edt", "fix_threshold"), ("edt*roi", "edt*roi", "fix_threshold"),
                                      ("roi+otsu", "roi", "automatic_threshold")):
            args = types.SimpleNamespace(scale=8, h_size=o.patch, batch_size=o.batch, myseed=0, sample_tr_patch=style,
                                         sample_tr_patch_th_style=th_style, sample_tr_patch_th=12, color_max=255)
            row = {}
            for arm, env, nb in (("device", None, o.device_batches), ("host", "1", o.host_batches)):
                os.environ.pop("SRHIP_HOST_SAMPLER", None)
                if env:
                    os.environ["SRHIP_HOST_SAMPLER"] = env
                np.random.seed(0)
                ts = ResidentTrainSet(args, pairs_h, pairs_l, "cuda")
                assert (ts.host_sampler is None) == (arm == "device")
                rate(ts, 2)                                  # warm-up: library load, allocator
                row[f"{arm}_batches_per_s"] = round(rate(ts, nb), 3)
                row[f"{arm}_batches_timed"] = nb
                if arm == "device":                          # the one-time cost, on the resident ROI images of this set
                    cost = []
                    for _ in range(2):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        DeviceWeightedSampler(ts.roi_src, o.patch, style,
                                              thresholds=12. if th_style == "fix_threshold" else None)
                        torch.cuda.synchronize()
                        cost.append((time.perf_counter() - t0) / o.tiles * 1e3)
                    row["construction_ms_per_tile"] = round(min(cost), 3)
            os.environ.pop("SRHIP_HOST_SAMPLER", None)
            row["device_over_host"] = round(row["device_batches_per_s"] / row["host_batches_per_s"], 1)
            res["styles"][name] = row
            print(name, row, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
    with open(o.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
