#!/usr/bin/env python
"""Training steps and evaluation forwards per second of DSR-Splines: the fused one-expert-per-pixel path (csrc/dsr_splines.hip
through TrainStep / the module) against a stock-PyTorch arm that evaluates every spline net over the whole interpolated image
and sums the masked results, as the reference formulates it -- both in this process, on the same box, alternating.

Workload: the registry default net (in_ksz 3, snet_type1, 16 splines, no residuals), x8, B = 8, 64 x 64 -> 512 x 512, L1 loss,
Adam.  Two inputs: 'uniform' (every grey level equally likely: the experts share the pixels evenly) and 'cells' (Gaussian
blobs on a dark field: most pixels belong to the first expert, the case the per-expert backward balances worst).  Each arm
is warmed up, then timed over --steps iterations ending in a device synchronise, --rounds times alternating; the median is
reported with the spread, and the peak of torch's allocator over the timed window.

    python tools/dsr_splines_rate.py --out profiles/dsr_splines_rate.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sr-caco-2_amd"))


def make_batch(kind, B, h, scale, seed):
    import torch
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(seed)
    H = h * scale
    if kind == "uniform":
        hr = (torch.rand(B, 1, H, H, generator=g) * 255).round() / 255
    else:
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(H, dtype=torch.float32), indexing="ij")
        hr = torch.zeros(B, 1, H, H)
        for b in range(B):
            for _ in range(6):
                cy, cx = torch.rand(2, generator=g) * H
                s = 8 + 32 * torch.rand(1, generator=g)
                hr[b, 0] += (30 + 90 * torch.rand(1, generator=g)) * torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
        hr = ((hr + 6 * torch.rand(B, 1, H, H, generator=g)).clamp(0, 255)).floor() / 255
    lr = F.interpolate(hr, scale_factor=1.0 / scale, mode='bicubic').clamp(0, 1)
    return lr.cuda(), hr.cuda()


def dense_net(n, scale):
    """The reference's formulation in stock torch: every spline net is a reflect-padded 3x3 conv 1 -> 16, ReLU, a 1x1 conv
    16 -> 1, ReLU, run over the whole image; its output counts where uint8(x * 255) lies in the spline's bin."""
    import numpy as np
    import torch
    import torch.nn as nn
    import torch.nn.functional as F

    class Dense(nn.Module):
        def __init__(self):
            super().__init__()
            self.nets = nn.ModuleList([nn.Sequential(nn.Conv2d(1, 16, 3, padding=1, padding_mode='reflect'), nn.ReLU(),
                                                     nn.Conv2d(16, 1, 1), nn.ReLU()) for _ in range(n)])
            self.bins = [(int(s[0]), int(s[-1])) for s in np.array_split(np.arange(256), n)]

        def forward(self, x):
            xi = F.interpolate(x, size=(scale * x.shape[2], scale * x.shape[3]), mode='bicubic', align_corners=False).clamp(0, 1)
            u = (xi * 255).to(torch.uint8).float().clamp(0, 255)
            out = None
            for net, (lo, hi) in zip(self.nets, self.bins):
                y = net(xi) * ((u >= lo) & (u <= hi)).float()
                out = y if out is None else out + y
            return out
    return Dense().cuda()


def timed(fn, steps):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--lr-size", type=int, default=64)
    ap.add_argument("--scale", type=int, default=8)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dsr_splines_rate.json"))
    o = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "dsr_splines_rate needs a GPU"
    from dlib.models.network_dsr_splines import DsrSplines
    from srhip.train import TrainStep
    n = 16
    res = {"tool": "tools/dsr_splines_rate.py", "device": torch.cuda.get_device_name(0),
           "net": "DSR-Splines in_ksz 3 snet_type1 16 splines", "scale": o.scale, "batch": o.batch,
           "lr": [o.lr_size, o.lr_size], "steps_timed": o.steps, "rounds": o.rounds, "loss": "l1", "optimizer": "adam", "inputs": {}}
    for kind in ("uniform", "cells"):
        lr, hr = make_batch(kind, o.batch, o.lr_size, o.scale, 3)
        torch.manual_seed(0)
        fused = DsrSplines(o.scale, 1, 3, "snet_type1", n, False, False).cuda().train()
        dense = dense_net(n, o.scale).train()
        with torch.no_grad():                                    # the same weights in both arms
            for k in range(n):
                m = fused.splines[k].model
                dense.nets[k][0].weight.copy_(m[0].conv.weight), dense.nets[k][0].bias.copy_(m[0].conv.bias)
                dense.nets[k][2].weight.copy_(m[1].conv.weight), dense.nets[k][2].bias.copy_(m[1].conv.bias)
            gap = (fused(lr) - dense(lr)).abs().max().item()
        assert gap <= 1e-5, f"the two arms disagree by {gap}"
        ts = TrainStep(fused, [("l1", 1.0)])
        opt = torch.optim.Adam(dense.parameters(), lr=2e-4)

        def dense_step():
            opt.zero_grad(set_to_none=True)
            (dense(lr) - hr).abs().mean().backward()
            opt.step()

        def evaluate(net):
            with torch.no_grad():
                net(lr)
        arms = {"fused_train_eager": lambda: ts.step(lr, hr), "fused_train_graph": lambda: ts.step_graph(lr, hr),
                "dense_train": dense_step, "fused_eval": lambda: evaluate(fused), "dense_eval": lambda: evaluate(dense)}
        rates = {k: [] for k in arms}
        peak = {}
        for k, fn in arms.items():
            for _ in range(o.warmup):
                fn()
        for _ in range(o.rounds):
            for k, fn in arms.items():
                if k.endswith("eval"):
                    fused.eval(), dense.eval()
                else:
                    fused.train(), dense.train()
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                rates[k].append(timed(fn, o.steps))
                peak[k] = max(peak.get(k, 0), torch.cuda.max_memory_allocated())
        row = {}
        for k in arms:
            row[k + "_per_s"] = round(statistics.median(rates[k]), 2)
            row[k + "_spread"] = [round(min(rates[k]), 2), round(max(rates[k]), 2)]
            row[k + "_peak_MiB"] = round(peak[k] / 2 ** 20, 1)
        row["forward_gap"] = gap
        row["train_fused_graph_over_dense"] = round(row["fused_train_graph_per_s"] / row["dense_train_per_s"], 2)
        row["train_fused_eager_over_dense"] = round(row["fused_train_eager_per_s"] / row["dense_train_per_s"], 2)
        row["eval_fused_over_dense"] = round(row["fused_eval_per_s"] / row["dense_eval_per_s"], 2)
        res["inputs"][kind] = row
        print(kind, row, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
    with open(o.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
